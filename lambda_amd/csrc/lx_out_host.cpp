// lx_out_host.cpp -- lx_out_*: an output file that is written piece by piece and is, after lx_out_close, byte for byte the file the
// one-shot writers make from the concatenated list (lx_write_records_ex + lx_write_footer, lx_write_records_bgzf, lx_write_text_dev,
// lx_write_bam_dev).  No kernel of its own: the existing writers get a caller that comes more than once.
//
// open renders the header (lx_render_records, no records) and, for a compressed file, sends its whole blocks through the encoder.
// append renders the piece's records without header and footer: on the host by lx_render_records, on the device by the kernels of
// lx_render_text_dev / lx_render_bam_dev.  A piece holds whole query groups, and everything the records of a group depend on (the
// comment lines of .m9, FLAG, IH, --sam-bam-seq uniq, the group's LCA; QUAL from the piece's own qualities, lx_out_append_ex) is
// decided inside the group, so nothing crosses a piece but the BGZF carry: a compressed stream is cut into 65 280-byte blocks counted from its first byte, as lx_bgzf_compress cuts the whole
// stream, and the bytes that do not fill a block wait in front of the next piece -- in host memory behind a host append, on the
// device (d_carry) behind a device append (lxi::text_append_dev, lxi::bam_append_dev: the records are compressed where they stand
// and only members come down); a change of side moves less than a block.  close puts the .m9 footer behind the carry, compresses
// what is left as the last block, and writes the EOF member.
#include <cstdio>
#include <memory>
#include <vector>

#include "lx_bgzf.h"
#include "lx_rec_host.h"

using namespace lxi;

struct lx_out
{
    lx_handle *       h = nullptr;
    std::FILE *       f = nullptr;
    std::string       path, program;
    int               format = 0;
    bool              bgzf = false, failed = false;
    lx_seq_names      subjects{};
    lx_output_options opt{};
    std::string       columns, sam_tags, version, command_line, db_name; // (the texts opt points to are the object's own)
    // the carry: on the host in `carry`, or on the device in d_carry[0, dev_carry)
    std::string carry;
    DevBuf      d_carry;
    uint64_t    dev_carry = 0;
    bool        on_dev    = false;
};

namespace
{

int refuse(lx_handle * h, int rc, std::string const & text)
{
    if (h)
        return fail(h, rc, "%s", text.c_str());
    set_output_error(text);
    return rc;
}

// a refusal of the host writer: its text is in lx_last_output_error()
int refuse_output(lx_handle * h, char const * who, int rc)
{
    return h ? rec_refuse(h, who, rc) : rc;
}

int write(lx_out * o, void const * p, uint64_t n)
{
    // (the one-shot writers' code and text for it; the callers end the file's use: an I/O error is no refusal)
    if (n && std::fwrite(p, 1, n, o->f) != n)
        return refuse(o->h, LX_EINVAL, "error while writing " + o->path + " (disk full?)");
    return LX_OK;
}

int carry_to_host(lx_out * o)
{
    if (!o->on_dev)
        return LX_OK;
    lx_handle * const h = o->h;
    int const         rc = bind(h);
    if (rc)
        return rc;
    o->carry.resize(o->dev_carry);
    if (o->dev_carry)
        LX_HIP(h, hipMemcpyAsync(&o->carry[0], o->d_carry.ptr, o->dev_carry, hipMemcpyDeviceToHost, h->stream));
    LX_HIP(h, hipStreamSynchronize(h->stream));
    o->on_dev = false;
    return LX_OK;
}

int carry_to_dev(lx_out * o)
{
    if (o->on_dev)
        return LX_OK;
    lx_handle * const h = o->h;
    int               rc = bind(h);
    if (rc || (rc = ensure(h, o->d_carry, lx::kBgzfBlock + 16)))
        return rc;
    if (!o->carry.empty())
        LX_HIP(h, hipMemcpyAsync(o->d_carry.ptr, o->carry.data(), o->carry.size(), hipMemcpyHostToDevice, h->stream));
    LX_HIP(h, hipStreamSynchronize(h->stream));
    o->dev_carry = o->carry.size();
    o->carry.clear();
    o->on_dev = true;
    return LX_OK;
}

// the whole blocks of the host carry through the encoder into the file; `all`: what is left too, and the EOF member
int flush_host(lx_out * o, bool all)
{
    uint64_t const whole = all ? o->carry.size() : o->carry.size() / lx::kBgzfBlock * lx::kBgzfBlock;
    if (!whole && !all)
        return LX_OK;
    std::vector<uint8_t> packed(lx_bgzf_bound(whole));
    uint64_t             got = 0;
    int rc = lx_bgzf_compress(o->h, reinterpret_cast<uint8_t const *>(o->carry.data()), whole, packed.data(), packed.size(), &got, all ? LX_BGZF_EOF : 0);
    if (rc)
        return o->failed = true, rc;
    o->carry.erase(0, whole);
    if ((rc = write(o, packed.data(), got)))
        o->failed = true;
    return rc;
}

// bytes made on the host (the header, a host append) into the file
int put_host(lx_out * o, lx_bytes * bytes)
{
    std::unique_ptr<lx_bytes, void (*)(lx_bytes *)> keep(bytes, lx_bytes_free);
    int rc = LX_OK;
    if (!o->bgzf)
    {
        if ((rc = write(o, lx_bytes_data(bytes), lx_bytes_size(bytes))))
            o->failed = true;
        return rc;
    }
    if ((rc = carry_to_host(o)))
        return o->failed = true, rc;
    o->carry.append(reinterpret_cast<char const *>(lx_bytes_data(bytes)), lx_bytes_size(bytes));
    return flush_host(o, false);
}

} // namespace

extern "C" {

int lx_out_open(lx_handle * h, char const * path, int format, int bgzf, char const * program, lx_seq_names const * subjects,
                lx_output_options const * opt, lx_out ** out)
{
    if (!h)
        set_output_error("");
    if (out)
        *out = nullptr;
    if (!path || !program || !subjects || !out)
        return refuse(h, LX_EINVAL, "lx_out_open: NULL argument");
    if (format < LX_OUT_BLAST_TAB || format > LX_OUT_BAM)
        return refuse(h, LX_EINVAL, "lx_out_open: unknown output format");
    if (format == LX_OUT_BAM)
        bgzf = 1;
    if (bgzf && !h)
        return refuse(h, LX_EINVAL, "lx_out_open: a compressed file (bgzf, LX_OUT_BAM) needs a handle: the encoder runs on its device");
    try
    {
        std::unique_ptr<lx_out> o(new lx_out);
        o->h        = h;
        o->path     = path;
        o->program  = program;
        o->format   = format;
        o->bgzf     = bgzf != 0;
        o->subjects = lx_seq_names{nullptr, nullptr, subjects->s_ids, subjects->s_lens, 0, subjects->n_s};
        lx_output_options_default(&o->opt);
        if (opt)
            o->opt = *opt;
        auto own = [](char const *& p, std::string & s)
        {
            if (p)
                p = (s = p).c_str();
        };
        own(o->opt.columns, o->columns);
        own(o->opt.sam_tags, o->sam_tags);
        own(o->opt.version, o->version);
        own(o->opt.command_line, o->command_line);
        own(o->opt.db_name, o->db_name);
        o->opt.lca_qid = nullptr;
        o->opt.lca_tax = nullptr;
        o->opt.n_lca   = 0;
        o->opt.q_qual  = nullptr; // (a piece's own: lx_out_append_ex)
        // the header; with it the refusals of the one-shot writers that need no record, before the file is touched
        lx_bytes * header = nullptr;
        int rc = lx_render_records(format, 1, program, nullptr, 0, nullptr, &o->subjects, nullptr, nullptr, &o->opt, -1, &header);
        if (rc)
            return refuse_output(h, "lx_out_open", rc);
        o->f = std::fopen(path, "wb");
        if (!o->f)
        {
            lx_bytes_free(header);
            return refuse(h, LX_EINVAL, std::string("cannot open ") + path);
        }
        if ((rc = put_host(o.get(), header))) // (no refusal: the encoder or the disk failed.  Nothing of the file stays behind)
        {
            std::fclose(o->f);
            std::remove(path);
            return rc;
        }
        *out = o.release();
        return LX_OK;
    }
    catch (std::bad_alloc const &)
    {
        return refuse(h, LX_ENOMEM, "lx_out_open: out of host memory");
    }
}

int lx_out_append(lx_out * o, int where, lx_blast_match const * m, uint64_t n, uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names,
                  uint8_t const * q_res_ascii, uint64_t const * q_ascii_off, uint64_t const * lca_qid, uint32_t const * lca_tax, uint64_t n_lca)
{
    return lx_out_append_ex(o, where, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, nullptr, lca_qid, lca_tax, n_lca);
}

// (the refusals keep lx_out_append's name: it is the call with a NULL q_qual)
int lx_out_append_ex(lx_out * o, int where, lx_blast_match const * m, uint64_t n, uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names,
                     uint8_t const * q_res_ascii, uint64_t const * q_ascii_off, uint8_t const * q_qual, uint64_t const * lca_qid,
                     uint32_t const * lca_tax, uint64_t n_lca)
{
    if (!o)
    {
        set_output_error("lx_out_append: NULL argument");
        return LX_EINVAL;
    }
    lx_handle * const h = o->h;
    if (!h)
        set_output_error("");
    if (where != LX_RENDER_HOST && where != LX_RENDER_DEV)
        return refuse(h, LX_EINVAL, "lx_out_append: where is neither LX_RENDER_HOST nor LX_RENDER_DEV");
    if (where == LX_RENDER_DEV && !h)
        return refuse(h, LX_EINVAL, "lx_out_append: LX_RENDER_DEV needs a handle");
    if (o->failed)
        return refuse(h, LX_EINVAL, "lx_out_append: an earlier call on " + o->path + " has failed");
    if (n == 0) // an empty piece: nothing to write, whatever the other arguments are
        return LX_OK;
    if (!m || !names)
        return refuse(h, LX_EINVAL, "lx_out_append: NULL argument");
    lx_seq_names const nm{names->q_ids, names->q_lens, o->subjects.s_ids, o->subjects.s_lens, names->n_q, o->subjects.n_s};
    lx_output_options  opt = o->opt;
    opt.lca_qid            = lca_qid;
    opt.lca_tax            = lca_tax;
    opt.n_lca              = n_lca;
    opt.q_qual             = q_qual;
    char const * const program = o->program.c_str();
    bool io_failed = false; // (told apart from a refusal by what happened, not by the code it shares with one)
    auto sink      = [&](uint8_t const * members, uint64_t bytes) -> int
    {
        int const r = write(o, members, bytes);
        io_failed   = io_failed || r != LX_OK;
        return r;
    };
    int rc = LX_OK;
    try
    {
        if (where == LX_RENDER_HOST)
        {
            lx_bytes * bytes = nullptr;
            if ((rc = lx_render_records(o->format, 0, program, m, n, ops, &nm, q_res_ascii, q_ascii_off, &opt, -1, &bytes)))
                return refuse_output(h, "lx_out_append", rc);
            rc = put_host(o, bytes);
        }
        else if (!o->bgzf) // (device text into a plain file: the ranges come down as in lx_write_text_dev)
        {
            lx_bytes * bytes = nullptr;
            if ((rc = lx_render_text_dev(h, o->format, 0, program, m, n, ops, ops_bytes, &nm, q_res_ascii, q_ascii_off, &opt, -1, &bytes)))
                return rc;
            rc = put_host(o, bytes);
        }
        else
        {
            if ((rc = carry_to_dev(o)))
                return o->failed = true, rc;
            uint64_t        c = o->dev_carry;
            uint8_t * const d = static_cast<uint8_t *>(o->d_carry.ptr);
            rc = o->format == LX_OUT_BAM
                     ? bam_append_dev(h, "lx_out_append", program, m, n, ops, ops_bytes, &nm, q_res_ascii, q_ascii_off, &opt, d, &c, sink)
                     : text_append_dev(h, "lx_out_append", o->format, program, m, n, ops, ops_bytes, &nm, q_res_ascii, q_ascii_off, &opt, d, &c, sink);
            // (a refusal -- LX_EINVAL, before a kernel ran -- leaves the file and the carry's bytes as they were; any other failure ends
            // the file's use)
            if (rc && (rc != LX_EINVAL || io_failed))
                o->failed = true;
            if (!rc)
                o->dev_carry = c;
        }
    }
    catch (std::bad_alloc const &)
    {
        o->failed = true;
        return refuse(h, LX_ENOMEM, "lx_out_append: out of host memory");
    }
    return rc;
}

int lx_out_close(lx_out * o, int64_t footer_records)
{
    if (!o)
        return LX_OK;
    std::unique_ptr<lx_out> keep(o);
    lx_handle * const       h = o->h;
    if (!h)
        set_output_error("");
    int rc = LX_OK;
    try
    {
        if (!o->failed)
        {
            lx_bytes * footer = nullptr; // (.m9's "# BLAST processed N queries"; nothing for the other formats)
            rc = lx_render_records(o->format, 0, o->program.c_str(), nullptr, 0, nullptr, &o->subjects, nullptr, nullptr, &o->opt, footer_records, &footer);
            if (rc)
                rc = refuse_output(h, "lx_out_close", rc);
            else if (!(rc = put_host(o, footer)) && o->bgzf)
                rc = flush_host(o, true);
        }
        else
            rc = refuse(h, LX_EINVAL, "lx_out_close: an earlier call on " + o->path + " has failed; the file is incomplete");
    }
    catch (std::bad_alloc const &)
    {
        rc = refuse(h, LX_ENOMEM, "lx_out_close: out of host memory");
    }
    if (std::fclose(o->f) != 0 && !rc)
        rc = refuse(h, LX_EINVAL, "error while writing " + o->path + " (disk full?)");
    if (h && o->d_carry.ptr)
        (void)bind(h); // (the block goes back to the handle's device)
    return rc;
}

} // extern "C"
