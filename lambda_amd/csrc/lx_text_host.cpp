// lx_text_host.cpp -- the host side of the text record kernels (lx_text.hip): lx_render_text_dev, lx_write_text_dev.
//
// A call checks its arguments first (LX_OUT_BAM, the host writer's refusals: lxi::resolve_output and lxi::check_rows, numbers outside
// the formatter's domain, then what the BAM writer checks: lxi::rec_inputs -- the extent of the ops for SAM only: the tabular formats do not read them,
// as in the host writer, and a front end that wrote .m8 never kept them), and uploads what the kernels read: the BAM writer's inputs (rows, ops,
// query letters, lengths and first words, taxonomy, the groups' LCA), and beside them the columns, the first words and lengths of the
// subjects THE ROWS NAME (re-indexed: a large database's name list stays on the host), for .m9 the whole query ids and the constant
// parts of the comment lines.  Numbers and measure run over the whole list, the host cuts ranges within LX_OPT_BAM_RANGE_BYTES from
// the tiles' totals, and per range scan + emit fill the handle's stream buffer (lx_rec_host.h has the scheme).  The SAM header and
// the .m9 footer are made on the host.  lx_render_text_dev copies each range down (lxi::rec_drain); lx_write_text_dev does the same
// and writes the file (bgzf = 0), or keeps the stream on the device and compresses it where it stands, the footer uploaded behind the
// last range (bgzf = 1, lxi::rec_encode_ranges): the members lx_write_records_bgzf makes.
//
// lx_last_phase_ms: phase 12 = the text record kernels (groups, numbers, measure, scans, emit), phase 4 = the encoder's.
#include <unordered_map>

#include "lx_bgzf.h"
#include "lx_numfmt.h"
#include "lx_rec_host.h"
#include "lx_text.h"

using namespace lxi;

namespace
{

struct TextJob
{
    RecJob      rec;
    lx::TextCtx c{};
    std::string footer;
};

// what the arguments resolve to
struct Checked
{
    OutputRequest rq;
    uint32_t      tags = 0, need = 0; // tagBit(kTag*) whose inputs are wanted, kTextNum* texts
};

// (the handle may still be NULL here: the arguments are judged first, so that a caller learns what is wrong with them without a device)
int refuse(lx_handle * h, char const * who, int rc)
{
    return h ? rec_refuse(h, who, rc) : rc;
}

// the refusals that need no device: the format, the host writer's own, the formatter's domain
int check_args(lx_handle * h, char const * who, int format, char const * program, lx_blast_match const * m, uint64_t n, lx_seq_names const * names,
               lx_output_options const * opt_in, Checked & ck)
{
    if (format == LX_OUT_BAM)
    {
        set_output_error("LX_OUT_BAM is binary: lx_render_bam_dev / lx_write_bam_dev make it");
        return refuse(h, who, LX_EINVAL);
    }
    if (format != LX_OUT_BLAST_TAB && format != LX_OUT_BLAST_TAB_COMMENTS && format != LX_OUT_SAM)
    {
        set_output_error("unknown output format");
        return refuse(h, who, LX_EINVAL);
    }
    int rc = resolve_output(format, program, m, n, names, opt_in, ck.rq);
    if (rc == LX_OK) // (the BAM writer has no text here)
        rc = check_rows(m, n, names, "a record names a query or a subject the name lists do not have");
    if (rc != LX_OK)
        return refuse(h, who, rc);
    if (names->n_s && (!names->s_ids || !names->s_lens))
        return refuse(h, who, LX_EINVAL);
    for (uint64_t k = 0; k < n; ++k)
    {
        uint64_t bs, id;
        double const idd = (double)m[k].identity;
        std::memcpy(&bs, &m[k].bit_score, 8);
        std::memcpy(&id, &idd, 8);
        if (!lx::num_f_domain(bs) || !lx::num_f_domain(id))
        {
            set_output_error("a record's bit_score or identity is not finite or not below 10^15: the device writer does not print it");
            return refuse(h, who, LX_EINVAL);
        }
    }
    uint32_t tags = ck.rq.tag_mask, need = 0;
    if (ck.rq.sam)
        need = ck.rq.tags[lx::kTagEValue] ? 1u << lx::kTextNumAe : 0u;
    else
        for (int c : ck.rq.cols)
        {
            tags |= c == lx::kColSTaxIds ? lx::tagBit(lx::kTagSTaxIds) : c == lx::kColLcaTaxId ? lx::tagBit(lx::kTagLcaTaxId) : 0u;
            need |= c == lx::kColEValue    ? 1u << lx::kTextNumEValue
                    : c == lx::kColBitScore ? 1u << lx::kTextNumBitScore
                    : c == lx::kColPIdent   ? 1u << lx::kTextNumPIdent
                    : c == lx::kColPPos     ? 1u << lx::kTextNumPPos
                                            : 0u;
        }
    ck.tags = tags;
    ck.need = need;
    return LX_OK;
}

int prepare(lx_handle * h, char const * who, Checked const & ck, int write_header, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
            uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off, int64_t footer_records,
            TextJob & job)
{
    std::vector<int> const & cols   = ck.rq.cols;
    uint32_t const           need   = ck.need;
    int const                format = ck.rq.format;
    bool const               sam    = ck.rq.sam;
    int                      rc;
    if ((rc = rec_inputs(h, who, 12, ck.rq, ck.tags, sam, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, job.rec)))
        return rc;
    if (sam && write_header)
        job.rec.header = sam_header(names, ck.rq);
    if (format == LX_OUT_BLAST_TAB_COMMENTS && footer_records >= 0) // lx_write_footer
        job.footer = "# BLAST processed " + std::to_string((unsigned long long)footer_records) + " queries\n";
    if (n == 0)
        return LX_OK;

    // ---- what the text kernels read beside the BAM writer's inputs
    lx::TextCtx & c = job.c;
    c.b             = job.rec.c;
    c.format        = format;
    c.need          = need;
    std::vector<uint8_t> cols8(cols.begin(), cols.end());
    // the subjects the rows name, in the order of their first row
    std::vector<uint32_t> row_s(n);
    std::vector<uint64_t> named;
    if (names->n_s <= 8 * n + 1024) // a table over all subjects while that is no more than a few words per row, a hash map beyond
    {
        std::vector<uint32_t> index(names->n_s, 0xffffffffu);
        for (uint64_t k = 0; k < n; ++k)
        {
            uint32_t & at = index[m[k].n_sid];
            if (at == 0xffffffffu)
            {
                at = (uint32_t)named.size();
                named.push_back(m[k].n_sid);
            }
            row_s[k] = at;
        }
    }
    else
    {
        std::unordered_map<uint64_t, uint32_t> index;
        for (uint64_t k = 0; k < n; ++k)
        {
            auto const it = index.emplace(m[k].n_sid, (uint32_t)named.size());
            if (it.second)
                named.push_back(m[k].n_sid);
            row_s[k] = it.first->second;
        }
    }
    uint64_t const        ns = named.size();
    std::vector<uint64_t> s_lens(ns), sn_off(ns + 1, 0);
    for (uint64_t i = 0; i < ns; ++i)
    {
        char const * const id = names->s_ids[named[i]];
        s_lens[i]             = names->s_lens[named[i]];
        sn_off[i + 1]         = id ? std::strcspn(id, " \t") : 0; // firstWord
        if (sn_off[i + 1] > kRecMaxName)
        {
            set_output_error("a subject id longer than the device writer takes (2^20)");
            return rec_refuse(h, who, LX_EINVAL);
        }
        sn_off[i + 1] += sn_off[i];
    }
    std::vector<uint8_t> sn_blob(sn_off[ns]);
    for (uint64_t i = 0; i < ns; ++i)
        if (sn_off[i + 1] > sn_off[i])
            std::memcpy(sn_blob.data() + sn_off[i], names->s_ids[named[i]], sn_off[i + 1] - sn_off[i]);
    // .m9: the whole ids of the queries (printf's "(null)" for a missing one), the constant parts of the comment lines
    std::vector<uint64_t> qid_off;
    std::vector<uint8_t>  qid_blob;
    std::string           comment;
    if (format == LX_OUT_BLAST_TAB_COMMENTS)
    {
        uint64_t const n_q = names->n_q;
        qid_off.assign(n_q + 1, 0);
        for (uint64_t i = 0; i < n_q; ++i)
        {
            uint64_t const len = std::strlen(names->q_ids[i] ? names->q_ids[i] : "(null)");
            if (len > kRecMaxName)
            {
                set_output_error("a query id longer than the device writer takes (2^20)");
                return rec_refuse(h, who, LX_EINVAL);
            }
            qid_off[i + 1] = qid_off[i] + len;
        }
        qid_blob.resize(qid_off[n_q]);
        for (uint64_t i = 0; i < n_q; ++i)
            if (qid_off[i + 1] > qid_off[i])
                std::memcpy(qid_blob.data() + qid_off[i], names->q_ids[i] ? names->q_ids[i] : "(null)", qid_off[i + 1] - qid_off[i]);
        for (int i = 0; i < 3; ++i)
        {
            c.comment_off[i] = (uint32_t)comment.size();
            comment += ck.rq.m9[i];
        }
        c.comment_off[3] = (uint32_t)comment.size();
    }

    auto &          T       = h->text;
    uint8_t const * d_cols8 = nullptr;
    if ((rc = rec_upload(h, T.d_cols, cols8.data(), cols8.size(), d_cols8)) || (rc = rec_upload(h, T.d_row_s, row_s.data(), n, c.row_s)) ||
        (rc = rec_upload(h, T.d_slens, s_lens.data(), ns, c.s_lens)) || (rc = rec_upload(h, T.d_sn_off, sn_off.data(), ns + 1, c.sn_off)) ||
        (rc = rec_upload(h, T.d_sn_blob, sn_blob.data(), sn_blob.size(), c.sn_blob)))
        return rc;
    c.cols   = d_cols8;
    c.n_cols = (uint32_t)cols8.size();
    if (format == LX_OUT_BLAST_TAB_COMMENTS &&
        ((rc = rec_upload(h, T.d_qid_off, qid_off.data(), qid_off.size(), c.qid_off)) ||
         (rc = rec_upload(h, T.d_qid_blob, qid_blob.data(), qid_blob.size(), c.qid_blob)) ||
         (rc = rec_upload(h, T.d_comment, reinterpret_cast<uint8_t const *>(comment.data()), comment.size(), c.comment))))
        return rc;
    if ((rc = ensure(h, T.d_nums, std::max<uint64_t>(need ? n * sizeof(lx::TextNum) : 0, 16))))
        return rc;
    c.nums = static_cast<lx::TextNum *>(T.d_nums.ptr);

    // ---- number texts, sizes, and the tiles' totals for the cuts
    {
        PhaseTimer t(h, h->stream, 12);
        LX_HIP(h, lx::text_launch_numbers(c, h->stream));
        LX_HIP(h, lx::text_launch_measure(c, static_cast<uint64_t *>(h->bam.d_tiles.ptr), h->stream));
        t.close();
    }
    return rec_ranges(h, who, job.rec); // (it waits for the stream: the uploads' host arrays may go)
}

// one range's records into `out` (device)
int emit_range(lx_handle * h, TextJob const & job, RecRange const & r, uint8_t * out)
{
    auto &     B = h->bam;
    PhaseTimer t(h, h->stream, 12);
    LX_HIP(h, lx::text_launch_emit(job.c, r.first, r.count, static_cast<uint32_t *>(B.d_off.ptr), static_cast<uint32_t *>(B.d_scan.ptr), out,
                                   h->stream));
    t.close();
    return LX_OK;
}

// the whole text in host memory: the header, the ranges as they come down, the footer
int drain(lx_handle * h, TextJob const & job, std::string & bytes)
{
    bytes.reserve(job.rec.header.size() + job.rec.total + job.footer.size());
    bytes        = job.rec.header;
    int const rc = rec_drain(h, job.rec, [&](RecRange const & r, uint8_t * d) { return emit_range(h, job, r, d); }, bytes);
    if (rc)
        return rc;
    bytes += job.footer;
    return LX_OK;
}

} // namespace

namespace lxi
{

int text_append_dev(lx_handle * h, char const * who, int format, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                    uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                    lx_output_options const * opt, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink)
{
    Checked ck;
    int     rc = check_args(h, who, format, program, m, n, names, opt, ck);
    if (rc)
        return rc;
    if ((rc = rec_begin(h)))
        return rc;
    HostPool::Call in_call;
    try
    {
        TextJob job;
        if ((rc = prepare(h, who, ck, 0, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, -1, job)))
            return rc;
        return rec_append_ranges(h, job.rec, [&](RecRange const & r, uint8_t * out) { return emit_range(h, job, r, out); }, d_carry, carry, sink);
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "%s: out of host memory", who);
    }
}

} // namespace lxi

extern "C" {

int lx_render_text_dev(lx_handle * h, int format, int write_header, char const * program, lx_blast_match const * m, uint64_t n,
                       uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
                       uint64_t const * q_ascii_off, lx_output_options const * opt, int64_t footer_records, lx_bytes ** out)
{
    if (out)
        *out = nullptr;
    Checked ck;
    int     rc = check_args(h, "lx_render_text_dev", format, program, m, n, names, opt, ck);
    if (rc)
        return rc;
    if (!h)
    {
        set_output_error("lx_render_text_dev: the handle is NULL");
        return LX_EINVAL;
    }
    if (!out)
        return fail(h, LX_EINVAL, "lx_render_text_dev: out is NULL");
    if ((rc = rec_begin(h)))
        return rc;
    HostPool::Call in_call;
    try
    {
        TextJob job;
        std::string bytes;
        if ((rc = prepare(h, "lx_render_text_dev", ck, write_header, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, footer_records, job)) ||
            (rc = drain(h, job, bytes)))
            return rc;
        *out = bytes_adopt(std::move(bytes));
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "lx_render_text_dev: out of host memory");
    }
    return LX_OK;
}

int lx_write_text_dev(lx_handle * h, char const * path, int format, int bgzf, char const * program, lx_blast_match const * m, uint64_t n,
                      uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
                      uint64_t const * q_ascii_off, lx_output_options const * opt, int64_t footer_records)
{
    Checked ck;
    int     rc = check_args(h, "lx_write_text_dev", format, program, m, n, names, opt, ck);
    if (rc)
        return rc;
    if (!h)
    {
        set_output_error("lx_write_text_dev: the handle is NULL");
        return LX_EINVAL;
    }
    if (!path)
        return fail(h, LX_EINVAL, "lx_write_text_dev: path is NULL");
    if ((rc = rec_begin(h)))
        return rc;
    HostPool::Call       in_call;
    std::string          text;   // plain: the file.  It is written at once, when everything is made
    std::vector<uint8_t> packed; // bgzf: its members
    try
    {
        TextJob job;
        if ((rc = prepare(h, "lx_write_text_dev", ck, 1, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, footer_records, job)))
            return rc;
        if (!bgzf)
        {
            if ((rc = drain(h, job, text)))
                return rc;
        }
        else
        {
            if ((rc = rec_stream_front(h, job.rec, job.rec.header, job.footer.size())))
                return rc;
            packed.reserve((size_t)((job.rec.header.size() + job.rec.total) / 3 + 4096));
            uint64_t carry = job.rec.header.size();
            if ((rc = rec_encode_ranges(h, job.rec, [&](RecRange const & r, uint8_t * d) { return emit_range(h, job, r, d); }, &carry, &job.footer,
                                        true, rec_collect(packed))))
                return rc;
            packed.insert(packed.end(), lx::kEofMember, lx::kEofMember + sizeof(lx::kEofMember));
        }
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "lx_write_text_dev: out of host memory");
    }
    return bgzf ? rec_write_file(h, path, packed.data(), packed.size()) : rec_write_file(h, path, text.data(), text.size());
}

} // extern "C"
