// lx_text_host.cpp -- the host side of the text record kernels (lx_text.hip): lx_render_text_dev, lx_write_text_dev.
//
// A call checks its arguments first (renderRecords' refusals through lxi::text_check, LX_OUT_BAM, numbers outside the formatter's
// domain, then what the BAM writer checks: lxi::rec_inputs -- the extent of the ops for SAM only: the tabular formats do not read them,
// as in the host writer, and a front end that wrote .m8 never kept them), and uploads what the kernels read: the BAM writer's inputs (rows, ops,
// query letters, lengths and first words, taxonomy, the groups' LCA), and beside them the columns, the first words and lengths of the
// subjects THE ROWS NAME (re-indexed: a large database's name list stays on the host), for .m9 the whole query ids and the constant
// parts of the comment lines.  Numbers and measure run over the whole list, the host cuts ranges within LX_OPT_BAM_RANGE_BYTES from
// the tiles' totals, and per range scan + emit fill the handle's stream buffer (lx_bam_host.cpp has the scheme).  The SAM header and
// the .m9 footer are made on the host.  lx_render_text_dev copies each range down; lx_write_text_dev writes the ranges to the file
// as they come (bgzf = 0), or keeps the stream on the device and compresses it where it stands, less than a block carried into the
// next range, the footer uploaded behind the last (bgzf = 1): the members lx_write_records_bgzf makes.
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
    std::vector<int> cols;
    uint32_t         tags = 0, need = 0; // kBamTag* whose inputs are wanted, kTextNum* texts
};

// (the handle may still be NULL here: the arguments are judged first, so that a caller learns what is wrong with them without a device)
int refuse(lx_handle * h, char const * who, int rc)
{
    return h ? rec_refuse(h, who, rc) : rc;
}

// the refusals that need no device: the format, renderRecords' own, the formatter's domain
int check_args(lx_handle * h, char const * who, int format, char const * program, lx_blast_match const * m, uint64_t n, lx_seq_names const * names,
               lx_output_options const * opt_in, Checked & ck)
{
    std::vector<int> & cols = ck.cols;
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
    uint32_t tags = 0;
    int      rc   = text_check(format, program, m, n, names, opt_in, cols, &tags);
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
    bool const sam = format == LX_OUT_SAM;
    uint32_t   need = 0;
    if (sam)
        need = tags & lx::kBamTagAe ? 1u << lx::kTextNumAe : 0u;
    else
    {
        tags = 0;
        for (int c : cols)
        {
            tags |= c == lx::kTextColSTaxIds ? lx::kBamTagSt : c == lx::kTextColLcaTaxId ? lx::kBamTagLt : 0u;
            need |= c == lx::kTextColEValue    ? 1u << lx::kTextNumEValue
                    : c == lx::kTextColBitScore ? 1u << lx::kTextNumBitScore
                    : c == lx::kTextColPIdent   ? 1u << lx::kTextNumPIdent
                    : c == lx::kTextColPPos     ? 1u << lx::kTextNumPPos
                                                : 0u;
        }
    }
    ck.tags = tags;
    ck.need = need;
    return LX_OK;
}

int prepare(lx_handle * h, char const * who, Checked const & ck, int format, int write_header, char const * program, lx_blast_match const * m,
            uint64_t n, uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
            uint64_t const * q_ascii_off, lx_output_options const * opt_in, int64_t footer_records, TextJob & job)
{
    std::vector<int> const & cols = ck.cols;
    uint32_t const           tags = ck.tags, need = ck.need;
    bool const               sam  = format == LX_OUT_SAM;
    int                      rc;
    if ((rc = rec_inputs(h, who, 12, tags, sam, program, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, opt_in, job.rec)))
        return rc;
    if (sam && write_header)
        job.rec.header = sam_header(names, opt_in, tags);
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
        std::string parts[3];
        m9_comment_parts(program, opt_in, cols, parts);
        for (int i = 0; i < 3; ++i)
        {
            c.comment_off[i] = (uint32_t)comment.size();
            comment += parts[i];
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
        if ((rc = prepare(h, who, ck, format, 0, program, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, opt, -1, job)))
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
        if ((rc = prepare(h, "lx_render_text_dev", ck, format, write_header, program, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, opt,
                          footer_records, job)))
            return rc;
        std::string bytes;
        bytes.reserve(job.rec.header.size() + job.rec.total + job.footer.size());
        bytes = job.rec.header;
        if ((rc = ensure(h, h->bam.d_stream, std::max<uint64_t>(job.rec.max_range, 16))))
            return rc;
        uint8_t * const d = static_cast<uint8_t *>(h->bam.d_stream.ptr);
        for (RecRange const & r : job.rec.ranges)
        {
            if ((rc = emit_range(h, job, r, d)))
                return rc;
            size_t const at = bytes.size();
            bytes.resize(at + r.bytes);
            LX_HIP(h, hipMemcpyAsync(&bytes[at], d, r.bytes, hipMemcpyDeviceToHost, h->stream));
            LX_HIP(h, hipStreamSynchronize(h->stream));
        }
        bytes += job.footer;
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
    std::vector<uint8_t> packed; // bgzf: the members; plain: the text.  The file is written at once, when everything is made
    try
    {
        TextJob job;
        if ((rc = prepare(h, "lx_write_text_dev", ck, format, 1, program, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, opt, footer_records,
                          job)))
            return rc;
        RecJob const &    rec = job.rec;
        hipStream_t const s   = h->stream;
        if (!bgzf)
        {
            packed.reserve((size_t)(rec.header.size() + rec.total + job.footer.size()));
            packed.assign(rec.header.begin(), rec.header.end());
            if ((rc = ensure(h, h->bam.d_stream, std::max<uint64_t>(rec.max_range, 16))))
                return rc;
            uint8_t * const d = static_cast<uint8_t *>(h->bam.d_stream.ptr);
            for (RecRange const & r : rec.ranges)
            {
                if ((rc = emit_range(h, job, r, d)))
                    return rc;
                size_t const at = packed.size();
                packed.resize(at + r.bytes);
                LX_HIP(h, hipMemcpyAsync(&packed[at], d, r.bytes, hipMemcpyDeviceToHost, s));
                LX_HIP(h, hipStreamSynchronize(s));
            }
            packed.insert(packed.end(), job.footer.begin(), job.footer.end());
        }
        else
        {
            // the stream buffer: what is carried (the header in front of the first range, less than a block later) + a range + the footer
            uint64_t const carry_max = std::max<uint64_t>(rec.header.size(), lx::kBgzfBlock);
            if ((rc = ensure(h, h->bam.d_stream, carry_max + rec.max_range + job.footer.size() + 16)))
                return rc;
            uint8_t * const d = static_cast<uint8_t *>(h->bam.d_stream.ptr);
            packed.reserve((size_t)((rec.header.size() + rec.total) / 3 + 4096));
            auto sink = [&](uint8_t const * members, uint64_t bytes) -> int
            {
                packed.insert(packed.end(), members, members + bytes);
                return LX_OK;
            };
            uint64_t carry = rec.header.size();
            if (carry)
                LX_HIP(h, hipMemcpyAsync(d, rec.header.data(), carry, hipMemcpyHostToDevice, s));
            if (rec.ranges.empty())
            {
                if (!job.footer.empty())
                    LX_HIP(h, hipMemcpyAsync(d + carry, job.footer.data(), job.footer.size(), hipMemcpyHostToDevice, s));
                if (carry + job.footer.size() && (rc = bgzf_compress_dev(h, d, carry + job.footer.size(), sink)))
                    return rc;
            }
            for (size_t i = 0; i < rec.ranges.size(); ++i)
            {
                RecRange const & r    = rec.ranges[i];
                bool const       last = i + 1 == rec.ranges.size();
                if ((rc = emit_range(h, job, r, d + carry)))
                    return rc;
                uint64_t have = carry + r.bytes;
                if (last && !job.footer.empty())
                {
                    LX_HIP(h, hipMemcpyAsync(d + have, job.footer.data(), job.footer.size(), hipMemcpyHostToDevice, s));
                    have += job.footer.size();
                }
                uint64_t const whole = last ? have : have / lx::kBgzfBlock * lx::kBgzfBlock;
                if ((rc = bgzf_compress_dev(h, d, whole, sink)))
                    return rc;
                carry = have - whole;
                if (carry && whole) // (whole is at least a block, the rest less: the two do not overlap)
                    LX_HIP(h, hipMemcpyAsync(d, d + whole, carry, hipMemcpyDeviceToDevice, s));
            }
            LX_HIP(h, hipStreamSynchronize(s));
            packed.insert(packed.end(), lx::kEofMember, lx::kEofMember + sizeof(lx::kEofMember));
        }
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "lx_write_text_dev: out of host memory");
    }
    std::FILE * f = std::fopen(path, "wb");
    if (!f)
        return fail(h, LX_EINVAL, "cannot open %s", path);
    bool ok = std::fwrite(packed.data(), 1, packed.size(), f) == packed.size();
    ok      = (std::fclose(f) == 0) && ok;
    return ok ? LX_OK : fail(h, LX_EINVAL, "error while writing %s (disk full?)", path);
}

} // extern "C"
