// lx_bam_host.cpp -- the host side of the BAM record kernels (lx_bam.hip): lx_render_bam_dev, lx_write_bam_dev, lxi::bam_append_dev.
//
// A call checks its arguments first (the host writer's refusals: lxi::resolve_output and lxi::check_rows; then lxi::rec_inputs'), has
// lxi::rec_inputs flatten and upload what the kernels read and run the groups kernels, runs its measure kernel, and has lxi::rec_ranges
// cut the list into ranges (lx_rec_host.h has the scheme).  Per range: scan + emit into the handle's stream buffer.  lx_render_bam_dev
// copies each range down behind the host-made header (lxi::rec_drain).  lx_write_bam_dev keeps the stream on the device: the header
// is uploaded in front of the first range and everything goes through the BGZF encoder where it stands (lxi::rec_encode_ranges): the
// file is the one lx_write_records_bgzf writes.  Only members come down.
//
// lx_last_phase_ms: phase 11 = the render kernels (groups, measure, scans, emit), phase 4 = the encoder's, as for lx_bgzf_compress.
#include "lx_bgzf.h"
#include "lx_rec_host.h"

using namespace lxi;

namespace
{

// checks, flattening, upload, groups + measure, the ranges
int prepare(lx_handle * h, char const * who, int write_header, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
            uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off, lx_output_options const * opt_in,
            RecJob & job)
{
    // ---- refusals, before any device work
    OutputRequest rq;
    int           rc = resolve_output(LX_OUT_BAM, program, m, n, names, opt_in, rq);
    if (rc == LX_OK)
        rc = check_rows(m, n, names, nullptr); // (no text, where the text writer has one: "bad arguments" -- kept as it is)
    if (rc != LX_OK)
        return rec_refuse(h, who, rc);
    if ((rc = rec_inputs(h, who, 11, rq, rq.tag_mask, true, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, job)))
        return rc;
    if (write_header)
        job.header = bam_header(names, rq);
    if (n == 0)
        return LX_OK;
    // ---- sizes, and the tiles' totals for the cuts
    {
        PhaseTimer t(h, h->stream, 11);
        LX_HIP(h, lx::bam_launch_measure(job.c, static_cast<uint64_t *>(h->bam.d_tiles.ptr), h->stream));
        t.close();
    }
    return rec_ranges(h, who, job);
}

// one range's records into `out` (device)
int emit_range(lx_handle * h, RecJob const & job, RecRange const & r, uint8_t * out)
{
    auto &     B = h->bam;
    PhaseTimer t(h, h->stream, 11);
    LX_HIP(h, lx::bam_launch_emit(job.c, r.first, r.count, static_cast<uint32_t *>(B.d_off.ptr), static_cast<uint32_t *>(B.d_scan.ptr), out, h->stream));
    t.close();
    return LX_OK;
}

} // namespace

namespace lxi
{

int bam_append_dev(lx_handle * h, char const * who, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                   uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                   lx_output_options const * opt, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink)
{
    int rc = rec_begin(h);
    if (rc)
        return rc;
    HostPool::Call in_call;
    try
    {
        RecJob job;
        if ((rc = prepare(h, who, 0, program, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, opt, job)))
            return rc;
        return rec_append_ranges(h, job, [&](RecRange const & r, uint8_t * out) { return emit_range(h, job, r, out); }, d_carry, carry, sink);
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "%s: out of host memory", who);
    }
}

} // namespace lxi

extern "C" {

int lx_render_bam_dev(lx_handle * h, int write_header, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                      uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                      lx_output_options const * opt, lx_bytes ** out)
{
    if (!h)
        return LX_EINVAL;
    if (!out)
        return fail(h, LX_EINVAL, "lx_render_bam_dev: out is NULL");
    *out   = nullptr;
    int rc = rec_begin(h);
    if (rc)
        return rc;
    HostPool::Call in_call;
    try
    {
        RecJob job;
        if ((rc = prepare(h, "lx_render_bam_dev", write_header, program, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, opt, job)))
            return rc;
        std::string bytes;
        bytes.reserve(job.header.size() + job.total);
        bytes = job.header;
        if ((rc = rec_drain(h, job, [&](RecRange const & r, uint8_t * d) { return emit_range(h, job, r, d); }, bytes)))
            return rc;
        *out = bytes_adopt(std::move(bytes));
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "lx_render_bam_dev: out of host memory");
    }
    return LX_OK;
}

int lx_write_bam_dev(lx_handle * h, char const * path, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                     uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                     lx_output_options const * opt)
{
    if (!h)
        return LX_EINVAL;
    if (!path)
        return fail(h, LX_EINVAL, "lx_write_bam_dev: path is NULL");
    int rc = rec_begin(h);
    if (rc)
        return rc;
    HostPool::Call       in_call;
    std::vector<uint8_t> packed; // the members: the file is written at once, like lx_write_records_bgzf's
    try
    {
        RecJob job;
        if ((rc = prepare(h, "lx_write_bam_dev", 1, program, m, n, ops, ops_bytes, names, q_res_ascii, q_ascii_off, opt, job)) ||
            (rc = rec_stream_front(h, job, job.header, 0)))
            return rc;
        packed.reserve((size_t)((job.header.size() + job.total) / 3 + 4096));
        uint64_t carry = job.header.size();
        if ((rc = rec_encode_ranges(h, job, [&](RecRange const & r, uint8_t * d) { return emit_range(h, job, r, d); }, &carry, nullptr, true,
                                    rec_collect(packed))))
            return rc;
        packed.insert(packed.end(), lx::kEofMember, lx::kEofMember + sizeof(lx::kEofMember));
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "lx_write_bam_dev: out of host memory");
    }
    return rec_write_file(h, path, packed.data(), packed.size());
}

} // extern "C"
