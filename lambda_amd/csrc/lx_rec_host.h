// lx_rec_host.h -- the host side the device record writers share (lx_bam_host.cpp: BAM, lx_text_host.cpp: .m8 / .m9 / .sam).  Not part
// of the ABI.  A call checks and flattens its inputs and uploads them (rec_inputs, which also runs the groups kernels), runs its own
// measure kernel, and cuts the list into ranges of whole tiles from the tiles' size totals (rec_ranges); per range it runs its emit.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "lx_bam.h"
#include "lx_internal.h"

namespace lxi
{

struct RecRange
{
    uint64_t first, count, bytes;
};

struct RecJob
{
    lx::BamCtx            c{};
    std::string           header;
    std::vector<RecRange> ranges;
    uint64_t              max_range = 0, total = 0;
};

constexpr uint64_t kRecMaxName = 1ull << 20; // characters of an id or a taxon name

// fail() with lx_last_output_error()'s text behind the caller's name
int rec_refuse(lx_handle * h, char const * who, int rc);
// binds the handle's device and forgets the last call's phases
int rec_begin(lx_handle * h);

template <class T>
int rec_upload(lx_handle * h, DevBuf & b, T const * src, uint64_t count, T const *& dev)
{
    uint64_t const bytes = count * sizeof(T);
    int const      rc    = ensure(h, b, std::max<uint64_t>(bytes, 16));
    if (rc)
        return rc;
    if (bytes)
        LX_HIP(h, hipMemcpyAsync(b.ptr, src, bytes, hipMemcpyHostToDevice, h->stream));
    dev = static_cast<T const *>(b.ptr);
    return LX_OK;
}

// The refusals beyond the writer's own (the extent of the ops, the kernels' counters), job.c filled from the arguments, everything
// the kernels of both writers read flattened and uploaded into h->bam, the per-record arrays sized, the groups made (device time to
// `phase`).  `tags`: the kBamTag* bits whose inputs are wanted (St: the subjects' taxa, Lt / Ls: the groups' LCA and its name, Qs: the
// genetic code).  opt_in->q_qual goes up only for a writer with ops (SAM, BAM), a DNA query and a sam_seq other than never.  with_ops false: the writer does not read the ops (the tabular formats, like the host writer's), so their extent is
// not checked and they are not uploaded.  n == 0: only the refusals and the flags of job.c.
int rec_inputs(lx_handle * h, char const * who, int phase, uint32_t tags, bool with_ops, char const * program, lx_blast_match const * m, uint64_t n,
               uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
               lx_output_options const * opt_in, RecJob & job);
// after the measure kernel: the tiles' totals come down, job.ranges / max_range / total are made (LX_OPT_BAM_RANGE_BYTES)
int rec_ranges(lx_handle * h, char const * who, RecJob & job);

// ---- one append of lx_out (lx_out_host.cpp) whose records are made on the device and compressed where they stand.  m[0, n) is
// rendered without header and footer behind the *carry (< 65 280) bytes of d_carry; the whole blocks of carry + records go through
// the BGZF encoder, their members to `sink`; what does not fill a block is back in d_carry (room for a block), its size in *carry.
// The refusals are those of the one-shot device writers, before any device work.
using MemberSink = std::function<int(uint8_t const *, uint64_t)>;
// the part both writers share: the job's ranges through `emit` (a range's records to a device address) and the encoder
int rec_append_ranges(lx_handle * h, RecJob const & job, std::function<int(RecRange const &, uint8_t *)> const & emit, uint8_t * d_carry,
                      uint64_t * carry, MemberSink const & sink);
int bam_append_dev(lx_handle * h, char const * who, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                   uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                   lx_output_options const * opt, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink);
int text_append_dev(lx_handle * h, char const * who, int format, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                    uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                    lx_output_options const * opt, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink);

} // namespace lxi
