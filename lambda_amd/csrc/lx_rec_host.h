// lx_rec_host.h -- the host side the device record writers share (lx_bam_host.cpp: BAM, lx_text_host.cpp: .m8 / .m9 / .sam), defined in
// lx_rec_host.cpp.  Not part of the ABI.  A call checks and flattens its inputs and uploads them (rec_inputs, which also runs the
// groups kernels), runs its own measure kernel, and cuts the list into ranges of whole tiles from the tiles' size totals (rec_ranges);
// the ranges then go, through the writer's emit, to host memory (rec_drain) or through the BGZF encoder (rec_encode_ranges).
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

// The refusals beyond the writer's own (the extent of the ops, the kernels' counters), job.c filled from the resolved request, everything
// the kernels of both writers read flattened and uploaded into h->bam, the per-record arrays sized, the groups made (device time to
// `phase`).  `tags`: the tagBit(kTag*) bits whose inputs are wanted (STaxIds: the subjects' taxa, LcaTaxId / LcaId: the groups' LCA and
// its name, ProtSeq: the genetic code).  rq.opt.q_qual goes up only for a writer with ops (SAM, BAM), a DNA query and a sam_seq other
// than never.  with_ops false: the writer does not read the ops (the tabular formats, like the host writer's), so their extent is not
// checked and they are not uploaded.  n == 0: only the refusals and the flags of job.c.
int rec_inputs(lx_handle * h, char const * who, int phase, OutputRequest const & rq, uint32_t tags, bool with_ops, lx_blast_match const * m,
               uint64_t n, uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
               uint64_t const * q_ascii_off, RecJob & job);
// after the measure kernel: the tiles' totals come down, job.ranges / max_range / total are made (LX_OPT_BAM_RANGE_BYTES)
int rec_ranges(lx_handle * h, char const * who, RecJob & job);

// a writer's emit: one range's records to a device address
using RecEmit    = std::function<int(RecRange const &, uint8_t *)>;
using MemberSink = std::function<int(uint8_t const *, uint64_t)>;

// The job's ranges to host memory, appended behind what `bytes` holds: the handle's stream buffer is sized for the largest range, and
// per range emit, copy, synchronise.
int rec_drain(lx_handle * h, RecJob const & job, RecEmit const & emit, std::string & bytes);
// The handle's stream buffer with room for `front` (or a carried block), the largest range and `tail_bytes`; `front` uploaded to its start.
int rec_stream_front(lx_handle * h, RecJob const & job, std::string const & front, uint64_t tail_bytes);
// The job's ranges through the BGZF encoder, the stream staying on the device: *carry bytes stand at the front of the stream buffer (a
// header of any length, or less than a block carried from an earlier call), each range is emitted behind what is carried, `tail` (NULL:
// none) goes behind the last range, the whole 65 280-byte blocks go through the encoder where they stand, their members to `sink`, and
// the rest moves to the front.  final: the rest is compressed too, as the stream's last block, and the stream is waited for; otherwise
// the rest stays at the front of the buffer, its size in *carry, and the caller waits for the stream when it has taken it away.  So the
// members are cut exactly where lx_bgzf_compress cuts them on the whole stream.
int rec_encode_ranges(lx_handle * h, RecJob const & job, RecEmit const & emit, uint64_t * carry, std::string const * tail, bool final,
                      MemberSink const & sink);
// a sink that collects the members in `packed`
MemberSink rec_collect(std::vector<uint8_t> & packed);
// a finished file's bytes to `path`, at once
int rec_write_file(lx_handle * h, char const * path, void const * data, size_t bytes);

// ---- one append of lx_out (lx_out_host.cpp) whose records are made on the device and compressed where they stand.  m[0, n) is
// rendered without header and footer behind the *carry (< 65 280) bytes of d_carry; the whole blocks of carry + records go through
// the BGZF encoder, their members to `sink`; what does not fill a block is back in d_carry (room for a block), its size in *carry.
// The refusals are those of the one-shot device writers, before any device work.
// the part both writers share: d_carry in front of the job's ranges, rec_encode_ranges, the rest back into d_carry
int rec_append_ranges(lx_handle * h, RecJob const & job, RecEmit const & emit, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink);
int bam_append_dev(lx_handle * h, char const * who, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                   uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                   lx_output_options const * opt, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink);
int text_append_dev(lx_handle * h, char const * who, int format, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                    uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                    lx_output_options const * opt, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink);

} // namespace lxi
