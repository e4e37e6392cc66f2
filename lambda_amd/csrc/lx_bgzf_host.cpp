// lx_bgzf_host.cpp -- the host side of the BGZF encoder (lx_bgzf.hip): lx_bgzf_bound, lx_bgzf_compress, lx_write_records_bgzf, and the
// same pipeline over bytes that stand on the device already (lxi::bgzf_compress_dev: the BAM records of lx_bam_host.cpp).
//
// lx_bgzf_compress streams its input through the device in chunks of kChunkBlocks blocks (33 MB), so that a large output never
// needs all of its bytes on the device at once.  Per chunk, on the handle's stream: upload from a pinned lane, the two kernels,
// the size of the chunk's members back; then the members themselves.  The host copies the next chunk into the other pinned lane
// while the device encodes this one, and copies this chunk's members out while the device encodes the next.
#include "lx_bgzf.h"
#include "lx_internal.h"

using namespace lxi;

namespace
{

constexpr uint32_t kChunkBlocks = 512;
constexpr uint64_t kChunkBytes  = (uint64_t)kChunkBlocks * lx::kBgzfBlock;

using lx::kEofMember;

// The chunk pipeline of lx_bgzf_compress over n bytes: from host memory (host_in: through the pinned lanes into the chunk's device
// buffer) or where they stand on the device (dev_in, 16-byte aligned: every chunk begins at a multiple of kChunkBytes).  Each chunk's
// members go to `sink` in order.
int compress_chunks(lx_handle * h, uint8_t const * host_in, uint8_t const * dev_in, uint64_t n,
                    std::function<int(uint8_t const *, uint64_t)> const & sink)
{
    int            rc     = LX_OK;
    auto &         B      = h->bgzf;
    uint64_t const first  = std::min(n, kChunkBytes);
    uint64_t const blocks = (first + lx::kBgzfBlock - 1) / lx::kBgzfBlock;
    if (n > 0 &&
        ((host_in && (rc = ensure(h, B.d_in, blocks * lx::kBgzfBlock))) || (rc = ensure(h, B.d_slots, blocks * lx::kBgzfSlot)) ||
         (rc = ensure(h, B.d_dist, blocks * lx::kBgzfBlock * 2)) || (rc = ensure(h, B.d_sym, blocks * lx::kBgzfBlock * 2)) ||
         (rc = ensure(h, B.d_sizes, blocks * 4)) || (rc = ensure(h, B.d_out, blocks * lx::kBgzfSlot)) || (rc = ensure(h, B.d_total, 8)) ||
         (host_in && ((rc = ensure_pinned(h, B.p_in[0], first, kExact)) || (rc = ensure_pinned(h, B.p_in[1], first, kExact)))) ||
         (rc = ensure_pinned(h, B.p_out, blocks * lx::kBgzfSlot, kExact)) || (rc = ensure_pinned(h, B.p_total, 8, kExact))))
        return rc;
    hipStream_t const s     = h->stream;
    uint64_t * const  total = static_cast<uint64_t *>(B.p_total.ptr);
    // queues chunk c (its bytes already in its pinned lane, or on the device): upload, kernels, the size of its members
    auto enqueue = [&](uint64_t c) -> int
    {
        uint64_t const at = c * kChunkBytes, len = std::min(kChunkBytes, n - at);
        if (host_in)
            LX_HIP(h, hipMemcpyAsync(B.d_in.ptr, B.p_in[c & 1].ptr, len, hipMemcpyHostToDevice, s));
        lx::BgzfParams p{host_in ? static_cast<uint8_t const *>(B.d_in.ptr) : dev_in + at, len, (uint32_t)((len + lx::kBgzfBlock - 1) / lx::kBgzfBlock),
                         static_cast<uint8_t *>(B.d_slots.ptr), static_cast<uint16_t *>(B.d_dist.ptr), static_cast<uint16_t *>(B.d_sym.ptr),
                         static_cast<uint32_t *>(B.d_sizes.ptr), static_cast<uint8_t *>(B.d_out.ptr), static_cast<uint64_t *>(B.d_total.ptr)};
        PhaseTimer t(h, s, 4);
        LX_HIP(h, lx::launch_bgzf(p, s));
        t.close();
        LX_HIP(h, hipMemcpyAsync(total, B.d_total.ptr, 8, hipMemcpyDeviceToHost, s));
        return LX_OK;
    };
    uint64_t const chunks = (n + kChunkBytes - 1) / kChunkBytes;
    if (chunks > 0)
    {
        if (host_in)
            std::memcpy(B.p_in[0].ptr, host_in, first);
        if ((rc = enqueue(0)))
            return rc;
    }
    for (uint64_t c = 0; c < chunks; ++c)
    {
        if (host_in && c + 1 < chunks) // the next chunk into the other lane (its last reader, the upload of chunk c - 1, is done)
        {
            uint64_t const at = (c + 1) * kChunkBytes;
            std::memcpy(B.p_in[(c + 1) & 1].ptr, host_in + at, std::min(kChunkBytes, n - at));
        }
        LX_HIP(h, hipStreamSynchronize(s));
        uint64_t const bytes = *total;
        if (bytes > blocks * lx::kBgzfSlot)
            return fail(h, LX_EHIP, "lx_bgzf_compress: the encoder reported %llu bytes for a chunk", (unsigned long long)bytes);
        LX_HIP(h, hipMemcpyAsync(B.p_out.ptr, B.d_out.ptr, bytes, hipMemcpyDeviceToHost, s));
        hipEvent_t const down = pool_event(h);
        if (!down)
            return fail(h, LX_EHIP, "lx_bgzf_compress: no event");
        LX_HIP(h, hipEventRecord(down, s));
        if (c + 1 < chunks && (rc = enqueue(c + 1)))
            return rc;
        LX_HIP(h, hipEventSynchronize(down));
        if ((rc = sink(static_cast<uint8_t const *>(B.p_out.ptr), bytes)))
            return rc;
    }
    return LX_OK;
}

} // namespace

namespace lxi
{
int bgzf_compress_dev(lx_handle * h, uint8_t const * d_in, uint64_t n, std::function<int(uint8_t const *, uint64_t)> const & sink)
{
    return compress_chunks(h, nullptr, d_in, n, sink);
}
} // namespace lxi

extern "C" {

uint64_t lx_bgzf_bound(uint64_t n)
{
    return n + (n + lx::kBgzfBlock - 1) / lx::kBgzfBlock * lx::kBgzfMemberOverhead + sizeof(kEofMember);
}

int lx_bgzf_compress(lx_handle * h, uint8_t const * in, uint64_t n, uint8_t * out, uint64_t cap, uint64_t * out_n, int32_t flags)
{
    if (!h)
        return LX_EINVAL;
    if ((!in && n) || !out || !out_n || (flags & ~LX_BGZF_EOF))
        return fail(h, LX_EINVAL, "lx_bgzf_compress: NULL buffer or unknown flags");
    if (cap < lx_bgzf_bound(n))
        return fail(h, LX_EINVAL, "lx_bgzf_compress: cap %llu is below lx_bgzf_bound(%llu) = %llu", (unsigned long long)cap,
                    (unsigned long long)n, (unsigned long long)lx_bgzf_bound(n));
    *out_n = 0;
    int rc = bind(h);
    if (rc)
        return rc;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    uint64_t w      = 0;
    rc              = compress_chunks(h, in, nullptr, n,
                                      [&](uint8_t const * members, uint64_t bytes) -> int
                                      {
                                          if (w + bytes > cap)
                                              return fail(h, LX_EHIP, "lx_bgzf_compress: the encoder reported %llu bytes for a chunk", (unsigned long long)bytes);
                                          std::memcpy(out + w, members, bytes);
                                          w += bytes;
                                          return LX_OK;
                                      });
    if (rc)
        return rc;
    if (flags & LX_BGZF_EOF)
    {
        std::memcpy(out + w, kEofMember, sizeof(kEofMember));
        w += sizeof(kEofMember);
    }
    *out_n = w;
    return LX_OK;
}

int lx_write_records_bgzf(lx_handle * h, char const * path, int format, char const * program, lx_blast_match const * m, uint64_t n,
                          uint8_t const * ops, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                          lx_output_options const * opt, int64_t footer_records)
{
    if (!h)
        return LX_EINVAL;
    if (!path)
        return fail(h, LX_EINVAL, "lx_write_records_bgzf: path is NULL");
    lx_bytes * raw = nullptr;
    int        rc  = lx_render_records(format, 1, program, m, n, ops, names, q_res_ascii, q_ascii_off, opt, footer_records, &raw);
    if (rc != LX_OK)
        return fail(h, rc, "lx_write_records_bgzf: %s", *lx_last_output_error() ? lx_last_output_error() : "bad arguments");
    uint64_t const       size = lx_bytes_size(raw);
    std::vector<uint8_t> packed;
    try
    {
        packed.resize(lx_bgzf_bound(size));
    }
    catch (...)
    {
        lx_bytes_free(raw);
        return fail(h, LX_ENOMEM, "lx_write_records_bgzf: out of host memory");
    }
    uint64_t got = 0;
    rc           = lx_bgzf_compress(h, lx_bytes_data(raw), size, packed.data(), packed.size(), &got, LX_BGZF_EOF);
    lx_bytes_free(raw);
    if (rc != LX_OK)
        return rc;
    std::FILE * f = std::fopen(path, "wb");
    if (!f)
        return fail(h, LX_EINVAL, "cannot open %s", path);
    bool ok = std::fwrite(packed.data(), 1, got, f) == got;
    ok      = (std::fclose(f) == 0) && ok;
    return ok ? LX_OK : fail(h, LX_EINVAL, "error while writing %s (disk full?)", path);
}

} // extern "C"
