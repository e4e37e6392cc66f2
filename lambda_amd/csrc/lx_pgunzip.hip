// lx_pgunzip.hip -- a plain gzip member on the device (gfx950 only): the launches around lx_pgunzip.h.  Per wave of chunks, cut by
// the host (lx_gunzip_host.cpp), in this order on one stream, with nothing for the host to do in between:
//   find_kernel     one workgroup per chunk but the first: its lanes run precheck() on consecutive bit offsets; the few offsets
//                   that pass are taken smallest first by one lane each through block_starts() with the tables in LDS.
//   decode_kernel   one decoder (one lane) per found chunk: decode_chunk() with the last 32 Ki symbols in an LDS ring (64 KiB; with
//                   the tables ~70 KiB, two decoders per CU), every symbol also to the chunk's room in global memory; the input is
//                   read from global memory.  A chunk's stop bit and room reach to the next found chunk (plan_chunk), at most kMaxAbsorb chunks away.
//   chain_kernel    one lane: chain_wave() -- the chunks that begin on the bit their predecessor ended on, their places in the
//                   wave's bytes, and the WaveResult the host reads after the wave (counts, end bit, first status).
//   window_kernel   one workgroup walks the verified chunks in order: window v + the last 32 Ki symbols of chunk v = window v + 1.
//   bytes_kernel    one workgroup per 32 Ki symbols: symbols to bytes through the chunk's window into LDS, from there to their
//                   final offset, and the CRC32 by per-lane slices weighted with x^(8 k) mod P (as lx_gunzip.hip's member_kernel).
//                   Both are launched for every slot and read the number of verified chunks on the device.
// Bounds: a chunk's symbols stay inside [slot * room, next found slot * room) (MarkerSink), the input reads inside the wave's bytes
// (Inflater, Bits), the windows inside (nslots + 1) windows, the bytes inside out_cap (checked per segment against the wave's length,
// which chain_wave() keeps within the slots' room).
#include <hip/hip_runtime.h>

#include "lx_pgunzip.h"

namespace lx
{
namespace pgunzip
{

constexpr uint32_t kFindThreads   = 256;
constexpr uint32_t kDecodeThreads = 64;
constexpr uint32_t kDecodeLds     = kWindow * 2 + sizeof(inflate::Tables);
constexpr uint32_t kSeg           = 32768; // symbols per workgroup of bytes_kernel
constexpr uint32_t kByteThreads   = 256;
constexpr uint32_t kBytesAtATime  = 8;     // bytes_kernel's grid in y: a chunk of the default size has about 8 segments

static_assert(2 * kDecodeLds <= 160 * 1024, "two decoders per CU");

__global__ __launch_bounds__(kFindThreads) void find_kernel(WaveParams p)
{
    __shared__ inflate::Tables T;
    __shared__ uint32_t        s_min, s_done;
    uint32_t const             tid = threadIdx.x, j = blockIdx.x + 1;
    if (j >= p.nslots)
        return;
    uint64_t const lo = 8ull * j * p.chunk, hi = min(8ull * (j + 1) * p.chunk, 8ull * p.n);
    if (tid == 0)
        s_done = 0;
    __syncthreads();
    for (uint64_t base = lo; base < hi; base += kFindThreads)
    {
        uint64_t const off  = base + tid;
        bool           cand = off < hi && precheck(p.in, p.n, off);
        for (;;) // the candidates of this round, smallest offset first
        {
            if (tid == 0)
                s_min = 0xffffffffu;
            __syncthreads();
            if (cand)
                atomicMin(&s_min, tid);
            __syncthreads();
            uint32_t const m = s_min;
            if (m == 0xffffffffu)
                break;
            if (tid == m)
            {
                cand = false;
                if (block_starts<uint32_t>(p.in, p.n, off, T))
                {
                    p.found[j] = off;
                    s_done     = 1;
                }
            }
            __syncthreads();
            if (s_done)
                return;
        }
    }
    if (tid == 0)
        p.found[j] = kNone;
}

__global__ __launch_bounds__(kDecodeThreads) void decode_kernel(WaveParams p)
{
    extern __shared__ __align__(16) uint8_t lds[];
    uint32_t const j = blockIdx.x;
    if (threadIdx.x != 0 || j >= p.nslots)
        return;
    ChunkPlan const pl = plan_chunk(p.found, p.nslots, j, p.room, p.stop_bit);
    if (pl.status)
    {
        p.res[j] = ChunkResult{0, 0, 0, pl.status, 0};
        return;
    }
    inflate::Tables & T = *reinterpret_cast<inflate::Tables *>(lds + kWindow * 2);
    MarkerSink        sink{reinterpret_cast<uint16_t *>(lds), p.sym + (uint64_t)j * p.room, 0, pl.cap, j == 0 && p.first_wave ? 0u : kWindow};
    p.res[j] = decode_chunk<uint32_t>(p.in, p.n, pl.b0, pl.b1, sink, T);
}

// one wavefront, one lane at work: the chain is a serial walk over at most kMaxWaveSlots slots
__global__ __launch_bounds__(64) void chain_kernel(ChainParams p)
{
    __shared__ uint32_t idx[kMaxWaveSlots];
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    WaveResult o{0, 0, 0, 0, 0, (uint32_t)kChunkSkipped, 0, 2, 0, 0};
    if (p.nslots <= kMaxWaveSlots)
        chain_wave(p.found, p.res, p.nslots, p.room, p.before, idx, p.ver, o);
    *p.out = o;
}

__global__ __launch_bounds__(1024) void window_kernel(ResolveParams p)
{
    bool           bad  = false;
    uint32_t const nver = min(p.wr->nver, p.nslots);
    for (uint32_t v = 0; v < nver; ++v)
    {
        Verified const         e   = p.ver[v];
        uint8_t const * const  win = p.win + (uint64_t)v * kWindow;
        uint8_t * const        nxt = p.win + (uint64_t)(v + 1) * kWindow;
        uint16_t const * const s   = p.sym + e.sym_off;
        for (uint32_t i = threadIdx.x; i < kWindow; i += 1024)
            nxt[i] = next_window_at(i, s, e.count, win, e.valid, bad);
        __syncthreads(); // (window v + 1 is complete, and visible to the workgroup, before it is read)
    }
    if (bad)
        atomicOr(&p.wr->bad, 1u);
}

// grid (nslots, segments at a time): workgroup (v, y) takes segments y, y + gridDim.y, ... of verified chunk v
__global__ __launch_bounds__(kByteThreads) void bytes_kernel(ResolveParams p)
{
    __shared__ __align__(16) uint8_t buf[kSeg];
    __shared__ uint32_t              tab[256];
    __shared__ uint32_t              s_crc;
    uint32_t const                   tid = threadIdx.x, v = blockIdx.x;
    if (v >= p.wr->nver || v >= p.nslots) // (uniform)
        return;
    Verified const e        = p.ver[v];
    uint64_t const wave_len = p.wr->wave_len;
    tab[tid] = crc_table_entry(tid);
    for (uint32_t seg = blockIdx.y; seg < p.max_seg && (uint64_t)seg * kSeg < e.count; seg += gridDim.y) // (uniform)
    {
        uint32_t const s0 = seg * kSeg;
        uint32_t const nb = min(kSeg, e.count - s0);
        if (wave_len > p.out_cap || e.byte_off > wave_len || (uint64_t)s0 + nb > wave_len - e.byte_off)
        {
            if (tid == 0)
                atomicOr(&p.wr->bad, 2u);
            return;
        }
        if (tid == 0)
            s_crc = 0;
        uint16_t const * const s   = p.sym + e.sym_off + s0;
        uint8_t const * const  win = p.win + (uint64_t)v * kWindow;
        bool                   bad = false;
        for (uint32_t i = tid; i < nb; i += kByteThreads)
            buf[i] = resolve(s[i], win, e.valid, bad);
        if (bad)
            atomicOr(&p.wr->bad, 1u);
        __syncthreads();
        uint64_t const at = e.byte_off + s0; // the segment's place in the wave's output
        {
            uint32_t const L = (nb + kByteThreads - 1) / kByteThreads, a = min(nb, tid * L), z = min(nb, a + L);
            uint32_t       r = 0;
            for (uint32_t i = a; i < z; ++i)
                r = (r >> 8) ^ tab[(r ^ buf[i]) & 0xff];
            if (z > a)
                atomicXor(&s_crc, mul_mod_p(x_pow_8n((uint32_t)(wave_len - (at + z))), r)); // (wave_len <= out_cap < 2^32)
        }
        uint8_t * const dst = p.out + at;
        if ((at & 3) == 0)
        {
            for (uint32_t i = tid; i < nb / 4; i += kByteThreads)
                reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<uint32_t const *>(buf)[i];
            for (uint32_t i = nb / 4 * 4 + tid; i < nb; i += kByteThreads)
                dst[i] = buf[i];
        }
        else
            for (uint32_t i = tid; i < nb; i += kByteThreads)
                dst[i] = buf[i];
        __syncthreads();
        if (tid == 0)
            atomicXor(&p.wr->crc, s_crc);
    }
}

hipError_t launch_find(WaveParams const & p, hipStream_t stream)
{
    if (p.nslots < 2)
        return hipSuccess;
    hipLaunchKernelGGL(find_kernel, dim3(p.nslots - 1), dim3(kFindThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_decode(WaveParams const & p, hipStream_t stream)
{
    if (p.nslots == 0)
        return hipSuccess;
    // (beyond 64 KB of LDS on request; set on the current device)
    hipError_t const attr =
      hipFuncSetAttribute(reinterpret_cast<void const *>(&decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDecodeLds);
    if (attr != hipSuccess)
        return attr;
    hipLaunchKernelGGL(decode_kernel, dim3(p.nslots), dim3(kDecodeThreads), kDecodeLds, stream, p);
    return hipGetLastError();
}

hipError_t launch_chain(ChainParams const & p, hipStream_t stream)
{
    if (p.nslots > kMaxWaveSlots)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_resolve(ResolveParams const & p, hipStream_t stream)
{
    if (p.nslots == 0)
        return hipSuccess;
    if (p.out_cap >> 32) // (bytes_kernel weighs a slice's CRC with a 32-bit distance to the wave's end)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_kernel, dim3(1), dim3(1024), 0, stream, p);
    hipError_t const e = hipGetLastError();
    if (e != hipSuccess || p.max_seg == 0)
        return e;
    hipLaunchKernelGGL(bytes_kernel, dim3(p.nslots, min(p.max_seg, kBytesAtATime)), dim3(kByteThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace pgunzip
} // namespace lx
