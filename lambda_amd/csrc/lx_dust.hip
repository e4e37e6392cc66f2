// lx_dust.hip -- the kernels of the nucleotide query masking, symmetric DUST (lx_dust.h has the rule; gfx950 only).  Like lx_qmask.hip
// they work on the letter buffer as it was uploaded and on words of 64 bits over it, and look no letter's sequence up; the stop bits
// (stops_kernel, gaps_kernel), the distance pass and the sequence count are lx_qmask.hip's.
//   breaks   one lane per letter, a wavefront's ballot = one word: the letters that are no A, C, G, T, and everything at or behind the
//            buffer's end.  A start's room is the letters from it up to the next break or stop bit, at most the window.
//   sweep    the hot path.  One lane per start letter, kDustBlock lanes per workgroup: it answers for the first dust_run(window) of
//            them and sweeps the window - 3 behind them as a halo (at window 64: 195 of 256, 1.31 lane steps per letter and length).
//            All lanes advance one length per step, 2 .. window - 2 triplets.  A lane keeps (r, l - 1) and M, the best score of any
//            sub-interval, in registers, and its 64 triplet counts as bytes in LDS: 16 KiB per workgroup, the byte of kind k of lane t
//            in dword (k / 4) * kDustBlock + t, so the lanes of a wavefront read and write 64 consecutive dwords whatever their kinds
//            are -- no two lanes of a half wavefront on one bank.  The right neighbour's M of the step before comes by a lane shift;
//            lane 63 takes it from the next wavefront's lane 0 through LDS, two slots in turn, one barrier per step.  A lane stops at
//            its room's end (a halo lane also where the workgroup's letters end); the workgroup stops with its last lane.  The result
//            is one byte per start: the letters of its longest perfect interval (0, or 7 .. 64 at the defaults).
//   cover    one lane per letter: letter j is covered iff some start i <= j has i + reach[i] > j; as reach <= 64 only the word in front
//            counts, so a wavefront takes that word's largest end and a prefix maximum over its own.  Ballot = the covered word, written
//            where the distance pass (lx_qmask.hip, its second instantiation) reads it.
// Integer work only; no host round trip between the kernels.
#include "lx_dust.h"

namespace lx
{
namespace qmask
{
namespace
{

// bits [g, g + 64) of a bit array whose words w and w + 1 are lo and hi (g & 63 = sh)
__device__ __forceinline__ uint64_t bits_at(uint64_t lo, uint64_t hi, int sh)
{
    return sh == 0 ? lo : (lo >> sh) | (hi << (64 - sh));
}

__global__ __launch_bounds__(256) void breaks_kernel(QmaskDev p, DustDev d)
{
    uint64_t const g = (uint64_t)blockIdx.x * 256 + threadIdx.x, w = g >> 6; // (w is the wavefront's)
    if (w > p.nWords)
        return;
    bool const     brk  = g >= p.extent || dust_is_break(p.qRes[g]);
    uint64_t const bits = __ballot(brk);
    if ((threadIdx.x & 63) == 0)
        d.brk[w] = bits;
}

__global__ __launch_bounds__(kDustBlock) void sweep_kernel(QmaskDev p, DustDev d)
{
    constexpr int       kWaves = kDustBlock / 64;
    __shared__ uint32_t cnt[kDustKinds / 4 * kDustBlock];
    __shared__ uint8_t  trip[kDustBlock];
    __shared__ uint32_t edge[2][kWaves + 1];
    __shared__ int      last;
    int const           t = threadIdx.x, lane = t & 63, wave = t >> 6, run = dust_run(d.window);
    uint64_t const      g = (uint64_t)blockIdx.x * (uint64_t)run + (uint64_t)t;
    if (t == 0)
    {
        last              = 0;
        edge[0][kWaves] = edge[1][kWaves] = kDustZero; // (the last lane never steps)
    }
    int      lim  = 0; // the triplets of this lane's longest interval
    uint32_t kind = 0;
    if (g < p.extent)
    {
        uint64_t const h     = g + 1;
        uint64_t const brk   = bits_at(d.brk[g >> 6], d.brk[(g >> 6) + 1], (int)(g & 63));              // letters g .. g + 63
        uint64_t const stops = bits_at(p.stop[h >> 6], p.stop[(h >> 6) + 1], (int)(h & 63));            // letters g + 1 .. g + 64
        uint64_t const bad   = brk | (stops << 1);
        int const      room  = bad ? (seg_ctz(bad) < d.window ? seg_ctz(bad) : d.window) : d.window;
        if (room >= 3)
        {
            kind = dust_triplet(p.qRes[g], p.qRes[g + 1], p.qRes[g + 2]);
            lim  = room - 2 < kDustBlock - t ? room - 2 : kDustBlock - t; // (lane t reads the triplets t .. t + lim - 1 of the workgroup)
        }
    }
    trip[t] = (uint8_t)kind;
    for (int k = 0; k < kDustKinds / 4; ++k)
        cnt[k * kDustBlock + t] = 0;
    uint8_t * const mine = reinterpret_cast<uint8_t *>(cnt + t); // the count of kind k: mine[(k >> 2) * kDustBlock * 4 + (k & 3)]
    mine[(kind >> 2) * (kDustBlock * 4) + (kind & 3u)] = 1;
    __syncthreads();
    if (lim >= 2)
        atomicMax(&last, lim);
    __syncthreads();
    int const steps = last;
    uint32_t  M = kDustZero, r = 0, reach = 0;
    for (int l = 2; l <= steps; ++l)
    {
        if (lane == 0)
            edge[l & 1][wave] = M;
        uint32_t right = (uint32_t)__shfl_down((int)M, 1);
        __syncthreads();
        if (lane == 63)
            right = edge[l & 1][wave + 1];
        if (l <= lim)
        {
            uint32_t const  k = trip[t + l - 1];
            uint8_t * const c = mine + (k >> 2) * (kDustBlock * 4) + (k & 3u);
            uint32_t const  n = *c;
            *c                = (uint8_t)(n + 1u);
            r += n;
            M = dust_step(dust_pack(r, (uint32_t)l - 1u), M, right, l, d.level, reach);
        }
    }
    if (t < run && g < p.extent)
        d.reach[g] = (uint8_t)reach;
}

__global__ __launch_bounds__(256) void cover_kernel(QmaskDev p, DustDev d)
{
    uint64_t const g = (uint64_t)blockIdx.x * 256 + threadIdx.x, w = g >> 6; // (w is the wavefront's)
    if (w >= p.nWords)
        return;
    int const lane = threadIdx.x & 63;
    // ends relative to this word's first letter: the word in front of it, then its own
    int front = g >= 64 ? lane - 64 + (int)d.reach[g - 64] : -64;
    int end   = lane + (int)d.reach[g];
    for (int s = 32; s > 0; s >>= 1)
    {
        int const o = __shfl_xor(front, s);
        front       = o > front ? o : front;
    }
    for (int s = 1; s < 64; s <<= 1)
    {
        int const o = __shfl_up(end, s);
        if (lane >= s && o > end)
            end = o;
    }
    uint64_t const covered = __ballot((front > end ? front : end) > lane);
    if (lane == 0)
        p.F[w + 1] = covered;
}

} // namespace

hipError_t dust_launch(QmaskDev const & p, DustDev const & d, hipStream_t stream)
{
    if (p.extent == 0 || p.nSeq == 0)
        return hipSuccess;
    unsigned const letterBlocks = (unsigned)((p.nWords * 64 + 255) / 256), run = (unsigned)dust_run(d.window);
    hipError_t     e            = qmask_launch_stops(p, stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(breaks_kernel, dim3((unsigned)(((p.nWords + 1) * 64 + 255) / 256)), dim3(256), 0, stream, p, d);
    hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)((p.extent + run - 1) / run)), dim3(kDustBlock), 0, stream, p, d);
    hipLaunchKernelGGL(cover_kernel, dim3(letterBlocks), dim3(256), 0, stream, p, d);
    e = hipGetLastError();
    return e != hipSuccess ? e : qmask_launch_covered(p, stream);
}

} // namespace qmask
} // namespace lx
