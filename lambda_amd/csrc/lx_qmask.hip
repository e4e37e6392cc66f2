// lx_qmask.hip -- the kernels of the query masking (lx_qmask.h has the rule; gfx950 only).  Everything works on the letter buffer as
// it was uploaded, q_res[0 .. extent), and on words of 64 bits over it -- no kernel looks a letter's sequence up:
//   stops    one lane per sequence: the bit of its first letter; one workgroup per gap between sequences (the host lists them; a dense
//            set has none): the bits of its letters, word by word.  A window is inside one sequence exactly when none of its letters
//            but the first has its bit set, and so is a look-ahead.
//   flags    one lane per window (= per letter, the window that starts there), the letters of a workgroup's windows and the W - 1 behind
//            them staged in LDS; a wavefront's two ballots are the words A and B of its 64 windows.  Reads cost what long sequences
//            cost: a workgroup takes 256 letters wherever the sequences' borders are.
//   tile ops one lane per word, kTileWords words per workgroup: the word's two operations on the carry (lx_qmask.h), combined over the
//            wavefront with two ballots (the last lane that does not keep the carry decides) and over the workgroup in LDS.
//   carries  one wavefront over the tiles' operations, upwards and downwards: the carry that arrives at every tile.
//   fill     the tile ops again, now with the carry that arrives: every word's windows whose run holds a trigger (F).
//   dist     one lane per letter: the letters F's windows cover (F and the word in front of it, shifted W - 1 times), then the first
//            covered letter among this one and the 63 behind it that no stop bit separates from it.  Counts the masked letters.
//            (A second instantiation reads covered letters that another rule left in F: lx_dust.hip.)
//   touched  one lane per sequence hops along its distance bytes to the first 0: the sequences with a masked letter.
// Integer work only; the tables come from the host (lx_seg_tables).
#include "lx_qmask.h"

namespace lx
{
namespace qmask
{
namespace
{

__global__ __launch_bounds__(256) void stops_kernel(QmaskDev p)
{
    uint64_t const s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.nSeq || p.qLen[s] == 0)
        return;
    uint64_t const at = p.qOff[s];
    if (at < p.extent)
        atomicOr(p.stop + (at >> 6), 1ull << (at & 63));
}

// gap k = the letters [gaps[2 k], gaps[2 k + 1]) of no sequence: their stop bits, a word per lane and step
__global__ __launch_bounds__(256) void gaps_kernel(QmaskDev p)
{
    uint64_t const from = p.gaps[2 * (uint64_t)blockIdx.x], to = p.gaps[2 * (uint64_t)blockIdx.x + 1] < p.extent ? p.gaps[2 * (uint64_t)blockIdx.x + 1] : p.extent;
    if (from >= to)
        return;
    for (uint64_t w = (from >> 6) + threadIdx.x; w <= ((to - 1) >> 6); w += 256)
    {
        uint64_t const lo = w * 64 < from ? from - w * 64 : 0, hi = to - w * 64 < 64 ? to - w * 64 : 64; // bits [lo, hi) of word w
        uint64_t const bits = (hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
        atomicOr(p.stop + w, (unsigned long long)bits);
    }
}

// bits [g, g + 64) of a bit array whose words w and w + 1 are lo and hi (g & 63 = sh)
__device__ __forceinline__ uint64_t bits_from(uint64_t lo, uint64_t hi, int sh)
{
    return sh == 0 ? lo : (lo >> sh) | (hi << (64 - sh));
}

__global__ __launch_bounds__(kFlagBlock) void flags_kernel(QmaskDev p)
{
    __shared__ uint8_t  letters[kFlagBlock + kSegMaxWindow];
    __shared__ uint32_t T[65];
    uint64_t const      g0 = (uint64_t)blockIdx.x * kFlagBlock, g = g0 + threadIdx.x;
    for (int i = threadIdx.x; i < kFlagBlock + p.W - 1; i += kFlagBlock)
        letters[i] = g0 + (uint64_t)i < p.extent ? p.qRes[g0 + (uint64_t)i] : (uint8_t)0;
    if (threadIdx.x < 65)
        T[threadIdx.x] = p.T[threadIdx.x];
    __syncthreads();
    bool a = false, b = false;
    if (g + (uint64_t)p.W <= p.extent)
    {
        uint64_t const first = g + 1; // no stop bit on letters g + 1 .. g + W - 1
        uint64_t const stops = bits_from(p.stop[first >> 6], p.stop[(first >> 6) + 1], (int)(first & 63));
        if ((stops & ((1ull << (p.W - 1)) - 1ull)) == 0)
        {
            uint32_t const S = seg_window_score(letters + threadIdx.x, p.W, T);
            a                = S >= p.thr2;
            b                = a && S >= p.thr1;
        }
    }
    uint64_t const wa = __ballot(a), wb = __ballot(b);
    uint64_t const w  = g >> 6;
    if ((threadIdx.x & 63) == 0 && w < p.nWords)
    {
        p.A[w] = wa;
        p.B[w] = wb;
    }
}

// The carry that arrives at this lane's word, from the operations of the words in front of it (UP: the lower ones, else the higher
// ones) in the workgroup and `arrives`, the carry at the workgroup's edge; `tile_op`: the workgroup's operation as a whole.
template <bool UP>
__device__ __forceinline__ uint32_t carry_at(uint32_t op, uint32_t arrives, uint32_t * wave_op, uint32_t & tile_op)
{
    int const      lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    uint64_t const acts = __ballot(op != kSegKeep), sets = __ballot(op == kSegSet);
    // the last lane in front of this one that acts decides
    uint64_t const front = UP ? acts & ((1ull << lane) - 1ull) : (lane == 63 ? 0ull : acts & ~((2ull << lane) - 1ull));
    int const      who   = front ? (UP ? 63 - seg_clz(front) : seg_ctz(front)) : -1;
    if (lane == 0)
        wave_op[wave] = acts == 0 ? (uint32_t)kSegKeep : ((sets >> (UP ? 63 - seg_clz(acts) : seg_ctz(acts))) & 1ull) ? (uint32_t)kSegSet : (uint32_t)kSegClear;
    __syncthreads();
    uint32_t carry = arrives, all = kSegKeep;
    for (int k = 0; k < waves; ++k)
    {
        int const      v = UP ? k : waves - 1 - k;
        uint32_t const o = wave_op[v];
        if (UP ? v < wave : v > wave)
            carry = seg_apply(o, carry);
        all = seg_combine(all, o);
    }
    tile_op = all;
    __syncthreads();
    return who >= 0 ? (uint32_t)((sets >> who) & 1ull) : carry;
}

__global__ __launch_bounds__(kTileWords) void tile_ops_kernel(QmaskDev p)
{
    __shared__ uint32_t wave_op[kTileWords / 64];
    uint64_t const      w = (uint64_t)blockIdx.x * kTileWords + threadIdx.x;
    uint64_t const      A = w < p.nWords ? p.A[w] : 0ull, B = w < p.nWords ? p.B[w] : 0ull;
    uint32_t            up, down;
    (void)carry_at<true>(seg_word_op_up(A, B), 0u, wave_op, up);
    (void)carry_at<false>(seg_word_op_down(A, B), 0u, wave_op, down);
    if (threadIdx.x == 0)
    {
        p.opUp[blockIdx.x]   = (uint8_t)up;
        p.opDown[blockIdx.x] = (uint8_t)down;
    }
}

// one wavefront: ops[t] becomes the carry that arrives at tile t
__global__ __launch_bounds__(64) void carries_kernel(QmaskDev p)
{
    __shared__ uint32_t wave_op[1];
    uint32_t            carry = 0, all;
    for (uint64_t t0 = 0; t0 < p.nTiles; t0 += 64)
    {
        uint64_t const t  = t0 + threadIdx.x;
        uint32_t const at = carry_at<true>(t < p.nTiles ? (uint32_t)p.opUp[t] : (uint32_t)kSegKeep, carry, wave_op, all);
        if (t < p.nTiles)
            p.opUp[t] = (uint8_t)at;
        carry = seg_apply(all, carry);
    }
    carry = 0;
    for (uint64_t t1 = (p.nTiles + 63) / 64 * 64; t1 > 0; t1 -= 64)
    {
        uint64_t const t  = t1 - 64 + threadIdx.x;
        uint32_t const at = carry_at<false>(t < p.nTiles ? (uint32_t)p.opDown[t] : (uint32_t)kSegKeep, carry, wave_op, all);
        if (t < p.nTiles)
            p.opDown[t] = (uint8_t)at;
        carry = seg_apply(all, carry);
    }
}

__global__ __launch_bounds__(kTileWords) void fill_kernel(QmaskDev p)
{
    __shared__ uint32_t wave_op[kTileWords / 64];
    uint64_t const      w = (uint64_t)blockIdx.x * kTileWords + threadIdx.x;
    uint64_t const      A = w < p.nWords ? p.A[w] : 0ull, B = w < p.nWords ? p.B[w] : 0ull;
    uint32_t            all;
    uint32_t const      up   = carry_at<true>(seg_word_op_up(A, B), (uint32_t)p.opUp[blockIdx.x], wave_op, all);
    uint32_t const      down = carry_at<false>(seg_word_op_down(A, B), (uint32_t)p.opDown[blockIdx.x], wave_op, all);
    if (w < p.nWords)
        p.F[w + 1] = seg_word_fill(A, B, up, down);
}

// COVERED: F holds the covered letters themselves (word w at F[w + 1]), not the windows that cover them
template <bool COVERED>
__global__ __launch_bounds__(kFlagBlock) void dist_kernel(QmaskDev p)
{
    uint64_t const g = (uint64_t)blockIdx.x * kFlagBlock + threadIdx.x, w = g >> 6; // (w is the wavefront's)
    if (w >= p.nWords)
        return;
    int const      lane = threadIdx.x & 63;
    uint64_t const f0 = p.F[w], f1 = p.F[w + 1], f2 = p.F[w + 2]; // the words w - 1, w, w + 1
    uint64_t const m1 = COVERED ? f1 : seg_cover(f0, f1, p.W), m2 = COVERED ? f2 : seg_cover(f1, f2, p.W);
    if (lane == 0 && m1 != 0)
        atomicAdd(p.count, (unsigned long long)__popcll((unsigned long long)m1));
    if (g >= p.extent)
        return;
    uint64_t const covered = bits_from(m1, m2, lane);                                                  // letters g .. g + 63
    uint64_t const stops   = bits_from(p.stop[(g + 1) >> 6], p.stop[((g + 1) >> 6) + 1], (int)((g + 1) & 63)); // letters g + 1 .. g + 64
    int const      d = covered ? seg_ctz(covered) : 64, room = stops ? seg_ctz(stops) : 64;            // (d <= room: no border in between)
    p.dist[g]        = d < kSegLookAhead && d <= room ? (uint8_t)d : (uint8_t)kSegFree;
}

__global__ __launch_bounds__(256) void touched_kernel(QmaskDev p)
{
    uint64_t const s   = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool           hit = false;
    if (s < p.nSeq)
    {
        uint8_t const * const d = p.dist + p.qOff[s];
        uint64_t const        L = p.qLen[s];
        for (uint64_t j = 0; j < L && !hit;)
        {
            uint32_t const x = d[j];
            hit              = x == 0;
            j += x == (uint32_t)kSegFree ? (uint64_t)kSegLookAhead : (uint64_t)x;
        }
    }
    uint64_t const hits = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && hits != 0)
        atomicAdd(p.count + 1, (unsigned long long)__popcll((unsigned long long)hits));
}

} // namespace

hipError_t qmask_launch(QmaskDev const & p, hipStream_t stream)
{
    if (p.extent == 0 || p.nSeq == 0)
        return hipSuccess;
    unsigned const seqBlocks = (unsigned)((p.nSeq + 255) / 256), letterBlocks = (unsigned)((p.nWords * 64 + kFlagBlock - 1) / kFlagBlock);
    hipLaunchKernelGGL(stops_kernel, dim3(seqBlocks), dim3(256), 0, stream, p);
    if (p.nGaps)
        hipLaunchKernelGGL(gaps_kernel, dim3((unsigned)p.nGaps), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(flags_kernel, dim3(letterBlocks), dim3(kFlagBlock), 0, stream, p);
    hipLaunchKernelGGL(tile_ops_kernel, dim3((unsigned)p.nTiles), dim3(kTileWords), 0, stream, p);
    hipLaunchKernelGGL(carries_kernel, dim3(1), dim3(64), 0, stream, p);
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)p.nTiles), dim3(kTileWords), 0, stream, p);
    hipLaunchKernelGGL(dist_kernel<false>, dim3(letterBlocks), dim3(kFlagBlock), 0, stream, p);
    hipLaunchKernelGGL(touched_kernel, dim3(seqBlocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t qmask_launch_stops(QmaskDev const & p, hipStream_t stream)
{
    hipLaunchKernelGGL(stops_kernel, dim3((unsigned)((p.nSeq + 255) / 256)), dim3(256), 0, stream, p);
    if (p.nGaps)
        hipLaunchKernelGGL(gaps_kernel, dim3((unsigned)p.nGaps), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t qmask_launch_covered(QmaskDev const & p, hipStream_t stream)
{
    unsigned const seqBlocks = (unsigned)((p.nSeq + 255) / 256), letterBlocks = (unsigned)((p.nWords * 64 + kFlagBlock - 1) / kFlagBlock);
    hipLaunchKernelGGL(dist_kernel<true>, dim3(letterBlocks), dim3(kFlagBlock), 0, stream, p);
    hipLaunchKernelGGL(touched_kernel, dim3(seqBlocks), dim3(256), 0, stream, p);
    return hipGetLastError();
}

} // namespace qmask
} // namespace lx
