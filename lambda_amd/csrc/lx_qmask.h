// lx_qmask.h -- low-complexity masking of the queries before seeding (include/lambda_ext.h: lx_seg_*, lx_query_mask_*): the rule,
// shared by the host function (lx_qmask_host.cpp) and the kernels (lx_qmask.hip), and what those two files share.  Not part of the ABI.
//
// The rule is SEG's first two stages (Wootton & Federhen 1993) on alignment ranks, in integers:
//   * a window of W letters scores S = sum over ranks r of T[count of r in the window], T[c] = round(c * log2 c * 65536); its
//     entropy is <= k bits exactly when S >= thr(k) = ceil(W * (log2 W - k) * 65536).  Every rank is a letter, 'X' and '*' too.
//   * a run is a maximal stretch of consecutive windows with S >= thr2; a run that holds a window with S >= thr1 masks every
//     letter from its first window's first letter to its last window's last one.  Windows never reach across a sequence's end; a
//     sequence shorter than W is never masked.
// SEG's third stage, which trims each raw segment to its least probable part, is NOT applied: a mask is SEG's segment or wider (an
// SP repeat between ordinary flanks takes a few flank letters on either side along).  This is not
// NCBI's segmasker.
//
// Runs are resolved on bit words: window p of a sequence is bit p & 63 of word p >> 6 of two words, A (S >= thr2) and B (S >= thr1,
// a subset of A).  "The run this window belongs to holds a trigger" travels over word borders as one of three operations on a
// carry bit -- keep it, clear it, set it --, which compose associatively (seg_combine): the host walks the words of a sequence, the
// kernels scan them over the whole letter buffer at once.
//
// What a mask stores is one byte per letter, indexed like the letters: the distance from the letter to the next masked letter at or
// behind it in its sequence, 255 where there is none within kSegLookAhead letters.  0 = the letter is masked; "a seed of n <= 63 letters
// that starts here covers a masked letter" is dist < n.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lx
{
namespace qmask
{

constexpr int kSegMinWindow = 4, kSegMaxWindow = 64;
constexpr int kSegLookAhead = 64; // a distance byte looks at this letter and the 63 behind it
constexpr int kSegFree      = 255;

// The kernels' edges: one lane per window in workgroups of kFlagBlock, a wavefront's ballot = one word of 64 windows; the carry
// scan takes kTileWords words per workgroup: kQmaskTile letters.
constexpr int kFlagBlock = 256, kTileWords = 256, kQmaskTile = kTileWords * 64;

struct SegTables
{
    int32_t  W;
    uint32_t T[65];
    uint32_t thr1, thr2; // (W * log2 W * 65536 <= 64 * 6 * 65536: 32 bits hold every score)
};

// S of the window w[0 .. W): each letter at its first occurrence adds T[how often it occurs]
__host__ __device__ inline uint32_t seg_window_score(uint8_t const * w, int W, uint32_t const * T)
{
    uint32_t S = 0;
    for (int i = 0; i < W; ++i)
    {
        uint8_t const c     = w[i];
        bool          first = true;
        for (int j = 0; j < i; ++j)
            first = first && w[j] != c;
        if (!first)
            continue;
        int n = 1;
        for (int j = i + 1; j < W; ++j)
            n += w[j] == c ? 1 : 0;
        S += T[n];
    }
    return S;
}

// what a stretch of windows does to the carry "the run that arrives holds a trigger"
enum : uint32_t
{
    kSegKeep  = 0, // all of it continues the run, without a trigger
    kSegClear = 1, // the run that leaves is another one, without a trigger so far
    kSegSet   = 2  // the run that leaves holds a trigger
};
// first a, then b
__host__ __device__ inline uint32_t seg_combine(uint32_t a, uint32_t b)
{
    return b == kSegKeep ? a : b;
}
__host__ __device__ inline uint32_t seg_apply(uint32_t op, uint32_t carry)
{
    return op == kSegKeep ? carry : op == kSegSet ? 1u : 0u;
}
__host__ __device__ inline int seg_clz(uint64_t x) // x != 0
{
    return __builtin_clzll((unsigned long long)x);
}
__host__ __device__ inline int seg_ctz(uint64_t x) // x != 0
{
    return __builtin_ctzll((unsigned long long)x);
}
// a word of 64 windows, walked towards higher windows: the run that leaves at bit 63 ...
__host__ __device__ inline uint32_t seg_word_op_up(uint64_t A, uint64_t B)
{
    if (A == ~0ull)
        return B ? kSegSet : kSegKeep;
    int const ones = seg_clz(~A); // the run at the top
    return ones != 0 && (B >> (64 - ones)) != 0 ? kSegSet : kSegClear;
}
// ... and towards lower windows: the run that leaves at bit 0
__host__ __device__ inline uint32_t seg_word_op_down(uint64_t A, uint64_t B)
{
    if (A == ~0ull)
        return B ? kSegSet : kSegKeep;
    int const ones = seg_ctz(~A);
    return ones != 0 && (B << (64 - ones)) != 0 ? kSegSet : kSegClear;
}
// the windows of the word whose run holds a trigger; up / down: the carry that arrives at bit 0 / at bit 63
__host__ __device__ inline uint64_t seg_word_fill(uint64_t A, uint64_t B, uint32_t up, uint32_t down)
{
    uint64_t const seeds = (B | (up ? 1ull : 0ull) | (down ? 1ull << 63 : 0ull)) & A;
    uint64_t       g = seeds, p = A; // towards higher bits
    for (int s = 1; s < 64; s <<= 1)
    {
        g |= p & (g << s);
        p &= p << s;
    }
    uint64_t d = seeds;
    p          = A; // towards lower bits
    for (int s = 1; s < 64; s <<= 1)
    {
        d |= p & (d >> s);
        p &= p >> s;
    }
    return g | d;
}
// the high word of (hi : lo) OR-ed with its shifts by 1 .. W - 1 towards higher bits: the letters the windows in hi : lo cover
__host__ __device__ inline uint64_t seg_cover(uint64_t lo, uint64_t hi, int W)
{
    for (int done = 1; done < W;)
    {
        int const sh = done < W - done ? done : W - done; // 1 .. 32
        hi |= (hi << sh) | (lo >> (64 - sh));
        lo |= lo << sh;
        done += sh;
    }
    return hi;
}

// ---- the rule for one sequence on the host: dist[0 .. L) from res[0 .. L).  A, B, F: (L + 63) / 64 words of workspace each.
// Returns the number of masked letters.  (S slides: the letter that leaves and the one that enters move two terms of the sum.)
inline uint64_t seg_mask_sequence(uint8_t const * res, uint64_t L, SegTables const & t, uint8_t * dist, uint64_t * A, uint64_t * B, uint64_t * F)
{
    for (uint64_t j = 0; j < L; ++j)
        dist[j] = (uint8_t)kSegFree;
    uint64_t const W = (uint64_t)t.W;
    if (L < W)
        return 0;
    uint64_t const nWin = L - W + 1, nW = (nWin + 63) / 64;
    for (uint64_t w = 0; w < nW; ++w)
        A[w] = B[w] = 0;
    int     cnt[256] = {0};
    int64_t S        = (int64_t)seg_window_score(res, t.W, t.T);
    for (uint64_t j = 0; j < W; ++j)
        ++cnt[res[j]];
    for (uint64_t p = 0;; ++p)
    {
        if ((uint64_t)S >= t.thr2)
            A[p >> 6] |= 1ull << (p & 63);
        if ((uint64_t)S >= t.thr1 && (uint64_t)S >= t.thr2)
            B[p >> 6] |= 1ull << (p & 63);
        if (p + 1 == nWin)
            break;
        int & out = cnt[res[p]];
        S -= (int64_t)t.T[out] - (int64_t)t.T[out - 1];
        --out;
        int & in = cnt[res[p + W]];
        S += (int64_t)t.T[in + 1] - (int64_t)t.T[in];
        ++in;
    }
    uint32_t carry = 0; // upwards: what arrives at every word's bit 0
    for (uint64_t w = 0; w < nW; ++w)
    {
        F[w]  = carry;
        carry = seg_apply(seg_word_op_up(A[w], B[w]), carry);
    }
    carry = 0;
    for (uint64_t w = nW; w-- > 0;)
    {
        uint32_t const down = carry;
        carry               = seg_apply(seg_word_op_down(A[w], B[w]), carry);
        F[w]                = seg_word_fill(A[w], B[w], (uint32_t)F[w], down);
    }
    uint64_t masked = 0, until = 0; // letters below `until` are done
    for (uint64_t w = 0; w < nW; ++w)
        for (uint64_t rest = F[w]; rest; rest &= rest - 1)
        {
            uint64_t const p = w * 64 + (uint64_t)seg_ctz(rest);
            for (uint64_t j = p > until ? p : until; j < p + W; ++j)
                dist[j] = 0, ++masked;
            until = p + W;
        }
    uint64_t next = ~0ull;
    for (uint64_t j = L; j-- > 0;)
    {
        if (dist[j] == 0)
            next = j;
        dist[j] = next != ~0ull && next - j < (uint64_t)kSegLookAhead ? (uint8_t)(next - j) : (uint8_t)kSegFree;
    }
    return masked;
}

// distance bytes from given 0 / 1 bytes (lx_query_mask_create); returns the number of masked letters
inline uint64_t dist_from_bytes(uint8_t const * masked, uint64_t L, uint8_t * dist)
{
    uint64_t next = ~0ull, n = 0;
    for (uint64_t j = L; j-- > 0;)
    {
        if (masked[j])
            next = j, ++n;
        dist[j] = next != ~0ull && next - j < (uint64_t)kSegLookAhead ? (uint8_t)(next - j) : (uint8_t)kSegFree;
    }
    return n;
}

// ---- the kernels (lx_qmask.hip).  The letters are q_res[0 .. extent); sequence s lies at off[s] .. off[s] + len[s], the sequences
// with letters in ascending order without overlap (gaps between them belong to no sequence).  Bit words cover the letter buffer:
// nWords = (extent + 63) / 64.
struct QmaskDev
{
    uint8_t const *      qRes;
    uint64_t const *     qOff;
    uint64_t const *     qLen;
    uint64_t             nSeq, extent, nWords, nTiles;
    uint64_t const *     gaps;  // nGaps pairs [from, to): the letters in front of and between the sequences that belong to none
    uint64_t             nGaps;
    int32_t              W;
    uint32_t             thr1, thr2;
    uint32_t const *     T;     // 65 values
    unsigned long long * stop;  // nWords + 2 words, zero: a window or a look-ahead may not step onto a letter whose bit is set
    uint64_t *           A;     // nWords
    uint64_t *           B;     // nWords
    uint64_t *           F;     // nWords + 2, F[0] and F[nWords + 1] zero: word w's windows with a trigger in their run at F[w + 1]
    uint8_t *            opUp;  // per tile of kTileWords words: its operation; then the carry that arrives at it
    uint8_t *            opDown;
    uint8_t *            dist;  // extent bytes
    unsigned long long * count; // [0] masked letters, [1] sequences with a masked letter; zero
};
hipError_t qmask_launch(QmaskDev const & p, hipStream_t stream);
// the first and the last two passes alone, for a rule that writes the covered letters itself (lx_dust.hip): the stop bits; the distance
// bytes and the two counters from F[w + 1] = the covered letters of word w
hipError_t qmask_launch_stops(QmaskDev const & p, hipStream_t stream);
hipError_t qmask_launch_covered(QmaskDev const & p, hipStream_t stream);

} // namespace qmask
} // namespace lx
