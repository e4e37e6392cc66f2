// lx_dust.h -- the nucleotide rule of the query masking (include/lambda_ext.h: lx_dust_params, lx_query_mask_create_dust): symmetric
// DUST (Morgulis et al. 2006), in integers, shared by the host function (lx_qmask_host.cpp) and the kernels (lx_dust.hip).  Not part
// of the ABI.  lx_qmask.h has what a mask stores (the distance bytes) and what the two rules share on the device.
//
// The rule works on alignment ranks: A, C, G, T = 0 .. 3; any other rank (N) is a break -- never masked, and in no interval.  A
// sequence is a set of maximal stretches of ranks 0 .. 3, each handled on its own:
//   * letter i of a stretch starts triplet t_i = 16 a_i + 4 a_{i+1} + a_{i+2} (64 kinds);
//   * an interval of l consecutive triplets covers l + 2 letters; with r = sum over kinds of c (c - 1) / 2, c the count of the kind
//     in the interval, it scores r / (l - 1) for l >= 2 and 0 for l = 1.  A score is the pair (r, l - 1) in one word, compared by
//     cross-multiplication: l <= 62 gives r <= 1891 and products under 2^17.  No floating point;
//   * an interval is perfect when 10 r > level (l - 1) and no sub-interval scores strictly higher (ties do not disqualify);
//   * a letter is masked exactly when it lies in a perfect interval of at most `window` letters (l <= window - 2).
// dustmasker's -linker (joining masked intervals one letter apart) is not built, and nothing here was compared with dustmasker or
// sdust byte for byte: the claim is the rule as stated.
//
// Both sides compute it as a sweep over lengths.  With S[i][l] the score of the interval of l triplets that starts at i,
//     M[i][l] = max(S[i][l], M[i][l - 1], M[i + 1][l - 1])          (the best score of any sub-interval)
// and (i, l) is perfect iff 10 r > level (l - 1) and S[i][l] >= max(M[i][l - 1], M[i + 1][l - 1]).  All starts advance together,
// length by length; a start needs its right neighbour's value of the step before; S grows by the count, so far, of the triplet that
// enters.  What a start keeps is its reach: the letters of its longest perfect interval (0 = none; the union of one start's perfect
// intervals is its longest).  Letter j is masked iff some start i <= j has i + reach[i] > j.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "lx_qmask.h"

namespace lx
{
namespace qmask
{

constexpr int kDustMinWindow = 4, kDustMaxWindow = 64, kDustMinLevel = 1, kDustMaxLevel = 1000;
constexpr int kDustKinds = 64;

// The sweep kernel's edges: one lane per start in workgroups of kDustBlock; a workgroup's starts need the window - 3 starts behind
// them (start i at length l reads start i + 1 at length l - 1, ..., start i + l - 1 at length 1), so it answers for
// dust_run(window) starts and sweeps the rest as a halo.
constexpr int kDustBlock = 256;
__host__ __device__ inline int dust_run(int window)
{
    return kDustBlock - (window - 3);
}

struct DustParams
{
    int32_t window, level;
};

__host__ __device__ inline bool dust_is_break(uint8_t rank)
{
    return rank > 3;
}
__host__ __device__ inline uint32_t dust_triplet(uint8_t a, uint8_t b, uint8_t c)
{
    return 16u * a + 4u * b + c;
}
// the score r / d, d = l - 1 >= 1 (the single triplet's 0 is 0 / 1)
__host__ __device__ inline uint32_t dust_pack(uint32_t r, uint32_t d)
{
    return r << 8 | d;
}
constexpr uint32_t kDustZero = 1; // dust_pack(0, 1)
__host__ __device__ inline uint32_t dust_r(uint32_t s)
{
    return s >> 8;
}
__host__ __device__ inline uint32_t dust_d(uint32_t s)
{
    return s & 255u;
}
// a >= b as fractions
__host__ __device__ inline bool dust_ge(uint32_t a, uint32_t b)
{
    return dust_r(a) * dust_d(b) >= dust_r(b) * dust_d(a);
}
__host__ __device__ inline uint32_t dust_max(uint32_t a, uint32_t b)
{
    return dust_ge(a, b) ? a : b;
}
// One step of a start: its interval reaches length l with the score s; mine / right are M[i][l - 1] and M[i + 1][l - 1].  Returns
// M[i][l]; `reach` becomes l + 2 where the interval is perfect.
__host__ __device__ inline uint32_t dust_step(uint32_t s, uint32_t mine, uint32_t right, int l, int level, uint32_t & reach)
{
    // (three comparisons that do not wait for one another)
    bool const     best = dust_ge(s, mine) && dust_ge(s, right);
    uint32_t const top  = dust_max(mine, right);
    if (best && 10u * dust_r(s) > (uint32_t)level * dust_d(s))
        reach = (uint32_t)l + 2u;
    return best ? s : top;
}

// ---- the rule for one sequence on the host: dist[0 .. L) from res[0 .. L), the same distance bytes as seg_mask_sequence's.  Returns
// the number of masked letters.  The host walks a stretch's starts from its last to its first and keeps, per length, the M of the
// start behind the current one: the same steps as the kernel's, start by start instead of length by length, so a start's counts
// and the two rows of M stay in the first-level cache.
struct DustWork
{
    std::vector<uint8_t> trip, reach; // per letter of the sequence
};
inline uint64_t dust_mask_sequence(uint8_t const * res, uint64_t L, DustParams const & p, uint8_t * dist, DustWork & w)
{
    uint64_t const Lmax = (uint64_t)p.window - 2;
    if (w.reach.size() < L)
        w.reach.resize(L), w.trip.resize(L);
    for (uint64_t j = 0; j < L; ++j)
        w.reach[j] = 0;
    uint32_t rows[2][kDustMaxWindow]; // M[start][l] of the start behind, and of this one
    for (uint64_t a = 0; a < L;)
    {
        if (dust_is_break(res[a]))
        {
            ++a;
            continue;
        }
        uint64_t b = a;
        while (b < L && !dust_is_break(res[b]))
            ++b;
        // the stretch [a, b): its b - a - 2 starts
        uint64_t const nT = b - a >= 3 ? b - a - 2 : 0;
        for (uint64_t i = 0; i < nT; ++i)
            w.trip[a + i] = (uint8_t)dust_triplet(res[a + i], res[a + i + 1], res[a + i + 2]);
        uint8_t const * const trip = w.trip.data() + a;
        for (uint64_t i = nT; i-- > 0;)
        {
            uint32_t * const       cur    = rows[i & 1];
            uint32_t const * const behind = rows[(i & 1) ^ 1];
            uint64_t const         lim    = nT - i < Lmax ? nT - i : Lmax;
            uint8_t                cnt[kDustKinds] = {0};
            cnt[trip[i]]          = 1;
            uint32_t M = kDustZero, r = 0, reach = 0;
            cur[1] = M;
            for (uint64_t l = 2; l <= lim; ++l)
            {
                r += cnt[trip[i + l - 1]]++;
                M      = dust_step(dust_pack(r, (uint32_t)l - 1u), M, behind[l - 1], (int)l, p.level, reach);
                cur[l] = M;
            }
            w.reach[a + i] = (uint8_t)reach;
        }
        a = b;
    }
    uint64_t masked = 0, until = 0, next = ~0ull;
    for (uint64_t j = 0; j < L; ++j)
    {
        if (w.reach[j] && j + w.reach[j] > until)
            until = j + w.reach[j];
        dist[j] = j < until ? 0 : (uint8_t)kSegFree;
        masked += j < until ? 1 : 0;
    }
    for (uint64_t j = L; j-- > 0;)
    {
        if (dist[j] == 0)
            next = j;
        dist[j] = next != ~0ull && next - j < (uint64_t)kSegLookAhead ? (uint8_t)(next - j) : (uint8_t)kSegFree;
    }
    return masked;
}

// ---- the kernels (lx_dust.hip), on QmaskDev's letters, stop bits, distance bytes and counters (lx_qmask.h).  The covered letters go
// to QmaskDev::F (word w at F[w + 1]), where the distance pass reads them.
struct DustDev
{
    int32_t    window, level;
    uint64_t * brk;   // nWords + 2 words, zero: the breaks, and every letter at or behind `extent`
    uint8_t *  reach; // nWords * 64 + 64 bytes, zero
};
hipError_t dust_launch(QmaskDev const & p, DustDev const & d, hipStream_t stream);

} // namespace qmask
} // namespace lx
