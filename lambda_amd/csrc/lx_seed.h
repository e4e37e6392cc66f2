// lx_seed.h -- what lx_seed.hip (the kernels of Level 3: word table and seeding) and lx_seed_host.cpp (lx_index_*, lx_seed_*)
// share.  Not part of the ABI; include/lambda_ext.h is.
#pragma once
#include <hip/hip_runtime.h>

#include "host/lx_seeding.hpp"

namespace lx
{

// One launch of seed_reads_kernel: the table, both sequence sets, the seeding parameters, the reads of the launch and where
// their matches go.
struct SeedDev
{
    lambda_amd::ReducedIndex::Entry const * entries;
    uint64_t const *                        pre;
    uint64_t                                pow[64];
    uint64_t                                base;
    int                                     preLen, keyLen, alph;
    uint8_t const *                         sRes; // subjects: alignment ranks, reduced letters
    uint8_t const *                         sRed;
    uint64_t const *                        sOff;
    uint64_t const *                        sLen;
    uint8_t const *                         qRes; // queries (frame-expanded)
    uint8_t const *                         qRed;
    uint64_t const *                        qOff;
    uint64_t const *                        qLen;
    uint64_t                                nQSeq;
    int                                     qNumFrames;
    int                                     unknownRank;
    int8_t const *                          matrix;
    int8_t const *                          matrixRev; // bisulfite: hits on odd subject frames (NULL otherwise)
    uint64_t                                maxMatches;
    int                                     halfExact, adaptive, preScoring;
    double                                  preScoringThresh;
    int                                     seedLength, seedOffset, maxSeedDist;
    uint64_t const *                        reads; // first frame sequence of every read of this launch
    uint64_t                                nReads;
    lx_match *                              out;
    unsigned long long *                    counters; // [0] matches written, [1] hitsAfterSeeding, [2] hitsFailedPreExtendTest, [3] buffer full
    uint64_t                                outCap;
    uint8_t *                               declined; // per read of this launch: 1 = seed it on the host
    uint8_t const *                         qMask;    // a query mask's distance bytes, indexed like qRes (NULL: no mask)
};

constexpr int      kMaxSecond   = 24;       // letters behind the exact part of a seed the depth-first walk holds
constexpr uint64_t kLaunchReads = 4u << 20; // reads of one launch at most (its match buffer holds 64 matches per read)

// one lane per read (blocks of 64); declined[0 .. nReads) and counters[0 .. 4) are zero before the launch
hipError_t seed_launch_reads(SeedDev const & p, hipStream_t stream);

// The word table: keys[e] / vals[e] = the word of keyLen letters (base alph + 1, the pad digit behind a sequence's end) at entry e and
// sequence << 32 | position, entries in (sequence, position) order -- first[s] = entry of sequence s's first position --; after the
// sort the entries interleaved, and pre[w] = first entry whose first preLen letters are >= the word w (nPre of them).
hipError_t seed_launch_table_keys(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                  int keyLen, uint64_t base, int alph, uint64_t * keys, uint64_t * vals, hipStream_t stream);
hipError_t seed_launch_table_entries(uint64_t const * keys, uint64_t const * vals, uint64_t total, lambda_amd::ReducedIndex::Entry * out, hipStream_t stream);
hipError_t seed_launch_table_prefix(uint64_t const * keys, uint64_t total, uint64_t preDiv, uint64_t nPre, uint64_t * pre, hipStream_t stream);

// The word table in slices of the key space (lx_seed_host.cpp: build_in_slices).  One workgroup of kTabBlock threads per kTabBlock
// positions; the 64-bit scan works on tiles of kTabScanTile values.
constexpr int kTabBlock = 256, kTabScanItems = 8, kTabScanTile = kTabBlock * kTabScanItems;
inline uint64_t tab_blocks(uint64_t total)
{
    return (total + kTabBlock - 1) / kTabBlock;
}
inline uint64_t tab_scan_tiles(uint64_t n)
{
    return (n + kTabScanTile - 1) / kTabScanTile;
}
// hist[w] += the positions whose first preLen letters are the word w (hist: nPre zeroed values; words are < nPre)
hipError_t seed_launch_table_counts(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                    int preLen, uint64_t base, int alph, uint64_t nPre, uint64_t * hist, hipStream_t stream);
// a[0 .. n) becomes its exclusive sum scan, in place; tile_tot: tab_scan_tiles(n) values of workspace
hipError_t seed_launch_scan64(uint64_t * a, uint64_t n, uint64_t * tile_tot, hipStream_t stream);
// block_cnt[b] = how many of positions [b * kTabBlock, (b + 1) * kTabBlock) have their first preLen letters in [wLo, wHi) (tab_blocks(total) values) ...
hipError_t seed_launch_table_slice_counts(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                          int preLen, uint64_t base, int alph, uint64_t wLo, uint64_t wHi, uint64_t * block_cnt, hipStream_t stream);
// ... and, block_before = their exclusive scan, those positions' keys / vals (as seed_launch_table_keys makes them) side by side in
// (sequence, position) order; cap = how many there are (nothing is written at or behind it)
hipError_t seed_launch_table_slice_keys(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                        int preLen, int keyLen, uint64_t base, int alph, uint64_t wLo, uint64_t wHi, uint64_t const * block_before, uint64_t cap,
                                        uint64_t * keys, uint64_t * vals, hipStream_t stream);

} // namespace lx
