// lx_seed.hip -- the kernels of Level 3 (include/lambda_ext.h): the seeding stage on the GPU and the word table it reads (gfx950 only).
//
// Same semantics as host/lx_seeding.hpp's seedQueries -- search() of the reference, src/search_algo.hpp:611-762:
// seeds every seedOffset letters of the reduced query, exact or half-exact search (:505-604), adaptive elongation (:679-727), the
// over-abundance cut (:729), seedLooksPromising per located hit (:426-481) -- over the same sorted word table.  What is serial
// there is serial here: the hits a read has collected so far steer the elongation of its next seeds, so ONE LANE owns a read and
// walks its frames, seeds, cursors and hits in the host's order; reads are independent, so a launch is one lane per read.  A
// lane's time is a chain of dependent table probes (the prefix table for a word's first letters, binary searches inside the
// range after that); what hides their latency is the other reads -- 100 000 reads are 1 563 wavefronts.
//   * The half-exact search is the host's level-by-level expansion walked depth first: the host's list of cursors after the
//     last level is in lexicographic order of the words (children are appended in letter order), which is the order a
//     depth-first walk with ascending letters reaches them -- same cursors, same order, so the same hitsThisSeq at every step.
//   * Beyond the table's key length a cursor keeps the entries of its range that still match as a bit mask (the host keeps a
//     list); a range of more than 32 entries at that point, or a seed longer than kMaxSecond letters behind its exact part,
//     sends the READ to the host (flag per read; lx_seed_queries seeds those reads with seedQueries on the library's host
//     threads) -- results are identical by construction, the device only declines.
//   * Matches leave through one atomic counter (a full buffer is reported; the reads of that launch then go to the host).
//     Their order is the lanes', not the host's: iterateMatches sorts its span first (src/search_algo.hpp:1141), so the order of
//     the list carries no meaning.
#include "lx_seed.h"

namespace lx
{

using lambda_amd::ReducedIndex;

struct DevCursor
{
    uint32_t lo, hi;
    uint32_t mask; // beyond the key length: which entries of [lo, hi) still match (bit e = entry lo + e)
    int      len;
    uint64_t prefix;
};

__device__ __forceinline__ uint32_t dev_count(DevCursor const & c, int keyLen)
{
    return c.len > keyLen ? (uint32_t)__popc(c.mask) : c.hi - c.lo;
}

// the cursor of word + c (ReducedIndex::extendRight); ok = false: the device declines (too many entries beyond the keys)
__device__ __forceinline__ DevCursor dev_extend(SeedDev const & p, DevCursor const & cu, uint32_t c, bool & ok)
{
    DevCursor n = cu;
    n.len       = cu.len + 1;
    if (cu.len >= p.keyLen)
    {
        uint32_t m = cu.len == p.keyLen ? (cu.hi - cu.lo >= 32 ? 0xffffffffu : ((1u << (cu.hi - cu.lo)) - 1u)) : cu.mask;
        if (cu.len == p.keyLen && cu.hi - cu.lo > 32)
        {
            ok = false;
            return n;
        }
        uint32_t keep = 0;
        for (uint32_t rest = m; rest != 0; rest &= rest - 1)
        {
            int const                   e = __ffs((int)rest) - 1;
            ReducedIndex::Entry const & x = p.entries[cu.lo + (uint32_t)e];
            if ((uint64_t)x.pos + (uint64_t)cu.len < p.sLen[x.seq] && p.sRed[p.sOff[x.seq] + x.pos + (uint64_t)cu.len] == c)
                keep |= 1u << e;
        }
        n.mask = keep;
        return n;
    }
    n.prefix = cu.prefix * p.base + c;
    if (n.len <= p.preLen)
    {
        uint64_t const span = p.pow[p.preLen - n.len];
        n.lo                = (uint32_t)p.pre[n.prefix * span];
        n.hi                = (uint32_t)p.pre[(n.prefix + 1) * span];
        return n;
    }
    uint64_t const scale = p.pow[p.keyLen - n.len], first = n.prefix * scale, last = first + (scale - 1);
    uint32_t       a = cu.lo, b = cu.hi;
    while (a < b) // first entry with key >= first
    {
        uint32_t const mid = a + (b - a) / 2;
        if (p.entries[mid].key < first)
            a = mid + 1;
        else
            b = mid;
    }
    n.lo = a;
    b    = cu.hi;
    while (a < b) // first entry with key > last
    {
        uint32_t const mid = a + (b - a) / 2;
        if (p.entries[mid].key <= last)
            a = mid + 1;
        else
            b = mid;
    }
    n.hi = a;
    return n;
}

// seedLooksPromising (host/lx_seeding.hpp, :426-481), the same integer arithmetic
__device__ __forceinline__ bool dev_promising(uint8_t const * q, uint64_t qLen, uint8_t const * s, uint64_t sLen, uint64_t qryStart, uint64_t qryEnd,
                                              uint64_t subjStart, int seedLength, int preScoring, double preScoringThresh, int8_t const * matrix)
{
    int64_t  qFrom = (int64_t)qryStart, sFrom = (int64_t)subjStart;
    uint64_t seedSpan = qryEnd - qryStart;
    uint64_t span     = (uint64_t)(seedLength * preScoring) > seedSpan ? (uint64_t)(seedLength * preScoring) : seedSpan;
    if (span > seedSpan)
    {
        qFrom -= (int64_t)((span - seedSpan) / 2);
        sFrom -= (int64_t)((span - seedSpan) / 2);
        int64_t const mn = qFrom < sFrom ? qFrom : sFrom;
        if (mn < 0)
        {
            qFrom -= mn;
            sFrom -= mn;
            span += (uint64_t)mn;
        }
        uint64_t const a = qLen - (uint64_t)qFrom, b = sLen - (uint64_t)sFrom;
        span             = a < span ? a : span;
        span             = b < span ? b : span;
    }
    int       sc = 0, maxScore = 0;
    int const thresh = (int)(preScoringThresh * (double)span);
    for (uint64_t i = 0; i < span; ++i)
    {
        sc += matrix[(q[(uint64_t)qFrom + i] & 31) * LX_ALPH + (s[(uint64_t)sFrom + i] & 31)];
        if (sc < 0)
            sc = 0;
        else if (sc > maxScore)
            maxScore = sc;
        if (maxScore >= thresh)
            return true;
    }
    return false;
}

// MASKED: p.qMask holds a query mask's distance bytes (lx_qmask.h) and a start whose seed covers a masked letter is blocked; the
// instantiation without a mask compiles the two tests away (profiles/query_mask_bench.txt: seeding without a mask takes what it took).
template <bool MASKED>
__global__ __launch_bounds__(64) void seed_reads_kernel(SeedDev p)
{
    uint64_t const r = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= p.nReads)
        return;
    uint64_t const read0 = p.reads[r];
    size_t         foundForRead = 0, framesTotal = 0, framesDone = 0;
    size_t const   kOccFactor  = 10;
    unsigned long long nHits = 0, nFailed = 0;
    bool               ok    = true;

    // one final cursor of a seed: adaptive elongation, the over-abundance cut, every located hit through seedLooksPromising
    auto finish_cursor = [&](DevCursor cursor, uint64_t i, uint64_t L, uint8_t const * red, uint8_t const * res, uint64_t seedBegin)
    {
        uint64_t seedLength = (uint64_t)p.seedLength;
        if (p.adaptive)
        {
            size_t const left        = (framesTotal - framesDone - seedBegin) / (size_t)p.seedOffset;
            size_t       wanted = foundForRead >= p.maxMatches ? 1 : (p.maxMatches - foundForRead) * kOccFactor / (left > 1 ? left : 1);
            if (wanted == 0)
                wanted = 1;
            DevCursor kept = cursor;
            size_t    keptCount  = dev_count(cursor, p.keyLen);
            while (seedBegin + seedLength < L)
            {
                cursor = dev_extend(p, cursor, red[seedBegin + seedLength], ok);
                if (!ok)
                    return;
                size_t const count = dev_count(cursor, p.keyLen);
                if (count < wanted && count < keptCount)
                {
                    cursor = kept;
                    break;
                }
                ++seedLength;
                keptCount  = count;
                kept = cursor;
            }
        }
        uint32_t const cnt = dev_count(cursor, p.keyLen);
        if (cnt > kOccFactor * p.maxMatches)
            return;
        bool const listed = cursor.len > p.keyLen;
        for (uint32_t e = cursor.lo; e < cursor.hi; ++e)
        {
            if (listed && !((cursor.mask >> (e - cursor.lo)) & 1u))
                continue;
            ReducedIndex::Entry const x = p.entries[e];
            ++nHits;
            int8_t const * mat = (p.matrixRev && (x.seq & 1u)) ? p.matrixRev : p.matrix;
            if (!dev_promising(res, L, p.sRes + p.sOff[x.seq], p.sLen[x.seq], seedBegin, seedBegin + seedLength, x.pos, p.seedLength, p.preScoring,
                               p.preScoringThresh, mat))
                ++nFailed;
            else
            {
                unsigned long long const at = atomicAdd(p.counters, 1ull);
                if (at < p.outCap)
                    p.out[at] = lx_match{i, x.seq, seedBegin, seedBegin + seedLength, x.pos, x.pos + seedLength};
                else
                    atomicExch(p.counters + 3, 1ull);
                ++foundForRead;
            }
        }
    };

    for (int f = 0; f < p.qNumFrames && ok; ++f)
    {
        uint64_t const i = read0 + (uint64_t)f;
        if (i >= p.nQSeq)
            break;
        if (f == 0) // (the per-read reset of seedQueries, before the length test like there)
        {
            foundForRead = framesTotal = framesDone = 0;
            for (int j = 0; j < p.qNumFrames && i + (uint64_t)j < p.nQSeq; ++j)
                framesTotal += p.qLen[i + (uint64_t)j];
        }
        if (p.qLen[i] < (uint64_t)p.seedLength)
            continue;
        uint64_t const        L   = p.qLen[i];
        uint8_t const * const red = p.qRed + p.qOff[i];
        uint8_t const * const res = p.qRes + p.qOff[i];
        uint8_t const * const dist = MASKED ? p.qMask + p.qOff[i] : nullptr;
        for (uint64_t seedBegin = 0; ok; seedBegin += (uint64_t)p.seedOffset)
        {
            while (seedBegin < L - (uint64_t)p.seedLength && (res[seedBegin] == (uint8_t)p.unknownRank || res[seedBegin] == res[seedBegin + 1] ||
                                                              (MASKED && dist[seedBegin] < (uint8_t)p.seedLength)))
                ++seedBegin;
            if (seedBegin > L - (uint64_t)p.seedLength)
                break;
            if (MASKED && dist[seedBegin] < (uint8_t)p.seedLength) // (the last start, still blocked: the frame ends)
                break;
            uint8_t const * const seed = red + seedBegin;
            int const firstHalf  = p.maxSeedDist == 0 ? p.seedLength : p.halfExact ? p.seedLength / 2 : 0;
            int const secondHalf = p.seedLength - firstHalf;
            if (secondHalf > kMaxSecond)
            {
                ok = false;
                break;
            }
            DevCursor c{0u, (uint32_t)p.pre[p.pow[p.preLen]], 0u, 0, 0ull};
            bool      alive = true;
            for (int k = 0; k < firstHalf && alive && ok; ++k)
            {
                c     = dev_extend(p, c, seed[k], ok);
                alive = dev_count(c, p.keyLen) != 0;
            }
            if (!ok)
                break;
            if (!alive)
                continue;
            if (secondHalf == 0)
            {
                finish_cursor(c, i, L, red, res, seedBegin);
                continue;
            }
            // depth-first over the second half: a cursor below the error budget branches into every letter (another letter costs
            // one error), the others go on with the seed's letter
            DevCursor stack[kMaxSecond + 1];
            uint8_t   errs[kMaxSecond + 1], next[kMaxSecond + 1];
            int       level = 0;
            stack[0] = c, errs[0] = 0, next[0] = 0;
            while (level >= 0 && ok)
            {
                if (level == secondHalf)
                {
                    finish_cursor(stack[level], i, L, red, res, seedBegin);
                    --level;
                    continue;
                }
                uint8_t const want = seed[firstHalf + level];
                uint32_t      letter;
                if ((int)errs[level] < p.maxSeedDist)
                {
                    if ((int)next[level] >= p.alph)
                    {
                        --level;
                        continue;
                    }
                    letter = next[level]++;
                }
                else
                {
                    if (next[level] != 0)
                    {
                        --level;
                        continue;
                    }
                    next[level] = 1;
                    letter      = want;
                }
                DevCursor const child = dev_extend(p, stack[level], letter, ok);
                if (!ok || dev_count(child, p.keyLen) == 0)
                    continue;
                stack[level + 1] = child;
                errs[level + 1]  = (uint8_t)(errs[level] + (letter != want ? 1 : 0));
                next[level + 1]  = 0;
                ++level;
            }
        }
        framesDone += L;
    }
    if (!ok)
    {
        p.declined[r] = 1; // (what the lane wrote so far is dropped by the host, which seeds the read again from its first frame)
        return;
    }
    if (nHits)
        atomicAdd(p.counters + 1, nHits);
    if (nFailed)
        atomicAdd(p.counters + 2, nFailed);
}

// ---- the word table on the GPU: the keys of all positions (one thread each), one radix sort of (key, sequence << 32 | position)
// pairs -- the library's own radix sort (lx_level2.hip: l2_launch_sort, through lx_sort_words_dev); stable, and the pairs start in
// (sequence, position) order, so equal words end up ordered by sequence and position as in the host's table --, the entries
// interleaved, the prefix table by one binary search per prefix.  The same table bit for bit as ReducedIndex::build's.
__global__ void table_keys_kernel(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                  int keyLen, uint64_t base, int alph, uint64_t * keys, uint64_t * vals)
{
    uint64_t const e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total)
        return;
    uint64_t a = 0, b = nSeq; // the sequence that holds entry e: last s with first[s] <= e (empty sequences share a start)
    while (b - a > 1)
    {
        uint64_t const mid = a + (b - a) / 2;
        if (first[mid] <= e)
            a = mid;
        else
            b = mid;
    }
    while (a + 1 < nSeq && first[a + 1] <= e) // (skip empty sequences that start where the next one does)
        ++a;
    uint64_t const pos = e - first[a], L = len[a];
    uint8_t const * r  = red + off[a] + pos;
    uint64_t        key = 0;
    for (int i = 0; i < keyLen; ++i)
        key = key * base + (pos + (uint64_t)i < L ? (uint64_t)r[i] : (uint64_t)alph);
    keys[e] = key;
    vals[e] = (a << 32) | pos;
}

__global__ void table_entries_kernel(uint64_t const * keys, uint64_t const * vals, uint64_t total, ReducedIndex::Entry * out)
{
    uint64_t const e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total)
        out[e] = ReducedIndex::Entry{keys[e], (uint32_t)(vals[e] >> 32), (uint32_t)vals[e]};
}

__global__ void table_prefix_kernel(uint64_t const * keys, uint64_t total, uint64_t preDiv, uint64_t nPre, uint64_t * pre)
{
    uint64_t const w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nPre)
        return;
    uint64_t a = 0, b = total; // first entry whose first preLen letters are >= the word w
    while (a < b)
    {
        uint64_t const mid = a + (b - a) / 2;
        if (keys[mid] / preDiv < w)
            a = mid + 1;
        else
            b = mid;
    }
    pre[w] = a;
}

// ---- the word table in slices of the key space (lx_seed_host.cpp: build_in_slices), for sets whose keys do not fit the device, or the
// sort's 32-bit ranks, all at once.  The words' first preLen letters are counted into a 64-bit histogram whose exclusive scan IS the
// prefix table; the host cuts it into runs of buckets (lx_index_plan_slices); per slice the positions whose prefix lies in the run are
// compacted in (sequence, position) order -- flag counts per block, a scan, the write --, sorted by the same radix sort and written as
// entries where the prefix table says the run begins.  Every pass reads the reduced subjects again: bandwidth next to a sort.

// the sequence that holds entry e and e's position in it (first[s] = entry of sequence s's first position; as table_keys_kernel)
__device__ __forceinline__ uint64_t place_of(uint64_t const * first, uint64_t nSeq, uint64_t e, uint64_t & pos)
{
    uint64_t a = 0, b = nSeq;
    while (b - a > 1)
    {
        uint64_t const mid = a + (b - a) / 2;
        if (first[mid] <= e)
            a = mid;
        else
            b = mid;
    }
    while (a + 1 < nSeq && first[a + 1] <= e) // (skip empty sequences that start where the next one does)
        ++a;
    pos = e - first[a];
    return a;
}

// letters [from, to) behind position pos appended to `word` (the pad digit behind the sequence's end)
__device__ __forceinline__ uint64_t word_more(uint64_t word, uint8_t const * r, uint64_t pos, uint64_t L, int from, int to, uint64_t base, int alph)
{
    for (int i = from; i < to; ++i)
        word = word * base + (pos + (uint64_t)i < L ? (uint64_t)r[i] : (uint64_t)alph);
    return word;
}

constexpr uint64_t kNoWord = ~0ull; // a lane behind the last position

// (a) hist[w] += the positions whose first preLen letters are the word w.  Real sets hold long runs of one word (poly-A, masked
// stretches, the pads): neighbouring lanes with the same word are combined, the run's first lane adds its length -- one atomic per
// run of a wavefront, not one per position.
__global__ __launch_bounds__(kTabBlock) void table_counts_kernel(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first,
                                                                 uint64_t nSeq, uint64_t total, int preLen, uint64_t base, int alph, uint64_t nPre,
                                                                 unsigned long long * hist)
{
    uint64_t const e = (uint64_t)blockIdx.x * kTabBlock + threadIdx.x;
    uint64_t       w = kNoWord;
    if (e < total)
    {
        uint64_t       pos;
        uint64_t const a = place_of(first, nSeq, e, pos);
        w                = word_more(0, red + off[a] + pos, pos, len[a], 0, preLen, base, alph);
    }
    int const      lane  = threadIdx.x & 63;
    uint64_t const left  = (uint64_t)__shfl_up((unsigned long long)w, 1);
    bool const     head  = lane == 0 || left != w;
    uint64_t const heads = __ballot(head);
    if (head && w < nPre)
    {
        uint64_t const above = lane == 63 ? 0ull : heads >> (lane + 1); // (bit k: lane + 1 + k begins the next run)
        int const      run   = above ? __ffsll((unsigned long long)above) : 64 - lane;
        atomicAdd(hist + w, (unsigned long long)run);
    }
}

// ---- an exclusive 64-bit sum scan in place (lx_scan.h's tiled scans carry uint32_t): the tiles' sums, one workgroup that turns them
// into what precedes each tile, the pass over the elements

__device__ __forceinline__ uint64_t block_inclusive64(uint64_t v, uint64_t * wave_tot, uint64_t & total)
{
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t  incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        uint64_t const up = (uint64_t)__shfl_up((unsigned long long)incl, o);
        if (lane >= o)
            incl += up;
    }
    if (lane == 63)
        wave_tot[wave] = incl;
    __syncthreads();
    uint64_t before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kTabBlock / 64; ++k)
    {
        uint64_t const x = wave_tot[k];
        if (k < wave)
            before += x;
        tot += x;
    }
    total = tot;
    __syncthreads();
    return before + incl;
}

__global__ __launch_bounds__(kTabBlock) void scan64_sums_kernel(uint64_t const * a, uint64_t n, uint64_t * tile_tot)
{
    __shared__ uint64_t wave_tot[kTabBlock / 64];
    uint64_t const      j0  = (uint64_t)blockIdx.x * kTabScanTile + threadIdx.x;
    uint64_t            acc = 0;
#pragma unroll
    for (int k = 0; k < kTabScanItems; ++k)
    {
        uint64_t const j = j0 + (uint64_t)k * kTabBlock;
        if (j < n)
            acc += a[j];
    }
    uint64_t total;
    (void)block_inclusive64(acc, wave_tot, total);
    if (threadIdx.x == 0)
        tile_tot[blockIdx.x] = total;
}

__global__ __launch_bounds__(kTabBlock) void scan64_tops_kernel(uint64_t * tile_tot, uint64_t tiles)
{
    __shared__ uint64_t wave_tot[kTabBlock / 64];
    uint64_t            carry = 0;
    for (uint64_t b0 = 0; b0 < tiles; b0 += kTabBlock)
    {
        uint64_t const b = b0 + threadIdx.x;
        uint64_t const v = b < tiles ? tile_tot[b] : 0;
        uint64_t       total;
        uint64_t const incl = block_inclusive64(v, wave_tot, total);
        if (b < tiles)
            tile_tot[b] = carry + incl - v;
        carry += total;
    }
}

// (a thread reads its kTabScanItems consecutive values before it writes them: in place)
__global__ __launch_bounds__(kTabBlock) void scan64_apply_kernel(uint64_t * a, uint64_t n, uint64_t const * tile_before)
{
    __shared__ uint64_t wave_tot[kTabBlock / 64];
    uint64_t const      j0 = (uint64_t)blockIdx.x * kTabScanTile + (uint64_t)threadIdx.x * kTabScanItems;
    uint64_t            v[kTabScanItems], acc = 0;
#pragma unroll
    for (int k = 0; k < kTabScanItems; ++k)
    {
        v[k] = j0 + (uint64_t)k < n ? a[j0 + (uint64_t)k] : 0;
        acc += v[k];
    }
    uint64_t       total;
    uint64_t const incl = block_inclusive64(acc, wave_tot, total);
    uint64_t       run  = tile_before[blockIdx.x] + incl - acc;
#pragma unroll
    for (int k = 0; k < kTabScanItems; ++k)
    {
        if (j0 + (uint64_t)k < n)
            a[j0 + (uint64_t)k] = run;
        run += v[k];
    }
}

// (d) a slice = the buckets [wLo, wHi).  block_cnt[b] = how many of block b's positions belong to it ...
__global__ __launch_bounds__(kTabBlock) void table_slice_counts_kernel(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first,
                                                                       uint64_t nSeq, uint64_t total, int preLen, uint64_t base, int alph, uint64_t wLo,
                                                                       uint64_t wHi, uint64_t * block_cnt)
{
    __shared__ uint32_t wave_cnt[kTabBlock / 64];
    uint64_t const      e  = (uint64_t)blockIdx.x * kTabBlock + threadIdx.x;
    bool                in = false;
    if (e < total)
    {
        uint64_t       pos;
        uint64_t const a = place_of(first, nSeq, e, pos);
        uint64_t const w = word_more(0, red + off[a] + pos, pos, len[a], 0, preLen, base, alph);
        in               = w >= wLo && w < wHi;
    }
    uint64_t const mine = __ballot(in);
    if ((threadIdx.x & 63) == 0)
        wave_cnt[threadIdx.x >> 6] = (uint32_t)__popcll((unsigned long long)mine);
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t sum = 0;
        for (int k = 0; k < kTabBlock / 64; ++k)
            sum += wave_cnt[k];
        block_cnt[blockIdx.x] = sum;
    }
}

// ... and, block_before = the exclusive scan of those counts, its keys and values at block_before[b] + the position's rank among the
// block's: the slice's pairs in (sequence, position) order, as the stable sort wants them.  cap = the slice's words.
__global__ __launch_bounds__(kTabBlock) void table_slice_keys_kernel(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first,
                                                                     uint64_t nSeq, uint64_t total, int preLen, int keyLen, uint64_t base, int alph, uint64_t wLo,
                                                                     uint64_t wHi, uint64_t const * block_before, uint64_t cap, uint64_t * keys, uint64_t * vals)
{
    __shared__ uint32_t wave_cnt[kTabBlock / 64];
    uint64_t const      e = (uint64_t)blockIdx.x * kTabBlock + threadIdx.x;
    int const           lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool                in = false;
    uint64_t            a = 0, pos = 0, w = 0;
    if (e < total)
    {
        a  = place_of(first, nSeq, e, pos);
        w  = word_more(0, red + off[a] + pos, pos, len[a], 0, preLen, base, alph);
        in = w >= wLo && w < wHi;
    }
    uint64_t const mine = __ballot(in);
    if (lane == 0)
        wave_cnt[wave] = (uint32_t)__popcll((unsigned long long)mine);
    __syncthreads();
    if (!in)
        return;
    uint64_t at = block_before[blockIdx.x] + (uint64_t)__popcll((unsigned long long)(mine & ((1ull << lane) - 1ull)));
    for (int k = 0; k < wave; ++k)
        at += wave_cnt[k];
    if (at >= cap)
        return;
    keys[at] = word_more(w, red + off[a] + pos, pos, len[a], preLen, keyLen, base, alph);
    vals[at] = (a << 32) | pos;
}

hipError_t seed_launch_table_counts(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                    int preLen, uint64_t base, int alph, uint64_t nPre, uint64_t * hist, hipStream_t stream)
{
    if (total == 0)
        return hipSuccess;
    hipLaunchKernelGGL(table_counts_kernel, dim3((unsigned)tab_blocks(total)), dim3(kTabBlock), 0, stream, red, off, len, first, nSeq, total, preLen, base, alph, nPre, reinterpret_cast<unsigned long long *>(hist));
    return hipGetLastError();
}

hipError_t seed_launch_scan64(uint64_t * a, uint64_t n, uint64_t * tile_tot, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    unsigned const tiles = (unsigned)tab_scan_tiles(n);
    hipLaunchKernelGGL(scan64_sums_kernel, dim3(tiles), dim3(kTabBlock), 0, stream, a, n, tile_tot);
    hipLaunchKernelGGL(scan64_tops_kernel, dim3(1), dim3(kTabBlock), 0, stream, tile_tot, (uint64_t)tiles);
    hipLaunchKernelGGL(scan64_apply_kernel, dim3(tiles), dim3(kTabBlock), 0, stream, a, n, tile_tot);
    return hipGetLastError();
}

hipError_t seed_launch_table_slice_counts(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                          int preLen, uint64_t base, int alph, uint64_t wLo, uint64_t wHi, uint64_t * block_cnt, hipStream_t stream)
{
    if (total == 0)
        return hipSuccess;
    hipLaunchKernelGGL(table_slice_counts_kernel, dim3((unsigned)tab_blocks(total)), dim3(kTabBlock), 0, stream, red, off, len, first, nSeq, total, preLen, base,
                       alph, wLo, wHi, block_cnt);
    return hipGetLastError();
}

hipError_t seed_launch_table_slice_keys(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                        int preLen, int keyLen, uint64_t base, int alph, uint64_t wLo, uint64_t wHi, uint64_t const * block_before, uint64_t cap,
                                        uint64_t * keys, uint64_t * vals, hipStream_t stream)
{
    if (total == 0 || cap == 0)
        return hipSuccess;
    hipLaunchKernelGGL(table_slice_keys_kernel, dim3((unsigned)tab_blocks(total)), dim3(kTabBlock), 0, stream, red, off, len, first, nSeq, total, preLen, keyLen,
                       base, alph, wLo, wHi, block_before, cap, keys, vals);
    return hipGetLastError();
}

hipError_t seed_launch_reads(SeedDev const & p, hipStream_t stream)
{
    if (p.nReads == 0)
        return hipSuccess;
    if (p.qMask)
        hipLaunchKernelGGL(seed_reads_kernel<true>, dim3((unsigned)((p.nReads + 63) / 64)), dim3(64), 0, stream, p);
    else
        hipLaunchKernelGGL(seed_reads_kernel<false>, dim3((unsigned)((p.nReads + 63) / 64)), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t seed_launch_table_keys(uint8_t const * red, uint64_t const * off, uint64_t const * len, uint64_t const * first, uint64_t nSeq, uint64_t total,
                                  int keyLen, uint64_t base, int alph, uint64_t * keys, uint64_t * vals, hipStream_t stream)
{
    if (total == 0)
        return hipSuccess;
    hipLaunchKernelGGL(table_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, red, off, len, first, nSeq, total, keyLen, base, alph, keys, vals);
    return hipGetLastError();
}

hipError_t seed_launch_table_entries(uint64_t const * keys, uint64_t const * vals, uint64_t total, ReducedIndex::Entry * out, hipStream_t stream)
{
    if (total == 0)
        return hipSuccess;
    hipLaunchKernelGGL(table_entries_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, keys, vals, total, out);
    return hipGetLastError();
}

hipError_t seed_launch_table_prefix(uint64_t const * keys, uint64_t total, uint64_t preDiv, uint64_t nPre, uint64_t * pre, hipStream_t stream)
{
    if (nPre == 0)
        return hipSuccess;
    hipLaunchKernelGGL(table_prefix_kernel, dim3((unsigned)((nPre + 255) / 256)), dim3(256), 0, stream, keys, total, preDiv, nPre, pre);
    return hipGetLastError();
}

} // namespace lx
