// lx_toprec.hip -- _writeRecord's sort / unique / sort / cut (/root/reference/src/search_algo.hpp:820-882; the host form is
// lx_postprocess_records, host/lx_postprocess.cpp) for lx_blast_match rows that stand in device memory grouped by n_qid (gfx950).
//
// Per run of equal n_qid (a "segment"; a run, not a query: rows that are not grouped give one segment per run, as on the host):
//   order 1   ascending by (n_sid, q_start, q_end, s_start, s_end, q_frame, s_frame) -- the five coordinates as unsigned 64-bit
//             words, the frames as SIGNED 16-bit values --, then bit_score DESCENDING (the double that stands in the row: nothing is
//             recomputed), then input position: std::stable_sort's guarantee made explicit
//   unique    a row whose seven-field key equals its predecessor's in order 1 is dropped (hits_duplicate2)
//   order 2   the survivors by bit_score descending, ties by place in order 1
//   cut       the first max_matches stay, the rest is counted (hits_abundant); pairs = distinct n_sid among those that stay
// and the rows that stay are written behind one another: segments in input order, order 2 inside each.
//
// No row is moved until its final place is known.  Every row is owned by one thread, and a place in a sorted order is the number
// of rows of the segment that come before: order 1's place and the duplicate flag are COUNTED (a row is a duplicate exactly when a
// row of equal key comes before it), then order 2's place among the rows that are no duplicates, then -- among the rows that stay --
// whether another one of the same subject comes before (pairs).  Three counting kernels of one shape:
//   * a workgroup of 256 threads owns 256 consecutive rows; the segments these rows belong to span rows [lo, hi) of the list;
//   * what the count compares (kernel 1: the seven fields and the bit score, 52 bytes; kernel 2: bit score and place, 12 bytes;
//     kernel 3: subject and place, 12 bytes) is staged in LDS for kTopTile = 512 rows of the span at a time, as one array per field;
//   * every thread walks the staged rows of ITS segment and counts.  The lanes of a wavefront (64 lanes) that share a segment read the
//     same staged row at the same time: one address, which the LDS broadcasts (MI355X_MICROARCH.md, LDS: "identical addresses
//     broadcast"; ds_read_b64 is served in 2 cycles per wave-instruction).
// Typical lists -- a few to a few hundred rows per query -- have a span of at most 512 rows for most workgroups: the keys are staged
// ONCE, a lane's walk is as long as its own segment, and the wavefront's walk as long as the longest segment among its lanes.
// The large-segment path is the same loop taking more than one turn: a span beyond kTopTile rows is staged tile by tile (a barrier
// pair per tile), every workgroup that owns rows of the segment walks all of its tiles.  Exact for any length (places are counts of
// a total order), quadratic in the segment's length: s rows cost s * s comparisons spread over s / 256 workgroups -- 9 M for the
// 3 000-row segment of the tests, 10^10 for a segment of 100 000 rows, which is where LSD passes of the radix sort over the key's 45
// bytes would win; no list of the front end comes near (a query has at most as many rows as it has windows).
// Sizes (cdna_hip_programming.md section 10 / MI355X_MICROARCH.md): 160 KiB of LDS per CU; kernel 1 declares 512 * 52 B = 26 KiB,
// so 6 workgroups = 24 of the CU's 32 wavefront slots by LDS; kernels 2 and 3 (6 KiB) are limited by the 32 wavefronts alone.
//
// Between the unique and the cut, where lx_cull_options asks for it (the rule: lx_cull.h), two more counts of the same shape over the
// rows that are no duplicates; "better" = earlier in order 2, which is the bit score and the place in order 1 that kernel 1 left:
//   kernel 4 (max_hsps = K > 0) stages subject, bit score and place (20 bytes a row) and counts the better rows of the row's subject:
//            K or more, and the row is dropped (hits_max_hsps);
//   kernel 5 (culling_limit = L > 0) stages the two ends of the query interval, bit score and place (20 bytes a row) and counts the
//            better rows, among those that kernel 4 left, whose interval envelops the row's: L or more, and the row is dropped
//            (hits_culled).  The intervals are computed once per row by an elementwise kernel into two uint32_t arrays of `work`
//            (a query beyond 2^32 - 1 letters is refused on the host).
// Each writes a copy of kernel 1's word with the flag also set for the rows it dropped; kernel 2 reads the last copy (TopParams::live),
// so that order 2's place and "stays" are counted among the rows that survive both.  Neither is launched when its option is 0: the
// default path queues the kernels, and takes the scratch, that it did before they existed.  Kernels 4 and 5 declare 512 * 20 B =
// 10 KiB of LDS each: 16 workgroups by LDS, more than the CU's 32 wavefront slots hold -- limited by the 32 wavefronts alone (8
// workgroups), as kernels 2 and 3.
//
// Segments come from one scan (lx_scan.h): heads by comparing neighbours, segment number = heads up to the row, start of segment k
// scattered by its head.  The rows' final places come from a second scan, over the flags "stays".  With alignment columns
// (rebase_ops) a third scan, 64-bit, over n_ops of the rows in OUTPUT order gives every row its new ops_off.  The Level-2 driver's
// columns never stand in device memory -- the host threads expand them from run-length codes (lx_level2_host.cpp) into the place
// the row names -- so the step moves each row's three code words (where its codes begin, where its columns go, how many) along
// with the row and re-bases the middle one: the columns of rows that the cut removes are never expanded, and no bytes are copied.
// The number of rows may stand in device memory (n_ptr): the driver queues the step behind the records kernels of a range without
// learning on the host how many records they made.  Vector stores and vector atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lx_cull.h"
#include "lx_level2.h"
#include "lx_toprec.h"

namespace lx
{

namespace
{

#include "lx_scan.h"

constexpr int      kTopBlock = 256;
constexpr uint32_t kTopTile  = 512; // staged rows per turn
constexpr uint32_t kFlag     = 0x80000000u;

__device__ __forceinline__ uint64_t rows_of(TopParams const & p)
{
    return p.n_ptr ? min(*p.n_ptr, p.n_cap) : p.n_cap;
}

// the frames as one word whose unsigned order is the order of (q_frame, s_frame) as signed values
__device__ __forceinline__ uint32_t frame_word(BlastMatchDev const & r)
{
    return ((uint32_t)(uint16_t)(r.q_frame ^ (int16_t)0x8000) << 16) | (uint32_t)(uint16_t)(r.s_frame ^ (int16_t)0x8000);
}

// ---- segments -----------------------------------------------------------------------------------------------------------------
struct SegVal
{
    TopParams p;
    __device__ uint32_t operator()(uint64_t i) const
    {
        uint64_t const n = rows_of(p);
        return i < n && (i == 0 || p.in[i].n_qid != p.in[i - 1].n_qid) ? 1u : 0u;
    }
};
struct SegOut
{
    TopParams p;
    __device__ void operator()(uint64_t i, uint32_t incl, uint32_t excl) const
    {
        uint64_t const n = rows_of(p);
        if (i >= n)
            return;
        p.seg_id[i] = incl - 1;
        if (incl != excl)
            p.seg_start[incl - 1] = (uint32_t)i;
        if (i == n - 1)
        {
            p.seg_start[incl]      = (uint32_t)n;
            p.counters[kTopQueries] = incl;
        }
    }
};

// what a workgroup's 256 rows need of the list: the rows of every segment one of them belongs to
struct Span
{
    uint64_t n, first, i;
    uint32_t lo, hi; // the span
    uint32_t s, e;   // the thread's own segment (s == e: no row)
    bool     valid;
};
__device__ __forceinline__ Span span_of(TopParams const & p)
{
    Span sp;
    sp.n     = rows_of(p);
    sp.first = (uint64_t)blockIdx.x * kTopBlock;
    sp.i     = sp.first + threadIdx.x;
    sp.valid = sp.i < sp.n;
    sp.lo = sp.hi = sp.s = sp.e = 0;
    if (sp.first >= sp.n)
        return sp;
    uint64_t const last = min(sp.n, sp.first + kTopBlock) - 1;
    sp.lo = p.seg_start[p.seg_id[sp.first]];
    sp.hi = p.seg_start[p.seg_id[last] + 1];
    if (sp.valid)
    {
        uint32_t const k = p.seg_id[sp.i];
        sp.s = p.seg_start[k];
        sp.e = p.seg_start[k + 1];
    }
    return sp;
}

// adds a flag of every thread to a counter: one atomic per wavefront
__device__ __forceinline__ void count_flag(bool f, uint64_t * counter)
{
    unsigned long long const m = __ballot(f);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long *>(counter), (unsigned long long)__popcll(m));
}

// ---- kernel 1: place in order 1 and the duplicate flag ---------------------------------------------------------------------------
__global__ __launch_bounds__(kTopBlock) void top_rank1_kernel(TopParams p)
{
    __shared__ uint64_t k_sid[kTopTile], k_qs[kTopTile], k_qe[kTopTile], k_ss[kTopTile], k_se[kTopTile];
    __shared__ double   k_bs[kTopTile];
    __shared__ uint32_t k_fr[kTopTile];
    Span const sp = span_of(p);
    if (sp.first >= sp.n)
        return;
    uint64_t sid = 0, qs = 0, qe = 0, ss = 0, se = 0;
    double   bs = 0;
    uint32_t fr = 0;
    if (sp.valid)
    {
        BlastMatchDev const & r = p.in[sp.i];
        sid = r.n_sid, qs = r.q_start, qe = r.q_end, ss = r.s_start, se = r.s_end, bs = r.bit_score, fr = frame_word(r);
    }
    uint32_t before = 0, dup = 0;
    for (uint32_t t0 = sp.lo; t0 < sp.hi; t0 += kTopTile)
    {
        uint32_t const t1 = min(sp.hi, t0 + kTopTile);
        for (uint32_t j = t0 + threadIdx.x; j < t1; j += kTopBlock)
        {
            BlastMatchDev const & r = p.in[j];
            uint32_t const        k = j - t0;
            k_sid[k] = r.n_sid, k_qs[k] = r.q_start, k_qe[k] = r.q_end, k_ss[k] = r.s_start, k_se[k] = r.s_end, k_bs[k] = r.bit_score, k_fr[k] = frame_word(r);
        }
        __syncthreads();
        uint32_t const a = max(sp.s, t0), b = min(sp.e, t1);
        for (uint32_t j = a; j < b; ++j)
        {
            uint32_t const k = j - t0;
            // lexicographic "row j's key < mine" and "== mine", from the last field to the first
            uint32_t const fj = k_fr[k];
            bool           lt = fj < fr, eq = fj == fr;
            uint64_t       x;
            x = k_se[k], lt = x < se || (x == se && lt), eq = eq && x == se;
            x = k_ss[k], lt = x < ss || (x == ss && lt), eq = eq && x == ss;
            x = k_qe[k], lt = x < qe || (x == qe && lt), eq = eq && x == qe;
            x = k_qs[k], lt = x < qs || (x == qs && lt), eq = eq && x == qs;
            x = k_sid[k], lt = x < sid || (x == sid && lt), eq = eq && x == sid;
            // equal keys: the better bit score first, then the earlier row (the comparator of lx_postprocess_records: b.bit_score <
            // a.bit_score as the last component, under std::stable_sort)
            double const bj    = k_bs[k];
            bool const   first = eq && (bs < bj || (!(bj < bs) && (uint64_t)j < sp.i));
            before += (lt || first) ? 1u : 0u;
            dup |= first ? 1u : 0u;
        }
        __syncthreads();
    }
    if (sp.valid)
        p.r1[sp.i] = before | (dup ? kFlag : 0u);
    count_flag(sp.valid && dup, p.counters + kTopDuplicate);
}

// ---- kernel 4 (max_hsps > 0): the better rows of the same subject among the rows that are no duplicates ---------------------------
__global__ __launch_bounds__(kTopBlock) void top_hsps_kernel(TopParams p)
{
    __shared__ uint64_t k_sid[kTopTile];
    __shared__ double   k_bs[kTopTile];
    __shared__ uint32_t k_r1[kTopTile];
    Span const sp = span_of(p);
    if (sp.first >= sp.n)
        return;
    uint64_t const sid = sp.valid ? p.in[sp.i].n_sid : 0;
    double const   bs  = sp.valid ? p.in[sp.i].bit_score : 0.0;
    uint32_t const r1  = sp.valid ? p.r1[sp.i] : kFlag;
    uint32_t       same = 0;
    for (uint32_t t0 = sp.lo; t0 < sp.hi; t0 += kTopTile)
    {
        uint32_t const t1 = min(sp.hi, t0 + kTopTile);
        for (uint32_t j = t0 + threadIdx.x; j < t1; j += kTopBlock)
        {
            k_sid[j - t0] = p.in[j].n_sid;
            k_bs[j - t0]  = p.in[j].bit_score;
            k_r1[j - t0]  = p.r1[j];
        }
        __syncthreads();
        uint32_t const a = max(sp.s, t0), b = min(sp.e, t1);
        for (uint32_t j = a; j < b; ++j)
        {
            uint32_t const rj = k_r1[j - t0];
            same += !(rj & kFlag) && k_sid[j - t0] == sid && cull::better(k_bs[j - t0], rj, bs, r1 & ~kFlag) ? 1u : 0u;
        }
        __syncthreads();
    }
    bool const dropped = sp.valid && !(r1 & kFlag) && (uint64_t)same >= p.max_hsps;
    if (sp.valid)
        p.live_hsps[sp.i] = r1 | (dropped ? kFlag : 0u);
    count_flag(dropped, p.counters + kTopMaxHsps);
}

// ---- culling_limit > 0: every row's query interval, once ------------------------------------------------------------------------------
__global__ __launch_bounds__(kTopBlock) void top_interval_kernel(TopParams p)
{
    uint64_t const i = (uint64_t)blockIdx.x * kTopBlock + threadIdx.x;
    if (i >= rows_of(p))
        return;
    BlastMatchDev const & r  = p.in[i];
    uint64_t const        at = r.n_qid * (uint64_t)p.q_len_stride;
    // (the callers refuse rows whose query is not in the list or whose interval does not fit: such a row would get [0, 0] here)
    uint64_t const len = r.n_qid < p.q_lens_n && at < p.q_lens_n ? p.q_lens[at] : 0;
    uint64_t       lo, hi;
    (void)cull::interval(r.q_start, r.q_end, r.q_frame, len, p.q_translated != 0, lo, hi);
    p.iv_lo[i] = (uint32_t)min(lo, (uint64_t)0xffffffffu);
    p.iv_hi[i] = (uint32_t)min(hi, (uint64_t)0xffffffffu);
}

// ---- kernel 5 (culling_limit > 0): the better rows whose interval envelops the row's, among the rows that kernel 4 left -----------------
__global__ __launch_bounds__(kTopBlock) void top_cull_kernel(TopParams p, uint32_t const * __restrict__ left)
{
    __shared__ double   k_bs[kTopTile];
    __shared__ uint32_t k_lo[kTopTile], k_hi[kTopTile], k_r1[kTopTile];
    Span const sp = span_of(p);
    if (sp.first >= sp.n)
        return;
    double const   bs = sp.valid ? p.in[sp.i].bit_score : 0.0;
    uint32_t const r1 = sp.valid ? left[sp.i] : kFlag;
    uint32_t const lo = sp.valid ? p.iv_lo[sp.i] : 0u, hi = sp.valid ? p.iv_hi[sp.i] : 0u;
    uint32_t       around = 0;
    for (uint32_t t0 = sp.lo; t0 < sp.hi; t0 += kTopTile)
    {
        uint32_t const t1 = min(sp.hi, t0 + kTopTile);
        for (uint32_t j = t0 + threadIdx.x; j < t1; j += kTopBlock)
        {
            k_bs[j - t0] = p.in[j].bit_score;
            k_lo[j - t0] = p.iv_lo[j];
            k_hi[j - t0] = p.iv_hi[j];
            k_r1[j - t0] = left[j];
        }
        __syncthreads();
        uint32_t const a = max(sp.s, t0), b = min(sp.e, t1);
        for (uint32_t j = a; j < b; ++j)
        {
            uint32_t const rj = k_r1[j - t0];
            // (rows that are themselves culled count: lx_cull.h says why that changes nothing)
            around += !(rj & kFlag) && cull::envelops(k_lo[j - t0], k_hi[j - t0], lo, hi) && cull::better(k_bs[j - t0], rj, bs, r1 & ~kFlag) ? 1u : 0u;
        }
        __syncthreads();
    }
    bool const culled = sp.valid && !(r1 & kFlag) && (uint64_t)around >= p.culling_limit;
    if (sp.valid)
        p.live[sp.i] = r1 | (culled ? kFlag : 0u);
    count_flag(culled, p.counters + kTopCulled);
}

// ---- kernel 2: place in order 2 among the rows that are no duplicates, and the cut ----------------------------------------------
__global__ __launch_bounds__(kTopBlock) void top_rank2_kernel(TopParams p)
{
    __shared__ double   k_bs[kTopTile];
    __shared__ uint32_t k_r1[kTopTile];
    Span const sp = span_of(p);
    if (sp.first >= sp.n)
        return;
    // (p.live is r1, or -- lx_cull.h -- r1 with the flag also set for the rows that kernels 4 and 5 dropped: no survivors either)
    double const   bs = sp.valid ? p.in[sp.i].bit_score : 0.0;
    uint32_t const r1 = sp.valid ? p.live[sp.i] : kFlag;
    uint32_t       before = 0;
    for (uint32_t t0 = sp.lo; t0 < sp.hi; t0 += kTopTile)
    {
        uint32_t const t1 = min(sp.hi, t0 + kTopTile);
        for (uint32_t j = t0 + threadIdx.x; j < t1; j += kTopBlock)
        {
            k_bs[j - t0] = p.in[j].bit_score;
            k_r1[j - t0] = p.live[j];
        }
        __syncthreads();
        uint32_t const a = max(sp.s, t0), b = min(sp.e, t1);
        for (uint32_t j = a; j < b; ++j)
        {
            double const   bj = k_bs[j - t0];
            uint32_t const rj = k_r1[j - t0];
            // (a duplicate's word has the flag set: it is no survivor, and never below a survivor's place either)
            before += !(rj & kFlag) && (bj > bs || (!(bs > bj) && rj < r1)) ? 1u : 0u;
        }
        __syncthreads();
    }
    bool const alive = sp.valid && !(r1 & kFlag), stays = alive && (uint64_t)before < p.max_matches;
    if (sp.valid)
        p.r2[sp.i] = before | (stays ? kFlag : 0u);
    count_flag(alive && !stays, p.counters + kTopAbundant);
    count_flag(stays, p.counters + kTopFinal);
}

// ---- the rows' places in the output: rows that stay in front of the row's segment + its place in order 2 -------------------------
struct KeepVal
{
    TopParams p;
    __device__ uint32_t operator()(uint64_t i) const
    {
        return i < rows_of(p) ? p.r2[i] >> 31 : 0u;
    }
};
struct KeepOut
{
    TopParams p;
    __device__ void operator()(uint64_t i, uint32_t, uint32_t excl) const
    {
        if (i < rows_of(p))
            p.kept_before[i] = excl;
    }
};

// ---- kernel 3: pairs, and the rows (with their code words) to their places --------------------------------------------------------
__global__ __launch_bounds__(kTopBlock) void top_scatter_kernel(TopParams p)
{
    __shared__ uint64_t k_sid[kTopTile];
    __shared__ uint32_t k_r2[kTopTile];
    __shared__ uint32_t place[kTopBlock];
    Span const sp = span_of(p);
    if (sp.first >= sp.n)
        return;
    uint64_t const sid   = sp.valid ? p.in[sp.i].n_sid : 0;
    uint32_t const r2    = sp.valid ? p.r2[sp.i] : 0u;
    bool const     stays = (r2 & kFlag) != 0;
    uint32_t       same  = 0;
    for (uint32_t t0 = sp.lo; t0 < sp.hi; t0 += kTopTile)
    {
        uint32_t const t1 = min(sp.hi, t0 + kTopTile);
        for (uint32_t j = t0 + threadIdx.x; j < t1; j += kTopBlock)
        {
            k_sid[j - t0] = p.in[j].n_sid;
            k_r2[j - t0]  = p.r2[j];
        }
        __syncthreads();
        uint32_t const a = max(sp.s, t0), b = min(sp.e, t1);
        for (uint32_t j = a; j < b; ++j)
        {
            uint32_t const rj = k_r2[j - t0];
            // a row that stays, of my subject, ahead of me in the output
            same |= (rj & kFlag) && rj < r2 && k_sid[j - t0] == sid ? 1u : 0u;
        }
        __syncthreads();
    }
    count_flag(stays && !same, p.counters + kTopPairs);
    uint32_t const at = stays ? p.kept_before[sp.s] + (r2 & ~kFlag) : 0xffffffffu;
    place[threadIdx.x] = at;
    if (stays && p.codes_in)
    {
        p.codes_out[3 * (uint64_t)at]     = p.codes_in[3 * sp.i];
        p.codes_out[3 * (uint64_t)at + 1] = p.codes_in[3 * sp.i + 1];
        p.codes_out[3 * (uint64_t)at + 2] = p.codes_in[3 * sp.i + 2];
    }
    __syncthreads();
    // a row is eight 16-byte pieces: eight neighbouring lanes move one row, a wavefront eight rows per turn
    uint4 const * const src = reinterpret_cast<uint4 const *>(p.in + sp.first);
    uint4 * const       dst = reinterpret_cast<uint4 *>(p.out);
    for (uint32_t r = threadIdx.x >> 3; r < (uint32_t)kTopBlock; r += kTopBlock / 8)
    {
        uint32_t const to = place[r];
        if (to != 0xffffffffu)
            dst[(uint64_t)to * 8 + (threadIdx.x & 7)] = src[(uint64_t)r * 8 + (threadIdx.x & 7)];
    }
}

// ---- the new ops_off: a 64-bit scan of n_ops over the rows in output order ------------------------------------------------------
constexpr int      kOpsItems = 4;
constexpr uint32_t kOpsTile  = kTopBlock * kOpsItems;

__device__ __forceinline__ uint64_t block_inclusive64(uint64_t v, uint64_t * wave_tot, uint64_t & total)
{
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t  incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
    {
        uint64_t const up = (uint64_t)__shfl_up((unsigned long long)incl, off);
        if (lane >= off)
            incl += up;
    }
    if (lane == 63)
        wave_tot[wave] = incl;
    __syncthreads();
    uint64_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kTopBlock / 64; ++w)
    {
        uint64_t const x = wave_tot[w];
        if (w < wave)
            before += x;
        tot += x;
    }
    total = tot;
    __syncthreads();
    return before + incl;
}

__device__ __forceinline__ uint64_t rows_out(TopParams const & p)
{
    return min(p.counters[kTopFinal], p.n_cap);
}

__global__ __launch_bounds__(kTopBlock) void top_ops_tile_kernel(TopParams p)
{
    __shared__ uint64_t wave_tot[kTopBlock / 64];
    uint64_t const      m = rows_out(p), t0 = (uint64_t)blockIdx.x * kOpsTile;
    uint64_t            acc = 0;
    if (t0 < m)
        for (int k = 0; k < kOpsItems; ++k)
        {
            uint64_t const j = t0 + (uint64_t)k * kTopBlock + threadIdx.x;
            if (j < m)
                acc += p.out[j].n_ops;
        }
    uint64_t total;
    (void)block_inclusive64(acc, wave_tot, total);
    if (threadIdx.x == 0)
        p.tile_ops[blockIdx.x] = total;
}

// one workgroup: the tiles' sums become what precedes each tile; the whole sum goes to the counters
__global__ __launch_bounds__(kTopBlock) void top_ops_tops_kernel(TopParams p, uint64_t tiles)
{
    __shared__ uint64_t wave_tot[kTopBlock / 64];
    uint64_t            carry = 0;
    for (uint64_t b0 = 0; b0 < tiles; b0 += kTopBlock)
    {
        uint64_t const b = b0 + threadIdx.x;
        uint64_t const v = b < tiles ? p.tile_ops[b] : 0;
        uint64_t       total;
        uint64_t const incl = block_inclusive64(v, wave_tot, total);
        if (b < tiles)
            p.tile_ops[b] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0)
        p.counters[kTopOps] = carry;
}

__global__ __launch_bounds__(kTopBlock) void top_ops_apply_kernel(TopParams p)
{
    __shared__ uint64_t wave_tot[kTopBlock / 64];
    uint64_t const      m = rows_out(p), t0 = (uint64_t)blockIdx.x * kOpsTile;
    if (t0 >= m)
        return;
    // (a thread takes kOpsItems consecutive rows, so that one workgroup scan serves the tile)
    uint64_t const j0 = t0 + (uint64_t)threadIdx.x * kOpsItems;
    uint32_t       v[kOpsItems];
    uint64_t       acc = 0;
#pragma unroll
    for (int k = 0; k < kOpsItems; ++k)
    {
        v[k] = j0 + k < m ? p.out[j0 + k].n_ops : 0u;
        acc += v[k];
    }
    uint64_t       total;
    uint64_t const incl = block_inclusive64(acc, wave_tot, total);
    uint64_t       run  = p.tile_ops[blockIdx.x] + incl - acc;
#pragma unroll
    for (int k = 0; k < kOpsItems; ++k)
    {
        if (j0 + k < m)
        {
            p.out[j0 + k].ops_off = run;
            if (p.codes_out)
                p.codes_out[3 * (j0 + k) + 1] = run;
        }
        run += v[k];
    }
}

} // namespace

namespace
{
size_t up16(size_t x)
{
    return (x + 15) & ~(size_t)15;
}
} // namespace

size_t toprec_work_bytes(uint64_t n_cap, bool max_hsps, bool culling_limit)
{
    uint64_t const tiles = l2_scan_tiles(n_cap), otiles = (n_cap + kOpsTile - 1) / kOpsTile;
    // (kernel 4: its flags; kernel 5: its flags and the two ends of the intervals)
    size_t const more = (max_hsps ? 1 : 0) + (culling_limit ? 3 : 0);
    return (4 + more) * up16(n_cap * sizeof(uint32_t)) + up16((n_cap + 1) * sizeof(uint32_t)) + up16((tiles + 1) * sizeof(uint32_t)) + up16((otiles + 1) * sizeof(uint64_t)) + 64;
}

hipError_t toprec_launch(TopParams p, void * work, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(p.counters, 0, kTopCounters * sizeof(uint64_t), stream);
    if (e != hipSuccess || p.n_cap == 0)
        return e;
    if (p.n_cap >= 0x7ffffff0ull)
        return hipErrorInvalidValue;
    uint64_t const tiles = l2_scan_tiles(p.n_cap), otiles = (p.n_cap + kOpsTile - 1) / kOpsTile;
    uint8_t *      w     = static_cast<uint8_t *>(work);
    auto           take  = [&](size_t bytes)
    {
        void * const at = w;
        w += up16(bytes);
        return at;
    };
    p.seg_id      = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
    p.r1          = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
    p.r2          = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
    p.kept_before = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
    p.seg_start   = static_cast<uint32_t *>(take((p.n_cap + 1) * sizeof(uint32_t)));
    p.block_tot   = static_cast<uint32_t *>(take((tiles + 1) * sizeof(uint32_t)));
    p.tile_ops    = static_cast<uint64_t *>(take((otiles + 1) * sizeof(uint64_t)));
    // (behind what the step always takes, so that the default path's scratch lies where it lay)
    if (p.culling_limit && !p.q_lens)
        return hipErrorInvalidValue;
    p.live_hsps = p.live = p.r1;
    if (p.max_hsps)
        p.live_hsps = p.live = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
    if (p.culling_limit)
    {
        p.live  = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
        p.iv_lo = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
        p.iv_hi = static_cast<uint32_t *>(take(p.n_cap * sizeof(uint32_t)));
    }
    dim3 const sgrid((unsigned)tiles), sblock(kL2ScanBlock), grid((unsigned)((p.n_cap + kTopBlock - 1) / kTopBlock)), block(kTopBlock);
    SegVal const sv{p};
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, SegVal>), sgrid, sblock, 0, stream, sv, p.n_cap, p.block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), sblock, 0, stream, p.block_tot, tiles);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, SegVal, SegOut>), sgrid, sblock, 0, stream, sv, SegOut{p}, p.n_cap, p.block_tot);
    hipLaunchKernelGGL(top_rank1_kernel, grid, block, 0, stream, p);
    if (p.max_hsps)
        hipLaunchKernelGGL(top_hsps_kernel, grid, block, 0, stream, p);
    if (p.culling_limit)
    {
        hipLaunchKernelGGL(top_interval_kernel, grid, block, 0, stream, p);
        hipLaunchKernelGGL(top_cull_kernel, grid, block, 0, stream, p, static_cast<uint32_t const *>(p.live_hsps));
    }
    hipLaunchKernelGGL(top_rank2_kernel, grid, block, 0, stream, p);
    KeepVal const kv{p};
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, KeepVal>), sgrid, sblock, 0, stream, kv, p.n_cap, p.block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), sblock, 0, stream, p.block_tot, tiles);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, KeepVal, KeepOut>), sgrid, sblock, 0, stream, kv, KeepOut{p}, p.n_cap, p.block_tot);
    hipLaunchKernelGGL(top_scatter_kernel, grid, block, 0, stream, p);
    if (p.rebase_ops)
    {
        hipLaunchKernelGGL(top_ops_tile_kernel, dim3((unsigned)otiles), block, 0, stream, p);
        hipLaunchKernelGGL(top_ops_tops_kernel, dim3(1), block, 0, stream, p, otiles);
        hipLaunchKernelGGL(top_ops_apply_kernel, dim3((unsigned)otiles), block, 0, stream, p);
    }
    return hipGetLastError();
}

} // namespace lx
