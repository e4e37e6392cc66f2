// lx_taxfilter.hip -- the taxon filter on the device (gfx950): which subjects a list of taxa keeps (the rule of lx_tax_subject_mask,
// lx_taxfilter_host.cpp, restated over the tree lx_tax_dev_create made resident), and the stable compaction of a match list by the
// mask that comes of it.
//
// The mask, on one stream:
//   1. listed[]: one byte per taxon, cleared, then the listed taxa below n_taxa marked -- plain byte stores; duplicates write the same 1.
//   2. under[]: one lane per taxon climbs its chain (t, its parent, ... up to the first element whose parent is <= 1, and taxon 1 where
//      that parent is 1) and stops at the first listed element.  A step is one 8-byte node load and one byte load from tables that fit
//      the Infinity Cache; n_taxa x height of them are small next to anything else a search does, so the climb is not shortened by
//      what other lanes found.
//   3. words: one lane per subject ORs under[] over its taxa and applies `exclude`; the wavefront's __ballot is its mask word, stored
//      by lane 0 with an ordinary 8-byte store (lanes beyond n_s vote 0: the last word's tail); the four words' popcounts meet in LDS
//      and one atomicAdd per workgroup counts the kept subjects.
// The filter: a flag per match (bit subjId / frames of the mask), the forward sum scan of lx_scan.h (tile sums, one workgroup over
// the tiles, the apply pass) and, in the apply pass, the scatter of the kept 48-byte records to dst[exclusive sum].
//
// How a record moves: as three 16-byte loads and three 16-byte stores by the lane that owns it, not through an LDS tile.  The apply
// pass hands consecutive lanes consecutive matches, so a wavefront's three loads cover one contiguous 3 KiB of the source (each line
// is fetched once from L2 and met again in L1 by the other two loads), and its kept lanes write dst[e], dst[e + 1], ...: the
// stores of a wavefront fill one contiguous run of 48 bytes per kept lane, every store 16 bytes wide and 16-byte aligned (48 = 3 x 16,
// the blocks come from hipMalloc).  An LDS tile would turn the same bytes into 1 KiB-per-instruction stores at the price of 96 KiB
// of LDS traffic per tile and two more barriers beside the scan's own 9 KiB; the list is read once and written at most once, so the
// L2 merges the partial lines either way and the simpler form is kept.
// Bounds: listed[] and under[] have max(n_taxa, 2) bytes; every parent and every taxon of a subject is < n_taxa by lx_check_tax_tree,
// which lx_tax_dev_create runs before it uploads anything; a climb gives up after max_height + 2 steps (unreachable on such a tree;
// the host rule gives up at the same step); a match whose subject is >= n_s reads no mask word, raises the error word and counts as
// dropped -- the host side then refuses the call before anything is scattered; dst has room for the count the scan itself produced.
#include <hip/hip_runtime.h>

#include "lx_level2.h"
#include "lx_taxfilter.h"

namespace lx
{
namespace
{

#include "lx_scan.h"

using taxfilter::FilterParams;
using taxfilter::kThreads;
using taxfilter::MaskParams;

__global__ __launch_bounds__(kThreads) void tf_clear_kernel(uint8_t * listed, uint64_t n)
{
    uint64_t const i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n)
        listed[i] = 0;
}

__global__ __launch_bounds__(kThreads) void tf_mark_kernel(MaskParams p)
{
    uint64_t const i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n_list)
        return;
    uint32_t const t = p.list[i];
    if (t < p.n_taxa)
        p.listed[t] = 1;
}

__global__ __launch_bounds__(kThreads) void tf_climb_kernel(MaskParams p)
{
    uint64_t const t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= p.n_taxa)
        return;
    uint32_t const lim   = p.tree.max_height + 2;
    uint32_t       c     = (uint32_t)t;
    uint8_t        found = 0;
    for (uint32_t step = 0; step < lim; ++step)
    {
        if (p.listed[c])
        {
            found = 1;
            break;
        }
        uint32_t const par = p.tree.nodes[c].parent;
        if (par <= 1) // the chain ends here; the root belongs to it where it is the parent
        {
            found = par == 1 && p.listed[1] ? 1 : 0;
            break;
        }
        c = par;
    }
    p.under[t] = found;
}

__global__ __launch_bounds__(kThreads) void tf_subjects_kernel(MaskParams p)
{
    __shared__ uint32_t wave_cnt[kThreads / 64];
    uint64_t const      s    = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool                keep = false;
    if (s < p.n_s)
    {
        uint64_t const a = p.tree.s_tax_off[s], b = p.tree.s_tax_off[s + 1];
        bool           hit = false;
        for (uint64_t x = a; x < b && !hit; ++x)
            hit = p.under[p.tree.s_tax_ids[x]] != 0;
        keep = hit != (p.exclude != 0);
    }
    unsigned long long const word = __ballot(keep);
    if ((threadIdx.x & 63) == 0)
    {
        if (s < p.n_s) // (s is the word's first subject)
            p.words[s >> 6] = word;
        wave_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(word);
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kThreads / 64; ++w)
            sum += wave_cnt[w];
        if (sum)
            atomicAdd(p.n_kept, (unsigned long long)sum);
    }
}

// a match's flag: the mask bit of its subject
struct KeepVal
{
    uint64_t const *    m; // the list as 64-bit words, six per match; word 1 = subjId
    uint64_t const *    words;
    uint64_t            n_s;
    uint32_t            frames;
    uint32_t *          err;
    __device__ uint32_t operator()(uint64_t k) const
    {
        uint64_t const id = m[k * 6 + 1];
        uint64_t const s  = (id >> 32) == 0 ? (uint64_t)((uint32_t)id / frames) : id / frames;
        if (s >= n_s)
        {
            atomicOr(err, 1u);
            return 0u;
        }
        return (uint32_t)((words[s >> 6] >> (s & 63)) & 1ull);
    }
};
// a kept match goes to dst[what precedes it]
struct Scatter
{
    uint4 const *   src;
    uint4 *         dst;
    __device__ void operator()(uint64_t k, uint32_t incl, uint32_t excl) const
    {
        if (incl == excl)
            return;
        uint4 const * const from = src + k * 3;
        uint4 const         a = from[0], b = from[1], c = from[2];
        uint4 * const       to = dst + (uint64_t)excl * 3;
        to[0] = a;
        to[1] = b;
        to[2] = c;
    }
};

} // namespace

namespace taxfilter
{

static dim3 grid_for(uint64_t n)
{
    return dim3((unsigned)((n + kThreads - 1) / kThreads));
}

hipError_t launch_mask(MaskParams const & p, hipStream_t stream)
{
    hipError_t const e = hipMemsetAsync(p.n_kept, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess)
        return e;
    uint64_t const n_flags = p.n_taxa > 2 ? p.n_taxa : 2;
    hipLaunchKernelGGL(tf_clear_kernel, grid_for(n_flags), dim3(kThreads), 0, stream, p.listed, n_flags);
    hipLaunchKernelGGL(tf_mark_kernel, grid_for(p.n_list), dim3(kThreads), 0, stream, p);
    if (p.n_taxa)
        hipLaunchKernelGGL(tf_climb_kernel, grid_for(p.n_taxa), dim3(kThreads), 0, stream, p);
    if (p.n_s)
        hipLaunchKernelGGL(tf_subjects_kernel, grid_for(p.n_s), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

uint64_t scan_tiles(uint64_t n)
{
    return (n + kL2ScanTile - 1) / kL2ScanTile;
}

static KeepVal keep_val(FilterParams const & p)
{
    return KeepVal{reinterpret_cast<uint64_t const *>(p.src), p.words, p.n_s, p.frames, p.err};
}

hipError_t launch_count(FilterParams const & p, hipStream_t stream)
{
    hipError_t const e = hipMemsetAsync(p.err, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess)
        return e;
    uint64_t const tiles = scan_tiles(p.n);
    dim3 const     grid((unsigned)tiles), block(kL2ScanBlock);
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, KeepVal>), grid, block, 0, stream, keep_val(p), p.n, p.block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), block, 0, stream, p.block_tot, tiles);
    return hipGetLastError();
}

hipError_t launch_scatter(FilterParams const & p, hipStream_t stream)
{
    dim3 const grid((unsigned)scan_tiles(p.n)), block(kL2ScanBlock);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, KeepVal, Scatter>), grid, block, 0, stream, keep_val(p), Scatter{p.src, p.dst}, p.n, p.block_tot);
    return hipGetLastError();
}

} // namespace taxfilter
} // namespace lx
