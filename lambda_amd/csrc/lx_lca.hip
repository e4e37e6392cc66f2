// lx_lca.hip -- the LCA step of _writeRecord (src/search_algo.hpp:884-907, computeLCA: src/search_misc.hpp:86-112) on the device
// (gfx950), for one range of whole queries whose columns lx_lca_host.cpp has uploaded: the rule of lx_compute_lca_ex
// (host/lx_postprocess.cpp), restated.
//
// Per range, on one stream:
//   1. heads: a row is a query's head if it is the first of the range or its n_qid differs from the row's before it; one sum scan of
//      the flags (lx_scan.h) numbers the queries and leaves every query's first row, as the record writers find their groups.
//   2. fold: one lane per query walks its rows in list order -- the best bit score where the top-percent rule is on, the starter
//      loop, the fold of every assigned taxon of every kept record.  The walk is a chain of dependent 8-byte loads ({parent, height}
//      side by side) from a table that fits the Infinity Cache: it is latency-bound, so what counts is the number of queries in
//      flight, not what a lane does; 256 lanes per workgroup and a handful of registers leave the occupancy to the grid.
// Bounds: first[q] < first[q + 1] <= n by the scan (checked: a range that breaks it raises the error word and reads nothing); sid[k] <
// n_s by the host's check of every row; the taxon lists, their ids and every parent lie inside the tree by lx_check_tax_tree, which
// lx_tax_dev_create runs before it uploads anything.  Every loop is bounded: the rows of a query, a subject's taxa, and the three loops
// of a climb, each of which gives up after max_height + 2 steps and raises the error word -- unreachable on a tree the check admits.
#include <hip/hip_runtime.h>

#include "lx_lca.h"
#include "lx_level2.h"

namespace lx
{
namespace
{

#include "lx_scan.h"

using lca::kFoldThreads;
using lca::Node;
using lca::RangeParams;
using lca::TreeView;

enum : uint32_t
{
    kErrNoRoot = 1, // "One of the paths didn't lead to root."
    kErrBound  = 2, // a climb did not end within max_height + 2 steps
    kErrRange  = 4  // a query without rows, or rows beyond the range
};

struct HeadVal
{
    uint64_t const *    qid;
    __device__ uint32_t operator()(uint64_t k) const { return k == 0 || qid[k] != qid[k - 1] ? 1u : 0u; }
};
struct HeadOut
{
    uint32_t *      first;
    uint64_t        n;
    __device__ void operator()(uint64_t k, uint32_t incl, uint32_t excl) const
    {
        if (incl != excl)
            first[incl - 1] = (uint32_t)k;
        if (k == n - 1)
            first[incl] = (uint32_t)n;
    }
};

// computeLCA (src/search_misc.hpp:86-112) as lca_of of host/lx_postprocess.cpp has it: level the two nodes, then climb together.  false:
// the paths never met (err gets kErrNoRoot) or a loop hit its bound (kErrBound).
__device__ __forceinline__ bool lca_of(TreeView const & t, uint32_t n1, uint32_t n2, uint32_t & out, uint32_t & err)
{
    if (n1 == n2)
    {
        out = n1;
        return true;
    }
    uint32_t const lim = t.max_height + 2;
    Node           a = t.nodes[n1], b = t.nodes[n2];
    uint32_t       steps = 0;
    for (uint32_t i = a.height; i > b.height; --i)
    {
        if (++steps > lim)
        {
            err |= kErrBound;
            return false;
        }
        n1 = a.parent;
        a  = t.nodes[n1];
    }
    steps = 0;
    for (uint32_t i = b.height; i > a.height; --i)
    {
        if (++steps > lim)
        {
            err |= kErrBound;
            return false;
        }
        n2 = b.parent;
        b  = t.nodes[n2];
    }
    steps = 0;
    while (n1 != 0 && n2 != 0)
    {
        if (n1 == n2)
        {
            out = n1;
            return true;
        }
        if (++steps > lim)
        {
            err |= kErrBound;
            return false;
        }
        n1 = a.parent;
        n2 = b.parent;
        a  = t.nodes[n1];
        b  = t.nodes[n2];
    }
    err |= kErrNoRoot;
    return false;
}

__global__ __launch_bounds__(kFoldThreads) void lca_fold_kernel(RangeParams p)
{
    uint32_t const q = blockIdx.x * kFoldThreads + threadIdx.x;
    if (q >= p.nq)
        return;
    uint32_t const lo = p.first[q], hi = p.first[q + 1];
    if (lo >= hi || hi > p.n)
    {
        atomicOr(&p.out[p.nq], (uint32_t)kErrRange);
        return;
    }
    TreeView const & t    = p.tree;
    bool const       all  = p.bits == nullptr;
    double           best = 0.0, cut = 0.0;
    if (!all)
    {
        best = p.bits[lo];
        for (uint32_t k = lo + 1; k < hi; ++k)
        {
            double const v = p.bits[k];
            best           = v > best ? v : best;
        }
        cut = best * p.f; // (one multiplication, as on the host)
    }
    auto const kept = [&](uint32_t k)
    {
        if (all)
            return true;
        double const v = p.bits[k];
        return v >= cut || v == best;
    };
    // the first kept record whose subject's first taxon is assigned (has a parent) starts the fold (:887-896)
    uint32_t lca = 0;
    for (uint32_t k = lo; k < hi && lca == 0; ++k)
    {
        if (!kept(k))
            continue;
        uint32_t const s = p.sid[k];
        uint64_t const a = t.s_tax_off[s], b = t.s_tax_off[s + 1];
        if (b > a)
        {
            uint32_t const first = t.s_tax_ids[a];
            if (t.nodes[first].parent != 0)
                lca = first;
        }
    }
    uint32_t err = 0;
    if (lca != 0) // every assigned taxon of every kept record (:898-906); unassigned ones are ignored
        for (uint32_t k = lo; k < hi && err == 0; ++k)
        {
            if (!kept(k))
                continue;
            uint32_t const s = p.sid[k];
            uint64_t const a = t.s_tax_off[s], b = t.s_tax_off[s + 1];
            for (uint64_t x = a; x < b && err == 0; ++x)
            {
                uint32_t const tax = t.s_tax_ids[x];
                if (t.nodes[tax].parent != 0)
                    (void)lca_of(t, tax, lca, lca, err);
            }
        }
    p.out[q] = err ? 0u : lca;
    if (err)
        atomicOr(&p.out[p.nq], err);
}

} // namespace

namespace lca
{

uint64_t scan_tiles(uint64_t n)
{
    return (n + kL2ScanTile - 1) / kL2ScanTile;
}

hipError_t launch_range(RangeParams const & p, hipStream_t stream)
{
    if (p.n == 0 || p.nq == 0)
        return hipSuccess;
    hipError_t const e = hipMemsetAsync(p.out + p.nq, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess)
        return e;
    uint64_t const tiles = scan_tiles(p.n);
    dim3 const     grid((unsigned)tiles), block(kL2ScanBlock);
    HeadVal const  hv{p.qid};
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, HeadVal>), grid, block, 0, stream, hv, (uint64_t)p.n, p.block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), block, 0, stream, p.block_tot, tiles);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, HeadVal, HeadOut>), grid, block, 0, stream, hv, HeadOut{p.first, p.n}, (uint64_t)p.n, p.block_tot);
    hipLaunchKernelGGL(lca_fold_kernel, dim3((p.nq + kFoldThreads - 1) / kFoldThreads), dim3(kFoldThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace lca
} // namespace lx
