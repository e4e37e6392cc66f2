// lx_taxfilter.h -- the taxon filter on the device: what the kernels (lx_taxfilter.hip) and their host side (lx_taxfilter_host.cpp)
// share.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lx_lca.h"

namespace lx
{
namespace taxfilter
{

constexpr uint32_t kThreads = 256; // of the mask kernels: four wavefronts, four mask words per workgroup

struct MaskParams
{
    lca::TreeView    tree;
    uint64_t         n_taxa, n_s;
    uint32_t const * list;    // [n_list] the listed taxa (none is 0)
    uint64_t         n_list;
    int32_t          exclude;
    uint8_t *        listed;  // [max(n_taxa, 2)] byte flag: the taxon is listed
    uint8_t *        under;   // [max(n_taxa, 2)] byte flag: the taxon's chain holds a listed taxon
    uint64_t *       words;   // [(n_s + 63) / 64] out
    unsigned long long * n_kept; // out (zeroed by the launch)
};
// listed[] cleared and marked, under[] by one lane per taxon, the words and their count by one lane per subject
hipError_t launch_mask(MaskParams const & p, hipStream_t stream);

struct FilterParams
{
    uint4 const *    src;       // n records of 48 bytes (lx_match), 16-byte aligned
    uint4 *          dst;       // room for the kept ones (launch_scatter)
    uint64_t         n;         // 1 .. 2^31 - 16
    uint64_t const * words;     // the mask
    uint64_t         n_s;
    uint32_t         frames;    // 1 .. 6
    uint32_t *       block_tot; // [tiles + 1] the scan's tile values; block_tot[tiles] = the kept count after launch_count
    uint32_t *       err;       // a match's subject lies beyond the mask (zeroed by launch_count)
};
uint64_t   scan_tiles(uint64_t n);
// the flags' tile sums and what precedes each tile: the kept count and the error word are there to be read
hipError_t launch_count(FilterParams const & p, hipStream_t stream);
// the flags again, scanned per tile, and the kept records written to dst in list order
hipError_t launch_scatter(FilterParams const & p, hipStream_t stream);

} // namespace taxfilter
} // namespace lx
