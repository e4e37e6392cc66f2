// lx_lca.h -- the per-query LCA on the device: what the kernels (lx_lca.hip) and their host side (lx_lca_host.cpp) share.  Not part of
// the ABI.
//
// The tree on the device is one 8-byte node per taxon, {parent, height}: a step of a climb is one load.  The subjects' taxon lists
// keep their CSR form (64-bit offsets, 32-bit ids).  A range of the list is three columns -- n_qid (64 bits), n_sid (32 bits after the
// host's range check) and, where the top-percent rule is on, bit_score (double).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lx_resources.h"

namespace lx
{
namespace lca
{

constexpr uint32_t kFoldThreads = 256;

struct Node
{
    uint32_t parent, height;
};
static_assert(sizeof(Node) == 8, "one 8-byte load per step");

struct TreeView
{
    Node const *     nodes; // [n_taxa]
    uint64_t const * s_tax_off; // [n_s + 1]
    uint32_t const * s_tax_ids;
    uint32_t         max_height;
};

struct RangeParams
{
    TreeView         tree;
    uint64_t const * qid;  // the range's rows
    uint32_t const * sid;
    double const *   bits; // NULL: every record is kept (top_percent == 100)
    double           f;    // 1.0 - top_percent / 100.0, computed on the host
    uint32_t         n;    // rows, > 0
    uint32_t         nq;   // queries (the host counted them; the scan's total is the same number)
    uint32_t *       first;     // [nq + 1] out of the scan: a query's first row; first[nq] = n
    uint32_t *       block_tot; // [tiles + 1] the scan's tile values
    uint32_t *       out;       // [nq] the LCA words; out[nq] = the range's error word (zeroed by the launch)
};

// the scan's tiles for n rows
uint64_t scan_tiles(uint64_t n);
// the error word to 0, the query heads (a head flag and one sum scan of lx_scan.h), the fold: one lane per query
hipError_t launch_range(RangeParams const & p, hipStream_t stream);

} // namespace lca
} // namespace lx

// a tree resident on its handle's device (lx_lca_host.cpp makes it; lx_taxfilter_host.cpp reads it too)
struct lx_tax_dev
{
    lx_handle *                  h = nullptr;
    uint64_t                     n_taxa = 0, n_s = 0;
    uint32_t                     max_height = 0;
    lxi::DevBlock<lx::lca::Node> d_nodes;
    lxi::DevBlock<uint64_t>      d_off;
    lxi::DevBlock<uint32_t>      d_ids;
    ~lx_tax_dev();
};
