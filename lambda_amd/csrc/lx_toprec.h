// lx_toprec.h -- _writeRecord's sort / unique / sort / cut on device rows (lx_toprec.hip) as the host sees it.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "lx_level2.h"

namespace lx
{

enum
{
    kTopQueries   = 0, // lx_record_stats, field by field
    kTopDuplicate = 1,
    kTopAbundant  = 2,
    kTopFinal     = 3, // = rows written to `out`
    kTopPairs     = 4,
    kTopOps       = 5, // rebase_ops: the n_ops of the rows in `out` together
    kTopMaxHsps   = 6, // lx_cull_stats: rows that max_hsps dropped,
    kTopCulled    = 7, // rows that culling_limit dropped
    kTopCounters  = 8
};

struct TopParams
{
    BlastMatchDev const * in;        // rows grouped by n_qid
    BlastMatchDev *       out;       // [<= rows]; not `in`
    uint64_t const *      codes_in;  // NULL, or three words per row that travel with it (RecParams::rec_codes) ...
    uint64_t *            codes_out; // ... to here; with rebase_ops the middle word becomes the row's new ops_off
    uint64_t const *      n_ptr;     // NULL, or where the number of rows stands in device memory (at most n_cap count)
    uint64_t              n_cap;     // rows (n_ptr == NULL), else their upper bound; < 2^31 - 16
    uint64_t              max_matches;
    int                   rebase_ops; // ops_off of the rows in `out` = sum of n_ops of the rows in front (else: as it stood)
    uint64_t *            counters;  // [kTopCounters], zeroed by the launch
    // the rule of lx_cull.h between the unique and the cut; both 0: the kernels of _writeRecord alone
    uint64_t         max_hsps      = 0;
    uint64_t         culling_limit = 0;
    uint32_t const * q_lens        = nullptr; // culling_limit > 0: the untranslated length of query n_qid at q_lens[n_qid * q_len_stride]
    uint64_t         q_lens_n      = 0;       // ... of q_lens_n entries: a row beyond them gets the interval [0, 0]
    uint32_t         q_len_stride  = 1;
    int              q_translated  = 0;
    // carved out of `work` by toprec_launch (live: r1 with the flag also set for the rows that the two rules dropped)
    uint32_t * seg_id, * seg_start, * r1, * r2, * kept_before, * block_tot, * live, * live_hsps, * iv_lo, * iv_hi;
    uint64_t * tile_ops;
};

// (max_hsps, culling_limit: whether the launch will have them set; the step without them takes what it took before they existed)
size_t     toprec_work_bytes(uint64_t n_cap, bool max_hsps = false, bool culling_limit = false);
hipError_t toprec_launch(TopParams p, void * work, hipStream_t stream);

} // namespace lx
