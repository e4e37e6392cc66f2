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
    // carved out of `work` by toprec_launch
    uint32_t * seg_id, * seg_start, * r1, * r2, * kept_before, * block_tot;
    uint64_t * tile_ops;
};

size_t     toprec_work_bytes(uint64_t n_cap);
hipError_t toprec_launch(TopParams p, void * work, hipStream_t stream);

} // namespace lx
