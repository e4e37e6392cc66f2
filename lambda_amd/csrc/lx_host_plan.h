// lx_host_plan.h -- the host plan of lx_extend_batch* and of the Level-2 driver's resident lists (lx_host_plan.cpp): which
// extensions are live, their order by query slice, the geometry classes of the one-query-per-wavefront kernels, and the
// multi-query sweep's plan -- the solo packing, or the pool + the streamed part of the free packing.  Pure CPU integer work:
// no HIP call is made here; lx_host.cpp runs the plan as a pipeline of chunks.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/lambda_ext.h"

namespace lxi
{

struct HostMarks;
struct ResidentInput;

constexpr uint64_t kWave = 16; // slots of a wavefront of the multi-query sweep

// Geometry class of a query length for the one-query-per-wavefront kernels: one panel of 104 / 152 / 200 / 208 columns, then
// two / three / ... panels of 152
inline uint32_t query_class(uint32_t lq)
{
    return lq <= 104 ? 0u : lq <= 152 ? 1u : lq <= 200 ? 2u : lq <= 208 ? 3u : 3u + (lq + 151) / 152;
}

// steps of a multi-query slot whose longest window has `maxs` rows
inline uint32_t mq_steps(uint64_t maxs) { return (uint32_t)((maxs + 8 - 1 + 15) & ~15ull); }

// Checkpoint dwords of one multi-query slot in strip geometry `cfg` (trace cfg), sized for a wavefront whose widest query sweeps
// `pan` columns per lane and whose longest window is `maxs`: int16 pairs (wide) or compact codes, per panel, + (with_ovf) an
// eighth of an int32 slot per panel -- the room a chunk keeps for the overflow slots of what the compact sweep declines
uint64_t slot_dwords(int cfg, uint64_t pan, uint64_t maxs, bool wide, bool with_ovf = false);

// Does the multi-query sweep serve this slot's lists (opt_band is NOT looked at: free_plan_applies adds it)?
bool mq_sweep_applies(lx_handle const * h, int slot);

// The host plan of one call.  It lives on the handle (lx_handle::plan), so that its vectors keep their pages between calls; the
// stages are called in this order by lx_host.cpp, which uploads the caller's list between choose() and sort() and, for the free
// packing, makes plan_stream() beside the pool's kernels.
struct HostPlan
{
    // ---- what the pipeline reads
    uint64_t              live = 0;     // extensions with both sides non-empty
    std::vector<uint32_t> idx;          // their positions in the caller's list, in plan order
    std::vector<uint8_t>  newrun;       // [live + 1]: 1 where a run of one query slice begins (the sentinel is 1)
    std::vector<uint64_t> starts;       // the positions where runs begin + the sentinel `live` (made when a stage needs them)
    bool                  use_mq = false, use_solo = false;
    int                   mq_cfg   = 1; // the multi-query sweep's strip geometry (trace cfg)
    uint64_t              mq_cells = 0; // sum q_len * s_len of the list (lx_last_extend_stats)
    uint64_t              nwf = 0, pool_wf = 0;       // wavefronts planned so far; the pool's (they come first)
    std::vector<uint32_t> plan_slot, wf_pan, wf_maxs; // caller index per slot (bit 31: filler); per wavefront: columns per lane, longest window

    // ---- the stages
    // validate the list; live extensions; order by query slice (dead extensions get score 0 -- and, unless as_list, an empty row)
    int order(lx_handle * h, lx_extension const * ext, uint64_t n, uint64_t q_bytes, uint64_t s_bytes, bool as_list, bool preplanned,
              int32_t * out_score, lx_hsp * out_hsp, uint64_t * out_ops_off, HostMarks & hm);
    // use_mq, use_solo; the geometry classes and whether a list is uniform
    int choose(lx_handle * h, int slot, ResidentInput const * ri, bool as_list);
    // the one-query-per-wavefront order (classes, then windows by length inside a run) where the plan needs it
    void sort(HostMarks & hm);
    // mq_cfg and the solo plan, or the pool of the free packing (a device plan is taken over)
    void plan_pool(ResidentInput const * ri, HostMarks & hm);
    // the streamed part of the free packing, behind the pool
    void plan_stream();
    // wavefronts [wlo, whi) of the plan into launch order: longest first
    void longest_first(uint64_t wlo, uint64_t whi);
    // before plan_stream: the streamed part's windows and runs, its widest query (columns per lane), its longest window, and the
    // checkpoint dwords of its windows in pairs, each sized for its own run (wide: int16 pairs)
    struct StreamBound
    {
        uint64_t windows = 0, runs = 0, pan = 1, maxs = 1, dwords = 0;
    };
    StreamBound stream_bound(bool wide) const;

private:
    lx_extension const * ext      = nullptr; // the call's list
    unsigned             nthreads = 1;
    bool                 preplanned = false;
    uint32_t             cls_min = ~0u, cls_max = 0; // geometry classes of the list
    bool                 ragged  = false;            // windows of one query differ in length
    // scratch
    std::vector<uint32_t> idx_tmp;
    std::vector<uint64_t> pool_at;                                // per run: first position of its pool part
    std::vector<uint32_t> run_key, run_order, run_tmp;            // the streamed runs in packing order
    std::vector<uint32_t> sb_first, sb_key, sb_order, sb_tmp;     // the pool's sub-blocks of 4 windows
    std::vector<uint8_t>  sb_cnt;
    std::vector<uint32_t> pool_pan, pool_maxs, pool_place, pool_order, pool_key, pool_tmp; // the pool's wavefronts before launch order

    void     mark_runs();
    void     run_starts();
    uint32_t mq_panels(uint32_t lq) const;
    void     choose_cfg();
    void     plan_solo(HostMarks & hm);
    void     plan_free_pool(HostMarks & hm);
    void     grow_plan(uint64_t wavefronts);
    uint64_t pack_runs(uint64_t lo, uint64_t hi, uint32_t * out_slot, uint32_t * out_pan, uint32_t * out_maxs) const;
};

} // namespace lxi
