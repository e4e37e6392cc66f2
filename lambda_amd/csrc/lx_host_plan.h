// lx_host_plan.h -- the host plan of lx_extend_batch* and of the Level-2 driver's resident lists (lx_host_plan.cpp): which
// extensions are live, their order by query slice, the geometry classes of the one-query-per-wavefront kernels, and the
// multi-query sweep's plan -- the solo packing, or the pool + the streamed part of the free packing.  Pure CPU integer work:
// no HIP call is made here; the chunk drivers (lx_xb_run.cpp, lx_xb_wf.cpp) cut the plan into chunks with the members below and run them.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/lambda_ext.h"
#include "lx_geo.h"

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

// Checkpoint dwords of one multi-query slot in strip geometry `geo`, sized for a wavefront whose widest query sweeps
// `pan` columns per lane and whose longest window is `maxs`: int16 pairs (wide) or compact codes, per panel, + (with_ovf) an
// eighth of an int32 slot per panel -- the room a chunk keeps for the overflow slots of what the compact sweep declines
uint64_t slot_dwords(lx::Geo geo, uint64_t pan, uint64_t maxs, bool wide, bool with_ovf = false);

// The budget of a multi-query chunk: its checkpoint slots' bytes within `trace_bytes` (LX_OPT_TRACE_BYTES), its survivors' ops slots
// -- `slots` of `ops_slot_bytes`, columns + rows of the chunk's widest query and longest window -- within 8 GiB.  The sites differ,
// on purpose, in what they put in: the cut of the chunks (wf_chunk_end) and the admission of ranges (ranges_admitted) size every
// slot with room for overflow slots (with_ovf) against the whole budget; ONE chunk in two calls (lx_xb_wf.cpp: two_calls) puts the
// pool's table WITHOUT overflow room against HALF the budget -- the overflow area and the second call's slots come out of the rest --
// and 16 slots + 4 bytes of margin into the ops side, since its slot count is an estimate; a redo (redo_piece_end) has wide slots
// and no overflow area, and its ops slots were admitted when the chunk was first cut (slots = 0).
inline bool chunk_fits(uint64_t slot_bytes, uint64_t trace_bytes, uint64_t slots, uint64_t ops_slot_bytes)
{
    return slot_bytes <= trace_bytes && slots * ops_slot_bytes <= (8ull << 30);
}

// Does the multi-query sweep serve this slot's lists (opt_band is NOT looked at: free_plan_applies adds it)?
bool mq_sweep_applies(lx_handle const * h, int slot);

// The host plan of one call.  It lives on the handle (lx_handle::plan), so that its vectors keep their pages between calls; the
// stages are called in this order by extend_pipeline (lx_host.cpp), which uploads the caller's list between choose() and sort(); for the
// free packing the wavefront driver (lx_xb_wf.cpp) makes plan_stream() beside the pool's kernels.
struct HostPlan
{
    // ---- what the pipeline reads
    uint64_t              live = 0;     // extensions with both sides non-empty
    std::vector<uint32_t> idx;          // their positions in the caller's list, in plan order
    std::vector<uint8_t>  newrun;       // [live + 1]: 1 where a run of one query slice begins (the sentinel is 1)
    std::vector<uint64_t> starts;       // the positions where runs begin + the sentinel `live` (made when a stage needs them)
    bool                  use_mq = false, use_solo = false;
    lx::Geo               mq_geo = lx::kGeo8x19; // the multi-query sweep's strip geometry
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
    // mq_geo and the solo plan, or the pool of the free packing (a device plan is taken over)
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

    // ---- cutting the plan into chunks (the drivers issue what is cut here)
    // checkpoint dwords of wavefront w's sixteen slots
    uint64_t wf_dwords(uint64_t w, bool wide) const { return kWave * slot_dwords(mq_geo, wf_pan[w], wf_maxs[w], wide); }
    // one-query-per-wavefront chunks: where the chunk of the ordered list that starts at k0 ends -- about chunk_target extensions, never
    // inside a query's run, never across geometry classes (the list is class-major)
    uint64_t run_chunk_end(uint64_t k0, uint64_t chunk_target) const;
    // multi-query chunks: where the chunk that starts at wavefront w0 ends -- at most per_chunk wavefronts within the budget (compact
    // codes, int16 pairs where the chunk may run wide), and (cut_at_pool) not across the end of the pool
    uint64_t wf_chunk_end(uint64_t w0, uint64_t per_chunk, uint64_t trace_bytes, bool maybe_wide, bool cut_at_pool) const;
    // a redo of wavefronts [a, end) with int16-pair slots, twice the codes': where the piece that starts at a ends
    uint64_t redo_piece_end(uint64_t a, uint64_t end, uint64_t trace_bytes) const;
    // records by range (ResidentInput::ChunkRecords): is every range [cut_wf[r], cut_wf[r + 1]) of the plan a chunk the budgets admit?
    bool ranges_admitted(uint64_t const * cut_wf, uint64_t n_ranges, uint64_t per_chunk, uint64_t trace_bytes, bool wide_ok) const;

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
