// lx_step_plan.h -- every decision about HOW a step runs: kernel family, geometry, panel count, slot layout, queries per wavefront,
// carry workspace.  Pure functions of a scheme's facts, the list's limits and the options: no handle, no HIP call.  The launchers
// (lx_step.cpp) follow these plans; lx_plan_step() shows plan_step to tests/test_plan.py.  A geometry is a Geo (lx_geo.h); what stays
// with the kernels (the .hip files) and is only declared here are the sizes of their slot layouts and of their LDS use.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lambda_ext.h"
#include "lx_geo.h"

namespace lx
{
size_t   score_pair_profile_bytes(Geo geo, int nrows);
// (these four: 0 for a geometry the kernels are not instantiated for)
int      trace_cfg_words(Geo geo);
uint64_t ckpt_slot_dwords(Geo geo, uint32_t steps_cap);
uint64_t ckpt16_slot_dwords(Geo geo, uint32_t steps_cap);
uint64_t ckpt_pair_slot_dwords(Geo geo, uint32_t steps_cap);
size_t   sweep_mq_lds_bytes(Geo geo, int nrows, int share);
} // namespace lx

namespace lxi
{
using lx::Geo;

// what lx_set_scoring derives from a scheme besides the tables (one per scoring slot; the plans decide by them): pass 2 applies
// (every matrix - gap_extend in [-31, 31]), byte profiles apply (0 <= matrix - gap_open <= 255), the largest entry
struct SchemeFacts
{
    int  alph = 0, gap_open = 0, gap_extend = 0, smax_entry = 0;
    bool trace_ok = false, b8_ok = false;
    int  nrows() const { return (alph + 1 + 3) / 4 * 4; } // rows of a query profile: the letters and the pad letter, in whole groups of 4
};
SchemeFacts scheme_facts(lx_scoring const & sc);

// What the caller of a device-list step states about the list: its widest query and longest window (0: unknown), the run of
// consecutive extensions that share a query (LX_OPT_QUERY_RUN), band mode's centres indexed like the list, the match rule of the
// backtrace (LX_OPT_BS_MATCH_RULE).  The device entry points take them from the handle's options; the pipelines from their chunks.
struct ListLimits
{
    uint64_t        max_qlen = 0, max_slen = 0, query_run = 0;
    int32_t const * band_diag = nullptr;
    uint64_t        bs_rule   = 0;
};

// ---- the rules the plans share, each written once
// compact checkpoint codes (Ckpt16Layout) hold a gap's first character up to 31
bool     compact_gaps_ok(SchemeFacts const & sc);
// checkpoint slots hold int16 pairs and address 65 535 rows
bool     fits_int16(SchemeFacts const & sc, uint64_t max_qlen, uint64_t max_slen);
// the largest value the widest admitted query can reach in a sweep of `steps` steps of G-lane groups (the kernels test per wavefront,
// on the actual query: this is the a-priori bound); beyond kCompactMaxScore the compact codes cannot hold it
int64_t  score_bound(SchemeFacts const & sc, uint64_t max_qlen, uint32_t steps, int G);
constexpr int64_t kCompactMaxScore = 2046;
// what the packed-half sweep (kHalfSweep) adds to that bound: the constant its frame is raised by so that no value of the sweep is
// negative (lx_score_f16.hip, "the biased frame"); the other families have none
int64_t  half_frame_bias(SchemeFacts const & sc, int G);
// steps of a window of max_slen rows in G-lane groups, in whole layout blocks of 16
uint32_t steps_for(uint64_t max_slen, int G);
// panels of `panel` columns that hold the query (at least one)
uint32_t panels_for(uint64_t max_qlen, int panel);
// carry pairs (8 bytes each) of n extensions wider than a panel: one per subject row
uint64_t carry_pairs(uint64_t n, uint64_t max_slen);

// ---- the geometry pickers
size_t pair_lds_limit();
Geo    pick_cfg(uint32_t qlen, bool shared);
Geo    ckpt_cfg_for(uint64_t max_q, bool packed16 = false);
Geo    mq_cfg_for(uint64_t max_q);
Geo    score_pair_cfg_for(uint32_t max_qlen);           // the packed-half geometry of pass 1 ({}: wider than any)
Geo    score_pair_cfg_for_runs_of_8(uint32_t max_qlen); // ... with 16-lane groups (8 extensions per wavefront)

// ---- pass 1 over a device list
struct ScoreOptions
{
    bool     f16  = true;
    uint64_t band = 0;
};
struct ScorePlan
{
    Geo      geo = lx::kGeo16x10;          // int32 geometry; any geometry is correct for any query length (multi-panel path)
    bool     multi = false, shared = false;
    Geo      pair_geo;                     // packed-half kernel in front of the int32 one ({}: none)
    bool     pair16 = false;               // ... or the packed 16-bit integer kernel, any query width
    int      pair_share = 0;               // lane groups per LDS profile of the packed-half kernel
    bool     narrow = false;               // band mode: (8,19) with one LDS profile per wavefront instead of the generic geometry
    uint64_t band = 0;
    bool     carry = false;                // a launch of the plan may use the carry workspace
    uint64_t max_slen = 0;
    Geo      launch_cfg() const { return band ? (narrow ? lx::kGeo8x19 : lx::kGeo16x10) : geo; }
    uint64_t carry_pairs(uint64_t n) const { return carry ? lxi::carry_pairs(n, max_slen) : 0; } // prepare_workspace's hint
};
ScorePlan plan_score(SchemeFacts const & sc, ListLimits const & lim, ScoreOptions const & o);
// the int32 geometry of a list without query runs (lx_score_batch's bins, pass 2's own pass 1)
ScorePlan plan_score_cfg(Geo geo, bool multi, bool shared, uint64_t band, Geo pair_geo = {}, bool pair16 = false);
void      describe_score(ScorePlan const & pl, char * buf, size_t len); // what lx_last_kernel_name reports

// ---- pass 2 over a device list.  share_slots = every aligned block of that many slots holds one query (0: no such guarantee); the
// 8-lane geometry puts 8 extensions in a wavefront and needs blocks of >= 4 (two LDS profiles per wavefront).
struct TraceOptions
{
    uint64_t band = 0, pass2 = 2, trace_bytes = 0;
};
struct TracePlan
{
    bool      ckpt = false;               // checkpoints (lx_ckpt.hip) instead of direction bits (lx_trace.hip)
    Geo       geo = lx::kGeo16x10;
    int       shared_profile = 0;
    uint32_t  panels_cap = 1, steps_cap = 0;
    uint64_t  stride = 0, per_ext = 0;    // uint32 / bytes of an extension's slot
    uint64_t  budget_ext = 1;             // slots the trace budget holds (the launcher sizes its chunks from this and the buffer it has)
    bool      carry = false;
    uint64_t  max_slen = 0;
    ScorePlan score;                      // pass 1 when no scores are handed in
    uint64_t  carry_pairs(uint64_t n) const { return carry ? lxi::carry_pairs(n, max_slen) : 0; }
};
TracePlan plan_trace(SchemeFacts const & sc, ListLimits const & lim, int share_slots, TraceOptions const & o);
void      describe_trace(TracePlan const & pl, char * buf, size_t len); // what lx_last_trace_kernel_name reports

// ---- the fused step
struct StepOptions
{
    uint64_t max_qlen = 0, max_slen = 0, query_run = 0, pass2 = 2, mq = 1, f16 = 1, band = 0, trace_bytes = 0, n = 0, adapt = 0;
    Geo      mq_geo;              // the strip geometry of the multi-query sweep ({}: mq_cfg_for picks)
    bool     mq_wide     = false; // the multi-query sweep writes int16-pair slots (lx_sweep_mq.hip: WIDE)
    double   surv_frac   = -1.0;
};
enum SweepFamily
{
    kNoSweep        = 0, // pass 1, then pass 2 on the survivors (modes 0 / 1)
    kHalfSweep      = 1, // lx_score_f16.hip score_pair_kernel<G,C,true>: packed half, compact codes, one panel
    kI16CompactWide = 2, // lx_score_i16.hip sweep_pair16_kernel<8,19,true,true,true>: packed int16, compact codes, several panels
    kI16Pairs       = 3, // lx_score_i16.hip sweep_pair16_kernel<G,C,MULTI>: packed int16, int16-pair slots
    kInt32Sweep     = 4, // lx_ckpt.hip ckpt_forward_kernel<G,C,false,MULTI> alone
    kMqSweep        = 5  // lx_sweep_mq.hip sweep_mq_kernel<C,MULTI>: byte profiles, up to four queries per wavefront
};
struct StepPlan
{
    bool        shared = false, sweep = false, adapted = false, compact = false, may_decline = true;
    bool        packed = false; // a packed sweep's launch structure: a spare slot behind the batch's, an overflow area for what it declines
    bool        wide   = false; // the multi-query sweep with int16-pair slots
    SweepFamily family = kNoSweep;
    Geo         geo;            // ({}: no candidate got as far as a geometry -- never a sweep)
    int         share = 0;
    uint32_t    steps = 0, panels = 1;
    uint64_t    stride = 0, stride32 = 0, ovf_cap = 0;
};
StepPlan plan_step(SchemeFacts const & sc, StepOptions const & o);
void     describe_plan(StepPlan const & pl, char * buf, size_t len);

} // namespace lxi
