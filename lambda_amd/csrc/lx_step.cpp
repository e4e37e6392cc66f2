// lx_step.cpp -- the launchers of the device-list steps: pass 1 (launch_score_list, score_dev_impl), pass 2 (align_dev_impl) and the
// fused step (fused_impl: sweep or pass 1 -> survivor selection -> backtrace or pass 2, all on the device).  What runs is decided in
// lx_step_plan.cpp; the functions here size the handle's buffers for a plan, fill the kernels' parameter blocks and launch.
#include "lx_internal.h"

using namespace lxi;

ListLimits lxi::option_limits(lx_handle const * h)
{
    return ListLimits{h->opt_max_qlen, h->opt_max_slen, h->opt_query_run, h->band_dev, h->opt_bs_rule};
}

ScoreOptions lxi::score_options(lx_handle const * h)
{
    return ScoreOptions{h->opt_f16 != 0, h->opt_band};
}

TraceOptions lxi::trace_options(lx_handle const * h)
{
    return TraceOptions{h->opt_band, h->opt_pass2, h->opt_trace_bytes};
}

int lxi::prepare_workspace(lx_handle * h, hipStream_t stream, uint64_t pairs_hint)
{
    uint64_t const want = std::min<uint64_t>(pairs_hint, 0xfffffff0ull) * 8 + 4096;
    if (pairs_hint != 0 && want > h->ws_grown)
        h->ws_grown = want;
    int rc = ensure(h, h->d_ws, std::max(h->opt_ws_bytes, h->ws_grown));
    if (rc)
        return rc;
    LX_HIP(h, hipMemsetAsync(ws_word(h, kWsBump), 0, 2 * sizeof(uint32_t), stream)); // (kWsBump and kWsError)
    return LX_OK;
}

// a launch that carries starts with an empty carry workspace
static hipError_t reset_carry(lx_handle * h, hipStream_t stream)
{
    return hipMemsetAsync(ws_word(h, kWsBump), 0, sizeof(uint32_t), stream);
}

// ---- the kernels' parameter blocks ---------------------------------------------------------------------------------------------

// What every TraceParams of the handle shares: the residues, the scheme, the trace buffer and end cells as they stand, the carry
// workspace, the error word, the backtrace's queue.  The caller adds its list's layout and outputs.
static lx::TraceParams trace_params(lx_handle * h, int slot, void const * d_q, void const * d_s, lx::Extension const * ext, uint64_t n, ListLimits const & lim)
{
    lx::TraceParams p{};
    p.q_res         = static_cast<uint8_t const *>(d_q);
    p.s_res         = static_cast<uint8_t const *>(d_s);
    p.ext           = ext;
    p.n             = n;
    p.sc            = h->sc_dev[slot];
    p.trace         = static_cast<uint32_t *>(h->d_trace.ptr);
    p.ends          = static_cast<lx::EndCell *>(h->d_ends.ptr);
    p.ws            = static_cast<int32_t *>(h->d_ws.ptr);
    p.ws_top        = ws_word(h, kWsBump);
    p.ws_cap        = (uint32_t)std::min<uint64_t>(h->d_ws.cap / 8, 0xffffffffu);
    p.err           = ws_error(h);
    p.nrows         = h->facts[slot].nrows();
    p.bs_match_rule = (int32_t)lim.bs_rule;
    p.work_counter  = ws_word(h, kWsWorkQueue);
    return p;
}

// the ScoreParams of a pass-1 launch over the list of `t` (carry: it may go panel by panel through the carry workspace)
static lx::ScoreParams score_params(lx::TraceParams const & t, int32_t * out_score, bool carry)
{
    lx::ScoreParams sp{};
    sp.q_res     = t.q_res;
    sp.s_res     = t.s_res;
    sp.ext       = t.ext;
    sp.n         = t.n;
    sp.sc        = t.sc;
    sp.out_score = out_score;
    sp.err       = t.err;
    sp.nrows     = t.nrows;
    if (carry)
    {
        sp.ws         = t.ws;
        sp.ws_top     = t.ws_top;
        sp.ws_cap     = t.ws_cap;
        sp.panels_cap = t.panels_cap;
    }
    return sp;
}

// ... of a packed sweep: it also writes the checkpoint slots and end cells of the checkpoint launch `t` of the same step
static lx::ScoreParams sweep_params(lx::TraceParams const & t, bool carry)
{
    lx::ScoreParams sp = score_params(t, t.score_out, carry);
    sp.ckpt            = t.trace;
    sp.ckpt_stride     = t.slot_stride;
    sp.steps_cap       = t.steps_cap;
    sp.ends            = t.ends;
    return sp;
}

// ---- pass 1 ------------------------------------------------------------------------------------------

// One kernel sequence for a device-resident extension list whose queries all fit the plan's geometry (or need the multi-panel
// path when wider).
int lxi::launch_score_list(lx_handle * h, int slot, void const * d_q, void const * d_s, void const * d_ext, uint64_t n, void * d_out,
                           ScorePlan const & pl, hipStream_t stream, int32_t const * band_diag)
{
    lx::ScoreParams p = score_params(trace_params(h, slot, d_q, d_s, static_cast<lx::Extension const *>(d_ext), n, ListLimits{}), static_cast<int32_t *>(d_out), true);
    p.shared_profile  = pl.shared ? 1 : 0;
    p.pair_share      = pl.pair_share;
    if (pl.band)
    {
        p.band           = (int32_t)pl.band;
        p.band_diag      = band_diag;
        p.shared_profile = pl.narrow ? 1 : 0;
        LX_HIP(h, lx::launch_score(pl.launch_cfg(), p, true, stream));
    }
    else if (pl.pair16)
    {
        // queries wider than the packed-half geometries: packed 16-bit integers (lx_score_i16.hip), panel by panel; what
        // fails its range test is left to the int32 kernel, which starts with an empty carry workspace
        LX_HIP(h, lx::launch_score_pair16(p, stream));
        LX_HIP(h, reset_carry(h, stream));
        p.fixup = 1;
        LX_HIP(h, lx::launch_score(pl.geo, p, pl.multi, stream));
    }
    else if (pl.pair_geo.chosen())
    {
        // packed-half kernel first (two extensions per lane group); wavefronts whose score bound does not fit half
        // precision leave the sentinel -1, which the int32 kernel then resolves in fix-up mode
        LX_HIP(h, lx::launch_score_pair(pl.pair_geo, p, stream));
        p.fixup = 1;
        LX_HIP(h, lx::launch_score(pl.geo, p, pl.multi, stream));
    }
    else
        LX_HIP(h, lx::launch_score(pl.geo, p, pl.multi, stream));
    char buf[128];
    describe_score(pl, buf, sizeof(buf));
    h->last_kernel = buf;
    return LX_OK;
}

int lxi::score_dev_impl(lx_handle * h, int slot, void const * d_q, void const * d_s, void const * d_ext, uint64_t n, void * d_out,
                        hipStream_t stream, ListLimits const & lim)
{
    ScorePlan const pl = plan_score(h->facts[slot], lim, score_options(h));
    PhaseTimer      pt(h, stream, 0);
    int const       rc = launch_score_list(h, slot, d_q, d_s, d_ext, n, d_out, pl, stream, lim.band_diag);
    if (rc)
        return rc;
    pt.close();
    return LX_OK;
}


// ---- pass 2 ------------------------------------------------------------------------------------------

// Runs pass 2 over a device-resident list of `n` extension slots, in chunks sized to the trace budget.
// src / d_count are set by the fused path (slots compacted by launch_select): results are then written to
// out_hsp[src[slot]] / ops_off[src[slot]] and slots beyond *d_count are skipped on the device.
int lxi::align_dev_impl(lx_handle * h, int slot, void const * d_q, void const * d_s, lx::Extension const * d_ext,
                        uint64_t n, lx::Hsp * d_hsp, uint8_t * d_ops, uint64_t const * d_ops_off, hipStream_t stream,
                        ListLimits const & lim, int share_slots, uint32_t const * d_src, uint64_t const * d_count,
                        int32_t const * d_score_in, bool by_pos, uint64_t ops_stride)
{
    if (!h->facts[slot].trace_ok)
        return fail(h, LX_EINVAL, "pass 2 needs every (matrix entry - gap_extend) in [-31, 31]");
    if ((reinterpret_cast<uintptr_t>(d_q) | reinterpret_cast<uintptr_t>(d_s)) & 15)
        return fail(h, LX_EINVAL, "pass 2 reads residues in aligned 16-byte groups: the residue buffers must be 16-byte aligned");
    if (lim.max_slen > (uint64_t)lx::kMaxTraceRows)
        return fail(h, LX_EINVAL, "pass 2 supports subject windows up to %d residues (got %llu)", lx::kMaxTraceRows, (unsigned long long)lim.max_slen);
    TracePlan const pl = plan_trace(h->facts[slot], lim, share_slots, trace_options(h));
    // The forward kernel finds the end cell cheaply when it knows each extension's best score; the fused path hands
    // over pass 1's scores, a stand-alone traceback call computes them first (a fraction of the traceback's cost).
    if (!d_score_in)
    {
        int rc0;
        if ((rc0 = ensure(h, h->d_trace_score, n * sizeof(int32_t))))
            return rc0;
        if ((rc0 = launch_score_list(h, slot, d_q, d_s, d_ext, n, h->d_trace_score.ptr, pl.score, stream, lim.band_diag)))
            return rc0;
        d_score_in = static_cast<int32_t const *>(h->d_trace_score.ptr);
    }
    // One trace buffer, forward kernel and backtrace of a chunk one after the other on `stream`: a chunk may use the whole budget --
    // as few launches (and kernel tails) as the budget allows.  (A backtrace on a second stream beside the next chunk's forward
    // kernel was measured on config 2: 46.9 against 46.5 ms per step -- both kernels saturate the chip -- and is gone.)  In the fused
    // path `n` is the capacity of the survivor list; launches beyond the device-side count exit at once.
    uint64_t chunk = std::min<uint64_t>(pl.budget_ext, n + 8);
    // a trace buffer that is already there and holds a fair chunk is used as it is: the fused step sizes this list for the
    // worst case (every extension survives), and growing a buffer of tens of GB costs seconds -- the adaptive mode-1 step
    // after a run of single sweeps would pay that once; chunks beyond the device-side count exit at once
    if (d_count && h->d_trace.cap / std::max<uint64_t>(pl.per_ext, 1) >= 65536)
        chunk = std::min<uint64_t>(chunk, h->d_trace.cap / pl.per_ext / 8 * 8);
    chunk = std::max<uint64_t>(8, (chunk + 7) / 8 * 8);
    int rc;
    if ((rc = ensure(h, h->d_trace, chunk * pl.per_ext)) || (rc = ensure(h, h->d_ends, chunk * sizeof(lx::EndCell))))
        return rc;
    bool const by_src = d_src && !by_pos; // records and ops slots are addressed through src, not by the position in the chunk
    for (uint64_t c0 = 0; c0 < n; c0 += chunk)
    {
        lx::TraceParams p = trace_params(h, slot, d_q, d_s, d_ext + c0, std::min<uint64_t>(chunk, n - c0), lim);
        p.slot_stride     = pl.stride;
        p.steps_cap       = pl.steps_cap;
        p.panels_cap      = pl.panels_cap;
        p.out_hsp         = by_src ? d_hsp : d_hsp + c0;
        p.out_ops         = d_ops;
        p.ops_off         = !d_ops_off ? nullptr : by_src ? d_ops_off : d_ops_off + c0;
        p.ops_stride      = ops_stride;
        if (!d_ops_off && !by_src && c0 != 0) // uniform slots are addressed by the index inside the chunk
            p.out_ops = d_ops + c0 * ops_stride;
        p.out_by_pos     = by_pos ? 1 : 0;
        p.src            = d_src ? d_src + c0 : nullptr;
        p.score_in       = d_score_in + c0;
        p.count_ptr      = d_count;
        p.chunk_start    = c0;
        p.band           = (int32_t)h->opt_band;
        p.band_diag      = lim.band_diag ? (d_src ? lim.band_diag : lim.band_diag + c0) : nullptr; // indexed like the caller's list
        p.shared_profile = pl.shared_profile;
        p.geo            = pl.geo;
        if (pl.panels_cap > 1) // each chunk starts with an empty carry workspace
            LX_HIP(h, reset_carry(h, stream));
        PhaseTimer ptf(h, stream, 2);
        LX_HIP(h, pl.ckpt ? lx::launch_ckpt_forward(p, stream) : lx::launch_trace_forward(p, stream));
        ptf.close();
        PhaseTimer ptb(h, stream, 3);
        LX_HIP(h, pl.ckpt ? lx::launch_ckpt_backtrace(p, stream) : lx::launch_backtrace(p, stream));
        ptb.close();
        char buf[96];
        describe_trace(pl, buf, sizeof(buf));
        h->last_trace_kernel = buf;
    }
    return LX_OK;
}


// ---- fused: pass 1 -> survivor selection -> pass 2, all on the device ------------------------------------

namespace
{

// One call of the fused step on its way through the stages below.
struct StepCtx
{
    lx_handle *         h;
    int                 slot;
    StepCall const &    c;
    SchemeFacts const & facts;
    hipStream_t         stream;
    StepPlan            plan{};
    bool                tab_on = false;             // the chunk's slots are by wavefront (MqTab) and the multi-query sweep takes them
    uint64_t            batch_dw = 0, tab_ovf_dw = 0; // uint32 of the batch's slots in front of the overflow area / of that area (slots by wavefront)
    uint32_t            run = 1, pad_to = 1;        // survivor selection: extensions per query run, slots a run's survivors are padded to
    uint64_t            nruns = 0, cap = 0;         // ... runs, capacity of the survivor list
    int                 share_slots() const { return plan.shared ? (int)pad_to : 0; } // what pass 2 may rely on in the survivor list
};

// How this call runs: plan_step() decides, the stages follow.  A chunk with slots by wavefront is planned for its maxima (family,
// geometry, multi-panel or not, layout of the overflow slots; the slots themselves are the table's); the second of a chunk's two
// calls goes on behind the first one's events.
int plan_for_call(StepCtx & x)
{
    lx_handle * const h   = x.h;
    StepCall const &  c   = x.c;
    MqTab const &     tab = c.tab; // (slots by wavefront: lx_extend_batch's multi-query chunks)
    x.tab_on              = tab.dev != nullptr;
    if (!(x.tab_on && tab.part == 2))
    {
        if (!c.keep_events)
        {
            h->phase_ev.clear();
            h->ev_pool_used = 0;
        }
        LX_HIP(h, hipEventRecord(h->ev0, x.stream));
    }
    StepOptions so{};
    so.max_qlen = c.lim.max_qlen, so.max_slen = c.lim.max_slen, so.query_run = c.lim.query_run, so.pass2 = h->opt_pass2;
    so.mq = h->opt_mq, so.f16 = h->opt_f16, so.band = h->opt_band, so.trace_bytes = h->opt_trace_bytes, so.n = c.n;
    so.mq_geo = c.mq_geo, so.adapt = h->opt_adapt, so.mq_wide = c.mq_wide, so.surv_frac = h->surv_frac;
    if (x.tab_on)
    {
        so.n   = 1;
        x.plan = plan_step(x.facts, so);
        so.n   = c.n;
        if (x.plan.family == kMqSweep)
            x.plan.ovf_cap = (x.plan.may_decline && x.plan.stride32 != 0) ? tab.ovf_cap : 0;
        else if (tab.part != 0)
            return fail(h, LX_ESTATE, "a chunk swept in two calls must be the multi-query sweep's");
        else // (a chunk the sweep does not take -- a window beyond the 65 535 rows its slots address: the per-survivor paths, as without a table)
            x.tab_on = false;
    }
    if (!x.tab_on)
        x.plan = plan_step(x.facts, so);
    StepPlan const & plan = x.plan;
    // the batch's slots (+ the spare slot of the compact layouts; whole wavefronts of slots when they are interleaved: the packed-half
    // sweep of one-panel queries interleaves the compact slots of a wavefront's windows -- ScoreParams::wave_slots --, so that what
    // one store instruction writes is one contiguous piece: headline sweep 11.87 -> 11.6 ms)
    // (slots by wavefront: [the wavefronts before slot n0][overflow slots][the wavefronts from n0 on])
    uint64_t const wave_w = plan.family == kHalfSweep ? 128 / (uint64_t)plan.geo.g : 1; // windows of a packed-half wavefront
    x.tab_ovf_dw          = x.tab_on ? plan.ovf_cap * plan.stride32 : 0;
    x.batch_dw            = x.tab_on                     ? tab.dw0
                            : plan.family == kHalfSweep ? (c.n + wave_w - 1) / wave_w * wave_w * plan.stride
                            : plan.packed               ? (c.n + 1) * plan.stride
                                                        : c.n * plan.stride;
    // the survivor list: runs padded to whole wavefronts -- half a wavefront of the 8-lane geometry, a whole one of the 16-lane; the
    // single sweep's backtrace needs no padding (the adaptive step has few survivors, one or two to a query: its lists pad every
    // query's to 2 slots -- four LDS profiles per wavefront of the int32 forward kernel -- instead of 4: 2.6 x -> 1.9 x the
    // survivors' cells at 2 % survivors)
    x.run    = plan.shared ? (uint32_t)c.lim.query_run : 1u;
    x.pad_to = (plan.shared && !plan.sweep) ? (plan.adapted ? 2u : 4u) : 1u;
    x.nruns  = (c.n + x.run - 1) / x.run;
    x.cap    = (c.n + (plan.shared ? x.nruns * 3 : 0) + 7) / 8 * 8;
    return LX_OK;
}

// The single sweep over all of the call's extensions: the launches of the plan's family, then the int32 fix-up launch where the plan
// says so.  A chunk swept in two calls (tab.part 1, then 2): the first call sizes the buffers, resets the counters and sweeps the
// slots before n0 -- first_part_only: the rest of the chunk is still being planned, the second call goes on from here --, the second
// sweeps the rest (the first one's sweep may still be running: nothing is sized or reset) and what follows a sweep covers all slots.
int sweep_stage(StepCtx & x, bool & first_part_only)
{
    lx_handle * const h      = x.h;
    StepCall const &  c      = x.c;
    StepPlan const &  plan   = x.plan;
    MqTab const &     tab    = c.tab;
    hipStream_t const stream = x.stream;
    uint64_t const    n      = c.n;
    bool const        second = x.tab_on && tab.part == 2;
    uint64_t const    need_dw = x.tab_on ? std::max(tab.total_dw, tab.dw0 + x.tab_ovf_dw + tab.dw1) : x.batch_dw + plan.ovf_cap * plan.stride32;
    int               rc;
    if (second)
    {
        if (need_dw * 4 > h->d_trace.cap)
            return fail(h, LX_ESTATE, "the second sweep of a chunk needs more slot memory than its first reserved");
    }
    else
    {
        if ((rc = ensure(h, h->d_trace, need_dw * 4)) || (rc = ensure(h, h->d_ends, n * sizeof(lx::EndCell))) ||
            (rc = prepare_workspace(h, stream, plan.panels > 1 ? carry_pairs(n, c.lim.max_slen) : 0)))
            return rc;
        LX_HIP(h, hipMemsetAsync(ws_word(h, kWsOvfCount), 0, sizeof(uint32_t), stream));
    }
    lx::TraceParams p = trace_params(h, x.slot, c.d_q, c.d_s, static_cast<lx::Extension const *>(c.d_ext), n, c.lim);
    p.slot_stride     = plan.stride;
    p.steps_cap       = plan.steps;
    p.panels_cap      = plan.panels;
    p.score_out       = static_cast<int32_t *>(c.d_out_score);
    // every wavefront holds one query (the multi-query sweep: every run; the solo packing: every window its own)
    p.shared_profile  = plan.family == kMqSweep ? (plan.share < 0 ? 1 : std::min(2 * plan.share, 8)) : plan.geo.groups();
    p.geo             = plan.geo;
    if (plan.packed)
    {
        p.ovf        = p.trace + x.batch_dw;
        p.ovf_stride = plan.stride32;
        p.ovf_cap    = (uint32_t)plan.ovf_cap;
        p.ovf_count  = ws_word(h, kWsOvfCount);
    }
    PhaseTimer pt0(h, stream, 0);
    switch (plan.family)
    {
        case kMqSweep:
        {
            lx::ScoreParams sp = sweep_params(p, true);
            sp.pair_share      = std::max(plan.share, 0);
            if (x.tab_on)
            {
                sp.wf_tab = static_cast<lx::WfSlots const *>(tab.dev);
                sp.wf_lo  = tab.part == 2 ? (uint32_t)(tab.n0 / 16) : 0u;
                sp.n      = tab.part == 1 ? tab.n0 : n;
                sp.ckpt   = tab.part == 2 ? p.trace + tab.dw0 + x.tab_ovf_dw : p.trace;
            }
            sp.wide        = plan.wide ? 1 : 0;
            sp.stat_beyond = ws_word(h, kWsStatBeyond);
            if (!second)
                LX_HIP(h, hipMemsetAsync(ws_word(h, kWsStatBeyond), 0, sizeof(uint32_t), stream));
            if (plan.share < 0) // the solo packing: rows for the alphabet's letters and the pad letter, no more
            {
                sp.solo  = 1;
                sp.nrows = x.facts.alph + 1;
            }
            sp.narrow = 1;
            LX_HIP(h, lx::launch_sweep_mq(plan.geo, sp, stream));
            if (x.tab_on && tab.part == 1)
            {
                pt0.close();
                first_part_only = true;
                return LX_OK;
            }
            if (plan.panels > 1) // (the fix-up launch carries)
                LX_HIP(h, reset_carry(h, stream));
            p.fixup = 1;
            break;
        }
        case kI16CompactWide:
        {
            lx::ScoreParams sp = sweep_params(p, true);
            sp.pair_share      = std::max(plan.share, 0);
            LX_HIP(h, lx::launch_sweep_pair16_compact(plan.geo, sp, stream));
            LX_HIP(h, reset_carry(h, stream)); // (the fix-up launch carries)
            p.fixup = 1;
            break;
        }
        case kHalfSweep:
        {
            lx::ScoreParams sp = sweep_params(p, false); // (always one panel)
            sp.pair_share      = std::max(plan.share, 0);
            sp.wave_slots      = 1;
            LX_HIP(h, lx::launch_score_pair(plan.geo, sp, stream));
            p.fixup = 1;
            break;
        }
        case kI16Pairs:
            LX_HIP(h, lx::launch_sweep_pair16(plan.geo, sweep_params(p, true), stream));
            if (plan.panels > 1) // (the fix-up launch carries)
                LX_HIP(h, reset_carry(h, stream));
            p.fixup = 1;
            break;
        default: break; // kInt32Sweep: the checkpoint forward kernel alone
    }
    if (!plan.packed || plan.may_decline) // (the packed-half kernel declines nothing when even the worst query passes its test)
        LX_HIP(h, lx::launch_ckpt_forward(p, stream));
    pt0.close();
    char buf[200];
    describe_plan(plan, buf, sizeof(buf));
    h->last_kernel       = buf;
    h->last_trace_kernel = buf;
    return LX_OK;
}

// No sweep: pass 1 (src/search_algo.hpp:1246).  Pass 2 may need the carry workspace even where pass 1 does not (its panels
// are narrower): size it now, while nothing is in flight
int pass1_stage(StepCtx & x)
{
    lx_handle * const h = x.h;
    StepCall const &  c = x.c;
    TracePlan const   tp = plan_trace(x.facts, c.lim, x.share_slots(), trace_options(h));
    int               rc;
    if (tp.carry && (rc = prepare_workspace(h, x.stream, tp.carry_pairs(c.n))))
        return rc;
    if ((rc = prepare_workspace(h, x.stream, plan_score(x.facts, c.lim, score_options(h)).carry_pairs(c.n))))
        return rc;
    return score_dev_impl(h, x.slot, c.d_q, c.d_s, c.d_ext, c.n, c.d_out_score, x.stream, c.lim);
}

// filter (src/search_algo.hpp:1251-1283) as an integer cut-off, compaction in input order, runs padded to whole wavefronts
int select_stage(StepCtx & x)
{
    lx_handle * const h = x.h;
    StepCall const &  c = x.c;
    int               rc;
    if ((rc = ensure(h, h->d_sel_ext, x.cap * sizeof(lx_extension))) || (rc = ensure(h, h->d_sel_src, x.cap * sizeof(uint32_t))) ||
        (rc = ensure(h, h->d_sel_runs, (x.nruns + 2 * lx::select_blocks(x.pad_to <= 1 ? c.n : x.nruns) + 2) * sizeof(uint64_t))) ||
        (rc = ensure(h, h->d_sel_score, x.cap * sizeof(int32_t))))
        return rc;
    lx::SelectParams sp{};
    sp.ext           = static_cast<lx::Extension const *>(c.d_ext);
    sp.score         = static_cast<int32_t const *>(c.d_out_score);
    sp.min_score     = static_cast<int32_t const *>(c.d_min_score);
    sp.min_score_all = c.min_score_all;
    sp.n             = c.n;
    sp.run           = x.run;
    sp.pad_to        = x.pad_to;
    sp.run_slots     = static_cast<uint64_t *>(h->d_sel_runs.ptr);
    sp.block_tot     = sp.run_slots + x.nruns;
    sp.out_ext       = static_cast<lx::Extension *>(h->d_sel_ext.ptr);
    sp.out_src       = static_cast<uint32_t *>(h->d_sel_src.ptr);
    sp.out_score     = static_cast<int32_t *>(h->d_sel_score.ptr);
    sp.out_count     = static_cast<uint64_t *>(c.d_out_count);
    sp.out_hsp       = c.by_pos ? nullptr : static_cast<lx::Hsp *>(c.d_out_hsp); // rows of the filtered-out extensions
    PhaseTimer pts(h, x.stream, 1);
    LX_HIP(h, lx::launch_select(sp, x.stream));
    pts.close();
    return LX_OK;
}

// after the backtrace (records and slots by list position): the survivors' ops as run-length codes, the list's original
// indices next to them
int fused_pack(StepCtx & x, bool packed_already)
{
    lx_handle * const  h  = x.h;
    StepCall const &   c  = x.c;
    FusedExtra const & fx = c.fx;
    if (!fx.d_rle)
        return LX_OK;
    if (fx.d_src_out)
        LX_HIP(h, hipMemcpyAsync(fx.d_src_out, h->d_sel_src.ptr, x.cap * sizeof(uint32_t), hipMemcpyDeviceToDevice, x.stream));
    if (packed_already) // (the checkpoint backtrace emits the codes itself)
        return LX_OK;
    lx::PackParams pp{};
    pp.hsp        = static_cast<lx::Hsp *>(c.d_out_hsp);
    pp.ops        = static_cast<uint8_t const *>(c.d_out_ops);
    pp.ops_off    = static_cast<uint64_t const *>(c.d_ops_off);
    pp.ops_stride = fx.ops_stride;
    pp.src        = static_cast<uint32_t const *>(h->d_sel_src.ptr);
    pp.count_ptr  = static_cast<uint64_t const *>(c.d_out_count);
    pp.n          = x.cap;
    pp.rle        = fx.d_rle;
    pp.rle_top    = fx.d_rle_top;
    pp.rle_cap    = fx.rle_cap;
    pp.rle_len    = fx.d_rle_len;
    pp.err        = ws_error(h);
    LX_HIP(h, hipMemsetAsync(fx.d_rle_top, 0, sizeof(unsigned long long), x.stream));
    LX_HIP(h, lx::launch_rle_pack(pp, x.stream));
    return LX_OK;
}

// after a sweep: backtrace of the survivors straight from its checkpoints (slots and end cells by original index)
int backtrace_stage(StepCtx & x)
{
    lx_handle * const h      = x.h;
    StepCall const &  c      = x.c;
    StepPlan const &  plan   = x.plan;
    hipStream_t const stream = x.stream;
    lx::TraceParams p = trace_params(h, x.slot, c.d_q, c.d_s, static_cast<lx::Extension const *>(h->d_sel_ext.ptr), x.cap, c.lim);
    p.slot_stride     = plan.stride;
    p.steps_cap       = plan.steps;
    p.panels_cap      = plan.panels;
    p.out_hsp         = static_cast<lx::Hsp *>(c.d_out_hsp);
    p.out_ops         = static_cast<uint8_t *>(c.d_out_ops);
    p.ops_off         = static_cast<uint64_t const *>(c.d_ops_off);
    p.ops_stride      = c.fx.ops_stride;
    if (c.fx.d_rle) // the backtrace writes run-length codes itself
    {
        p.rle     = c.fx.d_rle;
        p.rle_top = c.fx.d_rle_top;
        p.rle_cap = c.fx.rle_cap;
        p.rle_len = c.fx.d_rle_len;
        LX_HIP(h, hipMemsetAsync(c.fx.d_rle_top, 0, sizeof(unsigned long long), stream));
        if (c.fx.d_rle_len) // (positions the backtrace never visits -- padding, score-less -- read 0)
            LX_HIP(h, hipMemsetAsync(c.fx.d_rle_len, 0, x.cap * sizeof(uint32_t), stream));
    }
    p.src         = static_cast<uint32_t const *>(h->d_sel_src.ptr);
    p.count_ptr   = static_cast<uint64_t const *>(c.d_out_count);
    p.chunk_start = 0;
    p.geo         = plan.geo;
    p.slot_by_src = 1;
    p.out_by_pos  = c.by_pos ? 1 : 0;
    if (plan.packed)
    {
        p.ovf        = p.trace + x.batch_dw; // int16-pair slots of what the packed kernel declined
        p.ovf_stride = plan.stride32;
    }
    if (x.tab_on)
    {
        p.wf_tab  = static_cast<lx::WfSlots const *>(c.tab.dev);
        p.split_n = c.tab.dw1 ? c.tab.n0 : 0;
        p.trace2  = p.trace + c.tab.dw0 + x.tab_ovf_dw;
    }
    PhaseTimer ptb(h, stream, 3);
    LX_HIP(h, lx::launch_ckpt_backtrace(p, stream));
    ptb.close();
    return fused_pack(x, true);
}

// no sweep: pass 2 on the survivors (src/search_algo.hpp:1293-1296); the grid covers the worst case, wavefronts beyond
// *d_out_count exit
int pass2_stage(StepCtx & x)
{
    lx_handle * const h = x.h;
    StepCall const &  c = x.c;
    int const rc = align_dev_impl(h, x.slot, c.d_q, c.d_s, static_cast<lx::Extension const *>(h->d_sel_ext.ptr), x.cap, static_cast<lx::Hsp *>(c.d_out_hsp),
                                  static_cast<uint8_t *>(c.d_out_ops), static_cast<uint64_t const *>(c.d_ops_off), x.stream, c.lim, x.share_slots(),
                                  static_cast<uint32_t const *>(h->d_sel_src.ptr), static_cast<uint64_t const *>(c.d_out_count),
                                  static_cast<int32_t const *>(h->d_sel_score.ptr), c.by_pos, c.fx.ops_stride);
    return rc ? rc : fused_pack(x, false);
}

} // namespace

int lxi::fused_impl(lx_handle * h, int slot, StepCall const & c)
{
    if (slot < 0 || slot > 1 || !h->have_sc[slot])
        return fail(h, LX_ESTATE, "scoring slot %d not set", slot);
    if (c.n == 0)
        return LX_OK;
    if (!c.d_q || !c.d_s || !c.d_ext || !c.d_out_score || !c.d_out_count || !c.d_out_hsp || !c.d_out_ops || (!c.d_ops_off && !c.fx.ops_stride))
        return fail(h, LX_EINVAL, "NULL device pointer");
    if (c.lim.max_qlen == 0 || c.lim.max_slen == 0)
        return fail(h, LX_ESTATE, "lx_extend_batch_dev needs LX_OPT_MAX_QLEN and LX_OPT_MAX_SLEN (it never synchronises)");
    if (c.n > 0xfffffff0ull)
        return fail(h, LX_EINVAL, "at most 2^32-16 extensions per call");
    int rc = bind(h);
    if (rc)
        return rc;
    StepCtx x{h, slot, c, h->facts[slot], c.stream};
    if ((rc = plan_for_call(x)))
        return rc;
    bool first_part_only = false;
    if ((rc = x.plan.sweep ? sweep_stage(x, first_part_only) : pass1_stage(x)) || first_part_only)
        return rc;
    if ((rc = select_stage(x)) || (rc = x.plan.sweep ? backtrace_stage(x) : pass2_stage(x)))
        return rc;
    LX_HIP(h, hipEventRecord(h->ev1, x.stream));
    h->timed = true;
    return LX_OK;
}
