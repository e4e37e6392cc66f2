// lx_step_plan.cpp -- the plans of lx_step_plan.h: which kernels a step runs, in which geometry, with how much memory.  Nothing here
// touches a handle or the device; every kernel path of the library is chosen in this file.
#include "lx_step_plan.h"

#include <algorithm>
#include <cstdio>

#include "lx_device.h"

namespace lxi
{

SchemeFacts scheme_facts(lx_scoring const & sc)
{
    SchemeFacts f{};
    f.alph       = sc.alphabet_size;
    f.gap_open   = sc.gap_open;
    f.gap_extend = sc.gap_extend;
    f.trace_ok   = true;
    f.b8_ok      = true;
    f.smax_entry = 0;
    for (int a = 0; a < sc.alphabet_size; ++a)
        for (int b = 0; b < sc.alphabet_size; ++b)
        {
            int const v = sc.matrix[a * LX_ALPH + b];
            if (v - sc.gap_extend < -31 || v - sc.gap_extend > 31)
                f.trace_ok = false;
            if (v - sc.gap_open < 0 || v - sc.gap_open > 255)
                f.b8_ok = false;
            f.smax_entry = std::max(f.smax_entry, v);
        }
    return f;
}

// ---- the shared rules ----------------------------------------------------------------------------------------------------

bool compact_gaps_ok(SchemeFacts const & sc)
{
    return -sc.gap_open <= lx::kC16MaxGap && sc.gap_open <= sc.gap_extend;
}

bool fits_int16(SchemeFacts const & sc, uint64_t max_qlen, uint64_t max_slen)
{
    return (uint64_t)sc.smax_entry * std::min(max_qlen, max_slen) < 32000 && max_slen <= 65535; // (longer windows: direction bits)
}

int64_t score_bound(SchemeFacts const & sc, uint64_t max_qlen, uint32_t steps, int G)
{
    // (the packed kernels' exactness gate, lx_score_f16.hip; ScoringDev::smax = largest entry - ge)
    return (int64_t)max_qlen * std::max(sc.smax_entry, 0) + (int64_t)(-sc.gap_extend) * ((int64_t)steps + G + 2) + (sc.smax_entry - sc.gap_extend) + 2;
}

int64_t half_frame_bias(SchemeFacts const & sc, int G)
{
    // (|g2| + |ge| * G with g2 = gap_open - gap_extend, as lx_score_f16.hip adds it to its exactness test)
    return (int64_t)(sc.gap_extend - sc.gap_open) + (int64_t)(-sc.gap_extend) * G;
}

uint32_t steps_for(uint64_t max_slen, int G)
{
    return (uint32_t)((max_slen + G - 1 + 15) & ~15ull);
}

uint32_t panels_for(uint64_t max_qlen, int panel)
{
    return (uint32_t)std::max<uint64_t>(1, (max_qlen + panel - 1) / panel);
}

uint64_t carry_pairs(uint64_t n, uint64_t max_slen)
{
    return n * ((max_slen + 3) & ~3ull);
}

// ---- the geometry pickers ------------------------------------------------------------------------------------------------

// LDS a wavefront of the packed-half kernel may spend on two query profiles (one per half wavefront: query runs of 8)
// (24 KiB; protein profiles too: 12.8 vs 14.0 ms (pass 1), 16.6 vs 19.1 ms (sweep) for runs of 8)
size_t pair_lds_limit()
{
    return 24 * 1024;
}

// what two profiles of a packed-half geometry and the kernel's staging take of a wavefront's LDS
static size_t two_profiles_bytes(Geo geo, int nrows)
{
    return 2 * lx::score_pair_profile_bytes(geo, nrows) + 64 * 8 * 4;
}

// Smallest panel that holds the query; 8-lane geometries need one shared profile per wavefront (8 profile slots
// per wavefront would not fit the LDS budget), so without sharing only the 16/32/64-lane geometries are used.
Geo pick_cfg(uint32_t qlen, bool shared)
{
    if (shared)
    {
        if (qlen <= 64)
            return Geo{8, 8};
        if (qlen <= 104)
            return Geo{8, 13};
        if (qlen <= 128)
            return Geo{8, 16};
        if (qlen <= 152)
            return Geo{8, 19};
    }
    if (qlen <= 64 && !shared)
        return Geo{8, 8}; // 64 columns: 8 slots of a 64-column profile are small enough
    if (qlen <= 160)
        return Geo{16, 10};
    if (qlen <= 208)
        return Geo{16, 13};
    if (qlen <= 256)
        return Geo{16, 16};
    // Longer queries: several panels of a 16-lane geometry beat one wide panel of the 32- / 64-lane ones (400 aa x 442:
    // (16,13) x 2 panels 4.4 TCUPS, (16,16) x 2 3.8, (16,10) x 3 3.8, (32,10) x 2 2.6, (64,10) 2.3 -- the wide groups pay
    // for their long skew and cross-row shifts).  Pick the geometry with the least padded work, weighted by the time
    // each took per padded column in that measurement.
    struct Cand
    {
        Geo    geo;
        double cost;
    };
    static constexpr Cand cands[] = {{{16, 16}, 0.0581}, {{16, 13}, 0.0619}, {{16, 10}, 0.0621}};
    Geo    best      = cands[0].geo;
    double best_cost = 1e30;
    for (Cand const & c : cands)
    {
        uint32_t const panel = (uint32_t)c.geo.panel();
        double const   cost  = (double)((qlen + panel - 1) / panel * panel) * c.cost;
        if (cost < best_cost)
        {
            best_cost = cost;
            best      = c.geo;
        }
    }
    return best;
}

// Checkpoint geometry, (8,19) or (16,13), for a query of max_q columns: one panel if it fits, else the
// panel count x width x measured time per padded column that is least (int32 kernels: 0.070 vs 0.062 per column;
// packed16 = the sweep of lx_score_i16.hip will run).
Geo ckpt_cfg_for(uint64_t max_q, bool packed16)
{
    uint64_t const p1 = (uint64_t)lx::kGeo8x19.panel(), p2 = (uint64_t)lx::kGeo16x13.panel();
    if (max_q <= p1)
        return lx::kGeo8x19;
    if (max_q <= p2)
        return lx::kGeo16x13;
    // (the packed 16-bit sweep is bound by its checkpoint bytes: the 19-column strips of (8,19) store fewer boundary
    // columns -- 400 aa: 0.0134 ms per padded column against 0.0156 for (16,13) with int16-pair slots; with compact codes,
    // which only the (8,19) panels have, 0.0108)
    double const f1 = packed16 ? 0.0108 : 0.070, f2 = packed16 ? 0.0156 : 0.062;
    double const c1 = (double)((max_q + p1 - 1) / p1 * p1) * f1, c2 = (double)((max_q + p2 - 1) / p2 * p2) * f2;
    return c1 < c2 ? lx::kGeo8x19 : lx::kGeo16x13;
}

// Multi-query sweep (lx_sweep_mq.hip): checkpoint geometry for queries of up to max_q columns -- (8,19), (8,11) or
// (8,13), as many panels as the query needs: the one with the least padded work (columns swept x instructions
// per column: 3.75 per cell of the recurrence + ~12 per step and lane spread over the strip's columns).  lx_host_plan.cpp deals
// ragged lists to classes with the same function, so a chunk's geometry is the one its class was formed for.
Geo mq_cfg_for(uint64_t max_q)
{
    Geo    best = lx::kGeo8x19;
    double best_cost = 1e30;
    for (Geo geo : {Geo{8, 19}, Geo{8, 11}, Geo{8, 13}})
    {
        uint64_t const panel = (uint64_t)geo.panel();
        double const   C     = (double)panel / 8.0;
        double const   cost  =(double)((std::max<uint64_t>(max_q, 1) + panel - 1) / panel * panel) * (3.75 * C + 12.0) / C;
        if (cost < best_cost - 1e-9)
        {
            best_cost = cost;
            best      = geo;
        }
    }
    return best;
}

// The packed-half geometry of pass 1 for queries of up to max_qlen columns ({}: none is wide enough)
Geo score_pair_cfg_for(uint32_t max_qlen)
{
    if (max_qlen <= 64)
        return Geo{8, 8};
    if (max_qlen <= 104)
        return Geo{8, 13};
    if (max_qlen <= 128)
        return Geo{8, 16};
    if (max_qlen <= 152)
        return Geo{8, 19};
    if (max_qlen <= 192)
        return Geo{8, 24};
    if (max_qlen <= 200)
        return Geo{8, 25};
    if (max_qlen <= 208)
        return Geo{16, 13};
    return Geo{};
}

// geometries with 16-lane groups (8 extensions per wavefront)
Geo score_pair_cfg_for_runs_of_8(uint32_t max_qlen)
{
    if (max_qlen <= 160)
        return Geo{16, 10};
    if (max_qlen <= 208)
        return Geo{16, 13};
    return Geo{};
}

// ---- pass 1 ---------------------------------------------------------------------------------------------------------------

ScorePlan plan_score_cfg(Geo geo, bool multi, bool shared, uint64_t band, Geo pair_geo, bool pair16)
{
    ScorePlan pl{};
    pl.geo = geo, pl.multi = multi, pl.shared = shared, pl.pair_geo = pair_geo, pl.pair16 = pair16, pl.band = band;
    // band mode: the int32 kernel of the generic geometry, any query width (the packed kernels carry no band code) -- or, for query
    // runs of a multiple of 8 whose queries fit 152 columns, (8,19) with one LDS profile per wavefront
    pl.narrow = band && shared && geo == lx::kGeo8x19 && !multi;
    return pl;
}

ScorePlan plan_score(SchemeFacts const & sc, ListLimits const & lim, ScoreOptions const & o)
{
    uint32_t const q32 = (uint32_t)std::min<uint64_t>(lim.max_qlen, 0xffffffffu);
    // geometry from the caller's hints
    bool const want_shared = lim.query_run != 0 && lim.query_run % 8 == 0;
    Geo const  geo         = lim.max_qlen ? pick_cfg(q32, want_shared) : lx::kGeo16x10;
    bool const multi       = lim.max_qlen == 0 || lim.max_qlen > (uint64_t)geo.panel();
    bool const shared      = lim.query_run != 0 && (lim.query_run % (uint64_t)geo.groups()) == 0;
    // packed-half path: the extensions of a wavefront (or, where two LDS profiles fit, of each half of it) must
    // share their query and the query must fit one panel
    Geo  pair_geo;
    int  pair_share = 0;
    bool pair16     = false;
    if (o.f16 && shared && lim.max_qlen != 0)
    {
        Geo const pc = score_pair_cfg_for(q32);
        if (pc.chosen())
        {
            int const      groups   = pc.groups();
            uint64_t const per_wave = 2ull * groups;
            if (lim.query_run % per_wave == 0)
                pair_geo = pc;
            else if (groups >= 2 && lim.query_run % (per_wave / 2) == 0 && 2 * lx::score_pair_profile_bytes(pc, sc.nrows()) <= pair_lds_limit())
            {
                pair_geo   = pc;
                pair_share = groups / 2;
            }
            else if (lim.query_run % 8 == 0) // two profiles do not fit: a 16-lane geometry holds 8 extensions per wavefront
                pair_geo = score_pair_cfg_for_runs_of_8(q32);
        }
        else if (lim.query_run % 16 == 0 && lim.max_slen != 0) // wider than any packed-half geometry
            pair16 = true;
    }
    ScorePlan pl  = plan_score_cfg(geo, multi, shared, o.band, pair_geo, pair16);
    pl.pair_share = pair_share;
    pl.max_slen   = lim.max_slen;
    // carry pairs: where the launch's own panel does not hold the widest query (the packed 16-bit kernel sweeps wide queries in
    // (8,19) panels even where the int32 geometry is a single one)
    pl.carry = o.band ? (lim.max_qlen == 0 || lim.max_qlen > (uint64_t)pl.launch_cfg().panel()) : (multi || pair16);
    return pl;
}

void describe_score(ScorePlan const & pl, char * buf, size_t len)
{
    int const G = pl.geo.g, C = pl.geo.c;
    if (pl.band)
        snprintf(buf, len, "lx::score_kernel<%s,band> (band mode, +-%d diagonals)", pl.narrow ? "8,19,false" : "16,10,true", (int32_t)pl.band);
    else if (pl.pair16)
        snprintf(buf, len, "lx::sweep_pair16_kernel<8,19,true,false> (+ int32 fix-up lx::score_kernel<%d,%d,%s>)", G, C, pl.multi ? "true" : "false");
    else if (pl.pair_geo.chosen())
        snprintf(buf, len, "lx::score_pair_kernel<%d,%d> (+ int32 fix-up lx::score_kernel<%d,%d,%s>)", pl.pair_geo.g, pl.pair_geo.c, G, C,
                 pl.multi ? "true" : "false");
    else
        snprintf(buf, len, "lx::score_kernel<%d,%d,%s>%s", G, C, pl.multi ? "true" : "false", pl.shared ? " shared-profile" : "");
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------

TracePlan plan_trace(SchemeFacts const & sc, ListLimits const & lim, int share_slots, TraceOptions const & o)
{
    uint64_t const max_q = lim.max_qlen, max_s = lim.max_slen;
    Geo const      generic = lx::kGeo16x10, g8 = lx::kGeo8x19, g16 = lx::kGeo16x13;
    uint64_t const p1 = (uint64_t)g8.panel(), p2 = (uint64_t)g16.panel();
    TracePlan      pl{};
    // checkpoint mode (lx_ckpt.hip): shared-profile geometries (8,19) / (16,13), scores that fit int16; queries wider
    // than 208 columns take several (16,13) panels
    pl.ckpt = !o.band && o.pass2 >= 1 && share_slots >= 2 && fits_int16(sc, max_q, max_s);
    // Direction bits beyond one panel: the 16-lane geometry that pads the query less ((16,13) needs the shared profile).
    auto padded = [&](Geo g) { return (max_q + g.panel() - 1) / g.panel() * g.panel(); };
    pl.geo = (o.band && !(share_slots >= 4 && max_q <= p1))      ? generic // (band mode: (8,19) or generic)
             : (share_slots >= 2 && max_q <= p1)                 ? g8
             : (share_slots >= 2 && max_q <= p2)                 ? g16
             : pl.ckpt                                           ? ckpt_cfg_for(max_q)
             : (share_slots >= 4 && padded(g16) < padded(generic)) ? g16
                                                                 : generic;
    int const G = pl.geo.g, W = lx::trace_cfg_words(pl.geo);
    pl.panels_cap     = panels_for(max_q, pl.geo.panel());
    pl.steps_cap      = steps_for(max_s, G);
    pl.stride         = pl.ckpt ? (uint64_t)pl.panels_cap * lx::ckpt_slot_dwords(pl.geo, pl.steps_cap) : (uint64_t)pl.panels_cap * pl.steps_cap * G * W;
    pl.per_ext        = pl.stride * 4;
    pl.budget_ext     = std::max<uint64_t>(1, o.trace_bytes / std::max<uint64_t>(pl.per_ext, 1));
    pl.shared_profile = (o.band && pl.geo == generic) ? 0 : share_slots;
    // The forward kernel finds the end cell cheaply when it knows each extension's best score; a stand-alone traceback call
    // computes them first (a fraction of the traceback's cost), one profile per lane group
    Geo const sgeo = pick_cfg((uint32_t)std::min<uint64_t>(max_q, 0xffffffffu), false);
    pl.score       = plan_score_cfg(sgeo, max_q > (uint64_t)sgeo.panel(), false, o.band);
    pl.max_slen    = max_s;
    // (the panels of pass 2 are never wider than those of its pass 1: several panels there mean several here)
    pl.carry = pl.panels_cap > 1 || pl.score.multi || (o.band && max_q > (uint64_t)generic.panel());
    pl.score.carry = pl.carry, pl.score.max_slen = max_s;
    return pl;
}

void describe_trace(TracePlan const & pl, char * buf, size_t len)
{
    int const G = pl.geo.g, C = pl.geo.c;
    if (pl.ckpt)
        snprintf(buf, len, "lx::ckpt_forward_kernel<%d,%d>", G, C);
    else
        snprintf(buf, len, "lx::trace_forward_kernel<%d,%d,%s>", G, C, pl.panels_cap > 1 ? "true" : "false");
}

// ---- the fused step ---------------------------------------------------------------------------------------------------------

namespace
{

// One way to sweep the whole batch (the checkpoint forward kernel runs once over ALL extensions -- it is pass 1 and the forward half
// of pass 2 at the same time -- and the backtrace reads the checkpoints of the survivors in place).  runs: it applies and the
// batch's slots fit the trace budget.
struct SweepCand
{
    bool     runs = false;
    Geo      geo;
    int      share = 0;
    uint32_t steps = 0, panels = 1;
    uint64_t stride = 0;   // uint32 per slot of the batch
    uint64_t stride32 = 0; // ... of an int16-pair slot (the whole batch's, or the overflow area's)
    uint64_t ovf_cap = 0;
    bool     packed = false, may_decline = true, wide_compact = false, mq_wide = false;
};

// compact slots for the batch (+ the spare slot idle halves write to) fit the budget
bool packed_fits(StepOptions const & o, uint64_t stride)
{
    return (o.n + 1) * stride * 4 <= o.trace_bytes;
}

// ... and int16-pair slots for what the packed kernel declines, in whatever the budget leaves
uint64_t overflow_slots(StepOptions const & o, SweepCand const & c)
{
    return std::min<uint64_t>(o.n, (o.trace_bytes - (o.n + 1) * c.stride * 4) / (c.stride32 * 4));
}

// Multi-query sweep (lx_sweep_mq.hip): query runs of 4 or 8 (2 / 4 lane groups per LDS profile) -- what lx_extend_batch
// makes of a ragged list --, or any multiple of 4 when LX_OPT_MQ_SWEEP = 2 asks for it.  Needs byte profiles (no
// substitution dearer than a gap's first character) and compact codes (that character costs at most 31).
bool mq_wanted(SchemeFacts const & sc, StepOptions const & o)
{
    uint64_t const run = o.query_run;
    // (runs of 8: the packed-half sweep with one profile per half wavefront keeps its occupancy while both profiles fit
    // ~13 KB -- the small alphabets: configs[2] 29.1 against 31.8 ms, configs[4] 7.4 against 8.1 -- and loses it beyond)
    bool const half8_cheap = two_profiles_bytes(lx::kGeo8x19, sc.nrows()) <= 13 * 1024;
    // (... and for queries beyond 208 columns a run that is a multiple of 8 but not of 16 has no packed sweep with compact
    // codes of its own: the multi-query one serves it)
    bool const odd8 = run % 8 == 0 && run % 16 != 0 && run != 0;
    // (run 2 = the free packing: pairs of one query, at most four queries per wavefront -- only this sweep serves it;
    // run 1 = the solo packing: no promise, a byte profile per window, where 16 of them fit a wavefront's LDS share: the
    // alphabets of at most 6 rows -- nucleotides, bisulfite)
    bool const solo_fits = lx::sweep_mq_lds_bytes(lx::kGeo8x19, sc.alph + 1, -1) <= 20 * 1024;
    bool const wanted    = run == 1     ? (o.mq >= 1 && solo_fits)
                           : run == 2   ? o.mq >= 1
                           : o.mq == 2  ? (run != 0 && run % 4 == 0)
                           : o.mq == 1  ? (run == 4 || (odd8 && (!half8_cheap || o.max_qlen > 208)))
                                        : false;
    return wanted && o.pass2 == 2 && o.f16 && sc.trace_ok && sc.b8_ok && compact_gaps_ok(sc) && !o.band;
}

SweepCand mq_candidate(SchemeFacts const & sc, StepOptions const & o)
{
    SweepCand c{};
    if (!mq_wanted(sc, o))
        return c;
    c.geo    = o.mq_geo.chosen() ? o.mq_geo : mq_cfg_for(o.max_qlen);
    c.panels = panels_for(o.max_qlen, c.geo.panel());
    if (!fits_int16(sc, o.max_qlen, o.max_slen))
        return c;
    int const G = 8;
    c.steps     = steps_for(o.max_slen, G);
    c.stride32  = (uint64_t)c.panels * lx::ckpt_slot_dwords(c.geo, c.steps);
    // (mq_wide: int16-pair slots from the sweep itself -- lists whose windows score beyond the compact codes, lx_xb_wf.cpp)
    c.mq_wide   = o.mq_wide && c.geo == lx::kGeo8x19;
    c.stride    = c.mq_wide ? c.stride32 : (uint64_t)c.panels * lx::ckpt16_slot_dwords(c.geo, c.steps);
    // lane groups per query: a wavefront's 16 slots hold 16 / 8 / 4 windows of one query, whatever divides the run
    // (1 = the free packing: a lane group's pair shares a query, up to four queries per wavefront in any split; -1: solo)
    c.share     = o.query_run == 1 ? -1 : o.query_run == 2 ? 1 : (o.query_run % 16 == 0 ? 16 : o.query_run % 8 == 0 ? 8 : 4) / 2;
    c.runs      = packed_fits(o, c.stride); // (a batch beyond the slot budget: the per-survivor paths)
    int64_t const worst = score_bound(sc, o.max_qlen, c.steps, G);
    c.may_decline = c.mq_wide ? worst > 0x7BFF - 2048 : (worst > kCompactMaxScore || c.panels > 1);
    if (c.runs && c.may_decline)
        c.ovf_cap = overflow_slots(o, c);
    c.packed = c.runs;
    if (!c.runs)
        c.mq_wide = false;
    return c;
}

// One query per wavefront: one panel of (8,19) or (16,13); wider queries: several panels.  `c`: what a multi-query candidate that
// does not run leaves behind -- the plan keeps it where this candidate does not decide (the packed-half launch reads `share`).
SweepCand one_query_candidate(SchemeFacts const & sc, StepOptions const & o, SweepCand c)
{
    bool const run16 = o.query_run % 16 == 0;
    int const  nrows = sc.nrows();
    c.geo = ckpt_cfg_for(o.max_qlen, o.f16 && run16);
    // short queries (<= 104 columns, e.g. 100-residue reads): the (8,13) geometry where the packed-half sweep applies --
    // a third fewer padded columns than (8,19)
    bool const half_ok = o.f16 && compact_gaps_ok(sc);
    if (c.geo == lx::kGeo8x19 && half_ok && o.max_qlen <= (uint64_t)Geo{8, 13}.panel() && (run16 || two_profiles_bytes(Geo{8, 13}, nrows) <= pair_lds_limit()))
        c.geo = Geo{8, 13};
    // 153 - 200 columns: 25-column strips of 8-lane groups (16 extensions of one query per wavefront, 7 steps of skew
    // instead of 15, no padded column at 200) where the packed-half sweep applies
    if (c.geo == lx::kGeo16x13 && half_ok && o.max_qlen <= (uint64_t)Geo{8, 25}.panel() && run16)
        c.geo = Geo{8, 25};
    c.panels = panels_for(o.max_qlen, c.geo.panel());
    if (!fits_int16(sc, o.max_qlen, o.max_slen))
        return c;
    int const G = c.geo.g;
    c.steps     = steps_for(o.max_slen, G);
    c.stride32  = (uint64_t)c.panels * lx::ckpt_slot_dwords(c.geo, c.steps);
    // Packed half precision where its geometry matches the checkpoint layout ((8,19): 16 extensions of one query per
    // wavefront, or runs of 8 with one query per half wavefront where two LDS profiles fit, i.e. for the small
    // alphabets; (16,13): 8 extensions) and a gap's first character costs at most 31 (the compact checkpoint codes
    // of Ckpt16Layout).  Wavefronts it declines leave the sentinel -1; the int32 kernel fills those in.
    c.packed      = half_ok && c.panels == 1 && ((G == 8 && run16) || c.geo == lx::kGeo16x13);
    // Queries wider than a panel: compact codes as well, one part per (8,19) panel, written by the packed int16 kernel
    // (the half-precision one has no carry between panels); what scores beyond the codes goes to the int32 launch
    c.wide_compact = half_ok && c.panels > 1 && c.geo == lx::kGeo8x19 && run16;
    c.packed       = c.packed || c.wide_compact;
    if (half_ok && c.panels == 1 && (c.geo == lx::kGeo8x19 || c.geo == Geo{8, 13}) && !c.packed && o.query_run % 8 == 0 &&
        two_profiles_bytes(c.geo, nrows) <= pair_lds_limit())
    {
        c.packed = true;
        c.share  = 4;
    }
    if (c.packed)
    {
        // (the packed-half sweep keeps a pair of windows in one dword: CkptPairLayout, never larger than two Ckpt16Layout slots)
        c.stride = c.wide_compact ? (uint64_t)c.panels * lx::ckpt16_slot_dwords(c.geo, c.steps) : lx::ckpt_pair_slot_dwords(c.geo, c.steps);
        c.runs   = packed_fits(o, c.stride);
        // (the packed kernel cannot decline when even the worst query passes its test)
        // (the packed-half kernel computes in a frame raised by half_frame_bias and tests with it in; the int16 one has no bias)
        c.may_decline = c.wide_compact || score_bound(sc, o.max_qlen, c.steps, G) + half_frame_bias(sc, G) > kCompactMaxScore;
        if (c.runs && c.may_decline)
            c.ovf_cap = overflow_slots(o, c);
    }
    else
    {
        c.stride = c.stride32;
        c.runs   = o.n * c.stride * 4 <= o.trace_bytes;
    }
    return c;
}

} // namespace

// ---- the ONE place that decides how a fused step runs: which sweep kernel family (if any), geometry, panel count, slot
// layout, queries per wavefront.  A pure function of the scheme's facts and the step's options -- fused_impl follows it, and
// lx_plan_step() shows it to tests/test_plan.py, which walks it over query widths, run lengths and schemes on the CPU.
StepPlan plan_step(SchemeFacts const & sc, StepOptions const & o)
{
    bool const shared = o.query_run != 0 && o.query_run % 8 == 0;
    // Single sweep (LX_OPT_PASS2_MODE = 2): the multi-query sweep where it applies and fits, else one query per wavefront (needs a
    // shared-profile geometry)
    SweepCand const mqc = mq_candidate(sc, o);
    bool const      mq  = mqc.runs;
    SweepCand const c   = (!mq && o.pass2 == 2 && shared && sc.trace_ok && !o.band) ? one_query_candidate(sc, o, mqc) : mqc;
    // No packed-half sweep (queries wider than a panel, gap costs beyond the compact codes, ...): the packed int16 kernel
    // writes the int16-pair slots of the int32 kernel, two extensions per lane group; what fails its range test is left to
    // the int32 launch.  16 extensions of one query per wavefront at (8,19), 8 at (16,13).
    bool const i16_sweep = c.runs && !c.packed && o.f16 && o.query_run % (c.geo == lx::kGeo8x19 ? 16 : 8) == 0 && c.geo != Geo{8, 13} && c.geo != Geo{8, 25};
    // Adaptive choice (the one-query-per-wavefront sweep; lx_extend_batch's multi-query plan keeps its sweep): few survivors
    // last time -> plain pass 1, checkpoints for the survivors only (mode 1).
    bool const adapted = c.runs && !mq && o.adapt != 0 && o.surv_frac >= 0.0 && o.surv_frac * 1000.0 < (double)o.adapt;
    StepPlan pl{};
    pl.shared      = shared;
    pl.sweep       = c.runs && !adapted;
    pl.adapted     = adapted;
    pl.family      = !pl.sweep ? kNoSweep : mq ? kMqSweep : c.wide_compact ? kI16CompactWide : c.packed ? kHalfSweep : i16_sweep ? kI16Pairs : kInt32Sweep;
    pl.geo         = c.geo;
    pl.steps       = c.steps;
    pl.panels      = c.panels;
    pl.stride      = c.stride;
    pl.stride32    = c.stride32;
    pl.ovf_cap     = pl.sweep ? c.ovf_cap : 0;
    pl.share       = c.share;
    pl.compact     = pl.sweep && c.packed && !c.mq_wide;
    pl.packed      = pl.sweep && c.packed;
    pl.wide        = pl.sweep && c.mq_wide;
    pl.may_decline = c.may_decline;
    return pl;
}

// the sweep a plan names, as the launch sequence fused_impl issues for it (what lx_last_trace_kernel_name reports)
void describe_plan(StepPlan const & pl, char * buf, size_t len)
{
    int const nameG = pl.geo.g, nameC = pl.geo.c;
    switch (pl.family)
    {
        case kMqSweep:
            snprintf(buf, len, "lx::sweep_mq_kernel<%d,%s> (single sweep, %s%d queries per wavefront%s)", nameC, pl.wide ? "true,true" : pl.panels > 1 ? "true,false" : "false,false",
                     pl.share < 0 ? "solo packing: up to " : pl.share == 1 ? "free packing: up to " : "", pl.share < 0 ? 16 : pl.share == 1 ? 4 : 8 / std::max(1, pl.share),
                     pl.may_decline ? "; + int32 fix-up lx::ckpt_forward_kernel" : "");
            break;
        case kI16CompactWide:
            snprintf(buf, len, "lx::sweep_pair16_kernel<%d,%d,true,true,true> (single sweep, compact codes; + int32 fix-up lx::ckpt_forward_kernel<%d,%d,false>)",
                     nameG, nameC, nameG, nameC);
            break;
        case kHalfSweep:
            if (pl.may_decline)
                snprintf(buf, len, "lx::score_pair_kernel<%d,%d,true> (single sweep; + int32 fix-up lx::ckpt_forward_kernel<%d,%d,false>)", nameG, nameC,
                         nameG, nameC);
            else
                snprintf(buf, len, "lx::score_pair_kernel<%d,%d,true> (single sweep)", nameG, nameC);
            break;
        case kI16Pairs:
            snprintf(buf, len, "lx::sweep_pair16_kernel<%d,%d,%s> (single sweep; + int32 fix-up lx::ckpt_forward_kernel<%d,%d,false>)", nameG, nameC,
                     pl.panels > 1 ? "true" : "false", nameG, nameC);
            break;
        case kInt32Sweep: snprintf(buf, len, "lx::ckpt_forward_kernel<%d,%d,false> (single sweep)", nameG, nameC); break;
        default: snprintf(buf, len, "%s", pl.adapted ? "pass 1, then checkpoints for the survivors (few survived the last batch)" : "pass 1, then pass 2 on the survivors"); break;
    }
}

} // namespace lxi
