// lx_xb_wf.cpp -- the chunk driver of the multi-query sweep (lx_xb.h).  Chunks = ranges of the plan's wavefronts, about chunk_target
// slots.  The plan's order is a permutation of the caller's list (+ fillers): the host only touches 4 bytes per slot (the 24-byte
// records and their cut-offs are gathered from the device copy of the list at HBM speed, not by cache misses of a few host threads),
// the scores are scattered into caller order on the device and come back once, at the end of the call.  A chunk may span panel counts
// (its slots are sized for its widest query, its narrower queries run the multi-panel kernel over one panel): a chunk boundary
// wherever the panel count changes was measured on the ragged list of bench.py and costs more than it saves -- 3 chunks 20.8 ms,
// 2 chunks 18.9 ms: every chunk pays the fixed cost of a backtrace launch (~0.5-1 ms), the single-panel kernel saves a tenth of a
// 0.8 ms sweep
#include "lx_level2.h"
#include "lx_xb.h"

namespace lxi
{
namespace
{

// ONE chunk in TWO calls (slots by wavefront): the plan's pool goes to the GPU -- its slot list, its table, its sweep -- while the
// streamed part of the plan is still being made on the host threads; the second call sweeps the streamed wavefronts into slots
// behind the pool's and runs what follows a sweep ONCE over all of them: one selection, one backtrace, one result list.  (Rounds
// 3-4: the pool as a chunk of its own -- its backtrace is the latency of its longest walks, 1.6 ms for a fifth of the survivors --
// or, for small lists, everything planned before the first launch.)
struct TwoCall
{
    uint64_t n1 = 0, nw1 = 0, dw0 = 0, ovf_cap = 0, ovf_dw = 0, total_dw = 0, stride = 0, max_q = 0, max_s = 0, cap_slots = 0;
};

// what stage() found in the wavefronts it staged: the dwords of their table, their longest window and widest query (columns per
// lane), the cells they execute
struct Staged
{
    uint64_t dwords = 0, maxs = 1, pan = 1, padded = 0;
};

struct WfDriver
{
    Xb &              x;
    lx_handle * const h = x.h;
    HostPlan const &  p = x.p;
    TwoCall           two;
    std::vector<std::pair<uint64_t, uint64_t>> redo; // chunks (wavefront ranges) to run again with int16-pair slots
    uint64_t per_chunk = 0;
    bool     rows_cleared = false, stream_planned = false, merge_pool = false;
    bool     mq_wide = false; // the chunks' sweep writes int16-pair slots (decided chunk by chunk, with hysteresis: choose_wide)

    bool by_range() const { return x.sink.where == XbSink::kDeviceByRange; }
    bool wide_ok() const { return p.mq_geo == lx::kGeo8x19 && !lx::dev_aids().mq_no_wide; }
    bool maybe_wide() const { return wide_ok() && h->mq_decl_frac > 0.01; }

    // Compact codes hold scores up to 2046; a window beyond them is redone by the int32 launch, one profile per pair, at a tenth
    // of the sweep's speed.  Where the last chunks had more than a few such windows (long queries with strong hits: a 600-residue
    // query against its homologue scores ~3 000) the sweep writes int16 pairs itself (lx_sweep_mq.hip: WIDE) -- twice the
    // checkpoint bytes, no second launch; it goes back to the codes when fewer than 1 % of a chunk's windows need more.
    // (force_wide: a chunk that runs again because its overflow area filled up -- said by the caller, not inferred from the fraction
    // the OTHER lane's collect may have overwritten meanwhile)
    bool choose_wide(bool force_wide)
    {
        return mq_wide = wide_ok() && (force_wide || (mq_wide ? h->mq_decl_frac > 0.01 : h->mq_decl_frac > 0.03));
    }

    // the streamed part of the free packing, from wavefront `from` on in launch order
    void plan_stream(uint64_t from)
    {
        auto const tp0 = now();
        h->plan.plan_stream();
        stream_planned = true;
        h->plan.longest_first(from, p.nwf);
        x.t_prep += ms(tp0, now());
    }

    int run()
    {
        int rc;
        per_chunk      = std::max<uint64_t>(1, x.chunk_target / kWave);
        h->xb_stats[2] = p.mq_cells;
        if (!x.list_uploaded && (rc = x.upload_list()))
            return rc;
        x.t_prep += x.t_upload;
        if (x.sink.where == XbSink::kList && x.ri && x.ri->keep_on_device)
        {
            // records chunk by chunk where every range of the plan is a chunk the budgets admit (else: the call's list, one chain at the end)
            auto const * const cr = x.ri->chunk_records;
            if ((rc = device_sink(x, cr && cr->n_ranges >= 1 && x.preplanned && p.ranges_admitted(cr->cut_wf, cr->n_ranges, per_chunk, h->opt_trace_bytes, wide_ok()))))
                return rc;
        }
        stream_planned = p.use_solo || x.preplanned; // (the solo plan and a device plan are whole before the first chunk)
        // ONE launch for the pool and what follows it: the pool is a tenth of the list in wavefronts that run up to three times as long
        // as the others -- launched by itself it leaves most of the chip idle behind its longest windows (ragged list of bench.py: 5 000
        // of 37 000 wavefronts, but 5.9 of 11.8 ms), launched with the rest behind it the short wavefronts fill in.  The plan of the
        // streamed part is then made before the first launch.  (lists of up to ~200 000 windows: a dozen rounds of the chip's wavefront
        // slots.  Beyond that the pool by itself is several rounds and the streamed part's plan is better made beside its kernels:
        // 596 k windows 18.6 ms merged, 17.5 ms not; 64 k windows of 300-500-residue queries 11.9 ms merged, 16.3 ms not)
        merge_pool = !p.use_solo && !x.preplanned && p.live <= (lx::dev_aids().mq_merge_below ? lx::dev_aids().mq_merge_below : 200000);
        if (merge_pool && !stream_planned)
            plan_stream(0); // (one launch for the whole plan: the streamed part's long wavefronts would start late)
        uint64_t w0 = 0;
        if (!p.use_solo && !merge_pool && !stream_planned && !by_range() && p.pool_wf > 0 && (rc = two_calls(w0)))
            return rc;
        if ((rc = chunks(w0)) || (rc = x.drain([this](int L) { return collect(L); })) || (rc = run_redo()) || x.sink.on_device())
            return rc;
        return scores_in_caller_order(x);
    }

    // ---- the pool and what follows it as ONE chunk in two calls where the budgets admit it; w0: where the chunk loop goes on
    int two_calls(uint64_t & w0)
    {
        auto const tp0 = now();
        // what the streamed part may come to: its windows in pairs (a run's last pair may be half empty), a wavefront closed early for
        // every fifth run, one per planning thread; its slot bytes from every run's own panels and longest window
        bool const                  mw = maybe_wide();
        HostPlan::StreamBound const sb = p.stream_bound(mw);
        uint64_t cap_pan = sb.pan, cap_s = sb.maxs, dw0_est = 0, nstream = sb.windows, nstream_runs = sb.runs, dw1_est = sb.dwords;
        for (uint64_t w = 0; w < p.pool_wf; ++w)
        {
            cap_pan = std::max<uint64_t>(cap_pan, p.wf_pan[w]);
            cap_s   = std::max<uint64_t>(cap_s, p.wf_maxs[w]);
            dw0_est += p.wf_dwords(w, mw);
        }
        uint64_t const cap_slots = p.pool_wf * kWave + nstream + 5 * nstream_runs + kWave * (x.nthreads + 2);
        uint64_t const rest_dw   = dw1_est + dw1_est / 4 + (1u << 20); // (wavefronts share the largest of up to four runs' sizes)
        x.t_prep += ms(tp0, now());
        if (!(nstream != 0 && cap_slots < (1ull << 31) && chunk_fits(dw0_est * 4, h->opt_trace_bytes / 2, cap_slots + 16, cap_pan * 8 + cap_s + 4)))
            return LX_OK;
        int rc;
        if ((rc = enqueue_first(0, p.pool_wf, cap_slots, cap_pan, cap_s, rest_dw)))
            return rc;
        plan_stream(p.pool_wf); // (the second launch's wavefronts)
        auto const tp1 = now();
        // the wavefronts of the streamed part that fit behind the pool's (all of them, unless the estimate was short)
        uint64_t w_end = p.pool_wf, dw1 = 0;
        while (w_end < p.nwf && two.n1 + (w_end + 1 - p.pool_wf) * kWave <= two.cap_slots && p.wf_pan[w_end] <= cap_pan && p.wf_maxs[w_end] <= cap_s &&
               two.dw0 + two.ovf_dw + dw1 + p.wf_dwords(w_end, x.prep[0].wide) <= two.total_dw)
            dw1 += p.wf_dwords(w_end++, x.prep[0].wide);
        x.t_prep += ms(tp1, now());
        if (x.hm.on)
            fprintf(stderr, "[lx host ms]   one chunk in two calls: pool %llu wavefronts, then %llu of %llu (slots: %llu of at most %llu; dwords %llu + %llu + %llu of %llu)\n",
                    (unsigned long long)p.pool_wf, (unsigned long long)(w_end - p.pool_wf), (unsigned long long)(p.nwf - p.pool_wf), (unsigned long long)(w_end * kWave),
                    (unsigned long long)two.cap_slots, (unsigned long long)two.dw0, (unsigned long long)two.ovf_dw, (unsigned long long)dw1, (unsigned long long)two.total_dw);
        if ((rc = enqueue_second(0, p.pool_wf, w_end)))
            return rc;
        clear_rows_once();
        w0  = w_end;
        x.c = 1;
        return LX_OK;
    }

    // cut, collect the lane, enqueue, collect the other lane.  A chunk whose records are made by range is its range (the budgets
    // were checked when the mode was chosen: HostPlan::ranges_admitted).
    int chunks(uint64_t w0)
    {
        int rc;
        for (;;)
        {
            if (w0 >= p.nwf)
            {
                // the pool's wavefronts are queued (or there are none): the streamed part of the plan is made now, beside their kernels
                if (stream_planned)
                    return LX_OK;
                plan_stream(w0);
                continue;
            }
            uint64_t w1, range_now = 0;
            if (by_range())
            {
                while (x.ri->chunk_records->cut_wf[range_now + 1] <= w0)
                    ++range_now;
                w1 = x.ri->chunk_records->cut_wf[range_now + 1];
            }
            else
                w1 = p.wf_chunk_end(w0, per_chunk, h->opt_trace_bytes, maybe_wide(), !merge_pool);
            int const L = x.c & 1;
            if (x.in_flight[L] && (rc = collect(L)))
                return rc;
            x.prep[L].range = range_now;
            if ((rc = enqueue(L, w0, w1)))
                return rc;
            clear_rows_once();
            if (x.in_flight[L ^ 1] && (rc = collect(L ^ 1)))
                return rc;
            w0 = w1;
            ++x.c;
        }
    }

    // the chunks whose overflow area filled up, again with int16-pair slots -- one at a time; a WIDE chunk cannot ask again
    int run_redo()
    {
        int rc;
        while (!redo.empty())
        {
            auto const r = redo.back();
            redo.pop_back();
            if (by_range()) // (the range the chunk is: its records are made again behind the second sweep, and wait where the later ranges' stand)
                for (uint64_t k = 0; k < x.ri->chunk_records->n_ranges; ++k)
                    if (x.ri->chunk_records->cut_wf[k] == r.first)
                        x.prep[0].range = k;
            // (int16-pair slots are twice the codes': the range is run again in pieces that fit the slot budget -- a range whose records
            // are made chunk by chunk stays whole)
            for (uint64_t a = r.first; a < r.second; ++x.c)
            {
                uint64_t const b = by_range() ? r.second : p.redo_piece_end(a, r.second, h->opt_trace_bytes);
                if ((rc = enqueue(0, a, b, true)) || (rc = collect(0)))
                    return rc;
                a = b;
            }
        }
        return LX_OK;
    }

    // (beside the first chunk's kernels) every row starts as "no alignment"
    void clear_rows_once()
    {
        if (rows_cleared || x.sink.where != XbSink::kRows)
            return;
        rows_clear(x);
        rows_cleared = true;
    }

    // the table of wavefronts [wlo, whi) (lx::WfSlots): every wavefront's sixteen slots laid out for ITS longest window and widest
    // query, offsets from 0; returns the dwords they take
    uint64_t fill_table(lx::WfSlots * tab, uint64_t wlo, uint64_t whi, bool wide) const
    {
        uint64_t const pc  = (uint64_t)p.mq_geo.c;
        uint64_t       off = 0, per_panel = 0;
        uint32_t       last_steps = 0; // (a sorted plan repeats its step counts: the slot size is asked for once per run of them)
        for (uint64_t w = wlo; w < whi; ++w)
        {
            uint32_t const steps  = mq_steps(p.wf_maxs[w]);
            uint32_t const panels = (uint32_t)std::max<uint64_t>(1, ((uint64_t)p.wf_pan[w] + pc - 1) / pc);
            if (steps != last_steps)
            {
                per_panel  = slot_dwords(p.mq_geo, 1, p.wf_maxs[w], wide);
                last_steps = steps;
            }
            tab[w - wlo] = lx::WfSlots{off, steps, panels};
            off += kWave * (uint64_t)panels * per_panel;
        }
        return off;
    }

    // Wavefronts [wlo, whi) of the plan staged at slot `at` of lane L (whose pinned staging holds them): their slots' caller indices
    // (a device plan has them on the device already), their table, what they add to the call's statistics.  (what the wavefronts
    // execute: every one sweeps as many panels as its widest query needs, each for as many steps as its longest window has rows)
    Staged stage(int L, uint64_t wlo, uint64_t whi, uint64_t at, bool wide)
    {
        lx_handle::XbLane &   ln        = h->xb[L];
        uint32_t * const      slot_orig = static_cast<uint32_t *>(ln.p_orig.ptr) + at;
        unsigned const        nthreads  = x.nthreads;
        bool const            copy      = !x.preplanned;
        std::vector<uint64_t> tpad(nthreads, 0), tmaxs(nthreads, 1), tpan(nthreads, 1);
        parallel_ranges(whi - wlo, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint64_t padded = 0, smax = 1, pmax = 1; // (locals: the per-thread slots share cache lines)
                            if (copy)
                                std::memcpy(slot_orig + lo * kWave, p.plan_slot.data() + (wlo + lo) * kWave, (hi - lo) * kWave * sizeof(uint32_t));
                            for (uint64_t w = wlo + lo; w < wlo + hi; ++w)
                            {
                                padded += kWave * ((uint64_t)p.wf_pan[w] * 8) * ((uint64_t)p.wf_maxs[w] + 7);
                                smax = std::max<uint64_t>(smax, p.wf_maxs[w]);
                                pmax = std::max<uint64_t>(pmax, p.wf_pan[w]);
                            }
                            tpad[t]  = padded;
                            tmaxs[t] = smax;
                            tpan[t]  = pmax;
                        });
        Staged st;
        for (unsigned t = 0; t < nthreads; ++t)
        {
            st.padded += tpad[t];
            st.maxs = std::max(st.maxs, tmaxs[t]);
            st.pan  = std::max(st.pan, tpan[t]);
        }
        h->xb_stats[3] += st.padded;
        h->xb_stats[1] += (whi - wlo) * kWave;
        st.dwords = fill_table(static_cast<lx::WfSlots *>(ln.p_wft.ptr) + at / kWave, wlo, whi, wide);
        return st;
    }

    // what stage() staged onto the device, the slot records and cut-offs gathered from the device copy of the caller's list into lane L
    // at slot `at`.  gather_first: the gather is queued behind the slot list alone, the table follows beside it (else: one wait for both)
    int upload_staged(int L, uint64_t wlo, uint64_t whi, uint64_t at, bool gather_first)
    {
        lx_handle::XbLane & ln    = h->xb[L];
        uint64_t const      slots = (whi - wlo) * kWave, w_at = at / kWave;
        // (a device plan: the chunk's slots are a piece of it)
        uint32_t const * const d_orig = x.preplanned ? x.ri->d_plan + wlo * kWave : static_cast<uint32_t const *>(ln.d_orig.ptr) + at;
        auto const gather = [&]
        {
            Xb const & c = x;
            return lx::launch_slot_gather(static_cast<lx::Extension const *>(c.ri ? c.ri->d_ext_all : h->d_ext_all.ptr),
                                          (c.min_score || (c.ri && c.ri->d_min_all)) ? static_cast<int32_t const *>(c.ri ? c.ri->d_min_all : h->d_min_all.ptr) : nullptr,
                                          c.min_score_all, d_orig, slots, static_cast<lx::Extension *>(ln.d_ext.ptr) + at, static_cast<int32_t *>(ln.d_min.ptr) + at,
                                          h->stream);
        };
        if (!x.preplanned)
            LX_HIP(h, hipMemcpyAsync(static_cast<uint32_t *>(ln.d_orig.ptr) + at, static_cast<uint32_t const *>(ln.p_orig.ptr) + at, slots * sizeof(uint32_t),
                                     hipMemcpyHostToDevice, h->stream3));
        if (gather_first)
        {
            if (!x.preplanned)
            {
                LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
                LX_HIP(h, hipStreamWaitEvent(h->stream, ln.ev_up, 0));
            }
            LX_HIP(h, gather());
        }
        LX_HIP(h, hipMemcpyAsync(static_cast<lx::WfSlots *>(ln.d_wft.ptr) + w_at, static_cast<lx::WfSlots const *>(ln.p_wft.ptr) + w_at, (whi - wlo) * sizeof(lx::WfSlots),
                                 hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
        LX_HIP(h, hipStreamWaitEvent(h->stream, ln.ev_up, 0));
        if (!gather_first)
            LX_HIP(h, gather());
        return LX_OK;
    }

    // behind a multi-query sweep over `slots` slots whose caller indices are d_orig: the scores into caller order, then the counts' way down
    int finish(int L, uint32_t const * d_orig, uint64_t slots)
    {
        lx_handle::XbLane & ln = h->xb[L];
        LX_HIP(h, lx::launch_slot_scatter(d_orig, slots, static_cast<int32_t const *>(ln.d_score.ptr), static_cast<int32_t *>(h->d_score_all.ptr),
                                          static_cast<uint32_t *>(ln.d_src.ptr), static_cast<uint64_t *>(ln.d_cnt.ptr), x.prep[L].cap_sel, h->stream));
        return x.send_counts(L, 5);
    }

    // ---- wavefronts w0 .. w1 of the plan as one chunk in lane L: staged, uploaded, gathered, kernels, scatter of the scores
    int enqueue(int L, uint64_t w0, uint64_t w1, bool force_wide = false)
    {
        auto const          t0 = now();
        lx_handle::XbLane & ln = h->xb[L];
        XbPrep &            pr = x.prep[L];
        uint64_t const      slots = (w1 - w0) * kWave, nw = w1 - w0, panel = (uint64_t)p.mq_geo.panel();
        pr.k0 = w0, pr.k1 = w1, pr.slots = slots, pr.cap_sel = (slots + 7) / 8 * 8 + 8;
        int rc2;
        if ((!x.preplanned && (rc2 = ensure_pinned(h, ln.p_orig, slots * sizeof(uint32_t), kRoom))) || (rc2 = ensure_pinned(h, ln.p_wft, nw * sizeof(lx::WfSlots), kRoom)))
            return rc2;
        pr.wide         = choose_wide(force_wide);
        Staged const st = stage(L, w0, w1, 0, pr.wide);
        // the promises of the chunk: its widest query (as a panel count) and its longest window
        pr.exec_cells = st.padded, pr.max_s = st.maxs, pr.max_pan = st.pan;
        uint64_t const max_q = (st.pan + panel / 8 - 1) / (panel / 8) * panel; // (whole panels: the slots have one part per panel)
        x.t_prep += ms(t0, now());

        auto const     t1     = now();
        uint64_t const stride = (max_q + st.maxs + 3) & ~3ull;
        if ((rc2 = x.size_lane(L, slots, stride, !x.preplanned, true)) || (rc2 = ensure(h, ln.d_wft, nw * sizeof(lx::WfSlots))) || (rc2 = upload_staged(L, w0, w1, 0, true)))
            return rc2;
        // (ovf_cap: what the chunk's budget reserved, an eighth of its slots)
        // (the solo packing: no run promise; the free packing: pairs of one query, at most four queries per wavefront)
        rc2 = x.run_fused(L, slots, stride, max_q, st.maxs, p.use_solo ? 1 : 2, MqTab{ln.d_wft.ptr, slots, st.dwords, 0, std::min<uint64_t>(slots, slots / 8 + 64), 0, 0}, pr.wide);
        uint32_t const * const d_orig = x.preplanned ? x.ri->d_plan + w0 * kWave : static_cast<uint32_t const *>(ln.d_orig.ptr);
        if (rc2 || (rc2 = finish(L, d_orig, slots)))
            return rc2;
        x.t_issue += ms(t1, now());
        return LX_OK;
    }

    // first call: wavefronts [0, w1) = the pool; cap_slots bounds the chunk's slots, (cap_pan, cap_s) its widest query and longest window,
    // rest_dw is what the second call's slots are expected to take
    int enqueue_first(int L, uint64_t w1, uint64_t cap_slots, uint64_t cap_pan, uint64_t cap_s, uint64_t rest_dw)
    {
        auto const          t0    = now();
        lx_handle::XbLane & ln    = h->xb[L];
        XbPrep &            pr    = x.prep[L];
        uint64_t const      panel = (uint64_t)p.mq_geo.panel(), slots1 = w1 * kWave;
        pr.k0 = 0, pr.k1 = w1, pr.slots = slots1, pr.cap_sel = (cap_slots + 7) / 8 * 8 + 8, pr.max_s = cap_s, pr.max_pan = cap_pan;
        int rc2;
        if ((rc2 = ensure_pinned(h, ln.p_orig, cap_slots * sizeof(uint32_t), kRoom)) || (rc2 = ensure_pinned(h, ln.p_wft, (cap_slots / kWave + 1) * sizeof(lx::WfSlots), kRoom)))
            return rc2;
        pr.wide         = choose_wide(false);
        Staged const st = stage(L, 0, w1, 0, pr.wide);
        pr.exec_cells   = st.padded;
        two             = TwoCall{};
        two.dw0         = st.dwords;
        two.max_q    = (cap_pan + panel / 8 - 1) / (panel / 8) * panel;
        two.max_s     = cap_s;
        two.stride    = (two.max_q + two.max_s + 3) & ~3ull;
        two.cap_slots = cap_slots;
        two.n1        = slots1;
        two.nw1       = w1;
        x.t_prep += ms(t0, now());
        auto const t1 = now();
        if ((rc2 = x.size_lane(L, cap_slots, two.stride, true, true)) || (rc2 = ensure(h, ln.d_wft, (cap_slots / kWave + 1) * sizeof(lx::WfSlots))))
            return rc2;
        // (overflow slots have the size of the chunk's widest query and longest window: an eighth of the slots, within 16 GiB)
        uint64_t const s32 = slot_dwords(p.mq_geo, cap_pan, two.max_s, true);
        two.ovf_cap        = std::min<uint64_t>(std::min<uint64_t>(cap_slots, cap_slots / 8 + 64), std::max<uint64_t>(1024, (4ull << 30) / std::max<uint64_t>(s32, 1)));
        two.ovf_dw         = two.ovf_cap * s32;
        // (reserved now: the pool's slots, the overflow slots, what the caller expects the second call's slots to take -- within the budget)
        two.total_dw = std::max<uint64_t>(two.dw0 + two.ovf_dw, std::min<uint64_t>(h->opt_trace_bytes / 4, two.dw0 + two.ovf_dw + rest_dw));
        if ((rc2 = upload_staged(L, 0, w1, 0, false)))
            return rc2;
        rc2 = x.run_fused(L, cap_slots, two.stride, two.max_q, two.max_s, 2, MqTab{ln.d_wft.ptr, slots1, two.dw0, 0, two.ovf_cap, two.total_dw, 1}, pr.wide);
        x.t_issue += ms(t1, now());
        return rc2;
    }

    // second call: wavefronts [w_mid, w1) of the plan (none: the pool stays a chunk of its own) behind the first call's
    int enqueue_second(int L, uint64_t w_mid, uint64_t w1)
    {
        auto const          t0    = now();
        lx_handle::XbLane & ln    = h->xb[L];
        XbPrep &            pr    = x.prep[L];
        uint64_t const      total = two.n1 + (w1 - w_mid) * kWave;
        int                 rc2;
        Staged const        st = stage(L, w_mid, w1, two.n1, pr.wide);
        pr.exec_cells += st.padded;
        pr.k1    = w1;
        pr.slots = total;
        x.t_prep += ms(t0, now());
        auto const t1 = now();
        if (w1 > w_mid && (rc2 = upload_staged(L, w_mid, w1, two.n1, false)))
            return rc2;
        mq_wide = pr.wide;
        rc2     = x.run_fused(L, total, two.stride, two.max_q, two.max_s, 2, MqTab{ln.d_wft.ptr, two.n1, two.dw0, st.dwords, two.ovf_cap, two.total_dw, 2}, pr.wide);
        if (rc2 || (rc2 = finish(L, static_cast<uint32_t const *>(ln.d_orig.ptr), total)))
            return rc2;
        x.t_issue += ms(t1, now());
        return LX_OK;
    }

    // ---- results of a multi-query chunk: the survivors' records and ops, addressed by caller index (the device translated the list)
    int collect(int L)
    {
        XbPrep &         pr = x.prep[L];
        auto const       t0 = now();
        uint64_t const * cnt;
        int              rc2;
        if ((rc2 = x.wait_counts(L, cnt)))
            return rc2;
        auto const     t_ev  = now();
        uint64_t const count = cnt[0], nrle = cnt[2];
        uint32_t       flags[2];
        std::memcpy(flags, cnt + 3, sizeof(flags));
        if (x.hm.on)
            fprintf(stderr, "[lx host ms]   chunk %llu-%llu: %llu slots%s (%.2f G executed cells, longest window %llu, <= %llu columns per lane), error word %u, %u beyond the codes, %llu survivors\n",
                    (unsigned long long)pr.k0, (unsigned long long)pr.k1, (unsigned long long)pr.slots, pr.wide ? " (wide)" : "", (double)pr.exec_cells / 1e9,
                    (unsigned long long)pr.max_s, (unsigned long long)pr.max_pan, flags[1], (uint32_t)cnt[4], (unsigned long long)cnt[1]);
        if (flags[1] == 4 && !pr.wide && wide_ok())
        {
            // More windows beyond the compact codes than the overflow area holds int16-pair slots for (its slots are sized for the
            // chunk's longest window): the chunk runs again with int16 pairs from the sweep itself, which needs no overflow area.
            // Nothing of this attempt is kept (the scores it scattered are written again).
            redo.push_back({pr.k0, pr.k1});
            h->mq_decl_frac = 1.0;
            return LX_OK;
        }
        if ((rc2 = x.check_counts(pr, cnt)))
            return rc2;
        if (pr.slots)
            h->mq_decl_frac = (double)(uint32_t)cnt[4] / (double)pr.slots;
        if (x.sink.on_device())
            return device_collect(x, L, count, nrle, t0, t_ev);
        if ((rc2 = x.download_survivors(L, count, nrle)))
            return rc2;
        auto const t1 = now();
        x.t_wait += ms(t0, t1);
        if (x.sink.where == XbSink::kRows)
            return rows_of_survivors(x, L, count, t1);
        rc2 = list_append(x, L, count, nrle, nullptr);
        x.t_unpack += ms(t1, now());
        if (x.hm.on)
            fprintf(stderr, "[lx host ms]     ... its counts came after %.2f ms of waiting, its %llu records + %llu code bytes in %.2f more, appended in %.2f\n", ms(t0, t_ev),
                    (unsigned long long)count, (unsigned long long)nrle, ms(t_ev, t1), ms(t1, now()));
        return rc2;
    }
};

} // namespace

int run_chunks_of_wavefronts(Xb & x) { return WfDriver{x}.run(); }

} // namespace lxi
