// lx_host_plan.cpp -- the host plan of lx_extend_batch* (lx_host_plan.h): validation, the order by query slice, the geometry
// classes, and the multi-query sweep's plans.  lx_plan_free.hip plans lists that stand on the device; no HIP call here.
#include "lx_internal.h"
#include "lx_level2_plan.h" // choose_strips
using namespace lxi;

namespace
{

constexpr uint64_t kSub = 4;

// LSD radix sort of `order` by key: three passes of 10 bits (keys have 28)
void radix_sort(std::vector<uint32_t> & order, std::vector<uint32_t> & tmp, std::vector<uint32_t> const & key, uint64_t count)
{
    for (int pass = 0; pass < 3; ++pass)
    {
        int const shift = 10 * pass;
        uint32_t  hist[1025] = {0};
        for (uint64_t o = 0; o < count; ++o)
            ++hist[((key[order[o]] >> shift) & 1023u) + 1];
        bool one_bucket = false;
        for (int bk = 0; bk < 1024; ++bk)
        {
            one_bucket = one_bucket || hist[bk + 1] == count;
            hist[bk + 1] += hist[bk];
        }
        if (one_bucket)
            continue;
        for (uint64_t o = 0; o < count; ++o)
            tmp[hist[(key[order[o]] >> shift) & 1023u]++] = order[o];
        order.swap(tmp);
    }
}

} // namespace

uint64_t lxi::slot_dwords(lx::Geo geo, uint64_t pan, uint64_t maxs, bool wide, bool with_ovf)
{
    uint64_t const pc     = (uint64_t)geo.c;
    uint64_t const panels = std::max<uint64_t>(1, (pan + pc - 1) / pc);
    uint32_t const steps  = mq_steps(maxs);
    uint64_t const d32    = lx::ckpt_slot_dwords(geo, steps);
    return panels * ((wide ? d32 : lx::ckpt16_slot_dwords(geo, steps)) + (with_ovf ? d32 / 8 : 0));
}

bool lxi::mq_sweep_applies(lx_handle const * h, int slot)
{
    SchemeFacts const & f = h->facts[slot];
    return h->opt_mq >= 1 && h->opt_pass2 == 2 && h->opt_f16 && f.trace_ok && f.b8_ok && compact_gaps_ok(f);
}

// the solo packing needs 16 byte profiles in a wavefront's share of the LDS: the alphabets of at most six rows
static bool solo_fits(lx_handle const * h, int slot) { return lx::sweep_mq_lds_bytes(lx::kGeo8x19, h->sc_host[slot].alphabet_size + 1, -1) <= 20 * 1024; }

// does the multi-query sweep serve this slot's lists at all (free packing: what protein lists are planned for)?
bool lxi::free_plan_applies(lx_handle const * h, int slot) { return mq_sweep_applies(h, slot) && !h->opt_band; }

// does lx_extend_batch* serve this slot's lists with the solo packing of the multi-query sweep (a byte profile per window)?
bool lxi::solo_plan_applies(lx_handle const * h, int slot) { return free_plan_applies(h, slot) && solo_fits(h, slot); }

// ---- validate; is the list grouped by query (lambda's lists are sorted by query)?  The loops over the list are spread over a few
// host threads: at millions of extensions per call they would otherwise cost more than the kernels.  A device plan (lx_level2_host.cpp:
// the solo packing of a resident window list) looks at nothing of the list: `ext` may be NULL.
int HostPlan::order(lx_handle * h, lx_extension const * ext_, uint64_t n, uint64_t q_bytes, uint64_t s_bytes, bool as_list, bool preplanned_,
                    int32_t * out_score, lx_hsp * out_hsp, uint64_t * out_ops_off, HostMarks & hm)
{
    ext        = ext_;
    nthreads   = host_threads(n);
    preplanned = preplanned_;
    use_mq = use_solo = false;
    mq_geo            = lx::kGeo8x19;
    mq_cells = nwf = pool_wf = 0;
    starts.clear();
    if (preplanned)
    {
        live = n;
        hm.mark("scan");
        hm.mark("order");
        return LX_OK;
    }
    struct Part
    {
        uint64_t live = 0, bad = ~0ull;
        bool     monotone = true;
    };
    std::vector<Part> parts(nthreads);
    // (the same pass writes what the common case needs -- every extension live, the list grouped by query already: the order
    // is the identity and the runs begin where the slice changes)
    idx.resize(n);
    newrun.resize(n + 1);
    parallel_ranges(n, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        Part     pt;           // (a local: the per-thread slots share cache lines)
                        uint64_t prev = ~0ull; // last live extension before i (of the whole list)
                        for (uint64_t i = lo; i-- > 0;)
                            if (ext[i].q_len != 0 && ext[i].s_len != 0)
                            {
                                prev = i;
                                break;
                            }
                        for (uint64_t i = lo; i < hi; ++i)
                        {
                            lx_extension const & x = ext[i];
                            if (!lx_slice_ok(x.q_off, x.q_len, q_bytes) || !lx_slice_ok(x.s_off, x.s_len, s_bytes))
                            {
                                pt.bad = std::min(pt.bad, i);
                                continue;
                            }
                            if (x.q_len == 0 || x.s_len == 0)
                            {
                                out_score[i] = 0;
                                if (!as_list)
                                {
                                    out_hsp[i]     = lx_hsp{};
                                    out_ops_off[i] = 0;
                                }
                                continue;
                            }
                            if (prev != ~0ull && x.q_off < ext[prev].q_off)
                                pt.monotone = false;
                            idx[i]    = (uint32_t)i;
                            newrun[i] = (i == 0 || x.q_off != ext[i - 1].q_off || x.q_len != ext[i - 1].q_len) ? 1 : 0;
                            prev      = i;
                            ++pt.live;
                        }
                        parts[t] = pt;
                    });
    live          = 0;
    bool monotone = true;
    for (Part const & pt : parts)
    {
        if (pt.bad != ~0ull)
            return fail(h, LX_EINVAL, "extension %llu exceeds the residue buffers", (unsigned long long)pt.bad);
        live += pt.live;
        monotone = monotone && pt.monotone;
    }
    if (live == 0)
        return LX_OK;
    hm.mark("scan");
    bool const as_given = live == n && monotone;
    idx.resize(live);
    if (!as_given)
    {
        std::vector<uint64_t> first(nthreads + 1, 0);
        for (unsigned t = 0; t < nthreads; ++t)
            first[t + 1] = first[t] + parts[t].live;
        parallel_ranges(n, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint64_t o = first[t];
                            for (uint64_t i = lo; i < hi; ++i)
                                if (ext[i].q_len != 0 && ext[i].s_len != 0)
                                    idx[o++] = (uint32_t)i;
                        });
    }
    if (!monotone) // anything else is sorted first: equal slices become adjacent
        std::sort(idx.begin(), idx.end(),
                  [&](uint32_t a, uint32_t b)
                  {
                      lx_extension const &x = ext[a], &y = ext[b];
                      return x.q_off != y.q_off ? x.q_off < y.q_off : x.q_len != y.q_len ? x.q_len < y.q_len : a < b;
                  });
    newrun.resize(live + 1);
    if (!as_given)
        mark_runs();
    newrun[live] = 1;
    hm.mark("order");
    return LX_OK;
}

// where the runs of one query slice begin in the ordered list
void HostPlan::mark_runs()
{
    parallel_ranges(live, nthreads,
                    [&](unsigned, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t k = lo; k < hi; ++k)
                            newrun[k] = (k == 0 || ext[idx[k]].q_off != ext[idx[k - 1]].q_off || ext[idx[k]].q_len != ext[idx[k - 1]].q_len) ? 1 : 0;
                    });
}

// positions where the runs of one query slice begin, + the sentinel `live` (two parallel passes over newrun)
void HostPlan::run_starts()
{
    std::vector<uint64_t> cnt(nthreads + 1, 0);
    parallel_ranges(live + 1, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        uint64_t c = 0;
                        for (uint64_t k = lo; k < hi; ++k)
                            c += newrun[k];
                        cnt[t + 1] = c;
                    });
    for (unsigned t = 0; t < nthreads; ++t)
        cnt[t + 1] += cnt[t];
    starts.resize(cnt[nthreads]);
    parallel_ranges(live + 1, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        uint64_t o = cnt[t];
                        for (uint64_t k = lo; k < hi; ++k)
                            if (newrun[k])
                                starts[o++] = k;
                    });
}

// Multi-query sweep (lx_sweep_mq.hip) for lists that are not uniform: sub-blocks of 4 windows of one query, ordered by (geometry
// class, longest window) ACROSS queries, four sub-blocks per wavefront -- see plan_pool.  Needs what plan_step's multi-query candidate needs;
// uniform lists (one query length, one window length, runs that fill whole wavefronts) stay on the one-query-per-wavefront kernels.
// The SOLO packing of that sweep (LX_OPT_QUERY_RUN = 1): a byte profile per window, 16 windows of any queries per wavefront -- where
// 16 profiles fit a wavefront's share of the LDS (nucleotides, bisulfite).  A read set's seed list has one or two windows per read:
// at four queries per wavefront three slots in four were fillers (configs[2]-sized list: 4.1 M slots for 1.25 M windows).
int HostPlan::choose(lx_handle * h, int slot, ResidentInput const * ri, bool as_list)
{
    use_mq   = mq_sweep_applies(h, slot);
    use_solo = preplanned ? !ri->free_packing : (use_mq && solo_fits(h, slot));
    if (preplanned)
        return use_mq && as_list ? LX_OK : fail(h, LX_ESTATE, "a device plan needs the multi-query sweep and the list form");
    struct Scan
    {
        uint32_t cmin = ~0u, cmax = 0;
        bool     ragged = false;
    };
    std::vector<Scan> scans(nthreads);
    parallel_ranges(live, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        Scan sc; // (a local: the per-thread slots share cache lines)
                        for (uint64_t k = lo; k < hi; ++k)
                        {
                            if (newrun[k])
                            {
                                uint32_t const c = query_class(ext[idx[k]].q_len);
                                sc.cmin = std::min(sc.cmin, c);
                                sc.cmax = std::max(sc.cmax, c);
                            }
                            else if (ext[idx[k]].s_len != ext[idx[k - 1]].s_len)
                                sc.ragged = true;
                        }
                        scans[t] = sc;
                    });
    cls_min = ~0u, cls_max = 0, ragged = false;
    for (Scan const & sc : scans)
    {
        cls_min = std::min(cls_min, sc.cmin);
        cls_max = std::max(cls_max, sc.cmax);
        ragged  = ragged || sc.ragged;
    }
    if (use_mq && cls_min == cls_max && !ragged && h->opt_mq < 2)
    {
        // one geometry, one window length: uniform if every run fills whole wavefronts
        run_starts();
        bool all16 = true;
        for (size_t r = 0; r + 1 < starts.size() && all16; ++r)
            all16 = (starts[r + 1] - starts[r]) % 16 == 0;
        if (all16)
            use_mq = false;
    }
    return LX_OK;
}

// Mixed query lengths (a real seed list; the synthetic batches have one): a chunk runs the kernel geometry of its longest query, so
// runs are dealt to geometry classes first and every class goes through the pipeline by itself.  Inside a run the windows are ordered
// by length (merged windows are up to 3 x longer: src/search_algo.hpp:1153-1157), so that a wavefront's 16 windows take about as many
// steps each -- the reason the reference sorts its SIMD batches (:1229-1235).  Results are scattered by original index anyway.
void HostPlan::sort(HostMarks & hm)
{
    if (!preplanned && cls_min != cls_max && !use_mq)
    {
        std::vector<uint64_t> at(cls_max + 2, 0);
        for (uint64_t k = 0; k < live;)
        {
            uint64_t kk = k + 1;
            while (!newrun[kk])
                ++kk;
            at[query_class(ext[idx[k]].q_len) + 1] += kk - k;
            k = kk;
        }
        for (uint32_t c = 0; c <= cls_max; ++c)
            at[c + 1] += at[c];
        idx_tmp.resize(live);
        for (uint64_t k = 0; k < live;)
        {
            uint64_t kk = k + 1;
            while (!newrun[kk])
                ++kk;
            uint64_t & o = at[query_class(ext[idx[k]].q_len)];
            std::copy(idx.begin() + k, idx.begin() + kk, idx_tmp.begin() + o);
            o += kk - k;
            k = kk;
        }
        idx.swap(idx_tmp);
        mark_runs();
    }
    if (!preplanned && ragged && !(use_mq && use_solo)) // (the solo plan sorts all windows itself)
    {
        run_starts();
        parallel_ranges(starts.size() - 1, nthreads,
                        [&](unsigned, uint64_t lo, uint64_t hi)
                        {
                            for (uint64_t r = lo; r < hi; ++r)
                                std::sort(idx.begin() + starts[r], idx.begin() + starts[r + 1],
                                          [&](uint32_t a, uint32_t b) { return ext[a].s_len != ext[b].s_len ? ext[a].s_len < ext[b].s_len : a < b; });
                        });
    }
    hm.mark("classes+sort");
}

// columns per lane a query sweeps over all its panels (its class in the plan's keys; what a wavefront executes is 8 of them per
// step): whole panels, the last one with the narrowest strips that cover what is left (lx_device.h: narrow_code_for)
uint32_t HostPlan::mq_panels(uint32_t lq) const
{
    int const      C     = mq_geo.c;
    uint64_t const panel = (uint64_t)mq_geo.panel();
    uint64_t const P     = std::max<uint64_t>(1, ((uint64_t)lq + panel - 1) / panel);
    int const      rem   = (int)((uint64_t)std::max<uint32_t>(lq, 1) - (P - 1) * panel);
    int const      code  = lx::narrow_code_for(C, 8, rem);
    return (uint32_t)std::min<uint64_t>(0xfff, (P - 1) * (uint64_t)C + (uint64_t)lx::narrow_strip_cols(C, code));
}

void HostPlan::grow_plan(uint64_t wavefronts)
{
    if (plan_slot.size() < wavefronts * kWave)
        plan_slot.resize(wavefronts * kWave);
    if (wf_pan.size() < wavefronts)
    {
        wf_pan.resize(wavefronts);
        wf_maxs.resize(wavefronts);
    }
}

// ---- multi-query plan (free packing of lx_sweep_mq.hip: the two windows of a lane group share a query, a wavefront's 16 slots hold
// windows of at most four queries in any split).  Inside a run the windows are sorted by length; those clearly longer than the run's
// median -- the merged windows, up to 3 x longer (src/search_algo.hpp:1153-1157) -- go to the POOL in sub-blocks of 4 (filled up with
// the run's longest ordinary windows), the sub-blocks of the whole list are sorted by (columns per lane their query sweeps -- whole
// panels + the narrow last one --, longest window) and dealt four to a wavefront: a long window stretches three companions, not
// fifteen.  Everything else is STREAMED (plan_stream).  What is missing to a pair or a wavefront is filled with copies of the last
// window (as the reference pads its SIMD batches, :1063-1067): they cost what the window costs and never survive (cut-off INT_MAX).
// The plan is the slot list of the whole call (the caller's index per slot) + columns per lane and longest window per wavefront;
// chunks are ranges of wavefronts.
void HostPlan::plan_pool(ResidentInput const * ri, HostMarks & hm)
{
    if (use_mq && preplanned)
    {
        mq_geo   = ri->mq_geo;
        mq_cells = ri->cells;
        nwf = pool_wf = ri->nwf;
        wf_pan.assign(ri->wf_pan, ri->wf_pan + nwf);
        wf_maxs.assign(ri->wf_maxs, ri->wf_maxs + nwf);
    }
    else if (use_mq)
    {
        if (starts.empty())
            run_starts();
        choose_cfg();
        if (use_solo)
            plan_solo(hm);
        else
            plan_free_pool(hm);
    }
    hm.mark("plan");
}

// ONE strip geometry per call, the one that sweeps the fewest padded columns over the whole list (weighted by the instructions a
// column costs at that width): every further geometry is a further pair of launches, and the backtrace of a chunk with a few ten
// thousand survivors is bound by the latency of its longest walks (~1 ms), not by its work -- measured on the ragged list of
// bench.py: (8,11) + (8,13) + (8,19) chosen per query 28.5 % padded cells but 27-31 ms, one geometry 34.5 % / 39.9 % padded and
// 22.7-24.2 ms.
void HostPlan::choose_cfg()
{
    uint64_t const      nruns   = starts.size() - 1;
    int const           cand[3] = {19, 13, 11}; // columns per lane, in choose_strips' order
    std::vector<double> tc(3 * (size_t)nthreads, 0.0);
    parallel_ranges(nruns, nthreads,
                    [&](unsigned t, uint64_t rlo, uint64_t rhi)
                    {
                        double c[3] = {0, 0, 0};
                        for (uint64_t r = rlo; r < rhi; ++r)
                        {
                            uint64_t const lq = ext[idx[starts[r]]].q_len, nw = use_solo ? starts[r + 1] - starts[r] : (starts[r + 1] - starts[r] + 1) / 2 * 2;
                            for (int k = 0; k < 3; ++k)
                            {
                                uint64_t const panel = 8 * (uint64_t)cand[k], P = std::max<uint64_t>(1, (lq + panel - 1) / panel);
                                int const      Cc = cand[k], rem = (int)(std::max<uint64_t>(lq, 1) - (P - 1) * panel);
                                int const      code = lx::narrow_code_for(Cc, 8, rem);
                                // (a step costs 3.75 instructions per column and 12 besides, whatever the strip width)
                                c[k] += (double)nw * ((double)(P - 1) * (3.75 * Cc + 12.0) + 3.75 * lx::narrow_strip_cols(Cc, code) + 12.0);
                            }
                        }
                        for (int k = 0; k < 3; ++k)
                            tc[3 * t + k] = c[k];
                    });
    double cost[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k)
        for (unsigned t = 0; t < nthreads; ++t)
            cost[k] += tc[3 * t + k];
    // (narrower strips must save 15 %: more panels -- carries, profile builds -- and more tiles per walk in the backtrace; measured on
    // the ragged list of bench.py: 22.2 / 21.5 ms with 13 / 11 columns against 19.7 ms with 19, at 8 / 10 % fewer cells)
    mq_geo = choose_strips(cost);
}

// The solo plan is a sort: all windows by (columns per lane, length), longest first, 16 to a wavefront.  Keys: most columns per
// lane first, longest window first inside a width (28 bits); a stable LSD radix sort over the host threads (10 bits per pass:
// per-thread counts of a contiguous share, one scan, one scatter).
void HostPlan::plan_solo(HostMarks & hm)
{
    std::vector<uint32_t> &key = sb_key, &ord = sb_order, &tmp = sb_tmp;
    key.resize(live);
    ord.resize(live);
    tmp.resize(live);
    std::vector<uint64_t> tcells_plan(nthreads, 0);
    std::vector<uint32_t> tor(nthreads, 0), tand(nthreads, ~0u);
    parallel_ranges(live, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        uint64_t cells_t = 0;
                        uint32_t o = 0, a = ~0u;
                        for (uint64_t k = lo; k < hi; ++k)
                        {
                            lx_extension const & x = ext[idx[k]];
                            cells_t += (uint64_t)x.q_len * x.s_len;
                            uint32_t const kk = ((0xfffu - mq_panels(x.q_len)) << 16) | (0xffffu - std::min<uint32_t>(x.s_len, 0xffffu));
                            key[k] = kk;
                            ord[k] = (uint32_t)k;
                            o |= kk;
                            a &= kk;
                        }
                        tcells_plan[t] = cells_t;
                        tor[t]         = o;
                        tand[t]        = a;
                    });
    mq_cells         = 0;
    uint32_t varying = 0; // bits in which the keys differ
    {
        uint32_t o = 0, a = ~0u;
        for (unsigned t = 0; t < nthreads; ++t)
        {
            mq_cells += tcells_plan[t];
            o |= tor[t];
            a &= tand[t];
        }
        varying = o & ~a;
    }
    std::vector<uint32_t> cnt((size_t)nthreads * 1024);
    for (int shift = 0; shift < 30; shift += 10)
    {
        if (!((varying >> shift) & 1023u))
            continue;
        parallel_ranges(live, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint32_t * const c = cnt.data() + (size_t)t * 1024;
                            std::fill(c, c + 1024, 0u);
                            for (uint64_t k = lo; k < hi; ++k)
                                ++c[(key[ord[k]] >> shift) & 1023u];
                        });
        uint32_t at = 0;
        for (int b = 0; b < 1024; ++b)
            for (unsigned t = 0; t < nthreads; ++t)
            {
                uint32_t const c          = cnt[(size_t)t * 1024 + b];
                cnt[(size_t)t * 1024 + b] = at;
                at += c;
            }
        parallel_ranges(live, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint32_t * const c = cnt.data() + (size_t)t * 1024;
                            for (uint64_t k = lo; k < hi; ++k)
                                tmp[c[(key[ord[k]] >> shift) & 1023u]++] = ord[k];
                        });
        ord.swap(tmp);
    }
    nwf     = (live + kWave - 1) / kWave;
    pool_wf = nwf;
    grow_plan(nwf);
    parallel_ranges(nwf, nthreads,
                    [&](unsigned, uint64_t wlo, uint64_t whi)
                    {
                        for (uint64_t w = wlo; w < whi; ++w)
                        {
                            uint32_t pan = 0, maxs = 0;
                            for (uint64_t j = 0; j < kWave; ++j)
                            {
                                uint64_t const o = w * kWave + j;
                                uint32_t const i = idx[ord[std::min(o, live - 1)]]; // (the last wavefront repeats the last window as filler)
                                plan_slot[o]     = i | (o < live ? 0u : 0x80000000u);
                                pan              = std::max(pan, mq_panels(ext[i].q_len));
                                maxs             = std::max(maxs, ext[i].s_len);
                            }
                            wf_pan[w]  = pan;
                            wf_maxs[w] = maxs;
                        }
                    });
    hm.mark("solo plan");
}

// The pool of the free packing.  It goes to the GPU first -- the longest windows of the list -- and the streamed part is planned
// beside its kernels (plan_stream).
void HostPlan::plan_free_pool(HostMarks & hm)
{
    uint64_t const nruns = starts.size() - 1;
    // (1) per run: where its pool begins (the long windows + what fills their last sub-block up), its sub-blocks, its cells
    pool_at.assign(nruns, 0);
    std::vector<uint64_t> sb_off(nruns + 1, 0), tcells_plan(nthreads, 0);
    run_key.resize(nruns);
    parallel_ranges(nruns, nthreads,
                    [&](unsigned t, uint64_t rlo, uint64_t rhi)
                    {
                        uint64_t cells_t = 0;
                        for (uint64_t r = rlo; r < rhi; ++r)
                        {
                            uint64_t const a = starts[r], b = starts[r + 1];
                            uint64_t const med = ext[idx[a + (b - a - 1) / 2]].s_len, thr = med + std::max<uint64_t>(8, med / 8);
                            uint64_t       cut = b; // first long window
                            while (cut > a && ext[idx[cut - 1]].s_len > thr)
                                --cut;
                            for (uint64_t k = a; k < b; ++k)
                                cells_t += (uint64_t)ext[idx[k]].q_len * ext[idx[k]].s_len;
                            uint64_t const nsb_r = (b - cut + kSub - 1) / kSub;
                            pool_at[r]           = nsb_r * kSub >= b - a ? a : b - nsb_r * kSub;
                            sb_off[r + 1]        = nsb_r;
                            // the streamed part's place in the packing order: most panels first, longest windows first
                            if (pool_at[r] != a)
                                run_key[r] = ((0xfffu - mq_panels(ext[idx[a]].q_len)) << 16) |
                                             (0xffffu - std::min<uint32_t>(ext[idx[pool_at[r] - 1]].s_len, 0xffffu));
                        }
                        tcells_plan[t] = cells_t;
                    });
    mq_cells = 0;
    for (uint64_t c : tcells_plan)
        mq_cells += c;
    for (uint64_t r = 0; r < nruns; ++r)
        sb_off[r + 1] += sb_off[r];
    uint64_t const nsb = sb_off[nruns];
    sb_first.resize(nsb);
    sb_key.resize(nsb);
    sb_order.resize(nsb);
    sb_tmp.resize(nsb);
    sb_cnt.resize(nsb);
    // the pool's sub-blocks: sub-block j of a run (0 = its longest windows) = positions [max(pool, b - 4 (j + 1)), b - 4 j)
    parallel_ranges(nruns, nthreads,
                    [&](unsigned, uint64_t rlo, uint64_t rhi)
                    {
                        for (uint64_t r = rlo; r < rhi; ++r)
                        {
                            uint32_t const cls = 0xfffu - mq_panels(ext[idx[starts[r]]].q_len);
                            uint64_t       e   = starts[r + 1];
                            for (uint64_t o = sb_off[r]; o < sb_off[r + 1]; ++o)
                            {
                                uint64_t const first = std::max<uint64_t>(pool_at[r], e >= kSub ? e - kSub : 0);
                                sb_first[o] = (uint32_t)first;
                                sb_cnt[o]   = (uint8_t)(e - first);
                                // (most panels first, longest first inside a panel count: the wavefronts that run longest
                                // start first, the tail of the launch is made of short ones)
                                sb_key[o] = (cls << 16) | (0xffffu - std::min<uint32_t>(ext[idx[e - 1]].s_len, 0xffffu));
                                e         = first;
                            }
                        }
                    });
    hm.mark("sub-blocks");
    for (uint64_t o = 0; o < nsb; ++o)
        sb_order[o] = (uint32_t)o;
    radix_sort(sb_order, sb_tmp, sb_key, nsb);
    // (2) four sub-blocks per wavefront
    pool_wf = (nsb + 3) / 4;
    nwf     = pool_wf;
    grow_plan(nwf);
    // The wavefronts are made of neighbours in that order (a wavefront runs as many columns per lane as its widest query has and as
    // many steps as its longest window) and LAUNCHED longest first: what a wavefront executes is columns x steps, and the blocks of a
    // launch are dealt to the chip's wavefront slots in index order -- with two or three wavefronts per slot (a list of long queries)
    // the launch is as long as its unluckiest slot, which longest-first keeps at the longest wavefront itself.
    pool_pan.resize(pool_wf);
    pool_maxs.resize(pool_wf);
    pool_place.resize(pool_wf);
    parallel_ranges(pool_wf, nthreads,
                    [&](unsigned, uint64_t wlo, uint64_t whi)
                    {
                        for (uint64_t w = wlo; w < whi; ++w)
                        {
                            uint32_t pan = 0, maxs = 0;
                            for (uint64_t o = 4 * w; o < 4 * w + 4; ++o)
                            {
                                uint32_t const sb    = sb_order[std::min(o, nsb - 1)];
                                uint64_t const first = sb_first[sb], cnt = sb_cnt[sb];
                                pan = std::max(pan, 0xfffu - (sb_key[sb] >> 16));
                                for (uint64_t j = 0; j < cnt; ++j)
                                    maxs = std::max(maxs, ext[idx[first + j]].s_len);
                            }
                            pool_pan[w]  = pan;
                            pool_maxs[w] = maxs;
                        }
                    });
    pool_order.resize(pool_wf);
    pool_key.resize(pool_wf);
    pool_tmp.resize(pool_wf);
    for (uint64_t w = 0; w < pool_wf; ++w)
    {
        pool_order[w] = (uint32_t)w;
        pool_key[w]   = 0x3fffffffu - (uint32_t)std::min<uint64_t>((uint64_t)pool_pan[w] * (pool_maxs[w] + 7), 0x3fffffffu);
    }
    radix_sort(pool_order, pool_tmp, pool_key, pool_wf);
    for (uint64_t k = 0; k < pool_wf; ++k)
        pool_place[pool_order[k]] = (uint32_t)k;
    parallel_ranges(pool_wf, nthreads,
                    [&](unsigned, uint64_t wlo, uint64_t whi)
                    {
                        for (uint64_t w = wlo; w < whi; ++w)
                        {
                            uint64_t const at = pool_place[w]; // (its place in the launch)
                            for (uint64_t o = 4 * w; o < 4 * w + 4; ++o)
                            {
                                // (a wavefront that the pool cannot fill repeats its last sub-block as fillers)
                                bool const     real  = o < nsb;
                                uint32_t const sb    = sb_order[std::min(o, nsb - 1)];
                                uint64_t const first = sb_first[sb], cnt = sb_cnt[sb];
                                // (the longest window first, like the streamed pairs; the last one is repeated as filler)
                                for (uint64_t j = 0; j < kSub; ++j)
                                    plan_slot[at * kWave + (o - 4 * w) * kSub + j] =
                                      idx[first + cnt - 1 - std::min(j, cnt - 1)] | ((real && j < cnt) ? 0u : 0x80000000u);
                            }
                            wf_pan[at]  = pool_pan[w];
                            wf_maxs[at] = pool_maxs[w];
                        }
                    });
    hm.mark("pool");
}

// Runs [lo, hi) of the packing order into wavefronts (out_slot NULL: only counted): their windows pair by pair, a wavefront closed
// when it holds eight pairs or meets a fifth query -- the windows of a wavefront take about the same number of steps, and a query
// with five windows costs three lane groups, not two sub-blocks
uint64_t HostPlan::pack_runs(uint64_t lo, uint64_t hi, uint32_t * out_slot, uint32_t * out_pan, uint32_t * out_maxs) const
{
    uint32_t wq[4] = {0, 0, 0, 0}; // runs of the open wavefront
    uint32_t nq = 0, npairs = 0, pan = 0, maxs = 0, last = 0;
    uint64_t done = 0;             // wavefronts closed
    auto     close = [&]()
    {
        if (npairs == 0)
            return;
        if (out_slot)
        {
            for (uint32_t k = 2 * npairs; k < kWave; ++k)
                out_slot[done * kWave + k] = last | 0x80000000u;
            out_pan[done]  = pan;
            out_maxs[done] = maxs;
        }
        ++done;
        nq = npairs = pan = maxs = 0;
    };
    for (uint64_t x = lo; x < hi; ++x)
    {
        uint32_t const r  = run_order[x];
        uint32_t const rp = 0xfffu - (run_key[r] >> 16);
        // (longest first: the order descends over the runs, so it does inside one)
        for (uint64_t e = pool_at[r]; e > starts[r];)
        {
            if (npairs == kWave / 2)
                close();
            bool known = false;
            for (uint32_t k = 0; k < nq; ++k)
                known = known || wq[k] == r;
            if (!known)
            {
                if (nq == 4)
                    close();
                wq[nq++] = r;
            }
            bool const two = e - 1 > starts[r];
            if (out_slot)
            {
                uint32_t const i0 = idx[e - 1], i1 = two ? idx[e - 2] : (i0 | 0x80000000u);
                out_slot[done * kWave + 2 * npairs]     = i0;
                out_slot[done * kWave + 2 * npairs + 1] = i1;
                last                                    = i1;
                maxs                                    = std::max(maxs, ext[i0].s_len);
                pan                                     = std::max(pan, rp);
            }
            ++npairs;
            e -= two ? 2 : 1;
        }
    }
    close();
    return done;
}

HostPlan::StreamBound HostPlan::stream_bound(bool wide) const
{
    StreamBound    b;
    uint64_t const nruns = starts.size() - 1;
    for (uint64_t r = 0; r < nruns; ++r)
        if (pool_at[r] != starts[r])
        {
            uint64_t const cnt = pool_at[r] - starts[r], pan = 0xfffu - (run_key[r] >> 16), maxs = ext[idx[pool_at[r] - 1]].s_len;
            b.windows += cnt;
            ++b.runs;
            b.pan  = std::max(b.pan, pan);
            b.maxs = std::max(b.maxs, maxs);
            b.dwords += (cnt + 1) / 2 * 2 * slot_dwords(mq_geo, pan, maxs, wide);
        }
    return b;
}

// The streamed part: the runs in order of (columns per lane, ordinary window length), most panels and longest first, packed behind
// the pool.  What is missing to a pair or a wavefront is a copy of the last window.
void HostPlan::plan_stream()
{
    uint64_t const nruns = starts.size() - 1;
    run_order.resize(nruns);
    run_tmp.resize(nruns);
    uint64_t nstream_runs = 0;
    for (uint64_t r = 0; r < nruns; ++r)
        if (pool_at[r] != starts[r]) // (else the whole run stands in the pool)
            run_order[nstream_runs++] = (uint32_t)r;
    radix_sort(run_order, run_tmp, run_key, nstream_runs);
    // every thread packs a contiguous share of the sorted runs into wavefronts of its own (a share starts a new wavefront): once to
    // count them, once -- the offsets known -- to write the plan
    std::vector<uint64_t> wf_at(nthreads + 1, pool_wf);
    parallel_ranges(nstream_runs, nthreads, [&](unsigned t, uint64_t lo, uint64_t hi) { wf_at[t + 1] = pack_runs(lo, hi, nullptr, nullptr, nullptr); });
    for (unsigned t = 0; t < nthreads; ++t)
        wf_at[t + 1] += wf_at[t];
    nwf = wf_at[nthreads];
    grow_plan(nwf);
    parallel_ranges(nstream_runs, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    { (void)pack_runs(lo, hi, plan_slot.data() + wf_at[t] * kWave, wf_pan.data() + wf_at[t], wf_maxs.data() + wf_at[t]); });
}

// wavefronts [wlo, whi) of the plan in launch order = longest first (what a wavefront executes is columns x steps; the blocks of a
// launch are dealt to the chip's wavefront slots in index order, so a long wavefront late in the order ends the launch late)
void HostPlan::longest_first(uint64_t wlo, uint64_t whi)
{
    if (whi <= wlo + 1)
        return;
    uint64_t const          cnt = whi - wlo;
    std::vector<uint32_t> & by_len = pool_order, &tmp_slot = pool_place, &tmp_pan = pool_pan, &tmp_maxs = pool_maxs;
    by_len.resize(cnt);
    pool_tmp.resize(cnt);
    pool_key.resize(whi);
    for (uint64_t k = 0; k < cnt; ++k)
    {
        by_len[k]         = (uint32_t)(wlo + k);
        pool_key[wlo + k] = 0x3fffffffu - (uint32_t)std::min<uint64_t>((uint64_t)wf_pan[wlo + k] * (wf_maxs[wlo + k] + 7), 0x3fffffffu);
    }
    radix_sort(by_len, pool_tmp, pool_key, cnt);
    tmp_slot.resize(cnt * kWave);
    tmp_pan.resize(cnt);
    tmp_maxs.resize(cnt);
    parallel_ranges(cnt, nthreads,
                    [&](unsigned, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t k = lo; k < hi; ++k)
                        {
                            std::memcpy(tmp_slot.data() + k * kWave, plan_slot.data() + (uint64_t)by_len[k] * kWave, kWave * sizeof(uint32_t));
                            tmp_pan[k]  = wf_pan[by_len[k]];
                            tmp_maxs[k] = wf_maxs[by_len[k]];
                        }
                    });
    parallel_ranges(cnt, nthreads,
                    [&](unsigned, uint64_t lo, uint64_t hi)
                    {
                        std::memcpy(plan_slot.data() + (wlo + lo) * kWave, tmp_slot.data() + lo * kWave, (hi - lo) * kWave * sizeof(uint32_t));
                        std::memcpy(wf_pan.data() + wlo + lo, tmp_pan.data() + lo, (hi - lo) * sizeof(uint32_t));
                        std::memcpy(wf_maxs.data() + wlo + lo, tmp_maxs.data() + lo, (hi - lo) * sizeof(uint32_t));
                    });
}

// ---- cutting the plan into chunks

uint64_t HostPlan::run_chunk_end(uint64_t k0, uint64_t chunk_target) const
{
    uint64_t k1 = std::min<uint64_t>(live, k0 + chunk_target);
    while (k1 < live && !newrun[k1])
        ++k1;
    uint32_t const c0 = query_class(ext[idx[k0]].q_len);
    if (query_class(ext[idx[k1 - 1]].q_len) != c0)
    {
        uint64_t lo = k0, hi = k1 - 1; // first position of another class: the classes ascend
        while (hi - lo > 1)
        {
            uint64_t const mid = lo + (hi - lo) / 2;
            (query_class(ext[idx[mid]].q_len) == c0 ? lo : hi) = mid;
        }
        k1 = hi;
        while (k1 > k0 + 1 && !newrun[k1])
            --k1;
    }
    return k1;
}

// The chunk's checkpoint slots must fit the trace budget (fused_impl leaves the sweep otherwise): every slot is sized for the chunk's
// widest query and longest window -- compact codes, int16 pairs where the chunk may run WIDE -- plus room for the int32 overflow slots
// of what the sweep may decline; the chunk ends where one more wavefront would break the budget, or where the pool ends.
uint64_t HostPlan::wf_chunk_end(uint64_t w0, uint64_t per_chunk, uint64_t trace_bytes, bool maybe_wide, bool cut_at_pool) const
{
    uint64_t       w1 = w0, run_bytes = 0, run_q = 1, run_s = 1;
    uint64_t const pool_end = (use_solo || preplanned) ? 0 : pool_wf;
    while (w1 < nwf && w1 - w0 < per_chunk)
    {
        if (cut_at_pool && w0 < pool_end && w1 == pool_end)
            break;
        uint64_t const b2 = run_bytes + kWave * slot_dwords(mq_geo, wf_pan[w1], wf_maxs[w1], maybe_wide, true) * 4;
        uint64_t const q2 = std::max<uint64_t>(run_q, wf_pan[w1]), s2 = std::max<uint64_t>(run_s, wf_maxs[w1]);
        if (w1 > w0 && !chunk_fits(b2, trace_bytes, (w1 + 1 - w0) * kWave, q2 * 8 + s2))
            break;
        run_bytes = b2, run_q = q2, run_s = s2;
        ++w1;
    }
    return w1;
}

uint64_t HostPlan::redo_piece_end(uint64_t a, uint64_t end, uint64_t trace_bytes) const
{
    uint64_t b = a, bytes = 0;
    while (b < end)
    {
        uint64_t const wb = wf_dwords(b, true) * 4;
        if (b > a && !chunk_fits(bytes + wb, trace_bytes, 0, 0))
            break;
        bytes += wb;
        ++b;
    }
    return b;
}

bool HostPlan::ranges_admitted(uint64_t const * cut_wf, uint64_t n_ranges, uint64_t per_chunk, uint64_t trace_bytes, bool wide_ok) const
{
    bool ok = cut_wf[0] == 0 && cut_wf[n_ranges] == nwf;
    for (uint64_t r = 0; r < n_ranges && ok; ++r)
    {
        uint64_t const a = cut_wf[r], b = cut_wf[r + 1];
        uint64_t       pm = 1, sm = 1;
        for (uint64_t w = a; w < b; ++w)
        {
            pm = std::max<uint64_t>(pm, wf_pan[w]);
            sm = std::max<uint64_t>(sm, wf_maxs[w]);
        }
        uint64_t const slot_b = slot_dwords(mq_geo, pm, sm, false, true) * 4;
        // (a range whose sweep overflows runs again WHOLE with int16-pair slots, about twice the codes': admitted against those too)
        uint64_t const slot_w = wide_ok ? slot_dwords(mq_geo, pm, sm, true) * 4 : 0;
        ok = a < b && b - a <= 4 * per_chunk && chunk_fits((b - a) * kWave * std::max(slot_b, slot_w), trace_bytes, (b - a) * kWave, pm * 8 + sm);
    }
    return ok;
}
