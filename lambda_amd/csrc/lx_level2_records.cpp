// lx_level2_records.cpp -- RecordsJob: the records of a Level-2 call from survivors that the extension pipeline left on the device
// (lx_records.hip, lx_toprec.hip), brought into the call's result.  lx_level2_host.cpp drives it; lx_level2_host.h says what it is.
#include <thread>

#include "lx_level2_host.h"

using namespace lxi;

int lxi::ensure_records(lx_handle * h, uint64_t rows, uint64_t max_win, uint64_t max_entries, uint64_t nr, uint64_t nr_pinned)
{
    auto &         l2    = h->l2;
    uint64_t const tiles = (max_entries + 255) / 256;
    int            rc;
    if ((rc = ensure(h, l2.d_listat, max_win * sizeof(uint32_t) + 16)) || (rc = ensure(h, l2.d_reccnt, nr * lx::kRecCounters * sizeof(uint64_t))) ||
        (rc = ensure(h, l2.d_rec, rows * sizeof(lx_blast_match) + 16)) || (rc = ensure(h, l2.d_reccodes, 3 * rows * sizeof(uint64_t) + 16)) ||
        (rc = ensure(h, l2.d_tilekeep, (tiles + 1) * sizeof(uint32_t))) || (rc = ensure(h, l2.d_tileops, (tiles + 1) * sizeof(uint64_t))) ||
        (rc = ensure_pinned(h, l2.p_reccnt, nr_pinned * lx::kRecCounters * sizeof(uint64_t), kRoom)))
        return rc;
    return LX_OK;
}

int lxi::ensure_top_records(lx_handle * h, uint64_t rows, uint64_t max_win, uint64_t nr, CullRequest const * cull)
{
    auto & l2 = h->l2;
    int    rc;
    if ((rc = ensure(h, l2.d_toprows, rows * sizeof(lx_blast_match) + 16)) ||
        (rc = ensure(h, l2.d_topwork, lx::toprec_work_bytes(max_win, cull && cull->max_hsps, cull && cull->culling_limit))) ||
        (rc = ensure(h, l2.d_topcnt, nr * lx::kTopCounters * sizeof(uint64_t))))
        return rc;
    return LX_OK;
}

int lxi::top_account(lx_handle * h, uint64_t const * tc, uint64_t nrec, uint64_t max_ops, lx_record_stats * stats, lx_cull_stats * cull_stats)
{
    // (the two counters of lx_cull.h's kernels are zero where they did not run)
    uint64_t const sum = tc[lx::kTopFinal] + tc[lx::kTopDuplicate] + tc[lx::kTopAbundant] + tc[lx::kTopMaxHsps] + tc[lx::kTopCulled];
    if (sum != nrec || tc[lx::kTopOps] > max_ops)
        return fail(h, LX_ESTATE, "the cut's kernels account for %llu of %llu records", (unsigned long long)sum, (unsigned long long)nrec);
    stats->qrys_with_hit += tc[lx::kTopQueries], stats->hits_duplicate2 += tc[lx::kTopDuplicate], stats->hits_abundant += tc[lx::kTopAbundant];
    stats->hits_final += tc[lx::kTopFinal], stats->pairs += tc[lx::kTopPairs];
    if (cull_stats)
        cull_stats->hits_max_hsps += tc[lx::kTopMaxHsps], cull_stats->hits_culled += tc[lx::kTopCulled];
    return LX_OK;
}

int RecordsJob::prepare(lambda_amd::CutOffs & cutOffFor, std::vector<Range> rs, uint64_t max_entries, uint64_t max_wlen)
{
    using namespace lambda_amd;
    auto &            l2 = h->l2;
    hipStream_t const st = h->stream;
    int               rc;
    ranges   = std::move(rs);
    want_ops = !(params->flags & LX_ITERATE_NO_OPS);
    int const qFrames = std::max(1, params->qry_num_frames), sFrames = std::max(1, params->sbj_num_frames);
    std::vector<double> & pre = pre_host; // (a member: the upload below is asynchronous, the job outlives it)
    pre.assign(std::max<size_t>(l2.evlens.size(), 1), 0.0);
    for (size_t i = 0; i < l2.evlens.size(); ++i)
    {
        uint64_t const ql  = (uint64_t)l2.evlens[i] / (params->query_translated ? 3 : 1);
        auto           it  = cutOffFor.evalue.cachedLengthAdjustments.find(ql);
        uint64_t const adj = it != cutOffFor.evalue.cachedLengthAdjustments.end() ? it->second : lengthAdjustment(params->db_total_length, ql, params->karlin);
        pre[i]             = params->karlin.K * (double)(ql - adj) * (double)(params->db_total_length - adj);
    }
    if (l2.exp_lambda != params->karlin.lambda || l2.exp_n == 0)
    {
        std::vector<double> tab;
        for (uint32_t sc = 0; sc < (1u << 20); ++sc)
        {
            double const v = std::exp(-params->karlin.lambda * (double)sc);
            tab.push_back(v);
            if (v == 0.0)
                break;
        }
        if ((rc = upload(h, l2.d_exp, tab)))
            return rc;
        LX_HIP(h, hipStreamSynchronize(st)); // (`tab` is a local)
        l2.exp_lambda = params->karlin.lambda;
        l2.exp_n      = (uint32_t)tab.size();
    }
    int32_t bit_cut = INT32_MIN;
    if (params->min_bitscore >= 0)
    {
        auto const fails = [&](int32_t sc) { return computeBitScore(sc, params->karlin) < params->min_bitscore; };
        int64_t    lo = -(1ll << 30), hi = 1ll << 30; // fails(lo), !fails(hi)
        if (!fails((int32_t)lo))
            bit_cut = INT32_MIN;
        else if (fails((int32_t)hi))
            bit_cut = INT32_MAX;
        else
        {
            while (hi - lo > 1)
            {
                int64_t const mid = lo + (hi - lo) / 2;
                (fails((int32_t)mid) ? lo : hi) = mid;
            }
            bit_cut = (int32_t)hi;
        }
    }
    uint64_t max_win = 1;
    for (Range const & r : ranges)
        max_win = std::max(max_win, r.hi - r.lo);
    uint64_t const sort_n = std::max<uint64_t>(max_entries, 1), nr = ranges.size();
    if ((rc = upload(h, l2.d_pre, pre)) || (rc = ensure_records(h, n_part + 16, max_win, max_entries, nr, nr)) ||
        (rc = ensure(h, l2.d_pair[0], sort_n * 8 + 16)) || (rc = ensure(h, l2.d_pair[1], sort_n * 8 + 16)) || (rc = ensure(h, l2.d_s0[0], sort_n * 8 + 16)) ||
        (rc = ensure(h, l2.d_s0[1], sort_n * 8 + 16)) || (rc = ensure(h, l2.d_hist, (lx::l2_sort_tiles(sort_n) + 2) * 256 * sizeof(uint32_t))))
    {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    LX_HIP(h, hipMemsetAsync(l2.d_reccnt.ptr, 0, nr * lx::kRecCounters * sizeof(uint64_t), st));
    if (top && ((rc = ensure_top_records(h, n_part + 16, max_win, nr, &top->cull)) || (rc = ensure(h, l2.d_topcodes, 3 * (n_part + 16) * sizeof(uint64_t) + 16)) ||
                (rc = ensure_pinned(h, l2.p_topcnt, nr * lx::kTopCounters * sizeof(uint64_t), kRoom))))
    {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    base.q_len      = static_cast<uint32_t const *>(l2.d_qlen.ptr);
    base.q_evidx    = static_cast<uint32_t const *>(l2.d_qevidx.ptr);
    base.q_frames   = (uint32_t)qFrames;
    base.s_frames   = (uint32_t)sFrames;
    base.n_qid_end  = (uint32_t)((l2.q_len.size() + (uint64_t)qFrames - 1) / (uint64_t)qFrames);
    base.q_mode     = params->q_frame_mode;
    base.s_mode     = params->s_frame_mode;
    base.bit_cut    = bit_cut;
    base.id_cutoff  = params->id_cutoff;
    base.want_ops   = want_ops ? 1 : 0;
    base.lambda     = params->karlin.lambda;
    base.log_k      = std::log(params->karlin.K);
    base.log_2      = std::log(2.0);
    base.pre_by_len = static_cast<double const *>(l2.d_pre.ptr);
    base.exp_tab    = static_cast<double const *>(l2.d_exp.ptr);
    base.exp_n      = l2.exp_n;
    base.ops_base   = 0; // (the rows carry offsets inside their range; flush() knows where the range's columns begin)
    base.list_at    = static_cast<uint32_t *>(l2.d_listat.ptr);
    // the digits the keys can have set: (true query id | padding's id, query slice length), (subject slice length, window | entry)
    pair_bits = (bits_below((uint64_t)base.n_qid_end + 1) << 32) | bits_below((uint64_t)l2.max_qlen + 1);
    // (a window is as long as its subject at most; the plan knows the part's longest window: one digit instead of three on a genome)
    s0_bits   = (bits_below(std::min<uint64_t>(max_wlen ? max_wlen : l2.max_slen, 0xfffffffeull) + 1) << 32) | bits_below(std::max(max_win, max_entries) + 1);
    return LX_OK;
}

int RecordsJob::enqueue(uint64_t r, void const * d_hsp, void const * d_src, void const * d_count, void const * d_codes_off, uint64_t cap)
{
    auto &            l2 = h->l2;
    hipStream_t const st = h->stream;
    Range const &     rg = ranges[r];
    lx::RecParams     p  = base;
    p.hsp       = static_cast<lx::Hsp const *>(d_hsp);
    p.src       = static_cast<uint32_t const *>(d_src);
    p.codes_off = static_cast<uint64_t const *>(d_codes_off);
    p.count_ptr = static_cast<uint64_t const *>(d_count);
    p.n_entries = cap;
    p.src_base  = (uint32_t)rg.lo;
    p.win       = static_cast<lx::L2Window const *>(l2.d_win.ptr) + part_lo + rg.lo;
    p.score     = static_cast<int32_t const *>(h->d_score_all.ptr) + rg.lo;
    p.min_score = static_cast<int32_t const *>(h->d_min_all.ptr) + part_lo + rg.lo;
    p.n_win     = rg.hi - rg.lo;
    p.counters  = static_cast<uint64_t *>(l2.d_reccnt.ptr) + r * lx::kRecCounters;
    p.rec       = static_cast<lx::BlastMatchDev *>(l2.d_rec.ptr) + rg.lo;
    p.rec_codes = static_cast<uint64_t *>(l2.d_reccodes.ptr) + 3 * rg.lo;
    p.rank      = use_rank ? static_cast<uint32_t const *>(l2.d_rank.ptr) + rg.lo : nullptr;
    p.rank_pad  = (uint32_t)n_part;
    LX_HIP(h, hipMemsetAsync(p.counters, 0, lx::kRecCounters * sizeof(uint64_t), st)); // (a range whose chunk runs again starts over)
    LX_HIP(h, hipMemsetAsync(l2.d_listat.ptr, 0xff, p.n_win * sizeof(uint32_t), st));
    uint64_t * pair = static_cast<uint64_t *>(l2.d_pair[0].ptr), * pair_tmp = static_cast<uint64_t *>(l2.d_pair[1].ptr);
    uint64_t * s0 = static_cast<uint64_t *>(l2.d_s0[0].ptr), * s0_tmp = static_cast<uint64_t *>(l2.d_s0[1].ptr);
    LX_HIP(h, lx::rec_launch(p, &pair, &pair_tmp, &s0, &s0_tmp, use_rank ? 0ull : pair_bits, use_rank ? bits_below(n_part + 1) : s0_bits, static_cast<uint32_t *>(l2.d_hist.ptr),
                             static_cast<uint32_t *>(l2.d_tilekeep.ptr),
                             static_cast<uint64_t *>(l2.d_tileops.ptr), st));
    LX_HIP(h, hipMemcpyAsync(static_cast<uint64_t *>(l2.p_reccnt.ptr) + r * lx::kRecCounters, p.counters, lx::kRecCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (top)
    {
        // the range's records stand in p.rec, counters[kRecKept] of them: sorted, made unique, sorted and cut where they are
        lx::TopParams tp{};
        tp.in          = p.rec;
        tp.out         = static_cast<lx::BlastMatchDev *>(l2.d_toprows.ptr) + rg.lo;
        tp.codes_in    = want_ops ? p.rec_codes : nullptr;
        tp.codes_out   = want_ops ? static_cast<uint64_t *>(l2.d_topcodes.ptr) + 3 * rg.lo : nullptr;
        tp.n_ptr       = p.counters + lx::kRecKept;
        tp.n_cap       = p.n_win;
        tp.max_matches = top->max_matches;
        tp.rebase_ops  = want_ops ? 1 : 0;
        tp.counters    = static_cast<uint64_t *>(l2.d_topcnt.ptr) + r * lx::kTopCounters;
        top->cull.set(tp);
        PhaseTimer pt(h, st, 7);
        LX_HIP(h, lx::toprec_launch(tp, l2.d_topwork.ptr, st));
        pt.close();
        LX_HIP(h, hipMemcpyAsync(static_cast<uint64_t *>(l2.p_topcnt.ptr) + r * lx::kTopCounters, tp.counters, lx::kTopCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    return LX_OK;
}

int RecordsJob::collect(uint64_t r, uint64_t code_base, bool gpu_busy)
{
    ranges[r].done      = true;
    ranges[r].code_base = code_base;
    int rc = LX_OK;
    while (rc == LX_OK && next_flush < ranges.size() && ranges[next_flush].done)
        rc = flush(next_flush++, gpu_busy);
    return rc;
}

int RecordsJob::flush(uint64_t r, bool gpu_busy)
{
    using namespace lambda_amd;
    auto &                 l2  = h->l2;
    Range const &          rg  = ranges[r];
    uint64_t const * const cnt = static_cast<uint64_t const *>(l2.p_reccnt.ptr) + r * lx::kRecCounters;
    if (cnt[lx::kRecErr] & 1)
        return fail(h, LX_EOVERFLOW, "an extension of the list could not be traced");
    if (cnt[lx::kRecErr] & 2)
        return fail(h, LX_ESTATE, "a survivor names a window outside its range of the list");
    uint64_t const ns = cnt[lx::kRecSurvivors], nrec = cnt[lx::kRecKept];
    uint64_t       nkeep = nrec, nops = cnt[lx::kRecOps]; // what comes down
    if (ns > rg.hi - rg.lo || nkeep > ns)
        return fail(h, LX_ESTATE, "the records kernels report %llu records of %llu survivors of %llu windows", (unsigned long long)nkeep, (unsigned long long)ns,
                    (unsigned long long)(rg.hi - rg.lo));
    res->stats.failed_bitscore += cnt[lx::kRecFailedBit];
    res->stats.failed_evalue += cnt[lx::kRecFailedEv];
    if (ns == 0)
        return LX_OK;
    res->stats.num_ext_ali += ns; // :1287
    res->stats.failed_identity += ns - nrec;
    if (top && nrec)
    {
        uint64_t const * const tc = static_cast<uint64_t const *>(l2.p_topcnt.ptr) + r * lx::kTopCounters;
        if (int const rc = top_account(h, tc, nrec, want_ops ? nops : ~0ull, &top->stats, &top->cull.stats))
            return rc;
        nkeep = tc[lx::kTopFinal];
        nops  = want_ops ? tc[lx::kTopOps] : nops;
    }
    uint64_t const rec0 = res->matches.size(), ops0 = res->ops.size();
    if (!res->matches.resize(rec0 + nkeep) || !res->ops.resize(ops0 + nops))
        return fail(h, LX_ENOMEM, "out of host memory for the result records");
    if (nkeep == 0)
        return LX_OK;
    // On the copy stream, beside whatever the handle's stream computes (the next chunk's sweep): the rows' column offsets become
    // the result's, then -- 24 bytes per record -- where the records' codes begin and their columns go: the host threads expand the
    // columns from the run-length codes WHILE the rows themselves come down (1.8 ms of copy beside 2.0 ms of expansion on a million reads)
    hipStream_t const      cs = h->stream3;
    lx::BlastMatchDev *    d_rows = static_cast<lx::BlastMatchDev *>(top ? l2.d_toprows.ptr : l2.d_rec.ptr) + rg.lo;
    std::vector<uint64_t> & codes_at = l2.rec_codes;
    std::thread             expander;
    if (want_ops)
    {
        if (ops0)
            LX_HIP(h, lx::rec_launch_add_ops_base(d_rows, nkeep, ops0, cs));
        codes_at.resize(3 * nkeep);
        LX_HIP(h, hipMemcpyAsync(codes_at.data(), static_cast<uint64_t const *>(top ? l2.d_topcodes.ptr : l2.d_reccodes.ptr) + 3 * rg.lo, 3 * nkeep * sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
        LX_HIP(h, hipStreamSynchronize(cs));
        uint8_t const * const codes = h->ext_bytes.data() + rg.code_base;
        uint8_t * const       ops   = res->ops.data() + ops0;
        expander = std::thread(
            [&codes_at, codes, ops, nkeep]()
            {
                parallelRanges(nkeep,
                               [&](unsigned, uint64_t lo, uint64_t hi)
                               {
                                   for (uint64_t k = lo; k < hi; ++k)
                                   {
                                       if (k + 8 < hi)
                                           __builtin_prefetch(codes + codes_at[3 * (k + 8)]);
                                       (void)lx_expand_ops(codes + codes_at[3 * k], (int32_t)codes_at[3 * k + 2], ops + codes_at[3 * k + 1]);
                                   }
                               });
            });
    }
    // The rows.  While another chunk computes: into pinned memory (a copy engine's transfer, at the link's rate whatever the handle's
    // stream does -- a copy into the result's ordinary memory is staged by the runtime with the compute units the sweep is using:
    // 4.1 instead of 1.1 ms for half a million rows) and from there into the result by the host threads (2.0 ms with the columns,
    // hidden behind the chunk).  With the GPU idle -- the last range -- straight into the result (1.1 ms).
    hipError_t e_rows = hipSuccess;
    int        rc_pin = gpu_busy ? ensure_pinned(h, l2.p_rows, nkeep * sizeof(lx_blast_match) + 16, kRoom, hipHostMallocNonCoherent) : LX_OK;
    if (rc_pin == LX_OK)
    {
        e_rows = hipMemcpyAsync(gpu_busy ? l2.p_rows.ptr : static_cast<void *>(res->matches.data() + rec0), d_rows, nkeep * sizeof(lx_blast_match), hipMemcpyDeviceToHost, cs);
        if (e_rows == hipSuccess)
            e_rows = hipStreamSynchronize(cs);
    }
    if (expander.joinable())
        expander.join();
    if (rc_pin)
        return rc_pin;
    LX_HIP(h, e_rows);
    if (gpu_busy)
    {
        uint8_t const * const from = static_cast<uint8_t const *>(l2.p_rows.ptr);
        uint8_t * const       to   = reinterpret_cast<uint8_t *>(res->matches.data() + rec0);
        uint64_t const        bytes = nkeep * sizeof(lx_blast_match);
        // (pieces of 256 bytes: parallelRanges spreads lists of 32 768 items and more)
        parallelRanges((bytes + 255) / 256, [&](unsigned, uint64_t lo, uint64_t hi) { std::memcpy(to + lo * 256, from + lo * 256, std::min(bytes, hi * 256) - lo * 256); });
    }
    return LX_OK;
}

int lxi::toprec_host_rows(lx_handle * h, lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_record_stats * stats, uint64_t * out_n, CullRequest * cull)
{
    auto &            l2 = h->l2;
    hipStream_t const st = h->stream;
    int               rc;
    lx_record_stats   rs{};
    lx_cull_stats     cs{};
    *out_n = 0;
    if (n)
    {
        if ((rc = ensure(h, l2.d_topin, n * sizeof(lx_blast_match) + 16)) || (rc = ensure_top_records(h, n, n, 1, cull)))
            return rc;
        LX_HIP(h, hipMemcpyAsync(l2.d_topin.ptr, m, n * sizeof(lx_blast_match), hipMemcpyHostToDevice, st));
        lx::TopParams tp{};
        tp.in          = static_cast<lx::BlastMatchDev const *>(l2.d_topin.ptr);
        tp.out         = static_cast<lx::BlastMatchDev *>(l2.d_toprows.ptr);
        tp.n_cap       = n;
        tp.max_matches = max_matches;
        tp.counters    = static_cast<uint64_t *>(l2.d_topcnt.ptr);
        if (cull)
            cull->set(tp);
        PhaseTimer pt(h, st, 7);
        LX_HIP(h, lx::toprec_launch(tp, l2.d_topwork.ptr, st));
        pt.close();
        uint64_t cnt[lx::kTopCounters];
        LX_HIP(h, hipMemcpyAsync(cnt, tp.counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
        LX_HIP(h, hipStreamSynchronize(st));
        if ((rc = top_account(h, cnt, n, ~0ull, &rs, &cs)))
            return rc;
        if (cnt[lx::kTopFinal])
        {
            LX_HIP(h, hipMemcpyAsync(m, tp.out, cnt[lx::kTopFinal] * sizeof(lx_blast_match), hipMemcpyDeviceToHost, st));
            LX_HIP(h, hipStreamSynchronize(st));
        }
        *out_n = cnt[lx::kTopFinal];
    }
    if (stats)
        *stats = rs;
    if (cull)
        cull->stats = cs;
    return LX_OK;
}

extern "C" int lx_postprocess_records_dev(lx_handle * h, lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_record_stats * stats, uint64_t * out_n)
{
    if (!h || !out_n || (!m && n))
        return LX_EINVAL;
    *out_n = 0;
    if (n >= 0x7ffffff0ull)
        return fail(h, LX_EINVAL, "lx_postprocess_records_dev: at most 2^31 - 16 rows per call");
    int rc = bind(h);
    if (rc)
        return rc;
    h->phase_ev.clear();
    return toprec_host_rows(h, m, n, max_matches, stats, out_n);
}

extern "C" int lx_postprocess_records_dev_ex(lx_handle * h, lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_cull_options const * opt,
                                             lx_record_stats * stats, lx_cull_stats * cull_stats, uint64_t * out_n)
{
    if (!h || !out_n || (!m && n))
        return LX_EINVAL;
    *out_n = 0;
    if (n >= 0x7ffffff0ull)
        return fail(h, LX_EINVAL, "lx_postprocess_records_dev_ex: at most 2^31 - 16 rows per call");
    std::string why;
    if (cull_check(m, n, opt, 0xffffffffull, why) != LX_OK)
        return fail(h, LX_EINVAL, "%s", why.c_str());
    int rc = bind(h);
    if (rc)
        return rc;
    h->phase_ev.clear();
    CullRequest cull;
    if (opt)
        cull.max_hsps = opt->max_hsps, cull.culling_limit = opt->culling_limit, cull.translated = opt->q_translated != 0;
    if (cull.culling_limit && n)
    {
        // the lengths of the queries the rows name, as the 32-bit words the kernel reads (cull_check refused longer ones); queries
        // that no row names keep 0
        uint64_t max_qid = 0;
        for (uint64_t i = 0; i < n; ++i)
            max_qid = std::max<uint64_t>(max_qid, m[i].n_qid);
        std::vector<uint32_t> lens(max_qid + 1, 0u);
        for (uint64_t i = 0; i < n; ++i)
            lens[m[i].n_qid] = (uint32_t)opt->q_lens[m[i].n_qid];
        if ((rc = upload(h, h->l2.d_cullqlen, lens)))
        {
            (void)hipStreamSynchronize(h->stream);
            return rc;
        }
        LX_HIP(h, hipStreamSynchronize(h->stream)); // (`lens` is a local)
        cull.d_q_lens = static_cast<uint32_t const *>(h->l2.d_cullqlen.ptr);
        cull.q_lens_n = lens.size();
    }
    rc = toprec_host_rows(h, m, n, max_matches, stats, out_n, &cull);
    if (rc == LX_OK && cull_stats)
        *cull_stats = cull.stats;
    return rc;
}
