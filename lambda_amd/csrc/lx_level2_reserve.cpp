// lx_level2_reserve.cpp -- lx_reserve: what the first lx_iterate_matches_dev call of a handle would otherwise allocate inside the call:
// 21.9 ms against 11.9 ms for the calls behind it on a million reads (tools/dev/cold_iterate.py) -- 8.5 instead of 2.1 ms for the copy
// of the rows into result memory that was never touched, 3 ms of allocations in the pipeline -- and a search makes ONE such call per
// run.  The sizes are those of the call's own ensure()s: the same functions (lx_level2_host.h) and the same range rule
// (lx_level2_plan.h), asked with what lx_reserve is told about the list to come; where it deliberately asks for something else than
// the call, a comment says so.  What falls short grows in the call as before.
#include "lx_level2_host.h"

using namespace lxi;

namespace
{

// what lx_reserve works out about the list to come
struct Forecast
{
    uint64_t n_matches, n_windows, n_hsps, n_columns;
    bool     free_plan = false; // the free packing will plan the list (a protein scheme is set), not the solo packing
    uint64_t nwf_solo = 0;  // a wavefront per 16 windows
    uint64_t nwf = 0;       // the plan's wavefronts: the solo packing's count, the free packing's bound
    // survivor entries: the capacity the pipeline gives the call's survivor list (device_sink in lx_xb_sinks.cpp: the
    // windows + a margin for the padding of every chunk's list).  Rows are reserved by it as well, where the call takes windows + 16
    // (RecordsJob::prepare): the larger figure serves both
    uint64_t entries = 0;
};

// ---- the list work (level2_keys, level2_windows) and the device plan
int reserve_list_work(lx_handle * h, Forecast const & f)
{
    auto & l2 = h->l2;
    int    rc;
    if ((rc = ensure_list_keys(h, f.n_matches)) || (rc = ensure_list_work(h, f.n_matches, (size_t)l2.max_evlen + 1)))
        return rc;
    // (the plan: the solo packing takes a wavefront per 16 windows; the free packing of a protein list is bounded by its own formula and
    // has a workspace -- for the four ranges the size rule gives at most, not the ranges the call will cut: the bound grows with them)
    if ((rc = ensure_plan(h, f.nwf)) || (f.free_plan && (rc = ensure(h, l2.d_fp, lx::fp_workspace_bytes(f.n_windows, l2.q_len.size(), (uint32_t)kL2MaxRangesBySize) + 64))))
        return rc;
    return LX_OK;
}

// ---- the records (RecordsJob)
int reserve_records(lx_handle * h, Forecast const & f)
{
    auto & l2 = h->l2;
    int    rc;
    // (not the call's figures on purpose: rows and survivor entries by `entries`, the list as ONE range of all its windows; one range's
    // counters on the device, those of kFpMaxRanges ranges in pinned memory; three quarters of the expected records in the rows'
    // pinned block; eight wavefronts of room in the plan's)
    if ((rc = ensure(h, l2.d_surv_hsp, f.entries * sizeof(lx_hsp))) || (rc = ensure(h, l2.d_surv_src, f.entries * sizeof(uint32_t))) ||
        (rc = ensure(h, l2.d_surv_codes, f.entries * sizeof(uint64_t))) || (rc = ensure_records(h, f.entries, f.n_windows, f.entries, 1, lx::kFpMaxRanges)) ||
        (rc = ensure_pinned(h, l2.p_rows, (f.n_hsps * 3 / 4) * sizeof(lx_blast_match) + 16, kRoom, hipHostMallocNonCoherent)) ||
        (rc = ensure(h, l2.d_rank, (f.n_windows + 1) * sizeof(uint32_t) + 16)) || (rc = ensure_pinned(h, l2.p_plan, kPlanHead + 2 * (f.nwf + 8) * sizeof(uint32_t), kRoom)) ||
        (rc = ensure(h, l2.d_pre, std::max<size_t>(l2.evlens.size(), 1) * sizeof(double) + 16)) || (rc = ensure(h, l2.d_exp, (1u << 13) * sizeof(double))))
        return rc;
    if (f.n_columns)
    {
        l2.rec_codes.resize(3 * f.n_hsps); // (touched: value-initialised)
        if (!h->ext_bytes.grow(f.n_hsps * 8 + 4096))
            return fail(h, LX_ENOMEM, "lx_reserve: out of host memory");
        std::memset(h->ext_bytes.data(), 0, f.n_hsps * 8 + 4096);
    }
    return LX_OK;
}

// ---- the extension pipeline's two lanes (lx_xb_wf.cpp: WfDriver::enqueue), for chunks of the default size; the survivors' column slots for
// windows of up to three times the ordinary length (what a merged window comes to, src/search_algo.hpp:1153-1157); then the checkpoint
// slots of one chunk and the survivor selection's lists
int reserve_pipeline(lx_handle * h, Forecast const & f, HostMarks & hm)
{
    auto &         l2     = h->l2;
    int            rc;
    uint64_t const chunk  = h->opt_extend_chunk ? std::max<uint64_t>(h->opt_extend_chunk, 1024) : lxi::kExtendChunk;
    uint64_t const nwf_x  = f.free_plan ? f.nwf_solo + f.nwf_solo / 8 + 64 : f.nwf_solo; // (what a free-packing plan comes to, not its bound)
    uint64_t const panel  = (uint64_t)lx::kGeo8x19.panel();
    uint64_t const max_q  = std::max<uint64_t>(1, ((uint64_t)l2.max_qlen + panel - 1) / panel) * panel;
    // (the longest ORDINARY window, query + band on either side, :919-938: a list whose merged windows are longer grows its first chunk's
    // slots in the call)
    uint64_t const max_s  = (uint64_t)l2.max_qlen + 2 * (uint64_t)bandSize(l2.max_qlen) + 16, stride = (max_q + 3 * max_s + 3) & ~3ull;
    uint64_t const steps  = (max_s + 8 - 1 + 15) & ~15ull;
    uint64_t const slot_b = max_q / panel * (lx::ckpt16_slot_dwords(lx::kGeo8x19, (uint32_t)steps) + lx::ckpt_slot_dwords(lx::kGeo8x19, (uint32_t)steps) / 8) * 4;
    // (a device plan's chunks are the RANGES of the list, admitted up to four default chunks: the lanes and the checkpoint slots are
    // sized for the largest range, or the first call grows them.  The count is the call's own rule, l2_range_count -- asked generously:
    // every slot of the plan at an ordinary window's full size where the call halves the longest window's, against fresh memory alone,
    // and without LX_L2_RANGES, which steers measurements of a call.  The largest range likewise: of two, the first one's share and
    // kL2ReserveSlackPercent; of more, an eighth on top of an even share; 64 wavefronts for the cut's distance from its target)
    uint64_t const R_est  = l2_range_count(f.n_windows, true, 0, nwf_x * 16 * slot_b, kL2FreshSlotBytes);
    uint64_t const range  = (R_est == 1 ? nwf_x : R_est == 2 ? nwf_x * (kL2FirstOfTwoPercent + kL2ReserveSlackPercent) / 100 + 64 : nwf_x / R_est + nwf_x / (8 * R_est) + 64) * 16;
    uint64_t const chunk16 = (chunk + 15) / 16 * 16;
    uint64_t const slots  = std::min<uint64_t>(nwf_x * 16, std::max(chunk16, std::min(range, 4 * chunk16))), cap_sel = (slots + 7) / 8 * 8 + 8;
    if ((rc = ensure(h, h->d_score_all, f.n_windows * sizeof(int32_t) + 16)))
        return rc;
    unsigned const lanes = nwf_x * 16 > slots ? 2 : 1;
    for (unsigned L = 0; L < lanes; ++L)
    {
        lx_handle::XbLane & ln = h->xb[L];
        if ((rc = ensure(h, ln.d_ext, slots * sizeof(lx_extension))) || (rc = ensure(h, ln.d_min, slots * sizeof(int32_t))) ||
            (rc = ensure(h, ln.d_score, slots * sizeof(int32_t))) || (rc = ensure(h, ln.d_hsp, cap_sel * sizeof(lx_hsp))) ||
            (rc = ensure(h, ln.d_ops, cap_sel * stride + 16)) || (rc = ensure(h, ln.d_rle, cap_sel * stride + 16)) ||
            (rc = ensure(h, ln.d_src, cap_sel * sizeof(uint32_t))) || (rc = ensure(h, ln.d_len, cap_sel * sizeof(uint32_t))) ||
            (rc = ensure(h, ln.d_cnt, 5 * sizeof(uint64_t))) || (rc = ensure_pinned(h, ln.p_cnt, 5 * sizeof(uint64_t), kRoom)))
            return rc;
    }
    hm.mark("lanes");
    // the checkpoint slots of one chunk (what LX_OPT_TRACE_BYTES admits of them), its end cells, the survivor selection's lists
    // (select_stage in lx_step.cpp: room for every slot plus the padding of query runs), the carry workspace
    uint64_t const trace = std::min<uint64_t>(slots * slot_b, h->opt_trace_bytes);
    if ((rc = ensure(h, h->d_trace, trace)) || (rc = ensure(h, h->d_ends, slots * sizeof(lx::EndCell))) || (rc = ensure(h, h->d_sel_ext, 2 * slots * sizeof(lx_extension))) ||
        (rc = ensure(h, h->d_sel_src, 2 * slots * sizeof(uint32_t))) || (rc = ensure(h, h->d_sel_score, 2 * slots * sizeof(int32_t))) ||
        (rc = ensure(h, h->d_sel_runs, (2 * slots + 4096) * sizeof(uint64_t))) || (rc = ensure(h, h->d_ws, std::max(h->opt_ws_bytes, h->ws_grown))))
        return rc;
    return LX_OK;
}

// ---- every kernel of the call once, on a list of one match (query 0 against the start of subject 0, no filter: it survives and is
// traced): what a kernel's first launch costs the runtime (2-3 ms over the call's two dozen kernels) is paid here
int reserve_first_launches(lx_handle * h, uint64_t n_columns)
{
    auto & l2 = h->l2;
    int    rc;
    if (l2.q_len.empty() || l2.s_len.empty() || !h->db_bytes || l2.s_extent > h->db_bytes || !(h->have_sc[0] || h->have_sc[1]) || h->opt_band || l2.s_len[0] == 0)
        return LX_OK;
    lx_match const one{0, 0, 0, std::min<uint64_t>(l2.q_len[0], l2.s_len[0]), 0, std::min<uint64_t>(l2.q_len[0], l2.s_len[0])};
    if ((rc = ensure(h, l2.d_up, sizeof(lx_match) + 16)))
        return rc;
    LX_HIP(h, hipMemcpyAsync(l2.d_up.ptr, &one, sizeof(one), hipMemcpyHostToDevice, h->stream));
    LX_HIP(h, hipStreamSynchronize(h->stream));
    lx_search_params sp{};
    sp.max_evalue      = -1;
    sp.min_bitscore    = -1;
    sp.db_total_length = 1000000;
    sp.qry_num_frames  = l2.q_frames;
    sp.sbj_num_frames  = 1;
    sp.karlin          = lx_karlin{0.3, 0.1, 0.3, 1.0, -10.0};
    sp.flags           = n_columns ? 0 : LX_ITERATE_NO_OPS;
    lx_iterate_result * r = nullptr;
    // (the dummy call must not teach the handle anything: what the adaptive pass 2 and the wide sweep learnt from real lists stays)
    double const   surv_before = h->surv_frac, decl_before = h->mq_decl_frac;
    bool const     pending_before = h->count_pending;
    uint64_t const res_before     = h->res_count;
    rc = lx_iterate_matches_dev(h, h->have_sc[0] ? 0 : 1, l2.d_up.ptr, 1, &sp, &r);
    h->surv_frac     = surv_before;
    h->mq_decl_frac  = decl_before;
    h->count_pending = pending_before;
    h->res_count     = res_before;
    h->phase_ev.clear();
    h->ev_pool_used   = 0;
    if (r)
        lx_iterate_result_free(r);
    if (rc)
        return rc;
    l2.exp_lambda = 0; // (the table of exp(-lambda s) the dummy call left is not the search's)
    return LX_OK;
}

// ---- the result's memory: blocks of the sizes the first result will ask for, written once (a page the kernel has not handed out
// yet costs a fault when the rows' copy or the expanding threads reach it), kept where a result's arrays are taken from
int reserve_result_blocks(lx_handle * h, Forecast const & f)
{
    for (uint64_t bytes : {f.n_hsps * (uint64_t)sizeof(lx_blast_match), f.n_columns})
    {
        if (bytes < lambda_amd::BlockCache::kMinBytes)
            continue;
        lambda_amd::RawVec<uint8_t> block;
        if (!block.resize(bytes))
            return fail(h, LX_ENOMEM, "lx_reserve: out of host memory for the result blocks");
        uint8_t * const b = block.data();
        lambda_amd::parallelRanges(bytes / 4096, [&](unsigned, uint64_t lo, uint64_t hi) { std::memset(b + lo * 4096, 0, (hi - lo) * 4096); });
    } // (the destructor hands the block to the cache)
    return LX_OK;
}

} // namespace

extern "C" int lx_reserve(lx_handle * h, uint64_t n_matches, uint64_t n_windows, uint64_t n_hsps, uint64_t n_columns)
{
    if (!h)
        return LX_EINVAL;
    if (n_matches > 0x7ffffff0ull || n_windows > n_matches || n_hsps > n_windows)
        return fail(h, LX_EINVAL, "lx_reserve: n_hsps <= n_windows <= n_matches <= 2^31");
    int rc = bind(h);
    if (rc || n_matches == 0)
        return rc;
    auto &    l2       = h->l2;
    int const slot_set = h->have_sc[0] ? 0 : h->have_sc[1] ? 1 : -1;
    Forecast  f{n_matches, n_windows, n_hsps, n_columns};
    f.free_plan = slot_set >= 0 && !solo_plan_applies(h, slot_set) && free_plan_applies(h, slot_set) && n_windows > 0;
    f.nwf_solo  = (n_windows + 15) / 16;
    f.nwf       = f.free_plan ? lx::fp_wavefront_bound(n_windows, l2.q_len.size(), (uint32_t)kL2MaxRangesBySize) : f.nwf_solo;
    f.entries   = n_windows + n_windows / 64 + 8192;
    HostMarks hm("lx_reserve");
    if ((rc = reserve_list_work(h, f)))
        return rc;
    hm.mark("list work");
    if ((rc = reserve_records(h, f)))
        return rc;
    hm.mark("records");
    if ((rc = reserve_pipeline(h, f, hm)))
        return rc;
    hm.mark("checkpoint slots + selection");
    if ((rc = reserve_first_launches(h, n_columns)))
        return rc;
    hm.mark("one-match call");
    if ((rc = reserve_result_blocks(h, f)))
        return rc;
    hm.mark("result blocks");
    return LX_OK;
}
