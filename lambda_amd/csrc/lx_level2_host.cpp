// lx_level2_host.cpp -- the Level-2 driver on a DEVICE match list: lx_set_queries, lx_set_subject_seqs, lx_iterate_matches_dev.
//
// iterateMatchesFullSimd (/root/reference/src/search_algo.hpp:1177-1332) for matches that the seeding stage left in HBM: widen,
// sort, merge and unique (:1136-1175), the slices (:1200-1227) and the filter's cut-offs (:1251-1283) run as kernels
// (lx_level2.hip) on the resident sequence sets; the host receives the finished window list (24 B per WINDOW, a tenth of the
// matches), plans the sweep over it, and the extension pipeline (lx_host.cpp) reads list and cut-offs where the kernels wrote
// them.  What follows the two passes -- statistics, order, records (:1287-1325) -- is host/lx_iterate_common.hpp, shared with
// lx_iterate_matches.  lx_iterate_matches itself hands its lists to this path when they are large (host/lx_driver.cpp).
// The range plan of a call -- how many ranges, where they are cut, which strip geometry -- is lx_level2_plan.h (no HIP in it); the
// records made on the device are RecordsJob, lx_level2_records.cpp.
#include "lx_level2_host.h"

using namespace lxi;
using namespace lambda_amd;

// ---- buffer sizes that the calls and lx_reserve share (lx_level2_host.h)
int lxi::ensure_list_keys(lx_handle * h, uint64_t n)
{
    auto & l2 = h->l2;
    int    rc;
    if ((rc = ensure(h, l2.d_pair[0], n * 8 + 16)) || (rc = ensure(h, l2.d_s0[0], n * 8 + 16)) || (rc = ensure(h, l2.d_cnt, 16 * sizeof(uint64_t))))
        return rc;
    return LX_OK;
}

int lxi::ensure_list_work(lx_handle * h, uint64_t n, size_t cut_entries)
{
    auto &         l2    = h->l2;
    uint64_t const tiles = lx::l2_sort_tiles(n), stiles = lx::l2_scan_tiles(n);
    int            rc;
    if ((rc = ensure(h, l2.d_cut, cut_entries * sizeof(int32_t) + 16)) || (rc = ensure(h, l2.d_pair[1], n * 8 + 16)) || (rc = ensure(h, l2.d_s0[1], n * 8 + 16)) ||
        (rc = ensure(h, l2.d_hist, (tiles + 2) * 256 * sizeof(uint32_t))) || (rc = ensure(h, l2.d_head, n * 16 + 16)) ||
        (rc = ensure(h, l2.d_tot, (stiles + 2) * sizeof(uint32_t))) || (rc = ensure(h, l2.d_win, n * sizeof(lx::L2Window) + 16)) ||
        (rc = ensure(h, h->d_ext_all, n * sizeof(lx_extension) + 16)) || (rc = ensure(h, h->d_min_all, n * sizeof(int32_t) + 16)) ||
        (rc = ensure_pinned(h, l2.p_cnt, 16 * sizeof(uint64_t), kRoom)))
        return rc;
    return LX_OK;
}

int lxi::ensure_plan(lx_handle * h, uint64_t cap_wf)
{
    auto & l2 = h->l2;
    int    rc;
    if ((rc = ensure(h, l2.d_plan, cap_wf * 16 * sizeof(uint32_t) + 16)) || (rc = ensure(h, l2.d_wf, 2 * cap_wf * sizeof(uint32_t) + 64)))
        return rc;
    return LX_OK;
}

extern "C" {

int lx_set_queries(lx_handle * h, uint8_t const * q_res, uint64_t q_bytes, uint64_t const * q_seq_off, uint64_t const * q_seq_len, uint64_t n_qseq,
                   uint64_t const * q_orig_len, int32_t qry_num_frames)
{
    if (!h)
        return LX_EINVAL;
    if ((!q_res && q_bytes) || ((!q_seq_off || !q_seq_len) && n_qseq))
        return fail(h, LX_EINVAL, "NULL argument");
    if (n_qseq >= (1ull << 31))
        return fail(h, LX_EINVAL, "at most 2^31 (frame) query sequences");
    int rc = bind(h);
    if (rc)
        return rc;
    auto & l2   = h->l2;
    int const f = std::max(1, qry_num_frames);
    // Validated into locals, committed to the handle only after the uploads succeeded: a failing call leaves NOTHING resident
    // (q_bytes 0, empty tables -- what the device entry points test), never host tables of the new set over device arrays of the old.
    auto drop = [&]()
    {
        l2.q_bytes = 0;
        l2.q_hash  = 0;
        l2.q_off.clear();
        l2.q_len.clear();
        l2.q_evlen.clear();
        l2.evlens.clear();
        l2.max_evlen = 0;
    };
    drop();
    std::vector<uint64_t> q_off(q_seq_off, q_seq_off + n_qseq);
    std::vector<uint32_t> q_len(n_qseq), q_evlen(n_qseq), band(n_qseq);
    for (uint64_t i = 0; i < n_qseq; ++i)
    {
        if (q_seq_len[i] > 0xffffffffull || !lx_slice_ok(q_seq_off[i], q_seq_len[i], q_bytes))
            return fail(h, LX_EINVAL, "query sequence %llu exceeds the residue buffer", (unsigned long long)i);
        uint64_t const ev = q_orig_len ? q_orig_len[i / (uint64_t)f] : q_seq_len[i];
        if (ev > (1ull << 26))
            return fail(h, LX_EINVAL, "query %llu: a length of %llu is beyond the cut-off table", (unsigned long long)i, (unsigned long long)ev);
        q_len[i]   = (uint32_t)q_seq_len[i];
        q_evlen[i] = (uint32_t)ev;
        band[i]    = (uint32_t)bandSize(q_seq_len[i]);
    }
    std::vector<uint32_t> evlens = q_evlen;
    std::sort(evlens.begin(), evlens.end());
    evlens.erase(std::unique(evlens.begin(), evlens.end()), evlens.end());
    // (for the records kernel, lx_records.hip: which of the distinct e-value lengths a query has; the longest query bounds a sort digit)
    std::vector<uint32_t> evidx(n_qseq);
    uint32_t              max_qlen = 0;
    for (uint64_t i = 0; i < n_qseq; ++i)
    {
        evidx[i] = (uint32_t)(std::lower_bound(evlens.begin(), evlens.end(), q_evlen[i]) - evlens.begin());
        max_qlen = std::max(max_qlen, q_len[i]);
    }
    if ((rc = ensure(h, l2.d_qres, q_bytes + kSlack)))
        return rc;
    if (q_bytes)
        LX_HIP(h, hipMemcpyAsync(l2.d_qres.ptr, q_res, q_bytes, hipMemcpyHostToDevice, h->stream));
    LX_HIP(h, hipMemsetAsync(static_cast<uint8_t *>(l2.d_qres.ptr) + q_bytes, 0, kSlack, h->stream));
    if ((rc = upload(h, l2.d_qoff, q_off)) || (rc = upload(h, l2.d_qlen, q_len)) || (rc = upload(h, l2.d_qband, band)) ||
        (rc = upload(h, l2.d_qevlen, q_evlen)) || (rc = upload(h, l2.d_qevidx, evidx)))
    {
        (void)hipStreamSynchronize(h->stream); // (the uploads queued so far read this function's locals)
        return rc;
    }
    LX_HIP(h, hipStreamSynchronize(h->stream)); // (the uploads read the caller's arrays and this function's locals)
    l2.max_evlen = evlens.empty() ? 0 : evlens.back();
    l2.evlens.swap(evlens);
    l2.q_off.swap(q_off);
    l2.q_len.swap(q_len);
    l2.q_evlen.swap(q_evlen);
    l2.q_frames = f;
    l2.max_qlen = max_qlen;
    l2.q_bytes  = q_bytes;
    return LX_OK;
}

int lx_set_subject_seqs(lx_handle * h, uint64_t const * s_seq_off, uint64_t const * s_seq_len, uint64_t n_sseq)
{
    if (!h)
        return LX_EINVAL;
    if ((!s_seq_off || !s_seq_len) && n_sseq)
        return fail(h, LX_EINVAL, "NULL argument");
    if (n_sseq >= (1ull << 32))
        return fail(h, LX_EINVAL, "at most 2^32 (frame) subject sequences");
    int rc = bind(h);
    if (rc)
        return rc;
    auto & l2 = h->l2;
    // (as lx_set_queries: nothing of the old set stays visible while the new one is validated and uploaded)
    l2.s_hash = 0;
    l2.s_off.clear();
    l2.s_len.clear();
    l2.max_slen = l2.s_extent = 0;
    std::vector<uint64_t> s_off(s_seq_off, s_seq_off + n_sseq), s_len(s_seq_len, s_seq_len + n_sseq);
    uint64_t              max_slen = 0, s_extent = 0;
    for (uint64_t i = 0; i < n_sseq; ++i)
    {
        if (s_seq_off[i] + s_seq_len[i] < s_seq_off[i])
            return fail(h, LX_EINVAL, "subject sequence %llu: offset + length overflows", (unsigned long long)i);
        max_slen = std::max(max_slen, s_seq_len[i]);
        s_extent = std::max(s_extent, s_seq_off[i] + s_seq_len[i]);
    }
    if ((rc = upload(h, l2.d_soff, s_off)) || (rc = upload(h, l2.d_slen, s_len)))
    {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    LX_HIP(h, hipStreamSynchronize(h->stream));
    l2.s_off.swap(s_off);
    l2.s_len.swap(s_len);
    l2.max_slen = max_slen;
    l2.s_extent = s_extent;
    return LX_OK;
}

} // extern "C"

// Sort, merge, unique and the slices for matches that stand on the device as sort words already (`pair` / `s0` of lx_level2.h in
// l2.d_pair[0] / l2.d_s0[0]; l2.d_cnt[2] = the key kernel's error flag): the windows end up in l2.d_win, their slices and
// cut-offs in h->d_ext_all / h->d_min_all.  nw = windows, nEven = those of even subject frames (bisulfite: they come first).
static int level2_windows(lx_handle * h, uint64_t n_matches, bool bisulfite, std::vector<int32_t> const & cut_table, uint64_t & nw, uint64_t & nEven)
{
    auto &            l2 = h->l2;
    hipStream_t const st = h->stream;
    if (int const rc = ensure_list_work(h, n_matches, cut_table.size()))
        return rc;
    LX_HIP(h, hipMemcpyAsync(l2.d_cut.ptr, cut_table.data(), cut_table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    uint64_t * pair = static_cast<uint64_t *>(l2.d_pair[0].ptr), * pair_tmp = static_cast<uint64_t *>(l2.d_pair[1].ptr);
    uint64_t * s0 = static_cast<uint64_t *>(l2.d_s0[0].ptr), * s0_tmp = static_cast<uint64_t *>(l2.d_s0[1].ptr);
    uint64_t const pair_bits = (bisulfite ? 1ull << 63 : 0ull) | (bits_below(l2.q_len.size()) << 32) | bits_below(l2.s_len.size());
    uint64_t const s0_bits   = bits_below(l2.max_slen);
    LX_HIP(h, lx::l2_launch_sort(&pair, &pair_tmp, &s0, &s0_tmp, n_matches, pair_bits, s0_bits, static_cast<uint32_t *>(l2.d_hist.ptr), st));
    lx::L2Params p{};
    p.sets       = lx::L2Sets{static_cast<uint64_t const *>(l2.d_qoff.ptr),   static_cast<uint32_t const *>(l2.d_qlen.ptr),
                        static_cast<uint32_t const *>(l2.d_qband.ptr),  static_cast<uint32_t const *>(l2.d_qevlen.ptr),
                        static_cast<uint64_t const *>(l2.d_soff.ptr),   static_cast<uint64_t const *>(l2.d_slen.ptr),
                        (uint64_t)l2.q_len.size(),                      (uint64_t)l2.s_len.size()};
    p.n          = n_matches;
    p.ext_out    = static_cast<lx::Extension *>(h->d_ext_all.ptr);
    p.min_out    = static_cast<int32_t *>(h->d_min_all.ptr);
    p.win_out    = static_cast<lx::L2Window *>(l2.d_win.ptr);
    p.cut_by_len = static_cast<int32_t const *>(l2.d_cut.ptr);
    p.count_out  = static_cast<uint64_t *>(l2.d_cnt.ptr);
    p.bisulfite  = bisulfite ? 1 : 0;
    // (the span after merge right goes where the sort's spare buffers are, the span after swallow left into d_head)
    LX_HIP(h, lx::l2_launch_merge(pair, s0, p, pair_tmp, s0_tmp, static_cast<uint64_t *>(l2.d_head.ptr), static_cast<uint64_t *>(l2.d_head.ptr) + n_matches,
                                  static_cast<uint32_t *>(l2.d_tot.ptr), st));
    // what the plan of the sweep will want to know about the list (the strip geometry that sweeps it cheapest, its cells), behind
    // the same synchronisation
    LX_HIP(h, lx::l2_launch_plan_cost(p.ext_out, p.count_out, n_matches, 0,
                                      reinterpret_cast<unsigned long long *>(p.count_out + 3), st));
    LX_HIP(h, hipMemcpyAsync(l2.p_cnt.ptr, l2.d_cnt.ptr, 13 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    LX_HIP(h, hipStreamSynchronize(st)); // (also: `cut_table` is the caller's)
    uint64_t const * const cnt = static_cast<uint64_t const *>(l2.p_cnt.ptr);
    uint64_t const         flag = cnt[2];
    nw    = cnt[0];
    nEven = cnt[1];
    if (flag & 1)
        return fail(h, LX_EINVAL, "a match names a query or subject sequence outside the resident sets");
    if (flag & 2)
        return fail(h, LX_EINVAL, "a match lies beyond the end of its subject sequence");
    if (flag & 4)
        return fail(h, LX_EINVAL, "a merged window is longer than 2^32 residues");
    if (nw > n_matches || nEven > nw)
        return fail(h, LX_ESTATE, "the merge kernels report %llu windows of %llu matches", (unsigned long long)nw, (unsigned long long)n_matches);
    return LX_OK;
}

// matches in device memory -> sort words
static int level2_keys(lx_handle * h, void const * d_matches, uint64_t n_matches, bool bisulfite)
{
    auto & l2 = h->l2;
    if (int const rc = ensure_list_keys(h, n_matches))
        return rc;
    lx::L2Params p{};
    p.sets.n_qseq = l2.q_len.size();
    p.sets.n_sseq = l2.s_len.size();
    p.sets.s_len  = static_cast<uint64_t const *>(l2.d_slen.ptr);
    p.n           = n_matches;
    p.bisulfite   = bisulfite ? 1 : 0;
    uint64_t * const cnt = static_cast<uint64_t *>(l2.d_cnt.ptr);
    LX_HIP(h, hipMemsetAsync(cnt, 0, 4 * sizeof(uint64_t), h->stream));
    LX_HIP(h, lx::l2_launch_keys(d_matches, p, static_cast<uint64_t *>(l2.d_pair[0].ptr), static_cast<uint64_t *>(l2.d_s0[0].ptr), cnt + 2, h->stream));
    return LX_OK;
}

static_assert(sizeof(lx::BlastMatchDev) == sizeof(lx_blast_match) && offsetof(lx::BlastMatchDev, bit_score) == offsetof(lx_blast_match, bit_score) &&
                  offsetof(lx::BlastMatchDev, ops_off) == offsetof(lx_blast_match, ops_off) && offsetof(lx::BlastMatchDev, q_frame) == offsetof(lx_blast_match, q_frame) &&
                  offsetof(lx::BlastMatchDev, identity) == offsetof(lx_blast_match, identity) && offsetof(lx::BlastMatchDev, s_end) == offsetof(lx_blast_match, s_end),
              "the device writes lx_blast_match rows");

// The free-packing plan (lx_plan_free.hip) of a window list in ranges (bounds: {0, cut, ..., n}) queued on the handle's stream: ONE plan
// over the list, laid out range by range, its workspace and the plan's buffers sized by the plan's own bounds.  fa: what was launched.
static int launch_free_plan(lx_handle * h, void const * d_ext, uint64_t n_qseq, int strip_cols, std::vector<uint64_t> const & bounds, lx::FpArgs & fa)
{
    auto & l2 = h->l2;
    int    rc;
    fa            = lx::FpArgs{};
    fa.ext        = static_cast<lx::Extension const *>(d_ext);
    fa.n          = bounds.back();
    fa.n_qseq     = n_qseq;
    fa.C          = strip_cols;
    fa.no_narrow  = 0;
    fa.nranges    = (uint32_t)(bounds.size() - 1);
    std::copy(bounds.begin(), bounds.end(), fa.cut);
    fa.work_bytes = lx::fp_workspace_bytes(fa.n, n_qseq, fa.nranges);
    fa.cap_wf     = lx::fp_wavefront_bound(fa.n, n_qseq, fa.nranges);
    if ((rc = ensure(h, l2.d_fp, fa.work_bytes + 64)) || (rc = ensure_plan(h, fa.cap_wf)))
        return rc;
    fa.work    = l2.d_fp.ptr;
    fa.plan    = static_cast<uint32_t *>(l2.d_plan.ptr);
    fa.wf_pan  = static_cast<uint32_t *>(l2.d_wf.ptr);
    fa.wf_maxs = fa.wf_pan + fa.cap_wf;
    fa.report  = fa.wf_pan + 2 * fa.cap_wf; // (16 words behind the per-wavefront arrays)
    LX_HIP(h, lx::fp_launch_plan(fa, h->stream));
    return LX_OK;
}

// A plan whose report carries a flag (report[1], FpLayout::overflow of lx_plan_free.hip) is no plan: what the flag says, as LX_ESTATE.
static int free_plan_flag(lx_handle * h, uint64_t n, uint64_t n_qseq, uint64_t nwf, uint64_t cap_wf, uint32_t flag)
{
    if (flag == 3)
        return fail(h, LX_ESTATE, "the free-packing plan of %llu windows: the list has more runs than the run bound %llu (fp_run_bound of %llu query sequences): "
                                  "it is not grouped by query, or it holds more queries than stated",
                    (unsigned long long)n, (unsigned long long)lx::fp_run_bound(n, n_qseq), (unsigned long long)n_qseq);
    return fail(h, LX_ESTATE, "the free-packing plan of %llu windows reports %llu wavefronts (at most %llu), flag %u", (unsigned long long)n, (unsigned long long)nwf,
                (unsigned long long)cap_wf, flag);
}

namespace
{

// One strand direction of a call's window list -- windows [lo, lo + n) -- on its way through the stages of Level2Tail: what one stage
// finds out for the next.  Per-call state: nothing of it outlives serve_part.
struct Part
{
    int                   pi = 0; // which of the list's two parts (the cost words are per part)
    uint64_t              lo = 0, n = 0;
    int                   slot = 0;
    bool                  solo = false;          // the solo packing, else the free packing
    lx::Geo               geo  = lx::kGeo8x19;   // the strip geometry
    std::vector<uint64_t> bounds;                // the ranges in the part: {0, cut, ..., n}
    std::vector<uint64_t> cut_wf;                // the ranges' first wavefronts, and where the last one ends
    uint64_t              nwf = 0, cap_wf = 0;   // (cap_wf: what the per-wavefront arrays are spaced by on the device)
    bool                  try_rank      = false; // the rank kernel runs beside the plan
    uint32_t              rank_overflow = 0;     // (lx_records.hip: rec_launch_rank's flag, downloaded with the plan)
    ResidentInput         ri;
    lx_survivor_list      list{};                // the pipeline's survivors where they came to the host ...
    ResidentSurvivors     surv;                  // ... and where they stand

    size_t ranges() const { return bounds.size() - 1; }
};

// The list work and the extension for matches that stand on the device as sort words already, stage by stage.  Appends to *res.
struct Level2Tail
{
    lx_handle * const              h;
    int const                      slot;
    uint64_t const                 n_matches;
    lx_search_params const * const params;
    lx_iterate_result * const      res;
    bool const                     windows_to_host;
    // a bisulfite list's two strand directions are extended apart and a query has records in both: its cut needs the finished result
    TopRequest * const             top;
    lx_handle::Level2 &            l2;
    hipStream_t const              st;
    HostMarks                      hm;
    HostPool::Call const           in_flight_call;
    lambda_amd::CutOffs            cutOffFor;
    std::vector<int32_t>           table; // the cut-off of every query length of the resident set
    uint64_t                       nw = 0, nEven = 0;
    // The window list comes down (24 B per window) on the copy stream, beside what follows, where the host needs it: for the plan of
    // the sweep where that is made on the host, for the records where they are (LX_OPT_ITERATE_RECORDS = 1), for a caller's span
    // (lx_iterate_matches).  Records made on the device over a device plan need none of it.
    bool const                     records_on_device;
    bool                           win_queued = false, win_here = false;
    lx::L2Window const *           win  = nullptr; // (l2.p_win, once wait_windows has seen the list arrive)
    uint64_t const *               cost = nullptr; // [part][19, 13, 11 columns, cells], [8 + part] the part's longest window

    Level2Tail(lx_handle * h_, int slot_, uint64_t n_matches_, lx_search_params const * params_, lx_iterate_result * res_, bool windows_to_host_, TopRequest * top_req)
        : h(h_), slot(slot_), n_matches(n_matches_), params(params_), res(res_), windows_to_host(windows_to_host_), top(top_req && !params_->bisulfite ? top_req : nullptr),
          l2(h_->l2), st(h_->stream), hm("lx_iterate_matches_dev"), cutOffFor(params_), records_on_device(h_->opt_iterate_records == 0)
    {
    }

    int run(uint64_t * n_windows)
    {
        int rc;
        if ((rc = windows()))
            return rc;
        if (n_windows)
            *n_windows = nw;
        if (nw == 0)
            return LX_OK;
        if (!l2.ev_win)
            LX_HIP(h, hipEventCreateWithFlags(l2.ev_win.out(), hipEventDisableTiming));
        l2.score.resize(nw); // (written only where the pipeline hands the survivors to the host: lists it serves without the multi-query plan)
        cost = static_cast<uint64_t const *>(l2.p_cnt.ptr) + 3;
        // one strand direction per call of the pipeline: bisulfite lists are sorted by subjId % 2 first (:1369-1372), the even
        // subject frames take the forward scheme (slot 0), the odd ones the reverse scheme (slot 1)
        uint64_t const split = params->bisulfite ? nEven : nw;
        if ((rc = serve_part(0, 0, split, params->bisulfite ? 0 : slot)) || (rc = serve_part(1, split, nw, 1)))
            return rc;
        if (params->bisulfite) // the HSPs are stably re-sorted by query (:1379); the ops offsets stay valid: only the records move
            std::stable_sort(res->matches.begin(), res->matches.end(), [](lx_blast_match const & a, lx_blast_match const & b) { return a.n_qid < b.n_qid; });
        if (windows_to_host)
        {
            if ((rc = queue_windows()))
                return rc;
            LX_HIP(h, hipEventSynchronize(l2.ev_win));
        }
        return LX_OK;
    }

private:
    // ---- the cut-off table and the window list
    int windows()
    {
        res->stats.num_ext_score += n_matches; // lH.stats.numExtScore (:1187)
        // the cut-off of every query length of the resident set (one bisection each, :1251-1283 as an integer test)
        table.assign((size_t)l2.max_evlen + 1, 0x7fffffff);
        for (uint32_t len : l2.evlens)
            table[len] = cutOffFor(len);
        if (int const rc = level2_windows(h, n_matches, params->bisulfite != 0, table, nw, nEven))
            return rc;
        res->stats.hits_duplicate += n_matches - nw;
        hm.mark("sort+merge");
        return LX_OK;
    }

    // ---- the window list's download, queued once
    // (queued behind what `st` holds at that moment: where the plan is made on the device, behind the plan's kernels -- beside them
    // the copy's writes over PCIe held the first of them up for the whole 0.5 ms it takes -- and so beside the sweep)
    int queue_windows()
    {
        if (win_queued)
            return LX_OK;
        win_queued = true;
        int rcw;
        if ((rcw = ensure_pinned(h, l2.p_win, nw * sizeof(lx::L2Window) + 16, kRoom)))
            return rcw;
        LX_HIP(h, hipEventRecord(l2.ev_win, st));
        LX_HIP(h, hipStreamWaitEvent(h->stream2, l2.ev_win, 0));
        LX_HIP(h, hipMemcpyAsync(l2.p_win.ptr, l2.d_win.ptr, nw * sizeof(lx::L2Window), hipMemcpyDeviceToHost, h->stream2));
        LX_HIP(h, hipEventRecord(l2.ev_win, h->stream2));
        return LX_OK;
    }

    int wait_windows()
    {
        LX_HIP(h, hipEventSynchronize(l2.ev_win));
        win_here = true;
        win      = static_cast<lx::L2Window const *>(l2.p_win.ptr);
        return LX_OK;
    }

    // ---- one part through the pipeline, and its records
    int serve_part(int pi, uint64_t lo, uint64_t hi, int part_slot)
    {
        if (lo == hi)
            return LX_OK;
        Part pt;
        pt.pi           = pi;
        pt.lo           = lo;
        pt.n            = hi - lo;
        pt.slot         = part_slot;
        pt.ri.d_q       = l2.d_qres.ptr;
        pt.ri.q_bytes   = l2.q_bytes;
        pt.ri.d_ext_all = static_cast<lx_extension const *>(h->d_ext_all.ptr) + lo;
        pt.ri.d_min_all = static_cast<int32_t const *>(h->d_min_all.ptr) + lo;
        // the bisulfite overload of computeAlignmentStats (src/evaluate_bisulfite_alignment.hpp:97) for bisulfite lists
        pt.ri.bs_rule   = params->bisulfite ? 1 : h->opt_bs_rule;
        // The plan of the sweep on the device: the solo packing where 16 profiles fit a wavefront's share of the LDS (nucleotides,
        // bisulfite), else the free packing (protein lists: four queries per wavefront) -- nothing of size n comes to the host either way
        pt.solo = solo_plan_applies(h, part_slot);
        int rc;
        if (pt.solo || free_plan_applies(h, part_slot))
        {
            bool finished = false;
            if ((rc = plan_ranges(pt)) || (rc = plan_room(pt)) || (rc = launch_rank(pt)) || (rc = pt.solo ? plan_solo(pt) : plan_free(pt)) || (rc = read_plan(pt)) ||
                (rc = extend_device_plan(pt, finished)) || finished)
                return rc;
        }
        else if ((rc = extend_host_plan(pt)))
            return rc;
        hm.mark("extension");
        return pt.surv.where != ResidentSurvivors::kOnHost ? records_of_the_whole_part(pt) : records_on_the_host(pt);
    }

    // ---- the range plan (lx_level2_plan.h): the strip geometry, how many ranges, and the cuts from the windows around their targets
    int plan_ranges(Part & pt)
    {
        pt.geo = choose_strips(cost + 4 * pt.pi);
        uint64_t const forced = lx::dev_aids().l2_ranges;
        uint64_t       need = 0, have = 1;
        if (records_on_device && !forced)
        {
            uint64_t const panel  = (uint64_t)pt.geo.panel();
            uint64_t const panels = std::max<uint64_t>(1, ((uint64_t)l2.max_qlen + panel - 1) / panel);
            uint64_t const steps  = ((uint64_t)cost[8 + pt.pi] + 8 - 1 + 15) & ~15ull; // (the part's longest window)
            uint64_t const slot_b = panels * (lx::ckpt16_slot_dwords(pt.geo, (uint32_t)std::min<uint64_t>(steps, 65520)) + lx::ckpt_slot_dwords(pt.geo, (uint32_t)std::min<uint64_t>(steps, 65520)) / 8) * 4;
            need = l2_slot_need_bytes(pt.n, slot_b);
            have = std::min<uint64_t>(h->opt_trace_bytes, std::max<uint64_t>(h->d_trace.cap, kL2FreshSlotBytes));
        }
        std::vector<L2Probe> const probes = l2_probe_targets(pt.n, l2_range_count(pt.n, records_on_device, forced, need, have));
        lx::L2Window const *       probe  = nullptr;
        if (!probes.empty())
        {
            // the windows around every cut's target come down together (512 each), one synchronisation
            // (into pinned memory: a copy into ordinary memory is staged by the runtime, 40 us of an idle GPU each)
            if (int const rc = ensure_pinned(h, l2.p_plan, kPlanHead, kRoom))
                return rc;
            lx::L2Window * const to = reinterpret_cast<lx::L2Window *>(static_cast<uint8_t *>(l2.p_plan.ptr) + kPlanProbe);
            for (size_t k = 0; k < probes.size(); ++k)
                LX_HIP(h, hipMemcpyAsync(to + kL2ProbeWindows * k, static_cast<lx::L2Window const *>(l2.d_win.ptr) + pt.lo + probes[k].from,
                                         (probes[k].upto - probes[k].from) * sizeof(lx::L2Window), hipMemcpyDeviceToHost, st));
            LX_HIP(h, hipStreamSynchronize(st));
            probe = to;
        }
        pt.bounds = l2_cuts(probe, probes, pt.n, (uint32_t)std::max(1, params->qry_num_frames));
        return LX_OK;
    }

    // ---- the plan's wavefronts: counted (solo) or bounded (free packing), and their room
    int plan_room(Part & pt)
    {
        pt.cut_wf.assign(1, 0);
        if (pt.solo)
        {
            for (size_t r = 0; r < pt.ranges(); ++r)
            {
                pt.nwf += (pt.bounds[r + 1] - pt.bounds[r] + 15) / 16;
                pt.cut_wf.push_back(pt.nwf);
            }
            pt.cap_wf = pt.nwf;
        }
        else
            pt.cap_wf = lx::fp_wavefront_bound(pt.n, l2.q_len.size(), (uint32_t)pt.ranges());
        int rc;
        if ((rc = ensure_plan(h, pt.cap_wf)) || (rc = ensure_pinned(h, l2.p_plan, kPlanHead, kRoom)))
            return rc;
        return LX_OK;
    }
    uint32_t * d_pan() const { return static_cast<uint32_t *>(l2.d_wf.ptr); }
    uint32_t * d_maxs(Part const & pt) const { return d_pan() + pt.cap_wf; }
    uint32_t * h_report() const { return static_cast<uint32_t *>(l2.p_plan.ptr) + 16; }
    uint32_t * h_rankflag() const { return reinterpret_cast<uint32_t *>(static_cast<uint64_t *>(l2.p_cnt.ptr) + 15); } // (pinned; level2_windows reads words 0-12)

    // ---- the rank kernel
    // (records on the device: every window's place in the records' order, once -- lx_records.hip: the ranges' survivors are sorted by
    // it.  One large kernel that needs the window list only: on the second stream, beside the plan's three dozen small launches)
    int launch_rank(Part & pt)
    {
        pt.try_rank   = records_on_device && pt.n < 0xfffffff0ull;
        *h_rankflag() = 0;
        if (!pt.try_rank)
            return LX_OK;
        if (int const rc = ensure(h, l2.d_rank, (pt.n + 1) * sizeof(uint32_t) + 16))
            return rc;
        for (Event & ev : l2.ev_rank)
            if (!ev)
                LX_HIP(h, hipEventCreateWithFlags(ev.out(), hipEventDisableTiming));
        uint32_t * const d_rank = static_cast<uint32_t *>(l2.d_rank.ptr);
        LX_HIP(h, hipEventRecord(l2.ev_rank[0], st)); // (the window list is complete behind what `st` holds now)
        LX_HIP(h, hipStreamWaitEvent(h->stream2, l2.ev_rank[0], 0));
        LX_HIP(h, hipMemsetAsync(d_rank + pt.n, 0, sizeof(uint32_t), h->stream2));
        LX_HIP(h, lx::rec_launch_rank(static_cast<lx::L2Window const *>(l2.d_win.ptr) + pt.lo, pt.n, (uint32_t)std::max(1, params->qry_num_frames),
                                      static_cast<uint32_t const *>(l2.d_qlen.ptr), d_rank, d_rank + pt.n, h->stream2));
        LX_HIP(h, hipMemcpyAsync(h_rankflag(), d_rank + pt.n, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream2));
        LX_HIP(h, hipEventRecord(l2.ev_rank[1], h->stream2));
        return LX_OK;
    }

    // ---- the solo plan (the solo packing of lx_sweep_mq.hip: every window its own profile): all windows of a range by (columns per
    // lane, length), 16 to a wavefront
    int plan_solo(Part & pt)
    {
        for (size_t r = 0; r < pt.ranges(); ++r)
        {
            uint64_t * key = static_cast<uint64_t *>(l2.d_pair[0].ptr), * key_tmp = static_cast<uint64_t *>(l2.d_pair[1].ptr);
            uint64_t * idx = static_cast<uint64_t *>(l2.d_s0[0].ptr), * idx_tmp = static_cast<uint64_t *>(l2.d_s0[1].ptr);
            uint64_t const w0 = pt.cut_wf[r];
            LX_HIP(h, lx::l2_launch_plan(static_cast<lx::Extension const *>(pt.ri.d_ext_all) + pt.bounds[r], pt.bounds[r + 1] - pt.bounds[r], pt.geo.c,
                                         0, &key, &key_tmp, &idx, &idx_tmp, static_cast<uint32_t *>(l2.d_hist.ptr),
                                         static_cast<uint32_t *>(l2.d_plan.ptr) + w0 * 16, d_pan() + w0, d_maxs(pt) + w0, st, (uint32_t)pt.bounds[r],
                                         lx::l2_plan_key_bits(l2.max_qlen, cost[8 + pt.pi])));
        }
        return LX_OK;
    }

    // ---- the free-packing plan; how many wavefronts it takes is the plan's to say (its report comes down with the rank kernel's flag)
    int plan_free(Part & pt)
    {
        lx::FpArgs fa;
        if (int const rc = launch_free_plan(h, pt.ri.d_ext_all, l2.q_len.size(), pt.geo.c, pt.bounds, fa))
            return rc;
        LX_HIP(h, hipMemcpyAsync(h_report(), fa.report, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        return LX_OK;
    }
    int free_plan_report(Part & pt)
    {
        LX_HIP(h, hipStreamSynchronize(st));
        uint32_t const * const rep = h_report();
        pt.nwf = rep[0];
        if (rep[1] || pt.nwf == 0 || pt.nwf > pt.cap_wf)
            return free_plan_flag(h, pt.n, l2.q_len.size(), pt.nwf, pt.cap_wf, rep[1]);
        for (size_t r = 0; r < pt.ranges(); ++r)
            pt.cut_wf.push_back(rep[4 + r + 1]);
        if (pt.cut_wf.back() != pt.nwf)
            return fail(h, LX_ESTATE, "the free-packing plan's ranges end at wavefront %llu of %llu", (unsigned long long)pt.cut_wf.back(), (unsigned long long)pt.nwf);
        return LX_OK;
    }

    // ---- what the host reads of the plan, in pinned memory: columns per lane and longest window per wavefront
    int read_plan(Part & pt)
    {
        int rc;
        if (pt.try_rank)
            LX_HIP(h, hipStreamWaitEvent(st, l2.ev_rank[1], 0)); // (the records kernels on `st` read the ranks)
        if (!pt.solo && (rc = free_plan_report(pt)))
            return rc;
        // (no copy into the block is pending here: it may move)
        if ((rc = ensure_pinned(h, l2.p_plan, kPlanHead + 2 * pt.nwf * sizeof(uint32_t), kRoom)))
            return rc;
        uint32_t * const h_pan = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(l2.p_plan.ptr) + kPlanHead), * const h_maxs = h_pan + pt.nwf;
        LX_HIP(h, hipMemcpyAsync(h_pan, d_pan(), pt.nwf * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        LX_HIP(h, hipMemcpyAsync(h_maxs, d_maxs(pt), pt.nwf * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if ((windows_to_host || !records_on_device) && (rc = queue_windows()))
            return rc;
        LX_HIP(h, hipStreamSynchronize(st)); // (behind the rank kernel's event as well: its flag has arrived)
        pt.rank_overflow   = *h_rankflag();
        pt.ri.d_plan       = static_cast<uint32_t const *>(l2.d_plan.ptr);
        pt.ri.nwf          = pt.nwf;
        pt.ri.wf_pan       = h_pan;
        pt.ri.wf_maxs      = h_maxs;
        pt.ri.mq_geo       = pt.geo;
        pt.ri.free_packing = !pt.solo;
        pt.ri.cells        = cost[4 * pt.pi + 3];
        return LX_OK;
    }

    // ---- the pipeline over a device plan; finished: it made the records range by range, each behind its chunk
    int extend_device_plan(Part & pt, bool & finished)
    {
        int rc;
        pt.ri.keep_on_device = records_on_device;
        pt.ri.want_codes     = !(params->flags & LX_ITERATE_NO_OPS);
        RecordsJob job(h, params, res, hm, pt.lo, pt.n);
        job.top = top;
        ResidentInput::ChunkRecords cr;
        if (records_on_device)
        {
            std::vector<RecordsJob::Range> ranges;
            uint64_t                       max_entries = 0;
            for (size_t r = 0; r < pt.ranges(); ++r)
            {
                ranges.push_back(RecordsJob::Range{pt.bounds[r], pt.bounds[r + 1]});
                max_entries = std::max(max_entries, (pt.cut_wf[r + 1] - pt.cut_wf[r]) * 16 + 16);
            }
            uint64_t max_wlen = 1; // (the plan's per-wavefront maxima: every window of the part stands in one of them)
            for (uint64_t w = 0; w < pt.nwf; ++w)
                max_wlen = std::max<uint64_t>(max_wlen, pt.ri.wf_maxs[w]);
            if ((rc = job.prepare(cutOffFor, std::move(ranges), max_entries, max_wlen)))
                return rc;
            job.use_rank = pt.try_rank && pt.rank_overflow == 0; // (a query with more windows than the rank kernel counts: the full sort words)
            cr.cut_wf    = pt.cut_wf.data();
            cr.n_ranges  = pt.ranges();
            cr.enqueue   = [&job](uint64_t r, void const * d_hsp, void const * d_src, void const * d_count, uint64_t cap) { return job.enqueue(r, d_hsp, d_src, d_count, nullptr, cap); };
            cr.collect   = [&job](uint64_t r, uint64_t code_base, bool gpu_busy) { return job.collect(r, code_base, gpu_busy); };
            pt.ri.chunk_records = &cr;
        }
        hm.mark("plan");
        rc = extend_list_resident(h, pt.slot, pt.ri, nullptr, pt.n, nullptr, l2.score.data() + pt.lo, &pt.list, &pt.surv);
        pt.ri.chunk_records = nullptr; // (`cr` and `job` end here)
        if (rc || pt.surv.where != ResidentSurvivors::kOnDeviceByRange)
            return rc;
        if (job.next_flush != job.ranges.size())
            return fail(h, LX_ESTATE, "the pipeline finished with %llu of %llu ranges' records made", (unsigned long long)job.next_flush,
                        (unsigned long long)job.ranges.size());
        char name[80];
        snprintf(name, sizeof(name), "extension + records (range by range), %llu ranges", (unsigned long long)job.ranges.size());
        hm.mark(name);
        if (top)
            top->done = true;
        finished = true;
        return LX_OK;
    }

    // ---- the pipeline where the plan is made on the host (lx_host.cpp): its copies of the slices and cut-offs
    int extend_host_plan(Part & pt)
    {
        int rc;
        if ((rc = queue_windows()))
            return rc;
        if (!win_here)
        {
            if ((rc = wait_windows()))
                return rc;
            l2.ext.resize(nw);
            l2.min.resize(nw);
            parallelRanges(nw,
                           [&](unsigned, uint64_t lo, uint64_t hi)
                           {
                               for (uint64_t i = lo; i < hi; ++i)
                               {
                                   lx::L2Window const & w = win[i];
                                   lx_extension &       e = l2.ext[i];
                                   e.q_off   = l2.q_off[w.q];
                                   e.q_len   = l2.q_len[w.q];
                                   e.s_off   = l2.s_off[w.s] + w.beg;
                                   e.s_len   = w.end > w.beg ? (uint32_t)(w.end - w.beg) : 0u;
                                   l2.min[i] = table[l2.q_evlen[w.q]];
                               }
                           });
            hm.mark("windows");
        }
        pt.ri.keep_on_device = records_on_device;
        pt.ri.want_codes     = !(params->flags & LX_ITERATE_NO_OPS);
        return extend_list_resident(h, pt.slot, pt.ri, l2.ext.data() + pt.lo, pt.n, l2.min.data() + pt.lo, l2.score.data() + pt.lo, &pt.list, &pt.surv);
    }

    // ---- the records of a part whose survivors of all chunks stand in l2.d_surv_*: one range, its kernels now
    int records_of_the_whole_part(Part & pt)
    {
        int        rc;
        RecordsJob whole(h, params, res, hm, pt.lo, pt.n);
        whole.top = top;
        if ((rc = whole.prepare(cutOffFor, {RecordsJob::Range{0, pt.n}}, pt.surv.total)) ||
            (rc = whole.enqueue(0, l2.d_surv_hsp.ptr, l2.d_surv_src.ptr, nullptr, l2.d_surv_codes.ptr, pt.surv.total)))
            return rc;
        LX_HIP(h, hipStreamSynchronize(st));
        hm.mark("statistics+order+records (kernels)");
        if ((rc = whole.collect(0, 0, false)))
            return rc;
        hm.mark("rows + columns");
        if (top)
            top->done = true;
        return LX_OK;
    }

    // ---- the records of a part that the pipeline served without the multi-query plan -- a handful of windows, LX_OPT_MQ_SWEEP = 0 --
    // so that its survivors and scores are on the host: the host threads finish them, as for LX_OPT_ITERATE_RECORDS = 1
    int records_on_the_host(Part & pt)
    {
        int rc;
        if (!win_here && ((rc = queue_windows()) || (rc = wait_windows())))
            return rc;
        uint64_t const base = pt.lo;
        auto const     window = [&](uint64_t i)
        {
            lx::L2Window const & w = win[base + i];
            return lambda_amd::WindowView{w.q, w.s, 0, w.beg, l2.q_len[w.q], w.end > w.beg ? (uint32_t)(w.end - w.beg) : 0u, l2.q_evlen[w.q]};
        };
        auto const minOf = [&](uint64_t i) { return table[l2.q_evlen[win[base + i].q]]; };
        if ((rc = lambda_amd::finishSurvivors(pt.n, window, l2.score.data() + pt.lo, minOf, pt.list, params, res)))
            return fail(h, rc, "out of host memory for the result records");
        hm.mark("statistics+records");
        return LX_OK;
    }
};

} // namespace

// n_windows (may be NULL): what the list came to -- where windows_to_host, that many entries of l2.p_win
static int level2_sorted_tail(lx_handle * h, int slot, uint64_t n_matches, lx_search_params const * params, lx_iterate_result * res, bool windows_to_host,
                              TopRequest * top_req, uint64_t * n_windows)
{
    Level2Tail tail(h, slot, n_matches, params, res, windows_to_host, top_req);
    return tail.run(n_windows);
}

namespace
{

// 64-bit content hash of a buffer over the host threads: pieces of 1 MiB, each folded with a multiply-xorshift, combined in order
// (never 0: that is "no hash")
uint64_t content_hash(void const * data, uint64_t bytes, uint64_t seed)
{
    uint8_t const * const p       = static_cast<uint8_t const *>(data);
    uint64_t const        piece   = 1ull << 20, npieces = (bytes + piece - 1) / piece;
    std::vector<uint64_t> hp(npieces, 0);
    unsigned const        nt = npieces >= 8 ? std::max(1u, lxi::pool_width()) : 1u;
    auto fold = [&](unsigned t)
    {
        for (uint64_t k = t; k < npieces; k += nt)
        {
            uint64_t const a = k * piece, b = std::min(bytes, a + piece);
            uint64_t       x = 0x9E3779B97F4A7C15ull ^ k, i = a;
            for (; i + 8 <= b; i += 8)
            {
                uint64_t w;
                std::memcpy(&w, p + i, 8);
                x = (x ^ w) * 0xD6E8FEB86659FD93ull;
                x ^= x >> 32;
            }
            for (; i < b; ++i)
                x = (x ^ p[i]) * 0xD6E8FEB86659FD93ull;
            hp[k] = x;
        }
    };
    if (nt <= 1)
        fold(0);
    else
        lxi::pool_run(nt, fold);
    uint64_t x = seed ^ (bytes * 0x9E3779B97F4A7C15ull);
    for (uint64_t v : hp)
    {
        x = (x ^ v) * 0xD6E8FEB86659FD93ull;
        x ^= x >> 29;
    }
    return x ? x : 1;
}

} // namespace

int lxi::iterate_host_list_on_device(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint64_t const * q_seq_off, uint64_t const * q_seq_len,
                                     uint64_t n_qseq, uint64_t const * q_orig_len, uint8_t const * s_res, uint64_t s_bytes, uint64_t const * s_seq_off,
                                     uint64_t const * s_seq_len, uint64_t n_sseq, lx_match * matches, uint64_t n_matches, lx_search_params const * params,
                                     lx_iterate_result * res)
{
    using namespace lambda_amd;
    // what this path serves: lists large enough to pay for the hand-over, the reference's full rectangle, resident subjects
    if (n_matches < 4 * kParallelFrom || n_matches > 0x7ffffff0ull || params->band > 0 || h->opt_band || s_res != nullptr || s_bytes != 0 || !h->db_bytes || n_qseq >= (1ull << 31) ||
        n_sseq >= (1ull << 32) || lx::dev_aids().iterate_on_host)
        return kNotTaken;
    if (!params->bisulfite && (slot < 0 || slot > 1 || !h->have_sc[slot]))
        return kNotTaken; // (the host form reports it)
    if (params->bisulfite && (!h->have_sc[0] || !h->have_sc[1]))
        return kNotTaken;
    auto &    l2 = h->l2;
    HostMarks hm("lx_iterate_matches (device list work)");
    HostPool::Call const in_flight_call;
    int       rc;
    if ((rc = bind(h)))
        return rc;
    // ---- the sequence sets: resident already (the same content as last time) or set now
    int const      frames = std::max(1, params->qry_num_frames);
    uint64_t const n_orig = q_orig_len ? (n_qseq + (uint64_t)frames - 1) / (uint64_t)frames : 0;
    uint64_t const qh     = (content_hash(q_res, q_bytes, 1) ^ content_hash(q_seq_off, n_qseq * 8, 2) ^ content_hash(q_seq_len, n_qseq * 8, 3) ^
                         content_hash(q_orig_len, n_orig * 8, 4) ^ (uint64_t)frames) | 1;
    if (l2.q_len.size() != n_qseq || l2.q_bytes != q_bytes || l2.q_frames != frames || l2.q_hash != qh || n_qseq == 0)
    {
        if ((rc = lx_set_queries(h, q_res, q_bytes, q_seq_off, q_seq_len, n_qseq, q_orig_len, frames)))
            return rc == LX_EINVAL ? kNotTaken : rc; // (a set the resident form does not take: the host form copes or reports)
        l2.q_hash = qh;
    }
    uint64_t const sh = (content_hash(s_seq_off, n_sseq * 8, 5) ^ content_hash(s_seq_len, n_sseq * 8, 6)) | 1;
    if (l2.s_len.size() != n_sseq || l2.s_hash != sh || n_sseq == 0)
    {
        if ((rc = lx_set_subject_seqs(h, s_seq_off, s_seq_len, n_sseq)))
            return rc == LX_EINVAL ? kNotTaken : rc;
        l2.s_hash = sh;
    }
    if (l2.s_extent > h->db_bytes)
        return kNotTaken;
    hm.mark("sets");
    // ---- the matches as sort words (lx_level2.h), made by the host threads straight into pinned memory, 16 bytes each
    if ((rc = ensure_pinned(h, l2.p_up, n_matches * 16 + 16, kRoom)) || (rc = ensure_list_keys(h, n_matches)))
        return rc;
    uint64_t * const      pair = static_cast<uint64_t *>(l2.p_up.ptr), * const s0 = pair + n_matches;
    std::vector<uint8_t>  bad(std::max(1u, lxi::pool_width()), 0);
    bool const            bs = params->bisulfite != 0;
    parallelRanges(n_matches,
                   [&](unsigned t, uint64_t lo, uint64_t hi)
                   {
                       for (uint64_t i = lo; i < hi; ++i)
                       {
                           lx_match const & m = matches[i];
                           uint64_t const   d = m.subjStart < m.qryStart ? 0 : m.subjStart - m.qryStart; // _widenMatch's first line, :923
                           if (d >= s_seq_len[m.subjId])
                               bad[t] = 1;
                           pair[i] = ((bs ? (m.subjId & 1) : 0ull) << 63) | (m.qryId << 32) | m.subjId;
                           s0[i]   = d;
                       }
                   });
    for (uint8_t b : bad)
        if (b)
            return fail(h, LX_EINVAL, "a match lies beyond the end of its subject sequence");
    LX_HIP(h, hipMemsetAsync(l2.d_cnt.ptr, 0, 4 * sizeof(uint64_t), h->stream));
    LX_HIP(h, hipMemcpyAsync(l2.d_pair[0].ptr, pair, n_matches * 8, hipMemcpyHostToDevice, h->stream));
    LX_HIP(h, hipMemcpyAsync(l2.d_s0[0].ptr, s0, n_matches * 8, hipMemcpyHostToDevice, h->stream));
    hm.mark("sort words");
    uint64_t nw = 0;
    if ((rc = level2_sorted_tail(h, slot, n_matches, params, res, true, nullptr, &nw)))
        return rc;
    // ---- the reference's span now holds the windows (:1173-1174 shrinks it): the first n_windows records of `matches`
    lx::L2Window const * const win = static_cast<lx::L2Window const *>(l2.p_win.ptr);
    parallelRanges(nw,
                   [&](unsigned, uint64_t lo, uint64_t hi)
                   {
                       for (uint64_t i = lo; i < hi; ++i)
                           matches[i] = lx_match{win[i].q, win[i].s, 0, l2.q_len[win[i].q], win[i].beg, win[i].end};
                   });
    return LX_OK;
}

extern "C" {

static int iterate_matches_dev(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params, TopRequest * top, lx_iterate_result ** out)
{
    if (!h || !out || !params)
        return LX_EINVAL;
    *out = nullptr;
    if (!d_matches && n_matches)
        return fail(h, LX_EINVAL, "NULL argument");
    if (n_matches > 0x7ffffff0ull)
        return fail(h, LX_EINVAL, "at most 2^31 matches per call");
    auto & l2 = h->l2;
    if (l2.q_len.empty() || l2.s_len.empty() || !h->db_bytes)
        return fail(h, LX_ESTATE, "lx_iterate_matches_dev needs the resident sets: lx_set_queries, lx_set_subjects, lx_set_subject_seqs");
    if (l2.s_extent > h->db_bytes)
        return fail(h, LX_EINVAL, "the subject sequences reach byte %llu, the resident residue buffer holds %llu", (unsigned long long)l2.s_extent,
                    (unsigned long long)h->db_bytes);
    if (std::max(1, params->qry_num_frames) != l2.q_frames)
        return fail(h, LX_EINVAL, "qry_num_frames = %d, but the queries were set with %d frames", params->qry_num_frames, l2.q_frames);
    if (params->band > 0 || h->opt_band)
        return fail(h, LX_EINVAL, "lx_iterate_matches_dev: band mode (lx_search_params.band, LX_OPT_BAND) goes through lx_iterate_matches");
    if (params->flags & ~(int32_t)LX_ITERATE_NO_OPS)
        return fail(h, LX_EINVAL, "lx_search_params.flags = 0x%x: unknown bits (this library knows LX_ITERATE_NO_OPS)", (unsigned)params->flags);
    if (!params->bisulfite && (slot < 0 || slot > 1 || !h->have_sc[slot]))
        return fail(h, LX_ESTATE, "scoring slot %d not set", slot);
    if (params->bisulfite && (!h->have_sc[0] || !h->have_sc[1]))
        return fail(h, LX_ESTATE, "bisulfite mode needs both scoring slots");
    int rc = bind(h);
    if (rc)
        return rc;
    auto res = new lx_iterate_result();
    if (n_matches == 0)
    {
        *out = res;
        return LX_OK;
    }
    if ((rc = level2_keys(h, d_matches, n_matches, params->bisulfite != 0)) == LX_OK)
        rc = level2_sorted_tail(h, slot, n_matches, params, res, false, top, nullptr);
    if (rc != LX_OK)
    {
        delete res;
        return rc;
    }
    *out = res;
    return LX_OK;
}

int lx_iterate_matches_dev(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params, lx_iterate_result ** out)
{
    return iterate_matches_dev(h, slot, d_matches, n_matches, params, nullptr, out);
}

static int iterate_matches_dev_top(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params, uint64_t max_matches,
                                   lx_cull_options const * opt, lx_record_stats * rstats, lx_cull_stats * cull_stats, lx_iterate_result ** out)
{
    if (!h || !out || !params)
        return LX_EINVAL;
    TopRequest top;
    top.max_matches = max_matches;
    if (opt && (opt->max_hsps || opt->culling_limit))
    {
        // the lengths are the resident q_orig_len of lx_set_queries (32-bit words per frame sequence, the query's own in front of
        // its frames); iterate_matches_dev refuses a handle without them before any kernel reads them
        auto & l2 = h->l2;
        top.cull.max_hsps      = opt->max_hsps;
        top.cull.culling_limit = opt->culling_limit;
        top.cull.d_q_lens      = static_cast<uint32_t const *>(l2.d_qevlen.ptr);
        top.cull.q_lens_n      = l2.q_len.size();
        top.cull.stride        = (uint32_t)std::max(1, l2.q_frames);
        top.cull.translated    = params->q_frame_mode == LX_FRAMES_TRANSLATED;
    }
    int rc = iterate_matches_dev(h, slot, d_matches, n_matches, params, &top, out);
    if (rc != LX_OK)
        return rc;
    if (!top.done)
    {
        // the finished result (a query's records came out of more than one part of the call, or were made on the host): the same
        // kernels over its rows, then the columns of the rows that stay moved together
        lx_iterate_result * const res = *out;
        uint64_t                  kept = 0;
        if (res->matches.size() >= 0x7ffffff0ull)
            rc = fail(h, LX_EINVAL, "lx_iterate_matches_dev_top: at most 2^31 - 16 records per call");
        else
            rc = toprec_host_rows(h, res->matches.data(), res->matches.size(), max_matches, &top.stats, &kept, &top.cull);
        if (rc == LX_OK && kept && res->ops.size())
        {
            lambda_amd::RawVec<uint8_t> packed;
            uint64_t                    total = 0;
            for (uint64_t k = 0; k < kept; ++k)
                total += res->matches[k].n_ops;
            if (!packed.resize(total))
                rc = fail(h, LX_ENOMEM, "out of host memory for the result records");
            else
            {
                uint64_t at = 0;
                for (uint64_t k = 0; k < kept; ++k)
                {
                    lx_blast_match & r = res->matches[k];
                    std::memcpy(packed.data() + at, res->ops.data() + r.ops_off, r.n_ops);
                    r.ops_off = at;
                    at += r.n_ops;
                }
                std::swap(res->ops.p, packed.p), std::swap(res->ops.n, packed.n), std::swap(res->ops.cap, packed.cap);
            }
        }
        else if (rc == LX_OK && !kept)
            (void)res->ops.resize(0);
        if (rc != LX_OK)
        {
            delete res;
            *out = nullptr;
            return rc;
        }
        (void)res->matches.resize(kept);
    }
    if (rstats)
        *rstats = top.stats;
    if (cull_stats)
        *cull_stats = top.cull.stats;
    return LX_OK;
}

int lx_iterate_matches_dev_top(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params, uint64_t max_matches,
                               lx_record_stats * rstats, lx_iterate_result ** out)
{
    return iterate_matches_dev_top(h, slot, d_matches, n_matches, params, max_matches, nullptr, rstats, nullptr, out);
}

int lx_iterate_matches_dev_top_ex(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params, uint64_t max_matches,
                                  lx_cull_options const * opt, lx_record_stats * rstats, lx_cull_stats * cull_stats, lx_iterate_result ** out)
{
    return iterate_matches_dev_top(h, slot, d_matches, n_matches, params, max_matches, opt, rstats, cull_stats, out);
}

// The Level-2 radix sort (lx_level2.hip: l2_launch_sort) for a caller's own (key, value) words in device memory -- what the front end's
// word table is sorted with (lx_index_build, lx_seed_host.cpp), instead of a library primitive.
int lx_sort_words_dev(int device, uint64_t * key[2], uint64_t * value[2], uint64_t n, uint64_t key_bits, void * stream, int * sorted_in)
{
    if (!key || !value || !sorted_in || (n && (!key[0] || !key[1] || !value[0] || !value[1])) || n > 0x7fffffffull || device < 0 || device >= 64)
        return LX_EINVAL;
    *sorted_in = 0;
    if (n < 2)
        return LX_OK;
    // (the caller's current device is the caller's: restored on every exit)
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess)
        before = -1;
    struct Restore
    {
        int dev;
        ~Restore()
        {
            if (dev >= 0)
                (void)hipSetDevice(dev);
        }
    } const restore{before == device ? -1 : before};
    if (hipSetDevice(device) != hipSuccess)
        return LX_EHIP;
    // the digit counts: one allocation per (process, device), kept and grown -- a hipMalloc + hipFree per call synchronises the device.
    // Raw and never given back, on purpose: an owner (lx_resources.h) with static storage would call hipFree while the process
    // exits, when the runtime may be gone already.
    static std::mutex  hist_m[64];
    static uint32_t *  hist_buf[64] = {nullptr};
    static size_t      hist_cap[64] = {0};
    size_t const want = (lx::l2_sort_tiles(n) + 2) * 256 * sizeof(uint32_t);
    int const    d    = device & 63;
    std::lock_guard<std::mutex> lk(hist_m[d]); // (one sort at a time per DEVICE on its buffer; the devices of a node sort side by side)
    if (hist_cap[d] < want)
    {
        if (hist_buf[d])
            (void)hipFree(hist_buf[d]);
        hist_buf[d] = nullptr;
        hist_cap[d] = 0;
        if (hipMalloc(reinterpret_cast<void **>(&hist_buf[d]), want + want / 2) != hipSuccess)
            return LX_ENOMEM;
        hist_cap[d] = want + want / 2;
    }
    uint32_t * const hist = hist_buf[d];
    uint64_t * k = key[0], * kt = key[1], * v = value[0], * vt = value[1];
    hipError_t e = lx::l2_launch_sort(&k, &kt, &v, &vt, n, key_bits, 0, hist, static_cast<hipStream_t>(stream));
    if (e == hipSuccess)
        e = hipStreamSynchronize(static_cast<hipStream_t>(stream)); // (the digit counts are shared: the sort is over before the next one starts)
    *sorted_in = k == key[0] ? 0 : 1;
    return e == hipSuccess ? LX_OK : LX_EHIP;
}

// The free-packing plan (lx_plan_free.hip) of a window list in device memory, brought to the host: what tests/test_gpu_plan.py checks
// slot by slot.  out_plan: [lx_plan_free_packing_bound(n, n_qseq, nranges) * 16], out_pan / out_maxs: [that bound], out_report: [16].
uint64_t lx_plan_free_packing_bound(uint64_t n, uint64_t n_qseq, uint32_t nranges)
{
    return lx::fp_wavefront_bound(n, n_qseq, nranges);
}

int lx_plan_free_packing_dev(lx_handle * h, void const * d_ext, uint64_t n, uint64_t n_qseq, int32_t strip_cols, uint32_t nranges, uint64_t const * cut, uint32_t * out_plan,
                             uint32_t * out_pan, uint32_t * out_maxs, uint32_t * out_report)
{
    if (!h)
        return LX_EINVAL;
    if (!d_ext || !cut || !out_plan || !out_pan || !out_maxs || !out_report || n == 0 || nranges == 0 || nranges > lx::kFpMaxRanges || n >= 0x7ffffff0ull ||
        (strip_cols != 19 && strip_cols != 13 && strip_cols != 11))
        return fail(h, LX_EINVAL, "lx_plan_free_packing_dev: arguments");
    for (uint32_t r = 0; r < nranges; ++r)
        if (cut[r] >= cut[r + 1])
            return fail(h, LX_EINVAL, "lx_plan_free_packing_dev: range %u is empty", r);
    if (cut[0] != 0 || cut[nranges] != n)
        return fail(h, LX_EINVAL, "lx_plan_free_packing_dev: the ranges must cover the list");
    int rc = bind(h);
    if (rc)
        return rc;
    lx::FpArgs     fa;
    uint64_t const cap = lx::fp_wavefront_bound(n, n_qseq, nranges);
    if ((rc = launch_free_plan(h, d_ext, n_qseq, strip_cols, std::vector<uint64_t>(cut, cut + nranges + 1), fa)))
        return rc;
    LX_HIP(h, hipMemcpyAsync(out_report, fa.report, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    LX_HIP(h, hipMemcpyAsync(out_plan, fa.plan, cap * 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    LX_HIP(h, hipMemcpyAsync(out_pan, fa.wf_pan, cap * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    LX_HIP(h, hipMemcpyAsync(out_maxs, fa.wf_maxs, cap * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    LX_HIP(h, hipStreamSynchronize(h->stream));
    if (out_report[1])
        return free_plan_flag(h, n, n_qseq, out_report[0], cap, out_report[1]);
    return LX_OK;
}

// _widenAndPreprocessMatches (src/search_algo.hpp:1136-1175) alone, on a device match list over the resident sets
int lx_widen_and_preprocess_dev(lx_handle * h, void const * d_matches, uint64_t n_matches, int32_t bisulfite, lx_match * out, uint64_t * out_n)
{
    if (!h || !out_n)
        return LX_EINVAL;
    *out_n = 0;
    if ((!d_matches || !out) && n_matches)
        return fail(h, LX_EINVAL, "NULL argument");
    if (n_matches > 0x7ffffff0ull)
        return fail(h, LX_EINVAL, "at most 2^31 matches per call");
    auto & l2 = h->l2;
    if (l2.q_len.empty() || l2.s_len.empty())
        return fail(h, LX_ESTATE, "lx_widen_and_preprocess_dev needs the resident sets: lx_set_queries, lx_set_subject_seqs");
    int rc = bind(h);
    if (rc || n_matches == 0)
        return rc;
    std::vector<int32_t> const table((size_t)l2.max_evlen + 1, 0);
    uint64_t                   nw = 0, nEven = 0;
    if ((rc = level2_keys(h, d_matches, n_matches, bisulfite != 0)) || (rc = level2_windows(h, n_matches, bisulfite != 0, table, nw, nEven)))
        return rc;
    if (nw)
    {
        if ((rc = ensure_pinned(h, l2.p_win, nw * sizeof(lx::L2Window) + 16, kRoom)))
            return rc;
        LX_HIP(h, hipMemcpyAsync(l2.p_win.ptr, l2.d_win.ptr, nw * sizeof(lx::L2Window), hipMemcpyDeviceToHost, h->stream));
        LX_HIP(h, hipStreamSynchronize(h->stream));
        lx::L2Window const * const win = static_cast<lx::L2Window const *>(l2.p_win.ptr);
        for (uint64_t i = 0; i < nw; ++i)
            out[i] = lx_match{win[i].q, win[i].s, 0, l2.q_len[win[i].q], win[i].beg, win[i].end};
    }
    *out_n = nw;
    return LX_OK;
}

} // extern "C"
