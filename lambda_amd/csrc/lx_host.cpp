// lx_host.cpp -- lx_extend_batch / _rle / _list: the fused step (pass 1, filter, pass 2 -- _performAlignment at
// /root/reference/src/search_algo.hpp:1246 and :1296 with the filter loop :1251-1283 between them) on lists in host memory, as a
// pipeline of chunks (pinned staging, two chunks in flight, run-length coded ops on the wire), and the same pipeline over a list
// that is resident on the device already (lxi::extend_list_resident, what the Level-2 driver calls).  Ragged lists are planned for
// the multi-query sweep here (lx_plan_free.hip plans device lists).  The entry points of the single passes are lx_host_batch.cpp;
// the fused step all of them drive lives in lx_step.cpp; no DP arithmetic here.
#include "lx_internal.h"
#include "lx_level2.h"
using namespace lxi;

// Both passes on host buffers, as a pipeline of chunks.  The list is cut at query-run boundaries into chunks of a few
// hundred thousand extensions; per chunk the host groups the extensions by query slice and pads every run to 16 (or 8)
// slots -- the promise LX_OPT_QUERY_RUN makes to the device path -- into pinned staging, the GPU runs the whole fused step
// (sweep -> selection -> backtrace -> run-length packing of the ops, nothing in between comes back to the host), and the
// results return as scores + the survivors' records + their run-length codes.  Two chunks are in flight: uploads and
// downloads of one run on copy streams while the other's kernels run, and the host prepares chunk k + 1 / unpacks
// chunk k - 1 meanwhile.  What crosses PCIe per extension: 28 B up, 4 B + (survivors) 52 B + ~8 B of codes down.
namespace
{

struct XbPrep // what the host keeps about a chunk until its results are back
{
    uint64_t              k0 = 0, k1 = 0; // positions in the ordered list
    uint64_t              slots = 0, cap_sel = 0;
    bool                  wide = false;   // multi-query chunk: the sweep wrote int16-pair slots
    uint64_t              exec_cells = 0, max_s = 0, max_pan = 0; // (LX_HOST_TIMING: what the chunk's wavefronts execute)
    uint64_t              range = 0;      // records chunk by chunk (ResidentInput::ChunkRecords): the range this chunk is
    std::vector<uint32_t> slot_src;       // original index of every slot (0xffffffff = padding)
};

inline void rle_expand(uint8_t const * codes, int32_t n_ops, uint8_t * out)
{
    static char const kOp[4] = {'M', 'D', 'I', 'M'};
    int32_t done = 0;
    while (done < n_ops)
    {
        uint8_t const c   = *codes++;
        int32_t const len = (c & 63) + 1;
        if (done + ((len + 15) & ~15) <= n_ops)
        {
            // whole 16-byte stores while they stay inside this alignment's columns (the surplus is overwritten by the runs that
            // follow; a call to memset per run of a few columns costs more than the stores)
            for (int32_t k = 0; k < len; k += 16)
                std::memset(out + done + k, kOp[c >> 6], 16);
        }
        else
            std::memset(out + done, kOp[c >> 6], (size_t)len);
        done += len;
    }
}

using Clock = std::chrono::steady_clock;
inline Clock::time_point now() { return Clock::now(); }
inline double            ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// a chunk's survivors as they came down into lane staging: records, list positions (slots, or caller indices), code lengths, codes
struct Survivors
{
    lx_hsp const *   hs;
    uint32_t const * src;
    uint32_t const * code_len;
    uint8_t const *  codes;
    explicit Survivors(lx_handle::XbLane const & ln)
        : hs(static_cast<lx_hsp const *>(ln.p_hsp.ptr)), src(static_cast<uint32_t const *>(ln.p_src.ptr)),
          code_len(static_cast<uint32_t const *>(ln.p_len.ptr)), codes(static_cast<uint8_t const *>(ln.p_rle.ptr)) {}
};

// ONE chunk in TWO calls (slots by wavefront): the plan's pool goes to the GPU -- its slot list, its table, its sweep -- while the
// streamed part of the plan is still being made on the host threads; the second call sweeps the streamed wavefronts into slots
// behind the pool's and runs what follows a sweep ONCE over all of them: one selection, one backtrace, one result list.  (Rounds
// 3-4: the pool as a chunk of its own -- its backtrace is the latency of its longest walks, 1.6 ms for a fifth of the survivors --
// or, for small lists, everything planned before the first launch.)
struct TwoCall
{
    uint64_t n1 = 0, nw1 = 0, dw0 = 0, ovf_cap = 0, ovf_dw = 0, total_dw = 0, stride = 0, max_q = 0, max_s = 0, cap_slots = 0;
};

// The device half of a call: the host plan (h->plan) run as chunks in two lanes.  One driver per path -- run_one for the
// one-query-per-wavefront kernels (chunks = ranges of the ordered list), run_mq for the multi-query sweep (chunks = ranges of the
// plan's wavefronts) -- and the redo of chunks whose overflow area filled up.
class ExtendPipeline
{
public:
    ExtendPipeline(lx_handle * h_, int slot_, lx_extension const * ext_, uint64_t n_, int32_t const * min_score_, int32_t min_score_all_,
                   int32_t * out_score_, lx_hsp * out_hsp_, uint64_t * out_ops_off_, uint8_t const ** out_ops_, uint64_t * out_ops_bytes_, int mode,
                   ResidentInput const * ri_, HostMarks & hm_)
        : h(h_), slot(slot_), ext(ext_), n(n_), min_score(min_score_), min_score_all(min_score_all_), out_score(out_score_), out_hsp(out_hsp_),
          out_ops_off(out_ops_off_), out_ops(out_ops_), out_ops_bytes(out_ops_bytes_), want_rle(mode >= 1), as_list(mode == 2), ri(ri_),
          preplanned(ri_ && ri_->d_plan), p(h_->plan), hm(hm_), nthreads(host_threads(n_)), bs_rule(ri_ ? ri_->bs_rule : h_->opt_bs_rule)
    {
    }

    // the caller's list and cut-offs onto the device (pinned staging, filled by the host threads; scores in caller order zeroed)
    int upload_list()
    {
        int rc2;
        auto const tu0 = now();
        uint64_t const ext_bytes = n * sizeof(lx_extension), min_bytes = min_score ? n * sizeof(int32_t) : 0;
        // (the scores of a list whose records are made on the device stay there: no pinned block for their way down)
        if ((rc2 = ensure(h, h->d_score_all, n * sizeof(int32_t) + 16)) ||
            (!(as_list && ri && ri->keep_on_device) && (rc2 = ensure_pinned(h, h->p_score_all, n * sizeof(int32_t) + 16, kRoom))))
            return rc2;
        if (!ri) // (a resident list stands where the Level-2 kernels wrote it)
        {
            if ((rc2 = ensure_pinned(h, h->p_all, ext_bytes + min_bytes + 16, kRoom)) || (rc2 = ensure(h, h->d_ext_all, ext_bytes + 16)) ||
                (rc2 = ensure(h, h->d_min_all, min_bytes + 16)))
                return rc2;
            uint8_t * const stage_all = static_cast<uint8_t *>(h->p_all.ptr);
            parallel_ranges(n, nthreads,
                            [&](unsigned, uint64_t lo, uint64_t hi)
                            {
                                std::memcpy(stage_all + lo * sizeof(lx_extension), ext + lo, (hi - lo) * sizeof(lx_extension));
                                if (min_score)
                                    std::memcpy(stage_all + ext_bytes + lo * sizeof(int32_t), min_score + lo, (hi - lo) * sizeof(int32_t));
                            });
            LX_HIP(h, hipMemcpyAsync(h->d_ext_all.ptr, stage_all, ext_bytes, hipMemcpyHostToDevice, h->stream));
            if (min_score)
                LX_HIP(h, hipMemcpyAsync(h->d_min_all.ptr, stage_all + ext_bytes, min_bytes, hipMemcpyHostToDevice, h->stream));
        }
        LX_HIP(h, hipMemsetAsync(h->d_score_all.ptr, 0, n * sizeof(int32_t), h->stream));
        t_upload      = ms(tu0, now());
        list_uploaded = true;
        return LX_OK;
    }

    int run(void const * d_q_, void const * d_s_)
    {
        d_q          = d_q_;
        d_s          = d_s_;
        chunk_target = h->opt_extend_chunk ? std::max<uint64_t>(h->opt_extend_chunk, 1024) : lxi::kExtendChunk;
        h->ext_bytes.clear();
        h->xb_stats[0] = p.live;
        h->xb_stats[1] = h->xb_stats[2] = h->xb_stats[3] = 0; // slots, cells, cells the wavefronts execute
        if (int const rc = p.use_mq ? run_mq() : run_one())
            return rc;
        hm.mark("pipeline"); // (every chunk's error word came back with its counts: collect())
        if (hm.on)
            fprintf(stderr, "[lx host ms]   pipeline of %d chunks: prepare %.1f, issue %.1f, wait for the GPU %.1f, unpack %.1f (lengths %.1f, offsets %.1f)\n", c, t_prep, t_issue,
                    t_wait, t_unpack, t_u1, t_u2);
        if (as_list)
            h->xb_ops_total = ops_total;
        else
        {
            *out_ops       = h->ext_bytes.data();
            *out_ops_bytes = ops_total;
        }
        return LX_OK;
    }

    // where run() left the survivors (ResidentInput::keep_on_device: on the device where the multi-query plan served the list)
    ResidentSurvivors::Where survivors_where() const
    {
        return !dev_list ? ResidentSurvivors::kOnHost : by_range ? ResidentSurvivors::kOnDeviceByRange : ResidentSurvivors::kOnDevice;
    }

private:
    lx_handle * const           h;
    int const                   slot;
    lx_extension const * const  ext; // the caller's list, cut-offs and outputs
    uint64_t const              n;
    int32_t const * const       min_score;
    int32_t const               min_score_all;
    int32_t * const             out_score;
    lx_hsp * const              out_hsp;
    uint64_t * const            out_ops_off;
    uint8_t const ** const      out_ops;
    uint64_t * const            out_ops_bytes;
    bool const                  want_rle, as_list;
    ResidentInput const * const ri;
    bool const                  preplanned;
    HostPlan const &            p;
    HostMarks &                 hm;
    unsigned const              nthreads;
    uint64_t const              bs_rule; // the backtrace's match rule
    void const *                d_q = nullptr, *d_s = nullptr; // query and subject residues on the device
    XbPrep                      prep[2];                       // the two lanes
    bool                        in_flight[2] = {false, false};
    int                         c            = 0; // chunks issued
    TwoCall                     two;
    std::vector<std::pair<uint64_t, uint64_t>> redo; // chunks (wavefront ranges) to run again with int16-pair slots
    uint64_t chunk_target = 0, per_chunk = 0, ops_total = 0; // (ops_total: bytes handed out in h->ext_bytes so far)
    bool     dev_list = false, want_codes = true, by_range = false; // (set where the multi-query plan is known: ResidentInput::keep_on_device)
    bool     list_uploaded = false, rows_cleared = false, stream_planned = false, merge_pool = false;
    bool     mq_wide = false; // the multi-query chunks' sweep writes int16-pair slots (decided chunk by chunk, with hysteresis: enqueue_mq)
    double   t_upload = 0, t_prep = 0, t_issue = 0, t_wait = 0, t_unpack = 0, t_u1 = 0, t_u2 = 0; // LX_HOST_TIMING: where the host's time goes

    bool     wide_ok() const { return p.mq_cfg == 1 && !lx::dev_aids().mq_no_wide; }
    bool     maybe_wide() const { return wide_ok() && h->mq_decl_frac > 0.01; }
    uint64_t wf_dwords(uint64_t w, bool wide) const { return kWave * slot_dwords(p.mq_cfg, p.wf_pan[w], p.wf_maxs[w], wide); }

    // the lanes' chunks still in flight, oldest first
    int drain(bool mq)
    {
        int rc;
        for (int L : {c & 1, (c & 1) ^ 1})
            if (in_flight[L] && (rc = mq ? collect_mq(L) : collect(L)))
                return rc;
        return LX_OK;
    }

    // ---- the pipeline of the one-query-per-wavefront kernels: prepare + queue chunk c, then unpack chunk c - 1 while c runs
    int run_one()
    {
        int rc;
        for (uint64_t k0 = 0; k0 < p.live; ++c)
        {
            // about chunk_target extensions: never cut a query's run, and never mix geometry classes (the list is class-major)
            uint64_t k1 = std::min<uint64_t>(p.live, k0 + chunk_target);
            while (k1 < p.live && !p.newrun[k1])
                ++k1;
            uint32_t const c0 = query_class(ext[p.idx[k0]].q_len);
            if (query_class(ext[p.idx[k1 - 1]].q_len) != c0)
            {
                uint64_t lo = k0, hi = k1 - 1; // first position of another class: the classes ascend
                while (hi - lo > 1)
                {
                    uint64_t const mid = lo + (hi - lo) / 2;
                    (query_class(ext[p.idx[mid]].q_len) == c0 ? lo : hi) = mid;
                }
                k1 = hi;
                while (k1 > k0 + 1 && !p.newrun[k1])
                    --k1;
            }
            int const L = c & 1;
            if (in_flight[L] && (rc = collect(L)))
                return rc;
            if ((rc = enqueue(L, k0, k1)))
                return rc;
            if (in_flight[L ^ 1] && (rc = collect(L ^ 1)))
                return rc;
            k0 = k1;
        }
        return drain(false);
    }

    // lane L's device buffers: `slots` slots (+ caller indices: orig), prep[L].cap_sel survivors with ops slots of `stride` bytes, counts
    int size_lane(int L, uint64_t slots, uint64_t stride, bool orig, bool mq)
    {
        lx_handle::XbLane & ln      = h->xb[L];
        uint64_t const      cap_sel = prep[L].cap_sel, words = mq ? 5 : 4;
        int                 rc2;
        if ((orig && (rc2 = ensure(h, ln.d_orig, slots * sizeof(uint32_t)))) || (rc2 = ensure(h, ln.d_ext, slots * sizeof(lx_extension))) ||
            (rc2 = ensure(h, ln.d_min, slots * sizeof(int32_t))) || (rc2 = ensure(h, ln.d_score, slots * sizeof(int32_t))) ||
            (rc2 = ensure(h, ln.d_hsp, cap_sel * sizeof(lx_hsp))) || (rc2 = ensure(h, ln.d_ops, cap_sel * stride + 16)) ||
            (rc2 = ensure(h, ln.d_rle, cap_sel * stride + 16)) || (rc2 = ensure(h, ln.d_src, cap_sel * sizeof(uint32_t))) ||
            (rc2 = ensure(h, ln.d_len, cap_sel * sizeof(uint32_t))) || (rc2 = ensure(h, ln.d_cnt, words * sizeof(uint64_t))) ||
            (!mq && (rc2 = ensure_pinned(h, ln.p_score, slots * sizeof(int32_t), kRoom))) || (rc2 = ensure_pinned(h, ln.p_cnt, words * sizeof(uint64_t), kRoom)))
            return rc2;
        return LX_OK;
    }

    // the fused step over lane L's first `slots` slots, on the kernel stream: what it may assume of the chunk -- its widest query, its
    // longest window, its query run (1: the solo packing, 2: the free packing) -- and, for multi-query chunks, its slots by wavefront
    int run_fused(int L, uint64_t slots, uint64_t stride, uint64_t max_q, uint64_t max_s, uint64_t run, MqTab const & tab = MqTab{})
    {
        lx_handle::XbLane & ln    = h->xb[L];
        uint64_t * const    d_cnt = static_cast<uint64_t *>(ln.d_cnt.ptr);
        StepCall            c;
        c.d_q = d_q, c.d_s = d_s, c.d_ext = ln.d_ext.ptr, c.n = slots, c.d_min_score = ln.d_min.ptr;
        c.d_out_score = ln.d_score.ptr, c.d_out_hsp = ln.d_hsp.ptr, c.d_out_ops = ln.d_ops.ptr, c.d_out_count = d_cnt;
        c.stream       = h->stream;
        c.by_pos       = true;
        c.fx.ops_stride = stride; // one ops slot per position of the survivor list
        c.fx.d_rle      = static_cast<uint8_t *>(ln.d_rle.ptr);
        c.fx.d_rle_top  = reinterpret_cast<unsigned long long *>(d_cnt + 2);
        c.fx.rle_cap    = prep[L].cap_sel * stride;
        c.fx.d_src_out  = static_cast<uint32_t *>(ln.d_src.ptr);
        c.fx.d_rle_len  = static_cast<uint32_t *>(ln.d_len.ptr);
        c.lim           = ListLimits{max_q, max_s, run, h->band_dev, bs_rule};
        c.tab           = tab;
        c.mq_cfg        = p.use_mq ? p.mq_cfg : 0;
        c.mq_wide       = mq_wide;
        c.keep_events   = true; // (the call's phase list holds every chunk's events)
        return fused_impl(h, slot, c);
    }

    // ---- device side of a chunk whose padded slots stand in lane L's pinned staging: uploads and kernels queued
    int launch_chunk(int L, uint64_t slots, uint64_t max_q, uint64_t max_s, uint64_t kRun)
    {
        auto const           t1       = now();
        lx_handle::XbLane &  ln       = h->xb[L];
        lx_extension * const slot_ext = static_cast<lx_extension *>(ln.p_ext.ptr);
        int32_t * const      slot_min = static_cast<int32_t *>(ln.p_min.ptr);
        int                  rc2;
        uint64_t const       stride = (max_q + max_s + 3) & ~3ull;
        if ((rc2 = size_lane(L, slots, stride, false, false)))
            return rc2;
        LX_HIP(h, hipMemcpyAsync(ln.d_ext.ptr, slot_ext, slots * sizeof(lx_extension), hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipMemcpyAsync(ln.d_min.ptr, slot_min, slots * sizeof(int32_t), hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
        hipStream_t const ks = h->stream; // (all chunks' kernels in one stream: side by side they were measured slower, see extend_pipeline)
        LX_HIP(h, hipStreamWaitEvent(ks, ln.ev_up, 0));
        if ((rc2 = run_fused(L, slots, stride, max_q, max_s, kRun)))
            return rc2;
        // the device's error word of THIS chunk, saved in stream order (the next chunk's prepare_workspace clears it): it comes
        // back with the counts and is checked in collect()
        uint64_t * const d_cnt = static_cast<uint64_t *>(ln.d_cnt.ptr);
        hipStream_t const ke = ks;
        LX_HIP(h, hipMemcpyAsync(d_cnt + 3, ws_word(h, kWsBump), 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, ke));
        LX_HIP(h, hipEventRecord(ln.ev_k, ke));
        // what has a size the host knows goes back at once; records and codes follow when the counts have arrived
        LX_HIP(h, hipStreamWaitEvent(h->stream2, ln.ev_k, 0));
        LX_HIP(h, hipMemcpyAsync(ln.p_cnt.ptr, d_cnt, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream2));
        LX_HIP(h, hipMemcpyAsync(ln.p_score.ptr, ln.d_score.ptr, slots * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream2));
        LX_HIP(h, hipEventRecord(ln.ev_cnt, h->stream2));
        in_flight[L] = true;
        t_issue += ms(t1, now());
        return LX_OK;
    }

    // ---- chunk k0 .. k1 of the ordered list -> padded slots in lane L's pinned staging -> uploads and kernels queued
    int enqueue(int L, uint64_t k0, uint64_t k1)
    {
        auto const          t0 = now();
        lx_handle::XbLane & ln = h->xb[L];
        XbPrep &            pr = prep[L];
        std::vector<uint32_t> const & idx    = p.idx;
        std::vector<uint8_t> const &  newrun = p.newrun;
        pr.k0 = k0;
        pr.k1 = k1;
        // runs of one query slice; padded to 16 slots (one query per wavefront of the 8-lane packed geometry) or, when the
        // queries have few windows each, to 8 (one query per half wavefront, or the 16-lane geometries) -- whichever is less work
        std::vector<uint64_t> & grp = h->xb_grp; // (first position, first slot) of every run + a sentinel
        grp.clear();
        uint64_t slots16 = 0, slots8 = 0, max_q = 1, max_s = 1;
        for (uint64_t k = k0; k < k1;)
        {
            uint64_t kk = k + 1;
            while (kk < k1 && !newrun[kk])
                ++kk;
            grp.push_back(k);
            grp.push_back(0);
            slots16 += (kk - k + 15) / 16 * 16;
            slots8 += (kk - k + 7) / 8 * 8;
            max_q = std::max<uint64_t>(max_q, ext[idx[k]].q_len);
            k     = kk;
        }
        grp.push_back(k1);
        grp.push_back(0);
        uint64_t const ngroups = grp.size() / 2 - 1;
        // (measured on the ragged list of bench.py: a slot of a run of 8 costs ~1.1 x one of a run of 16 while the query fits a
        // panel; wider queries run (8,19) panels with compact codes at 16 and (16,13) panels with int16 pairs at 8 -- the
        // padded columns and 0.0108 against 0.0156 ms per column, ckpt_cfg_for in lx_step_plan.cpp, decide)
        double const   cost16 = max_q > 208 ? (double)slots16 * (double)((max_q + 151) / 152 * 152) * 1.08 : (double)slots16 * 8.0;
        double const   cost8  = max_q > 208 ? (double)slots8 * (double)((max_q + 207) / 208 * 208) * 1.56 : (double)slots8 * 9.0;
        uint64_t const kRun   = cost8 < cost16 ? 8 : 16;
        uint64_t       slots  = 0;
        for (uint64_t g = 0; g <= ngroups; ++g)
        {
            grp[2 * g + 1] = slots;
            if (g < ngroups)
                slots += (grp[2 * g + 2] - grp[2 * g] + kRun - 1) / kRun * kRun;
        }
        pr.slots   = slots;
        pr.cap_sel = (slots + slots / kRun * 3 + 7) / 8 * 8 + 8;
        pr.slot_src.resize(slots);
        int rc2;
        if ((rc2 = ensure_pinned(h, ln.p_ext, slots * sizeof(lx_extension), kRoom)) || (rc2 = ensure_pinned(h, ln.p_min, slots * sizeof(int32_t), kRoom)))
            return rc2;
        lx_extension * const  slot_ext = static_cast<lx_extension *>(ln.p_ext.ptr);
        int32_t * const       slot_min = static_cast<int32_t *>(ln.p_min.ptr);
        uint32_t * const      slot_src = pr.slot_src.data();
        std::vector<uint64_t> tmax(nthreads, 1), tcells(nthreads, 0), tpad(nthreads, 0);
        // (what the wavefronts will execute: every block of kRun slots runs all columns of its panels for as many steps as
        // its longest window has rows)
        uint64_t const panel = max_q <= 104 ? 104 : max_q <= 152 ? 152 : max_q <= 200 ? 200 : max_q <= 208 ? 208 : 152, lanes = panel == 208 ? 16 : 8;
        parallel_ranges(ngroups, nthreads,
                        [&](unsigned t, uint64_t glo, uint64_t ghi)
                        {
                            uint64_t ms = 1, cells = 0, padded = 0; // (locals: the per-thread slots share cache lines)
                            for (uint64_t g = glo; g < ghi; ++g)
                            {
                                uint64_t const a = grp[2 * g], b = grp[2 * g + 2], o1 = grp[2 * g + 3];
                                uint64_t       o    = grp[2 * g + 1];
                                uint64_t const cols = (ext[idx[a]].q_len + panel - 1) / panel * panel;
                                for (uint64_t j0 = a; j0 < b; j0 += kRun)
                                {
                                    uint64_t bmax = 0;
                                    for (uint64_t j = j0; j < std::min(b, j0 + kRun); ++j)
                                    {
                                        bmax = std::max<uint64_t>(bmax, ext[idx[j]].s_len);
                                        cells += (uint64_t)ext[idx[j]].q_len * ext[idx[j]].s_len;
                                    }
                                    padded += kRun * cols * (bmax + lanes - 1);
                                }
                                for (uint64_t j = a; j < b; ++j, ++o)
                                {
                                    slot_ext[o] = ext[idx[j]];
                                    slot_src[o] = idx[j];
                                    slot_min[o] = min_score ? min_score[idx[j]] : min_score_all;
                                    ms          = std::max<uint64_t>(ms, ext[idx[j]].s_len);
                                }
                                lx_extension dummy = ext[idx[a]];
                                dummy.s_len        = 0;
                                for (; o < o1; ++o)
                                {
                                    slot_ext[o] = dummy;
                                    slot_src[o] = 0xffffffffu;
                                    slot_min[o] = 0x7fffffff; // never survives
                                }
                            }
                            tmax[t]   = std::max(tmax[t], ms);
                            tcells[t] = cells;
                            tpad[t]   = padded;
                        });
        for (uint64_t v : tmax)
            max_s = std::max(max_s, v);
        h->xb_stats[1] += slots;
        for (unsigned t = 0; t < nthreads; ++t)
        {
            h->xb_stats[2] += tcells[t];
            h->xb_stats[3] += tpad[t];
        }
        t_prep += ms(t0, now());
        return launch_chunk(L, slots, max_q, max_s, kRun);
    }

    // lane L's counts have arrived (the chunk is no longer in flight, whatever they say)
    int wait_counts(int L, uint64_t const *& cnt)
    {
        lx_handle::XbLane & ln = h->xb[L];
        in_flight[L]           = false;
        LX_HIP(h, hipEventSynchronize(ln.ev_cnt));
        cnt = static_cast<uint64_t const *>(ln.p_cnt.ptr);
        return LX_OK;
    }

    // the chunk's error word and survivor count; the share that survived steers the adaptive pass-2 mode of the next chunks (fused_impl)
    int check_counts(XbPrep const & pr, uint64_t const * cnt)
    {
        uint32_t flags[2];
        std::memcpy(flags, cnt + 3, sizeof(flags));
        if (int const rcf = error_for_flag(h, flags[1]))
            return rcf;
        if (cnt[0] > pr.cap_sel)
            return fail(h, LX_ESTATE, "survivor list longer than its capacity");
        if (pr.slots)
            h->surv_frac = (double)cnt[1] / (double)pr.slots;
        return LX_OK;
    }

    // the survivors' records, list positions, code lengths and codes into lane L's pinned staging (on the upload stream: stream2
    // already holds the next chunk's first-stage copies, which wait for its kernels)
    int download_survivors(int L, uint64_t count, uint64_t nrle)
    {
        lx_handle::XbLane & ln = h->xb[L];
        int                 rc2;
        if ((rc2 = ensure_pinned(h, ln.p_hsp, count * sizeof(lx_hsp) + 16, kRoom)) || (rc2 = ensure_pinned(h, ln.p_src, count * sizeof(uint32_t) + 16, kRoom)) ||
            (rc2 = ensure_pinned(h, ln.p_len, count * sizeof(uint32_t) + 16, kRoom)) || (rc2 = ensure_pinned(h, ln.p_rle, nrle + 16, kRoom)))
            return rc2;
        if (count)
        {
            LX_HIP(h, hipMemcpyAsync(ln.p_hsp.ptr, ln.d_hsp.ptr, count * sizeof(lx_hsp), hipMemcpyDeviceToHost, h->stream3));
            LX_HIP(h, hipMemcpyAsync(ln.p_src.ptr, ln.d_src.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream3));
            LX_HIP(h, hipMemcpyAsync(ln.p_len.ptr, ln.d_len.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream3));
            if (nrle)
                LX_HIP(h, hipMemcpyAsync(ln.p_rle.ptr, ln.d_rle.ptr, nrle, hipMemcpyDeviceToHost, h->stream3));
        }
        LX_HIP(h, hipStreamSynchronize(h->stream3));
        return LX_OK;
    }

    // ---- results of the chunk in lane L -> the caller's arrays
    int collect(int L)
    {
        XbPrep &         pr = prep[L];
        auto const       t0 = now();
        uint64_t const * cnt;
        int              rc2;
        if ((rc2 = wait_counts(L, cnt)) || (rc2 = check_counts(pr, cnt)))
            return rc2;
        uint64_t const count = cnt[0], nrle = cnt[2];
        if ((rc2 = download_survivors(L, count, nrle)))
            return rc2;
        auto const t1 = now();
        t_wait += ms(t0, t1);
        Survivors const        sv(h->xb[L]);
        int32_t const * const  sc       = static_cast<int32_t const *>(h->xb[L].p_score.ptr);
        uint32_t const * const slot_src = pr.slot_src.data();
        if (as_list)
        {
            parallel_ranges(pr.slots, nthreads,
                            [&](unsigned, uint64_t lo, uint64_t hi)
                            {
                                for (uint64_t o = lo; o < hi; ++o)
                                    if (slot_src[o] != 0xffffffffu)
                                        out_score[slot_src[o]] = sc[o];
                            });
            rc2 = append_list(L, count, nrle, slot_src);
            t_unpack += ms(t1, now());
            return rc2;
        }
        // which list position a slot has; where the survivors' ops go
        std::vector<uint32_t> & slot_pos = h->xb_pos;
        slot_pos.resize(pr.slots);
        parallel_ranges(pr.slots, nthreads, [&](unsigned, uint64_t lo, uint64_t hi) { std::fill(slot_pos.begin() + lo, slot_pos.begin() + hi, 0xffffffffu); });
        if ((rc2 = survivor_offsets(sv, count, slot_pos.data(), t1)))
            return rc2;
        // one pass over the chunk's slots: score and record of every extension, the survivors' ops
        std::vector<uint64_t> untraced(nthreads, ~0ull);
        parallel_ranges(pr.slots, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            for (uint64_t o = lo; o < hi; ++o)
                            {
                                uint32_t const orig = slot_src[o];
                                if (orig == 0xffffffffu)
                                    continue;
                                out_score[orig]  = sc[o];
                                uint32_t const e = slot_pos[o];
                                if (e == 0xffffffffu)
                                {
                                    lx_hsp r{};
                                    r.score           = sc[o];
                                    out_hsp[orig]     = r;
                                    out_ops_off[orig] = 0;
                                }
                                else if (!write_row(sv, e, orig))
                                    untraced[t] = std::min<uint64_t>(untraced[t], orig);
                            }
                        });
        return rows_written(untraced, count, t1);
    }

    // Where the survivors' ops go in h->ext_bytes (column bytes or codes; none for padding and score 0): h->xb_off[e] from ops_total
    // on, [count] = the end -- lengths, a prefix over the threads' shares, one inside each share; slot_pos: each slot's list position
    int survivor_offsets(Survivors const & sv, uint64_t count, uint32_t * slot_pos, Clock::time_point t1)
    {
        std::vector<uint64_t> & pos_off = h->xb_off;
        pos_off.resize(count + 1);
        std::vector<uint64_t> part(nthreads + 1, 0);
        parallel_ranges(count, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint64_t sum = 0;
                            for (uint64_t e = lo; e < hi; ++e)
                            {
                                uint64_t len = 0;
                                if (sv.src[e] != 0xffffffffu)
                                {
                                    if (slot_pos)
                                        slot_pos[sv.src[e]] = (uint32_t)e;
                                    if (sv.hs[e].score > 0)
                                        len = want_rle ? (uint64_t)sv.code_len[e] : (uint64_t)sv.hs[e].n_ops;
                                }
                                pos_off[e] = len;
                                sum += len;
                            }
                            part[t + 1] = sum;
                        });
        auto const tu1 = now();
        t_u1 += ms(t1, tu1);
        part[0] = ops_total;
        for (unsigned t = 0; t < nthreads; ++t)
            part[t + 1] += part[t];
        uint64_t const total = part[nthreads];
        parallel_ranges(count, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint64_t at = part[t];
                            for (uint64_t e = lo; e < hi; ++e)
                            {
                                uint64_t const len = pos_off[e];
                                pos_off[e]         = at;
                                at += len;
                            }
                        });
        pos_off[count] = total;
        if (!h->ext_bytes.grow(total + 16))
            return fail(h, LX_ENOMEM, "out of host memory for %llu bytes of alignment ops", (unsigned long long)(total + 16));
        t_u2 += ms(tu1, now());
        return LX_OK;
    }

    // survivor e -> row `orig` of the caller's arrays, its ops at h->xb_off[e]; false: its backtrace gave up
    bool write_row(Survivors const & sv, uint64_t e, uint32_t orig) const
    {
        uint64_t const * const pos_off = h->xb_off.data();
        lx_hsp                 r       = sv.hs[e];
        if (r.score < 0)
            return false;
        uint8_t const * const cd  = sv.codes + (uint32_t)r.ops_shift;
        uint8_t * const       dst = h->ext_bytes.data() + pos_off[e];
        if (r.score > 0 && want_rle)
            std::memcpy(dst, cd, (size_t)(pos_off[e + 1] - pos_off[e]));
        else if (r.score > 0)
            rle_expand(cd, r.n_ops, dst);
        r.ops_shift       = 0;
        out_hsp[orig]     = r;
        out_ops_off[orig] = pos_off[e];
        return true;
    }

    // the end of a chunk's unpacking: the first survivor whose backtrace gave up, else the ops handed out so far
    int rows_written(std::vector<uint64_t> const & untraced, uint64_t count, Clock::time_point t1)
    {
        for (uint64_t u : untraced)
            if (u != ~0ull)
                return fail(h, LX_EOVERFLOW, "extension %llu could not be traced", (unsigned long long)u);
        ops_total = h->xb_off[count];
        t_unpack += ms(t1, now());
        return LX_OK;
    }

    // ---- the multi-query pipeline.  Chunks = ranges of the plan's wavefronts, about chunk_target slots.  A chunk may span panel counts
    // (its slots are sized for its widest query, its narrower queries run the multi-panel kernel over one panel): a chunk boundary
    // wherever the panel count changes was measured on the ragged list of bench.py and costs more than it saves -- 3 chunks 20.8 ms,
    // 2 chunks 18.9 ms: every chunk pays the fixed cost of a backtrace launch (~0.5-1 ms), the single-panel kernel saves a tenth of a
    // 0.8 ms sweep
    int run_mq()
    {
        int rc;
        per_chunk      = std::max<uint64_t>(1, chunk_target / kWave);
        h->xb_stats[2] = p.mq_cells;
        if (!list_uploaded && (rc = upload_list()))
            return rc;
        t_prep += t_upload;
        if (as_list && ri && ri->keep_on_device && (rc = keep_on_device()))
            return rc;
        stream_planned = p.use_solo || preplanned; // (the solo plan and a device plan are whole before the first chunk)
        // ONE launch for the pool and what follows it: the pool is a tenth of the list in wavefronts that run up to three times as long
        // as the others -- launched by itself it leaves most of the chip idle behind its longest windows (ragged list of bench.py: 5 000
        // of 37 000 wavefronts, but 5.9 of 11.8 ms), launched with the rest behind it the short wavefronts fill in.  The plan of the
        // streamed part is then made before the first launch.  (lists of up to ~200 000 windows: a dozen rounds of the chip's wavefront
        // slots.  Beyond that the pool by itself is several rounds and the streamed part's plan is better made beside its kernels:
        // 596 k windows 18.6 ms merged, 17.5 ms not; 64 k windows of 300-500-residue queries 11.9 ms merged, 16.3 ms not)
        merge_pool = !p.use_solo && !preplanned && p.live <= (lx::dev_aids().mq_merge_below ? lx::dev_aids().mq_merge_below : 200000);
        if (merge_pool && !stream_planned)
        {
            auto const tp0 = now();
            h->plan.plan_stream();
            stream_planned = true;
            h->plan.longest_first(0, p.nwf); // (one launch for the whole plan: the streamed part's long wavefronts would start late)
            t_prep += ms(tp0, now());
        }
        uint64_t w0 = 0;
        if (!p.use_solo && !merge_pool && !stream_planned && !by_range && p.pool_wf > 0 && (rc = two_calls(w0)))
            return rc;
        if ((rc = mq_chunks(w0)) || (rc = drain(true)) || (rc = run_redo()) || dev_list)
            return rc;
        // the scores of every extension, in caller order (a device list's scores stay on the device: h->d_score_all)
        auto const ts0 = now();
        LX_HIP(h, hipMemcpyAsync(h->p_score_all.ptr, h->d_score_all.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        LX_HIP(h, hipStreamSynchronize(h->stream));
        int32_t const * const sa = static_cast<int32_t const *>(h->p_score_all.ptr);
        parallel_ranges(n, nthreads,
                        [&](unsigned, uint64_t lo, uint64_t hi)
                        {
                            for (uint64_t i = lo; i < hi; ++i)
                            {
                                out_score[i] = sa[i];
                                if (!as_list && out_hsp[i].n_ops == 0)
                                    out_hsp[i].score = sa[i];
                            }
                        });
        t_unpack += ms(ts0, now());
        return LX_OK;
    }

    // the Level-2 driver makes its records on the device (lx_records.hip): room for every chunk's survivor list, padding included
    int keep_on_device()
    {
        auto & l2 = h->l2;
        // (fillers never survive, a chunk's list is padded by less than 16 entries: the list's windows + a margin per chunk -- not the
        // plan's slots: the streamed part of a host plan is made later)
        uint64_t const cap = n + n / 64 + 8192;
        int            rc;
        if ((rc = ensure(h, l2.d_surv_hsp, cap * sizeof(lx_hsp))) || (rc = ensure(h, l2.d_surv_src, cap * sizeof(uint32_t))) ||
            (rc = ensure(h, l2.d_surv_codes, cap * sizeof(uint64_t))))
            return rc;
        l2.surv_cap   = cap;
        l2.surv_total = 0;
        dev_list      = true;
        want_codes    = ri->want_codes;
        // records chunk by chunk where every range of the plan is a chunk the budgets admit (else: the call's list, one chain at the end)
        if (ri->chunk_records && ri->chunk_records->n_ranges >= 1 && preplanned)
        {
            auto const & cr = *ri->chunk_records;
            by_range        = cr.cut_wf[0] == 0 && cr.cut_wf[cr.n_ranges] == p.nwf;
            for (uint64_t r = 0; r < cr.n_ranges && by_range; ++r)
            {
                uint64_t const a = cr.cut_wf[r], b = cr.cut_wf[r + 1];
                uint64_t       pm = 1, sm = 1;
                for (uint64_t w = a; w < b; ++w)
                {
                    pm = std::max<uint64_t>(pm, p.wf_pan[w]);
                    sm = std::max<uint64_t>(sm, p.wf_maxs[w]);
                }
                uint64_t const slot_b = slot_dwords(p.mq_cfg, pm, sm, false, true) * 4;
                // (a range whose sweep overflows runs again WHOLE with int16-pair slots, about twice the codes': admitted against those too)
                uint64_t const slot_w = wide_ok() ? slot_dwords(p.mq_cfg, pm, sm, true) * 4 : 0;
                by_range = a < b && b - a <= 4 * per_chunk && (b - a) * kWave * std::max(slot_b, slot_w) <= h->opt_trace_bytes &&
                           (b - a) * kWave * (pm * 8 + sm) <= (8ull << 30);
            }
        }
        return LX_OK;
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
            dw0_est += wf_dwords(w, mw);
        }
        uint64_t const cap_slots = p.pool_wf * kWave + nstream + 5 * nstream_runs + kWave * (nthreads + 2);
        uint64_t const rest_dw   = dw1_est + dw1_est / 4 + (1u << 20); // (wavefronts share the largest of up to four runs' sizes)
        t_prep += ms(tp0, now());
        // (the budgets of a chunk: its checkpoint slots, its survivors' ops slots)
        if (!(nstream != 0 && cap_slots < (1ull << 31) && (cap_slots + 16) * (cap_pan * 8 + cap_s + 4) <= (8ull << 30) && dw0_est * 4 <= h->opt_trace_bytes / 2))
            return LX_OK;
        int rc;
        if ((rc = enqueue_mq_first(0, p.pool_wf, cap_slots, cap_pan, cap_s, rest_dw)))
            return rc;
        auto const tp1 = now();
        h->plan.plan_stream();
        stream_planned = true;
        h->plan.longest_first(p.pool_wf, p.nwf); // (the second launch's wavefronts)
        // the wavefronts of the streamed part that fit behind the pool's (all of them, unless the estimate was short)
        uint64_t w_end = p.pool_wf, dw1 = 0;
        while (w_end < p.nwf && two.n1 + (w_end + 1 - p.pool_wf) * kWave <= two.cap_slots && p.wf_pan[w_end] <= cap_pan && p.wf_maxs[w_end] <= cap_s &&
               two.dw0 + two.ovf_dw + dw1 + wf_dwords(w_end, prep[0].wide) <= two.total_dw)
            dw1 += wf_dwords(w_end++, prep[0].wide);
        t_prep += ms(tp1, now());
        if (hm.on)
            fprintf(stderr, "[lx host ms]   one chunk in two calls: pool %llu wavefronts, then %llu of %llu (slots: %llu of at most %llu; dwords %llu + %llu + %llu of %llu)\n",
                    (unsigned long long)p.pool_wf, (unsigned long long)(w_end - p.pool_wf), (unsigned long long)(p.nwf - p.pool_wf), (unsigned long long)(w_end * kWave),
                    (unsigned long long)two.cap_slots, (unsigned long long)two.dw0, (unsigned long long)two.ovf_dw, (unsigned long long)dw1, (unsigned long long)two.total_dw);
        if ((rc = enqueue_mq_second(0, p.pool_wf, w_end)))
            return rc;
        if (!as_list)
            clear_rows();
        w0 = w_end;
        c  = 1;
        return LX_OK;
    }

    int mq_chunks(uint64_t w0)
    {
        int rc;
        for (;;)
        {
            if (w0 >= p.nwf)
            {
                // the pool's wavefronts are queued (or there are none): the streamed part of the plan is made now, beside their kernels
                if (stream_planned)
                    return LX_OK;
                auto const tp0 = now();
                h->plan.plan_stream();
                h->plan.longest_first(w0, p.nwf);
                stream_planned = true;
                t_prep += ms(tp0, now());
                continue;
            }
            // The chunk's checkpoint slots must fit the trace budget (fused_impl leaves the sweep otherwise): every slot is sized for the
            // chunk's widest query and longest window -- compact codes, int16 pairs where the chunk may run WIDE -- plus room for the int32
            // overflow slots of what the sweep may decline; the chunk ends where one more wavefront would break the budget, or where the
            // pool ends.  A chunk whose records are made by range is its range (the budgets were checked when the mode was chosen).
            uint64_t       w1 = w0, range_now = 0, run_bytes = 0, run_q = 1, run_s = 1;
            bool const     mw       = maybe_wide();
            uint64_t const pool_end = (p.use_solo || preplanned) ? 0 : p.pool_wf;
            if (by_range)
            {
                while (ri->chunk_records->cut_wf[range_now + 1] <= w0)
                    ++range_now;
                w1 = ri->chunk_records->cut_wf[range_now + 1];
            }
            while (!by_range && w1 < p.nwf && w1 - w0 < per_chunk)
            {
                if (!merge_pool && w0 < pool_end && w1 == pool_end)
                    break;
                uint64_t const b2 = run_bytes + kWave * slot_dwords(p.mq_cfg, p.wf_pan[w1], p.wf_maxs[w1], mw, true) * 4;
                uint64_t const q2 = std::max<uint64_t>(run_q, p.wf_pan[w1]), s2 = std::max<uint64_t>(run_s, p.wf_maxs[w1]);
                if (w1 > w0 && (b2 > h->opt_trace_bytes || (w1 + 1 - w0) * kWave * (q2 * 8 + s2) > (8ull << 30)))
                    break;
                run_bytes = b2, run_q = q2, run_s = s2;
                ++w1;
            }
            int const L = c & 1;
            if (in_flight[L] && (rc = collect_mq(L)))
                return rc;
            prep[L].range = range_now;
            if ((rc = enqueue_mq(L, w0, w1)))
                return rc;
            if (!rows_cleared && !as_list)
                clear_rows();
            if (in_flight[L ^ 1] && (rc = collect_mq(L ^ 1)))
                return rc;
            w0 = w1;
            ++c;
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
            if (by_range) // (the range the chunk is: its records are made again behind the second sweep, and wait where the later ranges' stand)
                for (uint64_t k = 0; k < ri->chunk_records->n_ranges; ++k)
                    if (ri->chunk_records->cut_wf[k] == r.first)
                        prep[0].range = k;
            // (int16-pair slots are twice the codes': the range is run again in pieces that fit the slot budget -- a range whose records
            // are made chunk by chunk stays whole)
            for (uint64_t a = r.first; a < r.second;)
            {
                uint64_t b = a, bytes = 0;
                while (b < r.second)
                {
                    uint64_t const wb = wf_dwords(b, true) * 4;
                    if (!by_range && b > a && bytes + wb > h->opt_trace_bytes)
                        break;
                    bytes += wb;
                    ++b;
                }
                if ((rc = enqueue_mq(0, a, b, true)) || (rc = collect_mq(0)))
                    return rc;
                ++c;
                a = b;
            }
        }
        return LX_OK;
    }

    // (beside the first chunk's kernels) every row starts as "no alignment"; the survivors' rows are written by collect_mq, the scores
    // of all rows at the end of the call
    void clear_rows()
    {
        auto const tz0 = now();
        parallel_ranges(n, nthreads,
                        [&](unsigned, uint64_t lo, uint64_t hi)
                        {
                            std::memset(static_cast<void *>(out_hsp + lo), 0, (hi - lo) * sizeof(lx_hsp));
                            std::memset(out_ops_off + lo, 0, (hi - lo) * sizeof(uint64_t));
                        });
        rows_cleared = true;
        t_unpack += ms(tz0, now());
    }

    // the table of wavefronts [wlo, whi) (lx::WfSlots): every wavefront's sixteen slots laid out for ITS longest window and widest
    // query, offsets from 0; returns the dwords they take
    uint64_t fill_table(lx::WfSlots * tab, uint64_t wlo, uint64_t whi, bool wide) const
    {
        uint64_t const pc  = (uint64_t)lx::trace_cfg_panel(p.mq_cfg) / 8;
        uint64_t       off = 0, per_panel = 0;
        uint32_t       last_steps = 0; // (a sorted plan repeats its step counts: the slot size is asked for once per run of them)
        for (uint64_t w = wlo; w < whi; ++w)
        {
            uint32_t const steps  = mq_steps(p.wf_maxs[w]);
            uint32_t const panels = (uint32_t)std::max<uint64_t>(1, ((uint64_t)p.wf_pan[w] + pc - 1) / pc);
            if (steps != last_steps)
            {
                per_panel  = slot_dwords(p.mq_cfg, 1, p.wf_maxs[w], wide);
                last_steps = steps;
            }
            tab[w - wlo] = lx::WfSlots{off, steps, panels};
            off += kWave * (uint64_t)panels * per_panel;
        }
        return off;
    }

    // what wavefronts [wlo, whi) add to the chunk's and the call's statistics
    void chunk_stats(XbPrep & pr, uint64_t wlo, uint64_t whi)
    {
        uint64_t padded = 0;
        for (uint64_t w = wlo; w < whi; ++w)
            padded += kWave * ((uint64_t)p.wf_pan[w] * 8) * ((uint64_t)p.wf_maxs[w] + 7);
        pr.exec_cells += padded;
        h->xb_stats[3] += padded;
        h->xb_stats[1] += (whi - wlo) * kWave;
    }

    // the slot records and cut-offs of `slots` slots, gathered from the device copy of the caller's list into lane L at slot `at`
    hipError_t gather(uint32_t const * d_orig, uint64_t slots, int L, uint64_t at)
    {
        lx_handle::XbLane & ln = h->xb[L];
        return lx::launch_slot_gather(static_cast<lx::Extension const *>(ri ? ri->d_ext_all : h->d_ext_all.ptr),
                                      (min_score || (ri && ri->d_min_all)) ? static_cast<int32_t const *>(ri ? ri->d_min_all : h->d_min_all.ptr) : nullptr,
                                      min_score_all, d_orig, slots, static_cast<lx::Extension *>(ln.d_ext.ptr) + at, static_cast<int32_t *>(ln.d_min.ptr) + at,
                                      h->stream);
    }

    // ---- wavefronts w0 .. w1 of the plan -> the slots' caller indices in lane L's pinned staging -> upload, gather of the slot
    // records on the device, kernels, scatter of the scores into caller order.  The plan's order is a permutation of the caller's
    // list (+ fillers): the host only touches 4 bytes per slot here (the 24-byte records and their cut-offs are gathered from the
    // device copy of the list at HBM speed, not by cache misses of a few host threads).
    int enqueue_mq(int L, uint64_t w0, uint64_t w1, bool force_wide = false)
    {
        auto const          t0 = now();
        lx_handle::XbLane & ln = h->xb[L];
        XbPrep &            pr = prep[L];
        pr.k0                  = w0;
        pr.k1                  = w1;
        uint64_t const slots   = (w1 - w0) * kWave;
        pr.slots               = slots;
        pr.cap_sel             = (slots + 7) / 8 * 8 + 8;
        int rc2;
        if (!preplanned && (rc2 = ensure_pinned(h, ln.p_orig, slots * sizeof(uint32_t), kRoom)))
            return rc2;
        uint32_t * const      slot_orig = static_cast<uint32_t *>(ln.p_orig.ptr);
        uint64_t const        panel     = (uint64_t)lx::trace_cfg_panel(p.mq_cfg);
        std::vector<uint64_t> tpad(nthreads, 0), tmaxs(nthreads, 1), tpan(nthreads, 1);
        // (what the wavefronts execute: every one sweeps as many panels as its widest query needs, each for as many steps as its
        // longest window has rows)
        parallel_ranges(w1 - w0, nthreads,
                        [&](unsigned t, uint64_t wlo, uint64_t whi)
                        {
                            uint64_t padded = 0, smax = 1, pmax = 1; // (locals: the per-thread slots share cache lines)
                            if (!preplanned)
                                std::memcpy(slot_orig + wlo * kWave, p.plan_slot.data() + (w0 + wlo) * kWave, (whi - wlo) * kWave * sizeof(uint32_t));
                            for (uint64_t w = w0 + wlo; w < w0 + whi; ++w)
                            {
                                padded += kWave * ((uint64_t)p.wf_pan[w] * 8) * ((uint64_t)p.wf_maxs[w] + 7);
                                smax = std::max<uint64_t>(smax, p.wf_maxs[w]);
                                pmax = std::max<uint64_t>(pmax, p.wf_pan[w]);
                            }
                            tpad[t]  = padded;
                            tmaxs[t] = smax;
                            tpan[t]  = pmax;
                        });
        // the promises of the chunk: its widest query (as a panel count) and its longest window
        uint64_t max_s = 1, max_pan = 1;
        pr.exec_cells  = 0;
        for (unsigned t = 0; t < nthreads; ++t)
        {
            pr.exec_cells += tpad[t];
            h->xb_stats[3] += tpad[t];
            max_s   = std::max(max_s, tmaxs[t]);
            max_pan = std::max(max_pan, tpan[t]);
        }
        h->xb_stats[1] += slots;
        pr.max_s             = max_s;
        pr.max_pan           = max_pan;
        uint64_t const max_q = (max_pan + panel / 8 - 1) / (panel / 8) * panel; // (whole panels: the slots have one part per panel)
        t_prep += ms(t0, now());

        auto const     t1     = now();
        uint64_t const stride = (max_q + max_s + 3) & ~3ull;
        if ((rc2 = size_lane(L, slots, stride, !preplanned, true)))
            return rc2;
        // (a device plan: the chunk's slots are a piece of it)
        uint32_t const * const d_orig = preplanned ? ri->d_plan + w0 * kWave : static_cast<uint32_t const *>(ln.d_orig.ptr);
        if (!preplanned)
        {
            LX_HIP(h, hipMemcpyAsync(ln.d_orig.ptr, slot_orig, slots * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream3));
            LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
            LX_HIP(h, hipStreamWaitEvent(h->stream, ln.ev_up, 0));
        }
        LX_HIP(h, gather(d_orig, slots, L, 0));
        // Compact codes hold scores up to 2046; a window beyond them is redone by the int32 launch, one profile per pair, at a tenth
        // of the sweep's speed.  Where the last chunks had more than a few such windows (long queries with strong hits: a 600-residue
        // query against its homologue scores ~3 000) the sweep writes int16 pairs itself (lx_sweep_mq.hip: WIDE) -- twice the
        // checkpoint bytes, no second launch; it goes back to the codes when fewer than 1 % of a chunk's windows need more.
        // (force_wide: a chunk that runs again because its overflow area filled up -- said by the caller, not inferred from the fraction
        // the OTHER lane's collect may have overwritten meanwhile)
        mq_wide = wide_ok() && (force_wide || (mq_wide ? h->mq_decl_frac > 0.01 : h->mq_decl_frac > 0.03));
        pr.wide = mq_wide;
        // the chunk's slots by wavefront (lx::WfSlots)
        uint64_t const nw = w1 - w0;
        if ((rc2 = ensure_pinned(h, ln.p_wft, nw * sizeof(lx::WfSlots), kRoom)) || (rc2 = ensure(h, ln.d_wft, nw * sizeof(lx::WfSlots))))
            return rc2;
        lx::WfSlots * const tab = static_cast<lx::WfSlots *>(ln.p_wft.ptr);
        uint64_t const      off = fill_table(tab, w0, w1, pr.wide);
        LX_HIP(h, hipMemcpyAsync(ln.d_wft.ptr, tab, nw * sizeof(lx::WfSlots), hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
        LX_HIP(h, hipStreamWaitEvent(h->stream, ln.ev_up, 0));
        // (ovf_cap: what the chunk's budget reserved, an eighth of its slots)
        // (the solo packing: no run promise; the free packing: pairs of one query, at most four queries per wavefront)
        rc2 = run_fused(L, slots, stride, max_q, max_s, p.use_solo ? 1 : 2, MqTab{ln.d_wft.ptr, slots, off, 0, std::min<uint64_t>(slots, slots / 8 + 64), 0, 0});
        if (rc2 || (rc2 = finish_mq(L, d_orig, slots)))
            return rc2;
        t_issue += ms(t1, now());
        return LX_OK;
    }

    // behind a multi-query sweep: the scores into caller order, the chunk's error word and its windows beyond the compact codes, (by
    // range) the records kernels of the range behind the chunk's own (lx_level2_host.cpp), the counts on their way down
    int finish_mq(int L, uint32_t const * d_orig, uint64_t slots)
    {
        lx_handle::XbLane & ln    = h->xb[L];
        XbPrep &            pr    = prep[L];
        uint64_t * const    d_cnt = static_cast<uint64_t *>(ln.d_cnt.ptr);
        int                 rc2;
        LX_HIP(h, lx::launch_slot_scatter(d_orig, slots, static_cast<int32_t const *>(ln.d_score.ptr), static_cast<int32_t *>(h->d_score_all.ptr),
                                          static_cast<uint32_t *>(ln.d_src.ptr), d_cnt, pr.cap_sel, h->stream));
        LX_HIP(h, hipMemcpyAsync(d_cnt + 3, ws_word(h, kWsBump), 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
        LX_HIP(h, hipMemcpyAsync(d_cnt + 4, ws_word(h, kWsStatBeyond), sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
        if (by_range && (rc2 = ri->chunk_records->enqueue(pr.range, ln.d_hsp.ptr, ln.d_src.ptr, d_cnt, pr.cap_sel)))
            return rc2;
        LX_HIP(h, hipEventRecord(ln.ev_k, h->stream));
        LX_HIP(h, hipStreamWaitEvent(h->stream2, ln.ev_k, 0));
        LX_HIP(h, hipMemcpyAsync(ln.p_cnt.ptr, d_cnt, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream2));
        LX_HIP(h, hipEventRecord(ln.ev_cnt, h->stream2));
        in_flight[L] = true;
        return LX_OK;
    }

    // first call: wavefronts [0, w1) = the pool; cap_slots bounds the chunk's slots, (cap_pan, cap_s) its widest query and longest window,
    // rest_dw is what the second call's slots are expected to take
    int enqueue_mq_first(int L, uint64_t w1, uint64_t cap_slots, uint64_t cap_pan, uint64_t cap_s, uint64_t rest_dw)
    {
        auto const          t0    = now();
        lx_handle::XbLane & ln    = h->xb[L];
        XbPrep &            pr    = prep[L];
        uint64_t const      panel = (uint64_t)lx::trace_cfg_panel(p.mq_cfg), slots1 = w1 * kWave;
        pr.k0 = 0, pr.k1 = w1, pr.slots = slots1, pr.cap_sel = (cap_slots + 7) / 8 * 8 + 8, pr.exec_cells = 0, pr.max_s = cap_s, pr.max_pan = cap_pan;
        int rc2;
        if ((rc2 = ensure_pinned(h, ln.p_orig, cap_slots * sizeof(uint32_t), kRoom)) || (rc2 = ensure_pinned(h, ln.p_wft, (cap_slots / kWave + 1) * sizeof(lx::WfSlots), kRoom)))
            return rc2;
        uint32_t * const slot_orig = static_cast<uint32_t *>(ln.p_orig.ptr);
        std::memcpy(slot_orig, p.plan_slot.data(), slots1 * sizeof(uint32_t));
        chunk_stats(pr, 0, w1);
        two           = TwoCall{};
        two.max_q     = (cap_pan + panel / 8 - 1) / (panel / 8) * panel;
        two.max_s     = cap_s;
        two.stride    = (two.max_q + two.max_s + 3) & ~3ull;
        two.cap_slots = cap_slots;
        two.n1        = slots1;
        two.nw1       = w1;
        t_prep += ms(t0, now());
        auto const t1 = now();
        if ((rc2 = size_lane(L, cap_slots, two.stride, true, true)) || (rc2 = ensure(h, ln.d_wft, (cap_slots / kWave + 1) * sizeof(lx::WfSlots))))
            return rc2;
        mq_wide                 = wide_ok() && (mq_wide ? h->mq_decl_frac > 0.01 : h->mq_decl_frac > 0.03);
        pr.wide                 = mq_wide;
        lx::WfSlots * const tab = static_cast<lx::WfSlots *>(ln.p_wft.ptr);
        two.dw0                 = fill_table(tab, 0, w1, pr.wide);
        // (overflow slots have the size of the chunk's widest query and longest window: an eighth of the slots, within 16 GiB)
        uint64_t const s32 = slot_dwords(p.mq_cfg, cap_pan, two.max_s, true);
        two.ovf_cap        = std::min<uint64_t>(std::min<uint64_t>(cap_slots, cap_slots / 8 + 64), std::max<uint64_t>(1024, (4ull << 30) / std::max<uint64_t>(s32, 1)));
        two.ovf_dw         = two.ovf_cap * s32;
        // (reserved now: the pool's slots, the overflow slots, what the caller expects the second call's slots to take -- within the budget)
        two.total_dw = std::max<uint64_t>(two.dw0 + two.ovf_dw, std::min<uint64_t>(h->opt_trace_bytes / 4, two.dw0 + two.ovf_dw + rest_dw));
        LX_HIP(h, hipMemcpyAsync(ln.d_orig.ptr, slot_orig, slots1 * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipMemcpyAsync(ln.d_wft.ptr, tab, w1 * sizeof(lx::WfSlots), hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
        LX_HIP(h, hipStreamWaitEvent(h->stream, ln.ev_up, 0));
        LX_HIP(h, gather(static_cast<uint32_t const *>(ln.d_orig.ptr), slots1, L, 0));
        rc2 = run_fused(L, cap_slots, two.stride, two.max_q, two.max_s, 2, MqTab{ln.d_wft.ptr, slots1, two.dw0, 0, two.ovf_cap, two.total_dw, 1});
        t_issue += ms(t1, now());
        return rc2;
    }

    // second call: wavefronts [w_mid, w1) of the plan (none: the pool stays a chunk of its own) behind the first call's
    int enqueue_mq_second(int L, uint64_t w_mid, uint64_t w1)
    {
        auto const          t0     = now();
        lx_handle::XbLane & ln     = h->xb[L];
        XbPrep &            pr     = prep[L];
        uint64_t const      slots2 = (w1 - w_mid) * kWave, total = two.n1 + slots2;
        int                 rc2;
        uint32_t * const    slot_orig = static_cast<uint32_t *>(ln.p_orig.ptr);
        lx::WfSlots * const tab       = static_cast<lx::WfSlots *>(ln.p_wft.ptr) + two.nw1;
        if (slots2)
            std::memcpy(slot_orig + two.n1, p.plan_slot.data() + w_mid * kWave, slots2 * sizeof(uint32_t));
        chunk_stats(pr, w_mid, w1);
        uint64_t const dw1 = fill_table(tab, w_mid, w1, pr.wide);
        pr.k1              = w1;
        pr.slots           = total;
        t_prep += ms(t0, now());
        auto const t1 = now();
        if (slots2)
        {
            LX_HIP(h, hipMemcpyAsync(static_cast<uint32_t *>(ln.d_orig.ptr) + two.n1, slot_orig + two.n1, slots2 * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream3));
            LX_HIP(h, hipMemcpyAsync(static_cast<lx::WfSlots *>(ln.d_wft.ptr) + two.nw1, tab, (w1 - w_mid) * sizeof(lx::WfSlots), hipMemcpyHostToDevice, h->stream3));
            LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
            LX_HIP(h, hipStreamWaitEvent(h->stream, ln.ev_up, 0));
            LX_HIP(h, gather(static_cast<uint32_t const *>(ln.d_orig.ptr) + two.n1, slots2, L, two.n1));
        }
        mq_wide = pr.wide;
        rc2     = run_fused(L, total, two.stride, two.max_q, two.max_s, 2, MqTab{ln.d_wft.ptr, two.n1, two.dw0, dw1, two.ovf_cap, two.total_dw, 2});
        if (rc2 || (rc2 = finish_mq(L, static_cast<uint32_t const *>(ln.d_orig.ptr), total)))
            return rc2;
        t_issue += ms(t1, now());
        return LX_OK;
    }

    // ---- list form (lx_extend_batch_list): the chunk's survivors are appended to the handle's result buffers -- position in the
    // caller's list, record, where the codes begin -- and the chunk's codes to h->ext_bytes as one block; of the host's arrays
    // of size n only the scores are touched
    int append_list(int L, uint64_t count, uint64_t nrle, uint32_t const * slot_src /* NULL: the device translated */)
    {
        lx_handle::XbLane &    ln    = h->xb[L];
        lx_hsp const * const   hs    = static_cast<lx_hsp const *>(ln.p_hsp.ptr);
        uint32_t const * const src   = static_cast<uint32_t const *>(ln.p_src.ptr);
        uint8_t const * const  codes = static_cast<uint8_t const *>(ln.p_rle.ptr);
        std::vector<uint64_t>  part(nthreads + 1, 0), untraced(nthreads, ~0ull);
        parallel_ranges(count, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint64_t k = 0, bad = ~0ull; // (locals: the per-thread slots share cache lines)
                            for (uint64_t e = lo; e < hi; ++e)
                            {
                                if (src[e] == 0xffffffffu) // padding of the survivor list
                                    continue;
                                if (hs[e].score < 0)
                                    bad = std::min<uint64_t>(bad, slot_src ? slot_src[src[e]] : src[e]);
                                else
                                    ++k;
                            }
                            part[t + 1] = k;
                            untraced[t] = bad;
                        });
        for (uint64_t u : untraced)
            if (u != ~0ull)
                return fail(h, LX_EOVERFLOW, "extension %llu could not be traced", (unsigned long long)u);
        for (unsigned t = 0; t < nthreads; ++t)
            part[t + 1] += part[t];
        uint64_t const base = h->res_count, total = base + part[nthreads];
        if (!h->res_index.grow(total * sizeof(uint32_t) + 16) || !h->res_hsp.grow(total * sizeof(lx_hsp) + 16) ||
            !h->res_off.grow(total * sizeof(uint64_t) + 16) || !h->ext_bytes.grow(ops_total + nrle + 16))
            return fail(h, LX_ENOMEM, "out of host memory for %llu survivors", (unsigned long long)total);
        uint32_t * const res_index = reinterpret_cast<uint32_t *>(h->res_index.data());
        lx_hsp * const   res_hsp   = reinterpret_cast<lx_hsp *>(h->res_hsp.data());
        uint64_t * const res_off   = reinterpret_cast<uint64_t *>(h->res_off.data());
        uint8_t * const  dst       = h->ext_bytes.data() + ops_total;
        parallel_ranges(count, nthreads,
                        [&](unsigned t, uint64_t lo, uint64_t hi)
                        {
                            uint64_t k = base + part[t];
                            for (uint64_t e = lo; e < hi; ++e)
                            {
                                if (src[e] == 0xffffffffu)
                                    continue;
                                lx_hsp r     = hs[e];
                                res_index[k] = slot_src ? slot_src[src[e]] : src[e];
                                res_off[k]   = ops_total + (uint32_t)r.ops_shift;
                                r.ops_shift  = 0;
                                res_hsp[k]   = r;
                                ++k;
                            }
                        });
        parallel_ranges(nrle, nthreads, [&](unsigned, uint64_t lo, uint64_t hi) { std::memcpy(dst + lo, codes + lo, hi - lo); });
        h->res_count = total;
        ops_total += nrle;
        return LX_OK;
    }

    // ---- results of a multi-query chunk: the survivors' records and ops, addressed by caller index (the device translated the
    // list); the scores of every extension come back once, in caller order, at the end of the call
    int collect_mq(int L)
    {
        XbPrep &         pr = prep[L];
        auto const       t0 = now();
        uint64_t const * cnt;
        int              rc2;
        if ((rc2 = wait_counts(L, cnt)))
            return rc2;
        auto const     t_ev  = now();
        uint64_t const count = cnt[0], nrle = cnt[2];
        uint32_t       flags[2];
        std::memcpy(flags, cnt + 3, sizeof(flags));
        if (hm.on)
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
        if ((rc2 = check_counts(pr, cnt)))
            return rc2;
        if (pr.slots)
            h->mq_decl_frac = (double)(uint32_t)cnt[4] / (double)pr.slots;
        if (dev_list)
            return collect_on_device(L, count, nrle, t0, t_ev);
        if ((rc2 = download_survivors(L, count, nrle)))
            return rc2;
        auto const t1 = now();
        t_wait += ms(t0, t1);
        if (!as_list)
        {
            // the survivors -> their rows (cleared beside the first chunk; the scores come at the end of the call)
            Survivors const sv(h->xb[L]);
            if ((rc2 = survivor_offsets(sv, count, nullptr, t1)))
                return rc2;
            std::vector<uint64_t> untraced(nthreads, ~0ull);
            parallel_ranges(count, nthreads,
                            [&](unsigned t, uint64_t lo, uint64_t hi)
                            {
                                for (uint64_t e = lo; e < hi; ++e)
                                    if (sv.src[e] != 0xffffffffu && !write_row(sv, e, sv.src[e]))
                                        untraced[t] = std::min<uint64_t>(untraced[t], sv.src[e]);
                            });
            return rows_written(untraced, count, t1);
        }
        rc2 = append_list(L, count, nrle, nullptr);
        t_unpack += ms(t1, now());
        if (hm.on)
            fprintf(stderr, "[lx host ms]     ... its counts came after %.2f ms of waiting, its %llu records + %llu code bytes in %.2f more, appended in %.2f\n", ms(t0, t_ev),
                    (unsigned long long)count, (unsigned long long)nrle, ms(t_ev, t1), ms(t1, now()));
        return rc2;
    }

    // The survivors stay where the backtrace left them (lx_records.hip makes the result records from them): the chunk's list joins the
    // call's on the device -- a copy kernel in stream order, so that this lane's buffers are free for the chunk after next --, only the
    // run-length codes come down, into the call's code bytes.  By range, the range's rows and columns are collected instead.
    int collect_on_device(int L, uint64_t count, uint64_t nrle, Clock::time_point t0, Clock::time_point t_ev)
    {
        lx_handle::XbLane & ln        = h->xb[L];
        auto &              l2        = h->l2;
        uint64_t const      code_base = ops_total;
        if (!by_range)
        {
            if (l2.surv_total + count > l2.surv_cap)
                return fail(h, LX_ESTATE, "the call's survivor list is longer than its capacity");
            LX_HIP(h, lx::rec_launch_append(static_cast<lx::Hsp const *>(ln.d_hsp.ptr), static_cast<uint32_t const *>(ln.d_src.ptr),
                                            static_cast<uint64_t const *>(ln.d_cnt.ptr), count, ops_total, static_cast<lx::Hsp *>(l2.d_surv_hsp.ptr) + l2.surv_total,
                                            static_cast<uint32_t *>(l2.d_surv_src.ptr) + l2.surv_total, static_cast<uint64_t *>(l2.d_surv_codes.ptr) + l2.surv_total,
                                            h->stream));
        }
        l2.surv_total += count;
        if (nrle && want_codes)
        {
            if (!h->ext_bytes.grow(ops_total + nrle + 16))
                return fail(h, LX_ENOMEM, "out of host memory for %llu bytes of alignment codes", (unsigned long long)(ops_total + nrle));
            // (straight into the call's code bytes: a copy of this size into ordinary memory runs at the link's rate)
            LX_HIP(h, hipMemcpyAsync(h->ext_bytes.data() + ops_total, ln.d_rle.ptr, nrle, hipMemcpyDeviceToHost, h->stream3));
            LX_HIP(h, hipStreamSynchronize(h->stream3));
        }
        ops_total += nrle;
        h->res_count  = l2.surv_total;
        auto const t1 = now();
        t_wait += ms(t0, t1);
        if (!by_range)
        {
            if (hm.on)
                fprintf(stderr, "[lx host ms]     ... its counts came after %.2f ms of waiting, its %llu code bytes in %.2f more; the %llu records stay on the device\n",
                        ms(t0, t_ev), (unsigned long long)nrle, ms(t_ev, t1), (unsigned long long)count);
            return LX_OK;
        }
        int const rc2 = ri->chunk_records->collect(prep[L].range, code_base, in_flight[L ^ 1]);
        t_unpack += ms(t1, now());
        if (hm.on)
            fprintf(stderr, "[lx host ms]     ... its counts came after %.2f ms of waiting, its %llu code bytes in %.2f more; rows and columns of range %llu in %.2f\n",
                    ms(t0, t_ev), (unsigned long long)nrle, ms(t_ev, t1), (unsigned long long)prep[L].range, ms(t1, now()));
        return rc2;
    }
};

} // namespace

// Both passes on host buffers: validate and plan (lx_host_plan.cpp), then the pipeline of chunks.
// ri (lx_level2_host.cpp): the query residues and the caller's list + cut-offs stand on the device already (q_res is NULL, q_bytes the
// resident size; `ext` / `min_score` are the host's copies of the same list, for the plan)
// mode 0: column bytes, 1: run-length codes, 2: the survivors as a list in the handle's buffers (out_hsp, out_ops_off, out_ops,
// out_ops_bytes are NULL; lx_extend_batch_list hands the buffers out)
static int extend_pipeline(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                           lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                           lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes, int mode,
                           lxi::ResidentInput const * ri = nullptr, lxi::ResidentSurvivors * where = nullptr)
{
    bool const                 as_list = mode == 2;
    HostPool::Call const       in_flight_call; // (the host threads look for this call's next loop instead of going to sleep between two)
    h->res_count = 0;
    if (where)
        *where = lxi::ResidentSurvivors{};
    int rc = bind(h);
    if (rc)
        return rc;
    SubjectRef sref;
    if ((rc = resolve_subjects(h, s_res, s_bytes, sref)))
        return rc;
    s_bytes = sref.bytes;
    HostMarks hm(as_list ? "lx_extend_batch_list" : mode == 1 ? "lx_extend_batch_rle" : "lx_extend_batch");

    // a plan that was made on the device (lx_level2_host.cpp: the solo packing of a resident window list -- a sort by width and
    // length, 16 windows to a wavefront)
    bool const preplanned = ri && ri->d_plan;
    HostPlan & plan       = h->plan;
    if ((rc = plan.order(h, ext, n, q_bytes, s_bytes, as_list, preplanned, out_score, out_hsp, out_ops_off, hm)) || plan.live == 0)
        return rc;
    if ((rc = plan.choose(h, slot, ri, as_list)))
        return rc;
    ExtendPipeline pipe(h, slot, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off, out_ops, out_ops_bytes, mode, ri, hm);
    // the caller's list onto the device as soon as the multi-query path is known to be taken: the copy runs beside the planning of the pool
    if (plan.use_mq && !preplanned && (rc = pipe.upload_list()))
        return rc;
    plan.sort(hm);
    plan.plan_pool(ri, hm);

    // ---- the phase list collects every chunk's events; the streams are drained on every exit, before anything is torn down
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    struct Guard
    {
        lx_handle * h;
        ~Guard()
        {
            (void)hipStreamSynchronize(h->stream);
            (void)hipStreamSynchronize(h->stream2);
            (void)hipStreamSynchronize(h->stream3);
        }
    } const guard{h};

    if (!ri)
    {
        if ((rc = ensure(h, h->d_q, q_bytes + kSlack)))
            return rc;
        if (q_bytes)
            LX_HIP(h, hipMemcpyAsync(h->d_q.ptr, q_res, q_bytes, hipMemcpyHostToDevice, h->stream));
    }
    if (sref.upload)
        LX_HIP(h, hipMemcpyAsync(sref.dev, s_res, s_bytes, hipMemcpyHostToDevice, h->stream));
    // (measured in round 3 and removed again: two chunks' kernels side by side on two streams -- ragged list 28.5 against 24.4 ms,
    // headline batch 40.0 against 31.3 ms -- and a chunk's backtrace on a second stream beside the next chunk's sweep -- no gain on
    // the ragged list, 34.9 against 29.0 ms on the headline: kernels side by side cost more than their tails and latencies save)
    rc = pipe.run(ri ? ri->d_q : h->d_q.ptr, sref.dev);
    if (where && pipe.survivors_where() != lxi::ResidentSurvivors::kOnHost)
        *where = lxi::ResidentSurvivors{pipe.survivors_where(), h->l2.surv_total};
    return rc;
}

// the handle's survivor list of the last call, handed out
static void hand_out_list(lx_handle * h, lx_survivor_list * out)
{
    *out = lx_survivor_list{h->res_count, reinterpret_cast<uint32_t const *>(h->res_index.data()), reinterpret_cast<lx_hsp const *>(h->res_hsp.data()),
                            reinterpret_cast<uint64_t const *>(h->res_off.data()), h->ext_bytes.data(), h->res_count ? h->xb_ops_total : 0};
}

// the three entry points (mode as extend_pipeline's; `out` is the list form's): their argument checks, band mode, the list handed out
static int extend_entry(char const * what, lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                        lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score, lx_hsp * out_hsp,
                        uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes, lx_survivor_list * out, int mode)
{
    if (!h)
        return LX_EINVAL;
    if (slot < 0 || slot > 1 || !h->have_sc[slot])
        return fail(h, LX_ESTATE, "scoring slot %d not set", slot);
    if (out_ops)
        *out_ops = nullptr;
    if (out_ops_bytes)
        *out_ops_bytes = 0;
    if (out)
        *out = lx_survivor_list{};
    if (n == 0)
        return LX_OK;
    bool const outs_ok = mode == 2 ? out != nullptr : (out_hsp && out_ops_off && out_ops && out_ops_bytes);
    if (!ext || !out_score || !outs_ok || (!q_res && q_bytes))
        return fail(h, LX_EINVAL, "NULL argument");
    if (n > 0xfffffff0ull / 2)
        return fail(h, LX_EINVAL, "at most 2^31 extensions per call");
    if (h->opt_band && mode == 0)
        return host_banded(h, slot, 2, q_res, q_bytes, s_res, s_bytes, ext, n, nullptr, min_score, min_score_all, out_score, out_hsp, nullptr,
                           nullptr, out_ops_off, out_ops, out_ops_bytes);
    if (h->opt_band)
        return fail(h, LX_EINVAL, "%s: band mode returns column bytes only (lx_extend_batch)", what);
    int const rc = extend_pipeline(h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off, out_ops,
                                   out_ops_bytes, mode);
    if (rc == LX_OK && mode == 2)
        hand_out_list(h, out);
    return rc;
}

extern "C" {

int lx_extend_batch(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                    lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                    lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes)
{
    return extend_entry("lx_extend_batch", h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off,
                        out_ops, out_ops_bytes, nullptr, 0);
}

int lx_extend_batch_rle(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                        lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                        lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes)
{
    return extend_entry("lx_extend_batch_rle", h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off,
                        out_ops, out_ops_bytes, nullptr, 1);
}

int lx_extend_batch_list(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                         lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                         lx_survivor_list * out)
{
    return extend_entry("lx_extend_batch_list", h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, nullptr, nullptr,
                        nullptr, nullptr, out, 2);
}

} // extern "C"

// lx_extend_batch_list for the Level-2 driver on the device (lx_level2_host.cpp): query residues, window list and cut-offs are resident
int lxi::extend_list_resident(lx_handle * h, int slot, ResidentInput const & ri, lx_extension const * ext, uint64_t n, int32_t const * min_score,
                              int32_t * out_score, lx_survivor_list * out, ResidentSurvivors * where)
{
    *out   = lx_survivor_list{};
    *where = ResidentSurvivors{};
    if (n == 0)
        return LX_OK;
    if (slot < 0 || slot > 1 || !h->have_sc[slot])
        return fail(h, LX_ESTATE, "scoring slot %d not set", slot);
    if (n > 0xfffffff0ull / 2)
        return fail(h, LX_EINVAL, "at most 2^31 extensions per call");
    int const rc = extend_pipeline(h, slot, nullptr, ri.q_bytes, nullptr, 0, ext, n, min_score, 0, out_score, nullptr, nullptr, nullptr, nullptr, 2, &ri, where);
    if (rc == LX_OK)
        hand_out_list(h, out);
    return rc;
}

extern "C" {

int lx_last_extend_stats(lx_handle const * h, uint64_t * out4)
{
    if (!h || !out4)
        return LX_EINVAL;
    std::memcpy(out4, h->xb_stats, sizeof(h->xb_stats));
    return LX_OK;
}

int lx_expand_ops(uint8_t const * codes, int32_t n_ops, uint8_t * out)
{
    if (!codes || !out || n_ops < 0)
        return LX_EINVAL;
    rle_expand(codes, n_ops, out);
    return LX_OK;
}

} // extern "C"
