// lx_xb_run.cpp -- the chunk driver of the one-query-per-wavefront kernels (lx_xb.h).  The ordered list is cut at query-run
// boundaries into chunks of a few hundred thousand extensions; per chunk the host groups the extensions by query slice and pads
// every run to 16 (or 8) slots -- the promise LX_OPT_QUERY_RUN makes to the device path -- into pinned staging, the GPU runs the whole
// fused step, and the results return as scores by slot + the survivors' records + their run-length codes.  What crosses PCIe per
// extension: 28 B up, 4 B + (survivors) 52 B + ~8 B of codes down.
#include "lx_xb.h"

namespace lxi
{
namespace
{

struct RunDriver
{
    Xb & x;

    // ---- prepare + queue chunk c, then unpack chunk c - 1 while c runs
    int run()
    {
        int rc;
        for (uint64_t k0 = 0; k0 < x.p.live; ++x.c)
        {
            uint64_t const k1 = x.p.run_chunk_end(k0, x.chunk_target);
            int const      L  = x.c & 1;
            if (x.in_flight[L] && (rc = collect(L)))
                return rc;
            if ((rc = enqueue(L, k0, k1)))
                return rc;
            if (x.in_flight[L ^ 1] && (rc = collect(L ^ 1)))
                return rc;
            k0 = k1;
        }
        return x.drain([this](int L) { return collect(L); });
    }

    // ---- device side of a chunk whose padded slots stand in lane L's pinned staging: uploads and kernels queued
    int launch_chunk(int L, uint64_t slots, uint64_t max_q, uint64_t max_s, uint64_t kRun)
    {
        lx_handle * const    h        = x.h;
        auto const           t1       = now();
        lx_handle::XbLane &  ln       = h->xb[L];
        lx_extension * const slot_ext = static_cast<lx_extension *>(ln.p_ext.ptr);
        int32_t * const      slot_min = static_cast<int32_t *>(ln.p_min.ptr);
        int                  rc2;
        uint64_t const       stride = (max_q + max_s + 3) & ~3ull;
        if ((rc2 = x.size_lane(L, slots, stride, false, false)))
            return rc2;
        LX_HIP(h, hipMemcpyAsync(ln.d_ext.ptr, slot_ext, slots * sizeof(lx_extension), hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipMemcpyAsync(ln.d_min.ptr, slot_min, slots * sizeof(int32_t), hipMemcpyHostToDevice, h->stream3));
        LX_HIP(h, hipEventRecord(ln.ev_up, h->stream3));
        // (all chunks' kernels in one stream: side by side they were measured slower, see extend_pipeline)
        LX_HIP(h, hipStreamWaitEvent(h->stream, ln.ev_up, 0));
        if ((rc2 = x.run_fused(L, slots, stride, max_q, max_s, kRun)) || (rc2 = x.send_counts(L, 4, slots)))
            return rc2;
        x.t_issue += ms(t1, now());
        return LX_OK;
    }

    // ---- chunk k0 .. k1 of the ordered list -> padded slots in lane L's pinned staging -> uploads and kernels queued
    int enqueue(int L, uint64_t k0, uint64_t k1)
    {
        lx_handle * const             h         = x.h;
        lx_extension const * const    ext       = x.ext;
        int32_t const * const         min_score = x.min_score;
        int32_t const                 min_score_all = x.min_score_all;
        unsigned const                nthreads  = x.nthreads;
        auto const                    t0        = now();
        lx_handle::XbLane &           ln        = h->xb[L];
        XbPrep &                      pr        = x.prep[L];
        std::vector<uint32_t> const & idx       = x.p.idx;
        std::vector<uint8_t> const &  newrun    = x.p.newrun;
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
        x.t_prep += ms(t0, now());
        return launch_chunk(L, slots, max_q, max_s, kRun);
    }

    // ---- results of the chunk in lane L -> the caller's rows, or its scores + the handle's list
    int collect(int L)
    {
        XbPrep &         pr = x.prep[L];
        auto const       t0 = now();
        uint64_t const * cnt;
        int              rc2;
        if ((rc2 = x.wait_counts(L, cnt)) || (rc2 = x.check_counts(pr, cnt)))
            return rc2;
        uint64_t const count = cnt[0], nrle = cnt[2];
        if ((rc2 = x.download_survivors(L, count, nrle)))
            return rc2;
        auto const t1 = now();
        x.t_wait += ms(t0, t1);
        if (x.sink.where == XbSink::kRows)
            return rows_of_slots(x, L, count, t1);
        int32_t const * const  sc        = static_cast<int32_t const *>(x.h->xb[L].p_score.ptr);
        uint32_t const * const slot_src  = pr.slot_src.data();
        int32_t * const        out_score = x.out_score;
        parallel_ranges(pr.slots, x.nthreads,
                        [&](unsigned, uint64_t lo, uint64_t hi)
                        {
                            for (uint64_t o = lo; o < hi; ++o)
                                if (slot_src[o] != 0xffffffffu)
                                    out_score[slot_src[o]] = sc[o];
                        });
        rc2 = list_append(x, L, count, nrle, slot_src);
        x.t_unpack += ms(t1, now());
        return rc2;
    }
};

} // namespace

int run_chunks_of_runs(Xb & x) { return RunDriver{x}.run(); }

} // namespace lxi
