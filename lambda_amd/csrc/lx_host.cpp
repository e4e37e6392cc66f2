// lx_host.cpp -- lx_extend_batch / _rle / _list: the fused step (pass 1, filter, pass 2 -- _performAlignment at
// /root/reference/src/search_algo.hpp:1246 and :1296 with the filter loop :1251-1283 between them) on lists in host memory, as a
// pipeline of chunks (pinned staging, two chunks in flight, run-length coded ops on the wire), and the same pipeline over a list
// that is resident on the device already (lxi::extend_list_resident, what the Level-2 driver calls).  Here: the entry points and
// extend_pipeline, which validates, plans (lx_host_plan.cpp; lx_plan_free.hip plans device lists), says where the results go and
// hands the plan to the chunk pipeline -- lx_xb.h: the shared lanes (lx_xb_core.cpp), the result sinks (lx_xb_sinks.cpp) and one
// chunk driver per kind of plan (lx_xb_run.cpp, lx_xb_wf.cpp).  Two chunks are in flight: uploads and downloads of one run on copy
// streams while the other's kernels run, and the host prepares chunk k + 1 / unpacks chunk k - 1 meanwhile.  The entry points of
// the single passes are lx_host_batch.cpp; the fused step all of them drive lives in lx_step.cpp; no DP arithmetic here.
#include "lx_internal.h"
#include "lx_level2.h"
#include "lx_xb.h"
using namespace lxi;

// Both passes on host buffers: validate and plan (lx_host_plan.cpp), then the pipeline of chunks.
// ri (lx_level2_host.cpp): the query residues and the caller's list + cut-offs stand on the device already (q_res is NULL, q_bytes the
// resident size; `ext` / `min_score` are the host's copies of the same list, for the plan)
// sink: rows of column bytes or of run-length codes, or the survivors as a list in the handle's buffers (out_hsp, out_ops_off, out_ops,
// out_ops_bytes are NULL; lx_extend_batch_list hands the buffers out) -- which the wavefront driver turns into a list on the device
// where ri asks for one and the multi-query plan serves the call
static int extend_pipeline(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                           lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                           lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes, XbSink sink,
                           lxi::ResidentInput const * ri = nullptr, lxi::ResidentSurvivors * where = nullptr)
{
    bool const           as_list = sink.where == XbSink::kList;
    HostPool::Call const in_flight_call; // (the host threads look for this call's next loop instead of going to sleep between two)
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
    HostMarks hm(as_list ? "lx_extend_batch_list" : sink.codes ? "lx_extend_batch_rle" : "lx_extend_batch");

    // a plan that was made on the device (lx_level2_host.cpp: the solo packing of a resident window list -- a sort by width and
    // length, 16 windows to a wavefront)
    bool const preplanned = ri && ri->d_plan;
    HostPlan & plan       = h->plan;
    if ((rc = plan.order(h, ext, n, q_bytes, s_bytes, as_list, preplanned, out_score, out_hsp, out_ops_off, hm)) || plan.live == 0)
        return rc;
    if ((rc = plan.choose(h, slot, ri, as_list)))
        return rc;
    Xb pipe(h, slot, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off, sink, ri, hm);
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
    if (rc == LX_OK && as_list)
        h->xb_ops_total = pipe.ops_total;
    else if (rc == LX_OK)
    {
        *out_ops       = h->ext_bytes.data();
        *out_ops_bytes = pipe.ops_total;
    }
    // (ResidentInput::keep_on_device: the survivors are on the device where the multi-query plan served the list)
    if (where && pipe.sink.on_device())
        *where = lxi::ResidentSurvivors{pipe.sink.where == XbSink::kDevice ? lxi::ResidentSurvivors::kOnDevice : lxi::ResidentSurvivors::kOnDeviceByRange, h->l2.surv_total};
    return rc;
}

// the handle's survivor list of the last call, handed out
static void hand_out_list(lx_handle * h, lx_survivor_list * out)
{
    *out = lx_survivor_list{h->res_count, reinterpret_cast<uint32_t const *>(h->res_index.data()), reinterpret_cast<lx_hsp const *>(h->res_hsp.data()),
                            reinterpret_cast<uint64_t const *>(h->res_off.data()), h->ext_bytes.data(), h->res_count ? h->xb_ops_total : 0};
}

// the three entry points (sink as extend_pipeline's; `out` is the list form's): their argument checks, band mode, the list handed out
static int extend_entry(char const * what, lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                        lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score, lx_hsp * out_hsp,
                        uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes, lx_survivor_list * out, XbSink sink)
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
    bool const as_list = sink.where == XbSink::kList;
    bool const outs_ok = as_list ? out != nullptr : (out_hsp && out_ops_off && out_ops && out_ops_bytes);
    if (!ext || !out_score || !outs_ok || (!q_res && q_bytes))
        return fail(h, LX_EINVAL, "NULL argument");
    if (n > 0xfffffff0ull / 2)
        return fail(h, LX_EINVAL, "at most 2^31 extensions per call");
    if (h->opt_band && !as_list && !sink.codes)
        return host_banded(h, slot, 2, q_res, q_bytes, s_res, s_bytes, ext, n, nullptr, min_score, min_score_all, out_score, out_hsp, nullptr,
                           nullptr, out_ops_off, out_ops, out_ops_bytes);
    if (h->opt_band)
        return fail(h, LX_EINVAL, "%s: band mode returns column bytes only (lx_extend_batch)", what);
    int const rc = extend_pipeline(h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off, out_ops,
                                   out_ops_bytes, sink);
    if (rc == LX_OK && as_list)
        hand_out_list(h, out);
    return rc;
}

extern "C" {

int lx_extend_batch(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                    lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                    lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes)
{
    return extend_entry("lx_extend_batch", h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off,
                        out_ops, out_ops_bytes, nullptr, XbSink{XbSink::kRows, false});
}

int lx_extend_batch_rle(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                        lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                        lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes)
{
    return extend_entry("lx_extend_batch_rle", h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, out_hsp, out_ops_off,
                        out_ops, out_ops_bytes, nullptr, XbSink{XbSink::kRows, true});
}

int lx_extend_batch_list(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                         lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                         lx_survivor_list * out)
{
    return extend_entry("lx_extend_batch_list", h, slot, q_res, q_bytes, s_res, s_bytes, ext, n, min_score, min_score_all, out_score, nullptr, nullptr,
                        nullptr, nullptr, out, XbSink{XbSink::kList, true});
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
    int const rc = extend_pipeline(h, slot, nullptr, ri.q_bytes, nullptr, 0, ext, n, min_score, 0, out_score, nullptr, nullptr, nullptr, nullptr, XbSink{XbSink::kList, true}, &ri, where);
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
