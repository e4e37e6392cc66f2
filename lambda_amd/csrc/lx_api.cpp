// lx_api.cpp -- the C exports of include/lambda_ext.h that are neither the handle's own (lx_handle.cpp) nor a host-buffer entry point
// (lx_host.cpp, lx_host_batch.cpp): version and build id, the plan shown to tests (lx_plan_step), timing and kernel names of the
// last call, and the device entry points (lx_*_dev), which check their arguments and hand over to lx_step.cpp.
// The build compiles this file again whenever any source changed: it carries the build id.
#include "lx_internal.h"
#include "lx_numfmt.h"

static_assert(sizeof(lx_extension) == sizeof(lx::Extension), "ABI mismatch");
static_assert(sizeof(lx_hsp) == sizeof(lx::Hsp), "ABI mismatch");
static_assert(sizeof(lx_extension) == 24, "ABI mismatch");

using namespace lxi;

extern "C" {

int lx_abi_version(void)
{
    return LX_ABI_VERSION;
}

#ifndef LX_BUILD_ID
#define LX_BUILD_ID "unknown-build-id"
#endif
// "LXBUILDID:" + id: lambda_amd/build.py finds the marker in the file without loading it
static char const g_build_id[] = "LXBUILDID:" LX_BUILD_ID;
char const * lx_build_id(void)
{
    return g_build_id + 10;
}

int lx_plan_step(lx_scoring const * sc, uint64_t max_qlen, uint64_t max_slen, uint64_t query_run, uint64_t n, uint64_t pass2_mode,
                 uint64_t mq_sweep, uint64_t packed_half, uint64_t trace_bytes, double survivor_share, uint64_t adapt_permille,
                 lx_step_plan * out)
{
    if (!sc || !out || sc->alphabet_size < 1 || sc->alphabet_size > LX_ALPH - 1 || sc->gap_extend >= 0 || sc->gap_open > sc->gap_extend)
        return LX_EINVAL;
    lxi::SchemeFacts const f = lxi::scheme_facts(*sc);
    lxi::StepOptions o{};
    o.max_qlen = max_qlen, o.max_slen = max_slen, o.query_run = query_run, o.n = n, o.pass2 = pass2_mode > 2 ? 1 : pass2_mode;
    o.mq = mq_sweep > 2 ? 1 : mq_sweep, o.f16 = packed_half ? 1 : 0, o.trace_bytes = std::max<uint64_t>(trace_bytes, 1 << 20);
    o.surv_frac = survivor_share, o.adapt = std::min<uint64_t>(adapt_permille, 1000);
    lxi::StepPlan const pl = lxi::plan_step(f, o);
    std::memset(out, 0, sizeof(*out));
    out->family                = (int32_t)pl.family;
    out->adapted               = pl.adapted ? 1 : 0;
    lxi::describe_plan(pl, out->name, sizeof(out->name));
    if (pl.family == lxi::kNoSweep)
        return LX_OK;
    int const G = pl.geo.g, C = pl.geo.c, nrows = f.nrows();
    out->group_lanes           = G;
    out->strip_cols            = C;
    out->panels                = (int32_t)pl.panels;
    out->compact_codes         = pl.compact ? 1 : 0;
    out->may_decline           = pl.may_decline ? 1 : 0;
    out->slot_bytes            = pl.stride * 4;
    int const per_wave         = pl.family == lxi::kInt32Sweep ? 64 / G : 2 * (64 / G); // extensions a wavefront holds
    int const share_ext        = pl.family == lxi::kMqSweep ? std::max(1, 2 * pl.share) : (pl.family == lxi::kHalfSweep && pl.share) ? 2 * pl.share : per_wave;
    out->queries_per_wavefront = std::max(1, per_wave / std::max(1, share_ext));
    if (pl.family == lxi::kMqSweep && pl.share == 1)
        out->queries_per_wavefront = 4; // (free packing: up to four, in any split of the eight lane groups)
    switch (pl.family)
    {
        case lxi::kMqSweep: out->lds_bytes = lx::sweep_mq_lds_bytes(pl.geo, pl.share < 0 ? sc->alphabet_size + 1 : nrows, pl.share); break;
        case lxi::kInt32Sweep: out->lds_bytes = (uint64_t)out->queries_per_wavefront * nrows * ((C + 3) / 4 * G) * 4 + 64 * 4 * 4; break;
        default: out->lds_bytes = (uint64_t)out->queries_per_wavefront * lx::score_pair_profile_bytes(pl.geo, nrows) + 64 * 8 * 4; break;
    }
    // the a-priori bound may_decline is derived from
    out->score_bound = (uint64_t)(lxi::score_bound(f, max_qlen, pl.steps, G) + (pl.family == lxi::kHalfSweep ? lxi::half_frame_bias(f, G) : 0));
    return LX_OK;
}

int lx_synchronize(lx_handle * h)
{
    if (!h)
        return LX_EINVAL;
    int rc = bind(h);
    if (rc)
        return rc;
    return check_async_error(h);
}

char const * lx_last_kernel_name(lx_handle const * h)
{
    return h ? h->last_kernel.c_str() : "";
}

char const * lx_last_trace_kernel_name(lx_handle const * h)
{
    return h ? h->last_trace_kernel.c_str() : "";
}

static_assert(LX_NUM_E1 == lx::kNumE1 && LX_NUM_F1 == lx::kNumF1 && LX_NUM_F2 == lx::kNumF2 && LX_NUM_G_FLOAT == lx::kNumGFloat,
              "the ABI's kinds are the formatter's");

int lx_format_number(int kind, double v, char * out, uint64_t cap)
{
    if (!out || kind < LX_NUM_E1 || kind > LX_NUM_G_FLOAT)
        return LX_EINVAL;
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    char      text[lx::kNumMaxText];
    int const n = lx::num_format(kind, bits, text);
    if (n == 0 || (uint64_t)n + 1 > cap) // (0: an F value outside the domain)
        return LX_EINVAL;
    std::memcpy(out, text, (size_t)n);
    out[n] = 0;
    return n;
}

int lx_last_phase_ms(lx_handle * h, int phase, float * ms, int * launches)
{
    if (!h || !ms)
        return LX_EINVAL;
    int rc = bind(h);
    if (rc)
        return rc;
    float total = 0.f;
    int   cnt   = 0;
    for (auto const & pe : h->phase_ev)
        if (pe.phase == phase || pe.phase == phase + lxi::kPhaseTimeOnly)
        {
            float t = 0.f;
            LX_HIP(h, hipEventSynchronize(pe.b));
            LX_HIP(h, hipEventElapsedTime(&t, pe.a, pe.b));
            total += t;
            cnt += pe.phase == phase ? 1 : 0;
        }
    for (int i = 0; i < 3; ++i) // (lx_gunzip's plain-member kernels: summed per wave by the call itself)
        if (phase == 10 || phase == 101 + i)
        {
            total += h->gunzip.phase_ms[i];
            cnt += h->gunzip.phase_launches[i];
        }
    *ms = total;
    if (launches)
        *launches = cnt;
    return LX_OK;
}

int lx_last_kernel_ms(lx_handle * h, float * ms)
{
    if (!h || !ms)
        return LX_EINVAL;
    if (!h->timed)
        return fail(h, LX_ESTATE, "no timed launch yet");
    int rc = bind(h);
    if (rc)
        return rc;
    LX_HIP(h, hipEventSynchronize(h->ev1));
    LX_HIP(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return LX_OK;
}

int lx_score_batch_dev(lx_handle * h, int slot, void const * d_q_res, void const * d_s_res, void const * d_ext,
                       uint64_t n, void * d_out_score, void * stream_)
{
    if (!h)
        return LX_EINVAL;
    if (slot < 0 || slot > 1 || !h->have_sc[slot])
        return fail(h, LX_ESTATE, "scoring slot %d not set", slot);
    if (n == 0)
        return LX_OK;
    if (!d_q_res || !d_s_res || !d_ext || !d_out_score)
        return fail(h, LX_EINVAL, "NULL device pointer");
    int rc = bind(h);
    if (rc)
        return rc;
    hipStream_t const stream = stream_ ? static_cast<hipStream_t>(stream_) : h->stream;
    ListLimits const  lim    = option_limits(h);
    if ((rc = prepare_workspace(h, stream, plan_score(h->facts[slot], lim, score_options(h)).carry_pairs(n))))
        return rc;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    LX_HIP(h, hipEventRecord(h->ev0, stream));
    if ((rc = score_dev_impl(h, slot, d_q_res, d_s_res, d_ext, n, d_out_score, stream, lim)))
        return rc;
    LX_HIP(h, hipEventRecord(h->ev1, stream));
    h->timed = true;
    return LX_OK;
}

int lx_align_batch_dev(lx_handle * h, int slot, void const * d_q_res, void const * d_s_res, void const * d_ext,
                       uint64_t n, void * d_out_hsp, void * d_out_ops, void const * d_ops_off, void * stream_)
{
    if (!h)
        return LX_EINVAL;
    if (slot < 0 || slot > 1 || !h->have_sc[slot])
        return fail(h, LX_ESTATE, "scoring slot %d not set", slot);
    if (n == 0)
        return LX_OK;
    if (!d_q_res || !d_s_res || !d_ext || !d_out_hsp || !d_out_ops || !d_ops_off)
        return fail(h, LX_EINVAL, "NULL device pointer");
    int rc = bind(h);
    if (rc)
        return rc;
    hipStream_t stream = stream_ ? static_cast<hipStream_t>(stream_) : h->stream;
    ListLimits  lim    = option_limits(h);
    if (lim.max_qlen == 0 || lim.max_slen == 0)
    {
        // no hints: measure on the device (one small kernel + a stream synchronisation)
        lx::MaxLens * d_ml = reinterpret_cast<lx::MaxLens *>(ws_word(h, kWsMaxLens));
        LX_HIP(h, lx::launch_max_lens(static_cast<lx::Extension const *>(d_ext), n, d_ml, stream));
        lx::MaxLens ml{};
        LX_HIP(h, hipMemcpyAsync(&ml, d_ml, sizeof(ml), hipMemcpyDeviceToHost, stream));
        LX_HIP(h, hipStreamSynchronize(stream));
        lim.max_qlen = std::max<uint64_t>(ml.max_q, 1);
        lim.max_slen = std::max<uint64_t>(ml.max_s, 1);
    }
    int const share_slots = 0; // (no promise about the list)
    if ((rc = prepare_workspace(h, stream, plan_trace(h->facts[slot], lim, share_slots, trace_options(h)).carry_pairs(n))))
        return rc;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    LX_HIP(h, hipEventRecord(h->ev0, stream));
    rc = align_dev_impl(h, slot, d_q_res, d_s_res, static_cast<lx::Extension const *>(d_ext), n, static_cast<lx::Hsp *>(d_out_hsp),
                        static_cast<uint8_t *>(d_out_ops), static_cast<uint64_t const *>(d_ops_off), stream, lim, share_slots);
    if (rc)
        return rc;
    LX_HIP(h, hipEventRecord(h->ev1, stream));
    h->timed = true;
    return LX_OK;
}

int lx_extend_batch_dev(lx_handle * h, int slot, void const * d_q_res, void const * d_s_res, void const * d_ext,
                        uint64_t n, void const * d_min_score, int32_t min_score_all, void * d_out_score,
                        void * d_out_hsp, void * d_out_ops, void const * d_ops_off, void * d_out_count, void * stream_)
{
    if (!h)
        return LX_EINVAL;
    if (h->count_pending && hipEventQuery(h->ev_count) == hipSuccess)
    {
        // the previous call's survivor count has arrived: the adaptive choice of pass-2 mode (plan_step) goes by it
        h->count_pending = false;
        if (h->count_n)
            h->surv_frac = (double)h->p_count[1] / (double)h->count_n;
    }
    StepCall c;
    c.d_q = d_q_res, c.d_s = d_s_res, c.d_ext = d_ext, c.n = n, c.d_min_score = d_min_score, c.min_score_all = min_score_all;
    c.d_out_score = d_out_score, c.d_out_hsp = d_out_hsp, c.d_out_ops = d_out_ops, c.d_ops_off = d_ops_off, c.d_out_count = d_out_count;
    c.stream = stream_ ? static_cast<hipStream_t>(stream_) : h->stream;
    c.lim    = option_limits(h);
    int const rc = fused_impl(h, slot, c);
    if (rc == LX_OK && n != 0 && h->p_count && !h->count_pending)
    {
        hipStream_t const stream = c.stream;
        if (hipMemcpyAsync(h->p_count, d_out_count, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
            hipEventRecord(h->ev_count, stream) == hipSuccess)
        {
            h->count_pending = true;
            h->count_n       = n;
        }
    }
    return rc;
}

} // extern "C"
