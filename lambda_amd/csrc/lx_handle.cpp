// lx_handle.cpp -- the handle of the C ABI declared in include/lambda_ext.h (compiled with hipcc).
//
// Owns: device selection, the HIP streams, the handle's utilities (errors, growing buffers, timing events, the device's error
// word), its options, the device copies of the scoring schemes and the resident subjects.  The steps that run on a handle are in
// lx_step.cpp (device lists) and lx_host.cpp (host buffers); lx_internal.h is what they share.
// No DP arithmetic happens on the host and there is no CPU fallback: without a usable gfx950 device every entry point
// returns an error.
#include "lx_internal.h"

namespace
{
thread_local std::string g_create_error;
}

// every environment switch of the library (lx_aids.h has the table)
lx::DevAids const & lx::dev_aids()
{
    static DevAids const aids = []()
    {
        auto num = [](char const * name, long long dflt) -> long long
        {
            char const * e = getenv(name);
            return e && *e ? atoll(e) : dflt;
        };
        auto set = [](char const * name) { return getenv(name) != nullptr; };
        DevAids a{};
        a.host_threads    = (unsigned)std::max(0ll, num("LX_HOST_THREADS", 0));
        a.mq_no_wide      = set("LX_MQ_NO_WIDE");
        a.mq_merge_below  = (uint64_t)std::max(0ll, num("LX_MQ_MERGE_BELOW", 0));
        a.iterate_on_host = set("LX_ITERATE_ON_HOST");
        a.bt_tile_at      = (int)num("LX_BT_TILE_AT", 0);
        a.bt_refill_at    = (int)num("LX_BT_REFILL_AT", 0);
        a.l2_ranges       = (uint64_t)std::min<long long>(std::max(0ll, num("LX_L2_RANGES", 0)), 64);
        a.host_timing     = set("LX_HOST_TIMING");
        return a;
    }();
    return aids;
}

namespace lxi
{

int fail(lx_handle * h, int code, char const * fmt, ...)
{
    char    buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h)
        h->error = buf;
    else
        g_create_error = buf;
    return code;
}

hipEvent_t pool_event(lx_handle * h)
{
    if (h->ev_pool_used == h->ev_pool.size())
    {
        lxi::Event e;
        if (hipEventCreate(e.out()) != hipSuccess)
            return nullptr;
        h->ev_pool.push_back(std::move(e));
    }
    return h->ev_pool[h->ev_pool_used++];
}




int ensure(lx_handle * h, DevBuf & b, size_t bytes)
{
    if (bytes <= b.cap)
        return LX_OK;
    size_t const had = b.cap;
    if (b.ptr)
    {
        LX_HIP(h, hipDeviceSynchronize()); // (kernels on a caller's stream may still read the old block)
        LX_HIP(h, hipFree(b.ptr));
        b.ptr = nullptr;
        b.cap = 0;
    }
    // (room to grow into, less of it for the large blocks: fresh device memory costs 40 ms per GB)
    size_t const want = bytes + (bytes >= ((size_t)1 << 30) ? bytes / 16 : bytes / 4) + 4096;
    if (lx::dev_aids().host_timing && want >= (64u << 20)) // (LX_HOST_TIMING: which buffer a call still had to grow -- what lx_reserve did not cover)
        fprintf(stderr, "[lx host ms]   device buffer %+ld in the handle grows from %.1f to %.1f MB\n", (long)(reinterpret_cast<char *>(&b) - reinterpret_cast<char *>(h)),
                (double)had / 1e6, (double)want / 1e6);
    LX_HIP(h, hipMalloc(&b.ptr, want));
    b.cap = want;
    return LX_OK;
}

int ensure_pinned(lx_handle * h, Pinned & b, size_t bytes, PinGrowth growth, unsigned flags)
{
    if (bytes <= b.cap)
        return LX_OK;
    if (b.ptr)
    {
        LX_HIP(h, hipHostFree(b.ptr));
        b.ptr = nullptr;
        b.cap = 0;
    }
    size_t const want = growth == kRoom ? bytes + bytes / 4 + 4096 : bytes;
    LX_HIP(h, hipHostMalloc(&b.ptr, want, flags));
    b.cap = want;
    return LX_OK;
}

int bind(lx_handle * h)
{
    LX_HIP(h, hipSetDevice(h->device));
    return LX_OK;
}

// the device's error word (kWsError) as a return code
int error_for_flag(lx_handle * h, uint32_t flag)
{
    if (flag == 1)
        return fail(h, LX_EOVERFLOW, "multi-panel carry workspace exhausted (raise LX_OPT_WORKSPACE_BYTES)");
    if (flag == 2)
        return fail(h, LX_ESTATE, "LX_OPT_QUERY_RUN promise violated: extensions of one wavefront use different queries");
    if (flag == 3)
        return fail(h, LX_EOVERFLOW, "an extension exceeds the trace slot bounds (LX_OPT_MAX_QLEN / LX_OPT_MAX_SLEN too small, or a subject window beyond the pass-2 limit)");
    if (flag == 4)
        return fail(h, LX_EOVERFLOW, "single sweep: no checkpoint slot left for an extension the packed-half kernel declined "
                                     "(raise LX_OPT_TRACE_BYTES, or set LX_OPT_PASS2_MODE to 1)");
    if (flag != 0)
        return fail(h, flag == 5 ? LX_EOVERFLOW : LX_EHIP, "device reported error flag %u", flag);
    return LX_OK;
}

int check_async_error(lx_handle * h)
{
    uint32_t flags[2] = {0, 0};
    LX_HIP(h, hipMemcpyAsync(flags, ws_word(h, kWsBump), sizeof(flags), hipMemcpyDeviceToHost, h->stream)); // (kWsBump and kWsError)
    LX_HIP(h, hipStreamSynchronize(h->stream));
    return error_for_flag(h, flags[kWsError]);
}


} // namespace lxi
using namespace lxi;

int lxi::resolve_subjects(lx_handle * h, uint8_t const * s_res, uint64_t s_bytes, SubjectRef & out)
{
    if (!s_res && s_bytes == 0 && h->db_bytes)
    {
        out.dev   = h->d_db.ptr;
        out.bytes = h->db_bytes;
        return LX_OK;
    }
    if (!s_res && s_bytes)
        return fail(h, LX_EINVAL, "NULL argument");
    int rc = ensure(h, h->d_s, s_bytes + kSlack);
    if (rc)
        return rc;
    out.dev    = h->d_s.ptr;
    out.bytes  = s_bytes;
    out.upload = s_bytes != 0;
    return LX_OK;
}

extern "C" {

int lx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int lx_create(int device_id, lx_handle ** out)
{
    if (!out)
        return fail(nullptr, LX_EINVAL, "lx_create: out is NULL");
    *out  = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, LX_ENODEV, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return fail(nullptr, LX_EINVAL, "device_id %d out of range [0,%d)", device_id, n);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess)
        return fail(nullptr, LX_EHIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, LX_ENODEV, "device %d is %s; this library ships gfx950 (MI355X) code only", device_id,
                    prop.gcnArchName);

    lx_handle * h = new lx_handle();
    if (lx::dev_aids().host_threads) // (measurement aid of tools/host_curve.py; a caller uses LX_OPT_HOST_THREADS)
        lxi::HostPool::instance().set_width(lx::dev_aids().host_threads);
    h->device     = device_id;
    auto bail     = [&](char const * what, hipError_t err)
    {
        int rc = fail(nullptr, LX_EHIP, "%s: %s", what, hipGetErrorString(err));
        delete h; // (gives back what the steps before made)
        return rc;
    };
    if ((e = hipSetDevice(device_id)) != hipSuccess)
        return bail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking)) != hipSuccess)
        return bail("hipStreamCreate", e);
    if ((e = hipEventCreate(h->ev0.out())) != hipSuccess || (e = hipEventCreate(h->ev1.out())) != hipSuccess)
        return bail("hipEventCreate", e);
    if ((e = hipStreamCreateWithFlags(h->stream2.out(), hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(h->stream3.out(), hipStreamNonBlocking)) != hipSuccess)
        return bail("hipStreamCreate", e);
    for (auto & ln : h->xb)
        for (lxi::Event * ev : {&ln.ev_up, &ln.ev_k, &ln.ev_cnt})
            if ((e = hipEventCreateWithFlags(ev->out(), hipEventDisableTiming)) != hipSuccess)
                return bail("hipEventCreate", e);
    if ((e = hipMalloc(h->d_ws_top.out(), lxi::kWsWords * sizeof(uint32_t))) != hipSuccess)
        return bail("hipMalloc", e);
    if ((e = hipMemset(h->d_ws_top, 0, lxi::kWsWords * sizeof(uint32_t))) != hipSuccess)
        return bail("hipMemset", e);
    for (int s = 0; s < 2; ++s)
        if ((e = hipMalloc(h->sc_dev[s].out(), sizeof(lx::ScoringDev))) != hipSuccess)
            return bail("hipMalloc", e);
    if ((e = hipHostMalloc(h->p_count.out(), 2 * sizeof(uint64_t), hipHostMallocDefault)) != hipSuccess)
        return bail("hipHostMalloc", e);
    if ((e = hipEventCreateWithFlags(h->ev_count.out(), hipEventDisableTiming)) != hipSuccess)
        return bail("hipEventCreate", e);
    *out = h;
    return LX_OK;
}

void lx_destroy(lx_handle * h)
{
    delete h;
}

// All three streams are through before the first member goes: the copies of stream2 / stream3 use the buffers too.
lx_handle::~lx_handle()
{
    if (device >= 0)
        (void)hipSetDevice(device);
    for (hipStream_t st : {stream.raw, stream2.raw, stream3.raw})
        if (st)
            (void)hipStreamSynchronize(st);
}

char const * lx_last_error(lx_handle const * h)
{
    return h ? h->error.c_str() : g_create_error.c_str();
}

int lx_host_threads_info(uint32_t * width, uint32_t * granted_cpus, uint32_t * local_world_size)
{
    lxi::HostPool const & p = lxi::HostPool::instance();
    if (width)
        *width = p.width();
    if (granted_cpus)
        *granted_cpus = p.granted_cpus();
    if (local_world_size)
        *local_world_size = p.local_world();
    return LX_OK;
}

int lx_set_option(lx_handle * h, int option, uint64_t value)
{
    if (!h)
        return LX_EINVAL;
    switch (option)
    {
        case LX_OPT_MAX_QLEN: h->opt_max_qlen = value; return LX_OK;
        case LX_OPT_QUERY_RUN: h->opt_query_run = value; return LX_OK;
        case LX_OPT_WORKSPACE_BYTES: h->opt_ws_bytes = std::max<uint64_t>(value, 1 << 20); return LX_OK;
        case LX_OPT_MAX_SLEN: h->opt_max_slen = value; return LX_OK;
        case LX_OPT_TRACE_BYTES: h->opt_trace_bytes = std::max<uint64_t>(value, 1 << 20); return LX_OK;
        case LX_OPT_BS_MATCH_RULE: h->opt_bs_rule = value ? 1 : 0; return LX_OK;
        case LX_OPT_PACKED_HALF: h->opt_f16 = value ? 1 : 0; return LX_OK;
        case LX_OPT_PASS2_MODE: h->opt_pass2 = value > 2 ? 1 : value; return LX_OK;
        case LX_OPT_EXTEND_CHUNK: h->opt_extend_chunk = value; return LX_OK;
        case LX_OPT_MQ_SWEEP:
            h->opt_mq       = value > 2 ? 1 : value;
            h->mq_decl_frac = 0.0; // (what the last chunks taught about compact codes against int16 pairs starts over)
            return LX_OK;
        case LX_OPT_ADAPT_PERMILLE: h->opt_adapt = std::min<uint64_t>(value, 1000); h->surv_frac = -1.0; return LX_OK;
        case LX_OPT_ITERATE_RECORDS: h->opt_iterate_records = value ? 1 : 0; return LX_OK;
        case LX_OPT_HOST_THREADS:
            if (value > lxi::HostPool::kMaxParts)
                return fail(h, LX_EINVAL, "LX_OPT_HOST_THREADS: at most %u", lxi::HostPool::kMaxParts);
            lxi::HostPool::instance().set_width((unsigned)value); // (the host threads are the process's, not the handle's)
            return LX_OK;
        case LX_OPT_GUNZIP_CHUNK:
            if (value && (value < (32u << 10) || value > (4u << 20)))
                return fail(h, LX_EINVAL, "LX_OPT_GUNZIP_CHUNK: 0, or 32 KiB to 4 MiB");
            h->opt_gunzip_chunk = value;
            return LX_OK;
        case LX_OPT_GUNZIP_PARALLEL_FROM: h->opt_gunzip_from = value; return LX_OK;
        case LX_OPT_INDEX_SLICE_WORDS: h->opt_index_slice = value; return LX_OK;
        case LX_OPT_LCA_RANGE_ROWS: h->opt_lca_range = value; return LX_OK;
        case LX_OPT_BAM_RANGE_BYTES:
            if (value &&(value < (128u << 10) || value > (2ull << 30)))
                return fail(h, LX_EINVAL, "LX_OPT_BAM_RANGE_BYTES: 0, or 128 KiB to 2 GiB");
            h->opt_bam_range = value;
            return LX_OK;
        case lxi::kOptGunzipWaveTest:
            if (value == 1 || value > 512)
                return fail(h, LX_EINVAL, "chunks per wave: 0, or 2 to 512");
            h->gunzip_wave = value;
            return LX_OK;
        case LX_OPT_BAND:
            if (value > (1u << 20))
                return fail(h, LX_EINVAL, "LX_OPT_BAND: at most 2^20 diagonals on either side");
            h->opt_band = value;
            return LX_OK;
        default: return fail(h, LX_EINVAL, "unknown option %d", option);
    }
}

int lx_get_option(lx_handle const * h, int option, uint64_t * value)
{
    if (!h || !value)
        return LX_EINVAL;
    switch (option)
    {
        case LX_OPT_MAX_QLEN: *value = h->opt_max_qlen; return LX_OK;
        case LX_OPT_QUERY_RUN: *value = h->opt_query_run; return LX_OK;
        case LX_OPT_WORKSPACE_BYTES: *value = h->opt_ws_bytes; return LX_OK;
        case LX_OPT_MAX_SLEN: *value = h->opt_max_slen; return LX_OK;
        case LX_OPT_TRACE_BYTES: *value = h->opt_trace_bytes; return LX_OK;
        case LX_OPT_BS_MATCH_RULE: *value = h->opt_bs_rule; return LX_OK;
        case LX_OPT_PACKED_HALF: *value = h->opt_f16; return LX_OK;
        case LX_OPT_PASS2_MODE: *value = h->opt_pass2; return LX_OK;
        case LX_OPT_BAND: *value = h->opt_band; return LX_OK;
        case LX_OPT_EXTEND_CHUNK: *value = h->opt_extend_chunk; return LX_OK;
        case LX_OPT_MQ_SWEEP: *value = h->opt_mq; return LX_OK;
        case LX_OPT_ADAPT_PERMILLE: *value = h->opt_adapt; return LX_OK;
        case LX_OPT_ITERATE_RECORDS: *value = h->opt_iterate_records; return LX_OK;
        case LX_OPT_HOST_THREADS: *value = lxi::HostPool::instance().width(); return LX_OK;
        case LX_OPT_GUNZIP_CHUNK: *value = h->opt_gunzip_chunk; return LX_OK;
        case LX_OPT_GUNZIP_PARALLEL_FROM: *value = h->opt_gunzip_from; return LX_OK;
        case LX_OPT_INDEX_SLICE_WORDS: *value = h->opt_index_slice; return LX_OK;
        case LX_OPT_LCA_RANGE_ROWS: *value = h->opt_lca_range; return LX_OK;
        case LX_OPT_BAM_RANGE_BYTES: *value = h->opt_bam_range; return LX_OK;
        default: return LX_EINVAL;
    }
}

int lx_set_band_centres(lx_handle * h, int32_t const * diag, uint64_t n)
{
    if (!h || (!diag && n))
        return LX_EINVAL;
    h->band_host.assign(diag, diag + n);
    return LX_OK;
}

int lx_set_band_centres_dev(lx_handle * h, void const * d_diag)
{
    if (!h)
        return LX_EINVAL;
    h->band_dev = static_cast<int32_t const *>(d_diag);
    return LX_OK;
}

int lx_builtin_scoring(int scoring_method, int match, int mismatch, int gap_open_lambda, int gap_extend,
                       lx_scoring * sc)
{
    if (!sc)
        return LX_EINVAL;
    try
    {
        lambda_amd::builtinScoring(scoring_method, match, mismatch, gap_open_lambda, gap_extend, *sc);
    }
    catch (std::exception const &)
    {
        return LX_EINVAL;
    }
    return LX_OK;
}

int lx_set_scoring(lx_handle * h, int slot, lx_scoring const * sc)
{
    if (!h || !sc)
        return LX_EINVAL;
    if (slot < 0 || slot > 1)
        return fail(h, LX_EINVAL, "slot must be 0 or 1");
    if (sc->alphabet_size < 1 || sc->alphabet_size > LX_ALPH - 1)
        return fail(h, LX_EINVAL, "alphabet_size must be in [1,31]");
    if (sc->gap_extend >= 0 || sc->gap_open > sc->gap_extend)
        return fail(h, LX_EINVAL, "need gap_open <= gap_extend < 0 (got %d / %d)", sc->gap_open, sc->gap_extend);
    if (sc->gap_open < -120 || sc->gap_extend < -27)
        return fail(h, LX_EINVAL, "gap costs out of the supported range");
    lxi::SchemeFacts const f = lxi::scheme_facts(*sc);
    lx::ScoringDev d{};
    d.alph = sc->alphabet_size;
    d.go   = sc->gap_open;
    d.ge   = sc->gap_extend;
    d.g2   = sc->gap_open - sc->gap_extend;
    for (int a = 0; a < lx::kAlph; ++a)
        for (int b = 0; b < lx::kAlph; ++b)
        {
            bool const pad = a >= sc->alphabet_size || b >= sc->alphabet_size;
            int const  v   = pad ? lx::kNegPad : sc->matrix[a * LX_ALPH + b];
            if (!pad && (v > 100 || v < -100))
                return fail(h, LX_EINVAL, "matrix entry [%d][%d]=%d outside [-100,100]", a, b, v);
            d.mat[a * lx::kAlph + b]     = (int8_t)v;
            d.mat_adj[a * lx::kAlph + b] = (int8_t)(pad ? lx::kNegPad : v - sc->gap_extend);
            int const adj                = v - sc->gap_extend;
            d.mat_trace[a * lx::kAlph + b] = (int8_t)(pad || adj < -31 || adj > 31 ? -125 : 4 * adj + 3);
        }
    d.trace_ok = f.trace_ok ? 1 : 0;
    d.smax     = 0;
    d.b8_ok    = f.b8_ok ? 1 : 0;
    for (int a = 0; a < lx::kAlph; ++a)
        for (int b = 0; b < lx::kAlph; ++b)
        {
            bool const pad = a >= sc->alphabet_size || b >= sc->alphabet_size;
            int const  v   = pad ? 0 : sc->matrix[a * LX_ALPH + b] - sc->gap_open;
            d.mat_b8[a * lx::kAlph + b] = (uint8_t)std::min(std::max(v, 0), 255);
        }
    for (int a = 0; a < lx::kAlph; ++a)
    {
        int rm = 0;
        for (int b = 0; b < lx::kAlph; ++b)
        {
            bool const pad = a >= sc->alphabet_size || b >= sc->alphabet_size;
            int const  v   = pad ? lx::kNegPad : sc->matrix[a * LX_ALPH + b] - sc->gap_extend;
            // v * 2^-24 as a half: a subnormal whose magnitude bits are |v| itself (|v| <= 131)
            d.mat_h[a * lx::kAlph + b]   = (uint16_t)(v < 0 ? 0x8000 | -v : v);
            d.mat_i16[a * lx::kAlph + b] = (int16_t)v;
            if (!pad)
            {
                rm     = std::max(rm, (int)sc->matrix[a * LX_ALPH + b]);
                d.smax = std::max(d.smax, (int)sc->matrix[a * LX_ALPH + b] - sc->gap_extend);
            }
        }
        d.rowmax[a] = (int16_t)rm;
    }
    int rc = bind(h);
    if (rc)
        return rc;
    // *_dev calls may still be in flight on a caller-supplied (non-blocking) stream and read this table
    LX_HIP(h, hipDeviceSynchronize());
    LX_HIP(h, hipMemcpy(h->sc_dev[slot], &d, sizeof(d), hipMemcpyHostToDevice));
    h->sc_host[slot] = *sc;
    h->have_sc[slot] = true;
    h->facts[slot]   = f;
    return LX_OK;
}

int lx_set_subjects(lx_handle * h, uint8_t const * s_res, uint64_t s_bytes)
{
    if (!h || (!s_res && s_bytes))
        return LX_EINVAL;
    int rc = bind(h);
    if (rc)
        return rc;
    h->db_bytes = 0;
    if (s_bytes == 0)
        return LX_OK;
    if ((rc = ensure(h, h->d_db, s_bytes + kSlack)))
        return rc;
    LX_HIP(h, hipMemcpyAsync(h->d_db.ptr, s_res, s_bytes, hipMemcpyHostToDevice, h->stream));
    LX_HIP(h, hipMemsetAsync(static_cast<uint8_t *>(h->d_db.ptr) + s_bytes, 0, kSlack, h->stream));
    LX_HIP(h, hipStreamSynchronize(h->stream));
    h->db_bytes = s_bytes;
    return LX_OK;
}

} // extern "C"
