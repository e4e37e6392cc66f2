// lx_internal.h -- what lx_api.cpp (the C exports of the device entry points), lx_handle.cpp (handle, options, scoring), lx_step.cpp
// (the launchers and the fused step) and lx_host.cpp (the host-buffer entry points and their pipelines) share: the handle, the
// launchers of the kernel files, small host helpers.  The plans they follow are in lx_step_plan.h.  Not part of the ABI;
// include/lambda_ext.h is.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include <sched.h>

#include "../../include/lambda_ext.h"
#include "host/scoring_tables.hpp"
#include "lx_aids.h"
#include "lx_device.h"
#include "lx_host_plan.h"
#include "lx_host_pool.h"
#include "lx_output_host.h"
#include "lx_resources.h"
#include "lx_step_plan.h"


namespace lx
{
hipError_t launch_score(Geo geo, ScoreParams const & p, bool multi, hipStream_t stream);
hipError_t launch_score_pair(Geo geo, ScoreParams const & p, hipStream_t stream);
uint64_t   select_blocks(uint64_t nruns);
hipError_t launch_trace_forward(TraceParams const & p, hipStream_t stream);
hipError_t launch_backtrace(TraceParams const & p, hipStream_t stream);
hipError_t launch_max_lens(Extension const * ext, uint64_t n, MaxLens * out, hipStream_t stream);
hipError_t launch_select(SelectParams const & p, hipStream_t stream);
hipError_t launch_slot_gather(Extension const * ext_all, int32_t const * min_all, int32_t min_score_all, uint32_t const * orig, uint64_t slots,
                              Extension * out_ext, int32_t * out_min, hipStream_t stream);
hipError_t launch_slot_scatter(uint32_t const * orig, uint64_t slots, int32_t const * score, int32_t * score_all, uint32_t * src,
                               uint64_t const * count_ptr, uint64_t cap, hipStream_t stream);
hipError_t launch_ckpt_forward(TraceParams const & p, hipStream_t stream);
hipError_t launch_ckpt_backtrace(TraceParams const & p, hipStream_t stream);
hipError_t launch_sweep_pair16(Geo geo, ScoreParams const & p, hipStream_t stream);
hipError_t launch_score_pair16(ScoreParams const & p, hipStream_t stream);
hipError_t launch_sweep_pair16_compact(Geo geo, ScoreParams const & p, hipStream_t stream);
hipError_t launch_sweep_mq(Geo geo, ScoreParams const & p, hipStream_t stream);
hipError_t launch_prefilter(PrefilterParams const & p, hipStream_t stream);
hipError_t launch_rle_pack(PackParams const & p, hipStream_t stream);
} // namespace lx

using lxi::DevBuf;
using lxi::Pinned;

// Every buffer, event and stream below is an owner (lx_resources.h): the destructor binds the device and waits for the three streams,
// then the members give back what they hold.
struct lx_handle
{
    ~lx_handle();
    int         device = -1;
    lxi::Stream stream;
    lxi::Event  ev0, ev1;
    lxi::Stream stream2;                                 // downloads of lx_extend_batch
    bool        timed = false;
    std::string error;
    // lx_extend_batch: host staging that keeps its pages between calls
    lxi::HostPlan             plan; // lx_extend_batch*'s host plan (lx_host_plan.cpp)
    std::vector<uint32_t>     xb_src, xb_pos;
    uint64_t                  xb_stats[4] = {0, 0, 0, 0}; // lx_extend_batch: extensions, slots, cells, cells executed (padding included)
    std::vector<uint64_t>     xb_grp, xb_off;
    std::vector<lx_extension> xb_ext;
    std::vector<int32_t>      xb_min, xb_score;
    std::vector<uint8_t> ext_ops; // band mode: the ops of the last lx_extend_batch call (handed out by pointer)
    // lx_extend_batch: the ops of the last call, grown without touching what is already there
    struct Bytes
    {
        uint8_t * p   = nullptr;
        size_t    cap = 0;
        uint8_t * data() { return p; }
        void      clear() {}
        bool      grow(size_t bytes) // false: out of memory (the old block and its contents stay)
        {
            if (bytes <= cap)
                return true;
            size_t const want = std::max(bytes + bytes / 2, (size_t)1 << 20);
            void * const np   = std::realloc(p, want);
            if (!np)
                return false;
            p   = static_cast<uint8_t *>(np);
            cap = want;
            return true;
        }
        ~Bytes() { std::free(p); }
    };
    Bytes ext_bytes;
    // lx_extend_batch_list: the survivors of the last call (positions in the caller's list, records, where their codes begin)
    Bytes    res_index, res_hsp, res_off;
    uint64_t res_count = 0, xb_ops_total = 0;
    // lx_extend_batch's two chunks in flight: pinned staging, device buffers, events
    struct XbLane
    {
        Pinned     p_ext, p_min, p_score, p_cnt, p_hsp, p_src, p_rle, p_len, p_orig, p_wft;
        DevBuf     d_ext, d_min, d_score, d_hsp, d_ops, d_rle, d_src, d_cnt, d_len, d_orig, d_wft; // (wft: the chunk's lx::WfSlots table)
        lxi::Event ev_up, ev_k, ev_cnt;
    } xb[2];
    // multi-query plan: the caller's whole list, its cut-offs and the scores in caller order, on the device / in pinned staging
    DevBuf      d_ext_all, d_min_all, d_score_all;
    Pinned      p_all, p_score_all;
    lxi::Stream stream3; // uploads of lx_extend_batch (stream2 carries its downloads)
    std::string last_kernel; // human-readable name of the most recent DP kernel geometry (profiling aid)
    std::string last_trace_kernel;
    // per-phase HIP events of the most recent call: phase 0 score, 1 select, 2 trace forward, 3 backtrace
    struct PhaseEv
    {
        int        phase;
        hipEvent_t a, b;
    };
    std::vector<PhaseEv>    phase_ev;      // events recorded by the last call
    std::vector<lxi::Event> ev_pool;       // reusable timing events
    size_t                  ev_pool_used = 0;

    bool             have_sc[2] = {false, false};
    lxi::SchemeFacts facts[2];
    lx_scoring       sc_host[2];
    lxi::DevBlock<lx::ScoringDev> sc_dev[2];

    // staging for the host-buffer entry points
    DevBuf d_q, d_s, d_ext, d_out, d_ops, d_opsoff, d_keep, d_trace, d_ends, d_hsp, d_seeds, d_sel_ext, d_sel_src, d_sel_runs, d_sel_score, d_trace_score, d_db;
    // multi-panel carry workspace
    DevBuf     d_ws;
    lxi::DevBlock<uint32_t> d_ws_top; // its control words (lxi::WsWord)
    // options
    uint64_t opt_max_qlen  = 0;
    uint64_t opt_query_run = 0;
    uint64_t opt_ws_bytes  = 64ull << 20; // the caller's LX_OPT_WORKSPACE_BYTES
    uint64_t ws_grown      = 0;           // what the calls grew the workspace to by themselves (never shown to the caller)
    uint64_t opt_max_slen  = 0;
    uint64_t opt_trace_bytes = 64ull << 30;
    uint64_t opt_bs_rule   = 0;
    uint64_t opt_f16       = 1;
    uint64_t opt_mq        = 1; // LX_OPT_MQ_SWEEP
    uint64_t opt_iterate_records = 0; // LX_OPT_ITERATE_RECORDS: 0 = the Level-2 driver's records on the device (lx_records.hip), 1 = on the host threads
    // Adaptive pass 2 (LX_OPT_PASS2_MODE = 2): the share of the last batch's extensions that passed the cut-off.  Below
    // LX_OPT_ADAPT_PERMILLE the single sweep's checkpoints are mostly written for nothing, and the step runs as plain pass 1 +
    // checkpoints for the survivors only (mode 1) until the share rises again.  The device entry point never synchronises: it
    // copies the count back behind its kernels and reads it at the next call if it has arrived by then.
    double      surv_frac        = -1.0;   // < 0: unknown
    lxi::PinnedBlock<uint64_t> p_count;    // pinned: [0] = slots, [1] = survivors of the last device-resident call
    lxi::Event  ev_count;
    uint64_t    count_n          = 0;
    bool        count_pending    = false;
    uint64_t    opt_adapt        = 30;     // LX_OPT_ADAPT_PERMILLE
    double   mq_decl_frac  = 0.0;   // lx_extend_batch: the share of the last multi-panel chunk's windows that the compact sweep declined
    uint64_t opt_extend_chunk = 0; // LX_OPT_EXTEND_CHUNK: extensions per chunk of lx_extend_batch's pipeline (0 = default)
    uint64_t opt_band      = 0; // LX_OPT_BAND: half width in diagonals, 0 = full rectangle (the reference's BandOff)
    int32_t const * band_dev = nullptr;  // lx_set_band_centres_dev: the caller's device array for the *_dev calls
    std::vector<int32_t> band_host;      // lx_set_band_centres: centres of the next host-buffer call's extensions
    DevBuf   d_band;                     // ... uploaded
    uint64_t opt_pass2     = 2; // LX_OPT_PASS2_MODE: 0 = direction bits (lx_trace.hip), 1 = checkpoints (lx_ckpt.hip), 2 = single sweep; each where applicable
    uint64_t db_bytes      = 0; // lx_set_subjects: size of the resident subject buffer (0 = none)
    // Level 2 on the device (lx_level2_host.cpp): the resident sequence sets (lx_set_queries, lx_set_subject_seqs) and the buffers of
    // the list work -- sort words (two of each), digit counts, scan values, windows
    struct Level2
    {
        std::vector<uint64_t> q_off, s_off, s_len;
        std::vector<uint32_t> q_len, q_evlen, evlens; // evlens: the distinct e-value lengths of the query set
        uint64_t              q_hash = 0, s_hash = 0; // content hashes of the sets lx_iterate_matches made resident
        uint64_t              q_bytes = 0, max_slen = 0, s_extent = 0; // s_extent: where the last subject ends in the residue buffer
        uint32_t              max_evlen = 0;
        int                   q_frames  = 1;
        DevBuf                d_qres, d_qoff, d_qlen, d_qband, d_qevlen, d_soff, d_slen;
        DevBuf                d_pair[2], d_s0[2], d_hist, d_head, d_tot, d_win, d_cut, d_cnt, d_up, d_plan, d_wf, d_fp; // (d_fp: workspace of the free-packing plan)
        Pinned                p_cnt, p_win, p_up;
        std::vector<lx_extension> ext;   // host copies of the window list, its cut-offs and scores
        std::vector<int32_t>      min, score;
        lxi::Event                ev_win;    // the window list has arrived on the host
        lxi::Event                ev_rank[2]; // the window list is complete / the rank kernel (second stream) is through
        // records on the device (lx_records.hip): the call's survivors as the pipeline's chunks left them (alignment, window, where the
        // codes begin), the key / scan / record buffers, the host-made tables of the e-value
        uint32_t              max_qlen = 0;
        DevBuf                d_qevidx, d_surv_hsp, d_surv_src, d_surv_codes, d_listat, d_rec, d_reccodes, d_reccnt, d_tilekeep, d_tileops, d_pre, d_exp, d_rank;
        Pinned                p_reccnt, p_rows; // p_rows: a range's finished rows on their way into the result
        Pinned                p_plan; // what the host reads of a device plan: [rank flag + probe windows][columns per lane][longest window] per wavefront
        std::vector<uint64_t> rec_codes;              // where the records' run-length codes begin (host copy)
        uint64_t              surv_total = 0, surv_cap = 0; // entries of d_surv_* that the pipeline's chunks have filled, and their room
        double                exp_lambda = 0;         // the scheme d_exp was made for
        uint32_t              exp_n      = 0;
        // _writeRecord's sort / unique / sort / cut on the device (lx_toprec.hip): the rows that stay and their code words, the step's
        // scratch, its counters (per range of a Level-2 call) and the rows of lx_postprocess_records_dev on their way up and down
        DevBuf                d_toprows, d_topcodes, d_topwork, d_topcnt, d_topin;
        DevBuf                d_cullqlen; // lx_postprocess_records_dev_ex: lx_cull_options::q_lens as 32-bit words
        Pinned                p_topcnt;
    } l2;
    // lx_bgzf_compress (lx_bgzf_host.cpp): one chunk's device buffers, its input in two pinned lanes, its members on the way out
    struct Bgzf
    {
        DevBuf d_in, d_slots, d_dist, d_sym, d_sizes, d_out, d_total;
        Pinned p_in[2], p_out, p_total;
    } bgzf;
    // lx_gunzip (lx_gunzip_host.cpp): one chunk of BGZF members on the device; its bytes, member table and status words in two pinned lanes
    struct Gunzip
    {
        DevBuf d_in, d_mem, d_status, d_out;
        Pinned p_in[2], p_mem[2], p_status[2];
        // a plain member in parallel (lx_pgunzip.hip): one wave's input, found bits + chunk results, symbol pool, windows, verified
        // chunks, bytes, the WaveResult (d_crc); slot 0's bit on its way up and the WaveResult on its way down in pinned blocks
        DevBuf d_pin, d_slots, d_sym, d_win, d_ver, d_bytes, d_crc;
        Pinned p_slots, p_crc;
        lx_gunzip_stats stats{}; // of the last lx_gunzip or lx_gunzip_stream_next call (lx_last_gunzip_stats)
        float           phase_ms[3] = {0, 0, 0};      // ... its find, decode and chain + resolve kernels (lx_last_phase_ms 101..103, 10 = all)
        int             phase_launches[3] = {0, 0, 0};
    } gunzip;
    // lx_render_bam_dev / lx_write_bam_dev (lx_bam_host.cpp): the call's inputs flattened on the device, what the kernels leave per
    // record, a range's stream (the carried part of a BGZF block in front), the tile totals on their way up
    struct Bam
    {
        DevBuf d_rows, d_ops, d_ascii, d_qual, d_ascii_off, d_qlens, d_qn_blob, d_qn_off, d_tax_off, d_tax_ids, d_grp_tab, d_name_blob, d_codon;
        DevBuf d_grp, d_grp_first, d_aux, d_size, d_off, d_scan, d_tiles, d_stream;
        Pinned p_tiles;
    } bam;
    // lx_render_text_dev / lx_write_text_dev (lx_text_host.cpp) use `bam` for what both writers read, and beside it: the columns, the
    // first words and lengths of the subjects the rows name and each row's index among them, the whole query ids and the constant
    // parts of the comment lines (.m9), the number texts of every record
    struct Text
    {
        DevBuf d_cols, d_row_s, d_slens, d_sn_off, d_sn_blob, d_qid_off, d_qid_blob, d_comment, d_nums;
    } text;
    uint64_t opt_bam_range = 0; // LX_OPT_BAM_RANGE_BYTES (0 = default)
    uint64_t opt_gunzip_chunk = 0; // LX_OPT_GUNZIP_CHUNK (0 = default)
    uint64_t opt_gunzip_from  = 0; // LX_OPT_GUNZIP_PARALLEL_FROM (0 = default)
    uint64_t opt_index_slice  = 0; // LX_OPT_INDEX_SLICE_WORDS (0 = the single sort)
    uint64_t opt_lca_range    = 0; // LX_OPT_LCA_RANGE_ROWS (0 = default)
    // lx_compute_lca_dev (lx_lca_host.cpp): a range's columns in two lanes (pinned and on the device), the query heads, the scan's
    // tile values, the LCA words and the error word of a range on their way down
    struct Lca
    {
        Pinned     p_in[2], p_out[2];
        DevBuf     d_in[2], d_out[2], d_first, d_tot;
        lxi::Event ev_up[2], ev_k[2];
    } lca;
    uint64_t gunzip_wave      = 0; // kOptGunzipWaveTest: chunks per wave (0 = default), so that a test reaches a wave's edges with a megabyte
    // lx_seed_queries (lx_seed_host.cpp): a call's queries, reads, decline flags, counters, the two scoring matrices, subjects the
    // caller handed in; the match block of the last freed result, kept for the next call
    struct Seed
    {
        DevBuf d_qres, d_qred, d_qoff, d_qlen, d_reads, d_declined, d_cnt, d_matrix, d_sres, d_spare;
    } seed;
    // lx_subject_mask_create_dev / lx_seed_result_filter (lx_taxfilter_host.cpp): the listed taxa and the two byte flags per taxon,
    // the scan's tile values, the counter and error words
    struct TaxFilter
    {
        DevBuf d_list, d_flags, d_tot, d_words;
    } taxfilter;
};

// what lx_seed_queries returns (lx_seed_host.cpp); lx_seed_result_filter (lx_taxfilter_host.cpp) compacts its list
struct lx_seed_result
{
    lx_handle *           h = nullptr; // NULL: a host-path result
    lxi::DevBuf           d_out;
    std::vector<lx_match> host;
    bool                  have_host = false;
    lx_seed_stats         st{};
};

// what lx_query_mask_create* return (lx_qmask_host.cpp); lx_seed_queries_masked (lx_seed_host.cpp) reads it.  One distance byte per
// letter (lx_qmask.h), indexed like the letters: on the host, on the handle's device, or both.
struct lx_query_mask
{
    lx_handle *                  h = nullptr; // NULL: on the host only
    std::vector<uint64_t>        off, len;    // the sequence table it was made for
    uint64_t                     extent = 0, n_letters = 0, n_masked = 0, n_seqs_masked = 0;
    mutable std::vector<uint8_t> dist;        // a device mask's comes down on first use
    mutable bool                 have_host = false;
    mutable std::mutex           down;        // (host_dist fills `dist` once)
    lxi::DevBlock<uint8_t>       d_dist;

    uint8_t const * host_dist() const; // NULL: the copy failed
    ~lx_query_mask();
};

namespace lxi
{

// not part of the ABI: lx_set_option takes it for the tests of lx_gunzip's waves (2..512 chunks per wave, 0 = default)
constexpr int kOptGunzipWaveTest = 1017;

int        fail(lx_handle * h, int code, char const * fmt, ...);
hipEvent_t pool_event(lx_handle * h);

// Wall-clock marks of the host-buffer entry points, printed when LX_HOST_TIMING is set (development aid).
struct HostMarks
{
    bool                                                               on;
    char const *                                                       what;
    std::chrono::steady_clock::time_point                              t0, last;
    std::string                                                        line;
    explicit HostMarks(char const * w) : on(lx::dev_aids().host_timing), what(w)
    {
        t0 = last = std::chrono::steady_clock::now();
    }
    void mark(char const * name)
    {
        if (!on)
            return;
        auto const now = std::chrono::steady_clock::now();
        char       buf[96];
        snprintf(buf, sizeof(buf), " %s %.1f", name, std::chrono::duration<double, std::milli>(now - last).count());
        line += buf;
        last = now;
    }
    ~HostMarks()
    {
        if (on)
            fprintf(stderr, "[lx host ms] %s:%s | total %.1f\n", what, line.c_str(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

// a bracket of phase p + kPhaseTimeOnly adds its time to phase p but is no launch of it (the sliced word table's counting pass: its
// launches are its slices)
constexpr int kPhaseTimeOnly = 1000;

// RAII-less phase bracket: records a start event now, the end event on close()
struct PhaseTimer
{
    lx_handle * h;
    hipStream_t s;
    int         phase;
    hipEvent_t  a = nullptr, b = nullptr;
    PhaseTimer(lx_handle * h_, hipStream_t s_, int phase_) : h(h_), s(s_), phase(phase_)
    {
        if (h->phase_ev.size() < 512)
        {
            a = pool_event(h);
            b = pool_event(h);
            if (a && b)
                (void)hipEventRecord(a, s);
        }
    }
    void close()
    {
        if (a && b)
        {
            (void)hipEventRecord(b, s);
            h->phase_ev.push_back({phase, a, b});
        }
    }
};

#define LX_HIP(h, call)                                                                                         \
    do                                                                                                          \
    {                                                                                                           \
        hipError_t _e = (call);                                                                                 \
        if (_e != hipSuccess)                                                                                   \
            return fail((h), _e == hipErrorOutOfMemory ? LX_ENOMEM : LX_EHIP, "%s failed: %s", #call,           \
                        hipGetErrorString(_e));                                                                 \
    } while (0)

int    bind(lx_handle * h);
// (bytes_adopt, set_output_error, cull_check, the writers' resolved request and header texts: lx_output_host.h)
// (lx_bgzf_host.cpp) lx_bgzf_compress's members of n bytes that stand on the device already (16-byte aligned): the same chunks of 512
// blocks, the same member bytes, the same download pipeline; `sink` takes each chunk's members in order.  The phase events of the
// call so far stay.
int bgzf_compress_dev(lx_handle * h, uint8_t const * d_in, uint64_t n, std::function<int(uint8_t const *, uint64_t)> const & sink);
int    check_async_error(lx_handle * h);
int    error_for_flag(lx_handle * h, uint32_t flag);

// The control words of lx_handle::d_ws_top, named in one place.  kWsBump and kWsError are adjacent: one copy or memset takes both.
enum WsWord
{
    kWsBump       = 0, // carry workspace: pairs handed out (every launch that carries starts from 0)
    kWsError      = 1, // the device's error word (error_for_flag)
    kWsMaxLens    = 2, // lx::MaxLens of launch_max_lens (two words)
    kWsOvfCount   = 4, // single sweep: overflow checkpoint slots handed out
    kWsWorkQueue  = 5, // checkpoint backtrace: the queue its persistent lanes take list positions from
    kWsStatBeyond = 6, // multi-query sweep: windows beyond the compact codes
    kWsWords      = 8
};
inline uint32_t * ws_word(lx_handle * h, WsWord w)
{
    return h->d_ws_top + w;
}
inline int32_t * ws_error(lx_handle * h)
{
    return reinterpret_cast<int32_t *>(ws_word(h, kWsError));
}

// ---- lx_step.cpp: the launchers of pass 1, pass 2 and the fused step; each follows a plan of lx_step_plan.h
// pairs_hint: carry pairs (8 bytes each) the call can need at most (a plan's carry_pairs(n)); the workspace grows to that (the
// device cannot grow it, it can only report)
int prepare_workspace(lx_handle * h, hipStream_t stream, uint64_t pairs_hint = 0);
// the device entry points' limits and the plans' options: the handle's options
ListLimits   option_limits(lx_handle const * h);
ScoreOptions score_options(lx_handle const * h);
TraceOptions trace_options(lx_handle const * h);
// pass 1 over a device list as `pl` says; band_diag: band mode's centres, indexed like the list (NULL: the default diagonal)
int launch_score_list(lx_handle * h, int slot, void const * d_q, void const * d_s, void const * d_ext, uint64_t n, void * d_out,
                      ScorePlan const & pl, hipStream_t stream, int32_t const * band_diag);
// ... planned from the list's limits (phase 0 of the phase list; ev0 / ev1 and the carry workspace are the caller's)
int score_dev_impl(lx_handle * h, int slot, void const * d_q, void const * d_s, void const * d_ext, uint64_t n, void * d_out,
                   hipStream_t stream, ListLimits const & lim);

// padding of q/s staging buffers so that clamped / prefetching loads never leave the allocation
constexpr size_t kSlack = 256;
constexpr uint64_t kExtendChunk = 640ull << 10; // extensions per chunk of lx_extend_batch's pipeline unless LX_OPT_EXTEND_CHUNK says otherwise

// Subject side of a host-buffer call: either the caller's buffer, uploaded into d_s, or -- s_res == NULL, s_bytes == 0
// after lx_set_subjects -- the resident copy.
struct SubjectRef
{
    void *   dev   = nullptr;
    uint64_t bytes = 0;
    bool     upload = false;
};

int resolve_subjects(lx_handle * h, uint8_t const * s_res, uint64_t s_bytes, SubjectRef & out);

// lx_extend_batch's additions to the fused step: ops slots of one size instead of an offset per extension, the survivors'
// ops run-length packed into a dense stream (lx_pack.hip), a copy of the survivor list's original indices
struct FusedExtra
{
    uint64_t             ops_stride = 0;
    uint8_t *            d_rle      = nullptr;
    unsigned long long * d_rle_top  = nullptr;
    uint64_t             rle_cap    = 0;
    uint32_t *           d_src_out  = nullptr; // [survivor list capacity]
    uint32_t *           d_rle_len  = nullptr; // [survivor list capacity]: code bytes per position
};

int align_dev_impl(lx_handle * h, int slot, void const * d_q, void const * d_s, lx::Extension const * d_ext, uint64_t n, lx::Hsp * d_hsp,
                   uint8_t * d_ops, uint64_t const * d_ops_off, hipStream_t stream, ListLimits const & lim, int share_slots,
                   uint32_t const * d_src = nullptr, uint64_t const * d_count = nullptr, int32_t const * d_score_in = nullptr,
                   bool by_pos = false, uint64_t ops_stride = 0);

// lx_extend_batch's multi-query chunks: the chunk's slots BY WAVEFRONT (lx::WfSlots, lx_device.h) instead of by region: `dev` = the
// table of the chunk's wavefronts on the device; the slots of the wavefronts before slot n0 take dw0 uint32 at the trace buffer's start,
// room for ovf_cap int16-pair overflow slots follows, then the dw1 uint32 of the wavefronts from n0 on.  part: 0 = the chunk in one
// call, 1 = the first of two calls (sweep of the slots before n0, nothing else), 2 = the second (sweep of the rest, then what follows
// a sweep, over all slots).  total_dw: what the trace buffer must hold (fixed by the first call).
struct MqTab
{
    void const * dev = nullptr;
    uint64_t     n0 = 0, dw0 = 0, dw1 = 0, ovf_cap = 0, total_dw = 0;
    int          part = 0;
};

// One call of the fused step (fused_impl): the list and its outputs, what the caller states about the list, and what the chunk
// pipeline of lx_extend_batch adds.  by_pos: records and ops offsets are indexed by the position in the survivor list instead of by
// extension.
struct StepCall
{
    void const * d_q = nullptr, *d_s = nullptr, *d_ext = nullptr;
    uint64_t     n = 0;
    void const * d_min_score   = nullptr;
    int32_t      min_score_all = 0;
    void *       d_out_score = nullptr, *d_out_hsp = nullptr, *d_out_ops = nullptr;
    void const * d_ops_off   = nullptr;
    void *       d_out_count = nullptr;
    hipStream_t  stream      = nullptr;
    bool         by_pos      = false;
    FusedExtra   fx;
    ListLimits   lim;
    MqTab        tab;                 // (dev == NULL: slots by region)
    lx::Geo      mq_geo;              // the strip geometry the call chose for its chunks ({}: plan_step picks per chunk)
    bool         mq_wide     = false; // the multi-query sweep writes int16-pair slots (many windows of the last chunks scored beyond the compact codes)
    bool         keep_events = false; // the phase events of earlier steps stay (lx_extend_batch: lx_last_phase_ms sums its chunks')
};
int fused_impl(lx_handle * h, int slot, StepCall const & c);

// what stands on the device already when the Level-2 driver (lx_level2_host.cpp) calls the extension pipeline
struct ResidentInput
{
    void const * d_q       = nullptr; // query residues
    uint64_t     q_bytes   = 0;
    void const * d_ext_all = nullptr; // the caller's list (lx::Extension) and its cut-offs, in the order of the host's copies
    void const * d_min_all = nullptr;
    // a plan made on the device (the solo packing): the slot list (16 per wavefront: position in the list, bit 31 = filler), and
    // on the host per wavefront the columns per lane its widest query sweeps and its longest window, the strip geometry
    // (which the caller sets), the list's cells
    uint32_t const * d_plan  = nullptr;
    uint64_t         nwf     = 0;
    uint32_t const * wf_pan  = nullptr;
    uint32_t const * wf_maxs = nullptr;
    lx::Geo          mq_geo;
    bool             free_packing = false; // the device plan is the free packing (pairs of one query, at most four queries per wavefront), not the solo one
    uint64_t         cells   = 0;
    // the survivors stay on the device (lx_handle::Level2::d_surv_*; taken where the plan above is served: ResidentSurvivors says so),
    // the scores too (h->d_score_all); want_codes: their run-length codes come down into the handle's code bytes
    bool keep_on_device = false, want_codes = true;
    // Records chunk by chunk (lx_level2_host.cpp): the plan's chunks are RANGES of the query-sorted window list (cut_wf: the wavefront
    // each range begins with, n_ranges + 1 entries), so a chunk's survivors are a contiguous piece of the result -- `enqueue` queues
    // the records kernels behind the chunk's own (its survivor list stands in the lane's buffers: no copy), `collect` is called when
    // they are through, while the NEXT chunk computes: rows and columns of all but the last range come down beside the sweeps.
    struct ChunkRecords
    {
        uint64_t const * cut_wf   = nullptr;
        uint64_t         n_ranges = 0;
        std::function<int(uint64_t range, void const * d_hsp, void const * d_src, void const * d_count, uint64_t cap)> enqueue;
        std::function<int(uint64_t range, uint64_t code_base, bool gpu_busy)>                                         collect; // gpu_busy: another chunk computes meanwhile
    };
    ChunkRecords const * chunk_records = nullptr;
    uint64_t             bs_rule       = 0; // the backtrace's match rule (bisulfite lists: 1, whatever the handle's LX_OPT_BS_MATCH_RULE says)
};
// band mode's plain path of the host-buffer entry points (lx_host_batch.cpp; what: 0 = scores, 1 = alignments of known scores, 2 = both)
int  host_banded(lx_handle * h, int slot, int what, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                 lx_extension const * ext, uint64_t n, int32_t const * known_score, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                 lx_hsp * out_hsp, uint8_t * caller_ops, uint64_t const * caller_ops_off, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes);
bool solo_plan_applies(lx_handle const * h, int slot);
bool free_plan_applies(lx_handle const * h, int slot);
// where extend_list_resident left the call's survivors: in `out` on the host, or in lx_handle::Level2::d_surv_* as one list of
// `total` entries, or -- handed to ResidentInput::ChunkRecords range by range -- with their records made already
struct ResidentSurvivors
{
    enum Where
    {
        kOnHost,
        kOnDevice,
        kOnDeviceByRange
    } where = kOnHost;
    uint64_t total = 0;
};
int  extend_list_resident(lx_handle * h, int slot, ResidentInput const & ri, lx_extension const * ext, uint64_t n, int32_t const * min_score,
                         int32_t * out_score, lx_survivor_list * out, ResidentSurvivors * where);

// [off, off + len) inside a buffer of `bytes`, written so that offsets near 2^64 cannot wrap past the test
inline bool lx_slice_ok(uint64_t off, uint64_t len, uint64_t bytes)
{
    return len <= bytes && off <= bytes - len;
}


} // namespace lxi
