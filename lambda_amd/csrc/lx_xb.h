// lx_xb.h -- the chunk pipeline of lx_extend_batch* (not part of the ABI): what extend_pipeline (lx_host.cpp) sets up per call and
// the two chunk drivers share -- the call's constants, the two lanes (lx_xb_core.cpp), the places results go (lx_xb_sinks.cpp).  The
// drivers: lx_xb_run.cpp cuts the ordered list into chunks for the one-query-per-wavefront kernels and pads runs on the host,
// lx_xb_wf.cpp cuts the plan's wavefronts into chunks for the multi-query sweep and gathers on the device.
#pragma once
#include "lx_internal.h"

namespace lxi
{

using Clock = std::chrono::steady_clock;
inline Clock::time_point now() { return Clock::now(); }
inline double            ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

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

struct XbPrep // what the host keeps about a chunk until its results are back
{
    uint64_t              k0 = 0, k1 = 0; // positions in the ordered list (multi-query chunks: wavefronts of the plan)
    uint64_t              slots = 0, cap_sel = 0;
    bool                  wide = false;   // multi-query chunk: the sweep wrote int16-pair slots
    uint64_t              exec_cells = 0, max_s = 0, max_pan = 0; // (LX_HOST_TIMING: what the chunk's wavefronts execute)
    uint64_t              range = 0;      // records chunk by chunk (ResidentInput::ChunkRecords): the range this chunk is
    std::vector<uint32_t> slot_src;       // original index of every slot (0xffffffff = padding)
};

// Where a call's results go, decided once in extend_pipeline -- and, for the device forms, where the multi-query plan is known
// (device_sink).  codes: the ops are run-length codes, not column bytes (the list's always are; on the device: they come down at all)
struct XbSink
{
    enum Where
    {
        kRows,         // the caller's arrays, a row per extension
        kList,         // the handle's survivor list
        kDevice,       // lx_handle::Level2::d_surv_*, one list per call
        kDeviceByRange // the lanes' buffers, handed to ResidentInput::ChunkRecords range by range
    } where    = kRows;
    bool codes = false;
    bool on_device() const { return where == kDevice || where == kDeviceByRange; }
};

// The device half of a call: its constants and the two lanes the host plan (h->plan) is run in as chunks.
struct Xb
{
    lx_handle * const           h;
    int const                   slot;
    lx_extension const * const  ext; // the caller's list, cut-offs and outputs
    uint64_t const              n;
    int32_t const * const       min_score;
    int32_t const               min_score_all;
    int32_t * const             out_score;
    lx_hsp * const              out_hsp;
    uint64_t * const            out_ops_off;
    ResidentInput const * const ri;
    bool const                  preplanned;
    HostPlan const &            p;
    HostMarks &                 hm;
    unsigned const              nthreads;
    uint64_t const              bs_rule; // the backtrace's match rule
    XbSink                      sink;
    void const *                d_q = nullptr, *d_s = nullptr; // query and subject residues on the device
    XbPrep                      prep[2];                       // the two lanes
    bool                        in_flight[2] = {false, false};
    int                         c            = 0; // chunks issued
    uint64_t                    chunk_target = 0, ops_total = 0; // (ops_total: bytes handed out in h->ext_bytes so far)
    bool                        list_uploaded = false;
    double t_upload = 0, t_prep = 0, t_issue = 0, t_wait = 0, t_unpack = 0, t_u1 = 0, t_u2 = 0; // LX_HOST_TIMING: where the host's time goes

    Xb(lx_handle * h_, int slot_, lx_extension const * ext_, uint64_t n_, int32_t const * min_score_, int32_t min_score_all_, int32_t * out_score_,
       lx_hsp * out_hsp_, uint64_t * out_ops_off_, XbSink sink_, ResidentInput const * ri_, HostMarks & hm_)
        : h(h_), slot(slot_), ext(ext_), n(n_), min_score(min_score_), min_score_all(min_score_all_), out_score(out_score_), out_hsp(out_hsp_),
          out_ops_off(out_ops_off_), ri(ri_), preplanned(ri_ && ri_->d_plan), p(h_->plan), hm(hm_), nthreads(host_threads(n_)),
          bs_rule(ri_ ? ri_->bs_rule : h_->opt_bs_rule), sink(sink_)
    {
    }

    // ---- lx_xb_core.cpp
    // the caller's list and cut-offs onto the device (pinned staging, filled by the host threads; scores in caller order zeroed)
    int upload_list();
    // the plan as chunks, by the driver it was made for; the call's ops are h->ext_bytes[0, ops_total) then
    int run(void const * d_q_, void const * d_s_);
    // lane L's device buffers: `slots` slots (+ caller indices: orig), prep[L].cap_sel survivors with ops slots of `stride` bytes, counts
    int size_lane(int L, uint64_t slots, uint64_t stride, bool orig, bool mq);
    // the fused step over lane L's first `slots` slots, on the kernel stream: what it may assume of the chunk -- its widest query, its
    // longest window, its query run (1: the solo packing, 2: the free packing) -- and, for multi-query chunks, its slots by wavefront
    // and whether the sweep writes int16-pair slots
    int run_fused(int L, uint64_t slots, uint64_t stride, uint64_t max_q, uint64_t max_s, uint64_t run, MqTab const & tab = MqTab{}, bool wide = false);
    // behind a chunk's kernels: its error word (words = 5: and its windows beyond the compact codes) saved beside its counts, (by
    // range) the records kernels of its range, the counts -- and lane_scores scores by slot -- on their way down; the chunk is in flight
    int send_counts(int L, uint64_t words, uint64_t lane_scores = 0);
    // lane L's counts have arrived (the chunk is no longer in flight, whatever they say)
    int wait_counts(int L, uint64_t const *& cnt);
    // the chunk's error word and survivor count; the share that survived steers the adaptive pass-2 mode of the next chunks (fused_impl)
    int check_counts(XbPrep const & pr, uint64_t const * cnt);
    // the survivors' records, list positions, code lengths and codes into lane L's pinned staging
    int download_survivors(int L, uint64_t count, uint64_t nrle);
    // the lanes' chunks still in flight, oldest first
    template <typename Collect>
    int drain(Collect && collect)
    {
        int rc;
        for (int L : {c & 1, (c & 1) ^ 1})
            if (in_flight[L] && (rc = collect(L)))
                return rc;
        return LX_OK;
    }
};

// ---- the drivers
int run_chunks_of_runs(Xb & x);       // lx_xb_run.cpp: chunks = ranges of the ordered list
int run_chunks_of_wavefronts(Xb & x); // lx_xb_wf.cpp: chunks = ranges of the plan's wavefronts, + the redo of chunks whose overflow area filled up

// ---- the sinks (lx_xb_sinks.cpp); t1: when the chunk's survivors had come down
// rows: every row "no alignment" (beside the first multi-query chunk's kernels)
void rows_clear(Xb & x);
// rows: lane L's chunk by slot -- score and record of every extension (x.prep[L].slot_src says whose), the survivors' ops
int rows_of_slots(Xb & x, int L, uint64_t count, Clock::time_point t1);
// rows: lane L's survivors, addressed by caller index (the device translated the list)
int rows_of_survivors(Xb & x, int L, uint64_t count, Clock::time_point t1);
// rows and list, multi-query path: the scores of every extension come back once, in caller order, at the end of the call
int scores_in_caller_order(Xb & x);
// list: lane L's survivors appended to the handle's result buffers, its codes to h->ext_bytes
int list_append(Xb & x, int L, uint64_t count, uint64_t nrle, uint32_t const * slot_src /* NULL: the device translated */);
// device: room for every chunk's survivor list, padding included; x.sink becomes kDevice (by_range: kDeviceByRange)
int device_sink(Xb & x, bool by_range);
// device: lane L's survivor list joins the call's (by range: the range's rows and columns are collected), its codes come down
int device_collect(Xb & x, int L, uint64_t count, uint64_t nrle, Clock::time_point t0, Clock::time_point t_ev);

} // namespace lxi
