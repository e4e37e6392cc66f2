// lx_level2_host.h -- what the files of the Level-2 driver share: lx_level2_host.cpp (the resident sets, the list work, a call stage
// by stage), lx_level2_records.cpp (RecordsJob: the records made on the device, and _writeRecord's cut for rows in host memory) and
// lx_level2_reserve.cpp (lx_reserve).  The buffer sizes of a call stand here once each: the call and lx_reserve ask the same function.
#pragma once
#include <cmath>

#include "lx_internal.h"
#include "lx_level2.h"
#include "lx_toprec.h"

#include "host/lx_iterate_common.hpp"

namespace lxi
{

template <class T>
int upload(lx_handle * h, DevBuf & b, std::vector<T> const & v)
{
    int rc = ensure(h, b, v.size() * sizeof(T) + 16);
    if (rc)
        return rc;
    if (!v.empty())
        LX_HIP(h, hipMemcpyAsync(b.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return LX_OK;
}

inline uint64_t bits_below(uint64_t count) // mask of the bits a value in [0, count) can have set
{
    if (count <= 1)
        return 0;
    uint64_t m = 1;
    while (m < count - 1 && m != ~0ull)
        m = (m << 1) | 1;
    return m;
}

// what lx_iterate_matches_dev_top asks of a call: the cut, and where the parts' lx_record_stats add up (done: the step ran on
// the device for every record of the result; else the caller runs it on the finished result)
// lx_cull_options as the kernels take them (lx_cull.h): the lengths in device memory as 32-bit words, query n_qid's at
// d_q_lens[n_qid * stride]; where the parts' lx_cull_stats add up
struct CullRequest
{
    uint64_t         max_hsps = 0, culling_limit = 0;
    uint32_t const * d_q_lens = nullptr;
    uint64_t         q_lens_n = 0;
    uint32_t         stride   = 1;
    int              translated = 0;
    lx_cull_stats    stats{};

    void set(lx::TopParams & tp) const
    {
        tp.max_hsps = max_hsps, tp.culling_limit = culling_limit;
        tp.q_lens = d_q_lens, tp.q_lens_n = q_lens_n, tp.q_len_stride = stride, tp.q_translated = translated;
    }
};

struct TopRequest
{
    uint64_t        max_matches = 0;
    lx_record_stats stats{};
    bool            done = false;
    CullRequest     cull{};
};

// src/search_misc.hpp:46-50
inline int64_t bandSize(uint64_t const seqLength)
{
    return static_cast<int64_t>(std::sqrt(seqLength)) + 1;
}

constexpr size_t kPlanProbe  = 128;                                                              // l2.p_plan: [rank flag: 64 B][the free-packing plan's report: 64 B][probe windows] ...
constexpr size_t kPlanProbes = lx::kFpMaxRanges;                                                 // cuts a part's ranges may have: 512 probe windows each
constexpr size_t kPlanHead   = kPlanProbe + kPlanProbes * kL2ProbeWindows * sizeof(lx::L2Window); // ... in front of the per-wavefront arrays

// ---- buffer sizes that the call and lx_reserve share: one place per group -------------------------------------------------------
// the sort words of n matches and the list work's counters (level2_keys, iterate_host_list_on_device)
int ensure_list_keys(lx_handle * h, uint64_t n);
// what sort, merge, unique and the slices of n matches take beside the sort words (level2_windows); cut_entries: the cut-off table's
int ensure_list_work(lx_handle * h, uint64_t n, size_t cut_entries);
// a device plan of up to cap_wf wavefronts: its slots, and per wavefront the columns per lane and the longest window (+ the
// free-packing plan's report behind them)
int ensure_plan(lx_handle * h, uint64_t cap_wf);
// the records kernels' buffers: `rows` records and their code words, the windows of the largest range, survivor lists of up to
// max_entries entries (a tile per 256), counters for nr ranges on the device and nr_pinned on their way down
int ensure_records(lx_handle * h, uint64_t rows, uint64_t max_win, uint64_t max_entries, uint64_t nr, uint64_t nr_pinned);
// _writeRecord's cut on the device (lx_toprec.hip): `rows` rows that stay, scratch for ranges of up to max_win rows, counters for nr ranges
// (cull: NULL, or the options whose kernels the ranges' launches will add)
int ensure_top_records(lx_handle * h, uint64_t rows, uint64_t max_win, uint64_t nr, CullRequest const * cull = nullptr);
// The counters of the cut's kernels (tc: [lx::kTopCounters]) over nrec records whose columns are max_ops at most: checked, and added
// to *stats (and to *cull_stats, unless NULL)
int top_account(lx_handle * h, uint64_t const * tc, uint64_t nrec, uint64_t max_ops, lx_record_stats * stats, lx_cull_stats * cull_stats = nullptr);
// _writeRecord's sort / unique / sort / cut for rows in host memory: up, the kernels of lx_toprec.hip, the rows that stay down
// (cull: NULL, or the two rules of lx_cull.h with the lengths already in device memory; its stats are set, not added to)
int toprec_host_rows(lx_handle * h, lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_record_stats * stats, uint64_t * out_n, CullRequest * cull = nullptr);

// The tail of iterateMatchesFullSimd (src/search_algo.hpp:1287-1325) for a part of the window list whose survivors the extension
// pipeline left on the device: statistics, order, identity cut-off, records as kernels (lx_records.hip), then ONE copy of finished
// lx_blast_match rows into the result and the alignment columns expanded from the run-length codes by the host threads.  What
// host/lx_iterate_common.hpp's finishSurvivors does for lists in host memory, with the same results to the bit.
// A part is served as ONE range behind its last chunk (the survivors of all chunks in lx_handle::Level2::d_surv_*), or -- where the
// plan's chunks are ranges of the query-sorted list (ResidentInput::ChunkRecords) -- range by range: a range's kernels are queued
// behind its chunk's own, its rows and columns come down while the next chunk computes.
struct RecordsJob
{
    struct Range
    {
        uint64_t lo = 0, hi = 0;   // windows of the part
        uint64_t code_base = 0;    // where the chunk's codes begin in h->ext_bytes
        bool     done = false;
    };
    lx_handle *              h;
    lx_search_params const * params;
    lx_iterate_result *      res;
    HostMarks &              hm;
    uint64_t                 part_lo, n_part;
    std::vector<Range>       ranges;
    uint64_t                 next_flush = 0;
    lx::RecParams            base{};
    uint64_t                 pair_bits = 0, s0_bits = 0;
    bool                     want_ops  = true;
    std::vector<double>      pre_host; // the e-value factors per distinct length, until their upload is through
    bool                     use_rank = false; // the survivors are sorted by their windows' ranks (l2.d_rank: rec_launch_rank over the part)
    // lx_iterate_matches_dev_top: every range's rows go through _writeRecord's sort / unique / sort / cut (lx_toprec.hip) behind its
    // records kernels; what stays -- rows and code words in l2.d_toprows / d_topcodes -- is what comes down
    TopRequest *             top = nullptr;

    RecordsJob(lx_handle * h_, lx_search_params const * p_, lx_iterate_result * r_, HostMarks & hm_, uint64_t part_lo_, uint64_t n_part_)
        : h(h_), params(p_), res(r_), hm(hm_), part_lo(part_lo_), n_part(n_part_)
    {
    }

    // the host's share of the arithmetic, made once per call with the host's libm -- per distinct e-value length the factor
    // K * (ql - adj) * (dl - adj) of computeEValue (blast_stats.hpp), exp(-lambda s) for every score until it is zero, the bit-score
    // test as an integer cut-off -- and the buffers (entries: upper bound of the survivor entries of any range; every range has its
    // own rows in d_rec: at most as many as it has windows)
    int prepare(lambda_amd::CutOffs & cutOffFor, std::vector<Range> rs, uint64_t max_entries, uint64_t max_wlen = 0 /* longest window of the part, 0 = unknown */);
    // the kernels of range r over a survivor list of up to `cap` entries (count_ptr: how many are filled, NULL = all; codes_off: where
    // each entry's codes begin, NULL = the alignment's own offset inside its chunk), on the handle's stream; the counters follow
    int enqueue(uint64_t r, void const * d_hsp, void const * d_src, void const * d_count, void const * d_codes_off, uint64_t cap);
    // range r's kernels are through (the caller synchronised with them): every range up to the first unfinished one goes to the result
    int collect(uint64_t r, uint64_t code_base, bool gpu_busy);

private:
    int flush(uint64_t r, bool gpu_busy); // range r's counters checked and added up, its rows and columns into the result
};

} // namespace lxi
