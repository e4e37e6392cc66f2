// lx_level2_plan.h -- the Level-2 driver's range plan (lx_level2_host.cpp): into how many ranges a query-sorted window list is cut,
// where the cuts are looked for and where they fall, and which strip geometry sweeps the list.  Pure integer work on plain arrays: no
// HIP in here, so that tests/native/level2_plan_check.cpp can hold it against a restatement without a device or the library.
// level2_sorted_tail (lx_level2_host.cpp) and lx_reserve (lx_level2_reserve.cpp) both ask l2_range_count: the rule stands here and nowhere else.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lx_geo.h"

namespace lx
{

// One DP window after widen + merge + unique: what the reference's span holds when _widenAndPreprocessMatches returns
// (qryStart = 0 and qryEnd = the query's length are implied).
struct L2Window
{
    uint32_t q, s;     // frame-expanded ids
    uint64_t beg, end; // subjStart, subjEnd
};
static_assert(sizeof(L2Window) == 24, "L2Window layout");

constexpr uint32_t kFpMaxRanges = 8; // ranges a plan is laid out in at most: what the plan kernels (lx_level2.h: FpArgs) and the probe block take

} // namespace lx

namespace lxi
{

// ---- the range count ------------------------------------------------------------------------------------------------------------
// Ranges of the query-sorted list, each planned by itself and served as one chunk of the pipeline: a range's records are made
// behind its chunk and come down while the next range computes (RecordsJob).
// (measured on 1.25 M windows, bench.py --iterate: 1 range 11.8, 2 ranges 10.8-11.4, 3 ranges 11.3-11.9, 4 ranges 11.9 ms: a
// range costs a sweep's tail, a backtrace's tail and the records kernels' thirty launches; the protein list of bench.py --iterate
// --config 1, 3.2 M windows: 1 range 29.1, 2 ranges 24.6, 3 ranges 24.9, 4 ranges 25.5 ms)
constexpr uint64_t kL2OneRangeBelow     = 300000;  // windows below which a list is one range
constexpr uint64_t kL2WindowsPerRange   = 4000000; // from there on two ranges, and one more per this many windows ...
constexpr uint64_t kL2MaxRangesBySize   = 4;       // ... up to this many
// ... but a range's checkpoint slots stand in HBM together, and FRESH device memory is dear: 40 ms per GB the first time a
// process touches it (tools/dev/malloc_probe: hipMalloc of 12 / 32 GB 0.6 / 1.3 s) -- 1.3 s for the two ranges of the protein
// list above against a call of 25 ms.  So the ranges also fit what the handle holds already, or 8 GiB: a search's one call
// pays 0.3 s instead, a handle whose slots are larger (LX_OPT_TRACE_BYTES-sized by earlier calls) keeps the fewer ranges.
constexpr uint64_t kL2FreshSlotBytes    = 8ull << 30;
// (two ranges: the first one two thirds of the windows -- what follows the LAST range's kernels, its rows on the PCIe link and
// its columns, is nobody's shadow, while the first range's comes down beside the second's kernels as long as those
// take longer; bench.py --iterate, fastest of eight calls at 50 / 62 / 66 / 70 / 75 / 80 %: 10.7 / 10.55 / 10.5 / 10.5 /
// 10.9 / 11.4 ms)
constexpr uint64_t kL2FirstOfTwoPercent = 66;
// (lx_reserve sizes the larger of two ranges before the list exists, and asks for two points more than the share.  Slack, not a second
// opinion about the split: both figures came with one change.  A cut falls behind its mark, never in front of it, and a plan's
// wavefronts are not spread over the ranges exactly as its windows are)
constexpr uint64_t kL2ReserveSlackPercent = 2;

// the count by the list's size alone
inline uint64_t l2_ranges_by_size(uint64_t n)
{
    return n < kL2OneRangeBelow ? 1 : std::min<uint64_t>(kL2MaxRangesBySize, n / kL2WindowsPerRange + 2);
}

// what the checkpoint slots of n windows take when a slot of the list's LONGEST window takes slot_bytes
// (every slot sized for the LONGEST window: an upper bound -- slots are laid out wavefront by wavefront; ordinary windows
// are a half to a third of a merged one: half of it per slot is what a list takes at most)
inline uint64_t l2_slot_need_bytes(uint64_t n, uint64_t slot_bytes)
{
    return (n + n / 8) * (slot_bytes / 2 + 1);
}

// The ranges of a list of n windows.  records_on_device: else the host threads make the records from the whole list (one range);
// forced: LX_L2_RANGES (lx_aids.h), 0 = by the rule; need_bytes: what the list's checkpoint slots take (l2_slot_need_bytes),
// have_bytes: what the handle may use for one range's (> 0).
inline uint64_t l2_range_count(uint64_t n, bool records_on_device, uint64_t forced, uint64_t need_bytes, uint64_t have_bytes)
{
    if (!records_on_device)
        return 1;
    if (forced)
        return std::min<uint64_t>(forced, lx::kFpMaxRanges); // (LX_L2_RANGES may ask for more)
    return std::min<uint64_t>(lx::kFpMaxRanges, std::max<uint64_t>(l2_ranges_by_size(n), (need_bytes + have_bytes - 1) / have_bytes));
}

// ---- where the cuts are looked for ----------------------------------------------------------------------------------------------
// The cuts stand where the true query id changes (the result is ordered by it): the windows around n / R, 2 n / R, ... come down
// for that, 12 KB each.
constexpr uint64_t kL2ProbeWindows = 512; // windows of a probe: 256 on either side of its target

struct L2Probe
{
    uint64_t target, from, upto; // the cut is looked for in [max(target, from + 1), upto) of windows [from, upto)
};

// the probes of R ranges over n windows (a probe that would overlap the one before it is dropped)
inline std::vector<L2Probe> l2_probe_targets(uint64_t n, uint64_t R)
{
    uint64_t const      half = kL2ProbeWindows / 2;
    std::vector<L2Probe> probes;
    for (uint64_t k = 1; k < R && probes.size() < lx::kFpMaxRanges; ++k)
    {
        uint64_t const target = R == 2 ? n / 100 * kL2FirstOfTwoPercent : n * k / R, from = target > half ? target - half : 0, upto = std::min(n, target + half);
        if (upto - from >= 2 && (probes.empty() || from >= probes.back().upto))
            probes.push_back(L2Probe{target, from, upto});
    }
    return probes;
}

// The ranges' bounds {0, cut, ..., n} from the probes' windows (probe k's window `from + i` stands in win[kL2ProbeWindows * k + i]):
// a cut is the first position at or behind the target where the true query id (q / q_frames) changes, kept where it lies
// strictly inside (the cut before it, n) -- a probe inside one long query finds none, and its range merges with the next.
inline std::vector<uint64_t> l2_cuts(lx::L2Window const * win, std::vector<L2Probe> const & probes, uint64_t n, uint32_t q_frames)
{
    std::vector<uint64_t> bounds(1, 0);
    for (size_t k = 0; k < probes.size(); ++k)
    {
        lx::L2Window const * const pw   = win + kL2ProbeWindows * k;
        uint64_t const             from = probes[k].from, upto = probes[k].upto;
        uint64_t                   cut  = 0;
        for (uint64_t w = std::max<uint64_t>(probes[k].target, from + 1); w < upto && !cut; ++w)
            if (pw[w - from].q / q_frames != pw[w - from - 1].q / q_frames)
                cut = w;
        if (cut && cut > bounds.back() && cut < n)
            bounds.push_back(cut);
    }
    bounds.push_back(n);
    return bounds;
}

// ---- the strip geometry ---------------------------------------------------------------------------------------------------------
// ONE strip geometry per call, the one that sweeps the list cheapest (lx_host.cpp has the measurement behind "one" and behind
// the 15 % that narrower strips must save): cost[k] = the list's cost at 19 / 13 / 11 columns per lane, compared as doubles.  The
// host plan of lx_extend_batch (HostPlan::choose_cfg, sums of doubles) and the Level-2 driver (sums of uint64) decide by this function.
constexpr double kL2NarrowStripsMustSave = 1.15;

template <class Cost>
lx::Geo choose_strips(Cost const * cost)
{
    lx::Geo const cand[3] = {{8, 19}, {8, 13}, {8, 11}};
    lx::Geo       geo     = cand[0];
    double        best    = 1e300;
    for (int k = 0; k < 3; ++k)
    {
        double const c = (double)cost[k] * (k == 0 ? 1.0 : kL2NarrowStripsMustSave);
        if (c < best)
        {
            best = c;
            geo  = cand[k];
        }
    }
    return geo;
}

// ... as the columns per lane of the strips chosen (what tests/native/level2_plan_check.cpp answers a cfg request with)
inline int l2_choose_cfg(uint64_t const cost[3])
{
    return choose_strips(cost).c;
}

} // namespace lxi
