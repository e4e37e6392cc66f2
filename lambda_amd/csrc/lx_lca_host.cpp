// lx_lca_host.cpp -- lx_tax_dev_* and lx_compute_lca_dev: the LCA step of _writeRecord (src/search_algo.hpp:884-907, computeLCA:
// src/search_misc.hpp:86-112) with its fold as kernels (lx_lca.hip).  lx_compute_lca_ex (host/lx_postprocess.cpp) is the specification.
//
// The tree goes up once (lx_tax_dev_create, after lx_check_tax_tree) and stays: {parent, height} per taxon, the subjects' taxon lists.
// A call checks every row on the host threads (n_sid, and the bit score where the top-percent rule is on) before anything touches
// the device, cuts the list into ranges of whole queries of at most LX_OPT_LCA_RANGE_ROWS rows and serves them through two lanes:
// the host threads gather a range's columns (n_qid, n_sid as 32 bits, bit_score if needed) into a pinned lane while the kernels of
// the range before it run, the lane goes up on the handle's upload stream, the kernels follow on its launch stream, and one uint32
// per query plus the range's error word come down behind them.  out_qid is filled from the heads the gather meets.
#include "lx_host_pool.h"
#include "lx_internal.h"
#include "lx_lca.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace lxi;

// its handle's device bound and the launch stream through before the blocks go
lx_tax_dev::~lx_tax_dev()
{
    if (h && bind(h) == LX_OK)
        (void)hipStreamSynchronize(h->stream);
}

namespace
{

constexpr uint64_t kDefaultRangeRows = 1ull << 24;
constexpr char     kNoRoot[]         = "LCA-computation error: One of the paths didn't lead to root.";

struct Range
{
    uint64_t lo, hi;
};

// ranges of whole queries of at most `cap` rows; a query with more rows is a range of its own
std::vector<Range> cut_ranges(lx_blast_match const * m, uint64_t n, uint64_t cap)
{
    std::vector<Range> out;
    for (uint64_t lo = 0; lo < n;)
    {
        uint64_t hi = std::min(n, lo + cap);
        if (hi < n)
        {
            while (hi > lo && m[hi].n_qid == m[hi - 1].n_qid)
                --hi;
            if (hi == lo) // (the query at lo has more than cap rows)
                for (hi = lo + 1; hi < n && m[hi].n_qid == m[lo].n_qid;)
                    ++hi;
        }
        out.push_back(Range{lo, hi});
        lo = hi;
    }
    return out;
}

// where a range's columns stand in a lane of `rows` rows
struct LaneView
{
    uint64_t * qid;
    double *   bits; // NULL: not needed
    uint32_t * sid;
    size_t     bytes;
    static size_t size(uint64_t rows, bool with_bits) { return (size_t)(rows * (with_bits ? 20 : 12)); }
    LaneView(void * base, uint64_t rows, bool with_bits)
    {
        uint8_t * const b = static_cast<uint8_t *>(base);
        qid               = reinterpret_cast<uint64_t *>(b);
        bits              = with_bits ? reinterpret_cast<double *>(b + rows * 8) : nullptr;
        sid               = reinterpret_cast<uint32_t *>(b + rows * (with_bits ? 16 : 8));
        bytes             = size(rows, with_bits);
    }
};

struct Flight
{
    bool     on = false;
    uint64_t nq = 0, at = 0; // queries of the range, where its words go in out_lca
};

} // namespace

extern "C" {

int lx_tax_dev_create(lx_handle * h, lx_tax_tree const * tree, lx_tax_dev ** out)
{
    if (!h)
    {
        set_output_error("lx_tax_dev_create: h == NULL");
        return LX_EINVAL;
    }
    if (!tree || !out)
        return fail(h, LX_EINVAL, "lx_tax_dev_create: NULL argument");
    *out = nullptr;
    if (lx_check_tax_tree(tree) != LX_OK)
        return fail(h, LX_EINVAL, "lx_tax_dev_create: %s", lx_last_output_error());
    if (tree->n_s >= 0xffffffffull)
        return fail(h, LX_EINVAL, "lx_tax_dev_create: too many subjects");
    lx_tax_dev * t = nullptr;
    try
    {
        std::vector<lx::lca::Node> nodes(std::max<uint64_t>(tree->n_taxa, 1), lx::lca::Node{0, 0});
        uint32_t                   max_height = 0;
        for (uint64_t x = 0; x < tree->n_taxa; ++x)
        {
            nodes[x]   = lx::lca::Node{tree->parents[x], tree->heights[x]};
            max_height = std::max(max_height, tree->heights[x]);
        }
        t             = new lx_tax_dev;
        t->n_taxa     = tree->n_taxa;
        t->n_s        = tree->n_s;
        t->max_height = max_height;
        int rc        = bind(h);
        if (rc)
        {
            delete t;
            return rc;
        }
        t->h                 = h;
        uint64_t const n_ids = tree->s_tax_off[tree->n_s];
        hipError_t     e     = hipMalloc(t->d_nodes.out(), nodes.size() * sizeof(lx::lca::Node));
        if (e == hipSuccess)
            e = hipMalloc(t->d_off.out(), (tree->n_s + 1) * sizeof(uint64_t));
        if (e == hipSuccess)
            e = hipMalloc(t->d_ids.out(), std::max<uint64_t>(n_ids, 1) * sizeof(uint32_t));
        if (e == hipSuccess)
            e = hipMemcpy(t->d_nodes, nodes.data(), nodes.size() * sizeof(lx::lca::Node), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(t->d_off, tree->s_tax_off, (tree->n_s + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_ids)
            e = hipMemcpy(t->d_ids, tree->s_tax_ids, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess)
        {
            delete t;
            return fail(h, e == hipErrorOutOfMemory ? LX_ENOMEM : LX_EHIP, "lx_tax_dev_create: %s", hipGetErrorString(e));
        }
    }
    catch (std::bad_alloc const &)
    {
        delete t;
        return fail(h, LX_ENOMEM, "lx_tax_dev_create: out of host memory");
    }
    *out = t;
    return LX_OK;
}

void lx_tax_dev_destroy(lx_tax_dev * t)
{
    delete t;
}

int lx_compute_lca_dev(lx_handle * h, lx_tax_dev const * t, lx_blast_match const * m, uint64_t n, lx_lca_options const * opt,
                       uint64_t * out_qid, uint32_t * out_lca, uint64_t * out_n)
{
    if (!h)
    {
        set_output_error("lx_compute_lca_dev: h == NULL");
        return LX_EINVAL;
    }
    h->phase_ev.clear(); // (a refused call reports no launch)
    h->ev_pool_used = 0;
    if (!t || (!m && n) || !out_qid || !out_lca || !out_n)
        return fail(h, LX_EINVAL, "lx_compute_lca_dev: NULL argument");
    *out_n = 0;
    if (t->h != h)
        return fail(h, LX_EINVAL, "lx_compute_lca_dev: the tree was made on another handle");
    if (n >= 0x7ffffff0ull)
        return fail(h, LX_EINVAL, "lx_compute_lca_dev: at most 2^31 - 16 rows per call");
    double const top = opt ? opt->top_percent : 100.0;
    if (!(top >= 0.0 && top <= 100.0))
        return fail(h, LX_EINVAL, "lx_compute_lca_dev: top_percent must be in [0, 100]");
    bool const   with_bits = top < 100.0;
    double const f         = 1.0 - top / 100.0;
    if (n == 0)
        return LX_OK;
    HostPool::Call const in_flight_call;

    // ---- every row checked before any device work: the first bad row of the list is the one reported
    unsigned const        parts = std::max(1u, host_threads(n));
    std::vector<uint64_t> bad(parts, ~0ull);
    uint64_t const        n_s = t->n_s;
    parallel_ranges(n, parts,
                    [&](unsigned p, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t k = lo; k < hi; ++k)
                            if (m[k].n_sid >= n_s || (with_bits && !std::isfinite(m[k].bit_score)))
                            {
                                bad[p] = k;
                                break;
                            }
                    });
    uint64_t const first_bad = *std::min_element(bad.begin(), bad.end());
    if (first_bad != ~0ull)
        return m[first_bad].n_sid >= n_s
                   ? fail(h, LX_EINVAL, "lx_compute_lca_dev: row %llu names subject %llu of %llu", (unsigned long long)first_bad,
                          (unsigned long long)m[first_bad].n_sid, (unsigned long long)n_s)
                   : fail(h, LX_EINVAL, "lx_compute_lca_dev: a bit score that is not finite (row %llu)", (unsigned long long)first_bad);

    try
    {
        std::vector<Range> const ranges = cut_ranges(m, n, h->opt_lca_range ? h->opt_lca_range : kDefaultRangeRows);
        uint64_t                 cap    = 0;
        for (Range const & r : ranges)
            cap = std::max(cap, r.hi - r.lo);
        int rc = bind(h);
        if (rc)
            return rc;
        lx_handle::Lca & z      = h->lca;
        int const        lanes  = ranges.size() > 1 ? 2 : 1;
        size_t const     in_sz  = LaneView::size(cap, with_bits), out_sz = (size_t)(cap + 1) * 4;
        for (int l = 0; l < lanes; ++l)
        {
            if ((rc = ensure(h, z.d_in[l], in_sz)) || (rc = ensure(h, z.d_out[l], out_sz)) || (rc = ensure_pinned(h, z.p_in[l], in_sz, kRoom)) ||
                (rc = ensure_pinned(h, z.p_out[l], out_sz, kRoom)))
                return rc;
            if (!z.ev_up[l])
                LX_HIP(h, hipEventCreateWithFlags(z.ev_up[l].out(), hipEventDisableTiming));
            if (!z.ev_k[l])
                LX_HIP(h, hipEventCreateWithFlags(z.ev_k[l].out(), hipEventDisableTiming));
        }
        if ((rc = ensure(h, z.d_first, (size_t)(cap + 1) * 4)) || (rc = ensure(h, z.d_tot, (size_t)(lx::lca::scan_tiles(cap) + 1) * 4)))
            return rc;

        hipStream_t const ks = h->stream, us = h->stream3;
        Flight            flight[2];
        uint32_t          err_word = 0;
        uint64_t          w        = 0; // queries so far
        // whatever way out: nothing of the lanes is in flight behind the call
        struct Drain
        {
            hipStream_t a, b;
            ~Drain()
            {
                (void)hipStreamSynchronize(a);
                (void)hipStreamSynchronize(b);
            }
        } const drain{us, ks};
        auto collect = [&](int L) -> int
        {
            if (!flight[L].on)
                return LX_OK;
            flight[L].on = false;
            LX_HIP(h, hipEventSynchronize(z.ev_k[L]));
            uint32_t const * const words = static_cast<uint32_t const *>(z.p_out[L].ptr);
            std::memcpy(out_lca + flight[L].at, words, flight[L].nq * 4);
            err_word |= words[flight[L].nq];
            return LX_OK;
        };

        std::vector<std::vector<uint64_t>> heads(parts);
        for (size_t r = 0; r < ranges.size(); ++r)
        {
            int const      L    = (int)(r & 1);
            uint64_t const lo   = ranges[r].lo, rows = ranges[r].hi - ranges[r].lo;
            if ((rc = collect(L))) // (the range before the last one: its lanes are free after)
                return rc;
            // the columns into the pinned lane, the heads' n_qid on the side
            LaneView const       pv(z.p_in[L].ptr, rows, with_bits);
            lx_blast_match const * const mr = m + lo;
            parallel_ranges(rows, std::max(1u, std::min(parts, host_threads(rows))),
                            [&](unsigned p, uint64_t a, uint64_t b)
                            {
                                std::vector<uint64_t> & hd = heads[p];
                                hd.clear();
                                for (uint64_t k = a; k < b; ++k)
                                {
                                    pv.qid[k] = mr[k].n_qid;
                                    pv.sid[k] = (uint32_t)mr[k].n_sid;
                                    if (with_bits)
                                        pv.bits[k] = mr[k].bit_score;
                                    if (k == 0 || mr[k].n_qid != mr[k - 1].n_qid)
                                        hd.push_back(mr[k].n_qid);
                                }
                            });
            uint64_t const at = w;
            for (std::vector<uint64_t> & hd : heads)
            {
                std::copy(hd.begin(), hd.end(), out_qid + w);
                w += hd.size();
                hd.clear();
            }
            uint64_t const nq = w - at;
            LaneView const dv(z.d_in[L].ptr, rows, with_bits);
            LX_HIP(h, hipMemcpyAsync(z.d_in[L].ptr, z.p_in[L].ptr, pv.bytes, hipMemcpyHostToDevice, us));
            LX_HIP(h, hipEventRecord(z.ev_up[L], us));
            LX_HIP(h, hipStreamWaitEvent(ks, z.ev_up[L], 0));
            lx::lca::RangeParams p{};
            p.tree      = lx::lca::TreeView{t->d_nodes, t->d_off, t->d_ids, t->max_height};
            p.qid       = dv.qid;
            p.sid       = dv.sid;
            p.bits      = dv.bits;
            p.f         = f;
            p.n         = (uint32_t)rows;
            p.nq        = (uint32_t)nq;
            p.first     = static_cast<uint32_t *>(z.d_first.ptr);
            p.block_tot = static_cast<uint32_t *>(z.d_tot.ptr);
            p.out       = static_cast<uint32_t *>(z.d_out[L].ptr);
            PhaseTimer timer(h, ks, 13);
            LX_HIP(h, lx::lca::launch_range(p, ks));
            timer.close();
            LX_HIP(h, hipMemcpyAsync(z.p_out[L].ptr, z.d_out[L].ptr, (size_t)(nq + 1) * 4, hipMemcpyDeviceToHost, ks));
            LX_HIP(h, hipEventRecord(z.ev_k[L], ks));
            flight[L] = Flight{true, nq, at};
        }
        for (size_t r = ranges.size() >= 2 ? ranges.size() - 2 : 0; r < ranges.size(); ++r)
            if ((rc = collect((int)(r & 1))))
                return rc;
        if (err_word)
            return fail(h, LX_EINVAL, "%s", kNoRoot);
        *out_n = w;
    }
    catch (std::bad_alloc const &)
    {
        return fail(h, LX_ENOMEM, "lx_compute_lca_dev: out of host memory");
    }
    return LX_OK;
}

} // extern "C"
