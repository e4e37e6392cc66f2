// lx_qmask_host.cpp -- low-complexity masking of the queries (include/lambda_ext.h: lx_seg_*, lx_dust_*, lx_query_mask_*).  lx_qmask.h
// has the protein rule, SEG, lx_dust.h the nucleotide rule, DUST; here are SEG's tables, the host path (a rule per sequence on the
// host threads), the device path (the letters and the sequence table go up, lx_qmask.hip's or lx_dust.hip's kernels leave the distance
// bytes resident on the handle's device) and the mask object that lx_seed_queries_masked reads.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <memory>
#include <mutex>
#include <new>

#include "lx_internal.h"
#include "lx_dust.h"
#include "lx_qmask.h"
#include "host/lx_seeding.hpp"

using lxi::bind;
using lxi::fail;
namespace qm = lx::qmask;

lx_query_mask::~lx_query_mask()
{
    // its handle's device bound and the launch stream through before the block goes
    if (h && bind(h) == LX_OK)
        (void)hipStreamSynchronize(h->stream);
}

uint8_t const * lx_query_mask::host_dist() const
{
    std::lock_guard<std::mutex> once(down); // (two threads may seed with one mask)
    if (!have_host)
    {
        try
        {
            dist.resize(extent);
        }
        catch (std::bad_alloc const &)
        {
            return nullptr;
        }
        if (bind(h) != LX_OK || (extent && hipMemcpy(dist.data(), d_dist, extent, hipMemcpyDeviceToHost) != hipSuccess))
            return nullptr;
        have_host = true;
    }
    static uint8_t const none = 0;
    return dist.empty() ? &none : dist.data();
}

namespace
{

// the text goes to lx_last_output_error() and, with a handle, to lx_last_error(h) too
int say(lx_handle * h, int code, char const * fmt, ...)
{
    char    buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    lxi::set_output_error(buf);
    return h ? fail(h, code, "%s", buf) : code;
}

char const * params_error(lx_seg_params const * p)
{
    if (p->window < qm::kSegMinWindow || p->window > qm::kSegMaxWindow)
        return "window outside 4 .. 64";
    double const top = std::log2((double)p->window);
    if (!(p->k1 > 0.0) || !(p->k2 > 0.0) || !(p->k1 <= p->k2) || !(p->k2 <= top))
        return "k1, k2 must satisfy 0 < k1 <= k2 <= log2(window)";
    return nullptr;
}

void make_tables(lx_seg_params const & p, qm::SegTables & t)
{
    t.W = p.window;
    for (int c = 0; c <= 64; ++c)
        t.T[c] = c < 2 ? 0u : (uint32_t)std::llround((double)c * std::log2((double)c) * 65536.0);
    double const W = (double)p.window;
    t.thr1         = (uint32_t)std::ceil(W * (std::log2(W) - p.k1) * 65536.0);
    t.thr2         = (uint32_t)std::ceil(W * (std::log2(W) - p.k2) * 65536.0);
}

// The sequence table, checked: sequences with letters lie inside the address range, in ascending order, without overlap (a distance
// byte belongs to one letter of one sequence).
int take_table(lx_handle * h, char const * who, uint64_t const * q_off, uint64_t const * q_len, uint64_t n_qseq, lx_query_mask & m,
               std::vector<uint64_t> * gaps = nullptr)
{
    if (n_qseq && (!q_off || !q_len))
        return say(h, LX_EINVAL, "%s: NULL sequence table", who);
    uint64_t end = 0, total = 0;
    for (uint64_t i = 0; i < n_qseq; ++i)
    {
        if (q_len[i] == 0)
            continue;
        if (q_off[i] > ~0ull - q_len[i] || total > ~0ull - q_len[i])
            return say(h, LX_EINVAL, "%s: sequence %llu lies outside the address range", who, (unsigned long long)i);
        if (q_off[i] < end)
            return say(h, LX_EINVAL, "%s: sequence %llu begins in front of the end of the one before it (a mask needs the sequences in ascending order, without overlap)",
                       who, (unsigned long long)i);
        if (gaps && q_off[i] > end)
            gaps->push_back(end), gaps->push_back(q_off[i]);
        end = q_off[i] + q_len[i];
        total += q_len[i];
    }
    m.off.assign(q_off, q_off + n_qseq);
    m.len.assign(q_len, q_len + n_qseq);
    m.extent    = end;
    m.n_letters = total;
    return LX_OK;
}

unsigned threads_or_share(uint32_t asked)
{
    return asked ? asked : std::max(1u, lxi::pool_width());
}

// f(first sequence, one behind the last) over pieces of about equal letters, on the host threads
template <class F>
void over_sequences(lx_query_mask const & m, unsigned threads, F && f)
{
    uint64_t const n     = m.off.size();
    size_t const   parts = (size_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads * 4, m.n_letters >> 16));
    std::vector<uint64_t> cut(parts + 1, n);
    cut[0]         = 0;
    uint64_t seen  = 0;
    size_t   k     = 1;
    for (uint64_t s = 0; s < n && k < parts; ++s)
    {
        seen += m.len[s];
        while (k < parts && seen >= m.n_letters / parts * k)
            cut[k++] = s + 1;
    }
    lambda_amd::parallelChunks(threads, parts, [&](size_t c) { f(cut[c], cut[c + 1]); });
}

// one of the two rules: SEG's tables or DUST's parameters
struct Rule
{
    qm::SegTables const *  seg;
    qm::DustParams const * dust;
    char const *           who;
};

int mask_on_host(lx_query_mask & m, uint8_t const * q_res, Rule const & rule, unsigned threads)
{
    m.dist.assign(m.extent, (uint8_t)qm::kSegFree);
    std::vector<uint64_t> masked(1, 0), touched(1, 0);
    std::mutex            sum;
    over_sequences(m, threads,
                   [&](uint64_t a, uint64_t b)
                   {
                       std::vector<uint64_t> A, B, F;
                       qm::DustWork          work;
                       uint64_t              nm = 0, nt = 0;
                       for (uint64_t s = a; s < b; ++s)
                       {
                           uint64_t const L = m.len[s];
                           if (L == 0)
                               continue;
                           size_t const words = (size_t)((L + 63) / 64);
                           if (rule.seg && A.size() < words)
                               A.resize(words), B.resize(words), F.resize(words);
                           uint64_t const got = rule.seg ? qm::seg_mask_sequence(q_res + m.off[s], L, *rule.seg, m.dist.data() + m.off[s], A.data(), B.data(), F.data())
                                                         : qm::dust_mask_sequence(q_res + m.off[s], L, *rule.dust, m.dist.data() + m.off[s], work);
                           nm += got;
                           nt += got ? 1 : 0;
                       }
                       std::lock_guard<std::mutex> g(sum);
                       masked[0] += nm, touched[0] += nt;
                   });
    m.n_masked = masked[0], m.n_seqs_masked = touched[0];
    m.have_host = true;
    return LX_OK;
}

template <class T>
int dev_zeroed(lx_handle * h, lxi::DevBlock<T> & b, size_t count, hipStream_t st)
{
    size_t const bytes = std::max<size_t>(count * sizeof(T), 16);
    LX_HIP(h, hipMalloc(reinterpret_cast<void **>(b.out()), bytes));
    LX_HIP(h, hipMemsetAsync(b.raw, 0, bytes, st));
    return LX_OK;
}

int mask_on_device(lx_handle * h, lx_query_mask & m, uint8_t const * q_res, Rule const & rule, std::vector<uint64_t> const & gaps)
{
    int rc = bind(h);
    if (rc)
        return rc;
    hipStream_t const st   = h->stream;
    uint64_t const    nSeq = m.off.size(), nWords = (m.extent + 63) / 64, nTiles = (nWords + qm::kTileWords - 1) / qm::kTileWords;
    // (DUST's sweep has the most workgroups: one per dust_run(window) >= 195 letters)
    if (nWords * 64 / (rule.dust ? 128 : qm::kFlagBlock) + 1 > 0x7fffffffull || gaps.size() / 2 > 0x7fffffffull)
        return say(h, LX_EINVAL, "%s: %llu letters are beyond one launch: mask with h == NULL", rule.who, (unsigned long long)m.extent);
    lxi::DevBlock<uint8_t>            d_res, d_ops, d_reach;
    lxi::DevBlock<uint64_t>           d_off, d_len, d_A, d_B, d_F, d_gaps, d_brk;
    lxi::DevBlock<unsigned long long> d_stop, d_count;
    lxi::DevBlock<uint32_t>           d_T;
    LX_HIP(h, hipMalloc(reinterpret_cast<void **>(m.d_dist.out()), m.extent + 64));
    m.h = h;
    if ((rc = dev_zeroed(h, d_res, m.extent + 64, st)) || (rc = dev_zeroed(h, d_off, nSeq, st)) || (rc = dev_zeroed(h, d_len, nSeq, st)) ||
        (rc = dev_zeroed(h, d_F, nWords + 2, st)) || (rc = dev_zeroed(h, d_stop, nWords + 2, st)) || (rc = dev_zeroed(h, d_count, 2, st)) ||
        (rc = dev_zeroed(h, d_gaps, gaps.size(), st)))
        return rc;
    if (rule.seg ? (rc = dev_zeroed(h, d_A, nWords, st)) || (rc = dev_zeroed(h, d_B, nWords, st)) || (rc = dev_zeroed(h, d_T, 65, st)) ||
                       (rc = dev_zeroed(h, d_ops, 2 * nTiles, st))
                 : (rc = dev_zeroed(h, d_brk, nWords + 2, st)) || (rc = dev_zeroed(h, d_reach, nWords * 64 + 64, st)))
        return rc;
    if (!gaps.empty())
        LX_HIP(h, hipMemcpyAsync(d_gaps, gaps.data(), gaps.size() * 8, hipMemcpyHostToDevice, st));
    LX_HIP(h, hipMemsetAsync(m.d_dist, qm::kSegFree, m.extent + 64, st));
    if (m.extent)
        LX_HIP(h, hipMemcpyAsync(d_res, q_res, m.extent, hipMemcpyHostToDevice, st));
    if (nSeq)
    {
        LX_HIP(h, hipMemcpyAsync(d_off, m.off.data(), nSeq * 8, hipMemcpyHostToDevice, st));
        LX_HIP(h, hipMemcpyAsync(d_len, m.len.data(), nSeq * 8, hipMemcpyHostToDevice, st));
    }
    qm::QmaskDev p{};
    p.qRes = d_res, p.qOff = d_off, p.qLen = d_len, p.nSeq = nSeq, p.extent = m.extent, p.nWords = nWords, p.nTiles = nTiles;
    p.stop = d_stop, p.F = d_F, p.gaps = d_gaps, p.nGaps = gaps.size() / 2, p.dist = m.d_dist, p.count = d_count;
    if (rule.seg)
    {
        qm::SegTables const & t = *rule.seg;
        LX_HIP(h, hipMemcpyAsync(d_T, t.T, sizeof(t.T), hipMemcpyHostToDevice, st));
        p.W = t.W, p.thr1 = t.thr1, p.thr2 = t.thr2, p.T = d_T, p.A = d_A, p.B = d_B;
        p.opUp = d_ops, p.opDown = d_ops.raw + nTiles;
    }
    lxi::PhaseTimer timer(h, st, 15);
    if (rule.seg)
        LX_HIP(h, qm::qmask_launch(p, st));
    else
        LX_HIP(h, qm::dust_launch(p, qm::DustDev{rule.dust->window, rule.dust->level, d_brk, d_reach}, st));
    timer.close();
    unsigned long long count[2] = {0, 0};
    LX_HIP(h, hipMemcpyAsync(count, d_count, sizeof(count), hipMemcpyDeviceToHost, st));
    LX_HIP(h, hipStreamSynchronize(st));
    m.n_masked = count[0], m.n_seqs_masked = count[1];
    return LX_OK;
}

} // namespace

extern "C" {

void lx_seg_params_default(lx_seg_params * p)
{
    if (p)
        *p = lx_seg_params{12, 2.2, 2.5};
}

int lx_seg_tables(lx_seg_params const * p, int64_t T[65], int64_t * thr1, int64_t * thr2)
{
    if (!p || !T || !thr1 || !thr2)
        return say(nullptr, LX_EINVAL, "lx_seg_tables: NULL argument");
    if (char const * why = params_error(p))
        return say(nullptr, LX_EINVAL, "lx_seg_tables: %s", why);
    qm::SegTables t;
    make_tables(*p, t);
    for (int c = 0; c <= 64; ++c)
        T[c] = (int64_t)t.T[c];
    *thr1 = (int64_t)t.thr1, *thr2 = (int64_t)t.thr2;
    return LX_OK;
}

int lx_query_mask_create_seg(lx_handle * h, uint8_t const * q_res, uint64_t const * q_off, uint64_t const * q_len, uint64_t n_qseq, lx_seg_params const * p,
                             uint32_t host_threads, lx_query_mask ** out)
{
    if (h)
    {
        h->phase_ev.clear(); // (a refused call reports no launch)
        h->ev_pool_used = 0;
    }
    if (!out || !p)
        return say(h, LX_EINVAL, "lx_query_mask_create_seg: NULL argument");
    *out = nullptr;
    if (char const * why = params_error(p))
        return say(h, LX_EINVAL, "lx_query_mask_create_seg: %s", why);
    try
    {
        std::unique_ptr<lx_query_mask> m(new lx_query_mask);
        std::vector<uint64_t>          gaps;
        int                            rc = take_table(h, "lx_query_mask_create_seg", q_off, q_len, n_qseq, *m, &gaps);
        if (rc)
            return rc;
        if (m->extent && !q_res)
            return say(h, LX_EINVAL, "lx_query_mask_create_seg: NULL letters");
        qm::SegTables t;
        make_tables(*p, t);
        Rule const rule{&t, nullptr, "lx_query_mask_create_seg"};
        rc = h ? mask_on_device(h, *m, q_res, rule, gaps) : mask_on_host(*m, q_res, rule, threads_or_share(host_threads));
        if (rc)
            return rc;
        *out = m.release();
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_query_mask_create_seg: out of host memory");
    }
    return LX_OK;
}

void lx_dust_params_default(lx_dust_params * p)
{
    if (p)
        *p = lx_dust_params{64, 20};
}

int lx_query_mask_create_dust(lx_handle * h, uint8_t const * q_res, uint64_t const * q_off, uint64_t const * q_len, uint64_t n_qseq, lx_dust_params const * p,
                              uint32_t host_threads, lx_query_mask ** out)
{
    if (h)
    {
        h->phase_ev.clear(); // (a refused call reports no launch)
        h->ev_pool_used = 0;
    }
    if (!out || !p)
        return say(h, LX_EINVAL, "lx_query_mask_create_dust: NULL argument");
    *out = nullptr;
    if (p->window < qm::kDustMinWindow || p->window > qm::kDustMaxWindow)
        return say(h, LX_EINVAL, "lx_query_mask_create_dust: window outside 4 .. 64");
    if (p->level < qm::kDustMinLevel || p->level > qm::kDustMaxLevel)
        return say(h, LX_EINVAL, "lx_query_mask_create_dust: level outside 1 .. 1000");
    try
    {
        std::unique_ptr<lx_query_mask> m(new lx_query_mask);
        std::vector<uint64_t>          gaps;
        int                            rc = take_table(h, "lx_query_mask_create_dust", q_off, q_len, n_qseq, *m, &gaps);
        if (rc)
            return rc;
        if (m->extent && !q_res)
            return say(h, LX_EINVAL, "lx_query_mask_create_dust: NULL letters");
        qm::DustParams const dp{p->window, p->level};
        Rule const           rule{nullptr, &dp, "lx_query_mask_create_dust"};
        rc = h ? mask_on_device(h, *m, q_res, rule, gaps) : mask_on_host(*m, q_res, rule, threads_or_share(host_threads));
        if (rc)
            return rc;
        *out = m.release();
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_query_mask_create_dust: out of host memory");
    }
    return LX_OK;
}

int lx_query_mask_create(lx_handle * h, uint8_t const * masked, uint64_t const * q_off, uint64_t const * q_len, uint64_t n_qseq, lx_query_mask ** out)
{
    if (!out)
        return say(h, LX_EINVAL, "lx_query_mask_create: NULL argument");
    *out = nullptr;
    try
    {
        std::unique_ptr<lx_query_mask> m(new lx_query_mask);
        int                            rc = take_table(h, "lx_query_mask_create", q_off, q_len, n_qseq, *m);
        if (rc)
            return rc;
        if (m->extent && !masked)
            return say(h, LX_EINVAL, "lx_query_mask_create: NULL mask bytes");
        m->dist.assign(m->extent, (uint8_t)qm::kSegFree);
        for (uint64_t s = 0; s < n_qseq; ++s)
        {
            uint64_t const got = qm::dist_from_bytes(masked + m->off[s], m->len[s], m->dist.data() + m->off[s]);
            m->n_masked += got;
            m->n_seqs_masked += got ? 1 : 0;
        }
        m->have_host = true;
        if (h)
        {
            if ((rc = bind(h)))
                return rc;
            LX_HIP(h, hipMalloc(reinterpret_cast<void **>(m->d_dist.out()), m->extent + 64));
            m->h = h;
            LX_HIP(h, hipMemset(m->d_dist, qm::kSegFree, m->extent + 64));
            if (m->extent)
                LX_HIP(h, hipMemcpy(m->d_dist, m->dist.data(), m->extent, hipMemcpyHostToDevice));
        }
        *out = m.release();
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_query_mask_create: out of host memory");
    }
    return LX_OK;
}

int lx_query_mask_info(lx_query_mask const * m, uint64_t * n_letters, uint64_t * n_masked, uint64_t * n_seqs_masked)
{
    if (!m)
        return say(nullptr, LX_EINVAL, "lx_query_mask_info: NULL mask");
    if (n_letters)
        *n_letters = m->n_letters;
    if (n_masked)
        *n_masked = m->n_masked;
    if (n_seqs_masked)
        *n_seqs_masked = m->n_seqs_masked;
    return LX_OK;
}

int lx_query_mask_copy(lx_query_mask const * m, uint8_t * masked)
{
    if (!m || (!masked && m->extent))
        return say(nullptr, LX_EINVAL, "lx_query_mask_copy: NULL argument");
    uint8_t const * const d = m->host_dist();
    if (!d)
        return say(m->h, LX_EHIP, "lx_query_mask_copy: the mask did not come down from the device");
    for (uint64_t j = 0; j < m->extent; ++j)
        masked[j] = 0;
    for (size_t s = 0; s < m->off.size(); ++s)
        for (uint64_t j = m->off[s], e = m->off[s] + m->len[s]; j < e; ++j)
            masked[j] = d[j] == 0 ? 1 : 0;
    return LX_OK;
}

void lx_query_mask_destroy(lx_query_mask * m)
{
    delete m;
}

} // extern "C"
