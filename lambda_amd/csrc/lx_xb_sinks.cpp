// lx_xb_sinks.cpp -- where the chunk pipeline's results go (lx_xb.h, XbSink): the caller's rows (lx_extend_batch, _rle), the handle's
// survivor list (lx_extend_batch_list), or the device (the Level-2 driver's resident lists, lx_records.hip).
#include "lx_level2.h"
#include "lx_xb.h"

namespace lxi
{
namespace
{

// a chunk's survivors as they came down into lane staging: records, list positions (slots, or caller indices), code lengths, codes
struct Survivors
{
    lx_hsp const *   hs;
    uint32_t const * src;
    uint32_t const * code_len;
    uint8_t const *  codes;
    explicit Survivors(lx_handle::XbLane const & ln)
        : hs(static_cast<lx_hsp const *>(ln.p_hsp.ptr)), src(static_cast<uint32_t const *>(ln.p_src.ptr)),
          code_len(static_cast<uint32_t const *>(ln.p_len.ptr)), codes(static_cast<uint8_t const *>(ln.p_rle.ptr)) {}
};

// Where the survivors' ops go in h->ext_bytes (column bytes or codes; none for padding and score 0): h->xb_off[e] from ops_total
// on, [count] = the end -- lengths, a prefix over the threads' shares, one inside each share; slot_pos: each slot's list position
int survivor_offsets(Xb & x, Survivors const & sv, uint64_t count, uint32_t * slot_pos, Clock::time_point t1)
{
    lx_handle * const       h        = x.h;
    unsigned const          nthreads = x.nthreads;
    bool const              want_rle = x.sink.codes;
    std::vector<uint64_t> & pos_off  = h->xb_off;
    pos_off.resize(count + 1);
    std::vector<uint64_t> part(nthreads + 1, 0);
    parallel_ranges(count, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        uint64_t sum = 0;
                        for (uint64_t e = lo; e < hi; ++e)
                        {
                            uint64_t len = 0;
                            if (sv.src[e] != 0xffffffffu)
                            {
                                if (slot_pos)
                                    slot_pos[sv.src[e]] = (uint32_t)e;
                                if (sv.hs[e].score > 0)
                                    len = want_rle ? (uint64_t)sv.code_len[e] : (uint64_t)sv.hs[e].n_ops;
                            }
                            pos_off[e] = len;
                            sum += len;
                        }
                        part[t + 1] = sum;
                    });
    auto const tu1 = now();
    x.t_u1 += ms(t1, tu1);
    part[0] = x.ops_total;
    for (unsigned t = 0; t < nthreads; ++t)
        part[t + 1] += part[t];
    uint64_t const total = part[nthreads];
    parallel_ranges(count, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        uint64_t at = part[t];
                        for (uint64_t e = lo; e < hi; ++e)
                        {
                            uint64_t const len = pos_off[e];
                            pos_off[e]         = at;
                            at += len;
                        }
                    });
    pos_off[count] = total;
    if (!h->ext_bytes.grow(total + 16))
        return fail(h, LX_ENOMEM, "out of host memory for %llu bytes of alignment ops", (unsigned long long)(total + 16));
    x.t_u2 += ms(tu1, now());
    return LX_OK;
}

// survivor e -> row `orig` of the caller's arrays, its ops at h->xb_off[e]; false: its backtrace gave up
inline bool write_row(Xb const & x, Survivors const & sv, uint64_t e, uint32_t orig)
{
    uint64_t const * const pos_off = x.h->xb_off.data();
    lx_hsp                 r       = sv.hs[e];
    if (r.score < 0)
        return false;
    uint8_t const * const cd  = sv.codes + (uint32_t)r.ops_shift;
    uint8_t * const       dst = x.h->ext_bytes.data() + pos_off[e];
    if (r.score > 0 && x.sink.codes)
        std::memcpy(dst, cd, (size_t)(pos_off[e + 1] - pos_off[e]));
    else if (r.score > 0)
        rle_expand(cd, r.n_ops, dst);
    r.ops_shift         = 0;
    x.out_hsp[orig]     = r;
    x.out_ops_off[orig] = pos_off[e];
    return true;
}

// the end of a chunk's unpacking: the first survivor whose backtrace gave up, else the ops handed out so far
int rows_written(Xb & x, std::vector<uint64_t> const & untraced, uint64_t count, Clock::time_point t1)
{
    for (uint64_t u : untraced)
        if (u != ~0ull)
            return fail(x.h, LX_EOVERFLOW, "extension %llu could not be traced", (unsigned long long)u);
    x.ops_total = x.h->xb_off[count];
    x.t_unpack += ms(t1, now());
    return LX_OK;
}

} // namespace

// ---- rows
// (the survivors' rows are written by rows_of_survivors, the scores of all rows at the end of the call)
void rows_clear(Xb & x)
{
    auto const tz0 = now();
    parallel_ranges(x.n, x.nthreads,
                    [&](unsigned, uint64_t lo, uint64_t hi)
                    {
                        std::memset(static_cast<void *>(x.out_hsp + lo), 0, (hi - lo) * sizeof(lx_hsp));
                        std::memset(x.out_ops_off + lo, 0, (hi - lo) * sizeof(uint64_t));
                    });
    x.t_unpack += ms(tz0, now());
}

int rows_of_slots(Xb & x, int L, uint64_t count, Clock::time_point t1)
{
    lx_handle * const      h = x.h;
    XbPrep const &         pr = x.prep[L];
    Survivors const        sv(h->xb[L]);
    int32_t const * const  sc       = static_cast<int32_t const *>(h->xb[L].p_score.ptr);
    uint32_t const * const slot_src = pr.slot_src.data();
    // which list position a slot has; where the survivors' ops go
    std::vector<uint32_t> & slot_pos = h->xb_pos;
    slot_pos.resize(pr.slots);
    parallel_ranges(pr.slots, x.nthreads, [&](unsigned, uint64_t lo, uint64_t hi) { std::fill(slot_pos.begin() + lo, slot_pos.begin() + hi, 0xffffffffu); });
    if (int const rc2 = survivor_offsets(x, sv, count, slot_pos.data(), t1))
        return rc2;
    // one pass over the chunk's slots: score and record of every extension, the survivors' ops
    std::vector<uint64_t> untraced(x.nthreads, ~0ull);
    parallel_ranges(pr.slots, x.nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t o = lo; o < hi; ++o)
                        {
                            uint32_t const orig = slot_src[o];
                            if (orig == 0xffffffffu)
                                continue;
                            x.out_score[orig] = sc[o];
                            uint32_t const e  = slot_pos[o];
                            if (e == 0xffffffffu)
                            {
                                lx_hsp r{};
                                r.score             = sc[o];
                                x.out_hsp[orig]     = r;
                                x.out_ops_off[orig] = 0;
                            }
                            else if (!write_row(x, sv, e, orig))
                                untraced[t] = std::min<uint64_t>(untraced[t], orig);
                        }
                    });
    return rows_written(x, untraced, count, t1);
}

// (the rows were cleared beside the first chunk; the scores come at the end of the call)
int rows_of_survivors(Xb & x, int L, uint64_t count, Clock::time_point t1)
{
    Survivors const sv(x.h->xb[L]);
    if (int const rc2 = survivor_offsets(x, sv, count, nullptr, t1))
        return rc2;
    std::vector<uint64_t> untraced(x.nthreads, ~0ull);
    parallel_ranges(count, x.nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t e = lo; e < hi; ++e)
                            if (sv.src[e] != 0xffffffffu && !write_row(x, sv, e, sv.src[e]))
                                untraced[t] = std::min<uint64_t>(untraced[t], sv.src[e]);
                    });
    return rows_written(x, untraced, count, t1);
}

// (a device list's scores stay on the device: h->d_score_all)
int scores_in_caller_order(Xb & x)
{
    lx_handle * const h   = x.h;
    auto const        ts0 = now();
    LX_HIP(h, hipMemcpyAsync(h->p_score_all.ptr, h->d_score_all.ptr, x.n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    LX_HIP(h, hipStreamSynchronize(h->stream));
    int32_t const * const sa   = static_cast<int32_t const *>(h->p_score_all.ptr);
    bool const            rows = x.sink.where == XbSink::kRows;
    parallel_ranges(x.n, x.nthreads,
                    [&](unsigned, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t i = lo; i < hi; ++i)
                        {
                            x.out_score[i] = sa[i];
                            if (rows && x.out_hsp[i].n_ops == 0)
                                x.out_hsp[i].score = sa[i];
                        }
                    });
    x.t_unpack += ms(ts0, now());
    return LX_OK;
}

// ---- list form (lx_extend_batch_list): the chunk's survivors are appended to the handle's result buffers -- position in the
// caller's list, record, where the codes begin -- and the chunk's codes to h->ext_bytes as one block; of the host's arrays
// of size n only the scores are touched
int list_append(Xb & x, int L, uint64_t count, uint64_t nrle, uint32_t const * slot_src)
{
    lx_handle * const      h        = x.h;
    unsigned const         nthreads = x.nthreads;
    uint64_t const         ops_total = x.ops_total;
    lx_handle::XbLane &    ln    = h->xb[L];
    lx_hsp const * const   hs    = static_cast<lx_hsp const *>(ln.p_hsp.ptr);
    uint32_t const * const src   = static_cast<uint32_t const *>(ln.p_src.ptr);
    uint8_t const * const  codes = static_cast<uint8_t const *>(ln.p_rle.ptr);
    std::vector<uint64_t>  part(nthreads + 1, 0), untraced(nthreads, ~0ull);
    parallel_ranges(count, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        uint64_t k = 0, bad = ~0ull; // (locals: the per-thread slots share cache lines)
                        for (uint64_t e = lo; e < hi; ++e)
                        {
                            if (src[e] == 0xffffffffu) // padding of the survivor list
                                continue;
                            if (hs[e].score < 0)
                                bad = std::min<uint64_t>(bad, slot_src ? slot_src[src[e]] : src[e]);
                            else
                                ++k;
                        }
                        part[t + 1] = k;
                        untraced[t] = bad;
                    });
    for (uint64_t u : untraced)
        if (u != ~0ull)
            return fail(h, LX_EOVERFLOW, "extension %llu could not be traced", (unsigned long long)u);
    for (unsigned t = 0; t < nthreads; ++t)
        part[t + 1] += part[t];
    uint64_t const base = h->res_count, total = base + part[nthreads];
    if (!h->res_index.grow(total * sizeof(uint32_t) + 16) || !h->res_hsp.grow(total * sizeof(lx_hsp) + 16) ||
        !h->res_off.grow(total * sizeof(uint64_t) + 16) || !h->ext_bytes.grow(ops_total + nrle + 16))
        return fail(h, LX_ENOMEM, "out of host memory for %llu survivors", (unsigned long long)total);
    uint32_t * const res_index = reinterpret_cast<uint32_t *>(h->res_index.data());
    lx_hsp * const   res_hsp   = reinterpret_cast<lx_hsp *>(h->res_hsp.data());
    uint64_t * const res_off   = reinterpret_cast<uint64_t *>(h->res_off.data());
    uint8_t * const  dst       = h->ext_bytes.data() + ops_total;
    parallel_ranges(count, nthreads,
                    [&](unsigned t, uint64_t lo, uint64_t hi)
                    {
                        uint64_t k = base + part[t];
                        for (uint64_t e = lo; e < hi; ++e)
                        {
                            if (src[e] == 0xffffffffu)
                                continue;
                            lx_hsp r     = hs[e];
                            res_index[k] = slot_src ? slot_src[src[e]] : src[e];
                            res_off[k]   = ops_total + (uint32_t)r.ops_shift;
                            r.ops_shift  = 0;
                            res_hsp[k]   = r;
                            ++k;
                        }
                    });
    parallel_ranges(nrle, nthreads, [&](unsigned, uint64_t lo, uint64_t hi) { std::memcpy(dst + lo, codes + lo, hi - lo); });
    h->res_count = total;
    x.ops_total += nrle;
    return LX_OK;
}

// ---- device: the Level-2 driver makes its records on the device (lx_records.hip)
int device_sink(Xb & x, bool by_range)
{
    lx_handle * const h  = x.h;
    auto &            l2 = h->l2;
    // (fillers never survive, a chunk's list is padded by less than 16 entries: the list's windows + a margin per chunk -- not the
    // plan's slots: the streamed part of a host plan is made later)
    uint64_t const cap = x.n + x.n / 64 + 8192;
    int            rc;
    if ((rc = ensure(h, l2.d_surv_hsp, cap * sizeof(lx_hsp))) || (rc = ensure(h, l2.d_surv_src, cap * sizeof(uint32_t))) ||
        (rc = ensure(h, l2.d_surv_codes, cap * sizeof(uint64_t))))
        return rc;
    l2.surv_cap   = cap;
    l2.surv_total = 0;
    x.sink        = XbSink{by_range ? XbSink::kDeviceByRange : XbSink::kDevice, x.ri->want_codes};
    return LX_OK;
}

// The survivors stay where the backtrace left them (lx_records.hip makes the result records from them): the chunk's list joins the
// call's on the device -- a copy kernel in stream order, so that this lane's buffers are free for the chunk after next --, only the
// run-length codes come down, into the call's code bytes.  By range, the range's rows and columns are collected instead.
int device_collect(Xb & x, int L, uint64_t count, uint64_t nrle, Clock::time_point t0, Clock::time_point t_ev)
{
    lx_handle * const   h         = x.h;
    lx_handle::XbLane & ln        = h->xb[L];
    auto &              l2        = h->l2;
    uint64_t const      code_base = x.ops_total;
    bool const          by_range  = x.sink.where == XbSink::kDeviceByRange;
    if (!by_range)
    {
        if (l2.surv_total + count > l2.surv_cap)
            return fail(h, LX_ESTATE, "the call's survivor list is longer than its capacity");
        LX_HIP(h, lx::rec_launch_append(static_cast<lx::Hsp const *>(ln.d_hsp.ptr), static_cast<uint32_t const *>(ln.d_src.ptr),
                                        static_cast<uint64_t const *>(ln.d_cnt.ptr), count, x.ops_total, static_cast<lx::Hsp *>(l2.d_surv_hsp.ptr) + l2.surv_total,
                                        static_cast<uint32_t *>(l2.d_surv_src.ptr) + l2.surv_total, static_cast<uint64_t *>(l2.d_surv_codes.ptr) + l2.surv_total,
                                        h->stream));
    }
    l2.surv_total += count;
    if (nrle && x.sink.codes)
    {
        if (!h->ext_bytes.grow(x.ops_total + nrle + 16))
            return fail(h, LX_ENOMEM, "out of host memory for %llu bytes of alignment codes", (unsigned long long)(x.ops_total + nrle));
        // (straight into the call's code bytes: a copy of this size into ordinary memory runs at the link's rate)
        LX_HIP(h, hipMemcpyAsync(h->ext_bytes.data() + x.ops_total, ln.d_rle.ptr, nrle, hipMemcpyDeviceToHost, h->stream3));
        LX_HIP(h, hipStreamSynchronize(h->stream3));
    }
    x.ops_total += nrle;
    h->res_count  = l2.surv_total;
    auto const t1 = now();
    x.t_wait += ms(t0, t1);
    if (!by_range)
    {
        if (x.hm.on)
            fprintf(stderr, "[lx host ms]     ... its counts came after %.2f ms of waiting, its %llu code bytes in %.2f more; the %llu records stay on the device\n",
                    ms(t0, t_ev), (unsigned long long)nrle, ms(t_ev, t1), (unsigned long long)count);
        return LX_OK;
    }
    int const rc2 = x.ri->chunk_records->collect(x.prep[L].range, code_base, x.in_flight[L ^ 1]);
    x.t_unpack += ms(t1, now());
    if (x.hm.on)
        fprintf(stderr, "[lx host ms]     ... its counts came after %.2f ms of waiting, its %llu code bytes in %.2f more; rows and columns of range %llu in %.2f\n",
                ms(t0, t_ev), (unsigned long long)nrle, ms(t_ev, t1), (unsigned long long)x.prep[L].range, ms(t1, now()));
    return rc2;
}

} // namespace lxi
