// lx_xb_core.cpp -- the chunk pipeline's shared half (lx_xb.h): the list's upload, the two lanes' buffers, the fused step over a
// lane, and a chunk's way back -- counts first, then what the counts say has a size.
#include "lx_xb.h"

namespace lxi
{

int Xb::upload_list()
{
    int rc2;
    auto const tu0 = now();
    uint64_t const ext_bytes = n * sizeof(lx_extension), min_bytes = min_score ? n * sizeof(int32_t) : 0;
    // (the scores of a list whose records are made on the device stay there: no pinned block for their way down)
    if ((rc2 = ensure(h, h->d_score_all, n * sizeof(int32_t) + 16)) ||
        (!(sink.where != XbSink::kRows && ri && ri->keep_on_device) && (rc2 = ensure_pinned(h, h->p_score_all, n * sizeof(int32_t) + 16, kRoom))))
        return rc2;
    if (!ri) // (a resident list stands where the Level-2 kernels wrote it)
    {
        if ((rc2 = ensure_pinned(h, h->p_all, ext_bytes + min_bytes + 16, kRoom)) || (rc2 = ensure(h, h->d_ext_all, ext_bytes + 16)) ||
            (rc2 = ensure(h, h->d_min_all, min_bytes + 16)))
            return rc2;
        uint8_t * const stage_all = static_cast<uint8_t *>(h->p_all.ptr);
        parallel_ranges(n, nthreads,
                        [&](unsigned, uint64_t lo, uint64_t hi)
                        {
                            std::memcpy(stage_all + lo * sizeof(lx_extension), ext + lo, (hi - lo) * sizeof(lx_extension));
                            if (min_score)
                                std::memcpy(stage_all + ext_bytes + lo * sizeof(int32_t), min_score + lo, (hi - lo) * sizeof(int32_t));
                        });
        LX_HIP(h, hipMemcpyAsync(h->d_ext_all.ptr, stage_all, ext_bytes, hipMemcpyHostToDevice, h->stream));
        if (min_score)
            LX_HIP(h, hipMemcpyAsync(h->d_min_all.ptr, stage_all + ext_bytes, min_bytes, hipMemcpyHostToDevice, h->stream));
    }
    LX_HIP(h, hipMemsetAsync(h->d_score_all.ptr, 0, n * sizeof(int32_t), h->stream));
    t_upload      = ms(tu0, now());
    list_uploaded = true;
    return LX_OK;
}

int Xb::run(void const * d_q_, void const * d_s_)
{
    d_q          = d_q_;
    d_s          = d_s_;
    chunk_target = h->opt_extend_chunk ? std::max<uint64_t>(h->opt_extend_chunk, 1024) : lxi::kExtendChunk;
    h->ext_bytes.clear();
    h->xb_stats[0] = p.live;
    h->xb_stats[1] = h->xb_stats[2] = h->xb_stats[3] = 0; // slots, cells, cells the wavefronts execute
    if (int const rc = p.use_mq ? run_chunks_of_wavefronts(*this) : run_chunks_of_runs(*this))
        return rc;
    hm.mark("pipeline"); // (every chunk's error word came back with its counts: check_counts)
    if (hm.on)
        fprintf(stderr, "[lx host ms]   pipeline of %d chunks: prepare %.1f, issue %.1f, wait for the GPU %.1f, unpack %.1f (lengths %.1f, offsets %.1f)\n", c, t_prep, t_issue,
                t_wait, t_unpack, t_u1, t_u2);
    return LX_OK;
}

int Xb::size_lane(int L, uint64_t slots, uint64_t stride, bool orig, bool mq)
{
    lx_handle::XbLane & ln      = h->xb[L];
    uint64_t const      cap_sel = prep[L].cap_sel, words = mq ? 5 : 4;
    int                 rc2;
    if ((orig && (rc2 = ensure(h, ln.d_orig, slots * sizeof(uint32_t)))) || (rc2 = ensure(h, ln.d_ext, slots * sizeof(lx_extension))) ||
        (rc2 = ensure(h, ln.d_min, slots * sizeof(int32_t))) || (rc2 = ensure(h, ln.d_score, slots * sizeof(int32_t))) ||
        (rc2 = ensure(h, ln.d_hsp, cap_sel * sizeof(lx_hsp))) || (rc2 = ensure(h, ln.d_ops, cap_sel * stride + 16)) ||
        (rc2 = ensure(h, ln.d_rle, cap_sel * stride + 16)) || (rc2 = ensure(h, ln.d_src, cap_sel * sizeof(uint32_t))) ||
        (rc2 = ensure(h, ln.d_len, cap_sel * sizeof(uint32_t))) || (rc2 = ensure(h, ln.d_cnt, words * sizeof(uint64_t))) ||
        (!mq && (rc2 = ensure_pinned(h, ln.p_score, slots * sizeof(int32_t), kRoom))) || (rc2 = ensure_pinned(h, ln.p_cnt, words * sizeof(uint64_t), kRoom)))
        return rc2;
    return LX_OK;
}

int Xb::run_fused(int L, uint64_t slots, uint64_t stride, uint64_t max_q, uint64_t max_s, uint64_t run, MqTab const & tab, bool wide)
{
    lx_handle::XbLane & ln    = h->xb[L];
    uint64_t * const    d_cnt = static_cast<uint64_t *>(ln.d_cnt.ptr);
    StepCall            sc;
    sc.d_q = d_q, sc.d_s = d_s, sc.d_ext = ln.d_ext.ptr, sc.n = slots, sc.d_min_score = ln.d_min.ptr;
    sc.d_out_score = ln.d_score.ptr, sc.d_out_hsp = ln.d_hsp.ptr, sc.d_out_ops = ln.d_ops.ptr, sc.d_out_count = d_cnt;
    sc.stream        = h->stream;
    sc.by_pos        = true;
    sc.fx.ops_stride = stride; // one ops slot per position of the survivor list
    sc.fx.d_rle      = static_cast<uint8_t *>(ln.d_rle.ptr);
    sc.fx.d_rle_top  = reinterpret_cast<unsigned long long *>(d_cnt + 2);
    sc.fx.rle_cap    = prep[L].cap_sel * stride;
    sc.fx.d_src_out  = static_cast<uint32_t *>(ln.d_src.ptr);
    sc.fx.d_rle_len  = static_cast<uint32_t *>(ln.d_len.ptr);
    sc.lim           = ListLimits{max_q, max_s, run, h->band_dev, bs_rule};
    sc.tab           = tab;
    sc.mq_geo        = p.use_mq ? p.mq_geo : lx::Geo{};
    sc.mq_wide       = wide;
    sc.keep_events   = true; // (the call's phase list holds every chunk's events)
    return fused_impl(h, slot, sc);
}

int Xb::send_counts(int L, uint64_t words, uint64_t lane_scores)
{
    lx_handle::XbLane & ln    = h->xb[L];
    uint64_t * const    d_cnt = static_cast<uint64_t *>(ln.d_cnt.ptr);
    int                 rc2;
    // the device's error word of THIS chunk, saved in stream order (the next chunk's prepare_workspace clears it): it comes
    // back with the counts and is checked in check_counts
    LX_HIP(h, hipMemcpyAsync(d_cnt + 3, ws_word(h, kWsBump), 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    if (words > 4)
        LX_HIP(h, hipMemcpyAsync(d_cnt + 4, ws_word(h, kWsStatBeyond), sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    if (sink.where == XbSink::kDeviceByRange && (rc2 = ri->chunk_records->enqueue(prep[L].range, ln.d_hsp.ptr, ln.d_src.ptr, d_cnt, prep[L].cap_sel)))
        return rc2;
    LX_HIP(h, hipEventRecord(ln.ev_k, h->stream));
    // what has a size the host knows goes back at once; records and codes follow when the counts have arrived
    LX_HIP(h, hipStreamWaitEvent(h->stream2, ln.ev_k, 0));
    LX_HIP(h, hipMemcpyAsync(ln.p_cnt.ptr, d_cnt, words * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream2));
    if (lane_scores)
        LX_HIP(h, hipMemcpyAsync(ln.p_score.ptr, ln.d_score.ptr, lane_scores * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream2));
    LX_HIP(h, hipEventRecord(ln.ev_cnt, h->stream2));
    in_flight[L] = true;
    return LX_OK;
}

int Xb::wait_counts(int L, uint64_t const *& cnt)
{
    lx_handle::XbLane & ln = h->xb[L];
    in_flight[L]           = false;
    LX_HIP(h, hipEventSynchronize(ln.ev_cnt));
    cnt = static_cast<uint64_t const *>(ln.p_cnt.ptr);
    return LX_OK;
}

int Xb::check_counts(XbPrep const & pr, uint64_t const * cnt)
{
    uint32_t flags[2];
    std::memcpy(flags, cnt + 3, sizeof(flags));
    if (int const rcf = error_for_flag(h, flags[1]))
        return rcf;
    if (cnt[0] > pr.cap_sel)
        return fail(h, LX_ESTATE, "survivor list longer than its capacity");
    if (pr.slots)
        h->surv_frac = (double)cnt[1] / (double)pr.slots;
    return LX_OK;
}

// (on the upload stream: stream2 already holds the next chunk's first-stage copies, which wait for its kernels)
int Xb::download_survivors(int L, uint64_t count, uint64_t nrle)
{
    lx_handle::XbLane & ln = h->xb[L];
    int                 rc2;
    if ((rc2 = ensure_pinned(h, ln.p_hsp, count * sizeof(lx_hsp) + 16, kRoom)) || (rc2 = ensure_pinned(h, ln.p_src, count * sizeof(uint32_t) + 16, kRoom)) ||
        (rc2 = ensure_pinned(h, ln.p_len, count * sizeof(uint32_t) + 16, kRoom)) || (rc2 = ensure_pinned(h, ln.p_rle, nrle + 16, kRoom)))
        return rc2;
    if (count)
    {
        LX_HIP(h, hipMemcpyAsync(ln.p_hsp.ptr, ln.d_hsp.ptr, count * sizeof(lx_hsp), hipMemcpyDeviceToHost, h->stream3));
        LX_HIP(h, hipMemcpyAsync(ln.p_src.ptr, ln.d_src.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream3));
        LX_HIP(h, hipMemcpyAsync(ln.p_len.ptr, ln.d_len.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream3));
        if (nrle)
            LX_HIP(h, hipMemcpyAsync(ln.p_rle.ptr, ln.d_rle.ptr, nrle, hipMemcpyDeviceToHost, h->stream3));
    }
    LX_HIP(h, hipStreamSynchronize(h->stream3));
    return LX_OK;
}

} // namespace lxi
