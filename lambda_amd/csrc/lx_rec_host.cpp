// lx_rec_host.cpp -- what the host sides of the two device record writers share (lx_rec_host.h): lx_bam_host.cpp (BAM) and
// lx_text_host.cpp (.m8 / .m9 / .sam) keep their checks, their extra uploads, their measure and emit launches and their entry points.
//
// rec_inputs checks what both check beyond the host writer's refusals (the extent of the ops, the kernels' counters) and flattens
// what the kernels read -- rows, ops, the queries' letters, qualities (opt.q_qual) and lengths, the first words of their ids, the
// taxonomy lists, one LCA (and name) per query group from the forward cursor the host writer uses (LcaCursor), the genetic code over
// the 125 DNA5 triplets -- and uploads it; the groups kernels run.  After the writer's measure kernel rec_ranges reads the 64-bit size
// totals of the tiles and cuts the list into RANGES of whole tiles whose bytes stay within LX_OPT_BAM_RANGE_BYTES (a tile that alone
// exceeds it is a range of its own).  Per range the writer's emit (scan + emit) fills the handle's stream buffer, and the range is
// copied down (rec_drain) or compressed where it stands (rec_encode_ranges): the whole 65 280-byte blocks go through the BGZF encoder
// (lxi::bgzf_compress_dev), and the rest -- less than a block -- is carried to the front of the next range's buffer.
#include <unordered_map>

#include "lx_bgzf.h"
#include "lx_rec_host.h"

using namespace lxi;

namespace
{

constexpr uint64_t kDefaultRange = 256ull << 20;
constexpr uint64_t kMaxRows      = (1ull << 31) - 16;
constexpr uint64_t kMaxQlen      = 1ull << 30; // a record's bytes are counted in 32 bits
constexpr uint32_t kMaxOps       = 1u << 26;
constexpr uint64_t kMaxName      = kRecMaxName;

} // namespace

namespace lxi
{

int rec_refuse(lx_handle * h, char const * who, int rc)
{
    return fail(h, rc, "%s: %s", who, *lx_last_output_error() ? lx_last_output_error() : "bad arguments");
}

int rec_begin(lx_handle * h)
{
    int const rc = bind(h);
    if (rc)
        return rc;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    return LX_OK;
}

int rec_inputs(lx_handle * h, char const * who, int phase, OutputRequest const & rq, uint32_t tags, bool with_ops, lx_blast_match const * m,
               uint64_t n, uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
               uint64_t const * q_ascii_off, RecJob & job)
{
    auto                      refuse = rec_refuse;
    lx_output_options const & opt    = rq.opt;
    int                       rc     = LX_OK;
    if (!with_ops)
    {
        ops       = nullptr;
        ops_bytes = 0;
    }
    if ((!ops && ops_bytes) || (names->n_q && (!names->q_ids || !names->q_lens)))
        return refuse(h, who, LX_EINVAL);
    if (n > kMaxRows)
    {
        set_output_error("more records than the device writer takes in one call (2^31 - 16)");
        return refuse(h, who, LX_EINVAL);
    }
    for (uint64_t k = 0; with_ops && k < n; ++k)
        if (!lx_slice_ok(m[k].ops_off, m[k].n_ops, ops_bytes) || m[k].n_ops > kMaxOps)
        {
            set_output_error("a record's ops lie outside the ops buffer");
            return refuse(h, who, LX_EINVAL);
        }
    bool const     ascii = q_res_ascii && q_ascii_off;
    uint64_t const n_q   = names->n_q;
    uint64_t       extent = 0;
    for (uint64_t i = 0; i < n_q; ++i)
    {
        if (names->q_lens[i] > kMaxQlen)
        {
            set_output_error("a query longer than the device writer takes (2^30)");
            return refuse(h, who, LX_EINVAL);
        }
        if (ascii)
            extent = std::max(extent, q_ascii_off[i] + names->q_lens[i]);
    }
    lx::BamCtx & c = job.c;
    c.tags         = tags;
    c.sam_seq      = opt.sam_seq;
    c.hard         = opt.sam_hard_clip != 0;
    c.is_n         = rq.is_n;
    c.q_trans      = rq.q_trans;
    c.s_trans      = rq.s_trans;
    c.n            = n;
    if (n == 0)
        return LX_OK;

    // ---- what the kernels read
    // first words of the query ids (firstWord of host/lx_output.cpp: up to the first blank or tab)
    std::vector<uint64_t> qn_off(n_q + 1, 0);
    std::atomic<bool>     name_too_long{false};
    parallel_ranges(n_q, host_threads(n_q),
                    [&](unsigned, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t i = lo; i < hi; ++i)
                        {
                            qn_off[i + 1] = names->q_ids[i] ? std::strcspn(names->q_ids[i], " \t") : 0;
                            if (qn_off[i + 1] > kMaxName)
                                name_too_long = true;
                        }
                    });
    if (name_too_long)
    {
        set_output_error("a query id longer than the device writer takes (2^20)");
        return refuse(h, who, LX_EINVAL);
    }
    for (uint64_t i = 0; i < n_q; ++i)
        qn_off[i + 1] += qn_off[i];
    std::vector<uint8_t> qn_blob(qn_off[n_q]);
    parallel_ranges(n_q, host_threads(n_q),
                    [&](unsigned, uint64_t lo, uint64_t hi)
                    {
                        for (uint64_t i = lo; i < hi; ++i)
                            if (qn_off[i + 1] > qn_off[i])
                                std::memcpy(qn_blob.data() + qn_off[i], names->q_ids[i], qn_off[i + 1] - qn_off[i]);
                    });
    // one LCA per query group, from the host writer's forward-only cursor over (lca_qid, lca_tax); the name of tag ls beside it
    bool const            want_lca = tags & (lx::tagBit(lx::kTagLcaTaxId) | lx::tagBit(lx::kTagLcaId));
    std::vector<uint32_t> grp_tab; // [groups] lca, [groups] name offset, [groups] name length
    std::vector<uint8_t>  name_blob;
    uint64_t              groups = 0;
    if (want_lca)
    {
        std::vector<uint32_t> lca, noff, nlen;
        std::unordered_map<uint32_t, std::pair<uint32_t, uint32_t>> seen;
        LcaCursor                                                    cursor;
        for (uint64_t lo = 0; lo < n;)
        {
            uint64_t hi = lo + 1;
            while (hi < n && m[hi].n_qid == m[lo].n_qid)
                ++hi;
            uint32_t const t = cursor.of(opt, m[lo].n_qid);
            lca.push_back(t);
            std::pair<uint32_t, uint32_t> name{0u, 0xffffffffu};
            if ((tags & lx::tagBit(lx::kTagLcaId)) && opt.tax_names && opt.tax && t < opt.tax->n_taxa && opt.tax_names[t])
            {
                auto const it = seen.find(t);
                if (it != seen.end())
                    name = it->second;
                else
                {
                    size_t const len = std::strlen(opt.tax_names[t]);
                    if (len > kMaxName || name_blob.size() + len > 0xf0000000ull)
                    {
                        set_output_error("taxon names longer than the device writer takes");
                        return refuse(h, who, LX_EINVAL);
                    }
                    name = {(uint32_t)name_blob.size(), (uint32_t)len};
                    name_blob.insert(name_blob.end(), opt.tax_names[t], opt.tax_names[t] + len);
                    seen.emplace(t, name);
                }
            }
            noff.push_back(name.first);
            nlen.push_back(name.second);
            lo = hi;
        }
        groups = lca.size();
        grp_tab.reserve(3 * groups);
        grp_tab.insert(grp_tab.end(), lca.begin(), lca.end());
        grp_tab.insert(grp_tab.end(), noff.begin(), noff.end());
        grp_tab.insert(grp_tab.end(), nlen.begin(), nlen.end());
    }
    // tag qs of a translated query: the call's genetic code over all 125 DNA5 triplets, each translated by lx_translate_six_frames
    uint8_t codon[125];
    bool    have_codon = false;
    if (c.q_trans && (tags & lx::tagBit(lx::kTagProtSeq)))
    {
        have_codon = true;
        for (uint8_t x = 0; x < 125 && have_codon; ++x)
        {
            uint8_t const nt[3] = {(uint8_t)(x / 25), (uint8_t)(x / 5 % 5), (uint8_t)(x % 5)};
            uint8_t       aa[8];
            uint64_t      fo[6], fl[6];
            have_codon = lx_translate_six_frames(nt, 3, opt.genetic_code, aa, sizeof(aa), fo, fl) == LX_OK;
            codon[x]   = (uint8_t)lambda_amd::kSeqanOrder[std::min<uint8_t>(aa[fo[0]], 26)];
        }
    }

    // ---- upload
    auto & B = h->bam;
    if ((rc = rec_upload(h, B.d_rows, m, n, c.rows)) || (rc = rec_upload(h, B.d_ops, ops, ops_bytes, c.ops)) ||
        (rc = rec_upload(h, B.d_qlens, names->q_lens, n_q, c.q_lens)) || (rc = rec_upload(h, B.d_qn_off, qn_off.data(), n_q + 1, c.qn_off)) ||
        (rc = rec_upload(h, B.d_qn_blob, qn_blob.data(), qn_blob.size(), c.qn_blob)))
        return rc;
    if (ascii && ((rc = rec_upload(h, B.d_ascii, q_res_ascii, extent, c.q_ascii)) || (rc = rec_upload(h, B.d_ascii_off, q_ascii_off, n_q, c.q_ascii_off))))
        return rc;
    c.q_ascii_bytes = ascii ? extent : 0;
    // the qualities go up only where a record can carry them: a SAM or BAM writer (the ones that read the ops), a DNA query, SEQ written
    if (ascii && opt.q_qual && with_ops && (c.is_n || c.q_trans) && opt.sam_seq != LX_SAM_SEQ_NEVER)
    {
        if ((rc = rec_upload(h, B.d_qual, opt.q_qual, extent, c.q_qual)))
            return rc;
        c.q_qual_bytes = extent;
    }
    if ((tags & lx::tagBit(lx::kTagSTaxIds)) && opt.tax && opt.tax->s_tax_off && (opt.tax->s_tax_ids || opt.tax->s_tax_off[opt.tax->n_s] == 0))
    {
        c.tax_n_s = opt.tax->n_s;
        if ((rc = rec_upload(h, B.d_tax_off, opt.tax->s_tax_off, c.tax_n_s + 1, c.s_tax_off)) ||
            (rc = rec_upload(h, B.d_tax_ids, opt.tax->s_tax_ids, opt.tax->s_tax_off[c.tax_n_s], c.s_tax_ids)))
            return rc;
    }
    if (want_lca)
    {
        uint32_t const * tab = nullptr;
        if ((rc = rec_upload(h, B.d_grp_tab, grp_tab.data(), grp_tab.size(), tab)))
            return rc;
        c.grp_lca = tab;
        if (tags & lx::tagBit(lx::kTagLcaId))
        {
            c.grp_name_off = tab + groups;
            c.grp_name_len = tab + 2 * groups;
            if ((rc = rec_upload(h, B.d_name_blob, name_blob.data(), name_blob.size(), c.name_blob)))
                return rc;
        }
    }
    if (have_codon && (rc = rec_upload(h, B.d_codon, codon, (uint64_t)125, c.codon)))
        return rc;
    uint64_t const tiles = (n + lx::kBamTile - 1) / lx::kBamTile;
    if ((rc = ensure(h, B.d_grp, n * 4)) || (rc = ensure(h, B.d_grp_first, (n + 1) * 4)) || (rc = ensure(h, B.d_aux, n * sizeof(lx::BamAux))) ||
        (rc = ensure(h, B.d_size, n * 4)) || (rc = ensure(h, B.d_off, n * 4)) ||
        (rc = ensure(h, B.d_scan, (tiles + 2) * 4)) || (rc = ensure(h, B.d_tiles, tiles * 8)) || (rc = ensure_pinned(h, B.p_tiles, tiles * 8, kRoom)))
        return rc;
    c.grp       = static_cast<uint32_t *>(B.d_grp.ptr);
    c.grp_first = static_cast<uint32_t *>(B.d_grp_first.ptr);
    c.aux       = static_cast<lx::BamAux *>(B.d_aux.ptr);
    c.size      = static_cast<uint32_t *>(B.d_size.ptr);

    // ---- groups
    PhaseTimer t(h, h->stream, phase);
    LX_HIP(h, lx::bam_launch_groups(c, static_cast<uint32_t *>(B.d_scan.ptr), h->stream));
    t.close();
    LX_HIP(h, hipStreamSynchronize(h->stream)); // (the uploads' host arrays go with this frame)
    return LX_OK;
}

int rec_ranges(lx_handle * h, char const * who, RecJob & job)
{
    auto &            B     = h->bam;
    uint64_t const    n     = job.c.n;
    uint64_t const    tiles = (n + lx::kBamTile - 1) / lx::kBamTile;
    hipStream_t const s     = h->stream;
    // ---- the tiles' totals for the cuts
    LX_HIP(h, hipMemcpyAsync(B.p_tiles.ptr, B.d_tiles.ptr, tiles * 8, hipMemcpyDeviceToHost, s));
    LX_HIP(h, hipStreamSynchronize(s));
    uint64_t const * const tot    = static_cast<uint64_t const *>(B.p_tiles.ptr);
    uint64_t const         budget = h->opt_bam_range ? h->opt_bam_range : kDefaultRange;
    for (uint64_t t = 0; t < tiles;)
    {
        RecRange r{t * lx::kBamTile, 0, 0};
        do
        {
            if (tot[t] > 0xf0000000ull)
                return fail(h, LX_EINVAL, "%s: %llu bytes of records in one tile of %llu: more than a range holds", who, (unsigned long long)tot[t],
                            (unsigned long long)lx::kBamTile);
            r.bytes += tot[t];
            ++t;
        } while (t < tiles && r.bytes + tot[t] <= budget);
        r.count       = std::min(n, t * lx::kBamTile) - r.first;
        job.max_range = std::max(job.max_range, r.bytes);
        job.total += r.bytes;
        job.ranges.push_back(r);
    }
    return LX_OK;
}

int rec_drain(lx_handle * h, RecJob const & job, RecEmit const & emit, std::string & bytes)
{
    int rc = ensure(h, h->bam.d_stream, std::max<uint64_t>(job.max_range, 16));
    if (rc)
        return rc;
    uint8_t * const d = static_cast<uint8_t *>(h->bam.d_stream.ptr);
    for (RecRange const & r : job.ranges)
    {
        if ((rc = emit(r, d)))
            return rc;
        size_t const at = bytes.size();
        bytes.resize(at + r.bytes);
        LX_HIP(h, hipMemcpyAsync(&bytes[at], d, r.bytes, hipMemcpyDeviceToHost, h->stream));
        LX_HIP(h, hipStreamSynchronize(h->stream));
    }
    return LX_OK;
}

int rec_stream_front(lx_handle * h, RecJob const & job, std::string const & front, uint64_t tail_bytes)
{
    // what is carried (the header in front of the first range, less than a block later) + a range + the tail
    int const rc = ensure(h, h->bam.d_stream, std::max<uint64_t>(front.size(), lx::kBgzfBlock) + job.max_range + tail_bytes + 16);
    if (rc)
        return rc;
    if (!front.empty())
        LX_HIP(h, hipMemcpyAsync(h->bam.d_stream.ptr, front.data(), front.size(), hipMemcpyHostToDevice, h->stream));
    return LX_OK;
}

int rec_encode_ranges(lx_handle * h, RecJob const & job, RecEmit const & emit, uint64_t * carry, std::string const * tail, bool final,
                      MemberSink const & sink)
{
    uint8_t * const   d = static_cast<uint8_t *>(h->bam.d_stream.ptr);
    hipStream_t const s = h->stream;
    uint64_t          c = *carry;
    // (no ranges: one step without records, for what stands at the front and the tail)
    size_t const steps = std::max<size_t>(job.ranges.size(), 1);
    for (size_t i = 0; i < steps; ++i)
    {
        bool const last = i + 1 == steps;
        uint64_t   have = c;
        if (i < job.ranges.size())
        {
            int const rc = emit(job.ranges[i], d + c);
            if (rc)
                return rc;
            have += job.ranges[i].bytes;
        }
        if (last && tail && !tail->empty())
        {
            LX_HIP(h, hipMemcpyAsync(d + have, tail->data(), tail->size(), hipMemcpyHostToDevice, s));
            have += tail->size();
        }
        uint64_t const whole = last && final ? have : have / lx::kBgzfBlock * lx::kBgzfBlock;
        if (whole)
        {
            int const rc = bgzf_compress_dev(h, d, whole, sink);
            if (rc)
                return rc;
        }
        c = have - whole;
        if (c && whole) // (whole is at least a block, the rest less: the two do not overlap)
            LX_HIP(h, hipMemcpyAsync(d, d + whole, c, hipMemcpyDeviceToDevice, s));
    }
    if (final) // (otherwise the caller, who takes the carry away, waits for the stream)
        LX_HIP(h, hipStreamSynchronize(s));
    *carry = c;
    return LX_OK;
}

MemberSink rec_collect(std::vector<uint8_t> & packed)
{
    return [&packed](uint8_t const * members, uint64_t bytes) -> int
    {
        packed.insert(packed.end(), members, members + bytes);
        return LX_OK;
    };
}

int rec_write_file(lx_handle * h, char const * path, void const * data, size_t bytes)
{
    std::FILE * f = std::fopen(path, "wb");
    if (!f)
        return fail(h, LX_EINVAL, "cannot open %s", path);
    bool ok = std::fwrite(data, 1, bytes, f) == bytes;
    ok      = (std::fclose(f) == 0) && ok;
    return ok ? LX_OK : fail(h, LX_EINVAL, "error while writing %s (disk full?)", path);
}

int rec_append_ranges(lx_handle * h, RecJob const & job, RecEmit const & emit, uint8_t * d_carry, uint64_t * carry, MemberSink const & sink)
{
    std::string const none;
    int               rc = rec_stream_front(h, job, none, 0);
    if (rc)
        return rc;
    uint8_t * const   d = static_cast<uint8_t *>(h->bam.d_stream.ptr);
    hipStream_t const s = h->stream;
    uint64_t          c = *carry;
    if (c >= lx::kBgzfBlock)
        return fail(h, LX_EINVAL, "lx_out_append: a carry of a block or more");
    if (c)
        LX_HIP(h, hipMemcpyAsync(d, d_carry, c, hipMemcpyDeviceToDevice, s));
    if ((rc = rec_encode_ranges(h, job, emit, &c, nullptr, false, sink)))
        return rc;
    if (c)
        LX_HIP(h, hipMemcpyAsync(d_carry, d, c, hipMemcpyDeviceToDevice, s));
    LX_HIP(h, hipStreamSynchronize(s));
    *carry = c;
    return LX_OK;
}

} // namespace lxi
