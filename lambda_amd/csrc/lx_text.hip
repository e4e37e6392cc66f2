// lx_text.hip -- .m8, .m9 and .sam records made on the device (gfx950): formatRecord and the group loop of renderTable
// (host/lx_output.cpp; seqan's writeRecord for BlastTabular behind myWriteRecord, src/search_output.hpp:463-733) and
// samFields / samLine restated as kernels, byte for byte.  The host code is the specification: its quirks are kept (unsigned
// wrap-around of coordinates that make no sense, the casts of the SAM tags, POS of a translated subject's minus strand taken from the
// QUERY length -- a signed number).
//
//   groups   lx_bam.hip's (bam_launch_groups): the row's group, the groups' first rows -- the comment lines and hit count of .m9,
//            FLAG's secondary bit, tag IH, --sam-bam-seq uniq, the group's LCA.
//   numbers  one lane per record: the texts snprintf makes of e_value, bit_score, identity, ppos and (float)e_value, by the exact
//            integer formatter of lx_numfmt.h, kept per record (TextNum).  The formatter's limb array is indexed at run time and
//            lives in scratch; it has this kernel to itself so that measure and emit keep their registers and occupancy.
//   measure  one lane per record runs the line's layout function over a writer that only counts -> the record's bytes; 64-bit
//            totals per kBamTile records for the host's range cuts.
//   emit     per range: an exclusive scan of the sizes (uint32), then one wavefront per record runs THE SAME layout function over
//            a writer that stages the line in kTextStage bytes of LDS: lane 0 puts the digits and separators, the strings (ids,
//            SEQ, QUAL, qs, number texts) are put by all lanes, and whenever the stage is full, and at the end, the 64 lanes store it to
//            global memory, 64 consecutive bytes an instruction.  Every value of the layout is the same in all lanes of the
//            wavefront (it depends on the record alone), so the control flow is uniform.
//
// Every byte of a range is written exactly once: nothing is read back, no atomics, the stream is the same on every run.
//
// Bounds: a record's bytes lie in [off, off + size) of its range by construction (one layout function for measure and emit, the
// validity of the ops taken from measure), and the stage's stores are clamped to the record's size besides; ops reads stay inside
// the host-checked [ops_off, ops_off + n_ops); reads of the queries' letters beyond the uploaded extent are answered with 'N' (of their qualities: '!') and
// never made; a number text has at most 19 characters (lx_numfmt.h: an F value below 10^15 with its sign), its slot 20.
#include <hip/hip_runtime.h>

#include "lx_level2.h"
#include "lx_numfmt.h"
#include "lx_text.h"

namespace lx
{
namespace
{

#include "lx_scan.h"

#include "lx_recdev.h"

static_assert(kBamTile == kL2ScanTile, "a size total per scan tile");
static_assert(sizeof(TextNum::t[0]) >= 20, "a number text fits its slot");

// ---- the two writers the layout functions run over

// measure: only the length
struct Count
{
    uint64_t n = 0;
    __device__ __forceinline__ uint64_t mark() const { return n; } // grows by the bytes put
    __device__ __forceinline__ void ch(uint8_t) { ++n; }
    __device__ __forceinline__ void dec(uint64_t v) { n += dec_digits(v); }
    template <class G>
    __device__ __forceinline__ void str(uint64_t len, G &&)
    {
        n += len;
    }
};

// emit: one wavefront's line through its stage in LDS; every lane holds the same fill and positions
struct Stage
{
    uint8_t * lds;
    uint8_t * out;  // the next byte of the record in global memory
    uint64_t  left; // bytes of the record not yet stored
    uint32_t  fill;
    int       lane;
    // grows by the bytes put (a flush takes `fill` bytes off both)
    __device__ __forceinline__ uint64_t mark() const { return fill - left; }
    __device__ __forceinline__ void flush()
    {
        __builtin_amdgcn_wave_barrier();
        uint32_t const k = (uint32_t)(fill < left ? fill : left);
        for (uint32_t i = lane; i < k; i += 64)
            out[i] = lds[i];
        out += k;
        left -= k;
        fill = 0;
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void ch(uint8_t c)
    {
        if (lane == 0)
            lds[fill] = c;
        if (++fill == kTextStage)
            flush();
    }
    __device__ __forceinline__ void dec(uint64_t v)
    {
        uint32_t const d = dec_digits(v); // (at most 20)
        if (fill + d > kTextStage)
            flush();
        if (lane == 0)
            put_dec(lds + fill, v, d);
        fill += d;
        if (fill == kTextStage)
            flush();
    }
    // len bytes, byte i = get(i)
    template <class G>
    __device__ __forceinline__ void str(uint64_t len, G && get)
    {
        for (uint64_t done = 0; done < len;)
        {
            uint64_t const room = kTextStage - fill;
            uint32_t const take = (uint32_t)(len - done < room ? len - done : room);
            for (uint32_t i = lane; i < take; i += 64)
                lds[fill + i] = get(done + i);
            fill += take;
            done += take;
            if (fill == kTextStage)
                flush();
        }
    }
};

template <class W>
__device__ __forceinline__ void put_sdec(W & w, int64_t v) // %d / %lld
{
    if (v < 0)
    {
        w.ch('-');
        w.dec(0 - (uint64_t)v);
    }
    else
        w.dec((uint64_t)v);
}
template <class W>
__device__ __forceinline__ void put_lit(W & w, char const * s, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        w.ch((uint8_t)s[i]);
}
template <class W>
__device__ __forceinline__ void put_num(W & w, TextCtx const & c, uint64_t k, int which)
{
    TextNum const & t = c.nums[k];
    w.str(t.len[which], [&](uint64_t i) { return (uint8_t)t.t[which][i]; });
}
// taxIdsOf: the subject's taxa, ';' between them, or "*"
template <class W>
__device__ __forceinline__ void put_taxa(W & w, BamCtx const & c, Rec const & r)
{
    if (r.st_lo == r.st_hi)
        w.ch('*');
    for (uint64_t x = r.st_lo; x < r.st_hi; ++x)
    {
        if (x > r.st_lo)
            w.ch(';');
        w.dec(c.s_tax_ids[x]);
    }
}
template <class W>
__device__ __forceinline__ void put_qname(W & w, BamCtx const & c, Rec const & r)
{
    w.str(r.qn_len, [&](uint64_t i) { return c.qn_blob[r.qn_at + i]; });
}
template <class W>
__device__ __forceinline__ void put_sname(W & w, TextCtx const & c, uint64_t k)
{
    uint32_t const s  = c.row_s[k];
    uint64_t const at = c.sn_off[s];
    w.str(c.sn_off[s + 1] - at, [&](uint64_t i) { return c.sn_blob[at + i]; });
}

// formatRecord's untranslate (the arithmetic is uint64_t's, as there)
__device__ __forceinline__ void untranslate(uint64_t a, uint64_t e, int frame, uint64_t len, uint64_t & first, uint64_t & last)
{
    uint64_t const shift = (uint64_t)(frame < 0 ? -frame : frame) - 1;
    uint64_t const lo = 3 * a + shift, hi = 3 * e + shift;
    if (frame >= 0)
    {
        first = lo + 1;
        last  = hi;
    }
    else
    {
        first = len - lo;
        last  = len - hi + 1;
    }
}

// ---- tabular: the comment lines of .m9 in front of a group's first record, then formatRecord's line
template <class W>
__device__ __forceinline__ void tab_record(W & w, TextCtx const & c, Rec const & r, uint64_t k)
{
    lx_blast_match const & b = *r.b;
    if (c.format == LX_OUT_BLAST_TAB_COMMENTS && r.first)
    {
        auto part = [&](int i)
        {
            uint32_t const at = c.comment_off[i];
            w.str(c.comment_off[i + 1] - at, [&](uint64_t x) { return c.comment[at + x]; });
        };
        uint64_t const at = c.qid_off[b.n_qid];
        part(0);
        w.str(c.qid_off[b.n_qid + 1] - at, [&](uint64_t i) { return c.qid_blob[at + i]; });
        part(1);
        w.dec(r.ih);
        part(2);
    }
    uint64_t qs = b.q_start + 1, qe = b.q_end, ss = b.s_start + 1, se = b.s_end;
    uint64_t const slen = c.s_lens[c.row_s[k]];
    if (c.b.q_trans)
        untranslate(b.q_start, b.q_end, b.q_frame, r.qlen, qs, qe);
    else if (b.q_frame < 0)
    {
        qs                = r.qlen - b.q_end + 1;
        qe                = r.qlen - b.q_start;
        uint64_t const t = ss;
        ss                = se;
        se                = t;
    }
    if (c.b.s_trans)
        untranslate(b.s_start, b.s_end, b.s_frame, slen, ss, se);
    for (uint32_t i = 0; i < c.n_cols; ++i)
    {
        if (i)
            w.ch('\t');
        switch (c.cols[i])
        {
            case kColQSeqId: put_qname(w, c.b, r); break;
            case kColSSeqId: put_sname(w, c, k); break;
            case kColQLen: w.dec(r.qlen); break;
            case kColSLen: w.dec(slen); break;
            case kColQStart: w.dec(qs); break;
            case kColQEnd: w.dec(qe); break;
            case kColSStart: w.dec(ss); break;
            case kColSEnd: w.dec(se); break;
            case kColEValue: put_num(w, c, k, kTextNumEValue); break;
            case kColBitScore: put_num(w, c, k, kTextNumBitScore); break;
            case kColScore: put_sdec(w, b.score); break;
            case kColLength: put_sdec(w, b.alignment_length); break;
            case kColPIdent: put_num(w, c, k, kTextNumPIdent); break;
            case kColNIdent: put_sdec(w, b.num_matches); break;
            case kColMismatch: put_sdec(w, b.num_mismatches); break;
            case kColPositive: put_sdec(w, b.num_positives); break;
            case kColGapOpen: put_sdec(w, b.num_gap_opens); break;
            case kColGaps: put_sdec(w, (int32_t)((uint32_t)b.num_gap_opens + (uint32_t)b.num_gap_extensions)); break;
            case kColPPos: put_num(w, c, k, kTextNumPPos); break;
            case kColFrames:
                put_sdec(w, b.q_frame);
                w.ch('/');
                put_sdec(w, b.s_frame);
                break;
            case kColQFrame: put_sdec(w, b.q_frame); break;
            case kColSFrame: put_sdec(w, b.s_frame); break;
            case kColSTaxIds: put_taxa(w, c.b, r); break;
            case kColLcaTaxId: w.dec(r.lca); break;
            default: break;
        }
    }
    w.ch('\n');
}

// ---- SAM

// the runs of valid ops from the last to the first
template <class F>
__device__ __forceinline__ void walk_runs_back(uint8_t const * o, uint32_t n, F && run)
{
    for (uint32_t i = n; i > 0;)
    {
        uint8_t const  op = o[i - 1];
        uint32_t const i1 = i;
        while (i > 0 && o[i - 1] == op)
            --i;
        run(op, i1 - i);
    }
}

// cigarOf's text: the elements of walk_cigar, from the last to the first on the minus strand
template <class W>
__device__ __forceinline__ void put_cigar(W & w, BamCtx const & c, Rec const & r, uint8_t const * o, uint32_t n_ops)
{
    auto el = [&](uint32_t op, uint64_t len)
    {
        w.dec(len);
        w.ch((uint8_t)("MIDNSH"[op]));
    };
    if (!r.minus)
    {
        walk_cigar(c, r, o, n_ops, el);
        return;
    }
    if (c.hard)
    {
        if (r.rfc + r.rclip > 0)
            el(5u, r.rfc + r.rclip);
    }
    else
    {
        if (r.rfc > 0)
            el(5u, r.rfc);
        if (r.rclip > 0)
            el(4u, r.rclip);
    }
    walk_runs_back(o, n_ops, [&](uint8_t op, uint32_t cnt) { el(op == 'M' ? 0u : op == 'I' ? 1u : 2u, (uint64_t)cnt * r.trans); });
    if (c.hard)
    {
        if (r.lfc + r.lclip > 0)
            el(5u, r.lfc + r.lclip);
    }
    else
    {
        if (r.lclip > 0)
            el(4u, r.lclip);
        if (r.lfc > 0)
            el(5u, r.lfc);
    }
}

template <class W>
__device__ __forceinline__ void put_tag(W & w, char const * key, char type)
{
    w.ch('\t');
    w.ch((uint8_t)key[0]);
    w.ch((uint8_t)key[1]);
    w.ch(':');
    w.ch((uint8_t)type);
    w.ch(':');
}

// the line of samLine and the tags of samTags (host/lx_output.cpp); a.n_cigar / a.oc_len: whether the CIGAR / tag OC is made of the ops
// ("*" otherwise: another program, or a byte that is no op)
template <class W>
__device__ __forceinline__ void sam_record(W & w, TextCtx const & tc, Rec const & r, uint64_t k, BamAux a)
{
    BamCtx const &         c = tc.b;
    lx_blast_match const & b = *r.b;
    uint8_t const * const  o = c.ops + b.ops_off;
    put_qname(w, c, r);
    w.ch('\t');
    w.dec((r.first ? 0u : 256u) | (r.minus ? 16u : 0u));
    w.ch('\t');
    put_sname(w, tc, k);
    w.ch('\t');
    uint64_t pos1 = (uint64_t)r.pos + 1;
    if (c.s_trans && (int64_t)pos1 < 0) // samLine: signed where the subject is translated
    {
        w.ch('-');
        pos1 = 0 - pos1;
    }
    w.dec(pos1);
    put_lit(w, "\t255\t", 5);
    uint64_t const before = w.mark();
    if (a.n_cigar)
        put_cigar(w, c, r, o, b.n_ops);
    if (w.mark() == before) // (another program, a byte that is no op, or cigarOf's list without an element)
        w.ch('*');
    put_lit(w, "\t*\t0\t0\t", 7);
    if (r.l_seq)
        w.str(r.l_seq, [&](uint64_t i) { return seq_letter(c, r, i); });
    else
        w.ch('*');
    // QUAL: where SEQ is, over the same letters
    w.ch('\t');
    if (c.q_qual && r.l_seq)
        w.str(r.l_seq, [&](uint64_t i) { return qual_letter(c, r, i); });
    else
        w.ch('*');
    uint32_t const t = c.tags;
    if (t & tagBit(kTagEValue))
    {
        put_tag(w, "ae", 'f');
        put_num(w, tc, k, kTextNumAe);
    }
    if (t & tagBit(kTagBitScore))
    {
        put_tag(w, "AS", 'i');
        w.dec((uint16_t)(int32_t)b.bit_score);
    }
    if (t & tagBit(kTagScore))
    {
        put_tag(w, "ar", 'i');
        w.dec((uint8_t)b.score);
    }
    if (t & tagBit(kTagPIdent))
    {
        put_tag(w, "ai", 'i');
        w.dec((uint8_t)(int32_t)b.identity);
    }
    if (t & tagBit(kTagPPos))
    {
        put_tag(w, "ap", 'i');
        w.dec(ppos_u16(b.num_positives, b.alignment_length));
    }
    if (t & tagBit(kTagQFrame))
    {
        put_tag(w, "qf", 'i');
        put_sdec(w, (int8_t)b.q_frame);
    }
    if (t & tagBit(kTagSFrame))
    {
        put_tag(w, "sf", 'i');
        put_sdec(w, (int8_t)b.s_frame);
    }
    if (t & tagBit(kTagSTaxIds))
    {
        put_tag(w, "st", 'Z');
        put_taxa(w, c, r);
    }
    if (t & tagBit(kTagLcaId))
    {
        put_tag(w, "ls", 'Z');
        if (r.name_len == 0xffffffffu)
            w.ch('*');
        else
            w.str(r.name_len, [&](uint64_t i) { return c.name_blob[r.name_off + i]; });
    }
    if (t & tagBit(kTagLcaTaxId))
    {
        put_tag(w, "lt", 'i');
        w.dec(r.lca);
    }
    if (t & tagBit(kTagProtSeq))
    {
        put_tag(w, "qs", 'Z');
        if (r.qs_len)
            w.str(r.qs_len, [&](uint64_t i) { return qs_letter(c, r, i); });
        else
            w.ch('*');
    }
    if (t & tagBit(kTagProtCigar))
    {
        put_tag(w, "OC", 'Z');
        // protCigarOf; a text without elements is "*"
        uint64_t const right = r.frame_len >= b.q_end ? r.frame_len - b.q_end : 0;
        if (a.oc_len && (b.q_start || b.n_ops || right))
            walk_oc(c, r, o, b.n_ops,
                    [&](uint8_t op, uint64_t cnt)
                    {
                        w.dec(cnt);
                        w.ch(op);
                    });
        else
            w.ch('*');
    }
    if (t & tagBit(kTagEditDistance))
    {
        put_tag(w, "NM", 'i');
        w.dec((uint32_t)(b.alignment_length - b.num_matches));
    }
    if (t & tagBit(kTagMatchCount))
    {
        put_tag(w, "IH", 'i');
        w.dec(r.ih);
    }
    w.ch('\n');
}

template <class W>
__device__ __forceinline__ void record(W & w, TextCtx const & c, Rec const & r, uint64_t k, BamAux a)
{
    if (c.format == LX_OUT_SAM)
        sam_record(w, c, r, k, a);
    else
        tab_record(w, c, r, k);
}

// ---- kernels

__global__ __launch_bounds__(256) void text_numbers_kernel(TextCtx c)
{
    uint64_t const k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= c.b.n)
        return;
    lx_blast_match const & b = c.b.rows[k];
    TextNum &              t = c.nums[k];
    auto bits = [](double v) { return (uint64_t)__double_as_longlong(v); };
    if (c.need & 1u << kTextNumEValue)
        t.len[kTextNumEValue] = (uint8_t)num_format(kNumE1, bits(b.e_value), t.t[kTextNumEValue]);
    if (c.need & 1u << kTextNumBitScore)
        t.len[kTextNumBitScore] = (uint8_t)num_format(kNumF1, bits(b.bit_score), t.t[kTextNumBitScore]);
    if (c.need & 1u << kTextNumPIdent)
        t.len[kTextNumPIdent] = (uint8_t)num_format(kNumF2, bits((double)b.identity), t.t[kTextNumPIdent]);
    if (c.need & 1u << kTextNumPPos)
        t.len[kTextNumPPos] = (uint8_t)num_format(kNumF2, bits(ppos_double(b.num_positives, b.alignment_length)), t.t[kTextNumPPos]);
    if (c.need & 1u << kTextNumAe)
        t.len[kTextNumAe] = (uint8_t)num_format(kNumGFloat, bits((double)(float)b.e_value), t.t[kTextNumAe]);
}

__global__ __launch_bounds__(256) void text_measure_kernel(TextCtx c, unsigned long long * tile_total)
{
    uint64_t const k    = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t       size = 0;
    if (k < c.b.n)
    {
        Rec const r = rec_of(c.b, k);
        BamAux    a{0, 0};
        if (c.format == LX_OUT_SAM)
        {
            bool const need_oc = (c.b.tags & tagBit(kTagProtCigar)) && !c.b.is_n;
            bool const valid   = (r.cig || need_oc) ? ops_valid(c.b.ops + r.b->ops_off, r.b->n_ops) : true;
            a                  = BamAux{r.cig && valid ? 1u : 0u, need_oc && valid ? 1u : 0u};
        }
        Count w;
        record(w, c, r, k, a);
        size        = w.n;
        c.b.aux[k]  = a;
        c.b.size[k] = (uint32_t)size;
    }
    // the tile's total: a wavefront lies in one tile (kBamTile is a multiple of 64)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        size += (uint64_t)__shfl_down((unsigned long long)size, off);
    if ((threadIdx.x & 63) == 0 && k < c.b.n)
        atomicAdd(&tile_total[k / kBamTile], (unsigned long long)size);
}

__global__ __launch_bounds__(kTextEmitBlock) void text_emit_kernel(TextCtx c, uint64_t first, uint64_t count, uint32_t const * off, uint8_t * out)
{
    __shared__ uint8_t stage[kTextEmitRecs][kTextStage];
    uint64_t const     j = (uint64_t)blockIdx.x * kTextEmitRecs + (threadIdx.x >> 6);
    if (j >= count)
        return;
    uint64_t const k = first + j;
    Rec const      r = rec_of(c.b, k);
    Stage          w{stage[threadIdx.x >> 6], out + off[j], c.b.size[k], 0u, (int)(threadIdx.x & 63)};
    record(w, c, r, k, c.b.aux[k]);
    w.flush();
}

uint64_t scan_tiles(uint64_t n)
{
    return (n + kL2ScanTile - 1) / kL2ScanTile;
}

} // namespace

hipError_t text_launch_numbers(TextCtx const & c, hipStream_t stream)
{
    if (c.b.n == 0 || c.need == 0)
        return hipSuccess;
    hipLaunchKernelGGL(text_numbers_kernel, dim3((unsigned)((c.b.n + 255) / 256)), dim3(256), 0, stream, c);
    return hipGetLastError();
}

hipError_t text_launch_measure(TextCtx const & c, uint64_t * tile_total, hipStream_t stream)
{
    if (c.b.n == 0)
        return hipSuccess;
    hipError_t const e = hipMemsetAsync(tile_total, 0, scan_tiles(c.b.n) * sizeof(uint64_t), stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(text_measure_kernel, dim3((unsigned)((c.b.n + 255) / 256)), dim3(256), 0, stream, c,
                       reinterpret_cast<unsigned long long *>(tile_total));
    return hipGetLastError();
}

hipError_t text_launch_emit(TextCtx const & c, uint64_t first, uint64_t count, uint32_t * off, uint32_t * block_tot, uint8_t * out, hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    uint64_t const tiles = scan_tiles(count);
    dim3 const     grid((unsigned)tiles), block(kL2ScanBlock);
    SizeVal const  sv{c.b.size + first};
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, SizeVal>), grid, block, 0, stream, sv, count, block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), block, 0, stream, block_tot, tiles);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, SizeVal, OffOut>), grid, block, 0, stream, sv, OffOut{off}, count, block_tot);
    hipLaunchKernelGGL(text_emit_kernel, dim3((unsigned)((count + kTextEmitRecs - 1) / kTextEmitRecs)), dim3(kTextEmitBlock), 0, stream, c, first,
                       count, off, out);
    return hipGetLastError();
}

} // namespace lx
