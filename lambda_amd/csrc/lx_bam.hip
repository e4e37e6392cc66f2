// lx_bam.hip -- BAM alignment records made on the device (gfx950): samFields and bamRecord
// (host/lx_output.cpp; myWriteRecord, src/search_output.hpp:463-733) restated as kernels, byte for byte.  The host
// code is the specification: its quirks are kept (the CIGAR's runs and clips as cigarOf makes them, the truncated n_cigar_op /
// l_read_name / bin, POS of a translated subject's minus strand taken from the QUERY length, the wrapping casts of the tags).
//
//   groups   a head flag per row (n_qid differs from the row before) and a sum scan (lx_scan.h): the row's group, the groups' first
//            rows -- FLAG's secondary bit, tag IH, --sam-bam-seq uniq's "first of its group", the group's LCA.
//   measure  one lane per record walks its ops: CIGAR elements, the length of OC's text, l_seq, the tags' bytes -> the record's size;
//            64-bit totals per kBamTile records for the host's range cuts.
//   emit     per range: an exclusive scan of the sizes (uint32), then one wavefront per record.  Lane 0 writes the fixed fields, the
//            numeric tags, the CIGAR and the decimal texts (it walks the ops once more: a wavefront's latency hides behind the other
//            wavefronts of the CU); qname, SEQ, QUAL and the Z strings qs / ls are strided over the 64 lanes.
//
// Stores: DIRECT BYTE STORES TO GLOBAL MEMORY, no LDS staging.  A record starts at an arbitrary byte and has an arbitrary length (36
// bytes to more than a BGZF block for a long read with SEQ), so a staged copy could neither be bounded by an LDS budget nor written
// back with aligned dword stores without a read-modify-write at both ends shared with the neighbouring records.  The strided parts
// write 64 consecutive bytes per wavefront instruction, which the memory pipeline merges into whole-line writes; the serial parts are
// a few dozen bytes per record in one or two lines that stay in L2 until the wavefront's other stores complete them.  Every byte of a
// range is written exactly once: nothing is read back, no atomics, the stream is the same on every run.
//
// Bounds: a record's bytes lie in [off, off + size) of its range by construction (emit lays out with the function measure sized with,
// and takes the two walked counts from measure); ops reads stay inside the host-checked [ops_off, ops_off + n_ops); reads of the
// queries' letters beyond the uploaded extent are answered with 'N' and never made, those of their qualities with '!'.
//
// What the text writer (lx_text.hip) needs as well -- rec_of, the op walks, reverse complement, the frame's codon, the scan functors --
// is in lx_recdev.h.
#include <hip/hip_runtime.h>

#include "lx_bam.h"
#include "lx_level2.h"

namespace lx
{
namespace
{

#include "lx_scan.h"

#include "lx_recdev.h"

static_assert(kBamTile == kL2ScanTile, "a size total per scan tile");

// bamRecord's 4-bit code
__device__ __forceinline__ uint32_t nt16(uint8_t c)
{
    constexpr char k[17] = "=ACMGRSVTWYHKDBN";
    c                    = up(c);
    uint32_t code        = 15;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (c == (uint8_t)k[i])
            code = (uint32_t)i;
    return code;
}
__device__ __forceinline__ int reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14)
        return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17)
        return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20)
        return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23)
        return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26)
        return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
// bytes of the optional fields but the text of OC
__device__ __forceinline__ uint64_t tag_bytes(BamCtx const & c, Rec const & r, uint32_t oc_len)
{
    uint32_t const t = c.tags;
    uint64_t       s = 0;
    s += (t & tagBit(kTagEValue)) ? 7 : 0;
    s += (t & tagBit(kTagBitScore)) ? 5 : 0;
    s += (t & tagBit(kTagScore)) ? 4 : 0;
    s += (t & tagBit(kTagPIdent)) ? 4 : 0;
    s += (t & tagBit(kTagPPos)) ? 5 : 0;
    s += (t & tagBit(kTagQFrame)) ? 4 : 0;
    s += (t & tagBit(kTagSFrame)) ? 4 : 0;
    if (t & tagBit(kTagSTaxIds))
    {
        uint64_t len = 0;
        for (uint64_t x = r.st_lo; x < r.st_hi; ++x)
            len += dec_digits(c.s_tax_ids[x]) + (x > r.st_lo ? 1 : 0);
        s += 3 + (len ? len : 1) + 1;
    }
    if (t & tagBit(kTagLcaId))
        s += 3 + (r.name_len == 0xffffffffu ? 1u : r.name_len) + 1;
    s += (t & tagBit(kTagLcaTaxId)) ? 7 : 0;
    if (t & tagBit(kTagProtSeq))
        s += 3 + (r.qs_len ? r.qs_len : 1) + 1;
    if (t & tagBit(kTagProtCigar))
        s += 3 + (uint64_t)oc_len + 1;
    s += (t & tagBit(kTagEditDistance)) ? 7 : 0;
    s += (t & tagBit(kTagMatchCount)) ? 7 : 0;
    return s;
}
__global__ __launch_bounds__(256) void bam_measure_kernel(BamCtx c, unsigned long long * tile_total)
{
    uint64_t const k    = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t       size = 0;
    if (k < c.n)
    {
        Rec const              r = rec_of(c, k);
        lx_blast_match const & b = *r.b;
        uint8_t const * const  o = c.ops + b.ops_off;
        uint32_t               runs = 0, oc = 0;
        bool const             need_oc = (c.tags & tagBit(kTagProtCigar)) && !c.is_n;
        bool const             valid   = (r.cig || need_oc) ? walk_runs(o, b.n_ops,
                                                                    [&](uint8_t, uint32_t cnt)
                                                                    {
                                                                        ++runs;
                                                                        oc += dec_digits(cnt) + 1;
                                                                    })
                                                            : true;
        uint32_t n_cigar = 0;
        if (r.cig && valid)
        {
            n_cigar = runs;
            if (c.hard)
                n_cigar += (r.lfc + r.lclip > 0 ? 1 : 0) + (r.rfc + r.rclip > 0 ? 1 : 0);
            else
                n_cigar += (r.lfc > 0 ? 1 : 0) + (r.lclip > 0 ? 1 : 0) + (r.rclip > 0 ? 1 : 0) + (r.rfc > 0 ? 1 : 0);
        }
        uint32_t oc_len = 1; // "*"
        if (need_oc && valid)
        {
            // protCigarOf: clips in protein space, never reversed
            uint64_t const right = r.frame_len >= b.q_end ? r.frame_len - b.q_end : 0;
            uint32_t const len   = (b.q_start ? dec_digits(b.q_start) + 1 : 0) + oc + (right ? dec_digits(right) + 1 : 0);
            oc_len               = len ? len : 1;
        }
        c.aux[k] = BamAux{n_cigar, oc_len};
        size     = 36 + (uint64_t)r.qn_len + 1 + 4 * (uint64_t)n_cigar + (r.l_seq + 1) / 2 + r.l_seq + tag_bytes(c, r, oc_len);
        c.size[k] = (uint32_t)size;
    }
    // the tile's total: a wavefront lies in one tile (kBamTile is a multiple of 64)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        size += (uint64_t)__shfl_down((unsigned long long)size, off);
    if ((threadIdx.x & 63) == 0 && k < c.n)
        atomicAdd(&tile_total[k / kBamTile], (unsigned long long)size);
}

// one wavefront's cursor into its record: every lane keeps the same position, lane 0 writes the serial parts
struct Cursor
{
    uint8_t * p;
    int       lane;
    template <class T>
    __device__ __forceinline__ void le(T v, int bytes)
    {
        if (lane == 0)
            for (int i = 0; i < bytes; ++i)
                p[i] = (uint8_t)((uint64_t)v >> (8 * i));
        p += bytes;
    }
    __device__ __forceinline__ void tag(char a, char b, char type)
    {
        if (lane == 0)
        {
            p[0] = (uint8_t)a;
            p[1] = (uint8_t)b;
            p[2] = (uint8_t)type;
        }
        p += 3;
    }
};
__global__ __launch_bounds__(kBamEmitBlock) void bam_emit_kernel(BamCtx c, uint64_t first, uint64_t count, uint32_t const * off, uint8_t * out)
{
    uint64_t const j    = (uint64_t)blockIdx.x * kBamEmitRecs + (threadIdx.x >> 6);
    int const      lane = threadIdx.x & 63;
    if (j >= count)
        return;
    uint64_t const         k = first + j;
    Rec const              r = rec_of(c, k);
    lx_blast_match const & b = *r.b;
    BamAux const           a = c.aux[k];
    uint8_t const * const  o = c.ops + b.ops_off;
    uint8_t * const        rec = out + off[j];
    uint32_t const         size = c.size[k];
    Cursor                 w{rec, lane};

    // span of the reference the CIGAR covers: its M and D runs
    int64_t span = 0;
    if (a.n_cigar) // (a "*" has none)
    {
        uint64_t md = 0;
        for (uint32_t i = lane; i < b.n_ops; i += 64)
            md += o[i] != 'I' ? 1 : 0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
            md += (uint64_t)__shfl_xor((unsigned long long)md, s);
        span = (int64_t)(md * r.trans);
    }
    int64_t const pos0 = r.pos; // (its low 32 bits are stored)
    int const     flag = (r.first ? 0 : 256) | (r.minus ? 16 : 0);
    w.le<uint32_t>(size - 4, 4); // block_size
    w.le<int32_t>((int32_t)b.n_sid, 4);
    w.le<int32_t>((int32_t)pos0, 4);
    w.le<uint8_t>((uint8_t)(r.qn_len + 1), 1);
    w.le<uint8_t>(255, 1);
    w.le<uint16_t>((uint16_t)reg2bin(pos0, pos0 + (span > 0 ? span : 1)), 2);
    w.le<uint16_t>((uint16_t)a.n_cigar, 2);
    w.le<uint16_t>((uint16_t)flag, 2);
    w.le<int32_t>((int32_t)r.l_seq, 4);
    w.le<int32_t>(-1, 4);
    w.le<int32_t>(-1, 4);
    w.le<int32_t>(0, 4);
    // qname and its NUL
    for (uint32_t i = lane; i < r.qn_len; i += 64)
        w.p[i] = c.qn_blob[r.qn_at + i];
    if (lane == 0)
        w.p[r.qn_len] = 0;
    w.p += r.qn_len + 1;
    // CIGAR: cigarOf's elements, reversed on the minus strand
    if (a.n_cigar && lane == 0)
    {
        uint32_t e   = 0;
        auto     put = [&](uint32_t op, uint64_t len)
        {
            if (e < a.n_cigar)
            {
                uint32_t const  v = (uint32_t)len << 4 | op;
                uint8_t * const q = w.p + 4 * (uint64_t)(r.minus ? a.n_cigar - 1 - e : e);
                q[0]              = (uint8_t)v;
                q[1]              = (uint8_t)(v >> 8);
                q[2]              = (uint8_t)(v >> 16);
                q[3]              = (uint8_t)(v >> 24);
            }
            ++e;
        };
        walk_cigar(c, r, o, b.n_ops, put);
    }
    w.p += 4 * (uint64_t)a.n_cigar;
    // SEQ: two letters a byte, the odd last nibble 0; QUAL: the qualities - 33 over SEQ's letters, or absent (0xFF)
    uint64_t const seq_bytes = (r.l_seq + 1) / 2;
    for (uint64_t i = lane; i < seq_bytes; i += 64)
    {
        uint32_t v = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
        {
            uint64_t const x = 2 * i + h;
            uint32_t       code = 0;
            if (x < r.l_seq)
                code = nt16(seq_letter(c, r, x));
            v = v << 4 | code;
        }
        w.p[i] = (uint8_t)v;
    }
    w.p += seq_bytes;
    if (c.q_qual)
        for (uint64_t i = lane; i < r.l_seq; i += 64)
            w.p[i] = (uint8_t)(qual_letter(c, r, i) - 33);
    else
        for (uint64_t i = lane; i < r.l_seq; i += 64)
            w.p[i] = 0xff;
    w.p += r.l_seq;
    // the optional fields, in myWriteRecord's order
    uint32_t const t = c.tags;
    if (t & tagBit(kTagEValue))
    {
        w.tag('a', 'e', 'f');
        w.le<uint32_t>(__float_as_uint((float)b.e_value), 4);
    }
    if (t & tagBit(kTagBitScore))
    {
        w.tag('A', 'S', 'S');
        w.le<uint16_t>((uint16_t)(int32_t)b.bit_score, 2);
    }
    if (t & tagBit(kTagScore))
    {
        w.tag('a', 'r', 'C');
        w.le<uint8_t>((uint8_t)b.score, 1);
    }
    if (t & tagBit(kTagPIdent))
    {
        w.tag('a', 'i', 'C');
        w.le<uint8_t>((uint8_t)(int32_t)b.identity, 1);
    }
    if (t & tagBit(kTagPPos))
    {
        w.tag('a', 'p', 'S');
        w.le<uint16_t>(ppos_u16(b.num_positives, b.alignment_length), 2);
    }
    if (t & tagBit(kTagQFrame))
    {
        w.tag('q', 'f', 'c');
        w.le<uint8_t>((uint8_t)(int8_t)b.q_frame, 1);
    }
    if (t & tagBit(kTagSFrame))
    {
        w.tag('s', 'f', 'c');
        w.le<uint8_t>((uint8_t)(int8_t)b.s_frame, 1);
    }
    if (t & tagBit(kTagSTaxIds))
    {
        w.tag('s', 't', 'Z');
        uint64_t len = 0;
        for (uint64_t x = r.st_lo; x < r.st_hi; ++x)
        {
            uint32_t const id = c.s_tax_ids[x];
            uint32_t const d  = dec_digits(id);
            if (lane == 0)
            {
                if (x > r.st_lo)
                    w.p[len] = ';';
                put_dec(w.p + len + (x > r.st_lo ? 1 : 0), id, d);
            }
            len += d + (x > r.st_lo ? 1 : 0);
        }
        if (len == 0)
        {
            if (lane == 0)
                w.p[0] = '*';
            len = 1;
        }
        if (lane == 0)
            w.p[len] = 0;
        w.p += len + 1;
    }
    if (t & tagBit(kTagLcaId))
    {
        w.tag('l', 's', 'Z');
        uint32_t len = r.name_len;
        if (len == 0xffffffffu)
        {
            if (lane == 0)
                w.p[0] = '*';
            len = 1;
        }
        else
            for (uint32_t i = lane; i < len; i += 64)
                w.p[i] = c.name_blob[r.name_off + i];
        if (lane == 0)
            w.p[len] = 0;
        w.p += len + 1;
    }
    if (t & tagBit(kTagLcaTaxId))
    {
        w.tag('l', 't', 'I');
        w.le<uint32_t>(r.lca, 4);
    }
    if (t & tagBit(kTagProtSeq))
    {
        w.tag('q', 's', 'Z');
        uint64_t len = r.qs_len;
        if (len == 0)
        {
            if (lane == 0)
                w.p[0] = '*';
            len = 1;
        }
        else
            for (uint64_t i = lane; i < len; i += 64)
                w.p[i] = qs_letter(c, r, i);
        if (lane == 0)
            w.p[len] = 0;
        w.p += len + 1;
    }
    if (t & tagBit(kTagProtCigar))
    {
        w.tag('O', 'C', 'Z');
        if (lane == 0)
        {
            bool const need_oc = !c.is_n;
            uint32_t   at      = 0;
            auto       add     = [&](uint8_t op, uint64_t cnt)
            {
                uint32_t const d = dec_digits(cnt);
                if (at + d + 1 <= a.oc_len)
                {
                    put_dec(w.p + at, cnt, d);
                    w.p[at + d] = op;
                }
                at += d + 1;
            };
            // (one op byte that is no code makes the whole text "*": measure saw it and left oc_len 1)
            if (need_oc && ops_valid(o, b.n_ops))
                walk_oc(c, r, o, b.n_ops, add);
            if (at == 0)
                w.p[0] = '*';
            w.p[a.oc_len] = 0;
        }
        w.p += (uint64_t)a.oc_len + 1;
    }
    if (t & tagBit(kTagEditDistance))
    {
        w.tag('N', 'M', 'I');
        w.le<uint32_t>((uint32_t)(b.alignment_length - b.num_matches), 4);
    }
    if (t & tagBit(kTagMatchCount))
    {
        w.tag('I', 'H', 'I');
        w.le<uint32_t>(r.ih, 4);
    }
}

uint64_t scan_tiles(uint64_t n)
{
    return (n + kL2ScanTile - 1) / kL2ScanTile;
}

} // namespace

hipError_t bam_launch_groups(BamCtx const & c, uint32_t * block_tot, hipStream_t stream)
{
    if (c.n == 0)
        return hipSuccess;
    uint64_t const tiles = scan_tiles(c.n);
    dim3 const     grid((unsigned)tiles), block(kL2ScanBlock);
    HeadVal const  hv{c.rows};
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, HeadVal>), grid, block, 0, stream, hv, c.n, block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), block, 0, stream, block_tot, tiles);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, HeadVal, HeadOut>), grid, block, 0, stream, hv, HeadOut{c.rows, c.n, c.grp, c.grp_first}, c.n,
                       block_tot);
    return hipGetLastError();
}

hipError_t bam_launch_measure(BamCtx const & c, uint64_t * tile_total, hipStream_t stream)
{
    if (c.n == 0)
        return hipSuccess;
    hipError_t const e = hipMemsetAsync(tile_total, 0, scan_tiles(c.n) * sizeof(uint64_t), stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(bam_measure_kernel, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, stream, c, reinterpret_cast<unsigned long long *>(tile_total));
    return hipGetLastError();
}

hipError_t bam_launch_emit(BamCtx const & c, uint64_t first, uint64_t count, uint32_t * off, uint32_t * block_tot, uint8_t * out, hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    uint64_t const tiles = scan_tiles(count);
    dim3 const     grid((unsigned)tiles), block(kL2ScanBlock);
    SizeVal const  sv{c.size + first};
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, SizeVal>), grid, block, 0, stream, sv, count, block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), block, 0, stream, block_tot, tiles);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, SizeVal, OffOut>), grid, block, 0, stream, sv, OffOut{off}, count, block_tot);
    hipLaunchKernelGGL(bam_emit_kernel, dim3((unsigned)((count + kBamEmitRecs - 1) / kBamEmitRecs)), dim3(kBamEmitBlock), 0, stream, c, first, count,
                       off, out);
    return hipGetLastError();
}

} // namespace lx
