// lx_bgzf.hip -- BGZF (blocked gzip, SAM/BAM specification section 4.1) encoder on the device (gfx950 only).
//
// The input is cut into blocks of at most kBgzfBlock = 65 280 bytes (htslib's cut: a stored block never exceeds 64 KiB).  One
// workgroup encodes one block into one gzip member in a slot of kBgzfSlot bytes:
//   1. the block goes to LDS; CRC32 by per-lane slices, combined by multiplication with x^(8k) mod P (lx_crc32.h) and an atomic
//      XOR -- the order of the lanes does not matter;
//   2. LZ77 with one candidate per position: positions are taken 256 at a time; each lane looks up the last earlier position
//      with the same 4-byte hash BEFORE the chunk's inserts, then inserts with atomicMax (the largest position wins whatever
//      the timing), then measures the match (up to 258 bytes, distance up to 32 768);
//   3. a greedy parse (one lane: take the match where there is one);
//   4. symbol histograms (LDS atomics), then length-limited Huffman codes, the code-length code (symbols 16, 17, 18) and the
//      block header in one lane;
//   5. bit offsets per lane by a prefix sum over the lanes' ranges of symbols, then bit packing (words a lane owns alone are
//      stored, the shared first and last words of a range are ORed);
//   6. a stored block (BTYPE 0) instead when the dynamic one would not be smaller.
// A second kernel places the members one after another (each block sums the sizes in front of it).  Every step is
// deterministic: the same input gives the same bytes on every run, handle and stream.
#include <hip/hip_runtime.h>

#include "lx_bgzf.h"
#include "lx_crc32.h"

namespace lx
{
namespace bgzf
{

constexpr uint32_t kThreads  = 256;
constexpr uint32_t kHashBits = 13;
constexpr uint32_t kDataLds  = 65536;                  // the block (65 280 bytes used)
constexpr uint32_t kLenLds   = kBgzfBlock;             // match length - 3 per position, 0 = none
constexpr uint32_t kAuxLds   = 4u << kHashBits;        // the hash heads; after the matching the code tables
constexpr uint32_t kLdsBytes = kDataLds + kLenLds + kAuxLds;

static_assert(kLdsBytes <= 160 * 1024 - 256, "the encoder's LDS exceeds what gfx950 gives a workgroup");
static_assert((kDataLds + kLenLds) % 16 == 0, "the hash heads must be aligned");

// ---- DEFLATE symbols (RFC 1951 3.2.5)
__device__ __forceinline__ void length_symbol(uint32_t len, uint32_t & sym, uint32_t & nextra, uint32_t & extra)
{
    uint32_t const x = len - 3;
    if (x < 8)
    {
        sym = 257 + x, nextra = 0, extra = 0;
        return;
    }
    if (x == 255)
    {
        sym = 285, nextra = 0, extra = 0;
        return;
    }
    uint32_t const nb = 31 - __clz(x), hi = (x >> (nb - 2)) & 3;
    sym    = 257 + 4 * (nb - 1) + hi;
    nextra = nb - 2;
    extra  = x - ((4 | hi) << (nb - 2));
}

__device__ __forceinline__ void dist_symbol(uint32_t d, uint32_t & sym, uint32_t & nextra, uint32_t & extra)
{
    uint32_t const x = d - 1;
    if (x < 4)
    {
        sym = x, nextra = 0, extra = 0;
        return;
    }
    uint32_t const nb = 31 - __clz(x), hi = (x >> (nb - 1)) & 1;
    sym    = 2 * nb + hi;
    nextra = nb - 1;
    extra  = x - ((2 | hi) << (nb - 1));
}

__device__ __forceinline__ uint32_t reverse_bits(uint32_t code, uint32_t len)
{
    return __brev(code) >> (32 - len);
}

// Code lengths of a length-limited Huffman code over freq[0, n) (one lane).  Fewer than two used symbols get company (symbols 0
// and 1), as zlib does, so that every code is complete.  Moffat & Katajainen's in-place construction over the used symbols sorted
// by (frequency, symbol), then the lengths beyond `limit` folded in by the Kraft-sum repair of miniz; the longest lengths go to the
// rarest symbols.  work: 2 n words, idx: n entries.
__device__ void huffman_lengths(uint32_t * freq, uint32_t n, uint32_t limit, uint8_t * len, uint32_t * work, uint16_t * idx)
{
    uint32_t used = 0;
    for (uint32_t s = 0; s < n; ++s)
        used += freq[s] != 0;
    for (uint32_t s = 0; used < 2 && s < n; ++s)
        if (freq[s] == 0)
        {
            freq[s] = 1;
            ++used;
        }
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s)
    {
        len[s] = 0;
        if (freq[s] == 0)
            continue;
        // insertion by (frequency, symbol)
        uint32_t j = m++;
        while (j > 0 && freq[idx[j - 1]] > freq[s])
        {
            idx[j] = idx[j - 1];
            --j;
        }
        idx[j] = (uint16_t)s;
    }
    uint32_t * A = work;
    for (uint32_t i = 0; i < m; ++i)
        A[i] = freq[idx[i]];
    // calculate_minimum_redundancy (Moffat & Katajainen 1995)
    {
        int root = 0, leaf = 2, next;
        A[0] += A[1];
        for (next = 1; next < (int)m - 1; ++next)
        {
            if (leaf >= (int)m || A[root] < A[leaf])
            {
                A[next]   = A[root];
                A[root++] = (uint32_t)next;
            }
            else
                A[next] = A[leaf++];
            if (leaf >= (int)m || (root < next && A[root] < A[leaf]))
            {
                A[next] += A[root];
                A[root++] = (uint32_t)next;
            }
            else
                A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (next = (int)m - 3; next >= 0; --next)
            A[next] = A[A[next]] + 1;
        int avbl = 1, usedn = 0, dpth = 0;
        root = (int)m - 2;
        next = (int)m - 1;
        while (avbl > 0)
        {
            while (root >= 0 && (int)A[root] == dpth)
            {
                ++usedn;
                --root;
            }
            while (avbl > usedn)
            {
                A[next--] = (uint32_t)dpth;
                --avbl;
            }
            avbl  = 2 * usedn;
            ++dpth;
            usedn = 0;
        }
    }
    // A[i] is the length of the i-th rarest symbol (non-increasing); count, limit, hand out again
    uint32_t * cnt = work + n; // [0, 33)
    for (uint32_t l = 0; l <= 32; ++l)
        cnt[l] = 0;
    for (uint32_t i = 0; i < m; ++i)
        ++cnt[min(A[i], 32u)];
    for (uint32_t l = limit + 1; l <= 32; ++l)
    {
        cnt[limit] += cnt[l];
        cnt[l] = 0;
    }
    uint32_t total = 0;
    for (uint32_t l = 1; l <= limit; ++l)
        total += cnt[l] << (limit - l);
    while (total != (1u << limit))
    {
        --cnt[limit];
        for (uint32_t l = limit - 1; l > 0; --l)
            if (cnt[l])
            {
                --cnt[l];
                cnt[l + 1] += 2;
                break;
            }
        --total;
    }
    uint32_t i = 0;
    for (uint32_t l = limit; l > 0; --l)
        for (uint32_t k = 0; k < cnt[l]; ++k)
            len[idx[i++]] = (uint8_t)l;
}

// canonical codes, bit-reversed for LSB-first output
__device__ void huffman_codes(uint8_t const * len, uint32_t n, uint16_t * code)
{
    uint32_t cnt[16] = {}, next[16];
    for (uint32_t s = 0; s < n; ++s)
        ++cnt[len[s]];
    cnt[0]       = 0;
    uint32_t c   = 0;
    for (uint32_t l = 1; l < 16; ++l)
    {
        c       = (c + cnt[l - 1]) << 1;
        next[l] = c;
    }
    for (uint32_t s = 0; s < n; ++s)
        code[s] = len[s] ? (uint16_t)reverse_bits(next[len[s]]++, len[s]) : 0;
}

// ORs `nb` (<= 32) bits of v at bit position `at` of a zeroed word buffer (the lanes' shared words)
__device__ __forceinline__ void or_bits(uint32_t * words, uint32_t at, uint32_t v, uint32_t nb)
{
    if (nb == 0)
        return;
    uint64_t const x = (uint64_t)v << (at & 31);
    atomicOr(words + (at >> 5), (uint32_t)x);
    if ((at & 31) + nb > 32)
        atomicOr(words + (at >> 5) + 1, (uint32_t)(x >> 32));
}

// a lane's run of bits: words it alone covers are stored, its first and last (shared) words ORed
struct BitRun
{
    uint32_t * words;
    uint64_t   acc;
    uint32_t   nacc, widx;
    bool       first;
    __device__ BitRun(uint32_t * w, uint32_t at) : words(w), acc(0), nacc(at & 31), widx(at >> 5), first(true) {}
    __device__ __forceinline__ void put(uint32_t v, uint32_t nb)
    {
        acc |= (uint64_t)v << nacc;
        nacc += nb;
        if (nacc >= 32)
        {
            if (first)
                atomicOr(words + widx, (uint32_t)acc);
            else
                words[widx] = (uint32_t)acc;
            first = false;
            ++widx;
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ void finish()
    {
        if (nacc > 0)
            atomicOr(words + widx, (uint32_t)acc);
    }
};

// the code tables of a block, in the LDS of the hash heads once the matching is done
struct Tables
{
    uint32_t freq_ll[286], freq_d[30], freq_cl[19];
    uint32_t lane_bits[kThreads];
    uint32_t work[2 * 286 + 40];
    uint16_t code_ll[286], code_d[30], code_cl[19];
    uint16_t rle[286 + 30];
    uint16_t idx[286];
    uint8_t  len_ll[286], len_d[30], len_cl[19];
};
static_assert(sizeof(Tables) <= kAuxLds, "the code tables must fit where the hash heads were");

__device__ __forceinline__ uint32_t rle_extra_bits(uint32_t sym)
{
    return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
}

// run-length form of a list of code lengths (RFC 1951 3.2.7), appended to rle (sym | extra << 5)
__device__ uint32_t rle_lengths(uint8_t const * len, uint32_t n, uint16_t * rle, uint32_t k)
{
    for (uint32_t i = 0; i < n;)
    {
        uint32_t const cur = len[i];
        uint32_t       run = 1;
        while (i + run < n && len[i + run] == cur)
            ++run;
        i += run;
        if (cur == 0)
        {
            while (run >= 11)
            {
                uint32_t const r = min(run, 138u);
                rle[k++]         = (uint16_t)(18 | (r - 11) << 5);
                run -= r;
            }
            if (run >= 3)
            {
                rle[k++] = (uint16_t)(17 | (run - 3) << 5);
                run      = 0;
            }
            while (run--)
                rle[k++] = 0;
        }
        else
        {
            rle[k++] = (uint16_t)cur;
            --run;
            while (run >= 3)
            {
                uint32_t const r = min(run, 6u);
                rle[k++]         = (uint16_t)(16 | (r - 3) << 5);
                run -= r;
            }
            while (run--)
                rle[k++] = (uint16_t)cur;
        }
    }
    return k;
}

__global__ __launch_bounds__(kThreads) void block_kernel(BgzfParams p)
{
    extern __shared__ __align__(16) uint8_t lds[];
    uint8_t * const  data = lds;
    uint8_t * const  mlen = lds + kDataLds;
    uint32_t * const head = reinterpret_cast<uint32_t *>(lds + kDataLds + kLenLds);
    Tables &         T    = *reinterpret_cast<Tables *>(head);
    __shared__ uint32_t s_crc, s_nsym, s_hdr_bits, s_dynamic, s_dbytes;

    uint32_t const tid = threadIdx.x, b = blockIdx.x;
    uint64_t const off = (uint64_t)b * kBgzfBlock;
    uint32_t const n   = (uint32_t)min((uint64_t)kBgzfBlock, p.n - off);
    uint8_t * const  out   = p.slots + (uint64_t)b * kBgzfSlot;
    uint32_t * const words = reinterpret_cast<uint32_t *>(out);
    uint16_t * const dist  = p.dist + (uint64_t)b * kBgzfBlock;
    uint16_t * const sym   = p.sym + (uint64_t)b * kBgzfBlock;

    // ---- 1. the block into LDS (the block's start is 16-byte aligned in the chunk), a zeroed slot, the CRC table
    {
        uint8_t const * src = p.in + off;
        uint32_t const  n16 = n / 16;
        for (uint32_t i = tid; i < n16; i += kThreads)
            reinterpret_cast<uint4 *>(data)[i] = reinterpret_cast<uint4 const *>(src)[i];
        for (uint32_t i = n16 * 16 + tid; i < n; i += kThreads)
            data[i] = src[i];
        for (uint32_t i = tid; i < kBgzfSlot / 16; i += kThreads)
            reinterpret_cast<uint4 *>(out)[i] = uint4{0, 0, 0, 0};
        uint32_t c = tid;
        for (int k = 0; k < 8; ++k)
            c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        head[tid] = c; // (the byte table, where the hash heads go next)
        if (tid == 0)
            s_crc = 0;
    }
    __syncthreads();
    {
        uint32_t const L = (n + kThreads - 1) / kThreads, a = min(n, tid * L), e = min(n, a + L);
        uint32_t       r = 0;
        for (uint32_t i = a; i < e; ++i)
            r = (r >> 8) ^ head[(r ^ data[i]) & 0xff];
        uint32_t part = e > a ? mul_mod_p(x_pow_8n(n - e), r) : 0u;
        if (tid == 0)
            part ^= mul_mod_p(x_pow_8n(n), 0xffffffffu); // the initial register, carried over the whole block
        atomicXor(&s_crc, part);
    }
    __syncthreads();
    for (uint32_t i = tid; i < (1u << kHashBits); i += kThreads)
        head[i] = 0; // position + 1 of the last insert, 0 = none
    __syncthreads();

    // ---- 2. matches, 256 positions at a time
    for (uint32_t c0 = 0; c0 < n; c0 += kThreads)
    {
        uint32_t const pos = c0 + tid;
        bool const     has = pos + 4 <= n;
        uint32_t       h = 0, cand = 0;
        if (has)
        {
            uint32_t const w = (uint32_t)data[pos] | (uint32_t)data[pos + 1] << 8 | (uint32_t)data[pos + 2] << 16 | (uint32_t)data[pos + 3] << 24;
            h    = (w * 2654435761u) >> (32 - kHashBits);
            cand = head[h];
        }
        __syncthreads();
        if (has)
            atomicMax(&head[h], pos + 1);
        if (pos < n)
        {
            uint32_t len = 0, d = 0;
            if (cand)
            {
                uint32_t const q = cand - 1;
                d                = pos - q;
                if (d <= 32768)
                {
                    uint32_t const lim = min(258u, n - pos);
                    while (len < lim && data[q + len] == data[pos + len])
                        ++len;
                }
            }
            mlen[pos] = len >= 4 ? (uint8_t)(len - 3) : 0;
            if (len >= 4)
                dist[pos] = (uint16_t)d;
        }
        __syncthreads();
    }

    // ---- 3. greedy parse
    if (tid == 0)
    {
        uint32_t k = 0;
        for (uint32_t pos = 0; pos < n;)
        {
            sym[k++]         = (uint16_t)pos;
            uint32_t const m = mlen[pos];
            pos += m ? m + 3 : 1;
        }
        s_nsym = k;
    }
    __syncthreads();
    uint32_t const nsym = s_nsym;

    // ---- 4. histograms, codes, header
    for (uint32_t i = tid; i < 286 + 30 + 19; i += kThreads)
        (i < 286 ? T.freq_ll[i] : i < 316 ? T.freq_d[i - 286] : T.freq_cl[i - 316]) = 0;
    __syncthreads();
    for (uint32_t i = tid; i < nsym; i += kThreads)
    {
        uint32_t const pos = sym[i], m = mlen[pos];
        if (m)
        {
            uint32_t s, ne, ev;
            length_symbol(m + 3, s, ne, ev);
            atomicAdd(&T.freq_ll[s], 1u);
            dist_symbol(dist[pos], s, ne, ev);
            atomicAdd(&T.freq_d[s], 1u);
        }
        else
            atomicAdd(&T.freq_ll[data[pos]], 1u);
    }
    __syncthreads();
    if (tid == 0)
    {
        T.freq_ll[256] = 1;
        huffman_lengths(T.freq_ll, 286, 15, T.len_ll, T.work, T.idx);
        huffman_lengths(T.freq_d, 30, 15, T.len_d, T.work, T.idx);
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257 && T.len_ll[hlit - 1] == 0)
            --hlit;
        while (hdist > 1 && T.len_d[hdist - 1] == 0)
            --hdist;
        uint32_t nrle = rle_lengths(T.len_ll, hlit, T.rle, 0);
        nrle          = rle_lengths(T.len_d, hdist, T.rle, nrle);
        for (uint32_t i = 0; i < nrle; ++i)
            ++T.freq_cl[T.rle[i] & 31];
        huffman_lengths(T.freq_cl, 19, 7, T.len_cl, T.work, T.idx);
        huffman_codes(T.len_ll, 286, T.code_ll);
        huffman_codes(T.len_d, 30, T.code_d);
        huffman_codes(T.len_cl, 19, T.code_cl);
        uint8_t const order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        uint32_t      hclen     = 19;
        while (hclen > 4 && T.len_cl[order[hclen - 1]] == 0)
            --hclen;
        // the size of the dynamic block (the freq arrays were made complete above: every used symbol counts)
        uint64_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (uint32_t i = 0; i < nrle; ++i)
            bits += T.len_cl[T.rle[i] & 31] + rle_extra_bits(T.rle[i] & 31);
        for (uint32_t s = 0; s < 286; ++s)
            bits += (uint64_t)T.freq_ll[s] * (T.len_ll[s] + (s >= 265 && s < 285 ? (s - 261) / 4 : 0));
        for (uint32_t s = 0; s < 30; ++s)
            bits += (uint64_t)T.freq_d[s] * (T.len_d[s] + (s >= 4 ? s / 2 - 1 : 0));
        // (the frequencies of padded symbols -- fewer than two used -- add a few bits that are not sent: an over-estimate only)
        bool const dynamic = (bits + 7) / 8 < (uint64_t)n + 5;
        s_dynamic          = dynamic;
        if (dynamic)
        {
            uint32_t at = 18 * 8;
            or_bits(words, at, 1 | 2 << 1, 3); // BFINAL, BTYPE 2
            at += 3;
            or_bits(words, at, hlit - 257, 5);
            at += 5;
            or_bits(words, at, hdist - 1, 5);
            at += 5;
            or_bits(words, at, hclen - 4, 4);
            at += 4;
            for (uint32_t i = 0; i < hclen; ++i, at += 3)
                or_bits(words, at, T.len_cl[order[i]], 3);
            for (uint32_t i = 0; i < nrle; ++i)
            {
                uint32_t const s = T.rle[i] & 31, ne = rle_extra_bits(s);
                or_bits(words, at, T.code_cl[s], T.len_cl[s]);
                at += T.len_cl[s];
                or_bits(words, at, T.rle[i] >> 5, ne);
                at += ne;
            }
            s_hdr_bits = at;
        }
    }
    __syncthreads();

    // ---- 5. bit packing: lane t takes the symbols [t S, (t + 1) S)
    if (s_dynamic)
    {
        uint32_t const S = (nsym + kThreads - 1) / kThreads, s0 = min(nsym, tid * S), s1 = min(nsym, s0 + S);
        uint32_t       mine = 0;
        for (uint32_t i = s0; i < s1; ++i)
        {
            uint32_t const pos = sym[i], m = mlen[pos];
            if (m)
            {
                uint32_t s, ne, ev;
                length_symbol(m + 3, s, ne, ev);
                mine += T.len_ll[s] + ne;
                dist_symbol(dist[pos], s, ne, ev);
                mine += T.len_d[s] + ne;
            }
            else
                mine += T.len_ll[data[pos]];
        }
        T.lane_bits[tid] = mine;
        __syncthreads();
        if (tid == 0)
        {
            uint32_t run = s_hdr_bits;
            for (uint32_t t = 0; t < kThreads; ++t)
            {
                uint32_t const x = T.lane_bits[t];
                T.lane_bits[t]   = run;
                run += x;
            }
            or_bits(words, run, T.code_ll[256], T.len_ll[256]); // end of block
            run += T.len_ll[256];
            s_dbytes = (run + 7) / 8 - 18;
        }
        __syncthreads();
        BitRun w(words, T.lane_bits[tid]);
        for (uint32_t i = s0; i < s1; ++i)
        {
            uint32_t const pos = sym[i], m = mlen[pos];
            if (m)
            {
                uint32_t s, ne, ev;
                length_symbol(m + 3, s, ne, ev);
                w.put(T.code_ll[s], T.len_ll[s]);
                if (ne)
                    w.put(ev, ne);
                dist_symbol(dist[pos], s, ne, ev);
                w.put(T.code_d[s], T.len_d[s]);
                if (ne)
                    w.put(ev, ne);
            }
            else
            {
                uint32_t const c = data[pos];
                w.put(T.code_ll[c], T.len_ll[c]);
            }
        }
        w.finish();
    }
    else
    {
        for (uint32_t i = tid; i < n; i += kThreads)
            out[23 + i] = data[i];
        if (tid == 0)
        {
            out[18]  = 1; // BFINAL, BTYPE 0
            out[19]  = (uint8_t)n;
            out[20]  = (uint8_t)(n >> 8);
            out[21]  = (uint8_t)~n;
            out[22]  = (uint8_t)(~n >> 8);
            s_dbytes = 5 + n;
        }
    }
    __syncthreads();

    // ---- 6. gzip header with the BC subfield, trailer
    if (tid == 0)
    {
        uint32_t const size = 18 + s_dbytes + 8, crc = s_crc ^ 0xffffffffu;
        uint8_t const  hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (int i = 0; i < 16; ++i)
            out[i] = hdr[i];
        out[16]               = (uint8_t)(size - 1);
        out[17]               = (uint8_t)((size - 1) >> 8);
        uint8_t * const t     = out + 18 + s_dbytes;
        for (int i = 0; i < 4; ++i)
        {
            t[i]     = (uint8_t)(crc >> (8 * i));
            t[4 + i] = (uint8_t)(n >> (8 * i));
        }
        p.sizes[b] = size;
    }
}

// the members one after another: block b sums the sizes in front of it, then copies its member
__global__ __launch_bounds__(kThreads) void gather_kernel(BgzfParams p)
{
    __shared__ uint32_t part[kThreads];
    uint32_t const      tid = threadIdx.x, b = blockIdx.x;
    uint32_t            s   = 0;
    for (uint32_t j = tid; j < b; j += kThreads)
        s += p.sizes[j];
    part[tid] = s;
    __syncthreads();
    for (uint32_t w = kThreads / 2; w > 0; w >>= 1)
    {
        if (tid < w)
            part[tid] += part[tid + w];
        __syncthreads();
    }
    uint64_t const       at   = part[0];
    uint32_t const       size = p.sizes[b];
    uint8_t const *      src  = p.slots + (uint64_t)b * kBgzfSlot;
    uint8_t *            dst  = p.out + at;
    for (uint32_t i = tid; i < size; i += kThreads)
        dst[i] = src[i];
    if (b == p.nblk - 1 && tid == 0)
        *p.total = at + size;
}

} // namespace bgzf

hipError_t launch_bgzf(BgzfParams const & p, hipStream_t stream)
{
    if (p.nblk == 0 || p.n > (uint64_t)p.nblk * kBgzfBlock || p.n <= (uint64_t)(p.nblk - 1) * kBgzfBlock)
        return hipErrorInvalidValue;
    // (beyond 64 KB of LDS on request; set on the current device)
    hipError_t const attr = hipFuncSetAttribute(reinterpret_cast<void const *>(&bgzf::block_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bgzf::kLdsBytes);
    if (attr != hipSuccess)
        return attr;
    hipLaunchKernelGGL(bgzf::block_kernel, dim3(p.nblk), dim3(bgzf::kThreads), bgzf::kLdsBytes, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(bgzf::gather_kernel, dim3(p.nblk), dim3(bgzf::kThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace lx
