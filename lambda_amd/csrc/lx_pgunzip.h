// lx_pgunzip.h -- a plain gzip member's DEFLATE stream decoded in chunks that start in the middle of the stream (the scheme of pugz
// and rapidgzip), one statement for the host and the device: the kernels of lx_pgunzip.hip are launches around these functions,
// and tests/native/pgunzip_check.cpp runs the same functions chunk by chunk in a loop on the CPU.
//
//   find     the first bit at or after a chunk's nominal start where a non-final dynamic-Huffman block begins: precheck() throws
//            out nearly every bit offset from the header bits, the two counts, the Kraft sum of the code-length code and then the
//            Kraft sums of the two codes its lengths state; block_starts() is the authority -- Inflater's own dynamic_tables() and
//            codes() from that bit to the block's end-of-block without a status.  precheck() states necessary conditions of that
//            only, so a boundary it misses costs a merge of two chunks and never a byte.
//   decode   decode_chunk(): Inflater over a MarkerSink from bit b0 until a block ends at or beyond bit b1 or the final block ends.
//            The output is 16-bit symbols: 0..255 a byte, kMarker | w = byte w of the 32 KiB window in front of the chunk.
//   chain    chain(): chunk j is verified when chunk j - 1 is and ended on the very bit chunk j was found at.  chain_wave() is the
//            whole step as chain_kernel runs it: chain(), the verified chunks' places, and the WaveResult the host reads.
//   resolve  next_window_at() makes the window behind a chunk from the window in front of it and the chunk's last 32 Ki symbols;
//            resolve() turns a symbol into its byte.
// Bounds: the input reads are inside in[0, n) (Inflater and Bits check every one), the symbol writes inside the sink's room, the
// ring index is masked, a marker's window index is below kWindow by construction and checked against the window's valid part.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lx_crc32.h"
#include "lx_inflate.h"

namespace lx
{
namespace pgunzip
{

constexpr uint32_t kWindow = 32768;
constexpr uint16_t kMarker = 0x8000;
constexpr uint64_t kNone   = ~0ull; // no block start found in a chunk

// a chunk's status beyond lx::inflate::Status
enum : uint32_t
{
    kChunkSkipped    = 200, // nothing was found in this chunk: its bytes belong to the chunk before it
    kChunkNoBoundary = 201, // no boundary in the kMaxAbsorb chunks from this one on
};

// ---- find -----------------------------------------------------------------------------------------------------------------------

// a few bits at a time from any bit of in[0, n)
struct Bits
{
    uint8_t const * in;
    uint64_t        n, pos;
    uint64_t        acc = 0;
    uint32_t        cnt = 0;
    __host__ __device__ Bits(uint8_t const * in_, uint64_t n_, uint64_t bit) : in(in_), n(n_), pos(bit >> 3)
    {
        if (pos > n)
            pos = n;
        fill();
        uint32_t const skip = (uint32_t)(bit & 7);
        if (cnt >= skip)
        {
            acc >>= skip;
            cnt -= skip;
        }
    }
    __host__ __device__ void fill()
    {
        while (cnt <= 56 && pos < n)
        {
            acc |= (uint64_t)in[pos++] << cnt;
            cnt += 8;
        }
    }
    __host__ __device__ bool take(uint32_t k, uint32_t & v) // k <= 32
    {
        if (cnt < k)
        {
            fill();
            if (cnt < k)
                return false;
        }
        v = (uint32_t)(acc & ((1ull << k) - 1));
        acc >>= k;
        cnt -= k;
        return true;
    }
};

// what inflate::build(c, lens, n, true) accepts, from the counts per length alone
__host__ __device__ inline bool kraft_ok(uint16_t const * count, uint32_t n)
{
    int left = 1;
    for (uint32_t l = 1; l < 16; ++l)
    {
        left = (left << 1) - count[l];
        if (left < 0)
            return false;
    }
    return left == 0 || count[0] == n || (count[0] + 1u == n && count[1] == 1);
}

// necessary for a non-final dynamic block that Inflater::dynamic_tables() accepts to begin at `bit`: BFINAL 0, BTYPE 2, HLIT and
// HDIST in range, a complete code-length code, code lengths that decode (no repeat without a predecessor or past their number),
// an end-of-block code, and a literal / length and a distance code neither over-subscribed nor incomplete (zlib's exceptions kept)
__host__ __device__ inline bool precheck(uint8_t const * in, uint64_t n, uint64_t bit)
{
    Bits     r(in, n, bit);
    uint32_t v;
    if (!r.take(17, v) || (v & 7) != 4)
        return false;
    uint32_t const nlen = ((v >> 3) & 31) + 257, ndist = ((v >> 8) & 31) + 1, ncode = ((v >> 13) & 15) + 4;
    if (nlen > 286 || ndist > 30)
        return false;
    constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t           cl[19];
    for (uint32_t i = 0; i < 19; ++i)
        cl[i] = 0;
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < ncode; ++i)
    {
        uint32_t x;
        if (!r.take(3, x))
            return false;
        cl[order[i]] = (uint8_t)x;
        if (x)
            kraft += 128u >> x;
    }
    if (kraft != 128) // (complete: build(..., false) takes nothing else for the code-length code)
        return false;
    // the canonical code-length code, decoded bit by bit as Inflater::decode() does beyond its table
    uint8_t cnt[8], offs[8], syms[19];
    for (uint32_t l = 0; l < 8; ++l)
        cnt[l] = 0;
    for (uint32_t s = 0; s < 19; ++s)
        ++cnt[cl[s]];
    cnt[0]  = 0;
    offs[1] = 0;
    for (uint32_t l = 1; l < 7; ++l)
        offs[l + 1] = (uint8_t)(offs[l] + cnt[l]);
    for (uint32_t s = 0; s < 19; ++s)
        if (cl[s])
            syms[offs[cl[s]]++] = (uint8_t)s;
    uint16_t lc[16], dc[16];
    for (uint32_t l = 0; l < 16; ++l)
        lc[l] = dc[l] = 0;
    uint32_t const total = nlen + ndist;
    uint32_t       i = 0, prev = 0, eob = 0;
    while (i < total)
    {
        int32_t  code = 0, first = 0, index = 0;
        uint32_t sym = 19;
        for (uint32_t l = 1; l < 8; ++l)
        {
            uint32_t b;
            if (!r.take(1, b))
                return false;
            code |= (int32_t)b;
            int32_t const c = cnt[l];
            if (code - c < first)
            {
                sym = syms[index + (code - first)];
                break;
            }
            index += c;
            first += c;
            first <<= 1;
            code <<= 1;
        }
        if (sym >= 19)
            return false;
        uint32_t rep = 1, val = sym, x;
        if (sym == 16)
        {
            if (i == 0 || !r.take(2, x))
                return false;
            rep = 3 + x;
            val = prev;
        }
        else if (sym == 17)
        {
            if (!r.take(3, x))
                return false;
            rep = 3 + x;
            val = 0;
        }
        else if (sym == 18)
        {
            if (!r.take(7, x))
                return false;
            rep = 11 + x;
            val = 0;
        }
        if (i + rep > total)
            return false;
        for (; rep; --rep, ++i)
        {
            if (i < nlen)
            {
                ++lc[val];
                if (i == 256)
                    eob = val;
            }
            else
                ++dc[val];
        }
        prev = val;
    }
    return eob != 0 && kraft_ok(dc, ndist) && kraft_ok(lc, nlen);
}

// takes everything: the finder's test run of one block
struct NullSink
{
    __host__ __device__ bool put(uint8_t) { return true; }
    __host__ __device__ bool dist_ok(uint32_t) const { return true; }
    __host__ __device__ bool copy(uint32_t, uint32_t) { return true; }
};

// a non-final dynamic block begins at `bit` and decodes to its end-of-block without a status
template <class Index>
__host__ __device__ inline bool block_starts(uint8_t const * in, Index n, uint64_t bit, inflate::Tables & T)
{
    NullSink                           sink;
    inflate::Inflater<NullSink, Index> inf(in, n, sink, T);
    inf.seek_bit(bit);
    uint32_t last, type;
    if (!inf.take(1, last) || !inf.take(2, type) || last || type != 2)
        return false;
    return inf.dynamic_tables() == inflate::kOk && inf.codes() == inflate::kOk;
}

// the smallest bit in [lo, hi) at which a block starts, or kNone (one offset after the other: the kernel deals them to its lanes)
template <class Index>
__host__ __device__ inline uint64_t find_block(uint8_t const * in, Index n, uint64_t lo, uint64_t hi, inflate::Tables & T)
{
    for (uint64_t b = lo; b < hi; ++b)
        if (precheck(in, n, b) && block_starts<Index>(in, n, b, T))
            return b;
    return kNone;
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------

// a chunk's output as symbols: all of them to out[0, cap), the last kWindow of them also in a ring (the kernel's LDS) that the
// back-references read.  hist = bytes in front of the chunk that a distance may reach: kWindow, or 0 at the member's first bit
struct MarkerSink
{
    uint16_t * ring; // kWindow symbols
    uint16_t * out;
    uint32_t   pos, cap, hist;
    __host__ __device__ bool put(uint8_t b)
    {
        if (pos >= cap)
            return false;
        ring[pos & (kWindow - 1)] = b;
        out[pos++]                = b;
        return true;
    }
    __host__ __device__ bool dist_ok(uint32_t d) const { return d <= kWindow && (d <= pos || d - pos <= hist); }
    __host__ __device__ bool copy(uint32_t d, uint32_t len)
    {
        if (!dist_ok(d) || len > cap - pos)
            return false;
        for (uint32_t i = 0; i < len; ++i, ++pos) // (overlapping: symbol by symbol)
        {
            uint16_t const s          = d <= pos ? ring[(pos - d) & (kWindow - 1)] : (uint16_t)(kMarker | (kWindow + pos - d));
            ring[pos & (kWindow - 1)] = s;
            out[pos]                  = s;
        }
        return true;
    }
};

struct ChunkResult
{
    uint64_t end_bit; // the bit behind the last block decoded
    uint32_t count;   // symbols written
    uint32_t final;   // the last block was the stream's final one
    uint32_t status;  // 0, an lx::inflate::Status or kChunk*
    uint32_t pad;
};

// from bit b0 until a block ends at or beyond bit b1, or the final block ends
template <class Index>
__host__ __device__ inline ChunkResult decode_chunk(uint8_t const * in, Index n, uint64_t b0, uint64_t b1, MarkerSink & sink, inflate::Tables & T)
{
    inflate::Inflater<MarkerSink, Index> inf(in, n, sink, T);
    inf.seek_bit(b0);
    ChunkResult r{0, 0, 0, 0, 0};
    for (;;)
    {
        uint32_t last;
        if ((r.status = inf.block(last)))
            break;
        if (last)
        {
            r.final = 1;
            break;
        }
        if (inf.bit_pos() >= b1)
            break;
    }
    r.end_bit = inf.bit_pos();
    r.count   = sink.pos;
    return r;
}

// ---- the wave's rules (one statement for the kernel, the host and the CPU program) --------------------------------------------

constexpr uint32_t kRoomPerByte = 10; // symbols of room per compressed byte of a chunk
constexpr uint32_t kMaxAbsorb   = 4;  // chunks one decoder takes at most: its own and three behind it in which nothing was found

// what the decoder of slot j does: nothing (kChunkSkipped: nothing was found in its chunk), nothing but say so (kChunkNoBoundary: it
// would have to take more than kMaxAbsorb chunks -- stored or fixed-Huffman runs, blocks of hundreds of KB -- and one lane would
// decode for seconds), or decode [b0, b1) into (nx - j) slots of room
struct ChunkPlan
{
    uint32_t status; // 0: decode
    uint32_t cap;    // symbols of room
    uint64_t b0, b1;
};
__host__ __device__ inline ChunkPlan plan_chunk(uint64_t const * found, uint32_t nslots, uint32_t j, uint32_t room, uint64_t stop_bit)
{
    ChunkPlan p{kChunkSkipped, 0, 0, 0};
    if (found[j] == kNone)
        return p;
    uint32_t nx = j + 1;
    while (nx < nslots && found[nx] == kNone)
        ++nx;
    if (nx - j > kMaxAbsorb)
    {
        p.status = kChunkNoBoundary;
        return p;
    }
    p.status = 0;
    p.cap    = (nx - j) * room;
    p.b0     = found[j];
    p.b1     = nx < nslots ? found[nx] : stop_bit;
    return p;
}

// the chain check keeps breaking (block starts inside stored data): give the member to the host
__host__ __device__ inline bool chain_gives_up(uint64_t dropped, uint64_t verified) { return dropped > 4 * verified + 16; }

// ---- chain ----------------------------------------------------------------------------------------------------------------------

struct Chain
{
    uint32_t nver;    // verified chunks, their slots in ver[]; 0: the wave's first chunk failed
    uint32_t dropped; // found chunks the chain check threw out
    uint32_t final;   // the last verified chunk ended with the final block
    uint64_t end_bit; // where the last verified chunk ended: the next wave's start
};

// found[0] is a true boundary; every later chunk must begin on the bit where its verified predecessor ended
__host__ __device__ inline Chain chain(uint64_t const * found, ChunkResult const * r, uint32_t nslots, uint32_t * ver)
{
    Chain c{0, 0, 0, 0};
    if (nslots == 0 || r[0].status)
        return c;
    uint32_t cur = 0;
    ver[c.nver++] = 0;
    while (!r[cur].final)
    {
        uint32_t nx = cur + 1;
        while (nx < nslots && found[nx] == kNone)
            ++nx;
        if (nx >= nslots)
            break;
        if (r[cur].end_bit != found[nx] || r[nx].status)
        {
            for (uint32_t j = nx; j < nslots; ++j)
                c.dropped += found[j] != kNone;
            break;
        }
        ver[c.nver++] = cur = nx;
    }
    c.final   = r[cur].final;
    c.end_bit = r[cur].end_bit;
    return c;
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------

// a symbol's byte: win is the window in front of its chunk, of which the last `valid` bytes exist
__host__ __device__ inline uint8_t resolve(uint16_t sym, uint8_t const * win, uint32_t valid, bool & bad)
{
    if (!(sym & kMarker))
        return (uint8_t)sym;
    uint32_t const w = sym & (kWindow - 1);
    if (w < kWindow - valid)
    {
        bad = true; // a distance before the start of the member's output
        return 0;
    }
    return win[w];
}

// byte i of the window behind a chunk of `count` symbols
__host__ __device__ inline uint8_t next_window_at(uint32_t i, uint16_t const * syms, uint32_t count, uint8_t const * win, uint32_t valid, bool & bad)
{
    if (count >= kWindow)
        return resolve(syms[count - kWindow + i], win, valid, bad);
    return i + count < kWindow ? win[i + count] : resolve(syms[i + count - kWindow], win, valid, bad);
}

// x^(8 n) mod P for any n (a member may be longer than 2^32 bytes)
__host__ __device__ inline uint32_t x_pow_8n64(uint64_t n)
{
    uint32_t p = 1u << 31, t = 1u << 23;
    while (n)
    {
        if (n & 1)
            p = mul_mod_p(t, p);
        n >>= 1;
        if (n)
            t = mul_mod_p(t, t);
    }
    return p;
}

// ---- the launches (lx_pgunzip.hip) ----------------------------------------------------------------------------------------------

// one verified chunk of a wave for the resolve kernels
struct Verified
{
    uint64_t sym_off;  // its symbols in the wave's pool
    uint64_t byte_off; // its bytes in the wave's output
    uint32_t count;
    uint32_t valid;    // bytes of the window in front of it that exist
};

struct WaveParams
{
    uint8_t const * in;         // the wave's input: from the byte of its first bit on
    uint32_t        n;          // ... bytes of it
    uint32_t        chunk;      // compressed bytes per chunk: slot j's nominal start is byte j * chunk
    uint32_t        nslots;
    uint32_t        room;       // symbols of room per slot
    uint32_t        first_wave; // slot 0 begins at the member's first bit
    uint64_t        stop_bit;   // where the wave's last chunk may stop
    uint64_t *      found;      // [nslots]; found[0] is set by the host
    ChunkResult *   res;        // [nslots]
    uint16_t *      sym;        // [nslots * room]
};

constexpr uint32_t kMaxWaveSlots = 512; // slots of a wave at most (chain_kernel keeps their numbers in LDS)

// what a wave came to: written by the chain step, its crc and bad words completed by the resolve step; all the host reads of a
// wave besides its bytes
struct WaveResult
{
    uint64_t end_bit;  // where the last verified chunk ended: the next wave's start
    uint64_t wave_len; // bytes of the verified chunks
    uint32_t nver;     // verified chunks; 0: the wave's first chunk failed, with status0
    uint32_t dropped;  // found chunks the chain check threw out
    uint32_t final;    // the last verified chunk ended with the final block
    uint32_t status0;  // the first chunk's status (the decline reason when nver == 0)
    uint32_t crc;      // the wave's CRC register (no initial value, no final complement)
    uint32_t bad;      // 1: a marker before the start of the member's output, 2: a chunk outside the wave's bytes
    uint32_t longest;  // symbols of the longest verified chunk
    uint32_t pad;
};

// the chain step of a wave: chain(), then the verified chunks' places in the symbol pool and in the wave's bytes and the part of
// the window in front of each that exists (`before` = bytes of the member's text in front of the wave, kWindow at most).
// idx[nslots] is scratch; a count beyond the chunk's room (MarkerSink allows none) ends the chain in front of that chunk
__host__ __device__ inline void chain_wave(uint64_t const * found, ChunkResult const * r, uint32_t nslots, uint32_t room, uint32_t before,
                                           uint32_t * idx, Verified * ver, WaveResult & o)
{
    Chain const c = chain(found, r, nslots, idx);
    o             = WaveResult{c.end_bit, 0, c.nver, c.dropped, c.final, nslots ? r[0].status : (uint32_t)kChunkSkipped, 0, 0, 0, 0};
    for (uint32_t v = 0; v < c.nver; ++v)
    {
        uint32_t const j = idx[v], cnt = r[j].count;
        if (cnt > (uint64_t)(nslots - j) * room)
        {
            o.nver    = v;
            o.final   = 0;
            o.end_bit = v ? r[idx[v - 1]].end_bit : 0;
            o.bad |= 2;
            break;
        }
        uint64_t const seen = (uint64_t)before + o.wave_len;
        ver[v]              = Verified{(uint64_t)j * room, o.wave_len, cnt, (uint32_t)(seen < kWindow ? seen : kWindow)};
        o.wave_len += cnt;
        if (cnt > o.longest)
            o.longest = cnt;
    }
}

struct ChainParams
{
    uint64_t const *    found;  // [nslots]
    ChunkResult const * res;    // [nslots]
    uint32_t            nslots; // <= kMaxWaveSlots
    uint32_t            room;
    uint32_t            before; // bytes of the member's text in front of the wave, kWindow at most
    Verified *          ver;    // [nslots]
    WaveResult *        out;
};

struct ResolveParams
{
    uint16_t const *   sym;
    Verified const *   ver;     // [wr->nver], made by the chain step
    WaveResult *       wr;      // nver and wave_len are read on the device; crc ^= the wave's CRC register, bad |= 1 or 2
    uint32_t           nslots;  // the grid: workgroups beyond wr->nver exit
    uint32_t           max_seg; // 32 Ki-symbol segments of the longest chunk there can be
    uint8_t *          win;     // [(nslots + 1) * kWindow]: window v lies in front of verified chunk v
    uint8_t *          out;     // the wave's bytes
    uint64_t           out_cap; // ... the room for them
};

hipError_t launch_find(WaveParams const & p, hipStream_t stream);
hipError_t launch_decode(WaveParams const & p, hipStream_t stream);
hipError_t launch_chain(ChainParams const & p, hipStream_t stream);
hipError_t launch_resolve(ResolveParams const & p, hipStream_t stream);

} // namespace pgunzip
} // namespace lx
