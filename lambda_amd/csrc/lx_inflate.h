// lx_inflate.h -- DEFLATE (RFC 1951) decoding, one statement for the host and the device: the BGZF kernel (lx_gunzip.hip) runs it
// on one lane per member, the host decoder (lx_gunzip_host.cpp) on the calling thread for every other member.
//
// Every read stays inside in[0, n) and every write goes through the Sink, which owns the bounds of the output: whatever the bits
// say, a malformed stream ends in a status, never in an access outside those ranges.  Bad input this catches: a reserved block
// type, a stored length whose complement does not match, an over-subscribed or incomplete code (a distance or literal / length
// code of a single 1-bit code, and an empty distance code, excepted as in zlib), a code that is not in its table, a length or
// distance symbol beyond 285 / 29, a repeat of the code lengths with nothing before it or past their number, a distance before
// the start of the output, output past the sink's capacity, a stream that ends before its final block.
//
// Sink: __host__ __device__ members
//   bool put(uint8_t b)                     -- false: no room
//   bool copy(uint32_t dist, uint32_t len)  -- the back-reference; false: dist beyond the output or no room
//   bool dist_ok(uint32_t dist)             -- dist reaches no further back than the start of the output
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lx
{
namespace inflate
{

enum Status : uint32_t
{
    kOk = 0,
    kTruncated,     // the stream ends before its final block
    kBadBlockType,  // BTYPE 3
    kBadStored,     // LEN != ~NLEN
    kBadLengths,    // the code-length repeat codes, HLIT / HDIST beyond 286 / 30
    kBadCode,       // an over-subscribed or incomplete code, or bits that are no code of the table
    kBadSymbol,     // length symbol 286 / 287, distance symbol 30 / 31
    kDistTooFar,    // a distance before the start of the output
    kOutputFull,    // more output than the sink takes
    kStatusCount
};

__host__ __device__ inline char const * status_text(uint32_t s)
{
    switch (s)
    {
    case kOk: return "ok";
    case kTruncated: return "truncated DEFLATE stream";
    case kBadBlockType: return "reserved block type";
    case kBadStored: return "stored block length does not match its complement";
    case kBadLengths: return "invalid code lengths";
    case kBadCode: return "invalid Huffman code";
    case kBadSymbol: return "invalid length or distance symbol";
    case kDistTooFar: return "distance before the start of the output";
    case kOutputFull: return "more output than the member's ISIZE";
    default: return "?";
    }
}

constexpr uint32_t kFastBits = 10;

// a canonical Huffman code: counts per length, symbols in code order, and a table of the codes up to kFastBits long indexed by the
// next kFastBits input bits (entry = symbol | length << 9; 0 = a longer code, decoded from count / sym)
struct Code
{
    uint16_t count[16];
    uint16_t sym[288];
    uint16_t fast[1u << kFastBits];
};

// the code tables of one member (about 5.8 KB)
struct Tables
{
    Code    lit, dist;
    uint8_t lens[288 + 32];
};

// builds c from lens[0, n); false for an over-subscribed code, or an incomplete one -- unless `incomplete_ok` and the code has no
// symbol or a single one of length 1.  That is zlib's rule for the literal / length and the distance code (never for the
// code-length code): dynamic_tables() passes true for both, and has refused a literal / length code without end-of-block before.
// The bits that would select the missing half of such a code are in no table and decode() refuses them.
__host__ __device__ inline bool build(Code & c, uint8_t const * lens, uint32_t n, bool incomplete_ok)
{
    for (uint32_t l = 0; l < 16; ++l)
        c.count[l] = 0;
    for (uint32_t s = 0; s < n; ++s)
        ++c.count[lens[s]];
    uint16_t offs[16];
    int      left = 1;
    for (uint32_t l = 1; l < 16; ++l)
    {
        left = (left << 1) - c.count[l];
        if (left < 0)
            return false;
    }
    if (left > 0 && !(incomplete_ok && (c.count[0] == n || (c.count[0] + 1u == n && c.count[1] == 1))))
        return false;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l)
        offs[l + 1] = offs[l] + c.count[l];
    for (uint32_t s = 0; s < n; ++s)
        if (lens[s])
            c.sym[offs[lens[s]]++] = (uint16_t)s;
    for (uint32_t i = 0; i < (1u << kFastBits); ++i)
        c.fast[i] = 0;
    // canonical codes in order; each short code fills every entry whose low bits are its bit-reversed code
    uint32_t code = 0, k = 0;
    for (uint32_t l = 1; l <= kFastBits; ++l)
    {
        for (uint32_t j = 0; j < c.count[l]; ++j, ++k, ++code)
        {
            uint32_t rev = 0;
            for (uint32_t b = 0; b < l; ++b)
                rev |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t e = rev; e < (1u << kFastBits); e += 1u << l)
                c.fast[e] = (uint16_t)(c.sym[k] | l << 9);
        }
        code <<= 1;
    }
    return true;
}

// the decoder of one stream (Index: wide enough for the input's bytes -- 32 bits for a BGZF member, 64 for a plain one)
template <class Sink, class Index = uint32_t>
struct Inflater
{
    uint8_t const * in;
    Index           n; // input bytes
    Index           pos = 0;
    uint64_t        bits = 0;
    uint32_t        nbits = 0;
    Sink &          out;
    Tables &        T;

    __host__ __device__ Inflater(uint8_t const * in_, Index n_, Sink & out_, Tables & t_) : in(in_), n(n_), out(out_), T(t_) {}

    __host__ __device__ void refill()
    {
        if (n - pos >= 8) // whole bytes up to 56 bits, from eight independent loads (one latency, not one per byte)
        {
            uint64_t w = 0;
            for (uint32_t i = 0; i < 8; ++i)
                w |= (uint64_t)in[pos + i] << (8 * i);
            uint32_t const k = (63 - nbits) >> 3;
            bits |= (w & ((1ull << (8 * k)) - 1)) << nbits;
            pos += k;
            nbits += 8 * k;
            return;
        }
        while (nbits <= 56 && pos < n)
        {
            bits |= (uint64_t)in[pos++] << nbits;
            nbits += 8;
        }
    }
    // the next k (<= 32) bits; false when the input ends first
    __host__ __device__ bool take(uint32_t k, uint32_t & v)
    {
        if (nbits < k)
        {
            refill();
            if (nbits < k)
                return false;
        }
        v = (uint32_t)(bits & ((1ull << k) - 1));
        bits >>= k;
        nbits -= k;
        return true;
    }
    // one symbol of c; status on failure
    __host__ __device__ uint32_t decode(Code const & c, uint32_t & sym)
    {
        if (nbits < 15)
            refill();
        uint32_t const e = c.fast[bits & ((1u << kFastBits) - 1)];
        if (e)
        {
            uint32_t const l = e >> 9;
            if (l > nbits)
                return kTruncated;
            sym = e & 511;
            bits >>= l;
            nbits -= l;
            return kOk;
        }
        // longer than kFastBits (or no code at all): canonical decoding bit by bit
        int32_t code = 0, first = 0, index = 0;
        for (uint32_t l = 1; l < 16; ++l)
        {
            if (l > nbits)
                return kTruncated;
            code |= (int32_t)((bits >> (l - 1)) & 1);
            int32_t const cnt = c.count[l];
            if (code - cnt < first)
            {
                sym = c.sym[index + (code - first)];
                bits >>= l;
                nbits -= l;
                return kOk;
            }
            index += cnt;
            first += cnt;
            first <<= 1;
            code <<= 1;
        }
        return kBadCode;
    }

    __host__ __device__ uint32_t stored()
    {
        bits >>= nbits & 7; // to the byte boundary
        nbits -= nbits & 7;
        uint32_t len, nlen;
        if (!take(16, len) || !take(16, nlen))
            return kTruncated;
        if (len != (~nlen & 0xffffu))
            return kBadStored;
        for (; len && nbits; --len) // bytes still in the bit buffer first
        {
            uint32_t b;
            take(8, b);
            if (!out.put((uint8_t)b))
                return kOutputFull;
        }
        if (len > n - pos)
            return kTruncated;
        for (; len; --len)
            if (!out.put(in[pos++]))
                return kOutputFull;
        return kOk;
    }

    __host__ __device__ uint32_t codes()
    {
        for (;;)
        {
            uint32_t sym, rc;
            if ((rc = decode(T.lit, sym)))
                return rc;
            if (sym < 256)
            {
                if (!out.put((uint8_t)sym))
                    return kOutputFull;
                continue;
            }
            if (sym == 256)
                return kOk;
            sym -= 257;
            if (sym >= 29)
                return kBadSymbol;
            // RFC 1951 3.2.5: base lengths 3..10 without extra bits, then four per number of extra bits, 258 at 285
            uint32_t const le = sym < 8 || sym == 28 ? 0 : (sym >> 2) - 1;
            uint32_t const lb = sym < 8 ? 3 + sym : sym == 28 ? 258 : ((4 | (sym & 3)) << le) + 3;
            uint32_t       x, dsym;
            if (!take(le, x))
                return kTruncated;
            uint32_t const len = lb + x;
            if ((rc = decode(T.dist, dsym)))
                return rc;
            if (dsym >= 30)
                return kBadSymbol;
            uint32_t const de = dsym < 4 ? 0 : (dsym >> 1) - 1;
            if (!take(de, x))
                return kTruncated;
            uint32_t const dist = (dsym < 4 ? 1 + dsym : ((2 | (dsym & 1)) << de) + 1) + x;
            if (!out.copy(dist, len))
                return out.dist_ok(dist) ? kOutputFull : kDistTooFar;
        }
    }

    __host__ __device__ uint32_t fixed_tables()
    {
        for (uint32_t s = 0; s < 288; ++s)
            T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        build(T.lit, T.lens, 288, false);
        for (uint32_t s = 0; s < 32; ++s) // (30 and 31 complete the code; decoding refuses them)
            T.lens[s] = 5;
        build(T.dist, T.lens, 32, false);
        return kOk;
    }

    __host__ __device__ uint32_t dynamic_tables()
    {
        uint32_t nlen, ndist, ncode;
        if (!take(5, nlen) || !take(5, ndist) || !take(4, ncode))
            return kTruncated;
        nlen += 257, ndist += 1, ncode += 4;
        if (nlen > 286 || ndist > 30)
            return kBadLengths;
        constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = 0; i < 19; ++i)
            T.lens[order[i]] = 0;
        for (uint32_t i = 0; i < ncode; ++i)
        {
            uint32_t v;
            if (!take(3, v))
                return kTruncated;
            T.lens[order[i]] = (uint8_t)v;
        }
        if (!build(T.lit, T.lens, 19, false)) // (the code-length code, in the literal table's place for now)
            return kBadCode;
        for (uint32_t i = 0; i < nlen + ndist;)
        {
            uint32_t sym, rc;
            if ((rc = decode(T.lit, sym)))
                return rc;
            if (sym < 16)
            {
                T.lens[i++] = (uint8_t)sym;
                continue;
            }
            uint32_t rep, prev = 0, x;
            if (sym == 16)
            {
                if (i == 0)
                    return kBadLengths;
                prev = T.lens[i - 1];
                if (!take(2, x))
                    return kTruncated;
                rep = 3 + x;
            }
            else if (sym == 17)
            {
                if (!take(3, x))
                    return kTruncated;
                rep = 3 + x;
            }
            else
            {
                if (!take(7, x))
                    return kTruncated;
                rep = 11 + x;
            }
            if (i + rep > nlen + ndist)
                return kBadLengths;
            while (rep--)
                T.lens[i++] = (uint8_t)prev;
        }
        if (T.lens[256] == 0) // no end-of-block code
            return kBadCode;
        // (the distance lengths first: the literal table is rebuilt over T.lens[0, nlen) after)
        if (!build(T.dist, T.lens + nlen, ndist, true) || !build(T.lit, T.lens, nlen, true))
            return kBadCode;
        return kOk;
    }

    // one block, header included; last = its BFINAL bit
    __host__ __device__ uint32_t block(uint32_t & last)
    {
        uint32_t type, rc;
        if (!take(1, last) || !take(2, type))
            return kTruncated;
        if (type == 0)
            rc = stored();
        else if (type == 1)
            rc = fixed_tables() ? kBadCode : codes();
        else if (type == 2)
            rc = (rc = dynamic_tables()) ? rc : codes();
        else
            rc = kBadBlockType;
        return rc;
    }

    // the whole stream up to and including its final block
    __host__ __device__ uint32_t run()
    {
        for (;;)
        {
            uint32_t last, rc;
            if ((rc = block(last)))
                return rc;
            if (last)
                return kOk;
        }
    }

    // decoding goes on at bit b of the input (lx_pgunzip.h: a chunk in the middle of a stream); beyond the input every take fails
    __host__ __device__ void seek_bit(uint64_t b)
    {
        pos   = (b >> 3) < (uint64_t)n ? (Index)(b >> 3) : n;
        bits  = 0;
        nbits = 0;
        uint32_t v;
        if ((b & 7) && !take((uint32_t)(b & 7), v))
            pos = n, nbits = 0, bits = 0;
    }
    // the bit of the input the next take reads
    __host__ __device__ uint64_t bit_pos() const { return 8 * (uint64_t)pos - nbits; }

    // input bytes the stream took (its last byte counted whole); valid after run() returned kOk
    __host__ __device__ Index consumed() const { return pos - nbits / 8; }
};

} // namespace inflate
} // namespace lx
