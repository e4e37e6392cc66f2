// lx_gunzip_stream.h -- what lx_gunzip and lx_gunzip_stream_* do on the host, in a form that does not know the handle: the member
// headers, a member on the calling thread, a plain member wave by wave (MemberWaves, over whatever runs a wave: the kernels of
// lx_pgunzip.hip in lx_gunzip_host.cpp, the same functions in loops in tests/native/gunzip_stream_check.cpp), and the stream
// itself (Stream<Env>): pieces, the text a wave left over, the resume on the host where the device path declines.
//
// A plain member of a stream, on the device: a wave decodes [start_bit, ...) into the stream's buffer behind the text not handed
// out yet; pieces of piece_bytes leave from the front; when less than a piece is left the next wave runs.  Across calls the stream
// keeps the bit where the next wave starts, the raw CRC register and the length so far (MemberWaves), and the text (StreamBuf),
// whose last 32 KiB are the window the next wave is given.  A wave that declines changes none of that, so StepInflater goes on at
// start_bit, on a block's first bit, with the window, the CRC and the length of the text so far -- and finds what the device
// declined over (stored data, a damaged block) in the call whose piece reaches it.  The trailer is checked where the host path
// checks it: in the call that would hand out the member's last bytes.
//
// Bound: a wave's text is at most slots x room bytes, room = kRoomPerByte x chunk, slots = stream_slots(): with the default chunk
// 10 x max(piece_bytes, 128 KiB), and never more than 512 x 640 KiB = 320 MiB.  That, and O(piece_bytes), is what a stream holds
// between two calls.
#pragma once
#include <sys/mman.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "lambda_ext.h"
#include "lx_crc32.h"
#include "lx_gunzip.h"
#include "lx_inflate.h"
#include "lx_pgunzip.h"

namespace lx
{
namespace gz
{

// the parallel path of a plain member (DESIGN 4.10 has the sums)
constexpr uint64_t kPlainChunk     = 64u << 10; // compressed bytes per chunk unless LX_OPT_GUNZIP_CHUNK says otherwise
constexpr uint32_t kPlainWave      = 512;       // chunks per wave at most: two decoders on each of 256 CUs
constexpr uint64_t kPlainWaveBytes = 32u << 20; // ... and compressed bytes per wave at most
constexpr uint64_t kPlainFrom      = 8u << 20;  // LX_OPT_GUNZIP_PARALLEL_FROM's default: above the measured crossover
constexpr uint64_t kPlainProbe     = 64u << 10; // DEFLATE bytes the host tries first: a member that ends inside them stays on the host

static_assert(kPlainWave <= pgunzip::kMaxWaveSlots, "chain_kernel's table");

struct CrcTable
{
    uint32_t t[256];
    CrcTable()
    {
        for (uint32_t i = 0; i < 256; ++i)
            t[i] = lx::crc_table_entry(i);
    }
};

inline uint32_t crc32(uint8_t const * p, uint64_t n, uint32_t crc = 0)
{
    static CrcTable const T;
    uint32_t              r = ~crc;
    for (uint64_t i = 0; i < n; ++i)
        r = (r >> 8) ^ T.t[(r ^ p[i]) & 0xff];
    return ~r;
}

inline uint32_t le32(uint8_t const * p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the result: out[0, size) is written, out's own size is the room
struct Result
{
    std::string out;
    uint64_t    size = 0;
    uint8_t *   reserve(uint64_t need) // room for `need` more bytes; (std::bad_alloc reaches the caller)
    {
        if (size + need > out.size())
            out.resize(std::max<uint64_t>(size + need, std::max<uint64_t>(2 * out.size(), 1u << 16)));
        return reinterpret_cast<uint8_t *>(&out[0]) + size;
    }
};

// a plain member's output, appended to the result, growing it as needed
struct HostSink
{
    Result &       r;
    uint64_t const base; // where the member's output begins
    bool put(uint8_t b)
    {
        *r.reserve(1) = b;
        ++r.size;
        return true;
    }
    bool dist_ok(uint32_t d) const { return d <= r.size - base; }
    bool copy(uint32_t d, uint32_t len)
    {
        if (!dist_ok(d))
            return false;
        uint8_t * const dst = r.reserve(len);
        for (uint32_t i = 0; i < len; ++i) // (overlapping: byte by byte)
            dst[i] = dst[(int64_t)i - (int64_t)d];
        r.size += len;
        return true;
    }
};

struct Header
{
    uint64_t end   = 0;  // the first DEFLATE byte
    int64_t  bsize = -1; // BC subfield: member bytes - 1; -1 = none
};

// the member header at `at`; an error text, or nullptr
inline char const * parse_header(uint8_t const * in, uint64_t n, uint64_t at, Header & hd)
{
    uint64_t const rest = n - at;
    if (rest < 10 || in[at] != 0x1f || in[at + 1] != 0x8b)
        return rest < 10 && rest >= 2 && in[at] == 0x1f && in[at + 1] == 0x8b ? "truncated gzip header" : "not a gzip member (no 1f 8b magic)";
    if (in[at + 2] != 8)
        return "compression method is not DEFLATE";
    uint8_t const flg = in[at + 3];
    if (flg & 0xe0)
        return "reserved header flags set";
    uint64_t p = at + 10;
    if (flg & 4) // FEXTRA
    {
        if (n - p < 2)
            return "truncated gzip header";
        uint32_t const xlen = in[p] | in[p + 1] << 8;
        p += 2;
        if (n - p < xlen)
            return "truncated gzip header";
        for (uint64_t q = p, e = p + xlen; e - q >= 4;) // the subfields; BC with SLEN 2 is BGZF's BSIZE
        {
            uint32_t const slen = in[q + 2] | in[q + 3] << 8;
            if (e - q - 4 < slen)
                return "extra field subfield runs past XLEN";
            if (in[q] == 'B' && in[q + 1] == 'C' && slen == 2)
                hd.bsize = in[q + 4] | in[q + 5] << 8;
            q += 4 + slen;
        }
        p += xlen;
    }
    for (uint8_t f : {uint8_t(8), uint8_t(16)}) // FNAME, FCOMMENT: zero-terminated
        if (flg & f)
        {
            while (p < n && in[p])
                ++p;
            if (p >= n)
                return "truncated gzip header";
            ++p;
        }
    if (flg & 2) // FHCRC: the low 16 bits of the header's CRC32
    {
        if (n - p < 2)
            return "truncated gzip header";
        if ((crc32(in + at, p - at) & 0xffff) != (uint32_t)(in[p] | in[p + 1] << 8))
            return "header CRC16 mismatch";
        p += 2;
    }
    hd.end = p;
    return nullptr;
}

// the member at `at` decoded on this thread, appended to res; *next = the byte after its trailer.  An error text, or nullptr.  With
// a limit (the probe in front of the parallel path) the decoder sees that many DEFLATE bytes only, and a stream that does not end
// inside them leaves the result where it was: *small = false
inline char const * host_member(uint8_t const * in, uint64_t n, uint64_t at, Header const & hd, Result & res, uint64_t * next,
                                uint64_t limit = UINT64_MAX, bool * small = nullptr)
{
    lx::inflate::Tables                       T;
    HostSink                                  sink{res, res.size};
    lx::inflate::Inflater<HostSink, uint64_t> inf(in + hd.end, std::min(n - hd.end, limit), sink, T);
    uint32_t const                            st = inf.run();
    if (small && !(*small = st == lx::inflate::kOk))
    {
        res.size = sink.base;
        return nullptr;
    }
    if (st != lx::inflate::kOk)
        return lx::inflate::status_text(st);
    uint64_t const t = hd.end + inf.consumed();
    if (n - t < 8)
        return "truncated gzip trailer";
    uint64_t const len = res.size - sink.base;
    if (crc32(reinterpret_cast<uint8_t const *>(res.out.data()) + sink.base, len) != le32(in + t))
        return "CRC32 mismatch";
    if ((uint32_t)len != le32(in + t + 4))
        return "ISIZE mismatch";
    if (hd.bsize >= 0 && t + 8 != at + (uint64_t)hd.bsize + 1)
        return "BSIZE does not match the member's DEFLATE stream";
    *next = t + 8;
    return nullptr;
}

// true: the member at `a` of in[0, n) is one for the BGZF path (`end` = the byte after it, `isize` its text)
inline bool bgzf_member(uint8_t const * in, uint64_t n, Header const & hd, uint64_t a, uint64_t * end, uint32_t * isize)
{
    if (hd.bsize < 0 || (uint64_t)hd.bsize + 1 > n - a)
        return false;
    uint64_t const e = a + (uint64_t)hd.bsize + 1;
    if (e < hd.end + 8 || e - 8 - hd.end > lx::kGunzipMaxPayload || le32(in + e - 4) > lx::kGunzipMaxIsize)
        return false;
    *end   = e;
    *isize = le32(in + e - 4);
    return true;
}

// ---- a plain member wave by wave ------------------------------------------------------------------------------------------------

// chunks per wave: the test knob or kPlainWave, and kPlainWaveBytes of input at most
inline uint32_t wave_slots(uint64_t chunk, uint64_t knob)
{
    return (uint32_t)std::min<uint64_t>(knob ? knob : kPlainWave, std::max<uint64_t>(2, kPlainWaveBytes / chunk));
}
// ... of a stream: no more than make a piece's worth of input, so that slots x room bounds what the stream holds between calls
inline uint32_t stream_slots(uint64_t chunk, uint64_t knob, uint64_t piece)
{
    return (uint32_t)std::min<uint64_t>(wave_slots(chunk, knob), std::max<uint64_t>(2, piece / chunk));
}

// what a wave is made from
struct WaveJob
{
    uint8_t const * in;       // the wave's input: from the byte of its first bit on
    uint64_t        n;        // ... bytes of it
    uint32_t        chunk, nslots, room;
    bool            first;    // slot 0 begins at the member's first bit
    uint64_t        found0;   // slot 0's first bit, in `in`
    uint64_t        stop_bit; // where the wave's last chunk may stop
    uint8_t const * win;      // the last `before` bytes of the member's text; nullptr: the runner kept the window behind its last wave
    uint32_t        before;   // min(bytes of the member's text so far, kWindow)
};

// A runner has  int run(WaveJob const &, pgunzip::WaveResult &)  -- find, decode, chain, resolve; LX_OK or the code of an error it
// has reported -- and  int fetch(uint8_t * dst, uint64_t len)  -- the bytes of the wave it ran last.
struct MemberWaves
{
    uint8_t const * d = nullptr; // the member's DEFLATE bytes and what follows them
    uint64_t        dlen = 0;
    uint64_t        chunk = 0;
    uint32_t        slots = 0;
    // what a stream keeps across calls, beside the text itself
    uint64_t start_bit = 0, out_len = 0, verified = 0, dropped = 0;
    uint32_t crc_raw = 0;                // the CRC register of out_len bytes: no initial value, no final complement
    bool     first = true, final = false;
    uint64_t end_byte = 0;               // final: DEFLATE bytes the member took

    uint32_t crc() const { return crc_raw ^ lx::mul_mod_p(pgunzip::x_pow_8n64(out_len), 0xffffffffu) ^ 0xffffffffu; }

    // one wave.  *reason != 0: declined, and nothing here has changed.  dest(len) says where the wave's len bytes go; win as in WaveJob
    template <class Runner, class Dest>
    int wave(Runner & run, lx_gunzip_stats & S, uint8_t const * win, Dest && dest, int * reason)
    {
        namespace pg = lx::pgunzip;
        *reason = LX_GUNZIP_DECLINE_NONE;
        uint64_t const base = start_bit >> 3, remain = dlen - base;
        if (remain == 0)
            return *reason = LX_GUNZIP_DECLINE_STATUS, (int)LX_OK;
        WaveJob j{};
        j.nslots   = (uint32_t)std::min<uint64_t>(slots, (remain + chunk - 1) / chunk);
        j.in       = d + base;
        j.n        = std::min<uint64_t>(remain, (uint64_t)(j.nslots + 1) * chunk);
        j.chunk    = (uint32_t)chunk;
        j.room     = (uint32_t)(pg::kRoomPerByte * chunk);
        j.first    = first;
        j.found0   = start_bit - 8 * base;
        j.stop_bit = 8 * std::min<uint64_t>(j.n, (uint64_t)j.nslots * chunk);
        j.win      = win;
        j.before   = (uint32_t)std::min<uint64_t>(out_len, pg::kWindow);
        pg::WaveResult r{};
        if (int const rc = run.run(j, r))
            return rc;
        S.bytes_up += j.n;
        ++S.waves;
        if (r.nver == 0)
            return *reason = r.status0 == pg::kChunkNoBoundary          ? LX_GUNZIP_DECLINE_NO_BOUNDARY
                             : r.status0 == lx::inflate::kOutputFull ? LX_GUNZIP_DECLINE_ROOM
                                                                     : LX_GUNZIP_DECLINE_STATUS,
                   (int)LX_OK;
        S.chunks += r.nver;
        S.chunks_dropped += r.dropped;
        if (pg::chain_gives_up(dropped + r.dropped, verified + r.nver))
            return *reason = LX_GUNZIP_DECLINE_CHAIN, (int)LX_OK;
        if (r.bad || r.wave_len > (uint64_t)j.nslots * j.room) // a distance before the start of the member's output
            return *reason = LX_GUNZIP_DECLINE_STATUS, (int)LX_OK;
        if (int const rc = run.fetch(dest(r.wave_len), r.wave_len))
            return rc;
        S.bytes_down += r.wave_len;
        verified += r.nver;
        dropped += r.dropped;
        crc_raw = lx::mul_mod_p(pg::x_pow_8n64(r.wave_len), crc_raw) ^ r.crc;
        out_len += r.wave_len;
        first = false;
        if (r.final)
        {
            final    = true;
            end_byte = base + (r.end_bit + 7) / 8;
        }
        else
            start_bit = 8 * base + r.end_bit;
        return LX_OK;
    }
};

// ---- lx_gunzip_stream: the same walk, piece by piece ----------------------------------------------------------------------------
//
// The text not handed out yet: buf[base + keep, base + keep + fill), behind the last `keep` (<= 32 KiB) bytes of what was handed
// out -- the window a plain member's back-references still reach.  A piece taken from the front of a wave's text moves `base`,
// not the text.
struct StreamBuf
{
    std::string buf;
    uint64_t    base = 0, keep = 0, fill = 0;
    uint64_t    end() const { return base + keep + fill; }
    uint8_t *   room(uint64_t need) // room for `need` more bytes behind the text
    {
        if (end() + need > buf.size() && base)
        {
            std::memmove(&buf[0], buf.data() + base, keep + fill);
            base = 0;
        }
        uint64_t const at = end();
        if (at + need > buf.size())
            buf.resize(std::max<uint64_t>(at + need, std::max<uint64_t>(2 * buf.size(), 1u << 16)));
        return reinterpret_cast<uint8_t *>(&buf[0]) + at;
    }
    // the last w bytes of the text (handed out or not); w <= keep + fill
    uint8_t const * tail(uint64_t w) const { return reinterpret_cast<uint8_t const *>(buf.data()) + end() - w; }
    // the first len (<= fill) bytes of the text leave; the last 32 KiB in front of what stays, stay
    std::string take(uint64_t len)
    {
        std::string piece(buf.data() + base + keep, len);
        if (len == fill)
        {
            uint64_t const all = end(), w = std::min<uint64_t>(keep + fill, 32768);
            if (w)
                std::memmove(&buf[0], buf.data() + (all - w), w);
            base = 0;
            keep = w;
            fill = 0;
        }
        else
        {
            uint64_t const w = std::min<uint64_t>(keep + len, 32768);
            base += keep + len - w;
            keep = w;
            fill -= len;
        }
        return piece;
    }
    void forget() { base = keep = fill = 0; }
};

struct StreamSink
{
    StreamBuf & b;
    uint64_t    member = 0; // bytes of the current member so far
    bool put(uint8_t v)
    {
        *b.room(1) = v;
        ++b.fill;
        ++member;
        return true;
    }
    bool dist_ok(uint32_t d) const { return d <= member; }
    bool copy(uint32_t d, uint32_t len)
    {
        if (!dist_ok(d))
            return false;
        uint8_t * const dst = b.room(len); // (d <= min(member, 32768) <= keep + fill: the source is in the buffer)
        for (uint32_t i = 0; i < len; ++i)
            dst[i] = dst[(int64_t)i - (int64_t)d];
        b.fill += len;
        member += len;
        return true;
    }
};

// the Inflater, stopping between two symbols or two blocks once the sink holds `limit` bytes: at most 257 bytes (a copy) or
// 65 535 (a stored block) beyond it.  codes() is restated here with that one check; everything else is the Inflater's own.
struct StepInflater : lx::inflate::Inflater<StreamSink, uint64_t>
{
    using Base = lx::inflate::Inflater<StreamSink, uint64_t>;
    using Base::Base;
    bool     in_codes = false, done = false;
    uint32_t last = 0;

    // the decoder goes on at `bit`, a block's first bit in the middle of the member: the sink holds the window in front of it and
    // says how much text the member has so far
    void start_at(uint64_t bit)
    {
        seek_bit(bit);
        in_codes = done = false;
    }

    // kOk with done = false: the limit was reached
    uint32_t step(uint64_t limit)
    {
        namespace fl = lx::inflate;
        for (;;)
        {
            if (!in_codes)
            {
                if (out.b.fill >= limit)
                    return fl::kOk;
                uint32_t type, rc = fl::kOk;
                if (!take(1, last) || !take(2, type))
                    return fl::kTruncated;
                if (type == 0)
                {
                    if ((rc = stored()))
                        return rc;
                    if ((done = last != 0))
                        return fl::kOk;
                    continue;
                }
                if (type == 1)
                    fixed_tables();
                else if (type == 2)
                    rc = dynamic_tables();
                else
                    rc = fl::kBadBlockType;
                if (rc)
                    return rc;
                in_codes = true;
            }
            for (;;)
            {
                if (out.b.fill >= limit)
                    return fl::kOk;
                uint32_t sym, rc;
                if ((rc = decode(T.lit, sym)))
                    return rc;
                if (sym < 256)
                {
                    out.put((uint8_t)sym);
                    continue;
                }
                if (sym == 256)
                    break;
                sym -= 257;
                if (sym >= 29)
                    return fl::kBadSymbol;
                uint32_t const le = sym < 8 || sym == 28 ? 0 : (sym >> 2) - 1;
                uint32_t const lb = sym < 8 ? 3 + sym : sym == 28 ? 258 : ((4 | (sym & 3)) << le) + 3;
                uint32_t       x, dsym;
                if (!take(le, x))
                    return fl::kTruncated;
                uint32_t const len = lb + x;
                if ((rc = decode(T.dist, dsym)))
                    return rc;
                if (dsym >= 30)
                    return fl::kBadSymbol;
                uint32_t const de = dsym < 4 ? 0 : (dsym >> 1) - 1;
                if (!take(de, x))
                    return fl::kTruncated;
                uint32_t const dist = (dsym < 4 ? 1 + dsym : ((2 | (dsym & 1)) << de) + 1) + x;
                if (!out.copy(dist, len))
                    return fl::kDistTooFar;
            }
            in_codes = false;
            if ((done = last != 0))
                return fl::kOk;
        }
    }
};

// The stream over in[0, n).  Env is what the handle is to lx_gunzip_stream_* (and what a test puts in its place):
//   lx_gunzip_stats * stats()          the counts of the current call; nullptr: no device, every member on this thread
//   uint64_t parallel_from()           LX_OPT_GUNZIP_PARALLEL_FROM (0 = default), chunk_bytes(), wave_knob() likewise
//   Runner & runner()                  what runs a wave (MemberWaves)
//   int error(k, at, why)              reports "member k at byte at: why", returns its code
//   int group(in, len, k, at, Result&) whole BGZF members in[0, len) -- members k.. of the file, from its byte `at` -- appended to
//                                      the result, as lx_gunzip decodes them
template <class Env>
struct Stream
{
    Env &           env;
    uint8_t const * in = nullptr;
    uint64_t        n = 0;
    void *          map = nullptr; // the file, where it is mapped: pages in front of what is being decoded are given back
    uint64_t        piece = 0;
    bool            gz = false, failed = false;
    uint64_t        at = 0, k = 0; // the next member: its first byte, its number
    uint64_t        released = 0;  // pages of the mapping in front of this byte were given back
    StreamBuf       sb;
    // the plain member being decoded: by `inf` on this thread, or (on_device) by `mw` wave by wave
    lx::inflate::Tables           T;
    StreamSink                    sink{sb};
    std::unique_ptr<StepInflater> inf;
    MemberWaves                   mw;
    bool                          on_device = false;
    Header                        hd;
    uint64_t                      crc_done = 0; // bytes of the member in `crc`: the last sink.member - crc_done bytes of the text are not
                                                // (a count, not a place: the buffer moves its text when it makes room)
    uint32_t                      crc = 0;

    explicit Stream(Env & e) : env(e) {}

    int fail_member(char const * why)
    {
        failed = true;
        return env.error(k, at, why);
    }
    void crc_up()
    {
        uint64_t const todo = sink.member - crc_done; // (still in the buffer: a piece leaves only behind a crc_up)
        crc      = crc32(sb.tail(todo), todo, crc);
        crc_done = sink.member;
    }
    // the compressed bytes in front of `upto` are done with: their pages need not stay resident
    void release(uint64_t upto)
    {
        uint64_t const page = 4096, lo = (released + page - 1) / page * page, hi = upto / page * page;
        if (map && hi > lo)
        {
            madvise(static_cast<uint8_t *>(map) + lo, hi - lo, MADV_DONTNEED);
            released = hi;
        }
    }
    // a piece leaves (fill >= piece): all of the text, or, of a wave's text, piece bytes
    int emit(std::string & out, bool & have)
    {
        if (inf)
            crc_up();
        out  = sb.take(on_device || sb.fill > piece + 65536 ? std::min(piece, sb.fill) : sb.fill);
        have = true;
        release(inf ? hd.end + inf->pos - std::min<uint64_t>(inf->pos, 8) : on_device ? hd.end + (mw.start_bit >> 3) : at);
        return LX_OK;
    }
    // the trailer behind DEFLATE byte t of the current member: an error text, or nullptr
    char const * trailer(uint64_t t, uint32_t crc_, uint64_t len) const
    {
        return n - t < 8                                                ? "truncated gzip trailer"
               : crc_ != le32(in + t)                                   ? "CRC32 mismatch"
               : (uint32_t)len != le32(in + t + 4)                      ? "ISIZE mismatch"
               : hd.bsize >= 0 && t + 8 != at + (uint64_t)hd.bsize + 1 ? "BSIZE does not match the member's DEFLATE stream"
                                                                        : nullptr;
    }
    // lx_gunzip's condition for the device path, from where the stream stands: enough input behind the header, and a DEFLATE
    // stream that does not end inside the first kPlainProbe bytes (tried without output: ~0.4 ms).  One exception, kept from
    // before the stream had a device path: with a threshold of fewer than 10 bytes, where lx_gunzip skips its probe and goes to the
    // device, a stream stays on this thread.  Nothing in the design asks for it; tests/test_gpu_gunzip_stream.py sets the
    // threshold to 1 and holds the stream to the host path, and that behaviour is kept
    bool wants_device()
    {
        if (!env.stats())
            return false;
        uint64_t const from = env.parallel_from() ? env.parallel_from() : kPlainFrom;
        if (from == UINT64_MAX || from <= 9 || n - hd.end < from)
            return false;
        pgunzip::NullSink                                  none;
        lx::inflate::Inflater<pgunzip::NullSink, uint64_t> probe(in + hd.end, std::min(n - hd.end, std::min(from - 9, kPlainProbe)), none, T);
        return probe.run() != lx::inflate::kOk;
    }
    // the next piece; have = false at the end
    int next(std::string & out, bool & have)
    {
        have = false;
        if (!gz) // the file's own bytes
        {
            uint64_t const len = std::min(piece, n - at);
            if (len)
            {
                out  = std::string(reinterpret_cast<char const *>(in) + at, len);
                have = true;
            }
            at += len;
            release(at);
            return LX_OK;
        }
        for (;;)
        {
            if (sb.fill >= piece)
                return emit(out, have);
            if (on_device)
            {
                lx_gunzip_stats & S = *env.stats();
                if (mw.final) // (less than a piece of it is left: this call would hand out the member's last bytes)
                {
                    uint64_t const t = hd.end + mw.end_byte;
                    if (char const * bad = trailer(t, mw.crc(), mw.out_len))
                        return fail_member(bad);
                    on_device = false;
                    ++S.plain_parallel;
                    at = t + 8;
                    ++k;
                    release(at);
                    continue;
                }
                int            why = 0;
                uint64_t const had = mw.out_len, before = std::min<uint64_t>(had, pgunzip::kWindow);
                int const      rc  = mw.wave(env.runner(), S, sb.tail(before), [&](uint64_t len) { return sb.room(len); }, &why);
                if (rc)
                    return failed = true, rc;
                sb.fill += mw.out_len - had;
                if (why) // the host goes on where the last verified chunk ended; what it finds there is its to report
                {
                    ++S.declined;
                    S.last_decline = why;
                    on_device      = false;
                    sink.member    = mw.out_len;
                    crc            = mw.crc();
                    crc_done       = mw.out_len;
                    inf.reset(new StepInflater(in + hd.end, n - hd.end, sink, T));
                    inf->start_at(mw.start_bit);
                }
                else
                    release(hd.end + (mw.start_bit >> 3));
                continue;
            }
            if (inf)
            {
                uint32_t const st = inf->step(piece);
                if (st != lx::inflate::kOk)
                    return fail_member(lx::inflate::status_text(st));
                if (!inf->done)
                    continue; // (the limit: the piece leaves at the loop's head)
                uint64_t const t = hd.end + inf->consumed();
                crc_up();
                if (char const * bad = trailer(t, crc, sink.member))
                    return fail_member(bad);
                inf.reset();
                if (env.stats())
                    ++env.stats()->plain_host;
                at = t + 8;
                ++k;
                continue;
            }
            if (at >= n)
                return sb.fill ? emit(out, have) : (int)LX_OK;
            hd = Header{};
            if (char const * bad = parse_header(in, n, at, hd))
                return fail_member(bad);
            if (hd.bsize >= 0 && (uint64_t)hd.bsize + 1 > n - at)
                return fail_member("BSIZE points past the end of the data");
            uint64_t end   = 0;
            uint32_t isize = 0;
            if (bgzf_member(in, n, hd, at, &end, &isize))
            {
                // whole members until the piece is full, through the walk of lx_gunzip: on the device, or one by one on this thread
                uint64_t sum = isize, members = 1;
                for (Header g; sb.fill + sum < piece && end < n; ++members)
                {
                    g = Header{};
                    uint64_t e2 = 0;
                    if (parse_header(in, n, end, g) || !bgzf_member(in, n, g, end, &e2, &isize))
                        break;
                    sum += isize;
                    end = e2;
                }
                Result    r;
                int const rc = env.group(in + at, end - at, k, at, r);
                if (rc)
                    return failed = true, rc;
                at = end;
                k += members;
                release(at);
                if (sb.fill == 0 && r.size >= piece) // (nothing waits in front of it: the group's text is the piece)
                {
                    r.out.resize(r.size);
                    out  = std::move(r.out);
                    have = true;
                    sb.forget();
                    return LX_OK;
                }
                std::memcpy(sb.room(r.size), r.out.data(), r.size);
                sb.fill += r.size;
                continue;
            }
            if (env.stats() && hd.bsize >= 0 && at + (uint64_t)hd.bsize + 1 < hd.end + 8)
                return fail_member("BSIZE is smaller than the member's header and trailer");
            sink.member = 0;
            crc         = 0;
            crc_done    = 0;
            if (wants_device())
            {
                mw       = MemberWaves{};
                mw.d     = in + hd.end;
                mw.dlen  = n - hd.end;
                mw.chunk = env.chunk_bytes() ? env.chunk_bytes() : kPlainChunk;
                mw.slots = stream_slots(mw.chunk, env.wave_knob(), piece);
                on_device = true;
                continue;
            }
            inf.reset(new StepInflater(in + hd.end, n - hd.end, sink, T));
        }
    }
};

} // namespace gz
} // namespace lx
