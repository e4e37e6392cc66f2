// lx_gunzip_host.cpp -- lx_gunzip: gzip streams (RFC 1952) of one or more members; BGZF members on the device (lx_gunzip.hip),
// every other member on the calling thread with the same DEFLATE code (lx_inflate.h).
//
// The host walks the member headers.  A member with the BGZF subfield (BC, BSIZE) has its end, its trailer and so its ISIZE
// without being decoded: consecutive ones form a run, a table of (input offset, length, output offset, ISIZE, CRC), and the run
// streams through the device in chunks of kChunkMembers members.  Per chunk, on the handle's stream: its bytes and table up from a
// pinned lane, the kernel, its status words down to the pinned lane, its output down into the result itself.  The host fills the
// other pinned lane with the next chunk while the device decodes this one.  A member without BSIZE ends where its DEFLATE stream
// ends, so it is decoded here, in order, before the walk goes on; so is every member when no handle is given.
//
// A plain member with enough input behind its header goes to the device first (parallel_member, lx_pgunzip.h / .hip): its DEFLATE
// bytes in waves of chunks -- find, decode with markers, chain check here, resolve -- and its bytes down into the result.  Nothing
// of it counts before the trailer's CRC32 and ISIZE agree; in every other case the member is declined, the result is where it was,
// and host_member decodes it from its first byte: today's bytes or today's error text.
//
// lx_gunzip_stream_* is the same walk over a mapped file, handing the text out in pieces: BGZF members in groups whose text fills a
// piece, each group a Walk of its own over its slice of the file (so the device path and the error texts are lx_gunzip's); every
// other member through StepInflater, which stops between two symbols when the piece is full and keeps a 32 KiB window.  It never
// takes the parallel path: that one wants the whole member's text on the device at once.
#include "lx_crc32.h"
#include "lx_gunzip.h"
#include "lx_inflate.h"
#include "lx_internal.h"
#include "lx_pgunzip.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <memory>
#include <string>
#include <vector>

using namespace lxi;

namespace
{

constexpr uint32_t kChunkMembers = 512; // 32 MiB of input and output at most per chunk

// the parallel path of a plain member (DESIGN 4.10 has the sums)
constexpr uint64_t kPlainChunk     = 64u << 10; // compressed bytes per chunk unless LX_OPT_GUNZIP_CHUNK says otherwise
constexpr uint32_t kPlainWave      = 512;       // chunks per wave at most: two decoders on each of 256 CUs
constexpr uint64_t kPlainWaveBytes = 32u << 20; // ... and compressed bytes per wave at most
constexpr uint64_t kPlainFrom      = 8u << 20;  // LX_OPT_GUNZIP_PARALLEL_FROM's default: above the measured crossover
constexpr uint64_t kPlainProbe     = 64u << 10; // DEFLATE bytes the host tries first: a member that ends inside them stays on the host

struct CrcTable
{
    uint32_t t[256];
    CrcTable()
    {
        for (uint32_t i = 0; i < 256; ++i)
            t[i] = lx::crc_table_entry(i);
    }
};

uint32_t crc32(uint8_t const * p, uint64_t n, uint32_t crc = 0)
{
    static CrcTable const T;
    uint32_t              r = ~crc;
    for (uint64_t i = 0; i < n; ++i)
        r = (r >> 8) ^ T.t[(r ^ p[i]) & 0xff];
    return ~r;
}

uint32_t le32(uint8_t const * p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the result: out[0, size) is written, out's own size is the room
struct Result
{
    std::string out;
    uint64_t    size = 0;
    uint8_t *   reserve(uint64_t need) // room for `need` more bytes; (std::bad_alloc reaches lx_gunzip)
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
char const * parse_header(uint8_t const * in, uint64_t n, uint64_t at, Header & hd)
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

// what is wrong with member k, which begins at byte `at` of the file
int member_error(lx_handle * h, uint64_t k, uint64_t at, char const * why)
{
    char buf[320];
    snprintf(buf, sizeof(buf), "lx_gunzip: member %llu at byte %llu: %s", (unsigned long long)k, (unsigned long long)at, why);
    if (h)
        return fail(h, LX_EINVAL, "%s", buf);
    set_output_error(buf);
    return LX_EINVAL;
}

struct Walk
{
    lx_handle *     h;
    uint8_t const * in;
    uint64_t        n;
    Result &        res;
    uint64_t        k_base = 0, at_base = 0; // in[0, n) is a slice of a file (lx_gunzip_stream): the members and bytes in front of it

    int error(uint64_t k, uint64_t at, char const * why) { return member_error(h, k_base + k, at_base + at, why); }

    // a member decoded here; *next = the byte after its trailer.  With a limit (the probe in front of the parallel path) the decoder
    // sees that many DEFLATE bytes only, and a stream that does not end inside them leaves the result where it was: *small = false
    int host_member(uint64_t k, uint64_t at, Header const & hd, uint64_t * next, uint64_t limit = UINT64_MAX, bool * small = nullptr)
    {
        lx::inflate::Tables                            T;
        HostSink                                   sink{res, res.size};
        lx::inflate::Inflater<HostSink, uint64_t>      inf(in + hd.end, std::min(n - hd.end, limit), sink, T);
        uint32_t const                             st = inf.run();
        if (small && !(*small = st == lx::inflate::kOk))
        {
            res.size = sink.base;
            return LX_OK;
        }
        if (st != lx::inflate::kOk)
            return error(k, at, lx::inflate::status_text(st));
        uint64_t const t = hd.end + inf.consumed();
        if (n - t < 8)
            return error(k, at, "truncated gzip trailer");
        uint64_t const len = res.size - sink.base;
        if (crc32(reinterpret_cast<uint8_t const *>(res.out.data()) + sink.base, len) != le32(in + t))
            return error(k, at, "CRC32 mismatch");
        if ((uint32_t)len != le32(in + t + 4))
            return error(k, at, "ISIZE mismatch");
        if (hd.bsize >= 0 && t + 8 != at + (uint64_t)hd.bsize + 1)
            return error(k, at, "BSIZE does not match the member's DEFLATE stream");
        *next = t + 8;
        return LX_OK;
    }

    // a plain member through the device; *reason = 0: done, *next = the byte after its trailer; else declined (the result untouched)
    int parallel_member(uint64_t at, Header const & hd, uint64_t * next, int * reason)
    {
        namespace pg = lx::pgunzip;
        auto &                G = h->gunzip;
        lx_gunzip_stats &     S = G.stats;
        uint8_t const * const d = in + hd.end;
        uint64_t const        dlen = n - hd.end;
        uint64_t const        C    = h->opt_gunzip_chunk ? h->opt_gunzip_chunk : kPlainChunk;
        uint32_t const        W    = (uint32_t)std::min<uint64_t>(h->gunzip_wave ? h->gunzip_wave : kPlainWave, std::max<uint64_t>(2, kPlainWaveBytes / C));
        uint32_t const        room = (uint32_t)(pg::kRoomPerByte * C);
        auto decline = [&](int why)
        {
            *reason = why;
            return LX_OK;
        };
        *reason = LX_GUNZIP_DECLINE_NONE;
        int rc = bind(h);
        if (rc)
            return rc;
        hipStream_t const s      = h->stream;
        uint32_t const    wslots = (uint32_t)std::min<uint64_t>(W, (dlen + C - 1) / C);
        size_t const      slot_bytes = sizeof(uint64_t) + sizeof(pg::ChunkResult);
        if ((rc = ensure(h, G.d_pin, (size_t)std::min<uint64_t>(dlen, (uint64_t)(wslots + 1) * C))) || (rc = ensure(h, G.d_slots, wslots * slot_bytes)) ||
            (rc = ensure(h, G.d_sym, (size_t)wslots * room * 2)) || (rc = ensure(h, G.d_win, (size_t)(wslots + 1) * pg::kWindow)) ||
            (rc = ensure(h, G.d_ver, wslots * sizeof(pg::Verified))) || (rc = ensure(h, G.d_crc, 8)) ||
            (rc = ensure_pinned(h, G.p_slots, wslots * slot_bytes, kRoom)) || (rc = ensure_pinned(h, G.p_ver, wslots * sizeof(pg::Verified), kRoom)) ||
            (rc = ensure_pinned(h, G.p_crc, 8, kExact)))
            return rc;
        // (room for the whole member at once where the input's last four bytes can be its ISIZE: a hint, never a fact)
        if (n >= 4 && le32(in + n - 4) <= 1032 * dlen)
            res.reserve(le32(in + n - 4));
        uint64_t start_bit = 0, out_len = 0, verified = 0, dropped = 0;
        uint32_t crc_raw = 0, carry = 0;
        std::vector<uint32_t> ver(wslots);
        for (bool first = true;; first = false)
        {
            uint64_t const base   = start_bit >> 3;
            uint64_t const remain = dlen - base;
            if (remain == 0)
                return decline(LX_GUNZIP_DECLINE_STATUS);
            uint32_t const nslots = (uint32_t)std::min<uint64_t>(W, (remain + C - 1) / C);
            uint64_t const wave_n = std::min<uint64_t>(remain, (uint64_t)(nslots + 1) * C);
            auto * const   d_found = static_cast<uint64_t *>(G.d_slots.ptr);
            auto * const   d_res   = reinterpret_cast<pg::ChunkResult *>(d_found + nslots);
            auto * const   p_found = static_cast<uint64_t *>(G.p_slots.ptr);
            auto * const   p_res   = reinterpret_cast<pg::ChunkResult *>(p_found + nslots);
            pg::WaveParams wp{};
            wp.in         = static_cast<uint8_t const *>(G.d_pin.ptr);
            wp.n          = (uint32_t)wave_n;
            wp.chunk      = (uint32_t)C;
            wp.nslots     = nslots;
            wp.room       = room;
            wp.first_wave = first;
            wp.stop_bit   = 8 * std::min<uint64_t>(wave_n, (uint64_t)nslots * C);
            wp.found      = d_found;
            wp.res        = d_res;
            wp.sym        = static_cast<uint16_t *>(G.d_sym.ptr);
            p_found[0]    = start_bit - 8 * base;
            LX_HIP(h, hipMemcpyAsync(G.d_pin.ptr, d + base, wave_n, hipMemcpyHostToDevice, s));
            LX_HIP(h, hipMemcpyAsync(d_found, p_found, 8, hipMemcpyHostToDevice, s));
            // (three events per wave, read and given back at the wave's end: a member of any length keeps its phase times)
            size_t const   ev_mark = h->ev_pool_used;
            hipEvent_t const e0 = pool_event(h), e1 = pool_event(h), e2 = pool_event(h), e3 = pool_event(h), e4 = pool_event(h);
            if (!e0 || !e1 || !e2 || !e3 || !e4)
                return fail(h, LX_EHIP, "lx_gunzip: no event");
            LX_HIP(h, hipEventRecord(e0, s));
            LX_HIP(h, pg::launch_find(wp, s));
            LX_HIP(h, hipEventRecord(e1, s));
            LX_HIP(h, pg::launch_decode(wp, s));
            LX_HIP(h, hipEventRecord(e2, s));
            LX_HIP(h, hipMemcpyAsync(p_found, d_found, nslots * slot_bytes, hipMemcpyDeviceToHost, s));
            LX_HIP(h, hipStreamSynchronize(s));
            S.bytes_up += wave_n;
            ++S.waves;
            pg::Chain const c = pg::chain(p_found, p_res, nslots, ver.data());
            if (c.nver == 0)
                return decline(p_res[0].status == pg::kChunkNoBoundary          ? LX_GUNZIP_DECLINE_NO_BOUNDARY
                               : p_res[0].status == lx::inflate::kOutputFull ? LX_GUNZIP_DECLINE_ROOM
                                                                             : LX_GUNZIP_DECLINE_STATUS);
            S.chunks += c.nver;
            S.chunks_dropped += c.dropped;
            verified += c.nver;
            dropped += c.dropped;
            if (pg::chain_gives_up(dropped, verified))
                return decline(LX_GUNZIP_DECLINE_CHAIN);
            // ---- resolve: the verified chunks' places, windows, bytes
            auto *   pv = static_cast<pg::Verified *>(G.p_ver.ptr);
            uint64_t wave_len = 0;
            uint32_t longest = 0;
            for (uint32_t v = 0; v < c.nver; ++v)
            {
                pg::ChunkResult const & r = p_res[ver[v]];
                pv[v] = pg::Verified{(uint64_t)ver[v] * room, wave_len, r.count, (uint32_t)std::min<uint64_t>(pg::kWindow, out_len + wave_len)};
                wave_len += r.count;
                longest = std::max(longest, r.count);
            }
            if ((rc = ensure(h, G.d_bytes, (size_t)wave_len)))
                return rc;
            auto * const win = static_cast<uint8_t *>(G.d_win.ptr);
            if (!first && carry) // (the window behind the last wave's last chunk lies in front of this wave's first)
                LX_HIP(h, hipMemcpyAsync(win, win + (uint64_t)carry * pg::kWindow, pg::kWindow, hipMemcpyDeviceToDevice, s));
            LX_HIP(h, hipMemsetAsync(G.d_crc.ptr, 0, 8, s));
            LX_HIP(h, hipMemcpyAsync(G.d_ver.ptr, pv, c.nver * sizeof(pg::Verified), hipMemcpyHostToDevice, s));
            pg::ResolveParams rp{};
            rp.sym      = static_cast<uint16_t const *>(G.d_sym.ptr);
            rp.ver      = static_cast<pg::Verified const *>(G.d_ver.ptr);
            rp.nver     = c.nver;
            rp.segs     = (longest + pg::kWindow - 1) / pg::kWindow;
            rp.win      = win;
            rp.out      = static_cast<uint8_t *>(G.d_bytes.ptr);
            rp.wave_len = (uint32_t)wave_len;
            rp.crc      = static_cast<uint32_t *>(G.d_crc.ptr);
            LX_HIP(h, hipEventRecord(e3, s));
            LX_HIP(h, pg::launch_resolve(rp, s));
            LX_HIP(h, hipEventRecord(e4, s));
            carry = c.nver;
            uint8_t * const dst = res.reserve(out_len + wave_len) + out_len; // (no copy is in flight: the last wave's was waited for)
            if (wave_len)
                LX_HIP(h, hipMemcpyAsync(dst, G.d_bytes.ptr, wave_len, hipMemcpyDeviceToHost, s));
            LX_HIP(h, hipMemcpyAsync(G.p_crc.ptr, G.d_crc.ptr, 8, hipMemcpyDeviceToHost, s));
            LX_HIP(h, hipStreamSynchronize(s));
            S.bytes_down += wave_len;
            {
                hipEvent_t const ev[3][2] = {{e0, e1}, {e1, e2}, {e3, e4}};
                for (int i = 0; i < 3; ++i)
                {
                    float ms = 0.f;
                    LX_HIP(h, hipEventElapsedTime(&ms, ev[i][0], ev[i][1]));
                    G.phase_ms[i] += ms;
                    ++G.phase_launches[i];
                }
                h->ev_pool_used = ev_mark;
            }
            uint32_t const * const pc = static_cast<uint32_t const *>(G.p_crc.ptr);
            if (pc[1]) // a distance before the start of the member's output
                return decline(LX_GUNZIP_DECLINE_STATUS);
            crc_raw = lx::mul_mod_p(pg::x_pow_8n64(wave_len), crc_raw) ^ pc[0];
            out_len += wave_len;
            if (c.final)
            {
                uint64_t const t = hd.end + base + (c.end_bit + 7) / 8;
                if (n - t < 8 || (hd.bsize >= 0 && t + 8 != at + (uint64_t)hd.bsize + 1))
                    return decline(LX_GUNZIP_DECLINE_TRAILER);
                if ((crc_raw ^ lx::mul_mod_p(pg::x_pow_8n64(out_len), 0xffffffffu) ^ 0xffffffffu) != le32(in + t))
                    return decline(LX_GUNZIP_DECLINE_CRC);
                if ((uint32_t)out_len != le32(in + t + 4))
                    return decline(LX_GUNZIP_DECLINE_ISIZE);
                res.size += out_len;
                *next = t + 8;
                return LX_OK;
            }
            start_bit = 8 * base + c.end_bit;
        }
    }

    // a run of BGZF members (offsets absolute in `in`, output from res.size on) through the device
    int device_run(std::vector<lx::GunzipMember> & run, std::vector<uint64_t> const & starts, uint64_t k0)
    {
        if (run.empty())
            return LX_OK;
        uint64_t total = 0;
        for (auto const & m : run)
            total += m.isize;
        uint8_t * const dst0 = res.reserve(total);
        int             rc   = bind(h);
        if (rc)
            return rc;
        auto &         G      = h->gunzip;
        hipStream_t const s   = h->stream;
        uint64_t const nm     = run.size();
        uint64_t const chunks = (nm + kChunkMembers - 1) / kChunkMembers;
        size_t const   cap    = (size_t)std::min<uint64_t>(nm, kChunkMembers);
        if ((rc = ensure(h, G.d_in, cap * 65536)) || (rc = ensure(h, G.d_out, cap * 65536)) ||
            (rc = ensure(h, G.d_mem, cap * sizeof(lx::GunzipMember))) || (rc = ensure(h, G.d_status, cap * 4)))
            return rc;
        for (int l = 0; l < 2; ++l)
            if ((rc = ensure_pinned(h, G.p_in[l], cap * 65536, kExact)) || (rc = ensure_pinned(h, G.p_mem[l], cap * sizeof(lx::GunzipMember), kExact)) ||
                (rc = ensure_pinned(h, G.p_status[l], cap * 4, kExact)))
                return rc;
        struct Chunk
        {
            uint64_t m0, m1, in_lo, in_n, out_lo, out_n;
        };
        auto chunk = [&](uint64_t c)
        {
            Chunk ck;
            ck.m0    = c * kChunkMembers;
            ck.m1    = std::min(nm, ck.m0 + kChunkMembers);
            ck.in_lo = starts[ck.m0];
            ck.in_n  = starts[ck.m1] - ck.in_lo;
            ck.out_lo = run[ck.m0].out_off;
            ck.out_n  = run[ck.m1 - 1].out_off + run[ck.m1 - 1].isize - ck.out_lo;
            return ck;
        };
        // the chunk's bytes and table into its pinned lane (offsets made relative to the chunk)
        auto stage = [&](uint64_t c)
        {
            Chunk const ck = chunk(c);
            std::memcpy(G.p_in[c & 1].ptr, in + ck.in_lo, ck.in_n);
            auto * t = static_cast<lx::GunzipMember *>(G.p_mem[c & 1].ptr);
            for (uint64_t i = ck.m0; i < ck.m1; ++i)
            {
                t[i - ck.m0] = run[i];
                t[i - ck.m0].in_off -= ck.in_lo;
                t[i - ck.m0].out_off -= ck.out_lo;
            }
        };
        auto enqueue = [&](uint64_t c) -> int
        {
            Chunk const ck = chunk(c);
            LX_HIP(h, hipMemcpyAsync(G.d_in.ptr, G.p_in[c & 1].ptr, ck.in_n, hipMemcpyHostToDevice, s));
            LX_HIP(h, hipMemcpyAsync(G.d_mem.ptr, G.p_mem[c & 1].ptr, (ck.m1 - ck.m0) * sizeof(lx::GunzipMember), hipMemcpyHostToDevice, s));
            lx::GunzipParams p{static_cast<uint8_t const *>(G.d_in.ptr), ck.in_n, static_cast<lx::GunzipMember const *>(G.d_mem.ptr),
                               (uint32_t)(ck.m1 - ck.m0), static_cast<uint8_t *>(G.d_out.ptr), ck.out_n, static_cast<uint32_t *>(G.d_status.ptr)};
            PhaseTimer t(h, s, 5);
            LX_HIP(h, lx::launch_gunzip(p, s));
            t.close();
            LX_HIP(h, hipMemcpyAsync(G.p_status[c & 1].ptr, G.d_status.ptr, (ck.m1 - ck.m0) * 4, hipMemcpyDeviceToHost, s));
            return LX_OK;
        };
        // the status words of chunk c (its copy done)
        auto check = [&](uint64_t c) -> int
        {
            Chunk const      ck = chunk(c);
            uint32_t const * st = static_cast<uint32_t const *>(G.p_status[c & 1].ptr);
            for (uint64_t i = ck.m0; i < ck.m1; ++i)
                if (uint32_t const v = st[i - ck.m0])
                {
                    (void)hipStreamSynchronize(s);
                    char const * why = v == lx::kGunzipCrc        ? "CRC32 mismatch"
                                       : v == lx::kGunzipIsize    ? "ISIZE mismatch (the DEFLATE stream ends early)"
                                       : v == lx::kGunzipTrailing ? "BSIZE does not match the member's DEFLATE stream"
                                       : v == lx::kGunzipBounds   ? "member outside its chunk"
                                                                  : lx::inflate::status_text(v);
                    return error(k0 + i, starts[i], why);
                }
            return LX_OK;
        };
        stage(0);
        if ((rc = enqueue(0)))
            return rc;
        for (uint64_t c = 0; c < chunks; ++c)
        {
            if (c + 1 < chunks) // into the other lane while the device decodes chunk c (that lane's last uploads, chunk c - 1's, are done)
                stage(c + 1);
            Chunk const ck = chunk(c);
            // the output straight into the result (the single stream orders it before the next chunk's kernel)
            if (ck.out_n)
                LX_HIP(h, hipMemcpyAsync(dst0 + (ck.out_lo - run[0].out_off), G.d_out.ptr, ck.out_n, hipMemcpyDeviceToHost, s));
            hipEvent_t const done = pool_event(h);
            if (!done)
                return fail(h, LX_EHIP, "lx_gunzip: no event");
            LX_HIP(h, hipEventRecord(done, s));
            if (c + 1 < chunks && (rc = enqueue(c + 1)))
                return rc;
            LX_HIP(h, hipEventSynchronize(done));
            if ((rc = check(c)))
                return rc;
        }
        res.size += total;
        h->gunzip.stats.bgzf_members += nm;
        return LX_OK;
    }

    int run()
    {
        std::vector<lx::GunzipMember> bg; // the current run of BGZF members
        std::vector<uint64_t>         starts;
        uint64_t                      k = 0, k0 = 0, out_at = 0;
        auto flush = [&]() -> int
        {
            if (!bg.empty())
                starts.push_back(bg.back().in_off + bg.back().in_len + 8); // (the end of the run's last member)
            int const rc = device_run(bg, starts, k0);
            bg.clear();
            starts.clear();
            return rc;
        };
        for (uint64_t at = 0; at < n; ++k)
        {
            Header             hd;
            char const * const bad = parse_header(in, n, at, hd);
            if (bad)
                return error(k, at, bad);
            if (hd.bsize >= 0 && (uint64_t)hd.bsize + 1 > n - at)
                return error(k, at, "BSIZE points past the end of the data");
            if (h && hd.bsize >= 0)
            {
                uint64_t const end = at + (uint64_t)hd.bsize + 1;
                if (end < hd.end + 8)
                    return error(k, at, "BSIZE is smaller than the member's header and trailer");
                uint64_t const len = end - 8 - hd.end;
                uint32_t const isize = le32(in + end - 4);
                if (len <= lx::kGunzipMaxPayload && isize <= lx::kGunzipMaxIsize)
                {
                    if (bg.empty())
                    {
                        k0     = k;
                        out_at = res.size;
                    }
                    lx::GunzipMember m{};
                    m.in_off  = hd.end;
                    m.in_len  = (uint32_t)len;
                    m.out_off = out_at;
                    m.isize   = isize;
                    m.crc     = le32(in + end - 8);
                    out_at += isize;
                    bg.push_back(m);
                    starts.push_back(at);
                    at = end;
                    continue;
                }
            }
            int rc = flush();
            if (rc)
                return rc;
            uint64_t next = 0;
            uint64_t const from = h ? (h->opt_gunzip_from ? h->opt_gunzip_from : kPlainFrom) : 0;
            if (h && from != UINT64_MAX && n - hd.end >= from)
            {
                // (what follows the header may be many small members: one whose stream ends inside kPlainProbe bytes, or before `from`
                // bytes with its trailer, is the host's.  The probe is what a large member pays: 64 KiB of host decoding, ~0.4 ms)
                bool small = false;
                if (from > 9 && (rc = host_member(k, at, hd, &next, std::min(from - 9, kPlainProbe), &small)))
                    return rc;
                if (small)
                {
                    ++h->gunzip.stats.plain_host;
                    at = next;
                    continue;
                }
                int why = 0;
                if ((rc = parallel_member(at, hd, &next, &why)))
                    return rc;
                if (!why)
                {
                    ++h->gunzip.stats.plain_parallel;
                    at = next;
                    continue;
                }
                ++h->gunzip.stats.declined;
                h->gunzip.stats.last_decline = why;
            }
            if ((rc = host_member(k, at, hd, &next)))
                return rc;
            if (h)
                ++h->gunzip.stats.plain_host;
            at = next;
        }
        return flush();
    }
};

// ---- lx_gunzip_stream: the same walk, piece by piece
//
// The text not handed out yet: buf[keep, keep + fill), behind the last `keep` (<= 32 KiB) bytes of what was handed out -- the window
// a plain member's back-references still reach.
struct StreamBuf
{
    std::string buf;
    uint64_t    keep = 0, fill = 0;
    uint8_t *   room(uint64_t need) // room for `need` more bytes behind the text
    {
        uint64_t const at = keep + fill;
        if (at + need > buf.size())
            buf.resize(std::max<uint64_t>(at + need, std::max<uint64_t>(2 * buf.size(), 1u << 16)));
        return reinterpret_cast<uint8_t *>(&buf[0]) + at;
    }
    // the text leaves; its last 32 KiB stay in front of what comes next
    std::string take()
    {
        std::string    piece(buf.data() + keep, fill);
        uint64_t const all = keep + fill, w = std::min<uint64_t>(all, 32768);
        std::memmove(&buf[0], buf.data() + (all - w), w);
        keep = w;
        fill = 0;
        return piece;
    }
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

} // namespace

struct lx_gunzip_stream
{
    lx_handle *     h = nullptr;
    uint8_t const * in = nullptr;
    uint64_t        n = 0;
    void *          map = nullptr; // the file, mapped; or, where it cannot be mapped (a pipe), read into `held`
    std::string     held;
    uint64_t        piece = 0;
    bool            gz = false, failed = false;
    uint64_t        at = 0, k = 0; // the next member: its first byte, its number
    uint64_t        released = 0;  // pages of the mapping in front of this byte were given back
    StreamBuf       sb;
    // the plain member being decoded
    lx::inflate::Tables           T;
    StreamSink                    sink{sb};
    std::unique_ptr<StepInflater> inf;
    Header                        hd;
    uint64_t                      crc_from = 0; // sb.buf[crc_from, keep + fill) is the member's text not in `crc` yet
    uint32_t                      crc = 0;

    ~lx_gunzip_stream()
    {
        if (map)
            munmap(map, n);
    }
    int say(int code, char const * text)
    {
        failed = true;
        if (h)
            return fail(h, code, "%s", text);
        set_output_error(text);
        return code;
    }
    int error(char const * why) { return member_error(h, k, at, why); }
    void crc_up()
    {
        uint64_t const end = sb.keep + sb.fill;
        crc      = crc32(reinterpret_cast<uint8_t const *>(sb.buf.data()) + crc_from, end - crc_from, crc);
        crc_from = end;
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
    int emit(lx_bytes ** out)
    {
        if (inf)
            crc_up();
        *out = bytes_adopt(sb.take());
        crc_from = sb.keep;
        release(inf ? hd.end + inf->pos - std::min<uint64_t>(inf->pos, 8) : at);
        return LX_OK;
    }
    // true: the member at `at` goes into a group for the BGZF path (`end` = the byte after it, `isize` its text)
    bool bgzf_member(Header const & hd_, uint64_t a, uint64_t * end, uint32_t * isize) const
    {
        if (hd_.bsize < 0 || (uint64_t)hd_.bsize + 1 > n - a)
            return false;
        uint64_t const e = a + (uint64_t)hd_.bsize + 1;
        if (e < hd_.end + 8 || e - 8 - hd_.end > lx::kGunzipMaxPayload || le32(in + e - 4) > lx::kGunzipMaxIsize)
            return false;
        *end   = e;
        *isize = le32(in + e - 4);
        return true;
    }
    int next(lx_bytes ** out)
    {
        if (!gz) // the file's own bytes
        {
            uint64_t const len = std::min(piece, n - at);
            if (len)
                *out = bytes_adopt(std::string(reinterpret_cast<char const *>(in) + at, len));
            at += len;
            release(at);
            return LX_OK;
        }
        for (;;)
        {
            if (sb.fill >= piece)
                return emit(out);
            if (inf)
            {
                uint32_t const st = inf->step(piece);
                if (st != lx::inflate::kOk)
                    return failed = true, error(lx::inflate::status_text(st));
                if (!inf->done)
                    continue; // (the limit: the piece leaves at the loop's head)
                uint64_t const t = hd.end + inf->consumed();
                crc_up();
                char const * bad = n - t < 8                                                ? "truncated gzip trailer"
                                   : crc != le32(in + t)                                    ? "CRC32 mismatch"
                                   : (uint32_t)sink.member != le32(in + t + 4)              ? "ISIZE mismatch"
                                   : hd.bsize >= 0 && t + 8 != at + (uint64_t)hd.bsize + 1 ? "BSIZE does not match the member's DEFLATE stream"
                                                                                            : nullptr;
                if (bad)
                    return failed = true, error(bad);
                inf.reset();
                if (h)
                    ++h->gunzip.stats.plain_host;
                at = t + 8;
                ++k;
                continue;
            }
            if (at >= n)
                return sb.fill ? emit(out) : LX_OK;
            hd = Header{};
            if (char const * bad = parse_header(in, n, at, hd))
                return failed = true, error(bad);
            if (hd.bsize >= 0 && (uint64_t)hd.bsize + 1 > n - at)
                return failed = true, error("BSIZE points past the end of the data");
            uint64_t end   = 0;
            uint32_t isize = 0;
            if (bgzf_member(hd, at, &end, &isize))
            {
                // whole members until the piece is full, through the walk of lx_gunzip: on h's device, or one by one on this thread
                uint64_t sum = isize, members = 1;
                for (Header g; sb.fill + sum < piece && end < n; ++members)
                {
                    g = Header{};
                    uint64_t e2 = 0;
                    if (parse_header(in, n, end, g) || !bgzf_member(g, end, &e2, &isize))
                        break;
                    sum += isize;
                    end = e2;
                }
                if (h)
                {
                    h->phase_ev.clear();
                    h->ev_pool_used = 0;
                }
                Result    r;
                int const rc = Walk{h, in + at, end - at, r, k, at}.run();
                if (rc)
                    return failed = true, rc;
                if (sb.fill == 0 && r.size >= piece) // (nothing waits in front of it: the group's text is the piece)
                {
                    r.out.resize(r.size);
                    *out    = bytes_adopt(std::move(r.out));
                    sb.keep = 0;
                }
                else
                {
                    std::memcpy(sb.room(r.size), r.out.data(), r.size);
                    sb.fill += r.size;
                }
                at = end;
                k += members;
                release(at);
                if (*out)
                    return LX_OK;
                continue;
            }
            if (h && hd.bsize >= 0 && at + (uint64_t)hd.bsize + 1 < hd.end + 8)
                return failed = true, error("BSIZE is smaller than the member's header and trailer");
            sink.member = 0;
            crc         = 0;
            crc_from    = sb.keep + sb.fill;
            inf.reset(new StepInflater(in + hd.end, n - hd.end, sink, T));
        }
    }
};

extern "C" {

int lx_gunzip_stream_open(lx_handle * h, char const * path, uint64_t piece_bytes, lx_gunzip_stream ** out)
{
    auto refuse = [&](std::string const & text)
    {
        if (h)
            return fail(h, LX_EINVAL, "%s", text.c_str());
        set_output_error(text);
        return (int)LX_EINVAL;
    };
    if (!h)
        set_output_error("");
    if (!path || !out)
        return refuse("lx_gunzip_stream_open: NULL argument");
    *out = nullptr;
    int const fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0)
        return refuse(std::string("lx_gunzip_stream_open: cannot open ") + path);
    try
    {
        std::unique_ptr<lx_gunzip_stream> s(new lx_gunzip_stream);
        s->h     = h;
        s->piece = piece_bytes ? piece_bytes : 64ull << 20;
        struct stat st;
        void *      m = MAP_FAILED;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0)
            m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED)
        {
            s->map = m;
            s->n   = (uint64_t)st.st_size;
            s->in  = static_cast<uint8_t const *>(m);
            madvise(m, s->n, MADV_SEQUENTIAL);
        }
        else // (an empty file, a pipe: read to its end; its bytes are held whole, compressed)
        {
            char    buf[1 << 16];
            ssize_t got;
            while ((got = ::read(fd, buf, sizeof(buf))) > 0)
                s->held.append(buf, (size_t)got);
            if (got < 0)
            {
                ::close(fd);
                return refuse(std::string("lx_gunzip_stream_open: error while reading ") + path);
            }
            s->n  = s->held.size();
            s->in = reinterpret_cast<uint8_t const *>(s->held.data());
        }
        ::close(fd);
        s->gz = s->n >= 2 && s->in[0] == 0x1f && s->in[1] == 0x8b;
        if (h)
        {
            h->gunzip.stats = lx_gunzip_stats{};
            for (int i = 0; i < 3; ++i)
                h->gunzip.phase_ms[i] = 0.f, h->gunzip.phase_launches[i] = 0;
        }
        *out = s.release();
        return LX_OK;
    }
    catch (std::bad_alloc const &)
    {
        ::close(fd);
        if (h)
            return fail(h, LX_ENOMEM, "lx_gunzip_stream_open: out of host memory");
        set_output_error("lx_gunzip_stream_open: out of host memory");
        return LX_ENOMEM;
    }
}

int lx_gunzip_stream_next(lx_gunzip_stream * s, lx_bytes ** piece)
{
    if (!s || !piece)
    {
        set_output_error("lx_gunzip_stream_next: NULL argument");
        return s && s->h ? fail(s->h, LX_EINVAL, "lx_gunzip_stream_next: NULL argument") : (int)LX_EINVAL;
    }
    *piece = nullptr;
    if (!s->h)
        set_output_error("");
    if (s->failed)
        return s->say(LX_EINVAL, "lx_gunzip_stream_next: the stream has failed");
    try
    {
        return s->next(piece);
    }
    catch (std::bad_alloc const &)
    {
        return s->say(LX_ENOMEM, "lx_gunzip_stream_next: out of host memory");
    }
}

void lx_gunzip_stream_close(lx_gunzip_stream * s)
{
    delete s;
}

int lx_gunzip(lx_handle * h, uint8_t const * in, uint64_t n, lx_bytes ** out)
{
    if (!h)
        set_output_error("");
    if (!out || (!in && n))
    {
        if (h)
            return fail(h, LX_EINVAL, "lx_gunzip: NULL buffer");
        set_output_error("lx_gunzip: NULL buffer");
        return LX_EINVAL;
    }
    *out = nullptr;
    if (h)
    {
        h->phase_ev.clear();
        h->ev_pool_used = 0;
        h->gunzip.stats = lx_gunzip_stats{};
        for (int i = 0; i < 3; ++i)
            h->gunzip.phase_ms[i] = 0.f, h->gunzip.phase_launches[i] = 0;
    }
    Result r;
    int    rc = LX_OK;
    try
    {
        rc = Walk{h, in, n, r}.run();
        if (rc == LX_OK)
        {
            r.out.resize(r.size);
            *out = bytes_adopt(std::move(r.out));
        }
    }
    catch (std::bad_alloc const &)
    {
        if (h)
            return fail(h, LX_ENOMEM, "lx_gunzip: out of host memory");
        set_output_error("lx_gunzip: out of host memory");
        return LX_ENOMEM;
    }
    return rc;
}

int lx_last_gunzip_stats(lx_handle const * h, lx_gunzip_stats * stats)
{
    if (!h || !stats)
        return LX_EINVAL;
    *stats = h->gunzip.stats;
    return LX_OK;
}

char const * lx_gunzip_decline_text(int reason)
{
    switch (reason)
    {
    case LX_GUNZIP_DECLINE_NONE: return "none";
    case LX_GUNZIP_DECLINE_NO_BOUNDARY: return "no boundary";
    case LX_GUNZIP_DECLINE_ROOM: return "room";
    case LX_GUNZIP_DECLINE_STATUS: return "decode status";
    case LX_GUNZIP_DECLINE_CHAIN: return "chain";
    case LX_GUNZIP_DECLINE_TRAILER: return "trailer";
    case LX_GUNZIP_DECLINE_CRC: return "CRC32";
    case LX_GUNZIP_DECLINE_ISIZE: return "ISIZE";
    default: return "?";
    }
}

} // extern "C"
