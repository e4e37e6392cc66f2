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
#include "lx_crc32.h"
#include "lx_gunzip.h"
#include "lx_inflate.h"
#include "lx_internal.h"
#include "lx_pgunzip.h"

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

struct Walk
{
    lx_handle *     h;
    uint8_t const * in;
    uint64_t        n;
    Result &        res;

    int error(uint64_t k, uint64_t at, char const * why)
    {
        char buf[320];
        snprintf(buf, sizeof(buf), "lx_gunzip: member %llu at byte %llu: %s", (unsigned long long)k, (unsigned long long)at, why);
        if (h)
            return fail(h, LX_EINVAL, "%s", buf);
        set_output_error(buf);
        return LX_EINVAL;
    }

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

} // namespace

extern "C" {

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
