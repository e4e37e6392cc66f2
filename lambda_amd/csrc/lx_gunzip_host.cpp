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
// bytes in waves of chunks -- find, decode with markers, chain check, resolve: one submission and one synchronisation per wave (DeviceWaves)
// -- and its bytes down into the result.  Nothing of it counts before the trailer's CRC32 and ISIZE agree; in every other case the
// member is declined, the result is where it was, and host_member decodes it from its first byte: today's bytes or today's error
// text.
//
// lx_gunzip_stream_* is the same walk over a mapped file, handing the text out in pieces (lx_gunzip_stream.h has the walk and the
// bound on what it holds): BGZF members in groups whose text fills a piece, each group a Walk of its own over its slice of the
// file (so the device path and the error texts are lx_gunzip's); a plain member that lx_gunzip would give to the device wave by
// wave through the same DeviceWaves, the window uploaded from the stream's own text, so that the handle keeps nothing of the
// stream between two calls; every other member, and the rest of one the device path declines, through StepInflater, which stops
// between two symbols when the piece is full and keeps a 32 KiB window.
#include "lx_crc32.h"
#include "lx_gunzip.h"
#include "lx_gunzip_stream.h"
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
using namespace lx::gz;

namespace
{

constexpr uint32_t kChunkMembers = 512; // 32 MiB of input and output at most per chunk

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

// a wave of a plain member on the handle's device, as one submission: the input, slot 0's bit and (from a stream) the window up;
// find, decode, chain, resolve; the WaveResult down; one stream synchronisation.  The wave's bytes stay on the device until
// fetch(), a blocking copy of the length the WaveResult gave: the second and last trip to the device of a wave.
struct DeviceWaves
{
    lx_handle * h;
    uint32_t    carry = 0; // verified chunks of the last wave: the window behind the last of them lies in front of the next wave

    int run(WaveJob const & j, lx::pgunzip::WaveResult & r)
    {
        namespace pg = lx::pgunzip;
        auto & G  = h->gunzip;
        int    rc = bind(h);
        if (rc)
            return rc;
        hipStream_t const s = h->stream;
        size_t const      slot_bytes = sizeof(uint64_t) + sizeof(pg::ChunkResult);
        uint64_t const    out_cap    = (uint64_t)j.nslots * j.room;
        if ((rc = ensure(h, G.d_pin, (size_t)j.n)) || (rc = ensure(h, G.d_slots, j.nslots * slot_bytes)) || (rc = ensure(h, G.d_sym, (size_t)out_cap * 2)) ||
            (rc = ensure(h, G.d_win, (size_t)(j.nslots + 1) * pg::kWindow)) || (rc = ensure(h, G.d_ver, j.nslots * sizeof(pg::Verified))) ||
            (rc = ensure(h, G.d_bytes, (size_t)out_cap)) || (rc = ensure(h, G.d_crc, sizeof(pg::WaveResult))) ||
            (rc = ensure_pinned(h, G.p_slots, sizeof(uint64_t), kRoom)) || (rc = ensure_pinned(h, G.p_crc, sizeof(pg::WaveResult), kExact)))
            return rc;
        auto * const d_found = static_cast<uint64_t *>(G.d_slots.ptr);
        auto * const d_res   = reinterpret_cast<pg::ChunkResult *>(d_found + j.nslots);
        auto * const win     = static_cast<uint8_t *>(G.d_win.ptr);
        auto * const d_wr    = static_cast<pg::WaveResult *>(G.d_crc.ptr);
        pg::WaveParams wp{};
        wp.in         = static_cast<uint8_t const *>(G.d_pin.ptr);
        wp.n          = (uint32_t)j.n;
        wp.chunk      = j.chunk;
        wp.nslots     = j.nslots;
        wp.room       = j.room;
        wp.first_wave = j.first;
        wp.stop_bit   = j.stop_bit;
        wp.found      = d_found;
        wp.res        = d_res;
        wp.sym        = static_cast<uint16_t *>(G.d_sym.ptr);
        pg::ChainParams cp{d_found, d_res, j.nslots, j.room, j.before, static_cast<pg::Verified *>(G.d_ver.ptr), d_wr};
        pg::ResolveParams rp{};
        rp.sym     = wp.sym;
        rp.ver     = cp.ver;
        rp.wr      = d_wr;
        rp.nslots  = j.nslots;
        rp.max_seg = (uint32_t)((std::min<uint64_t>(out_cap, (uint64_t)pg::kMaxAbsorb * j.room) + pg::kWindow - 1) / pg::kWindow);
        rp.win     = win;
        rp.out     = static_cast<uint8_t *>(G.d_bytes.ptr);
        rp.out_cap = out_cap;
        *static_cast<uint64_t *>(G.p_slots.ptr) = j.found0;
        LX_HIP(h, hipMemcpyAsync(G.d_pin.ptr, j.in, j.n, hipMemcpyHostToDevice, s));
        LX_HIP(h, hipMemcpyAsync(d_found, G.p_slots.ptr, 8, hipMemcpyHostToDevice, s));
        if (j.win && j.before) // (the window's last `before` bytes exist: chain_wave() says so to the resolve kernels)
            LX_HIP(h, hipMemcpyAsync(win + (pg::kWindow - j.before), j.win, j.before, hipMemcpyHostToDevice, s));
        else if (!j.win && !j.first && carry)
            LX_HIP(h, hipMemcpyAsync(win, win + (uint64_t)carry * pg::kWindow, pg::kWindow, hipMemcpyDeviceToDevice, s));
        // (four events per wave, read and given back at the wave's end: a member of any length keeps its phase times)
        size_t const     ev_mark = h->ev_pool_used;
        hipEvent_t const e0 = pool_event(h), e1 = pool_event(h), e2 = pool_event(h), e3 = pool_event(h);
        if (!e0 || !e1 || !e2 || !e3)
            return fail(h, LX_EHIP, "lx_gunzip: no event");
        LX_HIP(h, hipEventRecord(e0, s));
        LX_HIP(h, pg::launch_find(wp, s));
        LX_HIP(h, hipEventRecord(e1, s));
        LX_HIP(h, pg::launch_decode(wp, s));
        LX_HIP(h, hipEventRecord(e2, s));
        LX_HIP(h, pg::launch_chain(cp, s));
        LX_HIP(h, pg::launch_resolve(rp, s));
        LX_HIP(h, hipEventRecord(e3, s));
        LX_HIP(h, hipMemcpyAsync(G.p_crc.ptr, d_wr, sizeof(pg::WaveResult), hipMemcpyDeviceToHost, s));
        LX_HIP(h, hipStreamSynchronize(s));
        ++G.stats.waits;
        {
            hipEvent_t const ev[3][2] = {{e0, e1}, {e1, e2}, {e2, e3}}; // (the chain step counts with the resolve kernels)
            for (int i = 0; i < 3; ++i)
            {
                float ms = 0.f;
                LX_HIP(h, hipEventElapsedTime(&ms, ev[i][0], ev[i][1]));
                G.phase_ms[i] += ms;
                ++G.phase_launches[i];
            }
            h->ev_pool_used = ev_mark;
        }
        r     = *static_cast<pg::WaveResult const *>(G.p_crc.ptr);
        carry = r.nver;
        return LX_OK;
    }
    // the bytes of the wave run() ran last, in one blocking copy (no other work is in flight on the stream)
    int fetch(uint8_t * dst, uint64_t len)
    {
        if (len)
            LX_HIP(h, hipMemcpy(dst, h->gunzip.d_bytes.ptr, len, hipMemcpyDeviceToHost));
        return LX_OK;
    }
};

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
        char const * const why = lx::gz::host_member(in, n, at, hd, res, next, limit, small);
        return why ? error(k, at, why) : (int)LX_OK;
    }

    // a plain member through the device; *reason = 0: done, *next = the byte after its trailer; else declined (the result untouched)
    int parallel_member(uint64_t at, Header const & hd, uint64_t * next, int * reason)
    {
        lx::gz::MemberWaves mw;
        mw.d     = in + hd.end;
        mw.dlen  = n - hd.end;
        mw.chunk = h->opt_gunzip_chunk ? h->opt_gunzip_chunk : kPlainChunk;
        mw.slots = wave_slots(mw.chunk, h->gunzip_wave);
        DeviceWaves dev{h};
        // (room for the whole member at once where the input's last four bytes can be its ISIZE: a hint, never a fact)
        if (n >= 4 && le32(in + n - 4) <= 1032 * mw.dlen)
            res.reserve(le32(in + n - 4));
        while (!mw.final)
        {
            // (the window behind a wave stays on the device for the next one; no copy is in flight when the result grows)
            int const rc = mw.wave(dev, h->gunzip.stats, nullptr, [&](uint64_t len) { return res.reserve(mw.out_len + len) + mw.out_len; }, reason);
            if (rc || *reason)
                return rc;
        }
        uint64_t const t = hd.end + mw.end_byte;
        if (n - t < 8 || (hd.bsize >= 0 && t + 8 != at + (uint64_t)hd.bsize + 1))
            return *reason = LX_GUNZIP_DECLINE_TRAILER, (int)LX_OK;
        if (mw.crc() != le32(in + t))
            return *reason = LX_GUNZIP_DECLINE_CRC, (int)LX_OK;
        if ((uint32_t)mw.out_len != le32(in + t + 4))
            return *reason = LX_GUNZIP_DECLINE_ISIZE, (int)LX_OK;
        res.size += mw.out_len;
        *next = t + 8;
        return LX_OK;
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

void reset_counts(lx_handle * h)
{
    h->gunzip.stats = lx_gunzip_stats{};
    for (int i = 0; i < 3; ++i)
        h->gunzip.phase_ms[i] = 0.f, h->gunzip.phase_launches[i] = 0;
}

// what the handle is to the stream (lx_gunzip_stream.h): its options and counts, its device for the groups of BGZF members and for
// the waves of a plain member; or, with no handle, the calling thread for every member
struct HandleEnv
{
    lx_handle * h;
    DeviceWaves dev{h};

    lx_gunzip_stats * stats() { return h ? &h->gunzip.stats : nullptr; }
    uint64_t          parallel_from() const { return h->opt_gunzip_from; }
    uint64_t          chunk_bytes() const { return h->opt_gunzip_chunk; }
    uint64_t          wave_knob() const { return h->gunzip_wave; }
    DeviceWaves &     runner() { return dev; }
    int error(uint64_t k, uint64_t at, char const * why) { return member_error(h, k, at, why); }
    int group(uint8_t const * in, uint64_t len, uint64_t k, uint64_t at, Result & r)
    {
        if (h)
        {
            h->phase_ev.clear();
            h->ev_pool_used = 0;
        }
        return Walk{h, in, len, r, k, at}.run();
    }
};

} // namespace

struct lx_gunzip_stream
{
    HandleEnv                 env;
    void *                    map = nullptr; // the file, mapped; or, where it cannot be mapped (a pipe), read into `held`
    uint64_t                  map_n = 0;
    std::string               held;
    lx::gz::Stream<HandleEnv> s{env};
    lx_gunzip_stats           total{}; // the counts of every call so far: what the call that reports the end leaves on the handle

    void add_call(lx_gunzip_stats const & c)
    {
        total.bgzf_members += c.bgzf_members;
        total.plain_parallel += c.plain_parallel;
        total.plain_host += c.plain_host;
        total.chunks += c.chunks;
        total.chunks_dropped += c.chunks_dropped;
        total.waves += c.waves;
        total.declined += c.declined;
        total.bytes_up += c.bytes_up;
        total.bytes_down += c.bytes_down;
        total.waits += c.waits;
        if (c.declined)
            total.last_decline = c.last_decline;
    }

    explicit lx_gunzip_stream(lx_handle * h) : env{h} {}
    ~lx_gunzip_stream()
    {
        if (map)
            munmap(map, map_n);
    }
    int say(int code, char const * text)
    {
        s.failed = true;
        if (env.h)
            return fail(env.h, code, "%s", text);
        set_output_error(text);
        return code;
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
        std::unique_ptr<lx_gunzip_stream> st_(new lx_gunzip_stream(h));
        auto &                            s = st_->s;
        s.piece = piece_bytes ? piece_bytes : 64ull << 20;
        struct stat st;
        void *      m = MAP_FAILED;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0)
            m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED)
        {
            st_->map = s.map = m;
            st_->map_n = s.n = (uint64_t)st.st_size;
            s.in = static_cast<uint8_t const *>(m);
            madvise(m, s.n, MADV_SEQUENTIAL);
        }
        else // (an empty file, a pipe: read to its end; its bytes are held whole, compressed)
        {
            char    buf[1 << 16];
            ssize_t got;
            while ((got = ::read(fd, buf, sizeof(buf))) > 0)
                st_->held.append(buf, (size_t)got);
            if (got < 0)
            {
                ::close(fd);
                return refuse(std::string("lx_gunzip_stream_open: error while reading ") + path);
            }
            s.n  = st_->held.size();
            s.in = reinterpret_cast<uint8_t const *>(st_->held.data());
        }
        ::close(fd);
        s.gz = s.n >= 2 && s.in[0] == 0x1f && s.in[1] == 0x8b;
        if (h)
            reset_counts(h);
        *out = st_.release();
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
        return s && s->env.h ? fail(s->env.h, LX_EINVAL, "lx_gunzip_stream_next: NULL argument") : (int)LX_EINVAL;
    }
    *piece = nullptr;
    if (!s->env.h)
        set_output_error("");
    if (s->s.failed)
        return s->say(LX_EINVAL, "lx_gunzip_stream_next: the stream has failed");
    if (s->env.h) // (the counts and the plain path's kernel times are this call's)
        reset_counts(s->env.h);
    try
    {
        std::string text;
        bool        have = false;
        int const   rc   = s->s.next(text, have);
        if (s->env.h)
        {
            s->add_call(s->env.h->gunzip.stats);
            if (rc == LX_OK && !have) // (the end: a caller that took every piece finds the whole file's counts, as after lx_gunzip)
                s->env.h->gunzip.stats = s->total;
        }
        if (rc == LX_OK && have)
            *piece = bytes_adopt(std::move(text));
        return rc;
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
        reset_counts(h);
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
