// lx_gunzip_host.cpp -- lx_gunzip: gzip streams (RFC 1952) of one or more members; BGZF members on the device (lx_gunzip.hip),
// every other member on the calling thread with the same DEFLATE code (lx_inflate.h).
//
// The host walks the member headers.  A member with the BGZF subfield (BC, BSIZE) has its end, its trailer and so its ISIZE
// without being decoded: consecutive ones form a run, a table of (input offset, length, output offset, ISIZE, CRC), and the run
// streams through the device in chunks of kChunkMembers members.  Per chunk, on the handle's stream: its bytes and table up from a
// pinned lane, the kernel, its status words down to the pinned lane, its output down into the result itself.  The host fills the
// other pinned lane with the next chunk while the device decodes this one.  A member without BSIZE ends where its DEFLATE stream
// ends, so it is decoded here, in order, before the walk goes on; so is every member when no handle is given.
#include "lx_crc32.h"
#include "lx_gunzip.h"
#include "lx_inflate.h"
#include "lx_internal.h"

#include <string>
#include <vector>

using namespace lxi;

namespace
{

constexpr uint32_t kChunkMembers = 512; // 32 MiB of input and output at most per chunk

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

    // a member decoded here; *next = the byte after its trailer
    int host_member(uint64_t k, uint64_t at, Header const & hd, uint64_t * next)
    {
        lx::inflate::Tables                            T;
        HostSink                                   sink{res, res.size};
        lx::inflate::Inflater<HostSink, uint64_t>      inf(in + hd.end, n - hd.end, sink, T);
        uint32_t const                             st = inf.run();
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
            if ((rc = host_member(k, at, hd, &next)))
                return rc;
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

} // extern "C"
