// gunzip_stream_check.cpp -- lx_gunzip_stream's walk (lambda_amd/csrc/lx_gunzip_stream.h: pieces, the text a wave leaves over, the
// resume on the host after a decline, the trailer) on the CPU.  The stream is the library's own Stream<Env>; where the library
// runs a wave on the device (DeviceWaves in lx_gunzip_host.cpp), CpuWaves runs the same __host__ __device__ functions of
// lx_pgunzip.h in loops: find, decode with markers, chain_wave() -- what chain_kernel runs --, window pass, byte pass, CRC.
// tests/test_gunzip_stream_parallel.py builds it with -fsanitize=address,undefined and compares what it prints with zlib.
//
// Every buffer of a wave is a heap block of its exact size: the wave's input, a chunk's symbol room (its own block, so a symbol
// past the room is a finding), the ring, the tables of the chain step, every window, the wave's bytes.
//
// Every wave's found / ChunkResult tables also go through chain_ref() below, a restatement of the chain rule that shares no code
// with lx_pgunzip.h, and chain(), chain_wave() and the Verified table must say the same: "X" lines count the waves checked.
//
// Corpus: "LXGS", u32 records, then per record u32 chunk, u32 wave knob, u32 piece, u32 device (0: no device, every member on the
// host path), u64 parallel_from, u32 n, n bytes (a file).
// Output per record: "R index rc calls" and per call "C piece_len plain_parallel plain_host declined last_decline chunks dropped
// waves bgzf_members bytes_down" (piece_len -1: the call failed or was the end), then "X waves_checked mismatches", then "E text" when the
// stream failed.  The pieces go to the file named second, one after the other.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lx_gunzip_stream.h"

namespace pg = lx::pgunzip;
namespace gz = lx::gz;

namespace
{

uint32_t crc_raw(uint8_t const * p, uint64_t n) // register 0 in, no complement
{
    uint32_t r = 0;
    for (uint64_t i = 0; i < n; ++i)
    {
        r ^= p[i];
        for (int k = 0; k < 8; ++k)
            r = (r & 1) ? (r >> 1) ^ lx::kCrcPoly : r >> 1;
    }
    return r;
}

// the chain rule, stated once more: slot 0 counts when it decoded; after a counted slot that did not end the stream comes the next
// slot in which something was found, and it counts when it starts where the last one ended and decoded; the first one that does
// not count ends the chain, and it and every found slot behind it are dropped
struct RefChain
{
    std::vector<uint32_t> slots;
    uint32_t              dropped = 0, final = 0;
    uint64_t              end_bit = 0;
};
RefChain chain_ref(uint64_t const * found, pg::ChunkResult const * r, uint32_t nslots)
{
    RefChain c;
    if (nslots == 0 || r[0].status != 0)
        return c;
    std::vector<uint32_t> cand; // the slots in which something was found, behind slot 0
    for (uint32_t j = 1; j < nslots; ++j)
        if (found[j] != pg::kNone)
            cand.push_back(j);
    c.slots.push_back(0);
    size_t i = 0;
    for (; i < cand.size() && !r[c.slots.back()].final; ++i)
    {
        if (found[cand[i]] != r[c.slots.back()].end_bit || r[cand[i]].status != 0)
            break;
        c.slots.push_back(cand[i]);
    }
    if (!r[c.slots.back()].final)
        c.dropped = (uint32_t)(cand.size() - i);
    c.final   = r[c.slots.back()].final;
    c.end_bit = r[c.slots.back()].end_bit;
    return c;
}

struct CpuWaves
{
    std::unique_ptr<uint8_t[]> bytes; // of the last wave
    uint64_t                   len = 0;
    std::unique_ptr<uint8_t[]> behind; // the window behind the last wave
    uint64_t                   checked = 0, mismatches = 0;

    int run(gz::WaveJob const & j, pg::WaveResult & r)
    {
        uint32_t const             n = (uint32_t)j.n, nslots = j.nslots;
        std::unique_ptr<uint8_t[]> in(new uint8_t[j.n]);
        std::memcpy(in.get(), j.in, j.n);
        std::unique_ptr<lx::inflate::Tables> T(new lx::inflate::Tables);
        // ---- find
        std::unique_ptr<uint64_t[]> found(new uint64_t[nslots]);
        found[0] = j.found0;
        for (uint32_t s = 1; s < nslots; ++s)
            found[s] = pg::find_block<uint32_t>(in.get(), n, 8ull * s * j.chunk, std::min<uint64_t>(8ull * (s + 1) * j.chunk, 8ull * n), *T);
        // ---- decode
        std::unique_ptr<pg::ChunkResult[]>       res(new pg::ChunkResult[nslots]);
        std::vector<std::unique_ptr<uint16_t[]>> sym(nslots);
        for (uint32_t s = 0; s < nslots; ++s)
        {
            pg::ChunkPlan const pl = pg::plan_chunk(found.get(), nslots, s, j.room, j.stop_bit);
            res[s] = pg::ChunkResult{0, 0, 0, pl.status, 0};
            if (pl.status)
                continue;
            sym[s].reset(new uint16_t[pl.cap]);
            std::unique_ptr<uint16_t[]> ring(new uint16_t[pg::kWindow]);
            pg::MarkerSink              sink{ring.get(), sym[s].get(), 0, pl.cap, s == 0 && j.first ? 0u : pg::kWindow};
            res[s] = pg::decode_chunk<uint32_t>(in.get(), n, pl.b0, pl.b1, sink, *T);
        }
        // ---- chain: what chain_kernel runs, and the same tables through chain() and chain_ref()
        std::unique_ptr<uint32_t[]>     idx(new uint32_t[nslots]);
        std::unique_ptr<pg::Verified[]> ver(new pg::Verified[nslots]);
        pg::chain_wave(found.get(), res.get(), nslots, j.room, j.before, idx.get(), ver.get(), r);
        {
            std::unique_ptr<uint32_t[]> idx2(new uint32_t[nslots]);
            pg::Chain const             c   = pg::chain(found.get(), res.get(), nslots, idx2.get());
            RefChain const              ref = chain_ref(found.get(), res.get(), nslots);
            bool ok = c.nver == ref.slots.size() && r.nver == c.nver && c.dropped == ref.dropped && r.dropped == c.dropped && c.final == ref.final &&
                      r.final == c.final && (c.nver == 0 || (c.end_bit == ref.end_bit && r.end_bit == c.end_bit)) && r.status0 == res[0].status;
            uint64_t at = 0;
            for (uint32_t v = 0; ok && v < c.nver; ++v)
            {
                uint32_t const s = ref.slots[v];
                ok = idx[v] == s && idx2[v] == s && ver[v].sym_off == (uint64_t)s * j.room && ver[v].byte_off == at && ver[v].count == res[s].count &&
                     ver[v].valid == std::min<uint64_t>(pg::kWindow, j.before + at);
                at += res[s].count;
            }
            ok = ok && r.wave_len == at;
            ++checked;
            mismatches += !ok;
        }
        // ---- resolve: windows in order, then every symbol through its chunk's window
        std::unique_ptr<uint8_t[]> win(new uint8_t[pg::kWindow]());
        if (j.win)
            std::memcpy(win.get() + (pg::kWindow - j.before), j.win, j.before);
        else if (!j.first && behind)
            std::memcpy(win.get(), behind.get(), pg::kWindow);
        bytes.reset(new uint8_t[r.wave_len]);
        len = r.wave_len;
        bool bad = false;
        for (uint32_t v = 0; v < r.nver; ++v)
        {
            pg::Verified const e = ver[v];
            uint16_t const *   s = sym[e.sym_off / j.room].get();
            for (uint32_t i = 0; i < e.count; ++i)
                bytes[e.byte_off + i] = pg::resolve(s[i], win.get(), e.valid, bad);
            std::unique_ptr<uint8_t[]> nxt(new uint8_t[pg::kWindow]);
            for (uint32_t i = 0; i < pg::kWindow; ++i)
                nxt[i] = pg::next_window_at(i, s, e.count, win.get(), e.valid, bad);
            win = std::move(nxt);
        }
        r.bad |= bad;
        r.crc  = crc_raw(bytes.get(), len);
        behind = std::move(win);
        return LX_OK;
    }
    int fetch(uint8_t * dst, uint64_t n)
    {
        if (n != len)
            return LX_EINVAL;
        std::memcpy(dst, bytes.get(), n);
        return LX_OK;
    }
};

struct TestEnv
{
    bool            device = true;
    uint64_t        from = 0, chunk = 0, knob = 0;
    lx_gunzip_stats st{};
    CpuWaves        cpu;
    std::string     message;

    lx_gunzip_stats * stats() { return device ? &st : nullptr; }
    uint64_t          parallel_from() const { return from; }
    uint64_t          chunk_bytes() const { return chunk; }
    uint64_t          wave_knob() const { return knob; }
    CpuWaves &        runner() { return cpu; }
    int error(uint64_t k, uint64_t at, char const * why)
    {
        char buf[320];
        snprintf(buf, sizeof(buf), "lx_gunzip: member %llu at byte %llu: %s", (unsigned long long)k, (unsigned long long)at, why);
        message = buf;
        return LX_EINVAL;
    }
    // whole BGZF members, one after the other on this thread
    int group(uint8_t const * in, uint64_t len, uint64_t k, uint64_t at, gz::Result & r)
    {
        for (uint64_t a = 0; a < len; ++k)
        {
            gz::Header hd;
            if (char const * bad = gz::parse_header(in, len, a, hd))
                return error(k, at + a, bad);
            uint64_t next = 0;
            if (char const * bad = gz::host_member(in, len, a, hd, r, &next))
                return error(k, at + a, bad);
            a = next;
            st.bgzf_members += device;
        }
        return LX_OK;
    }
};

} // namespace

int main(int argc, char ** argv)
{
    if (argc != 3)
        return 2;
    FILE * f = fopen(argv[1], "rb");
    FILE * g = fopen(argv[2], "wb");
    if (!f || !g)
        return 2;
    char     magic[4];
    uint32_t nrec = 0;
    if (fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "LXGS", 4) || fread(&nrec, 4, 1, f) != 1)
        return 2;
    for (uint32_t i = 0; i < nrec; ++i)
    {
        uint32_t hd[4], n = 0;
        uint64_t from = 0;
        if (fread(hd, 4, 4, f) != 4 || fread(&from, 8, 1, f) != 1 || fread(&n, 4, 1, f) != 1)
            return 2;
        std::unique_ptr<uint8_t[]> d(new uint8_t[n]);
        if (n && fread(d.get(), 1, n, f) != n)
            return 2;
        TestEnv env;
        env.chunk  = hd[0];
        env.knob   = hd[1];
        env.device = hd[3] != 0;
        env.from   = from;
        gz::Stream<TestEnv> s(env);
        s.in    = d.get();
        s.n     = n;
        s.piece = hd[2];
        s.gz    = n >= 2 && d[0] == 0x1f && d[1] == 0x8b;
        std::string lines;
        int         rc = LX_OK;
        uint32_t    calls = 0;
        for (;; ++calls)
        {
            env.st = lx_gunzip_stats{};
            std::string piece;
            bool        have = false;
            rc = s.next(piece, have);
            char buf[256];
            snprintf(buf, sizeof(buf), "C %lld %llu %llu %llu %d %llu %llu %llu %llu %llu\n", rc == LX_OK && have ? (long long)piece.size() : -1ll,
                     (unsigned long long)env.st.plain_parallel, (unsigned long long)env.st.plain_host, (unsigned long long)env.st.declined,
                     (int)env.st.last_decline, (unsigned long long)env.st.chunks, (unsigned long long)env.st.chunks_dropped,
                     (unsigned long long)env.st.waves, (unsigned long long)env.st.bgzf_members, (unsigned long long)env.st.bytes_down);
            lines += buf;
            if (rc != LX_OK || !have)
                break;
            if (fwrite(piece.data(), 1, piece.size(), g) != piece.size())
                return 2;
        }
        printf("R %u %d %u\n%sX %llu %llu\n", i, rc, calls + 1, lines.c_str(), (unsigned long long)env.cpu.checked, (unsigned long long)env.cpu.mismatches);
        if (rc != LX_OK)
            printf("E %s\n", env.message.c_str());
    }
    fclose(f);
    fclose(g);
    return 0;
}
