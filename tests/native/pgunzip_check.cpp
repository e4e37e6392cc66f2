// pgunzip_check.cpp -- the parallel decode of a plain gzip member (lambda_amd/csrc/lx_pgunzip.h) on the CPU, chunk by chunk in a
// loop where the device runs a wave of workgroups: find, decode with markers, chain, window pass, byte pass, CRC by combination.
// tests/test_pgunzip_cases.py builds it with -fsanitize=address,undefined and compares what it prints with zlib.
//
// Every buffer is a heap block of its exact size: a wave's input, a chunk's symbol room (its own block, so a symbol past the room
// is a finding), the ring, every window, a wave's bytes.
//
// Corpus: "LXPG", u32 records, then per record u32 chunk, u32 wave, u32 n, n bytes (a DEFLATE stream and whatever follows it).
// Output per record: index, decline reason (0 = decoded; the LX_GUNZIP_DECLINE_* numbers), bytes of input up to the end of the
// final block, bytes of output, their CRC32 (hex), verified chunks, dropped chunks, waves, markers resolved.  The bytes of every
// decoded record go to the file named second, one record after the other.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "lx_pgunzip.h"

namespace pg = lx::pgunzip;

namespace
{

struct Outcome
{
    int      reason = 0;
    uint64_t consumed = 0, out_len = 0, chunks = 0, dropped = 0, waves = 0, markers = 0;
    uint32_t crc = 0;
};

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

Outcome member(uint8_t const * d, uint64_t dlen, uint64_t C, uint32_t W, std::vector<uint8_t> & out)
{
    Outcome  o;
    uint32_t const room = (uint32_t)(pg::kRoomPerByte * C);
    uint64_t start_bit = 0;
    uint32_t raw = 0;
    std::unique_ptr<uint8_t[]> win(new uint8_t[pg::kWindow]()); // the window in front of the next chunk
    for (bool first = true;; first = false)
    {
        uint64_t const base = start_bit >> 3, remain = dlen - base;
        if (remain == 0)
            return o.reason = 3, o;
        uint32_t const nslots = (uint32_t)std::min<uint64_t>(W, (remain + C - 1) / C);
        uint64_t const wave_n = std::min<uint64_t>(remain, (uint64_t)(nslots + 1) * C);
        std::unique_ptr<uint8_t[]> in(new uint8_t[wave_n]);
        std::memcpy(in.get(), d + base, wave_n);
        uint32_t const n = (uint32_t)wave_n;
        std::unique_ptr<lx::inflate::Tables> T(new lx::inflate::Tables);
        // ---- find
        std::vector<uint64_t> found(nslots, pg::kNone);
        found[0] = start_bit - 8 * base;
        for (uint32_t j = 1; j < nslots; ++j)
            found[j] = pg::find_block<uint32_t>(in.get(), n, 8ull * j * C, std::min<uint64_t>(8ull * (j + 1) * C, 8ull * n), *T);
        // ---- decode
        uint64_t const stop_bit = 8 * std::min<uint64_t>(wave_n, (uint64_t)nslots * C);
        std::vector<pg::ChunkResult>             res(nslots, pg::ChunkResult{0, 0, 0, pg::kChunkSkipped, 0});
        std::vector<std::unique_ptr<uint16_t[]>> sym(nslots);
        for (uint32_t j = 0; j < nslots; ++j)
        {
            pg::ChunkPlan const pl = pg::plan_chunk(found.data(), nslots, j, room, stop_bit);
            if (pl.status)
            {
                res[j].status = pl.status;
                continue;
            }
            sym[j].reset(new uint16_t[pl.cap]);
            std::unique_ptr<uint16_t[]> ring(new uint16_t[pg::kWindow]);
            pg::MarkerSink              sink{ring.get(), sym[j].get(), 0, pl.cap, j == 0 && first ? 0u : pg::kWindow};
            res[j] = pg::decode_chunk<uint32_t>(in.get(), n, pl.b0, pl.b1, sink, *T);
        }
        ++o.waves;
        // ---- chain
        std::vector<uint32_t> ver(nslots);
        pg::Chain const       c = pg::chain(found.data(), res.data(), nslots, ver.data());
        if (c.nver == 0)
            return o.reason = res[0].status == pg::kChunkNoBoundary ? 1 : res[0].status == lx::inflate::kOutputFull ? 2 : 3, o;
        o.chunks += c.nver;
        o.dropped += c.dropped;
        if (pg::chain_gives_up(o.dropped, o.chunks))
            return o.reason = 4, o;
        // ---- resolve: windows in order, then every symbol through its chunk's window
        uint64_t wave_len = 0;
        for (uint32_t v = 0; v < c.nver; ++v)
            wave_len += res[ver[v]].count;
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[wave_len]);
        uint64_t at  = 0;
        bool     bad = false;
        for (uint32_t v = 0; v < c.nver; ++v)
        {
            uint32_t const   cnt   = res[ver[v]].count;
            uint16_t const * s     = sym[ver[v]].get();
            uint32_t const   valid = (uint32_t)std::min<uint64_t>(pg::kWindow, o.out_len + at);
            for (uint32_t i = 0; i < cnt; ++i)
            {
                o.markers += (s[i] & pg::kMarker) != 0;
                bytes[at + i] = pg::resolve(s[i], win.get(), valid, bad);
            }
            std::unique_ptr<uint8_t[]> nxt(new uint8_t[pg::kWindow]);
            for (uint32_t i = 0; i < pg::kWindow; ++i)
                nxt[i] = pg::next_window_at(i, s, cnt, win.get(), valid, bad);
            win = std::move(nxt);
            at += cnt;
        }
        if (bad)
            return o.reason = 3, o;
        raw = lx::mul_mod_p(pg::x_pow_8n64(wave_len), raw) ^ crc_raw(bytes.get(), wave_len);
        o.out_len += wave_len;
        out.insert(out.end(), bytes.get(), bytes.get() + wave_len);
        if (c.final)
        {
            o.consumed = base + (c.end_bit + 7) / 8;
            o.crc      = raw ^ lx::mul_mod_p(pg::x_pow_8n64(o.out_len), 0xffffffffu) ^ 0xffffffffu;
            return o;
        }
        start_bit = 8 * base + c.end_bit;
    }
}

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
    if (fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "LXPG", 4) || fread(&nrec, 4, 1, f) != 1)
        return 2;
    for (uint32_t i = 0; i < nrec; ++i)
    {
        uint32_t hd[3];
        if (fread(hd, 4, 3, f) != 3)
            return 2;
        std::unique_ptr<uint8_t[]> d(new uint8_t[hd[2]]);
        if (hd[2] && fread(d.get(), 1, hd[2], f) != hd[2])
            return 2;
        std::vector<uint8_t> out;
        Outcome const        o = member(d.get(), hd[2], hd[0], hd[1], out);
        if (o.reason == 0 && !out.empty() && fwrite(out.data(), 1, out.size(), g) != out.size())
            return 2;
        printf("%u %d %llu %llu %08x %llu %llu %llu %llu\n", i, o.reason, (unsigned long long)o.consumed, (unsigned long long)o.out_len, o.crc,
               (unsigned long long)o.chunks, (unsigned long long)o.dropped, (unsigned long long)o.waves, (unsigned long long)o.markers);
    }
    fclose(f);
    fclose(g);
    return 0;
}
