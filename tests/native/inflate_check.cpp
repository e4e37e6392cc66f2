// inflate_check.cpp -- the BGZF kernel's decoder under the sanitizers, without a device and without Python: the kernel's own
// instantiation, lx::inflate::Inflater<lx::LdsSink, uint32_t> (lx_inflate.h, lx_gunzip.h), on a corpus file.  Each input lies in a
// heap block of exactly its length and each output in a heap block of exactly the sink's capacity (the member's ISIZE), so a read
// or a write one byte outside what the kernel stages in LDS is an AddressSanitizer report.  Built and run by
// tests/test_inflate_cases.py (no GPU needed, never on one):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I<rocm>/include
//       -Ilambda_amd/csrc tests/native/inflate_check.cpp -o inflate_check && ./inflate_check corpus.bin > results.txt
// The corpus: "LXIC", u32 records, then per record u32 input bytes, u32 capacity, the input.  Per record one line:
//   index status consumed written crc32-of-the-output
// with the kernel's two checks after run() folded into the status as the kernel does (102: the stream ended before the end of the
// input, 101: fewer bytes than the capacity).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lx_gunzip.h"
#include "lx_inflate.h"

static bool read_u32(FILE * f, uint32_t & v)
{
    uint8_t b[4];
    if (std::fread(b, 1, 4, f) != 4)
        return false;
    v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    return true;
}

int main(int argc, char ** argv)
{
    if (argc != 2)
    {
        std::fprintf(stderr, "usage: inflate_check corpus.bin\n");
        return 2;
    }
    FILE * f = std::fopen(argv[1], "rb");
    char   magic[4];
    uint32_t records = 0;
    if (!f || std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "LXIC", 4) != 0 || !read_u32(f, records))
    {
        std::fprintf(stderr, "inflate_check: cannot read the corpus %s\n", argv[1]);
        return 2;
    }
    auto T = std::make_unique<lx::inflate::Tables>();
    for (uint32_t r = 0; r < records; ++r)
    {
        uint32_t n = 0, cap = 0;
        if (!read_u32(f, n) || !read_u32(f, cap) || n > lx::kGunzipMaxPayload || cap > lx::kGunzipMaxIsize)
        {
            std::fprintf(stderr, "inflate_check: record %u is malformed\n", r);
            return 2;
        }
        // (new[] of 0 bytes is a block of its own: an access to it is reported too)
        std::unique_ptr<uint8_t[]> in(new uint8_t[n]), out(new uint8_t[cap]);
        if (n && std::fread(in.get(), 1, n, f) != n)
        {
            std::fprintf(stderr, "inflate_check: record %u is cut short\n", r);
            return 2;
        }
        std::memset(T.get(), 0xa5, sizeof(*T)); // nothing may depend on what the member before left in the tables
        lx::LdsSink                             sink{out.get(), 0, cap};
        lx::inflate::Inflater<lx::LdsSink, uint32_t> inf(in.get(), n, sink, *T);
        uint32_t                                st = inf.run();
        uint32_t const                          used = st == lx::inflate::kOk ? inf.consumed() : 0;
        if (st == lx::inflate::kOk && used != n)
            st = lx::kGunzipTrailing;
        if (st == lx::inflate::kOk && sink.pos != cap)
            st = lx::kGunzipIsize;
        if (sink.pos > cap)
        {
            std::fprintf(stderr, "inflate_check: record %u: the sink holds %u bytes of %u\n", r, sink.pos, cap);
            return 1;
        }
        uint32_t crc = 0xffffffffu; // CRC-32 as in zlib, bit by bit
        for (uint32_t i = 0; i < sink.pos; ++i)
        {
            crc ^= out[i];
            for (int k = 0; k < 8; ++k)
                crc = (crc >> 1) ^ (0xedb88320u & (0u - (crc & 1u)));
        }
        std::printf("%u %u %u %u %08x\n", r, st, used, sink.pos, crc ^ 0xffffffffu);
    }
    std::fclose(f);
    return 0;
}
