// lx_gunzip.h -- what the BGZF decoder (lx_gunzip.hip) and its host side (lx_gunzip_host.cpp) share.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lx
{

constexpr uint32_t kGunzipMaxIsize   = 65536; // a BGZF member's output at most (BSIZE is 16 bits, so is its input)
constexpr uint32_t kGunzipMaxPayload = 65536; // its DEFLATE bytes at most

// one BGZF member of a chunk, found by the host from the headers (offsets relative to the chunk's input / output)
struct GunzipMember
{
    uint64_t in_off;  // the DEFLATE stream
    uint64_t out_off; // where its bytes go
    uint32_t in_len;  // BSIZE + 1 - header - trailer
    uint32_t isize;   // from the trailer, <= kGunzipMaxIsize
    uint32_t crc;     // from the trailer
    uint32_t pad;
};

// per-member status words: 0 = ok, else one of these (or an lx::inflate::Status below kGunzipCrc)
enum : uint32_t
{
    kGunzipCrc      = 100, // the CRC32 of the output differs from the trailer's
    kGunzipIsize    = 101, // the stream ended with fewer bytes than ISIZE
    kGunzipTrailing = 102, // the stream ended before the trailer
    kGunzipBounds   = 103, // the member's ranges lie outside the chunk (never made by the host's table)
};

struct GunzipParams
{
    uint8_t const *      in;     // the chunk's compressed bytes
    uint64_t             n_in;
    GunzipMember const * mem;
    uint32_t             nmem;
    uint8_t *            out;    // the chunk's output
    uint64_t             n_out;
    uint32_t *           status; // nmem words
};

// the member's output in the kernel's LDS, at most cap (= ISIZE) bytes: the only guard of those writes.  __host__ too, so that
// tests/native/inflate_check.cpp runs this very code on heap blocks of exactly cap bytes under the sanitizers
struct LdsSink
{
    uint8_t * o;
    uint32_t  pos, cap;
    __host__ __device__ bool put(uint8_t b)
    {
        if (pos >= cap)
            return false;
        o[pos++] = b;
        return true;
    }
    __host__ __device__ bool dist_ok(uint32_t d) const { return d <= pos; }
    __host__ __device__ bool copy(uint32_t d, uint32_t len)
    {
        if (d > pos || len > cap - pos)
            return false;
        uint8_t * dst = o + pos;
        for (uint32_t i = 0; i < len; ++i) // (overlapping: byte by byte, as the format defines it)
            dst[i] = dst[(int32_t)i - (int32_t)d];
        pos += len;
        return true;
    }
};

hipError_t launch_gunzip(GunzipParams const & p, hipStream_t stream);

} // namespace lx
