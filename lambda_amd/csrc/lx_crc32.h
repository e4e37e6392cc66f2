// lx_crc32.h -- the CRC32 of gzip (reflected, polynomial 0xedb88320; x^0 = bit 31) as GF(2) algebra, for the host and the device.
// The BGZF encoder (lx_bgzf.hip) and decoder (lx_gunzip.hip) both take a block's CRC as per-lane slices combined by
// multiplication with x^(8 k) mod P (the algebra of zlib's crc32_combine); the host decoder (lx_gunzip_host.cpp) runs the byte table.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lx
{

constexpr uint32_t kCrcPoly = 0xedb88320u;

// a * b mod P
__host__ __device__ inline uint32_t mul_mod_p(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;)
    {
        if (a & m)
        {
            p ^= b;
            if ((a & (m - 1)) == 0)
                break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 n) mod P
__host__ __device__ inline uint32_t x_pow_8n(uint32_t n)
{
    uint32_t p = 1u << 31, t = 1u << 23; // t = x^8
    while (n)
    {
        if (n & 1)
            p = mul_mod_p(t, p);
        n >>= 1;
        if (n)
            t = mul_mod_p(t, t);
    }
    return p;
}

// entry i of the byte table
__host__ __device__ inline uint32_t crc_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; ++k)
        c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}

} // namespace lx
