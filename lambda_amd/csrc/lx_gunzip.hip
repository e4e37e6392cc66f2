// lx_gunzip.hip -- BGZF decoder on the device (gfx950 only): one workgroup per member, members found by the host (lx_gunzip_host.cpp).
//
// A BGZF member's place in the input (BSIZE) and in the output (the prefix sum of the ISIZEs) are known before anything is
// decoded, so every workgroup writes its bytes straight to their final place.  Per member:
//   1. the member's DEFLATE bytes (<= 64 KiB) go to LDS, all lanes, and the CRC byte table beside them;
//   2. one lane decodes (lx_inflate.h, the host decoder's own code) into a 64 KiB output buffer in LDS: the symbol decode is
//      serial, and so are the back-reference copies, which are a few bytes each on sequence text;
//   3. all lanes: the CRC32 of the output by per-lane slices combined with x^(8 k) mod P (lx_crc32.h), the output to global memory.
// Bounds: the DEFLATE reads are inside the staged bytes (Inflater checks every read against the member's length) and the writes
// inside ISIZE (LdsSink); the staging and the final copy are inside the member's ranges, which the kernel checks against the
// chunk's sizes before it touches them.  A member that does not decode sets its status word and writes no output; one whose CRC
// differs has written its ISIZE bytes, inside its own range, and its status says so.
#include <hip/hip_runtime.h>

#include "lx_crc32.h"
#include "lx_gunzip.h"
#include "lx_inflate.h"

namespace lx
{
namespace gunzip
{

constexpr uint32_t kThreads  = 256;
constexpr uint32_t kOutLds   = kGunzipMaxIsize;
constexpr uint32_t kInLds    = kGunzipMaxPayload;
constexpr uint32_t kLdsBytes = kOutLds + kInLds + sizeof(inflate::Tables) + 256 * 4;

static_assert(kLdsBytes <= 160 * 1024 - 64, "the decoder's LDS exceeds what gfx950 gives a workgroup");
static_assert(sizeof(inflate::Tables) % 4 == 0, "the CRC table must be aligned");

__global__ __launch_bounds__(kThreads) void member_kernel(GunzipParams p)
{
    extern __shared__ __align__(16) uint8_t lds[];
    uint8_t * const         out = lds;
    uint8_t * const         in  = lds + kOutLds;
    inflate::Tables &       T   = *reinterpret_cast<inflate::Tables *>(lds + kOutLds + kInLds);
    uint32_t * const        tab = reinterpret_cast<uint32_t *>(lds + kOutLds + kInLds + sizeof(inflate::Tables));
    __shared__ uint32_t     s_status, s_crc;
    uint32_t const          tid = threadIdx.x, b = blockIdx.x;
    GunzipMember const      m   = p.mem[b];

    if (m.in_len > kInLds || m.isize > kOutLds || m.in_off > p.n_in || m.in_len > p.n_in - m.in_off || m.out_off > p.n_out ||
        m.isize > p.n_out - m.out_off)
    {
        if (tid == 0)
            p.status[b] = kGunzipBounds;
        return; // (uniform: every lane read the same member)
    }

    // ---- 1. the DEFLATE bytes and the CRC table into LDS
    {
        uint8_t const * src = p.in + m.in_off;
        for (uint32_t i = tid; i < m.in_len; i += kThreads)
            in[i] = src[i];
        tab[tid] = crc_table_entry(tid);
        if (tid == 0)
            s_crc = 0;
    }
    __syncthreads();

    // ---- 2. one lane decodes
    if (tid == 0)
    {
        LdsSink                    sink{out, 0, m.isize};
        inflate::Inflater<LdsSink> inf(in, m.in_len, sink, T);
        uint32_t                   st = inf.run();
        if (st == inflate::kOk && inf.consumed() != m.in_len)
            st = kGunzipTrailing;
        if (st == inflate::kOk && sink.pos != m.isize)
            st = kGunzipIsize;
        s_status = st;
    }
    __syncthreads();
    if (s_status != inflate::kOk)
    {
        if (tid == 0)
            p.status[b] = s_status;
        return;
    }

    // ---- 3. CRC32 by slices, the output to its place
    uint32_t const n = m.isize;
    {
        uint32_t const L = (n + kThreads - 1) / kThreads, a = min(n, tid * L), e = min(n, a + L);
        uint32_t       r = 0;
        for (uint32_t i = a; i < e; ++i)
            r = (r >> 8) ^ tab[(r ^ out[i]) & 0xff];
        uint32_t part = e > a ? mul_mod_p(x_pow_8n(n - e), r) : 0u;
        if (tid == 0)
            part ^= mul_mod_p(x_pow_8n(n), 0xffffffffu); // the initial register, carried over the whole member
        atomicXor(&s_crc, part);
    }
    uint8_t * const dst = p.out + m.out_off;
    if ((m.out_off & 3) == 0)
    {
        for (uint32_t i = tid; i < n / 4; i += kThreads)
            reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<uint32_t const *>(out)[i];
        for (uint32_t i = n / 4 * 4 + tid; i < n; i += kThreads)
            dst[i] = out[i];
    }
    else
        for (uint32_t i = tid; i < n; i += kThreads)
            dst[i] = out[i];
    __syncthreads();
    if (tid == 0)
        p.status[b] = (s_crc ^ 0xffffffffu) == m.crc ? 0u : kGunzipCrc;
}

} // namespace gunzip

hipError_t launch_gunzip(GunzipParams const & p, hipStream_t stream)
{
    if (p.nmem == 0)
        return hipSuccess;
    // (beyond 64 KB of LDS on request; set on the current device)
    hipError_t const attr = hipFuncSetAttribute(reinterpret_cast<void const *>(&gunzip::member_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)gunzip::kLdsBytes);
    if (attr != hipSuccess)
        return attr;
    hipLaunchKernelGGL(gunzip::member_kernel, dim3(p.nmem), dim3(gunzip::kThreads), gunzip::kLdsBytes, stream, p);
    return hipGetLastError();
}

} // namespace lx
