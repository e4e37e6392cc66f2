// lx_taxmap.hip -- the accession-to-taxon join on the device (gfx950): one chunk of whole map lines per call, the host's accession
// table in device memory (lx_taxmap_host.cpp builds and uploads it, streams the chunks through two lanes and turns the pairs into
// the per-subject lists).
//
// Per chunk, on one stream:
//   1. parse: one workgroup per 4 KiB tile.  The tile goes to LDS with one 16-byte load per lane; lane l then owns the line starts
//      in its 16 bytes (a byte whose predecessor is '\n') and parses each such line with the host's code (lx_taxmap.h): field 0
//      hashed and probed, the key's bytes compared on a fingerprint hit, the taxon parsed on a match.  A line that runs past the
//      tile is read on from global memory.  The tile's pairs go to its own slots of a scratch list in line order: lane counts, a
//      workgroup scan, at most kJoinTileCap pairs per tile.  A matched line whose taxon does not parse lowers one word to its
//      offset (atomicMin: the first such line of the chunk, whatever the order the workgroups run in).
//   2. scan of the tiles' counts (lx_scan.h): where each tile's pairs begin; the last word is the chunk's count.
//   3. compact: one wavefront per tile copies its pairs to their place.  No atomics decide an order, so the list is the same on
//      every run: the pairs of the chunk in line order.
// Bounds: every read of the text is below n (the tile's staging is cut at n, a line ends at its '\n' and the chunk ends in one,
// and get() answers '\n' beyond n); the scratch writes stay inside the tile's kJoinTileCap slots (checked, the overflow flag says
// so), the compacted writes inside the chunk's total.
#include <hip/hip_runtime.h>

#include "lx_level2.h"
#include "lx_taxmap.h"

namespace lx
{
namespace
{

#include "lx_scan.h"

using taxmap::JoinParams;
using taxmap::kJoinThreads;
using taxmap::kJoinTile;
using taxmap::kJoinTileCap;
using taxmap::Pair;

static_assert(kJoinThreads == (uint32_t)kL2ScanBlock, "the tile scan uses lx_scan.h's workgroup scan");

__global__ __launch_bounds__(kJoinThreads) void join_parse_kernel(JoinParams p)
{
    __shared__ __align__(16) uint8_t tile[kJoinTile];
    __shared__ uint32_t              wave_tot[kL2ScanBlock / 64];
    __shared__ uint32_t              s_lines;
    uint32_t const                   tid = threadIdx.x;
    uint64_t const                   t0  = (uint64_t)blockIdx.x * kJoinTile;
    uint32_t const                   tn  = (uint32_t)min<uint64_t>(kJoinTile, p.n - t0);
    uint32_t const                   i0  = tid * 16;
    if (i0 + 16 <= tn)
        *reinterpret_cast<uint4 *>(tile + i0) = *reinterpret_cast<uint4 const *>(p.text + t0 + i0);
    else
        for (uint32_t k = i0; k < tn; ++k)
            tile[k] = p.text[t0 + k];
    if (tid == 0)
        s_lines = 0;
    __syncthreads();

    uint8_t const * const text = p.text;
    uint64_t const        n    = p.n;
    auto get = [&](uint64_t q) -> uint8_t
    {
        uint64_t const r = q - t0;
        return r < tn ? tile[r] : q < n ? text[q] : (uint8_t)'\n';
    };
    Pair     a{0, 0}, b{0, 0};
    uint32_t cnt = 0, lines = 0;
    for (uint32_t k = i0; k < i0 + 16 && k < tn; ++k)
    {
        uint8_t const prev = k ? tile[k - 1] : t0 ? text[t0 - 1] : (uint8_t)'\n';
        if (prev != '\n')
            continue;
        ++lines;
        uint32_t subject = 0, taxid = 0;
        uint64_t ta = 0, tl = 0;
        int const r = taxmap::parse_line(p.table, p.format, get, t0 + k, &subject, &taxid, &ta, &tl);
        if (r == taxmap::kLinePair)
        {
            if (cnt == 0)
                a = Pair{subject, taxid};
            else
                b = Pair{subject, taxid};
            ++cnt;
        }
        else if (r == taxmap::kLineBadTax)
            atomicMin(&p.counters->bad_off, (uint32_t)(t0 + k));
    }
    if (cnt > 2) // (two lines that yield a pair start at least 8 bytes apart)
    {
        p.counters->overflow = 1;
        cnt                  = 2;
    }
    if (lines)
        atomicAdd(&s_lines, lines);
    uint32_t       total;
    uint32_t const excl = block_inclusive<kOpSum>(cnt, wave_tot, total) - cnt; // (its barriers order s_lines too)
    Pair * const   dst  = p.scratch + (uint64_t)blockIdx.x * kJoinTileCap;
    if (cnt >= 1 && excl < kJoinTileCap)
        dst[excl] = a;
    if (cnt >= 2 && excl + 1 < kJoinTileCap)
        dst[excl + 1] = b;
    if (tid == 0)
    {
        if (total > kJoinTileCap)
            p.counters->overflow = 1;
        p.tile_cnt[blockIdx.x] = min(total, kJoinTileCap);
        if (s_lines)
            atomicAdd(&p.counters->lines, (unsigned long long)s_lines);
    }
}

struct TileCount
{
    uint32_t const * cnt;
    __device__ uint32_t operator()(uint64_t j) const { return cnt[j]; }
};
struct TileOffset
{
    uint32_t * off;
    __device__ void operator()(uint64_t j, uint32_t, uint32_t excl) const { off[j] = excl; }
};

// one wavefront per tile
__global__ __launch_bounds__(kJoinThreads) void join_compact_kernel(JoinParams p, uint32_t tiles)
{
    uint32_t const t    = blockIdx.x * (kJoinThreads / 64) + (threadIdx.x >> 6);
    uint32_t const lane = threadIdx.x & 63;
    if (t >= tiles)
        return;
    uint32_t const c   = p.tile_cnt[t], at = p.tile_off[t];
    Pair const *   src = p.scratch + (uint64_t)t * kJoinTileCap;
    for (uint32_t k = lane; k < c; k += 64)
        p.pairs[(uint64_t)at + k] = src[k];
}

} // namespace

namespace taxmap
{

uint64_t join_scan_blocks(uint64_t tiles)
{
    return (tiles + kL2ScanTile - 1) / kL2ScanTile;
}

hipError_t launch_taxmap_join(JoinParams const & p, hipStream_t stream)
{
    uint32_t const tiles = join_tiles(p.n);
    if (tiles == 0)
        return hipSuccess;
    uint64_t const sb = join_scan_blocks(tiles);
    hipLaunchKernelGGL(join_parse_kernel, dim3(tiles), dim3(kJoinThreads), 0, stream, p);
    TileCount const  tv{p.tile_cnt};
    TileOffset const to{p.tile_off};
    hipLaunchKernelGGL((l2_scan_reduce_kernel<kOpSum, false, TileCount>), dim3((uint32_t)sb), dim3(kL2ScanBlock), 0, stream, tv, (uint64_t)tiles,
                       p.block_tot);
    hipLaunchKernelGGL((l2_scan_tops_kernel<kOpSum>), dim3(1), dim3(kL2ScanBlock), 0, stream, p.block_tot, sb);
    hipLaunchKernelGGL((l2_scan_apply_kernel<kOpSum, false, TileCount, TileOffset>), dim3((uint32_t)sb), dim3(kL2ScanBlock), 0, stream, tv, to,
                       (uint64_t)tiles, p.block_tot);
    uint32_t const per = kJoinThreads / 64;
    hipLaunchKernelGGL(join_compact_kernel, dim3((tiles + per - 1) / per), dim3(kJoinThreads), 0, stream, p, tiles);
    return hipGetLastError();
}

} // namespace taxmap
} // namespace lx
