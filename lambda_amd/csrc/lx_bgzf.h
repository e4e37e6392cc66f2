// lx_bgzf.h -- what the BGZF encoder (lx_bgzf.hip) and its host pipeline (lx_bgzf_host.cpp) share.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lx
{

constexpr uint32_t kBgzfBlock = 65280;  // input bytes per member at most (htslib's cut: a stored member stays below 64 KiB)
constexpr uint32_t kBgzfSlot  = 65536;  // device bytes per member before the members are placed one after another
constexpr uint32_t kBgzfMemberOverhead = 18 + 5 + 8; // header with the BC subfield, a stored block's header, CRC32 + ISIZE

// the empty member that ends a BGZF file (SAM/BAM specification 4.1.2)
constexpr uint8_t kEofMember[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct BgzfParams
{
    uint8_t const * in;    // the chunk, 16-byte aligned
    uint64_t        n;     // its bytes: (nblk - 1) * kBgzfBlock < n <= nblk * kBgzfBlock
    uint32_t        nblk;
    uint8_t *       slots; // nblk * kBgzfSlot
    uint16_t *      dist;  // nblk * kBgzfBlock: match distance per position
    uint16_t *      sym;   // nblk * kBgzfBlock: where the parse's symbols start
    uint32_t *      sizes; // nblk: member bytes
    uint8_t *       out;   // the members, one after another
    uint64_t *      total; // their bytes
};

hipError_t launch_bgzf(BgzfParams const & p, hipStream_t stream);

} // namespace lx
