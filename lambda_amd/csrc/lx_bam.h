// lx_bam.h -- what the BAM record kernels (lx_bam.hip) and their host side (lx_bam_host.cpp) share.  Not part of the ABI.
//
// The kernels restate samFields and bamRecord (host/lx_output.cpp) for LX_OUT_BAM: the same bytes.  Three steps
// per call: groups (a head flag per row and a sum scan: the row's group, the groups' first rows), measure (one lane per record: CIGAR
// elements, the text length of tag OC, the record's bytes; 64-bit totals per kBamTile records, which is all the host reads to cut the
// ranges), and per range an exclusive scan of the sizes (lx_scan.h, uint32: a range's stream stays below 4 GiB) and emit (one wavefront
// per record, kBamEmitBlock / 64 records per workgroup).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lambda_ext.h"
#include "lx_vocab.h" // BamCtx::tags: tagBit(kTag*)

namespace lx
{

constexpr int      kBamEmitBlock = 256;  // threads of an emit workgroup: four wavefronts = four records
constexpr uint32_t kBamEmitRecs  = kBamEmitBlock / 64;
constexpr uint64_t kBamTile      = 2048; // records per size total and per scan tile (= lx_scan.h's kL2ScanTile)

// what measure leaves per record for emit
struct BamAux
{
    uint32_t n_cigar; // elements of the CIGAR (0: "*")
    uint32_t oc_len;  // characters of tag OC's text
};

// the call's inputs on the device (NULL where the caller gave none)
struct BamCtx
{
    lx_blast_match const * rows;
    uint64_t               n;
    uint8_t const *        ops;
    uint8_t const *        q_ascii; // the queries' letters, q_ascii_bytes of them (reads beyond are answered with 'N', never made)
    uint64_t               q_ascii_bytes;
    uint64_t const *       q_ascii_off;
    uint8_t const *        q_qual; // the queries' base qualities, parallel to q_ascii, q_qual_bytes of them (NULL: none; reads beyond are
                                   // answered with '!', never made)
    uint64_t               q_qual_bytes;
    uint64_t const *       q_lens;
    uint8_t const *        qn_blob; // first words of the query ids, qn_off[q] .. qn_off[q + 1]
    uint64_t const *       qn_off;
    uint64_t const *       s_tax_off; // tag st (NULL: "*")
    uint32_t const *       s_tax_ids;
    uint64_t               tax_n_s;
    uint32_t const *       grp_lca; // per group: LcaCursor's value, and the name of tag ls (length 0xffffffff: "*")
    uint32_t const *       grp_name_off;
    uint32_t const *       grp_name_len;
    uint8_t const *        name_blob;
    uint8_t const *        codon; // 125 letters: the genetic code over DNA5 triplets (NULL: no translation, qs "*")
    uint32_t *             grp;   // per record: its group; grp_first[g]: the group's first row, grp_first[groups] = n
    uint32_t *             grp_first;
    BamAux *               aux;
    uint32_t *             size; // per record: its bytes, block_size included
    uint32_t               tags;
    int32_t                sam_seq, hard;
    int32_t                is_n, q_trans, s_trans;
};

// groups: grp / grp_first from the rows (block_tot: lx_scan.h's tile values, tiles + 1 of them)
hipError_t bam_launch_groups(BamCtx const & c, uint32_t * block_tot, hipStream_t stream);
// measure: aux, size, and tile_total[t] = bytes of records [t * kBamTile, (t + 1) * kBamTile)
hipError_t bam_launch_measure(BamCtx const & c, uint64_t * tile_total, hipStream_t stream);
// records [first, first + count) into out + their exclusive size scan (off: count words of scratch)
hipError_t bam_launch_emit(BamCtx const & c, uint64_t first, uint64_t count, uint32_t * off, uint32_t * block_tot, uint8_t * out, hipStream_t stream);

} // namespace lx
