// lx_text.h -- what the text record kernels (lx_text.hip) and their host side (lx_text_host.cpp) share.  Not part of the ABI.
//
// The kernels restate formatRecord and the group loop of renderTable (host/lx_output.cpp) for LX_OUT_BLAST_TAB and
// LX_OUT_BLAST_TAB_COMMENTS, and samFields / samLine for LX_OUT_SAM: the same bytes.  The steps are the BAM writer's (lx_bam.h), whose
// context, groups and size scan they use, with one in front: numbers (one lane per record: the decimal texts of its e-value, bit
// score, pident, ppos and ae by lx_numfmt.h, kept per record), measure (one lane per record: the bytes of its line, with the comment
// lines of .m9 in front of a group's first record; 64-bit totals per kBamTile records), and per range a scan of the sizes and emit
// (one wavefront per record, the line staged in LDS and stored 64 bytes an instruction).
#pragma once
#include "lx_bam.h"
#include "lx_vocab.h" // TextCtx::cols: kCol*

namespace lx
{

constexpr int      kTextEmitBlock = 256; // threads of an emit workgroup: four wavefronts = four records
constexpr uint32_t kTextEmitRecs  = kTextEmitBlock / 64;
constexpr uint32_t kTextStage     = 256; // bytes of LDS a wavefront stages its line in

// a record's number texts: "%.1e" of e_value, "%.1f" of bit_score, "%.2f" of identity, "%.2f" of ppos, "%g" of (float)e_value
enum
{
    kTextNumEValue, kTextNumBitScore, kTextNumPIdent, kTextNumPPos, kTextNumAe, kTextNums
};
struct TextNum
{
    uint8_t len[8];
    char    t[kTextNums][20]; // (the longest: "-999999999999999.99")
};

struct TextCtx
{
    BamCtx           b;      // what both writers read; b.tags: the SAM tags, or St / Lt where a column wants the taxa / the LCA
    int32_t          format; // LX_OUT_BLAST_TAB, LX_OUT_BLAST_TAB_COMMENTS or LX_OUT_SAM
    uint32_t         n_cols;
    uint8_t const *  cols;
    uint32_t         need; // bit kTextNum*: the texts the format asks for
    TextNum *        nums;
    uint32_t const * row_s;  // per record: its subject's index among the subjects the rows name
    uint64_t const * s_lens; // per named subject: its length, and its id's first word sn_blob[sn_off[s] .. sn_off[s + 1])
    uint64_t const * sn_off;
    uint8_t const *  sn_blob;
    uint64_t const * qid_off; // .m9: the whole id of query q, qid_blob[qid_off[q] .. qid_off[q + 1])
    uint8_t const *  qid_blob;
    uint8_t const *  comment; // .m9: the constant parts of the comment lines, part i = comment[comment_off[i] .. comment_off[i + 1])
    uint32_t         comment_off[4];
};

// nums of every record
hipError_t text_launch_numbers(TextCtx const & c, hipStream_t stream);
// b.aux, b.size, and tile_total[t] = bytes of records [t * kBamTile, (t + 1) * kBamTile)
hipError_t text_launch_measure(TextCtx const & c, uint64_t * tile_total, hipStream_t stream);
// records [first, first + count) into out + their exclusive size scan (off: count words of scratch)
hipError_t text_launch_emit(TextCtx const & c, uint64_t first, uint64_t count, uint32_t * off, uint32_t * block_tot, uint8_t * out, hipStream_t stream);

} // namespace lx
