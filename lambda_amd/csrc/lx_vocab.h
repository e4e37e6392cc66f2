// lx_vocab.h -- the output vocabulary: the tabular columns and the optional SAM / BAM tags, numbered once for the host writers
// (host/lx_output.cpp, whose key and description tables are in this order) and for the record kernels (lx_bam.hip, lx_text.hip) with
// their host sides.  HIP-free; not part of the ABI.
#pragma once
#include <cstdint>

namespace lx
{

// SamBamExtraTags, src/search_output.hpp:29-76, in the order of the enum (= the order of the header line)
enum
{
    kTagBitScore /* AS */, kTagProtCigar /* OC */, kTagEditDistance /* NM */, kTagMatchCount /* IH */, kTagScore /* ar */, kTagEValue /* ae */,
    kTagPIdent /* ai */, kTagPPos /* ap */, kTagQFrame /* qf */, kTagProtSeq /* qs */, kTagSFrame /* sf */, kTagSTaxIds /* st */,
    kTagLcaId /* ls */, kTagLcaTaxId /* lt */, kNumSamTags
};

// a tag's bit in a tag mask (BamCtx::tags)
constexpr uint32_t tagBit(int tag)
{
    return 1u << tag;
}

// the tabular columns (TextCtx::cols holds these)
enum
{
    kColQSeqId, kColSSeqId, kColPIdent, kColLength, kColMismatch, kColGapOpen, kColQStart, kColQEnd, kColSStart, kColSEnd, kColEValue,
    kColBitScore, kColQLen, kColSLen, kColScore, kColNIdent, kColPositive, kColGaps, kColPPos, kColFrames, kColQFrame, kColSFrame,
    kColSTaxIds, kColLcaTaxId, kNumColumns
};

} // namespace lx
