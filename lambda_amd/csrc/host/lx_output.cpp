// lx_output.cpp -- the BLAST-tabular / SAM / BAM writers.
//
// Host-side C++ mirror of
//   myWriteHeader         src/search_output.hpp:305-461
//   myWriteRecord         src/search_output.hpp:463-733                  (tabular via seqan::writeRecord; SAM records)
//   blastMatchOneCigar    src/search_output.hpp:115-194                  (hard or soft clips, frame clips always hard)
//   blastMatchTwoCigar    src/search_output.hpp:197-298                  (the protein-space cigar of tag OC)
//   the output options    src/search_options.hpp:224-379, :716-816       (lx_output_options: columns, SAM tags, sequence, clipping)
// Scope: every program in the tabular formats, in SAM and in BAM (the SAM records in binary, SAM/BAM specification 4.2; compressed
// by lx_bgzf.hip); not the pairwise .m0 report (seqan's writer, absent).  The
// number formats of the tabular columns are SeqAn2's (source absent): [UPSTREAM-RECALL] pident %.2f, evalue %.1e, bitscore %.1f,
// 1-based inclusive positions.
//
// A call is resolved once (lxi::resolve_output: the options with their defaults, the program, the columns or tags, the constant
// texts of .m9) and rendered once into a Sink (renderRecords).  The device writers (lx_bam_host.cpp, lx_text_host.cpp) take the same
// resolved request and the header texts from here.  What happens to a list before it is written is in lx_postprocess.cpp.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scoring_tables.hpp"

#include "../lx_host_pool.h" // the library's host threads
#include "../lx_output_host.h"

using namespace lx; // the vocabulary: kTag*, kCol*, tagBit
using lxi::LcaCursor;
using lxi::OutputRequest;

namespace
{

std::string firstWord(char const * id)
{
    std::string s(id ? id : "");
    size_t      p = s.find_first_of(" \t");
    return p == std::string::npos ? s : s.substr(0, p);
}

// blastMatchOneCigar, src/search_output.hpp:115-194.  qLen = length of the untranslated query; a translated query
// (qTrans) is reported in nucleotide space: every run x 3 (:124), the nucleotides in front of the frame and the
// incomplete codon behind it as hard clips (:126-127), the whole element list reversed on the minus strand (:192-193).
std::string cigarOf(lx_blast_match const & m, uint8_t const * ops, uint64_t qLen, bool hardClip, bool qTrans = false)
{
    std::vector<std::pair<char, uint64_t>> el;
    uint64_t const transFac       = qTrans ? 3 : 1;
    uint64_t const leftFrameClip  = (uint64_t)std::abs((int)m.q_frame) - (m.q_frame != 0 ? 1 : 0);
    uint64_t const rightFrameClip = qTrans ? (qLen - leftFrameClip) % 3 : 0;
    uint64_t const frameLen       = qTrans ? (qLen - leftFrameClip) / 3 : qLen; // length(source(alignRow0))
    uint64_t const leftClip = m.q_start * transFac, rightClip = (frameLen - m.q_end) * transFac;
    if (hardClip)
    {
        if (leftFrameClip + leftClip > 0)
            el.emplace_back('H', leftFrameClip + leftClip);
    }
    else
    {
        // (:126 takes |qFrameShift| - 1 for every program: 0 for the frames +-1 of BLASTN, 1 for the second bisulfite
        // duplicate of a strand, frames +-2 of :778-782)
        if (leftFrameClip > 0)
            el.emplace_back('H', leftFrameClip);
        if (leftClip > 0)
            el.emplace_back('S', leftClip);
    }
    uint8_t const * o = ops + m.ops_off;
    for (uint32_t i = 0; i < m.n_ops;)
    {
        uint32_t cnt = 0;
        while (i < m.n_ops && o[i] == 'D') // gap in row0 = deletion in query
        {
            ++cnt;
            ++i;
        }
        if (cnt)
            el.emplace_back('D', cnt * transFac);
        cnt = 0;
        while (i < m.n_ops && o[i] == 'I')
        {
            ++cnt;
            ++i;
        }
        if (cnt)
            el.emplace_back('I', cnt * transFac);
        cnt = 0;
        while (i < m.n_ops && o[i] == 'M')
        {
            ++cnt;
            ++i;
        }
        if (cnt)
            el.emplace_back('M', cnt * transFac);
        if (i < m.n_ops && o[i] != 'D' && o[i] != 'I' && o[i] != 'M') // (not an op byte: the caller's offsets are wrong -- no endless loop)
            return "*";
    }
    if (hardClip)
    {
        if (rightFrameClip + rightClip > 0)
            el.emplace_back('H', rightFrameClip + rightClip);
    }
    else
    {
        if (rightClip > 0)
            el.emplace_back('S', rightClip);
        if (rightFrameClip > 0)
            el.emplace_back('H', rightFrameClip);
    }
    if (m.q_frame < 0) // every program, BLASTN's reverse-complement query frame included (src/search_output.hpp:192-193)
        std::reverse(el.begin(), el.end());
    std::string c;
    for (auto const & e : el)
        c += std::to_string(e.second) + e.first;
    return c.empty() ? "*" : c; // (no element at all: the field is "*" in SAM, as BAM's empty list reads; [UPSTREAM-RECALL] seqan's SAM writer)
}

// The protein-space cigar of tag OC: blastMatchOneCigar for a protein query (transFac 1, no frame clips: BLASTP / TBLASTN,
// src/search_output.hpp:517-521) and the protCigar half of blastMatchTwoCigar for a translated one (:197-298: clips in
// protein space, hard or soft like the DNA cigar, never reversed).
std::string protCigarOf(lx_blast_match const & m, uint8_t const * ops, uint64_t qLen, bool hardClip, bool qTrans)
{
    uint64_t const leftFrameClip = (uint64_t)std::abs((int)m.q_frame) - (m.q_frame != 0 ? 1 : 0);
    uint64_t const frameLen      = qTrans ? (qLen - leftFrameClip) / 3 : qLen;
    uint64_t const leftClip = m.q_start, rightClip = frameLen >= m.q_end ? frameLen - m.q_end : 0;
    std::string    c;
    auto           add = [&](char op, uint64_t cnt)
    {
        if (cnt)
            c += std::to_string(cnt) + op;
    };
    add(hardClip ? 'H' : 'S', leftClip);
    uint8_t const * o = ops + m.ops_off;
    for (uint32_t i = 0; i < m.n_ops;)
    {
        if (o[i] != 'D' && o[i] != 'I' && o[i] != 'M')
            return "*";
        uint32_t const i0 = i;
        while (i < m.n_ops && o[i] == o[i0])
            ++i;
        add((char)o[i0], i - i0);
    }
    add(hardClip ? 'H' : 'S', rightClip);
    return c.empty() ? "*" : c;
}

thread_local std::string g_output_error;

// SamBamExtraTags, src/search_output.hpp:29-76: keys and descriptions in the order of lx_vocab.h's kTag*
struct SamTag
{
    char const * key, * desc;
};
constexpr SamTag kSamTags[] = {
    {"AS", "bit score"},
    {"OC", "query protein cigar (* for BLASTN)"},
    {"NM", "edit distance (in protein space unless BLASTN)"},
    {"IH", "number of matches this query has"},
    {"ar", "raw score"},
    {"ae", "expect value"},
    {"ai", "% identity (in protein space unless BLASTN) "},
    {"ap", "% positive (in protein space unless BLASTN)"},
    {"qf", "query frame"},
    {"qs", "query protein sequence (* for BLASTN)"},
    {"sf", "subject frame"},
    {"st", "subject taxonomy IDs (* if n/a)"},
    {"ls", "lowest common ancestor scientific name"},
    {"lt", "lowest common ancestor taxonomy ID"},
};
static_assert(sizeof(kSamTags) / sizeof(kSamTags[0]) == kNumSamTags, "one key and description per kTag* of lx_vocab.h");

std::vector<std::string> splitWords(char const * text)
{
    std::vector<std::string> out;
    std::string              cur;
    for (char const * p = text; p && *p; ++p)
    {
        if (std::isspace((unsigned char)*p))
        {
            if (!cur.empty())
                out.push_back(cur);
            cur.clear();
        }
        else
            cur += *p;
    }
    if (!cur.empty())
        out.push_back(cur);
    return out;
}

// --sam-bam-tags (src/search_options.hpp:772-806): every key must be one of the fourteen; the order given is not preserved
bool resolveTags(char const * text, bool (&tags)[kNumSamTags])
{
    for (std::string const & w : splitWords(text ? text : "AS NM ae ai qf")) // :351
    {
        int t = 0;
        while (t < kNumSamTags && w != kSamTags[t].key)
            ++t;
        if (t == kNumSamTags)
        {
            g_output_error = "Unknown column specifier \"" + w + "\". Please see \"--sam-bam-tags help\" for valid options.";
            return false;
        }
        tags[t] = true;
    }
    return true;
}

// --output-columns (src/search_options.hpp:716-760): NCBI's specifiers as seqan::BlastMatchField labels them; "std" = the twelve
// standard columns.  The descriptions are the "# Fields:" labels of .m9 (NCBI's).  Not offered: the columns that need sequence
// data or database titles the writer is not given (qseq, sseq, btop, stitle, ...), and the GI / accession variants.  In the order
// of lx_vocab.h's kCol*.
struct Column
{
    char const * label, * desc;
};
constexpr Column kColumns[] = {
    {"qseqid", "query id"},       {"sseqid", "subject id"},      {"pident", "% identity"},  {"length", "alignment length"},
    {"mismatch", "mismatches"},   {"gapopen", "gap opens"},      {"qstart", "q. start"},    {"qend", "q. end"},
    {"sstart", "s. start"},       {"send", "s. end"},            {"evalue", "evalue"},      {"bitscore", "bit score"},
    {"qlen", "query length"},     {"slen", "subject length"},    {"score", "score"},        {"nident", "identical"},
    {"positive", "positives"},    {"gaps", "gaps"},              {"ppos", "% positives"},   {"frames", "query/sbjct frames"},
    {"qframe", "query frame"},    {"sframe", "sbjct frame"},     {"staxids", "subject tax ids"}, {"lcataxid", "lowest common ancestor taxonomy ID"},
};
static_assert(sizeof(kColumns) / sizeof(kColumns[0]) == kNumColumns, "one label and description per kCol* of lx_vocab.h");

bool resolveColumns(char const * text, std::vector<int> & cols)
{
    for (std::string const & w : splitWords(text ? text : "std"))
    {
        if (w == "std")
        {
            for (int c = kColQSeqId; c <= kColBitScore; ++c)
                cols.push_back(c);
            continue;
        }
        int c = 0;
        while (c < kNumColumns && w != kColumns[c].label)
            ++c;
        if (c == kNumColumns)
        {
            g_output_error = "Unknown column specifier \"" + w + "\". Please see -oc help for valid options.";
            return false;
        }
        cols.push_back(c);
    }
    return !cols.empty();
}

void reverseComplementAscii(std::string & seq)
{
    std::reverse(seq.begin(), seq.end());
    for (char & ch : seq)
        switch (std::toupper((unsigned char)ch))
        {
            case 'A': ch = 'T'; break;
            case 'C': ch = 'G'; break;
            case 'G': ch = 'C'; break;
            case 'T': case 'U': ch = 'A'; break;
            default: ch = 'N';
        }
}

// Where the writers put their bytes: a file (lx_write_records_ex) or memory (lx_render_records)
struct Sink
{
    std::FILE *   f = nullptr;
    std::string * s = nullptr;
    bool          ok = true;
    void          write(void const * p, size_t k)
    {
        if (f)
            ok = std::fwrite(p, 1, k, f) == k && ok;
        else
            s->append(static_cast<char const *>(p), k);
    }
    void put(char c) { write(&c, 1); }
    __attribute__((format(printf, 2, 3))) void print(char const * fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        if (f)
            ok = std::vfprintf(f, fmt, ap) >= 0 && ok;
        else
        {
            char    buf[512];
            va_list aq;
            va_copy(aq, ap);
            int const k = std::vsnprintf(buf, sizeof(buf), fmt, aq);
            va_end(aq);
            if (k >= 0 && (size_t)k < sizeof(buf))
                s->append(buf, (size_t)k);
            else if (k >= 0)
            {
                std::string big((size_t)k + 1, '\0');
                std::vsnprintf(&big[0], big.size(), fmt, ap);
                s->append(big.data(), (size_t)k);
            }
        }
        va_end(ap);
    }
};

// ---- BAM (SAM/BAM specification section 4.2): little-endian fields
template <class T>
void putLe(std::string & o, T v)
{
    for (size_t i = 0; i < sizeof(T); ++i)
        o.push_back((char)(uint8_t)((uint64_t)v >> (8 * i)));
}

// the specification's reg2bin over [beg, end)
int reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14)
        return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17)
        return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20)
        return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23)
        return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26)
        return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// One optional field of a SAM / BAM record.  type: BAM's -- 'f' (f), 'Z' (str), or an integer type 'c' 'C' 'S' 'I' (num)
struct TagValue
{
    char const * key;
    char         type;
    int64_t      num;
    float        f;
    std::string  str;
};

// What a SAM line and a BAM record carry, before either is serialised (MAPQ 255, no mate)
struct SamFields
{
    std::string           qname, sname, cigar, seq, qual;
    bool                  haveQual = false; // (false: QUAL is absent; qual is cut as SEQ is)
    int                   flag     = 0;
    int32_t               refId    = 0;
    int64_t               pos      = 0;     // 0-based; of an untranslated subject: the 64 unsigned bits of s_start
    bool                  posSigned = false; // a translated subject's: it is negative for most minus-frame hits
    std::vector<TagValue> tags;         // in the order myWriteRecord appends them (:601-719)
};

// the SAM line of a record; the integer tags print as i whatever width BAM gives them
void samLine(Sink & f, SamFields const & r)
{
    unsigned long long const pos1 = (unsigned long long)r.pos + 1;
    f.print("%s\t%d\t%s\t", r.qname.c_str(), r.flag, r.sname.c_str());
    if (r.posSigned)
        f.print("%lld", (long long)pos1);
    else
        f.print("%llu", pos1);
    f.print("\t255\t%s\t*\t0\t0\t%s\t%s", r.cigar.c_str(), r.seq.c_str(), r.haveQual ? r.qual.c_str() : "*");
    for (TagValue const & t : r.tags)
        if (t.type == 'f')
            f.print("\t%s:f:%g", t.key, (double)t.f);
        else if (t.type == 'Z')
            f.print("\t%s:Z:%s", t.key, t.str.c_str());
        else
            f.print("\t%s:i:%lld", t.key, (long long)t.num);
    f.put('\n');
}

// the optional fields of a BAM record, with the types myWriteRecord passes (f, S, C, c, I, Z)
void bamTags(std::string & o, std::vector<TagValue> const & tags)
{
    for (TagValue const & t : tags)
    {
        o.append(t.key, 2);
        o.push_back(t.type);
        switch (t.type)
        {
            case 'f':
            {
                uint32_t bits;
                std::memcpy(&bits, &t.f, 4);
                putLe<uint32_t>(o, bits);
                break;
            }
            case 'Z': o.append(t.str.c_str(), t.str.size() + 1); break;
            case 'c': putLe<int8_t>(o, (int8_t)t.num); break;
            case 'C': putLe<uint8_t>(o, (uint8_t)t.num); break;
            case 'S': putLe<uint16_t>(o, (uint16_t)t.num); break;
            default: putLe<uint32_t>(o, (uint32_t)t.num); break;
        }
    }
}

// the BAM alignment record of the same fields (QUAL: the Phred+33 string's bytes - 33, taken modulo 256, or none = 0xFF per base)
void bamRecord(std::string & o, SamFields const & r)
{
    std::string const & cigar = r.cigar, & seq = r.seq, & qname = r.qname;
    std::string const * const qual = r.haveQual ? &r.qual : nullptr;
    int64_t const       pos0 = r.pos; // (BAM keeps its low 32 bits)
    int const           flag = r.flag;
    std::vector<uint32_t> ops;
    int64_t               span = 0;
    if (cigar != "*")
    {
        uint64_t len = 0;
        for (char c : cigar)
        {
            if (c >= '0' && c <= '9')
            {
                len = len * 10 + (uint64_t)(c - '0');
                continue;
            }
            char const * const kOps = "MIDNSHP=X";
            uint32_t const     op   = (uint32_t)(std::strchr(kOps, c) - kOps);
            ops.push_back((uint32_t)len << 4 | op);
            if (c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X')
                span += (int64_t)len;
            len = 0;
        }
    }
    size_t const lseq = seq == "*" ? 0 : seq.size();
    size_t const at   = o.size();
    putLe<int32_t>(o, 0); // block_size, filled in below
    putLe<int32_t>(o, r.refId);
    putLe<int32_t>(o, (int32_t)pos0);
    putLe<uint8_t>(o, (uint8_t)(qname.size() + 1));
    putLe<uint8_t>(o, 255);
    putLe<uint16_t>(o, (uint16_t)reg2bin(pos0, pos0 + (span > 0 ? span : 1)));
    putLe<uint16_t>(o, (uint16_t)ops.size());
    putLe<uint16_t>(o, (uint16_t)flag);
    putLe<int32_t>(o, (int32_t)lseq);
    putLe<int32_t>(o, -1); // next refID
    putLe<int32_t>(o, -1); // next pos
    putLe<int32_t>(o, 0);  // tlen
    o.append(qname.c_str(), qname.size() + 1);
    for (uint32_t x : ops)
        putLe<uint32_t>(o, x);
    static char const kNt16[] = "=ACMGRSVTWYHKDBN";
    for (size_t i = 0; i < lseq; i += 2)
    {
        auto code = [&](size_t k) -> uint8_t
        {
            if (k >= lseq)
                return 0;
            char const * p = std::strchr(kNt16, std::toupper((unsigned char)seq[k]));
            return p && *p ? (uint8_t)(p - kNt16) : (uint8_t)15;
        };
        o.push_back((char)(code(i) << 4 | code(i + 1)));
    }
    if (qual && qual->size() == lseq) // (nullptr: none; samFields cuts it as it cuts SEQ)
        for (char c : *qual)
            o.push_back((char)(uint8_t)((uint8_t)c - 33));
    else
        o.append(lseq, (char)0xff);
    bamTags(o, r.tags);
    uint32_t const bs = (uint32_t)(o.size() - at - 4);
    for (int i = 0; i < 4; ++i)
        o[at + i] = (char)(uint8_t)(bs >> (8 * i));
}

} // namespace

// the bytes lx_render_records and lx_gunzip hand out
struct lx_bytes
{
    std::string b;
};

namespace lxi
{
lx_bytes * bytes_adopt(std::string && s)
{
    lx_bytes * r = new lx_bytes();
    r->b.swap(s);
    return r;
}

void set_output_error(std::string const & msg)
{
    g_output_error = msg;
}
} // namespace lxi

extern "C" {

void lx_output_options_default(lx_output_options * o)
{
    if (!o)
        return;
    *o               = lx_output_options{};
    o->sam_seq       = LX_SAM_SEQ_UNIQ; // src/search_options.hpp:339
    o->sam_hard_clip = 1;               // :360
    o->genetic_code  = 1;               // :170
}

char const * lx_last_output_error(void)
{
    return g_output_error.c_str();
}

int lx_write_footer(char const * path, int format, uint64_t n_records)
{
    if (!path)
        return LX_EINVAL;
    if (format != LX_OUT_BLAST_TAB_COMMENTS)
        return LX_OK;
    std::FILE * f = std::fopen(path, "a");
    if (!f)
        return LX_EINVAL;
    bool ok = std::fprintf(f, "# BLAST processed %llu queries\n", (unsigned long long)n_records) >= 0; // [UPSTREAM-RECALL] seqan::writeFooter
    ok      = (std::fclose(f) == 0) && ok;
    if (!ok)
        g_output_error = std::string("error while writing ") + path;
    return ok ? LX_OK : LX_EINVAL;
}

} // extern "C"

// ---- the request

namespace
{

// the options with their defaults, the format's kind
void applyOptions(int format, lx_output_options const * opt_in, OutputRequest & rq)
{
    rq        = OutputRequest{};
    rq.format = format;
    lx_output_options_default(&rq.opt);
    if (opt_in)
        rq.opt = *opt_in;
    rq.sam = format == LX_OUT_SAM || format == LX_OUT_BAM;
    // BAM always carries the reference sequences (seqan's writeHeader, src/search_output.hpp:440-456): its header text is what
    // --sam-with-refheader writes
    if (format == LX_OUT_BAM)
        rq.opt.sam_with_ref_header = 1;
}

// the tags or the columns the options ask for
bool resolveSpec(OutputRequest & rq)
{
    if (!rq.sam)
        return resolveColumns(rq.opt.columns, rq.cols);
    if (!resolveTags(rq.opt.sam_tags, rq.tags))
        return false;
    for (int t = 0; t < kNumSamTags; ++t)
        rq.tag_mask |= rq.tags[t] ? tagBit(t) : 0u;
    return true;
}

// "# <PROGRAM> 2.2.26+", followed by lambda's tag when the version goes to the output file (src/search_output.hpp:313-345), and the
// other constant texts of a group's comment lines
void m9Texts(char const * program, OutputRequest & rq)
{
    lx_output_options const & opt = rq.opt;
    std::string               versionLine(program);
    for (char & c : versionLine)
        c = (char)std::toupper((unsigned char)c);
    versionLine += " 2.2.26+";
    if (opt.version_to_output)
        versionLine += std::string(" [created by LAMBDA") + (opt.version ? std::string("-") + opt.version : std::string()) +
                       ", see http://seqan.de/lambda and please cite correctly in your academic work]";
    std::string fields;
    for (int c : rq.cols)
        fields += (fields.empty() ? "" : ", ") + std::string(kColumns[c].desc);
    rq.m9[0] = "# " + versionLine + "\n# Query: ";
    rq.m9[1] = std::string("\n# Database: ") + (opt.db_name ? opt.db_name : "lambda_ext") + "\n# Fields: " + fields + "\n# ";
    rq.m9[2] = " hits found\n";
}

} // namespace

namespace lxi
{

// what the caller asked for is resolved before a file or a device is touched (the reference fails while parsing its options)
int resolve_output(int format, char const * program, lx_blast_match const * m, uint64_t n, lx_seq_names const * names,
                   lx_output_options const * opt_in, OutputRequest & rq)
{
    g_output_error.clear();
    if (!names || (!m && n) || !program)
        return LX_EINVAL;
    applyOptions(format, opt_in, rq);
    rq.is_n    = std::strcmp(program, "blastn") == 0;
    rq.q_trans = std::strcmp(program, "blastx") == 0 || std::strcmp(program, "tblastx") == 0;  // qIsTranslated
    rq.s_trans = std::strcmp(program, "tblastn") == 0 || std::strcmp(program, "tblastx") == 0; // sIsTranslated
    if (!rq.is_n && !rq.q_trans && !rq.s_trans && std::strcmp(program, "blastp") != 0)
        return LX_EINVAL;
    if (!resolveSpec(rq))
        return LX_EINVAL;
    if (format == LX_OUT_BLAST_TAB_COMMENTS)
        m9Texts(program, rq);
    // BAM holds a reference's length and a record's position in 32 signed bits (specification 4.2): a longer subject would wrap both
    // silently.  Every BAM entry point resolves its request here, before a file or a device is touched; the text formats print 64 bits
    if (format == LX_OUT_BAM && names->s_lens)
        for (uint64_t i = 0; i < names->n_s; ++i)
            if (names->s_lens[i] > 0x7fffffffull)
            {
                g_output_error = "subject \"" + firstWord(names->s_ids ? names->s_ids[i] : nullptr) + "\" (number " + std::to_string(i) + ") has " +
                                 std::to_string(names->s_lens[i]) + " letters: BAM holds at most 2147483647 (2^31 - 1) per reference";
                return LX_EINVAL;
            }
    return LX_OK;
}

int check_rows(lx_blast_match const * m, uint64_t n, lx_seq_names const * names, char const * text)
{
    for (uint64_t k = 0; k < n; ++k)
        if (m[k].n_qid >= names->n_q || m[k].n_sid >= names->n_s)
        {
            if (text)
                g_output_error = text;
            return LX_EINVAL;
        }
    return LX_OK;
}

// The SAM header text (src/search_output.hpp:347-460): @HD, one @SQ per subject with --sam-with-refheader, @PG, the @CO lines
std::string sam_header(lx_seq_names const * names, OutputRequest const & rq)
{
    lx_output_options const & opt = rq.opt;
    std::string               text;
    Sink                      hs{nullptr, &text};
    hs.print("@HD\tVN:1.4\tGO:query\n");
    // --sam-with-refheader: seqan's writeHeader adds one @SQ per subject from the context ([UPSTREAM-RECALL] behind @HD)
    if (opt.sam_with_ref_header)
        for (uint64_t i = 0; i < names->n_s; ++i)
            hs.print("@SQ\tSN:%s\tLN:%llu\n", firstWord(names->s_ids[i]).c_str(), (unsigned long long)names->s_lens[i]);
    if (opt.version_to_output) // :391-399
        hs.print("@PG\tID:lambda\tPN:lambda\tVN:%s\tCL:%s\n", opt.version ? opt.version : "", opt.command_line ? opt.command_line : "");
    hs.print("@CO\tLambda is a high performance BLAST compatible local aligner, please see http://seqan.de/lambda "
             "for more information.\n");
    hs.print("@CO\tSAM/BAM dialect documentation is available here: https://github.com/seqan/lambda/wiki/Output-Formats\n");
    hs.print("@CO\tIf you use any results found by Lambda, please cite Hauswedell et al. (2014) doi: "
             "10.1093/bioinformatics/btu439\n");
    std::string tagLine = "Optional tags as follow"; // :424-437
    for (int t = 0; t < kNumSamTags; ++t)
        if (rq.tags[t])
            tagLine += std::string("\t") + kSamTags[t].key + ":" + kSamTags[t].desc;
    hs.print("@CO\t%s\n", tagLine.c_str());
    return text;
}

// What stands in front of a BAM stream's records: the magic, the SAM header text, the reference list
std::string bam_header(lx_seq_names const * names, OutputRequest const & rq)
{
    std::string const headerText = sam_header(names, rq);
    std::string       h          = "BAM\1";
    putLe<int32_t>(h, (int32_t)headerText.size());
    h += headerText;
    putLe<int32_t>(h, (int32_t)names->n_s);
    for (uint64_t i = 0; i < names->n_s; ++i)
    {
        std::string const sn = firstWord(names->s_ids[i]);
        putLe<int32_t>(h, (int32_t)(sn.size() + 1));
        h.append(sn.c_str(), sn.size() + 1);
        putLe<int32_t>(h, (int32_t)names->s_lens[i]);
    }
    return h;
}

} // namespace lxi

// ---- the writers of myWriteHeader / myWriteRecord into a sink

namespace
{

// the caller's list, as the writers read it
struct Records
{
    lx_blast_match const * m;
    uint64_t               n;
    uint8_t const *        ops;
    lx_seq_names const *   names;
    uint8_t const *        q_res_ascii;
    uint64_t const *       q_ascii_off;
};

// taxonomy of a subject (NULL tree: "*", as for an index without taxonomy)
std::string taxIdsOf(lx_output_options const & opt, uint64_t n_sid)
{
    if (!opt.tax || n_sid >= opt.tax->n_s || opt.tax->s_tax_off[n_sid + 1] == opt.tax->s_tax_off[n_sid])
        return "*";
    std::string out;
    for (uint64_t x = opt.tax->s_tax_off[n_sid]; x < opt.tax->s_tax_off[n_sid + 1]; ++x)
        out += (out.empty() ? "" : ";") + std::to_string(opt.tax->s_tax_ids[x]);
    return out;
}

// The protein sequence of a query frame (tags qs / OC): the query itself (BLASTP, TBLASTN), its translation (BLASTX, TBLASTX), whose
// six frames are kept for the query translated last
struct QueryProteins
{
    uint64_t    ofQid = ~0ull;
    std::string frames[6];
    std::string of(OutputRequest const & rq, Records const & in, lx_blast_match const & b)
    {
        if (!in.q_res_ascii || !in.q_ascii_off)
            return std::string();
        char const *   src  = reinterpret_cast<char const *>(in.q_res_ascii) + in.q_ascii_off[b.n_qid];
        uint64_t const qLen = in.names->q_lens[b.n_qid];
        if (!rq.q_trans)
            return std::string(src, qLen);
        if (b.q_frame == 0 || std::abs((int)b.q_frame) > 3)
            return std::string();
        if (ofQid != b.n_qid)
        {
            std::vector<uint8_t> nt(qLen), aa(2 * qLen + 8);
            for (uint64_t i = 0; i < qLen; ++i)
                switch (std::toupper((unsigned char)src[i]))
                {
                    case 'A': nt[i] = 0; break;
                    case 'C': nt[i] = 1; break;
                    case 'G': nt[i] = 2; break;
                    case 'T': case 'U': nt[i] = 4; break;
                    default: nt[i] = 3;
                }
            uint64_t fo[6], fl[6];
            if (lx_translate_six_frames(nt.data(), qLen, rq.opt.genetic_code, aa.data(), aa.size(), fo, fl) != LX_OK)
                return std::string();
            for (int fr = 0; fr < 6; ++fr)
            {
                frames[fr].resize(fl[fr]);
                for (uint64_t i = 0; i < fl[fr]; ++i)
                    frames[fr][i] = lambda_amd::kSeqanOrder[std::min<uint8_t>(aa[fo[fr] + i], 26)];
            }
            ofQid = b.n_qid;
        }
        return frames[b.q_frame > 0 ? b.q_frame - 1 : 2 - b.q_frame];
    }
};

// SEQ and QUAL of a record whose SEQ is written, from the query's letters (and opt.q_qual): QUAL is cut and turned exactly as SEQ is
// -- the same window, reversed (not complemented) on the minus strand -- and absent wherever SEQ is
void samSeqQual(OutputRequest const & rq, Records const & in, lx_blast_match const & b, SamFields & r)
{
    uint64_t const     qLen = in.names->q_lens[b.n_qid];
    bool const         hard = rq.opt.sam_hard_clip != 0;
    char const * const src  = reinterpret_cast<char const *>(in.q_res_ascii) + in.q_ascii_off[b.n_qid];
    char const * const qsrc = rq.opt.q_qual ? reinterpret_cast<char const *>(rq.opt.q_qual) + in.q_ascii_off[b.n_qid] : nullptr;
    std::string &      seq = r.seq, & qual = r.qual;
    if (rq.is_n)
    {
        // the aligned sequence is the frame's (the reverse complement on the minus strand); hard clips keep only the
        // matched part of it (:555-582)
        seq.assign(src, qLen);
        if (b.q_frame < 0)
            reverseComplementAscii(seq);
        bool const cut = b.q_end <= qLen && b.q_start <= b.q_end;
        if (hard)
            seq = cut ? seq.substr(b.q_start, b.q_end - b.q_start) : std::string("*");
        if (qsrc && (!hard || cut))
        {
            r.haveQual = true;
            qual.assign(qsrc, qLen);
            if (b.q_frame < 0)
                std::reverse(qual.begin(), qual.end());
            if (hard)
                qual = qual.substr(b.q_start, b.q_end - b.q_start);
        }
    }
    else if (rq.q_trans && b.q_frame != 0)
    {
        // _untranslateSequence (:84-109, :583-598): protein [a, e) of frame f covers the nucleotides
        // [3a + |f| - 1, 3e + |f| - 1) of the strand that was read -- from the read's start on the plus strand,
        // from its end (then reverse-complemented) on the minus strand; soft clips keep the whole frame
        uint64_t const fc = (uint64_t)std::abs((int)b.q_frame) - 1, L = (qLen - fc) / 3;
        uint64_t const a = hard ? b.q_start : 0, e = hard ? b.q_end : L;
        if (e > L || a > e)
            seq = "*";
        else if (b.q_frame > 0)
            seq.assign(src + 3 * a + fc, 3 * (e - a));
        else
        {
            seq.assign(src + (qLen - (3 * e + fc)), 3 * (e - a));
            reverseComplementAscii(seq);
        }
        if (qsrc && !(e > L || a > e))
        {
            r.haveQual = true;
            qual.assign(qsrc + (b.q_frame > 0 ? 3 * a + fc : qLen - (3 * e + fc)), 3 * (e - a));
            if (b.q_frame < 0)
                std::reverse(qual.begin(), qual.end());
        }
    } // BLASTP / TBLASTN: the query is protein -- no SEQ (:599)
    if (seq.empty())
        seq = "*";
    if (seq == "*") // (also the one-letter sequence that reads "*": bamRecord takes it for the absent one)
        r.haveQual = false;
}

void addNum(std::vector<TagValue> & tags, int tag, char type, int64_t v)
{
    tags.push_back({kSamTags[tag].key, type, v, 0.f, std::string()});
}

void addStr(std::vector<TagValue> & tags, int tag, std::string const & v)
{
    tags.push_back({kSamTags[tag].key, 'Z', 0, 0.f, v});
}

// the optional fields in the order myWriteRecord appends them (:601-719), with the widths it casts to
void samTags(OutputRequest const & rq, Records const & in, lx_blast_match const & b, uint64_t hits, uint32_t lca, bool writeSeq,
             std::string const & protCigar, QueryProteins & proteins, std::vector<TagValue> & tags)
{
    lx_output_options const & opt = rq.opt;
    tags.clear();
    if (rq.tags[kTagEValue])
        tags.push_back({kSamTags[kTagEValue].key, 'f', 0, (float)b.e_value, std::string()});
    if (rq.tags[kTagBitScore])
        addNum(tags, kTagBitScore, 'S', (uint16_t)b.bit_score);
    if (rq.tags[kTagScore])
        addNum(tags, kTagScore, 'C', (uint8_t)b.score); // (uint8_t in the reference, :612-616: scores beyond 255 wrap)
    if (rq.tags[kTagPIdent])
        addNum(tags, kTagPIdent, 'C', (uint8_t)b.identity);
    if (rq.tags[kTagPPos])
        addNum(tags, kTagPPos, 'S', (uint16_t)(b.alignment_length ? 100.0 * b.num_positives / b.alignment_length : 0.0));
    if (rq.tags[kTagQFrame])
        addNum(tags, kTagQFrame, 'c', (int8_t)b.q_frame);
    if (rq.tags[kTagSFrame])
        addNum(tags, kTagSFrame, 'c', (int8_t)b.s_frame);
    if (rq.tags[kTagSTaxIds])
        addStr(tags, kTagSTaxIds, taxIdsOf(opt, b.n_sid));
    if (rq.tags[kTagLcaId])
        addStr(tags, kTagLcaId, (opt.tax_names && opt.tax && lca < opt.tax->n_taxa && opt.tax_names[lca]) ? opt.tax_names[lca] : "*");
    if (rq.tags[kTagLcaTaxId])
        addNum(tags, kTagLcaTaxId, 'I', lca);
    if (rq.tags[kTagProtSeq]) // :669-689
    {
        std::string prot = (rq.is_n || !writeSeq) ? std::string() : proteins.of(rq, in, b);
        if (!prot.empty() && opt.sam_hard_clip != 0)
            prot = b.q_end <= prot.size() && b.q_start <= b.q_end ? prot.substr(b.q_start, b.q_end - b.q_start) : std::string();
        addStr(tags, kTagProtSeq, prot.empty() ? "*" : prot);
    }
    if (rq.tags[kTagProtCigar])
        addStr(tags, kTagProtCigar, protCigar);
    if (rq.tags[kTagEditDistance])
        addNum(tags, kTagEditDistance, 'I', (uint32_t)(b.alignment_length - b.num_matches));
    if (rq.tags[kTagMatchCount])
        addNum(tags, kTagMatchCount, 'I', (uint32_t)hits);
}

// The fields of record k of the query group [lo, hi), whose LCA is lca.  false: the row names a query or a subject the name lists do
// not have
bool samFields(OutputRequest const & rq, Records const & in, uint64_t lo, uint64_t hi, uint64_t k, uint32_t lca, QueryProteins & proteins,
               SamFields & r)
{
    lx_blast_match const * const m = in.m;
    lx_blast_match const &       b = m[k];
    if (b.n_qid >= in.names->n_q || b.n_sid >= in.names->n_s)
        return false;
    lx_output_options const & opt  = rq.opt;
    uint64_t const            qLen = in.names->q_lens[b.n_qid];
    bool const                hard = opt.sam_hard_clip != 0;
    r.flag  = ((k == lo) ? 0 : 256) | (b.q_frame < 0 ? 16 : 0); // secondary (:505, :723), RC (:506-507)
    r.qname = firstWord(in.names->q_ids[b.n_qid]);
    r.sname = firstWord(in.names->s_ids[b.n_sid]);
    r.refId = (int32_t)b.n_sid;
    // the DNA cigar: every program but BLASTP / TBLASTN, whose query is protein (:513-531)
    r.cigar = (rq.is_n || rq.q_trans) ? cigarOf(b, in.ops, qLen, hard, rq.q_trans) : std::string("*");
    std::string protCigar = "*";
    if (rq.tags[kTagProtCigar] && !rq.is_n) // OC: protein-space cigar, clips like the DNA one, never reversed (:197-298)
        protCigar = protCigarOf(b, in.ops, qLen, hard, rq.q_trans);
    // --sam-bam-seq (:533-553): always, never, or once per query region and frame
    bool writeSeq = opt.sam_seq >= LX_SAM_SEQ_ALWAYS;
    if (opt.sam_seq == LX_SAM_SEQ_UNIQ)
        writeSeq = (k == lo) || b.q_frame != m[k - 1].q_frame || b.q_start != m[k - 1].q_start || b.q_end != m[k - 1].q_end;
    r.seq      = "*";
    r.haveQual = false;
    if (writeSeq && in.q_res_ascii && in.q_ascii_off)
        samSeqQual(rq, in, b, r);
    // POS: a translated subject is reported in nucleotide space (:493-499; the minus-strand branch there
    // subtracts from the QUERY length -- restated as it stands).  That difference is a signed quantity: beginPos is, and a query is
    // shorter than where most hits begin
    r.pos       = (int64_t)b.s_start;
    r.posSigned = rq.s_trans;
    if (rq.s_trans)
    {
        uint64_t const p = b.s_start * 3 + (uint64_t)std::abs((int)b.s_frame) - (b.s_frame != 0 ? 1 : 0);
        r.pos            = (int64_t)(b.s_frame < 0 ? qLen - p : p);
    }
    samTags(rq, in, b, hi - lo, lca, writeSeq, protCigar, proteins, r.tags);
    return true;
}

// the SAM / BAM branch of myWriteHeader and myWriteRecord (src/search_output.hpp:347-460, :463-733)
int renderSam(Sink & f, OutputRequest const & rq, int write_header, Records const & in)
{
    bool const bam = rq.format == LX_OUT_BAM;
    if (write_header)
    {
        std::string const h = bam ? lxi::bam_header(in.names, rq) : lxi::sam_header(in.names, rq);
        f.write(h.data(), h.size());
    }
    bool const    wantLca = rq.tags[kTagLcaTaxId] || rq.tags[kTagLcaId];
    LcaCursor     lcaCursor;
    QueryProteins proteins;
    SamFields     r;
    std::string   rec; // (BAM: one record)
    for (uint64_t lo = 0; lo < in.n;)
    {
        uint64_t hi = lo + 1;
        while (hi < in.n && in.m[hi].n_qid == in.m[lo].n_qid)
            ++hi;
        uint32_t const lca = wantLca ? lcaCursor.of(rq.opt, in.m[lo].n_qid) : 0u;
        for (uint64_t k = lo; k < hi; ++k)
        {
            if (!samFields(rq, in, lo, hi, k, lca, proteins, r))
                return LX_EINVAL;
            if (!bam)
            {
                samLine(f, r);
                continue;
            }
            rec.clear();
            bamRecord(rec, r);
            f.write(rec.data(), rec.size());
        }
        lo = hi;
    }
    return LX_OK;
}

template <class... Args>
void put(std::string & out, char const * fmt, Args... args)
{
    char tmp[64];
    out.append(tmp, (size_t)std::snprintf(tmp, sizeof(tmp), fmt, args...));
}

// A translated side is reported in nucleotide positions of the original sequence ([UPSTREAM-RECALL] seqan blast module,
// _untranslatePositions): protein [a, e) of frame f covers the nucleotides [3a + |f| - 1, 3e + |f| - 1) of the strand that was read; on
// the minus strand the positions are mirrored and start > end
void untranslate(uint64_t a, uint64_t e, int frame, uint64_t len, unsigned long long & first, unsigned long long & last)
{
    uint64_t const shift = (uint64_t)std::abs(frame) - 1;
    uint64_t const lo = 3 * a + shift, hi = 3 * e + shift;
    if (frame >= 0)
    {
        first = lo + 1;
        last  = hi;
    }
    else
    {
        first = len - lo;
        last  = len - hi + 1;
    }
}

// one record -> one line, appended to `out` (the same text whichever thread makes it)
void formatRecord(OutputRequest const & rq, lx_seq_names const * names, lx_blast_match const & b, uint32_t lca, std::string & out)
{
    // 1-based inclusive; a hit of the reverse-complemented query is reported BLAST-style on the forward query
    // strand with descending subject coordinates
    unsigned long long qs = b.q_start + 1, qe = b.q_end, ss = b.s_start + 1, se = b.s_end;
    if (rq.q_trans)
        untranslate(b.q_start, b.q_end, b.q_frame, names->q_lens[b.n_qid], qs, qe);
    else if (b.q_frame < 0)
    {
        unsigned long long const ql = names->q_lens[b.n_qid];
        qs = ql - b.q_end + 1;
        qe = ql - b.q_start;
        std::swap(ss, se);
    }
    if (rq.s_trans)
        untranslate(b.s_start, b.s_end, b.s_frame, names->s_lens[b.n_sid], ss, se);
    bool first = true;
    for (int c : rq.cols)
    {
        if (!first)
            out.push_back('\t');
        first = false;
        switch (c)
        {
            case kColQSeqId: out += firstWord(names->q_ids[b.n_qid]).c_str(); break;
            case kColSSeqId: out += firstWord(names->s_ids[b.n_sid]).c_str(); break;
            case kColQLen: put(out, "%llu", (unsigned long long)names->q_lens[b.n_qid]); break;
            case kColSLen: put(out, "%llu", (unsigned long long)names->s_lens[b.n_sid]); break;
            case kColQStart: put(out, "%llu", qs); break;
            case kColQEnd: put(out, "%llu", qe); break;
            case kColSStart: put(out, "%llu", ss); break;
            case kColSEnd: put(out, "%llu", se); break;
            case kColEValue: put(out, "%.1e", b.e_value); break;
            case kColBitScore: put(out, "%.1f", b.bit_score); break;
            case kColScore: put(out, "%d", b.score); break;
            case kColLength: put(out, "%d", b.alignment_length); break;
            case kColPIdent: put(out, "%.2f", (double)b.identity); break;
            case kColNIdent: put(out, "%d", b.num_matches); break;
            case kColMismatch: put(out, "%d", b.num_mismatches); break;
            case kColPositive: put(out, "%d", b.num_positives); break;
            case kColGapOpen: put(out, "%d", b.num_gap_opens); break;
            case kColGaps: put(out, "%d", b.num_gap_opens + b.num_gap_extensions); break; // every gap character
            case kColPPos: put(out, "%.2f", b.alignment_length ? 100.0 * b.num_positives / b.alignment_length : 0.0); break;
            case kColFrames: put(out, "%d/%d", (int)b.q_frame, (int)b.s_frame); break;
            case kColQFrame: put(out, "%d", (int)b.q_frame); break;
            case kColSFrame: put(out, "%d", (int)b.s_frame); break;
            case kColSTaxIds: out += taxIdsOf(rq.opt, b.n_sid).c_str(); break;
            case kColLcaTaxId: put(out, "%u", lca); break;
            default: break;
        }
    }
    out.push_back('\n');
}

// the comment lines in front of a query group in .m9 (printf's "(null)" for a missing id)
void writeComments(Sink & f, OutputRequest const & rq, char const * q_id, uint64_t hits)
{
    if (!q_id)
        q_id = "(null)";
    f.write(rq.m9[0].data(), rq.m9[0].size());
    f.write(q_id, std::strlen(q_id));
    f.write(rq.m9[1].data(), rq.m9[1].size());
    f.print("%llu", (unsigned long long)hits);
    f.write(rq.m9[2].data(), rq.m9[2].size());
}

// a plain table of many records: the lines are made on the library's host threads, piece by piece, and written in order
int renderTableBulk(Sink & f, OutputRequest const & rq, Records const & in)
{
    unsigned const           nt = lxi::pool_width();
    uint64_t const           n  = in.n;
    std::vector<std::string> piece(nt);
    std::vector<uint8_t>     failed(nt, 0);
    uint64_t const           step = (n + nt - 1) / nt;
    lxi::pool_run(nt,
                  [&](unsigned t)
                  {
                      try // (an exception must not leave a pool thread: out of memory is reported below)
                      {
                          std::string & out = piece[t];
                          out.reserve((size_t)(std::min(n, (t + 1) * step) - std::min(n, t * step)) * 96);
                          for (uint64_t k = std::min(n, t * step); k < std::min(n, (t + 1) * step); ++k)
                              formatRecord(rq, in.names, in.m[k], 0u, out);
                      }
                      catch (...)
                      {
                          failed[t] = 1;
                      }
                  });
    for (unsigned t = 0; t < nt; ++t)
    {
        if (failed[t])
        {
            g_output_error = "out of memory while formatting the records";
            return LX_ENOMEM;
        }
        f.write(piece[t].data(), piece[t].size());
    }
    return LX_OK;
}

// the tabular branch of myWriteRecord: per query group the comment lines (.m9), then a line per record
int renderTable(Sink & f, OutputRequest const & rq, Records const & in)
{
    if (lxi::check_rows(in.m, in.n, in.names, nullptr) != LX_OK)
        return LX_EINVAL;
    bool const comments = rq.format == LX_OUT_BLAST_TAB_COMMENTS;
    bool const hasLca   = std::find(rq.cols.begin(), rq.cols.end(), (int)kColLcaTaxId) != rq.cols.end();
    if (!comments && !hasLca && in.n >= 65536 && lxi::pool_width() > 1)
        return renderTableBulk(f, rq, in);
    LcaCursor   lcaCursor;
    std::string line;
    for (uint64_t lo = 0; lo < in.n;)
    {
        uint64_t hi = lo + 1;
        while (hi < in.n && in.m[hi].n_qid == in.m[lo].n_qid)
            ++hi;
        if (comments)
            writeComments(f, rq, in.names->q_ids[in.m[lo].n_qid], hi - lo);
        uint32_t const lca = hasLca ? lcaCursor.of(rq.opt, in.m[lo].n_qid) : 0u;
        for (uint64_t k = lo; k < hi; ++k)
        {
            line.clear();
            formatRecord(rq, in.names, in.m[k], lca, line);
            f.write(line.data(), line.size());
        }
        lo = hi;
    }
    return LX_OK;
}

// a resolved request's header (write_header) and records into the sink: the text formats, or BAM (the SAM records in binary, the SAM
// header with its @SQ lines and the reference list in front)
int renderRecords(Sink & f, OutputRequest const & rq, int write_header, Records const & in)
{
    return rq.sam ? renderSam(f, rq, write_header, in) : renderTable(f, rq, in);
}

} // namespace

extern "C" {

// what lx_write_records_ex would refuse before it touches a file: the format, the column specifiers / SAM tags
int lx_check_output_options(int format, lx_output_options const * opt_in)
{
    g_output_error.clear();
    if (format != LX_OUT_BLAST_TAB && format != LX_OUT_BLAST_TAB_COMMENTS && format != LX_OUT_SAM && format != LX_OUT_BAM)
    {
        g_output_error = "unknown output format";
        return LX_EINVAL;
    }
    OutputRequest rq;
    applyOptions(format, opt_in, rq);
    return resolveSpec(rq) ? LX_OK : LX_EINVAL;
}

int lx_write_records(char const * path, int format, int write_header, char const * program, lx_blast_match const * m,
                     uint64_t n, uint8_t const * ops, lx_seq_names const * names, uint8_t const * q_res_ascii,
                     uint64_t const * q_ascii_off)
{
    return lx_write_records_ex(path, format, write_header, program, m, n, ops, names, q_res_ascii, q_ascii_off, nullptr);
}

int lx_write_records_ex(char const * path, int format, int write_header, char const * program, lx_blast_match const * m,
                        uint64_t n, uint8_t const * ops, lx_seq_names const * names, uint8_t const * q_res_ascii,
                        uint64_t const * q_ascii_off, lx_output_options const * opt_in)
{
    g_output_error.clear();
    if (!path || format == LX_OUT_BAM) // (BAM is binary and BGZF-compressed: lx_write_records_bgzf)
        return LX_EINVAL;
    // what the caller asked for is resolved before the file is touched
    OutputRequest rq;
    int           rc = lxi::resolve_output(format, program, m, n, names, opt_in, rq);
    if (rc != LX_OK)
        return rc;
    std::FILE * file = std::fopen(path, write_header ? "w" : "a");
    if (!file)
    {
        g_output_error = std::string("cannot open ") + path;
        return LX_EINVAL;
    }
    Sink f{file, nullptr};
    rc = renderRecords(f, rq, write_header, Records{m, n, ops, names, q_res_ascii, q_ascii_off});
    // (the fprintf paths set the stream's error indicator: one look at the end covers them)
    bool io_ok = f.ok && !std::ferror(file);
    io_ok      = (std::fclose(file) == 0) && io_ok;
    if (rc != LX_OK)
        return rc;
    if (!io_ok)
    {
        g_output_error = std::string("error while writing ") + path + " (disk full?)";
        return LX_EINVAL;
    }
    return LX_OK;
}

int lx_render_records(int format, int write_header, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                      lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                      lx_output_options const * opt, int64_t footer_records, lx_bytes ** out)
{
    g_output_error.clear();
    if (!out || format < LX_OUT_BLAST_TAB || format > LX_OUT_BAM)
        return LX_EINVAL;
    *out = nullptr;
    OutputRequest rq;
    int           rc = lxi::resolve_output(format, program, m, n, names, opt, rq);
    if (rc != LX_OK)
        return rc;
    lx_bytes * r = nullptr;
    try
    {
        r = new lx_bytes();
        Sink s{nullptr, &r->b};
        rc = renderRecords(s, rq, write_header, Records{m, n, ops, names, q_res_ascii, q_ascii_off});
        if (rc == LX_OK && footer_records >= 0 && format == LX_OUT_BLAST_TAB_COMMENTS) // lx_write_footer
            s.print("# BLAST processed %llu queries\n", (unsigned long long)footer_records);
    }
    catch (std::bad_alloc const &)
    {
        g_output_error = "out of memory while formatting the records";
        rc             = LX_ENOMEM;
    }
    if (rc != LX_OK)
    {
        delete r;
        return rc;
    }
    *out = r;
    return LX_OK;
}

uint8_t const * lx_bytes_data(lx_bytes const * b)
{
    return b ? reinterpret_cast<uint8_t const *>(b->b.data()) : nullptr;
}

uint64_t lx_bytes_size(lx_bytes const * b)
{
    return b ? b->b.size() : 0;
}

void lx_bytes_free(lx_bytes * b)
{
    delete b;
}

} // extern "C"
