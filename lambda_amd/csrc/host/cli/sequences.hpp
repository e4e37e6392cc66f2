// cli/sequences.hpp -- the sequence sets of the lambda3 front end: input files (FASTA or FASTQ, plain or gzip-compressed) into ranks and
// frames, the query file as a stream for --lazy-query, and the reduced alphabet of the seeding stage.  Included by lambda3_main.cpp only.
#pragma once

#include "common.hpp"

namespace
{

struct SeqSet
{
    std::vector<std::string> ids;
    std::vector<uint8_t>     res;   // ranks, concatenated (frame-expanded for nucleotide queries)
    std::vector<uint64_t>    off, len;
    std::string              ascii; // original letters of the untranslated sequences, concatenated
    std::string              qual;  // --sam-bam-qual yes, a FASTQ file: their base qualities, parallel to `ascii`; else empty
    std::vector<uint64_t>    ascii_off, orig_len;
};

// the sum of the (frame-expanded) sequence lengths (the subjects': dbTotalLength, src/search_algo.hpp:317-319)
uint64_t totalLetters(SeqSet const & set)
{
    uint64_t n = 0;
    for (uint64_t l : set.len)
        n += l;
    return n;
}

// byte -> rank: the letters of `order`, in either case, rank by their place in it (U as T where `uAsT`), every other byte ranks `unknown`
std::array<uint8_t, 256> rankTable(char const * order, uint8_t unknown, bool uAsT)
{
    std::array<uint8_t, 256> t;
    t.fill(unknown);
    for (size_t r = 0; order[r]; ++r)
        t[(unsigned char)order[r]] = t[(unsigned char)std::tolower(order[r])] = (uint8_t)r;
    if (uAsT)
        t['U'] = t['u'] = t['T'];
    return t;
}

uint8_t aaRank(char c) // SeqAn2 AminoAcid rank (src/seqan2_to_biocpp.hpp:352-366), unknown -> X
{
    static auto const table = rankTable(lambda_amd::kSeqanOrder, 25, false);
    return table[(unsigned char)c];
}

uint8_t dnaRank(char c) // BioC++ dna5 rank A,C,G,N,T (Simple-scored alphabets pass it through, :392-393)
{
    static auto const table = rankTable("ACGNT", 3, true);
    return table[(unsigned char)c];
}

uint8_t dnaRankSeqan(char c) // SeqAn Dna5 rank A,C,G,T,N: the bisulfite schemes are matrices over it (src/bisulfite_scoring.hpp:54-93)
{
    static auto const table = rankTable("ACGTN", 4, true);
    return table[(unsigned char)c];
}

// ---- input files: FASTA or FASTQ, plain or gzip-compressed (BGZF or not), told apart by their bytes, not their names
// (the reference reads fa, fq, fasta, fastq, fna, faa, each optionally .gz: src/search_options.hpp:157-167, src/mkindex_options.hpp:96-105)
struct InputText
{
    std::string text;
    double      msGunzip = 0; // decompression time (0: the file was not compressed)
    bool        onDevice = false;
    uint64_t    plainMembers = 0, plainChunks = 0; // plain members lx_gunzip decoded in parallel on the device, and their chunks
};

// the file's bytes, decompressed by lx_gunzip when they start with the gzip magic: BGZF members on `device` (< 0: every member on the
// host) and so the large plain members, in parallel chunks; other members on this thread.  One handle per call, so that the two
// reader threads never share one.
InputText readInput(std::string const & path, int device)
{
    std::FILE * f = std::fopen(path.c_str(), "rb");
    if (!f)
        throw std::runtime_error("cannot open " + path);
    InputText r;
    std::string raw;
    char        buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;)
        raw.append(buf, got);
    bool const err = std::ferror(f) != 0;
    std::fclose(f);
    if (err)
        throw std::runtime_error("error while reading " + path);
    if (raw.size() >= 3 && raw.compare(0, 3, "BZh") == 0)
        throw std::runtime_error(path + ": bzip2-compressed input is not supported (decompress it, or recompress it with gzip or bgzip)");
    if (raw.size() < 2 || (uint8_t)raw[0] != 0x1f || (uint8_t)raw[1] != 0x8b)
    {
        r.text.swap(raw);
        return r;
    }
    auto const        t0    = Clock::now();
    HandleOwner const keepH = device >= 0 ? makeHandle(device) : HandleOwner();
    lx_handle * const h     = keepH.get();
    lx_bytes *        out   = nullptr;
    if (lx_gunzip(h, reinterpret_cast<uint8_t const *>(raw.data()), raw.size(), &out) != LX_OK)
        throw std::runtime_error(path + ": " + (h ? lx_last_error(h) : lx_last_output_error()));
    BytesOwner const keep(out);
    r.text.assign(reinterpret_cast<char const *>(lx_bytes_data(out)), lx_bytes_size(out));
    r.msGunzip = msSince(t0);
    r.onDevice = h != nullptr;
    lx_gunzip_stats st;
    if (h && lx_last_gunzip_stats(h, &st) == LX_OK)
    {
        r.plainMembers = st.plain_parallel;
        r.plainChunks  = st.chunks;
    }
    return r;
}

// f(id, letters) per record of a FASTA (">") or FASTQ ("@") text, until f returns false: the rules are lx_query_blocks.hpp's, an
// incremental parser that is fed the whole text here.
using lx_query_blocks::forEachRecord;

// one record into the set: its letters, ranks and frames (`cur` is used up), and its qualities where they are kept (`qual`)
// translate = six protein frames per nucleotide sequence (BLASTX queries: qryNumFrames = 6, translate_join)
// bsFrames: 0 = none; 1 = bisulfite subjects (every sequence twice: views::duplicate, src/shared_definitions.hpp:249-250);
// 2 = bisulfite queries (strand, strand, reverse complement, reverse complement: add_reverse_complement | duplicate, :260-261)
void addRecord(SeqSet & out, std::string const & id, std::string & cur, bool protein, bool addRevComp, bool translate, int geneticCode, int bsFrames,
               std::string const * qual = nullptr)
{
    out.ids.push_back(id);
    out.ascii_off.push_back(out.ascii.size());
    out.orig_len.push_back(cur.size());
    out.ascii += cur;
    if (qual)
        out.qual += *qual;
    if (translate)
    {
        std::vector<uint8_t> nt(cur.size());
        for (size_t i = 0; i < cur.size(); ++i)
            nt[i] = dnaRank(cur[i]);
        std::vector<uint8_t> aa(2 * cur.size() + 8);
        uint64_t             fo[6], fl[6];
        if (lx_translate_six_frames(nt.data(), nt.size(), geneticCode, aa.data(), aa.size(), fo, fl) != LX_OK)
            throw std::runtime_error("translation failed for " + out.ids.back() + " (genetic code " + std::to_string(geneticCode) + ")");
        for (int f = 0; f < 6; ++f)
        {
            out.off.push_back(out.res.size());
            out.len.push_back(fl[f]);
            out.res.insert(out.res.end(), aa.begin() + fo[f], aa.begin() + fo[f] + fl[f]);
        }
        cur.clear();
        return;
    }
    if (bsFrames)
    {
        auto push = [&](bool rc)
        {
            out.off.push_back(out.res.size());
            out.len.push_back(cur.size());
            static uint8_t const comp[5] = {3, 2, 1, 0, 4};
            size_t const at = out.res.size(), n = cur.size();
            out.res.resize(at + n);
            if (!rc)
                for (size_t k = 0; k < n; ++k)
                    out.res[at + k] = dnaRankSeqan(cur[k]);
            else
                for (size_t k = 0; k < n; ++k)
                    out.res[at + k] = comp[dnaRankSeqan(cur[n - 1 - k])];
        };
        push(false);
        push(false);
        if (bsFrames == 2)
        {
            push(true);
            push(true);
        }
        cur.clear();
        return;
    }
    out.off.push_back(out.res.size());
    out.len.push_back(cur.size());
    {
        size_t const at = out.res.size();
        out.res.resize(at + cur.size());
        if (protein)
            for (size_t k = 0; k < cur.size(); ++k)
                out.res[at + k] = aaRank(cur[k]);
        else
            for (size_t k = 0; k < cur.size(); ++k)
                out.res[at + k] = dnaRank(cur[k]);
    }
    if (addRevComp) // qryNumFrames = 2 for BLASTN (src/search_datastructures.hpp:380-385)
    {
        out.off.push_back(out.res.size());
        out.len.push_back(cur.size());
        static uint8_t const comp[5] = {4, 2, 1, 3, 0};
        size_t const at = out.res.size(), n = cur.size();
        out.res.resize(at + n);
        for (size_t k = 0; k < n; ++k) // (the forward frame's ranks stand right before)
            out.res[at + k] = comp[out.res[at - 1 - k]];
    }
    cur.clear();
}

void readFasta(std::string const & text, std::string const & path, bool protein, bool addRevComp, SeqSet & out, bool translate = false,
               int geneticCode = 1, int bsFrames = 0, bool keepQual = false)
{
    lx_query_blocks::RecordParser parser(path);
    parser.keepQualities(keepQual);
    auto f = [&](std::string const & id, std::string & letters)
    {
        addRecord(out, id, letters, protein, addRevComp, translate, geneticCode, bsFrames, keepQual ? &parser.quality() : nullptr);
        return true;
    };
    if (parser.feed(text.data(), text.size(), f))
        parser.finish(f);
}

// --sam-bam-qual yes: the set's qualities for the writers (lx_output_options::q_qual), NULL where the file had none (FASTA)
uint8_t const * qualOf(SeqSet const & set)
{
    return !set.ascii.empty() && set.qual.size() == set.ascii.size() ? reinterpret_cast<uint8_t const *>(set.qual.data()) : nullptr;
}

// the reference lets BioC++ detect the query alphabet (src/search_options.hpp); here: nucleotide if >= 90 % of the
// letters of the first sequences are ACGTUN
struct DnaVote
{
    uint64_t nuc = 0, all = 0;
    bool     operator()(std::string const &, std::string const & letters) // (false: enough letters seen)
    {
        for (char c : letters)
            nuc += std::strchr("ACGTUNacgtun", c) != nullptr;
        all += letters.size();
        return all < 100000;
    }
    bool dna() const { return all > 0 && nuc * 10 >= all * 9; }
};

bool looksLikeDna(std::string const & text, std::string const & path)
{
    DnaVote vote;
    forEachRecord(text, path, [&](std::string const & id, std::string const & letters) { return vote(id, letters); });
    return vote.dna();
}

// ---- --lazy-query: the query file as a stream of pieces (lx_gunzip_stream: decompressed where needed, BGZF groups and large plain
// members on `device`)
// and of records (lx_query_blocks::RecordParser).  The first two pieces are taken at once: the bzip2 refusal and the alphabet come
// from the first, and whether it is the whole file from the second.
struct QueryStream
{
    std::string                   path;
    HandleOwner                   h;
    lx_gunzip_stream *            s = nullptr;
    std::vector<lx_bytes *>       ahead; // pieces taken and not parsed yet
    bool                          ended = false;
    lx_query_blocks::RecordParser parser;

    QueryStream(std::string const & path_, int device, bool keepQual = false) : path(path_), parser(path_)
    {
        parser.keepQualities(keepQual);
        if (device >= 0)
            h = makeHandle(device);
        if (lx_gunzip_stream_open(h.get(), path.c_str(), kPiece, &s) != LX_OK)
        {
            std::string const why = h ? lx_last_error(h.get()) : lx_last_output_error();
            throw std::runtime_error(why.find("cannot open") != std::string::npos ? "cannot open " + path : path + ": " + why);
        }
        take();
        take();
        if (!ahead.empty() && lx_bytes_size(ahead[0]) >= 3 && std::memcmp(lx_bytes_data(ahead[0]), "BZh", 3) == 0)
            throw std::runtime_error(path + ": bzip2-compressed input is not supported (decompress it, or recompress it with gzip or bgzip)");
    }
    QueryStream(QueryStream const &) = delete;
    ~QueryStream()
    {
        for (lx_bytes * b : ahead)
            lx_bytes_free(b);
        lx_gunzip_stream_close(s);
    }
    void take() // one more piece into `ahead`, or the end
    {
        if (ended)
            return;
        lx_bytes * piece = nullptr;
        if (lx_gunzip_stream_next(s, &piece) != LX_OK)
            throw std::runtime_error(path + ": " + (h ? lx_last_error(h.get()) : lx_last_output_error()));
        if (piece)
            ahead.push_back(piece);
        else
            ended = true;
        lx_gunzip_stats st; // (of the whole file, behind the call that reports its end)
        if (ended && h && lx_last_gunzip_stats(h.get(), &st) == LX_OK)
        {
            plainMembers  = st.plain_parallel;
            plainChunks   = st.chunks;
            plainDeclined = st.declined;
        }
    }
    // for the stage-time line, what readInput says of the eager path: the plain members the stream decoded on the device
    std::string gunzipNote() const
    {
        if (!plainMembers && !plainDeclined)
            return std::string();
        return " (query stream: " + std::to_string(plainMembers) + " plain member(s) in " + std::to_string(plainChunks) + " chunks on the GPU" +
               (plainDeclined ? ", " + std::to_string(plainDeclined) + " finished on the host after a decline" : std::string()) + ")";
    }
    // looksLikeDna over the first piece (all of the file a small file has)
    bool looksLikeDna() const
    {
        DnaVote                       vote;
        auto                          f = [&](std::string const & id, std::string const & letters) { return vote(id, letters); };
        lx_query_blocks::RecordParser p(path);
        try
        {
            if (!ahead.empty() && p.feed(reinterpret_cast<char const *>(lx_bytes_data(ahead[0])), lx_bytes_size(ahead[0]), f) && ahead.size() == 1)
                p.finish(f);
        }
        catch (std::runtime_error const &)
        {
            // (a malformed record: the letters in front of it decide; the block that holds it reports it)
        }
        return vote.dna();
    }
    // f(id, letters) per record from where the last call stopped, until f returns false (true: more may follow) or the file ends
    // (false).  A piece is parsed whole, so records f has not asked for wait in `kept`.  While f runs, quality() is the record's
    // quality string (empty unless the stream was opened to keep them and the file is FASTQ).
    template <class F>
    bool records(F && f)
    {
        for (;;)
        {
            while (keptAt < kept.size())
            {
                auto & r = kept[keptAt++];
                if (!f(r.first, r.second))
                    return true;
            }
            kept.clear();
            keptQual.clear();
            keptAt = 0;
            if (malformed) // (the records in front of it have been handed out)
                std::rethrow_exception(malformed);
            auto keep = [&](std::string const & id, std::string & letters)
            {
                kept.emplace_back(id, std::string());
                kept.back().second.swap(letters);
                keptQual.emplace_back();
                keptQual.back().swap(parser.quality());
                return true;
            };
            if (!ahead.empty()) // (a slice of the piece at a time: `kept` stays small)
            {
                lx_bytes * const b = ahead.front();
                uint64_t const   n = std::min<uint64_t>(kSlice, lx_bytes_size(b) - pieceAt);
                try
                {
                    parser.feed(reinterpret_cast<char const *>(lx_bytes_data(b)) + pieceAt, n, keep);
                }
                catch (std::runtime_error const &)
                {
                    malformed = std::current_exception();
                }
                if ((pieceAt += n) == lx_bytes_size(b))
                {
                    lx_bytes_free(b);
                    ahead.erase(ahead.begin());
                    pieceAt = 0;
                    take();
                }
            }
            else if (!finished)
            {
                finished = true;
                try
                {
                    parser.finish(keep);
                }
                catch (std::runtime_error const &)
                {
                    malformed = std::current_exception();
                }
            }
            else
                return false;
        }
    }
    std::string const & quality() const { return keptQual[keptAt - 1]; }
    std::vector<std::pair<std::string, std::string>> kept;
    std::vector<std::string>                         keptQual; // parallel to `kept`
    size_t                                           keptAt = 0;
    uint64_t                                         pieceAt = 0; // bytes of ahead[0] the parser has
    bool                                             finished = false;
    std::exception_ptr                               malformed; // the parser's error, kept until the records in front of it are out
    uint64_t                                         plainMembers = 0, plainChunks = 0, plainDeclined = 0; // of the whole file, once the stream has ended
    // text per piece of the stream; per call of the parser.  A wave of a plain member has a piece's worth of input at most, so 32 MiB
    // are 512 chunks of 64 KiB, one per decoder the device runs at a time (lx_gunzip's own wave).  Not measured: no run at size yet.
    // The cost is memory, for every kind of input: the reader holds up to two pieces of 32 MiB, inside a plain member up to
    // 320 MiB of a wave's text on top (a third of that is typical), and the stream's handle about 1 GiB of device buffers.
    static constexpr uint64_t kPiece = 32ull << 20, kSlice = 1ull << 20;
};

// ---- the reduced alphabet of the seeding stage (the word table is made over the reduced subjects, the seeds from the reduced queries)
struct Reduction
{
    bool            prot = false, bs = false;
    uint8_t const * tab  = nullptr; // rank -> reduced letter (none: the ranks stay; bisulfite: two tables, by frame)
    int             alph = 27;      // letters of the reduced alphabet
};

Reduction chooseReduction(bool prot, bool bs, std::string const & name)
{
    Reduction r;
    r.prot = prot, r.bs = bs;
    if (prot && name == "li10")
        r.tab = lambda_amd::kLi10, r.alph = 10;
    else if (prot && name == "murphy10")
        r.tab = lambda_amd::kMurphy10, r.alph = 10;
    else if (bs)
        r.alph = 6;
    else if (!prot)
        r.tab = lambda_amd::kDna4, r.alph = 4;
    return r;
}

// bisulfite: the reduction alternates with the frame (even: forward, odd: reverse; src/view_reduce_to_bisulfite.hpp:132-136)
std::vector<uint8_t> reduce(SeqSet const & set, Reduction const & r)
{
    std::vector<uint8_t> red(set.res.size());
    if (r.bs)
    {
        for (size_t f = 0; f < set.off.size(); ++f)
            for (uint64_t i = 0; i < set.len[f]; ++i)
                red[set.off[f] + i] = ((f & 1) ? lambda_amd::kBsRev : lambda_amd::kBsFwd)[std::min<uint8_t>(set.res[set.off[f] + i], 4)];
        return red;
    }
    uint8_t const * const tab  = r.tab;
    uint8_t const         size = r.prot ? 27 : 5;
    for (size_t i = 0; i < set.res.size(); ++i)
        red[i] = tab ? tab[set.res[i] < size ? set.res[i] : 0] : set.res[i];
    return red;
}

} // namespace
