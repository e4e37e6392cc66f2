// lambda3_main.cpp -- minimal `lambda3 searchp|searchn|searchbs` front end around liblambda_ext (SURVEY.md section 7 step 9,
// section 8f rows N2/N3): plumbing for BASELINE.json configs[0], not a port of the reference's driver.
//
//   lambda3 searchp -q queries.fasta -d db.fasta -o out.m8 [-e 1e-2] [-n 25] [--seed-length 10] [--seed-offset 5]
//                   [--devices 0,1,...] [-t THREADS] [--table gpu|host|auto] [--table-slice WORDS] [--seeding gpu|host] [--records gpu|host|auto]
//                   [--render gpu|host|auto]
//
// --render: where the records of the output are made, for every format.  host: the host writer (lx_write_records_ex for a plain
// text file; lx_render_records, the stream uploaded and compressed by lx_bgzf_compress, for .bam and *.gz: what this front end always
// did).  gpu: the records are kernels' work on the first device -- lx_write_bam_dev for .bam, lx_write_text_dev for .m8, .m9 and .sam;
// with .bam and *.gz they are compressed where they stand and only BGZF members come down; the file is byte-identical.  auto = host
// until the measurements of DESIGN.md (4.13, "BAM records on the device"; 4.14, "Text records on the device") decide otherwise.
//
// --records: where _writeRecord's sort / unique / sort / cut to -n (src/search_algo.hpp:820-882) runs.  host: lx_postprocess_records
// once, over the records of all workers (what this front end always did).  gpu: a worker's Level-2 call on a DEVICE match list
// (the passes whose seeding ran on its GPU) goes through lx_iterate_matches_dev_top, so that only the records that stay come down;
// that is legitimate because every record of a query comes out of ONE call -- the workers own disjoint ranges of reads, the exact
// pass and the half-exact pass work on disjoint queries, a bisulfite call holds both strand directions (and runs the step over its
// finished result) --; a pass whose matches stand in host memory (host seeding, LAMBDA3_HOST_LIST; reads the device declined no longer: lx_seed_queries
// appends their matches to its device list) keeps
// the host step, applied to that pass's records alone; the statistics of the parts are summed; -n 0 keeps the host step (the second
// pass searches the queries WITHOUT records).  auto: see DESIGN.md ("_writeRecord on the device") for the measurement behind it.
// LCA and the writers stay on the host, fed with the kept records; the output is byte-identical either way.
//
// --lazy-query 1 [--query-block N]: the query file block by block, in bounded memory -- the reference's batch loop with its reader
// thread behind a bounded queue (src/search.cpp:389-459, src/search_algo.hpp:374-413).  One reader takes the file as a stream
// (lx_gunzip_stream: BGZF groups on the first device, other members on its thread), parses it piece by piece
// (lx_query_blocks.hpp) and makes blocks of at most N reads (default 2^20, NOT measured yet: tools/query_blocks_bench.py; a block
// also closes at 2^30 letters): ranks, frames, reduction.  One worker per entry of --devices takes the next block and searches all of
// it as the eager path searches a worker's range -- lx_set_queries and lx_reserve for the block, the --search0 pre-pass and the
// second pass for its reads without a record, _writeRecord's cut (--records gpu | host: every record of a read comes out of its
// block), the LCA.  The main thread appends the finished blocks in their order through lx_out (--render gpu: rendered, and for
// .bam / *.gz compressed, on the first device).  At most workers + 2 blocks exist at a time; a full pipeline makes the reader wait.
// The output is byte-identical to the eager run's; the two summary lines keep their wording with counts summed over the blocks and a
// worker's times accumulated, and a third line names the blocks, the reads of the largest and the most blocks alive at once.  An
// error in block k (a malformed record) ends the run non-zero with the eager run's message; the output file then holds the blocks
// in front of k (the eager path fails before it writes).  --query-block N alone implies --lazy-query 1; --lazy-query 0 and
// --query-block 0 are the eager path.  A query file that cannot be mapped (a pipe) is held whole in memory, compressed.
//
// Inputs (-q, -d of search* and mkindex*) are FASTA or FASTQ, plain or gzip-compressed, as the reference's (fa, fq, fasta, fastq,
// fna, faa, each optionally .gz: src/search_options.hpp:157-167, src/mkindex_options.hpp:96-105); the format comes from the bytes
// (gzip magic, then ">" or "@"), not the name.  lx_gunzip decompresses: BGZF members on the first device of --devices for search*
// (mkindex*: on the host unless --table gpu), other members on the reading thread.  FASTQ qualities are read and dropped
// (src/search_algo.hpp:342); bzip2 is refused.
//
// What it mirrors from the reference, and what it does not:
//   * subcommand split and the search command line (src/lambda.cpp:30-118; src/search_options.hpp:143-816): -q, -o (format from
//     the extension, :684-710), -e, --bit-score, --percent-identity, -n, the seeding options (--seed-length/-offset/-delta[0],
//     --search0, --adaptive-seeding, --seed-half-exact), --pre-scoring[-threshold], the scoring options (-s 45|62|80 for
//     proteins, --score-match/-mismatch for nucleotides, --score-gap, --score-gap-open), the profiles (-p fast | sensitive |
//     pairs-default | pairs-sensitive: they overwrite the seeding options, :634-681), the output options (--output-columns,
//     --sam-bam-tags/-seq/-clip, --sam-with-refheader, --version-to-outputfile), -g, --input-alphabet;
//   * the thread split of realMain (src/search.cpp:379-385): one worker per entry of --devices (default: all visible devices), each
//     with its own handle -- one LocalDataHolder per thread there, one lx_handle = device + stream here --, the queries dealt to
//     them in contiguous ranges, the records concatenated in range order before _writeRecord; -t host threads (default: what
//     the machine grants) build the word table and are shared out among the workers for the seeding of their reads;
//   * searchbs (src/lambda.cpp:103; domain_t::bisulfite, src/search_options.hpp:127, :261-264, :328): four query frames
//     (strand x bisulfite duplicate), two subject frames, the 6-letter reduction of src/view_reduce_to_bisulfite.hpp for
//     seeding, both scoring schemes (src/bisulfite_scoring.hpp:67-93), iterateMatches' bisulfite branch (:1367-1379);
//   * the per-batch flow of realMain (src/search.cpp:389-459): seeding -> seedLooksPromising -> iterateMatches ->
//     writeRecords, with the three middle stages on the GPU through the C ABI;
//   * mkindexp | mkindexn | mkindexbs (src/lambda.cpp:86-88, src/mkindex_options.hpp:96-262: -d, -i with the .lba / .lta name and the
//     refusal to overwrite, -r, -g, --input-alphabet, --truncate-ids, --db-index-type, -t) and `search* -i INDEX`: the index file
//     holds what the reference's holds (the options that fix the types, ids, sequences in the translated alphabet; with -m / -x the
//     subjects' taxa and the taxonomic tree, :107-128, src/mkindex_algo.hpp:277-598: accessions of the ids joined with a plain or
//     .gz NCBI *.accession2taxid or UniProt *.dat map -- on the device under --table gpu, else on the -t host threads --, the tree
//     from nodes.dmp / names.dmp)
//     with this front end's word table in the FM-index's place -- its own format, not the reference's cereal archive; the
//     searches take the domain, the reduction and the subjects' genetic code from it and refuse an index of another domain
//     with the reference's messages (src/search.cpp:157-207);
//   * NOT the FM-index: the reference searches an index built by `lambda3 mkindexp` (fmindex-collection, absent here,
//     out of scope).  This front end answers the seeding stage's questions from a
//     sorted table of reduced words (host/lx_seeding.hpp), read from its index file (-i) or made in memory from FASTA (-d) -- with the reference's seeding semantics: Li-10 reduction,
//     exact seeds 10/5 first, then (queries without a result) half-exact seeds 11/3 with one substitution in the second
//     half, adaptive elongation, over-abundant seeds dropped, seedLooksPromising per hit (src/search_algo.hpp:426-762,
//     :1391-1457; defaults src/search_options.hpp:309-337).  Everything after seeding follows the reference too.
#include <sched.h>

#include <algorithm>
#include <array>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <functional>
#include <iostream>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "blast_stats.hpp"
#include "lambda_ext.hpp"
#include "lx_query_blocks.hpp"
#include "lx_seeding.hpp"
#include "scoring_tables.hpp"

namespace
{

struct SeqSet
{
    std::vector<std::string> ids;
    std::vector<uint8_t>     res;   // ranks, concatenated (frame-expanded for nucleotide queries)
    std::vector<uint64_t>    off, len;
    std::string              ascii; // original letters of the untranslated sequences, concatenated
    std::vector<uint64_t>    ascii_off, orig_len;
};

uint8_t aaRank(char c) // SeqAn2 AminoAcid rank (src/seqan2_to_biocpp.hpp:352-366)
{
    static auto const table = []()
    {
        std::array<uint8_t, 256> t;
        for (int ch = 0; ch < 256; ++ch)
        {
            char const * p = std::strchr(lambda_amd::kSeqanOrder, std::toupper(ch));
            t[(size_t)ch]  = (ch != 0 && p && *p) ? (uint8_t)(p - lambda_amd::kSeqanOrder) : 25; // unknown -> X
        }
        return t;
    }();
    return table[(unsigned char)c];
}

uint8_t dnaRank(char c) // BioC++ dna5 rank A,C,G,N,T (Simple-scored alphabets pass it through, :392-393)
{
    static auto const table = []()
    {
        std::array<uint8_t, 256> t;
        t.fill(3);
        t['A'] = t['a'] = 0, t['C'] = t['c'] = 1, t['G'] = t['g'] = 2, t['T'] = t['t'] = t['U'] = t['u'] = 4;
        return t;
    }();
    return table[(unsigned char)c];
}

uint8_t dnaRankSeqan(char c) // SeqAn Dna5 rank A,C,G,T,N: the bisulfite schemes are matrices over it (src/bisulfite_scoring.hpp:54-93)
{
    static auto const table = []()
    {
        std::array<uint8_t, 256> t;
        t.fill(4);
        t['A'] = t['a'] = 0, t['C'] = t['c'] = 1, t['G'] = t['g'] = 2, t['T'] = t['t'] = t['U'] = t['u'] = 3;
        return t;
    }();
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
    auto const  t0 = std::chrono::steady_clock::now();
    lx_handle * h  = nullptr;
    if (device >= 0 && lx_create(device, &h) != LX_OK)
        throw std::runtime_error(lx_last_error(nullptr));
    std::unique_ptr<lx_handle, void (*)(lx_handle *)> keepH(h, lx_destroy);
    lx_bytes *                                        out = nullptr;
    if (lx_gunzip(h, reinterpret_cast<uint8_t const *>(raw.data()), raw.size(), &out) != LX_OK)
        throw std::runtime_error(path + ": " + (h ? lx_last_error(h) : lx_last_output_error()));
    std::unique_ptr<lx_bytes, void (*)(lx_bytes *)> keep(out, lx_bytes_free);
    r.text.assign(reinterpret_cast<char const *>(lx_bytes_data(out)), lx_bytes_size(out));
    r.msGunzip = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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

// translate = six protein frames per nucleotide sequence (BLASTX queries: qryNumFrames = 6, translate_join)
// bsFrames: 0 = none; 1 = bisulfite subjects (every sequence twice: views::duplicate, src/shared_definitions.hpp:249-250);
// 2 = bisulfite queries (strand, strand, reverse complement, reverse complement: add_reverse_complement | duplicate, :260-261)
// one record into the set: its letters, ranks and frames (`cur` is used up)
void addRecord(SeqSet & out, std::string const & id, std::string & cur, bool protein, bool addRevComp, bool translate, int geneticCode, int bsFrames)
{
    {
        out.ids.push_back(id);
        out.ascii_off.push_back(out.ascii.size());
        out.orig_len.push_back(cur.size());
        out.ascii += cur;
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
}

void readFasta(std::string const & text, std::string const & path, bool protein, bool addRevComp, SeqSet & out, bool translate = false,
               int geneticCode = 1, int bsFrames = 0)
{
    forEachRecord(text, path,
                  [&](std::string const & id, std::string & letters)
                  {
                      addRecord(out, id, letters, protein, addRevComp, translate, geneticCode, bsFrames);
                      return true;
                  });
}

struct Options
{
    std::string cmd, query, db, output = "output.m8";
    double      maxEValue   = 1e-2; // src/search_options.hpp:97
    uint64_t    maxMatches  = 25;   // :99
    int         seedLength  = 0, seedOffset = 0, seedDelta = 1;     // searchOpts  (:309-337)
    int         seedLength0 = 0, seedOffset0 = 0;                   // searchOpts0: the exact pre-search
    bool        search0 = true;       // iterativeSearch (:107, --search0)
    bool        adaptive = true, halfExact = true; // :75-76
    std::string reduction = "li10";   // mkindexp -r (src/mkindex_options.hpp:182-205)
    int         geneticCode = 1;      // :170
    int         preScoring  = 2;    // :104
    double      preScoringThresh = 2.0;
    int         idCutOff    = 0;
    int         minBitScore = -1;   // :96, --bit-score
    int         seedDelta0  = 0;    // searchOpts0.maxSeedDist (:314, :322, :331)
    std::string profile     = "none"; // :107, -p
    int         scoringMethod = 62; // :89, -s (searchp)
    int         match = 2, misMatch = -3; // :93-94 (searchn / searchbs)
    int         gapOpen = -11, gapExtend = -1; // :91-92; -5 / -2 outside the protein domain (:293-294)
    // output (:224-379): columns of .m8 / .m9, tags / sequence / clipping of .sam
    std::string outputColumns = "std", samTags = "AS NM ae ai qf", samSeq = "uniq", samClip = "hard";
    bool        samWithRefHeader = false, versionToOutput = true;
    std::string commandLine;
    std::vector<int> devices;         // --devices (default: every visible device)
    std::string table       = "auto"; // --table gpu | host | auto: where the word table is made (auto: search* on the GPU, mkindex* on the host)
    uint64_t    tableSlice  = 0;      // --table-slice N: the GPU makes the table in slices of at most N words (0: one sort where it can, slices of 2^30 where it cannot)
    std::string seeding     = "gpu";  // --seeding gpu | host: where search() runs (lx_seed_queries on the worker's handle -- one lane per read, reads
                                      // the device declines are finished on the host threads inside the call --, or on the -t threads)
    std::string render      = "auto"; // --render gpu | host | auto: where the records of the output are made (the header comment)
    std::string records     = "auto"; // --records gpu | host | auto: where _writeRecord's sort / unique / sort / cut runs (the header comment)
    int         threads     = 0;    // -t host threads for the word table and the seeding (default: what the machine grants)
    bool        lazyQuery   = false; // --lazy-query 1: the query file block by block (the header comment)
    uint64_t    queryBlock  = 0;     // --query-block N: at most N reads per block; given and > 0, it implies --lazy-query 1
    bool        queryBlockGiven = false;
    // mkindex* (src/mkindex_options.hpp:96-262): -d the database (FASTA), -i the index file to write
    std::string index;                // -i of mkindex* (default: DATABASE.lba, :132, :249-250)
    std::string dbIndexType = "fm";   // --db-index-type fm | bifm (:157-165; recorded, the word table answers both)
    bool        truncateIds = false;  // --truncate-ids (:167-173)
    bool        geneticCodeGiven = false;
    std::string accTaxMap, taxDumpDir; // -m / -x of mkindex* (:107-128)
    std::string qryAlphabet = "auto"; // searchp: "aminoacid" = BLASTP, "dna5" = BLASTX, "auto" = decide from the letters
    std::string dbAlphabet  = "auto"; // searchp: "dna5" = six-frame translated subjects (TBLASTN / TBLASTX)
};

// the reference lets BioC++ detect the query alphabet (src/search_options.hpp); here: nucleotide if >= 90 % of the
// letters of the first sequences are ACGTUN
bool looksLikeDna(std::string const & text, std::string const & path)
{
    uint64_t nuc = 0, all = 0;
    forEachRecord(text, path,
                  [&](std::string const &, std::string const & letters)
                  {
                      for (char c : letters)
                          nuc += std::strchr("ACGTUNacgtun", c) != nullptr;
                      all += letters.size();
                      return all < 100000;
                  });
    return all > 0 && nuc * 10 >= all * 9;
}

// ---- --lazy-query: the query file as a stream of pieces (lx_gunzip_stream: decompressed where needed, BGZF groups on `device`)
// and of records (lx_query_blocks::RecordParser).  The first two pieces are taken at once: the bzip2 refusal and the alphabet come
// from the first, and whether it is the whole file from the second.
struct QueryStream
{
    std::string                                       path;
    std::unique_ptr<lx_handle, void (*)(lx_handle *)> h{nullptr, lx_destroy};
    lx_gunzip_stream *                                s = nullptr;
    std::vector<lx_bytes *>                           ahead; // pieces taken and not parsed yet
    bool                                              ended = false;
    lx_query_blocks::RecordParser                     parser;

    QueryStream(std::string const & path_, int device) : path(path_), parser(path_)
    {
        lx_handle * raw = nullptr;
        if (device >= 0 && lx_create(device, &raw) != LX_OK)
            throw std::runtime_error(lx_last_error(nullptr));
        h.reset(raw);
        if (lx_gunzip_stream_open(raw, path.c_str(), kPiece, &s) != LX_OK)
        {
            std::string const why = raw ? lx_last_error(raw) : lx_last_output_error();
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
    }
    // looksLikeDna over the first piece (all of the file a small file has)
    bool looksLikeDna() const
    {
        uint64_t nuc = 0, all = 0;
        auto     f   = [&](std::string const &, std::string const & letters)
        {
            for (char c : letters)
                nuc += std::strchr("ACGTUNacgtun", c) != nullptr;
            all += letters.size();
            return all < 100000;
        };
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
        return all > 0 && nuc * 10 >= all * 9;
    }
    // f(id, letters) per record from where the last call stopped, until f returns false (true: more may follow) or the file ends
    // (false).  A piece is parsed whole, so records f has not asked for wait in `kept`.
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
            keptAt = 0;
            if (malformed) // (the records in front of it have been handed out)
                std::rethrow_exception(malformed);
            auto keep = [&](std::string const & id, std::string & letters)
            {
                kept.emplace_back(id, std::string());
                kept.back().second.swap(letters);
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
    std::vector<std::pair<std::string, std::string>> kept;
    size_t                                           keptAt = 0;
    uint64_t                                         pieceAt = 0; // bytes of ahead[0] the parser has
    bool                                             finished = false;
    std::exception_ptr                               malformed; // the parser's error, kept until the records in front of it are out
    static constexpr uint64_t kPiece = 8ull << 20, kSlice = 1ull << 20; // text per piece of the stream; per call of the parser
};

static int outputFormat(std::string const & path, bool & gz);

Options parse(int argc, char ** argv)
{
    Options o;
    if (argc < 2)
        throw std::runtime_error("usage: lambda3 searchp|searchn|searchbs -q QUERY.{fa,fq,fasta,fastq,fna,faa}[.gz] (-i DB.lba | -d DB.fasta[.gz]) -o OUT.{m8,m9,sam,bam,m8.gz,m9.gz,sam.gz} [-e EVALUE] [-n N] "
                                 "[--devices 0,1,...] [-t THREADS]\n                 [--lazy-query 1] [--query-block N]   search the query file block by block in bounded memory: at most N reads per block\n"
                                 "                 (default 1048576, not measured yet; a block also closes at 2^30 letters; a query read from a pipe is held whole, compressed)\n       lambda3 mkindexp|mkindexn|mkindexbs -d DB.{fa,fq,fasta,fastq,fna,faa}[.gz] [-i DB.lba] [-r li10|murphy10|none] [-g CODE] [-t THREADS]\n                 [-m MAP.{accession2taxid,dat}[.gz] [-x TAXDUMP_DIR]]");
    o.cmd = argv[1];
    bool const mk = o.cmd == "mkindexp" || o.cmd == "mkindexn" || o.cmd == "mkindexbs";
    if (o.cmd != "searchp" && o.cmd != "searchn" && o.cmd != "searchbs" && !mk)
        throw std::runtime_error("unknown subcommand '" + o.cmd + "' (searchp, searchn, searchbs, mkindexp, mkindexn, mkindexbs: src/lambda.cpp:86-88)");
    bool const prot = o.cmd == "searchp" || o.cmd == "mkindexp", bs = o.cmd == "searchbs" || o.cmd == "mkindexbs";
    // per-domain defaults, src/search_options.hpp:309-337 (bisulfite: :261-264, :328-336)
    o.seedLength0      = prot ? 10 : bs ? 17 : 14;
    o.seedOffset0      = prot ? 5 : bs ? 10 : 9;
    o.seedLength       = prot ? 11 : bs ? 17 : 14;
    o.seedOffset       = prot ? 3 : bs ? 10 : 7;
    o.preScoringThresh = prot ? 2.0 : bs ? 1.5 : 1.4;
    if (bs)
        o.maxEValue = 1e-9;
    if (!prot)
        o.gapOpen = -5, o.gapExtend = -2;
    for (int i = 1; i < argc; ++i) // (the reference keeps the command line from the subcommand on, :106-109)
        o.commandLine += std::string(i > 1 ? " " : "") + argv[i];
    auto onOff = [](std::string const & v) // sharg's bool options take 0 / 1 / true / false; the help pages write ON / OFF
    {
        std::string u;
        for (char c : v)
            u += (char)std::toupper((unsigned char)c);
        if (u == "1" || u == "TRUE" || u == "ON")
            return true;
        if (u == "0" || u == "FALSE" || u == "OFF")
            return false;
        throw std::runtime_error("expected 0 / 1 / true / false / ON / OFF, got " + v);
    };
    auto inRange = [](std::string const & name, double v, double lo, double hi)
    {
        if (v < lo || v > hi)
            throw std::runtime_error("Value " + std::to_string(v) + " of option " + name + " is not in range [" + std::to_string(lo) + "," + std::to_string(hi) + "].");
    };
    for (int i = 2; i < argc; ++i)
    {
        std::string a = argv[i];
        auto        val = [&]() -> std::string
        {
            if (i + 1 >= argc)
                throw std::runtime_error("missing value for " + a);
            return argv[++i];
        };
        if (a == "-q" || a == "--query")
            o.query = val();
        else if (mk && (a == "-i" || a == "--index"))
            o.index = val();
        else if (mk && a == "--db-index-type")
        {
            o.dbIndexType = val();
            if (o.dbIndexType != "fm" && o.dbIndexType != "bifm")
                throw std::runtime_error("--db-index-type takes fm or bifm");
        }
        else if (mk && a == "--truncate-ids")
            o.truncateIds = true;
        else if (mk && (a == "-m" || a == "--acc-tax-map"))
            o.accTaxMap = val();
        else if (mk && (a == "-x" || a == "--tax-dump-dir"))
            o.taxDumpDir = val();
        else if (a == "-d" || a == "--database" || a == "-i" || a == "--index")
            o.db = val();
        else if (a == "-o" || a == "--output")
            o.output = val();
        else if (a == "-e" || a == "--e-value")
            o.maxEValue = std::stod(val());
        else if (a == "-n" || a == "--num-matches")
            o.maxMatches = std::stoull(val());
        else if (a == "--seed-length")
            o.seedLength = std::stoi(val());
        else if (a == "--seed-offset")
            o.seedOffset = std::stoi(val());
        else if (a == "--seed-delta")
            o.seedDelta = std::stoi(val());
        else if (a == "--seed-length0")
            o.seedLength0 = std::stoi(val());
        else if (a == "--seed-offset0")
            o.seedOffset0 = std::stoi(val());
        else if (a == "--seed-delta0")
            o.seedDelta0 = std::stoi(val());
        else if (a == "--search0")
            o.search0 = onOff(val());
        else if (a == "--adaptive-seeding")
            o.adaptive = onOff(val());
        else if (a == "--seed-half-exact")
            o.halfExact = onOff(val());
        else if (a == "--pre-scoring") // (the validator's range is 1..10, :488-497; 0 = off is what the description offers)
        {
            o.preScoring = std::stoi(val());
            inRange(a, o.preScoring, 0, 10);
        }
        else if (a == "--pre-scoring-threshold")
        {
            o.preScoringThresh = std::stod(val());
            inRange(a, o.preScoringThresh, 0, 20);
        }
        else if (a == "--bit-score")
        {
            o.minBitScore = std::stoi(val());
            inRange(a, o.minBitScore, -1, 1000);
        }
        else if ((a == "-s" || a == "--scoring-scheme") && prot) // :510-521
        {
            o.scoringMethod = std::stoi(val());
            if (o.scoringMethod != 45 && o.scoringMethod != 62 && o.scoringMethod != 80)
                throw std::runtime_error("--scoring-scheme takes 45, 62 or 80");
        }
        else if (a == "--score-match" && !prot) // :523-540
            o.match = std::stoi(val());
        else if (a == "--score-mismatch" && !prot)
            o.misMatch = std::stoi(val());
        else if (a == "--score-gap")
            o.gapExtend = std::stoi(val());
        else if (a == "--score-gap-open")
            o.gapOpen = std::stoi(val());
        else if (a == "-p" || a == "--profile")
        {
            o.profile = val();
            if (o.profile != "none" && o.profile != "fast" && o.profile != "sensitive" && o.profile != "pairs-default" && o.profile != "pairs-sensitive")
                throw std::runtime_error("--profile takes none, fast, sensitive, pairs-default or pairs-sensitive");
        }
        else if (a == "--output-columns")
            o.outputColumns = val();
        else if (a == "--sam-bam-tags")
            o.samTags = val();
        else if (a == "--sam-bam-seq")
        {
            o.samSeq = val();
            if (o.samSeq != "always" && o.samSeq != "uniq" && o.samSeq != "never")
                throw std::runtime_error("--sam-bam-seq takes always, uniq or never");
        }
        else if (a == "--sam-bam-clip")
        {
            o.samClip = val();
            if (o.samClip != "hard" && o.samClip != "soft")
                throw std::runtime_error("--sam-bam-clip takes hard or soft");
        }
        else if (a == "--sam-with-refheader")
            o.samWithRefHeader = onOff(val());
        else if (a == "--version-to-outputfile")
            o.versionToOutput = onOff(val());
        else if (a == "-r" || a == "--alphabet-reduction")
        {
            o.reduction = val();
            if (o.reduction != "none" && o.reduction != "murphy10" && o.reduction != "li10")
                throw std::runtime_error("--alphabet-reduction takes none, murphy10 or li10");
        }
        else if (a == "-g" || a == "--genetic-code")
        {
            o.geneticCode      = std::stoi(val());
            o.geneticCodeGiven = true;
        }
        else if (a == "--percent-identity")
            o.idCutOff = std::stoi(val());
        else if (a == "--device" || a == "--devices")
        {
            o.devices.clear();
            std::string const v = val();
            for (size_t at = 0; at <= v.size();)
            {
                size_t const e = std::min(v.find(',', at), v.size());
                if (e > at)
                    o.devices.push_back(std::stoi(v.substr(at, e - at)));
                at = e + 1;
            }
            if (o.devices.empty())
                throw std::runtime_error("--devices takes a comma-separated list of device numbers");
        }
        else if (a == "-t" || a == "--threads")
            o.threads = std::stoi(val());
        else if (a == "--table")
        {
            o.table = val();
            if (o.table != "gpu" && o.table != "host" && o.table != "auto")
                throw std::runtime_error("--table takes gpu, host or auto");
        }
        else if (a == "--table-slice") // (LX_OPT_INDEX_SLICE_WORDS: the device build in slices of the key space)
        {
            std::string const v = val();
            bool              ok = !v.empty() && v.size() <= 18 && std::all_of(v.begin(), v.end(), [](char c) { return c >= '0' && c <= '9'; });
            o.tableSlice         = ok ? std::stoull(v) : 0;
            if (o.tableSlice == 0)
                throw std::runtime_error("--table-slice takes a number of words (at least 1): the most one slice of the GPU's word table build may hold");
        }
        else if (a == "--records")
        {
            o.records = val();
            if (o.records != "gpu" && o.records != "host" && o.records != "auto")
                throw std::runtime_error("--records takes gpu, host or auto");
        }
        else if (a == "--render")
        {
            o.render = val();
            if (o.render != "gpu" && o.render != "host" && o.render != "auto")
                throw std::runtime_error("--render takes gpu, host or auto");
        }
        else if (a == "--seeding")
        {
            o.seeding = val();
            if (o.seeding != "host" && o.seeding != "gpu")
                throw std::runtime_error("--seeding takes host or gpu");
        }
        else if (a == "--db-alphabet")
        {
            o.dbAlphabet = val();
            if (o.dbAlphabet != "auto" && o.dbAlphabet != "dna5" && o.dbAlphabet != "aminoacid")
                throw std::runtime_error("--db-alphabet takes auto, dna5 or aminoacid");
        }
        else if (a == "-a" || a == "--query-alphabet" || a == "--input-alphabet") // (the reference's name is --input-alphabet, :172-185)
        {
            std::string & which = mk ? o.dbAlphabet : o.qryAlphabet; // (mkindexp: the database's, src/mkindex_options.hpp:189-197)
            which               = val();
            if (which != "auto" && which != "dna5" && which != "aminoacid")
                throw std::runtime_error("--input-alphabet takes auto, dna5 or aminoacid");
        }
        else if (a == "--lazy-query") // (the reference's switch: the query file in blocks, src/search.cpp:389-459)
            o.lazyQuery = onOff(val());
        else if (a == "--query-block") // (this front end's: reads per block; giving it implies lazy loading, 0 = the eager path)
        {
            long long const v = std::stoll(val());
            if (v < 0)
                throw std::runtime_error("--query-block takes a number of reads (0 = read the whole file at once)");
            o.queryBlock      = (uint64_t)v;
            o.queryBlockGiven = true;
        }
        else if (a == "-v" || a == "--verbosity")
            (void)val(); // accepted for command-line compatibility, no effect here
        else
            throw std::runtime_error("unknown option " + a);
    }
    if (mk)
    {
        if (o.db.empty())
            throw std::runtime_error("-d is required");
        if (o.index.empty())
            o.index = o.db + ".lba"; // :249-250
        auto ends = [&](char const * suf)
        { return o.index.size() >= std::strlen(suf) && o.index.compare(o.index.size() - std::strlen(suf), std::string::npos, suf) == 0; };
        if (!ends(".lba") && !ends(".lta")) // :133, :145
            throw std::runtime_error("the index file name must end in .lba or .lta");
        if (!o.taxDumpDir.empty() && o.accTaxMap.empty()) // :256-264
            throw std::runtime_error("There is no point in including a taxonomic tree in the index, if you don't also include taxonomic IDs for your sequences.");
        if (!o.accTaxMap.empty())
        {
            auto mapEnds = [&](char const * suf)
            { return o.accTaxMap.size() >= std::strlen(suf) && o.accTaxMap.compare(o.accTaxMap.size() - std::strlen(suf), std::string::npos, suf) == 0; };
            if (mapEnds(".accession2taxid.bz2") || mapEnds(".dat.bz2"))
                throw std::runtime_error(o.accTaxMap + ": bzip2-compressed input is not supported (decompress it, or recompress it with gzip or bgzip)");
            if (!mapEnds(".accession2taxid") && !mapEnds(".accession2taxid.gz") && !mapEnds(".dat") && !mapEnds(".dat.gz"))
                throw std::runtime_error("-m " + o.accTaxMap + ": the accession-to-taxonomy map must be named *.accession2taxid or *.dat, optionally .gz");
        }
        if (std::ifstream(o.index).good()) // :252-256
            throw std::runtime_error("ERROR: An output file already exists at " + o.index + "\n       Remove it, or choose a different location.");
        return o;
    }
    if (o.query.empty() || o.db.empty())
        throw std::runtime_error("-q and -d (a FASTA file) or -i (an index made by lambda3 mkindex*) are required");
    // "Setting a profile other than none always overwrites manually given command line arguments" (:563-566, applied :634-681)
    if (o.profile == "fast")
    {
        if (!prot)
        {
            o.search0   = false;
            o.seedDelta = 0;
            if (!bs)
                o.seedOffset = 9;
        }
        else
            o.seedLength0 = 12, o.seedOffset0 = 8, o.seedLength = 10, o.seedOffset = 5, o.seedDelta = 0;
    }
    else if (o.profile != "none") // sensitive, pairs-default, pairs-sensitive
    {
        if (prot)
            o.seedLength0 = 9, o.seedOffset0 = 4, o.seedLength = 8, o.seedOffset = 3, o.preScoring = 3, o.preScoringThresh = 1.9;
        else if (bs)
            o.seedLength0 = 16, o.seedOffset0 = 8, o.seedLength = 15, o.seedOffset = 10;
        else
            o.seedOffset0 = 3, o.seedOffset = 3;
        if (o.profile.rfind("pairs", 0) == 0)
            o.search0 = false;
        if (o.profile == "pairs-sensitive")
            --o.seedLength;
    }
    if (o.seedLength < 2 || o.seedLength0 < 2 || o.seedOffset < 1 || o.seedOffset0 < 1 || o.seedDelta < 0 || o.seedDelta > 3 || o.seedDelta0 < 0 ||
        o.seedDelta0 > 5)
        throw std::runtime_error("seed length / offset / delta out of range");
    {
        // the output format and what the writers are asked for, before anything is read or searched (:684-816: the reference fails
        // while it parses its options)
        bool      gz  = false;
        int const fmt = outputFormat(o.output, gz);
        lx_output_options oo;
        lx_output_options_default(&oo);
        oo.columns  = o.outputColumns.c_str();
        oo.sam_tags = o.samTags.c_str();
        if (lx_check_output_options(fmt, &oo) != LX_OK)
            throw std::runtime_error(lx_last_output_error());
    }
    return o;
}

// The output format from the file name (src/search_options.hpp:684-710): .m8, .m9, .sam or .bam; the text formats also BGZF-
// compressed (.gz).  .m0 (the pairwise report), .bz2 and .bam.gz are refused.
static char const * const kFormatMessage =
    "output format is chosen by the extension: .m8, .m9, .sam or .bam, the first three optionally with .gz (.m0, .bz2 and .bam.gz are not supported)";
static int outputFormat(std::string const & path, bool & gz)
{
    auto ends = [&](std::string const & p, char const * suf)
    { return p.size() >= std::strlen(suf) && p.compare(p.size() - std::strlen(suf), std::string::npos, suf) == 0; };
    gz                 = ends(path, ".gz");
    std::string const base = gz ? path.substr(0, path.size() - 3) : path;
    if (ends(base, ".m9"))
        return LX_OUT_BLAST_TAB_COMMENTS;
    if (ends(base, ".sam"))
        return LX_OUT_SAM;
    if (ends(base, ".m8"))
        return LX_OUT_BLAST_TAB;
    if (ends(base, ".bam") && !gz)
        return LX_OUT_BAM;
    throw std::runtime_error(kFormatMessage);
}

// ---- the index file of `lambda3 mkindex*`.  It holds what the reference's index_file holds (src/shared_definitions.hpp:343-379:
// the options that fix the types, the ids, the sequences in the translated alphabet, the taxonomy when -m was given), and this front end's
// word table in place of the FM-index.  NOT the reference's on-disk format: that is a cereal archive of fmindex-collection
// objects, neither of which is available here; a file of the reference is recognised by the missing magic and refused.
constexpr char kIndexMagic[8] = {'L', 'X', 'I', 'N', 'D', 'E', 'X', '1'};
// AlphabetEnum / DbIndexType with the reference's numbering (src/shared_definitions.hpp:62-66, :127-136)
enum : uint8_t { kAlphUndefined = 0, kAlphDna3Bs = 1, kAlphDna4 = 2, kAlphDna5 = 3, kAlphAminoAcid = 4, kAlphMurphy10 = 5, kAlphLi10 = 6 };
struct IndexFileOptions // index_file_options, :318-341
{
    uint64_t generation = 0; // supportedIndexGeneration, :316
    uint8_t  indexType = 0, origAlph = kAlphUndefined, transAlph = kAlphUndefined, redAlph = kAlphUndefined, geneticCode = 1, pad[3] = {0, 0, 0};
};
char const * alphName(uint8_t a) // _alphabetEnumToName, :138-160
{
    static char const * const names[] = {"UNDEFINED", "dna3bs", "dna4", "dna5", "aminoacid", "murphy10", "li10"};
    return a < 7 ? names[a] : "?";
}

bool isIndexFile(std::string const & path)
{
    std::ifstream f(path, std::ios::binary);
    char          m[8] = {0};
    return f.read(m, 8) && std::memcmp(m, kIndexMagic, 8) == 0;
}

// The taxonomy of an index (mkindex* -m / -x; the reference's indexFile.sTaxIds, taxonParentIDs, taxonHeights, taxonNames).
struct IndexTaxonomy
{
    bool                     has = false;     // the index holds subject taxa
    std::vector<uint64_t>    off;             // n_s + 1
    std::vector<uint32_t>    ids;
    bool                     hasTree = false; // ... and the tree
    std::vector<uint32_t>    parents, heights;
    std::vector<std::string> names;
};
constexpr char kTaxonMagic[8] = {'L', 'X', 'T', 'A', 'X', 'O', 'N', '1'};

// The file, in this order (integers little-endian, as the machine writes them):
//   "LXINDEX1"; IndexFileOptions (16 bytes); u64 n ids, then per id u64 length + bytes; u64 n frames, u64 off[n], u64 len[n];
//   u64 n, u64 orig_len[n]; u64 n residues + the residues; the word table (ReducedIndex::save).
//   Optional, only in an index built with -m -- an index without it ends with the word table, as before the section existed:
//   "LXTAXON1"; u64 n_s; u64 s_tax_off[n_s + 1]; u32 s_tax_ids[s_tax_off[n_s]] (subject s's taxa, in the map's order);
//   u64 has_tree (0 or 1); if 1: u64 n_taxa, u32 parents[n_taxa], u32 heights[n_taxa], u32 name_len[n_taxa], then the names'
//   bytes one after another (no terminators; "" for the taxa the tree does not keep).
void writeIndexFile(std::string const & path, IndexFileOptions const & io, SeqSet const & db, lx_index const * ix, IndexTaxonomy const & tax)
{
    lx_bytes * table = nullptr; // (lx_index_save writes ReducedIndex::save's bytes)
    if (lx_index_save(ix, &table) != LX_OK)
        throw std::runtime_error(lx_last_output_error());
    std::unique_ptr<lx_bytes, void (*)(lx_bytes *)> keepTable(table, lx_bytes_free);
    FILE * f = std::fopen(path.c_str(), "wb");
    if (!f)
        throw std::runtime_error("cannot write " + path);
    bool ok    = true;
    auto write = [&](void const * p, size_t bytes) { ok = ok && (bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes); };
    auto u64   = [&](uint64_t v) { write(&v, sizeof(v)); };
    write(kIndexMagic, 8);
    write(&io, sizeof(io));
    u64(db.ids.size());
    for (std::string const & id : db.ids)
    {
        u64(id.size());
        write(id.data(), id.size());
    }
    u64(db.off.size());
    write(db.off.data(), db.off.size() * sizeof(uint64_t));
    write(db.len.data(), db.len.size() * sizeof(uint64_t));
    u64(db.orig_len.size());
    write(db.orig_len.data(), db.orig_len.size() * sizeof(uint64_t));
    u64(db.res.size());
    write(db.res.data(), db.res.size());
    write(lx_bytes_data(table), lx_bytes_size(table));
    if (tax.has)
    {
        write(kTaxonMagic, 8);
        u64(tax.off.size() - 1);
        write(tax.off.data(), tax.off.size() * sizeof(uint64_t));
        write(tax.ids.data(), tax.ids.size() * sizeof(uint32_t));
        u64(tax.hasTree ? 1 : 0);
        if (tax.hasTree)
        {
            u64(tax.parents.size());
            write(tax.parents.data(), tax.parents.size() * sizeof(uint32_t));
            write(tax.heights.data(), tax.heights.size() * sizeof(uint32_t));
            std::vector<uint32_t> lens;
            for (std::string const & n : tax.names)
                lens.push_back((uint32_t)n.size());
            write(lens.data(), lens.size() * sizeof(uint32_t));
            for (std::string const & n : tax.names)
                write(n.data(), n.size());
        }
    }
    ok = (std::fclose(f) == 0) && ok;
    if (!ok)
    {
        std::remove(path.c_str());
        throw std::runtime_error("error while writing " + path);
    }
}

// everything but the word table (which wants the reduced residues first); the file stays open in *fp
void readIndexHead(std::string const & path, IndexFileOptions & io, SeqSet & db, FILE ** fp)
{
    FILE * f = std::fopen(path.c_str(), "rb");
    if (!f)
        throw std::runtime_error("cannot open " + path);
    auto bad = [&](char const * what) -> std::runtime_error
    {
        std::fclose(f);
        return std::runtime_error("index file " + path + ": " + what);
    };
    auto read = [&](void * p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; };
    char m[8];
    if (!read(m, 8) || std::memcmp(m, kIndexMagic, 8) != 0)
        throw bad("not an index of this front end (an index of the reference -- a cereal archive of an fmindex-collection FM-index -- cannot be "
                  "read here: run lambda3 mkindexp|mkindexn|mkindexbs on the FASTA file)");
    if (!read(&io, sizeof(io)))
        throw bad("truncated");
    if (io.generation != 0) // :316 "bump this on incompatible changes"; src/search.cpp readIndexOptions
        throw bad("unsupported index generation");
    uint64_t n = 0;
    auto     count = [&](uint64_t limit) -> uint64_t
    {
        uint64_t v = 0;
        if (!read(&v, sizeof(v)) || v > limit)
            throw bad("truncated or corrupt");
        return v;
    };
    n = count(1ull << 40);
    db.ids.resize(n);
    for (std::string & id : db.ids)
    {
        id.resize(count(1ull << 24));
        if (!read(id.data(), id.size()))
            throw bad("truncated");
    }
    n = count(1ull << 40);
    db.off.resize(n);
    db.len.resize(n);
    if (!read(db.off.data(), n * sizeof(uint64_t)) || !read(db.len.data(), n * sizeof(uint64_t)))
        throw bad("truncated");
    n = count(1ull << 40);
    db.orig_len.resize(n);
    if (!read(db.orig_len.data(), n * sizeof(uint64_t)))
        throw bad("truncated");
    n = count(1ull << 46);
    db.res.resize(n);
    if (!read(db.res.data(), n))
        throw bad("truncated");
    if (db.ids.empty() || db.orig_len.size() != db.ids.size() || db.off.empty() || db.off.size() % db.ids.size() != 0)
        throw bad("inconsistent sequence tables");
    for (size_t i = 0; i < db.off.size(); ++i)
        if (db.len[i] > db.res.size() || db.off[i] > db.res.size() - db.len[i])
            throw bad("a sequence lies outside the residues");
    {
        // the residues index the scoring and reduction tables: none beyond the translated alphabet (aa27: 27 ranks, dna5: 5)
        unsigned const size = io.transAlph == kAlphAminoAcid ? 27u : io.transAlph == kAlphDna5 ? 5u : 0u;
        uint8_t        top  = 0;
        for (uint8_t r : db.res)
            top = std::max(top, r);
        if (size == 0 || (!db.res.empty() && top >= size))
            throw bad("residues outside the index's alphabet");
    }
    *fp = f;
}

// the optional taxonomy section after the word table (writeIndexFile); f stands right behind the word table
void readIndexTaxonomy(std::string const & path, FILE * f, uint64_t nSubjects, IndexTaxonomy & tax)
{
    auto read = [&](void * p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; };
    auto bad  = [&](char const * what) { return std::runtime_error("index file " + path + ": taxonomy section: " + what); };
    char m[8];
    size_t const got = std::fread(m, 1, 8, f);
    if (got == 0)
        return; // (no section: an index built without -m)
    if (got != 8 || std::memcmp(m, kTaxonMagic, 8) != 0)
        throw bad("unknown data after the word table");
    auto count = [&](uint64_t limit) -> uint64_t
    {
        uint64_t v = 0;
        if (!read(&v, sizeof(v)) || v > limit)
            throw bad("truncated or corrupt");
        return v;
    };
    if (count(1ull << 40) != nSubjects)
        throw bad("its subject count differs from the index's");
    tax.off.resize(nSubjects + 1);
    if (!read(tax.off.data(), tax.off.size() * sizeof(uint64_t)))
        throw bad("truncated");
    for (uint64_t s = 0; s < nSubjects; ++s)
        if (tax.off[s + 1] < tax.off[s] || tax.off[0] != 0)
            throw bad("corrupt subject lists");
    if (tax.off.back() > (1ull << 40))
        throw bad("corrupt subject lists");
    tax.ids.resize(tax.off.back());
    if (!read(tax.ids.data(), tax.ids.size() * sizeof(uint32_t)))
        throw bad("truncated");
    tax.has     = true;
    tax.hasTree = count(1) == 1;
    if (!tax.hasTree)
        return;
    uint64_t const n = count(1ull << 33);
    tax.parents.resize(n);
    tax.heights.resize(n);
    std::vector<uint32_t> lens(n);
    if (!read(tax.parents.data(), n * sizeof(uint32_t)) || !read(tax.heights.data(), n * sizeof(uint32_t)) || !read(lens.data(), n * sizeof(uint32_t)))
        throw bad("truncated");
    tax.names.resize(n);
    for (uint64_t t = 0; t < n; ++t)
    {
        tax.names[t].resize(lens[t]);
        if (!read(tax.names[t].data(), lens[t]))
            throw bad("truncated");
    }
}

// The taxonomy of mkindex -m [-x]: the ids' accessions joined with the map (lx_taxmap_*: on the device of `h`, else on `threads` host
// threads), then the tree from the taxdump (lx_taxonomy_build).  Progress and the reference's counts go to stderr.
void buildIndexTaxonomy(std::string const & map, std::string const & dumpDir, std::vector<std::string> const & ids, lx_handle * h,
                        unsigned threads, IndexTaxonomy & tax, double & msJoin, float & msKernel)
{
    auto const t0 = std::chrono::steady_clock::now();
    auto ends = [&](char const * suf) { return map.size() >= std::strlen(suf) && map.compare(map.size() - std::strlen(suf), std::string::npos, suf) == 0; };
    bool const ncbi = ends(".accession2taxid") || ends(".accession2taxid.gz"); // (else *.dat[.gz]: parse() admits nothing else)
    std::string blob;
    std::vector<uint64_t> off{0};
    for (std::string const & id : ids)
    {
        blob += id;
        off.push_back(blob.size());
    }
    lx_taxmap * tm = nullptr;
    if (lx_taxmap_create(h, ncbi ? LX_TAXMAP_NCBI : LX_TAXMAP_UNIPROT, reinterpret_cast<uint8_t const *>(blob.data()), off.data(), ids.size(), 0,
                         threads, &tm) != LX_OK)
        throw std::runtime_error(h ? lx_last_error(h) : lx_last_output_error());
    std::unique_ptr<lx_taxmap, void (*)(lx_taxmap *)> keep(tm, lx_taxmap_destroy);
    auto check = [&](int rc)
    {
        if (rc != LX_OK)
            throw std::runtime_error("-m " + map + ": " + (h ? lx_last_error(h) : lx_last_output_error()));
    };
    std::FILE * f = std::fopen(map.c_str(), "rb");
    if (!f)
        throw std::runtime_error("cannot open " + map);
    std::unique_ptr<std::FILE, int (*)(std::FILE *)> keepF(f, std::fclose);
    std::vector<char> buf(64u << 20);
    size_t got = std::fread(buf.data(), 1, buf.size(), f);
    if (got >= 2 && (uint8_t)buf[0] == 0x1f && (uint8_t)buf[1] == 0x8b)
    {
        // a .gz map is decompressed whole (as -d is), then fed in pieces
        std::string raw(buf.data(), got);
        for (size_t k; (k = std::fread(buf.data(), 1, buf.size(), f)) > 0;)
            raw.append(buf.data(), k);
        lx_bytes * text = nullptr;
        if (lx_gunzip(h, reinterpret_cast<uint8_t const *>(raw.data()), raw.size(), &text) != LX_OK)
            throw std::runtime_error(map + ": " + (h ? lx_last_error(h) : lx_last_output_error()));
        std::unique_ptr<lx_bytes, void (*)(lx_bytes *)> keepT(text, lx_bytes_free);
        std::string().swap(raw);
        uint8_t const * p = lx_bytes_data(text);
        for (uint64_t at = 0, n = lx_bytes_size(text); at < n; at += buf.size())
            check(lx_taxmap_feed(tm, p + at, std::min<uint64_t>(buf.size(), n - at)));
    }
    else
    {
        // a plain map is read and fed in pieces, never whole
        for (; got > 0; got = std::fread(buf.data(), 1, buf.size(), f))
            check(lx_taxmap_feed(tm, reinterpret_cast<uint8_t const *>(buf.data()), got));
    }
    if (std::ferror(f))
        throw std::runtime_error("error while reading " + map);
    lx_taxmap_result r;
    check(lx_taxmap_finish(tm, &r));
    msJoin = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    msKernel = 0;
    if (h)
        (void)lx_last_phase_ms(h, 6, &msKernel, nullptr);
    tax.has = true;
    tax.off.assign(r.s_tax_off, r.s_tax_off + r.n_s + 1);
    tax.ids.assign(r.s_tax_ids, r.s_tax_ids + r.s_tax_off[r.n_s]);
    uint64_t const n = ids.size();
    std::fprintf(stderr,
                 "lambda3 taxonomy: %llu map lines, %llu matched; subjects without accession: %llu/%llu, with more than one accession: %llu/%llu\n"
                 "Subjects without tax IDs:             %llu/%llu\nSubjects with more than one tax ID:   %llu/%llu\n",
                 (unsigned long long)r.lines, (unsigned long long)r.matched, (unsigned long long)r.no_acc, (unsigned long long)n,
                 (unsigned long long)r.multi_acc, (unsigned long long)n, (unsigned long long)r.no_tax, (unsigned long long)n,
                 (unsigned long long)r.multi_tax, (unsigned long long)n);
    if (r.no_tax > 0 && n / r.no_tax < 5) // src/mkindex_algo.hpp:343-349
        std::fprintf(stderr, "WARNING: %g%% of subjects have no taxID.\n         Maybe you specified the wrong map file?\n", double(r.no_tax) * 100 / n);
    if (dumpDir.empty())
        return;
    auto slurp = [](std::string const & path)
    {
        std::ifstream in(path, std::ios::binary);
        if (!in)
            throw std::runtime_error("cannot open " + path);
        return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    };
    std::string const nodes = slurp(dumpDir + "/nodes.dmp"), names = slurp(dumpDir + "/names.dmp");
    lx_taxonomy *     tree  = nullptr;
    if (lx_taxonomy_build(nodes.data(), nodes.size(), names.data(), names.size(), r.present, r.n_present, &tree) != LX_OK)
        throw std::runtime_error("-x " + dumpDir + ": " + lx_last_output_error());
    std::unique_ptr<lx_taxonomy, void (*)(lx_taxonomy *)> keepTree(tree, lx_taxonomy_free);
    lx_taxonomy_info info;
    (void)lx_taxonomy_get(tree, &info);
    std::fputs(info.warnings, stderr);
    tax.hasTree = true;
    tax.parents.assign(info.parents, info.parents + info.n_taxa);
    tax.heights.assign(info.heights, info.heights + info.n_taxa);
    tax.names.assign(info.names, info.names + info.n_taxa);
    std::fprintf(stderr, "Number of nodes in tree: %llu\nMaximum Tree Height: %u\n", (unsigned long long)info.n_nodes, info.max_height);
}

// host threads this process may use: the hardware's, capped by the affinity mask and the cgroup's CPU quota
unsigned grantedThreads()
{
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0)
        n = std::min<unsigned>(n, (unsigned)CPU_COUNT(&set));
    std::ifstream f("/sys/fs/cgroup/cpu.max");
    std::string   quota;
    double        period = 0;
    if (f >> quota >> period && quota != "max" && period > 0)
        n = std::min<unsigned>(n, std::max(1u, (unsigned)(std::stod(quota) / period + 0.5)));
    return std::min(n, 64u);
}

} // namespace

int main(int argc, char ** argv)
{
    try
    {
        Options const opt  = parse(argc, argv);
        auto const    tStart = std::chrono::steady_clock::now();
        auto          msSince = [](std::chrono::steady_clock::time_point a)
        { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
        bool const    mk = opt.cmd.rfind("mkindex", 0) == 0;
        bool const    prot = opt.cmd == "searchp" || opt.cmd == "mkindexp", bs = opt.cmd == "searchbs" || opt.cmd == "mkindexbs";
        // -i / -d names an index made by `lambda3 mkindex*`, or the database as FASTA (the table is then made in memory)
        bool const    fromIndex = !mk && isIndexFile(opt.db);
        // --lazy-query 1 / --query-block N: the query file block by block (the header comment); --query-block 0 = the eager path
        bool const     lazy       = !mk && (opt.queryBlockGiven ? opt.queryBlock > 0 : opt.lazyQuery);
        uint64_t const blockReads = opt.queryBlock ? opt.queryBlock : (1ull << 20); // (the default is not measured yet: DESIGN.md 5.1)
        SeqSet           qs, db;
        IndexFileOptions ifo;
        struct FileCloser
        {
            void operator()(FILE * f) const
            {
                if (f)
                    std::fclose(f);
            }
        };
        std::unique_ptr<FILE, FileCloser> indexFileOwner; // (closed on every way out of main)
        FILE *                            indexFile = nullptr;
        if (fromIndex)
        {
            readIndexHead(opt.db, ifo, db, &indexFile);
            indexFileOwner.reset(indexFile);
            // the index fixes the domain (src/search.cpp:189-207)
            {
                if (prot && ifo.transAlph != kAlphAminoAcid)
                    throw std::runtime_error("Attempting to use nucleotide or bisulfite index for protein search.");
                if (!prot && ifo.transAlph != kAlphDna5)
                    throw std::runtime_error(bs ? "Attempting to use protein index for bisulfite search." : "Attempting to use protein index for nucleotide search.");
                if (!prot && !bs && ifo.redAlph != kAlphDna4)
                    throw std::runtime_error("Attempting to use bisulfite index for nucleotide search.");
                if (bs && ifo.redAlph != kAlphDna3Bs)
                    throw std::runtime_error("Attempting to use nucleotid index for bisulfite search.");
            }
        }
        // the input files' bytes, decompressed (two files, two threads and a handle each; -t 1 keeps it to one): search* decodes BGZF
        // members on the first device of --devices, mkindex* on the host unless --table gpu already asks for a device
        int const   gunzipDevice = (!mk || opt.table == "gpu") ? (opt.devices.empty() ? 0 : opt.devices[0]) : -1;
        InputText   qIn, dIn;
        std::string loadError;
        std::unique_ptr<QueryStream> qStream; // --lazy-query: the query file stays a stream (its first pieces are here: format, alphabet)
        if (lazy)
            qStream.reset(new QueryStream(opt.query, gunzipDevice));
        {
            std::thread qLoader;
            auto        loadQueries = [&]()
            {
                try
                {
                    qIn = readInput(opt.query, gunzipDevice);
                }
                catch (std::exception const & e)
                {
                    loadError = e.what();
                }
            };
            struct LoadJoiner
            {
                std::thread & t;
                ~LoadJoiner()
                {
                    if (t.joinable())
                        t.join();
                }
            } loadJoiner{qLoader};
            if (!mk && !lazy && opt.threads != 1)
                qLoader = std::thread(loadQueries);
            else if (!mk && !lazy)
                loadQueries();
            if (!fromIndex)
                dIn = readInput(opt.db, gunzipDevice);
        }
        if (!loadError.empty())
            throw std::runtime_error(loadError);
        double const msGunzip = std::max(qIn.msGunzip, dIn.msGunzip);
        bool const   gunzipOnDevice = qIn.onDevice || dIn.onDevice;
        uint64_t const plainMembers = qIn.plainMembers + dIn.plainMembers, plainChunks = qIn.plainChunks + dIn.plainChunks;
        std::string const reduction = !fromIndex ? opt.reduction : ifo.redAlph == kAlphLi10 ? "li10" : ifo.redAlph == kAlphMurphy10 ? "murphy10" : "none";
        // searchp with nucleotide queries is BLASTX: six translated frames per query against the protein database
        bool const    blastx = !mk && prot && (opt.qryAlphabet == "dna5" || (opt.qryAlphabet == "auto" && (lazy ? qStream->looksLikeDna() : looksLikeDna(qIn.text, opt.query))));
        // searchp against a nucleotide database translates the subjects instead (TBLASTN), or both sides (TBLASTX)
        bool const    sTrans  = fromIndex ? (prot && ifo.origAlph != ifo.transAlph)
                                          : prot && (opt.dbAlphabet == "dna5" || (opt.dbAlphabet == "auto" && looksLikeDna(dIn.text, opt.db)));
        // genetic code: the subjects' is the index's; the queries' is -g, else the index's (src/search.cpp:157-178)
        int const geneticCodeDb  = fromIndex ? (int)ifo.geneticCode : opt.geneticCode;
        int const geneticCodeQry = (opt.geneticCodeGiven || !fromIndex || !sTrans) ? opt.geneticCode : (int)ifo.geneticCode;
        if (fromIndex && sTrans && geneticCodeQry != geneticCodeDb)
            std::cerr << "WARNING: The genetic code used when creating the index: " << geneticCodeDb
                      << "\n         is not the same as now selected for the query sequences: " << geneticCodeQry
                      << "\n         Are you sure this is what you want?\n";
        // frames per sequence, src/search_datastructures.hpp:380-385
        int const     qFrames = bs ? 4 : blastx ? 6 : prot ? 1 : 2;
        int const     sFrames = bs ? 2 : sTrans ? 6 : 1;
        char const *  program = blastx ? (sTrans ? "tblastx" : "blastx") : sTrans ? "tblastn" : prot ? "blastp" : "blastn";

        // the queries are read beside the database (two files, two threads; -t 1 keeps it to one)
        std::string qryError;
        std::thread qryReader;
        auto        readQueries = [&]()
        {
            try
            {
                readFasta(qIn.text, opt.query, prot, !prot, qs, blastx, geneticCodeQry, bs ? 2 : 0);
            }
            catch (std::exception const & e)
            {
                qryError = e.what();
            }
        };
        struct Joiner // (joined on every way out)
        {
            std::thread & t;
            ~Joiner()
            {
                if (t.joinable())
                    t.join();
            }
        } joiner{qryReader};
        if (!mk && !lazy && opt.threads != 1)
            qryReader = std::thread(readQueries);
        else if (!mk && !lazy)
            readQueries();
        if (!fromIndex)
        {
            size_t const first = dIn.text.find_first_not_of(" \t\r\n\v\f");
            if (first != std::string::npos && dIn.text[first] != '>' && dIn.text[first] != '@')
                throw std::runtime_error(opt.db + " is neither a FASTA file nor an index of this front end (nor FASTQ, plain or gzip-compressed; an index written by the reference -- a cereal "
                                         "archive of an fmindex-collection FM-index -- cannot be read here: run lambda3 mkindexp|mkindexn|mkindexbs on the FASTA file)");
            readFasta(dIn.text, opt.db, prot, false, db, sTrans, geneticCodeDb, bs ? 1 : 0);
        }
        if (qryReader.joinable())
            qryReader.join();
        if (!qryError.empty())
            throw std::runtime_error(qryError);
        if ((!mk && !lazy && qs.ids.empty()) || db.ids.empty())
            throw std::runtime_error("empty query or database file");
        if (fromIndex && db.off.size() != db.ids.size() * (size_t)sFrames)
            throw std::runtime_error("index file " + opt.db + ": the frames of its sequences do not fit its alphabets");
        if (mk && opt.truncateIds) // src/mkindex_algo.hpp:123
            for (std::string & id : db.ids)
                id.resize(std::min(id.size(), id.find_first_of(" \t")));
        double const      msRead = msSince(tStart);
        std::string const gunzipNote = msGunzip > 0 ? " (gzip decompression " + std::string(gunzipOnDevice ? "of BGZF on the GPU " : "on the host ") +
                                                          std::to_string((long)(msGunzip + 0.5)) +
                                                          (plainMembers ? ", " + std::to_string(plainMembers) + " plain member(s) in " + std::to_string(plainChunks) + " chunks on the GPU" : std::string()) + ")"
                                                    : std::string();
        unsigned const nThreads = opt.threads > 0 ? (unsigned)opt.threads : grantedThreads();

        // ---- the reduced alphabet of the seeding stage and the word table over the reduced database (the FM-index's place)
        uint8_t const * redTab = nullptr;
        int             alph   = 27;
        if (prot && reduction == "li10")
            redTab = lambda_amd::kLi10, alph = 10;
        else if (prot && reduction == "murphy10")
            redTab = lambda_amd::kMurphy10, alph = 10;
        else if (bs)
            alph = 6;
        else if (!prot)
            redTab = lambda_amd::kDna4, alph = 4;
        // bisulfite: the reduction alternates with the frame (even: forward, odd: reverse; src/view_reduce_to_bisulfite.hpp:132-136)
        auto reduce = [&](SeqSet const & set)
        {
            std::vector<uint8_t> red(set.res.size());
            if (bs)
            {
                for (size_t f = 0; f < set.off.size(); ++f)
                    for (uint64_t i = 0; i < set.len[f]; ++i)
                        red[set.off[f] + i] = ((f & 1) ? lambda_amd::kBsRev : lambda_amd::kBsFwd)[std::min<uint8_t>(set.res[set.off[f] + i], 4)];
                return red;
            }
            for (size_t i = 0; i < set.res.size(); ++i)
                red[i] = redTab ? redTab[set.res[i] < (prot ? 27 : 5) ? set.res[i] : 0] : set.res[i];
            return red;
        };
        if (!mk || opt.table == "gpu") // (before the first device is touched: the library's own wording)
            for (int d : opt.devices)
                if (d < 0 || d >= lx_device_count())
                    throw std::runtime_error("device_id " + std::to_string(d) + " out of range [0," + std::to_string(lx_device_count()) + ")");
        auto const                 tIndex = std::chrono::steady_clock::now();
        // taxonomy columns (src/search_options.hpp:736-820): lcataxid, lt or ls ask for the LCA
        IndexTaxonomy indexTax;
        auto          hasWord = [](std::string const & list, char const * w)
        {
            for (size_t at = 0; at < list.size();)
            {
                size_t const b = list.find_first_not_of(" \t", at);
                if (b == std::string::npos)
                    break;
                size_t const e = std::min(list.find_first_of(" \t", b), list.size());
                if (list.compare(b, e - b, w) == 0)
                    return true;
                at = e;
            }
            return false;
        };
        bool const wantLca = !mk && (hasWord(opt.outputColumns, "lcataxid") || hasWord(opt.samTags, "lt") || hasWord(opt.samTags, "ls"));
        std::vector<uint8_t> const dbRed = reduce(db);
        // the word table (Level 3 of include/lambda_ext.h): made or loaded with the first device's handle where the seeding or the
        // table is the GPU's -- table and reduced subjects then stay on that device, and worker 0 works with that handle --, else on
        // the -t host threads
        using IndexOwner = std::unique_ptr<lx_index, void (*)(lx_index *)>;
        std::unique_ptr<lx_handle, void (*)(lx_handle *)> firstHandle(nullptr, lx_destroy);
        IndexOwner                                        ix(nullptr, lx_index_destroy);
        bool                                              tableOnGpu = false;
        int                                               tableSlices = 0; // (> 0: the GPU made the table in that many slices)
        bool const gpuSeedingWanted = !mk && opt.seeding == "gpu";
        auto       makeFirstHandle  = [&]()
        {
            lx_handle * h = nullptr;
            if (lx_create(opt.devices.empty() ? 0 : opt.devices[0], &h) != LX_OK)
                throw std::runtime_error(std::string("lambda_ext: ") + lx_last_error(nullptr));
            firstHandle.reset(h);
        };
        if (fromIndex)
        {
            // the table's bytes: its header says how many (ReducedIndex::save: 16 + 16 bytes, the entries, the prefix table)
            std::vector<uint8_t> bytes(32);
            bool                 ok = std::fread(bytes.data(), 1, 32, indexFile) == 32;
            if (ok)
            {
                uint64_t cnt[2];
                std::memcpy(cnt, bytes.data() + 16, sizeof(cnt));
                uint64_t dbLetters = 0;
                for (uint64_t l : db.len)
                    dbLetters += l;
                ok = cnt[0] == dbLetters && cnt[1] <= (1ull << 32);
                if (ok)
                {
                    bytes.resize(32 + cnt[0] * 16 + cnt[1] * 8);
                    ok = std::fread(bytes.data() + 32, 1, bytes.size() - 32, indexFile) == bytes.size() - 32;
                }
            }
            lx_index * raw = nullptr;
            if (ok && gpuSeedingWanted && lx_device_count() > 0)
                makeFirstHandle();
            if (ok && firstHandle && lx_index_load(firstHandle.get(), bytes.data(), bytes.size(), dbRed.data(), db.off.data(), db.len.data(), db.off.size(), &raw) != LX_OK)
                firstHandle.reset(); // (no room on the device, 2^32 - 1 entries or more, ...: the host copy alone; a table that is wrong fails again below)
            ok = ok && (raw || lx_index_load(nullptr, bytes.data(), bytes.size(), dbRed.data(), db.off.data(), db.len.data(), db.off.size(), &raw) == LX_OK);
            ix.reset(raw);
            lx_index_info info{};
            ok = ok && lx_index_get_info(raw, &info) == LX_OK && info.alph == alph;
            if (!ok)
                throw std::runtime_error("index file " + opt.db + ": the word table is truncated or does not fit the sequences");
            readIndexTaxonomy(opt.db, indexFile, db.ids.size(), indexTax);
            indexFileOwner.reset();
            // an LCA needs the tree (src/search_algo.hpp:309-313); an index without any taxonomy keeps printing "*" and 0
            if (wantLca && indexTax.has && !indexTax.hasTree)
                throw std::runtime_error("You requested taxonomic binning, but the index does not contain a taxonomic tree. Recreate it and provide --tax-dump-dir .");
        }
        else
        {
            // on the GPU (keys, one radix sort, prefix table: lx_seed.hip) where there is one to take it, else on the -t host threads;
            // the same table either way.  The GPU makes it in slices of the key space where --table-slice says so, where the set has
            // 2^31 words or more (beyond one sort) and, once, where one sort's memory is more than the device has left.
            bool const wantGpu = opt.table == "gpu" || (opt.table == "auto" && !mk);
            lx_index * raw     = nullptr;
            if (wantGpu && lx_device_count() > 0)
            {
                makeFirstHandle();
                uint64_t const kAutoSlice = 1ull << 30;
                uint64_t       dbLetters  = 0;
                for (uint64_t l : db.len)
                    dbLetters += l;
                uint64_t slice = opt.tableSlice ? opt.tableSlice : dbLetters >= (1ull << 31) ? kAutoSlice : 0;
                auto     build = [&]()
                {
                    if (slice && lx_set_option(firstHandle.get(), LX_OPT_INDEX_SLICE_WORDS, slice) != LX_OK)
                        throw std::runtime_error(std::string("lambda_ext: ") + lx_last_error(firstHandle.get()));
                    return lx_index_build(firstHandle.get(), dbRed.data(), db.off.data(), db.len.data(), db.off.size(), alph, nThreads, &raw);
                };
                int rc = build();
                if (rc == LX_ENOMEM && !slice)
                {
                    slice = kAutoSlice;
                    rc    = build();
                }
                tableOnGpu = rc == LX_OK;
                float msTable = 0;
                if (tableOnGpu && slice && lx_last_phase_ms(firstHandle.get(), 8, &msTable, &tableSlices) != LX_OK)
                    tableSlices = 0;
                if (rc != LX_OK && rc != LX_EINVAL && rc != LX_ENOMEM) // (too large for the device build or for its memory: the host threads make it)
                {
                    if (opt.table == "gpu")
                        throw std::runtime_error(std::string("lambda_ext: ") + lx_last_error(firstHandle.get()));
                    std::cerr << "WARNING: the word table is made on the host threads (" << lx_last_error(firstHandle.get()) << ")\n";
                }
            }
            else if (opt.table == "gpu")
                throw std::runtime_error("--table gpu: no HIP device available");
            if (!tableOnGpu)
            {
                if (lx_index_build(nullptr, dbRed.data(), db.off.data(), db.len.data(), db.off.size(), alph, nThreads, &raw) != LX_OK)
                    throw std::runtime_error(std::string("lambda_ext: ") + lx_last_output_error());
                if (firstHandle && gpuSeedingWanted) // the seeding is the GPU's all the same: the host-made table becomes resident
                {
                    lx_index * att = nullptr;
                    if (lx_index_attach(raw, firstHandle.get(), &att) == LX_OK)
                    {
                        lx_index_destroy(raw);
                        raw = att;
                    }
                    else
                        firstHandle.reset();
                }
                else
                    firstHandle.reset();
            }
            ix.reset(raw);
        }
        double const      msIndex = msSince(tIndex);
        std::string const onGpu   = tableSlices > 0 ? "on the GPU in " + std::to_string(tableSlices) + " slices" : "on the GPU";
        if (mk)
        {
            // mkindexp | mkindexn | mkindexbs (src/mkindex.cpp): the options that fix the types, ids, sequences, table -> one file
            IndexFileOptions out;
            out.indexType   = opt.dbIndexType == "bifm" ? 1 : 0;
            out.origAlph    = prot ? (sTrans ? kAlphDna5 : kAlphAminoAcid) : kAlphDna5; // :206-224, :235
            out.transAlph   = prot ? kAlphAminoAcid : kAlphDna5;
            out.redAlph     = bs ? kAlphDna3Bs : !prot ? kAlphDna4 : reduction == "li10" ? kAlphLi10 : reduction == "murphy10" ? kAlphMurphy10 : kAlphAminoAcid;
            out.geneticCode = (uint8_t)geneticCodeDb;
            IndexTaxonomy tax;
            double        msTax = 0;
            float         msTaxKernel = 0;
            if (!opt.accTaxMap.empty())
            {
                // the join on the device under --table gpu, else on the -t host threads (the same bytes either way)
                lx_handle * th = nullptr;
                if (opt.table == "gpu" && lx_create(opt.devices.empty() ? 0 : opt.devices[0], &th) != LX_OK)
                    throw std::runtime_error(lx_last_error(nullptr));
                std::unique_ptr<lx_handle, void (*)(lx_handle *)> keepH(th, lx_destroy);
                buildIndexTaxonomy(opt.accTaxMap, opt.taxDumpDir, db.ids, th, nThreads, tax, msTax, msTaxKernel);
                std::fprintf(stderr, "lambda3 times [ms]: taxonomy %.0f (%s)\n", msTax,
                             th ? ("join on the GPU, kernels " + std::to_string((long)(msTaxKernel + 0.5))).c_str() : (std::to_string(nThreads) + " host thread(s)").c_str());
            }
            auto const tWrite = std::chrono::steady_clock::now();
            writeIndexFile(opt.index, out, db, ix.get(), tax);
            uint64_t residues = 0;
            for (auto l : db.len)
                residues += l;
            std::fprintf(stderr,
                         "lambda3 %s: %zu sequences (%llu residues in %d frame(s); original alphabet %s, translated %s, reduced %s, genetic code %d) -> %s\n"
                         "lambda3 times [ms]: read %.0f%s, reduce + word table %.0f (%s), write %.0f, total %.0f\n",
                         opt.cmd.c_str(), db.ids.size(), (unsigned long long)residues, sFrames, alphName(out.origAlph), alphName(out.transAlph),
                         alphName(out.redAlph), (int)out.geneticCode, opt.index.c_str(), msRead, gunzipNote.c_str(), msIndex, tableOnGpu ? onGpu.c_str() : (std::to_string(nThreads) + " host thread(s)").c_str(),
                         msSince(tWrite), msSince(tStart));
            return 0;
        }
        std::vector<uint8_t> const qRed = reduce(qs);

        // ---- scoring + statistics (prepareScoring, src/search_algo.hpp:166-234): bisulfite = two matrices over SeqAn Dna5
        // (forward: slot 0, reverse: slot 1, :176-186), statistics from the match / mismatch scheme
        lx_scoring sc, scRev;
        int const  gapOpen = opt.gapOpen, gapExtend = opt.gapExtend;
        lambda_amd::builtinScoring(prot ? opt.scoringMethod : bs ? -1 : 0, opt.match, opt.misMatch, gapOpen, gapExtend, sc);
        if (bs)
            lambda_amd::builtinScoring(-2, opt.match, opt.misMatch, gapOpen, gapExtend, scRev);
        lx_karlin ka;
        if (!lambda_amd::karlinParams(prot ? opt.scoringMethod : 0, opt.match, opt.misMatch, gapOpen, gapExtend, ka))
            throw std::runtime_error("Could not compute Karlin-Altschul-Values for Scoring Scheme."); // :232-233

        // ---- devices and worker threads (src/search.cpp:379-385: one LocalDataHolder per thread; here one handle per thread)
        std::vector<int> devices = opt.devices;
        if (devices.empty())
            for (int d = 0; d < lx_device_count(); ++d)
                devices.push_back(d);
        if (devices.empty())
            throw std::runtime_error("no HIP device available (this front end has no CPU path)");
        // one worker = one handle per entry of --devices (a device may be listed twice); -t host threads in all, shared out among
        // the workers for the seeding of their reads (the reference: -t OpenMP threads, each with its own LocalDataHolder; a GPU
        // wants few, large extension batches, the seeding wants every core)
        size_t const   nWorkers = lazy ? devices.size() : std::max<size_t>(1, std::min<size_t>(devices.size(), qs.ids.size()));
        unsigned const seedThreads = std::max(1u, nThreads / (unsigned)nWorkers);

        // ---- seeding (search(), src/search_algo.hpp:611-762) over the sorted table of reduced words
        lambda_amd::SeedingInput sin{};
        sin.qRes = qs.res.data(), sin.qRed = qRed.data(), sin.qOff = qs.off.data(), sin.qLen = qs.len.data(), sin.nQSeq = qs.off.size();
        sin.qNumFrames       = qFrames;
        sin.unknownRank      = prot ? 25 : bs ? 4 : 3; // 'X' / 'N'
        sin.sRes = db.res.data(), sin.sOff = db.off.data(), sin.sLen = db.len.data();
        sin.alph             = alph;
        sin.matrix           = sc.matrix;
        sin.matrixRev        = bs ? scRev.matrix : nullptr;
        sin.maxMatches       = opt.maxMatches;
        sin.halfExact        = opt.halfExact;
        sin.adaptive         = opt.adaptive;
        sin.preScoring       = opt.preScoring;
        sin.preScoringThresh = opt.preScoringThresh;

        // dbTotalLength = sum of the (frame-expanded) subject lengths, src/search_algo.hpp:317-319
        uint64_t dbTotal = 0;
        for (auto l : db.len)
            dbTotal += l;
        lx_search_params sp{};
        sp.max_evalue       = opt.maxEValue;
        sp.min_bitscore     = opt.minBitScore;
        sp.id_cutoff        = opt.idCutOff;
        sp.db_total_length  = dbTotal;
        sp.query_translated = blastx ? 1 : 0;
        sp.qry_num_frames   = qFrames;
        sp.sbj_num_frames   = sFrames;
        sp.bisulfite        = bs ? 1 : 0;
        sp.q_frame_mode     = bs ? LX_FRAMES_BISULFITE : blastx ? LX_FRAMES_TRANSLATED : prot ? LX_FRAMES_NONE : LX_FRAMES_REVCOMP; // _setFrames, :768-814
        sp.s_frame_mode     = bs ? LX_FRAMES_BISULFITE : sTrans ? LX_FRAMES_TRANSLATED : LX_FRAMES_NONE;
        sp.karlin           = ka;
        // only the SAM writer reads alignment columns (its CIGAR); the tables are made from the counts
        bool       outGz    = false;
        int const  outFmt   = outputFormat(opt.output, outGz);
        bool const wantOps  = outFmt == LX_OUT_SAM || outFmt == LX_OUT_BAM;
        sp.flags            = wantOps ? 0 : LX_ITERATE_NO_OPS;

        lambda_amd::SeedParams const so1{opt.seedLength, opt.seedOffset, opt.seedDelta}, so0{opt.seedLength0, opt.seedOffset0, opt.seedDelta0};
        // what a worker keeps for its range of reads
        struct Part
        {
            std::vector<lx_blast_match> bms;
            std::vector<uint8_t>        ops;
            lx_iterate_stats            ist{};
            lambda_amd::SeedingStats    sst{};
            size_t                      nPromising = 0;
            double                      msSeed = 0, msExtend = 0, msRecords = 0;
            lx_record_stats             rst{}; // --records gpu: _writeRecord's statistics of this worker's passes
            bool                        gpuSeeding = false; // the seeding stage of this worker ran on its device
            size_t                      nDeclined = 0, nPassesOnHost = 0; // reads the GPU seeding stage left to the host; passes whose match buffer was full
            std::string                 error;
        };
        std::vector<Part> parts(nWorkers);
        uint64_t const    nReads = qs.ids.size();
        // --records (the header comment): auto = host -- the measured rule of DESIGN.md ("_writeRecord on the device")
        bool const recordsOnGpu = opt.records == "gpu" && opt.maxMatches > 0;
        // what a worker searches in one go: a range of the reads of a sequence set, its records into `bms` / `ops` (the eager path: one
        // range of all reads per worker; --lazy-query: one block after the other, all of its reads)
        struct Job
        {
            SeqSet const *                q   = nullptr;
            std::vector<uint8_t> const *  red = nullptr;
            uint64_t                      rLo = 0, rHi = 0;
            std::vector<lx_blast_match> * bms = nullptr;
            std::vector<uint8_t> *        ops = nullptr;
            void *                        block = nullptr;
        };
        auto worker = [&](size_t w, std::function<bool(Job &)> const & nextJob, std::function<void(Job &)> const & jobDone)
        {
            Part & pt = parts[w];
            try
            {
                // worker 0 works with the handle the table is resident on; the others make their own and attach the table to it
                bool const         borrow = w == 0 && firstHandle;
                lambda_amd::Engine eng(borrow ? firstHandle.get() : nullptr, devices[w % devices.size()]);
                eng.setScoring(sc, 0);
                if (bs)
                    eng.setScoring(scRev, 1);
                // the database stays on the GPU for the whole run (the reference keeps it in the index file it maps at start-up)
                eng.check(lx_set_subjects(eng.raw(), db.res.data(), db.res.size()));
                // one pass of the batch loop of realMain (src/search.cpp:426-459): seed, extend (GPU), collect
                IndexOwner       attached(nullptr, lx_index_destroy);
                lx_index const * gpuIndex = nullptr; // the table on this worker's handle (NULL: the seeding is the host threads')
                if (opt.seeding == "gpu")
                {
                    if (borrow)
                        gpuIndex = ix.get();
                    else
                    {
                        lx_index * att = nullptr;
                        if (lx_index_attach(ix.get(), eng.raw(), &att) == LX_OK)
                            attached.reset(att), gpuIndex = att;
                        else // (the table and the sequences did not fit beside the extension's buffers: host threads)
                            std::cerr << "WARNING: seeding on the host threads (" << lx_last_error(eng.raw()) << ")\n";
                    }
                }
                pt.gpuSeeding = gpuIndex != nullptr;
                // with the seeding on the device its matches stay there: the sequence sets become resident for the Level-2 kernels
                // (LAMBDA3_HOST_LIST=1: the matches come down and go through lx_iterate_matches, the A/B switch of the tests)
                bool const deviceList = gpuIndex && !std::getenv("LAMBDA3_HOST_LIST");
                if (deviceList)
                    eng.check(lx_set_subject_seqs(eng.raw(), db.off.data(), db.len.data(), db.off.size()));
                Job job;
                // the job's queries for the Level-2 kernels, and room for its one call per seeding pass
                auto beginJob = [&]()
                {
                    SeqSet const & qs  = *job.q;
                    uint64_t const rLo = job.rLo, rHi = job.rHi;
                    if (!deviceList)
                        return;
                    eng.check(lx_set_queries(eng.raw(), qs.res.data(), qs.res.size(), qs.off.data(), qs.len.data(), qs.off.size(), qs.orig_len.data(), qFrames));
                    // this worker makes ONE Level-2 call per seeding pass: what that call would allocate and touch inside itself is asked
                    // for here, before the seeding (a dozen promising seeds per read, a window per seven of them, a record per twelve --
                    // what the read sets of tools/cli_scale_nucl.py come to; a short estimate only moves an allocation back into the call)
                    uint64_t const est = std::min<uint64_t>(12 * (rHi - rLo), 0x7ffffff0ull);
                    uint64_t       len = 0;
                    for (uint64_t i = rLo * (uint64_t)qFrames; i < rHi * (uint64_t)qFrames && i < qs.len.size(); ++i)
                        len = std::max<uint64_t>(len, qs.len[i]);
                    if (est >= 100000)
                        eng.check(lx_reserve(eng.raw(), est, est / 7, est / 12, wantOps ? est / 12 * (len + len / 16) : 0));
                };
                lx_seed_params spar{};
                spar.half_exact = sin.halfExact ? 1 : 0, spar.adaptive = sin.adaptive ? 1 : 0, spar.pre_scoring = sin.preScoring;
                spar.pre_scoring_thresh = sin.preScoringThresh, spar.max_matches = sin.maxMatches, spar.q_num_frames = sin.qNumFrames;
                spar.unknown_rank = sin.unknownRank, spar.matrix = sin.matrix, spar.matrix_rev = sin.matrixRev, spar.host_threads = seedThreads;
                auto pass = [&](lambda_amd::SeedParams const & so, std::vector<uint64_t> const & which)
                {
                    SeqSet const &               qs   = *job.q;
                    std::vector<uint8_t> const & qRed = *job.red;
                    std::vector<lx_blast_match> & outBms = *job.bms;
                    std::vector<uint8_t> &        outOps = *job.ops;
                    if (std::getenv("LAMBDA3_TRACE"))
                        std::fprintf(stderr, "[worker %zu] seeding %zu frame sequences (seed %d/%d, delta %d)\n", w, which.size(), so.seedLength, so.seedOffset, so.maxSeedDist);
                    auto const            tSeed = std::chrono::steady_clock::now();
                    std::vector<uint64_t> reads; // (lx_seed_queries takes a read by its first frame sequence)
                    for (uint64_t i : which)
                        if (i % (uint64_t)qFrames == 0)
                            reads.push_back(i);
                    spar.seed_length = so.seedLength, spar.seed_offset = so.seedOffset, spar.max_seed_dist = so.maxSeedDist;
                    lx_seed_result * sr = nullptr;
                    // the device takes the reads; those it declines (words far beyond the table's keys with many occurrences) and those of
                    // a launch whose match buffer filled up are finished on the host threads inside the call
                    if (gpuIndex && lx_seed_queries(eng.raw(), gpuIndex, nullptr, qs.res.data(), qRed.data(), qs.off.data(), qs.len.data(), qs.off.size(), reads.data(),
                                                    reads.size(), &spar, &sr) != LX_OK)
                    {
                        // a HIP error in the seeding stage (its match buffer did not fit, ...): this pass and the following ones are
                        // seeded on the host threads, from a clean slate
                        std::cerr << "WARNING: seeding on the host threads from here on (" << lx_last_error(eng.raw()) << ")\n";
                        gpuIndex      = nullptr;
                        pt.gpuSeeding = false;
                    }
                    if (!sr && lx_seed_queries(nullptr, ix.get(), db.res.data(), qs.res.data(), qRed.data(), qs.off.data(), qs.len.data(), qs.off.size(), reads.data(),
                                               reads.size(), &spar, &sr) != LX_OK)
                        throw std::runtime_error(std::string("lambda_ext: ") + lx_last_output_error());
                    std::unique_ptr<lx_seed_result, void (*)(lx_seed_result *)> keepSeeds(sr, lx_seed_result_free);
                    lx_seed_stats const sst = lx_seed_result_stats(sr);
                    pt.sst.hitsAfterSeeding += sst.hits_after_seeding, pt.sst.hitsFailedPreExtendTest += sst.hits_failed_pre_extend;
                    pt.nDeclined += sst.reads_declined, pt.nPassesOnHost += sst.launches_full;
                    // the matches where the seeding left them: the device list for the Level-2 kernels, else the list in host memory
                    void const * const dList    = deviceList ? lx_seed_result_matches_dev(sr) : nullptr;
                    uint64_t const     nMatches = sst.n_matches;
                    lx_match * const   hList    = dList || nMatches == 0 ? nullptr : lx_seed_result_matches(sr);
                    if (!dList && nMatches && !hList)
                        throw std::runtime_error("the match list did not fit into host memory");
                    pt.msSeed += msSince(tSeed);
                    pt.nPromising += nMatches;
                    if (std::getenv("LAMBDA3_TRACE"))
                        std::fprintf(stderr, "[worker %zu] %zu promising seeds -> extension\n", w, (size_t)nMatches);
                    if (nMatches == 0)
                        return;
                    lx_iterate_result * res = nullptr;
                    auto const          tExt = std::chrono::steady_clock::now();
                    lx_record_stats passRst{};
                    bool            cutDone = false;
                    if (dList && recordsOnGpu) // ... with _writeRecord's cut before the records come down
                    {
                        eng.check(lx_iterate_matches_dev_top(eng.raw(), 0, dList, nMatches, &sp, opt.maxMatches, &passRst, &res));
                        float msTop = 0;
                        if (lx_last_phase_ms(eng.raw(), 7, &msTop, nullptr) == LX_OK)
                            pt.msRecords += msTop;
                        cutDone = true;
                    }
                    else if (dList) // the Level-2 driver on the list where the seeding kernel left it (include/lambda_ext.h)
                        eng.check(lx_iterate_matches_dev(eng.raw(), 0, dList, nMatches, &sp, &res));
                    else
                        eng.check(lx_iterate_matches(eng.raw(), 0, qs.res.data(), qs.res.size(), qs.off.data(), qs.len.data(), qs.off.size(),
                                                     qs.orig_len.data(), nullptr, 0, db.off.data(), db.len.data(), db.off.size(), hList, nMatches, &sp, &res));
                    pt.msExtend += msSince(tExt);
                    uint64_t               n  = lx_iterate_result_count(res);
                    lx_blast_match const * bm = lx_iterate_result_matches(res);
                    std::vector<lx_blast_match> cutRows;
                    if (recordsOnGpu && !cutDone) // (a list in host memory: the host step, on this pass's records -- all a query has)
                    {
                        auto const tRec = std::chrono::steady_clock::now();
                        cutRows.assign(bm, bm + n);
                        n  = lx_postprocess_records(cutRows.data(), n, opt.maxMatches, &passRst);
                        bm = cutRows.data();
                        pt.msRecords += msSince(tRec);
                    }
                    pt.rst.qrys_with_hit += passRst.qrys_with_hit, pt.rst.hits_duplicate2 += passRst.hits_duplicate2, pt.rst.hits_abundant += passRst.hits_abundant;
                    pt.rst.hits_final += passRst.hits_final, pt.rst.pairs += passRst.pairs;
                    uint64_t const         ob = outOps.size();
                    uint64_t opsEnd = 0; // (the records are ordered by query, their ops as the passes produced them: bisulfite runs two)
                    for (uint64_t k = 0; k < n && wantOps; ++k)
                        opsEnd = std::max<uint64_t>(opsEnd, bm[k].ops_off + bm[k].n_ops);
                    if (opsEnd)
                        outOps.insert(outOps.end(), lx_iterate_result_ops(res), lx_iterate_result_ops(res) + opsEnd);
                    for (uint64_t k = 0; k < n; ++k)
                    {
                        outBms.push_back(bm[k]);
                        outBms.back().ops_off += ob;
                    }
                    lx_iterate_stats const st = lx_iterate_result_stats(res);
                    pt.ist.hits_duplicate += st.hits_duplicate, pt.ist.failed_bitscore += st.failed_bitscore, pt.ist.failed_evalue += st.failed_evalue;
                    pt.ist.failed_identity += st.failed_identity, pt.ist.num_ext_score += st.num_ext_score, pt.ist.num_ext_ali += st.num_ext_ali;
                    lx_iterate_result_free(res);
                };
                while (nextJob(job))
                {
                beginJob();
                std::vector<uint64_t> all;
                for (uint64_t i = job.rLo * (uint64_t)qFrames; i < job.rHi * (uint64_t)qFrames; ++i)
                    all.push_back(i);
                if (opt.search0) // iterativeSearch (:1391-1457): the exact pre-search first, the default parameters for reads without a result
                {
                    pass(so0, all);
                    std::vector<uint8_t> successful(job.q->ids.size(), 0);
                    for (auto const & bm : *job.bms)
                        successful[bm.n_qid] = 1;
                    std::vector<uint64_t> rest;
                    for (uint64_t i : all)
                        if (!successful[i / (uint64_t)qFrames])
                            rest.push_back(i);
                    if (!rest.empty())
                        pass(so1, rest);
                    // (the reference writes phase 1's records of a batch before phase 2's; here both lists are written together:
                    // order by read, as one batch holding every read would give)
                    std::stable_sort(job.bms->begin(), job.bms->end(), [](lx_blast_match const & a, lx_blast_match const & b) { return a.n_qid < b.n_qid; });
                }
                else
                    pass(so1, all);
                jobDone(job);
                }
            }
            catch (std::exception const & e)
            {
                pt.error = e.what();
            }
        };
        // ---- what the writers are told, on both paths (the LCA pairs are added per list)
        lx_tax_tree               tree{};
        std::vector<char const *> taxNames;
        if (indexTax.has)
        {
            tree.parents   = indexTax.parents.data();
            tree.heights   = indexTax.heights.data();
            tree.n_taxa    = indexTax.parents.size();
            tree.s_tax_off = indexTax.off.data();
            tree.s_tax_ids = indexTax.ids.data();
            tree.n_s       = indexTax.off.size() - 1;
            if (wantLca && indexTax.hasTree)
                for (std::string const & n : indexTax.names)
                    taxNames.push_back(n.c_str());
        }
        auto outputOptions = [&](lx_output_options & oo)
        {
            lx_output_options_default(&oo);
            oo.columns             = opt.outputColumns.c_str();
            oo.sam_tags            = opt.samTags.c_str();
            oo.sam_seq             = opt.samSeq == "never" ? LX_SAM_SEQ_NEVER : opt.samSeq == "uniq" ? LX_SAM_SEQ_UNIQ : LX_SAM_SEQ_ALWAYS;
            oo.sam_hard_clip       = opt.samClip == "hard";
            oo.sam_with_ref_header = opt.samWithRefHeader;
            oo.version_to_output   = opt.versionToOutput;
            oo.version             = "3.0.0-lx"; // (the reference release this front end follows, src/CMakeLists.txt:14-19)
            oo.command_line        = opt.commandLine.c_str();
            oo.db_name             = opt.db.c_str(); // the index path there (src/search_algo.hpp:320)
            oo.genetic_code        = geneticCodeQry;
            if (indexTax.has)
            {
                oo.tax = &tree;
                if (wantLca && indexTax.hasTree)
                    oo.tax_names = taxNames.data();
            }
        };
        int const fmt = outFmt;
        double    msCompress = 0;  // (.bam, *.gz: BGZF on the first handle's device)
        double    msRenderDev = 0; // (--render gpu: the render kernels' device time)
        bool      renderedOnGpu = false;
        // --lazy-query: what the blocks came to
        struct LazyTotals
        {
            uint64_t        blocks = 0, largest = 0, maxAlive = 0, reads = 0, hsps = 0, written = 0;
            lx_record_stats rst{};
        } lazyTotals;
        auto const tSearch = std::chrono::steady_clock::now();
        if (!lazy)
        {
            // contiguous ranges of reads, as `omp for schedule(dynamic)` over whole batches would hand a thread (:384-385)
            auto run = [&](size_t w)
            {
                bool given = false;
                worker(w,
                       [&](Job & job)
                       {
                           if (given)
                               return false;
                           given = true;
                           job   = Job{&qs, &qRed, nReads * w / nWorkers, nReads * (w + 1) / nWorkers, &parts[w].bms, &parts[w].ops, nullptr};
                           return job.rLo != job.rHi;
                       },
                       [](Job &) {});
            };
            std::vector<std::thread> pool;
            for (size_t w = 1; w < nWorkers; ++w)
                pool.emplace_back(run, w);
            run(0);
            for (auto & t : pool)
                t.join();
        }
        else
        {
            // ---- the block pipeline (the reference's batch loop, src/search.cpp:389-459, with its reader thread behind a bounded
            // queue, src/search_algo.hpp:374-413): one reader makes blocks of at most blockReads reads (stream -> parser -> SeqSet:
            // ranks, frames, reduction), one worker per entry of --devices takes the next block and searches all of it as the eager
            // path searches a worker's range (then _writeRecord's cut and the LCA, both per query and so per block), and this thread
            // appends the finished blocks in their order through lx_out.  At most nWorkers + 2 blocks exist at any time: the reader
            // waits for a free place before it begins one.  An error in block k (a malformed record, a failed call) ends the run with
            // its message; the blocks in front of k are written and the file is closed behind them.
            struct Block
            {
                uint64_t                    index = 0;
                SeqSet                      qs;
                std::vector<uint8_t>        red;
                std::vector<lx_blast_match> bms;
                std::vector<uint8_t>        ops;
                uint64_t                    found = 0, kept = 0; // records before and after _writeRecord's cut
                lx_record_stats             rst{};               // (--records host: this block's step)
                std::vector<uint64_t>       lcaQid;
                std::vector<uint32_t>       lcaTax;
                uint64_t                    nLca = 0;
            };
            std::mutex                                   mu;
            std::condition_variable                      cv;
            std::deque<std::unique_ptr<Block>>           toSearch;
            std::map<uint64_t, std::unique_ptr<Block>>   done;
            uint64_t                                     alive = 0, made = 0;
            bool                                         readerDone = false, stop = false;
            std::string                                  pipeError;
            uint64_t const                               cap = nWorkers + 2;
            // the run's error; hard: nothing more is searched (a block failed), else the blocks made so far go through (the reader failed)
            auto fail = [&](std::string const & why, bool hard) // (under no lock)
            {
                std::lock_guard<std::mutex> lock(mu);
                if (pipeError.empty())
                    pipeError = why;
                stop = stop || hard;
                cv.notify_all();
            };
            auto reader = [&]()
            {
                bool holding = false; // a place taken for a block that is not in the queue yet
                try
                {
                    lx_query_blocks::BlockCutter cut(blockReads);
                    for (bool more = true; more;)
                    {
                        {
                            std::unique_lock<std::mutex> lock(mu);
                            cv.wait(lock, [&] { return alive < cap || stop; });
                            if (stop)
                                break;
                            ++alive;
                            holding = true;
                            lazyTotals.maxAlive = std::max(lazyTotals.maxAlive, alive);
                        }
                        std::unique_ptr<Block> b(new Block);
                        more = qStream->records(
                            [&](std::string const & id, std::string & letters)
                            {
                                uint64_t const n = letters.size();
                                addRecord(b->qs, id, letters, prot, !prot, blastx, geneticCodeQry, bs ? 2 : 0);
                                return !cut.add(n);
                            });
                        if (!b->qs.ids.empty())
                            b->red = reduce(b->qs);
                        std::lock_guard<std::mutex> lock(mu);
                        holding = false;
                        if (b->qs.ids.empty()) // (the file ended where the last block closed)
                        {
                            --alive;
                            break;
                        }
                        b->index = made++;
                        lazyTotals.blocks  = made;
                        lazyTotals.largest = std::max<uint64_t>(lazyTotals.largest, b->qs.ids.size());
                        lazyTotals.reads += b->qs.ids.size();
                        toSearch.push_back(std::move(b));
                        cv.notify_all();
                    }
                }
                catch (std::exception const & e)
                {
                    fail(e.what(), false);
                }
                std::lock_guard<std::mutex> lock(mu);
                if (holding)
                    --alive;
                readerDone = true;
                cv.notify_all();
            };
            auto run = [&](size_t w)
            {
                std::unique_ptr<Block> current; // the block this worker searches
                worker(w,
                       [&](Job & job)
                       {
                           std::unique_lock<std::mutex> lock(mu);
                           cv.wait(lock, [&] { return !toSearch.empty() || readerDone || stop; });
                           if (stop || toSearch.empty())
                               return false;
                           current = std::move(toSearch.front());
                           toSearch.pop_front();
                           Block * const b = current.get();
                           job = Job{&b->qs, &b->red, 0, b->qs.ids.size(), &b->bms, &b->ops, b};
                           return true;
                       },
                       [&](Job & job)
                       {
                           std::unique_ptr<Block> b = std::move(current);
                           b->found = b->kept = b->bms.size();
                           if (!recordsOnGpu) // _writeRecord's cut: every record of a read is in its block
                           {
                               auto const tRec = std::chrono::steady_clock::now();
                               b->kept         = lx_postprocess_records(b->bms.data(), b->bms.size(), opt.maxMatches, &b->rst);
                               parts[w].msRecords += msSince(tRec);
                           }
                           if (indexTax.has && wantLca && indexTax.hasTree)
                           {
                               b->lcaQid.resize(std::max<uint64_t>(b->kept, 1));
                               b->lcaTax.resize(std::max<uint64_t>(b->kept, 1));
                               if (lx_compute_lca(b->bms.data(), b->kept, &tree, b->lcaQid.data(), b->lcaTax.data(), &b->nLca) != LX_OK)
                                   throw std::runtime_error("LCA-computation error: One of the paths didn't lead to root.");
                           }
                           std::lock_guard<std::mutex> lock(mu);
                           uint64_t const              at = b->index;
                           done[at] = std::move(b);
                           cv.notify_all();
                       });
                if (!parts[w].error.empty())
                    fail(parts[w].error, true);
            };
            std::thread              readerThread(reader);
            std::vector<std::thread> pool;
            for (size_t w = 0; w < nWorkers; ++w)
                pool.emplace_back(run, w);
            struct JoinAll // (joined on every way out; an error first tells the others to stop)
            {
                std::thread &              r;
                std::vector<std::thread> & p;
                std::function<void()>      halt;
                ~JoinAll()
                {
                    halt();
                    r.join();
                    for (auto & t : p)
                        t.join();
                }
            } joinAll{readerThread, pool, [&] {
                          std::lock_guard<std::mutex> lock(mu);
                          if (!readerDone || !toSearch.empty())
                              stop = true;
                          cv.notify_all();
                      }};
            // ---- the writer: this thread
            bool const  dev = opt.render == "gpu";
            lx_handle * zh  = nullptr;
            if ((dev || outGz || fmt == LX_OUT_BAM) && lx_create(devices[0], &zh) != LX_OK)
                throw std::runtime_error(lx_last_error(nullptr));
            std::unique_ptr<lx_handle, void (*)(lx_handle *)> keepH(zh, lx_destroy);
            auto outError = [&]() { return std::string(zh ? lx_last_error(zh) : lx_last_output_error()); };
            std::vector<char const *> sidL;
            for (auto const & s : db.ids)
                sidL.push_back(s.c_str());
            lx_seq_names const subjects{nullptr, nullptr, sidL.data(), db.orig_len.data(), 0, sidL.size()};
            lx_output_options  oo;
            outputOptions(oo);
            lx_out * out = nullptr;
            struct CloseOut // (an error on the way: the file is closed behind the blocks it holds)
            {
                lx_out *& o;
                ~CloseOut()
                {
                    if (o)
                        (void)lx_out_close(o, -1);
                }
            } closeOut{out};
            renderedOnGpu = dev;
            for (uint64_t next = 0;; ++next)
            {
                std::unique_ptr<Block> b;
                {
                    std::unique_lock<std::mutex> lock(mu);
                    cv.wait(lock, [&] { return done.count(next) || stop || (readerDone && next == made); });
                    auto it = done.find(next);
                    if (it == done.end())
                        break; // (every block is written, or the one that comes next never will be)
                    b = std::move(it->second);
                    done.erase(it);
                }
                if (!out && lx_out_open(zh, opt.output.c_str(), fmt, outGz ? 1 : 0, program, &subjects, &oo, &out) != LX_OK)
                {
                    std::string const why = outError();
                    throw std::runtime_error(!why.empty() ? why : "cannot write " + opt.output);
                }
                std::vector<char const *> qidB;
                for (auto const & s : b->qs.ids)
                    qidB.push_back(s.c_str());
                lx_seq_names const nm{qidB.data(), b->qs.orig_len.data(), nullptr, nullptr, qidB.size(), 0};
                if (lx_out_append(out, dev ? LX_RENDER_DEV : LX_RENDER_HOST, b->bms.data(), b->kept, b->ops.data(), b->ops.size(), &nm,
                                  reinterpret_cast<uint8_t const *>(b->qs.ascii.data()), b->qs.ascii_off.data(), b->lcaQid.data(), b->lcaTax.data(),
                                  b->nLca) != LX_OK)
                {
                    std::string const why = outError();
                    throw std::runtime_error((dev ? "records on the GPU: " : "") + (!why.empty() ? why : "cannot write " + opt.output));
                }
                float msK = 0;
                if (dev && b->kept && lx_last_phase_ms(zh, fmt == LX_OUT_BAM ? 11 : 12, &msK, nullptr) == LX_OK)
                    msRenderDev += msK;
                if (!dev && zh && b->kept && lx_last_phase_ms(zh, 4, &msK, nullptr) == LX_OK)
                    msCompress += msK;
                lazyTotals.hsps += b->found;
                lazyTotals.written += b->kept;
                lazyTotals.rst.qrys_with_hit += b->rst.qrys_with_hit, lazyTotals.rst.hits_duplicate2 += b->rst.hits_duplicate2;
                lazyTotals.rst.hits_abundant += b->rst.hits_abundant, lazyTotals.rst.hits_final += b->rst.hits_final, lazyTotals.rst.pairs += b->rst.pairs;
                b.reset();
                std::lock_guard<std::mutex> lock(mu);
                --alive;
                cv.notify_all();
            }
            std::string error;
            {
                std::lock_guard<std::mutex> lock(mu);
                error = pipeError;
            }
            if (error.empty() && lazyTotals.reads == 0)
                error = "empty query or database file";
            uint64_t withHit = lazyTotals.rst.qrys_with_hit; // (--records gpu: counted in the workers' passes, which are over)
            for (Part const & pt : parts)
                withHit += error.empty() ? pt.rst.qrys_with_hit : 0;
            if (out)
            {
                lx_out * const o = out;
                out              = nullptr;
                if (lx_out_close(o, (int64_t)withHit) != LX_OK && error.empty())
                    error = "cannot write " + opt.output;
            }
            if (!error.empty())
                throw std::runtime_error(error);
        }
        double const msSearch = msSince(tSearch);
        auto const   tOut     = std::chrono::steady_clock::now();
        // the ranges are disjoint and ascending: concatenation in range order is the order one thread would have produced
        std::vector<lx_blast_match> bms;
        std::vector<uint8_t>        ops;
        lx_iterate_stats            ist{};
        lambda_amd::SeedingStats    sst{};
        size_t                      nPromising = 0;
        double                      msSeedMax = 0, msExtendMax = 0, msRecords = 0;
        lx_record_stats             rst{};
        uint64_t                    nHspParts = 0; // --records gpu: the records before the cut
        size_t                      nDeclined = 0, nPassesOnHost = 0;
        bool                        anyGpuSeeding = false;
        for (Part & pt : parts)
        {
            if (!pt.error.empty())
                throw std::runtime_error(pt.error);
            uint64_t const ob = ops.size();
            ops.insert(ops.end(), pt.ops.begin(), pt.ops.end());
            for (lx_blast_match m : pt.bms)
            {
                m.ops_off += ob;
                bms.push_back(m);
            }
            ist.hits_duplicate += pt.ist.hits_duplicate, ist.failed_bitscore += pt.ist.failed_bitscore, ist.failed_evalue += pt.ist.failed_evalue;
            ist.failed_identity += pt.ist.failed_identity, ist.num_ext_score += pt.ist.num_ext_score, ist.num_ext_ali += pt.ist.num_ext_ali;
            sst.hitsAfterSeeding += pt.sst.hitsAfterSeeding, sst.hitsFailedPreExtendTest += pt.sst.hitsFailedPreExtendTest;
            nPromising += pt.nPromising;
            nDeclined += pt.nDeclined, nPassesOnHost += pt.nPassesOnHost;
            anyGpuSeeding = anyGpuSeeding || pt.gpuSeeding;
            msSeedMax   = std::max(msSeedMax, pt.msSeed);
            msExtendMax = std::max(msExtendMax, pt.msExtend);
            msRecords   = std::max(msRecords, pt.msRecords);
            rst.qrys_with_hit += pt.rst.qrys_with_hit, rst.hits_duplicate2 += pt.rst.hits_duplicate2, rst.hits_abundant += pt.rst.hits_abundant;
            rst.hits_final += pt.rst.hits_final, rst.pairs += pt.rst.pairs;
        }
        nHspParts = rst.hits_final + rst.hits_duplicate2 + rst.hits_abundant;
        uint64_t const nHsp   = recordsOnGpu ? nHspParts : lazy ? lazyTotals.hsps : bms.size();
        if (lazy) // (the blocks' host steps; --records gpu counted in the passes above)
        {
            rst.qrys_with_hit += lazyTotals.rst.qrys_with_hit, rst.hits_duplicate2 += lazyTotals.rst.hits_duplicate2, rst.hits_abundant += lazyTotals.rst.hits_abundant;
            rst.hits_final += lazyTotals.rst.hits_final, rst.pairs += lazyTotals.rst.pairs;
        }
        size_t const   nSeeds = (size_t)sst.hitsAfterSeeding;

        // ---- _writeRecord + writer
        uint64_t nOut = lazy ? lazyTotals.written : bms.size(); // (--records gpu: every pass's records are cut already)
        if (!recordsOnGpu && !lazy)
        {
            auto const tRec = std::chrono::steady_clock::now();
            nOut      = lx_postprocess_records(bms.data(), bms.size(), opt.maxMatches, &rst);
            msRecords = msSince(tRec);
        }
        std::vector<char const *> qid, sid;
        for (auto const & s : qs.ids)
            qid.push_back(s.c_str());
        for (auto const & s : db.ids)
            sid.push_back(s.c_str());
        lx_seq_names names{qid.data(), qs.orig_len.data(), sid.data(), db.orig_len.data(), qid.size(), sid.size()};
        if (!lazy)
        {
            lx_output_options oo;
            outputOptions(oo);
            // the LCA per query (the reference's _writeRecord, src/search_algo.hpp:884-908), over the records of every worker together
            std::vector<uint64_t> lcaQid;
            std::vector<uint32_t> lcaTax;
            if (indexTax.has)
            {
                if (wantLca && indexTax.hasTree)
                {
                    lcaQid.resize(std::max<uint64_t>(nOut, 1));
                    lcaTax.resize(std::max<uint64_t>(nOut, 1));
                    uint64_t nLca = 0;
                    if (lx_compute_lca(bms.data(), nOut, &tree, lcaQid.data(), lcaTax.data(), &nLca) != LX_OK)
                        throw std::runtime_error("LCA-computation error: One of the paths didn't lead to root.");
                    oo.lca_qid = lcaQid.data();
                    oo.lca_tax = lcaTax.data();
                    oo.n_lca   = nLca;
                }
            }
            if (fmt == LX_OUT_BAM && !outGz && opt.render == "gpu")
            {
                // --render gpu: the records made and compressed on the first device, only the members come down
                lx_handle * zh = nullptr;
                if (lx_create(devices[0], &zh) != LX_OK)
                    throw std::runtime_error(lx_last_error(nullptr));
                std::unique_ptr<lx_handle, void (*)(lx_handle *)> keepH(zh, lx_destroy);
                if (lx_write_bam_dev(zh, opt.output.c_str(), program, bms.data(), nOut, ops.data(), ops.size(), &names,
                                     reinterpret_cast<uint8_t const *>(qs.ascii.data()), qs.ascii_off.data(), &oo) != LX_OK)
                    throw std::runtime_error(std::string("BAM records on the GPU: ") + lx_last_error(zh));
                float msK = 0;
                (void)lx_last_phase_ms(zh, 11, &msK, nullptr);
                msRenderDev = msK;
                renderedOnGpu = true;
            }
            else if (opt.render == "gpu")
            {
                // --render gpu, a text format: the records made on the first device; *.gz compressed there, too
                lx_handle * zh = nullptr;
                if (lx_create(devices[0], &zh) != LX_OK)
                    throw std::runtime_error(lx_last_error(nullptr));
                std::unique_ptr<lx_handle, void (*)(lx_handle *)> keepH(zh, lx_destroy);
                if (lx_write_text_dev(zh, opt.output.c_str(), fmt, outGz ? 1 : 0, program, bms.data(), nOut, ops.data(), ops.size(), &names,
                                      reinterpret_cast<uint8_t const *>(qs.ascii.data()), qs.ascii_off.data(), &oo,
                                      (int64_t)rst.qrys_with_hit) != LX_OK)
                    throw std::runtime_error(std::string("text records on the GPU: ") + lx_last_error(zh));
                float msK = 0;
                (void)lx_last_phase_ms(zh, 12, &msK, nullptr);
                msRenderDev   = msK;
                renderedOnGpu = true;
            }
            else if (fmt == LX_OUT_BAM || outGz)
            {
                // records, footer and header rendered on the host threads, compressed on the device, written at once
                lx_bytes * raw = nullptr;
                if (lx_render_records(fmt, 1, program, bms.data(), nOut, ops.data(), &names, reinterpret_cast<uint8_t const *>(qs.ascii.data()),
                                      qs.ascii_off.data(), &oo, (int64_t)rst.qrys_with_hit, &raw) != LX_OK)
                    throw std::runtime_error(*lx_last_output_error() ? lx_last_output_error() : ("cannot write " + opt.output).c_str());
                std::unique_ptr<lx_bytes, void (*)(lx_bytes *)> keep(raw, lx_bytes_free);
                auto const           tZip = std::chrono::steady_clock::now();
                lx_handle *          zh   = nullptr;
                if (lx_create(devices[0], &zh) != LX_OK)
                    throw std::runtime_error(lx_last_error(nullptr));
                std::unique_ptr<lx_handle, void (*)(lx_handle *)> keepH(zh, lx_destroy);
                std::vector<uint8_t> packed(lx_bgzf_bound(lx_bytes_size(raw)));
                uint64_t             got = 0;
                if (lx_bgzf_compress(zh, lx_bytes_data(raw), lx_bytes_size(raw), packed.data(), packed.size(), &got, LX_BGZF_EOF) != LX_OK)
                    throw std::runtime_error(std::string("BGZF compression: ") + lx_last_error(zh));
                msCompress     = msSince(tZip);
                std::FILE * of = std::fopen(opt.output.c_str(), "wb");
                bool        ok = of && std::fwrite(packed.data(), 1, got, of) == got;
                ok             = of && (std::fclose(of) == 0) && ok;
                if (!ok)
                    throw std::runtime_error("cannot write " + opt.output);
            }
            else
            {
                int const rcw = lx_write_records_ex(opt.output.c_str(), fmt, 1, program, bms.data(), nOut, ops.data(), &names,
                                                    reinterpret_cast<uint8_t const *>(qs.ascii.data()), qs.ascii_off.data(), &oo);
                if (rcw != LX_OK)
                    throw std::runtime_error(*lx_last_output_error() ? lx_last_output_error() : ("cannot write " + opt.output).c_str());
                if (lx_write_footer(opt.output.c_str(), fmt, rst.qrys_with_hit) != LX_OK) // myWriteFooter, src/search.cpp
                    throw std::runtime_error("cannot write " + opt.output);
            }
        }

        std::fprintf(stderr,
                     "lambda3 %s (%s, %u host thread(s), %zu handle(s) on %zu device(s)): %zu queries, %zu subjects (%llu residues); seeds %zu -> promising %zu -> "
                     "windows %llu -> traced %llu -> HSPs %llu -> written %llu (queries with hit: %llu)\n",
                     opt.cmd.c_str(), program, nThreads, nWorkers, devices.size(), lazy ? (size_t)lazyTotals.reads : qs.ids.size(), db.ids.size(), (unsigned long long)dbTotal, nSeeds, nPromising,
                     (unsigned long long)(ist.num_ext_score - ist.hits_duplicate), (unsigned long long)ist.num_ext_ali,
                     (unsigned long long)nHsp, (unsigned long long)nOut, (unsigned long long)rst.qrys_with_hit);
        // where the wall clock went (the reference prints its own at verbosity 2, src/search.cpp): per worker the slowest counts
        std::fprintf(stderr,
                     "lambda3 times [ms]: read %.0f%s, reduce + word table %s%.0f, search %.0f (seeding on the %s %.0f [%zu read(s) and %zu launch(es) left to "
                     "the host] + extension on the GPU incl. widen / merge / statistics %.0f on the slowest worker), records %.1f (%s), records + output %.0f%s, total %.0f\n",
                     msRead, gunzipNote.c_str(), fromIndex ? "(read from the index) " : tableOnGpu ? ("(" + onGpu + ") ").c_str() : "", msIndex, msSearch, anyGpuSeeding ? "GPU" : "host", msSeedMax, nDeclined,
                     nPassesOnHost, msExtendMax, msRecords, recordsOnGpu ? "kernels on the GPU, slowest worker" : "host", msSince(tOut) - msCompress,
                     renderedOnGpu                  ? (std::string(", ") + (fmt == LX_OUT_BAM ? "BAM" : fmt == LX_OUT_SAM ? "SAM" : "tabular") + " records rendered" +
                                                       (fmt == LX_OUT_BAM || outGz ? " and BGZF-compressed" : "") + " on the GPU (render kernels " +
                                                       std::to_string((long)(msRenderDev + 0.5)) + ")").c_str()
                     : (fmt == LX_OUT_BAM || outGz) ? (", BGZF compression on the GPU " + std::to_string((long)(msCompress + 0.5))).c_str()
                                                    : "",
                     msSince(tStart));
        if (lazy)
            std::fprintf(stderr, "lambda3 query blocks: %llu block(s) of at most %llu read(s), %llu read(s) in the largest, at most %llu block(s) alive at once\n",
                         (unsigned long long)lazyTotals.blocks, (unsigned long long)blockReads, (unsigned long long)lazyTotals.largest,
                         (unsigned long long)lazyTotals.maxAlive);
        return 0;
    }
    catch (std::exception const & e)
    {
        std::cerr << "\nERROR: " << e.what() << "\n";
        return -1; // src/search.cpp:98-125
    }
}
