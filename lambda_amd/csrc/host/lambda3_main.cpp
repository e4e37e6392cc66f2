// lambda3_main.cpp -- minimal `lambda3 searchp|searchn|searchbs` front end around liblambda_ext (SURVEY.md section 7 step 9,
// section 8f rows N2/N3): plumbing for BASELINE.json configs[0], not a port of the reference's driver.
//
//   lambda3 searchp -q queries.fasta -d db.fasta -o out.m8 [-e 1e-2] [-n 25] [--seed-length 10] [--seed-offset 5]
//                   [--devices 0,1,...] [-t THREADS] [--table gpu|host|auto] [--table-slice WORDS] [--seeding gpu|host] [--records gpu|host|auto]
//                   [--render gpu|host|auto] [--lca-top-percent P] [--lca gpu|host|auto]
//                   [--taxon-list T1,T2,... | --taxon-exclude T1,T2,...] [--taxon-filter gpu|host|auto]
//                   [--query-masking none|seg] [--masking gpu|host|auto] [--seg-window W] [--seg-k1 X] [--seg-k2 Y]   (searchp)
//                   [--query-masking none|dust] [--masking gpu|host|auto] [--dust-window W] [--dust-level L]          (searchn, searchbs)
//
// --taxon-list / --taxon-exclude (BLAST's -taxids / -negative_taxids, DIAMOND's --taxonlist / --taxon-exclude): search only the
// subjects under the listed taxa of the index's tree (mkindex* -m -x), or all but them.  lx_tax_subject_mask has the rule: a taxon is
// under the list if its chain of parents holds a listed taxon, a subject is hit if one of its taxa is; a subject without taxa is
// dropped by a list and kept by an exclusion.  The mask is made once per worker; in every pass the promising seeds (the match list
// of lx_seed_queries) on unwanted subjects are dropped before lx_iterate_matches*, so they cost no extension and take none of a
// query's -n places.  --taxon-filter: gpu = the mask by kernels over the tree resident on the worker's device
// (lx_subject_mask_create_dev) and a device match list compacted where it stands (lx_seed_result_filter); host = the mask by
// lx_tax_subject_mask, a device list brought down and the pass run from host memory; auto = where the pass's list stands.  A list
// in host memory (--seeding host) is always filtered there.  What is stated: e-values and bit scores keep the WHOLE database's length,
// as BLAST's -taxids does; with --search0 1 the "read had a result" decision is made on the filtered results, so a read whose hits
// all lie outside the list goes on to the second pass; the stage counters keep their meaning ("promising" counts the seeds before
// the filter) and one more stderr line names the kept subjects, the dropped seeds, the place and the time.  The seeding itself does
// not know the list, and it thins a read's seeds towards -n matches (adaptive elongation, the over-abundance cut): so that the
// dropped subjects cannot use that budget up, with a list it aims at -n + the number of dropped subjects, capped at the 64 matches
// per read a device launch has room for (never below -n: from -n 64 on the seeding is exactly the unrestricted run's; below it a
// list can find kept subjects that the unrestricted run's thinning loses).  Refused while the options
// are parsed: both options, an empty list, anything but numbers 1 .. 2^32 - 1, --taxon-filter without a list.  Refused once the index
// is read: an index (or a -d FASTA database) without subject taxa and tree, and a --taxon-list taxon that the index's tree does not
// hold (the reference's tree skips unassigned taxa with one child); --taxon-exclude of such a taxon is a warning.
//
// --query-masking seg (searchp; default none: nothing is masked and every byte of output is what it was): low-complexity query regions
// are masked before seeding, as BLAST does with SEG on the translated frames of blastx / tblastn queries.  Soft masking: a masked letter
// starts and carries no seed; pre-scoring, extension, statistics and output read the unmasked query.  The rule (lx_query_mask_create_seg)
// is SEG's first two stages on alignment ranks in integers -- windows of --seg-window letters (4 .. 64, default 12) with at most --seg-k2
// bits of entropy (default 2.5) form runs, a run that holds a window with at most --seg-k1 bits (default 2.2; 0 < k1 <= k2 <= log2 W)
// masks every letter its windows cover --, WITHOUT SEG's third stage, the trimming of each raw segment: a mask is SEG's segment or a few
// letters wider, and is not NCBI segmasker's.  The mask is made once per query set after frame expansion (--lazy-query: once per block)
// and both passes (--search0 and the main search) seed with it.  --masking: gpu = by kernels on the worker's device, where the seeding
// kernel reads it; host = on the -t threads (and uploaded where the seeding runs on the device); auto = where --seeding runs (profiles/query_mask_bench.txt:
// 10^6 reads x 6 frames x 50 letters take 147 ms on 16 host threads and 76 ms on the device, upload included; the kernels 27 ms).  One line on stderr reports the parameters, the letters masked, the sequences touched, the
// place and the time.  Refused while the options are parsed: --query-masking seg on searchn / searchbs (SEG is the protein rule; theirs
// is dust, below), --masking or --seg-* without --query-masking seg, parameters outside the ranges.
//
// --query-masking dust (searchn, searchbs; default none): the same soft masking with the nucleotide rule (lx_query_mask_create_dust),
// symmetric DUST (Morgulis et al. 2006) in integers: within a maximal stretch of A, C, G, T letter i starts the triplet of letters i,
// i + 1, i + 2; an interval of l consecutive triplets covers l + 2 letters and scores r / (l - 1), r = the sum over the 64 triplet kinds
// of c (c - 1) / 2 with c the kind's count in the interval; a letter is masked exactly when it lies in an interval of at most
// --dust-window letters (4 .. 64, default 64) whose score is above --dust-level / 10 (1 .. 1000, default 20) and which holds no
// sub-interval that scores strictly higher.  N is never masked and ends every interval.  The defaults are dustmasker's and sdust's; its
// -linker (joining masked intervals one letter apart) is NOT built, and no mask was compared with dustmasker's or sdust's output: what is
// claimed is the rule as stated.  The mask is made on the read's own letters after frame expansion (searchbs: the unreduced letters;
// the bisulfite reduction differs per frame), once per query set or lazy block, for both passes.  --masking as above (profiles/dust_mask_bench.txt: 10^6 reads x 2 frames x 150 letters take 1944 ms on 16 host threads and 39 ms on the device, upload included; the kernels 26 ms).  The report line reads "dust W/L" for the
// parameters.  Refused while the options are parsed: --query-masking dust on searchp, --dust-* without --query-masking dust, --masking
// on searchn / searchbs without it, --seg-* on searchn / searchbs, --dust-window outside 4 .. 64, --dust-level outside 1 .. 1000.
//
// --lca-top-percent P (0 .. 100, default 100): which records of a query enter its LCA (lcataxid, lt, ls).  100 is the reference's
// rule, every record (src/search_algo.hpp:884-907); below it only the records whose bit score lies within P percent of the query's
// best one (MEGAN's "top percent", DIAMOND's --top), 0 the best ones alone: lx_compute_lca_ex has the rule.  --lca: where the fold
// runs.  host: lx_compute_lca_ex on the thread that has the records.  gpu: lx_compute_lca_dev -- the tree resident on the device, one
// lane per query -- on a handle on the first device (the eager path) or on the handle of the worker that searched the block
// (--lazy-query; one resident tree per worker, made at its first block).  The output is byte-identical either way.  auto = gpu:
// DESIGN.md (4.12.1, "The LCA on the device") has the measurement and the rule.  Where --lca gpu or --lca-top-percent was given, a
// line of its own on stderr names the rule, the place and the time.
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
// The LCA (--lca) and the writers (--render) are fed with the kept records; the output is byte-identical either way.
//
// --max-hsps K, --culling-limit L (numbers >= 0, default 0 = off; BLAST's -max_hsps and -culling_limit, the reference has neither):
// which of a query's records take the -n places.  Between _writeRecord's unique and its cut, per query, over the records in output
// order (bit score descending, ties by place in the first order; a record is BETTER than another when it comes earlier): with K > 0 a
// record is dropped when at least K better records have the same subject; then, over what is left, with L > 0 a record is dropped
// when at least L better records have a query interval that envelops its own -- the interval is qstart .. qend as the .m8 prints
// them (nucleotide positions for BLASTX, mirrored on the minus strand), equal intervals envelop each other, a partial overlap never
// culls.  Then the cut to -n as always.  The rules run wherever the step runs (--records gpu: two more counting kernels of
// lx_toprec.hip behind lx_iterate_matches_dev_top_ex; the host step of the eager path, of a --lazy-query block, and of a pass whose
// list stands in host memory: lx_postprocess_records_ex); every record of a query comes out of one call or one block, so the rules
// see all of them.  The output is byte-identical wherever they ran.  -n 0 keeps its meaning.  The seeding's budget stays -n: a
// query whose seeding stopped at -n matches per read has no more records to promote.  With either option a line of its own on
// stderr names K, L, what each rule dropped and where the step ran.
//
// --lazy-query 1 [--query-block N]: the query file block by block, in bounded memory -- the reference's batch loop with its reader
// thread behind a bounded queue (src/search.cpp:389-459, src/search_algo.hpp:374-413).  One reader takes the file as a stream
// (lx_gunzip_stream: BGZF groups and plain members of 8 MiB and more on the first device, other members on its thread), parses it piece by piece
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
// (src/search_algo.hpp:342) unless --sam-bam-qual yes asks for them; bzip2 is refused.
//
// --sam-bam-qual no|yes (search*, .sam / .sam.gz / .bam; default no: every byte of output is what it was, QUAL '*' / 0xFF; the
// reference has no such option): a FASTQ query's base qualities are kept by the parser (a byte outside '!' .. '~' in a quality line
// is refused with the file, the read and the byte) and written as QUAL exactly where SEQ is written -- the rule of --sam-bam-seq
// decides whether, the window of --sam-bam-clip which letters, the minus strand reverses (and does not complement) them; a
// translated query's are those of the nucleotides [3a + |f| - 1, 3e + |f| - 1) of the strand that was read; a record whose SEQ is
// '*' has QUAL '*'.  SAM carries the Phred+33 characters, BAM the values.  Both paths pass them: the eager writers in
// lx_output_options::q_qual, a --lazy-query block its own through lx_out_append_ex; --render gpu | host | auto give the same bytes
// (the rule of auto does not change).  Under yes a sequence set, and so a lazy block, holds its letters twice: the letters and as
// many quality bytes.  A FASTA query under yes is accepted: one line on stderr says that the file has no qualities, QUAL stays '*'.
// Refused while the options are parsed: yes with an output that is not SAM or BAM, and yes with --sam-bam-seq never (QUAL goes
// where SEQ goes).
//
// What it mirrors from the reference, and what it does not:
//   * subcommand split and the search command line (src/lambda.cpp:30-118; src/search_options.hpp:143-816): -q, -o (format from
//     the extension, :684-710), -e, --bit-score, --percent-identity, -n, the seeding options (--seed-length/-offset/-delta[0],
//     --search0, --adaptive-seeding, --seed-half-exact), --pre-scoring[-threshold], the scoring options (-s 45|62|80 for
//     proteins, --score-match/-mismatch for nucleotides, --score-gap, --score-gap-open), the profiles (-p fast | sensitive |
//     pairs-default | pairs-sensitive: they overwrite the seeding options, :634-681), the output options (--output-columns,
//     --sam-bam-tags/-seq/-clip (and this front end's --sam-bam-qual), --sam-with-refheader, --version-to-outputfile), -g, --input-alphabet;
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
//
// The source: cli/options.hpp (the command line), cli/sequences.hpp (input files, sequence sets, the query stream, the reduction),
// cli/index_file.hpp (the index file and its taxonomy), cli/common.hpp (owners, clock, sums); this file holds the stages of a run,
// each a function or a small class that is handed what it reads, and main(), which calls them in turn.
#include <sched.h>

#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <functional>
#include <iostream>
#include <map>
#include <mutex>

#include "blast_stats.hpp"
#include "cli/common.hpp"
#include "cli/index_file.hpp"
#include "cli/options.hpp"
#include "cli/sequences.hpp"

namespace
{

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

bool hasWord(std::string const & list, char const * w) // `w` is one of the blank-separated words of `list`
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
}

// ---- the facts of a run, derived once: the first half from the options alone, the second by loadInputs from what the files hold
struct Run
{
    Clock::time_point tStart = Clock::now();
    bool              mk, prot, bs;
    bool              fromIndex;  // -i / -d names an index made by `lambda3 mkindex*`, or the database as FASTA (the table is then made in memory)
    bool              lazy;       // --lazy-query 1 / --query-block N: the query file block by block (the header comment); --query-block 0 = the eager path
    uint64_t          blockReads; // (the default is not measured yet: DESIGN.md 5.1)
    int               firstDevice;
    // search* decodes BGZF members on the first device of --devices, mkindex* on the host unless --table gpu already asks for a device
    int               gunzipDevice;
    unsigned          nThreads;
    bool              wantLca; // taxonomy columns (src/search_options.hpp:736-820): lcataxid, lt or ls ask for the LCA
    int               outFmt = LX_OUT_BLAST_TAB;
    bool              outGz = false, wantOps = false; // only the SAM writer reads alignment columns (its CIGAR); the tables are made from the counts
    bool              recordsOnGpu; // --records (the header comment): auto = host -- the measured rule of DESIGN.md ("_writeRecord on the device")

    // searchp with nucleotide queries is BLASTX: six translated frames per query against the protein database;
    // searchp against a nucleotide database translates the subjects instead (TBLASTN), or both sides (TBLASTX)
    bool         blastx = false, sTrans = false;
    // genetic code: the subjects' is the index's; the queries' is -g, else the index's (src/search.cpp:157-178)
    int          geneticCodeDb = 1, geneticCodeQry = 1;
    int          qFrames = 1, sFrames = 1; // frames per sequence, src/search_datastructures.hpp:380-385
    char const * program = "";
    std::string  reduction;
    Reduction    red;

    explicit Run(Options const & opt)
    {
        mk           = opt.cmd.rfind("mkindex", 0) == 0;
        prot         = opt.cmd == "searchp" || opt.cmd == "mkindexp";
        bs           = opt.cmd == "searchbs" || opt.cmd == "mkindexbs";
        fromIndex    = !mk && isIndexFile(opt.db);
        lazy         = !mk && (opt.queryBlockGiven ? opt.queryBlock > 0 : opt.lazyQuery);
        blockReads   = opt.queryBlock ? opt.queryBlock : (1ull << 20);
        firstDevice  = opt.devices.empty() ? 0 : opt.devices[0];
        gunzipDevice = (!mk || opt.table == "gpu") ? firstDevice : -1;
        nThreads     = opt.threads > 0 ? (unsigned)opt.threads : grantedThreads();
        wantLca      = !mk && (hasWord(opt.outputColumns, "lcataxid") || hasWord(opt.samTags, "lt") || hasWord(opt.samTags, "ls"));
        if (!mk)
            outFmt = outputFormat(opt.output, outGz);
        wantOps      = outFmt == LX_OUT_SAM || outFmt == LX_OUT_BAM;
        recordsOnGpu = opt.records == "gpu" && opt.maxMatches > 0;
    }
};

// ---- input loading
struct Inputs
{
    alignas(64) SeqSet           qs; // (two threads fill the two sets at once: each begins a cache line of its own)
    alignas(64) SeqSet           db;
    IndexFileOptions             ifo;
    FileOwner                    indexFile; // -i: the index file, open behind its head (closed on every way out)
    std::unique_ptr<QueryStream> qStream;   // --lazy-query: the query file stays a stream (its first pieces are here: format, alphabet)
    double                       msRead = 0;
    std::string                  gunzipNote;
};

// the index fixes the domain (src/search.cpp:189-207)
void refuseOtherDomain(Run const & run, IndexFileOptions const & ifo)
{
    if (run.prot && ifo.transAlph != kAlphAminoAcid)
        throw std::runtime_error("Attempting to use nucleotide or bisulfite index for protein search.");
    if (!run.prot && ifo.transAlph != kAlphDna5)
        throw std::runtime_error(run.bs ? "Attempting to use protein index for bisulfite search." : "Attempting to use protein index for nucleotide search.");
    if (!run.prot && !run.bs && ifo.redAlph != kAlphDna4)
        throw std::runtime_error("Attempting to use bisulfite index for nucleotide search.");
    if (run.bs && ifo.redAlph != kAlphDna3Bs)
        throw std::runtime_error("Attempting to use nucleotid index for bisulfite search.");
}

// the query file's half of a loading phase on a second thread beside the database's half on this one (two files, two threads; -t 1
// keeps it to one: the query's half first); the database's error counts first, the thread is joined on every way out
template <class Q, class D>
void sideBySide(bool withQuery, bool secondThread, Q && queryHalf, D && dbHalf)
{
    std::string error;
    auto        guarded = [&]()
    {
        try
        {
            queryHalf();
        }
        catch (std::exception const & e)
        {
            error = e.what();
        }
    };
    {
        std::thread      t;
        JoinOnExit const join(t);
        if (withQuery && secondThread)
            t = std::thread(guarded);
        else if (withQuery)
            guarded();
        dbHalf();
    }
    if (!error.empty())
        throw std::runtime_error(error);
}

// --sam-bam-qual yes and a query file without qualities: said once
char const * const kNoQualNote = "--sam-bam-qual yes: the query file has no qualities (FASTA); QUAL is written as '*'\n";

// the two phases of loading: the files' bytes, decompressed (a handle each), then -- once the bytes have settled the alphabets, the
// second half of `run` -- their records into sequence sets.  --lazy-query leaves the query file a stream; -i has read the subjects.
Inputs loadInputs(Options const & opt, Run & run)
{
    Inputs in;
    if (run.fromIndex)
    {
        FILE * f = nullptr;
        readIndexHead(opt.db, in.ifo, in.db, &f);
        in.indexFile.reset(f);
        refuseOtherDomain(run, in.ifo);
    }
    if (run.lazy)
        in.qStream.reset(new QueryStream(opt.query, run.gunzipDevice, opt.samQual));
    bool const eagerQuery = !run.mk && !run.lazy, secondThread = opt.threads != 1;
    InputText  qIn, dIn;
    sideBySide(
        eagerQuery, secondThread, [&]() { qIn = readInput(opt.query, run.gunzipDevice); },
        [&]()
        {
            if (!run.fromIndex)
                dIn = readInput(opt.db, run.gunzipDevice);
        });

    IndexFileOptions const & ifo = in.ifo;
    bool const               fromIndex = run.fromIndex, prot = run.prot, bs = run.bs;
    run.reduction = !fromIndex ? opt.reduction : ifo.redAlph == kAlphLi10 ? "li10" : ifo.redAlph == kAlphMurphy10 ? "murphy10" : "none";
    run.red       = chooseReduction(prot, bs, run.reduction);
    run.blastx    = !run.mk && prot &&
                 (opt.qryAlphabet == "dna5" || (opt.qryAlphabet == "auto" && (run.lazy ? in.qStream->looksLikeDna() : looksLikeDna(qIn.text, opt.query))));
    run.sTrans = fromIndex ? (prot && ifo.origAlph != ifo.transAlph)
                           : prot && (opt.dbAlphabet == "dna5" || (opt.dbAlphabet == "auto" && looksLikeDna(dIn.text, opt.db)));
    run.geneticCodeDb  = fromIndex ? (int)ifo.geneticCode : opt.geneticCode;
    run.geneticCodeQry = (opt.geneticCodeGiven || !fromIndex || !run.sTrans) ? opt.geneticCode : (int)ifo.geneticCode;
    if (fromIndex && run.sTrans && run.geneticCodeQry != run.geneticCodeDb)
        std::cerr << "WARNING: The genetic code used when creating the index: " << run.geneticCodeDb
                  << "\n         is not the same as now selected for the query sequences: " << run.geneticCodeQry
                  << "\n         Are you sure this is what you want?\n";
    run.qFrames = bs ? 4 : run.blastx ? 6 : prot ? 1 : 2;
    run.sFrames = bs ? 2 : run.sTrans ? 6 : 1;
    run.program = run.blastx ? (run.sTrans ? "tblastx" : "blastx") : run.sTrans ? "tblastn" : prot ? "blastp" : "blastn";

    sideBySide(
        eagerQuery, secondThread, [&]() { readFasta(qIn.text, opt.query, prot, !prot, in.qs, run.blastx, run.geneticCodeQry, bs ? 2 : 0, opt.samQual); },
        [&]()
        {
            if (fromIndex)
                return;
            size_t const first = dIn.text.find_first_not_of(" \t\r\n\v\f");
            if (first != std::string::npos && dIn.text[first] != '>' && dIn.text[first] != '@')
                throw std::runtime_error(opt.db + " is neither a FASTA file nor an index of this front end (nor FASTQ, plain or gzip-compressed; an index written by the reference -- a cereal "
                                         "archive of an fmindex-collection FM-index -- cannot be read here: run lambda3 mkindexp|mkindexn|mkindexbs on the FASTA file)");
            readFasta(dIn.text, opt.db, prot, false, in.db, run.sTrans, run.geneticCodeDb, bs ? 1 : 0);
        });
    if ((eagerQuery && in.qs.ids.empty()) || in.db.ids.empty())
        throw std::runtime_error("empty query or database file");
    if (eagerQuery && opt.samQual && !qualOf(in.qs))
        std::cerr << kNoQualNote;
    if (fromIndex && in.db.off.size() != in.db.ids.size() * (size_t)run.sFrames)
        throw std::runtime_error("index file " + opt.db + ": the frames of its sequences do not fit its alphabets");
    if (run.mk && opt.truncateIds) // src/mkindex_algo.hpp:123
        for (std::string & id : in.db.ids)
            id.resize(std::min(id.size(), id.find_first_of(" \t")));
    in.msRead = msSince(run.tStart);
    double const   msGunzip     = std::max(qIn.msGunzip, dIn.msGunzip);
    uint64_t const plainMembers = qIn.plainMembers + dIn.plainMembers, plainChunks = qIn.plainChunks + dIn.plainChunks;
    if (msGunzip > 0)
        in.gunzipNote = " (gzip decompression " + std::string(qIn.onDevice || dIn.onDevice ? "of BGZF on the GPU " : "on the host ") +
                        std::to_string((long)(msGunzip + 0.5)) +
                        (plainMembers ? ", " + std::to_string(plainMembers) + " plain member(s) in " + std::to_string(plainChunks) + " chunks on the GPU" : std::string()) + ")";
    return in;
}

// ---- the word table over the reduced database (the FM-index's place; Level 3 of include/lambda_ext.h): made or loaded with the first
// device's handle where the seeding or the table is the GPU's -- table and reduced subjects then stay on that device, and worker 0
// works with that handle --, else on the -t host threads
struct Table
{
    HandleOwner   firstHandle; // (declared in front of the table: an index is destroyed before the handle it was made with)
    IndexOwner    ix;
    bool          tableOnGpu  = false;
    int           tableSlices = 0; // (> 0: the GPU made the table in that many slices)
    double        msIndex     = 0;
    IndexTaxonomy indexTax;

    std::string onGpu() const { return tableSlices > 0 ? "on the GPU in " + std::to_string(tableSlices) + " slices" : "on the GPU"; }
};

// -i: the table's bytes from the index file, then the file's taxonomy section
void loadWordTable(Options const & opt, Run const & run, SeqSet const & db, std::vector<uint8_t> const & dbRed, FileOwner & indexFile, Table & t)
{
    std::vector<uint8_t> bytes;
    bool                 ok  = readIndexTable(indexFile.get(), totalLetters(db), bytes);
    lx_index *           raw = nullptr;
    if (ok && opt.seeding == "gpu" && lx_device_count() > 0)
        t.firstHandle = makeHandle(run.firstDevice, "lambda_ext: ");
    if (ok && t.firstHandle && lx_index_load(t.firstHandle.get(), bytes.data(), bytes.size(), dbRed.data(), db.off.data(), db.len.data(), db.off.size(), &raw) != LX_OK)
        t.firstHandle.reset(); // (no room on the device, 2^32 - 1 entries or more, ...: the host copy alone; a table that is wrong fails again below)
    ok = ok && (raw || lx_index_load(nullptr, bytes.data(), bytes.size(), dbRed.data(), db.off.data(), db.len.data(), db.off.size(), &raw) == LX_OK);
    t.ix.reset(raw);
    lx_index_info info{};
    ok = ok && lx_index_get_info(raw, &info) == LX_OK && info.alph == run.red.alph;
    if (!ok)
        throw std::runtime_error("index file " + opt.db + ": the word table is truncated or does not fit the sequences");
    readIndexTaxonomy(opt.db, indexFile.get(), db.ids.size(), t.indexTax);
    indexFile.reset();
    // an LCA needs the tree (src/search_algo.hpp:309-313); an index without any taxonomy keeps printing "*" and 0
    if (run.wantLca && t.indexTax.has && !t.indexTax.hasTree)
        throw std::runtime_error("You requested taxonomic binning, but the index does not contain a taxonomic tree. Recreate it and provide --tax-dump-dir .");
}

// -d: on the GPU (keys, one radix sort, prefix table: lx_seed.hip) where there is one to take it, else on the -t host threads;
// the same table either way.  The GPU makes it in slices of the key space where --table-slice says so, where the set has
// 2^31 words or more (beyond one sort) and, once, where one sort's memory is more than the device has left.
void buildWordTable(Options const & opt, Run const & run, SeqSet const & db, std::vector<uint8_t> const & dbRed, Table & t)
{
    bool const gpuSeedingWanted = !run.mk && opt.seeding == "gpu";
    bool const wantGpu          = opt.table == "gpu" || (opt.table == "auto" && !run.mk);
    lx_index * raw              = nullptr;
    if (wantGpu && lx_device_count() > 0)
    {
        t.firstHandle             = makeHandle(run.firstDevice, "lambda_ext: ");
        lx_handle * const h       = t.firstHandle.get();
        uint64_t const kAutoSlice = 1ull << 30;
        uint64_t       slice      = opt.tableSlice ? opt.tableSlice : totalLetters(db) >= (1ull << 31) ? kAutoSlice : 0;
        auto           build      = [&]()
        {
            if (slice && lx_set_option(h, LX_OPT_INDEX_SLICE_WORDS, slice) != LX_OK)
                throw std::runtime_error(std::string("lambda_ext: ") + lx_last_error(h));
            return lx_index_build(h, dbRed.data(), db.off.data(), db.len.data(), db.off.size(), run.red.alph, run.nThreads, &raw);
        };
        int rc = build();
        if (rc == LX_ENOMEM && !slice)
        {
            slice = kAutoSlice;
            rc    = build();
        }
        t.tableOnGpu  = rc == LX_OK;
        float msTable = 0;
        if (t.tableOnGpu && slice && lx_last_phase_ms(h, 8, &msTable, &t.tableSlices) != LX_OK)
            t.tableSlices = 0;
        if (rc != LX_OK && rc != LX_EINVAL && rc != LX_ENOMEM) // (too large for the device build or for its memory: the host threads make it)
        {
            if (opt.table == "gpu")
                throw std::runtime_error(std::string("lambda_ext: ") + lx_last_error(h));
            std::cerr << "WARNING: the word table is made on the host threads (" << lx_last_error(h) << ")\n";
        }
    }
    else if (opt.table == "gpu")
        throw std::runtime_error("--table gpu: no HIP device available");
    if (!t.tableOnGpu)
    {
        if (lx_index_build(nullptr, dbRed.data(), db.off.data(), db.len.data(), db.off.size(), run.red.alph, run.nThreads, &raw) != LX_OK)
            throw std::runtime_error(std::string("lambda_ext: ") + lx_last_output_error());
        lx_index * att = nullptr;
        // the seeding is the GPU's all the same: the host-made table becomes resident
        if (t.firstHandle && gpuSeedingWanted && lx_index_attach(raw, t.firstHandle.get(), &att) == LX_OK)
        {
            lx_index_destroy(raw);
            raw = att;
        }
        else
            t.firstHandle.reset();
    }
    t.ix.reset(raw);
}

Table makeWordTable(Options const & opt, Run const & run, SeqSet const & db, FileOwner & indexFile)
{
    if (!run.mk || opt.table == "gpu") // (before the first device is touched: the library's own wording)
        for (int d : opt.devices)
            if (d < 0 || d >= lx_device_count())
                throw std::runtime_error("device_id " + std::to_string(d) + " out of range [0," + std::to_string(lx_device_count()) + ")");
    auto const                 tIndex = Clock::now();
    Table                      t;
    std::vector<uint8_t> const dbRed = reduce(db, run.red); // (the index keeps its own copy)
    if (run.fromIndex)
        loadWordTable(opt, run, db, dbRed, indexFile, t);
    else
        buildWordTable(opt, run, db, dbRed, t);
    t.msIndex = msSince(tIndex);
    return t;
}

// ---- mkindexp | mkindexn | mkindexbs (src/mkindex.cpp): the options that fix the types, ids, sequences, table -> one file
int runMkindex(Options const & opt, Run const & run, Inputs const & in, Table const & table)
{
    bool const       prot = run.prot;
    IndexFileOptions out;
    out.indexType   = opt.dbIndexType == "bifm" ? 1 : 0;
    out.origAlph    = prot ? (run.sTrans ? kAlphDna5 : kAlphAminoAcid) : kAlphDna5; // :206-224, :235
    out.transAlph   = prot ? kAlphAminoAcid : kAlphDna5;
    out.redAlph     = run.bs ? kAlphDna3Bs : !prot ? kAlphDna4 : run.reduction == "li10" ? kAlphLi10 : run.reduction == "murphy10" ? kAlphMurphy10 : kAlphAminoAcid;
    out.geneticCode = (uint8_t)run.geneticCodeDb;
    std::string const hostThreads = std::to_string(run.nThreads) + " host thread(s)";
    IndexTaxonomy     tax;
    if (!opt.accTaxMap.empty())
    {
        // the join on the device under --table gpu, else on the -t host threads (the same bytes either way)
        HandleOwner const th      = opt.table == "gpu" ? makeHandle(run.firstDevice) : HandleOwner();
        double            msTax   = 0;
        float             msKernel = 0;
        buildIndexTaxonomy(opt.accTaxMap, opt.taxDumpDir, in.db.ids, th.get(), run.nThreads, tax, msTax, msKernel);
        std::string const where = th ? "join on the GPU, kernels " + std::to_string((long)(msKernel + 0.5)) : hostThreads;
        std::fprintf(stderr, "lambda3 times [ms]: taxonomy %.0f (%s)\n", msTax, where.c_str());
    }
    auto const tWrite = Clock::now();
    writeIndexFile(opt.index, out, in.db, table.ix.get(), tax);
    std::fprintf(stderr,
                 "lambda3 %s: %zu sequences (%llu residues in %d frame(s); original alphabet %s, translated %s, reduced %s, genetic code %d) -> %s\n"
                 "lambda3 times [ms]: read %.0f%s, reduce + word table %.0f (%s), write %.0f, total %.0f\n",
                 opt.cmd.c_str(), in.db.ids.size(), (unsigned long long)totalLetters(in.db), run.sFrames, alphName(out.origAlph), alphName(out.transAlph),
                 alphName(out.redAlph), (int)out.geneticCode, opt.index.c_str(), in.msRead, in.gunzipNote.c_str(), table.msIndex,
                 table.tableOnGpu ? table.onGpu().c_str() : hostThreads.c_str(), msSince(tWrite), msSince(run.tStart));
    return 0;
}

// ---- what every worker of a search is told: scoring + statistics, the parameters of Level 2, the seeds of both passes, the devices
struct SearchSetup
{
    lx_scoring             sc, scRev; // bisulfite = two matrices over SeqAn Dna5 (forward: slot 0, reverse: slot 1, :176-186)
    lx_search_params       sp{};
    lambda_amd::SeedParams so0, so1; // the exact pre-search (--search0), the search proper
    // one worker = one handle per entry of --devices (a device may be listed twice); -t host threads in all, shared out among
    // the workers for the seeding of their reads (the reference: -t OpenMP threads, each with its own LocalDataHolder; a GPU
    // wants few, large extension batches, the seeding wants every core)
    std::vector<int>       devices;
    size_t                 nWorkers    = 1;
    unsigned               seedThreads = 1;
};

SearchSetup prepareSearch(Options const & opt, Run const & run, Inputs const & in)
{
    SearchSetup s;
    bool const  prot = run.prot, bs = run.bs;
    // scoring + statistics (prepareScoring, src/search_algo.hpp:166-234): statistics from the match / mismatch scheme
    lambda_amd::builtinScoring(prot ? opt.scoringMethod : bs ? -1 : 0, opt.match, opt.misMatch, opt.gapOpen, opt.gapExtend, s.sc);
    if (bs)
        lambda_amd::builtinScoring(-2, opt.match, opt.misMatch, opt.gapOpen, opt.gapExtend, s.scRev);
    if (!lambda_amd::karlinParams(prot ? opt.scoringMethod : 0, opt.match, opt.misMatch, opt.gapOpen, opt.gapExtend, s.sp.karlin))
        throw std::runtime_error("Could not compute Karlin-Altschul-Values for Scoring Scheme."); // :232-233

    // devices and worker threads (src/search.cpp:379-385: one LocalDataHolder per thread; here one handle per thread)
    s.devices = opt.devices;
    if (s.devices.empty())
        for (int d = 0; d < lx_device_count(); ++d)
            s.devices.push_back(d);
    if (s.devices.empty())
        throw std::runtime_error("no HIP device available (this front end has no CPU path)");
    s.nWorkers    = run.lazy ? s.devices.size() : std::max<size_t>(1, std::min<size_t>(s.devices.size(), in.qs.ids.size()));
    s.seedThreads = std::max(1u, run.nThreads / (unsigned)s.nWorkers);

    s.sp.max_evalue       = opt.maxEValue;
    s.sp.min_bitscore     = opt.minBitScore;
    s.sp.id_cutoff        = opt.idCutOff;
    s.sp.db_total_length  = totalLetters(in.db); // dbTotalLength = sum of the (frame-expanded) subject lengths, src/search_algo.hpp:317-319
    s.sp.query_translated = run.blastx ? 1 : 0;
    s.sp.qry_num_frames   = run.qFrames;
    s.sp.sbj_num_frames   = run.sFrames;
    s.sp.bisulfite        = bs ? 1 : 0;
    s.sp.q_frame_mode     = bs ? LX_FRAMES_BISULFITE : run.blastx ? LX_FRAMES_TRANSLATED : prot ? LX_FRAMES_NONE : LX_FRAMES_REVCOMP; // _setFrames, :768-814
    s.sp.s_frame_mode     = bs ? LX_FRAMES_BISULFITE : run.sTrans ? LX_FRAMES_TRANSLATED : LX_FRAMES_NONE;
    s.sp.flags            = run.wantOps ? 0 : LX_ITERATE_NO_OPS;
    s.so1 = lambda_amd::SeedParams{opt.seedLength, opt.seedOffset, opt.seedDelta};
    s.so0 = lambda_amd::SeedParams{opt.seedLength0, opt.seedOffset0, opt.seedDelta0};
    return s;
}

// ---- --taxon-list / --taxon-exclude: the list against the index's taxonomy, once the index is read.  The host rule
// (lx_tax_subject_mask) says which listed taxa the tree knows and gives the mask's words: the mask of --taxon-filter host and of
// every pass whose match list stands in host memory, and the kept count of the stderr line.
struct TaxonSetup
{
    bool                  on = false;
    lx_tax_tree           tree{};
    lx_taxon_filter       filter{};
    std::vector<uint64_t> words;
    uint64_t              nSubjects = 0, nKept = 0;

    TaxonSetup(Options const & opt, Run const & run, IndexTaxonomy const & tax)
    {
        if (opt.taxonList.empty())
            return;
        if (!run.fromIndex || !tax.has || !tax.hasTree)
            throw std::runtime_error(std::string(opt.taxonExclude ? "--taxon-exclude" : "--taxon-list") +
                                     ": the index has no taxonomy: build it with mkindex* -m and -x");
        on             = true;
        tree.parents   = tax.parents.data();
        tree.heights   = tax.heights.data();
        tree.n_taxa    = tax.parents.size();
        tree.s_tax_off = tax.off.data();
        tree.s_tax_ids = tax.ids.data();
        tree.n_s       = tax.off.size() - 1;
        filter         = lx_taxon_filter{opt.taxonList.data(), opt.taxonList.size(), opt.taxonExclude ? 1 : 0, 0};
        nSubjects      = tree.n_s;
        words.assign((nSubjects + 63) / 64, 0);
        std::vector<uint8_t> known(opt.taxonList.size(), 0);
        if (lx_tax_subject_mask(&tree, &filter, words.data(), &nKept, known.data()) != LX_OK)
            throw std::runtime_error(std::string("the taxon list: ") + lx_last_output_error());
        for (size_t i = 0; i < known.size(); ++i)
        {
            if (known[i])
                continue;
            std::string const what = "taxon " + std::to_string(opt.taxonList[i]) +
                                     ": the index's tree does not hold it (it has no subjects there, or the tree skipped it as an unassigned taxon with one "
                                     "child: name a taxon above or below it)";
            if (!opt.taxonExclude)
                throw std::runtime_error("--taxon-list " + what);
            std::cerr << "WARNING: --taxon-exclude " << what << "\n";
        }
    }
};

// everything a search stage reads, none of which changes once the search begins
struct SearchContext
{
    Options const &     opt;
    Run const &         run;
    SearchSetup const & setup;
    SeqSet const &      db;
    Table const &       table;
    TaxonSetup const &  taxon;
};

// --max-hsps / --culling-limit as the library takes them, over the queries that the records' n_qid name (their untranslated lengths)
lx_cull_options cullOptions(Options const & opt, Run const & run, SeqSet const & qs)
{
    lx_cull_options co;
    lx_cull_options_default(&co);
    co.max_hsps = opt.maxHsps, co.culling_limit = opt.cullingLimit;
    co.q_lens = qs.orig_len.data(), co.n_q = qs.orig_len.size(), co.q_translated = run.blastx ? 1 : 0;
    return co;
}

// _writeRecord's step on the host, with the two rules where they were asked for: the new count
uint64_t hostRecordsStep(Options const & opt, Run const & run, SeqSet const & qs, lx_blast_match * m, uint64_t n, lx_record_stats * rst, lx_cull_stats * cst)
{
    if (!opt.maxHsps && !opt.cullingLimit)
        return lx_postprocess_records(m, n, opt.maxMatches, rst);
    lx_cull_options const co   = cullOptions(opt, run, qs);
    int64_t const         kept = lx_postprocess_records_ex(m, n, opt.maxMatches, &co, rst, cst);
    if (kept < 0)
        throw std::runtime_error(std::string("lambda_ext: ") + lx_last_output_error());
    return (uint64_t)kept;
}

// what a worker keeps for its range of reads (--lazy-query: for its blocks, whose records stay with them)
struct Part
{
    std::vector<lx_blast_match> bms;
    std::vector<uint8_t>        ops;
    lx_iterate_stats            ist{};
    lambda_amd::SeedingStats    sst{};
    size_t                      nPromising = 0;
    double                      msSeed = 0, msExtend = 0, msRecords = 0;
    double                      msLca = 0; // (--lazy-query: the LCA of this worker's blocks)
    lx_record_stats             rst{}; // --records gpu: _writeRecord's statistics of this worker's passes
    lx_cull_stats               cst{}; // ... and what --max-hsps / --culling-limit dropped there
    bool                        gpuSeeding = false; // the seeding stage of this worker ran on its device
    size_t                      nDeclined = 0, nPassesOnHost = 0; // reads the GPU seeding stage left to the host; passes whose match buffer was full
    uint64_t                    nTaxonDropped = 0; // --taxon-list / --taxon-exclude: promising seeds on subjects the mask drops
    double                      msTaxon = 0;       // ... the mask and the filter: the kernels' time on the GPU, the wall clock on the host
    bool                        taxonOnGpu = false; // ... a pass of this worker filtered its list on the device
    // --query-masking seg | dust: the masks this worker made (one per job: its query set, or each of its blocks)
    uint64_t                    nMaskLetters = 0, nMasked = 0, nMaskSeqs = 0;
    double                      msMask = 0;        // ... the calls' wall clock (on the GPU: upload included)
    bool                        maskOnGpu = false;
    std::string                 error;
};

// what a worker searches in one go: a range of the reads of a sequence set, its records into `bms` / `ops` (the eager path: one
// range of all reads per worker; --lazy-query: one block after the other, all of its reads)
struct Job
{
    SeqSet const *                q   = nullptr;
    std::vector<uint8_t> const *  red = nullptr;
    uint64_t                      rLo = 0, rHi = 0;
    std::vector<lx_blast_match> * bms = nullptr;
    std::vector<uint8_t> *        ops = nullptr;
};

// ---- one worker: a handle of its own on its device (worker 0: the handle the table is resident on) with the scoring, the subjects
// and the table set up once; then job after job, each one pass of the batch loop of realMain (src/search.cpp:426-459) or two
class Worker
{
public:
    Worker(size_t w, SearchContext const & c, Part & part) :
        w_(w), c_(c), pt_(part), borrow_(w == 0 && c.table.firstHandle), eng_(borrow_ ? c.table.firstHandle.get() : nullptr, c.setup.devices[w % c.setup.devices.size()])
    {
        Options const & opt = c.opt;
        SeqSet const &  db  = c.db;
        eng_.setScoring(c.setup.sc, 0);
        if (c.run.bs)
            eng_.setScoring(c.setup.scRev, 1);
        // the database stays on the GPU for the whole run (the reference keeps it in the index file it maps at start-up)
        eng_.check(lx_set_subjects(eng_.raw(), db.res.data(), db.res.size()));
        // the table on this worker's handle: worker 0 borrows the resident one, the others attach the table to their own
        if (opt.seeding == "gpu")
        {
            if (borrow_)
                gpuIndex_ = c.table.ix.get();
            else
            {
                lx_index * att = nullptr;
                if (lx_index_attach(c.table.ix.get(), eng_.raw(), &att) == LX_OK)
                    attached_.reset(att), gpuIndex_ = att;
                else // (the table and the sequences did not fit beside the extension's buffers: host threads)
                    std::cerr << "WARNING: seeding on the host threads (" << lx_last_error(eng_.raw()) << ")\n";
            }
        }
        pt_.gpuSeeding = gpuIndex_ != nullptr;
        // with the seeding on the device its matches stay there: the sequence sets become resident for the Level-2 kernels
        // (LAMBDA3_HOST_LIST=1: the matches come down and go through lx_iterate_matches, the A/B switch of the tests)
        // (--taxon-filter host: the list is filtered in host memory, so the passes take it from there)
        deviceList_ = gpuIndex_ && !std::getenv("LAMBDA3_HOST_LIST") && !(c.taxon.on && opt.taxonFilter == "host");
        if (deviceList_)
            eng_.check(lx_set_subject_seqs(eng_.raw(), db.off.data(), db.len.data(), db.off.size()));
        // search() (src/search_algo.hpp:611-762) over the sorted table of reduced words: what both passes share
        spar_.half_exact = opt.halfExact ? 1 : 0, spar_.adaptive = opt.adaptive ? 1 : 0, spar_.pre_scoring = opt.preScoring;
        spar_.pre_scoring_thresh = opt.preScoringThresh, spar_.max_matches = opt.maxMatches, spar_.q_num_frames = c.run.qFrames;
        spar_.unknown_rank = c.run.prot ? 25 : c.run.bs ? 4 : 3; // 'X' / 'N'
        spar_.matrix = c.setup.sc.matrix, spar_.matrix_rev = c.run.bs ? c.setup.scRev.matrix : nullptr, spar_.host_threads = c.setup.seedThreads;
        if (c.taxon.on)
            makeTaxonMasks();
    }

    void search(Job const & job)
    {
        uint64_t const qFrames = (uint64_t)c_.run.qFrames;
        beginJob(job);
        if (c_.opt.queryMasking != "none")
            makeQueryMask(job);
        std::vector<uint64_t> all;
        for (uint64_t i = job.rLo * qFrames; i < job.rHi * qFrames; ++i)
            all.push_back(i);
        if (!c_.opt.search0)
        {
            pass(job, c_.setup.so1, all);
            return;
        }
        // iterativeSearch (:1391-1457): the exact pre-search first, the default parameters for reads without a result
        pass(job, c_.setup.so0, all);
        std::vector<uint8_t> successful(job.q->ids.size(), 0);
        for (auto const & bm : *job.bms)
            successful[bm.n_qid] = 1;
        std::vector<uint64_t> rest;
        for (uint64_t i : all)
            if (!successful[i / qFrames])
                rest.push_back(i);
        if (!rest.empty())
            pass(job, c_.setup.so1, rest);
        // (the reference writes phase 1's records of a batch before phase 2's; here both lists are written together:
        // order by read, as one batch holding every read would give)
        std::stable_sort(job.bms->begin(), job.bms->end(), [](lx_blast_match const & a, lx_blast_match const & b) { return a.n_qid < b.n_qid; });
    }

    lx_handle * handle() { return eng_.raw(); }

private:
    // the job's queries for the Level-2 kernels, and room for its one call per seeding pass
    void beginJob(Job const & job)
    {
        if (!deviceList_)
            return;
        SeqSet const & qs      = *job.q;
        uint64_t const qFrames = (uint64_t)c_.run.qFrames;
        eng_.check(lx_set_queries(eng_.raw(), qs.res.data(), qs.res.size(), qs.off.data(), qs.len.data(), qs.off.size(), qs.orig_len.data(), c_.run.qFrames));
        // this worker makes ONE Level-2 call per seeding pass: what that call would allocate and touch inside itself is asked
        // for here, before the seeding (a dozen promising seeds per read, a window per seven of them, a record per twelve --
        // what the read sets of tools/cli_scale_nucl.py come to; a short estimate only moves an allocation back into the call)
        uint64_t const est = std::min<uint64_t>(12 * (job.rHi - job.rLo), 0x7ffffff0ull);
        uint64_t       len = 0;
        for (uint64_t i = job.rLo * qFrames; i < job.rHi * qFrames && i < qs.len.size(); ++i)
            len = std::max<uint64_t>(len, qs.len[i]);
        if (est >= 100000)
            eng_.check(lx_reserve(eng_.raw(), est, est / 7, est / 12, c_.run.wantOps ? est / 12 * (len + len / 16) : 0));
    }

    // --query-masking seg | dust, once per job (the eager path: the worker's query set; --lazy-query: each block), after frame expansion; both
    // passes seed with it.  The mask is made where --masking says (auto: where the seeding runs).  Seeding on the device needs the mask
    // on this handle: one made on the host goes up as bytes; the host seeder reads a device mask's copy, which comes down on first use.
    void makeQueryMask(Job const & job)
    {
        SeqSet const &       qs   = *job.q;
        bool const           dust = c_.opt.queryMasking == "dust"; // (on qs.res, the read's own letters: searchbs reduces them per frame)
        std::string const    what = "--query-masking " + c_.opt.queryMasking + ": ";
        lx_seg_params const  sp{c_.opt.segWindow, c_.opt.segK1, c_.opt.segK2};
        lx_dust_params const dp{c_.opt.dustWindow, c_.opt.dustLevel};
        bool const           onGpu = c_.opt.masking == "gpu" || (c_.opt.masking == "auto" && gpuIndex_);
        auto const          tMask = Clock::now();
        seedMask_.reset();
        madeMask_.reset();
        lx_query_mask * m = nullptr;
        lx_handle * const at = onGpu ? eng_.raw() : nullptr;
        // (the rule reads A, C, G, T = 0 .. 3 and takes every other rank as a break: searchbs' ranks; searchn's are A, C, G, N, T, so its
        // letters go in with 3 and 4 exchanged)
        std::vector<uint8_t> swapped;
        if (dust && c_.opt.cmd == "searchn")
        {
            swapped.resize(qs.res.size());
            for (size_t j = 0; j < swapped.size(); ++j)
                swapped[j] = qs.res[j] == 3 ? 4 : qs.res[j] == 4 ? 3 : qs.res[j];
        }
        if ((dust ? lx_query_mask_create_dust(at, swapped.empty() ? qs.res.data() : swapped.data(), qs.off.data(), qs.len.data(), qs.off.size(), &dp, c_.setup.seedThreads, &m)
                  : lx_query_mask_create_seg(at, qs.res.data(), qs.off.data(), qs.len.data(), qs.off.size(), &sp, c_.setup.seedThreads, &m)) != LX_OK)
            throw std::runtime_error(what + lx_last_output_error());
        madeMask_.reset(m);
        if (!onGpu && gpuIndex_)
        {
            std::vector<uint8_t> bytes(qs.res.size() + 1, 0);
            lx_query_mask *      up = nullptr;
            if (lx_query_mask_copy(m, bytes.data()) != LX_OK ||
                lx_query_mask_create(eng_.raw(), bytes.data(), qs.off.data(), qs.len.data(), qs.off.size(), &up) != LX_OK)
                throw std::runtime_error(what + lx_last_output_error());
            seedMask_.reset(up);
        }
        uint64_t letters = 0, masked = 0, seqs = 0;
        (void)lx_query_mask_info(m, &letters, &masked, &seqs);
        pt_.nMaskLetters += letters, pt_.nMasked += masked, pt_.nMaskSeqs += seqs;
        pt_.msMask += msSince(tMask);
        pt_.maskOnGpu = pt_.maskOnGpu || onGpu;
    }
    lx_query_mask const * queryMask() const { return seedMask_ ? seedMask_.get() : madeMask_.get(); }

    // --taxon-list / --taxon-exclude, once per handle: the mask in host memory for the lists that stand there, and -- where the
    // matches stay on the device and --taxon-filter does not say host -- the tree resident on this handle and the mask by kernels
    void makeTaxonMasks()
    {
        TaxonSetup const & tx = c_.taxon;
        // The seeding thins a read's seeds towards -n matches (adaptive elongation, the over-abundance cut: src/search_algo.hpp:679-729)
        // and does not know the mask: matches on subjects the filter drops would use that budget up, and an elongated seed would lose
        // the kept subject that differs a little for the dropped ones that do not.  Every dropped subject can take one of the places,
        // so the seeding aims at -n plus the number of dropped subjects -- but at no more than the 64 matches per read a device launch
        // has room for (lx_seed_queries), unless -n itself is larger: from -n 64 on the seeding is the unrestricted run's.
        constexpr uint64_t kLaunchRoomPerRead = 64;
        if (c_.opt.maxMatches > 0)
            spar_.max_matches = std::min<uint64_t>(c_.opt.maxMatches + (tx.nSubjects - tx.nKept), std::max<uint64_t>(c_.opt.maxMatches, kLaunchRoomPerRead));
        lx_subject_mask * m = nullptr;
        if (lx_subject_mask_create(nullptr, tx.words.data(), tx.nSubjects, &m) != LX_OK)
            throw std::runtime_error(std::string("the taxon filter: ") + lx_last_output_error());
        hostMask_.reset(m);
        if (!deviceList_)
        {
            if (c_.opt.taxonFilter == "gpu")
                std::cerr << "WARNING: --taxon-filter gpu: this worker's match lists stand in host memory and are filtered there\n";
            return;
        }
        lx_tax_dev * t = nullptr;
        eng_.check(lx_tax_dev_create(eng_.raw(), &tx.tree, &t));
        taxDev_.reset(t);
        eng_.check(lx_subject_mask_create_dev(eng_.raw(), t, &tx.filter, &m));
        devMask_.reset(m);
        float ms = 0;
        if (lx_last_phase_ms(eng_.raw(), 14, &ms, nullptr) == LX_OK)
            pt_.msTaxon += ms;
        uint64_t kept = 0;
        if (lx_subject_mask_info(m, nullptr, &kept) != LX_OK || kept != tx.nKept)
            throw std::runtime_error("the taxon filter: the mask made on the GPU keeps another number of subjects than the host rule");
    }

    // drops the matches on subjects the mask does not keep from the pass's list, where the list stands; the number that stay.  A
    // device list is compacted on the device; a host-path result by the library on its host list; a device result whose matches
    // this worker takes from host memory (--taxon-filter host, LAMBDA3_HOST_LIST) in its host copy, here.
    uint64_t filterByTaxon(lx_seed_result * sr)
    {
        bool const resultOnDevice = lx_seed_result_matches_dev(sr) != nullptr;
        uint64_t   before = 0, kept = 0;
        if (resultOnDevice && deviceList_)
        {
            eng_.check(lx_seed_result_filter(sr, devMask_.get(), c_.run.sFrames, &before, &kept));
            float ms = 0;
            if (lx_last_phase_ms(eng_.raw(), 14, &ms, nullptr) == LX_OK)
                pt_.msTaxon += ms;
            pt_.taxonOnGpu = true;
            pt_.nTaxonDropped += before - kept;
            return kept;
        }
        auto const tFilter = Clock::now();
        if (!resultOnDevice)
        {
            if (lx_seed_result_filter(sr, hostMask_.get(), c_.run.sFrames, &before, &kept) != LX_OK)
                throw std::runtime_error(std::string("the taxon filter: ") + lx_last_output_error());
        }
        else
        {
            before                = lx_seed_result_stats(sr).n_matches;
            lx_match * const list = before ? lx_seed_result_matches(sr) : nullptr;
            if (before && !list)
                throw std::runtime_error("the match list did not fit into host memory");
            uint64_t const frames = (uint64_t)c_.run.sFrames;
            for (uint64_t k = 0; k < before; ++k)
            {
                uint64_t const s = list[k].subjId / frames;
                if (s >= c_.taxon.nSubjects)
                    throw std::runtime_error("the taxon filter: a match names a subject the index's taxonomy does not have");
                if ((c_.taxon.words[s >> 6] >> (s & 63)) & 1)
                    list[kept++] = list[k];
            }
        }
        pt_.msTaxon += msSince(tFilter);
        pt_.nTaxonDropped += before - kept;
        return kept;
    }

    // one pass: seed the frame sequences `which` of the job, extend (GPU), collect the records
    void pass(Job const & job, lambda_amd::SeedParams const & so, std::vector<uint64_t> const & which)
    {
        Options const &               opt    = c_.opt;
        SeqSet const &                db     = c_.db;
        SeqSet const &                qs     = *job.q;
        std::vector<uint8_t> const &  qRed   = *job.red;
        std::vector<lx_blast_match> & outBms = *job.bms;
        std::vector<uint8_t> &        outOps = *job.ops;
        bool const                    wantOps = c_.run.wantOps, recordsOnGpu = c_.run.recordsOnGpu;
        if (std::getenv("LAMBDA3_TRACE"))
            std::fprintf(stderr, "[worker %zu] seeding %zu frame sequences (seed %d/%d, delta %d)\n", w_, which.size(), so.seedLength, so.seedOffset, so.maxSeedDist);
        auto const            tSeed = Clock::now();
        std::vector<uint64_t> reads; // (lx_seed_queries takes a read by its first frame sequence)
        for (uint64_t i : which)
            if (i % (uint64_t)c_.run.qFrames == 0)
                reads.push_back(i);
        spar_.seed_length = so.seedLength, spar_.seed_offset = so.seedOffset, spar_.max_seed_dist = so.maxSeedDist;
        lx_seed_result * sr = nullptr;
        // the device takes the reads; those it declines (words far beyond the table's keys with many occurrences) and those of
        // a launch whose match buffer filled up are finished on the host threads inside the call
        // (--query-masking seg | dust: with the job's mask; without one the call is lx_seed_queries)
        if (gpuIndex_ && lx_seed_queries_masked(eng_.raw(), gpuIndex_, nullptr, qs.res.data(), qRed.data(), qs.off.data(), qs.len.data(), qs.off.size(), reads.data(),
                                                reads.size(), queryMask(), &spar_, &sr) != LX_OK)
        {
            // a HIP error in the seeding stage (its match buffer did not fit, ...): this pass and the following ones are
            // seeded on the host threads, from a clean slate
            std::cerr << "WARNING: seeding on the host threads from here on (" << lx_last_error(eng_.raw()) << ")\n";
            gpuIndex_      = nullptr;
            pt_.gpuSeeding = false;
        }
        if (!sr && lx_seed_queries_masked(nullptr, c_.table.ix.get(), db.res.data(), qs.res.data(), qRed.data(), qs.off.data(), qs.len.data(), qs.off.size(),
                                          reads.data(), reads.size(), madeMask_.get(), &spar_, &sr) != LX_OK)
            throw std::runtime_error(std::string("lambda_ext: ") + lx_last_output_error());
        std::unique_ptr<lx_seed_result, FreeWith<lx_seed_result_free>> const keepSeeds(sr);
        lx_seed_stats const sst = lx_seed_result_stats(sr);
        pt_.sst.hitsAfterSeeding += sst.hits_after_seeding, pt_.sst.hitsFailedPreExtendTest += sst.hits_failed_pre_extend;
        pt_.nDeclined += sst.reads_declined, pt_.nPassesOnHost += sst.launches_full;
        // the matches where the seeding left them: the device list for the Level-2 kernels, else the list in host memory
        // (--taxon-list / --taxon-exclude: without the matches on subjects the mask drops; "promising" counts them all the same)
        uint64_t const     nMatches = c_.taxon.on && sst.n_matches ? filterByTaxon(sr) : sst.n_matches;
        void const * const dList    = deviceList_ ? lx_seed_result_matches_dev(sr) : nullptr;
        lx_match * const   hList    = dList || nMatches == 0 ? nullptr : lx_seed_result_matches(sr);
        if (!dList && nMatches && !hList)
            throw std::runtime_error("the match list did not fit into host memory");
        pt_.msSeed += msSince(tSeed);
        pt_.nPromising += sst.n_matches;
        if (std::getenv("LAMBDA3_TRACE"))
            std::fprintf(stderr, "[worker %zu] %zu promising seeds -> extension\n", w_, (size_t)nMatches);
        if (nMatches == 0)
            return;
        lx_iterate_result * res  = nullptr;
        auto const          tExt = Clock::now();
        lx_record_stats     passRst{};
        lx_cull_stats       passCst{};
        bool                cutDone = false;
        if (dList && recordsOnGpu) // ... with _writeRecord's cut before the records come down
        {
            if (opt.maxHsps || opt.cullingLimit) // (the lengths: the resident q_orig_len of beginJob's lx_set_queries)
            {
                lx_cull_options const co = cullOptions(opt, c_.run, qs);
                eng_.check(lx_iterate_matches_dev_top_ex(eng_.raw(), 0, dList, nMatches, &c_.setup.sp, opt.maxMatches, &co, &passRst, &passCst, &res));
            }
            else
                eng_.check(lx_iterate_matches_dev_top(eng_.raw(), 0, dList, nMatches, &c_.setup.sp, opt.maxMatches, &passRst, &res));
            float msTop = 0;
            if (lx_last_phase_ms(eng_.raw(), 7, &msTop, nullptr) == LX_OK)
                pt_.msRecords += msTop;
            cutDone = true;
        }
        else if (dList) // the Level-2 driver on the list where the seeding kernel left it (include/lambda_ext.h)
            eng_.check(lx_iterate_matches_dev(eng_.raw(), 0, dList, nMatches, &c_.setup.sp, &res));
        else
            eng_.check(lx_iterate_matches(eng_.raw(), 0, qs.res.data(), qs.res.size(), qs.off.data(), qs.len.data(), qs.off.size(),
                                          qs.orig_len.data(), nullptr, 0, db.off.data(), db.len.data(), db.off.size(), hList, nMatches, &c_.setup.sp, &res));
        std::unique_ptr<lx_iterate_result, FreeWith<lx_iterate_result_free>> const keepRes(res);
        pt_.msExtend += msSince(tExt);
        uint64_t                    n  = lx_iterate_result_count(res);
        lx_blast_match const *      bm = lx_iterate_result_matches(res);
        std::vector<lx_blast_match> cutRows;
        if (recordsOnGpu && !cutDone) // (a list in host memory: the host step, on this pass's records -- all a query has)
        {
            auto const tRec = Clock::now();
            cutRows.assign(bm, bm + n);
            n  = hostRecordsStep(opt, c_.run, qs, cutRows.data(), n, &passRst, &passCst);
            bm = cutRows.data();
            pt_.msRecords += msSince(tRec);
        }
        pt_.rst += passRst;
        pt_.cst += passCst;
        uint64_t const ob     = outOps.size();
        uint64_t       opsEnd = 0; // (the records are ordered by query, their ops as the passes produced them: bisulfite runs two)
        for (uint64_t k = 0; k < n && wantOps; ++k)
            opsEnd = std::max<uint64_t>(opsEnd, bm[k].ops_off + bm[k].n_ops);
        if (opsEnd)
            outOps.insert(outOps.end(), lx_iterate_result_ops(res), lx_iterate_result_ops(res) + opsEnd);
        for (uint64_t k = 0; k < n; ++k)
        {
            outBms.push_back(bm[k]);
            outBms.back().ops_off += ob;
        }
        pt_.ist += lx_iterate_result_stats(res);
    }

    size_t                w_;
    SearchContext const & c_;
    Part &                pt_;
    bool                  borrow_;
    lambda_amd::Engine    eng_;
    IndexOwner            attached_;
    lx_index const *      gpuIndex_   = nullptr; // the table on this worker's handle (NULL: the seeding is the host threads')
    bool                  deviceList_ = false;
    lx_seed_params        spar_{};
    // --taxon-list / --taxon-exclude (behind eng_: destroyed before the handle)
    std::unique_ptr<lx_tax_dev, FreeWith<lx_tax_dev_destroy>>           taxDev_;
    std::unique_ptr<lx_subject_mask, FreeWith<lx_subject_mask_destroy>> devMask_, hostMask_;
    // --query-masking seg | dust: the job's mask as it was made, and -- made on the host while the seeding runs on the device -- its upload
    std::unique_ptr<lx_query_mask, FreeWith<lx_query_mask_destroy>> madeMask_, seedMask_;
};

// worker w's thread: its set-up, then the jobs nextJob hands it (false: no more), each reported to jobDone with the worker's handle
// (for what follows a search on the same device); an error ends it and stays in its part.  `leave` runs before the handle goes.
template <class Next, class Done, class Leave>
void runWorker(size_t w, SearchContext const & c, Part & part, Next && nextJob, Done && jobDone, Leave && leave)
{
    try
    {
        Worker worker(w, c, part);
        struct AtExit
        {
            Leave & f;
            ~AtExit() { f(); }
        } const atExit{leave};
        for (Job job; nextJob(job);)
        {
            worker.search(job);
            jobDone(job, worker.handle());
        }
    }
    catch (std::exception const & e)
    {
        part.error = e.what();
    }
}

// ---- the eager search: contiguous ranges of reads, as `omp for schedule(dynamic)` over whole batches would hand a thread (:384-385);
// a worker's error is the run's, before anything is written
void runEager(SearchContext const & c, SeqSet const & qs, std::vector<uint8_t> const & qRed, std::vector<Part> & parts)
{
    size_t const   nWorkers = parts.size();
    uint64_t const nReads   = qs.ids.size();
    auto           run      = [&](size_t w)
    {
        bool given = false;
        runWorker(
            w, c, parts[w],
            [&](Job & job)
            {
                if (given)
                    return false;
                given = true;
                job   = Job{&qs, &qRed, nReads * w / nWorkers, nReads * (w + 1) / nWorkers, &parts[w].bms, &parts[w].ops};
                return job.rLo != job.rHi;
            },
            [](Job &, lx_handle *) {}, [] {});
    };
    {
        std::vector<std::thread> pool;
        JoinOnExit const         join(pool);
        for (size_t w = 1; w < nWorkers; ++w)
            pool.emplace_back(run, w);
        run(0);
    }
    for (Part const & pt : parts)
        if (!pt.error.empty())
            throw std::runtime_error(pt.error);
}

// ---- what the writers are told, on both paths (the LCA pairs are added per list)
struct OutputSetup
{
    lx_tax_tree               tree{};
    std::vector<char const *> taxNames;
    bool                      lca = false; // the LCA per query is asked for and the index has the tree for it
    bool                      lcaOnGpu = false; // --lca gpu | auto
    lx_lca_options            lcaOptions;       // --lca-top-percent
    lx_output_options         options;

    OutputSetup(Options const & opt, Run const & run, IndexTaxonomy const & tax)
    {
        lca      = tax.has && run.wantLca && tax.hasTree;
        lcaOnGpu = opt.lca != "host"; // (auto = gpu: DESIGN.md 4.12.1, profiles/lca_bench.txt)
        lx_lca_options_default(&lcaOptions);
        lcaOptions.top_percent = opt.lcaTopPercent;
        if (tax.has)
        {
            tree.parents   = tax.parents.data();
            tree.heights   = tax.heights.data();
            tree.n_taxa    = tax.parents.size();
            tree.s_tax_off = tax.off.data();
            tree.s_tax_ids = tax.ids.data();
            tree.n_s       = tax.off.size() - 1;
            if (lca)
                taxNames = cstrs(tax.names);
        }
        lx_output_options & oo = options;
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
        oo.genetic_code        = run.geneticCodeQry;
        if (tax.has)
        {
            oo.tax = &tree;
            if (lca)
                oo.tax_names = taxNames.data();
        }
    }
    OutputSetup(OutputSetup const &) = delete; // (`options` points into it)
};

using TaxDevOwner = std::unique_ptr<lx_tax_dev, FreeWith<lx_tax_dev_destroy>>;

// the index's tree resident on h's device (--lca gpu); destroyed before h
TaxDevOwner makeTaxDev(lx_handle * h, OutputSetup const & out)
{
    lx_tax_dev * t = nullptr;
    if (lx_tax_dev_create(h, &out.tree, &t) != LX_OK)
        throw std::runtime_error(std::string("the taxonomic tree on the GPU: ") + lx_last_error(h));
    return TaxDevOwner(t);
}

// the LCA per query (the reference's _writeRecord, src/search_algo.hpp:884-908) over the n records of a list, of the records
// --lca-top-percent keeps: on the host, or (--lca gpu: h and its resident tree) as kernels
void computeLca(OutputSetup const & out, lx_handle * h, lx_tax_dev const * dev, lx_blast_match const * bms, uint64_t n, std::vector<uint64_t> & lcaQid,
                std::vector<uint32_t> & lcaTax, uint64_t & nLca)
{
    lcaQid.resize(std::max<uint64_t>(n, 1));
    lcaTax.resize(std::max<uint64_t>(n, 1));
    if (dev)
    {
        if (lx_compute_lca_dev(h, dev, bms, n, &out.lcaOptions, lcaQid.data(), lcaTax.data(), &nLca) != LX_OK)
            throw std::runtime_error(lx_last_error(h)); // ("LCA-computation error: ..." where the fold failed)
    }
    else if (lx_compute_lca_ex(bms, n, &out.tree, &out.lcaOptions, lcaQid.data(), lcaTax.data(), &nLca) != LX_OK)
        throw std::runtime_error("LCA-computation error: One of the paths didn't lead to root.");
}

// where the records of the output were made, and what that took
struct RenderTimes
{
    double msCompress  = 0; // (.bam, *.gz: BGZF on the first handle's device)
    double msRenderDev = 0; // (--render gpu: the render kernels' device time)
    double msLca       = 0; // (the eager path: the LCA over all records, the resident tree's upload included)
    bool   onGpu       = false;
};

// ---- --lazy-query: the block pipeline (the reference's batch loop, src/search.cpp:389-459, with its reader thread behind a bounded
// queue, src/search_algo.hpp:374-413): one reader makes blocks of at most blockReads reads (stream -> parser -> SeqSet: ranks,
// frames, reduction), one worker per entry of --devices takes the next block and searches all of it as the eager path searches a
// worker's range (then _writeRecord's cut and the LCA, both per query and so per block), and the main thread appends the finished
// blocks in their order through lx_out.  At most nWorkers + 2 blocks exist at any time: the reader waits for a free place before it
// begins one.  An error in block k (a malformed record, a failed call) ends the run with its message; the blocks in front of k are
// written and the file is closed behind them.
struct Block
{
    uint64_t                    index = 0;
    SeqSet                      qs;
    std::vector<uint8_t>        red;
    std::vector<lx_blast_match> bms;
    std::vector<uint8_t>        ops;
    uint64_t                    found = 0, kept = 0; // records before and after _writeRecord's cut
    lx_record_stats             rst{};               // (--records host: this block's step)
    lx_cull_stats               cst{};
    std::vector<uint64_t>       lcaQid;
    std::vector<uint32_t>       lcaTax;
    uint64_t                    nLca = 0;
};

// the blocks between the three kinds of thread: the places, the queue to the workers, the finished blocks by index, the run's error
class BlockPipeline
{
public:
    struct Counts
    {
        uint64_t blocks = 0, largest = 0, maxAlive = 0, reads = 0;
    };

    explicit BlockPipeline(uint64_t cap) : cap_(cap) {}

    // the reader: a place for one more block, waited for (false: the search has stopped)
    bool acquirePlace()
    {
        std::unique_lock<std::mutex> lock(mu_);
        cv_.wait(lock, [&] { return alive_ < cap_ || stop_; });
        if (stop_)
            return false;
        ++alive_;
        counts_.maxAlive = std::max(counts_.maxAlive, alive_);
        return true;
    }
    // the reader: the block, which has a place, takes the next index and goes to the workers
    void publish(std::unique_ptr<Block> b)
    {
        std::lock_guard<std::mutex> lock(mu_);
        b->index        = made_++;
        counts_.blocks  = made_;
        counts_.largest = std::max<uint64_t>(counts_.largest, b->qs.ids.size());
        counts_.reads += b->qs.ids.size();
        toSearch_.push_back(std::move(b));
        cv_.notify_all();
    }
    // a place is free again: its block is written (the writer), or it never came to hold one (the reader)
    void release()
    {
        std::lock_guard<std::mutex> lock(mu_);
        --alive_;
        cv_.notify_all();
    }
    // the reader is through (holding: with a place it took for a block it did not publish)
    void readerFinished(bool holding)
    {
        std::lock_guard<std::mutex> lock(mu_);
        if (holding)
            --alive_;
        readerDone_ = true;
        cv_.notify_all();
    }
    // a worker: the next block to search, waited for (none: no more will come, or the search has stopped)
    std::unique_ptr<Block> takeNext()
    {
        std::unique_lock<std::mutex> lock(mu_);
        cv_.wait(lock, [&] { return !toSearch_.empty() || readerDone_ || stop_; });
        if (stop_ || toSearch_.empty())
            return nullptr;
        std::unique_ptr<Block> b = std::move(toSearch_.front());
        toSearch_.pop_front();
        return b;
    }
    // a worker: the block is searched
    void finish(std::unique_ptr<Block> b)
    {
        std::lock_guard<std::mutex> lock(mu_);
        uint64_t const              at = b->index;
        done_[at]                      = std::move(b);
        cv_.notify_all();
    }
    // the writer: block `next`, waited for (none: every block is written, or the one that comes next never will be)
    std::unique_ptr<Block> takeDone(uint64_t next)
    {
        std::unique_lock<std::mutex> lock(mu_);
        cv_.wait(lock, [&] { return done_.count(next) || stop_ || (readerDone_ && next == made_); });
        auto it = done_.find(next);
        if (it == done_.end())
            return nullptr;
        std::unique_ptr<Block> b = std::move(it->second);
        done_.erase(it);
        return b;
    }
    // the run's error (the first one counts); hard: nothing more is searched (a block failed), else the blocks made so far go through
    // (the reader failed)
    void fail(std::string const & why, bool hard)
    {
        std::lock_guard<std::mutex> lock(mu_);
        if (error_.empty())
            error_ = why;
        stop_ = stop_ || hard;
        cv_.notify_all();
    }
    // the writer leaves: whoever still waits or works stops (nothing is stopped where every block went through)
    void halt()
    {
        std::lock_guard<std::mutex> lock(mu_);
        if (!readerDone_ || !toSearch_.empty())
            stop_ = true;
        cv_.notify_all();
    }
    std::string error()
    {
        std::lock_guard<std::mutex> lock(mu_);
        return error_;
    }
    Counts counts()
    {
        std::lock_guard<std::mutex> lock(mu_);
        return counts_;
    }

private:
    std::mutex                                 mu_;
    std::condition_variable                    cv_;
    std::deque<std::unique_ptr<Block>>         toSearch_;
    std::map<uint64_t, std::unique_ptr<Block>> done_;
    uint64_t                                   alive_ = 0, made_ = 0;
    uint64_t const                             cap_;
    bool                                       readerDone_ = false, stop_ = false;
    std::string                                error_;
    Counts                                     counts_;
};

// the reader's thread: a place, then a block of the stream's next records; its error lets the blocks made so far go through
void readBlocks(Run const & run, bool keepQual, QueryStream & stream, BlockPipeline & pipe)
{
    bool holding = false; // a place taken for a block that is not in the queue yet
    bool noted   = false; // kNoQualNote has been printed
    try
    {
        lx_query_blocks::BlockCutter cut(run.blockReads);
        for (bool more = true; more && pipe.acquirePlace();)
        {
            holding = true;
            std::unique_ptr<Block> b(new Block);
            more = stream.records(
                [&](std::string const & id, std::string & letters)
                {
                    uint64_t const n = letters.size();
                    addRecord(b->qs, id, letters, run.prot, !run.prot, run.blastx, run.geneticCodeQry, run.bs ? 2 : 0, keepQual ? &stream.quality() : nullptr);
                    return !cut.add(n);
                });
            if (b->qs.ids.empty()) // (the file ended where the last block closed)
                break;
            if (keepQual && !noted && !b->qs.ascii.empty() && !qualOf(b->qs))
            {
                std::cerr << kNoQualNote;
                noted = true;
            }
            b->red = reduce(b->qs, run.red);
            pipe.publish(std::move(b));
            holding = false;
        }
    }
    catch (std::exception const & e)
    {
        pipe.fail(e.what(), false);
    }
    pipe.readerFinished(holding);
}

// a worker's thread: block after block; what follows the search of a block is per query and so per block.  Its error stops the search.
void searchBlocks(size_t w, SearchContext const & c, OutputSetup const & out, BlockPipeline & pipe, Part & part)
{
    std::unique_ptr<Block> current; // the block this worker searches
    TaxDevOwner            taxDev;  // --lca gpu: the tree on this worker's handle, made at its first block
    runWorker(
        w, c, part,
        [&](Job & job)
        {
            current = pipe.takeNext();
            if (!current)
                return false;
            job = Job{&current->qs, &current->red, 0, current->qs.ids.size(), &current->bms, &current->ops};
            return true;
        },
        [&](Job &, lx_handle * h)
        {
            std::unique_ptr<Block> b = std::move(current);
            b->found = b->kept = b->bms.size();
            if (!c.run.recordsOnGpu) // _writeRecord's cut: every record of a read is in its block
            {
                auto const tRec = Clock::now();
                b->kept         = hostRecordsStep(c.opt, c.run, b->qs, b->bms.data(), b->bms.size(), &b->rst, &b->cst);
                part.msRecords += msSince(tRec);
            }
            if (out.lca)
            {
                auto const tLca = Clock::now();
                if (out.lcaOnGpu && !taxDev)
                    taxDev = makeTaxDev(h, out);
                computeLca(out, h, taxDev.get(), b->bms.data(), b->kept, b->lcaQid, b->lcaTax, b->nLca);
                part.msLca += msSince(tLca);
            }
            pipe.finish(std::move(b));
        },
        [&] { taxDev.reset(); });
    if (!part.error.empty())
        pipe.fail(part.error, true);
}

// what the blocks came to
struct LazyTotals
{
    BlockPipeline::Counts counts;
    uint64_t              hsps = 0, written = 0;
    lx_record_stats       rst{};
    lx_cull_stats         cst{};
    RenderTimes           times;
};

// the whole lazy run: reader and workers started, the finished blocks appended by this thread in their order, everything joined on
// every way out (an error first tells the others to stop) and the file closed behind the blocks it holds
LazyTotals runLazy(SearchContext const & c, QueryStream & stream, OutputSetup const & output, std::vector<Part> & parts)
{
    Options const & opt = c.opt;
    Run const &     run = c.run;
    LazyTotals      totals;
    BlockPipeline   pipe(parts.size() + 2);
    std::thread              reader;
    std::vector<std::thread> pool;
    JoinOnExit const         joinPool(pool), joinReader(reader);
    struct HaltOnExit
    {
        BlockPipeline & p;
        ~HaltOnExit() { p.halt(); }
    } const haltOnExit{pipe};
    reader = std::thread(readBlocks, std::cref(run), opt.samQual, std::ref(stream), std::ref(pipe));
    for (size_t w = 0; w < parts.size(); ++w)
        pool.emplace_back(searchBlocks, w, std::cref(c), std::cref(output), std::ref(pipe), std::ref(parts[w]));

    // ---- the writer: this thread
    bool const        dev = opt.render == "gpu";
    int const         fmt = run.outFmt;
    HandleOwner const keepH = (dev || run.outGz || fmt == LX_OUT_BAM) ? makeHandle(c.setup.devices[0]) : HandleOwner();
    lx_handle * const zh    = keepH.get();
    std::vector<char const *> const sidL = cstrs(c.db.ids);
    lx_seq_names const              subjects{nullptr, nullptr, sidL.data(), c.db.orig_len.data(), 0, sidL.size()};
    struct CloseOut // (an error on the way: the file is closed behind the blocks it holds)
    {
        void operator()(lx_out * o) const { (void)lx_out_close(o, -1); }
    };
    std::unique_ptr<lx_out, CloseOut> out;
    totals.times.onGpu = dev;
    for (uint64_t next = 0;; ++next)
    {
        std::unique_ptr<Block> b = pipe.takeDone(next);
        if (!b)
            break;
        if (!out)
        {
            lx_out * o = nullptr;
            if (lx_out_open(zh, opt.output.c_str(), fmt, run.outGz ? 1 : 0, run.program, &subjects, &output.options, &o) != LX_OK)
                throw std::runtime_error(outputError(zh, opt.output));
            out.reset(o);
        }
        std::vector<char const *> const qidB = cstrs(b->qs.ids);
        lx_seq_names const              nm{qidB.data(), b->qs.orig_len.data(), nullptr, nullptr, qidB.size(), 0};
        if (lx_out_append_ex(out.get(), dev ? LX_RENDER_DEV : LX_RENDER_HOST, b->bms.data(), b->kept, b->ops.data(), b->ops.size(), &nm,
                             reinterpret_cast<uint8_t const *>(b->qs.ascii.data()), b->qs.ascii_off.data(), opt.samQual ? qualOf(b->qs) : nullptr,
                             b->lcaQid.data(), b->lcaTax.data(), b->nLca) != LX_OK)
            throw std::runtime_error((dev ? "records on the GPU: " : "") + outputError(zh, opt.output));
        float msK = 0;
        if (dev && b->kept && lx_last_phase_ms(zh, fmt == LX_OUT_BAM ? 11 : 12, &msK, nullptr) == LX_OK)
            totals.times.msRenderDev += msK;
        if (!dev && zh && b->kept && lx_last_phase_ms(zh, 4, &msK, nullptr) == LX_OK)
            totals.times.msCompress += msK;
        totals.hsps += b->found;
        totals.written += b->kept;
        totals.rst += b->rst;
        totals.cst += b->cst;
        b.reset();
        pipe.release();
    }
    totals.counts     = pipe.counts();
    std::string error = pipe.error();
    if (error.empty() && totals.counts.reads == 0)
        error = "empty query or database file";
    uint64_t withHit = totals.rst.qrys_with_hit; // (--records gpu: counted in the workers' passes, which are over)
    for (Part const & pt : parts)
        withHit += error.empty() ? pt.rst.qrys_with_hit : 0;
    if (out && lx_out_close(out.release(), (int64_t)withHit) != LX_OK && error.empty())
        error = "cannot write " + opt.output;
    if (!error.empty())
        throw std::runtime_error(error);
    return totals;
}

// ---- the sums over the parts, a part themselves: the records concatenated (the ranges are disjoint and ascending: concatenation in
// range order is the order one thread would have produced), the counts added, of the times the slowest worker's, the seeding on a GPU
// where any worker's was
struct Totals : Part
{
    uint64_t nHsp = 0, nOut = 0; // records before and after _writeRecord's cut
    uint64_t maskSum[3] = {0, 0, 0};

    void add(Part const & pt)
    {
        uint64_t const ob = ops.size();
        ops.insert(ops.end(), pt.ops.begin(), pt.ops.end());
        for (lx_blast_match m : pt.bms)
        {
            m.ops_off += ob;
            bms.push_back(m);
        }
        ist += pt.ist;
        sst.hitsAfterSeeding += pt.sst.hitsAfterSeeding, sst.hitsFailedPreExtendTest += pt.sst.hitsFailedPreExtendTest;
        nPromising += pt.nPromising;
        nDeclined += pt.nDeclined, nPassesOnHost += pt.nPassesOnHost;
        gpuSeeding = gpuSeeding || pt.gpuSeeding;
        msSeed     = std::max(msSeed, pt.msSeed);
        msExtend   = std::max(msExtend, pt.msExtend);
        msRecords  = std::max(msRecords, pt.msRecords);
        msLca      = std::max(msLca, pt.msLca);
        nTaxonDropped += pt.nTaxonDropped;
        msTaxon    = std::max(msTaxon, pt.msTaxon);
        taxonOnGpu = taxonOnGpu || pt.taxonOnGpu;
        // (the eager path: every worker masks the whole query set, so the counts are one worker's; --lazy-query: the blocks' sums)
        maskSum[0] += pt.nMaskLetters, maskSum[1] += pt.nMasked, maskSum[2] += pt.nMaskSeqs;
        nMaskLetters = std::max(nMaskLetters, pt.nMaskLetters), nMasked = std::max(nMasked, pt.nMasked), nMaskSeqs = std::max(nMaskSeqs, pt.nMaskSeqs);
        msMask    = std::max(msMask, pt.msMask);
        maskOnGpu = maskOnGpu || pt.maskOnGpu;
        rst += pt.rst;
        cst += pt.cst;
    }
};

// the parts summed; the eager path's records through _writeRecord's step where no pass has done it (--records gpu: every pass's
// records are cut already), the lazy path's counts from its blocks
Totals sumParts(Options const & opt, Run const & run, SeqSet const & qs, std::vector<Part> const & parts, LazyTotals const & lazy)
{
    Totals t;
    for (Part const & pt : parts)
        t.add(pt);
    t.nHsp = run.recordsOnGpu ? t.rst.hits_final + t.rst.hits_duplicate2 + t.rst.hits_abundant + t.cst.hits_max_hsps + t.cst.hits_culled
             : run.lazy       ? lazy.hsps
                              : t.bms.size();
    t.nOut = run.lazy ? lazy.written : t.bms.size();
    if (run.lazy) // (the blocks' host steps; --records gpu counted in the passes above)
    {
        t.rst += lazy.rst;
        t.cst += lazy.cst;
    }
    else if (!run.recordsOnGpu)
    {
        auto const tRec = Clock::now();
        t.nOut          = hostRecordsStep(opt, run, qs, t.bms.data(), t.bms.size(), &t.rst, &t.cst);
        t.msRecords     = msSince(tRec);
    }
    return t;
}

// ---- the eager writers: all records at once, the file written when everything is made.  What the four of them are handed:
struct EagerRecords
{
    char const *              program;
    lx_blast_match const *    bms;
    uint64_t                  n;
    std::vector<uint8_t> const & ops;
    lx_seq_names const *      names;
    uint8_t const *           ascii;
    uint64_t const *          asciiOff;
    lx_output_options const * oo;
    int64_t                   withHit;
};

// --render gpu, .bam: the records made and compressed on the first device, only the members come down
void writeBamOnGpu(std::string const & path, lx_handle * zh, EagerRecords const & r)
{
    if (lx_write_bam_dev(zh, path.c_str(), r.program, r.bms, r.n, r.ops.data(), r.ops.size(), r.names, r.ascii, r.asciiOff, r.oo) != LX_OK)
        throw std::runtime_error(std::string("BAM records on the GPU: ") + lx_last_error(zh));
}

// --render gpu, a text format: the records made on the first device; *.gz compressed there, too
void writeTextOnGpu(std::string const & path, lx_handle * zh, int fmt, bool gz, EagerRecords const & r)
{
    if (lx_write_text_dev(zh, path.c_str(), fmt, gz ? 1 : 0, r.program, r.bms, r.n, r.ops.data(), r.ops.size(), r.names, r.ascii, r.asciiOff, r.oo,
                          r.withHit) != LX_OK)
        throw std::runtime_error(std::string("text records on the GPU: ") + lx_last_error(zh));
}

// .bam and *.gz rendered on the host: records, footer and header rendered on the host threads, compressed on the device, written at once
void writeCompressed(std::string const & path, int device, int fmt, EagerRecords const & r, RenderTimes & times)
{
    lx_bytes * raw = nullptr;
    if (lx_render_records(fmt, 1, r.program, r.bms, r.n, r.ops.data(), r.names, r.ascii, r.asciiOff, r.oo, r.withHit, &raw) != LX_OK)
        throw std::runtime_error(outputError(nullptr, path));
    BytesOwner const     keep(raw);
    auto const           tZip = Clock::now();
    HandleOwner const    zh   = makeHandle(device);
    std::vector<uint8_t> packed(lx_bgzf_bound(lx_bytes_size(raw)));
    uint64_t             got = 0;
    if (lx_bgzf_compress(zh.get(), lx_bytes_data(raw), lx_bytes_size(raw), packed.data(), packed.size(), &got, LX_BGZF_EOF) != LX_OK)
        throw std::runtime_error(std::string("BGZF compression: ") + lx_last_error(zh.get()));
    times.msCompress = msSince(tZip);
    std::FILE * of   = std::fopen(path.c_str(), "wb");
    bool        ok   = of && std::fwrite(packed.data(), 1, got, of) == got;
    ok               = of && (std::fclose(of) == 0) && ok;
    if (!ok)
        throw std::runtime_error("cannot write " + path);
}

// a plain text file: the host writer
void writePlain(std::string const & path, int fmt, EagerRecords const & r)
{
    if (lx_write_records_ex(path.c_str(), fmt, 1, r.program, r.bms, r.n, r.ops.data(), r.names, r.ascii, r.asciiOff, r.oo) != LX_OK)
        throw std::runtime_error(outputError(nullptr, path));
    if (lx_write_footer(path.c_str(), fmt, (uint64_t)r.withHit) != LX_OK) // myWriteFooter, src/search.cpp
        throw std::runtime_error("cannot write " + path);
}

// the LCA over the records of every worker together, then the writer --render and the format ask for
RenderTimes writeEager(Options const & opt, Run const & run, int device, OutputSetup const & output, Inputs const & in, Totals const & t)
{
    std::vector<char const *> const qid = cstrs(in.qs.ids), sid = cstrs(in.db.ids);
    lx_seq_names const names{qid.data(), in.qs.orig_len.data(), sid.data(), in.db.orig_len.data(), qid.size(), sid.size()};
    lx_output_options     oo = output.options;
    oo.q_qual                = opt.samQual ? qualOf(in.qs) : nullptr; // (--sam-bam-qual yes: every eager writer reads it from the options)
    std::vector<uint64_t> lcaQid;
    std::vector<uint32_t> lcaTax;
    RenderTimes           times;
    if (output.lca)
    {
        uint64_t          nLca = 0;
        auto const        tLca = Clock::now();
        HandleOwner const lh   = output.lcaOnGpu ? makeHandle(device) : HandleOwner();
        TaxDevOwner const dev  = output.lcaOnGpu ? makeTaxDev(lh.get(), output) : TaxDevOwner();
        computeLca(output, lh.get(), dev.get(), t.bms.data(), t.nOut, lcaQid, lcaTax, nLca);
        times.msLca = msSince(tLca);
        oo.lca_qid  = lcaQid.data();
        oo.lca_tax  = lcaTax.data();
        oo.n_lca    = nLca;
    }
    EagerRecords const r{run.program, t.bms.data(), t.nOut, t.ops, &names, reinterpret_cast<uint8_t const *>(in.qs.ascii.data()), in.qs.ascii_off.data(),
                         &oo,         (int64_t)t.rst.qrys_with_hit};
    if (opt.render == "gpu")
    {
        bool const        bam = run.outFmt == LX_OUT_BAM;
        HandleOwner const zh  = makeHandle(device);
        if (bam)
            writeBamOnGpu(opt.output, zh.get(), r);
        else
            writeTextOnGpu(opt.output, zh.get(), run.outFmt, run.outGz, r);
        float msK = 0;
        (void)lx_last_phase_ms(zh.get(), bam ? 11 : 12, &msK, nullptr);
        times.msRenderDev = msK;
        times.onGpu       = true;
    }
    else if (run.outFmt == LX_OUT_BAM || run.outGz)
        writeCompressed(opt.output, device, run.outFmt, r, times);
    else
        writePlain(opt.output, run.outFmt, r);
    return times;
}

// ---- the summary on stderr: the counts, where the wall clock went (the reference prints its own at verbosity 2, src/search.cpp),
// and for --lazy-query the blocks
void report(Options const & opt, Run const & run, Inputs const & in, Table const & table, SearchSetup const & setup, TaxonSetup const & taxon, Totals const & t,
            LazyTotals const & lazy, RenderTimes const & times, double msSearch, double msOutput)
{
    int const fmt = run.outFmt;
    std::fprintf(stderr,
                 "lambda3 %s (%s, %u host thread(s), %zu handle(s) on %zu device(s)): %zu queries, %zu subjects (%llu residues); seeds %zu -> promising %zu -> "
                 "windows %llu -> traced %llu -> HSPs %llu -> written %llu (queries with hit: %llu)\n",
                 opt.cmd.c_str(), run.program, run.nThreads, setup.nWorkers, setup.devices.size(), run.lazy ? (size_t)lazy.counts.reads : in.qs.ids.size(),
                 in.db.ids.size(), (unsigned long long)setup.sp.db_total_length, (size_t)t.sst.hitsAfterSeeding, t.nPromising,
                 (unsigned long long)(t.ist.num_ext_score - t.ist.hits_duplicate), (unsigned long long)t.ist.num_ext_ali, (unsigned long long)t.nHsp,
                 (unsigned long long)t.nOut, (unsigned long long)t.rst.qrys_with_hit);
    // (--lazy-query: the query file was decompressed while the blocks were searched; its stream has the counts)
    std::string const gunzipNote = in.gunzipNote + (in.qStream ? in.qStream->gunzipNote() : std::string());
    std::string const tableNote = run.fromIndex ? "(read from the index) " : table.tableOnGpu ? "(" + table.onGpu() + ") " : "";
    std::string       outputNote;
    if (times.onGpu)
        outputNote = std::string(", ") + (fmt == LX_OUT_BAM ? "BAM" : fmt == LX_OUT_SAM ? "SAM" : "tabular") + " records rendered" +
                     (fmt == LX_OUT_BAM || run.outGz ? " and BGZF-compressed" : "") + " on the GPU (render kernels " + std::to_string((long)(times.msRenderDev + 0.5)) + ")";
    else if (fmt == LX_OUT_BAM || run.outGz)
        outputNote = ", BGZF compression on the GPU " + std::to_string((long)(times.msCompress + 0.5));
    std::fprintf(stderr,
                 "lambda3 times [ms]: read %.0f%s, reduce + word table %s%.0f, search %.0f (seeding on the %s %.0f [%zu read(s) and %zu launch(es) left to "
                 "the host] + extension on the GPU incl. widen / merge / statistics %.0f on the slowest worker), records %.1f (%s), records + output %.0f%s, total %.0f\n",
                 in.msRead, gunzipNote.c_str(), tableNote.c_str(), table.msIndex, msSearch, t.gpuSeeding ? "GPU" : "host", t.msSeed, t.nDeclined,
                 t.nPassesOnHost, t.msExtend, t.msRecords, run.recordsOnGpu ? "kernels on the GPU, slowest worker" : "host", msOutput - times.msCompress,
                 outputNote.c_str(), msSince(run.tStart));
    if (opt.maxHsps || opt.cullingLimit)
        std::fprintf(stderr, "lambda3 culling: --max-hsps %llu dropped %llu record(s), --culling-limit %llu dropped %llu record(s), %s\n",
                     (unsigned long long)opt.maxHsps, (unsigned long long)t.cst.hits_max_hsps, (unsigned long long)opt.cullingLimit,
                     (unsigned long long)t.cst.hits_culled, run.recordsOnGpu ? "on the GPU (the host for a pass whose list stood in host memory)" : "on the host");
    if (run.wantLca && (opt.lca == "gpu" || opt.lcaTopGiven))
        std::fprintf(stderr, "lambda3 LCA: records within %g percent of a query's best bit score, folded on the %s: %.1f ms%s\n", opt.lcaTopPercent,
                     opt.lca != "host" ? "GPU" : "host", run.lazy ? t.msLca : times.msLca, run.lazy ? " on the slowest worker" : "");
    if (taxon.on)
        std::fprintf(stderr, "lambda3 taxon filter: %llu of %llu subjects kept; %llu of %zu promising seeds dropped; on the %s (%.1f ms)\n",
                     (unsigned long long)taxon.nKept, (unsigned long long)taxon.nSubjects, (unsigned long long)t.nTaxonDropped, t.nPromising,
                     t.taxonOnGpu ? "GPU" : "host", t.msTaxon);
    if (opt.queryMasking == "dust")
        std::fprintf(stderr, "lambda3 query masking: dust %d/%d, %llu of %llu letters masked, %llu sequence(s) touched, on the %s, %.1f ms\n", opt.dustWindow,
                     opt.dustLevel, (unsigned long long)(run.lazy ? t.maskSum[1] : t.nMasked), (unsigned long long)(run.lazy ? t.maskSum[0] : t.nMaskLetters),
                     (unsigned long long)(run.lazy ? t.maskSum[2] : t.nMaskSeqs), t.maskOnGpu ? "GPU" : "host", t.msMask);
    if (opt.queryMasking == "seg")
        std::fprintf(stderr, "lambda3 query masking: seg %d/%g/%g, %llu of %llu letters masked, %llu sequence(s) touched, on the %s, %.1f ms\n", opt.segWindow, opt.segK1,
                     opt.segK2, (unsigned long long)(run.lazy ? t.maskSum[1] : t.nMasked), (unsigned long long)(run.lazy ? t.maskSum[0] : t.nMaskLetters),
                     (unsigned long long)(run.lazy ? t.maskSum[2] : t.nMaskSeqs), t.maskOnGpu ? "GPU" : "host", t.msMask);
    if (run.lazy)
        std::fprintf(stderr, "lambda3 query blocks: %llu block(s) of at most %llu read(s), %llu read(s) in the largest, at most %llu block(s) alive at once\n",
                     (unsigned long long)lazy.counts.blocks, (unsigned long long)run.blockReads, (unsigned long long)lazy.counts.largest,
                     (unsigned long long)lazy.counts.maxAlive);
}

} // namespace

int main(int argc, char ** argv)
{
    try
    {
        Options const opt = parse(argc, argv);
        Run           run(opt);
        Inputs        in    = loadInputs(opt, run);
        Table const   table = makeWordTable(opt, run, in.db, in.indexFile);
        if (run.mk)
            return runMkindex(opt, run, in, table);
        std::vector<uint8_t> const qRed = reduce(in.qs, run.red);
        TaxonSetup const           taxon(opt, run, table.indexTax);
        SearchSetup const          setup = prepareSearch(opt, run, in);
        OutputSetup const          output(opt, run, table.indexTax);
        SearchContext const        search{opt, run, setup, in.db, table, taxon};
        std::vector<Part>          parts(setup.nWorkers);

        auto const tSearch = Clock::now();
        LazyTotals lazy;
        if (run.lazy)
            lazy = runLazy(search, *in.qStream, output, parts);
        else
            runEager(search, in.qs, qRed, parts);
        double const msSearch = msSince(tSearch);

        auto const   tOut   = Clock::now();
        Totals const totals = sumParts(opt, run, in.qs, parts, lazy);
        RenderTimes const times = run.lazy ? lazy.times : writeEager(opt, run, setup.devices[0], output, in, totals);
        report(opt, run, in, table, setup, taxon, totals, lazy, times, msSearch, msSince(tOut));
        return 0;
    }
    catch (std::exception const & e)
    {
        std::cerr << "\nERROR: " << e.what() << "\n";
        return -1; // src/search.cpp:98-125
    }
}
