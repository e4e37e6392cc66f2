// cli/options.hpp -- the command line of the lambda3 front end: its options with the reference's defaults, the parser with the
// reference's refusals, the output format from the file name.  Included by lambda3_main.cpp only (its header comment is the manual).
#pragma once

#include "common.hpp"

namespace
{

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
    bool        samQual = false;      // --sam-bam-qual yes: a FASTQ query's base qualities into SAM's column 11 / BAM's qual (the header comment)
    std::string commandLine;
    std::vector<int> devices;         // --devices (default: every visible device)
    std::string table       = "auto"; // --table gpu | host | auto: where the word table is made (auto: search* on the GPU, mkindex* on the host)
    uint64_t    tableSlice  = 0;      // --table-slice N: the GPU makes the table in slices of at most N words (0: one sort where it can, slices of 2^30 where it cannot)
    std::string seeding     = "gpu";  // --seeding gpu | host: where search() runs (lx_seed_queries on the worker's handle -- one lane per read, reads
                                      // the device declines are finished on the host threads inside the call --, or on the -t threads)
    std::string render      = "auto"; // --render gpu | host | auto: where the records of the output are made (the header comment)
    std::string records     = "auto"; // --records gpu | host | auto: where _writeRecord's sort / unique / sort / cut runs (the header comment)
    uint64_t    maxHsps     = 0;      // --max-hsps K: at most K records per (query, subject) pair, the best ones (0: off; the header comment)
    uint64_t    cullingLimit = 0;     // --culling-limit L: drop a record whose query interval L better records of its query envelop (0: off)
    std::string lca         = "auto"; // --lca gpu | host | auto: where the LCA per query is folded (the header comment)
    double      lcaTopPercent = 100;  // --lca-top-percent P: only the records within P percent of a query's best bit score enter its LCA (100: all)
    bool        lcaTopGiven = false;
    std::vector<uint32_t> taxonList;     // --taxon-list T1,T2,... / --taxon-exclude T1,T2,...: search only the subjects under these taxa, or all but them
    bool        taxonExclude = false;    // (the list came from --taxon-exclude)
    std::string taxonFilter = "auto";    // --taxon-filter gpu | host | auto: where the subject mask is made and the match list filtered (auto: where the list stands)
    std::string queryMasking = "none";   // --query-masking none | seg (searchp) | dust (searchn, searchbs): mask low-complexity query regions before seeding (the header comment)
    std::string masking     = "auto";    // --masking gpu | host | auto: where the query mask is made (auto: where the seeding runs)
    int         segWindow   = 12;        // --seg-window W, --seg-k1 X, --seg-k2 Y: the rule's window and its two entropy bounds in bits (SEG's defaults)
    double      segK1 = 2.2, segK2 = 2.5;
    int         dustWindow = 64, dustLevel = 20; // --dust-window W, --dust-level L: DUST's longest interval in letters and ten times its score bound (dustmasker's defaults)
    int         threads    = 0;    // -t host threads for the word table and the seeding (default: what the machine grants)
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

// The output format from the file name (src/search_options.hpp:684-710): .m8, .m9, .sam or .bam; the text formats also BGZF-
// compressed (.gz).  .m0 (the pairwise report), .bz2 and .bam.gz are refused.
char const * const kFormatMessage =
    "output format is chosen by the extension: .m8, .m9, .sam or .bam, the first three optionally with .gz (.m0, .bz2 and .bam.gz are not supported)";
int outputFormat(std::string const & path, bool & gz)
{
    gz                     = endsWith(path, ".gz");
    std::string const base = gz ? path.substr(0, path.size() - 3) : path;
    if (endsWith(base, ".m9"))
        return LX_OUT_BLAST_TAB_COMMENTS;
    if (endsWith(base, ".sam"))
        return LX_OUT_SAM;
    if (endsWith(base, ".m8"))
        return LX_OUT_BLAST_TAB;
    if (endsWith(base, ".bam") && !gz)
        return LX_OUT_BAM;
    throw std::runtime_error(kFormatMessage);
}

Options parse(int argc, char ** argv)
{
    Options o;
    if (argc < 2)
        throw std::runtime_error("usage: lambda3 searchp|searchn|searchbs -q QUERY.{fa,fq,fasta,fastq,fna,faa}[.gz] (-i DB.lba | -d DB.fasta[.gz]) -o OUT.{m8,m9,sam,bam,m8.gz,m9.gz,sam.gz} [-e EVALUE] [-n N] "
                                 "[--devices 0,1,...] [-t THREADS]\n                 [--max-hsps K] [--culling-limit L]   between the duplicate removal and the cut to -n, per query, best records first: drop a record\n"
                                 "                 when K better ones hit the same subject; then drop a record when L better ones envelop its query interval (qstart .. qend as the\n"
                                 "                 .m8 prints them; equal intervals envelop each other).  0 = off (default); the seeding's budget stays -n\n                 [--lca-top-percent P] [--lca gpu|host|auto]   the LCA per query (lcataxid, lt, ls) over the records within P percent of the query's best\n"
                                 "                 bit score (0 .. 100, default 100: all records, the reference's rule), folded on the GPU or on the host (auto: the GPU)\n                 [--taxon-list T1,T2,... | --taxon-exclude T1,T2,...] [--taxon-filter gpu|host|auto]   search only the subjects under the listed taxa of the\n"
                                 "                 index's tree (mkindex* -m -x), or all but them (a subject without taxa is dropped by a list and kept by an exclusion); the promising\n"
                                 "                 seeds on other subjects are dropped before the extension, on the GPU or on the host (auto: where the seeding left them); e-values\n"
                                 "                 and bit scores keep the whole database's length; with --search0 1 a read whose hits all lie outside goes on to the second pass; the seeding aims\n"
                                 "                 at -n + the number of dropped subjects (at most 64 matches per read, never fewer than -n) instead of -n\n                 [--query-masking none|seg] [--masking gpu|host|auto] [--seg-window W] [--seg-k1 X] [--seg-k2 Y]   searchp: mask low-complexity query regions\n"
                                 "                 before seeding (default none): a window of W letters (4 .. 64, default 12) of at most Y bits of entropy (default 2.5) belongs to a\n"
                                 "                 low-complexity run, a run with a window of at most X bits (default 2.2) is masked -- SEG's first two stages, without its trimming, so\n"
                                 "                 a mask is SEG's segment or wider; not segmasker.  A masked letter starts and carries no seed; extension, statistics and output read\n"
                                 "                 the unmasked query.  The mask is made on the GPU or on the host threads (auto: where the seeding runs)\n                 [--query-masking none|dust] [--masking gpu|host|auto] [--dust-window W] [--dust-level L]   searchn, searchbs: the same with the nucleotide\n"
                                 "                 rule, symmetric DUST (Morgulis et al. 2006) in integers: within a stretch of A, C, G, T an interval of l overlapping triplets scores\n"
                                 "                 r / (l - 1), r = the sum over triplet kinds of c (c - 1) / 2; a letter is masked when it lies in an interval of at most W letters\n"
                                 "                 (4 .. 64, default 64) that scores above L / 10 (1 .. 1000, default 20) and holds no sub-interval that scores higher; N is never\n"
                                 "                 masked and ends every interval.  dustmasker's -linker is not built, and the masks were not compared with dustmasker's or sdust's\n"
                                 "                 (10^6 reads x 2 frames x 150 letters: 1944 ms on 16 host threads, 39 ms on the GPU with the upload)\n                 [--lazy-query 1] [--query-block N]   search the query file block by block in bounded memory: at most N reads per block\n"
                                 "                 (default 1048576, not measured yet; a block also closes at 2^30 letters; a query read from a pipe is held whole, compressed)\n                 [--sam-bam-qual no|yes]   .sam, .sam.gz, .bam: write a FASTQ query's base qualities as QUAL (default no: '*' / 0xFF, the bytes\n"
                                 "                 every earlier version wrote): exactly where SEQ is written (--sam-bam-seq, --sam-bam-clip), over the same letters, reversed on the\n"
                                 "                 minus strand; a translated query's over the nucleotides of its window.  A byte outside '!' .. '~' in a quality line is refused; a\n"
                                 "                 FASTA query has none (one note on stderr, QUAL stays '*').  Under yes a block of reads holds its letters twice (letters, qualities)\n       lambda3 mkindexp|mkindexn|mkindexbs -d DB.{fa,fq,fasta,fastq,fna,faa}[.gz] [-i DB.lba] [-r li10|murphy10|none] [-g CODE] [-t THREADS]\n                 [-m MAP.{accession2taxid,dat}[.gz] [-x TAXDUMP_DIR]]");
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
        if (!(v >= lo && v <= hi)) // (not a number is outside, too)
            throw std::runtime_error("Value " + std::to_string(v) + " of option " + name + " is not in range [" + std::to_string(lo) + "," + std::to_string(hi) + "].");
    };
    auto oneOf = [](std::string const & v, std::initializer_list<char const *> allowed, char const * message) // v, if it is one of them
    {
        for (char const * word : allowed)
            if (v == word)
                return v;
        throw std::runtime_error(message);
    };
    auto taxa = [](std::string const & name, std::string const & v) // T1,T2,...: taxon ids, 1 .. 2^32 - 1
    {
        std::vector<uint32_t> out;
        for (size_t at = 0; at <= v.size();)
        {
            size_t const      e = std::min(v.find(',', at), v.size());
            std::string const t = v.substr(at, e - at);
            bool const        digits = !t.empty() && t.size() <= 10 && std::all_of(t.begin(), t.end(), [](char c) { return c >= '0' && c <= '9'; });
            unsigned long long const id = digits ? std::stoull(t) : 0;
            if (!digits || id == 0 || id > 0xffffffffull)
                throw std::runtime_error(name + " takes a comma-separated list of taxon ids (numbers from 1 to 4294967295), got '" + t + "' in '" + v + "'");
            out.push_back((uint32_t)id);
            at = e + 1;
        }
        return out;
    };
    bool taxonFilterGiven = false;
    std::string maskingDetail; // the first of --masking / --seg-* that was given
    std::string segDetail, dustDetail; // the first of --seg-* / of --dust-*
    bool        maskingGiven = false;
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
            o.dbIndexType = oneOf(val(), {"fm", "bifm"}, "--db-index-type takes fm or bifm");
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
            o.profile = oneOf(val(), {"none", "fast", "sensitive", "pairs-default", "pairs-sensitive"},
                              "--profile takes none, fast, sensitive, pairs-default or pairs-sensitive");
        else if (a == "--output-columns")
            o.outputColumns = val();
        else if (a == "--sam-bam-tags")
            o.samTags = val();
        else if (a == "--sam-bam-seq")
            o.samSeq = oneOf(val(), {"always", "uniq", "never"}, "--sam-bam-seq takes always, uniq or never");
        else if (a == "--sam-bam-clip")
            o.samClip = oneOf(val(), {"hard", "soft"}, "--sam-bam-clip takes hard or soft");
        else if (!mk && a == "--sam-bam-qual")
            o.samQual = oneOf(val(), {"no", "yes"}, "--sam-bam-qual takes no or yes") == "yes";
        else if (a == "--sam-with-refheader")
            o.samWithRefHeader = onOff(val());
        else if (a == "--version-to-outputfile")
            o.versionToOutput = onOff(val());
        else if (a == "-r" || a == "--alphabet-reduction")
            o.reduction = oneOf(val(), {"none", "murphy10", "li10"}, "--alphabet-reduction takes none, murphy10 or li10");
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
            o.table = oneOf(val(), {"gpu", "host", "auto"}, "--table takes gpu, host or auto");
        else if (a == "--table-slice") // (LX_OPT_INDEX_SLICE_WORDS: the device build in slices of the key space)
        {
            std::string const v = val();
            bool              ok = !v.empty() && v.size() <= 18 && std::all_of(v.begin(), v.end(), [](char c) { return c >= '0' && c <= '9'; });
            o.tableSlice         = ok ? std::stoull(v) : 0;
            if (o.tableSlice == 0)
                throw std::runtime_error("--table-slice takes a number of words (at least 1): the most one slice of the GPU's word table build may hold");
        }
        else if (a == "--records")
            o.records = oneOf(val(), {"gpu", "host", "auto"}, "--records takes gpu, host or auto");
        else if (!mk && (a == "--max-hsps" || a == "--culling-limit"))
        {
            std::string const v  = val();
            bool const        ok = !v.empty() && v.size() <= 18 && std::all_of(v.begin(), v.end(), [](char c) { return c >= '0' && c <= '9'; });
            if (!ok)
                throw std::runtime_error(a + " takes a number (0 = off, the default), got '" + v + "'");
            (a == "--max-hsps" ? o.maxHsps : o.cullingLimit) = std::stoull(v);
        }
        else if (a == "--lca")
            o.lca = oneOf(val(), {"gpu", "host", "auto"}, "--lca takes gpu, host or auto");
        else if (a == "--lca-top-percent")
        {
            o.lcaTopPercent = std::stod(val());
            inRange(a, o.lcaTopPercent, 0, 100);
            o.lcaTopGiven = true;
        }
        else if (!mk && (a == "--taxon-list" || a == "--taxon-exclude"))
        {
            if (!o.taxonList.empty())
                throw std::runtime_error("--taxon-list and --taxon-exclude are given once, and only one of them: search under some taxa or everything except some");
            o.taxonList    = taxa(a, val());
            o.taxonExclude = a == "--taxon-exclude";
        }
        else if (!mk && a == "--taxon-filter")
        {
            o.taxonFilter   = oneOf(val(), {"gpu", "host", "auto"}, "--taxon-filter takes gpu, host or auto");
            taxonFilterGiven = true;
        }
        else if (!mk && a == "--query-masking")
        {
            std::string const v = val();
            if (v == "seg" && !prot)
                throw std::runtime_error("--query-masking seg: SEG is the protein rule (searchp); for " + o.cmd +
                                         " the nucleotide form of SEG, unlike DUST, is not built: use --query-masking dust");
            o.queryMasking = prot ? oneOf(v, {"none", "seg"}, "--query-masking takes none or seg (dust is the rule of searchn and searchbs)")
                                  : oneOf(v, {"none", "dust"}, "--query-masking takes none or dust");
        }
        else if (!mk && (a == "--masking" || a == "--seg-window" || a == "--seg-k1" || a == "--seg-k2"))
        {
            if (maskingDetail.empty())
                maskingDetail = a;
            if (a != "--masking" && segDetail.empty())
                segDetail = a;
            if (a == "--masking")
            {
                o.masking    = oneOf(val(), {"gpu", "host", "auto"}, "--masking takes gpu, host or auto");
                maskingGiven = true;
            }
            else if (a == "--seg-window")
                o.segWindow = std::stoi(val());
            else
                (a == "--seg-k1" ? o.segK1 : o.segK2) = std::stod(val());
        }
        else if (!mk && (a == "--dust-window" || a == "--dust-level"))
        {
            if (dustDetail.empty())
                dustDetail = a;
            (a == "--dust-window" ? o.dustWindow : o.dustLevel) = std::stoi(val());
        }
        else if (a == "--render")
            o.render = oneOf(val(), {"gpu", "host", "auto"}, "--render takes gpu, host or auto");
        else if (a == "--seeding")
            o.seeding = oneOf(val(), {"host", "gpu"}, "--seeding takes host or gpu");
        else if (a == "--db-alphabet")
            o.dbAlphabet = oneOf(val(), {"auto", "dna5", "aminoacid"}, "--db-alphabet takes auto, dna5 or aminoacid");
        else if (a == "-a" || a == "--query-alphabet" || a == "--input-alphabet") // (the reference's name is --input-alphabet, :172-185)
            // (mkindexp: the database's, src/mkindex_options.hpp:189-197)
            (mk ? o.dbAlphabet : o.qryAlphabet) = oneOf(val(), {"auto", "dna5", "aminoacid"}, "--input-alphabet takes auto, dna5 or aminoacid");
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
        if (!endsWith(o.index, ".lba") && !endsWith(o.index, ".lta")) // :133, :145
            throw std::runtime_error("the index file name must end in .lba or .lta");
        if (!o.taxDumpDir.empty() && o.accTaxMap.empty()) // :256-264
            throw std::runtime_error("There is no point in including a taxonomic tree in the index, if you don't also include taxonomic IDs for your sequences.");
        if (!o.accTaxMap.empty())
        {
            std::string const & map = o.accTaxMap;
            if (endsWith(map, ".accession2taxid.bz2") || endsWith(map, ".dat.bz2"))
                throw std::runtime_error(map + ": bzip2-compressed input is not supported (decompress it, or recompress it with gzip or bgzip)");
            if (!endsWith(map, ".accession2taxid") && !endsWith(map, ".accession2taxid.gz") && !endsWith(map, ".dat") && !endsWith(map, ".dat.gz"))
                throw std::runtime_error("-m " + map + ": the accession-to-taxonomy map must be named *.accession2taxid or *.dat, optionally .gz");
        }
        if (std::ifstream(o.index).good()) // :252-256
            throw std::runtime_error("ERROR: An output file already exists at " + o.index + "\n       Remove it, or choose a different location.");
        return o;
    }
    if (!dustDetail.empty() && o.queryMasking != "dust")
        throw std::runtime_error(dustDetail + " belongs to --query-masking dust" + (prot ? ", the rule of searchn and searchbs" : ": give that too"));
    if (prot && !maskingDetail.empty() && o.queryMasking != "seg")
        throw std::runtime_error(maskingDetail + " belongs to --query-masking seg: give that too");
    if (!prot && !segDetail.empty())
        throw std::runtime_error(segDetail + " belongs to --query-masking seg, the protein rule (searchp)");
    if (!prot && maskingGiven && o.queryMasking != "dust")
        throw std::runtime_error("--masking belongs to --query-masking dust: give that too");
    if (o.queryMasking == "dust")
    {
        if (o.dustWindow < 4 || o.dustWindow > 64)
            throw std::runtime_error("--dust-window takes 4 .. 64 (letters: the longest interval the rule scores)");
        if (o.dustLevel < 1 || o.dustLevel > 1000)
            throw std::runtime_error("--dust-level takes 1 .. 1000 (ten times the score bound; 20 is dustmasker's)");
    }
    if (o.queryMasking == "seg")
    {
        lx_seg_params const sp{o.segWindow, o.segK1, o.segK2};
        int64_t             T[65], thr1 = 0, thr2 = 0;
        if (lx_seg_tables(&sp, T, &thr1, &thr2) != LX_OK)
            throw std::runtime_error(std::string("--seg-window takes 4 .. 64, --seg-k1 and --seg-k2 bits with 0 < k1 <= k2 <= log2(window) (") + lx_last_output_error() + ")");
    }
    if (o.query.empty() || o.db.empty())
        throw std::runtime_error("-q and -d (a FASTA file) or -i (an index made by lambda3 mkindex*) are required");
    if (taxonFilterGiven && o.taxonList.empty())
        throw std::runtime_error("--taxon-filter says where --taxon-list / --taxon-exclude is applied: give one of them");
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
        if (o.samQual && fmt != LX_OUT_SAM && fmt != LX_OUT_BAM)
            throw std::runtime_error("--sam-bam-qual yes: base qualities are a field of SAM and BAM records (.sam, .sam.gz, .bam); " + o.output +
                                     " is a tabular format, which has no column for them");
        if (o.samQual && o.samSeq == "never")
            throw std::runtime_error("--sam-bam-qual yes with --sam-bam-seq never: QUAL is written where SEQ is written, over the same letters, so "
                                     "without SEQ every record's QUAL would be '*'");
    }
    return o;
}

} // namespace
