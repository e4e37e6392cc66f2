// cli/index_file.hpp -- the index file of `lambda3 mkindex*`: its layout, writer and readers, and the taxonomy of mkindex -m / -x.
// Included by lambda3_main.cpp only.
//
// The file holds what the reference's index_file holds (src/shared_definitions.hpp:343-379:
// the options that fix the types, the ids, the sequences in the translated alphabet, the taxonomy when -m was given), and this front end's
// word table in place of the FM-index.  NOT the reference's on-disk format: that is a cereal archive of fmindex-collection
// objects, neither of which is available here; a file of the reference is recognised by the missing magic and refused.
#pragma once

#include "sequences.hpp"

namespace
{

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
    BytesOwner const keepTable(table);
    FILE *           f = std::fopen(path.c_str(), "wb");
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

// the word table's bytes; f stands right behind the head (readIndexHead).  Its header says how many (ReducedIndex::save: 16 + 16
// bytes, the entries, the prefix table).  false: truncated, or not a table over `dbLetters` letters
bool readIndexTable(FILE * f, uint64_t dbLetters, std::vector<uint8_t> & bytes)
{
    bytes.resize(32);
    if (std::fread(bytes.data(), 1, 32, f) != 32)
        return false;
    uint64_t cnt[2];
    std::memcpy(cnt, bytes.data() + 16, sizeof(cnt));
    if (cnt[0] != dbLetters || cnt[1] > (1ull << 32))
        return false;
    bytes.resize(32 + cnt[0] * 16 + cnt[1] * 8);
    return std::fread(bytes.data() + 32, 1, bytes.size() - 32, f) == bytes.size() - 32;
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
    auto const t0 = Clock::now();
    bool const ncbi = endsWith(map, ".accession2taxid") || endsWith(map, ".accession2taxid.gz"); // (else *.dat[.gz]: parse() admits nothing else)
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
    std::unique_ptr<lx_taxmap, FreeWith<lx_taxmap_destroy>> const keep(tm);
    auto check = [&](int rc)
    {
        if (rc != LX_OK)
            throw std::runtime_error("-m " + map + ": " + (h ? lx_last_error(h) : lx_last_output_error()));
    };
    std::FILE * f = std::fopen(map.c_str(), "rb");
    if (!f)
        throw std::runtime_error("cannot open " + map);
    FileOwner const   keepF(f);
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
        BytesOwner const keepT(text);
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
    msJoin   = msSince(t0);
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
    std::unique_ptr<lx_taxonomy, FreeWith<lx_taxonomy_free>> const keepTree(tree);
    lx_taxonomy_info info;
    (void)lx_taxonomy_get(tree, &info);
    std::fputs(info.warnings, stderr);
    tax.hasTree = true;
    tax.parents.assign(info.parents, info.parents + info.n_taxa);
    tax.heights.assign(info.heights, info.heights + info.n_taxa);
    tax.names.assign(info.names, info.names + info.n_taxa);
    std::fprintf(stderr, "Number of nodes in tree: %llu\nMaximum Tree Height: %u\n", (unsigned long long)info.n_nodes, info.max_height);
}

} // namespace
