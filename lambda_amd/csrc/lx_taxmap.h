// lx_taxmap.h -- the accession-to-taxon join, one statement for the host and the device: the join kernel (lx_taxmap.hip) and the host
// threads (lx_taxmap_host.cpp) parse the map lines with the same code, and mkindex's accession extraction uses the same matcher.
// Not part of the ABI.
//
//   * find_accession: the reference's accession regex (src/mkindex_algo.hpp:72-80) written out by hand, with ECMAScript's
//     semantics: at the leftmost position where any alternative matches, the first alternative in order that matches wins; its
//     {1,2}, {8,10} and + are greedy, and nothing follows them inside their alternative, so each alternative has exactly one length
//     to try per count.  Every non-overlapping match, left to right (std::cregex_iterator).
//   * the two map formats (src/mkindex_misc.hpp:69-144): tab-separated lines; field 0 is the accession, field 2 the taxon; the UniProt
//     form only counts lines whose field 1 is "NCBI_TaxID".  A missing field is empty.
//   * parse_taxid: std::from_chars into uint32_t, checking only the error code: leading digits, no sign, no space; none or too many
//     is an error, anything after the digits is ignored.
//   * the accession table: open addressing over 64-bit FNV-1a hashes; a slot holds (upper 32 bits of the hash) << 32 | key index,
//     and a fingerprint hit is confirmed by comparing the key's bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lx
{
namespace taxmap
{

enum : int
{
    kFormatNcbi    = 0, // *.accession2taxid: header "accession\taccession.version\ttaxid\tgi", then acc / acc.version / taxid / gi
    kFormatUniprot = 1, // *.dat (idmapping.dat): acc / category / value, only category NCBI_TaxID
};

constexpr uint64_t kEmptySlot = ~0ull;

__host__ __device__ inline bool is_upper(uint8_t c) { return c >= 'A' && c <= 'Z'; }
__host__ __device__ inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// the length of the match at s[p] (0: none); s[0, n)
__host__ __device__ inline uint32_t match_at(uint8_t const * s, uint64_t n, uint64_t p)
{
    uint64_t const r = n - p; // bytes left
    auto up  = [&](uint64_t k) { return k < r && is_upper(s[p + k]); };
    auto dig = [&](uint64_t k) { return k < r && is_digit(s[p + k]); };
    auto aln = [&](uint64_t k) { return up(k) || dig(k); };
    auto digits = [&](uint64_t a, uint64_t cnt) // cnt digits from a
    {
        for (uint64_t k = a; k < a + cnt; ++k)
            if (!dig(k))
                return false;
        return true;
    };
    auto uppers = [&](uint64_t cnt)
    {
        for (uint64_t k = 0; k < cnt; ++k)
            if (!up(k))
                return false;
        return true;
    };
    if (!up(0))
        return 0;
    uint8_t const c0 = s[p];
    // [OPQ][0-9][A-Z0-9]{3}[0-9]
    if ((c0 == 'O' || c0 == 'P' || c0 == 'Q') && dig(1) && aln(2) && aln(3) && aln(4) && dig(5))
        return 6;
    // [A-NR-Z][0-9]([A-Z][A-Z0-9]{2}[0-9]){1,2}
    if (!(c0 == 'O' || c0 == 'P' || c0 == 'Q') && dig(1) && up(2) && aln(3) && aln(4) && dig(5))
        return (up(6) && aln(7) && aln(8) && dig(9)) ? 10 : 6;
    // [A-Z][0-9]{5}
    if (digits(1, 5))
        return 6;
    // [A-Z]{2}[0-9]{6}
    if (uppers(2) && digits(2, 6))
        return 8;
    // [A-Z]{3}[0-9]{5}
    if (uppers(3) && digits(3, 5))
        return 8;
    // [A-Z]{4}[0-9]{8,10}
    if (uppers(4) && digits(4, 8))
        return dig(12) ? (dig(13) ? 14 : 13) : 12;
    // [A-Z]{5}[0-9]{7}
    if (uppers(5) && digits(5, 7))
        return 12;
    // (NC|AC|NG|NT|NW|NZ|NM|NR|XM|XR|NP|AP|XP|YP|ZP)_[0-9]+
    if (up(1) && r > 3 && s[p + 2] == '_' && dig(3))
    {
        uint8_t const a = c0, b = s[p + 1];
        bool const    ok = (a == 'N' && (b == 'C' || b == 'G' || b == 'T' || b == 'W' || b == 'Z' || b == 'M' || b == 'R' || b == 'P')) ||
                        (a == 'A' && (b == 'C' || b == 'P')) || (a == 'X' && (b == 'M' || b == 'R' || b == 'P')) ||
                        ((a == 'Y' || a == 'Z') && b == 'P');
        if (ok)
        {
            uint64_t k = 4;
            while (dig(k))
                ++k;
            return (uint32_t)k;
        }
    }
    // UPI[A-F0-9]{10}
    if (c0 == 'U' && r >= 13 && s[p + 1] == 'P' && s[p + 2] == 'I')
    {
        for (uint64_t k = 3; k < 13; ++k)
        {
            uint8_t const c = s[p + k];
            if (!(is_digit(c) || (c >= 'A' && c <= 'F')))
                return 0;
        }
        return 13;
    }
    return 0;
}

// the next match at or after `from`: its start (n if none) and *len
__host__ __device__ inline uint64_t find_accession(uint8_t const * s, uint64_t n, uint64_t from, uint32_t * len)
{
    for (uint64_t p = from; p < n; ++p)
        if (uint32_t const l = match_at(s, n, p))
        {
            *len = l;
            return p;
        }
    *len = 0;
    return n;
}

__host__ __device__ inline uint64_t fnv1a_step(uint64_t h, uint8_t c) { return (h ^ c) * 0x100000001b3ull; }
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;

__host__ __device__ inline uint64_t hash_bytes(uint8_t const * p, uint64_t n)
{
    uint64_t h = kFnvBasis;
    for (uint64_t i = 0; i < n; ++i)
        h = fnv1a_step(h, p[i]);
    return h;
}

// std::from_chars(first, last, uint32_t&) over get(a .. a + n) as the reference uses it: false = its error code is set
template <class Get>
__host__ __device__ inline bool parse_taxid(Get const & get, uint64_t a, uint64_t n, uint32_t * out)
{
    uint64_t v = 0, k = 0;
    bool     over = false;
    for (uint8_t c; k < n && is_digit(c = get(a + k)); ++k)
    {
        v = v * 10 + (c - '0');
        if (v > 0xffffffffull)
        {
            over = true;
            v    = 0xffffffffull + 1; // (stays above the limit; the digits are consumed to the end, as from_chars does)
        }
    }
    if (k == 0 || over)
        return false;
    *out = (uint32_t)v;
    return true;
}

// one accession of the table: its bytes at bytes[off, off + len), the subject it maps to
struct Key
{
    uint64_t off;
    uint32_t len;
    uint32_t subject;
};

struct TableView
{
    uint64_t const * slots;   // mask + 1 of them
    uint64_t         mask;
    Key const *      keys;
    uint8_t const *  bytes;
    uint32_t         max_len; // the longest key: a longer field 0 cannot match
};

// the subject of the accession at line bytes [a, a + len) read through `get`, or -1
template <class Get>
__host__ __device__ inline int64_t lookup(TableView const & t, Get const & get, uint64_t a, uint64_t len)
{
    if (len == 0 || len > t.max_len)
        return -1;
    uint64_t h = kFnvBasis;
    for (uint64_t i = 0; i < len; ++i)
        h = fnv1a_step(h, get(a + i));
    uint32_t const fp = (uint32_t)(h >> 32);
    for (uint64_t at = h & t.mask;; at = (at + 1) & t.mask)
    {
        uint64_t const sl = t.slots[at];
        if (sl == kEmptySlot)
            return -1;
        if ((uint32_t)(sl >> 32) != fp)
            continue;
        Key const k = t.keys[(uint32_t)sl];
        if (k.len != len)
            continue;
        uint64_t i = 0;
        while (i < len && t.bytes[k.off + i] == get(a + i))
            ++i;
        if (i == len)
            return k.subject;
    }
}

enum : int
{
    kLineNoMatch = 0,
    kLinePair    = 1, // *subject, *taxid set
    kLineBadTax  = 2, // the accession is in the table, the taxon field does not parse
};

// The line that starts at s and ends at the first '\n' (which the caller guarantees; get(p) for p up to it).  *tax_a / *tax_n: the
// taxon field (for the error text).
template <class Get>
__host__ __device__ inline int parse_line(TableView const & t, int format, Get const & get, uint64_t s, uint32_t * subject, uint32_t * taxid,
                                          uint64_t * tax_a, uint64_t * tax_n)
{
    uint64_t e0 = s;
    uint8_t  c  = 0;
    while ((c = get(e0)) != '\t' && c != '\n')
        ++e0;
    // field 1 from e0 + 1 (if there is one)
    uint64_t f1 = e0, e1 = e0;
    if (c == '\t')
    {
        f1 = e1 = e0 + 1;
        while ((c = get(e1)) != '\t' && c != '\n')
            ++e1;
    }
    if (format == kFormatUniprot)
    {
        char const * const cat = "NCBI_TaxID";
        if (e1 - f1 != 10)
            return kLineNoMatch;
        for (int k = 0; k < 10; ++k)
            if (get(f1 + k) != (uint8_t)cat[k])
                return kLineNoMatch;
    }
    uint64_t f2 = e1, e2 = e1;
    if (c == '\t')
    {
        f2 = e2 = e1 + 1;
        while ((c = get(e2)) != '\t' && c != '\n')
            ++e2;
    }
    int64_t const subj = lookup(t, get, s, e0 - s);
    if (subj < 0)
        return kLineNoMatch;
    *tax_a = f2;
    *tax_n = e2 - f2;
    if (!parse_taxid(get, f2, e2 - f2, taxid))
        return kLineBadTax;
    *subject = (uint32_t)subj;
    return kLinePair;
}

// one (subject, taxon) pair of a matched line
struct Pair
{
    uint32_t subject;
    uint32_t taxid;
};

// ---- the join kernel (lx_taxmap.hip) on one chunk of whole lines: every byte of text[0, n) belongs to a line that ends in '\n'
constexpr uint32_t kJoinThreads = 256;
constexpr uint32_t kJoinTile    = kJoinThreads * 16; // bytes per workgroup, 16 per lane
// pairs per tile at most: a line that yields one is at least 8 bytes long ("NC_1\t\t1\n"; accessions are 4 bytes or more), so two
// of them start at least 8 bytes apart
constexpr uint32_t kJoinTileCap = kJoinTile / 8;

struct JoinCounters
{
    unsigned long long lines;    // lines that start in the chunk
    uint32_t           bad_off;  // the first matched line whose taxon does not parse (byte offset), ~0u = none
    uint32_t           overflow; // a tile made more than kJoinTileCap pairs (never, by the bound above)
};

struct JoinParams
{
    TableView      table;
    int            format;
    uint8_t const * text;       // the chunk, n bytes (< 2^32)
    uint32_t       n;
    Pair *         scratch;     // tiles * kJoinTileCap: each tile's pairs, in line order
    uint32_t *     tile_cnt;    // tiles
    uint32_t *     tile_off;    // tiles: where each tile's pairs go
    uint32_t *     block_tot;   // scan_blocks(tiles) + 1; [scan_blocks] = the chunk's pairs
    Pair *         pairs;       // the chunk's pairs in line order
    JoinCounters * counters;
};

inline uint32_t join_tiles(uint64_t n) { return (uint32_t)((n + kJoinTile - 1) / kJoinTile); }
uint64_t        join_scan_blocks(uint64_t tiles);
hipError_t      launch_taxmap_join(JoinParams const & p, hipStream_t stream);

} // namespace taxmap
} // namespace lx
