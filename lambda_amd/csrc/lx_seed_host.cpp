// lx_seed_host.cpp -- Level 3 of the C ABI (include/lambda_ext.h): the word index (lx_index_*) and search() (lx_seed_queries).
// The table and the host seeder are host/lx_seeding.hpp's (ReducedIndex, seedQueries: the semantics, checked against brute force
// by tests/seeding_check.cpp); the kernels are lx_seed.hip's.  On a handle the table, the reduced subjects and their sequence
// table stay on the handle's device with the index; a call uploads its queries, launches one lane per read and finishes what the
// device declined on the host threads.
#include <memory>
#include <new>

#include "lx_internal.h"
#include "lx_seed.h"

using lambda_amd::ReducedIndex;
using lxi::bind;
using lxi::ensure;
using lxi::fail;

static_assert(sizeof(lx_index_entry) == sizeof(ReducedIndex::Entry) && sizeof(lx_index_entry) == 16, "lx_index_entry is the table's row");
static_assert(sizeof(lx_match) == 48, "six words per match");

namespace
{

// the table on the host, the sequences it refers to (the index's own copy): shared by the indexes lx_index_attach makes
struct HostTable
{
    std::vector<uint8_t>  red;
    std::vector<uint64_t> off, len;
    uint64_t              total = 0; // letters = entries
    ReducedIndex          ix;
    bool                  built_on_device = false;
};

// the text goes where the caller looks for it: the handle, or lx_last_output_error() without one
int say(lx_handle * h, int code, char const * fmt, ...)
{
    char    buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h)
        return fail(h, code, "%s", buf);
    lxi::set_output_error(buf);
    return code;
}

#define LXS_HIP(h, call)                                                                                                                    \
    do                                                                                                                                      \
    {                                                                                                                                       \
        hipError_t e_ = (call);                                                                                                             \
        if (e_ != hipSuccess)                                                                                                               \
            return fail((h), e_ == hipErrorOutOfMemory ? LX_ENOMEM : LX_EHIP, "%s failed: %s", #call, hipGetErrorString(e_));               \
    } while (0)

unsigned threads_or_share(uint32_t asked)
{
    return asked ? asked : std::max(1u, lxi::pool_width());
}

// the largest letter of b[0 .. n) (0 for none), on the host threads
uint8_t top_letter(uint8_t const * b, uint64_t n, unsigned threads)
{
    size_t const         parts = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(threads, n >> 20));
    std::vector<uint8_t> top(parts, 0);
    lambda_amd::parallelChunks(threads, parts,
                               [&](size_t k)
                               {
                                   uint8_t t = 0;
                                   for (uint64_t i = n * k / parts, e = n * (k + 1) / parts; i < e; ++i)
                                       t = std::max(t, b[i]);
                                   top[k] = t;
                               });
    return *std::max_element(top.begin(), top.end());
}

// where the sequences end in their residue buffer (false: a slice wraps around)
bool extent_of(uint64_t const * off, uint64_t const * len, uint64_t n, uint64_t & extent, uint64_t & total)
{
    extent = total = 0;
    for (uint64_t i = 0; i < n; ++i)
    {
        if (off[i] > ~0ull - len[i] || total > ~0ull - len[i])
            return false;
        if (len[i])
            extent = std::max(extent, off[i] + len[i]);
        total += len[i];
    }
    return true;
}

enum DeviceBuild // which builder's limits take_subjects applies
{
    kNoDeviceBuild = 0, // h == NULL, or a load (no sort runs; upload_table has the resident table's limit)
    kSingleSort,
    kInSlices
};

// the index's own copy of the subjects, checked: what every later step relies on
int take_subjects(lx_handle * h, char const * who, uint8_t const * s_red, uint64_t const * s_off, uint64_t const * s_len, uint64_t n_sseq, int alph,
                  unsigned threads, DeviceBuild build, HostTable & t)
{
    if (n_sseq && (!s_off || !s_len))
        return say(h, LX_EINVAL, "%s: NULL sequence table", who);
    if (alph < 2 || alph > 26)
        return say(h, LX_EINVAL, "%s: alphabet size %d outside 2..26", who, alph);
    if (n_sseq > 0xffffffffull)
        return say(h, LX_EINVAL, "%s: %llu sequences (an entry names its sequence with 32 bits)", who, (unsigned long long)n_sseq);
    uint64_t extent = 0;
    if (!extent_of(s_off, s_len, n_sseq, extent, t.total))
        return say(h, LX_EINVAL, "%s: a sequence lies outside the address range", who);
    // (what the lengths alone say comes before the letters are read and copied)
    if (build == kSingleSort && (t.total > 0x7fffffffull || n_sseq >= 0xffffffffull))
        return fail(h, LX_EINVAL, "%s: %llu words in %llu sequences are beyond the device (fewer than 2^31 words, fewer than 2^32 - 1 sequences): build with h == NULL", who,
                    (unsigned long long)t.total, (unsigned long long)n_sseq);
    if (build == kInSlices && (t.total >= 0xffffffffull || n_sseq >= 0xffffffffull))
        return fail(h, LX_EINVAL,
                    "%s: %llu words in %llu sequences are beyond the device (a cursor on the device is a 32-bit range: fewer than 2^32 - 1 words, fewer than 2^32 - 1 "
                    "sequences): build with h == NULL",
                    who, (unsigned long long)t.total, (unsigned long long)n_sseq);
    for (uint64_t i = 0; i < n_sseq; ++i)
        if (s_len[i] >= 0xffffffffull)
            return say(h, LX_EINVAL, "%s: sequence %llu has %llu letters (an entry names its position with 32 bits)", who, (unsigned long long)i,
                       (unsigned long long)s_len[i]);
    if (extent && !s_red)
        return say(h, LX_EINVAL, "%s: NULL buffer", who);
    if (extent && top_letter(s_red, extent, threads) >= alph)
        return say(h, LX_EINVAL, "%s: a reduced letter is not below the alphabet size %d", who, alph);
    t.red.assign(s_red, s_red + extent);
    t.off.assign(s_off, s_off + n_sseq);
    t.len.assign(s_len, s_len + n_sseq);
    return LX_OK;
}

} // namespace

struct lx_index
{
    std::shared_ptr<HostTable> t;
    lx_handle *                h      = nullptr; // the handle the device copy belongs to (NULL: none)
    int                        device = -1;
    lxi::DevBlock<ReducedIndex::Entry> d_entries;
    lxi::DevBlock<uint64_t>            d_pre, d_soff, d_slen;
    lxi::DevBlock<uint8_t>             d_sred;
};

namespace
{

template <class T>
int dev_block(lx_handle * h, lxi::DevBlock<T> & b, size_t count)
{
    LXS_HIP(h, hipMalloc(reinterpret_cast<void **>(b.out()), std::max<size_t>(count * sizeof(T), 16)));
    return LX_OK;
}

// the subjects' reduced letters and sequence table on the handle's device (64 bytes of slack behind the letters)
int upload_subjects(lx_handle * h, lx_index & ix)
{
    HostTable const & t = *ix.t;
    int               rc;
    if ((rc = dev_block(h, ix.d_sred, t.red.size() + 64)) || (rc = dev_block(h, ix.d_soff, t.off.size())) || (rc = dev_block(h, ix.d_slen, t.len.size())))
        return rc;
    if (!t.red.empty())
        LXS_HIP(h, hipMemcpy(ix.d_sred, t.red.data(), t.red.size(), hipMemcpyHostToDevice));
    if (!t.off.empty())
    {
        LXS_HIP(h, hipMemcpy(ix.d_soff, t.off.data(), t.off.size() * 8, hipMemcpyHostToDevice));
        LXS_HIP(h, hipMemcpy(ix.d_slen, t.len.data(), t.len.size() * 8, hipMemcpyHostToDevice));
    }
    return LX_OK;
}

// a table that stands in host memory becomes resident
int upload_table(lx_handle * h, lx_index & ix)
{
    ReducedIndex const & r = ix.t->ix;
    int                  rc;
    if (r.entriesCount() >= 0xffffffffull)
        return fail(h, LX_EINVAL, "the table has %llu entries (a cursor on the device is a 32-bit range): seed with h == NULL", (unsigned long long)r.entriesCount());
    if ((rc = bind(h)) || (rc = upload_subjects(h, ix)) || (rc = dev_block(h, ix.d_entries, r.entriesCount())) || (rc = dev_block(h, ix.d_pre, r.prefixCount())))
        return rc;
    if (r.entriesCount())
        LXS_HIP(h, hipMemcpy(ix.d_entries, r.entriesData(), r.entriesCount() * sizeof(ReducedIndex::Entry), hipMemcpyHostToDevice));
    LXS_HIP(h, hipMemcpy(ix.d_pre, r.prefixData(), r.prefixCount() * 8, hipMemcpyHostToDevice));
    ix.h = h, ix.device = h->device;
    return LX_OK;
}

// The table made by kernels (lx_seed.hip) on the handle's stream: the keys of all positions, one radix sort of (key, sequence << 32 |
// position) pairs, the entries interleaved, the prefix table; entries and prefix table come down into the host table and stay on the
// device.  The limits are the sort's (it ranks with 32 bits) and the entry's.
int build_on_device(lx_handle * h, lx_index & ix, int alph)
{
    HostTable &    t     = *ix.t;
    uint64_t const total = t.total;
    size_t const   nSeq  = t.off.size();
    int rc = bind(h);
    if (rc)
        return rc;
    size_t freeB = 0, totalB = 0;
    LXS_HIP(h, hipMemGetInfo(&freeB, &totalB));
    if ((double)total * 72.0 + (double)t.red.size() + (64 << 20) > (double)freeB) // keys + values twice, entries, sort workspace
        return fail(h, LX_ENOMEM, "lx_index_build: the device has no room for a table of %llu words: build with h == NULL", (unsigned long long)total);
    t.ix.prepareExternal(t.red, t.off, t.len, alph);
    std::vector<uint64_t> first(nSeq + 1, 0);
    for (size_t s = 0; s < nSeq; ++s)
        first[s + 1] = first[s] + t.len[s];
    if ((rc = upload_subjects(h, ix)))
        return rc;
    lxi::DevBlock<uint64_t> dFirst, k0, k1, v0, v1;
    if ((rc = dev_block(h, dFirst, nSeq + 1)) || (rc = dev_block(h, k0, total)) || (rc = dev_block(h, k1, total)) || (rc = dev_block(h, v0, total)) ||
        (rc = dev_block(h, v1, total)) || (rc = dev_block(h, ix.d_entries, total)) || (rc = dev_block(h, ix.d_pre, t.ix.prefixCount())))
        return rc;
    LXS_HIP(h, hipMemcpy(dFirst, first.data(), (nSeq + 1) * 8, hipMemcpyHostToDevice));
    int const         keyLen = t.ix.keyLen(), preLen = t.ix.prefixLen();
    uint64_t const    nPre   = t.ix.prefixCount();
    hipStream_t const st     = h->stream;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    lxi::PhaseTimer pt(h, st, 8);
    LXS_HIP(h, lx::seed_launch_table_keys(ix.d_sred, ix.d_soff, ix.d_slen, dFirst, (uint64_t)nSeq, total, keyLen, (uint64_t)alph + 1, alph, k0, v0, st));
    int bits = 1;
    while (bits < 64 && (t.ix.power(keyLen) - 1) >> bits)
        ++bits;
    uint64_t * kk[2] = {k0, k1}, * vv[2] = {v0, v1};
    int        where = 0;
    if ((rc = lx_sort_words_dev(h->device, kk, vv, total, bits >= 64 ? ~0ull : ((1ull << bits) - 1), st, &where)) != LX_OK)
        return fail(h, rc, "lx_index_build: the sort of the word table failed");
    LXS_HIP(h, lx::seed_launch_table_entries(kk[where], vv[where], total, ix.d_entries, st));
    LXS_HIP(h, lx::seed_launch_table_prefix(kk[where], total, t.ix.power(keyLen - preLen), nPre, ix.d_pre, st));
    pt.close();
    LXS_HIP(h, hipStreamSynchronize(st));
    if (total)
        LXS_HIP(h, hipMemcpy(t.ix.entriesForFill(), ix.d_entries, total * sizeof(ReducedIndex::Entry), hipMemcpyDeviceToHost));
    LXS_HIP(h, hipMemcpy(t.ix.prefixForFill(), ix.d_pre, nPre * 8, hipMemcpyDeviceToHost));
    t.built_on_device = true;
    ix.h = h, ix.device = h->device;
    return LX_OK;
}

// The walk of lx_index_plan_slices (include/lambda_ext.h has the rule): begin(w) for every bucket that opens a slice but the first;
// the number of slices, or 0 for a prefix table that descends or a bucket beyond the sort.
template <class Begin>
uint64_t walk_slices(uint64_t const * pre, uint64_t n_prefix, uint64_t slice_words, Begin && begin)
{
    uint64_t n = 1, words = 0; // (words + c <= pre[w + 1]: no overflow)
    for (uint64_t w = 0; w + 1 < n_prefix; ++w)
    {
        if (pre[w + 1] < pre[w] || pre[w + 1] - pre[w] > 0x7fffffffull)
            return 0;
        uint64_t const c = pre[w + 1] - pre[w];
        if (words != 0 && words + c > slice_words)
        {
            begin(w);
            ++n, words = 0;
        }
        words += c;
    }
    return n > 1 && words == 0 ? n - 1 : n; // (empty buckets behind a full slice are that slice's)
}

// The table made slice by slice (lx_seed.hip), for sets beyond the single sort: the words counted by their first prefix_len letters,
// the counts' scan = the prefix table, which comes down and is cut (lx_index_plan_slices); per slice its positions' keys compacted in
// (sequence, position) order, the radix sort, the entries written where the prefix table says the slice begins, and brought down.
// On the device at once: the entries (16 bytes a word), keys and values twice for the largest slice (32 bytes a word of it), the
// prefix table, the blocks' counts (8 bytes per 256 words), the subjects, the sort's digit counts.
int build_in_slices(lx_handle * h, lx_index & ix, int alph, uint64_t slice_words)
{
    HostTable &    t     = *ix.t;
    uint64_t const total = t.total, n_max = std::min<uint64_t>(slice_words, 0x7fffffffull); // (a slice is one sort)
    size_t const   nSeq  = t.off.size();
    int            rc    = bind(h);
    if (rc)
        return rc;
    t.ix.prepareExternal(t.red, t.off, t.len, alph);
    int const      keyLen = t.ix.keyLen(), preLen = t.ix.prefixLen();
    uint64_t const nPre = t.ix.prefixCount(), blocks = lx::tab_blocks(total);
    uint64_t const tiles = std::max(lx::tab_scan_tiles(blocks), lx::tab_scan_tiles(nPre));
    auto const     no_room = [&](uint64_t largest) // what a build with slices of `largest` words still has to take from the device
    {
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess)
            return true;
        return (double)largest * 32.5 + (double)(64 << 20) > (double)freeB; // keys + values twice, the sort's digit counts
    };
    {
        size_t freeB = 0, totalB = 0;
        LXS_HIP(h, hipMemGetInfo(&freeB, &totalB));
        double const fixed = (double)total * 16.0 + (double)nPre * 8.0 + (double)(blocks + tiles) * 8.0 + (double)t.red.size() + (double)nSeq * 24.0;
        if (fixed + (double)std::min(total, n_max) * 32.5 + (double)(64 << 20) > (double)freeB)
            return fail(h, LX_ENOMEM, "lx_index_build: the device has no room for a table of %llu words in slices of %llu: build with h == NULL",
                        (unsigned long long)total, (unsigned long long)n_max);
    }
    std::vector<uint64_t> first(nSeq + 1, 0);
    for (size_t s = 0; s < nSeq; ++s)
        first[s + 1] = first[s] + t.len[s];
    if ((rc = upload_subjects(h, ix)))
        return rc;
    lxi::DevBlock<uint64_t> dFirst, dBlocks, dTiles, k0, k1, v0, v1;
    if ((rc = dev_block(h, dFirst, nSeq + 1)) || (rc = dev_block(h, ix.d_entries, total)) || (rc = dev_block(h, ix.d_pre, nPre)) || (rc = dev_block(h, dBlocks, blocks)) ||
        (rc = dev_block(h, dTiles, tiles)))
        return rc;
    LXS_HIP(h, hipMemcpy(dFirst, first.data(), (nSeq + 1) * 8, hipMemcpyHostToDevice));
    uint64_t const    base = (uint64_t)alph + 1;
    hipStream_t const st   = h->stream;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    // the counts and their scan: the prefix table itself (pre[w] = first entry whose word is >= w, pre[nPre - 1] = total)
    lxi::PhaseTimer pc(h, st, 8 + lxi::kPhaseTimeOnly);
    LXS_HIP(h, hipMemsetAsync(ix.d_pre, 0, nPre * 8, st));
    LXS_HIP(h, lx::seed_launch_table_counts(ix.d_sred, ix.d_soff, ix.d_slen, dFirst, (uint64_t)nSeq, total, preLen, base, alph, nPre, ix.d_pre, st));
    LXS_HIP(h, lx::seed_launch_scan64(ix.d_pre, nPre, dTiles, st));
    pc.close();
    LXS_HIP(h, hipStreamSynchronize(st));
    uint64_t * const pre = t.ix.prefixForFill();
    LXS_HIP(h, hipMemcpy(pre, ix.d_pre, nPre * 8, hipMemcpyDeviceToHost));
    if (pre[0] != 0 || pre[nPre - 1] != total)
        return fail(h, LX_EHIP, "lx_index_build: the word counts do not add up to the %llu words of the set", (unsigned long long)total);
    uint64_t n_slices = 0;
    if (lx_index_plan_slices(pre, nPre, n_max, nullptr, 0, &n_slices) != LX_OK)
        return fail(h, LX_EINVAL, "lx_index_build: one prefix of %d letters begins more than 2^31 - 1 words, which is beyond the device's sort: build with h == NULL", preLen);
    std::vector<uint64_t> cut(n_slices + 1, nPre - 1);
    (void)lx_index_plan_slices(pre, nPre, n_max, cut.data(), n_slices, &n_slices);
    uint64_t largest = 0;
    for (uint64_t s = 0; s < n_slices; ++s)
        largest = std::max(largest, pre[cut[s + 1]] - pre[cut[s]]);
    if (no_room(largest))
        return fail(h, LX_ENOMEM, "lx_index_build: the device has no room for a slice of %llu words of the table: build with h == NULL", (unsigned long long)largest);
    if ((rc = dev_block(h, k0, largest)) || (rc = dev_block(h, k1, largest)) || (rc = dev_block(h, v0, largest)) || (rc = dev_block(h, v1, largest)))
        return rc;
    int bits = 1;
    while (bits < 64 && (t.ix.power(keyLen) - 1) >> bits)
        ++bits;
    for (uint64_t s = 0; s < n_slices; ++s)
    {
        uint64_t const  at = pre[cut[s]], n = pre[cut[s + 1]] - at;
        lxi::PhaseTimer pt(h, st, 8);
        LXS_HIP(h, lx::seed_launch_table_slice_counts(ix.d_sred, ix.d_soff, ix.d_slen, dFirst, (uint64_t)nSeq, total, preLen, base, alph, cut[s], cut[s + 1], dBlocks, st));
        LXS_HIP(h, lx::seed_launch_scan64(dBlocks, blocks, dTiles, st));
        LXS_HIP(h, lx::seed_launch_table_slice_keys(ix.d_sred, ix.d_soff, ix.d_slen, dFirst, (uint64_t)nSeq, total, preLen, keyLen, base, alph, cut[s], cut[s + 1], dBlocks,
                                                    n, k0, v0, st));
        uint64_t * kk[2] = {k0, k1}, * vv[2] = {v0, v1};
        int        where = 0;
        if ((rc = lx_sort_words_dev(h->device, kk, vv, n, bits >= 64 ? ~0ull : ((1ull << bits) - 1), st, &where)) != LX_OK)
            return fail(h, rc, "lx_index_build: the sort of slice %llu of the word table failed", (unsigned long long)s);
        LXS_HIP(h, lx::seed_launch_table_entries(kk[where], vv[where], n, ix.d_entries.raw + at, st));
        pt.close();
        LXS_HIP(h, hipStreamSynchronize(st));
        if (n)
            LXS_HIP(h, hipMemcpy(t.ix.entriesForFill() + at, ix.d_entries.raw + at, n * sizeof(ReducedIndex::Entry), hipMemcpyDeviceToHost));
    }
    t.built_on_device = true;
    ix.h = h, ix.device = h->device;
    return LX_OK;
}

int finish_index(int rc, std::unique_ptr<lx_index> & ix, lx_index ** out)
{
    if (rc == LX_OK)
        *out = ix.release();
    else if (ix && ix->device >= 0)
        (void)hipSetDevice(ix->device);
    return rc;
}

} // namespace

int lx_index_build(lx_handle * h, uint8_t const * s_red, uint64_t const * s_off, uint64_t const * s_len, uint64_t n_sseq, int32_t alph, uint32_t host_threads,
                   lx_index ** out)
{
    if (!out)
        return say(h, LX_EINVAL, "lx_index_build: NULL out");
    *out = nullptr;
    if (!h)
        lxi::set_output_error("");
    try
    {
        unsigned const            threads = threads_or_share(host_threads);
        std::unique_ptr<lx_index> ix(new lx_index());
        ix->t  = std::make_shared<HostTable>();
        uint64_t const slice_words = h ? h->opt_index_slice : 0;
        int rc = take_subjects(h, "lx_index_build", s_red, s_off, s_len, n_sseq, alph, threads, !h ? kNoDeviceBuild : slice_words ? kInSlices : kSingleSort, *ix->t);
        if (rc)
            return rc;
        if (h && ix->t->total > 0)
        {
            ix->device = h->device; // (blocks that were taken before a failure go back on this device)
            return finish_index(slice_words ? build_in_slices(h, *ix, alph, slice_words) : build_on_device(h, *ix, alph), ix, out);
        }
        ix->t->ix.build(ix->t->red, ix->t->off, ix->t->len, alph, threads);
        if (h) // (nothing to sort: the empty table, resident)
        {
            ix->device = h->device;
            return finish_index(upload_table(h, *ix), ix, out);
        }
        *out = ix.release();
        return LX_OK;
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_index_build: out of host memory");
    }
}

int lx_index_plan_slices(uint64_t const * pre, uint64_t n_prefix, uint64_t slice_words, uint64_t * first_word, uint64_t cap, uint64_t * n_slices)
{
    if (n_slices)
        *n_slices = 0;
    if (!pre || !n_slices || (cap && !first_word) || slice_words == 0 || n_prefix < 2)
    {
        lxi::set_output_error("lx_index_plan_slices: NULL argument, slices of no words or a prefix table of fewer than two values");
        return LX_EINVAL;
    }
    uint64_t const n = walk_slices(pre, n_prefix, slice_words, [](uint64_t) {});
    if (n == 0)
    {
        lxi::set_output_error("lx_index_plan_slices: the prefix table does not ascend, or one of its buckets holds more than 2^31 - 1 words (beyond the sort: build with h == NULL)");
        return LX_EINVAL;
    }
    *n_slices = n;
    if (cap >= n)
    {
        uint64_t s    = 0;
        first_word[0] = 0;
        (void)walk_slices(pre, n_prefix, slice_words,
                          [&](uint64_t w)
                          {
                              if (++s < n)
                                  first_word[s] = w;
                          });
    }
    return LX_OK;
}

int lx_index_load(lx_handle * h, uint8_t const * bytes, uint64_t n, uint8_t const * s_red, uint64_t const * s_off, uint64_t const * s_len, uint64_t n_sseq,
                  lx_index ** out)
{
    if (!out)
        return say(h, LX_EINVAL, "lx_index_load: NULL out");
    *out = nullptr;
    if (!h)
        lxi::set_output_error("");
    if (!bytes || n < 32)
        return say(h, LX_EINVAL, bytes ? "lx_index_load: truncated (no header)" : "lx_index_load: NULL buffer");
    try
    {
        int32_t  geo[4];
        uint64_t cnt[2];
        std::memcpy(geo, bytes, sizeof(geo));
        std::memcpy(cnt, bytes + sizeof(geo), sizeof(cnt));
        // (what the header alone says comes before the letters are read and copied: the bytes its counts ask for)
        if (cnt[0] > (~0ull >> 5) || cnt[1] > (~0ull >> 5) || n != 32 + cnt[0] * sizeof(ReducedIndex::Entry) + cnt[1] * 8)
            return say(h, LX_EINVAL, "lx_index_load: the word table is truncated or has bytes left over (its header counts %llu entries and %llu prefixes)",
                       (unsigned long long)cnt[0], (unsigned long long)cnt[1]);
        std::unique_ptr<lx_index> ix(new lx_index());
        ix->t  = std::make_shared<HostTable>();
        int rc = take_subjects(h, "lx_index_load", s_red, s_off, s_len, n_sseq, geo[0], threads_or_share(0), kNoDeviceBuild, *ix->t);
        if (rc)
            return rc;
        uint64_t at   = 0;
        auto     read = [&](void * p, size_t want)
        {
            if (want > n - at)
                return false;
            if (want)
                std::memcpy(p, bytes + at, want);
            at += want;
            return true;
        };
        // (the counts are checked against the sequences before anything is allocated: load() compares them with the letters)
        if (!ix->t->ix.load(read, ix->t->red, ix->t->off, ix->t->len) || at != n)
            return say(h, LX_EINVAL, "lx_index_load: the word table is truncated, has bytes left over or does not fit the sequences");
        if (h)
        {
            ix->device = h->device;
            return finish_index(upload_table(h, *ix), ix, out);
        }
        *out = ix.release();
        return LX_OK;
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_index_load: out of host memory");
    }
}

int lx_index_save(lx_index const * ix, lx_bytes ** out)
{
    if (!ix || !out)
    {
        lxi::set_output_error("lx_index_save: NULL argument");
        return LX_EINVAL;
    }
    *out = nullptr;
    try
    {
        ReducedIndex const & r = ix->t->ix;
        std::string          s;
        s.reserve(32 + r.entriesCount() * sizeof(ReducedIndex::Entry) + r.prefixCount() * 8);
        r.save([&](void const * p, size_t bytes) { s.append(static_cast<char const *>(p), bytes); });
        *out = lxi::bytes_adopt(std::move(s));
        return LX_OK;
    }
    catch (std::bad_alloc const &)
    {
        lxi::set_output_error("lx_index_save: out of host memory");
        return LX_ENOMEM;
    }
}

int lx_index_attach(lx_index const * src, lx_handle * h, lx_index ** out)
{
    if (!src || !out)
        return say(h, LX_EINVAL, "lx_index_attach: NULL argument");
    *out = nullptr;
    try
    {
        std::unique_ptr<lx_index> ix(new lx_index());
        ix->t = src->t;
        if (h)
        {
            ix->device = h->device;
            return finish_index(upload_table(h, *ix), ix, out);
        }
        *out = ix.release();
        return LX_OK;
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_index_attach: out of host memory");
    }
}

int lx_index_get_info(lx_index const * ix, lx_index_info * out)
{
    if (!ix || !out)
        return LX_EINVAL;
    ReducedIndex const & r = ix->t->ix;
    *out = lx_index_info{r.entriesCount(), r.prefixCount(), r.alphabet(), r.keyLen(), r.prefixLen(), ix->t->built_on_device ? 1 : 0};
    return LX_OK;
}

int lx_index_copy_entries(lx_index const * ix, uint64_t first, uint64_t n, lx_index_entry * out)
{
    if (!ix || (n && !out) || !lxi::lx_slice_ok(first, n, ix->t->ix.entriesCount()))
        return LX_EINVAL;
    if (n)
        std::memcpy(out, ix->t->ix.entriesData() + first, n * sizeof(lx_index_entry));
    return LX_OK;
}

void lx_index_destroy(lx_index * ix)
{
    if (!ix)
        return;
    if (ix->device >= 0)
        (void)hipSetDevice(ix->device); // (the blocks go back on their device)
    delete ix;
}

// ---- search()

namespace
{

struct SeedCall // a checked call
{
    lx_seed_params const *   p;
    lambda_amd::SeedingInput in{};
    lambda_amd::SeedParams   so{};
    std::vector<uint64_t>    reads;
    uint64_t                 q_extent = 0;
    unsigned                 threads  = 1;
    lx_query_mask const *    mask     = nullptr; // (on the device: the kernel reads its resident bytes; the host copy is for declined reads)
};

int check_call(lx_handle * h, lx_index const * ix, uint8_t const * s_res, uint8_t const * q_res, uint8_t const * q_red, uint64_t const * q_off,
               uint64_t const * q_len, uint64_t n_qseq, uint64_t const * reads, uint64_t n_reads, lx_seed_params const * p, SeedCall & c)
{
    if (!ix || !p || !p->matrix || (n_qseq && (!q_off || !q_len)))
        return say(h, LX_EINVAL, "lx_seed_queries: NULL argument");
    if (h && ix->h != h)
        return say(h, LX_EINVAL, "lx_seed_queries: the index was not built, loaded or attached with this handle");
    if (!h && !s_res && !ix->t->red.empty())
        return say(h, LX_EINVAL, "lx_seed_queries: NULL subjects (without a handle there is no resident copy)");
    if (p->seed_length < 2 || p->seed_length > 63 || p->seed_offset < 1 || p->max_seed_dist < 0 || p->max_seed_dist > 5)
        return say(h, LX_EINVAL, "lx_seed_queries: seed length / offset / delta out of range");
    if (p->pre_scoring < 0 || p->q_num_frames < 1 || p->q_num_frames > 6 || p->unknown_rank < 0 || p->unknown_rank > 31)
        return say(h, LX_EINVAL, "lx_seed_queries: pre-scoring, frames per read or the unknown letter's rank out of range");
    uint64_t total = 0;
    if (!extent_of(q_off, q_len, n_qseq, c.q_extent, total))
        return say(h, LX_EINVAL, "lx_seed_queries: a query lies outside the address range");
    if (c.q_extent && (!q_res || !q_red))
        return say(h, LX_EINVAL, "lx_seed_queries: NULL query buffer");
    c.threads = threads_or_share(p->host_threads);
    if (c.q_extent && top_letter(q_red, c.q_extent, c.threads) >= ix->t->ix.alphabet())
        return say(h, LX_EINVAL, "lx_seed_queries: a reduced query letter is not below the index's alphabet size %d", ix->t->ix.alphabet());
    uint64_t const frames = (uint64_t)p->q_num_frames;
    if (reads)
    {
        for (uint64_t k = 0; k < n_reads; ++k)
            if (reads[k] >= n_qseq || reads[k] % frames != 0)
                return say(h, LX_EINVAL, "lx_seed_queries: reads[%llu] = %llu is not the first frame of a read of the set", (unsigned long long)k,
                           (unsigned long long)reads[k]);
        c.reads.assign(reads, reads + n_reads);
    }
    else
        for (uint64_t i = 0; i < n_qseq; i += frames)
            c.reads.push_back(i);
    c.p  = p;
    c.so = lambda_amd::SeedParams{p->seed_length, p->seed_offset, p->max_seed_dist};
    c.in.qRes = q_res, c.in.qRed = q_red, c.in.qOff = q_off, c.in.qLen = q_len, c.in.nQSeq = n_qseq, c.in.qNumFrames = p->q_num_frames;
    c.in.unknownRank = (uint8_t)p->unknown_rank;
    c.in.sRes = s_res, c.in.sOff = ix->t->off.data(), c.in.sLen = ix->t->len.data(), c.in.alph = ix->t->ix.alphabet();
    c.in.matrix = p->matrix, c.in.matrixRev = p->matrix_rev, c.in.maxMatches = p->max_matches;
    c.in.halfExact = p->half_exact != 0, c.in.adaptive = p->adaptive != 0, c.in.preScoring = p->pre_scoring, c.in.preScoringThresh = p->pre_scoring_thresh;
    return LX_OK;
}

// seedQueries for `reads` on the host threads, appended to `matches`
void seed_on_host(lx_index const * ix, SeedCall const & c, std::vector<uint64_t> const & reads, std::vector<lx_match> & matches, lx_seed_stats & st)
{
    std::vector<uint64_t> which;
    which.reserve(reads.size() * (size_t)c.in.qNumFrames);
    for (uint64_t rd : reads)
        for (int f = 0; f < c.in.qNumFrames && rd + (uint64_t)f < c.in.nQSeq; ++f)
            which.push_back(rd + (uint64_t)f);
    lambda_amd::SeedingStats sst{};
    lambda_amd::seedQueriesParallel(ix->t->ix, c.in, c.so, which, matches, sst, c.threads);
    st.hits_after_seeding += sst.hitsAfterSeeding;
    st.hits_failed_pre_extend += sst.hitsFailedPreExtendTest;
}

// room for `records` matches in the result's block; what it holds (kept records) moves along
int grow_out(lx_handle * h, lxi::DevBuf & out, uint64_t kept, uint64_t records)
{
    size_t const want = std::max<size_t>(records * sizeof(lx_match), 16);
    if (want <= out.cap)
        return LX_OK;
    lxi::DevBuf nb;
    LXS_HIP(h, hipMalloc(&nb.ptr, want));
    nb.cap = want;
    if (kept)
        LXS_HIP(h, hipMemcpy(nb.ptr, out.ptr, kept * sizeof(lx_match), hipMemcpyDeviceToDevice));
    LXS_HIP(h, hipDeviceSynchronize());
    out = std::move(nb); // (the old block goes with nb)
    return LX_OK;
}

int seed_on_device(lx_handle * h, lx_index const * ix, SeedCall & c, lx_seed_result & res)
{
    auto &            S  = h->seed;
    HostTable const & t  = *ix->t;
    hipStream_t const st = h->stream;
    int               rc = bind(h);
    if (rc)
        return rc;
    // the subjects in alignment ranks: the caller's for this call, or what lx_set_subjects left on the device
    uint8_t const * d_sres = nullptr;
    if (c.in.sRes)
    {
        if ((rc = ensure(h, S.d_sres, t.red.size() + 64)))
            return rc;
        if (!t.red.empty())
            LXS_HIP(h, hipMemcpy(S.d_sres.ptr, c.in.sRes, t.red.size(), hipMemcpyHostToDevice));
        d_sres = static_cast<uint8_t const *>(S.d_sres.ptr);
    }
    else
    {
        if (h->db_bytes < t.red.size())
            return fail(h, LX_EINVAL, "lx_seed_queries: NULL subjects and the handle's resident subjects (lx_set_subjects: %llu bytes) do not cover the index's (%llu)",
                        (unsigned long long)h->db_bytes, (unsigned long long)t.red.size());
        d_sres = static_cast<uint8_t const *>(h->d_db.ptr);
    }
    uint64_t const nQ = c.in.nQSeq, nReads = c.reads.size();
    if ((rc = ensure(h, S.d_qres, c.q_extent + 64)) || (rc = ensure(h, S.d_qred, c.q_extent + 64)) || (rc = ensure(h, S.d_qoff, nQ * 8 + 16)) ||
        (rc = ensure(h, S.d_qlen, nQ * 8 + 16)) || (rc = ensure(h, S.d_reads, nReads * 8 + 16)) || (rc = ensure(h, S.d_cnt, 4 * sizeof(unsigned long long))) ||
        (rc = ensure(h, S.d_matrix, 2 * LX_ALPH * LX_ALPH)) || (rc = ensure(h, S.d_declined, std::min<uint64_t>(nReads, lx::kLaunchReads) + 16)))
        return rc;
    if (c.q_extent)
    {
        LXS_HIP(h, hipMemcpy(S.d_qres.ptr, c.in.qRes, c.q_extent, hipMemcpyHostToDevice));
        LXS_HIP(h, hipMemcpy(S.d_qred.ptr, c.in.qRed, c.q_extent, hipMemcpyHostToDevice));
    }
    if (nQ)
    {
        LXS_HIP(h, hipMemcpy(S.d_qoff.ptr, c.in.qOff, nQ * 8, hipMemcpyHostToDevice));
        LXS_HIP(h, hipMemcpy(S.d_qlen.ptr, c.in.qLen, nQ * 8, hipMemcpyHostToDevice));
    }
    if (nReads)
        LXS_HIP(h, hipMemcpy(S.d_reads.ptr, c.reads.data(), nReads * 8, hipMemcpyHostToDevice));
    int8_t * const d_matrix = static_cast<int8_t *>(S.d_matrix.ptr);
    LXS_HIP(h, hipMemcpy(d_matrix, c.in.matrix, LX_ALPH * LX_ALPH, hipMemcpyHostToDevice));
    if (c.in.matrixRev)
        LXS_HIP(h, hipMemcpy(d_matrix + LX_ALPH * LX_ALPH, c.in.matrixRev, LX_ALPH * LX_ALPH, hipMemcpyHostToDevice));

    lx::SeedDev d{};
    d.entries = ix->d_entries, d.pre = ix->d_pre, d.base = (uint64_t)t.ix.alphabet() + 1, d.preLen = t.ix.prefixLen(), d.keyLen = t.ix.keyLen(), d.alph = t.ix.alphabet();
    for (int k = 0; k <= t.ix.keyLen() && k < 64; ++k)
        d.pow[k] = t.ix.power(k);
    d.sRes = d_sres, d.sRed = ix->d_sred, d.sOff = ix->d_soff, d.sLen = ix->d_slen;
    d.qRes = static_cast<uint8_t const *>(S.d_qres.ptr), d.qRed = static_cast<uint8_t const *>(S.d_qred.ptr);
    d.qOff = static_cast<uint64_t const *>(S.d_qoff.ptr), d.qLen = static_cast<uint64_t const *>(S.d_qlen.ptr), d.nQSeq = nQ, d.qNumFrames = c.in.qNumFrames;
    d.unknownRank = c.in.unknownRank, d.matrix = d_matrix, d.matrixRev = c.in.matrixRev ? d_matrix + LX_ALPH * LX_ALPH : nullptr;
    d.maxMatches = c.in.maxMatches, d.halfExact = c.in.halfExact ? 1 : 0, d.adaptive = c.in.adaptive ? 1 : 0, d.preScoring = c.in.preScoring;
    d.preScoringThresh = c.in.preScoringThresh;
    d.seedLength = c.so.seedLength, d.seedOffset = c.so.seedOffset, d.maxSeedDist = c.so.maxSeedDist;
    d.counters = static_cast<unsigned long long *>(S.d_cnt.ptr), d.declined = static_cast<uint8_t *>(S.d_declined.ptr);
    d.qMask = c.mask ? c.mask->d_dist.raw : nullptr;

    // (development aids of the front end's tests: several launches on a small input; a small buffer exercises "buffer full")
    uint64_t launchReads = lx::kLaunchReads, forcedCap = 0;
    if (char const * forced = std::getenv("LAMBDA3_SEED_LAUNCH"))
        launchReads = std::min<uint64_t>(lx::kLaunchReads, std::max<uint64_t>(1, std::strtoull(forced, nullptr, 10)));
    if (char const * forced = std::getenv("LAMBDA3_SEED_CAP"))
        forcedCap = std::max<uint64_t>(1, std::strtoull(forced, nullptr, 10));
    lxi::DevBuf & out = res.d_out;
    out               = std::move(S.d_spare); // the block of the last freed result
    uint64_t              kept = 0;           // records of the list so far
    std::vector<uint64_t> declined;           // reads the host finishes
    std::vector<uint8_t>  decl;
    std::vector<lx_match> down;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    for (uint64_t a = 0; a < nReads; a += launchReads)
    {
        uint64_t const nr = std::min<uint64_t>(launchReads, nReads - a);
        // room for 64 matches per read of the launch, as far as the device's free memory allows: no more than half of what it has left
        // (a launch whose buffer fills up is the host's, which is slow but right; a failed allocation would end the search)
        uint64_t cap = forcedCap ? forcedCap : std::max<uint64_t>(1u << 20, 64ull * nr);
        if ((kept + cap) * sizeof(lx_match) > out.cap)
        {
            size_t freeB = 0, totalB = 0;
            LXS_HIP(h, hipMemGetInfo(&freeB, &totalB));
            uint64_t const most = (freeB + out.cap) / 2 / sizeof(lx_match);
            uint64_t const to   = std::max<uint64_t>(out.cap / sizeof(lx_match), std::min<uint64_t>(kept + cap, most));
            if ((rc = grow_out(h, out, kept, to)))
                return rc;
            cap = std::min<uint64_t>(cap, out.cap / sizeof(lx_match) - kept);
        }
        unsigned long long cnt[4] = {0, 0, 0, 1};
        if (cap > 0)
        {
            LXS_HIP(h, hipMemsetAsync(S.d_declined.ptr, 0, nr, st));
            LXS_HIP(h, hipMemsetAsync(S.d_cnt.ptr, 0, sizeof(cnt), st));
            lx::SeedDev p = d;
            p.reads = static_cast<uint64_t const *>(S.d_reads.ptr) + a, p.nReads = nr;
            p.out = static_cast<lx_match *>(out.ptr) + kept, p.outCap = cap;
            lxi::PhaseTimer pt(h, st, 9);
            LXS_HIP(h, lx::seed_launch_reads(p, st));
            pt.close();
            LXS_HIP(h, hipStreamSynchronize(st));
            LXS_HIP(h, hipMemcpy(cnt, S.d_cnt.ptr, sizeof(cnt), hipMemcpyDeviceToHost));
        }
        if (cnt[3] != 0)
        {
            // the buffer filled up: nothing of this launch is kept, its reads are the host's
            declined.insert(declined.end(), c.reads.begin() + (std::ptrdiff_t)a, c.reads.begin() + (std::ptrdiff_t)(a + nr));
            ++res.st.launches_full;
            continue;
        }
        decl.resize(nr);
        LXS_HIP(h, hipMemcpy(decl.data(), S.d_declined.ptr, nr, hipMemcpyDeviceToHost));
        std::vector<uint64_t> mine;
        for (uint64_t k = 0; k < nr; ++k)
            if (decl[k])
                mine.push_back(c.reads[a + k]);
        uint64_t got = cnt[0];
        if (!mine.empty() && got)
        {
            // a declined read's matches are the host's to make: what its lane wrote before it gave up is dropped (it counted nothing)
            std::sort(mine.begin(), mine.end());
            down.resize(got);
            lx_match * const at = static_cast<lx_match *>(out.ptr) + kept;
            LXS_HIP(h, hipMemcpy(down.data(), at, got * sizeof(lx_match), hipMemcpyDeviceToHost));
            uint64_t o = 0;
            for (uint64_t k = 0; k < got; ++k)
                if (!std::binary_search(mine.begin(), mine.end(), down[k].qryId - down[k].qryId % (uint64_t)c.in.qNumFrames))
                    down[o++] = down[k];
            if (o != got && o)
                LXS_HIP(h, hipMemcpy(at, down.data(), o * sizeof(lx_match), hipMemcpyHostToDevice));
            got = o;
        }
        declined.insert(declined.end(), mine.begin(), mine.end());
        kept += got;
        res.st.hits_after_seeding += cnt[1];
        res.st.hits_failed_pre_extend += cnt[2];
    }
    if (!declined.empty())
    {
        // the host threads finish them inside the call; their matches are appended to the device list
        std::vector<uint8_t> s_down;
        if (!c.in.sRes)
        {
            s_down.resize(t.red.size());
            if (!s_down.empty())
                LXS_HIP(h, hipMemcpy(s_down.data(), d_sres, s_down.size(), hipMemcpyDeviceToHost));
            c.in.sRes = s_down.data();
        }
        if (c.mask && !(c.in.qMaskDist = c.mask->host_dist()))
            return fail(h, LX_EHIP, "lx_seed_queries_masked: the mask did not come down from the device");
        std::sort(declined.begin(), declined.end());
        std::vector<lx_match> more;
        seed_on_host(ix, c, declined, more, res.st);
        if ((rc = grow_out(h, out, kept, kept + more.size())))
            return rc;
        if (!more.empty())
            LXS_HIP(h, hipMemcpy(static_cast<lx_match *>(out.ptr) + kept, more.data(), more.size() * sizeof(lx_match), hipMemcpyHostToDevice));
        kept += more.size();
        res.st.reads_declined = declined.size();
    }
    if (!out.ptr && (rc = grow_out(h, out, 0, 1))) // (an empty list still has an address)
        return rc;
    res.st.n_matches = kept;
    res.h            = h;
    return LX_OK;
}

} // namespace

int lx_seed_queries(lx_handle * h, lx_index const * ix, uint8_t const * s_res, uint8_t const * q_res, uint8_t const * q_red, uint64_t const * q_off,
                    uint64_t const * q_len, uint64_t n_qseq, uint64_t const * reads, uint64_t n_reads, lx_seed_params const * p, lx_seed_result ** out)
{
    return lx_seed_queries_masked(h, ix, s_res, q_res, q_red, q_off, q_len, n_qseq, reads, n_reads, nullptr, p, out);
}

int lx_seed_queries_masked(lx_handle * h, lx_index const * ix, uint8_t const * s_res, uint8_t const * q_res, uint8_t const * q_red, uint64_t const * q_off,
                           uint64_t const * q_len, uint64_t n_qseq, uint64_t const * reads, uint64_t n_reads, lx_query_mask const * m, lx_seed_params const * p,
                           lx_seed_result ** out)
{
    if (!out)
        return say(h, LX_EINVAL, "lx_seed_queries: NULL out");
    *out = nullptr;
    if (!h)
        lxi::set_output_error("");
    try
    {
        SeedCall c;
        int      rc = check_call(h, ix, s_res, q_res, q_red, q_off, q_len, n_qseq, reads, n_reads, p, c);
        if (rc)
            return rc;
        if (m)
        {
            if (m->off.size() != n_qseq || !std::equal(m->off.begin(), m->off.end(), q_off) || !std::equal(m->len.begin(), m->len.end(), q_len))
                return say(h, LX_EINVAL, "lx_seed_queries_masked: the mask was made for another sequence table (%llu sequences; the call has %llu)",
                           (unsigned long long)m->off.size(), (unsigned long long)n_qseq);
            if (h && !m->h)
                return say(h, LX_EINVAL, "lx_seed_queries_masked: seeding on the device needs a mask made with its handle (this one is on the host only)");
            if (h && m->h != h)
                return say(h, LX_EINVAL, "lx_seed_queries_masked: the mask was made on another handle");
            c.mask = m;
            if (!h && !(c.in.qMaskDist = m->host_dist()))
                return say(h, LX_EHIP, "lx_seed_queries_masked: the mask did not come down from its device");
        }
        std::unique_ptr<lx_seed_result> res(new lx_seed_result());
        if (h)
        {
            rc = seed_on_device(h, ix, c, *res);
            if (rc)
            {
                // (what the failed call held goes back on the handle's device; a block taken from the handle returns to it)
                (void)hipSetDevice(h->device);
                if (res->d_out.cap > h->seed.d_spare.cap)
                    std::swap(res->d_out, h->seed.d_spare);
                return rc;
            }
        }
        else
        {
            seed_on_host(ix, c, c.reads, res->host, res->st);
            res->st.n_matches = res->host.size();
            res->have_host    = true;
        }
        *out = res.release();
        return LX_OK;
    }
    catch (std::bad_alloc const &)
    {
        if (h)
            (void)hipSetDevice(h->device);
        return say(h, LX_ENOMEM, "lx_seed_queries: out of host memory");
    }
}

lx_seed_stats lx_seed_result_stats(lx_seed_result const * r)
{
    return r ? r->st : lx_seed_stats{};
}

lx_match * lx_seed_result_matches(lx_seed_result * r)
{
    if (!r)
        return nullptr;
    if (!r->have_host)
    {
        try
        {
            r->host.resize(r->st.n_matches);
        }
        catch (std::bad_alloc const &)
        {
            return nullptr;
        }
        if (hipSetDevice(r->h->device) != hipSuccess ||
            (r->st.n_matches && hipMemcpy(r->host.data(), r->d_out.ptr, r->st.n_matches * sizeof(lx_match), hipMemcpyDeviceToHost) != hipSuccess))
            return nullptr;
        r->have_host = true;
    }
    static lx_match none{};
    return r->host.empty() ? &none : r->host.data();
}

void const * lx_seed_result_matches_dev(lx_seed_result const * r)
{
    return r && r->h ? r->d_out.ptr : nullptr;
}

void lx_seed_result_free(lx_seed_result * r)
{
    if (!r)
        return;
    if (r->h)
    {
        (void)hipSetDevice(r->h->device);
        if (r->d_out.cap > r->h->seed.d_spare.cap) // the larger block stays with the handle, the other goes back with the result
            std::swap(r->d_out, r->h->seed.d_spare);
    }
    delete r;
}
