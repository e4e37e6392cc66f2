// lx_taxmap_host.cpp -- lx_find_accessions and lx_taxmap_*: the accession table of a database's ids and its join with an
// accession-to-taxon map (src/mkindex_algo.hpp:68-107, :277-352, src/mkindex_misc.hpp:69-144).
//
// The table is built here from the subject ids (two passes: count the accessions, then insert them into an open-addressing table of
// twice that many slots; a later subject overwrites an earlier one's accession, as accToIdRank[acc] = rank does).  The map arrives
// in pieces of any size; they are gathered into chunks of whole lines (a piece's unfinished last line is carried into the next
// chunk), and each chunk is joined either
//   * on the device (a handle was given): the table is uploaded once; the chunk goes up from one of two pinned lanes while the host
//     fills the other, the kernels of lx_taxmap.hip leave the chunk's (subject, taxon) pairs in line order and three counters, and
//     the pairs come down on a second stream once the chunk's event has passed; or
//   * on the library's host threads: the chunk is cut at line starts into parts, each part parsed with the same lx_taxmap.h code.
// Either way the chunks are taken in file order, so the pairs are in file order and the first bad line of the file is the first
// one reported.  lx_taxmap_finish turns the pairs into per-subject lists with a stable counting sort.
#include "lx_host_pool.h"
#include "lx_internal.h"
#include "lx_taxmap.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace lxi;
using lx::taxmap::Key;
using lx::taxmap::Pair;

namespace
{

constexpr uint64_t kDefaultChunk = 256ull << 20;
constexpr uint64_t kMaxChunk     = 1ull << 30; // (offsets in a chunk are 32-bit on the device)
constexpr char     kNcbiHeader[] = "accession\taccession.version\ttaxid\tgi";

struct PendingHost // a chunk joined on the host threads, waiting to be taken in order
{
    std::vector<Pair> pairs;
    uint64_t          lines   = 0;
    uint64_t          bad_off = ~0ull;
};

} // namespace

struct lx_taxmap
{
    lx_handle * h       = nullptr;
    int         format  = 0;
    uint32_t    threads = 0;
    uint64_t    chunk   = kDefaultChunk;
    uint64_t    n_s     = 0;
    // the table
    std::vector<uint64_t> slots;
    std::vector<Key>      keys;
    std::vector<uint8_t>  kbytes;
    uint32_t              max_len = 0;
    uint64_t              no_acc = 0, multi_acc = 0;
    lx::taxmap::TableView host_view{};
    lx::taxmap::TableView dev_view{};
    // the device's buffers (a handle was given)
    DevBlock<uint64_t> d_slots;
    DevBlock<Key>      d_keys;
    DevBlock<uint8_t>  d_bytes, d_text[2];
    DevBlock<Pair>     d_scratch, d_pairs[2];
    DevBlock<uint32_t> d_tile_cnt, d_tile_off, d_block_tot;
    DevBlock<lx::taxmap::JoinCounters>    d_counters;
    Stream                                down;
    Event                                 ev[2];
    PinnedBlock<lx::taxmap::JoinCounters> p_cnt;   // [lane]
    PinnedBlock<uint32_t>                 p_total; // [lane]
    // the staging lanes: pinned with a handle, malloc'ed without one, so given back by hand (the destructor)
    uint8_t * lane[2] = {nullptr, nullptr};
    uint64_t  fill    = 0;
    int       cur     = 0;
    struct Flight
    {
        bool     on = false;
        int      lane = 0;
        uint64_t len  = 0;
    } flight;
    PendingHost pending;
    // the header (NCBI), the running line count, the pairs so far
    bool              header_done = false;
    std::string       header;
    uint64_t          lines = 0;
    std::vector<Pair> pairs;
    // state
    int         err = LX_OK;
    std::string err_text;
    bool        finished = false;
    std::vector<uint64_t> off;
    std::vector<uint32_t> ids, present;
    lx_taxmap_result      res{};

    // with a handle: its device bound and the streams through before the lanes and then the members go
    ~lx_taxmap()
    {
        if (h)
        {
            (void)bind(h);
            (void)hipStreamSynchronize(h->stream);
            if (down)
                (void)hipStreamSynchronize(down);
        }
        for (uint8_t * l : lane)
            if (l && h)
                (void)hipHostFree(l);
            else
                std::free(l);
    }
};

namespace
{

int report(lx_handle * h, int code, std::string const & msg)
{
    if (h)
        return fail(h, code, "%s", msg.c_str());
    set_output_error(msg);
    return code;
}

int tm_fail(lx_taxmap * tm, int code, std::string const & msg)
{
    tm->err      = code;
    tm->err_text = msg;
    return report(tm->h, code, msg);
}

#define TM_HIP(tm, call)                                                                                                        \
    do                                                                                                                          \
    {                                                                                                                           \
        hipError_t _e = (call);                                                                                                 \
        if (_e != hipSuccess)                                                                                                   \
            return tm_fail((tm), _e == hipErrorOutOfMemory ? LX_ENOMEM : LX_EHIP,                                                \
                           std::string("lx_taxmap: ") + #call + " failed: " + hipGetErrorString(_e));                           \
    } while (0)

// the error of a matched line whose taxon does not parse: the line at byte `at` of a chunk whose first line is line `first`
int bad_taxon(lx_taxmap * tm, uint8_t const * text, uint64_t at, uint64_t first)
{
    uint64_t const line = first + (uint64_t)std::count(text, text + at, '\n');
    auto           get  = [&](uint64_t q) { return text[q]; };
    uint32_t       subj = 0, tax = 0;
    uint64_t       ta = 0, tl = 0;
    (void)lx::taxmap::parse_line(tm->host_view, tm->format, get, at, &subj, &tax, &ta, &tl);
    std::string const field(reinterpret_cast<char const *>(text + ta), (size_t)std::min<uint64_t>(tl, 200));
    return tm_fail(tm, LX_EINVAL, "lx_taxmap: line " + std::to_string(line) +
                                      ": Error: Expected taxonomical ID, but got something I couldn't read: " + field);
}

// the host threads' join of text[0, n) (whole lines)
void host_join(lx_taxmap * tm, uint8_t const * text, uint64_t n, PendingHost & out)
{
    unsigned const parts = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(
                               tm->threads ? tm->threads : HostPool::instance().width(), std::max<uint64_t>(1, n / 4096)));
    std::vector<uint64_t> start(parts + 1, n);
    start[0] = 0;
    for (unsigned k = 1; k < parts; ++k)
    {
        uint64_t c = std::max(start[k - 1], n * k / parts);
        if (c > 0)
        {
            void const * nl = c - 1 < n ? std::memchr(text + c - 1, '\n', n - (c - 1)) : nullptr;
            c               = nl ? (uint64_t)(static_cast<uint8_t const *>(nl) - text) + 1 : n;
        }
        start[k] = c;
    }
    std::vector<PendingHost> part(parts);
    auto const               get = [text](uint64_t q) { return text[q]; };
    HostPool::instance().run(parts,
                             [&](unsigned k)
                             {
                                 PendingHost & o = part[k];
                                 for (uint64_t p = start[k]; p < start[k + 1];)
                                 {
                                     ++o.lines;
                                     uint32_t subj = 0, tax = 0;
                                     uint64_t ta = 0, tl = 0;
                                     int const r = lx::taxmap::parse_line(tm->host_view, tm->format, get, p, &subj, &tax, &ta, &tl);
                                     if (r == lx::taxmap::kLinePair)
                                         o.pairs.push_back(Pair{subj, tax});
                                     else if (r == lx::taxmap::kLineBadTax && o.bad_off == ~0ull)
                                         o.bad_off = p;
                                     p = (uint64_t)(static_cast<uint8_t const *>(std::memchr(text + p, '\n', n - p)) - text) + 1;
                                 }
                             });
    out = PendingHost{};
    for (PendingHost & o : part)
    {
        out.lines += o.lines;
        if (out.bad_off == ~0ull)
            out.bad_off = o.bad_off;
        out.pairs.insert(out.pairs.end(), o.pairs.begin(), o.pairs.end());
    }
}

// chunk lane[L][0, len) on its way: up, the kernels, the counters down (device); joined now (host)
int dispatch(lx_taxmap * tm, int L, uint64_t len)
{
    if (!tm->h)
    {
        host_join(tm, tm->lane[L], len, tm->pending);
        return LX_OK;
    }
    lx_handle * const h = tm->h;
    hipStream_t const s = h->stream;
    TM_HIP(tm, hipMemsetAsync(tm->d_counters, 0, sizeof(lx::taxmap::JoinCounters), s));
    TM_HIP(tm, hipMemsetAsync(reinterpret_cast<uint8_t *>(tm->d_counters.raw) + offsetof(lx::taxmap::JoinCounters, bad_off), 0xff, 4, s));
    TM_HIP(tm, hipMemcpyAsync(tm->d_text[L], tm->lane[L], len, hipMemcpyHostToDevice, s));
    lx::taxmap::JoinParams p{};
    p.table     = tm->dev_view;
    p.format    = tm->format;
    p.text      = tm->d_text[L];
    p.n         = (uint32_t)len;
    p.scratch   = tm->d_scratch;
    p.tile_cnt  = tm->d_tile_cnt;
    p.tile_off  = tm->d_tile_off;
    p.block_tot = tm->d_block_tot;
    p.pairs     = tm->d_pairs[L];
    p.counters  = tm->d_counters;
    PhaseTimer t(h, s, 6);
    TM_HIP(tm, lx::taxmap::launch_taxmap_join(p, s));
    t.close();
    TM_HIP(tm, hipMemcpyAsync(&tm->p_cnt[L], tm->d_counters, sizeof(lx::taxmap::JoinCounters), hipMemcpyDeviceToHost, s));
    uint64_t const sb = lx::taxmap::join_scan_blocks(lx::taxmap::join_tiles(len));
    TM_HIP(tm, hipMemcpyAsync(&tm->p_total[L], tm->d_block_tot + sb, 4, hipMemcpyDeviceToHost, s));
    TM_HIP(tm, hipEventRecord(tm->ev[L], s));
    return LX_OK;
}

// the chunk in flight, taken in order: its pairs appended, its lines counted, its first bad line reported
int collect(lx_taxmap * tm)
{
    if (!tm->flight.on)
        return LX_OK;
    tm->flight.on        = false;
    int const      L     = tm->flight.lane;
    uint64_t const first = tm->lines + 1;
    uint64_t       lines = 0, bad = ~0ull;
    if (!tm->h)
    {
        lines = tm->pending.lines;
        bad   = tm->pending.bad_off;
        tm->pairs.insert(tm->pairs.end(), tm->pending.pairs.begin(), tm->pending.pairs.end());
        tm->pending = PendingHost{};
    }
    else
    {
        TM_HIP(tm, hipEventSynchronize(tm->ev[L]));
        lx::taxmap::JoinCounters const c = tm->p_cnt[L];
        if (c.overflow)
            return tm_fail(tm, LX_EINVAL, "lx_taxmap: a tile of the join made more pairs than it has room for");
        lines = c.lines;
        bad   = c.bad_off == ~0u ? ~0ull : c.bad_off;
        if (bad == ~0ull && tm->p_total[L])
        {
            uint64_t const at = tm->pairs.size(), k = tm->p_total[L];
            tm->pairs.resize(at + k);
            TM_HIP(tm, hipMemcpyAsync(tm->pairs.data() + at, tm->d_pairs[L], k * sizeof(Pair), hipMemcpyDeviceToHost, tm->down));
            TM_HIP(tm, hipStreamSynchronize(tm->down));
        }
    }
    if (bad != ~0ull)
        return bad_taxon(tm, tm->lane[L], bad, first);
    tm->lines += lines;
    return LX_OK;
}

// the current lane up to its last '\n' goes out; what follows it moves to the other lane
int cut_and_dispatch(lx_taxmap * tm)
{
    int const       L   = tm->cur;
    uint8_t * const buf = tm->lane[L];
    uint64_t        pos = tm->fill;
    while (pos > 0 && buf[pos - 1] != '\n')
        --pos;
    if (pos == 0)
    {
        int const rc = collect(tm);
        if (rc)
            return rc;
        return tm_fail(tm, LX_EINVAL, "lx_taxmap: line " + std::to_string(tm->lines + 1) + " is longer than the chunk size (" +
                                          std::to_string(tm->chunk) + " bytes)");
    }
    int rc = dispatch(tm, L, pos);
    if (rc)
        return rc;
    if ((rc = collect(tm))) // (the chunk before this one: its lane is free after)
        return rc;
    tm->flight = lx_taxmap::Flight{true, L, pos};
    if (!tm->h && (rc = collect(tm)))
        return rc;
    uint64_t const rem = tm->fill - pos;
    std::memcpy(tm->lane[1 - L], buf + pos, rem); // (the device reads lane L meanwhile: reads only)
    tm->fill = rem;
    tm->cur  = 1 - L;
    return LX_OK;
}

int check_header(lx_taxmap * tm)
{
    tm->header_done = true;
    tm->lines       = 1;
    if (tm->header != kNcbiHeader)
        return tm_fail(tm, LX_EINVAL, "lx_taxmap: line 1: Unexpected first line in NCBI taxid file.");
    return LX_OK;
}

int build_table(lx_taxmap * tm, uint8_t const * ids, uint64_t const * id_off)
{
    uint64_t total = 0;
    for (uint64_t s = 0; s < tm->n_s; ++s)
    {
        uint8_t const * id  = ids + id_off[s];
        uint64_t const  len = id_off[s + 1] - id_off[s];
        uint32_t        l   = 0;
        for (uint64_t p = lx::taxmap::find_accession(id, len, 0, &l); p < len; p = lx::taxmap::find_accession(id, len, p + l, &l))
            ++total;
    }
    if (total >= 0x7fffffffull)
        return tm_fail(tm, LX_EINVAL, "lx_taxmap_create: too many accessions");
    uint64_t cap = 16;
    while (cap < 2 * total)
        cap <<= 1;
    tm->slots.assign(cap, lx::taxmap::kEmptySlot);
    tm->keys.reserve(total);
    uint64_t const mask = cap - 1;
    for (uint64_t s = 0; s < tm->n_s; ++s)
    {
        uint8_t const * id  = ids + id_off[s];
        uint64_t const  len = id_off[s + 1] - id_off[s];
        uint32_t        l = 0, count = 0;
        for (uint64_t p = lx::taxmap::find_accession(id, len, 0, &l); p < len; p = lx::taxmap::find_accession(id, len, p + l, &l), ++count)
        {
            uint64_t const h  = lx::taxmap::hash_bytes(id + p, l);
            uint32_t const fp = (uint32_t)(h >> 32);
            for (uint64_t at = h & mask;; at = (at + 1) & mask)
            {
                uint64_t & sl = tm->slots[at];
                if (sl == lx::taxmap::kEmptySlot)
                {
                    sl = (uint64_t)fp << 32 | tm->keys.size();
                    tm->keys.push_back(Key{tm->kbytes.size(), l, (uint32_t)s});
                    tm->kbytes.insert(tm->kbytes.end(), id + p, id + p + l);
                    tm->max_len = std::max(tm->max_len, l);
                    break;
                }
                Key & k = tm->keys[(uint32_t)sl];
                if ((uint32_t)(sl >> 32) == fp && k.len == l && std::memcmp(tm->kbytes.data() + k.off, id + p, l) == 0)
                {
                    k.subject = (uint32_t)s; // the later subject wins (accToIdRank[acc] = rank)
                    break;
                }
            }
        }
        tm->no_acc += count == 0;
        tm->multi_acc += count > 1;
    }
    if (tm->kbytes.empty())
        tm->kbytes.push_back(0);
    if (tm->keys.empty())
        tm->keys.push_back(Key{0, 0, 0}); // (never reached: every slot is empty)
    tm->host_view = lx::taxmap::TableView{tm->slots.data(), mask, tm->keys.data(), tm->kbytes.data(), tm->max_len};
    return LX_OK;
}

int setup_device(lx_taxmap * tm)
{
    lx_handle * const h  = tm->h;
    int               rc = bind(h);
    if (rc)
        return rc;
    h->phase_ev.clear();
    h->ev_pool_used = 0;
    uint64_t const tiles = lx::taxmap::join_tiles(tm->chunk), sb = lx::taxmap::join_scan_blocks(tiles);
    size_t const   pair_bytes = (size_t)tiles * lx::taxmap::kJoinTileCap * sizeof(Pair);
    TM_HIP(tm, hipMalloc(tm->d_slots.out(), tm->slots.size() * 8));
    TM_HIP(tm, hipMalloc(tm->d_keys.out(), tm->keys.size() * sizeof(Key)));
    TM_HIP(tm, hipMalloc(tm->d_bytes.out(), tm->kbytes.size()));
    TM_HIP(tm, hipMalloc(tm->d_scratch.out(), pair_bytes));
    TM_HIP(tm, hipMalloc(tm->d_tile_cnt.out(), tiles * 4));
    TM_HIP(tm, hipMalloc(tm->d_tile_off.out(), tiles * 4));
    TM_HIP(tm, hipMalloc(tm->d_block_tot.out(), (sb + 1) * 4));
    TM_HIP(tm, hipMalloc(tm->d_counters.out(), sizeof(lx::taxmap::JoinCounters)));
    for (int l = 0; l < 2; ++l)
    {
        TM_HIP(tm, hipMalloc(tm->d_text[l].out(), tm->chunk + 16));
        TM_HIP(tm, hipMalloc(tm->d_pairs[l].out(), pair_bytes));
        TM_HIP(tm, hipHostMalloc(reinterpret_cast<void **>(&tm->lane[l]), tm->chunk + 16, hipHostMallocDefault));
        TM_HIP(tm, hipEventCreateWithFlags(tm->ev[l].out(), hipEventDisableTiming));
    }
    TM_HIP(tm, hipHostMalloc(tm->p_cnt.out(), 2 * sizeof(lx::taxmap::JoinCounters), hipHostMallocDefault));
    TM_HIP(tm, hipHostMalloc(tm->p_total.out(), 2 * 4, hipHostMallocDefault));
    TM_HIP(tm, hipStreamCreateWithFlags(tm->down.out(), hipStreamNonBlocking));
    TM_HIP(tm, hipMemcpy(tm->d_slots, tm->slots.data(), tm->slots.size() * 8, hipMemcpyHostToDevice));
    TM_HIP(tm, hipMemcpy(tm->d_keys, tm->keys.data(), tm->keys.size() * sizeof(Key), hipMemcpyHostToDevice));
    TM_HIP(tm, hipMemcpy(tm->d_bytes, tm->kbytes.data(), tm->kbytes.size(), hipMemcpyHostToDevice));
    tm->dev_view = lx::taxmap::TableView{tm->d_slots, tm->host_view.mask, tm->d_keys, tm->d_bytes, tm->max_len};
    return LX_OK;
}

} // namespace

extern "C" {

int lx_find_accessions(uint8_t const * text, uint64_t n, uint64_t * out_begin, uint32_t * out_len, uint64_t cap, uint64_t * n_found)
{
    if ((!text && n) || !n_found || (cap && (!out_begin || !out_len)))
        return LX_EINVAL;
    uint64_t k = 0;
    uint32_t l = 0;
    for (uint64_t p = lx::taxmap::find_accession(text, n, 0, &l); p < n; p = lx::taxmap::find_accession(text, n, p + l, &l), ++k)
        if (k < cap)
        {
            out_begin[k] = p;
            out_len[k]   = l;
        }
    *n_found = k;
    return LX_OK;
}

int lx_taxmap_create(lx_handle * h, int format, uint8_t const * ids, uint64_t const * id_off, uint64_t n_s, uint64_t chunk_bytes,
                     uint32_t n_threads, lx_taxmap ** out)
{
    if (!h)
        set_output_error("");
    if (!out || (!id_off && n_s) || (!ids && n_s && id_off[n_s]) || (format != LX_TAXMAP_NCBI && format != LX_TAXMAP_UNIPROT) || n_s >= 0xffffffffull)
        return report(h, LX_EINVAL, "lx_taxmap_create: NULL buffer, unknown format or too many subjects");
    *out = nullptr;
    if (chunk_bytes > kMaxChunk || (chunk_bytes && chunk_bytes < 16))
        return report(h, LX_EINVAL, "lx_taxmap_create: chunk_bytes must be 0 or in [16, 2^30]");
    lx_taxmap * tm = nullptr;
    try
    {
        tm          = new lx_taxmap;
        tm->h       = h;
        tm->format  = format;
        tm->threads = n_threads;
        tm->chunk   = chunk_bytes ? chunk_bytes : kDefaultChunk;
        tm->n_s     = n_s;
        tm->header_done = format != LX_TAXMAP_NCBI;
        int rc      = build_table(tm, ids, id_off);
        if (rc == LX_OK && h)
            rc = setup_device(tm);
        else if (rc == LX_OK)
            for (int l = 0; l < 2; ++l)
                if (!(tm->lane[l] = static_cast<uint8_t *>(std::malloc(tm->chunk + 16))))
                    throw std::bad_alloc();
        if (rc)
        {
            lx_taxmap_destroy(tm);
            return rc;
        }
    }
    catch (std::bad_alloc const &)
    {
        lx_taxmap_destroy(tm);
        return report(h, LX_ENOMEM, "lx_taxmap_create: out of host memory");
    }
    *out = tm;
    return LX_OK;
}

int lx_taxmap_feed(lx_taxmap * tm, uint8_t const * bytes, uint64_t n)
{
    if (!tm || (!bytes && n))
        return report(tm ? tm->h : nullptr, LX_EINVAL, "lx_taxmap_feed: NULL argument");
    if (tm->err)
        return report(tm->h, tm->err, tm->err_text);
    if (tm->finished)
        return tm_fail(tm, LX_EINVAL, "lx_taxmap_feed: the map was finished");
    try
    {
        if (!tm->header_done)
        {
            void const * nl = std::memchr(bytes, '\n', n);
            if (!nl)
            {
                tm->header.append(reinterpret_cast<char const *>(bytes), n);
                if (tm->header.size() > 4096)
                    return check_header(tm);
                return LX_OK;
            }
            uint64_t const k = (uint64_t)(static_cast<uint8_t const *>(nl) - bytes);
            tm->header.append(reinterpret_cast<char const *>(bytes), k);
            if (int rc = check_header(tm))
                return rc;
            bytes += k + 1;
            n -= k + 1;
        }
        while (n)
        {
            uint64_t const take = std::min(n, tm->chunk - tm->fill);
            std::memcpy(tm->lane[tm->cur] + tm->fill, bytes, take);
            tm->fill += take;
            bytes += take;
            n -= take;
            if (tm->fill == tm->chunk)
                if (int rc = cut_and_dispatch(tm))
                    return rc;
        }
    }
    catch (std::bad_alloc const &)
    {
        return tm_fail(tm, LX_ENOMEM, "lx_taxmap_feed: out of host memory");
    }
    return LX_OK;
}

int lx_taxmap_finish(lx_taxmap * tm, lx_taxmap_result * out)
{
    if (!tm || !out)
        return report(tm ? tm->h : nullptr, LX_EINVAL, "lx_taxmap_finish: NULL argument");
    if (tm->err)
        return report(tm->h, tm->err, tm->err_text);
    try
    {
        if (!tm->finished)
        {
            if (!tm->header_done)
                if (int rc = check_header(tm))
                    return rc;
            if (tm->fill)
            {
                if (tm->lane[tm->cur][tm->fill - 1] != '\n') // (an unterminated last line is a line; the lanes have room for it)
                    tm->lane[tm->cur][tm->fill++] = '\n';
                if (int rc = cut_and_dispatch(tm))
                    return rc;
            }
            if (int rc = collect(tm))
                return rc;
            // the per-subject lists in file order: a stable counting sort of the pairs by subject
            tm->off.assign(tm->n_s + 1, 0);
            for (Pair const & p : tm->pairs)
                ++tm->off[p.subject + 1];
            for (uint64_t s = 0; s < tm->n_s; ++s)
                tm->off[s + 1] += tm->off[s];
            tm->ids.resize(tm->pairs.size());
            std::vector<uint64_t> at(tm->off.begin(), tm->off.end() - 1);
            for (Pair const & p : tm->pairs)
                tm->ids[at[p.subject]++] = p.taxid;
            tm->present = tm->ids;
            tm->present.push_back(1); // the root is always present
            std::sort(tm->present.begin(), tm->present.end());
            tm->present.erase(std::unique(tm->present.begin(), tm->present.end()), tm->present.end());
            lx_taxmap_result & r = tm->res;
            r           = lx_taxmap_result{};
            r.s_tax_off = tm->off.data();
            r.s_tax_ids = tm->ids.data();
            r.n_s       = tm->n_s;
            r.present   = tm->present.data();
            r.n_present = tm->present.size();
            r.no_acc    = tm->no_acc;
            r.multi_acc = tm->multi_acc;
            for (uint64_t s = 0; s < tm->n_s; ++s)
            {
                uint64_t const k = tm->off[s + 1] - tm->off[s];
                r.no_tax += k == 0;
                r.multi_tax += k > 1;
            }
            r.lines   = tm->lines;
            r.matched = tm->pairs.size();
            std::vector<Pair>().swap(tm->pairs);
            tm->finished = true;
        }
    }
    catch (std::bad_alloc const &)
    {
        return tm_fail(tm, LX_ENOMEM, "lx_taxmap_finish: out of host memory");
    }
    *out = tm->res;
    return LX_OK;
}

void lx_taxmap_destroy(lx_taxmap * tm)
{
    delete tm;
}

} // extern "C"
