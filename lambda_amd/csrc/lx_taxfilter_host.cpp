// lx_taxfilter_host.cpp -- restricting a search to taxa of the index (include/lambda_ext.h: lx_tax_subject_mask, lx_subject_mask_*,
// lx_seed_result_filter).  lx_tax_subject_mask is the rule, on the host, and the specification of the kernels (lx_taxfilter.hip) that
// lx_subject_mask_create_dev runs over a resident tree.  A mask keeps its words on the host and, made with a handle, on that handle's
// device; lx_seed_result_filter compacts a host-path result here and a device result there, into a second block that takes the
// place of the result's own (the handle's spare block where it is large enough; the old one goes back as lx_seed_result_free
// returns one).
#include <memory>
#include <new>

#include "lx_internal.h"
#include "lx_taxfilter.h"

using lxi::bind;
using lxi::ensure;
using lxi::fail;

struct lx_subject_mask
{
    lx_handle *             h = nullptr; // NULL: the words are on the host only
    uint64_t                n_s = 0, n_kept = 0;
    std::vector<uint64_t>   words;
    lxi::DevBlock<uint64_t> d_words;

    // its handle's device bound and the launch stream through before the block goes
    ~lx_subject_mask()
    {
        if (h && bind(h) == LX_OK)
            (void)hipStreamSynchronize(h->stream);
    }
};

namespace
{

// the text goes to lx_last_output_error() and, with a handle, to lx_last_error(h) too
int say(lx_handle * h, int code, char const * fmt, ...)
{
    char    buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    lxi::set_output_error(buf);
    return h ? fail(h, code, "%s", buf) : code;
}

// what both makers of a mask refuse about the list itself (NULL: nothing)
char const * list_error(lx_taxon_filter const * f)
{
    if (f->n == 0)
        return "an empty list of taxa (n == 0)";
    if (!f->taxa)
        return "NULL list of taxa";
    for (uint64_t i = 0; i < f->n; ++i)
        if (f->taxa[i] == 0)
            return "taxon 0 is listed (0 is no taxon: it stands for 'unassigned')";
    return nullptr;
}

uint64_t mask_words(uint64_t n_s)
{
    return (n_s + 63) / 64;
}

uint64_t subject_of(uint64_t subjId, uint64_t frames)
{
    return subjId / frames;
}

} // namespace

extern "C" {

int lx_tax_subject_mask(lx_tax_tree const * tree, lx_taxon_filter const * f, uint64_t * mask, uint64_t * n_kept, uint8_t * known)
{
    if (!tree || !f || !mask || !n_kept)
        return say(nullptr, LX_EINVAL, "lx_tax_subject_mask: NULL argument");
    if (char const * why = list_error(f))
        return say(nullptr, LX_EINVAL, "lx_tax_subject_mask: %s", why);
    if (lx_check_tax_tree(tree) != LX_OK)
    {
        std::string const why = lx_last_output_error();
        return say(nullptr, LX_EINVAL, "lx_tax_subject_mask: %s", why.c_str());
    }
    try
    {
        lx_tax_tree const &  t = *tree;
        std::vector<uint8_t> listed(std::max<uint64_t>(t.n_taxa, 2), 0), under(t.n_taxa, 0);
        for (uint64_t i = 0; i < f->n; ++i)
            if (f->taxa[i] < t.n_taxa)
                listed[f->taxa[i]] = 1;
        uint32_t max_height = 0;
        for (uint64_t x = 0; x < t.n_taxa; ++x)
            max_height = std::max(max_height, t.heights[x]);
        uint64_t const lim = (uint64_t)max_height + 2;
        for (uint64_t x = 0; x < t.n_taxa; ++x)
        {
            uint32_t c = (uint32_t)x;
            for (uint64_t step = 0; step < lim; ++step)
            {
                if (listed[c])
                {
                    under[x] = 1;
                    break;
                }
                uint32_t const par = t.parents[c];
                if (par <= 1) // the chain ends here; the root belongs to it where it is the parent
                {
                    under[x] = par == 1 && listed[1] ? 1 : 0;
                    break;
                }
                c = par;
            }
        }
        uint64_t const nw = mask_words(t.n_s);
        std::fill(mask, mask + nw, 0ull);
        uint64_t kept = 0;
        for (uint64_t s = 0; s < t.n_s; ++s)
        {
            bool hit = false;
            for (uint64_t x = t.s_tax_off[s]; x < t.s_tax_off[s + 1] && !hit; ++x)
                hit = under[t.s_tax_ids[x]] != 0;
            if (hit != (f->exclude != 0))
            {
                mask[s >> 6] |= 1ull << (s & 63);
                ++kept;
            }
        }
        *n_kept = kept;
        if (known)
        {
            std::vector<uint8_t> seen(t.n_taxa, 0); // a parent of some taxon, or a taxon of some subject
            for (uint64_t x = 0; x < t.n_taxa; ++x)
                seen[t.parents[x]] = 1;
            for (uint64_t x = 0, e = t.s_tax_off[t.n_s]; x < e; ++x)
                seen[t.s_tax_ids[x]] = 1;
            for (uint64_t i = 0; i < f->n; ++i)
            {
                uint32_t const L = f->taxa[i];
                known[i]         = L < t.n_taxa && (t.parents[L] != 0 || seen[L]) ? 1 : 0;
            }
        }
    }
    catch (std::bad_alloc const &)
    {
        return say(nullptr, LX_ENOMEM, "lx_tax_subject_mask: out of host memory");
    }
    return LX_OK;
}

int lx_subject_mask_create_dev(lx_handle * h, lx_tax_dev const * t, lx_taxon_filter const * f, lx_subject_mask ** out)
{
    if (!h)
        return say(nullptr, LX_EINVAL, "lx_subject_mask_create_dev: h == NULL");
    h->phase_ev.clear(); // (a refused call reports no launch)
    h->ev_pool_used = 0;
    if (!t || !f || !out)
        return say(h, LX_EINVAL, "lx_subject_mask_create_dev: NULL argument");
    *out = nullptr;
    if (t->h != h)
        return say(h, LX_EINVAL, "lx_subject_mask_create_dev: the tree was made on another handle");
    if (char const * why = list_error(f))
        return say(h, LX_EINVAL, "lx_subject_mask_create_dev: %s", why);
    if (f->n > 0x7ffffff0ull)
        return say(h, LX_EINVAL, "lx_subject_mask_create_dev: at most 2^31 - 16 listed taxa");
    try
    {
        std::unique_ptr<lx_subject_mask> m(new lx_subject_mask);
        int                              rc = bind(h);
        if (rc)
            return rc;
        uint64_t const nw = mask_words(t->n_s), n_flags = std::max<uint64_t>(t->n_taxa, 2);
        m->words.assign(nw, 0);
        m->n_s = t->n_s;
        lx_handle::TaxFilter & z = h->taxfilter;
        if ((rc = ensure(h, z.d_list, f->n * 4)) || (rc = ensure(h, z.d_flags, 2 * n_flags)) || (rc = ensure(h, z.d_words, 16)))
            return rc;
        LX_HIP(h, hipMalloc(m->d_words.out(), std::max<uint64_t>(nw * 8, 16)));
        m->h                 = h;
        hipStream_t const st = h->stream;
        LX_HIP(h, hipMemcpyAsync(z.d_list.ptr, f->taxa, f->n * 4, hipMemcpyHostToDevice, st));
        lx::taxfilter::MaskParams p{};
        p.tree    = lx::lca::TreeView{t->d_nodes, t->d_off, t->d_ids, t->max_height};
        p.n_taxa  = t->n_taxa;
        p.n_s     = t->n_s;
        p.list    = static_cast<uint32_t const *>(z.d_list.ptr);
        p.n_list  = f->n;
        p.exclude = f->exclude ? 1 : 0;
        p.listed  = static_cast<uint8_t *>(z.d_flags.ptr);
        p.under   = p.listed + n_flags;
        p.words   = m->d_words;
        p.n_kept  = static_cast<unsigned long long *>(z.d_words.ptr);
        lxi::PhaseTimer timer(h, st, 14);
        LX_HIP(h, lx::taxfilter::launch_mask(p, st));
        timer.close();
        unsigned long long kept = 0;
        LX_HIP(h, hipMemcpyAsync(&kept, p.n_kept, sizeof(kept), hipMemcpyDeviceToHost, st));
        if (nw)
            LX_HIP(h, hipMemcpyAsync(m->words.data(), m->d_words, nw * 8, hipMemcpyDeviceToHost, st));
        LX_HIP(h, hipStreamSynchronize(st));
        m->n_kept = kept;
        *out      = m.release();
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_subject_mask_create_dev: out of host memory");
    }
    return LX_OK;
}

int lx_subject_mask_create(lx_handle * h, uint64_t const * words, uint64_t n_s, lx_subject_mask ** out)
{
    if (!out || (n_s && !words))
        return say(h, LX_EINVAL, "lx_subject_mask_create: NULL argument");
    *out = nullptr;
    if (h && n_s >= 0xffffffffull)
        return say(h, LX_EINVAL, "lx_subject_mask_create: too many subjects for the device");
    uint64_t const nw = mask_words(n_s);
    if ((n_s & 63) && (words[nw - 1] >> (n_s & 63)) != 0)
        return say(h, LX_EINVAL, "lx_subject_mask_create: a bit at or beyond subject %llu is set", (unsigned long long)n_s);
    try
    {
        std::unique_ptr<lx_subject_mask> m(new lx_subject_mask);
        m->words.assign(words, words + nw);
        m->n_s = n_s;
        for (uint64_t w : m->words)
            m->n_kept += (uint64_t)__builtin_popcountll(w);
        if (h)
        {
            int rc = bind(h);
            if (rc)
                return rc;
            LX_HIP(h, hipMalloc(m->d_words.out(), std::max<uint64_t>(nw * 8, 16)));
            m->h = h;
            if (nw)
                LX_HIP(h, hipMemcpy(m->d_words, m->words.data(), nw * 8, hipMemcpyHostToDevice));
        }
        *out = m.release();
    }
    catch (std::bad_alloc const &)
    {
        return say(h, LX_ENOMEM, "lx_subject_mask_create: out of host memory");
    }
    return LX_OK;
}

int lx_subject_mask_info(lx_subject_mask const * m, uint64_t * n_s, uint64_t * n_kept)
{
    if (!m)
        return say(nullptr, LX_EINVAL, "lx_subject_mask_info: NULL mask");
    if (n_s)
        *n_s = m->n_s;
    if (n_kept)
        *n_kept = m->n_kept;
    return LX_OK;
}

int lx_subject_mask_copy(lx_subject_mask const * m, uint64_t * words)
{
    if (!m || (!words && !m->words.empty()))
        return say(nullptr, LX_EINVAL, "lx_subject_mask_copy: NULL argument");
    if (!m->words.empty())
        std::memcpy(words, m->words.data(), m->words.size() * 8);
    return LX_OK;
}

void lx_subject_mask_destroy(lx_subject_mask * m)
{
    delete m;
}

int lx_seed_result_filter(lx_seed_result * r, lx_subject_mask const * m, int32_t sbj_num_frames, uint64_t * n_before, uint64_t * n_kept)
{
    lx_handle * const h = r ? r->h : nullptr;
    if (h)
    {
        h->phase_ev.clear(); // (a refused call reports no launch)
        h->ev_pool_used = 0;
    }
    if (!r || !m)
        return say(h, LX_EINVAL, "lx_seed_result_filter: NULL argument");
    if (sbj_num_frames < 1 || sbj_num_frames > 6)
        return say(h, LX_EINVAL, "lx_seed_result_filter: %d subject frames (1 .. 6)", (int)sbj_num_frames);
    if (h && !m->h)
        return say(h, LX_EINVAL, "lx_seed_result_filter: a match list on the device needs a mask made with its handle (this one is on the host only)");
    if (h && m->h != h)
        return say(h, LX_EINVAL, "lx_seed_result_filter: the mask was made on another handle");
    uint64_t const n = r->st.n_matches, frames = (uint64_t)sbj_num_frames;
    if (n_before)
        *n_before = n;
    if (n_kept)
        *n_kept = n;
    if (n == 0)
        return LX_OK;
    if (!h)
    {
        std::vector<lx_match> & list = r->host;
        for (uint64_t k = 0; k < n; ++k)
            if (subject_of(list[k].subjId, frames) >= m->n_s)
                return say(nullptr, LX_EINVAL, "lx_seed_result_filter: match %llu names subject %llu of %llu", (unsigned long long)k,
                           (unsigned long long)subject_of(list[k].subjId, frames), (unsigned long long)m->n_s);
        uint64_t o = 0;
        for (uint64_t k = 0; k < n; ++k)
        {
            uint64_t const s = subject_of(list[k].subjId, frames);
            if ((m->words[s >> 6] >> (s & 63)) & 1)
                list[o++] = list[k];
        }
        list.resize(o);
        r->st.n_matches = o;
        if (n_kept)
            *n_kept = o;
        return LX_OK;
    }
    if (n > 0x7ffffff0ull)
        return say(h, LX_EINVAL, "lx_seed_result_filter: at most 2^31 - 16 matches");
    int rc = bind(h);
    if (rc)
        return rc;
    lx_handle::TaxFilter & z     = h->taxfilter;
    uint64_t const         tiles = lx::taxfilter::scan_tiles(n);
    if ((rc = ensure(h, z.d_tot, (size_t)(tiles + 1) * 4)) || (rc = ensure(h, z.d_words, 16)))
        return rc;
    hipStream_t const           st = h->stream;
    lx::taxfilter::FilterParams p{};
    p.src       = static_cast<uint4 const *>(r->d_out.ptr);
    p.n         = n;
    p.words     = m->d_words;
    p.n_s       = m->n_s;
    p.frames    = (uint32_t)sbj_num_frames;
    p.block_tot = static_cast<uint32_t *>(z.d_tot.ptr);
    p.err       = static_cast<uint32_t *>(z.d_words.ptr) + 2; // (behind the mask maker's 8-byte counter)
    lxi::PhaseTimer count_timer(h, st, 14);
    LX_HIP(h, lx::taxfilter::launch_count(p, st));
    count_timer.close();
    uint32_t kept = 0, err = 0;
    LX_HIP(h, hipMemcpyAsync(&kept, p.block_tot + tiles, 4, hipMemcpyDeviceToHost, st));
    LX_HIP(h, hipMemcpyAsync(&err, p.err, 4, hipMemcpyDeviceToHost, st));
    LX_HIP(h, hipStreamSynchronize(st));
    if (err)
        return say(h, LX_EINVAL, "lx_seed_result_filter: a match names a subject beyond the mask's %llu", (unsigned long long)m->n_s);
    if (n_kept)
        *n_kept = kept;
    if (kept == n) // all kept: the list stays where it is
        return LX_OK;
    // the second block: the handle's spare one where it has the room, else a new one
    size_t const want = std::max<size_t>((size_t)kept * sizeof(lx_match), 16);
    lxi::DevBuf  nb;
    if (h->seed.d_spare.cap >= want)
        nb = std::move(h->seed.d_spare);
    else
    {
        LX_HIP(h, hipMalloc(&nb.ptr, want));
        nb.cap = want;
    }
    if (kept)
    {
        p.dst = static_cast<uint4 *>(nb.ptr);
        lxi::PhaseTimer scatter_timer(h, st, 14);
        hipError_t const e = lx::taxfilter::launch_scatter(p, st);
        scatter_timer.close();
        hipError_t const e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
        if (e2 != hipSuccess)
        {
            if (nb.cap > h->seed.d_spare.cap)
                std::swap(nb, h->seed.d_spare);
            return fail(h, LX_EHIP, "lx_seed_result_filter: %s", hipGetErrorString(e2));
        }
    }
    std::swap(r->d_out, nb); // nb: the old block, which goes back as lx_seed_result_free returns one
    if (nb.cap > h->seed.d_spare.cap)
        std::swap(nb, h->seed.d_spare);
    r->st.n_matches = kept;
    r->have_host    = false;
    std::vector<lx_match>().swap(r->host);
    return LX_OK;
}

} // extern "C"
