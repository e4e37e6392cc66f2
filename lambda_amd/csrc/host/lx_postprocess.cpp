// lx_postprocess.cpp -- what happens to a record list between the extension and the writers.
//
// Host-side C++ mirror of
//   _writeRecord          src/search_algo.hpp:820-913   (sort, dedupe, bit-score order, top-N; :884-907 the LCA fold)
//   computeLCA            src/search_misc.hpp:86-112
// with the two culling rules of lx_cull.h between the unique and the cut (lx_postprocess_records_ex), the LCA over the records within
// a share of the best bit score (lx_compute_lca_ex), and the check of a taxonomy tree's invariants (lx_check_tax_tree).  The writers
// are in lx_output.cpp; refusal texts go to lx_last_output_error() through lxi::set_output_error.
#include <algorithm>
#include <cmath>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../lx_cull.h" // the rule of lx_cull_options, shared with the kernels
#include "../lx_output_host.h"

using lxi::set_output_error;

namespace lxi
{
int cull_check(lx_blast_match const * m, uint64_t n, lx_cull_options const * opt, uint64_t max_len, std::string & why)
{
    if (!opt || opt->culling_limit == 0)
        return LX_OK;
    if (!opt->q_lens && n)
    {
        why = "lx_cull_options: culling_limit > 0 needs q_lens";
        return LX_EINVAL;
    }
    for (uint64_t i = 0; i < n; ++i)
    {
        if (m[i].n_qid >= opt->n_q)
        {
            why = "lx_cull_options: row " + std::to_string(i) + " names query " + std::to_string(m[i].n_qid) + ", q_lens has " + std::to_string(opt->n_q) + " entries";
            return LX_EINVAL;
        }
        uint64_t const len = opt->q_lens[m[i].n_qid];
        if (len > max_len)
        {
            why = "lx_cull_options: query " + std::to_string(m[i].n_qid) + " is " + std::to_string(len) + " letters long, the device step takes " + std::to_string(max_len) + " at most";
            return LX_EINVAL;
        }
        uint64_t lo, hi;
        if (!lx::cull::interval(m[i].q_start, m[i].q_end, m[i].q_frame, len, opt->q_translated != 0, lo, hi))
        {
            why = "lx_cull_options: the query interval of row " + std::to_string(i) + " does not fit its query's length of " + std::to_string(len);
            return LX_EINVAL;
        }
    }
    return LX_OK;
}
} // namespace lxi

namespace
{

// _writeRecord's step for a whole list; cull: NULL, or the two rules between the unique and the cut (lx_cull.h)
uint64_t postprocessRecords(lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_cull_options const * cull, lx_record_stats * stats, lx_cull_stats * cull_stats)
{
    lx_record_stats st{};
    lx_cull_stats   cs{};
    uint64_t        w = 0;
    for (uint64_t lo = 0; lo < n;)
    {
        uint64_t hi = lo + 1;
        while (hi < n && m[hi].n_qid == m[lo].n_qid)
            ++hi;
        ++st.qrys_with_hit; // :826
        std::vector<lx_blast_match> rec(m + lo, m + hi);
        // order by subject, coordinates and frames; among equal keys the better bit score comes first (b and a swapped in the
        // last tie component), so that std::unique below keeps it (:832-853)
        std::stable_sort(rec.begin(), rec.end(),
                         [](lx_blast_match const & a, lx_blast_match const & b)
                         {
                             return std::tie(a.n_sid, a.q_start, a.q_end, a.s_start, a.s_end, a.q_frame, a.s_frame, b.bit_score) <
                                    std::tie(b.n_sid, b.q_start, b.q_end, b.s_start, b.s_end, b.q_frame, b.s_frame, a.bit_score);
                         });
        // one record per (subject, coordinates, frames): the first of each group survives (:856-862)
        auto const before = rec.size();
        rec.erase(std::unique(rec.begin(), rec.end(),
                              [](lx_blast_match const & a, lx_blast_match const & b)
                              {
                                  return std::tie(a.n_sid, a.q_start, a.q_end, a.s_start, a.s_end, a.q_frame, a.s_frame) ==
                                         std::tie(b.n_sid, b.q_start, b.q_end, b.s_start, b.s_end, b.q_frame, b.s_frame);
                              }),
                  rec.end());
        st.hits_duplicate2 += before - rec.size();
        // output order: best bit score (= smallest e-value) first; stable like the reference's list sort (:865)
        std::stable_sort(rec.begin(), rec.end(),
                         [](lx_blast_match const & a, lx_blast_match const & b) { return a.bit_score > b.bit_score; });
        // rec now stands in order 2: row j is better than row i exactly when j < i (lx_cull.h).  Every row's fate is a count over
        // the better rows, as in the kernels of lx_toprec.hip
        if (cull && cull->max_hsps)
        {
            std::vector<lx_blast_match> left;
            for (size_t i = 0; i < rec.size(); ++i)
            {
                uint64_t same = 0;
                for (size_t j = 0; j < i && same < cull->max_hsps; ++j)
                    same += rec[j].n_sid == rec[i].n_sid;
                if (same < cull->max_hsps)
                    left.push_back(rec[i]);
            }
            cs.hits_max_hsps += rec.size() - left.size();
            rec.swap(left);
        }
        if (cull && cull->culling_limit)
        {
            std::vector<uint64_t> lo(rec.size()), hi(rec.size());
            for (size_t i = 0; i < rec.size(); ++i)
                (void)lx::cull::interval(rec[i].q_start, rec[i].q_end, rec[i].q_frame, cull->q_lens[rec[i].n_qid], cull->q_translated != 0, lo[i], hi[i]);
            std::vector<lx_blast_match> left;
            for (size_t i = 0; i < rec.size(); ++i)
            {
                uint64_t around = 0;
                for (size_t j = 0; j < i && around < cull->culling_limit; ++j)
                    around += lx::cull::envelops(lo[j], hi[j], lo[i], hi[i]);
                if (around < cull->culling_limit)
                    left.push_back(rec[i]);
            }
            cs.hits_culled += rec.size() - left.size();
            rec.swap(left);
        }
        // at most max_matches records per query, the rest is counted (:867-872)
        if (rec.size() > max_matches)
        {
            st.hits_abundant += rec.size() - max_matches;
            rec.resize(max_matches);
        }
        st.hits_final += rec.size();
        std::set<uint64_t> uniq; // :876-882
        for (auto const & r : rec)
            uniq.insert(r.n_sid);
        st.pairs += uniq.size();
        for (auto const & r : rec)
            m[w++] = r;
        lo = hi;
    }
    if (stats)
        *stats = st;
    if (cull_stats)
        *cull_stats = cs;
    return w;
}

// computeLCA (src/search_misc.hpp:86-112): level the two nodes, then climb together; 0 = the paths never met
bool lca_of(lx_tax_tree const & t, uint32_t n1, uint32_t n2, uint32_t & out)
{
    if (n1 == n2)
    {
        out = n1;
        return true;
    }
    if (n1 >= t.n_taxa || n2 >= t.n_taxa)
        return false;
    for (uint32_t i = t.heights[n1]; i > t.heights[n2]; --i)
    {
        n1 = t.parents[n1];
        if (n1 >= t.n_taxa)
            return false;
    }
    for (uint32_t i = t.heights[n2]; i > t.heights[n1]; --i)
    {
        n2 = t.parents[n2];
        if (n2 >= t.n_taxa)
            return false;
    }
    while (n1 != 0 && n2 != 0)
    {
        if (n1 == n2)
        {
            out = n1;
            return true;
        }
        n1 = t.parents[n1];
        n2 = t.parents[n2];
        if (n1 >= t.n_taxa || n2 >= t.n_taxa)
            return false;
    }
    return false; // "LCA-computation error: One of the paths didn't lead to root."
}

} // namespace

extern "C" {

uint64_t lx_postprocess_records(lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_record_stats * stats)
{
    return postprocessRecords(m, n, max_matches, nullptr, stats, nullptr);
}

void lx_cull_options_default(lx_cull_options * o)
{
    if (o)
        *o = lx_cull_options{};
}

int64_t lx_postprocess_records_ex(lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_cull_options const * opt, lx_record_stats * stats,
                                  lx_cull_stats * cull_stats)
{
    set_output_error("");
    if (!m && n)
    {
        set_output_error("lx_postprocess_records_ex: NULL rows");
        return LX_EINVAL;
    }
    std::string why;
    if (lxi::cull_check(m, n, opt, ~0ull, why) != LX_OK)
    {
        set_output_error(why);
        return LX_EINVAL;
    }
    return (int64_t)postprocessRecords(m, n, max_matches, opt, stats, cull_stats);
}

int lx_compute_lca(lx_blast_match const * m, uint64_t n, lx_tax_tree const * tree, uint64_t * out_qid, uint32_t * out_lca,
                   uint64_t * out_n)
{
    if ((!m && n) || !tree || !out_qid || !out_lca || !out_n || !tree->parents || !tree->heights || !tree->s_tax_off ||
        (!tree->s_tax_ids && tree->n_s && tree->s_tax_off[tree->n_s]))
        return LX_EINVAL;
    lx_tax_tree const & t = *tree;
    uint64_t            w = 0;
    for (uint64_t lo = 0; lo < n;)
    {
        uint64_t hi = lo + 1;
        while (hi < n && m[hi].n_qid == m[lo].n_qid)
            ++hi;
        for (uint64_t k = lo; k < hi; ++k)
            if (m[k].n_sid >= t.n_s)
                return LX_EINVAL;
        // the first match whose subject's first taxon is assigned (has a parent) starts the fold (:887-896)
        uint32_t lca = 0;
        for (uint64_t k = lo; k < hi && lca == 0; ++k)
        {
            uint64_t const a = t.s_tax_off[m[k].n_sid], b = t.s_tax_off[m[k].n_sid + 1];
            if (b > a)
            {
                uint32_t const first = t.s_tax_ids[a];
                if (first >= t.n_taxa)
                    return LX_EINVAL;
                if (t.parents[first] != 0)
                    lca = first;
            }
        }
        if (lca != 0) // every assigned taxon of every match (:898-906); unassigned ones are ignored
            for (uint64_t k = lo; k < hi; ++k)
                for (uint64_t x = t.s_tax_off[m[k].n_sid]; x < t.s_tax_off[m[k].n_sid + 1]; ++x)
                {
                    uint32_t const tax = t.s_tax_ids[x];
                    if (tax >= t.n_taxa)
                        return LX_EINVAL;
                    if (t.parents[tax] != 0 && !lca_of(t, tax, lca, lca))
                        return LX_EINVAL;
                }
        out_qid[w] = m[lo].n_qid;
        out_lca[w] = lca;
        ++w;
        lo = hi;
    }
    *out_n = w;
    return LX_OK;
}

void lx_lca_options_default(lx_lca_options * o)
{
    if (!o)
        return;
    *o             = lx_lca_options{};
    o->top_percent = 100.0;
}

// lx_compute_lca (src/search_algo.hpp:884-907, src/search_misc.hpp:86-112) over the records within top_percent of the query's best
// bit score: the same two loops, both over the kept records only
int lx_compute_lca_ex(lx_blast_match const * m, uint64_t n, lx_tax_tree const * tree, lx_lca_options const * opt, uint64_t * out_qid,
                      uint32_t * out_lca, uint64_t * out_n)
{
    double const top = opt ? opt->top_percent : 100.0;
    set_output_error("");
    if (!(top >= 0.0 && top <= 100.0)) // (a NaN fails both)
    {
        set_output_error("lx_compute_lca_ex: top_percent must be in [0, 100]");
        return LX_EINVAL;
    }
    if (top == 100.0)
        return lx_compute_lca(m, n, tree, out_qid, out_lca, out_n);
    if ((!m && n) || !tree || !out_qid || !out_lca || !out_n || !tree->parents || !tree->heights || !tree->s_tax_off ||
        (!tree->s_tax_ids && tree->n_s && tree->s_tax_off[tree->n_s]))
        return LX_EINVAL;
    lx_tax_tree const & t = *tree;
    double const        f = 1.0 - top / 100.0;
    uint64_t            w = 0;
    for (uint64_t lo = 0; lo < n;)
    {
        uint64_t hi = lo + 1;
        while (hi < n && m[hi].n_qid == m[lo].n_qid)
            ++hi;
        for (uint64_t k = lo; k < hi; ++k)
        {
            if (m[k].n_sid >= t.n_s)
                return LX_EINVAL;
            if (!std::isfinite(m[k].bit_score))
            {
                set_output_error("lx_compute_lca_ex: a bit score that is not finite (row " + std::to_string(k) + ")");
                return LX_EINVAL;
            }
        }
        double best = m[lo].bit_score;
        for (uint64_t k = lo + 1; k < hi; ++k)
            best = m[k].bit_score > best ? m[k].bit_score : best;
        double const cut  = best * f; // (one multiplication: the device's is the same)
        auto const   kept = [&](uint64_t k) { return m[k].bit_score >= cut || m[k].bit_score == best; };
        uint32_t     lca  = 0;
        for (uint64_t k = lo; k < hi && lca == 0; ++k) // :887-896, over the kept records
        {
            if (!kept(k))
                continue;
            uint64_t const a = t.s_tax_off[m[k].n_sid], b = t.s_tax_off[m[k].n_sid + 1];
            if (b > a)
            {
                uint32_t const first = t.s_tax_ids[a];
                if (first >= t.n_taxa)
                    return LX_EINVAL;
                if (t.parents[first] != 0)
                    lca = first;
            }
        }
        if (lca != 0) // :898-906, over the kept records
            for (uint64_t k = lo; k < hi; ++k)
            {
                if (!kept(k))
                    continue;
                for (uint64_t x = t.s_tax_off[m[k].n_sid]; x < t.s_tax_off[m[k].n_sid + 1]; ++x)
                {
                    uint32_t const tax = t.s_tax_ids[x];
                    if (tax >= t.n_taxa)
                        return LX_EINVAL;
                    if (t.parents[tax] != 0 && !lca_of(t, tax, lca, lca))
                    {
                        set_output_error("LCA-computation error: One of the paths didn't lead to root.");
                        return LX_EINVAL;
                    }
                }
            }
        out_qid[w] = m[lo].n_qid;
        out_lca[w] = lca;
        ++w;
        lo = hi;
    }
    *out_n = w;
    return LX_OK;
}

// the invariants of lx_taxonomy_build's trees (host/lx_taxonomy.cpp, step 4) that make every climb of lca_of end
int lx_check_tax_tree(lx_tax_tree const * tree)
{
    auto const refuse = [](std::string const & why)
    {
        set_output_error("lx_check_tax_tree: " + why);
        return LX_EINVAL;
    };
    if (!tree || !tree->parents || !tree->heights || !tree->s_tax_off)
        return refuse("NULL tree, parents, heights or s_tax_off");
    lx_tax_tree const & t = *tree;
    if (t.s_tax_off[0] != 0)
        return refuse("s_tax_off does not start at 0");
    for (uint64_t s = 0; s < t.n_s; ++s)
        if (t.s_tax_off[s + 1] < t.s_tax_off[s])
            return refuse("s_tax_off descends at subject " + std::to_string(s));
    uint64_t const n_ids = t.s_tax_off[t.n_s];
    if (n_ids && !t.s_tax_ids)
        return refuse("NULL s_tax_ids");
    for (uint64_t x = 0; x < n_ids; ++x)
        if (t.s_tax_ids[x] >= t.n_taxa)
            return refuse("taxon " + std::to_string(t.s_tax_ids[x]) + " of a subject is not in the tree (" + std::to_string(t.n_taxa) + " taxa)");
    for (uint64_t x = 0; x < t.n_taxa; ++x)
    {
        uint32_t const p = t.parents[x];
        if (p >= t.n_taxa)
            return refuse("the parent of taxon " + std::to_string(x) + " is not in the tree");
        if (p > 1 && t.heights[x] != (uint64_t)t.heights[p] + 1)
            return refuse("the height of taxon " + std::to_string(x) + " is not its parent's plus one");
        if (p <= 1 && t.heights[x] != 0)
            return refuse("taxon " + std::to_string(x) + " has no parent below the root and a height that is not 0");
    }
    return LX_OK;
}

} // extern "C"
