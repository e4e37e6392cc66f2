// lx_taxonomy.cpp -- lx_taxonomy_build: the taxonomic tree of an index from NCBI's taxdump, as the reference's
// parseAndStoreTaxTree makes it (src/mkindex_algo.hpp:354-598).  Host code: nodes.dmp has a few million lines and every step is a
// pass over them.
//
//   1. nodes.dmp: parent[field 0] = field 2 (tab-separated, fields 1 and 3 are '|').
//   2. the present taxa (those of the subjects, the root among them) and all their ancestors are kept; every other parent is 0.
//   3. in-degrees; a parent of in-degree 1 that is not itself present is skipped (flattening), then disconnected.
//   4. heights: the steps from a taxon to a parent of at most 1.
//   5. names.dmp: the "scientific name" rows name the kept taxa; an id beyond the tree is an error.  Name 0 is "invalid", a kept
//      taxon without a name "n/a".
// One deviation: the arrays cover every taxon that occurs -- node ids, parent ids and present taxa alike.  The reference sizes
// them by the largest node id and reads past their end for a present taxon (or a parent) beyond it; here such a taxon has parent 0,
// so it counts as unassigned, and lx_compute_lca skips it instead of failing.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "lambda_ext.h"

namespace lxi
{
void set_output_error(std::string const & msg);
}

struct lx_taxonomy
{
    std::vector<uint32_t>     parents, heights;
    std::vector<std::string>  names;
    std::vector<char const *> name_ptrs;
    uint64_t                  n_nodes    = 0;
    uint32_t                  max_height = 0, unnamed = 0;
    std::string               warnings;
};

namespace
{

struct Fail
{
    std::string msg;
};

// the lines of text[0, n) (the part after the last '\n' is a line when it is not empty), split at '\t'
template <class F>
void for_each_line(char const * text, uint64_t n, F && f)
{
    std::vector<std::string_view> fields;
    uint64_t                      line = 0;
    for (uint64_t p = 0; p < n;)
    {
        char const *   nl = static_cast<char const *>(std::memchr(text + p, '\n', n - p));
        uint64_t const e  = nl ? (uint64_t)(nl - text) : n;
        fields.clear();
        for (uint64_t a = p;;)
        {
            char const *   tab = static_cast<char const *>(std::memchr(text + a, '\t', e - a));
            uint64_t const b   = tab ? (uint64_t)(tab - text) : e;
            fields.emplace_back(text + a, b - a);
            if (!tab)
                break;
            a = b + 1;
        }
        f(++line, fields);
        p = e + 1;
    }
}

// std::from_chars into uint32_t, checking only the error code
bool from_chars_u32(std::string_view s, uint32_t & out)
{
    uint64_t v = 0;
    size_t   k = 0;
    for (; k < s.size() && s[k] >= '0' && s[k] <= '9'; ++k)
    {
        v = v * 10 + (uint64_t)(s[k] - '0');
        if (v > 0xffffffffull)
            v = 0x100000000ull; // (stays out of range)
    }
    if (k == 0 || v > 0xffffffffull)
        return false;
    out = (uint32_t)v;
    return true;
}

uint32_t read_id(std::string_view s, char const * file, uint64_t line)
{
    uint32_t v = 0;
    if (!from_chars_u32(s, v))
        throw Fail{std::string(file) + " line " + std::to_string(line) + ": Error: Expected taxonomical ID, but got something I couldn't read: " +
                   std::string(s.substr(0, 200))};
    return v;
}

void build(lx_taxonomy & T, char const * nodes, uint64_t nodes_n, char const * names, uint64_t names_n, uint32_t const * present_ids,
           uint64_t n_present)
{
    // ---- 1. nodes.dmp
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    uint64_t                                   size = 2;
    for_each_line(nodes, nodes_n,
                  [&](uint64_t line, std::vector<std::string_view> const & f)
                  {
                      uint32_t const id     = read_id(f[0], "nodes.dmp", line);
                      uint32_t const parent = read_id(f.size() > 2 ? f[2] : std::string_view(), "nodes.dmp", line);
                      edges.emplace_back(id, parent);
                      size = std::max<uint64_t>(size, (uint64_t)std::max(id, parent) + 1);
                  });
    for (uint64_t k = 0; k < n_present; ++k)
        size = std::max<uint64_t>(size, (uint64_t)present_ids[k] + 1);
    std::vector<uint32_t> & parent = T.parents;
    parent.assign(size, 0);
    for (auto const & e : edges) // (a later line for the same id wins, as in the reference)
        parent[e.first] = e.second;
    std::vector<bool> present(size, false);
    for (uint64_t k = 0; k < n_present; ++k)
        present[present_ids[k]] = true;
    present[1] = true; // the root

    // ---- 2. the present taxa and their ancestors
    std::vector<bool> kept(present);
    for (uint64_t i = 0; i < size; ++i)
        if (present[i])
        {
            uint32_t cur   = (uint32_t)i;
            uint64_t steps = 0;
            do
            {
                cur       = parent[cur];
                kept[cur] = true;
                if (++steps > size)
                    throw Fail{"nodes.dmp: the ancestors of taxon " + std::to_string(i) + " form a cycle"};
            } while (cur > 1);
        }
    for (uint64_t i = 0; i < size; ++i)
        if (!kept[i])
            parent[i] = 0;

    // ---- 3. in-degrees, flattening, disconnecting
    std::vector<uint32_t> indeg(size, 0);
    for (uint64_t i = 0; i < size; ++i)
        ++indeg[parent[i]];
    for (uint64_t i = 0; i < size; ++i)
    {
        uint32_t cur = parent[i];
        while (cur > 1 && indeg[cur] == 1 && !present[cur])
            cur = parent[cur];
        parent[i] = cur;
    }
    for (uint64_t i = 0; i < size; ++i)
        if (indeg[i] == 1 && !present[i])
        {
            parent[i] = 0;
            kept[i]   = false;
        }

    // ---- 4. heights
    T.heights.assign(size, 0);
    for (uint64_t i = 0; i < size; ++i)
    {
        if (parent[i] > 0)
            ++T.n_nodes;
        uint32_t h = 0;
        for (uint32_t cur = parent[i]; cur > 1; cur = parent[cur])
            ++h;
        T.heights[i] = h;
        T.max_height = std::max(T.max_height, h);
    }

    // ---- 5. names.dmp
    T.names.assign(size, std::string());
    for_each_line(names, names_n,
                  [&](uint64_t line, std::vector<std::string_view> const & f)
                  {
                      if (f.size() < 7 || f[6] != "scientific name")
                          return;
                      uint32_t const id = read_id(f[0], "names.dmp", line);
                      if (id >= size)
                          throw Fail{"Error: taxonomical ID is " + std::to_string(id) + ", but no such taxon in tree."};
                      if (kept[id])
                          T.names[id].assign(f[2].data(), f[2].size());
                  });
    T.names[0] = "invalid";
    for (uint64_t i = 0; i < size; ++i)
        if (kept[i] && T.names[i].empty())
        {
            T.warnings += "Warning: Taxon with ID " + std::to_string(i) + " has no name associated, defaulting to \"n/a\".\n";
            T.names[i] = "n/a";
            ++T.unnamed;
        }
    if ((uint64_t)T.unnamed * 10 > size)
        T.warnings += "Warning: More than 10% of taxa have no valid name entry.\n";
    T.name_ptrs.resize(size);
    for (uint64_t i = 0; i < size; ++i)
        T.name_ptrs[i] = T.names[i].c_str();
}

} // namespace

extern "C" {

int lx_taxonomy_build(char const * nodes, uint64_t nodes_n, char const * names, uint64_t names_n, uint32_t const * present, uint64_t n_present,
                      lx_taxonomy ** out)
{
    lxi::set_output_error("");
    if (!out || (!nodes && nodes_n) || (!names && names_n) || (!present && n_present))
    {
        lxi::set_output_error("lx_taxonomy_build: NULL buffer");
        return LX_EINVAL;
    }
    *out            = nullptr;
    lx_taxonomy * t = nullptr;
    try
    {
        t = new lx_taxonomy;
        build(*t, nodes, nodes_n, names, names_n, present, n_present);
    }
    catch (Fail const & e)
    {
        delete t;
        lxi::set_output_error(e.msg);
        return LX_EINVAL;
    }
    catch (std::bad_alloc const &)
    {
        delete t;
        lxi::set_output_error("lx_taxonomy_build: out of host memory");
        return LX_ENOMEM;
    }
    *out = t;
    return LX_OK;
}

int lx_taxonomy_get(lx_taxonomy const * t, lx_taxonomy_info * out)
{
    if (!t || !out)
        return LX_EINVAL;
    out->parents    = t->parents.data();
    out->heights    = t->heights.data();
    out->names      = t->name_ptrs.data();
    out->n_taxa     = t->parents.size();
    out->n_nodes    = t->n_nodes;
    out->max_height = t->max_height;
    out->unnamed    = t->unnamed;
    out->warnings   = t->warnings.c_str();
    return LX_OK;
}

void lx_taxonomy_free(lx_taxonomy * t)
{
    delete t;
}

} // extern "C"
