// cli/common.hpp -- the small pieces every part of the lambda3 front end uses: owners for what the library hands out, the clock,
// a thread joiner, the sums of the library's statistics.  The front end is one translation unit: lambda3_main.cpp includes the
// cli/ headers, and this one carries the standard headers and the library's for all of them.
#pragma once

#include <algorithm>
#include <array>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../lambda_ext.hpp"
#include "../lx_query_blocks.hpp"
#include "../lx_seeding.hpp"
#include "../scoring_tables.hpp"

namespace
{

using Clock = std::chrono::steady_clock;
double msSince(Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); }

// ---- owners: one alias per kind of thing that has to be given back
template <auto Free>
struct FreeWith
{
    template <class T>
    void operator()(T * p) const
    {
        if (p)
            (void)Free(p);
    }
};
using HandleOwner = std::unique_ptr<lx_handle, FreeWith<lx_destroy>>;
using IndexOwner  = std::unique_ptr<lx_index, FreeWith<lx_index_destroy>>;
using BytesOwner  = std::unique_ptr<lx_bytes, FreeWith<lx_bytes_free>>;
using FileOwner   = std::unique_ptr<std::FILE, FreeWith<std::fclose>>;

// a handle of its own on `device`; the library's text (behind `prefix`) where there is none to be had
HandleOwner makeHandle(int device, char const * prefix = "")
{
    lx_handle * h = nullptr;
    if (lx_create(device, &h) != LX_OK)
        throw std::runtime_error(std::string(prefix) + lx_last_error(nullptr));
    return HandleOwner(h);
}

// the text of a failed output call (h: the handle it ran on, or none), or "cannot write <path>" where the library has none
std::string outputError(lx_handle const * h, std::string const & path)
{
    std::string const why = h ? lx_last_error(h) : lx_last_output_error();
    return !why.empty() ? why : "cannot write " + path;
}

// joins a thread, or every thread of a pool, on every way out of the scope
struct JoinOnExit
{
    std::thread *              one  = nullptr;
    std::vector<std::thread> * pool = nullptr;
    explicit JoinOnExit(std::thread & t) : one(&t) {}
    explicit JoinOnExit(std::vector<std::thread> & p) : pool(&p) {}
    JoinOnExit(JoinOnExit const &) = delete;
    ~JoinOnExit()
    {
        if (one && one->joinable())
            one->join();
        for (size_t i = 0; pool && i < pool->size(); ++i)
            if ((*pool)[i].joinable())
                (*pool)[i].join();
    }
};

bool endsWith(std::string const & s, char const * suf)
{
    return s.size() >= std::strlen(suf) && s.compare(s.size() - std::strlen(suf), std::string::npos, suf) == 0;
}

// the names of a sequence set as lx_seq_names wants them (they point into `names`)
std::vector<char const *> cstrs(std::vector<std::string> const & names)
{
    std::vector<char const *> out;
    for (std::string const & s : names)
        out.push_back(s.c_str());
    return out;
}

lx_record_stats & operator+=(lx_record_stats & a, lx_record_stats const & b)
{
    a.qrys_with_hit += b.qrys_with_hit, a.hits_duplicate2 += b.hits_duplicate2, a.hits_abundant += b.hits_abundant;
    a.hits_final += b.hits_final, a.pairs += b.pairs;
    return a;
}

lx_cull_stats & operator+=(lx_cull_stats & a, lx_cull_stats const & b)
{
    a.hits_max_hsps += b.hits_max_hsps, a.hits_culled += b.hits_culled;
    return a;
}

lx_iterate_stats & operator+=(lx_iterate_stats & a, lx_iterate_stats const & b)
{
    a.hits_duplicate += b.hits_duplicate, a.failed_bitscore += b.failed_bitscore, a.failed_evalue += b.failed_evalue;
    a.failed_identity += b.failed_identity, a.num_ext_score += b.num_ext_score, a.num_ext_ali += b.num_ext_ali;
    return a;
}

} // namespace
