// lx_cull.h -- the rule of --max-hsps and --culling-limit (include/lambda_ext.h: lx_cull_options), in plain integers and doubles,
// shared by the host function (lx_postprocess_records_ex, host/lx_postprocess.cpp) and the kernels (lx_toprec.hip).  Not part of the ABI.
//
// Per run of equal n_qid, over the rows that survive _writeRecord's unique step, in its order 2 (bit score descending, ties by place
// in order 1).  Row a is BETTER than row b when it comes earlier in that order: a strict total order.
//   max_hsps = K > 0       a row is dropped when at least K better rows have the same n_sid (hits_max_hsps)
//   culling_limit = L > 0  over the rows that max_hsps left: a row is dropped when at least L better rows have a query interval that
//                          envelops its own (lo_b <= lo and hi <= hi_b; equal intervals envelop each other) (hits_culled)
// A row's query interval is the closed interval [min, max] of the 1-based qstart / qend that the .m8 writer prints for it
// (host/lx_output.cpp, formatRecord): nucleotide positions 3 a + |f| - 1 for a translated query, mirrored on the minus strand;
// mirrored by the query's length for the minus frames of BLASTN and bisulfite; q_start + 1 .. q_end otherwise.
// The count runs over all rows that max_hsps left, rows that are themselves culled included: enveloping is transitive, so a culled
// enveloping row has L better rows that envelop the row in question as well, and "at least L better enveloping rows" equals "at
// least L better SURVIVING enveloping rows".  No iteration, no processing order: every row's fate is a count, which is what the
// kernels of lx_toprec.hip compute.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lx
{
namespace cull
{

// a better than b: order 2 (the places are the rows' places in order 1, distinct inside a segment)
__host__ __device__ inline bool better(double bs_a, uint32_t place_a, double bs_b, uint32_t place_b)
{
    return bs_a > bs_b || (!(bs_b > bs_a) && place_a < place_b);
}

// The query interval of a row on a query of q_len untranslated letters; false when it does not fit the query (an empty or inverted
// range, or one that ends behind the query's last letter) -- lo and hi are then not to be used.
__host__ __device__ inline bool interval(uint64_t q_start, uint64_t q_end, int q_frame, uint64_t q_len, bool translated, uint64_t & lo, uint64_t & hi)
{
    lo = hi = 0;
    if (q_start >= q_end || q_end > q_len) // (the second test also keeps 3 * q_end from overflowing)
        return false;
    uint64_t first = q_start, end = q_end; // 0-based [first, end) on the strand that was read
    if (translated)
    {
        uint64_t const shift = (uint64_t)(q_frame < 0 ? -q_frame : q_frame) - (q_frame != 0 ? 1 : 0);
        first = 3 * q_start + shift;
        end   = 3 * q_end + shift;
        if (end > q_len)
            return false;
    }
    if (q_frame < 0)
    {
        lo = q_len - end + 1;
        hi = q_len - first;
    }
    else
    {
        lo = first + 1;
        hi = end;
    }
    return true;
}

// b's interval envelops a's
__host__ __device__ inline bool envelops(uint64_t lo_b, uint64_t hi_b, uint64_t lo, uint64_t hi)
{
    return lo_b <= lo && hi <= hi_b;
}

} // namespace cull
} // namespace lx
