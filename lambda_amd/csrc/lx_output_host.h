// lx_output_host.h -- what the host writers (host/lx_output.cpp) and the record post-processing (host/lx_postprocess.cpp) offer the
// rest of the library.  HIP-free; not part of the ABI.
#pragma once
#include <string>
#include <vector>

#include "../../include/lambda_ext.h"
#include "lx_vocab.h"

struct lx_bytes;

namespace lxi
{

// (host/lx_output.cpp) an lx_bytes that takes over s; the message lx_last_output_error() returns
lx_bytes * bytes_adopt(std::string && s);
void       set_output_error(std::string const & msg);
// (host/lx_postprocess.cpp) the refusals of lx_cull_options for n rows in host memory (include/lambda_ext.h); `why` gets the text.
// max_len: the longest query the caller can take (the device forms keep the intervals in 32-bit words)
int cull_check(lx_blast_match const * m, uint64_t n, lx_cull_options const * opt, uint64_t max_len, std::string & why);

// What a writer's call asks for, resolved once (host/lx_output.cpp): by the host writers, and by the device writers (lx_bam_host.cpp,
// lx_text_host.cpp), which render the same bytes.
struct OutputRequest
{
    int               format = 0;
    lx_output_options opt{};                              // the caller's, or the defaults; LX_OUT_BAM: sam_with_ref_header = 1
    bool              is_n = false, q_trans = false, s_trans = false; // the program: BLASTN, a translated query, a translated subject
    bool              sam = false;                        // LX_OUT_SAM or LX_OUT_BAM: tags / tag_mask hold; else cols
    bool              tags[lx::kNumSamTags] = {};
    uint32_t          tag_mask = 0;                       // lx::tagBit of every tag
    std::vector<int>  cols;                               // kCol*, in the order asked for
    // LX_OUT_BLAST_TAB_COMMENTS: the constant parts of a query group's comment lines -- in front of the query's id, between the id and
    // the hit count, behind the count
    std::string m9[3];
};

// The LCA of a query's records from the options' (lca_qid, lca_tax) pairs, which are in list order, like the records: a cursor
// that only moves forward (no pairs: 0)
struct LcaCursor
{
    uint64_t at = 0;
    uint32_t of(lx_output_options const & opt, uint64_t n_qid)
    {
        while (at < opt.n_lca && opt.lca_qid && opt.lca_qid[at] != n_qid)
            ++at;
        return (at < opt.n_lca && opt.lca_qid && opt.lca_tax) ? opt.lca_tax[at] : 0u;
    }
};

// The refusals that need no look at a row, in the host writer's order: NULL names / rows / program, an unknown program, an unknown
// tag key or column specifier, for LX_OUT_BAM a subject of more than 2^31 - 1 letters (lx_last_output_error() has that text).  A format
// that is neither SAM nor BAM counts as tabular.
int resolve_output(int format, char const * program, lx_blast_match const * m, uint64_t n, lx_seq_names const * names,
                   lx_output_options const * opt_in, OutputRequest & rq);
// LX_EINVAL if a row names a query or a subject the name lists do not have; `text` (or none: NULL) becomes lx_last_output_error()
int check_rows(lx_blast_match const * m, uint64_t n, lx_seq_names const * names, char const * text);
// the SAM header text; the bytes in front of a BAM stream's records (magic, that text, the reference list)
std::string sam_header(lx_seq_names const * names, OutputRequest const & rq);
std::string bam_header(lx_seq_names const * names, OutputRequest const & rq);

} // namespace lxi
