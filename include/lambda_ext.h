/*
 * lambda_ext.h -- C ABI of the MI355X seed-extension engine (liblambda_ext.so).
 *
 * This is the drop-in boundary for lambda3's per-hit gapped extension.  The reference has no
 * FFI; its seam is the C++ template call
 *
 *     _performAlignment(depSetH, depSetV, blastMatches, lH, bool_constant<withTrace>, bsDirection)
 *         /root/reference/src/search_algo.hpp:1070-1076, called at :1246 (score) and :1296 (trace)
 *
 * whose inputs are N (query slice, subject slice) pairs plus the scoring scheme of the strand
 * direction, and whose outputs are alignmentScore per pair (:1129) or the gapped rows (:1127).
 * The entry points below replace exactly that call (lx_score_batch / lx_align_batch) and, one level
 * up, the whole of iterateMatchesFullSimd (:1177-1332) (lx_iterate_matches).  INTEGRATION.md shows
 * the reference-side binding.
 *
 * Conventions
 *   - residues are 1 byte each, already in the rank encoding the reference feeds to SeqAn
 *     (src/seqan2_to_biocpp.hpp:382-395): SeqAn AminoAcid order for proteins, BioC++ rank for
 *     match/mismatch-scored nucleotides, SeqAn Dna5 order in bisulfite mode.
 *   - query = horizontal / outer sequence, subject = vertical / inner (src/search_algo.hpp:1058-1059)
 *   - gap_open is SeqAn's scoreGapOpen, i.e. lambda's gapOpen + gapExtend (src/search_algo.hpp:226-230)
 *   - every function returns LX_OK (0) or a negative LX_E* code; lx_last_error() gives the text.
 *     The C++ wrapper (lambda_amd/csrc/host/lambda_ext.hpp) rethrows std::runtime_error, which is what
 *     the reference does on failure (src/search.cpp:98-125).
 *   - caller owns every buffer; nothing allocated here crosses the boundary.
 *   - a handle is bound to one device and one HIP stream; use one handle per host thread, as the
 *     reference uses one LocalDataHolder per OpenMP thread (src/search.cpp:379-381).
 *   - there is NO CPU fallback: if no gfx950 device / kernel image is usable every call fails loudly.
 */
#ifndef LAMBDA_EXT_H
#define LAMBDA_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LX_ABI_VERSION 3
#define LX_ALPH 32 /* matrix stride; alphabet_size <= 31, rank 31 is reserved as padding */

enum
{
    LX_OK        = 0,
    LX_EINVAL    = -1, /* bad argument                         */
    LX_ENODEV    = -2, /* no usable gfx950 device              */
    LX_ENOMEM    = -3, /* device or host allocation failed     */
    LX_EHIP      = -4, /* HIP runtime error                    */
    LX_EOVERFLOW = -5, /* workspace / output capacity exceeded */
    LX_ESTATE    = -6  /* call sequence error                  */
};

/* Scoring scheme of one strand direction: TScoreSchemeAlign, src/search_datastructures.hpp:360-365;
 * filled like prepareScoring(), src/search_algo.hpp:166-234. */
typedef struct lx_scoring
{
    int32_t alphabet_size;            /* number of valid ranks (27 aa, 5 nucleotide)              */
    int32_t gap_open;                 /* cost of the first gap character  (negative)               */
    int32_t gap_extend;               /* cost of each further gap character (negative)             */
    int32_t reserved;
    int8_t  matrix[LX_ALPH * LX_ALPH]; /* matrix[query_rank * 32 + subject_rank]                   */
} lx_scoring;

/* One (query slice, subject slice) pair = one element of depSetH/depSetV (src/search_algo.hpp:1056-1060). */
typedef struct lx_extension
{
    uint64_t q_off; /* byte offset of the query slice in the query residue buffer    */
    uint64_t s_off; /* byte offset of the subject slice in the subject residue buffer */
    uint32_t q_len;
    uint32_t s_len;
} lx_extension;

/* Result of the traceback pass: what _adaptTraceSegmentsTo + beginPosition/endPosition give
 * (src/search_algo.hpp:1127, :1032-1035) and what computeAlignmentStats derives (:1308). */
typedef struct lx_hsp
{
    int32_t score;
    int32_t q_begin, q_end; /* 0-based half-open, relative to the query slice   */
    int32_t s_begin, s_end; /* 0-based half-open, relative to the subject slice */
    int32_t n_ops;          /* alignment columns written to the ops buffer      */
    int32_t num_matches, num_mismatches, num_positives;
    int32_t num_gap_opens, num_gap_extensions;
    int32_t ops_shift;      /* the n_ops bytes start at ops_off[i] + ops_shift (the walk fills the slot back to front;
                               ops_shift = q_len + s_len - n_ops) */
} lx_hsp;

/* src/search_datastructures.hpp:46-61 */
typedef struct lx_match
{
    uint64_t qryId, subjId, qryStart, qryEnd, subjStart, subjEnd;
} lx_match;

typedef struct lx_handle lx_handle;

/* ---- lifetime ------------------------------------------------------------------------------- */
int          lx_abi_version(void);
/* Hash of the sources this library was compiled from (lambda_amd/build.py source_id()): lets a test or a deployment assert
 * that the binary matches the tree. */
char const * lx_build_id(void);
int          lx_device_count(void);
int          lx_create(int device_id, lx_handle ** out);
void         lx_destroy(lx_handle * h);
char const * lx_last_error(lx_handle const * h); /* h may be NULL: error of the failed lx_create */

/* Tuning knobs.  They never change results, only which kernel geometry is launched:
 *   LX_OPT_MAX_QLEN        longest query slice the *_dev calls will see (0 = unknown -> generic geometry)
 *   LX_OPT_QUERY_RUN       promise for the *_dev calls: extensions come in runs of this many consecutive entries
 *                          that share one query slice (a multiple of 8, or 4 for the multi-query sweep; 0 = no promise).  Lets a wavefront
 *                          build one LDS profile instead of one per extension.  2 = the multi-query sweep's free packing:
 *                          entries 2k and 2k + 1 share a query slice and every aligned block of 16 entries holds windows of
 *                          at most four query slices, in any split (what lx_extend_batch streams a ragged list into).  1 = the
 *                          sweep's SOLO packing: no promise at all, every window has its own byte profile, 16 windows per
 *                          wavefront -- for the schemes whose profiles are small enough (nucleotide, bisulfite; what
 *                          lx_extend_batch and the Level-2 driver plan read sets with).  A violated promise is detected on
 *                          the device and reported as LX_ESTATE by lx_synchronize().
 *   LX_OPT_WORKSPACE_BYTES carry workspace for queries wider than one panel in the *_dev calls (default 64 MiB; with
 *                          LX_OPT_MAX_SLEN set it grows by itself to 8 bytes per subject row of the batch)
 *   (LX_OPT_BS_MATCH_RULE is the one option that is not a tuning knob: it selects which of the reference's two
 *   computeAlignmentStats overloads the pass-2 match counts follow.) */
enum
{
    LX_OPT_MAX_QLEN        = 1,
    LX_OPT_QUERY_RUN       = 2,
    LX_OPT_WORKSPACE_BYTES = 3,
    LX_OPT_MAX_SLEN        = 4, /* longest subject slice the *_dev calls will see (0 = unknown: measured on the
                                   device, which costs lx_align_batch_dev one stream synchronisation)          */
    LX_OPT_TRACE_BYTES     = 5, /* HBM budget for direction bits in pass 2 (default 64 GiB); larger batches are
                                   processed in chunks, in order, on the same stream                            */
    LX_OPT_BS_MATCH_RULE   = 6, /* 1: lx_hsp match counts use the bisulfite rule score(c0,c1)==score(c0,c0)
                                   (src/evaluate_bisulfite_alignment.hpp:97) instead of rank equality        */
    LX_OPT_PACKED_HALF     = 7, /* 1 (default): the packed kernels (two extensions per lane group: half precision, or
                                   16-bit integers for wider queries) run where a per-wavefront score bound proves them
                                   exact (results are bit-identical either way); 0: int32 kernels only */
    LX_OPT_PASS2_MODE      = 8, /* how pass 2 keeps what the traceback needs (results are bit-identical in every mode):
                                   0 = 4 direction bits per cell of every survivor;
                                   1 = strip boundaries + row checkpoints of every survivor, tiles recomputed by the
                                       backtrace -- where its limits hold (extensions in blocks of >= 4 per query,
                                       scores below 32000; queries of any width, panel by panel), else mode 0;
                                   2 (default) = single sweep in lx_extend_batch_dev: one checkpointing kernel over ALL
                                       extensions is pass 1 and the forward half of pass 2 at once -- where mode 1
                                       applies, LX_OPT_QUERY_RUN is a multiple of 8 and the checkpoints of the whole
                                       batch (7.7 KB per 150 x 176 extension as compact codes of the packed-half kernel,
                                       13.5 KB as int16 pairs) fit LX_OPT_TRACE_BYTES, else mode 1 */
    LX_OPT_EXTEND_CHUNK    = 10, /* extensions per chunk of lx_extend_batch's pipeline (0 = default, ~640 k; at least 1024):
                                   smaller chunks start returning results earlier, larger ones amortise the per-chunk launches */
    LX_OPT_MQ_SWEEP        = 11, /* multi-query single sweep (ragged seed lists: up to four queries per wavefront, byte profiles
                                   in LDS): 1 (default) = where LX_OPT_QUERY_RUN is 2, 4 or 8 -- 2 is what lx_extend_batch
                                   makes of a list whose queries have few windows each; 2 = for every run that is a multiple
                                   of 4; 0 = never (runs of 8 / 16 on the one-query-per-wavefront kernels).  Needs what the
                                   single sweep needs and a scheme in which no substitution costs more than a gap's first
                                   character (every scheme of the reference with its default gap costs) */
    LX_OPT_ADAPT_PERMILLE  = 12, /* adaptive pass 2 (with LX_OPT_PASS2_MODE = 2): when fewer than this many per mille of the previous
                                   batch's extensions passed the cut-off, the step runs plain pass 1 and writes checkpoints for
                                   the survivors only (mode 1) instead of checkpoints for every window -- the reference's own
                                   order, src/search_algo.hpp:1246 / :1251-1283 / :1296; default 30, 0 = always the single sweep.
                                   Results are identical either way */
    LX_OPT_ITERATE_RECORDS = 13, /* where lx_iterate_matches_dev (and lx_iterate_matches on lists it hands to the device) makes the result
                                   records behind the two passes (src/search_algo.hpp:1287-1325: statistics, order, identity cut-off, bit
                                   score, e-value): 0 (default) = kernels on the survivors where the backtrace left them, finished rows come
                                   down in one copy; 1 = the host threads, from the survivors' alignments (rounds 1-4).  The records are the
                                   same to the bit either way (tests/test_gpu_level2.py) */
    LX_OPT_HOST_THREADS    = 14, /* parts the host loops of the host-buffer entry points and of the Level-2 driver are cut into (= the host
                                   threads that can work on one loop).  PROCESS-WIDE, whichever handle it is set through: the library keeps
                                   ONE set of host threads, and the loops of all handles -- one handle per host thread is the intended use,
                                   as the reference keeps one LocalDataHolder per OpenMP thread, src/search.cpp:379-385 -- share them part
                                   by part, side by side.  0 (default) = min(CPU affinity mask, cgroup CPU quota) / LOCAL_WORLD_SIZE (the
                                   ranks of a node, one process per GPU, share its CPUs), at most 16; at most 64.  Never changes results */
    LX_OPT_GUNZIP_CHUNK    = 15, /* lx_gunzip, plain members on the device: compressed bytes per chunk (0 = default, 64 KiB; accepted
                                    from 32 KiB to 4 MiB).  Like the next it changes where the work runs, never the result */
    LX_OPT_GUNZIP_PARALLEL_FROM = 16, /* lx_gunzip: DEFLATE bytes left in the input from which a plain member takes the device path
                                         (0 = default, 8 MiB: above the measured crossover against the host thread; UINT64_MAX = never).  The input behind a
                                         header may be many small members, so the host tries the first 64 KiB (or this many bytes,
                                         if fewer) itself and keeps a member that ends inside them */
    LX_OPT_BAM_RANGE_BYTES = 17, /* lx_render_bam_dev / lx_write_bam_dev and lx_render_text_dev / lx_write_text_dev: rendered bytes per
                                    range of records, i.e. what stands on the device at once (0 = default, 256 MiB; accepted from 128 KiB to 2 GiB; a range is whole tiles of 2048 records,
                                    at least one).  It changes where the cuts fall, never a byte of the output */
    LX_OPT_INDEX_SLICE_WORDS = 18, /* lx_index_build on a handle: 0 (default) = one radix sort over all words (fewer than 2^31 of them, about
                                      72 bytes of device memory per word at once); N >= 1 = the build in slices of the key space of at most
                                      N words each (lx_index_plan_slices), for sets of fewer than 2^32 - 1 words: 16 bytes per word for the
                                      entries and 32 per word of the largest slice.  The same table entry for entry either way */
    LX_OPT_LCA_RANGE_ROWS  = 19, /* lx_compute_lca_dev: rows per range of whole queries, i.e. what stands on the device at once (0 = default,
                                    2^24; a query with more rows is a range of its own).  It changes where the cuts fall, never a result */
    LX_OPT_BAND            = 9 /* band mode -- NOT the reference's configuration (src/search_algo.hpp:1081 runs BandOff, :1102
                                   says why; _bandSize only pads the window, src/search_misc.hpp:46-50) and therefore not a
                                   parity mode: 0 (default) = full rectangle; b > 0 = only cells whose diagonal i - j (row i of
                                   the subject slice, column j of the query slice, 0-based) lies within b of the extension's
                                   centre diagonal exist, as in a banded SeqAn alignment: cells off the band are never
                                   computed, no gap runs through them.  Centres: lx_set_band_centres[_dev]; without them
                                   min(_bandSize(q_len), s_len - q_len), the seed diagonal of a window built by _widenMatch
                                   that was not clipped at the subject's start.  Applies to every score / align / extend entry
                                   point; runs int32 kernels and direction bits (results are those of the oracle's
                                   lxo_score_banded / lxo_align_banded).  PERFORMANCE: band mode exists for its semantics only --
                                   it is SLOWER per window than the full rectangle (headline batch: 51 ms per step with b = 64
                                   against 15.7 ms without a band): at 150 x 176 with b = 64 the band removes 27 % of the cells and
                                   no step of the strip mapping, and every remaining cell pays for its mask.  A caller who wants
                                   throughput leaves the band off, which is also what the reference computes */
};
int lx_set_option(lx_handle * h, int option, uint64_t value);
/* The host threads as the library sized them (no handle, no device needed): parts per loop (LX_OPT_HOST_THREADS or the default),
 * the CPUs granted to the process (affinity mask and cgroup quota), LOCAL_WORLD_SIZE as read from the environment.  Any pointer
 * may be NULL. */
int lx_host_threads_info(uint32_t * width, uint32_t * granted_cpus, uint32_t * local_world_size);

/* Introspection, no device needed: how lx_extend_batch_dev would run a batch of n extensions of queries up to max_qlen and
 * windows up to max_slen under the given options (the LX_OPT_* of the same names; survivor_share < 0 = unknown).  The
 * library decides this in ONE function; this entry point shows its answer, and tests/test_plan.py walks it over query
 * widths, run lengths and schemes.  family: 0 = no sweep (pass 1, then pass 2 on the survivors), 1 = packed-half sweep,
 * 2 = packed-int16 sweep with compact codes over several panels, 3 = packed-int16 sweep with int16-pair slots, 4 = int32 sweep,
 * 5 = multi-query sweep (byte profiles).  name = what lx_last_trace_kernel_name() reports after such a step. */
typedef struct lx_step_plan
{
    int32_t  family, group_lanes, strip_cols, panels;
    int32_t  compact_codes, queries_per_wavefront, may_decline, adapted;
    uint64_t slot_bytes;  /* checkpoint bytes per extension */
    uint64_t lds_bytes;   /* LDS of one wavefront of the sweep kernel */
    uint64_t score_bound; /* a-priori bound of every intermediate for the widest admitted query */
    char     name[160];
} lx_step_plan;
int lx_plan_step(lx_scoring const * sc, uint64_t max_qlen, uint64_t max_slen, uint64_t query_run, uint64_t n, uint64_t pass2_mode,
                 uint64_t mq_sweep, uint64_t packed_half, uint64_t trace_bytes, double survivor_share, uint64_t adapt_permille,
                 lx_step_plan * out);
/* current value of an option (what the caller set or the default; never the library's internal growth of a workspace) */
int lx_get_option(lx_handle const * h, int option, uint64_t * value);

/* Band mode (LX_OPT_BAND > 0): centre diagonal of every extension of the NEXT host-buffer call, diag[i] for ext[i] (n must
 * equal that call's n; diag = NULL, n = 0 returns to the default centres).  The *_dev calls read a device array of int32,
 * one per extension, that must stay valid while they run (NULL = default centres). */
int lx_set_band_centres(lx_handle * h, int32_t const * diag, uint64_t n);
int lx_set_band_centres_dev(lx_handle * h, void const * d_diag);

/* slot 0 = forward scheme, slot 1 = bisulfite reverse scheme (scoringSchemeAlignBSRev,
 * src/search_algo.hpp:1097-1098).  Must be called before any batch call using that slot. */
int lx_set_scoring(lx_handle * h, int slot, lx_scoring const * sc);

/* Fills *sc with a built-in scheme the way prepareScoring() does: scoring_method 45/62/80 = BLOSUM
 * (protein), 0 = match/mismatch (nucleotide), -1 = bisulfite forward, -2 = bisulfite reverse.
 * gap_open_lambda / gap_extend are lambda's options (e.g. -11/-1), NOT SeqAn's. */
int lx_builtin_scoring(int scoring_method, int match, int mismatch, int gap_open_lambda, int gap_extend,
                       lx_scoring * sc);

/* ---- resident subjects -------------------------------------------------------------------------------------------
 * The subject sequences of a search do not change between query batches (the reference holds them in its index file,
 * src/shared_definitions.hpp:343-379).  lx_set_subjects uploads the (frame-expanded, rank-encoded) subject residues
 * once; afterwards every host-buffer call (lx_score_batch, lx_align_batch, lx_prefilter_batch, lx_iterate_matches)
 * may pass s_res = NULL, s_bytes = 0 to use the resident copy instead of uploading its own.  s_bytes = 0 drops it. */
int lx_set_subjects(lx_handle * h, uint8_t const * s_res, uint64_t s_bytes);

/* ---- pass 1: score only  (replaces _performAlignment<false>, src/search_algo.hpp:1246) ------- */
/* Host buffers in, host buffers out; copies through pinned staging, runs on the handle's stream, returns
 * after the results have landed. out_score[i] is what the reference stores at :1129. */
int lx_score_batch(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res,
                   uint64_t s_bytes, lx_extension const * ext, uint64_t n, int32_t * out_score);

/* Device-resident variant: every pointer is a device pointer on the handle's device; asynchronous on
 * `stream` (a hipStream_t; NULL = the handle's own stream).  This is what bench.py times.
 * The residue buffers must start 16-byte aligned (hipMalloc's do) and keep 256 readable bytes after the last
 * residue: the kernels fetch residues in aligned groups. */
int lx_score_batch_dev(lx_handle * h, int slot, void const * d_q_res, void const * d_s_res, void const * d_ext,
                       uint64_t n, void * d_out_score, void * stream);

/* ---- pass 2: traceback  (replaces _performAlignment<true>, src/search_algo.hpp:1296) --------- */
/* LIMIT: pass 2 (lx_align_batch*, and the second half of every lx_extend_batch* / lx_iterate_matches call) needs every
 * (matrix entry - gap_extend) of the slot's scheme in [-31, 31] -- the tagged recurrence keeps two tag bits next to values
 * scaled by 4 in 8-bit profile entries, there is no int32 fall-back for it.  Every scheme of the reference with its default
 * costs satisfies this (BLOSUM45/62/80 with gap_extend -1 ... -2, +2/-3 nucleotide and bisulfite matrices); a user-chosen
 * --match / --mismatch beyond that range (src/search_options.hpp:93-94) makes these calls return LX_EINVAL with that text.
 * Pass 1 (lx_score_batch*) has no such limit.
 * ops: one byte per alignment column ('M','D','I'; 'D' = gap in the query row), begin -> end order.  The caller gives
 * extension i a slot of q_len+s_len bytes at out_ops + ops_off[i]; its out_hsp[i].n_ops bytes are written at the END
 * of that slot, i.e. they start at out_ops + ops_off[i] + out_hsp[i].ops_shift. */
int lx_align_batch(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res,
                   uint64_t s_bytes, lx_extension const * ext, uint64_t n, int32_t const * known_score, lx_hsp * out_hsp,
                   uint8_t * out_ops, uint64_t const * ops_off);
/* known_score: NULL, or the pass-1 score of every extension (the reference runs pass 2 on survivors of pass 1, so the
 * caller has them): pass 2 locates the end cell through the best score and computes it itself when not given.  A wrong
 * score is detected (LX_EOVERFLOW), never turned into a wrong alignment.  Extensions of one query should be adjacent
 * (lambda's lists are): runs of the same query slice then share one LDS profile. */

int lx_align_batch_dev(lx_handle * h, int slot, void const * d_q_res, void const * d_s_res, void const * d_ext,
                       uint64_t n, void * d_out_hsp, void * d_out_ops, void const * d_ops_off, void * stream);

/* ---- both passes fused on the device (the middle of iterateMatchesFullSimd, src/search_algo.hpp:1246-1296) --- */
/* pass 1 on all n extensions -> keep extension i iff score >= (d_min_score ? d_min_score[i] : min_score_all) [the
 * bit-score / e-value tests of :1251-1283 expressed as integer score cut-offs, which the host derives from
 * lx_evalue()/lx_bitscore(); both are monotone in the score] -> pass 2 on the survivors.  Nothing leaves the GPU and
 * nothing synchronises: d_out_score[n] (int32), d_out_hsp[n] (lx_hsp; filtered-out rows carry the score and n_ops = 0),
 * ops of extension i at d_out_ops + d_ops_off[i], d_out_count[0] = pass-2 slots used, [1] = survivors (uint64).
 * Requires LX_OPT_MAX_QLEN and LX_OPT_MAX_SLEN; honours LX_OPT_QUERY_RUN. */
int lx_extend_batch_dev(lx_handle * h, int slot, void const * d_q_res, void const * d_s_res, void const * d_ext,
                        uint64_t n, void const * d_min_score, int32_t min_score_all, void * d_out_score,
                        void * d_out_hsp, void * d_out_ops, void const * d_ops_off, void * d_out_count, void * stream);

/* The same on host buffers (what lx_iterate_matches uses).  Extension order is free; extensions of one query slice are
 * best adjacent (lambda's lists are).  out_score[n] as in pass 1; out_hsp[n]: filtered-out rows carry the score and
 * n_ops = 0; the ops of a survivor i are *out_ops + out_ops_off[i] + out_hsp[i].ops_shift (the callee lays them out
 * compactly; the buffer belongs to the handle and stays valid until its next lx_extend_batch[_rle] call).  The list is
 * processed as a pipeline of chunks (uploads, kernels, downloads and the host's share overlap); only scores, the
 * survivors' records and their run-length coded ops cross PCIe.  A list that is not uniform -- what
 * _widenAndPreprocessMatches really hands over: queries of mixed lengths, a few windows each, merged windows of up to three
 * times the length (:1136-1175) -- is planned for the multi-query sweep (LX_OPT_MQ_SWEEP): a wavefront's 16 slots hold windows
 * of up to four queries, the long (merged) windows of the list pooled in sub-blocks of 4 and dealt by length, the others
 * streamed pair by pair in order of length; the records are gathered from a device copy of the list and the scores scattered
 * back into the caller's order on the device.  lx_last_extend_stats() reports extensions,
 * slots, cells and the cells the wavefronts executed (padding included) of the last call.
 * Throughput depends on the batch size -- a call has a fixed cost of ~0.7 ms (INTEGRATION.md has the curve): hand over the
 * windows of at least ~1 000 queries per call. */
int lx_extend_batch(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                    lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                    lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes);

/* The same with the ops in the form they cross PCIe in: run-length codes instead of one byte per column -- one byte per run,
 * (op << 6) | (length - 1) with op 0 = 'M', 1 = 'D', 2 = 'I', runs longer than 64 columns split (the remainder first, then
 * pieces of 64: one alignment has one code string), begin -> end order.  The codes
 * of a survivor i start at *out_ops + out_ops_off[i] and end where their lengths add up to out_hsp[i].n_ops (the number of
 * alignment columns, as ever); out_hsp[i].ops_shift is 0.  This is what a binding that fills SeqAn's gapped rows wants (ArrayGaps
 * stores run lengths) and what lx_iterate_matches uses; lx_expand_ops turns one survivor's codes into column bytes. */
int lx_extend_batch_rle(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                        lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                        lx_hsp * out_hsp, uint64_t * out_ops_off, uint8_t const ** out_ops, uint64_t * out_ops_bytes);
int lx_expand_ops(uint8_t const * codes, int32_t n_ops, uint8_t * out /* n_ops bytes */);

/* The same with the result in the form the reference's filter loop leaves behind: it ERASES the matches that fail the
 * e-value / bit-score test from its list (src/search_algo.hpp:1251-1283) and goes on with the survivors only (:1287-1385).
 * out_score[n] as ever (the filter's statistics need every score); the survivors come back as a list -- position in the
 * caller's list, record, run-length codes as lx_extend_batch_rle -- in buffers that belong to the handle and stay valid
 * until its next lx_extend_batch* call.  The order of the list is the order the device finished the chunks in (ascending
 * positions for a list that is grouped by query and uniform; otherwise grouped by chunk): `index` says which row is whose.
 * This is the fastest host entry point: nothing of size n except the scores is written on the host (lx_extend_batch fills
 * n records of 48 bytes, which at millions of extensions per call costs as much as the kernels). */
typedef struct lx_survivor_list
{
    uint64_t         count;
    uint32_t const * index;       /* [count] position in the caller's list                                            */
    lx_hsp const *   hsp;         /* [count] ops_shift = 0                                                            */
    uint64_t const * codes_off;   /* [count] the codes of survivor k start at codes + codes_off[k] and end where their
                                     lengths add up to hsp[k].n_ops                                                   */
    uint8_t const *  codes;
    uint64_t         codes_bytes;
} lx_survivor_list;
int lx_extend_batch_list(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res, uint64_t s_bytes,
                         lx_extension const * ext, uint64_t n, int32_t const * min_score, int32_t min_score_all, int32_t * out_score,
                         lx_survivor_list * out);
/* Padding of the last lx_extend_batch* call: out4 = {extensions with residues, slots (windows + fillers), cells (sum q_len *
 * s_len), cells the wavefronts execute (per wavefront: 16 slots x the columns its widest query sweeps -- whole panels, the last
 * one with narrower strips where that covers the query -- x the steps of its longest window)}. */
int lx_last_extend_stats(lx_handle const * h, uint64_t * out4);

/* ---- pre-extension filter (seedLooksPromising, src/search_algo.hpp:426-481) ------------------ */
/* One diagonal per item; out_keep[i] = 1 if the ungapped max-segment score reaches the threshold.  LX_EINVAL, before any kernel runs
 * and with the handle as usable as before: a seed with qry_end < qry_start, qry_end > q_len or subj_start + (qry_end - qry_start) >
 * s_len, a sequence that does not lie inside q_bytes / s_bytes, and -- unlike the other batch calls, which say LX_ESTATE -- a scoring
 * slot that is not set. */
typedef struct lx_seed
{
    uint64_t q_off, s_off; /* start of the whole (frame) query / subject sequence */
    uint32_t q_len, s_len; /* their full lengths                                 */
    uint32_t qry_start, qry_end, subj_start, reserved;
} lx_seed;
int lx_prefilter_batch(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint8_t const * s_res,
                       uint64_t s_bytes, lx_seed const * seeds, uint64_t n, uint32_t seed_length,
                       int32_t pre_scoring, double pre_scoring_thresh, uint8_t * out_keep);


/* ---- host mirror of the extension driver (one level above the two passes) ---------------------------- */
/* Karlin-Altschul parameters of a scoring scheme (seqan::BlastScoringScheme; call sites src/search_misc.hpp:73-78,
 * src/search_algo.hpp:1258).  Tables are NCBI's published values; returns LX_EINVAL for combinations that have
 * none, which is what makes prepareScoring() throw (src/search_algo.hpp:232-233). */
typedef struct lx_karlin
{
    double lambda, K, H, alpha, beta;
} lx_karlin;
int      lx_karlin_params(int scoring_method, int match, int mismatch, int gap_open_lambda, int gap_extend, lx_karlin * out);
uint64_t lx_length_adjustment(uint64_t db_len, uint64_t q_len, lx_karlin const * ka);
double   lx_evalue(int32_t score, uint64_t q_len_adj, uint64_t db_len_adj, lx_karlin const * ka);
double   lx_bitscore(int32_t score, lx_karlin const * ka);

/* Rank bridge (seqan2_to_rank_inner / biocpp_rank_to_seqan2rank, src/seqan2_to_biocpp.hpp:352-366, :382-395): turns
 * n BioC++ ranks into the ranks the scoring tables of this library are indexed by.  in == out is allowed.
 *   LX_RANKS_AA27      aa27 (A..W, X, Y, Z, '*')  ->  SeqAn AminoAcid order (.. W, Y, Z, X, '*')
 *   LX_RANKS_DNA5_BS   dna5 (A, C, G, N, T)       ->  SeqAn Dna5 order (A, C, G, T, N); bisulfite mode only
 *   LX_RANKS_SIMPLE    alphabets scored by match/mismatch keep their BioC++ rank (plain copy)
 * Returns LX_EINVAL for an unknown kind or a rank outside the alphabet. */
enum
{
    LX_RANKS_AA27    = 0,
    LX_RANKS_DNA5_BS = 1,
    LX_RANKS_SIMPLE  = 2
};
int lx_convert_ranks(int kind, uint8_t const * in, uint64_t n, uint8_t * out);

/* _widenAndPreprocessMatches (src/search_algo.hpp:1136-1175), in place; qlens/slens are indexed by the
 * frame-expanded qryId/subjId.  Returns the new match count. */
uint64_t lx_widen_and_preprocess(lx_match * m, uint64_t n, uint64_t const * qlens, uint64_t const * slens);

/* Options of iterateMatchesFullSimd that live in LambdaOptions / the BLAST context. */
typedef struct lx_search_params
{
    double    max_evalue;       /* < 0: no e-value filter   (src/search_options.hpp:96-97)          */
    int32_t   min_bitscore;     /* < 0: no bit-score filter                                           */
    int32_t   id_cutoff;        /* percent identity cut-off (src/search_algo.hpp:1310-1315)           */
    uint64_t  db_total_length;  /* context.dbTotalLength    (src/search_algo.hpp:317-319)             */
    int32_t   query_translated; /* 1: ql /= 3 before the length adjustment (src/search_misc.hpp:70)   */
    int32_t   qry_num_frames;   /* qryId / qry_num_frames = true query id (src/search_algo.hpp:1210)  */
    int32_t   sbj_num_frames;
    int32_t   bisulfite;        /* 1: iterateMatches' bisulfite branch (src/search_algo.hpp:1367-1379): matches on even subject
                                   frames are extended with slot 0 (forward scheme), odd ones with slot 1 (reverse scheme);
                                   the `slot` argument is ignored; match counts / identity follow the bisulfite overload of
                                   computeAlignmentStats (score(c0,c1)==score(c0,c0), src/evaluate_bisulfite_alignment.hpp:97)
                                   for this call whatever LX_OPT_BS_MATCH_RULE says                                         */
    int32_t   q_frame_mode;     /* LX_FRAMES_*: how _setFrames derives qFrameShift from the frame-expanded qryId            */
    int32_t   s_frame_mode;     /* same for sFrameShift / subjId                                                            */
    lx_karlin karlin;
    int32_t   band;             /* 0: full rectangle, what the reference computes; b > 0: band mode (LX_OPT_BAND) with the default
                                   centres for the duration of the call -- not a parity mode                               */
    int32_t   flags;            /* LX_ITERATE_*; 0 = the reference's behaviour                                                     */
} lx_search_params;
/* lx_search_params.flags: the result carries no alignment columns -- lx_iterate_result_ops() is NULL, every record's n_ops is still the
 * alignment's length and ops_off is 0.  For callers whose output needs none (BLAST-tabular: every column comes from the counts; the
 * SAM writer needs them for its CIGAR): a million HSPs are 110 MB of column bytes that nobody reads. */
#define LX_ITERATE_NO_OPS 1

/* ---- frame bookkeeping (_setFrames, _untrueQryId, _untrueSubjId; src/search_algo.hpp:768-814, :940-996) ------------
 * The reference expands every sequence into its frames (translate_join: 6, add_reverse_complement: 2, bisulfite
 * query: 4 / subject: 2; src/shared_definitions.hpp:246-281) and numbers them id * numFrames + k.  The mode says
 * which expansion a side uses:
 *   LX_FRAMES_NONE        frame 0                                        (protein sequences)
 *   LX_FRAMES_REVCOMP     k = 0 -> +1, k = 1 -> -1                       (blastn query)
 *   LX_FRAMES_TRANSLATED  k = 0..2 -> +1..+3, k = 3..5 -> -1..-3         (blastx / tblastx query, tblastn / tblastx subject)
 *   LX_FRAMES_BISULFITE   query: k = 0..3 -> +1, +2, -1, -2;  subject: k = 0, 1 -> +1, +2 */
enum
{
    LX_FRAMES_NONE       = 0,
    LX_FRAMES_REVCOMP    = 1,
    LX_FRAMES_TRANSLATED = 2,
    LX_FRAMES_BISULFITE  = 3
};
void     lx_set_frames(int q_mode, int s_mode, uint64_t qry_id, uint64_t subj_id, int32_t * q_frame, int32_t * s_frame);
/* the frame-expanded id whose sequence an HSP with this frame was aligned on (the bisulfite duplicates are identical
 * sequences, so the reference maps them onto the first copy) */
uint64_t lx_untrue_qry_id(int q_mode, uint64_t n_qid, int32_t q_frame);
uint64_t lx_untrue_subj_id(int s_mode, uint64_t n_sid, int32_t s_frame);

/* Six-frame translation (what bio::views::translate_join hands to the extension in the translated programs,
 * src/shared_definitions.hpp:246-281): `dna5` holds n BioC++ dna5 ranks (A, C, G, N, T).  Writes the frames
 * +1, +2, +3, -1, -2, -3 back to back into `out` (SeqAn AminoAcid ranks; 2n bytes are always enough) and their
 * offsets/lengths into frame_off/frame_len.  A codon with N becomes the amino acid all its completions agree on,
 * else X.  genetic_code: an NCBI translation table id as bio::alphabet::genetic_code numbers them (1 = canonical, the
 * reference's default, src/search_options.hpp:170; 2-6, 9-16, 21-25).  Returns LX_EINVAL for other ids, bad ranks or a
 * too small `out`. */
int lx_translate_six_frames(uint8_t const * dna5, uint64_t n, int genetic_code, uint8_t * out, uint64_t out_capacity,
                            uint64_t * frame_off, uint64_t * frame_len);

/* One finished HSP: the fields of TBlastMatch the writers read (src/search_datastructures.hpp:470-484). */
typedef struct lx_blast_match
{
    uint64_t qry_id, subj_id;   /* frame-expanded ids of the lx_match this HSP came from */
    uint64_t n_qid, n_sid;      /* true ids (_n_qId/_n_sId)                              */
    uint64_t q_start, q_end;    /* in the (frame) query sequence, 0-based half-open      */
    uint64_t s_start, s_end;    /* in the (frame) subject sequence                       */
    int32_t  score;
    int32_t  alignment_length;
    int32_t  num_matches, num_mismatches, num_positives, num_gap_opens, num_gap_extensions;
    float    identity;
    double   bit_score, e_value;
    uint64_t ops_off;           /* into the result's ops buffer */
    uint32_t n_ops;
    int16_t  q_frame;           /* qFrameShift (lx_set_frames): 0 = none, +-1 strands, +-1..3 translation frames */
    int16_t  s_frame;           /* sFrameShift                                                                    */
} lx_blast_match;

typedef struct lx_iterate_stats
{
    uint64_t hits_duplicate, failed_bitscore, failed_evalue, failed_identity, num_ext_score, num_ext_ali;
} lx_iterate_stats;

typedef struct lx_iterate_result lx_iterate_result;

/* iterateMatchesFullSimd (src/search_algo.hpp:1177-1332) for one strand direction: widen/merge the seed hits,
 * score every window on the GPU, filter by bit score / e-value, trace the survivors on the GPU, expand to
 * sequence coordinates, apply the identity cut-off.  q_seq_off/q_seq_len (s_*) give, per frame-expanded sequence
  * id, where that sequence lives in q_res (s_res).  q_orig_len[n_qid] is the untranslated query length used for
 * the e-value (bm.qLength, src/search_algo.hpp:1213).  `matches` is modified in place (like the reference's span). */
/* Lists of 131 072 matches and more (at most 2^31 - 16) over resident subjects are handed to the Level-2 kernels (lx_iterate_matches_dev's
 * path): same records and statistics; two differences a caller can see -- a seed on a diagonal beyond its subject's end is LX_EINVAL there
 * (the host form widens it to an empty window), and after a bisulfite call `matches[0 .. windows)` holds the window list contiguously (even
 * subject frames first), where the host form leaves its two halves where the sort put them. */
int lx_iterate_matches(lx_handle * h, int slot, uint8_t const * q_res, uint64_t q_bytes, uint64_t const * q_seq_off,
                       uint64_t const * q_seq_len, uint64_t n_qseq, uint64_t const * q_orig_len,
                       uint8_t const * s_res, uint64_t s_bytes, uint64_t const * s_seq_off, uint64_t const * s_seq_len,
                       uint64_t n_sseq, lx_match * matches, uint64_t n_matches, lx_search_params const * params,
                       lx_iterate_result ** out);

/* The same for matches that stand in DEVICE memory -- where a seeding stage on the GPU leaves them -- over sequence sets that are
 * resident on the handle's device: _widenMatch (src/search_algo.hpp:919-938), the sort, both merge passes and unique of
 * _widenAndPreprocessMatches (:1136-1175), the slices (:1200-1227) and the filter's cut-offs (:1251-1283) run as kernels; only the
 * finished window list (24 bytes per window) comes down for the plan of the sweep, the extension reads list and cut-offs where the
 * kernels wrote them.  Results are lx_iterate_matches' (same order, same records, same statistics).
 *   lx_set_queries       the (frame-expanded) query set: residues, where each sequence lies, q_orig_len[n_qseq / qry_num_frames]
 *                        (NULL: the sequences' own lengths) -- what lH.transQrySeqs / qrySeqs are to the reference's thread;
 *                        replaces the previous set; nothing of the caller's is referenced after the call returns
 *   lx_set_subjects      the subject residues (above), lx_set_subject_seqs where each (frame) subject lies in them
 *   d_matches            n_matches lx_match records in device memory of the handle's device, finished before the call (the call
 *                        runs on the handle's stream); not modified
 * params->qry_num_frames must be the value the queries were set with; params->band is not served here (lx_iterate_matches).
 * LX_EINVAL: a match names a sequence outside the sets or lies beyond its subject's end. */
int lx_set_queries(lx_handle * h, uint8_t const * q_res, uint64_t q_bytes, uint64_t const * q_seq_off, uint64_t const * q_seq_len, uint64_t n_qseq,
                   uint64_t const * q_orig_len, int32_t qry_num_frames);
int lx_set_subject_seqs(lx_handle * h, uint64_t const * s_seq_off, uint64_t const * s_seq_len, uint64_t n_sseq);
int lx_iterate_matches_dev(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params,
                           lx_iterate_result ** out);
/* Introspection: the plan lx_iterate_matches_dev makes for a PROTEIN window list -- the multi-query sweep's free packing (LX_OPT_QUERY_RUN
 * = 2: the two windows of a lane group share a query slice, a wavefront's 16 slots hold windows of at most four slices) -- for a list
 * of n lx_extension records in device memory that is grouped by query slice, as kernels (what the reference does with its sort by slice
 * lengths, src/search_algo.hpp:1229-1235, so that a SIMD batch's windows take about as many steps), brought to the host.
 * strip_cols: 19, 13 or 11 (columns per lane of a strip).  Ranges: cut[0] = 0 < ... < cut[nranges] = n, every cut where the query
 * changes; the plan's wavefronts are laid out range by range.  out_plan: [bound * 16] slots -- position in the list, bit 31 = filler (a
 * copy that never survives), 0xffffffff beyond the plan's wavefronts --, out_pan / out_maxs: [bound] columns per lane of a wavefront's
 * widest query / its longest window, bound = lx_plan_free_packing_bound(n, n_qseq, nranges); out_report: [16] = {wavefronts, error
 * flag (0), runs, quads of the pool, first wavefront of range 0, 1, ..., nranges}.  n_qseq: the number of query slices in the list, or
 * more; a list with more runs than that allows (it is not grouped by query slice, or n_qseq is too small) and any other non-zero
 * flag are LX_ESTATE with a text, the outputs then hold no plan.  tests/test_gpu_plan.py checks every slot against these promises,
 * tests/test_gpu_plan_edges.py against a sequential model of the plan's rules. */
uint64_t lx_plan_free_packing_bound(uint64_t n, uint64_t n_qseq, uint32_t nranges);
int      lx_plan_free_packing_dev(lx_handle * h, void const * d_ext, uint64_t n, uint64_t n_qseq, int32_t strip_cols, uint32_t nranges, uint64_t const * cut,
                                  uint32_t * out_plan, uint32_t * out_pan, uint32_t * out_maxs, uint32_t * out_report);
/* The library's own radix sort (least significant digit first, 8 bits per pass; stable) for n (key, value) word pairs in device memory.
 * key_bits is a bit MASK, not a number of bits: there is one pass for every 8-bit digit (bits 8k .. 8k+7) in which key_bits has any bit
 * set, and that pass sorts by the WHOLE digit, so the words end up ordered by key & (the 0xff bytes key_bits touches), equal ones in
 * their input order; key_bits == 0 sorts nothing.  key[0] / value[0] hold the input, key[1] / value[1] are scratch of the same size;
 * *sorted_in says which of the two holds the sorted words afterwards (the number of passes modulo 2).  Synchronises `stream`; the
 * caller's current device is left as it was.  n < 2^31.  (lx_index_build sorts its word table with it;
 * the Level-2 driver sorts matches and survivors with the same kernels.) */
int lx_sort_words_dev(int device, uint64_t * key[2], uint64_t * value[2], uint64_t n, uint64_t key_bits, void * stream, int * sorted_in);
/* Ahead of a handle's first lx_iterate_matches_dev (or large lx_iterate_matches) call: allocates -- and, on the host side, touches -- the
 * buffers a call on up to n_matches matches needs when they become up to n_windows windows and n_hsps result records with n_columns
 * alignment columns in all (0: results without columns, LX_ITERATE_NO_OPS).  Call it after lx_set_queries (the lanes are sized for the
 * longest query).  A first call costs what the tenth costs then (bench.py --iterate --cold); nothing changes but when the memory is
 * asked for, and estimates that fall short only mean that the call grows what is missing, as it does without lx_reserve.  The reference
 * has no counterpart: its threads' LocalDataHolder grows inside the search loop (src/search_datastructures.hpp:386-468). */
int lx_reserve(lx_handle * h, uint64_t n_matches, uint64_t n_windows, uint64_t n_hsps, uint64_t n_columns);
/* _widenAndPreprocessMatches (:1136-1175) alone on a device match list over the resident sets: the window list comes back as
 * lx_match records in `out` (room for n_matches), *out_n of them -- what lx_widen_and_preprocess leaves in its span.  bisulfite != 0:
 * ordered by subjId % 2 first, as iterateMatches' bisulfite branch sorts (:1369-1372). */
int lx_widen_and_preprocess_dev(lx_handle * h, void const * d_matches, uint64_t n_matches, int32_t bisulfite, lx_match * out, uint64_t * out_n);
uint64_t               lx_iterate_result_count(lx_iterate_result const * r);
lx_blast_match const * lx_iterate_result_matches(lx_iterate_result const * r);
uint8_t const *        lx_iterate_result_ops(lx_iterate_result const * r);
lx_iterate_stats       lx_iterate_result_stats(lx_iterate_result const * r);
void                   lx_iterate_result_free(lx_iterate_result * r);
/* A freed result's large arrays are kept for the next result (a block the allocator has just mapped costs a page fault per 4 KB when the
 * threads write it): a handful of blocks, at most 1 GiB per process.  This call gives them back; returns the bytes released. */
uint64_t               lx_trim_result_cache(void);


/* ---- record post-processing and writers (row N2: _writeRecord + BLAST-tabular / SAM output) --------------- */
/* _writeRecord (src/search_algo.hpp:820-913) for a whole result list: `m` must be grouped by n_qid (the order
 * lx_iterate_matches returns).  Per query: sort by (n_sid, q_start, q_end, s_start, s_end, frames, bit score
 * descending), drop duplicates of the same coordinates keeping the best, stable-sort by bit score descending, keep at
 * most max_matches.  In place; returns the new count. */
typedef struct lx_record_stats
{
    uint64_t qrys_with_hit, hits_duplicate2, hits_abundant, hits_final, pairs;
} lx_record_stats;
uint64_t lx_postprocess_records(lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_record_stats * stats);
/* _writeRecord's sort / unique / sort / cut (src/search_algo.hpp:820-882) on h's device for n rows in HOST memory grouped by n_qid:
 * uploads, runs the kernels, brings the kept rows back into m[0 .. *out_n).  Same rows, order and stats as lx_postprocess_records
 * (rows that are not grouped: every run of equal n_qid is a query, as there).  stats may be NULL.  LX_EINVAL, before any device
 * work: NULL h, NULL m with n > 0, NULL out_n, n >= 2^31 - 16.  lx_last_phase_ms(h, 7, ...) = device time of the kernels. */
int lx_postprocess_records_dev(lx_handle * h, lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_record_stats * stats, uint64_t * out_n);
/* lx_iterate_matches_dev followed by that step, before anything comes down: the result holds only the kept records
 * (count, rows, ops with re-based ops_off; LX_ITERATE_NO_OPS as before), *rstats (may be NULL) what lx_postprocess_records would
 * report for lx_iterate_matches_dev's result.  lx_iterate_result_stats() is unchanged (it counts what the extension did, not what
 * the cut removed).  Where the call's records are made on the device and every query's records come out of one range of the
 * list (every list but bisulfite ones, whose two strand directions are extended apart), the step runs range by range behind the
 * records kernels and only the kept rows come down, only their columns are expanded; elsewhere (bisulfite, LX_OPT_ITERATE_RECORDS =
 * 1, lists served without the multi-query plan) the finished result goes through lx_postprocess_records_dev and its columns are
 * moved together on the host.  lx_last_phase_ms(h, 7, ...) = device time of the step's kernels in the call. */
int lx_iterate_matches_dev_top(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params,
                               uint64_t max_matches, lx_record_stats * rstats, lx_iterate_result ** out);
/* Culling a query's records between _writeRecord's unique and its cut (BLAST's -max_hsps and -culling_limit; the reference has no
 * counterpart).  Per run of equal n_qid, over the rows that survive the unique step, in the output order (bit score descending, ties
 * by place in the first order); row a is BETTER than row b when it comes earlier in that order.
 *   max_hsps = K > 0:      a row is dropped when at least K better rows have the same n_sid (hits_max_hsps).
 *   culling_limit = L > 0: over the rows that max_hsps left, a row is dropped when at least L better rows have a query interval that
 *                          envelops its own (lo_b <= lo and hi <= hi_b; equal intervals envelop each other) (hits_culled).  A row's
 *                          query interval is the closed interval [min, max] of the 1-based qstart / qend that the .m8 writer prints:
 *                          nucleotide positions for a translated query (q_translated != 0), mirrored by the query's length on a
 *                          minus frame.  q_lens[n_qid], n_q entries, is the untranslated query length.
 * Then the cut to max_matches, hits_abundant, pairs and the output order as before.  All zero (lx_cull_options_default): nothing
 * changes anywhere.  q_lens may be NULL only when culling_limit == 0.  LX_EINVAL with culling_limit > 0, before any device work
 * and with a text (lx_last_output_error() for the host form, lx_last_error(h) for the device forms): a row whose n_qid >= n_q, a
 * row whose interval does not fit its query's length (q_start >= q_end, or an end behind the query's last letter), a query longer
 * than 2^32 - 1 (device forms). */
typedef struct lx_cull_options
{
    uint64_t         max_hsps;
    uint64_t         culling_limit;
    uint64_t const * q_lens;
    uint64_t         n_q;
    int32_t          q_translated;
} lx_cull_options;
typedef struct lx_cull_stats
{
    uint64_t hits_max_hsps, hits_culled;
} lx_cull_stats;
void lx_cull_options_default(lx_cull_options * o); /* all zero: both rules off */
/* lx_postprocess_records with the two rules; opt == NULL or all zero: exactly lx_postprocess_records.  stats and cull_stats may be
 * NULL.  Returns the new count (>= 0), or -- a refusal above -- LX_EINVAL (< 0) with m, *stats and *cull_stats as they were. */
int64_t lx_postprocess_records_ex(lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_cull_options const * opt, lx_record_stats * stats,
                                  lx_cull_stats * cull_stats);
/* lx_postprocess_records_dev with the two rules as two more counting kernels (lx_toprec.hip); neither is launched when its option
 * is 0.  Same rows, order and counters as lx_postprocess_records_ex. */
int lx_postprocess_records_dev_ex(lx_handle * h, lx_blast_match * m, uint64_t n, uint64_t max_matches, lx_cull_options const * opt,
                                  lx_record_stats * stats, lx_cull_stats * cull_stats, uint64_t * out_n);
/* lx_iterate_matches_dev_top with the two rules.  The lengths are the resident q_orig_len of lx_set_queries and q_translated is
 * params->q_frame_mode == LX_FRAMES_TRANSLATED: opt->q_lens, n_q and q_translated are ignored. */
int lx_iterate_matches_dev_top_ex(lx_handle * h, int slot, void const * d_matches, uint64_t n_matches, lx_search_params const * params,
                                  uint64_t max_matches, lx_cull_options const * opt, lx_record_stats * rstats, lx_cull_stats * cull_stats,
                                  lx_iterate_result ** out);

/* The taxonomy the reference keeps in its index (indexFile.taxonParentIDs / taxonHeights / sTaxIds): parents[t] and heights[t]
 * for taxon t < n_taxa (parent 0 = unassigned or the root), and per true subject id the taxa it is assigned to in CSR form:
 * s_tax_ids[s_tax_off[s] .. s_tax_off[s + 1]). */
typedef struct lx_tax_tree
{
    uint32_t const * parents;
    uint32_t const * heights;
    uint64_t         n_taxa;
    uint64_t const * s_tax_off; /* n_s + 1 entries */
    uint32_t const * s_tax_ids;
    uint64_t         n_s;
} lx_tax_tree;
/* The LCA step of _writeRecord (src/search_algo.hpp:884-907, computeLCA: src/search_misc.hpp:86-112) over a result list
 * grouped by n_qid (what lx_postprocess_records returns): per query the lowest common ancestor of the taxa of its subjects --
 * starting from the first match whose subject has a first taxon with a parent, folding in every assigned taxon of every match.
 * Writes one (n_qid, lcaTaxId) pair per query in list order (lcaTaxId 0 = no assigned subject) and their number; out arrays
 * need one entry per query with hits (at most n).  LX_EINVAL for ids outside the tree or a path that does not lead to the root
 * (the reference throws "LCA-computation error"). */
int lx_compute_lca(lx_blast_match const * m, uint64_t n, lx_tax_tree const * tree, uint64_t * out_qid, uint32_t * out_lca,
                   uint64_t * out_n);
/* Which records of a query enter its LCA.  top_percent = 100 is the reference's rule (src/search_algo.hpp:884-907: every record of
 * the query); below 100 only the records whose bit score lies within top_percent percent of the query's best one (what MEGAN calls
 * "top percent" and DIAMOND --top): with best = the largest bit_score of the query and f = 1.0 - top_percent / 100.0 (computed once,
 * in double), a record is kept iff bit_score >= best * f || bit_score == best.  0 keeps the best records only. */
typedef struct lx_lca_options
{
    double   top_percent; /* 0 .. 100; 100 = the reference's rule */
    uint64_t reserved;
} lx_lca_options;
void lx_lca_options_default(lx_lca_options * o); /* top_percent = 100 */
/* lx_compute_lca (src/search_algo.hpp:884-907, computeLCA: src/search_misc.hpp:86-112) over the records lx_lca_options keeps: a
 * query is a maximal run of equal n_qid; the fold starts from the first KEPT record whose subject has a first taxon with a parent and
 * takes in every assigned taxon of every KEPT record, in list order; one pair per query as there (0 = nothing started the fold).
 * opt == NULL or top_percent == 100: exactly lx_compute_lca, for every input (bit scores are not looked at).  LX_EINVAL for what
 * lx_compute_lca refuses, for a top_percent outside [0, 100] or not a number, and below 100 for a bit_score that is not finite.
 * This function is the specification of lx_compute_lca_dev. */
int lx_compute_lca_ex(lx_blast_match const * m, uint64_t n, lx_tax_tree const * tree, lx_lca_options const * opt, uint64_t * out_qid,
                      uint32_t * out_lca, uint64_t * out_n);
/* Whether `tree` is one on which every climb of computeLCA (src/search_misc.hpp:86-112) ends, as the trees of lx_taxonomy_build are
 * (their heights are counted from the final parents): the pointers lx_compute_lca needs are there; s_tax_off starts at 0 and
 * ascends; every s_tax_ids[x] < n_taxa; for every t < n_taxa parents[t] < n_taxa, parents[t] > 1 implies heights[t] ==
 * heights[parents[t]] + 1, and parents[t] <= 1 implies heights[t] == 0.  A climb then ends after at most max height + 2 steps.
 * Trees with two roots or with disconnected taxa pass (a query that mixes them is the fold's LX_EINVAL, src/search_algo.hpp:884-907).
 * No device is touched.  LX_OK, or LX_EINVAL with the broken rule in lx_last_output_error(). */
int lx_check_tax_tree(lx_tax_tree const * tree);

/* The LCA step (src/search_algo.hpp:884-907, src/search_misc.hpp:86-112) on h's device.  lx_tax_dev is a tree resident there:
 * lx_tax_dev_create runs lx_check_tax_tree (a failure is LX_EINVAL before any device work, the text in lx_last_error(h)) and uploads
 * parents and heights side by side, the subjects' taxon lists and the largest height; destroy it before its handle.
 * lx_compute_lca_dev gives what lx_compute_lca_ex gives for n rows in HOST memory: the same pairs in the same order, the same count.
 * Only n_qid, n_sid (as 32 bits) and, below top_percent 100, bit_score go up, through pinned staging, in ranges of whole queries of
 * at most LX_OPT_LCA_RANGE_ROWS rows (a longer query is a range of its own); a range's upload overlaps the kernels of the range
 * before it.  One lane folds one query, its rows in list order; every loop of the kernel ends after max height + 2 steps.  One
 * uint32 per query and one error word per range come down: an error word that is set (two taxa of a query without a common ancestor)
 * makes the call LX_EINVAL with the reference's text, "LCA-computation error: One of the paths didn't lead to root.", and nothing of
 * the out arrays is then promised.  LX_EINVAL with a text, before any device work: NULL arguments, a handle that is not the tree's,
 * n >= 2^31 - 16, a row with n_sid >= n_s, the option errors of lx_compute_lca_ex.  lx_last_phase_ms(h, 13, ...) = device time of
 * the kernels in the call. */
typedef struct lx_tax_dev lx_tax_dev;
int  lx_tax_dev_create(lx_handle * h, lx_tax_tree const * tree, lx_tax_dev ** out);
void lx_tax_dev_destroy(lx_tax_dev * t);
int  lx_compute_lca_dev(lx_handle * h, lx_tax_dev const * t, lx_blast_match const * m, uint64_t n, lx_lca_options const * opt,
                        uint64_t * out_qid, uint32_t * out_lca, uint64_t * out_n);

/* ---- restricting a search to taxa of the index (BLAST's -taxids / -negative_taxids, DIAMOND's --taxonlist / --taxon-exclude) ----
 * Which subjects a list of taxa keeps.  The chain of a taxon t < n_taxa is t, parents[t], parents[parents[t]], ...; it ends with the
 * first element c that has parents[c] <= 1, and where parents[c] == 1 taxon 1 belongs to it too (listing 1 selects everything
 * connected to the root); on a tree lx_check_tax_tree admits it has at most max height + 2 elements.  t is UNDER THE LIST iff its
 * chain holds a listed taxon; subject s is HIT iff one of its taxa s_tax_ids[s_tax_off[s] .. s_tax_off[s + 1]) is under the list. */
typedef struct lx_taxon_filter
{
    uint32_t const * taxa;    /* listed taxa, any order, duplicates allowed */
    uint64_t         n;       /* >= 1 */
    int32_t          exclude; /* 0: keep subjects under a listed taxon; 1: keep the others */
    uint32_t         reserved;
} lx_taxon_filter;
/* Bit s of mask (word s / 64, bit s % 64) = hit for exclude == 0, !hit for exclude != 0: a subject without taxa is dropped by an
 * include list and kept by an exclude list (DIAMOND's rule).  Bits at and beyond n_s are 0; *n_kept = the number of set bits.
 * known (may be NULL): known[i] = 1 iff taxa[i] is in the tree -- below n_taxa and with a parent, or the parent of some taxon, or a
 * taxon of some subject --, else 0.  A listed taxon that is not known matches nothing and is no error here (the trees of
 * lx_taxonomy_build skip and disconnect unassigned taxa of in-degree 1).  LX_EINVAL with a text in lx_last_output_error(): NULL
 * arguments, n == 0, a listed taxon 0, a tree lx_check_tax_tree refuses.  No handle and no device is touched.  This function is the
 * specification of lx_subject_mask_create_dev. */
int lx_tax_subject_mask(lx_tax_tree const * tree, lx_taxon_filter const * f, uint64_t * mask /* [(n_s + 63) / 64] */, uint64_t * n_kept,
                        uint8_t * known /* [f->n] or NULL */);

/* What the writers need to know about the sequences (the reference reads these from lH.qryIds / indexFile.ids). */
typedef struct lx_seq_names
{
    char const * const * q_ids;  /* per true query id (n_qid)   */
    uint64_t const *     q_lens; /* untranslated query lengths  */
    char const * const * s_ids;  /* per true subject id (n_sid) */
    uint64_t const *     s_lens;
    uint64_t             n_q, n_s;
} lx_seq_names;

enum
{
    LX_OUT_BLAST_TAB          = 0, /* -m8: 12 standard columns (src/search_options.hpp:716-760 default)         */
    LX_OUT_BLAST_TAB_COMMENTS = 1, /* -m9                                                                        */
    LX_OUT_SAM                = 2, /* SAM, default tags "AS NM ae ai qf" (src/search_options.hpp:351)            */
    LX_OUT_BAM                = 3  /* BAM: lx_render_records / lx_write_records_bgzf only (binary, BGZF-compressed) */
};
/* Appends header (if write_header) and records to `path` (myWriteHeader / myWriteRecord,
 * src/search_output.hpp:305-461, :463-733).  `ops` is the ops buffer the matches' ops_off index into; `program` is
 * "blastp", "blastn", "blastx", "tblastn" or "tblastx": positions of a translated side are reported in nucleotide
 * coordinates of the original sequence (names->q_lens / s_lens = untranslated lengths), start > end on the minus
 * strand in the tabular formats; SAM of a translated query carries the nucleotide-space CIGAR (runs x 3, frame
 * clips as H, reversed on the minus strand) and the covered part of the untranslated read. */
int lx_write_records(char const * path, int format, int write_header, char const * program, lx_blast_match const * m,
                     uint64_t n, uint8_t const * ops, lx_seq_names const * names, uint8_t const * q_res_ascii,
                     uint64_t const * q_ascii_off);

/* The output options of the reference's command line (src/search_options.hpp:224-379, parsed :716-816): which tabular columns,
 * which optional SAM tags, whether a SAM record carries the sequence and how it clips.  Initialise with
 * lx_output_options_default (= the reference's defaults: the 12 standard columns; tags "AS NM ae ai qf"; sequence "uniq";
 * hard clips; no @SQ lines), then change what the caller asked for. */
enum
{
    LX_SAM_SEQ_NEVER  = 0, /* --sam-bam-seq never  (:765-770) */
    LX_SAM_SEQ_UNIQ   = 1, /*               uniq: omitted iff frame and query range equal the previous match's (:536-553) */
    LX_SAM_SEQ_ALWAYS = 2
};
typedef struct lx_output_options
{
    char const * columns;             /* --output-columns: space-separated NCBI specifiers; NULL = "std".  Supported: std qseqid
                                         qlen sseqid slen qstart qend sstart send evalue bitscore score length pident nident
                                         mismatch positive gapopen gaps ppos frames qframe sframe staxids lcataxid            */
    char const * sam_tags;            /* --sam-bam-tags: space-separated keys of SamBamExtraTags (src/search_output.hpp:29-76):
                                         AS OC NM IH ar ae ai ap qf qs sf st ls lt; NULL = "AS NM ae ai qf" (:351)            */
    int32_t      sam_seq;             /* LX_SAM_SEQ_*                                                                         */
    int32_t      sam_hard_clip;       /* --sam-bam-clip hard (1, default) | soft (0)                                          */
    int32_t      sam_with_ref_header; /* --sam-with-refheader: one @SQ line per subject (:276-286)                            */
    int32_t      version_to_output;   /* --version-to-outputfile: `version` into the tabular version line / an @PG line       */
    char const * version;             /* (the reference writes SEQAN_APP_VERSION; this library has no lambda version: the
                                         caller names one)                                                                    */
    char const * command_line;        /* @PG CL: (src/search_output.hpp:391-399)                                              */
    char const * db_name;             /* "# Database:" of .m9 -- the reference writes the index path (search_algo.hpp:320)    */
    int32_t      genetic_code;        /* translated queries: the table the frames were made with (tags qs / OC)               */
    int32_t      reserved;
    /* taxonomy columns (staxids / st, lcataxid / lt, ls): NULL = "*" / 0, as for an index without taxonomy */
    lx_tax_tree const *  tax;
    uint64_t const *     lca_qid;     /* lx_compute_lca's output: n_lca (n_qid, taxon) pairs in list order                    */
    uint32_t const *     lca_tax;
    uint64_t             n_lca;
    char const * const * tax_names;   /* scientific name per taxon (tag ls), NULL = "*"                                       */
    /* base qualities of the queries (FASTQ, Phred+33), parallel to the writers' q_res_ascii: query q's are
     * q_qual[q_ascii_off[q] .. + q_lens[q]).  NULL (the default) = none: every writer then makes the bytes it made before the
     * field existed.  SAM and BAM write QUAL exactly where they write SEQ, over the same letters and in the same direction (the
     * minus strand reversed, not complemented; hard clips cut it as they cut SEQ; a translated query's window is the nucleotides
     * [3a + |f| - 1, 3e + |f| - 1) of the strand that was read); a record whose SEQ is "*" has QUAL "*".  SAM carries the
     * characters as they stand, BAM byte - 33 per base, reduced modulo 256.  NOT CHECKED: the bytes are not validated (the
     * documented precondition is '!' .. '~'; whatever is given, the host and the device writers do the same with it), and the
     * buffer's extent is the caller's word, as q_res_ascii's is.  Honoured by every one-shot entry that takes options
     * (lx_write_records_ex, lx_render_records, lx_write_records_bgzf, lx_render_bam_dev, lx_write_bam_dev, lx_render_text_dev,
     * lx_write_text_dev); ignored by the tabular formats; not read when q_res_ascii or q_ascii_off is NULL; not read by
     * lx_out_open (a piece's qualities go through lx_out_append_ex). */
    uint8_t const * q_qual;
} lx_output_options;
void lx_output_options_default(lx_output_options * o);
/* lx_write_records with options (NULL = defaults).  LX_EINVAL also for an unknown column specifier or tag key (the reference
 * throws "Unknown column specifier", :755-758, :803-806); lx_last_output_error() has the text. */
int lx_write_records_ex(char const * path, int format, int write_header, char const * program, lx_blast_match const * m,
                        uint64_t n, uint8_t const * ops, lx_seq_names const * names, uint8_t const * q_res_ascii,
                        uint64_t const * q_ascii_off, lx_output_options const * opt);
/* What lx_write_records_ex refuses before it touches a file -- an unknown format, column specifier or SAM tag -- so that a front
 * end can fail while it parses its options, as the reference does (src/search_options.hpp:684-816), not after the search. */
int lx_check_output_options(int format, lx_output_options const * opt);
/* myWriteFooter (src/search_output.hpp:739-750): .m9 ends with "# BLAST processed N queries" (N = records written), the other
 * formats have no footer. */
int lx_write_footer(char const * path, int format, uint64_t n_records);
char const * lx_last_output_error(void);

/* ---- rendered output and BGZF compression ------------------------------------------------------ */
/* An opaque byte buffer handed out by lx_render_records and lx_gunzip. */
typedef struct lx_bytes lx_bytes;
uint8_t const * lx_bytes_data(lx_bytes const * b);
uint64_t        lx_bytes_size(lx_bytes const * b);
void            lx_bytes_free(lx_bytes * b);
/* The bytes a writer produces, in memory (host only).  Same arguments as lx_write_records_ex, plus footer_records: >= 0 appends
 * what lx_write_footer(format, footer_records) would, < 0 no footer.  For LX_OUT_BLAST_TAB, LX_OUT_BLAST_TAB_COMMENTS and LX_OUT_SAM
 * exactly what lx_write_records_ex + lx_write_footer put in a file.  For LX_OUT_BAM the uncompressed BAM stream (SAM/BAM
 * specification 4.2): magic, the SAM header text with one @SQ line per subject (BAM always carries the references, as seqan's
 * writeHeader does), the reference list, then the SAM writer's records in binary (refID = n_sid, MAPQ 255, bin by reg2bin over the
 * CIGAR's reference span, no mate, QUAL 0xFF per base or opt->q_qual's bytes - 33; tag types ae f, AS ap S, ar ai C, qf sf c, lt NM IH I, st ls qs OC Z,
 * src/search_output.hpp:601-717).  LX_EINVAL as lx_write_records_ex, and, for LX_OUT_BAM here and in every other call that makes BAM,
 * for a subject of more than 2^31 - 1 letters (l_ref and pos have 32 signed bits; lx_last_output_error() names the subject; the text
 * formats are not limited).  *out is released with lx_bytes_free. */
int lx_render_records(int format, int write_header, char const * program, lx_blast_match const * m, uint64_t n, uint8_t const * ops,
                      lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                      lx_output_options const * opt, int64_t footer_records, lx_bytes ** out);
enum
{
    LX_BGZF_EOF = 1 /* lx_bgzf_compress: append the 28-byte empty member that ends a BGZF file */
};
/* Bytes lx_bgzf_compress may write for n input bytes (EOF member included). */
uint64_t lx_bgzf_bound(uint64_t n);
/* BGZF (blocked gzip, SAM/BAM specification 4.1) on the handle's device: the input cut into blocks of at most 65 280 bytes, each a
 * gzip member with the BC subfield (dynamic Huffman DEFLATE, or stored where that is not larger), the members one after another.
 * Every member is a complete gzip member, so the output is also a valid .gz file.  Deterministic: the same input gives the same
 * bytes on every call and handle.  Large inputs stream through the device in chunks.  cap must be >= lx_bgzf_bound(n); *out_n =
 * bytes written.  lx_last_phase_ms(h, 4, ...) = device time of the encoder's kernels in the last call.  LX_EINVAL for NULL
 * buffers, a short cap or unknown flags, before any device work. */
int lx_bgzf_compress(lx_handle * h, uint8_t const * in, uint64_t n, uint8_t * out, uint64_t cap, uint64_t * out_n, int32_t flags);
/* lx_render_records (header, records, footer when footer_records >= 0) compressed by lx_bgzf_compress with the EOF member, written
 * to `path` (created or truncated).  LX_OUT_BAM gives a .bam file, the text formats their .gz form. */
int lx_write_records_bgzf(lx_handle * h, char const * path, int format, char const * program, lx_blast_match const * m, uint64_t n,
                          uint8_t const * ops, lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off,
                          lx_output_options const * opt, int64_t footer_records);
/* LX_OUT_BAM of lx_render_records, the records made by kernels on h's device: the same bytes.  The record loop of myWriteRecord
 * (src/search_output.hpp:463-733) runs as the kernels of lx_bam.hip -- query groups (FLAG, IH, --sam-bam-seq uniq), CIGAR, SEQ, POS,
 * all fourteen tags -- over ranges of records whose bytes stay within LX_OPT_BAM_RANGE_BYTES; the header (magic, SAM text, reference
 * list; myWriteHeader, :305-461) is made on the host.  `ops_bytes` is the extent of `ops` (the device copy must know it): a row whose
 * ops_off + n_ops exceeds it is refused.  LX_EINVAL, before any device work and with lx_last_output_error()'s text, for what
 * lx_render_records refuses (program, NULL arguments, unknown tag keys, n_qid >= n_q, n_sid >= n_s), for a NULL h, and for lists
 * beyond the kernels' counters (2^31 - 16 rows, queries of 2^30 letters, ids of 2^20 characters).  *out is released with
 * lx_bytes_free.  lx_last_phase_ms(h, 11, ...) = device time of the render kernels in the call. */
int lx_render_bam_dev(lx_handle * h, int write_header, char const * program, lx_blast_match const * m, uint64_t n,
                      uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
                      uint64_t const * q_ascii_off, lx_output_options const * opt, lx_bytes ** out);
/* lx_write_records_bgzf(LX_OUT_BAM) with the records rendered AND compressed on the device (myWriteRecord,
 * src/search_output.hpp:463-733, then the BGZF encoder where the bytes stand): rows, ops and query letters go up, only members come
 * down.  The file is byte-identical: the part of a range's stream that does not fill a 65 280-byte block is carried into the next
 * range, so the members are cut where lx_bgzf_compress cuts them.  Refusals as lx_render_bam_dev; `path` is created or truncated once
 * everything is made.  lx_last_phase_ms: 11 = the render kernels, 4 = the encoder's. */
int lx_write_bam_dev(lx_handle * h, char const * path, char const * program, lx_blast_match const * m, uint64_t n,
                     uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
                     uint64_t const * q_ascii_off, lx_output_options const * opt);

/* The characters glibc's printf writes for a number, made with integer arithmetic alone (no printf, no double operation beyond
 * taking the bits apart): what the device text writers below print, and what the host writer's snprintf calls print
 * (host/lx_output.cpp: "%.1e" of the e-value, "%.1f" of the bit score, "%.2f" of pident and ppos, "%g" of SAM's ae -- seqan's
 * BlastTabular writeRecord behind myWriteRecord, src/search_output.hpp:463-733).  Rounding is to nearest, an exact tie to even.
 * LX_NUM_E1: "%.1e" of any double (subnormals, +-0, inf, -inf, nan, -nan).  LX_NUM_G_FLOAT: "%g" of v, which the callers have
 * narrowed to float and widened again.  LX_NUM_F1 / LX_NUM_F2: "%.1f" / "%.2f" of a finite v with |v| < 1e15.  Writes the text and a
 * terminating NUL into out[0 .. cap) and returns its length (at most 24); LX_EINVAL for a cap that is too short, an unknown kind, a
 * NULL out, or an F value outside the domain. */
enum
{
    LX_NUM_E1      = 0,
    LX_NUM_F1      = 1,
    LX_NUM_F2      = 2,
    LX_NUM_G_FLOAT = 3
};
int lx_format_number(int kind, double v, char * out, uint64_t cap);

/* lx_render_records for LX_OUT_BLAST_TAB, LX_OUT_BLAST_TAB_COMMENTS and LX_OUT_SAM with the records made by kernels on h's device:
 * the same bytes.  The tabular record of seqan's writeRecord (behind myWriteRecord, src/search_output.hpp:463-733; every column of
 * --output-columns, in any order and as often as named, src/search_options.hpp:716-760) and the SAM record with its tags (:463-733)
 * run as the kernels of lx_text.hip over query groups (the comment lines and hit count of .m9, FLAG, IH, --sam-bam-seq uniq) in
 * ranges of records whose bytes stay within LX_OPT_BAM_RANGE_BYTES; numbers are printed by lx_format_number's formatter.  The SAM
 * header (myWriteHeader, :347-460) and the .m9 footer (myWriteFooter, :739-750; footer_records >= 0) are made on the host.  Only the
 * first words of the subject ids the rows name go up.  `ops` is read for LX_OUT_SAM only (the tabular formats have no column made of
 * them, as in lx_write_records_ex: there they may be NULL, and the rows' ops_off / n_ops are not looked at).  LX_EINVAL, before any device work and with lx_last_output_error()'s text,
 * for what lx_render_bam_dev refuses, for an unknown column specifier, for LX_OUT_BAM (lx_render_bam_dev makes it), and for a row
 * whose bit_score or identity is not finite or not below 1e15 in magnitude (the host writer's own buffer is no yardstick there).
 * *out is released with lx_bytes_free.  lx_last_phase_ms(h, 12, ...) = device time of the text record kernels in the call. */
int lx_render_text_dev(lx_handle * h, int format, int write_header, char const * program, lx_blast_match const * m, uint64_t n,
                       uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
                       uint64_t const * q_ascii_off, lx_output_options const * opt, int64_t footer_records, lx_bytes ** out);
/* The file of a text format with the records rendered on the device (myWriteHeader, myWriteRecord, myWriteFooter,
 * src/search_output.hpp:305-750).  bgzf = 0: the plain file lx_write_records_ex(write_header = 1) + lx_write_footer write.  bgzf = 1:
 * the file lx_write_records_bgzf writes, byte for byte, compressed where the stream stands as in lx_write_bam_dev: less than a block
 * is carried into the next range, the footer goes behind the last range, then the EOF member; only members come down.  Refusals
 * as lx_render_text_dev; `path` is created or truncated once everything is made.  lx_last_phase_ms: 12 = the text record kernels,
 * 4 = the encoder's. */
int lx_write_text_dev(lx_handle * h, char const * path, int format, int bgzf, char const * program, lx_blast_match const * m, uint64_t n,
                      uint8_t const * ops, uint64_t ops_bytes, lx_seq_names const * names, uint8_t const * q_res_ascii,
                      uint64_t const * q_ascii_off, lx_output_options const * opt, int64_t footer_records);

/* An output file written piece by piece.  After lx_out_close the file is byte for byte the file the one-shot writers make from
 * the concatenated list -- lx_write_records_ex + lx_write_footer (plain text), lx_write_records_bgzf (bgzf, LX_OUT_BAM),
 * lx_write_text_dev / lx_write_bam_dev (which agree with those) --, wherever the pieces were rendered and however the list was cut.
 *
 * lx_out_open writes the header: the SAM header, or the BAM magic with header text and reference list, from `subjects` (only s_ids,
 * s_lens and n_s are read; they, opt->tax and opt->tax_names must stay valid until lx_out_close; the texts of opt are copied; its
 * lca_* and q_qual are not read).  bgzf = 1, and LX_OUT_BAM always: the stream is BGZF-compressed on h's device, cut into 65 280-byte blocks
 * exactly as lx_bgzf_compress cuts the whole stream.  Refusals are those of the one-shot writers -- an unknown format, program,
 * column or tag -- and bgzf or LX_OUT_BAM without a handle; all before `path` is created or truncated.  A failure behind them
 * (the encoder, the disk) removes the file again.  h may be NULL for a plain
 * file rendered on the host; the texts are then in lx_last_output_error(), else in lx_last_error(h).
 *
 * lx_out_append renders n records: where = LX_RENDER_HOST by the code of lx_render_records, LX_RENDER_DEV by the kernels of
 * lx_render_text_dev / lx_render_bam_dev (it needs a handle).  A piece holds WHOLE query groups: everything that is decided per
 * query (the comment lines of .m9, FLAG, IH, --sam-bam-seq uniq, the LCA) is then decided inside the piece.  `names` describes this
 * piece's queries (q_ids, q_lens, n_q; m[].n_qid, q_ascii_off and lca_qid count within the piece); m[].n_sid counts within the
 * subjects given at open.  Of a compressed stream, the bytes that do not fill a block (always fewer than 65 280) stay in the
 * object -- on the device when the piece was rendered there, where the records are compressed as they stand and only members come
 * down -- and go in front of the next piece.  n = 0 is a no-op whatever the other arguments are.  A refused piece (LX_EINVAL from
 * the checks of the one-shot writers, made before any kernel runs) leaves the file as it was; after any other failure every later
 * append is refused.  lx_last_phase_ms(h, 4 / 11 / 12, ...) report the last append.
 *
 * lx_out_close writes the footer of .m9 (footer_records >= 0: "# BLAST processed N queries"), the last partial block and the
 * EOF member, closes the file and frees o -- also when it fails. */
typedef struct lx_out lx_out;
enum
{
    LX_RENDER_HOST = 0,
    LX_RENDER_DEV  = 1
};
int lx_out_open(lx_handle * h, char const * path, int format, int bgzf, char const * program, lx_seq_names const * subjects,
                lx_output_options const * opt, lx_out ** out);
int lx_out_append(lx_out * o, int where, lx_blast_match const * m, uint64_t n, uint8_t const * ops, uint64_t ops_bytes,
                  lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off, uint64_t const * lca_qid,
                  uint32_t const * lca_tax, uint64_t n_lca);
/* lx_out_append plus the piece's base qualities: q_qual is parallel to the piece's q_res_ascii, as lx_output_options::q_qual is to
 * a one-shot writer's (same rule, same things not checked); NULL = none, which is what lx_out_append passes.  Pieces with and
 * without qualities may follow each other in one file, rendered on either side. */
int lx_out_append_ex(lx_out * o, int where, lx_blast_match const * m, uint64_t n, uint8_t const * ops, uint64_t ops_bytes,
                     lx_seq_names const * names, uint8_t const * q_res_ascii, uint64_t const * q_ascii_off, uint8_t const * q_qual,
                     uint64_t const * lca_qid, uint32_t const * lca_tax, uint64_t n_lca);
int lx_out_close(lx_out * o, int64_t footer_records);

/* Decompresses a gzip stream of one or more members (RFC 1952): BGZF members on h's device, other members on the calling
 * thread; h may be NULL (every member on the host).  *out is released with lx_bytes_free.  Malformed input: LX_EINVAL.
 * A member with the BGZF subfield (BC, BSIZE) whose DEFLATE bytes and ISIZE are at most 64 KiB is decoded on the device, one
 * workgroup per member; a member without it (what gzip, pigz and most downloads make) is decoded on the host, as is every member
 * when h is NULL.  Every member's CRC32, ISIZE and final block are checked; a malformed one (invalid code, distance before the
 * start of the output, output past ISIZE, truncation, BSIZE past the end of the data, bytes that are no gzip member) fails the
 * call with a message that names the member and its byte offset: lx_last_error(h), or lx_last_output_error() when h is NULL.
 * lx_last_phase_ms(h, 5, ...) = device time of the decoder's kernel in the last call.
 *
 * A plain member (no BC subfield, or one beyond those limits) with at least LX_OPT_GUNZIP_PARALLEL_FROM bytes of input left behind
 * its header, and not ending inside the first 64 KiB of them, is decoded on h's device in parallel: its DEFLATE bytes are cut into chunks of LX_OPT_GUNZIP_CHUNK bytes and handled in
 * waves of at most 512 chunks.  Per wave a finder kernel looks in every chunk but the first for the first bit where a
 * non-final dynamic-Huffman block begins; a decode kernel runs one decoder per found chunk up to the next found bit, writing 16-bit
 * symbols in which a back-reference into the unknown 32 KiB in front of the chunk is a marker; a chain kernel keeps the chunks that
 * begin on the very bit their predecessor ended on, and the next wave starts where the last of them ended; a window pass and a byte
 * pass turn the symbols into bytes at their final offsets and take the CRC32.  The four steps of a wave are one submission with
 * one stream synchronisation (lx_gunzip_stats.waits) behind it; the wave's bytes then come down in one blocking copy.  Only bytes that passed the trailer's CRC32 and
 * ISIZE are returned: in every other case (no block boundary in four chunks on end, a chunk that ends in a decode status or runs out of room --
 * ten symbols per compressed byte --, a chain that keeps breaking, a CRC32, ISIZE, BSIZE or trailer difference) the member is
 * DECLINED and decoded on the calling thread from its first byte, which gives the bytes or the error text that path gives.  The
 * options move work between the device and the host and never change a byte or a verdict.  lx_last_phase_ms(h, 10, ...) = device
 * time of the plain-member kernels in the last call (101, 102, 103 = its find, its decode, and its chain and resolve kernels alone). */
int lx_gunzip(lx_handle * h, uint8_t const * in, uint64_t n, lx_bytes ** out);

/* Why the parallel path declined a plain member. */
enum
{
    LX_GUNZIP_DECLINE_NONE        = 0,
    LX_GUNZIP_DECLINE_NO_BOUNDARY = 1, /* no dynamic-Huffman block start found (stored or fixed-Huffman blocks only) */
    LX_GUNZIP_DECLINE_ROOM        = 2, /* a chunk's output exceeds its room */
    LX_GUNZIP_DECLINE_STATUS      = 3, /* a chunk that starts on a true boundary ends in a decode status */
    LX_GUNZIP_DECLINE_CHAIN       = 4, /* the chain check keeps dropping chunks (block starts inside stored data) */
    LX_GUNZIP_DECLINE_TRAILER     = 5, /* fewer than 8 bytes behind the final block, or a BSIZE that says otherwise */
    LX_GUNZIP_DECLINE_CRC         = 6,
    LX_GUNZIP_DECLINE_ISIZE       = 7
};
typedef struct lx_gunzip_stats
{
    uint64_t bgzf_members;   /* BGZF members decoded by the BGZF kernel */
    uint64_t plain_parallel; /* plain members decoded in parallel on the device */
    uint64_t plain_host;     /* plain members decoded on the calling thread: below the threshold, or declined */
    uint64_t chunks;         /* chunks decoded and verified, of the members in plain_parallel and of the declined ones */
    uint64_t chunks_dropped; /* found chunks the chain check dropped */
    uint64_t waves;
    uint64_t declined;       /* plain members the parallel path began and gave to the host */
    uint64_t bytes_up;       /* bytes the plain path moved to the device ... */
    uint64_t bytes_down;     /* ... and from it */
    int32_t  last_decline;   /* LX_GUNZIP_DECLINE_* of the last declined member */
    int32_t  waits;          /* stream synchronisations of the plain path: one per wave (its bytes then come down in one blocking copy) */
} lx_gunzip_stats;
/* The counts of h's last lx_gunzip call, or of its last lx_gunzip_stream_next call: of that call alone where it returned a piece,
 * of the whole file (every call of the stream summed) where it reported the end. */
int lx_last_gunzip_stats(lx_handle const * h, lx_gunzip_stats * stats);
/* A decline reason in words ("no boundary", "room", ...). */
char const * lx_gunzip_decline_text(int reason);

/* lx_gunzip over a FILE, piece by piece, in bounded memory.  The pieces, concatenated, are exactly what lx_gunzip(h, the file's
 * bytes) returns; for a file that does not begin with the gzip magic they are the file's own bytes.  Every piece but the last has
 * at least one byte and at most piece_bytes + 65536 (piece_bytes = 0: 64 MiB).  The stream walks the members as lx_gunzip does:
 * BGZF members (BC subfield, at most 64 KiB of DEFLATE bytes and of text) are gathered, whole, until their ISIZE sum fills the
 * piece, and the group is decoded by the BGZF path -- on h's device, or member by member on the calling thread when h is NULL --;
 * only that group's compressed bytes are read from the file.  A plain member that lx_gunzip would decode on h's device -- at least
 * LX_OPT_GUNZIP_PARALLEL_FROM bytes of the file behind its header, and not ending inside the first 64 KiB of them; with a threshold
 * of fewer than 10 bytes a stream keeps to the calling thread, as it did before it had this path -- is decoded
 * there wave by wave, by the kernels and under the options of lx_gunzip: a call runs a wave when less than a piece of text is
 * left from the last one, and across calls the stream keeps the bit where the next wave starts, the CRC register and the length so
 * far, and the text not handed out yet, whose last 32 KiB are the window the next wave is given (h keeps nothing of the stream
 * between two calls).  A wave has at most max(2, piece_bytes / chunk) chunks, so that its text is at most 10 x max(piece_bytes,
 * 2 chunks) bytes -- ten symbols of room per compressed byte -- and never more than 320 MiB with the default chunk; only the wave's
 * compressed bytes are read from the file.  Where lx_gunzip would decline (no block boundary in four chunks on end, a decode
 * status, a chunk out of room, a chain that keeps breaking) the stream does not fail: pieces handed out cannot be taken back, so the
 * calling thread goes on where the last verified chunk ended, with the window, CRC and length so far, and finishes the member
 * (stats: declined, last_decline, plain_host).  Every other member is decoded on the calling thread by the same
 * DEFLATE code, which stops between two symbols once the piece is full and keeps the last 32 KiB of text as the window; CRC32 and
 * ISIZE are checked at the trailer, for a member from the device in the call that hands out its last bytes.  The file is mapped (a
 * file that cannot be mapped is read whole, compressed); between calls the stream holds O(piece_bytes) of text and, inside such a
 * plain member, what is left of one wave's text.  A corrupt stream fails in the call that reaches the damage, with lx_gunzip's
 * message for the whole file: member number, and byte offset from the start of the file; every later call fails.  A plain member's CRC32 is
 * known at its trailer only, so pieces handed out before the failing call may hold text of the member that failed.  NULL arguments and a file
 * that cannot be opened: LX_EINVAL with a text (lx_last_error(h), or lx_last_output_error() when h is NULL).  While the stream is
 * open, h serves no other call between lx_gunzip_stream_next and the reading of its phase times (5; 10 and 101 to 103 for the
 * waves) or stats, which are those of that call alone; behind the call that reports the end the stats are the whole file's. */
typedef struct lx_gunzip_stream lx_gunzip_stream;
int  lx_gunzip_stream_open(lx_handle * h, char const * path, uint64_t piece_bytes, lx_gunzip_stream ** out);
/* The next piece (released with lx_bytes_free); LX_OK with *piece == NULL at the end. */
int  lx_gunzip_stream_next(lx_gunzip_stream * s, lx_bytes ** piece);
void lx_gunzip_stream_close(lx_gunzip_stream * s);

/* ---- taxonomy of an index (mkindex -m / -x: src/mkindex_algo.hpp:68-107, :277-598, src/mkindex_misc.hpp:69-144) ----------- */
/* Every non-overlapping match of the reference's accession regex in text[0, n) (UniProt, NCBI nucleotide / protein / WGS / MGA,
 * RefSeq, UniParc; ECMAScript's leftmost-first alternation, greedy counts), left to right: the first min(cap, *n_found) of them
 * into out_begin / out_len; *n_found = their number.  No handle, no device. */
int lx_find_accessions(uint8_t const * text, uint64_t n, uint64_t * out_begin, uint32_t * out_len, uint64_t cap, uint64_t * n_found);

enum
{
    LX_TAXMAP_NCBI    = 0, /* *.accession2taxid: first line "accession\taccession.version\ttaxid\tgi"; field 0 = accession, 2 = taxon */
    LX_TAXMAP_UNIPROT = 1  /* *.dat (idmapping.dat): lines with field 1 == "NCBI_TaxID"; field 0 = accession, 2 = taxon          */
};
typedef struct lx_taxmap lx_taxmap;
/* The accession table of n_s subjects: ids[id_off[s] .. id_off[s + 1]) is subject s's id (after --truncate-ids); each accession
 * in it maps to s, the later subject winning an accession two share.  h: the join runs on h's device (the table is uploaded
 * here, once), NULL: on the library's host threads (n_threads parts; 0 = LX_OPT_HOST_THREADS' width).  chunk_bytes: the map is
 * joined in chunks of whole lines of at most this many bytes (0 = 256 MiB; a line longer than a chunk is refused).  Errors go to
 * lx_last_error(h), or lx_last_output_error() when h is NULL, for this call and the lx_taxmap_* calls on *out. */
int lx_taxmap_create(lx_handle * h, int format, uint8_t const * ids, uint64_t const * id_off, uint64_t n_s, uint64_t chunk_bytes,
                     uint32_t n_threads, lx_taxmap ** out);
/* The next n bytes of the map, cut anywhere (a line may span calls).  LX_EINVAL with the reference's text and the 1-based line
 * number: "Unexpected first line in NCBI taxid file." (NCBI format), "Error: Expected taxonomical ID, but got something I couldn't
 * read: X" (a line whose accession is in the table and whose taxon field is no number; on other lines it is not read).  Both
 * paths name the first such line of the file.  After an error every later call returns it again. */
int lx_taxmap_feed(lx_taxmap * tm, uint8_t const * bytes, uint64_t n);
typedef struct lx_taxmap_result
{
    uint64_t const * s_tax_off;     /* n_s + 1: subject s's taxa are s_tax_ids[s_tax_off[s] .. s_tax_off[s + 1]), in file order,
                                       duplicates kept */
    uint32_t const * s_tax_ids;
    uint64_t         n_s;
    uint32_t const * present;       /* the taxa that occur, ascending, taxon 1 (the root) always among them */
    uint64_t         n_present;
    uint64_t         no_acc, multi_acc; /* subjects whose id holds no / more than one accession                  */
    uint64_t         no_tax, multi_tax; /* subjects with no / more than one taxon                                  */
    uint64_t         lines, matched;    /* lines of the map (the NCBI header included), lines that gave a pair  */
} lx_taxmap_result;
/* The end of the map (an unterminated last line is a line) and the result, valid until lx_taxmap_destroy.
 * lx_last_phase_ms(h, 6, ...) = device time of the join kernels since lx_taxmap_create. */
int  lx_taxmap_finish(lx_taxmap * tm, lx_taxmap_result * out);
void lx_taxmap_destroy(lx_taxmap * tm);

/* The reference's tree (parseAndStoreTaxTree): nodes.dmp (field 0 = taxon, field 2 = parent) and names.dmp (field 6 ==
 * "scientific name": field 2 names field 0) as text, present = the taxa of the subjects (lx_taxmap_result.present).  Present
 * taxa and their ancestors are kept, every other parent becomes 0; parents of in-degree 1 that are not present themselves are
 * skipped and disconnected; heights count the steps to a parent of at most 1; name 0 is "invalid", a kept taxon without a name
 * "n/a" (one warning each, and one more when over 10 % of the taxa have none).  The arrays cover every node and every present
 * taxon: a present taxon without a node has parent 0 (the reference reads past its arrays there).  No handle; errors (unreadable
 * ids, "Error: taxonomical ID is N, but no such taxon in tree.") go to lx_last_output_error(). */
typedef struct lx_taxonomy lx_taxonomy;
int lx_taxonomy_build(char const * nodes, uint64_t nodes_n, char const * names, uint64_t names_n, uint32_t const * present, uint64_t n_present,
                      lx_taxonomy ** out);
typedef struct lx_taxonomy_info
{
    uint32_t const *     parents;  /* n_taxa */
    uint32_t const *     heights;  /* n_taxa */
    char const * const * names;    /* n_taxa, "" for the taxa that are not kept */
    uint64_t             n_taxa;
    uint64_t             n_nodes;  /* taxa with a parent after the thinning */
    uint32_t             max_height;
    uint32_t             unnamed;  /* kept taxa named "n/a" */
    char const *         warnings; /* the warnings, one per line ("" = none) */
} lx_taxonomy_info;
int  lx_taxonomy_get(lx_taxonomy const * t, lx_taxonomy_info * out);
void lx_taxonomy_free(lx_taxonomy * t);

/* ---- Level 3: the word index and search() (row N3: seeding) ------------------------------------------------ */
/* What the reference's FM-index answers for search() (src/search_algo.hpp:611-762) -- how often does this reduced word occur, and
 * where -- is answered here by a sorted table of packed words over the reduced, frame-expanded subjects: per subject position the key
 * of its next key_len reduced letters (base alph + 1; the extra digit pads sequence ends), entries in (key, sequence, position)
 * order, and a prefix table (n_prefix = (alph + 1)^prefix_len + 1 entries: where the words with every prefix of prefix_len letters
 * begin).  key_len is the largest with (alph + 1)^key_len < 2^63: 18 for ten letters, 27 for four.  The caller reduces: s_red holds
 * letters 0 .. alph - 1 (Li-10, Murphy-10, dna4, the bisulfite pair -- src/mkindex_options.hpp:182-185), sequence i at
 * s_red[s_off[i] .. s_off[i] + s_len[i]).  The index keeps its own copy of s_red / s_off / s_len. */
typedef struct lx_index lx_index;
typedef struct lx_index_info
{
    uint64_t n_entries, n_prefix;
    int32_t  alph, key_len, prefix_len, built_on_device;
} lx_index_info;
typedef struct lx_index_entry /* one row of the table */
{
    uint64_t key;
    uint32_t seq, pos;
} lx_index_entry;

/* The table the reference's mkindex step would put into its index (src/mkindex_algo.hpp generateIndexAndDump; the FM-index's place).
 * h != NULL: keys, the library's radix sort, entries and prefix table as kernels on h's device and stream (lx_last_phase_ms phase 8),
 * and the table and the reduced subjects stay resident there for lx_seed_queries on h.  That needs fewer than 2^31 words in all (the
 * sort ranks with 32 bits) and fewer than 2^32 - 1 sequences: beyond, LX_EINVAL with a text (LX_ENOMEM: the device has no room for
 * the build) -- build with h == NULL then, or in slices: with LX_OPT_INDEX_SLICE_WORDS = N >= 1 on h the words are counted by their
 * first prefix_len letters (the counts' scan is the prefix table), the buckets are cut into slices (lx_index_plan_slices) and every
 * slice is compacted, sorted and written on its own.  That takes fewer than 2^32 - 1 words (a cursor on the device is a 32-bit range)
 * with no bucket beyond 2^31 - 1; phase 8 then reports the slices as its launches.  h == NULL: on host_threads host threads (0 = the
 * library's share of the CPUs), no device is touched.  The same table entry for entry every way.  Needs every sequence shorter than
 * 2^32 - 1 letters and at most 2^32 - 1 sequences. */
int lx_index_build(lx_handle * h, uint8_t const * s_red, uint64_t const * s_off, uint64_t const * s_len, uint64_t n_sseq, int32_t alph,
                   uint32_t host_threads, lx_index ** out);
/* How the sliced build cuts a prefix table (pre[w] = first entry whose word is >= w, n_prefix values; bucket w holds pre[w + 1] - pre[w]
 * words) into slices of at most slice_words words; no device is touched.  The buckets are walked in order with one running slice: a
 * bucket joins it if the slice still has no words or if its words plus the bucket's do not exceed slice_words, otherwise the slice
 * closes and the bucket opens the next one -- a bucket larger than slice_words is a slice of its own --; a last slice without words
 * (empty buckets behind a slice that is full) is joined to the one before it, so that every slice of a table with words has some.
 * first_word[s] = the first bucket of slice s (slice s ends where s + 1 begins, the last at bucket n_prefix - 1).  *n_slices is always
 * written, first_word only when cap >= *n_slices.  LX_EINVAL for NULL pre / n_slices (or first_word with cap > 0), slice_words == 0,
 * n_prefix < 2, a pre that does not ascend, a bucket of more than 2^31 - 1 words (beyond the sort). */
int lx_index_plan_slices(uint64_t const * pre, uint64_t n_prefix, uint64_t slice_words, uint64_t * first_word, uint64_t cap, uint64_t * n_slices);
/* An index file's table: exactly the bytes lx_index_save writes -- int32 {alph, key_len, prefix_len, 0}, uint64 {n_entries,
 * n_prefix}, the entries (16 bytes each), the prefix table --, over the sequences they were made from.  LX_EINVAL for truncated
 * bytes, bytes that are left over, a geometry or counts that do not fit the sequences, a prefix table that does not ascend, an entry
 * outside its sequence.  h != NULL: the table becomes resident on h's device as after lx_index_build; no sort runs, so the only
 * limit is the device cursor's: fewer than 2^32 - 1 entries (and the device's memory). */
int lx_index_load(lx_handle * h, uint8_t const * bytes, uint64_t n, uint8_t const * s_red, uint64_t const * s_off, uint64_t const * s_len,
                  uint64_t n_sseq, lx_index ** out);
int lx_index_save(lx_index const * ix, lx_bytes ** out);
/* The same table for another handle (h == NULL: for no device): shares the host copy with ix, uploads its own device copy.  Either
 * index may be destroyed first.  (One handle per host thread and device: the table is built once and attached to each.) */
int lx_index_attach(lx_index const * ix, lx_handle * h, lx_index ** out);
int lx_index_get_info(lx_index const * ix, lx_index_info * out);
/* entries [first, first + n) of the table (for checks and tools); LX_EINVAL beyond its end */
int lx_index_copy_entries(lx_index const * ix, uint64_t first, uint64_t n, lx_index_entry * out);
/* Destroy an index before the handle it was made with. */
void lx_index_destroy(lx_index * ix);

/* SearchOptions' seeding part (src/search_options.hpp:309-337) and what search() reads from LambdaOptions: seeds of seed_length
 * letters every seed_offset letters, up to max_seed_dist substitutions (0: exact, :505-535; half_exact != 0: only in the second half,
 * searchHalfExactImpl :537-604), adaptive elongation (:679-727), seedLooksPromising (:426-481) with pre_scoring /
 * pre_scoring_thresh, the over-abundance cut (:729) from max_matches.  The ranges are the bundled front end's: seed_length 2 .. 63,
 * seed_offset >= 1, max_seed_dist 0 .. 5, pre_scoring >= 0, q_num_frames 1 .. 6, unknown_rank 0 .. 31. */
typedef struct lx_seed_params
{
    int32_t        seed_length, seed_offset, max_seed_dist, half_exact, adaptive, pre_scoring;
    double         pre_scoring_thresh;
    uint64_t       max_matches;
    int32_t        q_num_frames, unknown_rank; /* frames per read (adjacent sequences); 'X' / 'N' in alignment ranks: no seed starts there */
    int8_t const * matrix;                     /* LX_ALPH x LX_ALPH: matrix[q_rank * LX_ALPH + s_rank] */
    int8_t const * matrix_rev;                 /* bisulfite: the reverse scheme, for hits on odd subject frames (:464-466); else NULL */
    uint32_t       host_threads;               /* host threads of the h == NULL path and of the reads the device declines (0 = the library's share) */
} lx_seed_params;
typedef struct lx_seed_stats
{
    uint64_t n_matches, hits_after_seeding, hits_failed_pre_extend; /* the list's length; stats.hitsAfterSeeding, hitsFailedPreExtendTest */
    uint64_t reads_declined, launches_full; /* reads the host threads finished inside the call (those of full launches included); launches whose match buffer filled up */
} lx_seed_stats;
typedef struct lx_seed_result lx_seed_result;

/* search() (src/search_algo.hpp:611-762) for the reads whose first frame sequences are listed in `reads` (NULL: every read of the
 * set): the match list iterateMatches consumes.  Sequence i of the queries lies at q_res / q_red[q_off[i] .. q_off[i] + q_len[i])
 * (alignment ranks / reduced letters); s_res are the subjects in alignment ranks at the index's offsets.
 *   h != NULL  (the handle the index was built, loaded or attached with): one lane per read on h's device and stream (phase 9 of
 *              lx_last_phase_ms), launches of at most 4 Mi reads with room for 64 matches per read.  The device declines what it
 *              cannot hold: a read with a word beyond key_len letters that occurs more than 32 times or with more than 24 letters
 *              behind a seed's exact part, and all reads of a launch whose match buffer filled up.  Those reads are seeded on the
 *              host threads inside the call and their matches appended, so the result is always the complete list, contiguous in
 *              device memory.  Only the queries are uploaded: the table and s_red are resident with the index; s_res == NULL
 *              means the subjects lx_set_subjects made resident on h (else s_res is uploaded for the call).
 *   h == NULL  (any index): seedQueries on the host threads; s_res must be given.
 * The ORDER of the list carries no meaning -- the lanes' on the device, the reads' on the host --: iterateMatches sorts its span
 * before use (src/search_algo.hpp:1141), and so do lx_iterate_matches*.  Two results are compared as sorted lists.
 * LX_EINVAL before any device work, with a text (lx_last_error(h); lx_last_output_error() when h is NULL): NULL buffers, parameters
 * outside the ranges above, a read id that is not a first frame or outside the set, a handle that is not the index's. */
int lx_seed_queries(lx_handle * h, lx_index const * ix, uint8_t const * s_res, uint8_t const * q_res, uint8_t const * q_red, uint64_t const * q_off,
                    uint64_t const * q_len, uint64_t n_qseq, uint64_t const * reads, uint64_t n_reads, lx_seed_params const * p, lx_seed_result ** out);
lx_seed_stats lx_seed_result_stats(lx_seed_result const * r);
/* the list in host memory (a device result's copy is made on first use; NULL: out of memory).  The caller may modify it
 * (lx_iterate_matches does). */
lx_match *    lx_seed_result_matches(lx_seed_result * r);
/* the list in device memory, n_matches records: d_matches of lx_iterate_matches_dev / lx_iterate_matches_dev_top on the same handle,
 * without a copy.  NULL for a host-path result.  Valid until the result is freed. */
void const *  lx_seed_result_matches_dev(lx_seed_result const * r);
/* Results are freed in any order, before their handle is destroyed (a freed result's device block is kept by the handle for the next call). */
void          lx_seed_result_free(lx_seed_result * r);

/* A subject mask: one bit per true subject id, as lx_tax_subject_mask lays them out, on the host and -- made with a handle -- on that
 * handle's device too.  Destroy it before its handle.
 *   lx_subject_mask_create_dev  the rule of lx_tax_subject_mask by kernels over the tree resident in t (h must be t's handle): the
 *                               listed taxa go up in one small copy and are marked in a byte per taxon, one lane per taxon climbs its
 *                               chain (every loop ends after max height + 2 steps), one lane per subject ORs over its taxa and a
 *                               wavefront's ballot is one mask word.  The words equal lx_tax_subject_mask's bit for bit.  `known` is
 *                               not computed here.  LX_EINVAL with a text (lx_last_error(h)): NULL arguments, n == 0, a listed
 *                               taxon 0, a tree of another handle.
 *   lx_subject_mask_create      from given words ((n_s + 63) / 64 of them, bits at and beyond n_s 0, else LX_EINVAL): h == NULL keeps
 *                               them on the host, else they are also uploaded to h's device.
 *   lx_subject_mask_info / _copy  the number of subjects and of set bits; the words. */
typedef struct lx_subject_mask lx_subject_mask;
int  lx_subject_mask_create_dev(lx_handle * h, lx_tax_dev const * t, lx_taxon_filter const * f, lx_subject_mask ** out);
int  lx_subject_mask_create(lx_handle * h, uint64_t const * words, uint64_t n_s, lx_subject_mask ** out);
int  lx_subject_mask_info(lx_subject_mask const * m, uint64_t * n_s, uint64_t * n_kept);
int  lx_subject_mask_copy(lx_subject_mask const * m, uint64_t * words); /* [(n_s + 63) / 64] */
void lx_subject_mask_destroy(lx_subject_mask * m);
/* Drops from r's list every match whose subject's bit is 0 (subject = subjId / sbj_num_frames, sbj_num_frames 1 .. 6): a stable
 * compaction, the kept matches in their old order.  *n_before / *n_kept (either may be NULL): the list's length before and after.
 *   a device result (seeded with a handle): m must be a mask of the same handle.  A flag per match from the mask words, one sum scan,
 *       a scatter of the records into a second device block that replaces the result's own; nothing of the list comes to the host.
 *       Afterwards lx_seed_result_stats(r).n_matches is the kept count (the other fields are unchanged), lx_seed_result_matches_dev(r)
 *       the new list, and a host copy made earlier is dropped (lx_seed_result_matches makes it anew).  At most 2^31 - 16 matches.
 *   a host-path result: the same compaction of the host list; any mask serves.
 * A match whose subject lies beyond the mask makes the call LX_EINVAL and leaves the result exactly as it was.  LX_EINVAL with a text
 * (lx_last_error(h) for a device result, lx_last_output_error() always): NULL arguments, sbj_num_frames outside 1 .. 6, a device
 * result with a host-only mask or a mask of another handle.  lx_last_phase_ms(h, 14, ...) = device time of the kernels. */
int  lx_seed_result_filter(lx_seed_result * r, lx_subject_mask const * m, int32_t sbj_num_frames, uint64_t * n_before, uint64_t * n_kept);

/* ---- low-complexity masking of the queries ------------------------------------------------------
 * Soft masking as BLAST does it: a masked query letter starts and carries no seed; pre-scoring, extension, statistics and output
 * read the unmasked letters.  The rule is SEG's first two stages on alignment ranks, in integers (host and device cannot differ by
 * a rounding):
 *   T[c] = round(c * log2 c * 65536) for c = 0 .. 64 (T[0] = T[1] = 0); thr(k) = ceil(window * (log2 window - k) * 65536).
 *   Window p of a sequence of L >= window letters covers letters [p, p + window); its score S(p) is the sum over ranks r of
 *   T[count of r in the window] -- every rank is a letter, 'X' and '*' too --, and its entropy is <= k bits exactly when S(p) >= thr(k).
 *   A run is a maximal stretch of consecutive windows with S >= thr(k2); a run that holds a window with S >= thr(k1) masks every
 *   letter from its first window's first letter to its last window's last letter.  A sequence shorter than the window is never
 *   masked; windows never reach across a sequence's end.
 * SEG's third stage, which trims each raw segment to its least probable part, is NOT applied, so a mask is SEG's segment or wider (an
 * SP repeat between ordinary flanks takes a few flank letters on either side along).  This is not NCBI's
 * segmasker and does not reproduce its output.
 * Ranges: window 4 .. 64 (default 12), 0 < k1 <= k2 <= log2 window in bits (defaults 2.2 and 2.5, SEG's). */
typedef struct lx_seg_params
{
    int32_t window;
    double  k1, k2;
} lx_seg_params;
void lx_seg_params_default(lx_seg_params * p);
/* the rule's tables, as the host function and the kernels use them; LX_EINVAL outside the ranges above */
int  lx_seg_tables(lx_seg_params const * p, int64_t T[65], int64_t * thr1, int64_t * thr2);
/* A query mask: per letter of a sequence set (indexed like q_res) whether it is masked.  Destroy it before its handle.
 *   lx_query_mask_create_seg  the rule above.  h != NULL: q_res and the sequence table go up and kernels on h's device and stream make
 *                             the mask, which stays resident there (lx_last_phase_ms(h, 15, ...) = their device time); h == NULL:
 *                             the same rule on host_threads host threads (0 = the library's share).
 *   lx_query_mask_create      from given 0 / 1 bytes, indexed like q_res (any rule of the caller's); h != NULL: also uploaded.
 *   lx_query_mask_info        letters of the set, masked letters, sequences with a masked letter (any may be NULL).
 *   lx_query_mask_copy        0 / 1 per letter into masked[0 .. end of the last sequence), 0 between sequences; a device mask comes
 *                             down on first use.
 * LX_EINVAL with a text (lx_last_output_error(), and lx_last_error(h) with a handle), before any device work: NULL arguments,
 * parameters outside the ranges, a sequence outside the address range, and sequences with letters that are not in ascending order
 * without overlap (a letter of two sequences has no mask byte of its own). */
typedef struct lx_query_mask lx_query_mask;
int  lx_query_mask_create_seg(lx_handle * h, uint8_t const * q_res, uint64_t const * q_off, uint64_t const * q_len, uint64_t n_qseq, lx_seg_params const * p,
                              uint32_t host_threads, lx_query_mask ** out);
int  lx_query_mask_create(lx_handle * h, uint8_t const * masked, uint64_t const * q_off, uint64_t const * q_len, uint64_t n_qseq, lx_query_mask ** out);
int  lx_query_mask_info(lx_query_mask const * m, uint64_t * n_letters, uint64_t * n_masked, uint64_t * n_seqs_masked);
int  lx_query_mask_copy(lx_query_mask const * m, uint8_t * masked);
void lx_query_mask_destroy(lx_query_mask * m);
/* The nucleotide rule: symmetric DUST (Morgulis et al. 2006) on alignment ranks, in integers.  A, C, G, T = 0 .. 3; any other rank
 * (N) is a break: never masked, and in no interval, so a sequence is a set of maximal stretches of ranks 0 .. 3, each on its own.
 * (These are lambda3 searchbs' ranks; a caller with the ranks A, C, G, N, T, as searchn's, exchanges 3 and 4 in the letters it
 * passes here -- the rule does not care which of 0 .. 3 is which letter.)
 *   Letter i of a stretch starts triplet 16 a[i] + 4 a[i + 1] + a[i + 2].  An interval of l consecutive triplets covers l + 2 letters;
 *   with r = the sum over the 64 triplet kinds of c (c - 1) / 2, c the count of the kind in the interval, its score is r / (l - 1) for
 *   l >= 2 and 0 for l = 1 (scores are compared by cross-multiplication).  An interval is perfect when 10 r > level (l - 1) and no
 *   sub-interval scores strictly higher.  A letter is masked exactly when it lies in a perfect interval of at most `window` letters.
 * dustmasker's -linker is NOT built, and the masks were not compared with dustmasker's or sdust's: the claim is the rule as stated.
 * Ranges: window 4 .. 64 (default 64), level 1 .. 1000 (default 20): dustmasker's and sdust's defaults.
 * lx_query_mask_create_dust has lx_query_mask_create_seg's contract (h != NULL: by kernels, resident, phase 15; h == NULL: on
 * host_threads host threads; the same LX_EINVAL refusals) and makes an ordinary lx_query_mask. */
typedef struct lx_dust_params
{
    int32_t window, level;
} lx_dust_params;
void lx_dust_params_default(lx_dust_params * p);
int  lx_query_mask_create_dust(lx_handle * h, uint8_t const * q_res, uint64_t const * q_off, uint64_t const * q_len, uint64_t n_qseq, lx_dust_params const * p,
                               uint32_t host_threads, lx_query_mask ** out);
/* lx_seed_queries with a mask (m == NULL: exactly lx_seed_queries).  A start p of a sequence is blocked when one of the seed's first
 * seed_length letters, [p, p + seed_length), is masked.  The loop that moves a start off the unknown letter passes a blocked start
 * over in the same way; it stops at L - seed_length, and a start that is still blocked there makes no seed, which ends the frame.
 * Adaptive elongation may run on over masked letters; the bookkeeping of the reads' lengths is unchanged.  On a handle the seeding
 * kernel reads the device mask where it stands; only the reads the device declines use the host copy.  LX_EINVAL in addition to
 * lx_seed_queries': a mask whose sequence table differs from the call's (n_qseq, offsets or lengths), a device call with a
 * host-only mask or a mask of another handle. */
int  lx_seed_queries_masked(lx_handle * h, lx_index const * ix, uint8_t const * s_res, uint8_t const * q_res, uint8_t const * q_red, uint64_t const * q_off,
                            uint64_t const * q_len, uint64_t n_qseq, uint64_t const * reads, uint64_t n_reads, lx_query_mask const * m, lx_seed_params const * p,
                            lx_seed_result ** out);

/* ---- misc ------------------------------------------------------------------------------------ */
/* Blocks until everything queued on the handle's stream has finished. */
int lx_synchronize(lx_handle * h);
/* Duration in ms of the most recent score / align kernel launch sequence on this handle, measured with HIP
 * events on the launch stream (valid after lx_synchronize or a host-buffer call). */
int lx_last_kernel_ms(lx_handle * h, float * ms);
/* Name of the kernel instantiation the most recent pass-1 launch used, e.g. "lx::score_kernel<8,19,false> shared-profile"
 * (profiling aid: matches the kernel names rocprofv3 reports). */
char const * lx_last_kernel_name(lx_handle const * h);
char const * lx_last_trace_kernel_name(lx_handle const * h);
/* Device time (HIP events on the launch stream) the most recent call spent in one phase, summed over its launches:
 * phase 0 = pass-1 score kernel, 1 = survivor selection, 2 = pass-2 forward kernel, 3 = pass-2 backtrace kernel,
 * 4 = BGZF encoder (lx_bgzf_compress), 5 = BGZF decoder (lx_gunzip), 6 = accession-to-taxon join (lx_taxmap_*),
 * 7 = _writeRecord's sort / unique / sort / cut on the device (lx_postprocess_records_dev, lx_iterate_matches_dev_top and their _ex
 *     forms, whose two culling kernels count here as well),
 * 8 = the word table's kernels (lx_index_build on a handle; in slices: launches = the number of slices), 9 = the seeding kernel (lx_seed_queries on a handle),
 * 10 = the plain-member kernels of lx_gunzip (find, decode, resolve), 11 = the BAM record kernels (lx_render_bam_dev,
 * lx_write_bam_dev: groups, measure, scans, emit), 12 = the text record kernels (lx_render_text_dev, lx_write_text_dev: groups,
 * numbers, measure, scans, emit), 13 = the LCA kernels (lx_compute_lca_dev: query heads, fold; launches = the number of ranges),
 * 14 = the taxon filter's kernels (lx_subject_mask_create_dev: mark, climb, subjects; lx_seed_result_filter: flags + count, scatter),
 * 15 = the query masking kernels (lx_query_mask_create_seg on a handle: stops, flags, carries, fill, distances, count;
 * lx_query_mask_create_dust on a handle: stops, breaks, sweep, cover, distances, count). */
int lx_last_phase_ms(lx_handle * h, int phase, float * ms, int * launches);

#ifdef __cplusplus
}
#endif
#endif /* LAMBDA_EXT_H */
