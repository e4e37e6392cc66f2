// lx_score_f16.hip -- pass-1 score kernel in packed half precision: two extensions per lane group (gfx950 only).
//
// Same strip-systolic mapping and row-skewed recurrence as lx_score.hip (see there for the reference lines), but
// every VGPR holds the DP value of TWO extensions (A in the low half, B in the high half) that share the query, and
// the arithmetic is v_pk_add_f16 / v_pk_maximum3_f16.  On gfx950 the packed ops issue at the same rate as the
// int32 max/max3 (tools/ubench.hip), so a cell costs 7.5 issue slots instead of 11.  Scores are small integers, and
// the kernel computes on them in units of 2^-24 (hunits below: subnormals and the first binade, on which gfx950 issues
// at the same rate -- profiles/r11_ubench_subnormal.txt): half precision represents every n * 2^-24 with |n| <= 2048
// exactly and -inf stands in for "minus infinity", so
// the results are bit-identical to the int32 kernel AS LONG AS no intermediate exceeds 2048.  That is decided per
// wavefront from an upper bound:
//         sum_j max(0, max_b s(q_j, b))  +  |ge| * (rows processed)  +  max entry  +  B  <=  2046
// (a local alignment cannot score more than the sum of the best positive score of each query column; B: below).  A wavefront
// that fails the test writes the sentinel -1 for its extensions and the host follows up with the int32 kernel in
// "fix-up" mode, which recomputes exactly those.  Nothing is approximated.
//
// The biased frame.  Two of the three adds per pair of cells add a wave-constant gap cost: A = h + g2 and E = max(E, A) + ge.
// The bit pattern of a non-negative value n * 2^-24 is n, so such an add is ONE 32-bit integer subtract of |c| * 0x10001 for
// both halves -- v_sub_u32 with two VGPR operands, which gfx950 issues at about 1.75 times the rate of the packed ops
// (profiles/r03_ubench_valu_issue_rates.txt; in the sweep's dependent mix: profiles/r12_ubench_swar.txt) -- as long as no half
// borrows, i.e. the minuend is a non-negative pattern >= the subtrahend in BOTH halves.  For that the skewed frame is raised by
//         B = |g2| + |ge| * G :      Z starts at ge * g + B  >=  |g2| + |ge|  (smallest in lane group G - 1 at step 0)
// and grows by |ge| per step.  Then, in every lane, half and step:
//   * F0 >= Z: it starts at Z and is max3(F0, A, ZN) afterwards, ZN being the next step's Z;
//   * h = max3(tt, E, F0) >= F0 >= Z > 0, whatever tt and E are: columns beyond the query and rows before or behind the window
//     (profile rows of the pad letter, tt far below) and the first lane group's E = -inf only lose that maximum;
//   * A = h - |g2| >= Z - |g2| >= |ge|: no borrow, A is finite and >= 0;
//   * max(E, A) >= A is finite (-inf, 0xfc00, never reaches a subtract), and E' = max(E, A) - |ge| >= 0: no borrow.
// An idle half (an extension beyond the list) is always the HIGH half or the whole pair: its letters are pad letters or valid
// subject bytes and the same argument holds; and a borrow out of the high half would leave the register, never enter the low one.
// Everything that leaves the kernel is a difference of two values of one frame -- the codes h - Z, h - E, Hrow - z_i,
// Hrow - F0 - ge, and rowmax - Z for the best score -- so B cancels: nothing but Z's start value, the two subtracts and the
// exactness test knows about it.  The third add, tt = dg + sub, adds a profile entry that may be negative: it stays packed.
// B is tested as the plain integer it is (never through hunits' clamp); lx_set_scoring admits |g2| <= 119 and |ge| <= 27, so
// B <= 551, and the planner adds the same B to its a-priori bound (lx_step_plan.cpp, half_frame_bias).
//
// LDS: one query profile per wavefront in half precision, lane-contiguous rows (24 halves = 48 B per lane per subject
// letter, read with two ds_read_b128 + one ds_read_b64); the two subject letters of a lane give two reads whose
// halves are interleaved with one v_perm_b32 per column.  All extensions of a wavefront (16, or 8 for G = 16) must share the query
// (LX_OPT_QUERY_RUN multiple of 16, or host-side padding).
#include <hip/hip_runtime.h>

#include "lx_aids.h"
#include "lx_dp_common.h"

namespace lx
{

typedef _Float16 h2 __attribute__((ext_vector_type(2)));

#ifndef LX_F16_UNROLL
#define LX_F16_UNROLL 2 // steps unrolled in the main loop: 2 removes the register-rotation moves at 168 VGPRs
#endif
#ifndef LX_F16_CKPT_WAVES
#define LX_F16_CKPT_WAVES 3 // wavefronts per SIMD the checkpointing instantiations are compiled for (headline sweep: 2 -> 12.1 ms, 3 -> 11.9 ms; steps unrolled 1 / 2 / 4 -> 12.7 / 11.9 / 12.0 ms)
#endif
#define LX_PRAGMA(x) _Pragma(#x)
#define LX_UNROLL(n) LX_PRAGMA(unroll n)

__device__ __forceinline__ h2 hmax3(h2 a, h2 b, h2 c)
{
    return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c); // v_pk_maximum3_f16
}
__device__ __forceinline__ h2 hmax(h2 a, h2 b)
{
    return __builtin_elementwise_maximum(a, b);
}
__device__ __forceinline__ h2 as_h2(uint32_t x)
{
    return __builtin_bit_cast(h2, x);
}
__device__ __forceinline__ uint32_t as_u32(h2 x)
{
    return __builtin_bit_cast(uint32_t, x);
}

// The kernel's unit is 2^-24: the integer n stands as n * 2^-24, a half-precision subnormal (|n| < 1024) or a value of the
// first binade, both spaced 2^-24 -- sums and maxima of such values are as exact as those of the integers themselves as long
// as |n| <= 2047, and the bit pattern of a non-negative value IS n (FP16 denormals are on in the kernel descriptor, the
// compiler's default).  Minus infinity stays 0xfc00.  (a gap cost beyond -2047 acts like -2047: no value reaches that far)
__device__ __forceinline__ h2 hunits(int n)
{
    uint32_t const m = (uint32_t)min(n < 0 ? -n : n, 2047);
    return as_h2((n < 0 ? 0x8000u | m : m) * 0x10001u);
}
__device__ __forceinline__ int units_of(uint32_t half_bits) // of a value >= 0
{
    return (int)(half_bits & 0x7fffu);
}
constexpr uint32_t kHalfNegInf2 = 0xfc00fc00u; // (-inf, -inf)

// Ckpt16Layout codes without a conversion instruction: both fields are non-negative values in the kernel's unit, whose bit
// patterns are the integers themselves.
__device__ __forceinline__ uint32_t c16_pack(h2 value, h2 diff)
{
    return (as_u32(diff) << 11) | as_u32(value); // both halves at once: diff < 32 stays inside its half
}

template <int G, int C>
struct PairGeo
{
    static constexpr int kGroups   = 64 / G;                 // lane groups per wavefront, two extensions each
    static constexpr int kPanel    = G * C;
    static constexpr int kUsedDw   = (C + 1) / 2;            // dwords that hold real columns
    static constexpr int kLaneDw   = (kUsedDw + 3) & ~3;     // halves of a lane's columns per profile row, 16-byte granules
    // (padding the rows to spread different subject letters over more bank offsets was measured: no effect -- the
    // kernel is VALU-issue bound, LDS is ~1/3 busy including its bank conflicts)
    static constexpr int kRowDw    = kLaneDw * G;
};

// CKPT = single sweep: the kernel additionally writes what pass 2's backtrace needs (layout and meaning as in
// lx_ckpt.hip: strip boundaries per step, row checkpoints every 16 steps, here as the compact codes of CkptPairLayout) and
// keeps, per strip and extension, the best value, the block of sixteen steps whose rows reached it first and whether a later block tied.
template <int G, int C, bool CKPT>
__global__ __launch_bounds__(64, (CKPT ? (C > 19 ? 2 : LX_F16_CKPT_WAVES) : 1)) void score_pair_kernel(ScoreParams p) // (25-column strips: 168 VGPRs spill, and their LDS profile leaves 9 wavefronts per CU anyway)
{
    static_assert(C <= 32, "profile rows hold 32 halves per lane");
    using Geo = PairGeo<G, C>;
    extern __shared__ uint32_t lds[];

    static_assert(G == 8 || G == 16, "lane groups of half a DPP row or a whole one");
    // G = 8: the two lane groups of a 16-lane DPP row sit on its even and its odd lanes.  A strip's left neighbour is then
    // row_shr:2, and the first lane of either group has no source lane in its row: with bound_ctrl off it keeps the DPP's
    // `old` operand, so the left boundary needs no select (G = 16: row_shr:1 does the same).  kGs = lanes between two strips.
    constexpr int kGs     = G == 8 ? 2 : 1;
    constexpr int kDppShr = 0x110 + kGs; // row_shr:kGs
    int const  lane     = threadIdx.x;
    int const  g        = G == 8 ? (lane & 15) >> 1 : lane % G;
    int const  grp      = G == 8 ? ((lane >> 4) << 1) | (lane & 1) : lane / G;
    bool const is_first = (g == 0);
    auto lane_of = [](int group, int strip) { return G == 8 ? ((group >> 1) << 4) | (strip << 1) | (group & 1) : group * G + strip; };

    uint64_t const pair   = (uint64_t)blockIdx.x * Geo::kGroups + grp;
    uint64_t const eA     = 2 * pair, eB = 2 * pair + 1;
    bool const     actA   = eA < p.n, actB = eB < p.n;

    ScoringDev const * __restrict__ sc = p.sc;
    int const      ge    = sc->ge;
    int const      nrows = p.nrows;
    uint32_t const padt  = (uint32_t)(nrows - 1);

    int             lq = 0, lsA = 0, lsB = 0;
    uint8_t const * q  = p.q_res;
    uint8_t const * sA = p.s_res;
    uint8_t const * sB = p.s_res;
    uint64_t        q_off = 0;
    if (actA)
    {
        Extension const x = p.ext[eA];
        lq    = (int)x.q_len;
        q_off = x.q_off;
        q += x.q_off;
        lsA = (int)x.s_len;
        if (lsA != 0)
            sA += x.s_off;
    }
    uint64_t q_offB = q_off;
    int      lqB    = lq;
    if (actB)
    {
        Extension const x = p.ext[eB];
        lqB    = (int)x.q_len;
        q_offB = x.q_off;
        lsB    = (int)x.s_len;
        if (lsB != 0)
            sB += x.s_off;
    }
    // p.pair_share lane groups (0 = all of them) use one LDS profile: the extensions of such a block share the query
    int const share_g = (p.pair_share > 0 && p.pair_share < Geo::kGroups) ? p.pair_share : Geo::kGroups;
    int const blk     = grp / share_g;
    uint64_t  q_blk;  // the block's query as its first lane has it: the profile below is built from these by all of its lanes
    int       lq_blk;
    {
        // the caller promised one query per block: verify against the block's first lane, fail loudly otherwise
        int const      leader = lane_of(blk * share_g, 0);
        uint64_t const q0     = ((uint64_t)(uint32_t)__shfl((int)(q_off >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)q_off, leader);
        int const      l0     = __shfl(lq, leader);
        bool const     lead_in = __shfl(actA ? 1 : 0, leader) != 0;
        if (lead_in && ((actA && (q_off != q0 || lq != l0)) || (actB && (q_offB != q0 || lqB != l0))))
            atomicExch(p.err, 2);
        q_blk  = q0;
        lq_blk = l0;
    }

    int ls_max = max(lsA, lsB);
    int ls_min = min(actA ? lsA : 0x7fffffff, actB ? lsB : 0x7fffffff);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
    {
        ls_max = max(ls_max, __shfl_xor(ls_max, off));
        ls_min = min(ls_min, __shfl_xor(ls_min, off));
    }
    ls_max = __builtin_amdgcn_readfirstlane(ls_max);
    ls_min = __builtin_amdgcn_readfirstlane(ls_min);
    int const steps = (ls_max + G - 1 + 3) & ~3;

    // ---- exactness test (wave-uniform): an upper bound of every intermediate must stay <= 2046
    // (first the bound no query of this length exceeds -- every column at the matrix' largest entry: where that passes for the whole
    // wavefront, the residues need not be looked at: two dependent loads per column in front of everything else)
    int const col0  = g * C;
    int       bound = lq * sc->smax;
    int const bias  = (-sc->g2) + (-ge) * G; // B of the biased frame (header comment): plain integers, never hunits' clamp
    if (__ballot(bound + (-ge) * (steps + G + 2) + sc->smax + 2 + bias > 2046) != 0)
    {
        bound = 0;
#pragma unroll
        for (int c = 0; c < C; ++c)
        {
            int const j = col0 + c;
            if (j < lq)
                bound += sc->rowmax[q[j] & (kAlph - 1)];
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1)
            bound += __shfl_xor(bound, off * kGs);
    }
    // (every group summed its own query; one block over the limit sends the whole wavefront to the fix-up launch)
    bool too_big = __ballot((lq > Geo::kPanel) || (bound + (-ge) * (steps + G + 2) + sc->smax + 2 + bias > 2046)) != 0;
    if constexpr (CKPT)
    {
        // LX_OPT_MAX_QLEN / LX_OPT_MAX_SLEN promise broken: reported here (the int32 launch, which would report it too, is
        // skipped when no query the promise admits can fail the exactness test)
        bool const broken = (__ballot(lq > Geo::kPanel) != 0) || (uint32_t)steps > p.steps_cap;
        if (broken && lane == 0)
            atomicExch(p.err, 3);
        too_big = too_big || broken;
    }

    if (too_big)
    {
        if (is_first)
        {
            if (actA)
                p.out_score[eA] = -1;
            if (actB)
                p.out_score[eB] = -1;
            if constexpr (CKPT)
            {
                EndCell none{};
                none.score = -1; // until the int32 fix-up launch has been here
                if (actA)
                    p.ends[eA] = none;
                if (actB)
                    p.ends[eB] = none;
            }
        }
        return;
    }

    // ---- profile: prof[t][g][h] = (s(q_col, t) - ge) as half (in the kernel's unit, as ScoringDev::mat_h holds it), lane-contiguous
    // Built by every lane of the block that shares it.  A unit of work is one dword column d of one strip (two query columns)
    // for eight letters: one 16-byte load from the matrix row of either column, eight permutes, eight LDS writes.  The units are
    // dealt round robin; letters at or beyond nrows are not built (the small alphabets have one group of eight).
    int const slot_dw = blk * (nrows * Geo::kRowDw);
    {
        constexpr int  kStripDw = G * Geo::kUsedDw;           // (strip, dword column) pairs of the panel
        int const      units    = ((nrows + 7) >> 3) * kStripDw;
        int const      in_blk   = (grp - blk * share_g) * G + g; // this lane among the block's share_g * G
        uint8_t const * qb      = p.q_res + q_blk;             // the block's query (every lane builds for every strip)
#pragma unroll 1
        for (int u = in_blk; u < units; u += share_g * G)
        {
            int const x  = u / kStripDw;                      // letters 8 x .. 8 x + 7
            int const sd = u - x * kStripDw;
            int const sg = sd / Geo::kUsedDw, d = sd - sg * Geo::kUsedDw;
            uint4     rows[2];
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
            {
                int const c  = 2 * d + cc;
                int const j  = sg * C + c;
                uint32_t  ql = kAlph - 1;
                if (c < C && j < lq_blk)
                    ql = qb[j] & (kAlph - 1);
                rows[cc] = reinterpret_cast<uint4 const *>(sc->mat_h + ql * kAlph)[x];
            }
            uint32_t const r0[4] = {rows[0].x, rows[0].y, rows[0].z, rows[0].w}, r1[4] = {rows[1].x, rows[1].y, rows[1].z, rows[1].w};
            uint32_t *     dst   = lds + slot_dw + (8 * x) * Geo::kRowDw + sg * Geo::kLaneDw + d;
#pragma unroll
            for (int w = 0; w < 4; ++w)
            {
                if (8 * x + 2 * w < nrows)
                {
                    // letters t = 8x + 2w (low halves) and t + 1 (high halves) of both columns
                    dst[(2 * w) * Geo::kRowDw]     = __builtin_amdgcn_perm(r1[w], r0[w], 0x05040100u);
                    dst[(2 * w + 1) * Geo::kRowDw] = __builtin_amdgcn_perm(r1[w], r0[w], 0x07060302u);
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    uint32_t const row_base  = (uint32_t)(slot_dw + g * Geo::kLaneDw) * 4u;
    constexpr uint32_t kRowBytes = Geo::kRowDw * 4;

    h2 const GE = hunits(ge), NGE = hunits(-ge);
    // the two wave-constant gap adds of the column step as 32-bit integer subtracts of both halves at once (header comment);
    // the constants are pinned in VGPRs: v_sub_u32 is full-rate only with two VGPR operands (tools/ubench.hip)
    // (the 24-column score-only form keeps the packed adds: it stands at 167 VGPRs, and two more cost it the third wavefront per
    // SIMD -- 192-column queries, pass 1 alone: 15.14 -> 15.31 ms with the subtracts)
    constexpr bool kIntSub = CKPT || C != 24;
    h2 const       G2 = hunits(sc->g2);
    uint32_t       G2u = (uint32_t)(-sc->g2) * 0x10001u, GEu = (uint32_t)(-ge) * 0x10001u;
    if constexpr (kIntSub)
        asm volatile("" : "+v"(G2u), "+v"(GEu));
    h2       Z  = hunits(ge * g + bias); // z_i of the first processed row i = -g, plus the frame's bias
    h2       Hrow[C], F0[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
    {
        Hrow[c] = Z + GE;
        F0[c]   = Z;
    }
    h2 diag0 = Z + GE;
    h2 sendH = Z + GE;
    h2 sendE = as_h2(kHalfNegInf2);
    h2 recvE = as_h2(kHalfNegInf2); // E from the left: the shift's own `old`, so a group's first lane stays at -inf for good
    h2 best  = hunits(0);
    // CKPT: first row that reached this strip's best value, "a later row reached it again" (bit 0 = A, bit 1 = B)
    int      rowA = 0, rowB = 0;
    uint32_t tie  = 0;
    h2       cmax = as_h2(kHalfNegInf2); // best un-skewed row maximum of the current chunk
    // Pair slots (CkptPairLayout, lx_device.h): the region of this wavefront's W windows holds the code dwords as the registers
    // do, window A in the low half and B in the high one -- nothing is re-paired on the way out.  An idle half's codes ride along
    // in its pair's dwords; nobody reads them.
    using Lay = CkptPairLayout<G, C>;
    constexpr uint32_t kW       = 2 * Geo::kGroups;
    uint4 * const      waveBase = CKPT ? reinterpret_cast<uint4 *>(p.ckpt + (uint64_t)blockIdx.x * kW * p.ckpt_stride) : nullptr;
    uint4 * const      bndBase  = CKPT ? waveBase + Lay::bnd_quad_index((uint32_t)grp, 0, (uint32_t)g) : nullptr;
    uint4 * const      ckBase   = CKPT ? waveBase + kW * (uint32_t)(Lay::bnd_dwords(p.steps_cap) / 4) + Lay::rowck_quad_index((uint32_t)grp, 0, (uint32_t)g, 0) : nullptr;
    constexpr uint32_t kOctMul  = Lay::bnd_quad_index(0, 8, 0);      // uint4 units between two groups of eight steps
    constexpr uint32_t kHalfOct = Lay::bnd_quad_index(0, 4, 0);      // ... between the two quads of a group
    constexpr uint32_t kCkMul   = Lay::rowck_quad_index(0, 1, 0, 0); // ... between two row checkpoints
    // staging of the boundary codes: [step % 8][lane] -- lane-minor, free of bank conflicts
    uint32_t * const stage = lds + ((Geo::kGroups + share_g - 1) / share_g) * (nrows * Geo::kRowDw) + lane;

    // (slot8 = step % 8: where the step's boundary codes are staged)
    auto step = [&](uint32_t tA, uint32_t tB, int slot8)
    {
        uint4 const * ra = reinterpret_cast<uint4 const *>(reinterpret_cast<char const *>(lds) + row_base + tA * kRowBytes);
        uint4 const * rb = reinterpret_cast<uint4 const *>(reinterpret_cast<char const *>(lds) + row_base + tB * kRowBytes);
        uint32_t      pa[Geo::kLaneDw], pb[Geo::kLaneDw];
#pragma unroll
        for (int x = 0; x < (Geo::kUsedDw + 3) / 4; ++x)
        {
            if (4 * x + 2 >= Geo::kUsedDw) // only two more dwords are needed: ds_read_b64
            {
                uint2 const va = *reinterpret_cast<uint2 const *>(ra + x), vb = *reinterpret_cast<uint2 const *>(rb + x);
                pa[4 * x] = va.x; pa[4 * x + 1] = va.y;
                pb[4 * x] = vb.x; pb[4 * x + 1] = vb.y;
            }
            else
            {
                uint4 const va = ra[x], vb = rb[x];
                pa[4 * x] = va.x; pa[4 * x + 1] = va.y; pa[4 * x + 2] = va.z; pa[4 * x + 3] = va.w;
                pb[4 * x] = vb.x; pb[4 * x + 1] = vb.y; pb[4 * x + 2] = vb.z; pb[4 * x + 3] = vb.w;
            }
        }

        // left boundary: H[i][-1] = 0 (skewed: z), E = -inf
        h2 const recvH = as_h2((uint32_t)__builtin_amdgcn_update_dpp((int)as_u32(Z), (int)as_u32(sendH), kDppShr, 0xf, 0xf, false));
        recvE          = as_h2((uint32_t)__builtin_amdgcn_update_dpp((int)as_u32(recvE), (int)as_u32(sendE), kDppShr, 0xf, 0xf, false));
        h2       Ecur  = recvE;
        h2       dg    = diag0;
        diag0          = recvH;

        h2 const ZN     = Z + NGE;
        h2       rowmax = as_h2(kHalfNegInf2);
        h2       h      = Z;
#pragma unroll
        for (int c = 0; c < C; ++c)
        {
            // (score of column c vs letter tA, score of column c vs letter tB)
            uint32_t const sel = (c & 1) ? 0x07060302u : 0x05040100u;
            h2 const       sub = as_h2(__builtin_amdgcn_perm(pb[c >> 1], pa[c >> 1], sel));
            h2 const       tt  = dg + sub;
            dg                 = Hrow[c];
            h                  = hmax3(tt, Ecur, F0[c]);
            h2 const A         = kIntSub ? as_h2(as_u32(h) - G2u) : h + G2; // h + g2: h >= Z >= |g2| in both halves
            F0[c]              = hmax3(F0[c], A, ZN); // (floating-point max is not re-associated: no fences needed)
            Ecur               = kIntSub ? as_h2(as_u32(hmax(Ecur, A)) - GEu) : hmax(Ecur, A) + GE; // max(E, A) + ge: A is finite and >= |ge|
            Hrow[c]            = h;
            if (c & 1)
                rowmax = hmax3(rowmax, Hrow[c - 1], h);
        }
        if (C & 1)
            rowmax = hmax(rowmax, h);
        sendH = h;
        sendE = Ecur;
        h2 const cand = rowmax - Z;
        if constexpr (CKPT)
        {
            // (the rose / met-again logic runs once per block of sixteen steps -- book; the main loop's two unrolled steps share one
            // v_pk_maximum3_f16 for this: the compiler folds the two maxima)
            cmax = hmax(cmax, cand);
            // un-skewed boundary pair (H of the strip's last column, E as the next strip's first column uses it) as
            // 16-bit codes of both extensions in one dword, staged for two 16-byte stores per pair every eight steps
            stage[slot8 * 64] = c16_pack(h - Z, h - Ecur);
        }
        else
            best = hmax(best, cand);
        Z = ZN;
    };
    // CKPT: the staged codes of the eight steps up to k0 + 3 leave as they stand, two quads of four steps: whole 128-byte lines
    // per lane group, no branch around the stores.
    auto flush_codes = [&](int k0)
    {
        if constexpr (CKPT)
        {
            uint32_t cw[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                cw[u] = stage[u * 64];
            uint4 * const dst = bndBase + ((uint32_t)k0 / 8) * kOctMul;
            dst[0]        = make_uint4(cw[0], cw[1], cw[2], cw[3]);
            dst[kHalfOct] = make_uint4(cw[4], cw[5], cw[6], cw[7]);
        }
    };
    // CKPT: the best-value bookkeeping, once per block of sixteen steps (the backtrace's tiles are these blocks: its first tile looks
    // at every row of the block up to the one reported here -- lx_ckpt.hip, need_col).  Per four steps, as rounds 2-5 had it, the
    // selects below were 3 % of the sweep's issue slots.
    auto book = [&](int k0) // k0: the first of the block's last four steps
    {
        if constexpr (CKPT)
        {
            // per half: did the strip's best rise in this block (then its first row is one of the block's sixteen; the
            // backtrace finds it), or was it only met again (a tie for the end cell)?  Rows beyond the window and
            // columns beyond the query stay strictly below a positive best: no validity test.
            h2 const       nb   = hmax(best, cmax);
            uint32_t const rose = as_u32(nb) ^ as_u32(best), met = as_u32(cmax) ^ as_u32(best);
            bool const     gtA = (rose & 0xffffu) != 0, gtB = (rose >> 16) != 0;
            bool const     eqA = (met & 0xffffu) == 0, eqB = (met >> 16) == 0;
            int const last = k0 + 3 - g; // the block's last row in this lane
            rowA = gtA ? last : rowA;
            rowB = gtB ? last : rowB;
            tie  = (gtA ? (tie & ~1u) : (tie | (eqA ? 1u : 0u)));
            tie  = (gtB ? (tie & ~2u) : (tie | (eqB ? 2u : 0u)));
            best = nb;
            cmax = as_h2(kHalfNegInf2);
        }
    };
    // CKPT: after every eighth step the staged boundary codes leave
    auto chunk_done = [&](int k0)
    {
        if constexpr (CKPT)
        {
#ifndef LX_EXP_NO_FLUSH
            if (k0 & 4)
                flush_codes(k0);
#endif
        }
    };
    // CKPT: the row checkpoint behind step k0 + 3 (k0 % 16 == 12).  Issued at the top of the next chunk, before that
    // chunk's loads, so that these stores never stand between a load and its wait (see chunk_done).
    auto rowck_store = [&](int k0)
    {
        if constexpr (CKPT)
        {
            // Hrow is in the frame of the row just processed (z_i = Z + ge after the update), F0 in the next row's:
            // H - F un-skewed = (Hrow - z_i) - (F0 - Z) = Hrow - F0 - ge.  (Hrow - F0 alone is no field for a code: the folded F has
            // the floor 0 of the local alignment in it, so where H < -ge the difference is negative.)
            h2 const      zi  = Z + GE;
            uint4 * const dst = ckBase + ((uint32_t)(k0 + 3) / 16) * kCkMul;
#pragma unroll
            for (int x = 0; x < Lay::kCkQuads; ++x)
            {
                uint32_t code[4]; // columns 4 x .. 4 x + 3 of both windows
#pragma unroll
                for (int b = 0; b < 4; ++b)
                {
                    int const c = 4 * x + b;
                    code[b]     = c < C ? c16_pack(Hrow[c < C ? c : 0] - zi, (Hrow[c < C ? c : 0] - F0[c < C ? c : 0]) + NGE) : 0u;
                }
                dst[x] = make_uint4(code[0], code[1], code[2], code[3]);
            }
        }
    };

    uint32_t const lscA = (uint32_t)max(lsA, 1) - 1u, lscB = (uint32_t)max(lsB, 1) - 1u;
    auto fetch_checked = [&](int k0, uint32_t (&ta)[4], uint32_t (&tb)[4])
    {
#pragma unroll
        for (int u = 0; u < 4; ++u)
        {
            uint32_t const i = (uint32_t)(k0 + u - g);
            ta[u]            = sA[min(i, lscA)];
            tb[u]            = sB[min(i, lscB)];
        }
    };
    auto mask_checked = [&](int k0, uint32_t (&ta)[4], uint32_t (&tb)[4])
    {
#pragma unroll
        for (int u = 0; u < 4; ++u)
        {
            uint32_t const i = (uint32_t)(k0 + u - g);
            ta[u]            = (i < (uint32_t)lsA) ? (ta[u] & (kAlph - 1)) : padt;
            tb[u]            = (i < (uint32_t)lsB) ? (tb[u] & (kAlph - 1)) : padt;
        }
    };

    int const steady_lo = (G - 1 + 3) & ~3;
    int const steady_hi = ls_min - 3;
    uint8_t const * spA = sA - g;
    uint8_t const * spB = sB - g;

    // The letters of the NEXT chunk are loaded at a chunk's top and taken over behind its steps, IN FRONT of its checkpoint stores:
    // gfx950 counts loads and stores with one in-order counter, so a wait for a load that stands behind stores is a wait for the
    // stores' acknowledgements from HBM (rounds 1-4 took the letters over at the loop's end, behind the stores: `s_waitcnt vmcnt(0)`
    // straight after them in every chunk -- a fifth of the sweep's wave cycles parked there).  The empty asm is the use that pins
    // the wait; the row checkpoint follows the chunk it belongs to instead of opening the next one.
    auto chunk_stores = [&](int k0)
    {
        chunk_done(k0);
        if (((k0 + 4) & 15) == 0)
        {
            book(k0);
#ifndef LX_EXP_NO_ROWCK
            rowck_store(k0);
#endif
        }
    };
    int      k0 = 0;
    uint32_t na[4], nb[4];
    fetch_checked(0, na, nb);
    while (k0 < steps)
    {
        bool const cur_steady = (k0 >= steady_lo) && (k0 < steady_hi);
        if (!cur_steady)
        {
            uint32_t ca[4] = {na[0], na[1], na[2], na[3]}, cb[4] = {nb[0], nb[1], nb[2], nb[3]};
            mask_checked(k0, ca, cb);
            fetch_checked(k0 + 4, na, nb);
#pragma unroll 1
            for (int u = 0; u < 4; ++u)
                step(ca[u], cb[u], (k0 & 4) + u);
            if constexpr (CKPT)
                asm volatile("" : "+v"(na[0]), "+v"(na[1]), "+v"(na[2]), "+v"(na[3]), "+v"(nb[0]), "+v"(nb[1]), "+v"(nb[2]), "+v"(nb[3])::"memory");
            chunk_stores(k0);
            k0 += 4;
        }
        else
        {
            uint32_t wa = *reinterpret_cast<unaligned_u32 const *>(spA + k0);
            uint32_t wb = *reinterpret_cast<unaligned_u32 const *>(spB + k0);
            if constexpr (CKPT) // (here, once, and not as a pending load that the loop's first use waits for in every iteration)
                asm volatile("" : "+v"(wa), "+v"(wb)::"memory");
            while (k0 < steady_hi)
            {
                uint32_t const ca = wa, cb = wb;
                int const      kn = max(min(k0 + 4, ls_min - 4), 0);
                wa                = *reinterpret_cast<unaligned_u32 const *>(spA + kn);
                wb                = *reinterpret_cast<unaligned_u32 const *>(spB + kn);
LX_UNROLL(LX_F16_UNROLL)
                for (int u = 0; u < 4; ++u)
                    step((ca >> (8 * u)) & (kAlph - 1), (cb >> (8 * u)) & (kAlph - 1), (k0 & 4) + u);
                if constexpr (CKPT)
                    asm volatile("" : "+v"(wa), "+v"(wb)::"memory");
                chunk_stores(k0);
                k0 += 4;
            }
            fetch_checked(k0, na, nb);
        }
    }
    if (steps & 4)
        flush_codes(steps); // the last four steps' codes (the other half of the group is stale: beyond every row)
    if (steps & 15)
        book(steps - 4); // the last, partial block

    if constexpr (!CKPT)
    {
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1)
            best = hmax(best, as_h2((uint32_t)__shfl_xor((int)as_u32(best), off * kGs)));

        if (is_first)
        {
            if (actA)
                p.out_score[eA] = units_of(as_u32(best));
            if (actB)
                p.out_score[eB] = units_of(as_u32(best) >> 16);
        }
    }
    else
    {
        // per extension: best strip value over the group; among equal ones the lowest strip (its columns come first)
        auto finish = [&](int lbest, int lrow, int ltie, bool act, uint64_t e)
        {
            int gbest = lbest, gstrip = g, grow = lrow, gtie = ltie;
#pragma unroll
            for (int off = 1; off < G; off <<= 1)
            {
                int const  ob = __shfl_xor(gbest, off * kGs), os = __shfl_xor(gstrip, off * kGs), orow = __shfl_xor(grow, off * kGs), ot = __shfl_xor(gtie, off * kGs);
                bool const take = ob > gbest || (ob == gbest && os < gstrip);
                gbest  = take ? ob : gbest;
                gstrip = take ? os : gstrip;
                grow   = take ? orow : grow;
                gtie   = take ? ot : gtie;
            }
            if (is_first && act)
            {
                EndCell ec{};
                if (gbest > 0)
                {
                    ec.score = gbest;
                    ec.q_end = -(gstrip + 1); // the backtrace finds the column inside this strip
                    ec.s_end = grow + 1;
                    ec.flags = (gtie ? kEndAmbiguous : 0) | kEndCompact | kEndWaveSlots | kEndPairSlots; // compact codes, a pair per dword
                }
                p.ends[e]      = ec;
                p.out_score[e] = gbest;
            }
        };
        finish(units_of(as_u32(best)), rowA, (int)(tie & 1u), actA, eA);
        finish(units_of(as_u32(best) >> 16), rowB, (int)((tie >> 1) & 1u), actB, eB);
    }
}

template <int G, int C, bool CKPT = false>
static hipError_t launch_pair_cfg(ScoreParams const & p, hipStream_t stream)
{
    using Geo = PairGeo<G, C>;
    uint64_t const per_wave = 2ull * Geo::kGroups;
    uint64_t const blocks   = (p.n + per_wave - 1) / per_wave;
    if (blocks > 0x7fffffffull)
        return hipErrorInvalidValue;
    // (the kernel deals a profile's build over the share_g lane groups of its block: every block must have that many)
    bool const   split = p.pair_share > 0 && p.pair_share < Geo::kGroups;
    int const    slots = split ? Geo::kGroups / p.pair_share : 1;
    if (split && slots * p.pair_share != Geo::kGroups)
        return hipErrorInvalidValue;
    size_t const lds = ((size_t)slots * (size_t)p.nrows * Geo::kRowDw + (CKPT ? 64 * 8 : 0)) * sizeof(uint32_t);
    hipLaunchKernelGGL((score_pair_kernel<G, C, CKPT>), dim3((unsigned)blocks), dim3(64), lds, stream, p);
    return hipGetLastError();
}

// The single sweep: the geometries lx_ckpt.hip's layout is instantiated for -- (8,13) for short queries, (8,25) for 153 - 200 columns.
// Pass 1: ScorePairGeos (lx_device.h) -- (16,10) and (16,13) hold 8 extensions per wavefront, for query runs that are a multiple of 8
// but not of 16; (8,25) takes 200-residue queries without a padded column: 7.7 against 6.7 TCUPS for (16,13).
using HalfSweepGeos = GeoList<GeoT<8, 19>, GeoT<16, 13>, GeoT<8, 13>, GeoT<8, 25>>;

hipError_t launch_score_pair(Geo geo, ScoreParams const & p, hipStream_t stream)
{
    if (p.n == 0)
        return hipSuccess;
    if (p.ckpt)
    {
        if (!p.ends || p.steps_cap % 16 != 0)
            return hipErrorInvalidValue;
        return geo_dispatch(HalfSweepGeos{}, geo, hipErrorInvalidValue, [&](auto t) { return launch_pair_cfg<t.g, t.c, true>(p, stream); });
    }
    return geo_dispatch(ScorePairGeos{}, geo, hipErrorInvalidValue, [&](auto t) { return launch_pair_cfg<t.g, t.c>(p, stream); });
}

// LDS bytes of one profile (the kernel's occupancy allows about 13 KB per wavefront)
size_t score_pair_profile_bytes(Geo geo, int nrows)
{
    return (size_t)nrows * (size_t)((((geo.c + 1) / 2 + 3) & ~3) * geo.g) * sizeof(uint32_t);
}

} // namespace lx
