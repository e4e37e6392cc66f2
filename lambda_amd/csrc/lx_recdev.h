// lx_recdev.h -- the device functions both record writers need (lx_bam.hip: BAM, lx_text.hip: .m8 / .m9 / .sam): what one record is
// made of besides its ops (rec_of: the clips of cigarOf, --sam-bam-seq, SEQ, tag qs, POS, the taxonomy of its group), the walk over
// the runs of its ops, QUAL's character beside SEQ's letter, the elements of the DNA CIGAR and of tag OC in the host writer's order, reverse complement, the codon of a
// translated query's frame, decimal digits, the functors of the group and size scans.  Restated from host/lx_output.cpp, which is the
// specification.  Included inside `namespace lx { namespace { ... } }` of a .hip file, after lx_bam.h and lx_scan.h.
#pragma once

__device__ __forceinline__ uint8_t up(uint8_t c)
{
    return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c;
}
__device__ __forceinline__ uint32_t dec_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10)
    {
        v /= 10;
        ++d;
    }
    return d;
}
__device__ __forceinline__ void put_dec(uint8_t * p, uint64_t v, uint32_t d)
{
    for (uint32_t i = d; i-- > 0;)
    {
        p[i] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
}
// reverseComplementAscii's letter
__device__ __forceinline__ uint8_t rc_letter(uint8_t c)
{
    switch (up(c))
    {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        case 'T':
        case 'U': return 'A';
        default: return 'N';
    }
}
// QueryProteins' nucleotide ranks and lx_translate_six_frames' complement
__device__ __forceinline__ uint32_t nt5(uint8_t c)
{
    switch (up(c))
    {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T':
        case 'U': return 4;
        default: return 3;
    }
}
__device__ __forceinline__ uint32_t comp5(uint32_t x)
{
    return x == 0 ? 4u : x == 1 ? 2u : x == 2 ? 1u : x == 3 ? 3u : 0u; // A <-> T (rank 4), C <-> G, N stays
}
__device__ __forceinline__ bool is_op(uint8_t o)
{
    return o == 'D' || o == 'I' || o == 'M';
}

__device__ __forceinline__ uint8_t letter(BamCtx const & c, uint64_t at)
{
    return at < c.q_ascii_bytes ? c.q_ascii[at] : (uint8_t)'N';
}

__device__ __forceinline__ uint8_t quality(BamCtx const & c, uint64_t at)
{
    return at < c.q_qual_bytes ? c.q_qual[at] : (uint8_t)'!';
}

// what one record is made of besides its ops: the same values for measure and emit
struct Rec
{
    lx_blast_match const * b;
    uint64_t               qlen, base; // the untranslated query's length, where its letters begin
    uint32_t               g, ih;      // group, its size
    bool                   first, minus;
    bool                   cig; // the program has a DNA cigar
    uint64_t               trans, lfc, rfc, lclip, rclip, frame_len;
    uint64_t               l_seq, seq_at; // letter i: seq_at + i (plus strand) / complement of seq_at - 1 - i (minus)
    uint64_t               qs_len, qs_a;  // tag qs: 0 = "*"
    int                    qs_mode;       // 1 = the query's letters, 2 / 3 = translated, plus / minus strand
    uint64_t               qs_shift;
    uint64_t               qn_at;
    uint32_t               qn_len;
    int64_t                pos; // 0-based; signed where the subject is translated (c.s_trans), else the 64 unsigned bits of s_start
    uint32_t               lca, name_off, name_len; // name_len 0xffffffff: "*"
    uint64_t               st_lo, st_hi;            // the subject's taxa (st_lo == st_hi: "*")
};

__device__ __forceinline__ Rec rec_of(BamCtx const & c, uint64_t k)
{
    Rec                    r;
    lx_blast_match const & b = c.rows[k];
    r.b                      = &b;
    r.qlen                   = c.q_lens[b.n_qid];
    bool const ascii         = c.q_ascii != nullptr && c.q_ascii_off != nullptr;
    r.base                   = ascii ? c.q_ascii_off[b.n_qid] : 0;
    r.g                      = c.grp[k];
    uint32_t const lo        = c.grp_first[r.g];
    r.ih                     = c.grp_first[r.g + 1] - lo;
    r.first                  = k == lo;
    int const qf             = (int)b.q_frame;
    int const aqf            = qf < 0 ? -qf : qf;
    r.minus                  = qf < 0;
    r.qn_at                  = c.qn_off[b.n_qid];
    r.qn_len                 = (uint32_t)(c.qn_off[b.n_qid + 1] - r.qn_at);
    // cigarOf's clips
    r.cig       = c.is_n || c.q_trans;
    r.trans     = c.q_trans ? 3 : 1;
    r.lfc       = (uint64_t)aqf - (qf != 0 ? 1 : 0);
    r.rfc       = c.q_trans ? (r.qlen - r.lfc) % 3 : 0;
    r.frame_len = c.q_trans ? (r.qlen - r.lfc) / 3 : r.qlen;
    r.lclip     = b.q_start * r.trans;
    r.rclip     = (r.frame_len - b.q_end) * r.trans;
    // --sam-bam-seq
    bool write_seq = c.sam_seq >= LX_SAM_SEQ_ALWAYS;
    if (c.sam_seq == LX_SAM_SEQ_UNIQ)
    {
        write_seq = r.first;
        if (!r.first)
        {
            lx_blast_match const & p = c.rows[k - 1];
            write_seq                = b.q_frame != p.q_frame || b.q_start != p.q_start || b.q_end != p.q_end;
        }
    }
    // SEQ
    r.l_seq  = 0;
    r.seq_at = 0;
    if (c.is_n && write_seq && ascii)
    {
        uint64_t a = 0, len = r.qlen;
        if (c.hard)
        {
            bool const ok = b.q_end <= r.qlen && b.q_start <= b.q_end;
            a             = ok ? b.q_start : 0;
            len           = ok ? b.q_end - b.q_start : 0;
        }
        r.l_seq  = len;
        r.seq_at = r.base + (r.minus ? r.qlen - a : a);
    }
    else if (c.q_trans && write_seq && ascii && qf != 0)
    {
        uint64_t const fc = (uint64_t)aqf - 1, L = (r.qlen - fc) / 3;
        uint64_t const a = c.hard ? b.q_start : 0, e = c.hard ? b.q_end : L;
        if (!(e > L || a > e))
        {
            r.l_seq  = 3 * (e - a);
            r.seq_at = r.base + (r.minus ? (r.qlen - (3 * e + fc)) + r.l_seq : 3 * a + fc);
        }
    }
    if (r.l_seq == 1 && !r.minus && letter(c, r.seq_at) == '*') // (a sequence that reads "*" is the absent one to bamRecord)
        r.l_seq = 0;
    // tag qs
    r.qs_len   = 0;
    r.qs_a     = 0;
    r.qs_mode  = 0;
    r.qs_shift = 0;
    if ((c.tags & tagBit(kTagProtSeq)) && !c.is_n && write_seq && ascii)
    {
        uint64_t fl = 0;
        if (!c.q_trans)
        {
            fl        = r.qlen;
            r.qs_mode = 1;
        }
        else if (qf != 0 && aqf <= 3 && c.codon)
        {
            r.qs_shift = (uint64_t)aqf - 1;
            fl         = r.qlen >= r.qs_shift ? (r.qlen - r.qs_shift) / 3 : 0;
            r.qs_mode  = r.minus ? 3 : 2;
        }
        if (fl > 0 && c.hard)
        {
            bool const ok = b.q_end <= fl && b.q_start <= b.q_end;
            r.qs_a        = ok ? b.q_start : 0;
            r.qs_len      = ok ? b.q_end - b.q_start : 0;
        }
        else
            r.qs_len = fl;
    }
    // POS (the minus-strand branch subtracts from the QUERY length, as the host writer does: a signed difference)
    r.pos = (int64_t)b.s_start;
    if (c.s_trans)
    {
        int const      sf = (int)b.s_frame;
        uint64_t const p  = b.s_start * 3 + (uint64_t)(sf < 0 ? -sf : sf) - (sf != 0 ? 1 : 0);
        r.pos             = (int64_t)(sf < 0 ? r.qlen - p : p);
    }
    // taxonomy
    r.lca      = c.grp_lca ? c.grp_lca[r.g] : 0u;
    r.name_off = 0;
    r.name_len = 0xffffffffu;
    if (c.grp_name_len)
    {
        r.name_off = c.grp_name_off[r.g];
        r.name_len = c.grp_name_len[r.g];
    }
    r.st_lo = r.st_hi = 0;
    if (c.s_tax_off && b.n_sid < c.tax_n_s)
    {
        r.st_lo = c.s_tax_off[b.n_sid];
        r.st_hi = c.s_tax_off[b.n_sid + 1];
    }
    return r;
}

// the runs of the ops (maximal runs of one code, which is what cigarOf's D / I / M loops and protCigarOf's loop both cut): run(op, count)
// for each; false if a byte is no op code
template <class F>
__device__ __forceinline__ bool walk_runs(uint8_t const * o, uint32_t n, F && run)
{
    for (uint32_t i = 0; i < n;)
    {
        uint8_t const op = o[i];
        if (!is_op(op))
            return false;
        uint32_t const i0 = i;
        while (i < n && o[i] == op)
            ++i;
        run(op, i - i0);
    }
    return true;
}
__device__ __forceinline__ bool ops_valid(uint8_t const * o, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        if (!is_op(o[i]))
            return false;
    return true;
}

struct HeadVal
{
    lx_blast_match const * rows;
    __device__ uint32_t    operator()(uint64_t k) const { return k == 0 || rows[k].n_qid != rows[k - 1].n_qid ? 1u : 0u; }
};
struct HeadOut
{
    lx_blast_match const * rows;
    uint64_t               n;
    uint32_t *             grp, *grp_first;
    __device__ void        operator()(uint64_t k, uint32_t incl, uint32_t excl) const
    {
        grp[k] = incl - 1;
        if (incl != excl)
            grp_first[incl - 1] = (uint32_t)k;
        if (k == n - 1)
            grp_first[incl] = (uint32_t)n;
    }
};
struct SizeVal
{
    uint32_t const *    size;
    __device__ uint32_t operator()(uint64_t j) const { return size[j]; }
};
struct OffOut
{
    uint32_t *      off;
    __device__ void operator()(uint64_t j, uint32_t, uint32_t excl) const { off[j] = excl; }
};

// the double expression of ppos and tag ap, divided as IEEE does (no contraction, no reciprocal)
__device__ __forceinline__ double ppos_double(int32_t num_positives, int32_t alignment_length)
{
#pragma clang fp contract(off)
    return alignment_length ? 100.0 * num_positives / alignment_length : 0.0;
}
__device__ __forceinline__ uint16_t ppos_u16(int32_t num_positives, int32_t alignment_length)
{
    return (uint16_t)(int32_t)ppos_double(num_positives, alignment_length);
}

// cigarOf's elements in its order before the reversal of the minus strand: put(op, len) with op 0 = M, 1 = I, 2 = D, 4 = S, 5 = H
template <class F>
__device__ __forceinline__ void walk_cigar(BamCtx const & c, Rec const & r, uint8_t const * o, uint32_t n_ops, F && put)
{
    if (c.hard)
    {
        if (r.lfc + r.lclip > 0)
            put(5u, r.lfc + r.lclip);
    }
    else
    {
        if (r.lfc > 0)
            put(5u, r.lfc);
        if (r.lclip > 0)
            put(4u, r.lclip);
    }
    (void)walk_runs(o, n_ops, [&](uint8_t op, uint32_t cnt) { put(op == 'M' ? 0u : op == 'I' ? 1u : 2u, (uint64_t)cnt * r.trans); });
    if (c.hard)
    {
        if (r.rfc + r.rclip > 0)
            put(5u, r.rfc + r.rclip);
    }
    else
    {
        if (r.rclip > 0)
            put(4u, r.rclip);
        if (r.rfc > 0)
            put(5u, r.rfc);
    }
}

// protCigarOf's elements (tag OC; the ops are valid): add(letter, count) for every count that is not 0
template <class F>
__device__ __forceinline__ void walk_oc(BamCtx const & c, Rec const & r, uint8_t const * o, uint32_t n_ops, F && add)
{
    uint8_t const  clip  = c.hard ? 'H' : 'S';
    uint64_t const right = r.frame_len >= r.b->q_end ? r.frame_len - r.b->q_end : 0;
    if (r.b->q_start)
        add(clip, r.b->q_start);
    (void)walk_runs(o, n_ops, [&](uint8_t op, uint32_t cnt) { add(op, (uint64_t)cnt); });
    if (right)
        add(clip, right);
}

// letter i of SEQ (i < r.l_seq), as reverseComplementAscii leaves it on the minus strand
__device__ __forceinline__ uint8_t seq_letter(BamCtx const & c, Rec const & r, uint64_t i)
{
    return r.minus ? rc_letter(letter(c, r.seq_at - 1 - i)) : letter(c, r.seq_at + i);
}

// character i of QUAL (i < r.l_seq, c.q_qual given): the quality of the read position seq_letter(c, r, i) comes from -- reversed on the
// minus strand, not complemented
__device__ __forceinline__ uint8_t qual_letter(BamCtx const & c, Rec const & r, uint64_t i)
{
    return quality(c, r.minus ? r.seq_at - 1 - i : r.seq_at + i);
}

// letter i of tag qs (i < r.qs_len): the query's own, or lx_translate_six_frames' codon of the frame's letter r.qs_a + i
__device__ __forceinline__ uint8_t qs_letter(BamCtx const & c, Rec const & r, uint64_t i)
{
    if (r.qs_mode == 1)
        return letter(c, r.base + r.qs_a + i);
    uint64_t const p = r.qs_shift + 3 * (r.qs_a + i);
    uint32_t       x0, x1, x2;
    if (r.qs_mode == 2)
    {
        x0 = nt5(letter(c, r.base + p));
        x1 = nt5(letter(c, r.base + p + 1));
        x2 = nt5(letter(c, r.base + p + 2));
    }
    else
    {
        x0 = comp5(nt5(letter(c, r.base + r.qlen - 1 - p)));
        x1 = comp5(nt5(letter(c, r.base + r.qlen - 2 - p)));
        x2 = comp5(nt5(letter(c, r.base + r.qlen - 3 - p)));
    }
    return c.codon[25 * x0 + 5 * x1 + x2];
}
