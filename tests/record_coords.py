"""Records at the coordinates a real database produces, and an independent model of what the record writers print for them.

The writer tests draw their rows from tests.test_bam_encoding._case, whose subjects are a few thousand letters long.  The lists here keep
_case's names, queries, ops and options and move the rows: across the boundaries of all six levels of BAM's binning scheme, across the
sign change of a translated subject's POS, across every power of ten a decimal field can reach, and onto an actual six-frame
translation.  The writers are handed only the subjects' LENGTHS, so a subject of 2^31 - 1 letters costs nothing.

The model is written from the reference's myWriteRecord (src/search_output.hpp:463-733) and blastMatchOneCigar (:115-194), from BLAST's
tabular conventions and from the SAM/BAM specification (sections 1.4, 4.2, 5.3), in plain Python integers; not from the project's
host writer, which is one of the things it is compared with.  No GPU, no handle."""
import functools
import itertools
from typing import NamedTuple

import numpy as np

from lambda_amd import capi
from tests import bam_decode
from tests.test_bam_encoding import _case

M8_COLUMNS = "qstart qend sstart send qlen slen"
BAM_MAX_REF = 2 ** 31 - 1  # l_ref and pos are int32_t (specification 4.2)
FRAMES = (1, 2, 3, -1, -2, -3)
SHIFTS = (14, 17, 20, 23, 26)  # reg2bin's levels 5 (16 kb bins) .. 1 (64 Mb bins); level 0 is bin 0


class Cases(NamedTuple):
    name: str
    program: str
    m: np.ndarray
    ops: bytes
    names: dict
    qa: bytes | None
    qoff: np.ndarray | None
    sam_seq: int
    bam: bool  # whether the list may be written as BAM (its subjects and positions fit 32 bits, its clips 28)
    labels: list

    def args(self):
        return self.m, self.ops, self.names["q_ids"], self.names["q_lens"], self.names["s_ids"], self.names["s_lens"]

    def kw(self, options=None):
        return dict(program=self.program, q_ascii=self.qa, q_ascii_off=self.qoff, options=options)


def options(cases: Cases, hard: int = 1, tags: str = "AS OC NM IH ar ae ai ap qf qs sf st ls lt"):
    return capi.output_options(sam_tags=tags, sam_seq=cases.sam_seq, sam_hard_clip=hard, sam_with_ref_header=1, columns=M8_COLUMNS)


# ---- the model

def q_translated(program):
    return program in ("blastx", "tblastx")


def s_translated(program):
    return program in ("tblastn", "tblastx")


def frame_length(program, qlen, q_frame):
    """length(source(alignRow0)): the query itself, or the frame of a translated one"""
    return (qlen - (abs(q_frame) - 1)) // 3 if q_translated(program) else qlen


def cigar_elements(program, row, ops, qlen, hard):
    """blastMatchOneCigar: [(letter, length)] as written (reversed on a minus query frame), None where myWriteRecord makes none (:529-531)"""
    if program in ("blastp", "tblastn"):
        return None
    fac = 3 if q_translated(program) else 1
    qf = int(row["q_frame"])
    left_frame = abs(qf) - 1
    right_frame = (qlen - left_frame) % 3 if fac == 3 else 0
    left = int(row["q_start"]) * fac
    right = (frame_length(program, qlen, qf) - int(row["q_end"])) * fac
    assert left >= 0 and right >= 0  # (the reference computes these in `unsigned`: a case list must not make them wrap)
    el = []
    if hard:
        if left_frame + left > 0:
            el.append(("H", left_frame + left))
    else:
        if left_frame > 0:
            el.append(("H", left_frame))
        if left > 0:
            el.append(("S", left))
    o = ops[int(row["ops_off"]): int(row["ops_off"]) + int(row["n_ops"])]
    for op, run in itertools.groupby(o):  # maximal runs, which is what the D / I / M loops of :146-177 cut
        el.append((chr(op), sum(1 for _ in run) * fac))
    if hard:
        if right_frame + right > 0:
            el.append(("H", right_frame + right))
    else:
        if right > 0:
            el.append(("S", right))
        if right_frame > 0:
            el.append(("H", right_frame))
    return el[::-1] if qf < 0 else el


def reference_span(elements):
    """what the CIGAR covers on the reference: its M and D elements (there is no N, = or X here); 1 for an absent or clips-only CIGAR
    (specification 4.2: `bin` is computed as if the alignment covered one base)"""
    return sum(n for op, n in elements or () if op in "MD") or 1


def sam_pos(program, row, qlen):
    """bamR.beginPos of :493-503 as a signed integer, 0-based.  The minus-frame branch subtracts from the QUERY length, as it stands"""
    if not s_translated(program):
        return int(row["s_start"])
    p = int(row["s_start"]) * 3 + abs(int(row["s_frame"])) - 1
    return qlen - p if int(row["s_frame"]) < 0 else p


def low32_signed(v):
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def bin_level(beg, end):
    """0 (bin 0) .. 5 (the 16 kb bins): the level reg2bin files [beg, end) at"""
    for i, shift in enumerate(SHIFTS):
        if beg >> shift == (end - 1) >> shift:
            return 5 - i
    return 0


def untranslated_interval(a, e, frame, length):
    """protein [a, e) of a frame in 1-based inclusive nucleotide positions of the sequence it was translated from: [3a + |f| - 1,
    3e + |f| - 1) of the strand that was read, a minus frame counted from the sequence's end, first > last"""
    lo, hi = 3 * a + abs(frame) - 1, 3 * e + abs(frame) - 1
    return (lo + 1, hi) if frame > 0 else (length - lo, length - hi + 1)


def tabular_coordinates(program, row, qlen, slen):
    """qstart, qend, sstart, send as BLAST reports them: 1-based inclusive; BLASTN's minus strand on the forward query with the subject
    descending"""
    qs, qe, ss, se = int(row["q_start"]) + 1, int(row["q_end"]), int(row["s_start"]) + 1, int(row["s_end"])
    if q_translated(program):
        qs, qe = untranslated_interval(int(row["q_start"]), int(row["q_end"]), int(row["q_frame"]), qlen)
    elif int(row["q_frame"]) < 0:
        qs, qe = qlen - int(row["q_end"]) + 1, qlen - int(row["q_start"])
        ss, se = se, ss
    if s_translated(program):
        ss, se = untranslated_interval(int(row["s_start"]), int(row["s_end"]), int(row["s_frame"]), slen)
    return qs, qe, ss, se


def model_row(cases: Cases, k: int, hard: int = 1) -> dict:
    row = cases.m[k]
    qlen, slen = int(cases.names["q_lens"][int(row["n_qid"])]), int(cases.names["s_lens"][int(row["n_sid"])])
    el = cigar_elements(cases.program, row, cases.ops, qlen, hard)
    pos = sam_pos(cases.program, row, qlen)
    span = reference_span(el)
    qs, qe, ss, se = tabular_coordinates(cases.program, row, qlen, slen)
    return dict(pos=pos, pos_text=str(pos + 1), cigar_text="".join(f"{n}{op}" for op, n in el or ()) or "*", n_cigar=len(el or ()),
                span=span, bam_pos=low32_signed(pos), bam_bin=bam_decode.reg2bin(pos, pos + span) & 0xFFFF, level=bin_level(pos, pos + span),
                m8=[str(x) for x in (qs, qe, ss, se, qlen, slen)], sstart=ss, send=se)


def model(cases: Cases, hard: int = 1) -> list:
    return [model_row(cases, k, hard) for k in range(len(cases.m))]


# ---- the case lists

LONG_OPS = ((b"M" * 37 + b"D" * 2 + b"M" * 11 + b"I" * 3) * 400)[:20_000]


class _Builder:
    """Rows of one _case, copied and moved; queries and ops added behind _case's own"""

    def __init__(self, program, seed):
        self.program = program
        self.base, self.ops, names, self.qa, qoff = _case(program, seed=seed)
        self.q_ids, self.q_lens, self.qoff = list(names["q_ids"]), [int(x) for x in names["q_lens"]], [int(x) for x in qoff]
        self.s_ids, self.s_lens = list(names["s_ids"]), [int(x) for x in names["s_lens"]]
        self.rng = np.random.default_rng(seed)
        self.rows, self.labels = [], []

    def add_query(self, length):
        alph = "ACGT" if self.program in ("blastn", "blastx", "tblastx") else "ARNDCQEGHILKMFPSTWYV"
        self.q_ids.append(f"q{len(self.q_ids)} added")
        self.q_lens.append(length)
        self.qoff.append(len(self.qa))
        self.qa += "".join(alph[i] for i in self.rng.integers(0, len(alph), length)).encode()
        return len(self.q_ids) - 1

    def template(self, i):
        return self.base[i % len(self.base)].copy()

    def align(self, r, o: bytes, q_start: int):
        """the row's ops and the query interval they consume"""
        r["ops_off"], r["n_ops"], r["alignment_length"] = len(self.ops), len(o), len(o)
        r["num_matches"] = r["num_positives"] = max(len(o) - 1, 0)
        r["q_start"], r["q_end"] = q_start, q_start + o.count(b"M") + o.count(b"I")
        self.ops += o

    def row_ops(self, r):
        return self.ops[int(r["ops_off"]): int(r["ops_off"]) + int(r["n_ops"])]

    def subject_columns(self, r):
        o = self.row_ops(r)
        return (o.count(b"M") + o.count(b"D")) or 1

    def place(self, r, pos):
        """the subject interval whose POS is `pos` (a translated subject: on the plus frame that has it)"""
        if s_translated(self.program):
            r["s_frame"], r["s_start"] = pos % 3 + 1, pos // 3
        else:
            r["s_start"] = pos
        r["s_end"] = int(r["s_start"]) + self.subject_columns(r)

    def add(self, r, label):
        self.rows.append(r)
        self.labels.append(label)

    def cases(self, name, sam_seq, bam, ascii=True):
        m = np.array(self.rows, dtype=capi.BLAST_MATCH_DTYPE)
        order = np.argsort(m["n_qid"], kind="stable")  # (the writers take a list grouped by query)
        m = m[order]
        m["qry_id"] = m["n_qid"]
        names = dict(q_ids=self.q_ids, q_lens=np.array(self.q_lens, np.int64), s_ids=self.s_ids, s_lens=np.array(self.s_lens, np.uint64))
        return Cases(name, self.program, m, self.ops, names, self.qa if ascii else None, np.array(self.qoff, np.uint64) if ascii else None,
                     sam_seq, bam, [self.labels[i] for i in order])


BIN_PROGRAMS = ("blastn", "blastx", "tblastn", "tblastx")


def bin_levels(program) -> Cases:
    """Rows on both sides of, and across, a boundary of every level of the binning scheme, at three spans: 1 (no CIGAR), a few columns,
    and an alignment of 20 000 ops.  TBLASTN writes no CIGAR, so there every span is 1 and only the finest level can occur."""
    b = _Builder(program, seed=100 + BIN_PROGRAMS.index(program))
    for s in range(len(b.s_lens)):
        b.s_lens[s] = BAM_MAX_REF
    long_q = b.add_query(3 * 20_100 + 2 if q_translated(program) else 20_500)
    count = itertools.count()

    def make(kind):
        i = next(count)
        r = b.template(i)
        if program == "blastn":
            r["q_frame"] = 1 if i % 2 == 0 else -1  # both query strands
        qlen = b.q_lens[int(r["n_qid"])]
        if kind == "one":  # no ops and no clips but the frame's: nothing that covers the reference
            b.align(r, b"", 0)
            r["q_end"] = frame_length(program, qlen, int(r["q_frame"]))
        elif kind == "long":
            r["n_qid"] = long_q
            b.align(r, LONG_OPS, 5)
        span = reference_span(cigar_elements(program, r, b.ops, b.q_lens[int(r["n_qid"])], 1))
        return r, span

    def add(kind, where, label, least=1):
        r, span = make(kind)
        if span < least:
            return
        b.place(r, where(span))
        b.add(r, f"{kind}: {label}")

    for shift, k in zip(SHIFTS, (5, 5, 7, 9, 3)):  # (5 << 14: above the longest span, 3 * 18 868)
        B = k << shift
        for kind in ("one", "few", "long"):
            add(kind, lambda span: B - span, f"ends at {k} << {shift}, less one")
            add(kind, lambda span: B - 1, f"begins one before {k} << {shift} and crosses it", least=2)
            add(kind, lambda span: B, f"begins at {k} << {shift}")
    for kind in ("one", "few", "long"):
        add(kind, lambda span: 2 ** 29 - span, "ends where the binning scheme ends")
        add(kind, lambda span: 2 ** 29, "begins at 2^29: the 16-bit field holds the formula's value modulo 65536")
        add(kind, lambda span: BAM_MAX_REF - span, "ends at the last position a BAM reference has")
    for kind in ("few", "long"):
        add(kind, lambda span: (5 << 26) - span // 2, "across an odd multiple of 2^26: bin 0", least=2)
    add("few", lambda span: 2 ** 30 + 12_345, "begins beyond 2^30")
    return b.cases(f"bin_levels-{program}", capi.LX_SAM_SEQ_UNIQ, True)


def sign_change(qlen, frame):
    """the first s_start at which 3 * s_start + |f| - 1 exceeds the query length"""
    return next(s for s in itertools.count() if 3 * s + abs(frame) - 1 > qlen)


def translated_subject_pos(program) -> Cases:
    """Six subject frames at s_start 0, 1, around the sign change of the minus frames' POS, at 10^6 and at the last codon a BAM
    reference has room for"""
    assert s_translated(program)
    b = _Builder(program, seed=120 + BIN_PROGRAMS.index(program))
    for s in range(len(b.s_lens)):
        b.s_lens[s] = BAM_MAX_REF
    i = 0
    for f in FRAMES:
        r0 = b.template(i)
        t = sign_change(b.q_lens[int(r0["n_qid"])], f)
        for s_start, what in ((0, "0"), (1, "1"), (t - 1, "t - 1"), (t, "t"), (t + 1, "t + 1"), (10 ** 6, "10^6"), ((2 ** 31 - 4) // 3, "(2^31 - 4) / 3")):
            r = b.template(i)  # (one query per frame: t is that query's)
            if s_start > 10 ** 6:  # one codon: there is no room for more
                b.align(r, b"M", int(r["q_start"]))
            r["s_frame"], r["s_start"] = f, s_start
            r["s_end"] = s_start + b.subject_columns(r)
            b.add(r, f"frame {f}, s_start {what}")
        i += 1
    return b.cases(f"translated_subject_pos-{program}", capi.LX_SAM_SEQ_UNIQ, True)


def digit_edges(bam: bool) -> Cases:
    """BLASTN's plus strand: s_start + 1 = 10^k - 1 and 10^k, and, with --sam-bam-seq never, queries whose clips are 10^k - 1 and 10^k
    letters long on either side of the alignment"""
    b = _Builder("blastn", seed=140)
    top = 9 if bam else 12
    for s in range(len(b.s_lens)):
        b.s_lens[s] = BAM_MAX_REF if bam else 10 ** 13
    clips = [v for k in range(1, 9) for v in (10 ** k - 1, 10 ** k)]
    o = b.row_ops(b.base[0])
    b.q_ids, b.q_lens, b.qoff = [], [], []  # a query of its own per row; no letters: SEQ is never written
    i = 0
    for k in range(1, top + 1):
        for v in (10 ** k - 1, 10 ** k):
            r = b.template(0)
            left, right = clips[i % len(clips)], clips[(i + 5) % len(clips)]
            b.align(r, o, left)
            r["n_qid"], r["n_sid"], r["q_frame"] = i, i % len(b.s_ids), 1
            b.q_ids.append(f"d{i} edge")
            b.q_lens.append(int(r["q_end"]) + right)
            r["s_start"] = v - 1
            r["s_end"] = v - 1 + b.subject_columns(r)
            b.add(r, f"s_start + 1 = {v}, clips {left} and {right}")
            i += 1
    return b.cases("digit_edges-" + ("bam" if bam else "text"), capi.LX_SAM_SEQ_NEVER, bam, ascii=False)


SUBJECT_LETTERS = 3 * 2 ** 14 + 50
_COMPLEMENT5 = np.array([4, 2, 1, 3, 0], np.uint8)  # dna5 ranks A C G N T


def untranslate_property(program="tblastn"):
    """Rows on the first codon, the last codon and a few random intervals of each frame of an actual random subject; returns the list,
    the subject (dna5 ranks) and its six frames"""
    assert s_translated(program)
    b = _Builder(program, seed=160 + BIN_PROGRAMS.index(program))
    dna = b.rng.choice(np.array([0, 1, 2, 3, 4], np.uint8), SUBJECT_LETTERS, p=[0.24, 0.24, 0.24, 0.04, 0.24])
    frames = capi.translate_six_frames(dna)
    for s in range(len(b.s_lens)):
        b.s_lens[s] = SUBJECT_LETTERS
    i = 0
    for f, frame in zip(FRAMES, frames):
        n = len(frame)
        assert n == (SUBJECT_LETTERS - (abs(f) - 1)) // 3
        cuts = [(0, 1), (n - 1, n)] + [tuple(sorted(int(x) for x in b.rng.choice(n + 1, 2, replace=False))) for _ in range(3)]
        for a, e in cuts:
            r = b.template(i)
            r["s_frame"], r["s_start"], r["s_end"] = f, a, e
            b.add(r, f"frame {f}, [{a}, {e})")
            i += 1
    return b.cases(f"untranslate_property-{program}", capi.LX_SAM_SEQ_UNIQ, True), dna, frames


def translation_of_interval(dna, sstart, send):
    """the translation of the nucleotides sstart .. send (1-based, inclusive; sstart > send: of their reverse complement)"""
    seg = dna[sstart - 1: send] if sstart <= send else _COMPLEMENT5[dna[send - 1: sstart][::-1]]
    return capi.translate_six_frames(seg)[0]


LIST_NAMES = ([f"bin_levels-{p}" for p in BIN_PROGRAMS] + [f"translated_subject_pos-{p}" for p in ("tblastn", "tblastx")] +
              ["digit_edges-text", "digit_edges-bam"] + [f"untranslate_property-{p}" for p in ("tblastn", "tblastx")])
BAM_LIST_NAMES = [n for n in LIST_NAMES if n != "digit_edges-text"]


@functools.lru_cache(maxsize=None)
def lists() -> dict:
    """every list by its name, made once (the callers leave them as they are)"""
    made = ([bin_levels(p) for p in BIN_PROGRAMS] + [translated_subject_pos(p) for p in ("tblastn", "tblastx")] +
            [digit_edges(False), digit_edges(True), untranslate_property("tblastn")[0], untranslate_property("tblastx")[0]])
    assert [c.name for c in made] == LIST_NAMES and [c.name for c in made if c.bam] == BAM_LIST_NAMES
    assert all(len(c.m) <= 100 for c in made)
    return {c.name: c for c in made}


@functools.lru_cache(maxsize=None)
def models(name: str, hard: int = 1) -> list:
    return model(lists()[name], hard)


# ---- a writer's bytes against the model (the assertions the host and the device tests share)

def _rows_differ(name, what, got, want):
    labels = lists()[name].labels
    bad = [(k, labels[k], g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad and len(got) == len(want), f"{name}: {what} of {len(bad)} of {len(want)} rows differ from the model, (row, case, got, model): {bad[:6]}"


def assert_m8_equals_model(text: bytes, name: str):
    """.m8 with the columns qstart qend sstart send qlen slen"""
    _rows_differ(name, "qstart qend sstart send qlen slen", [line.split("\t") for line in text.decode().splitlines()], [r["m8"] for r in models(name)])


def assert_sam_equals_model(text: bytes, name: str, hard: int):
    """POS and CIGAR of the SAM lines"""
    fields = [line.split("\t") for line in text.decode().splitlines() if not line.startswith("@")]
    _rows_differ(name, "POS", [f[3] for f in fields], [r["pos_text"] for r in models(name, hard)])
    _rows_differ(name, "CIGAR", [f[5] for f in fields], [r["cigar_text"] for r in models(name, hard)])


def assert_bam_equals_model(bam: bytes, name: str, hard: int):
    """pos, bin and n_cigar_op of the BAM records, and the reference lengths"""
    cases = lists()[name]
    _, refs, recs = bam_decode.decode(bam)
    assert [length for _, length in refs] == [int(x) for x in cases.names["s_lens"]]
    want = models(name, hard)
    _rows_differ(name, "pos", [r["pos"] for r in recs], [w["bam_pos"] for w in want])
    _rows_differ(name, "bin", [r["bin"] for r in recs], [w["bam_bin"] for w in want])
    _rows_differ(name, "n_cigar_op", [len(r["cigar"]) for r in recs], [w["n_cigar"] for w in want])
