"""--max-hsps / --culling-limit on the device: the two counting kernels of lx_toprec.hip (lx_postprocess_records_dev_ex,
lx_iterate_matches_dev_top_ex) against the host form lx_postprocess_records_ex -- which tests/test_cull_records.py holds against an
independent model --, and `lambda3 --records gpu` against `--records host` with both options given."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lambda_amd import capi
from tests import cull_ranges_case
from tests import cull_reference as cref
from tests import toprec_reference as ref
from tests.test_cli import CODONS, STD, _cli, _fasta
from tests.test_gpu_toprec_cli import _inputs, _mutate

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# segment lengths on the kernels' edges (a workgroup's 256 rows, the staged tile of 512, several tiles); in this order the segments
# begin at rows 0, 1, 3, 258, 514, 771, 1282, 1794, 2307, 3332: most of them straddle a workgroup's first row
SEGMENTS = [1, 2, 255, 256, 257, 511, 512, 513, 1025, 3000]
VARIANTS = ("nested", "one_subject", "equal_intervals", "equal_scores")


@pytest.fixture(scope="module")
def lists():
    """The crafted lists, made once: {variant: (rows, q_lens, translated)}."""
    out = {}
    for k, variant in enumerate(VARIANTS):
        rng = np.random.default_rng(50 + k)
        m, q_lens, translated = cref.nested_rows(rng, SEGMENTS, "translated" if variant == "nested" else "revcomp", n_sid=6, q_len_range=(3001, 9000))
        if variant == "one_subject":
            m["n_sid"] = 7
        elif variant == "equal_intervals":  # one interval per query, on both strands: [10, 110) read forwards, its mirror read backwards
            ql = q_lens[m["n_qid"].astype(np.int64)]
            minus = m["q_frame"] < 0
            m["q_start"], m["q_end"] = np.where(minus, ql - 110, 10), np.where(minus, ql - 10, 110)
            m["s_start"] = np.arange(len(m))  # (no duplicates of the seven-field key: the rule has every row in front of it)
        elif variant == "equal_scores":
            m["bit_score"] = 33.25
        out[variant] = (m, q_lens, translated)
    return out


@pytest.mark.parametrize("variant", VARIANTS)
def test_device_step_equals_the_host_step(handle, lists, variant):
    m, q_lens, translated = lists[variant]
    starts = np.concatenate([[0], np.cumsum(SEGMENTS)[:-1]])
    assert ((starts % 256 != 0).sum() >= 8) and len(m) == sum(SEGMENTS)
    dropped = [0, 0]
    for K in (0, 1, 3):
        for L in (0, 1, 3):
            for mm in (25, 2 ** 40):
                want, wst, wcst = capi.postprocess_records_ex(m, mm, K, L, q_lens, translated)
                got, gst, gcst = capi.postprocess_records_dev_ex(handle, m, mm, K, L, q_lens, translated)
                assert cref.stats_dict(gst, gcst) == cref.stats_dict(wst, wcst), (K, L, mm)
                assert len(got) == len(want) and got.tobytes() == want.tobytes(), (K, L, mm)  # (rows, order, ops_off: all 128 bytes)
                dropped[0] += wcst.hits_max_hsps
                dropped[1] += wcst.hits_culled
    assert dropped[0] > 1000 and dropped[1] > 1000
    if variant == "equal_intervals":  # at L = 1 one row per query stays
        got, _, gcst = capi.postprocess_records_dev_ex(handle, m, 2 ** 40, 0, 1, q_lens, translated)
        assert len(got) == len(SEGMENTS) and gcst.hits_culled + len(got) + capi.postprocess_records(m, 2 ** 40)[1].hits_duplicate2 == len(m)


def test_options_off_are_the_plain_device_step(handle, lists):
    m, q_lens, translated = lists["nested"]
    plain, pst = capi.postprocess_records_dev(handle, m, 25)
    got, gst, gcst = capi.postprocess_records_dev_ex(handle, m, 25, 0, 0, q_lens, translated)
    assert got.tobytes() == plain.tobytes() and ref.stats_dict(gst) == ref.stats_dict(pst) and (gcst.hits_max_hsps, gcst.hits_culled) == (0, 0)
    got, gst, gcst = capi.postprocess_records_dev_ex(handle, m[:0], 25, 1, 1, q_lens, translated)
    assert len(got) == 0 and ref.stats_dict(gst) == dict.fromkeys(ref.STAT_FIELDS, 0)


def test_refusals_come_before_any_device_work(handle, lists):
    m, q_lens, translated = lists["nested"]
    with pytest.raises(capi.LambdaExtError, match="names query"):
        capi.postprocess_records_dev_ex(handle, m, 25, 0, 1, q_lens[:3], translated)
    short = q_lens.copy()
    short[int(m["n_qid"][-1])] = 2
    with pytest.raises(capi.LambdaExtError, match="does not fit its query's length of 2"):
        capi.postprocess_records_dev_ex(handle, m, 25, 0, 1, short, translated)
    long_ = q_lens.copy()
    long_[0] = 2 ** 32
    with pytest.raises(capi.LambdaExtError, match="the device step takes 4294967295 at most"):
        capi.postprocess_records_dev_ex(handle, m, 25, 0, 1, long_, translated)
    with pytest.raises(capi.LambdaExtError, match="needs q_lens"):
        capi.postprocess_records_dev_ex(handle, m, 25, 0, 1, None, translated)
    capi.postprocess_records_dev_ex(handle, m, 25, 1, 0, None, translated)  # (culling_limit == 0: the lengths are not looked at)


def test_iterate_top_with_the_options_on_the_long_query_list(handle):
    """700 records of one query on eight subjects, all over the whole query: --max-hsps 1 leaves eight of them, --culling-limit 1 one."""
    dropped = cull_ranges_case.compare(handle, "long_query")
    assert dropped[(1, 0)][0] >= 600 and dropped[(0, 1)][1] >= 600 and dropped[(1, 1)][0] >= 600


def test_iterate_top_with_the_options_range_by_range():
    """The same under LX_L2_RANGES = 3 (read once per process: a process of its own): the read list is served in three ranges, each
    with the two kernels behind its records kernels."""
    env = dict(os.environ, LX_L2_RANGES="3", LX_HOST_TIMING="1")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "cull_ranges_case.py"), "reads", "long_query"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ok reads" in r.stdout and "ok long_query" in r.stdout
    reads = r.stderr[: r.stderr.index("list reads done")]
    assert {int(x) for x in re.findall(r"extension \+ records \(range by range\), (\d+) ranges", reads)} == {3}


# ---- the front end --------------------------------------------------------------------------------------------------------------------

def _blastx_inputs(tmp):
    """Protein families, and nucleotide contigs that carry two genes each -- a strong one and, elsewhere on the contig, a diverged one,
    on either strand: the case the options are for."""
    rng = np.random.default_rng(77)
    base = ["".join(STD[i] for i in rng.integers(0, 20, 150)) for _ in range(8)]
    subj = [_mutate(rng, b, STD, 0.10) for b in base for _ in range(12)]
    encode = lambda p: "".join(CODONS[c][int(rng.integers(0, len(CODONS[c])))] for c in p)
    noise = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    comp = str.maketrans("ACGT", "TGCA")
    qry = []
    for k in range(16):
        strong, weak = base[k % 8][10:120], _mutate(rng, base[(k + 3) % 8], STD, 0.25)[20:100]
        contig = noise(int(rng.integers(1, 30))) + "TAA" + encode(strong) + "TAA" + noise(int(rng.integers(20, 60))) + "TAA" + encode(weak) + "TAA" + noise(int(rng.integers(1, 9)))
        qry.append(contig.translate(comp)[::-1] if k % 2 else contig)
    _fasta(tmp / "d.fasta", [f"s{i}" for i in range(len(subj))], subj)
    _fasta(tmp / "q.fasta", [f"q{i}" for i in range(len(qry))], qry)


def _culling(stderr):
    m = re.search(r"lambda3 culling: --max-hsps 1 dropped (\d+) record\(s\), --culling-limit 1 dropped (\d+) record\(s\), on the (GPU|host)", stderr)
    assert m, stderr
    return int(m.group(1)), int(m.group(2)), m.group(3)


def _runner(tmp_path, case):
    program = "searchp" if case == "blastx" else case
    _blastx_inputs(tmp_path) if case == "blastx" else _inputs(tmp_path, program)

    def run(out, *more):
        r = subprocess.run([str(_cli()), program, "-q", str(tmp_path / "q.fasta"), "-d", str(tmp_path / "d.fasta"), "-o", str(tmp_path / out), "-n", "5",
                            "--max-hsps", "1", "--culling-limit", "1", "--version-to-outputfile", "0", *more], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert (case == "blastx") == ("blastx" in r.stderr)
        hsps = re.search(r"HSPs (\d+) -> written (\d+)", r.stderr).groups()
        return (tmp_path / out).read_bytes(), _culling(r.stderr), hsps

    return run


CASES = ["searchp", "blastx", "searchn"]


@pytest.mark.parametrize("case", CASES)
def test_records_on_the_gpu_write_the_same_files_with_the_options(tmp_path, case):
    run = _runner(tmp_path, case)
    host, gpu = run("host.m8", "--records", "host"), run("gpu.m8", "--records", "gpu")
    assert host[1][2] == "host" and gpu[1][2] == "GPU"
    assert gpu[0] == host[0] and len(host[0]) > 0
    assert gpu[1][:2] == host[1][:2] and gpu[2] == host[2]  # (the counters; HSPs counts the records that either rule dropped, too)
    assert host[1][1] > 0  # the culling limit had something to drop
    lines = [l.split("\t") for l in host[0].decode().splitlines()]
    assert len({(x[0], x[1]) for x in lines}) == len(lines)  # --max-hsps 1
    assert run("host.bam", "--records", "host")[0] == run("gpu.bam", "--records", "gpu")[0]


@pytest.mark.parametrize("case", CASES)
def test_blocks_of_the_query_file_write_the_eager_run_s_file_with_the_options(tmp_path, case):
    """--query-block 7: every record of a read is in its block, so the rules see all of them -- in the block's host step and in the
    Level-2 calls of a block, whose n_qid and lengths are the block's own."""
    run = _runner(tmp_path, case)
    eager = run("eager.m8", "--records", "host")
    for where in ("host", "gpu"):
        blocks = run(f"blocks_{where}.m8", "--records", where, "--query-block", "7")
        assert blocks[0] == eager[0] and blocks[1][:2] == eager[1][:2] and blocks[2] == eager[2], where
