"""`lambda3`'s refusals around --query-masking while it parses its options: before any file is opened, without a GPU."""
import subprocess

import pytest

from lambda_amd import build


def _run(cwd, *a):
    return subprocess.run([str(build.build_cli()), *map(str, a)], capture_output=True, text=True, cwd=cwd, timeout=60)


@pytest.mark.parametrize("cmd,extra,text", [
    ("searchn", ["--query-masking", "seg"], "DUST, is not built"),
    ("searchbs", ["--query-masking", "seg"], "DUST, is not built"),
    ("searchp", ["--masking", "gpu"], "--masking belongs to --query-masking seg"),
    ("searchp", ["--query-masking", "none", "--masking", "host"], "--masking belongs to --query-masking seg"),
    ("searchp", ["--seg-window", "12"], "--seg-window belongs to --query-masking seg"),
    ("searchp", ["--seg-k1", "2.0"], "--seg-k1 belongs to --query-masking seg"),
    ("searchp", ["--seg-k2", "2.0", "--query-masking", "none"], "--seg-k2 belongs to --query-masking seg"),
    ("searchp", ["--query-masking", "dust"], "--query-masking takes none or seg"),
    ("searchp", ["--query-masking", "seg", "--masking", "x"], "--masking takes gpu, host or auto"),
    ("searchp", ["--query-masking", "seg", "--seg-window", "3"], "--seg-window takes 4 .. 64"),
    ("searchp", ["--query-masking", "seg", "--seg-window", "65"], "--seg-window takes 4 .. 64"),
    ("searchp", ["--query-masking", "seg", "--seg-k1", "2.6"], "0 < k1 <= k2 <= log2(window)"),
    ("searchp", ["--query-masking", "seg", "--seg-k2", "3.7"], "0 < k1 <= k2 <= log2(window)"),
    ("searchp", ["--query-masking", "seg", "--seg-k1", "0"], "0 < k1 <= k2 <= log2(window)"),
])
def test_front_end_refuses_while_parsing(tmp_path, cmd, extra, text):
    r = _run(tmp_path, cmd, "-q", "nowhere.fasta", "-i", "nowhere.lba", "-o", "x.m8", *extra)
    assert r.returncode != 0 and text in r.stderr, r.stderr
    assert "nowhere" not in r.stderr  # (no file was looked for)


def test_searchn_without_masking_is_not_refused_for_it(tmp_path):
    r = _run(tmp_path, "searchn", "-q", "nowhere.fasta", "-i", "nowhere.lba", "-o", "x.m8", "--query-masking", "none")
    assert r.returncode != 0 and "DUST" not in r.stderr and "nowhere" in r.stderr
