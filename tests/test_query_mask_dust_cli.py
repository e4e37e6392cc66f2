"""`lambda3`'s refusals around --query-masking dust while it parses its options: before any file is opened, without a GPU."""
import subprocess

import pytest

from lambda_amd import build


def _run(cwd, *a):
    return subprocess.run([str(build.build_cli()), *map(str, a)], capture_output=True, text=True, cwd=cwd, timeout=60)


@pytest.mark.parametrize("cmd,extra,text", [
    ("searchp", ["--query-masking", "dust"], "--query-masking takes none or seg (dust is the rule of searchn and searchbs)"),
    ("searchn", ["--query-masking", "seg"], "unlike DUST, is not built: use --query-masking dust"),
    ("searchbs", ["--query-masking", "seg"], "unlike DUST, is not built: use --query-masking dust"),
    ("searchn", ["--query-masking", "sdust"], "--query-masking takes none or dust"),
    ("searchn", ["--dust-window", "64"], "--dust-window belongs to --query-masking dust"),
    ("searchbs", ["--dust-level", "20", "--query-masking", "none"], "--dust-level belongs to --query-masking dust"),
    ("searchp", ["--query-masking", "seg", "--dust-level", "20"], "--dust-level belongs to --query-masking dust"),
    ("searchn", ["--masking", "gpu"], "--masking belongs to --query-masking dust"),
    ("searchbs", ["--query-masking", "none", "--masking", "host"], "--masking belongs to --query-masking dust"),
    ("searchn", ["--query-masking", "dust", "--seg-window", "12"], "--seg-window belongs to --query-masking seg"),
    ("searchbs", ["--query-masking", "dust", "--seg-k1", "2.0"], "--seg-k1 belongs to --query-masking seg"),
    ("searchn", ["--seg-k2", "2.0"], "--seg-k2 belongs to --query-masking seg"),
    ("searchn", ["--query-masking", "dust", "--masking", "x"], "--masking takes gpu, host or auto"),
    ("searchn", ["--query-masking", "dust", "--dust-window", "3"], "--dust-window takes 4 .. 64"),
    ("searchn", ["--query-masking", "dust", "--dust-window", "65"], "--dust-window takes 4 .. 64"),
    ("searchbs", ["--query-masking", "dust", "--dust-level", "0"], "--dust-level takes 1 .. 1000"),
    ("searchn", ["--query-masking", "dust", "--dust-level", "1001"], "--dust-level takes 1 .. 1000"),
])
def test_front_end_refuses_while_parsing(tmp_path, cmd, extra, text):
    r = _run(tmp_path, cmd, "-q", "nowhere.fasta", "-i", "nowhere.lba", "-o", "x.m8", *extra)
    assert r.returncode != 0 and text in r.stderr, r.stderr
    assert "nowhere" not in r.stderr  # (no file was looked for)


@pytest.mark.parametrize("cmd", ["searchn", "searchbs"])
def test_dust_with_its_options_is_not_refused(tmp_path, cmd):
    r = _run(tmp_path, cmd, "-q", "nowhere.fasta", "-i", "nowhere.lba", "-o", "x.m8", "--query-masking", "dust", "--masking", "host", "--dust-window", "4",
             "--dust-level", "1000")
    assert r.returncode != 0 and "DUST" not in r.stderr and "dust" not in r.stderr and "nowhere" in r.stderr


def test_the_usage_text_names_the_rule(tmp_path):
    r = _run(tmp_path)
    assert "--query-masking none|dust" in r.stderr and "--dust-window W" in r.stderr and "--dust-level L" in r.stderr
