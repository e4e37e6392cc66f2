"""CPU tests of the device BAM writer's boundary: lx_render_bam_dev, lx_write_bam_dev and LX_OPT_BAM_RANGE_BYTES are declared, exported
and bound; both entries refuse a NULL handle before anything else; the front end parses --render.  No GPU needed."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from lambda_amd import build, capi

ROOT = Path(__file__).resolve().parent.parent
NEW = ["lx_render_bam_dev", "lx_write_bam_dev"]


def test_symbols_and_option_are_declared_exported_and_bound():
    lib = capi.load()
    header = (ROOT / "include" / "lambda_ext.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", code), name
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    assert re.search(r"\bLX_OPT_BAM_RANGE_BYTES\s*=\s*17\b", code)
    assert capi.LX_OPT_BAM_RANGE_BYTES == 17
    assert lib.lx_abi_version() == 3
    assert hasattr(capi.Handle, "render_bam") and hasattr(capi.Handle, "write_bam")
    # the kernels and their host side are part of the product's sources
    assert {"lx_bam.hip", "lx_bam_host.cpp"} <= set(build.HIP_SOURCES)


def test_null_handle_is_refused_first(tmp_path):
    lib = capi.load()
    out = C.c_void_p(1)
    assert lib.lx_render_bam_dev(None, 1, b"blastp", None, 0, None, 0, None, None, None, None, C.byref(out)) == capi.LX_EINVAL
    p = tmp_path / "x.bam"
    assert lib.lx_write_bam_dev(None, str(p).encode(), b"blastp", None, 0, None, 0, None, None, None, None) == capi.LX_EINVAL
    assert not p.exists()


def _parse(tmp_path, *extra):
    cli = build.build_cli()
    # (the query and database do not exist: options are refused before they are opened)
    return subprocess.run([str(cli), "searchp", "-q", str(tmp_path / "none.fa"), "-d", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.bam"), *extra],
                          capture_output=True, text=True)


def test_cli_refuses_an_unknown_render_mode_at_parse_time(tmp_path):
    r = _parse(tmp_path, "--render", "sideways")
    assert r.returncode != 0
    assert "--render takes gpu, host or auto" in r.stderr, r.stderr


@pytest.mark.parametrize("mode", ["host", "gpu", "auto"])
def test_cli_accepts_render_modes_at_parse_time(tmp_path, mode):
    r = _parse(tmp_path, "--render", mode)
    assert r.returncode != 0 and "--render" not in r.stderr and "chosen by the extension" not in r.stderr, r.stderr
