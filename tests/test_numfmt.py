"""CPU tests of the exact number formatter (lambda_amd/csrc/lx_numfmt.h) through lx_format_number: the characters printf writes for
"%.1e", "%.1f", "%.2f" and "%g" of a float, made with integer arithmetic alone.  The reference is Python's % formatting, which rounds
the exact binary value to nearest with ties to even as glibc's printf does.  The device text writers print with the same functions
(tests/test_gpu_text_render.py pins their bytes to the host writer's snprintf)."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from lambda_amd import capi

E1, F1, F2, G = capi.LX_NUM_E1, capi.LX_NUM_F1, capi.LX_NUM_F2, capi.LX_NUM_G_FLOAT
FMT = {E1: "%.1e", F1: "%.1f", F2: "%.2f", G: "%g"}
N_RANDOM = 200_000


def f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _many(kind, values):
    """The texts of all values in one go (a ctypes call per value through capi.format_number costs too much for 200 000)."""
    lib = capi.load()
    buf = C.create_string_buffer(32)
    fn, out = lib.lx_format_number, []
    for v in values:
        n = fn(kind, v, buf, 32)
        assert n > 0, (kind, v, n)
        out.append(buf.raw[:n])
    return out


def _check(kind, values):
    fmt = FMT[kind]
    got = _many(kind, values)
    bad = [(v.hex() if math.isfinite(v) else v, g, (fmt % v)) for v, g in zip(values, got) if g != (fmt % v).encode()]
    assert not bad, bad[:10]


TABLE = [
    (F2, 0.125, "0.12"), (F2, 0.375, "0.38"), (F1, 0.25, "0.2"), (F1, 0.75, "0.8"), (E1, 1.25, "1.2e+00"), (E1, 1.75, "1.8e+00"),
    (E1, 9.95e-5, "1.0e-04"), (E1, 9.96e-10, "1.0e-09"), (E1, 5e-324, "4.9e-324"), (E1, 1.7976931348623157e308, "1.8e+308"),
    (F2, 99.995, "100.00"), (F1, -0.04, "-0.0"), (G, f32(1e-5), "1e-05"), (G, f32(1e-4), "0.0001"), (G, 999999.5, "1e+06"),
    (G, 123456.703125, "123457"), (G, struct.unpack("<f", struct.pack("<I", 1))[0], "1.4013e-45"), (G, 0.0, "0"),
]


@pytest.mark.parametrize("kind,value,text", TABLE)
def test_ties_and_edges(kind, value, text):
    assert capi.format_number(kind, value) == text
    assert FMT[kind] % value == text  # (the reference agrees with the table)


def test_zeros_infinities_and_nans():
    nan, inf = float("nan"), float("inf")
    neg_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
    assert [capi.format_number(E1, v) for v in (0.0, -0.0, inf, -inf, nan, neg_nan)] == ["0.0e+00", "-0.0e+00", "inf", "-inf", "nan", "-nan"]
    assert [capi.format_number(G, v) for v in (-0.0, inf, -inf, nan, neg_nan)] == ["-0", "inf", "-inf", "nan", "-nan"]
    assert [capi.format_number(F1, v) for v in (0.0, -0.0)] == ["0.0", "-0.0"]
    assert capi.format_number(F2, 999999999999999.875) == "999999999999999.88"
    assert capi.format_number(E1, 2.2250738585072014e-308) == "2.2e-308"


def test_e1_of_random_bit_patterns():
    bits = np.random.default_rng(1).integers(0, 1 << 64, N_RANDOM, dtype=np.uint64)
    _check(E1, [v for v in bits.view(np.float64).tolist() if not math.isnan(v)])  # (Python's % drops a nan's sign: see above for nans)


def test_g_of_random_float_bit_patterns():
    bits = np.random.default_rng(2).integers(0, 1 << 32, N_RANDOM, dtype=np.uint64).astype(np.uint32)
    with np.errstate(invalid="ignore"):  # (signalling nans among the patterns)
        values = bits.view(np.float32).astype(np.float64).tolist()
    _check(G, [v for v in values if not math.isnan(v)])


@pytest.mark.parametrize("kind", [F1, F2])
def test_f_of_random_values(kind):
    rng = np.random.default_rng(3 + kind)
    # the binades of the domain: from the subnormals' up to [2^48, 2^49) (2^49 < 1e15), random mantissas and signs
    ex = rng.integers(0, 1023 + 49, N_RANDOM, dtype=np.uint64)
    ex[: N_RANDOM // 2] = rng.integers(1023 - 12, 1023 + 12, N_RANDOM // 2, dtype=np.uint64)  # half of them where scores and percentages lie
    bits = (rng.integers(0, 2, N_RANDOM, dtype=np.uint64) << np.uint64(63)) | (ex << np.uint64(52)) | rng.integers(0, 1 << 52, N_RANDOM, dtype=np.uint64)
    values = bits.view(np.float64).tolist()
    assert all(abs(v) < 1e15 for v in values)
    _check(kind, values)


def test_f_exact_ties_on_a_grid():
    grid = range(-2000, 2001)
    _check(F1, [k / 8 for k in grid] + [k / 16 for k in grid])  # exact doubles: x.x5 (a tie of %.1f) wherever k/8 or k/16 ends in 25 or 75
    # k/800 and k/1600 are ties of %.2f only where the double is exact (k a multiple of 25 resp. 50 over a power of two); the others
    # lie a hair off the tie, on whichever side the nearest double fell
    _check(F2, [k / 800 for k in grid] + [k / 1600 for k in grid])
    _check(F2, [k / 8 for k in grid] + [k / 16 for k in grid] + [k / 32 for k in grid])


def test_refusals():
    lib = capi.load()
    buf = C.create_string_buffer(32)
    assert lib.lx_format_number(E1, 1.25, buf, 8) == 7 and buf.value == b"1.2e+00"  # the text and its NUL fit exactly
    assert lib.lx_format_number(E1, 1.25, buf, 7) == capi.LX_EINVAL
    assert lib.lx_format_number(E1, 1.25, buf, 0) == capi.LX_EINVAL
    assert lib.lx_format_number(E1, 1.25, None, 32) == capi.LX_EINVAL
    for kind in (-1, 4, 99):
        assert lib.lx_format_number(kind, 1.25, buf, 32) == capi.LX_EINVAL
    for kind in (F1, F2):
        for v in (1e15, -1e15, 1e300, float("inf"), float("-inf"), float("nan")):
            assert lib.lx_format_number(kind, v, buf, 32) == capi.LX_EINVAL
        assert lib.lx_format_number(kind, math.nextafter(1e15, 0.0), buf, 32) > 0
    with pytest.raises(capi.LambdaExtError):
        capi.format_number(F1, 1e15)
