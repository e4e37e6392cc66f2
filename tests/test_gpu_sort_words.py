"""GPU tests of the library's radix sort (lx_sort_words_dev; l2_sort_count_kernel, l2_sort_scan_kernel, l2_sort_scatter_kernel and
l2_launch_sort in lx_level2.hip) called directly, against numpy's stable argsort.

key_bits is a mask: l2_launch_sort runs one pass for every 8-bit digit in which the mask has any bit set, and the pass sorts by the
whole digit.  So the reference sorts by key & (the 0xff bytes the mask touches), stably, and the result holds the full keys and the
values in that order; values are arange(n), so a stability error is an inequality.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from lambda_amd import capi

pytestmark = pytest.mark.gpu

TILE = 4096  # kL2SortTile: 4 wavefronts x 16 rounds x 64 lanes
MASKS = [
    0xFFFFFFFFFFFFFFFF,  # all 8 passes
    0xFF,                # one pass, digit 0
    0xFF00FF0000,        # digits 2 and 4: `continue` between them in l2_launch_sort's shift loop
    0x10,                # one bit selects its whole digit: `(bits >> shift) & 255ull` is a test, the kernels take `& 255u`
    0xFF << 56,          # the top digit alone: shift 56, bit 63 is part of an unsigned digit
    0,                   # no pass
]


def digit_mask(key_bits: int) -> int:
    return sum(0xFF << (8 * k) for k in range(8) if (key_bits >> (8 * k)) & 0xFF)


def reference(keys: np.ndarray, key_bits: int):
    dm = digit_mask(key_bits)
    order = np.argsort(keys & np.uint64(dm), kind="stable")
    return keys[order], order.astype(np.uint64), bin(dm).count("1") // 8


def device_sort(keys: np.ndarray, key_bits: int, stream=None):
    """(sorted keys, their values, sorted_in, buffer 0 afterwards) of one lx_sort_words_dev call; the scratch pair starts as all ones"""
    n = len(keys)
    k0 = torch.from_numpy(keys.view(np.int64).copy()).to("cuda:0")
    v0 = torch.arange(n, dtype=torch.int64, device="cuda:0")
    k1, v1 = torch.full_like(k0, -1), torch.full_like(v0, -1)
    torch.cuda.synchronize()
    where = capi.sort_words_dev(k0.data_ptr(), k1.data_ptr(), v0.data_ptr(), v1.data_ptr(), n, key_bits, 0, stream)
    assert where in (0, 1)
    k, v = ((k0, v0), (k1, v1))[where]
    return k.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint64), where, k0.cpu().numpy().view(np.uint64)


def check(keys: np.ndarray, key_bits: int, stream=None, what=""):
    want_k, want_v, passes = reference(keys, key_bits)
    got_k, got_v, where, buf0 = device_sort(keys, key_bits, stream)
    assert where == passes % 2, (what, hex(key_bits), where, passes)  # each pass swaps the buffers once
    bad = np.nonzero((got_k != want_k) | (got_v != want_v))[0]
    assert len(bad) == 0, (what, len(keys), hex(key_bits), len(bad), bad[:5], got_k[bad[:5]], want_k[bad[:5]], got_v[bad[:5]], want_v[bad[:5]])
    if passes == 0:
        assert where == 0 and (buf0 == keys).all(), what  # buffer 0 holds its input bytes unchanged


def random_keys(n: int, seed: int) -> np.ndarray:
    """uint64 keys over the whole range (half of them with bit 63 set), drawn from n // 2 + 1 values so that whole keys repeat"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 64, n // 2 + 1, dtype=np.uint64)
    keys = pool[rng.integers(0, len(pool), n)]
    assert n < 8 or ((keys >> np.uint64(63)) == 1).any()
    return keys


SIZES = [
    2, 63, 64, 65,                                       # a wavefront's row: the `valid` lanes of match_digit's ballot
    1023, 1024, 1025,                                    # a wavefront's share of a tile (kL2SortTile / 4): cnt[w] and the c0, c1, c2 offsets
    TILE - 1, TILE, TILE + 1,                            # one tile, and a second one with a single valid lane
    256 * TILE - 1, 256 * TILE, 256 * TILE + 1,          # 256 tiles: one round of l2_sort_scan_kernel's loop; 257: its second round and `carry`
]


@pytest.mark.parametrize("n", SIZES)
def test_sort_sizes_and_masks(lx_lib, n):
    keys = random_keys(n, n)
    for bits in MASKS:
        check(keys, bits, what=f"random n={n}")


def test_sort_degenerate_digits(lx_lib):
    rng = np.random.default_rng(17)
    n = TILE + 1
    distinct = rng.permutation(np.arange(1, 3 * n + 1, dtype=np.uint64))[:n] * np.uint64(0x9E3779B97F4A7C15)
    row = distinct.copy()
    row[1024 + 5 * 64: 1024 + 6 * 64] = row[0]  # round 5 of wavefront 1: `peers` is all 64 lanes, one leader adds 64
    cases = [
        # one digit value in every pass: a single nonzero row of ghist, the scan's totals all in one gtot entry
        ("all keys equal", np.full(5000, 0x0123456789ABCDEF, np.uint64)),
        # n = 4097: the last tile has 1 valid lane and 4095 invalid ones whose digit reads 0 as well (match_digit's `valid`)
        ("all digits 0", np.zeros(n, np.uint64)),
        # the same among other digits: were the invalid lanes counted as peers, the lone valid lane would not lead its group, digit 0
        # would be one short in gtot, and every other digit's base one too low
        ("random keys, the last tile's lone key is 0", np.concatenate([random_keys(TILE, 5), np.zeros(1, np.uint64)])),
        ("random keys, 65 zeros end in a row with 1 valid lane", np.concatenate([random_keys(TILE, 6), np.zeros(65, np.uint64)])),
        # digit 255 is the last row of ghist and the last entry of gtot (dbase[255] = everything before it)
        ("all digits 255", np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64)),
        # two groups per row interleaved: rank = popcount(peers below the lane) over every other lane
        ("two keys alternating", np.where(np.arange(n) % 2 == 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x00FF00FF00FF00FF))),
        ("64 equal keys in one wavefront row among distinct ones", row),
        ("sorted input", np.sort(random_keys(3 * TILE + 7, 3))),
        ("reversed input", np.sort(random_keys(3 * TILE + 7, 4))[::-1].copy()),
    ]
    for what, keys in cases:
        for bits in MASKS:
            check(keys, bits, what=what)


def test_sort_is_stable_across_tiles_and_wavefronts(lx_lib):
    """Keys drawn from 3 values over 3 tiles: every group spans all 12 wavefront shares, so the order inside a group is decided by the
    tile offsets (ghist after the scan), the wavefront offsets (cnt[w] = b + c0 + ...) and the rank inside a row, not by the keys."""
    rng = np.random.default_rng(23)
    vals = np.array([0x8000000000000001, 0x00000000000000FF, 0x8000000000000000], dtype=np.uint64)
    for n in (3 * TILE, 3 * TILE - 5):
        keys = vals[rng.integers(0, 3, n)]
        for bits in MASKS:
            check(keys, bits, what="3 values over 3 tiles")


def test_sort_digit_count_buffer_is_grown_and_reused(lx_lib):
    """hist_buf (lx_sort_words_dev) is kept per device and grown: 100 words, then 257 tiles (gtot sits behind tiles * 256 counts of the
    larger buffer), then 100 again on the large buffer with gtot back at 256."""
    for n, seed in ((100, 1), (256 * TILE + 1, 2), (100, 3)):
        check(random_keys(n, seed), 0xFFFFFFFFFFFFFFFF, what=f"n={n} in a row")
        check(random_keys(n, seed), 0xFF00, what=f"n={n} in a row")


def test_sort_on_a_stream_of_the_callers(lx_lib):
    """A non-default stream (the kernels and the final hipStreamSynchronize take `stream`); the caller's current device stays."""
    before = torch.cuda.current_device()
    s = torch.cuda.Stream(device="cuda:0")
    for n in (TILE + 1, 100_000):
        check(random_keys(n, n), 0xFFFFFFFFFFFFFFFF, stream=s.cuda_stream, what="stream")
        check(random_keys(n, n), 0xFF00FF0000, stream=s.cuda_stream, what="stream")
    assert torch.cuda.current_device() == before
