"""GPU parity at every query width where the rule for the multi-panel carry workspace changes its answer: 152 | 153 (the (8,19) panel),
160 | 161 (the generic (16,10) panel), 208 | 209 (the (16,13) panel) and 305 (two (8,19) panels plus one column).  The hint each entry
point hands to the workspace comes from the plan that runs (plan_trace / plan_score / plan_step, lambda_amd/csrc/lx_step_plan.cpp): it is
zero where one panel holds every query and covers every subject row where a launch carries.  Three entry points take pass 2 there:
pass 2 alone on a device list (lx_align_batch_dev, with hints), pass 2 alone on a host list (lx_align_batch) and the fused step
(lx_extend_batch_dev) with LX_OPT_PASS2_MODE 1 and 2.

Every case runs on a fresh handle with LX_OPT_WORKSPACE_BYTES at its minimum (1 MiB = 131 072 carry pairs), so the workspace is what the
call itself asked for.  32 extensions fit the minimum whatever the hint (32 x 329 rows); the `crowded` cases -- 1024 extensions, 189 440
to 336 896 rows -- do not: where their launch carries, a missing hint is the device's "carry workspace exhausted" error and no luck.

Asserted: scores, begin / end cells and op bytes against the oracle, and the kernel each call reports."""
import numpy as np
import pytest

from lambda_amd import capi, synth
from tests import limit_gpu
from tests.test_oracle import SCHEMES

pytestmark = pytest.mark.gpu

WIDTHS = (152, 153, 160, 161, 208, 209, 305)
CROWDED = (161, 209, 305)  # the first width of each rule that carries
ENTRIES = ("align_dev", "align_host", "fused_mode1", "fused_mode2")
RUN = 16
CUTOFF = 60  # (the fused step's filter; pass 2 alone aligns every extension)

# the kernels each call reports, (lx_last_trace_kernel_name, lx_last_kernel_name): literals from a run of the commit before the plans moved
# to lx_step_plan.cpp
NAMES = {
    ("align_dev", 152): ("lx::trace_forward_kernel<16,10,false>", "lx::score_kernel<16,10,false>"),
    ("align_dev", 153): ("lx::trace_forward_kernel<16,10,false>", "lx::score_kernel<16,10,false>"),
    ("align_dev", 160): ("lx::trace_forward_kernel<16,10,false>", "lx::score_kernel<16,10,false>"),
    ("align_dev", 161): ("lx::trace_forward_kernel<16,10,true>", "lx::score_kernel<16,13,false>"),
    ("align_dev", 208): ("lx::trace_forward_kernel<16,10,true>", "lx::score_kernel<16,13,false>"),
    ("align_dev", 209): ("lx::trace_forward_kernel<16,10,true>", "lx::score_kernel<16,16,false>"),
    ("align_dev", 305): ("lx::trace_forward_kernel<16,10,true>", "lx::score_kernel<16,10,true>"),
    ("align_host", 152): ("lx::ckpt_forward_kernel<8,19>", "lx::score_kernel<16,10,false>"),
    ("align_host", 153): ("lx::ckpt_forward_kernel<16,13>", "lx::score_kernel<16,10,false>"),
    ("align_host", 160): ("lx::ckpt_forward_kernel<16,13>", "lx::score_kernel<16,10,false>"),
    ("align_host", 161): ("lx::ckpt_forward_kernel<16,13>", "lx::score_kernel<16,13,false>"),
    ("align_host", 208): ("lx::ckpt_forward_kernel<16,13>", "lx::score_kernel<16,13,false>"),
    ("align_host", 209): ("lx::ckpt_forward_kernel<8,19>", "lx::score_kernel<16,16,false>"),
    ("align_host", 305): ("lx::ckpt_forward_kernel<16,13>", "lx::score_kernel<16,10,true>"),
    ("fused_mode1", 152): ("lx::ckpt_forward_kernel<8,19>", "lx::score_pair_kernel<8,19> (+ int32 fix-up lx::score_kernel<8,19,false>)"),
    ("fused_mode1", 153): ("lx::ckpt_forward_kernel<16,13>", "lx::score_pair_kernel<8,24> (+ int32 fix-up lx::score_kernel<16,10,false>)"),
    ("fused_mode1", 160): ("lx::ckpt_forward_kernel<16,13>", "lx::score_pair_kernel<8,24> (+ int32 fix-up lx::score_kernel<16,10,false>)"),
    ("fused_mode1", 161): ("lx::ckpt_forward_kernel<16,13>", "lx::score_pair_kernel<8,24> (+ int32 fix-up lx::score_kernel<16,13,false>)"),
    ("fused_mode1", 208): ("lx::ckpt_forward_kernel<16,13>", "lx::score_pair_kernel<16,13> (+ int32 fix-up lx::score_kernel<16,13,false>)"),
    ("fused_mode1", 209): ("lx::ckpt_forward_kernel<8,19>", "lx::sweep_pair16_kernel<8,19,true,false> (+ int32 fix-up lx::score_kernel<16,16,false>)"),
    ("fused_mode1", 305): ("lx::ckpt_forward_kernel<16,13>", "lx::sweep_pair16_kernel<8,19,true,false> (+ int32 fix-up lx::score_kernel<16,10,true>)"),
    ("fused_mode2", 152): ("lx::score_pair_kernel<8,19,true> (single sweep)",) * 2,
    ("fused_mode2", 153): ("lx::score_pair_kernel<8,25,true> (single sweep)",) * 2,
    ("fused_mode2", 160): ("lx::score_pair_kernel<8,25,true> (single sweep)",) * 2,
    ("fused_mode2", 161): ("lx::score_pair_kernel<8,25,true> (single sweep)",) * 2,
    ("fused_mode2", 208): ("lx::score_pair_kernel<16,13,true> (single sweep; + int32 fix-up lx::ckpt_forward_kernel<16,13,false>)",) * 2,
    ("fused_mode2", 209): ("lx::sweep_pair16_kernel<8,19,true,true,true> (single sweep, compact codes; + int32 fix-up lx::ckpt_forward_kernel<8,19,false>)",) * 2,
    ("fused_mode2", 305): ("lx::sweep_pair16_kernel<8,19,true,true,true> (single sweep, compact codes; + int32 fix-up lx::ckpt_forward_kernel<8,19,false>)",) * 2,
}


def batch(width, n_queries):
    """n_queries x 16 windows of width + 24 rows (cut from the generator's windows of width + 2 (isqrt(width) + 1) >= width + 26)"""
    q, s, ext = synth.make_batch_np(n_queries, width, RUN, seed=1000 + width)
    ext["s_len"] = width + 24
    return q, s, ext


def fresh_handle(mode):
    h = capi.Handle(0)
    h.set_scoring(SCHEMES["blosum62"], 0)
    h.set_option(capi.LX_OPT_WORKSPACE_BYTES, 0)  # (the library's floor: 1 MiB)
    assert h.get_option(capi.LX_OPT_WORKSPACE_BYTES) == 1 << 20
    h.set_option(capi.LX_OPT_PASS2_MODE, mode)
    return h


def align_dev(h, q, s, ext):
    """lx_align_batch_dev with LX_OPT_MAX_QLEN / LX_OPT_MAX_SLEN: (hsp, ops offsets, ops, kernel names)"""
    import torch

    n, dev, pad = len(ext), torch.device("cuda:0"), np.zeros(256, np.uint8)
    d_q, d_s = torch.from_numpy(np.concatenate([q, pad])).to(dev), torch.from_numpy(np.concatenate([s, pad])).to(dev)
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).to(dev)
    sizes = ext["q_len"].astype(np.uint64) + ext["s_len"].astype(np.uint64)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)[:-1]
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_ops = torch.zeros(int(sizes.sum()) + 16, dtype=torch.uint8, device=dev)
    d_hsp = torch.full((n * 48,), 0xEE, dtype=torch.uint8, device=dev)
    h.set_option(capi.LX_OPT_MAX_QLEN, int(ext["q_len"].max()))
    h.set_option(capi.LX_OPT_MAX_SLEN, int(ext["s_len"].max()))
    torch.cuda.synchronize()
    h.align_batch_dev(d_q, d_s, d_ext, n, d_hsp, d_ops, d_off)
    h.synchronize()
    hsp = np.frombuffer(d_hsp.cpu().numpy().tobytes(), dtype=capi.HSP_DTYPE)
    return hsp, off, d_ops.cpu().numpy(), (h.last_trace_kernel_name(), h.last_kernel_name())


def run_case(entry, width, n_queries):
    """One call of `entry` on a fresh handle: (scores, hsp, ops offsets, ops, kernel names)"""
    q, s, ext = batch(width, n_queries)
    h = fresh_handle(2 if entry == "fused_mode2" else 1)
    try:
        if entry == "align_dev":
            hsp, off, ops, names = align_dev(h, q, s, ext)
            return hsp["score"].copy(), hsp, off, ops, names
        if entry == "align_host":
            hsp, ops, off = h.align_batch(q, s, ext, raw=True)
            return hsp["score"].copy(), hsp, off, ops, (h.last_trace_kernel_name(), h.last_kernel_name())
        score, hsp, off, ops, name = limit_gpu.run_dev(h, q, s, ext, RUN, CUTOFF, 2 if entry == "fused_mode2" else 1)
        return score, hsp, off, ops, (name, h.last_kernel_name())
    finally:
        h.close()


def check(oracle, entry, width, n_queries):
    q, s, ext = batch(width, n_queries)
    cutoff = CUTOFF if entry.startswith("fused") else 0
    want, surv, want_ops, want_rec = limit_gpu.oracle_results(oracle, ("carry", width, n_queries), SCHEMES["blosum62"], q, s, ext, cutoff)
    score, hsp, off, ops, names = run_case(entry, width, n_queries)
    print(entry, width, n_queries, names)
    if entry.startswith("fused"):
        assert (score == want).all(), (entry, width)
    assert len(surv) > 5
    for i, oops, rec in zip(surv, want_ops, want_rec):
        g = hsp[i]
        assert tuple(int(g[f]) for f in limit_gpu.FIELDS[:6]) == rec[:6], (entry, width, i)  # score, begin / end cells, number of ops
        st = int(off[i]) + int(g["ops_shift"])
        assert bytes(ops[st: st + rec[5]]) == oops, (entry, width, i)
    assert names == NAMES[(entry, width)], (entry, width, names)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_carry_edge(oracle, lx_lib, entry, width):
    check(oracle, entry, width, 2)


@pytest.mark.parametrize("width", CROWDED)
@pytest.mark.parametrize("entry", ENTRIES)
def test_carry_edge_crowded(oracle, lx_lib, entry, width):
    check(oracle, entry, width, 64)
