"""GPU (-m gpu): the attention kernels (csrc/attention.hip, attention_bwd.hip, transformer_ops.hip) at tile edges, masks and
magnitudes, against the float64 autograd reference of tests/attention_cases.py, whose docstring defines the per-block error, the
bounds and the cases.  Every test prints the figures it measured before it asserts (`attn_edges ...` lines: error, float32-CPU
yardstick, their ratio, bound, worst block); profiles/attn_edges_errors.txt is that output.

The two ends of the gradient-magnitude sweep are what the per-query-row lift of dS in the split-f16 backward (ab_row_scale in
csrc/attention_bwd.hip) is held in place by: with the fixed 2^14 lift alone, dO in [-15, 15] gave non-finite
dq / dk (D_g15-dh64, J_L7_g15, J_L32_g15: dS reaches 4.3 .. 6.5, past 65504 / 2^14) and dO of 1e-6 gave 2.2e-4 / 4.3e-5 of the
block maximum against the bound of 2e-5 (D_g1e-06-dh64, J_L32_g1e-06); now 8e-7 and 1.7e-5 / 1.1e-5.
"""
import importlib.util
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("attention_cases", ROOT / "tests" / "attention_cases.py")
    mod = sys.modules.setdefault("attention_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclass looks itself up)
    if not hasattr(mod, "DENSE"):
        spec.loader.exec_module(mod)
    return mod


ac = load_cases()


def _assert_report(rep):
    print(ac.describe(rep))
    assert rep["finite"], (rep["case"], "non-finite output inside a sequence")
    for qn, w in rep["worst"].items():
        assert w["err"] <= w["bound"], (rep["case"], w)


# ------------------------------------------------------------------------------------------------------------ dense: A - E, H
@pytest.mark.parametrize("name", list(ac.DENSE))
def test_dense(dev, name):
    """attn_dense_train, ops.attn_dense and attn_dense_bwd on one case: all outputs finite; out, lse, D and dq / dk / dv per
    (sequence, head) block against float64; out bit-equal to the inference forward of the same tile-walking kernel, and the
    inference forward as dispatched (the short-sequence kernel for small launches) within the bound of out (H); rows outside every
    sequence untouched (B; every case runs into sentinel-filled buffers); dk and dv exactly zero at masked keys (C)"""
    c = ac.DENSE[name]
    got, flags, _ = ac.run_dense(c, dev)
    _assert_report(ac.report(c, got))
    assert flags["fwd_equal"], "attn_dense_train's out differs from ops.attn_dense"
    assert flags["outside_kept"], "a row outside every sequence was written"
    assert flags["masked_zero"], "dk / dv at a masked key is not exactly zero"


@pytest.mark.parametrize("name", ac.F_CASES)
def test_dense_backward_in_parts_and_with_planes_is_the_same_bits(dev, name):
    """F: pfpp_attn_dense_bwd_parts with bits 1, 2, 4 as three calls on one stream, and with bits = 7 as one call, write the bits
    of pfpp_attn_dense_bwd (dqkv and D).  G: pfpp_attn_dense_bwd_p with both outputs writes the same fp32 bits, and planes whose
    hi + lo carries G x that result (test_gpu_train_ops._assert_planes_carry: 22 bits, hi a nearest fp16 of the value)."""
    import test_gpu_train_ops as tto
    from pfpp_hip import _lib, ops, planes as P

    c = ac.DENSE[name]
    _, _, d = ac.run_dense(c, dev)
    lib, ptr, st = _lib.load(), ops._ptr, ops._stream
    n_seq, C = len(c.lens), c.H * c.dh
    inside = ac.inputs(c)["inside"].to(dev)

    def parts(bits_list):
        dvec, dqkv = torch.full_like(d["dvec"], ac.SENTINEL), torch.full_like(d["dqkv"], ac.SENTINEL)
        for bits in bits_list:
            _lib.check(lib.pfpp_attn_dense_bwd_parts(ptr(d["qkv"]), ptr(d["out"]), ptr(d["dout"]), ptr(d["lse"]), ptr(dvec), ptr(dqkv),
                                                     ptr(d["so"]), ptr(d["sl"]), None, 0, n_seq, c.T, c.H, c.dh, c.scale, bits, st()),
                       "pfpp_attn_dense_bwd_parts")
        torch.cuda.synchronize()
        return dvec, dqkv

    for bits_list in ((1, 2, 4), (7,)):
        dvec, dqkv = parts(bits_list)
        assert torch.equal(dvec, d["dvec"]), bits_list
        assert torch.equal(dqkv, d["dqkv"]), bits_list
    dvec, dq32 = torch.full_like(d["dvec"], ac.SENTINEL), torch.full_like(d["dqkv"], ac.SENTINEL)
    dqp = P.Planes.empty(dq32.shape[0], 3 * C, dev, ac.G_PLANES)
    _lib.check(lib.pfpp_attn_dense_bwd_p(ptr(d["qkv"]), ptr(d["out"]), ptr(d["dout"]), ptr(d["lse"]), ptr(dvec), ptr(dq32), ptr(d["so"]),
                                         ptr(d["sl"]), None, 0, n_seq, c.T, c.H, c.dh, c.scale, P._pl(dqp), st()), "pfpp_attn_dense_bwd_p")
    torch.cuda.synchronize()
    assert torch.equal(dq32, d["dqkv"]) and torch.equal(dvec, d["dvec"])
    assert bool(torch.isfinite(dq32[inside]).all())
    tto._assert_planes_carry(dq32[inside], dqp.hi[inside], dqp.lo[inside], ac.G_PLANES, f"attn_dense_bwd planes {name}")


# ------------------------------------------------------------------------------------------------------------ block-diagonal: I - K
@pytest.mark.parametrize("name", list(ac.BLOCKDIAG))
def test_blockdiag(dev, name):
    """ops.attn_blockdiag and attn_blockdiag_bwd per (fragment, head, part) block against float64, over L in [1, 32] (I) and over the
    gradient-magnitude and logit-range sweeps (J: the kernel recomputes its own softmax with the keys past L masked, so it has no
    zero-staged pad keys; this pins that it stays that way)"""
    c = ac.BLOCKDIAG[name]
    got, _ = ac.run_blockdiag(c, dev)
    _assert_report(ac.report(c, got))


@pytest.mark.parametrize("L", ac.K_LS)
def test_blockdiag_backward_with_planes_is_the_same_bits(dev, L):
    """K: pfpp_attn_blockdiag_bwd_p with both outputs: the fp32 bits of the plain call, planes that carry G x them"""
    import test_gpu_train_ops as tto
    from pfpp_hip import _lib, ops, planes as P

    c = ac.BLOCKDIAG[f"I_L{L}_f3h2"]
    _, d = ac.run_blockdiag(c, dev)
    dq32 = torch.full_like(d["dqkv"], ac.SENTINEL)
    dqp = P.Planes.empty(dq32.shape[0], dq32.shape[1], dev, ac.G_PLANES)
    _lib.check(_lib.load().pfpp_attn_blockdiag_bwd_p(ops._ptr(d["qkv"]), ops._ptr(d["dout"]), ops._ptr(dq32), len(c.lens), L, c.H, c.dh,
                                                     c.scale, P._pl(dqp), ops._stream()), "pfpp_attn_blockdiag_bwd_p")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dq32).all())
    assert torch.equal(dq32, d["dqkv"])
    tto._assert_planes_carry(dq32, dqp.hi, dqp.lo, ac.G_PLANES, f"attn_blockdiag_bwd planes L={L}")


# ------------------------------------------------------------------------------------------------------------ the switched-off kernels
@pytest.mark.parametrize("names", ac.CROSS_CHECKS, ids="+".join)
def test_kernels_behind_the_process_static_switches(dev, names):
    """The exact-fp32 kernels (attn_dense_bwd_*_kernel<64> unmasked, attn_blockdiag_bwd_mfma_kernel, attn_blockdiag_bwd_kernel and
    the forward kernels the same settings select) are never picked at the defaults (csrc/attn_choice.h), so cases A, C and I run once
    more per cross-check setting (ops.attention_cross_check; once environment switches read once per process, hence the name) and are
    held to the same bounds, finiteness and bitwise properties."""
    from pfpp_hip import ops

    bad = {}
    ops._sync_attention_mode()          # the default mode, whatever ran before: attn_dense_train does not put it back itself
    with ops.attention_cross_check(*names):
        for name in ac.CHILD_DENSE + ac.CHILD_BD:
            if name in ac.DENSE:
                c = ac.DENSE[name]
                got, flags, _ = ac.run_dense(c, dev)
            else:
                c = ac.BLOCKDIAG[name]
                (got, _), flags = ac.run_blockdiag(c, dev), {}
            rep = ac.report(c, got)
            print(ac.describe(rep))
            over = {qn: w for qn, w in rep["worst"].items() if not w["err"] <= w["bound"]}
            if not rep["finite"] or over or not all(flags.values()):
                bad[name] = dict(finite=rep["finite"], over=over, flags=flags)
    assert not bad, bad
