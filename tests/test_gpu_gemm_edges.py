"""GPU (-m gpu): every GEMM instantiation (csrc/gemm.hip, gemm_pl.hip, gemm_grad.hip, gemm_wd.hip, gemm_small.hip) at its tile
edges, with leading dimensions wider than the matrices and sentinel / NaN guard rows and columns around every buffer, against the
float64 reference of tests/gemm_cases.py, whose docstring defines the buffers, the per-band error, the bounds and the cases.  Every
test prints the figures it measured before it asserts (`gemm_edges ...` lines: case, kernel, output, band, error, bound);
profiles/gemm_edges_errors.txt is that output for the whole table."""
import importlib.util
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("gemm_cases", ROOT / "tests" / "gemm_cases.py")
    mod = sys.modules.setdefault("gemm_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclasses look themselves up)
    if not hasattr(mod, "CASES"):
        spec.loader.exec_module(mod)
    return mod


gc = load_cases()
KERNELS = {}               # case -> pfpp_last_gemm_kernel() of its launch (the coverage test reads it)


def _run(dev, name):
    c = gc.CASES[name]
    rep, flags = gc.run(c, dev)
    print(gc.describe(rep))
    KERNELS[name] = rep["kernel"]
    assert rep["finite"], (name, "non-finite output")
    assert rep["guards_ok"], (name, "a guard row or column of an output was written")
    for tag, band, e, bound in rep["lines"]:
        assert e <= bound, (name, rep["kernel"], tag, band, e, bound)
    return rep, flags


@pytest.mark.parametrize("name", gc.GROUPS["A"])
def test_a_plane_gemm_variants_and_forms(dev, name):
    """pfpp_gemm_planes: every forced variant of the nt, nn (dX) and tn (dW) forms on both sides of its tile in M and N, ragged
    contractions with NaN rows after row K (dW), K splits through the workspace / atomics / with the fused column sum, alpha,
    bias + residual with ldr != ldc, the activations, the single-pass mode; the non-accumulating nt launches without a K split also equal
    pfpp_gemm on the same planes bit for bit"""
    _, flags = _run(dev, name)
    c = gc.CASES[name]
    if c.form == "nt" and not c.o("accumulate") and c.o("splits") == 1 and c.N > 64:      # (pfpp_gemm never splits K; it needs N > 64)
        assert flags["same_bits"] is True, (name, "pfpp_gemm_planes differs from pfpp_gemm on the same planes")


@pytest.mark.parametrize("name", gc.GROUPS["B"])
def test_b_gemm_with_a_pre_split_activation(dev, name):
    """pfpp_gemm with a SplitAct A: the tiles choose_planes_variant picks at 200, 3,850 and 16,385 rows on both sides of their edges,
    plane output with ldc > N, GEGLU at N = 128 and 192, the single-pass mode; wherever pfpp_gemm_planes accepts the call (all but
    GEGLU and plane output) it gives the same bits on the same planes"""
    _, flags = _run(dev, name)
    if gc.planes_twin(gc.CASES[name]):
        assert flags["same_bits"] is True, (name, "pfpp_gemm differs from pfpp_gemm_planes on the same planes")


@pytest.mark.parametrize("name", gc.GROUPS["C"])
def test_c_gemm_register_staged_fp32_and_fused_paths(dev, name):
    """pfpp_gemm: one group of cases per Kern:: value of choose_kernel, each at the smallest size that selects it and off the tile
    grid in M and N; NaN in the K .. lda pads; fused BatchNorm operand, statistics, pooling with c_min; split K with and without the
    lent workspace; the fused grouping"""
    _run(dev, name)


@pytest.mark.parametrize("name", gc.GROUPS["D"])
def test_d_gemm_batched(dev, name):
    """pfpp_gemm with batch = 6, zdiv = 2 and every one of sA, sW, sC, sV non-zero, on the f16x3 plain-W path and the fp32
    w_kmajor path; guard rows between the batch slices of C"""
    _run(dev, name)


@pytest.mark.parametrize("name", gc.GROUPS["E"])
def test_e_gemm_grad(dev, name):
    """pfpp_gemm_grad (nt, nn, tn; two tiles each; K in {1, 31, 148, 353}; split_k in {0, 1, 3} with accumulate; colsum; operand
    scales) and a pfpp_gemm_grad_group launch of 8 ragged problems"""
    _run(dev, name)


@pytest.mark.parametrize("name", gc.GROUPS["F"])
def test_f_dw_group(dev, name):
    """pfpp_gemm_dw_group: variants 0, 3, 6, 7 on four jobs of different sizes in one launch, K in {1, 33, 97, 385} with NaN rows after
    row K, gb = None on one job"""
    _run(dev, name)


@pytest.mark.parametrize("name", gc.GROUPS["G"])
def test_g_weight_direct_and_few_row_gemm(dev, name):
    """pfpp_gemm_wd (also transposed and _f16) and pfpp_gemm_small at M in {1, 31, 33, 127, 129}, the smallest N and K each accepts,
    ldc > N, the residual aliasing the output; gemm_wd equals the tiled plane GEMM on the same operands bit for bit"""
    _, flags = _run(dev, name)
    if gc.CASES[name].entry == "wd":
        assert flags["same_bits"] is True, (name, "pfpp_gemm_wd differs from the tiled plane GEMM")


def test_every_pinned_instantiation_ran_against_a_reference(dev):
    """the kernel names recorded by groups A to G include every distinct expected name of the tables of
    test_gemm_kernel_choice_is_pinned and test_wd_and_small_kernel_choice_is_pinned: no instantiation is left that is launched by
    name only"""
    import test_gpu_parity as tgp

    for name in [n for g in "ABCDEFG" for n in gc.GROUPS[g]]:     # (a run of this test alone: launch what has not run yet)
        if name not in KERNELS:
            rep, _ = gc.run(gc.CASES[name], dev)
            KERNELS[name] = rep["kernel"]
    want = {k for _, k in tgp._gemm_choice_cases().values()} | {k for _, k in tgp._wd_small_choice_cases().values()}
    missing = sorted(want - set(KERNELS.values()))
    assert not missing, missing
