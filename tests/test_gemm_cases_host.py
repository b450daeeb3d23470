"""Host (no GPU): the GEMM edge-case table of tests/gemm_cases.py checks itself.  The table holds the groups it is meant to, every
float64 reference is finite and no band of it is identically zero, every guard layout satisfies the entry point's alignment rules,
the float32 CPU evaluation of each case passes the band bounds with a factor 8 to spare (for every tile shape a launch could
report: the bounds are not set by the inputs), and the NaN rows after row K of a k-major operand are outside every reference."""
import importlib.util
import math
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("gemm_cases", ROOT / "tests" / "gemm_cases.py")
    mod = sys.modules.setdefault("gemm_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclasses look themselves up)
    if not hasattr(mod, "CASES"):
        spec.loader.exec_module(mod)
    return mod


gc = load_cases()
TILES = ((32, 128), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (256, 128), (256, 256))


def test_the_table_holds_the_groups_it_is_meant_to():
    C = gc.CASES
    assert all(gc.GROUPS[g] for g in "ABCDEFG")
    # A: every variant a form accepts, three sizes around its tile; K splits three ways; alpha; bias + residual; activations; single pass
    for form in ("nt", "nn", "tn"):
        for v in gc.PL_VARIANTS:
            bm, bn = gc.PL_TILE[form][v]
            ms = [C[f"A_{form}_v{v}_{s}"].M for s in "m0p"]
            ns = [C[f"A_{form}_v{v}_{s}"].N for s in "m0p"]
            assert ms[0] < bm == ms[1] < ms[2] and ns[0] < bn == ns[1] < ns[2]
        for s in ("split3_ws", "split3_ws_acc", "split3_atomic", "alpha", "bias_res"):
            assert f"A_{form}_{s}" in C
        assert C[f"A_{form}_split3_ws"].K == 352 and C[f"A_{form}_alpha"].o("alpha") == 0.37
    assert {C[n].K for n in gc.GROUPS["A"] if C[n].form == "tn"} >= {1, 31, 33, 97}
    assert {C[n].K for n in gc.GROUPS["A"] if C[n].form != "tn"} >= {32, 96}
    assert {C[n].o("act") for n in gc.GROUPS["A"]} >= {"relu", "silu", "gelu"}
    assert sum(bool(C[n].o("single_pass")) for n in gc.GROUPS["A"]) == 4 and sum(bool(C[n].o("colsum")) for n in gc.GROUPS["A"]) >= 6
    # B: pre-split A at 200 / 3850 / 16385 rows, plane output, GEGLU at N = 128 and 192
    assert {C[n].M for n in gc.GROUPS["B"]} >= {200, 3850, 16385} and C["B_geglu_n128"].N == 128 and C["B_geglu_n192"].N == 192
    assert C["B_planes_out"].o("out_planes") and all(C[n].o("a") == "planes" for n in gc.GROUPS["B"])
    # C: one group per Kern:: value
    for stem in ("pre256x256", "pre256x128pf2", "pre256x128pf2_aff", "deep64x64_m1", "deep64x128_geglu_m65", "pre128x64pf2_1008_tiles",
                 "pre128x128pf2_1024_tiles", "pre128x128_2048_tiles", "pre128x64_stats", "plain128x128_k7", "plain128x64_k132",
                 "f32_128x128", "f32_128x64", "f32k_128x128", "f32k_128x64", "af32_n72", "af32_n136_affine_stats", "af32_pool32_cmin",
                 "split_k_ws", "split_k_no_ws", "gather_d0", "gather_d32"):
        assert "C_" + stem in C
    assert C["C_af32_n72"].M == 65537 and C["C_pre256x256"].M == 8193 and C["C_split_k_ws"].K == 2048
    # D: batch 6, zdiv 2 on the two paths of the denoiser
    assert all(C[n].o("batch") == 6 and C[n].o("zdiv") == 2 for n in gc.GROUPS["D"]) and {C[n].M for n in gc.GROUPS["D"]} == {7, 33}
    # E
    assert {C[n].K for n in gc.GROUPS["E"] if C[n].entry == "grad"} >= {1, 31, 148, 353}
    assert {C[n].o("split_k") for n in gc.GROUPS["E"] if C[n].o("accumulate")} >= {0, 1, 3}
    assert {(4, 260), (8, 8)} <= {j[:2] for j in C["E_group"].jobs} and len(C["E_group"].jobs) == 8
    # F
    assert {C[n].o("variant") for n in gc.GROUPS["F"]} == {0, 3, 6, 7} and {C[n].K for n in gc.GROUPS["F"]} == {1, 33, 97, 385}
    assert all(C[n].jobs == ((8, 8), (72, 136), (264, 120), (136, 264)) for n in gc.GROUPS["F"])
    # G
    for kind in ("wd", "small"):
        assert {C[n].M for n in gc.GROUPS["G"] if n.startswith(f"G_{kind}_m")} == {1, 31, 33, 127, 129}
    assert C["G_wd_transposed"].o("kind") == "t" and C["G_wd_f16"].o("kind") == "f16"


@pytest.mark.parametrize("name", list(gc.CASES))
def test_reference_layout_and_float32_yardstick(name):
    c = gc.CASES[name]
    b = gc.built(c)
    gc.check_layout(c)
    for p in b["problems"]:
        assert bool(torch.isfinite(p.ref).all()) and p.ref.dtype == torch.float64, (name, p.tag)
    for buf_name, buf in b["bufs"].items():
        fill = buf.alloc[buf.guard_mask()]
        if buf_name.startswith(("out", "colsum", "gb", "c_min")):
            assert bool((fill == (gc.SENTINEL_F16 if buf.alloc.dtype == torch.float16 else gc.SENTINEL)).all()), (name, buf_name)
        elif not buf_name.startswith("stats"):
            assert bool(torch.isnan(fill).all()) and fill.numel() > 0, (name, buf_name)
    for BM, BN in TILES:
        for tag, band, e, bound in gc.yardstick(c, BM, BN):
            # the factor 8 belongs to the band bounds; the whole-matrix bounds are the entry points' own, float32 only has to meet them
            assert math.isfinite(e) and e * (1.0 if band == "whole" else gc.YARD_SPARE) <= bound, (name, (BM, BN), tag, band, e, bound)


K_TAIL_CASES = [n for n, c in gc.CASES.items() if c.entry in ("planes", "grad", "dw_group", "grad_group") and
                (c.form == "tn" or c.entry in ("dw_group", "grad_group"))]


@pytest.mark.parametrize("name", K_TAIL_CASES)
def test_reference_of_a_weight_gradient_does_not_depend_on_the_rows_after_k(name):
    """the k-major operands carry KTAIL rows of NaN directly after row K.  The case built again with 0 and with 1e30 in those rows
    has bit for bit the same references, and the same product when it is restated from the allocations a launch reads; read one row
    further (what a kernel that rounds K up would do), that product is no longer finite: the NaN sits where such a kernel reads"""
    c = gc.CASES[name]
    b = gc.built(c)
    refs = [p.ref.clone() for p in b["problems"]]
    read = gc.read_reference(c, b)
    assert all(bool(torch.isfinite(v).all()) for v in read.values())
    assert all(not bool(torch.isfinite(v).any()) for v in gc.read_reference(c, b, extra_rows=1).values())
    for fill in (0.0, 1e30):
        b2 = gc.built_with_tail(c, fill)
        for name_, buf in b2["bufs"].items():
            if buf.alloc.shape[0] - buf.top - buf.rows == gc.KTAIL:
                tail = buf.alloc[buf.top + buf.rows:].float()
                assert bool((tail == torch.tensor(fill, dtype=buf.alloc.dtype).float()).all()), (name, name_)
        assert all(torch.equal(p.ref, r) for p, r in zip(b2["problems"], refs)), (name, fill)
        read2 = gc.read_reference(c, b2)
        assert all(torch.equal(read2[j], read[j]) for j in read), (name, fill)
    # and the product read from the allocations is the one inside the reference (which adds C0, bias, residual, alpha around it)
    if not (c.o("bias") or c.o("residual")):
        scale = 4096.0 if c.entry in ("dw_group", "planes") else 1.0
        for j, prod in read.items():
            p = next(q for q in b["problems"] if q.out == f"out{j}")
            c0 = b["bufs"][f"out{j}"].view.double() if (c.o("accumulate") or c.entry in ("dw_group", "grad_group")) else 0.0
            want = c0 + b.get("alpha", 1.0) * prod / scale
            assert float((p.ref - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
