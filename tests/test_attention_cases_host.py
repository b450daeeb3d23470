"""Host (no GPU): the attention edge-case table of tests/attention_cases.py checks itself.  Every case's float64 reference is
finite, the float32 CPU autograd of the same formula (the yardstick of the GPU tests' bounds) stays inside the bound it defines, and
the negative-logit cases really are inputs at which a zero-staged pad key overflows the lifted dS of the split-f16 dq pass."""
import importlib.util
import math
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("attention_cases", ROOT / "tests" / "attention_cases.py")
    mod = sys.modules.setdefault("attention_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclass looks itself up)
    if not hasattr(mod, "DENSE"):
        spec.loader.exec_module(mod)
    return mod


ac = load_cases()
ALL = {**ac.DENSE, **ac.BLOCKDIAG}


def test_the_table_holds_the_cases_it_is_meant_to():
    assert sum(ac.EDGE_LENS) == 1249
    for path in ac.DENSE_PATHS:
        for stem in ["A", "A_h3", "B"] + [f"D_g{g:g}" for g in (1e-6, 1e-3, 1.0, 15.0)] + \
                    [f"E_{v}" for v in ("neg8", "neg10", "neg12", "pos8", "pos12", "x4", "neg6_do1")]:
            assert f"{stem}-{path}" in ac.DENSE
    assert ac.DENSE["A_h3-dh64"].H == 3 and ac.DENSE["A_h3-dh64"].lens == (33, 1, 129)
    b = ac.DENSE["B-dh64"]
    rows, off, inside = ac.layout(b)
    assert b.T == 384 > max(b.lens) and off != sorted(off) and rows == 1249 + 5 * 11 and int(inside.sum()) == 1249
    assert not bool(inside[:5].any()) and not bool(inside[-5:].any())
    assert {c.mask for n, c in ac.DENSE.items() if n.startswith("C_")} == set(ac.MASKS)
    assert all(min(c.lens) > 32 for n, c in ac.DENSE.items() if n.startswith("C_no_"))
    for L in ac.BD_LS:
        assert ac.BLOCKDIAG[f"I_L{L}_f3h2"].lens == (L,) * 3 and ac.BLOCKDIAG[f"I_L{L}_f1h1"].H == 1
    assert all(c.dh == 64 for c in ac.BLOCKDIAG.values())
    assert [n for n in ac.CHILD_DENSE if n[0] not in "AC"] == [] and len(ac.CHILD_DENSE) == 8 + 10 and len(ac.CHILD_BD) == 20


@pytest.mark.parametrize("name", list(ALL))
def test_reference_is_finite_and_float32_autograd_stays_within_the_bound(name):
    c = ALL[name]
    r64, _ = ac.refs(c)
    for k in ("out", "lse", "D", "dqkv"):
        assert bool(torch.isfinite(r64[k]).all()), (name, k)
    if c.mask is not None:         # a masked key gets no gradient, and still acts as a query
        C = c.H * c.dh
        inp = ac.inputs(c)
        for s, (o, n) in enumerate(inp["groups"]):
            bad = ~inp["key_valid"][s, :n]
            assert bool((r64["dqkv"][o:o + n, C:][bad] == 0).all())
            if int((~bad).sum()) > 1:          # (with one valid key every query's softmax is that key alone: dq = 0)
                assert bool((r64["dqkv"][o:o + n, :C][bad].abs().amax(1) > 0).all())
    yard, bnd = ac.yardstick(c), ac.bounds(c)
    over = {b: (y, bnd[b]) for b, y in yard.items() if not y <= bnd[b]}
    assert not over, (name, over)
    assert all(math.isfinite(v) and v >= ac.floor_of(c, b[0]) for b, v in bnd.items())


def test_negative_logit_cases_reach_the_pad_key_overflow():
    """ab_dq_f16_body (csrc/attention_bwd.hip) stages the keys past the end of a sequence as zero rows: S = 0 there, so the
    recomputed 'probability' is exp(-lse_q) and the lifted dS is exp(-lse_q) (v_{T-1} . dO_q - D_q) scale 2^14 (the line
    `s[e] = pv * (dp[e] * (1.0f / AB_GS) - Dq) * (scale * AB_DS)`), which the fp16 split turns into +-inf from 65520 on (the
    kernel now selects zero for those keys on the last tile, so these inputs are what keeps that select in place).  This is a
    property of the inputs, computed in float64 from the reference: the cases m = -10 and -12 with dO of
    1e-3, and m = -6 with dO of 1, have query rows at or over that threshold.  m = -8 with dO of 1e-3 is an order of
    magnitude short of it (lse >= -6.4 there: exp(6.4) 1e-2 2048 ~ 1e4), so it runs as a case below the condition and is asserted to be one."""
    frac = {}
    for v in ("neg8", "neg10", "neg12", "neg6_do1"):
        c = ac.DENSE[f"E_{v}-dh64"]
        assert c.shift < 0 and all(n % 32 for n in c.lens)
        frac[v] = ac.overflow_margin(c)
    print(frac)
    for v in ("neg10", "neg12", "neg6_do1"):
        assert frac[v][0] >= 65520.0 and frac[v][1] > 0, (v, frac[v])
    assert frac["neg12"][1] > 0.5                     # most rows (94 % in a float64 emulation of the kernel's arithmetic)
    assert frac["neg8"][0] < 65520.0, frac["neg8"]
    for v in ("neg8", "neg10", "neg12", "neg6_do1"):  # while the true gradients are finite and well scaled
        assert float(ac.refs(ac.DENSE[f"E_{v}-dh64"])[0]["dqkv"].abs().max()) < 10.0
