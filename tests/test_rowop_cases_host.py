"""Host (no GPU): the case table of tests/rowop_cases.py checks itself.  Case names are unique and every entry point of FAMILY is
declared in include/pfpp.h and reached by at least one case; the table holds the shapes it is meant to; every reference is finite
(the loss over an empty selection aside, which is NaN by contract) and at most MAX_EXCLUDED of a check's elements are left out of a
comparison; the float32 CPU evaluation of each case is within 1/8 of its bound (the bounds are not set by the inputs); no reference
depends on what the NaN guards hold; the guard layout satisfies the entry point's alignment and divisibility rules; a result off by
one fp16 rounding is over every bound; the restated dropout generator agrees with its arithmetic in Python integers."""
import importlib.util
import math
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("rowop_cases", ROOT / "tests" / "rowop_cases.py")
    mod = sys.modules.setdefault("rowop_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclasses look themselves up)
    if not hasattr(mod, "CASES"):
        spec.loader.exec_module(mod)
    return mod


rc = load_cases()


def test_names_are_unique_and_the_family_is_declared_and_covered():
    names = [c.name for t in (rc._table_l, rc._table_d, rc._table_b, rc._table_s, rc._table_g, rc._table_n, rc._table_p, rc._table_m,
                              rc._table_a) for c in t()]
    assert len(names) == len(set(names)) == len(rc.CASES)
    header = (ROOT / "include" / "pfpp.h").read_text()
    entries = {c.entry for c in rc.CASES.values()}
    for fn in rc.FAMILY:
        assert re.search(r"\bint\s+" + fn + r"\s*\(", header), fn
        assert fn in entries, fn
    assert entries <= set(rc.FAMILY)
    assert rc.MAX_EXCLUDED == 0.02 and set(rc.K) == set(rc.GROUPS) and all(rc.GROUPS.values())
    assert (rc.SENTINEL, rc.TOP, rc.GCOL, rc.YARD_SPARE) == (rc.gc.SENTINEL, rc.gc.TOP, rc.gc.GCOL, rc.gc.YARD_SPARE)


def test_the_table_holds_the_shapes_it_is_meant_to():
    C = rc.CASES
    of = lambda g, kind=None: [C[n] for n in rc.GROUPS[g] if kind is None or C[n].kind == kind]
    # L: three widths x fp32 / split output; rows next to the 4-row workgroup; a last batch of one row; truncated last groups
    L = of("L")
    assert {(c.o("C"), c.o("split")) for c in L} == {(w, s) for w in (256, 512, 1024) for s in (False, True)}
    assert {c.o("rows") for c in L} == {1, 3, 4, 5, 37} and {c.o("form") for c in L} == {"plain", "affine", "mod", "grp"}
    assert {c.o("gr") for c in L if c.o("form") == "grp"} == {1, 5, 25} and any(c.o("rpb") == 12 and c.o("rows") == 37 for c in L)
    assert all(rc.built(c)["bufs"]["mod"].ld == 2 * c.o("C") + 8 for c in L if c.o("form") in ("mod", "grp"))
    # D
    D = of("D")
    assert {c.o("C") for c in D} == {256, 512} and {c.o("rows") for c in D} == {1, 5, 37} and {c.o("p") for c in D} == {0.0, 0.2}
    assert {c.o("res") for c in D} == {False, True} and {c.o("planes") for c in D} == {False, True}
    assert {c.o("form") for c in D} == {"plain", "affine", "mod", "grp"} and any(c.o("p") == 0.0 and not c.o("res") for c in D)
    # B: 1, 1, 1, 2, 4, 4 and 5 slices of 8 rows per group
    B = of("B")
    assert {c.o("gr") for c in B} == set(rc.LNB_GROUP_ROWS) == {1, 3, 8, 9, 25, 32, 33}
    assert [-(-g // 8) for g in rc.LNB_GROUP_ROWS] == [1, 1, 1, 2, 4, 4, 5]
    assert {c.o("form") for c in B} == {"grp", "uni", "gamma", "none"}
    assert all(c.o("rows") == (70 if c.o("gr") == 33 else 2 * c.o("gr") + 1) for c in B if c.o("form") in ("gamma", "none"))
    for w in (256, 512):
        assert sum(c.o("C") == w and c.o("drop") is not None for c in B) >= 1 and sum(c.o("C") == w and bool(c.o("planes")) for c in B) >= 1
    assert any(bool(rc.built(c)["info"]["untouched"].any()) for c in B if c.o("form") == "grp")
    # S
    S = of("S", "colsum")
    assert {(c.o("cols"), c.o("rows")) for c in S if c.o("pad") == 4} == {(w, r) for w in (4, 252, 256, 260) for r in (1, 3, 4, 63, 64, 65, 129)}
    assert {(c.o("cols"), c.o("rows")) for c in S if c.o("x_off") == 3} == {(w, r) for w in (1, 3, 7) for r in (1, 63, 64, 65)}
    assert any(c.o("cols") == 8 and rc.built(c)["bufs"]["x"].ld == 9 for c in S) and {c.o("acc") for c in S} == {False, True}
    SP = of("S", "colsum_planes")
    assert {(c.o("cols"), c.o("rows")) for c in SP} == {(w, r) for w in (4, 256, 260) for r in (1, 15, 16, 17, 129)} | {(8, 8200)}
    assert {c.o("n") for c in of("S", "split")} == {4, 1020, 1024, 1028}
    # G
    shapes = {(1, 4), (3, 344), (1, 1024), (5, 12), (2, 2048)}
    for kind in ("geglu", "geglu_bwd"):
        assert {(c.o("rows"), c.o("inner")) for c in of("G", kind)} == shapes
        assert {(c.o("p"), c.o("planes")) for c in of("G", kind)} == {(p, q) for p in (0.0, 0.1) for q in (False, True)}
    assert {(c.o("act"), c.o("n"), c.o("bwd")) for c in of("G", "act")} == {(a, n, b) for a in ("none", "relu", "silu", "gelu")
                                                                           for n in (1, 255, 256, 257) for b in (False, True)}
    assert {(c.o("n"), c.o("res"), c.o("p")) for c in of("G", "dropout")} == {(n, r, p) for n in (1, 5, 1023, 1024, 1025)
                                                                             for r in (False, True) for p in (0.0, 0.2)}
    assert set(rc.GATE_VALUES) >= {0.0, 1e-3, -1e-3, 1.0, -1.0, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0, 1e4, -1e4, 3.5, -3.5}
    assert math.copysign(1.0, rc.GATE_VALUES[1]) == -1.0 and {100.0, -100.0} <= set(rc.ACT_VALUES)
    # N: every width at a slab edge and below its row phases (256 / (C / 4)); one row
    NS = of("N", "bn_stats")
    for w in (64, 128, 256, 512, 1024):
        rows = {c.o("rows") for c in NS if c.o("C") == w}
        assert rows & {2047, 2048, 2049, 4097} and any(r < max(2, 256 // (w // 4) + 1) for r in rows), (w, rows)
    assert any(c.o("rows") == 1 and c.o("running") for c in NS) and {c.o("running") for c in NS} == {False, True}
    NA = of("N", "bn_apply")
    assert {c.o("C") for c in NA} == {4, 36, 64, 1024} and {c.o("pool") for c in NA} == {0, 32, 64} and {c.o("orows") for c in NA} == {1, 3, 65}
    assert {(c.o("copies"), c.o("C")) for c in of("N", "bn_finalize")} == {(k, w) for k in (1, 64) for w in (64, 300)}
    assert of("N", "bn_minmax")
    # P
    PS = of("P", "softmax")
    assert {c.o("T") for c in PS} == {1, 63, 64, 65, 200} and {c.o("ld") - c.o("T") for c in PS} == {0, 3}
    assert {c.o("rows") for c in PS} == {1, 5, 13} and {c.o("rpb") for c in PS} == {1, 5, 13}
    assert {c.o("mask") for c in PS} == {"none", "trailing", "scattered", "batch_masked"}
    assert {(c.o("n"), c.o("L"), c.o("C"), c.o("bwd")) for c in of("P", "mean_pool")} == {(n, l, w, b) for n in (1, 3) for l in (1, 25, 32)
                                                                                        for w in (4, 260, 512) for b in (False, True)}
    # M
    M = of("M")
    assert {(c.o("n"), c.o("sel"), c.o("masked")) for c in M} == {(n, s, m) for n in (1, 63, 1023, 1024, 1025, 2049)
                                                                 for s in ("none", "all", "one", "random") for m in (False, True)}
    assert {c.o("grad_out") for c in M} == {1.0, 4096.0}
    # A
    A = of("A")
    assert {c.o("n") for c in A} == {1, 255, 256, 257, 1000} and {c.o("planes") for c in A} == {False, True}
    assert any(c.o("zero_grad") for c in A) and any(c.o("g_scale") == 1.0 / 4096 for c in A) and rc.ADAM_STEPS == 3
    for c in A:
        if c.o("guarded"):
            bad = rc.adam_bad_positions(c.o("n"))
            assert 0 in bad and c.o("n") - 1 in bad and (c.o("n") <= 256 or {255, 256} <= set(bad))


def _guard_fill_ok(name, buf_name, buf):
    fill = buf.alloc[buf.guard_mask()]
    assert fill.numel() > 0, (name, buf_name)
    if fill.dtype.is_floating_point:
        nan, sen = torch.isnan(fill), fill == (rc.SENTINEL_F16 if fill.dtype == torch.float16 else rc.SENTINEL)
        assert bool(nan.all()) or bool(sen.all()) or bool((fill == 1.0).all()), (name, buf_name)


def _out_names(ch):
    return [k if k.startswith("ret:") else k.partition(":")[0] for k in (ch.out if isinstance(ch.out, tuple) else (ch.out,))]


@pytest.mark.parametrize("name", list(rc.CASES))
def test_reference_layout_and_float32_yardstick(name):
    c = rc.CASES[name]
    b = rc.built(c)
    rc.check_layout(c)
    assert b["checks"]
    for ch in b["checks"]:
        # every compared output is a guarded buffer of the case (the overflow counters of a guarded AdamW aside: two ints the kernel
        # reaches through atomics at fixed offsets), and its guards hold a sentinel
        for k in _out_names(ch):
            if k.startswith("ret:"):
                assert c.kind == "adamw" and ch.tag == "overflow", (name, ch.tag)
                continue
            g = b["bufs"][k].alloc[b["bufs"][k].guard_mask()]
            if g.dtype.is_floating_point:          # (NaN: a buffer written in place, an input as well; every guard is compared in bits)
                sen = g == (rc.SENTINEL_F16 if g.dtype == torch.float16 else rc.SENTINEL)
                assert g.numel() and (bool(sen.all()) or bool(torch.isnan(g).all())), (name, ch.tag, k)
            elif g.dtype == torch.uint8:
                assert bool((g == rc.SENTINEL_U8).all()), (name, ch.tag, k)
        if ch.kind == "planes":
            assert ch.x32 is not None and (not ch.x32.startswith("twin:") or ch.x32[5:] in rc.built(rc.twin_of(c))["bufs"]), (name, ch.tag)
        if ch.kind == "bits":
            empty_loss = c.kind == "mse" and c.o("sel") == "none" and ch.tag == "loss"
            assert empty_loss or not ch.ref.dtype.is_floating_point or bool(torch.isfinite(ch.ref).all()), (name, ch.tag)
            continue
        assert ch.ref.dtype == torch.float64 and ch.unit.shape == ch.ref.shape and bool((ch.unit >= 0).all()), (name, ch.tag)
        assert rc.excluded_fraction(ch) <= rc.MAX_EXCLUDED, (name, ch.tag, rc.excluded_fraction(ch))
        assert bool(torch.isfinite(ch.ref).all()), (name, ch.tag)
    for buf_name, buf in b["bufs"].items():
        _guard_fill_ok(name, buf_name, buf)
    for tag, e in rc.yardstick(c):
        assert math.isfinite(e) and e * rc.YARD_SPARE <= rc.K[c.group], (name, tag, e, rc.K[c.group])
    for tag, e in rc.yardstick(c, True):
        assert math.isfinite(e) and e * rc.YARD_SPARE <= rc.KX[c.group], (name, tag, e, rc.KX[c.group])


@pytest.mark.parametrize("name", [n for n in rc.CASES if rc.CASES[n].kind not in ("dropout_mask",)])
def test_no_reference_depends_on_what_the_guards_hold(name):
    c = rc.CASES[name]
    refs = [(ch.ref.clone(), None if ch.unit is None else ch.unit.clone()) for ch in rc.built(c)["checks"]]
    for fill in (0.0, 1e30):
        b2 = rc.built_with_guards(c, fill)
        seen = False
        for buf in b2["bufs"].values():
            g = buf.alloc[buf.guard_mask()]
            seen |= g.numel() > 0 and g.dtype in (torch.float32, torch.float16) and bool((g.float() == min(fill, 65504.0 if g.dtype == torch.float16 else fill)).all())
        # (AdamW and the softmax work in place: their floating-point buffers are outputs, with sentinel guards)
        assert seen or c.kind in ("adamw", "softmax"), name
        for ch, (r, u) in zip(b2["checks"], refs):
            assert rc.same_bits(ch.ref, r), (name, ch.tag, fill)
            assert u is None or torch.equal(ch.unit, u), (name, ch.tag, fill)


def test_keep_mask_restates_the_generator():
    """three values of the splitmix64 finaliser worked by hand arithmetic in Python integers, and the mask's keep rate"""
    def rng(seed, site, idx):
        M = (1 << 64) - 1
        z = seed ^ ((site * 0xD6E8FEB86659FD93) & M)
        z = (z + (idx + 1) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return (z ^ (z >> 31)) >> 32
    thresh = int(float(torch.tensor(0.2, dtype=torch.float32)) * 4294967296.0)
    want = [int(rng(77, 3, i) >= thresh) for i in range(300)]
    assert rc.keep_mask(300, 0.2, 77, 3).tolist() == want
    assert bool(rc.keep_mask(1000, 0.0, 5, 1).all())
    assert abs(float(rc.keep_mask(200000, 0.2, 9, 2).float().mean()) - 0.8) < 0.005


@pytest.mark.parametrize("name", list(rc.CASES))
def test_a_result_off_by_one_fp16_rounding_is_over_the_bound(name):
    """the bounds are tight enough to matter: the reference itself, off by 2^-11 relative (a value that went through one fp16
    rounding, the smallest mistake a split-f16 path can make), is over the bound of every bounded check and of every plane pair"""
    c = rc.CASES[name]
    for ch in rc.built(c)["checks"]:
        ok = torch.isfinite(ch.ref) if ch.kind != "bits" else None
        if ch.kind == "bits" or not bool((ch.ref[ok] != 0).any()):
            continue
        wrong = torch.where(ok, ch.ref * (1.0 + 2.0 ** -11), torch.zeros((), dtype=torch.float64))
        if ch.kind == "bound":
            assert rc.units_error(ch, wrong) > rc.K[c.group], (name, ch.tag)
        else:
            hi, lo = rc.split_cpu(wrong.float(), ch.scale)
            assert rc.planes_error(ch, hi, lo, c.group) > 1.0, (name, ch.tag)
            x32 = ch.ref.float()
            hi, lo = rc.split_cpu(x32, ch.scale)                         # the exact split of a float32 value keeps the bare contract,
            assert max(rc.planes_contract(ch, x32, hi, lo)) <= 1.0, (name, ch.tag)
            bad_hi = (hi.float() * (1.0 + 2.0 ** -10)).half()             # a hi one fp16 ulp off the one lo was computed against does not
            assert rc.planes_contract(ch, x32, bad_hi, lo)[0] > 1.0, (name, ch.tag)
            if c.kind == "split":
                assert rc.planes_error(ch, hi, lo, c.group) <= 1.0, (name, ch.tag)
