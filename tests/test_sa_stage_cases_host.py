"""Host (no GPU): the case table of tests/sa_stage_cases.py checks itself.  The table is compared with the source (every SaKern
enumerator of csrc/sa_train.hip and every eval entry point has cases, the kernel names are the launch statements'); it holds the
edges it is meant to (G, grid caps, N, live-slot counts, reappearing slot 0, class mixes at the wrap points of the walk, one
workgroup per slice, workgroups without work); every reference is finite and no index list leaves its contract; the CPU yardstick
passes every bound with YARD_SPARE to spare; no reference depends on what the guards hold; each deliberately wrong variant of the
yardstick fails; the numpy schedule agrees with a brute-force restatement."""
import importlib.util
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("sa_stage_cases", ROOT / "tests" / "sa_stage_cases.py")
    mod = sys.modules.setdefault("sa_stage_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclasses look themselves up)
    if not hasattr(mod, "CASES"):
        spec.loader.exec_module(mod)
    return mod


sc = load_cases()
SRC = (ROOT / "puzzlefusion-plusplus_amd" / "csrc" / "sa_train.hip").read_text()
C = sc.CASES


def test_the_table_covers_every_enumerator_and_entry_point_of_the_source():
    enum = re.search(r"enum class SaKern \{([^}]*)\}", SRC).group(1)
    enumerators = {e.strip() for e in enum.split(",") if e.strip()}
    assert len(enumerators) == 13 and enumerators == {sc.KERN[k].enum for k in sc.T_KERNS}
    for k in sc.T_KERNS:
        kern = sc.KERN[k]
        # the reported name is the string of the enumerator's launch statement
        assert re.search(r"case SaKern::" + kern.enum + r":[^;]*\"" + re.escape(kern.name) + "\"", SRC), k
        mine = [c for c in C.values() if c.kern == k]
        assert any(not c.sched for c in mine), k
        assert any(c.sched for c in mine) == kern.sched_ok, k
        assert all(sc.nosched_twin(c).kern == k and not sc.nosched_twin(c).sched for c in mine if c.sched), k
    # the schedule-taking kernels are the ones the entry point lets a schedule through to
    assert {k for k in sc.T_KERNS if sc.KERN[k].sched_ok} == {"rows8", "tab128", "tab256", "wide2", "wide3"}
    header = (ROOT / "include" / "pfpp.h").read_text()
    for fn in sc.EVAL_ENTRIES + ("pfpp_sa_pad_schedule", "pfpp_sa_train_stage"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", header), fn
    assert {sc.KERN[k].enum for k in sc.E_KERNS} == set(sc.EVAL_ENTRIES)
    assert {sc.KERN[k].D for k in sc.E_KERNS if sc.KERN[k].enum == "pfpp_sa_table_planes"} == {128, 256}
    assert all(any(c.kern == k for c in C.values()) for k in sc.E_KERNS) and sc.GROUPS["P"]
    assert len({c.name for c in sc._table_t() + sc._table_p() + sc._table_e()}) == len(C)
    assert (sc.SENTINEL, sc.TOP, sc.YARD_SPARE) == (sc.gc.SENTINEL, sc.gc.TOP, sc.gc.YARD_SPARE)
    copies = re.search(r"BN_STAT_COPIES = (\d+)", (ROOT / "puzzlefusion-plusplus_amd" / "pfpp_hip" / "train_ops.py").read_text())
    assert int(copies.group(1)) == 64 == sc.COPIES[2]


def test_the_table_holds_the_edges_it_is_meant_to():
    assert sc.LIVE_SET == (1, 2, 16, 17, 31, 32, 33, 34, 47, 48, 49, 63, 64)
    assert [c.G for c in C.values() if c.group == "P"] == [1, 1023, 1024, 1025, 32768, 32769, 40000]
    per_reg = int(re.search(r"constexpr int PER_REG = (\d+);", SRC).group(1))
    assert sum(-(-c.G // 1024) > per_reg for c in C.values() if c.group == "P") == 2
    for k in sc.T_KERNS + ("mlp2_tab",):
        mine = [c for c in C.values() if c.kern == k]
        assert {c.G for c in mine} == set(sc.G_SET) and {c.wgs for c in mine} >= set(sc.WGS_SET), k
        assert {c.N for c in mine} == set(sc.N_SET) and {c.profile for c in mine} == {"unit", "span", "offset"}, k
        assert (3, 5, 48) in {(c.F, c.S, c.N) for c in mine}
        g = [sc.grids(k, c.G, c.wgs) + (c.G,) for c in mine]
        assert any(per == 1 for _, per, _, _ in g), k                                   # one workgroup per column slice
        assert any(stride > G for _, _, stride, G in g) and any(stride < G for _, _, stride, G in g), k
        if sc.KERN[k].grid.startswith("rows:"):
            assert any(4 * (per - 1) >= G for _, per, _, G in g), k                     # a workgroup with no work at all
        if k in sc.T_KERNS:
            assert {c.copies for c in mine} == {1, 3, 64}, k
    for k in sc.E_KERNS:
        assert {c.G for c in C.values() if c.kern == k} == set(sc.G_SET) and {c.N for c in C.values() if c.kern == k} == set(sc.N_SET), k
    # 64-neighbour levels: every live count and both reappearing lists in the base shape; class mixes at the wrap points
    for k in sc.KERN:
        if sc.KERN[k].ns != 64:
            continue
        base = next(c for c in C.values() if c.kern == k and c.G == 15 and c.wgs is None and c.N == 48 and c.profile == "unit" and not c.sched)
        want = sc.wanted_lives(base)
        assert {v for v, _ in want} >= set(sc.LIVE_SET) and {(v, r) for v, r in want if r is not None} == set(sc.REAPPEAR)
        idx = sc.make_idx(base)
        for i, (v, r) in enumerate(want):
            if r is not None:
                assert idx[i, r] == idx[i, 0] and v > r + 1 and idx[i, v - 1] != idx[i, 0]
    for k in sc.T_KERNS:
        if not sc.KERN[k].sched_ok:
            continue
        seen = set()
        for c in C.values():
            if c.kern == k and c.lives.startswith("n2="):
                n2, stride = int(c.lives[3:]), sc.grids(k, c.G, c.wgs)[2]
                assert stride == (8 if k == "rows8" else 4) * sc.grids(k, c.G, c.wgs)[1]
                if c.sched:
                    assert int(sc.built(c)["bufs"]["sched"].view[0, c.G]) == n2, c.name
                    assert sc.nosched_twin(c).lives == c.lives
                seen |= {"none" if n2 == 0 else "all" if n2 == c.G else "one" if n2 == 1 else f"stride{n2 - stride:+d}" if abs(n2 - stride) <= 1 else "?"}
        assert seen >= {"none", "all", "one", "stride-1", "stride+0", "stride+1"}, (k, seen)


@pytest.mark.parametrize("name", list(C))
def test_reference_index_lists_and_yardstick(name):
    c = C[name]
    b = sc.built(c)
    idx = b["o"]["idx"]
    assert int(idx.min()) == 0 and int(idx.max()) == c.N - 1 and not bool((idx == c.N - 2).any()), name
    if c.group == "P":
        assert sc.passes(sc.yardstick(c))
        return
    k = sc.KERN[c.kern]
    if k.ns == 64:
        assert sc.live_counts(idx.numpy()).tolist() == [v for v, _ in sc.wanted_lives(c)], name
        assert bool((idx == idx[:, :1])[torch.arange(64)[None] >= torch.from_numpy(b["o"]["live"]).long()[:, None]].all())
    assert b["ref"] and set(b["ref"]) == set(b["unit"])
    for tag, r in b["ref"].items():
        u = b["unit"][tag]
        assert r.dtype == torch.float64 and u.shape == r.shape and bool(torch.isfinite(r).all()) and bool(torch.isfinite(u).all()), (name, tag)
        assert bool((u >= 0).all()), (name, tag)
    for n, buf in b["bufs"].items():
        g = buf.alloc[buf.guard_mask()]
        assert g.numel() > 0, (name, n)
        if n in b["outs"]:
            want = sc.SENTINEL_F16 if g.dtype == torch.float16 else sc.SENTINEL
            assert bool((g == want).all()) and bool((buf.view == want).all() or n == "stats"), (name, n)
        elif g.dtype.is_floating_point:
            assert bool(torch.isnan(g).all()), (name, n)
        else:
            assert bool((g == (sc.SENTINEL_I32 if n == "sched" else c.N - 2)).all()), (name, n)
        assert n in ("xyz", "ctr") or (buf.off * buf.alloc.element_size()) % 16 == 0, (name, n)      # (coordinates are read one float at a time)
    if "stats" in b["bufs"]:
        assert bool((b["bufs"]["stats"].view != 0).all())
    if "y_prev" in b["bufs"]:
        fed = b["bufs"]["y_prev"].view
        assert bool(torch.isnan(fed[b["o"]["copy_rows"]]).all()) == c.sched and bool(torch.isfinite(fed[~b["o"]["copy_rows"]]).all())
    rep = sc.yardstick(c)
    assert rep["lines"] and all(rep["flags"].values()), (name, rep["flags"])
    for tag, e, bound in rep["lines"]:
        assert math.isfinite(e) and e * sc.YARD_SPARE <= bound, (name, tag, e, bound)


def _subset():
    names = []
    for k in sc.KERN:
        mine = [c for c in C.values() if c.kern == k and c.G == 15 and c.N == 48]
        for pick in (lambda c: c.wgs is None and c.profile == "unit" and not c.sched, lambda c: c.profile == "offset" and not c.sched,
                     lambda c: c.wgs is None and c.profile == "unit" and c.sched):
            names += [c.name for c in mine if pick(c)][:1]
    return names + ["P_sched_g1025"]


@pytest.mark.parametrize("name", _subset())
def test_no_reference_depends_on_what_the_guards_hold(name):
    c = C[name]
    b = sc.built(c)
    for fill in (0.0, 1e30):
        b2 = sc.built_with_guards(c, fill)
        seen = False
        for n, buf in b2["bufs"].items():
            g = buf.alloc[buf.guard_mask()]
            seen |= n in b2["inputs"] and g.dtype in (torch.float32, torch.float16) and bool((g.float() == min(fill, 65504.0 if g.dtype == torch.float16 else fill)).all())
        assert seen or c.group == "P", name
        for tag, r in b["ref"].items():
            assert sc.same_bits(b2["ref"][tag], r), (name, tag, fill)
            assert tag not in b["unit"] or sc.same_bits(b2["unit"][tag], b["unit"][tag]), (name, tag, fill)


def _fails(name, mut):
    return not sc.passes(sc.evaluate(C[name], sc.emulate(C[name], mut)))


SCHED_BASE = [f"T_{k}_g15_wall_sched" for k in ("rows8", "tab128", "tab256", "wide2", "wide3")]
MIXES = [n for n, c in C.items() if c.lives.startswith("n2=") and c.sched]
SENSITIVITY = {
    "drop_lo_hi": ["T_sa1_2_g15_wall", "T_sa2_2_g15_wall", "T_rows8_g15_wall", "T_wide1_g15_wall", "E_mlp3_g15_wall", "E_mlp2_tab_g15_wall"],
    "drop_hi_lo": ["T_sa1_3_g15_wall", "T_sa2_1_g15_wall", "T_tab256_g15_wall", "T_wide3_g15_wall", "E_mlp2_p_g15_wall"],
    "row_left_out": [f"T_{k}_g15_wall" for k in sc.T_KERNS],
    "live33_one_half": SCHED_BASE,
    "copies31": SCHED_BASE,
    "copies33": SCHED_BASE,
    "copies_row1": SCHED_BASE,
    "maxmin_swapped": ["T_sa1_3_g15_wall", "T_rows8_g15_wall", "T_rows8_g15_wall_sched", "T_wide3_g15_wall", "T_wide3_g15_wall_sched"],
    "channels_swapped": [f"T_{k}_g15_wall" for k in sc.T_KERNS] + [f"E_{k}_g15_wall" for k in sc.E_KERNS],
    "half1_rows_in_half0": ["T_sa2_2_g15_wall", "T_tab128_g15_wall", "T_tab128_g15_wall_sched", "T_tab256_g15_wall_sched", "T_wide1_g15_wall",
                            "T_wide2_g15_wall_sched"],
    "visited_twice": [f"T_{k}_g15_w1" for k in sc.T_KERNS],
    "skip_wrap": MIXES + [f"E_{k}_g15_wall" for k in sc.E_KERNS],
    "wrong_fragment": [f"T_{k}_g15_wall" for k in sc.T_KERNS if sc.KERN[k].src != "rows"] + [f"E_{k}_g15_wall" for k in sc.E_KERNS],
}


@pytest.mark.parametrize("mut", sorted(SENSITIVITY))
def test_a_deliberately_wrong_yardstick_fails(mut):
    """the table catches what it is for: every listed case fails under the mutation (and passes without it, by the test above)"""
    assert mut in sc.MUTATIONS and len(MIXES) >= 5 * 7
    for name in SENSITIVITY[mut]:
        assert _fails(name, mut), (mut, name)


def test_a_walk_with_the_wrong_wrap_point_fails_where_the_classes_do_not_fill_a_round():
    """ib without the "+ stride" of the waves below the wrap point: neighbourhoods visited twice and others never; every mix whose
    visit counts that changes fails"""
    hit = 0
    for name in MIXES:
        c = C[name]
        n2, stride = int(c.lives[3:]), sc.grids(c.kern, c.G, c.wgs)[2]
        base = sc.walk_visits(c.G, n2, stride, np.arange(c.G))
        assert base.tolist() == [1] * c.G, name                      # the restated walk visits every neighbourhood once
        wrong = sc.walk_visits(c.G, n2, stride, np.arange(c.G), True).tolist() != [1] * c.G      # (n2 a multiple of the stride: no wave is below the wrap point)
        assert wrong <= bool(n2 % stride), name
        assert _fails(name, "wrap_bug") == wrong, name
        hit += wrong
    assert hit >= 10, hit


def test_the_schedule_reference_agrees_with_a_brute_force_restatement():
    g = torch.Generator().manual_seed(5)
    for G in (1, 2, 7, 40):
        idx = torch.randint(0, 9, (G, 64), generator=g).numpy().astype(np.int32)
        for i in range(G):
            live = int(torch.randint(1, 65, (1,), generator=g))
            idx[i, live:] = idx[i, 0]
        lives = []
        for i in range(G):
            last = 0
            for j in range(64):
                if idx[i, j] != idx[i, 0]:
                    last = j
            lives.append(last + 1)
        two = [i for i in range(G) if lives[i] > 32]
        one = [i for i in range(G) if lives[i] <= 32]
        want = two + one + [len(two)] + lives + [lives[i] for i in two + one]
        got = sc.sched_ref(idx)
        assert got.dtype == np.int32 and got.tolist() == want
        assert sorted(got[:G].tolist()) == list(range(G))                                   # a permutation
        assert sc.live_counts(idx).tolist() == lives
