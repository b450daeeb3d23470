"""No GPU: pfpp_hip.matching_assign.assign_reference, the numpy restatement the device solver is held to bit for bit, against
scipy.optimize.linear_sum_assignment on float64 of the same float32 matrix, against its own optimality certificate, and through
match_edges; the launch plan; and the argument checks of the two new entry points, all of which return before a launch."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import matching_assign_cases as AC

ROOT = Path(__file__).resolve().parents[1]


def weight(c: np.ndarray, col: np.ndarray) -> float:
    """sum_i c[i, col_i] in float64, in row order"""
    total = 0.0
    for x in c[np.arange(col.size), col].astype(np.float64):
        total += float(x)
    return total


@pytest.mark.parametrize("name", AC.NAMES)
def test_reference_against_scipy(name):
    """a permutation of scipy's weight; every row scipy matches to a positive entry has scipy's column, and the rows that differ
    sit on exact zeros in both (group 6, exact ties, by weight alone)"""
    case, ref, want = AC.case(name), AC.reference(name), AC.scipy_col(name)
    c, n = case.c, case.c.shape[0]
    assert ref.status == 0 and ref.col.dtype == np.int64
    assert sorted(ref.col.tolist()) == list(range(n))
    assert weight(c, ref.col) == weight(c, want)
    if case.by_weight:
        return
    rows = np.arange(n)
    positive = c[rows, want] > 0
    assert (ref.col[positive] == want[positive]).all(), np.nonzero(ref.col != want)[0][:8]
    differ = ref.col != want
    assert (c[rows, ref.col][differ] == 0).all() and (c[rows, want][differ] == 0).all()


@pytest.mark.parametrize("name", AC.NAMES)
def test_reference_duals_certify_the_optimum(name):
    """independent of scipy: cost_ij - u_i - v_j >= -1e-12 everywhere and |.| <= 1e-12 on the matched entries.  Entries are of order
    1 and a dual is rewritten at most once per augmentation with a rounding of 2^-53: at most a few hundred augmentations here
    (1,025 rows at the very most), so the error stays below 1e-13 and the bar leaves a factor of ten or more."""
    c, ref = AC.case(name).c, AC.reference(name)
    red = -c.astype(np.float64) - ref.u[:, None] - ref.v[None, :]
    assert red.min() >= -1e-12, red.min()
    assert np.abs(red[np.arange(c.shape[0]), ref.col]).max() <= 1e-12


@pytest.mark.parametrize("name", AC.SINKHORN_LIKE)
def test_match_edges_of_the_reference_equal_scipys(name):
    """rows that differ sit on same-piece zeros, which match_edges never counts: edges and correspondence lists are equal"""
    from pfpp_hip.matching import match_edges

    case = AC.case(name)
    nc = np.asarray(case.pieces)
    e0, c0 = match_edges(AC.scipy_col(name), nc, nc.size)
    e1, c1 = match_edges(AC.reference(name).col, nc, nc.size)
    assert e0.shape[0] >= 1 and np.array_equal(e0, e1) and len(c0) == len(c1)
    assert all(np.array_equal(a, b) for a, b in zip(c0, c1))


def test_case_properties_the_kernel_tests_rely_on():
    """the shapes the cases were chosen for, so that a case cannot silently lose them"""
    ref = AC.reference
    assert ref("identity_257").augmentations == 0 and ref("identity_257").steps == 0
    assert ref("chain_130").augmentations == 1 and ref("chain_130").steps == 130        # one search that scans every column
    assert ref("dominated_65").augmentations == 64                                     # n - 1 rows left free
    assert ref("uniform_1").steps == 0 and ref("uniform_1").col.tolist() == [0]
    c = AC.case("sk_200_20_30").c
    assert int((c[np.arange(250), ref("sk_200_20_30").col] == 0).sum()) == 150          # forced onto exact zeros
    assert all(AC.case(k).c.dtype == np.float32 and AC.case(k).c.flags.c_contiguous for k in AC.NAMES)
    assert [AC.case(k).c.shape[0] for k in AC.SINKHORN_LIKE] == [63, 65, 97, 250, 257, 600, 192, 2492]
    for k in AC.SINKHORN_LIKE:
        piece = np.repeat(np.arange(len(AC.case(k).pieces)), AC.case(k).pieces)
        assert (AC.case(k).c[piece[:, None] == piece[None, :]] == 0).all()
    assert ref("workload_2492").steps > 2492                                            # a workload-sized search load


def test_budget():
    from pfpp_hip.matching_assign import BUDGET_FACTOR, assign_reference, default_budget

    c, full = AC.case("sk_30_35").c, AC.reference("sk_30_35")
    assert full.steps >= 2
    assert assign_reference(c, max_steps=1).status == 1
    assert assign_reference(c, max_steps=full.steps - 1).status == 1
    again = assign_reference(c, max_steps=full.steps)
    assert again.status == 0 and again.steps == full.steps and np.array_equal(again.col, full.col)
    assert default_budget(2492) == BUDGET_FACTOR * 2492 and default_budget(0) == 1
    with pytest.raises(ValueError, match="budget"):
        assign_reference(c, max_steps=0)


def test_plan_assign_restates_the_launch_ladder():
    from pfpp_hip.matching_assign import MAX_N, MAX_PUZZLES, plan_assign, workgroup_shape

    header = (ROOT / "include" / "pfpp.h").read_text()
    for name, value in (("MAX_N", MAX_N), ("MAX_PUZZLES", MAX_PUZZLES)):
        assert int(re.search(rf"#define PFPP_MATCH_ASSIGN_{name} (\d+)", header).group(1)) == value
    src = (ROOT / "puzzlefusion-plusplus_amd" / "csrc" / "matching_assign.hip").read_text()
    ladder = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"n_max <= (\d+)\) launch_solve<(\d+), (\d+)>", src)]
    assert len(ladder) == 9 and re.search(r"else launch_solve<1024, 8>", src)
    for cap, t, k in ladder:
        assert workgroup_shape(cap) == (t, k) and t * k >= cap
        assert workgroup_shape(cap + 1) != (t, k)
    assert workgroup_shape(1) == (64, 1) and workgroup_shape(MAX_N) == (1024, 8)
    with pytest.raises(ValueError):
        workgroup_shape(MAX_N + 1)
    sizes = [5] * MAX_PUZZLES + [300, 7]
    assert plan_assign(sizes) == [(0, MAX_PUZZLES, 64, 1), (MAX_PUZZLES, 2, 512, 1)]
    assert plan_assign([2492] * 16) == [(0, 16, 1024, 3)] and plan_assign([]) == []


def test_new_entries_are_declared_and_refuse_bad_arguments_before_a_launch(hip_lib):
    import torch

    from pfpp_hip import _lib
    from pfpp_hip.matching_assign import assign_batch

    header = (ROOT / "include" / "pfpp.h").read_text()
    assert "int pfpp_match_assign(" in header and "int64_t pfpp_match_assign_workspace(" in header
    assert "linear_solvers.py:279-340" in header
    lib = _lib.load()
    arr = lambda ctype, vals: (ctype * len(vals))(*vals)
    one = 4096                                              # any non-null address: never dereferenced on these paths
    p = C.c_void_p(one)
    n2, mats = arr(C.c_int64, [4, 7]), arr(C.c_void_p, [one, one])
    assert lib.pfpp_match_assign_workspace(2, n2) == 4 * 11
    assert lib.pfpp_match_assign_workspace(0, n2) == -1 and lib.pfpp_match_assign_workspace(2, None) == -1
    assert lib.pfpp_match_assign_workspace(2, arr(C.c_int64, [4, 0])) == -1
    assert lib.pfpp_match_assign_workspace(2, arr(C.c_int64, [8192, 8193])) == -1
    assert lib.pfpp_match_assign_workspace(1, arr(C.c_int64, [8192])) == 4 * 8192
    budget = arr(C.c_int64, [10, 10])

    def call(B=2, c=mats, n=n2, steps=budget, outs=None, ws=p, ws_bytes=44):
        outs = [p] * 6 if outs is None else outs
        return lib.pfpp_match_assign(B, c, n, steps, *outs, ws, ws_bytes, None)

    assert call(B=0) == -1 and b"B < 1" in lib.pfpp_last_error()
    for kw in ({"c": None}, {"n": None}, {"steps": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null" in lib.pfpp_last_error(), kw
    for bad in range(6):
        outs = [p] * 6
        outs[bad] = None
        assert call(outs=outs) == -1 and b"null" in lib.pfpp_last_error(), bad
    assert call(c=arr(C.c_void_p, [one, None])) == -1 and b"null matrix" in lib.pfpp_last_error()
    assert call(n=arr(C.c_int64, [4, 0])) == -1 and b"n < 1" in lib.pfpp_last_error()
    assert call(n=arr(C.c_int64, [4, 8193])) == -2 and b"unsupported" in lib.pfpp_last_error()        # PFPP_EUNSUPPORTED
    assert call(steps=arr(C.c_int64, [10, 0])) == -1 and b"budget" in lib.pfpp_last_error()
    assert call(ws_bytes=43) == -1 and b"workspace" in lib.pfpp_last_error()
    assert call(ws=C.c_void_p(one + 2)) == -1 and b"aligned" in lib.pfpp_last_error()
    with pytest.raises(ValueError, match="GPU"):
        assign_batch([torch.zeros(2, 2)])
    with pytest.raises(ValueError, match="no matrices"):
        assign_batch([])
