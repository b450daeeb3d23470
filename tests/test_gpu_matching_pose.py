"""GPU: the matcher's pairwise RANSAC and the ragged nearest distance (csrc/matching_pose.hip, pfpp_hip/matching_eval.py) against the
float64 restatement of tests/matching_pose_cases.py, which tests/test_matching_pose_host.py pins to Random123's known answers and to
the reference's own horn_87.  Every test prints the figures it measured before it asserts.

Bars.
* Draws are integer arithmetic: the kernel's hypothesis h must use the restatement's triple.  A count only depends on the triple, so
  counts equal to the restatement's for every hypothesis are the check; hypotheses too close to a decision to be compared between two
  fp64 evaluations are set aside - relative eigen-gap below 1e-6, or some | d^2 - max_dist^2 | < 1e-9 - and at most 1 % of a case's
  hypotheses may be (hypotheses that both sides call degenerate are compared, not set aside).
* The winner: its count is the restatement's maximum, and it is one of the restatement's hypotheses with that count whose sumsq is
  within 1e-9 relative of the least.
* The winner's pose against the restatement's float64 pose of the same hypothesis: R within 2^-24, t within 2^-24 max(|t|, 1) (one
  rounding to fp32 is 2^-25 of a value below 1; the Jacobi's own error over a relative gap >= 0.02, asserted, is orders below);
  |R R^T - 1| <= 4 x 2^-24, det R > 0.
* Refinement: against the restatement's refined pose (fed the GPU's winner) at the same bars; against the planted pose 4 x the
  restatement's own deviation from it, floor 4 x 2^-24.
* Ragged nearest distance: bit for bit the float32 evaluation (dx dx + dy dy) + dz dz of numpy and bit for bit pfpp_nn_dist on every
  segment; against float64 6 x 2^-24 d^2: three roundings of the differences enter squared (2 each), three of the squares, two of
  the sums - at most 2 + 1 + 2 roundings of 2^-24 on any term, and the minimum of perturbed values moves by no more."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("matching_pose_cases", Path(__file__).resolve().parent / "matching_pose_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

U24 = cases.U24
H_MAX = 1024
H_LIST = (1, 255, 256, 257, 1024)
M_LIST = (3, 4, 7, 64, 65, 300, cases.TILE, cases.TILE + 1)
SEED = (0x5851F42D << 32) | 11            # both halves of the key in use
CASE_SEED = 3

_refs = {}


def reference(M: int, pad: int = 5):
    """the planted case of M correspondences and its restatement at H_MAX hypotheses, computed once"""
    if M not in _refs:
        k = cases.planted_case(M, seed=CASE_SEED, pad=pad)
        _refs[M] = (k, cases.ransac_reference(k["pts"], k["pair"], k["corr"], H_MAX, seed=SEED))
    return _refs[M]


def run(dev, pts, pairs, corr, H, **kw):
    from pfpp_hip.matching_eval import ransac_pairs

    out = ransac_pairs(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), pairs, corr, n_hyp=H, seed=SEED, return_counts=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_pair(tag, got, e, ref, H, *, pose=True):
    """one pair of a launch against its restatement (at >= H hypotheses)"""
    counts, sumsq, aside = ref["counts"][:H], ref["sumsq"][:H], ref["aside"][:H]
    g = got["counts"][e]
    both_degenerate = (g == -1) & (counts == -1)
    set_aside = aside & ~both_degenerate
    wrong = (g != counts) & ~set_aside
    h = int(got["best_h"][e])
    print(f"{tag} H={H}: set aside {int(set_aside.sum())}, degenerate {int((counts < 0).sum())}, wrong {int(wrong.sum())}, winner h={h} "
          f"count={int(got['count'][e])} (restatement h={int(np.lexsort((np.arange(H), sumsq, -counts))[0])} count={int(counts.max())})")
    assert set_aside.sum() <= 0.01 * H
    assert not wrong.any(), np.nonzero(wrong)[0][:8]
    assert got["status"][e] == 1 and 0 <= h < H
    assert got["count"][e] == counts.max() == g[h]
    tied = np.nonzero(counts == counts.max())[0]
    assert h in tied and sumsq[h] <= sumsq[tied].min() * (1 + 1e-9)
    # sumsq itself: two fp64 evaluations of d whose poses differ by the solvers' 1e-13 at most
    delta = 1e-13
    bar = 2 * np.sqrt(sumsq[h] * max(counts[h], 1)) * delta + counts[h] * delta ** 2
    print(f"    sumsq {got['sumsq'][e]:.6e} vs {sumsq[h]:.6e} (bar {bar:.1e}), gap {ref['gap'][h]:.3f}")
    assert abs(got["sumsq"][e] - sumsq[h]) <= bar
    if not pose:                                                     # counts and the winner only
        return
    assert ref["gap"][h] >= cases.GAP_MIN
    check_pose(got["R"][e], got["t"][e], ref["R64"][h], ref["t64"][h])


def check_pose(R, t, R64, t64):
    dR, dt = np.abs(R - R64).max(), np.abs(t - t64).max()
    orth = np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(3)).max()
    print(f"    |R - R64| {dR:.2e} (bar {U24:.2e}), |t - t64| {dt:.2e} (bar {U24 * max(np.abs(t64).max(), 1):.2e}), |R R^T - 1| {orth:.2e}")
    assert dR <= U24 and dt <= U24 * max(np.abs(t64).max(), 1.0)
    assert orth <= 4 * U24 and np.linalg.det(R.astype(np.float64)) > 0


@pytest.mark.parametrize("M", M_LIST)
def test_every_hypothesis_and_the_winner_match_the_restatement(dev, M):
    k, ref = reference(M)
    for H in H_LIST:
        got = run(dev, k["pts"], [k["pair"]], [k["corr"]], H)
        check_pair(f"M={M}", got, 0, ref, H)
    # the planted pose is found once enough hypotheses are drawn
    assert got["count"][0] >= int(k["inlier"].sum())


def three_pairs():
    """three pairs of different sizes in one launch, the first two sharing their source piece: pts = A | filler | B | C | D | E"""
    rng = np.random.default_rng(17)
    ka, kb, kc = (cases.planted_case(M, seed=s, pad=p) for M, s, p in ((300, 21, 3), (7, 22, 0), (65, 23, 9)))
    # pair 0: A -> B (300 matches).  pair 1: A -> C over seven of A's points.  pair 2: D -> E, a case of its own
    nA = 300
    A = ka["pts"][3:3 + nA]
    B = ka["pts"][ka["pair"][1]:ka["pair"][1] + nA]
    R1, t1 = cases.rotation(rng), rng.uniform(-1, 1, 3)
    pick = rng.permutation(nA)[:7]
    C = (A[pick].astype(np.float64) @ R1.T + t1).astype(np.float32)
    pts = np.concatenate([A, rng.uniform(-1, 1, (11, 3)).astype(np.float32), B, C, kc["pts"]])
    oB, oC, oK = nA + 11, nA + 11 + nA, nA + 11 + nA + 7
    pairs = [(0, oB), (0, oC), (oK + kc["pair"][0], oK + kc["pair"][1])]
    corr = [ka["corr"], np.stack([pick, np.arange(7)], 1), kc["corr"]]
    return pts, pairs, corr


def test_three_pairs_of_different_sizes_two_of_them_sharing_a_piece(dev):
    pts, pairs, corr = three_pairs()
    refs = [cases.ransac_reference(pts, pairs[e], corr[e], H_MAX, e=e, seed=SEED) for e in range(3)]
    assert not np.array_equal(refs[2]["triples"], cases.draw_triples(65, np.arange(H_MAX), 0, SEED))          # the pair index moves the stream
    for H in H_LIST:
        got = run(dev, pts, pairs, corr, H)
        for e in range(3):
            check_pair(f"pair {e} (M={len(corr[e])})", got, e, refs[e], H)
    again = run(dev, pts, pairs, corr, 1024)
    for key in got:
        assert np.array_equal(got[key], again[key]), key                                        # two runs agree bitwise
    # a pair's result does not depend on the launch it is part of, only on its index (the Philox counter)
    alone = run(dev, pts, pairs[:1], corr[:1], 1024)
    for key in ("R", "t", "best_h", "count", "sumsq", "status", "counts"):
        assert np.array_equal(got[key][0], alone[key][0]), key


def test_production_call_without_counts_empty_batch_and_wrong_dtype(dev):
    from pfpp_hip.matching_eval import ransac_pairs

    k, _ = reference(65)
    pts = torch.from_numpy(k["pts"]).to(dev)
    with_counts = ransac_pairs(pts, [k["pair"]], [k["corr"]], n_hyp=300, seed=SEED, return_counts=True)
    plain = ransac_pairs(pts, [k["pair"]], [k["corr"]], n_hyp=300, seed=SEED)                   # counts_out is null, as in production
    assert "counts" not in plain
    for key in plain:
        assert torch.equal(plain[key], with_counts[key]), key
    other = ransac_pairs(pts, [k["pair"]], [k["corr"]], n_hyp=300, seed=SEED + 1, return_counts=True)
    assert not torch.equal(other["counts"], with_counts["counts"])                              # the seed moves the draws
    none = ransac_pairs(pts, np.zeros((0, 2), dtype=np.int64), [], n_hyp=300, return_counts=True)
    assert none["R"].shape == (0, 3, 3) and none["t"].shape == (0, 3) and none["counts"].shape == (0, 300) and none["status"].numel() == 0
    with pytest.raises(ValueError, match="dtype"):
        ransac_pairs(pts.double(), [k["pair"]], [k["corr"]], n_hyp=300)


def test_all_outliers_repeated_points_and_collinear_triples(dev):
    rng = np.random.default_rng(29)
    # every correspondence an outlier: unrelated clouds
    pts = rng.uniform(-0.5, 0.5, (80, 3)).astype(np.float32)
    corr = np.stack([np.arange(40), rng.permutation(40)], 1)
    ref = cases.ransac_reference(pts, (0, 40), corr, 512, seed=SEED)
    check_pair("all outliers", run(dev, pts, [(0, 40)], [corr], 512), 0, ref, 512, pose=False)
    # repeated points: correspondences 0 and 1 are the same pair of points, as are 2 and 3
    k = cases.planted_case(8, seed=5, outliers=0.0)
    corr = k["corr"].copy()
    corr[1], corr[3] = corr[0], corr[2]
    ref = cases.ransac_reference(k["pts"], k["pair"], corr, 512, seed=SEED)
    assert (ref["counts"] == -1).sum() > 20                                                      # triples holding a point twice
    check_pair("repeated", run(dev, k["pts"], [k["pair"]], [corr], 512), 0, ref, 512)
    # M = 3, exactly collinear: every hypothesis degenerate -> R = 1, t = cT - cS, finite outputs
    line = np.outer(np.arange(3.0), [0.25, -0.5, 0.125]).astype(np.float32)
    pts = np.concatenate([line + np.float32(0.125), line[::-1] * np.float32(2) - np.float32(0.5)])
    corr = np.stack([np.arange(3)] * 2, 1)
    got = run(dev, pts, [(0, 3)], [corr], 300, refine=True)
    ref = cases.ransac_reference(pts, (0, 3), corr, 300, seed=SEED)
    print("collinear: status", got["status"][0], "t", got["t"][0], "restatement", ref["t"])
    assert ref["status"] == 0 and got["status"][0] == 0 and got["best_h"][0] == -1 and got["count"][0] == -1
    assert (got["counts"] == -1).all() and got["sumsq"][0] == 0
    assert np.array_equal(got["R"][0], np.eye(3, dtype=np.float32)) and np.isfinite(got["t"]).all()
    assert np.abs(got["t"][0] - ref["t"]).max() <= U24 * max(np.abs(ref["t"]).max(), 1.0)


@pytest.mark.parametrize("M", [65, 300])
def test_refinement_over_the_winners_inliers(dev, M):
    k = cases.planted_case(M, seed=CASE_SEED + 1, pad=4)
    rng = np.random.default_rng([M, 77])
    pts = k["pts"].copy()
    t0 = k["pair"][1]
    pts[t0:t0 + M] += (0.004 * rng.normal(size=(M, 3))).astype(np.float32)                       # measurement noise on the targets
    ref = cases.ransac_reference(pts, k["pair"], k["corr"], H_MAX, seed=SEED)
    plain = run(dev, pts, [k["pair"]], [k["corr"]], H_MAX)
    got = run(dev, pts, [k["pair"]], [k["corr"]], H_MAX, refine=True)
    check_pair(f"M={M} unrefined", plain, 0, ref, H_MAX)
    h = int(got["best_h"][0])
    assert h == plain["best_h"][0] and got["count"][0] == plain["count"][0] and got["sumsq"][0] == plain["sumsq"][0]
    assert not ref["aside"][h]                                                                   # the inlier set is the same on both sides
    want = cases.refine_pose(ref["S"], ref["T"], ref["R64"][h], ref["t64"][h])
    print(f"M={M}: winner h={h} count={got['count'][0]}, refined over {got['n_refined'][0]:.0f} (restatement {want['n_refined']}), status {got['status'][0]}")
    assert want["status"] == 3 and got["status"][0] == 3 and got["n_refined"][0] == want["n_refined"] == got["count"][0]
    check_pose(got["R"][0], got["t"][0], want["R"], want["t"])
    # against the planted pose: the restatement's own deviation is what the data allow
    for name, g, w, p in (("R", got["R"][0], want["R"], k["R0"]), ("t", got["t"][0], want["t"], k["t0"])):
        own, mine, before = np.abs(w - p).max(), np.abs(g - p).max(), np.abs(plain[name][0] - p).max()
        print(f"    {name}: |refined - planted| {mine:.3e}, restatement {own:.3e} (bar {max(4 * own, 4 * U24):.3e}); three-point pose {before:.3e}")
        assert mine <= max(4 * own, 4 * U24)


def test_ragged_nearest_distance(dev):
    from pfpp_hip import ops
    from pfpp_hip.matching_eval import nn_dist_ragged

    rng = np.random.default_rng(31)
    ns, nd = [0, 1, 63, 64, 65, 1000, 3, 1030], [7, 1000, 1, 65, 64, 63, 0, 2049]
    so, do = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(nd)])
    src, dst = rng.normal(size=(so[-1], 3)).astype(np.float32), rng.normal(size=(do[-1], 3)).astype(np.float32)
    s_d, d_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    got = nn_dist_ragged(s_d, so, d_d, do).cpu().numpy()
    worst = 0.0
    for s in range(len(ns)):
        a, b, g = src[so[s]:so[s + 1]], dst[do[s]:do[s + 1]], got[so[s]:so[s + 1]]
        if nd[s] == 0:
            assert np.isinf(g).all() and (g > 0).all()
            continue
        if ns[s] == 0:
            continue
        d = a[:, None, :] - b[None, :, :]
        want32 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(1)
        assert want32.dtype == np.float32 and np.array_equal(g, want32), s
        want64 = ((a[:, None, :].astype(np.float64) - b[None].astype(np.float64)) ** 2).sum(-1).min(1)
        worst = max(worst, float((np.abs(g - want64) / want64).max()))
        assert (np.abs(g - want64) <= 6 * U24 * want64).all(), s
        dense = ops.nn_dist(s_d[so[s]:so[s + 1]][None], d_d[do[s]:do[s + 1]][None])[0].cpu().numpy()
        assert np.array_equal(g, dense), s
    print(f"ragged nearest distance: worst relative deviation from float64 {worst:.2e} (bar {6 * U24:.2e})")
    assert np.array_equal(got, nn_dist_ragged(s_d, so, d_d, do).cpu().numpy())
    # a dense batch as segments of equal sizes
    B, n, m = 3, 257, 1025
    s, d = torch.randn(B, n, 3, device=dev), torch.randn(B, m, 3, device=dev)
    rag = nn_dist_ragged(s.reshape(-1, 3), np.arange(B + 1) * n, d.reshape(-1, 3), np.arange(B + 1) * m)
    assert torch.equal(rag.reshape(B, n), ops.nn_dist(s, d))
    # rows outside every segment are left alone (zero), an empty call launches nothing
    part = nn_dist_ragged(s_d, [5, 9], d_d, [0, 7]).cpu().numpy()
    assert (part[:5] == 0).all() and (part[9:] == 0).all() and (part[5:9] > 0).all()
    assert nn_dist_ragged(s_d[:0], [0], d_d, [0]).numel() == 0


# ------------------------------------------------------------------------------------------------------------------ end to end
# Bars: pred_dict against the restatement FED THE GPU's edge poses is host float64 on both sides: 1e-12.  The metrics against the
# restatement's own values (float64 RANSAC poses, float64 metrics): 4 x its value, with a floor from fp32 rounding: an edge pose is
# rounded once to fp32 (2^-24 on entries below 1), a piece is up to four edges from vertex 0 and one more product from the pivot, and
# the metrics themselves are formed in fp32: 16 x 2^-24 on a translation component, 16 x 2^-24 rad = 5.5e-5 degrees on an Euler angle
# plus the fp32 angle's own 2^-24 x 180; the mse floors are the squares.
E2E_HYP = 512
TRANS_FLOOR = 16 * U24
ROT_FLOOR = 16 * U24 * 180 / np.pi + U24 * 180
FIVE = dict(sizes=[200, 210, 190, 205, 195], links=[(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)])


def evaluate(dev, data, **kw):
    from pfpp_hip.matching_eval import MatchingEvaluator

    ev = MatchingEvaluator(n_hyp=E2E_HYP, seed=SEED, **kw)
    dd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in data.items() if k != "perm_mat"}
    metric = ev.transformation_metrics(dd, {"perm_mat": data["perm_mat"]})
    return ev, metric


def restatement(data, ev):
    """(the restatement on its own float64 RANSAC poses, the restatement fed the GPU's edge poses)"""
    from pfpp_hip import matching_eval as me

    base = np.concatenate([[0], np.cumsum([g["n_ransac"] for g in ev.graphs])])

    def own(b, k, idx1, idx2, src, tgt, corr):
        r = cases.ransac_reference(np.concatenate([src, tgt]).astype(np.float32), (0, len(src)), corr, E2E_HYP, e=int(base[b]) + k, seed=SEED)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = r["R"], r["t"]
        return T

    fed = lambda b, k, *a: ev.graphs[b]["transformations"][k]
    return cases.global_transformation_reference(data, own, me.global_alignment), cases.global_transformation_reference(data, fed, me.global_alignment)


def check_end_to_end(tag, data, ev, metric, *, accurate=True, chamfer=True):
    own, fed = restatement(data, ev)
    for b, g in enumerate(ev.graphs):
        assert np.array_equal(g["edges"], fed["graphs"][b]["edges"]) and g["n_ransac"] == fed["graphs"][b]["n_ransac"]
        assert np.array_equal(g["uncertainty"], fed["graphs"][b]["uncertainty"])
        assert np.abs(g["transformations"] - fed["graphs"][b]["transformations"]).max(initial=0) <= 1e-12
    dr, dt = np.abs(metric["pred_dict"]["rot"] - fed["rot"]).max(), np.abs(metric["pred_dict"]["trans"] - fed["trans"]).max()
    print(f"{tag}: pivots {ev.pivots}, pred_dict against the restatement fed the GPU's edge poses: rot {dr:.1e}, trans {dt:.1e}")
    assert ev.pivots == fed["pivots"] and dr <= 1e-12 and dt <= 1e-12
    want = cases.pose_metrics_reference(data, own)
    for key in ("trans_mse", "trans_rmse", "trans_mae", "rot_mse", "rot_rmse", "rot_mae"):
        floor = (TRANS_FLOOR if key.startswith("trans") else ROT_FLOOR) ** (2 if key.endswith("_mse") else 1)
        print(f"    {key}: {float(metric[key]):.3e}, restatement {want[key]:.3e} (bar {max(4 * want[key], floor):.3e})")
        if accurate:
            assert float(metric[key]) <= max(4 * want[key], floor)
    print(f"    part_acc {float(metric['part_acc'])}, chamfer_distance {float(metric['chamfer_distance']):.3e}")
    if accurate:
        assert float(metric["part_acc"]) == 1.0 and (not chamfer or float(metric["chamfer_distance"]) < 1e-6)


def test_end_to_end_five_pieces(dev):
    data = cases.make_puzzle(seed=61, **FIVE)
    ev, metric = evaluate(dev, data)
    assert set(ev.KEYS) <= set(metric) and len(ev.graphs[0]["edges"]) == ev.graphs[0]["n_ransac"] == 5
    assert (ev.graphs[0]["ransac"]["count"] == 12).all()
    check_end_to_end("five pieces", data, ev, metric)
    assert all(len(v) == 1 for v in ev.stats.values()) and ev.stats["pred_rot"][0].shape == (1, 5, 3, 3)
    again, metric2 = evaluate(dev, data)
    assert np.array_equal(metric["pred_dict"]["rot"], metric2["pred_dict"]["rot"]) and all(torch.equal(metric[k], metric2[k]) for k in ev.KEYS)


def test_end_to_end_piece_with_two_matches_takes_the_translation_only_edge(dev):
    data = cases.make_puzzle(seed=61, sizes=FIVE["sizes"], links=[(0, 1), (1, 2), (2, 3), (3, 4)], cut=(3, 4, 2))
    ev, metric = evaluate(dev, data)
    g = ev.graphs[0]
    assert g["n_ransac"] == 3 and len(g["edges"]) == 4 and g["uncertainty"][3] == 1 and np.array_equal(g["transformations"][3, :3, :3], np.eye(3))
    check_end_to_end("cut to two matches", data, ev, metric, accurate=False)         # piece 4 is placed by a translation alone


def test_end_to_end_two_pieces_and_no_match_at_all(dev):
    data = cases.make_puzzle(seed=61, sizes=[200, 210], links=[(0, 1)])
    ev, metric = evaluate(dev, data)
    assert ev.graphs[0]["n_ransac"] == 1
    check_end_to_end("two pieces", data, ev, metric)
    data = cases.make_puzzle(seed=61, sizes=[200, 210, 190], links=[(0, 1), (1, 2)])
    data["perm_mat"] = [np.zeros_like(data["perm_mat"][0])]
    ev, metric = evaluate(dev, data)
    assert len(ev.graphs[0]["edges"]) == 0 and ev.pivots == [0]
    check_end_to_end("no match", data, ev, metric, accurate=False)
    R0 = cases.quat_rmat(data["part_quat"][0, 0])
    assert np.allclose(metric["pred_dict"]["rot"][0], R0) and np.allclose(metric["pred_dict"]["trans"][0], data["part_trans"][0, 0].astype(np.float64))


def test_end_to_end_two_layouts_in_one_batch_and_the_shape_cd_keyword(dev):
    data = cases.stack_puzzles([cases.make_puzzle(seed=61, **FIVE), cases.make_puzzle(seed=62, sizes=[250, 250, 300, 200], links=[(0, 1), (1, 2), (2, 3)])])
    ev, metric = evaluate(dev, data)
    check_end_to_end("two layouts", data, ev, metric, chamfer=False)          # the whole-shape term is the keyword's subject, below
    fixed, metric_fixed = evaluate(dev, data, shape_cd_index="corrected")
    ref_cd, fix_cd = ev.stats["chamfer_distance"][0], fixed.stats["chamfer_distance"][0]
    print("shape chamfer, reference indexing", ref_cd, "corrected", fix_cd)
    assert ref_cd[0] == fix_cd[0]                      # puzzle 0 is indexed by its own layout either way
    assert fix_cd[1] < 1e-6 < ref_cd[1]                # puzzle 1 is read at puzzle 0's offsets (eval_utils.py:141) unless corrected
    assert np.array_equal(metric["pred_dict"]["rot"], metric_fixed["pred_dict"]["rot"]) and torch.equal(metric["part_acc"], metric_fixed["part_acc"])
    alone, metric_alone = evaluate(dev, cases.make_puzzle(seed=61, **FIVE))
    assert np.array_equal(metric_alone["pred_dict"]["rot"][0], metric["pred_dict"]["rot"][0])          # a puzzle's poses do not depend on the batch


def test_evaluate_matching_command_line(dev, tmp_path, capsys):
    """the script over a directory of descriptor files with a seeded head: it runs the head, the evaluator and prints one JSON line;
    the line is reproducible and its numbers are the evaluator's own for the same head output"""
    import json

    from pfpp_hip import evaluate_matching as cli

    spec = importlib.util.spec_from_file_location("matching_cases", Path(__file__).resolve().parent / "matching_cases.py")
    mc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mc)
    feats = tmp_path / "features"
    feats.mkdir()
    torch.save({"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in mc.head_state_dict().items()}}, tmp_path / "jigsaw.ckpt")
    names = list(mc.DATA_ID)[:3]
    for name in names:
        pz = mc.make_puzzle(name)
        P = pz["n_pcs"].shape[0]
        quat = np.zeros((P, 4), dtype=np.float32)
        quat[:, 0] = 1
        np.savez(feats / f"{pz['data_id']}.npz", part_feats=pz["part_feats"], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"],
                 part_pcs=pz["gt_pcs"], part_quat=quat, part_trans=np.zeros((P, 3), dtype=np.float32))
    argv = ["--features", str(feats), "--checkpoint", str(tmp_path / "jigsaw.ckpt"), "--n-hyp", "256", "--seed", "5", "--batch-size", "2"]
    assert cli.main(argv) == 0
    first = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(first)
    assert first["puzzles"] == len(names) and first["n_hyp"] == 256 and first["seed"] == 5 and first["refine"] is False
    for key in ("part_acc", "chamfer_distance", "trans_mse", "trans_rmse", "trans_mae", "rot_mse", "rot_rmse", "rot_mae"):
        assert np.isfinite(first[key]) and first[key] >= 0
    assert 0 <= first["part_acc"] <= 1
    assert cli.main(argv) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == first
