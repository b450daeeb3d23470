"""GPU: the matcher's ragged PointNet++ encoder (csrc/pointnet_ragged.hip, pfpp_hip/matching_encoder.py) against (a)
tests/golden/matching_encoder.npz, written by tools/make_matching_encoder_goldens.py from the reference's own module, (b)
oracle.fps_start and (c) the float64 / float32 restatements of tests/matching_encoder_cases.py and below.  Inputs are regenerated
from the case file.  Every test prints the figures it measured before it asserts.

Bars.  Discrete results (sampling chains, neighbour sets, counts, padded slots) are compared exactly; a neighbour
set that differs from the float64 restatement is excused only when float64's own gap between the last neighbour kept and the
first left out is below 4 ulp (4 x 2^-23, relative), for at most 0.5 % of a level's queries; no sampling chain is excused.
The interpolation weights repeat the reference's fp32 operations in its order and are compared bitwise with their float32
restatement, and within max(4 x reference deviation, 4 x 2^-23) with the fixture's per-centroid sums.  Features: the fixture
records, per tensor, the deviation of the reference's own fp32 run from its float64 run relative to the tensor's largest magnitude;
the bar is 4 x that for the exact-fp32 products (same operations, another summation order) and 16 x for split-f16 (22 instead of 24
bits per operand), the multiples DESIGN.md 5.4 uses.

The reference's own deviation on the fixture is 1.8e-7 .. 1.5e-6 of a tensor's maximum; the measured values are in DESIGN.md 5.5."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MULT = {"f32": 4.0, "f16x3": 16.0}
ULP4 = 4.0 * 2.0 ** -23
MAX_EXCUSED = 0.005
SA_WIDTH = {1: 96, 2: 256, 3: 512, 4: 1024}
FP_LEVELS = (("fp4", 3, 512), ("fp3", 2, 256), ("fp2", 1, 96), ("fp1", 0, 0))       # name, fine level, width of points1


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_encoder_cases", ROOT / "tests" / "matching_encoder_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_RUNS = {}
_ENC = {}


def encoder(dev, mode):
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    if mode not in _ENC:
        enc = PointNet2PTMSGDynamic(3, 128, gemm_mode=mode)
        enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.encoder_state_dict().items()}, strict=True)
        _ENC[mode] = enc.to(dev)
    return _ENC[mode]


def case_inputs(name):
    pzs = cases.make_case(name)
    return (np.concatenate([pz["points"] for pz in pzs]), np.concatenate([pz["lengths"] for pz in pzs]),
            np.concatenate([pz["start"] for pz in pzs], 1))


def run(dev, name, mode="f32"):
    """one forward per (case, mode), shared by the tests and left unchanged: (descriptors, levels) on the host"""
    if (name, mode) not in _RUNS:
        pts, lengths, start = case_inputs(name)
        y, lv = encoder(dev, mode)(torch.from_numpy(pts).to(dev), lengths, start=start.T, return_levels=True)
        torch.cuda.synchronize()
        _RUNS[(name, mode)] = (y.cpu().numpy(), {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in lv.items()})
    return _RUNS[(name, mode)]


def level_geometry(name, lv):
    """per level 0..4: (xyz float32 [N_l, 3], CSR offsets)"""
    pts, lengths, _ = case_inputs(name)
    counts = cases.level_counts(lengths)
    off = np.concatenate([np.zeros((5, 1), np.int64), np.cumsum(counts, 1)], 1)
    return [pts] + [lv[f"l{l}_xyz"] for l in range(1, 5)], off, counts


# ------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("name", ["small", "two", "batch"])
def test_ragged_fps_equals_the_oracle_per_piece(dev, hip_lib, golden, name):
    from oracle import pfpp_oracle as O

    _, lv = run(dev, name)
    xyz, off, counts = level_geometry(name, lv)
    _, lengths, start = case_inputs(name)
    assert np.array_equal(lv["counts"], counts)
    assert np.array_equal(counts[1], np.ceil(np.float32(0.15) * lengths.astype(np.float32)).astype(np.int64))
    bad, chains, margin = 0, 0, np.inf
    for l in range(4):
        cen = lv[f"l{l + 1}_centroids"]
        assert cen.shape == (off[l + 1, -1],)
        for p in range(len(lengths)):
            src = xyz[l][off[l, p]:off[l, p + 1]]
            want = O.fps_start(torch.from_numpy(src), int(counts[l + 1, p]), int(start[l, p])).numpy() + off[l, p]
            got = cen[off[l + 1, p]:off[l + 1, p + 1]]
            bad += int(not np.array_equal(got, want))
            chains += 1
            margin = min(margin, cases.fps_f64_margin(src, want - off[l, p]))
        assert np.array_equal(lv[f"l{l + 1}_xyz"], xyz[l][cen]), "new_xyz is not the sampled points"
    print(f"{name}: {chains} sampling chains, {bad} differ from oracle.fps_start; smallest float64 gap of the top two running minima {margin:.3g}")
    assert bad == 0
    if name in ("small",):
        g = golden("matching_encoder")
        for l in range(4):
            assert np.array_equal(lv[f"l{l + 1}_centroids"], g[f"{name}_l{l + 1}_centroids"].astype(np.int64))


def test_largest_piece_dimensions(dev, hip_lib):
    _, lv = run(dev, "two")
    assert lv["counts"][:, 0].tolist() == [4970, 746, 187, 47, 12]


# ------------------------------------------------------------------------------------------------ neighbours
def check_knn(xyz_p, off_p, xyz_q, off_q, idx, cnt, K, label):
    """idx int [M, K] (global) against the float64 restatement per piece; returns (queries, mismatching, excused)"""
    M = xyz_q.shape[0]
    assert idx.shape == (M, K)
    total = mism = excused = 0
    for p in range(len(off_p) - 1):
        a, b, qa, qb = off_p[p], off_p[p + 1], off_q[p], off_q[p + 1]
        n, real = b - a, min(K, b - a)
        want, gap = cases.knn_f64(xyz_p[a:b], xyz_q[qa:qb], K)
        got = idx[qa:qb].astype(np.int64) - a
        assert ((got >= 0) & (got < n)).all(), f"{label}: an index outside the query's piece"
        assert (got[:, real:] == got[:, :1]).all(), f"{label}: padded slots must repeat the first index"
        if cnt is not None:
            assert (cnt[qa:qb] == real).all(), f"{label}: real-neighbour count"
        # ascending by the fp32 distance, lower index first on ties; no index twice
        q32, p32 = xyz_q[qa:qb], xyz_p[a:b]
        d = p32[got[:, :real]] - q32[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert (np.diff(d2, axis=1) >= 0).all(), f"{label}: not ascending"
        tie = np.diff(d2, axis=1) == 0
        assert (np.diff(got[:, :real], axis=1)[tie] > 0).all(), f"{label}: a tie not broken towards the lower index"
        assert (np.diff(np.sort(got[:, :real], axis=1), axis=1) > 0).all(), f"{label}: an index twice"
        diff = (np.sort(got[:, :real], axis=1) != np.sort(want, axis=1)).any(1)
        assert not (diff & ~(gap < ULP4)).any(), f"{label}: a neighbour set differs from float64 although its boundary gap is {gap[diff].max():.3g}"
        total, mism, excused = total + (qb - qa), mism + int(diff.sum()), excused + int((diff & (gap < ULP4)).sum())
    return total, mism, excused


@pytest.mark.parametrize("name", ["small", "two", "batch"])
def test_ragged_knn_equals_the_float64_restatement(dev, hip_lib, golden, name):
    _, lv = run(dev, name)
    xyz, off, counts = level_geometry(name, lv)
    for l in range(4):
        idx = lv[f"l{l + 1}_knn"]
        for K in (16, 32):            # the encoder takes the K = 16 neighbourhood as the head of the K = 32 one
            sub = np.ascontiguousarray(idx[:, :K])       # (a piece with fewer than 16 points pads columns n .. 31 alike)
            total, mism, exc = check_knn(xyz[l], off[l], xyz[l + 1], off[l + 1], sub, None, K, f"{name} sa{l + 1} K={K}")
            print(f"{name} level {l + 1} K = {K}: {total} queries, {mism} sets differ from float64, {exc} excused (gap < 4 ulp)")
            assert exc <= MAX_EXCUSED * total
        if f"fp{l + 1}_idx" in lv and lv[f"fp{l + 1}_idx"] is not None:
            total, mism, exc = check_knn(xyz[l + 1], off[l + 1], xyz[l], off[l], lv[f"fp{l + 1}_idx"], lv[f"fp{l + 1}_cnt"], 3, f"{name} fp{l + 1}")
            print(f"{name} propagation {l + 1} K = 3: {total} queries, {mism} sets differ from float64, {exc} excused")
            assert exc <= MAX_EXCUSED * total
    if name == "small":
        g = golden("matching_encoder")
        for l in range(4):
            idx = lv[f"l{l + 1}_knn"].astype(np.int64)
            for K in (16, 32):
                rows = np.sort(idx[:, :K], axis=1)
                want = g[f"{name}_l{l + 1}_knn{K}"].astype(np.int64)
                diff = (rows != want).any(1)
                print(f"{name} level {l + 1} K = {K}: {int(diff.sum())} of {len(rows)} sorted rows differ from the fixture")
                assert not diff.any()      # the float64 comparison above excused nothing on this case, so nothing may differ here


def test_knn_direct_call_counts_and_padding_for_every_k(dev, hip_lib):
    """the kernel on its own for K = 3 / 16 / 32 with pieces smaller than K, equal to K and across the 64 / 65 wave boundary"""
    from pfpp_hip.matching_encoder import ragged_knn

    pz = cases.make_case("small")[0]
    pts, lengths = pz["points"], pz["lengths"]
    off = np.concatenate([[0], np.cumsum(lengths)])
    qoff = np.concatenate([[0], np.cumsum(np.minimum(lengths, 7))])
    qry = np.concatenate([pts[a:a + 7] + np.float32(0.01) for a in off[:-1]])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for K in (3, 16, 32):
        idx, cnt = ragged_knn(t(pts), t(off), t(qry), t(qoff), K, want_count=True)
        total, mism, exc = check_knn(pts, off, qry, qoff, idx.cpu().numpy(), cnt.cpu().numpy(), K, f"direct K={K}")
        print(f"direct K = {K}: {total} queries, {mism} differ, {exc} excused")
        assert exc <= MAX_EXCUSED * total


# ------------------------------------------------------------------------------------------------ interpolation
def weights_f32(xyz1, xyz2, idx, cnt):
    """the reference's weight arithmetic (pointnet2_dynamic_utils.py:199-210) operation by operation in float32"""
    a = xyz1[:, None, :].astype(np.float32)
    b = xyz2[idx].astype(np.float32)
    t = (a * a + b * b) - (np.float32(2) * a) * b
    d = (t[..., 0] + t[..., 1]) + t[..., 2]
    d = np.where(np.arange(3)[None, :] < cnt[:, None], d, np.float32(1e8)).astype(np.float32)
    r = np.float32(1) / (d + np.float32(1e-8))
    return (r / ((r[:, 0] + r[:, 1]) + r[:, 2])[:, None]).astype(np.float32), d


@pytest.mark.parametrize("name", ["small", "second"])
def test_interpolation_weights(dev, hip_lib, golden, name):
    g = golden("matching_encoder")
    _, lv = run(dev, name)
    xyz, off, counts = level_geometry(name, lv)
    for fp, l, _ in FP_LEVELS:
        idx, cnt, w = lv[f"{fp}_idx"].astype(np.int64), lv[f"{fp}_cnt"], lv[f"{fp}_w"]
        want, d = weights_f32(xyz[l], xyz[l + 1], idx, cnt)
        print(f"{name} {fp}: {len(w)} points, weights differ from the float32 restatement in {int((w != want).sum())} places; "
              f"smallest distance {d.min():.3g}, points on a centroid {int((d[:, 0] == 0).sum())}")
        assert np.array_equal(w, want)
        # against the reference: the weight each centroid carries (padded slots fall on the first centroid)
        S = xyz[l + 1].shape[0]
        dense = np.zeros((len(w), S), dtype=np.float32)
        for j in range(3):
            np.add.at(dense, (np.arange(len(w)), idx[:, j]), w[:, j])
        ref_idx, ref_w = g[f"{name}_{fp}_w_idx"].astype(np.int64), g[f"{name}_{fp}_w"]
        got = np.where(ref_idx >= 0, np.take_along_axis(dense, np.maximum(ref_idx, 0), 1), 0)
        bar = max(4 * float(g[f"{name}_{fp}_w_refdev"]), ULP4)
        err = float(np.abs(got - ref_w).max())
        print(f"{name} {fp}: per-centroid weights vs the reference {err:.3g} (bar {bar:.3g}); rows sum to {dense.sum(1).min():.7f} .. {dense.sum(1).max():.7f}")
        assert err <= bar
        assert (np.count_nonzero(dense, axis=1) == (ref_idx >= 0).sum(1)).all()


def test_a_fine_point_on_a_centroid_takes_that_centroids_features(dev, hip_lib):
    """level-1 centroids ARE input points: d == 0 exactly in the reference's form, r = 1 / 1e-8, and the centroid carries
    w0 = r0 / ((r0 + r1) + r2).  The propagated row then differs from the centroid's features by at most the weight left to the
    two others times the feature range, plus fp32 rounding."""
    _, lv = run(dev, "small")
    xyz, off, counts = level_geometry("small", lv)
    cen = lv["l1_centroids"]
    idx, cnt, w, rows, feats = lv["fp1_idx"][cen], lv["fp1_cnt"][cen], lv["fp1_w"][cen], lv["fp1_in"][cen], lv["fp2_out"]
    assert np.array_equal(idx[:, 0], np.arange(len(cen))), "the nearest centroid of a sampled point is itself"
    want, d = weights_f32(xyz[0][cen], xyz[1], idx.astype(np.int64), cnt)
    assert (d[:, 0] == 0).all() and np.array_equal(w, want)
    fmax = float(np.abs(feats).max())
    slack = (1.0 - w[:, 0].astype(np.float64)) * 2 * fmax + ULP4 * fmax
    err = np.abs(rows.astype(np.float64) - feats[idx[:, 0]]).max(1)
    print(f"{len(cen)} coincident points: w0 {w[:, 0].min():.7f} .. {w[:, 0].max():.7f}, row deviation {err.max():.3g} (largest allowance {slack.max():.3g})")
    assert (err <= slack).all()
    many = cnt == 3
    lone = (1.0 - w[:, 0]) < 2.0 ** -24
    print(f"{int(lone.sum())} of them keep the whole weight: their rows equal the centroid's to fp32 rounding ({err[lone].max() if lone.any() else 0:.3g})")
    assert many.any()


def test_a_piece_with_one_centroid_gets_the_padded_weights(dev, hip_lib, golden):
    """fp4 of `small`: every piece has one level-4 centroid while the call has six, so k = 3 finds one neighbour and the two
    other slots carry the first index and d = 1e8 (to_dense_batch's fill values)"""
    _, lv = run(dev, "small")
    xyz, off, counts = level_geometry("small", lv)
    assert counts[4].tolist() == [1] * 6 and xyz[4].shape[0] == 6
    idx, cnt, w = lv["fp4_idx"], lv["fp4_cnt"], lv["fp4_w"]
    piece = np.repeat(np.arange(6), counts[3])
    assert (cnt == 1).all() and (idx == piece[:, None]).all()
    want, d = weights_f32(xyz[3], xyz[4], idx.astype(np.int64), cnt)
    assert (d[:, 1:] == np.float32(1e8)).all() and np.array_equal(w, want)
    print(f"fp4 weights: first slot {w[:, 0].min():.9f} .. {w[:, 0].max():.9f}, padded slots {w[:, 1:].min():.3g} .. {w[:, 1:].max():.3g}")
    assert (w[:, 1:] > 0).all() and (w[:, 1:] < 1e-6).all()


def test_single_centroid_call_broadcasts(dev, hip_lib):
    """S == 1 for the whole call (:191-192): every fine point receives the one centroid's features unchanged"""
    from pfpp_hip.matching_encoder import ragged_interp

    g = torch.Generator().manual_seed(3)
    xyz1, xyz2 = torch.rand((70, 3), generator=g).to(dev), torch.rand((1, 3), generator=g).to(dev)
    p2, p1 = torch.randn((1, 64), generator=g).to(dev), torch.randn((70, 32), generator=g).to(dev)
    out, w = ragged_interp(xyz1, xyz2, None, None, p2, p1, want_weights=True)
    assert torch.equal(out[:, :32], p1) and torch.equal(out[:, 32:], p2.expand(70, 64))
    assert torch.equal(w, torch.tensor([1.0, 0.0, 0.0], device=dev).expand(70, 3))


# ------------------------------------------------------------------------------------------------ features
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ["small", "second"])
def test_every_level_and_the_descriptors_against_the_reference(dev, hip_lib, golden, name, mode):
    g = golden("matching_encoder")
    y, lv = run(dev, name, mode)
    stride, rstride = int(g["stride"]), int(g["row_stride"])
    got = {f"l{l}_points": lv[f"l{l}_points"] for l in range(1, 5)}
    for fp, _, d1 in FP_LEVELS:
        got[f"{fp}_interp"] = lv[f"{fp}_in"][:, d1:]
        got[f"{fp}_out"] = lv[f"{fp}_out"]
    worst = 0.0
    for key, a in got.items():
        want, dev_ref, amax = g[f"{name}_{key}"], float(g[f"{name}_{key}_refdev"]), float(g[f"{name}_{key}_max"])
        sample = np.ascontiguousarray(a).reshape(-1)[::stride]
        assert sample.shape == want.shape, key
        err, bar = float(np.abs(sample - want).max()) / amax, MULT[mode] * dev_ref
        worst = max(worst, err / bar)
        print(f"{name} {mode} {key}: {err:.3g} of the maximum {amax:.4g} (reference fp32 vs float64 {dev_ref:.3g}, bar {bar:.3g})")
        assert err <= bar, key
    want, dev_ref, amax = g[f"{name}_final"], float(g[f"{name}_final_refdev"]), float(g[f"{name}_final_max"])
    assert y.shape == (lv["counts"][0].sum(), 128) and np.isfinite(y).all()
    err, bar = float(np.abs(y[::rstride] - want).max()) / amax, MULT[mode] * dev_ref
    print(f"{name} {mode} descriptors: {err:.3g} of the maximum {amax:.4g} (reference {dev_ref:.3g}, bar {bar:.3g}); worst level at {worst:.2f} of its bar")
    assert err <= bar


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_a_batch_of_puzzles_equals_the_puzzles_alone_bitwise(dev, hip_lib, mode):
    yb, lb = run(dev, "batch", mode)
    ys, ls = run(dev, "small", mode)
    y2, l2 = run(dev, "second", mode)
    n = ys.shape[0]
    assert np.array_equal(yb[:n], ys) and np.array_equal(yb[n:], y2)
    for l in range(1, 5):
        s = ls[f"l{l}_points"].shape[0]
        assert np.array_equal(lb[f"l{l}_points"][:s], ls[f"l{l}_points"]) and np.array_equal(lb[f"l{l}_points"][s:], l2[f"l{l}_points"])
    # the helper: per-puzzle views of one call
    enc = encoder(dev, mode)
    pzs = cases.make_case("batch")
    start = np.concatenate([pz["start"] for pz in pzs], 1).T
    n_pcs = [np.concatenate([pz["lengths"], np.zeros(20 - len(pz["lengths"]), np.int64)]) for pz in pzs]
    outs = enc.encode_puzzles([(torch.from_numpy(pz["points"]).to(dev), n) for pz, n in zip(pzs, n_pcs)], start=start)
    assert len(outs) == 2 and np.array_equal(outs[0].cpu().numpy(), ys) and np.array_equal(outs[1].cpu().numpy(), y2)
    assert outs[0].untyped_storage().data_ptr() == outs[1].untyped_storage().data_ptr()


def test_two_runs_of_the_largest_case_agree_bitwise(dev, hip_lib):
    y1, l1 = run(dev, "two")
    pts, lengths, start = case_inputs("two")
    y2, l2 = encoder(dev, "f32")(torch.from_numpy(pts).to(dev), lengths, start=start.T, return_levels=True)
    assert np.isfinite(y1).all() and np.array_equal(y1, y2.cpu().numpy())
    for k in ("l1_centroids", "l4_centroids", "l1_knn", "l4_points", "fp1_w", "fp1_out"):
        assert np.array_equal(l1[k], l2[k].cpu().numpy()), k


def test_forward_sees_a_weight_change_and_seeded_starts_repeat(dev, hip_lib):
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.encoder_state_dict().items()}
    enc = PointNet2PTMSGDynamic().to(dev)
    enc.load_state_dict(sd, strict=True)
    pts, lengths, start = case_inputs("second")
    x = torch.from_numpy(pts).to(dev)
    y0 = enc(x, lengths, start=start.T)
    assert np.array_equal(y0.cpu().numpy(), run(dev, "second")[0])
    with torch.no_grad():
        enc.conv1.bias.add_(1.0)
    y1 = enc(x, lengths, start=start.T)
    assert float((y1 - y0 - 1.0).abs().max()) < 1e-5
    with torch.no_grad():
        enc.sa1.bn_blocks[0][0].running_var.mul_(4.0)          # a buffer inside the folded part
    y2 = enc(x, lengths, start=start.T)
    assert float((y2 - y1).abs().max()) > 1e-3
    enc.load_state_dict(sd, strict=True)
    assert torch.equal(enc(x, lengths, start=start.T), y0)
    # start=None: drawn on the device from a seeded generator
    a, la = enc(x, lengths, seed=5, return_levels=True)
    b, lb = enc(x, lengths, seed=5, return_levels=True)
    c, lc = enc(x, lengths, seed=6, return_levels=True)
    counts = cases.level_counts(lengths)
    assert torch.equal(a, b) and torch.equal(la["start"], lb["start"]) and not torch.equal(la["start"], lc["start"])
    assert (la["start"].cpu().numpy() < counts[:4]).all() and (la["start"] >= 0).all()
    with pytest.raises(ValueError, match="start"):
        enc(x, lengths, start=np.full((3, 4), 1000))
    with pytest.raises(ValueError, match="sums to"):
        enc(x, lengths[:-1])
