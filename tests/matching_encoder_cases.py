"""Seeded inputs of the matcher's ragged PointNet++ encoder tests (no test in here): weights under the reference's parameter names
(PointNet2PTMSGDynamic, Jigsaw_matching/model/modules/encoder/pointnet2_pointwise/pointnet2_msg.py:48-66), the puzzles (points and
piece lengths) and the per-level start indices of the farthest-point sampling.  tools/make_matching_encoder_goldens.py feeds exactly
these arrays to the reference's module and stores what it returns in tests/golden/matching_encoder.npz; the tests regenerate them
from the same seeds, so the fixture holds results only (the 1.9 M parameters never reach a file).  numpy only: the golden tool runs
in a process that must not import the product.

Also here, because the tool and the tests both need them: the float32 sample-count rule of torch_cluster.fps and the float64
restatement of the k nearest neighbours of a piece."""
from __future__ import annotations

import numpy as np

RATIOS = (0.15, 0.25, 0.25, 0.25)
NSAMPLE = (16, 32)
FEAT_IN, FEAT_OUT = 3, 128
# (name, input channels, MLP widths of the two scales)
SA = (("sa1", FEAT_IN, ((16, 16, 32), (32, 32, 64))), ("sa2", 96, ((64, 64, 128), (64, 96, 128))),
      ("sa3", 256, ((128, 196, 256), (128, 196, 256))), ("sa4", 512, ((256, 256, 512), (256, 384, 512))))
# (name, input channels, MLP widths)
FP = (("fp4", 1536, (256, 256)), ("fp3", 512, (256, 256)), ("fp2", 352, (256, 128)), ("fp1", 128, (128, 128, 128)))

# name -> list of puzzles, each a list of piece lengths
CASES = {
    # wave-boundary sizes 64 / 65; n = 200 samples 31 (float32), not 30; the 30-point piece shrinks 30 -> 5 -> 2 -> 1 -> 1
    "small": [[30, 33, 64, 65, 200, 417]],
    # the largest piece the configuration allows next to the smallest: 746 samples at level 1
    "two": [[4970, 30]],
    # n = 100 -> 16, 20 -> 3, 340 -> 52 in float32 (15, 5, 51 in exact arithmetic order: see sample_count)
    "second": [[100, 20, 340]],
    "batch": [[30, 33, 64, 65, 200, 417], [100, 20, 340]],
}
PUZZLE_SEED = {(30, 33, 64, 65, 200, 417): 101, (4970, 30): 102, (100, 20, 340): 103}
MIN_DIST = 1e-3


def sample_count(n, ratio: float):
    """torch_cluster.fps: ceil(ratio * n) evaluated in float32 (the ratio tensor has the points' dtype).  n = 100, ratio 0.15 -> 16"""
    return np.ceil(np.float32(ratio) * np.asarray(n).astype(np.float32)).astype(np.int64)


def level_counts(lengths) -> np.ndarray:
    """int64 [5, P]: the piece lengths at the input and behind each of the four set-abstraction levels"""
    out = [np.asarray(lengths, dtype=np.int64)]
    for r in RATIOS:
        out.append(sample_count(out[-1], r))
    return np.stack(out)


def state_dict_spec() -> list:
    """[(name, shape)] of PointNet2PTMSGDynamic(3, 128).state_dict() in the reference's order"""
    spec = []

    def bn(prefix, c):
        return [(f"{prefix}.weight", (c,)), (f"{prefix}.bias", (c,)), (f"{prefix}.running_mean", (c,)), (f"{prefix}.running_var", (c,)),
                (f"{prefix}.num_batches_tracked", ())]

    for name, cin, scales in SA:
        convs, bns = [], []
        for i, widths in enumerate(scales):
            last = cin + 3
            for j, c in enumerate(widths):
                convs += [(f"{name}.conv_blocks.{i}.{j}.weight", (c, last, 1, 1)), (f"{name}.conv_blocks.{i}.{j}.bias", (c,))]
                bns += bn(f"{name}.bn_blocks.{i}.{j}", c)
                last = c
        spec += convs + bns
    for name, cin, widths in FP:
        convs, bns = [], []
        last = cin
        for j, c in enumerate(widths):
            convs += [(f"{name}.mlp_convs.{j}.weight", (c, last, 1)), (f"{name}.mlp_convs.{j}.bias", (c,))]
            bns += bn(f"{name}.mlp_bns.{j}", c)
            last = c
        spec += convs + bns
    spec += [("conv1.weight", (FEAT_OUT, 128, 1)), ("conv1.bias", (FEAT_OUT,))]
    return spec


def encoder_state_dict(seed: int = 11) -> dict:
    """float32 arrays (int64 for num_batches_tracked) under the reference's names.  Convolutions are He-scaled so that activations
    keep their magnitude through the levels; BatchNorm running statistics and affine terms are non-trivial."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in state_dict_spec():
        leaf = name.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            sd[name] = np.asarray(0, dtype=np.int64)
        elif leaf == "running_mean":
            sd[name] = rng.normal(0, 0.1, shape).astype(np.float32)
        elif leaf == "running_var":
            sd[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif "bn" in name and leaf == "weight":
            sd[name] = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif "bn" in name and leaf == "bias":
            sd[name] = rng.normal(0.1, 0.1, shape).astype(np.float32)
        elif leaf == "weight":
            fan_in = shape[1]
            sd[name] = rng.normal(0, np.sqrt(2.0 / fan_in), shape).astype(np.float32)
        else:
            sd[name] = rng.normal(0, 0.05, shape).astype(np.float32)
    return sd


def min_pairwise_distance(pts: np.ndarray) -> float:
    """smallest distance between two points of one piece (float64 of the float32 coordinates), in row blocks"""
    p = pts.astype(np.float64)
    best = np.inf
    for i in range(0, len(p), 512):
        d = ((p[i:i + 512, None, :] - p[None, :, :]) ** 2).sum(-1)
        d[np.arange(min(512, len(p) - i)), np.arange(i, min(i + 512, len(p)))] = np.inf
        best = min(best, float(d.min()))
    return float(np.sqrt(best))


def _patch(rng, n: int) -> np.ndarray:
    """n points on a perturbed patch of a sphere of radius 0.4, in random order, no two closer than MIN_DIST"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    u = np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(axis, u)

    def draw(k):
        theta = 0.8 * np.sqrt(rng.uniform(0, 1, k))
        phi = rng.uniform(0, 2 * np.pi, k)
        r = 0.4 * (1 + 0.05 * rng.normal(size=k))
        d = np.cos(theta)[:, None] * axis + np.sin(theta)[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)
        return (r[:, None] * d).astype(np.float32)

    pts = draw(n)
    for _ in range(100):
        p = pts.astype(np.float64)
        bad = np.zeros(n, dtype=bool)
        for i in range(0, n, 512):
            d = ((p[i:i + 512, None, :] - p[None, :, :]) ** 2).sum(-1)
            d[np.arange(min(512, n - i)), np.arange(i, min(i + 512, n))] = np.inf
            bad[i:i + 512] = d.min(1) < (1.5 * MIN_DIST) ** 2
        if not bad.any():
            break
        pts[bad] = draw(int(bad.sum()))
    return pts


_PUZZLES = {}


def make_puzzle(lengths) -> dict:
    """-> points float32 [N, 3], lengths int64 [P], start int64 [4, P] (local first index of each level's sampling: non-zero
    wherever the level has more than one point to choose from)"""
    key = tuple(int(n) for n in lengths)
    if key in _PUZZLES:
        return _PUZZLES[key]
    rng = np.random.default_rng([23, PUZZLE_SEED[key]])
    pts = [_patch(rng, n) for n in key]
    for p in pts:
        assert min_pairwise_distance(p) >= MIN_DIST, "two points of a piece closer than 1e-3"
    counts = level_counts(key)
    start = np.stack([np.where(counts[l] > 1, rng.integers(1, np.maximum(counts[l], 2)), 0) for l in range(4)]).astype(np.int64)
    assert (start < counts[:4]).all()
    _PUZZLES[key] = {"points": np.concatenate(pts), "lengths": np.asarray(key, dtype=np.int64), "start": start}
    return _PUZZLES[key]


def make_case(name: str) -> list:
    return [make_puzzle(lengths) for lengths in CASES[name]]


def knn_f64(points: np.ndarray, queries: np.ndarray, K: int):
    """float64 restatement of the neighbours of one piece: for every query the min(K, n) nearest points, ascending by
    (dx dx + dy dy) + dz dz, lower index first on ties -> (idx int64 [M, min(K, n)], gap float64 [M]: the relative distance
    (d_(K+1) - d_K) / d_(K+1) between the last neighbour kept and the first one left out; inf when nothing is left out)"""
    p, q = points.astype(np.float64), queries.astype(np.float64)
    d = q[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.argsort(d2, axis=1, kind="stable")
    k = min(K, p.shape[0])
    gap = np.full(q.shape[0], np.inf)
    if p.shape[0] > k:
        srt = np.take_along_axis(d2, order[:, :k + 1], 1)
        gap = (srt[:, k] - srt[:, k - 1]) / np.maximum(srt[:, k], 1e-300)
    return order[:, :k], gap


def fps_f64_margin(points: np.ndarray, chain: np.ndarray) -> float:
    """smallest relative gap between the top two running minima along a sampling chain, in float64 (how close the chain ever came
    to forking)"""
    p = points.astype(np.float64)
    dist = np.full(len(p), np.inf)
    worst = np.inf
    for s in range(len(chain) - 1):
        d = p - p[chain[s]]
        dist = np.minimum(dist, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        if len(p) > 1:
            top = np.partition(dist, -2)[-2:]
            if top[1] > 0:
                worst = min(worst, (top[1] - top[0]) / top[1])
    return float(worst)
