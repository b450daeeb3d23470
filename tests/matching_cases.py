"""Seeded inputs of the matcher back-end tests (no test in here): the head's weights under the reference's parameter names and
small puzzles whose descriptors are built so that matches exist.  tools/make_matching_goldens.py feeds exactly these arrays to the
reference's code and stores what it returns in tests/golden/matching_head.npz; the tests regenerate them from the same seeds, so the
fixture holds results only.  numpy only: the golden tool runs in a process that must not import the product.

Construction.  The affinity extractor sees h = relu(BatchNorm(x)).  With a signed pre-activation y = (zp, -zp, zd, -zd, flags) the
1 x 1 convolution recovers the 31-d latents zp (primal) and zd (dual) as differences and lifts both with one 256 x 31 matrix with
orthonormal columns, so primal_i . dual_j = zp_i . zd_j up to the small dense part of the weights.  A match i -> j (row i, column j of
the assignment) is zd_j = normalise(zp_i + 0.3 unit noise).  Every critical point has one partner as a row and one as a column
(symmetric pairs i <-> j, or 3-cycles i -> j -> k -> i over three pieces, which put their third leg into the block BELOW the
diagonal so that the transposed block wins for that pair), so the optimal assignment is determined by large entries only and does
not hinge on the last bits of the matrix.  Two flag channels drive the classifier far from its threshold."""
from __future__ import annotations

import numpy as np

P_MAX = 20
LATENT = 31
EPS = 1e-5

# name -> (points per piece, symmetric matches [(a, b, count)], 3-cycles [(a, b, c, count)] with a < b < c)
CASES = {
    # piece 4 has no critical point; (1, 3) has 2 matches per direction (dropped: fewer than 3); (0, 3) has 2 above and 2 + 6 below
    # the diagonal (the transposed block wins)
    "five": ([160, 140, 120, 100, 80], [(0, 1, 40), (1, 2, 25), (1, 3, 2), (0, 3, 2)], [(0, 2, 3, 6)]),
    "two": ([220, 180], [(0, 1, 60)], []),
    # all matches inside (0, 1) and (2, 3): the four other pairs have critical points on both sides and no match, so they reach the
    # `mat_s == 0` rule.  (All matches inside ONE pair is not possible with critical points elsewhere: the assignment is a full
    # permutation.)  The rule cannot be told apart from the `fewer than 3 non-zeros` rule behind it by any data: see the host test.
    "split": ([150, 130, 120, 100], [(0, 1, 35), (2, 3, 30)], []),
}
DATA_ID = {"five": 11, "two": 12, "split": 13}


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def head_state_dict(seed: int = 7) -> dict:
    """float32 arrays under the reference's names: pc_classifier.{0,2}.*, affinity_extractor.{0,2}.*, affinity_layer.A"""
    rng = np.random.default_rng(seed)
    C, D, H = 128, 512, 256
    bn_a = {"weight": rng.uniform(0.8, 1.2, C), "bias": rng.normal(0, 0.02, C), "running_mean": rng.normal(0, 0.1, C),
            "running_var": rng.uniform(0.5, 1.5, C)}
    bn_c = {"weight": bn_a["weight"] * (1 + 0.1 * rng.uniform(-1, 1, C)), "bias": bn_a["bias"] + 0.02 * rng.uniform(-1, 1, C),
            "running_mean": bn_a["running_mean"] + 0.02 * rng.uniform(-1, 1, C), "running_var": bn_a["running_var"] * (1 + 0.1 * rng.uniform(-1, 1, C))}
    lift, _ = np.linalg.qr(rng.normal(size=(H, LATENT)))
    w = 0.02 * rng.normal(size=(D, C))
    L = LATENT
    w[:H, 0:L] += lift; w[:H, L:2 * L] -= lift
    w[H:, 2 * L:3 * L] += lift; w[H:, 3 * L:4 * L] -= lift
    wc = 0.01 * rng.normal(size=C)
    wc[124], wc[125] = 3.0, -3.0
    stdv = 1.0 / np.sqrt(H)                                   # AffinityDual.reset_parameters: uniform(-stdv, stdv) + eye
    A = rng.uniform(-stdv, stdv, (H, H)) + np.eye(H)
    sd = {}
    for name, bn in (("pc_classifier", bn_c), ("affinity_extractor", bn_a)):
        for k, v in bn.items():
            sd[f"{name}.0.{k}"] = v.astype(np.float32)
        sd[f"{name}.0.num_batches_tracked"] = np.asarray(0, dtype=np.int64)
    sd["pc_classifier.2.weight"] = wc.astype(np.float32).reshape(1, C, 1)
    sd["pc_classifier.2.bias"] = np.asarray([0.05], dtype=np.float32)
    sd["affinity_extractor.2.weight"] = w.astype(np.float32).reshape(D, C, 1)
    sd["affinity_extractor.2.bias"] = (0.01 * rng.normal(size=D)).astype(np.float32)
    sd["affinity_layer.A"] = A.astype(np.float32)
    return sd


def make_puzzle(name: str, seed: int = 7) -> dict:
    """the fixture's puzzle `name` (build_puzzle of its CASES entry)"""
    sizes, sym, cycles = CASES[name]
    return build_puzzle(sizes, sym, cycles, DATA_ID[name], seed)


def build_puzzle(sizes, sym, cycles, data_id: int, seed: int = 7) -> dict:
    """-> part_feats float32 [N, 128], gt_pcs float32 [N, 3], thresholds float32 [N], n_pcs int64 [20], part_valids float32 [20],
    data_id, critical (bool [N]: the points built to be critical), partner (int64 [N]: the column built for each critical row, -1)"""
    rng = np.random.default_rng([seed, data_id])
    sd = head_state_dict(seed)
    n_pcs = np.zeros(P_MAX, dtype=np.int64)
    n_pcs[:len(sizes)] = sizes
    start = np.cumsum(n_pcs) - n_pcs
    N = int(n_pcs.sum())
    zp, zd = _unit(rng.normal(size=(N, LATENT))), _unit(rng.normal(size=(N, LATENT)))
    critical = np.zeros(N, dtype=bool)
    partner = np.full(N, -1, dtype=np.int64)
    free = [list(rng.permutation(s)) for s in sizes]

    def take(p):
        i = int(start[p] + free[p].pop())
        critical[i] = True
        return i

    def link(i, j):          # row i -> column j
        zd[j] = _unit(zp[i] + 0.3 * _unit(rng.normal(size=LATENT)))
        partner[i] = j

    for a, b, cnt in sym:
        for _ in range(cnt):
            i, j = take(a), take(b)
            link(i, j); link(j, i)
    for a, b, c, cnt in cycles:
        for _ in range(cnt):
            i, j, k = take(a), take(b), take(c)
            link(i, j); link(j, k); link(k, i)
    y = np.empty((N, 128))
    L = LATENT
    y[:, 0:L], y[:, L:2 * L], y[:, 2 * L:3 * L], y[:, 3 * L:4 * L] = zp, -zp, zd, -zd
    t = rng.uniform(0.2, 1.0, N)
    y[:, 124] = np.where(critical, t, -0.5)
    y[:, 125] = np.where(critical, -0.5, t)
    y[:, 126:] = 0.05 * rng.normal(size=(N, 2))
    g, b_, m, v = (sd[f"affinity_extractor.0.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    x = (y - b_) * np.sqrt(v + EPS) / g + m
    # geometry: piece p is the slab x in [0.3 p, 0.3 (p + 1)] of a bar, so points near an interface have close neighbours in another piece
    piece = np.repeat(np.arange(P_MAX), n_pcs)
    gt = rng.uniform(0, 0.3, (N, 3))
    gt[:, 0] += 0.3 * piece
    part_valids = np.zeros(P_MAX, dtype=np.float32)
    part_valids[:len(sizes)] = 1
    return {"part_feats": x.astype(np.float32), "gt_pcs": gt.astype(np.float32), "thresholds": rng.uniform(0.02, 0.08, N).astype(np.float32),
            "n_pcs": n_pcs, "part_valids": part_valids, "data_id": data_id, "critical": critical, "partner": partner}
