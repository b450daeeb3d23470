"""Seeded inputs and the float64 reference of the matcher's pairwise RANSAC (no test in here).

The reference of record is `ransac_reference`: a float64 numpy restatement of the procedure DESIGN.md 5.12 fixes - open3d's RANSAC,
which the reference's test pass calls (Jigsaw_matching/utils/estimate_transform.py:8-66), draws at random and cannot be run as an
oracle.  Hypothesis h of pair e draws three distinct correspondences from Philox4x32-10 (key = the seed's halves, counter = (h, e, 0,
0)), solves Horn's closed form with unit weights on them (utils/pairwise_alignment.py:11-79; the eigenvector by the ten-sweep cyclic
Jacobi the procedure names, in the kernel's order of operations, so that exact ties are ordered alike), counts the correspondences
within max_dist of their images and sums the inliers' squared distances; degenerate hypotheses (relative eigen-gap at most 1e-9) score
-1; the winner has the largest count, then the smallest sumsq, then the smallest h.
tools/make_matching_pose_goldens.py feeds seeded triples to the reference's own horn_87 and stores what it returns in
tests/golden/matching_pose.npz; tests/test_matching_pose_host.py pins `horn` to that file.  Inputs are regenerated here from seeds, so
the fixture holds results only.

The Philox rounds are written twice, `philox4x32_10` (numpy, vectorised) and `philox4x32_10_scalar` (Python integers), and the draw
likewise, so that each checks the other."""
from __future__ import annotations

import numpy as np

MAX_DIST = 0.05
GAP_DEGENERATE = 1e-9        # the kernel's rule
GAP_ASIDE = 1e-6             # hypotheses with a smaller relative gap are not compared
D2_ASIDE = 1e-9              # nor those with some | d^2 - max_dist^2 | below this
GAP_MIN = 0.02               # the winner's pose is compared when its relative gap is at least this
TILE = 1024                  # PFPP_RANSAC_TILE
U24 = 2.0 ** -24
HORN_SEED, HORN_TRIPLES = 41, 64         # the golden's triples

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ Philox, the draw
def philox4x32_10(ctr: np.ndarray, key) -> np.ndarray:
    """ctr uint [n, 4], key (k0, k1) -> uint64 [n, 4] holding the 32-bit outputs"""
    c = [np.asarray(ctr)[:, k].astype(np.uint64) for k in range(4)]
    k0, k1 = np.uint64(int(key[0]) & _MASK), np.uint64(int(key[1]) & _MASK)
    mask, s32 = np.uint64(_MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & mask, (p0 >> s32) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(_W0)) & mask, (k1 + np.uint64(_W1)) & mask
    return np.stack(c, 1)


def philox4x32_10_scalar(c0: int, c1: int, c2: int, c3: int, k0: int, k1: int):
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
        hi0, lo0 = divmod(_M0 * c0, 1 << 32)
        hi1, lo1 = divmod(_M1 * c2, 1 << 32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def draw_triples(M: int, hs, e: int, seed: int) -> np.ndarray:
    """the three distinct correspondence indices of hypotheses hs of pair e -> int64 [len(hs), 3]"""
    hs = np.asarray(hs, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((hs.size, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = hs, e
    x = philox4x32_10(ctr, (seed & _MASK, seed >> 32))
    s32 = np.uint64(32)
    i0 = (x[:, 0] * np.uint64(M)) >> s32
    i1 = (x[:, 1] * np.uint64(M - 1)) >> s32
    i1 = i1 + (i1 >= i0)
    i2 = (x[:, 2] * np.uint64(M - 2)) >> s32
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = i2 + (i2 >= lo)
    i2 = i2 + (i2 >= hi)
    return np.stack([i0, i1, i2], 1).astype(np.int64)


def draw_triple_scalar(M: int, h: int, e: int, seed: int):
    x0, x1, x2, _ = philox4x32_10_scalar(h, e, 0, 0, seed & _MASK, seed >> 32)
    i0 = (x0 * M) >> 32
    i1 = (x1 * (M - 1)) >> 32
    if i1 >= i0:
        i1 += 1
    i2 = (x2 * (M - 2)) >> 32
    for taken in sorted((i0, i1)):
        if i2 >= taken:
            i2 += 1
    return i0, i1, i2


# ------------------------------------------------------------------------------------------------------------------ Horn
def rotation(rng) -> np.ndarray:
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def horn_n(M: np.ndarray) -> np.ndarray:
    """pairwise_alignment.py:20-47 on M [..., 3, 3] -> N [..., 4, 4]"""
    m = lambda a, b: M[..., a, b]
    rows = [[m(0, 0) + m(1, 1) + m(2, 2), m(1, 2) - m(2, 1), m(2, 0) - m(0, 2), m(0, 1) - m(1, 0)],
            [m(1, 2) - m(2, 1), m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(0, 2) + m(2, 0)],
            [m(2, 0) - m(0, 2), m(0, 1) + m(1, 0), m(1, 1) - m(0, 0) - m(2, 2), m(1, 2) + m(2, 1)],
            [m(0, 1) - m(1, 0), m(2, 0) + m(0, 2), m(1, 2) + m(2, 1), m(2, 2) - m(0, 0) - m(1, 1)]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def quat_to_rot(q: np.ndarray) -> np.ndarray:
    """pairwise_alignment.py:52-70 on q [..., 4] -> [..., 3, 3]"""
    q0, q1, q2, q3 = (q[..., k] for k in range(4))
    rows = [[q0 ** 2 + q1 ** 2 - q2 ** 2 - q3 ** 2, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
            [2 * (q2 * q1 + q0 * q3), q0 ** 2 - q1 ** 2 + q2 ** 2 - q3 ** 2, 2 * (q2 * q3 - q0 * q1)],
            [2 * (q3 * q1 - q0 * q2), 2 * (q3 * q2 + q0 * q1), q0 ** 2 - q1 ** 2 - q2 ** 2 + q3 ** 2]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def jacobi_top(N: np.ndarray):
    """the kernels' eigen-solver, operation for operation (csrc/horn_common.h): a cyclic Jacobi of ten sweeps from the identity over the
    planes (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) on N [H, 4, 4] -> eigenvalues [H, 4] (unsorted), the eigenvector [H, 4] of the FIRST
    of the largest.  Every step is one IEEE operation on float64, as in the kernel, which is compiled without contraction"""
    A, V = np.array(N, dtype=np.float64), np.broadcast_to(np.eye(4), N.shape).copy()
    with np.errstate(all="ignore"):
        for _ in range(10):
            for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                apq = A[:, p, q]
                on = apq != 0.0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                tt = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(tt * tt + 1.0)
                sn = tt * c
                c, sn = np.where(on, c, 1.0)[:, None], np.where(on, sn, 0.0)[:, None]
                for X in (A, V):                                     # columns p, q of A and of V
                    xp, xq = X[:, :, p].copy(), X[:, :, q].copy()
                    X[:, :, p], X[:, :, q] = np.where(on[:, None], c * xp - sn * xq, xp), np.where(on[:, None], sn * xp + c * xq, xq)
                rp, rq = A[:, p, :].copy(), A[:, q, :].copy()          # rows p, q of A
                A[:, p, :], A[:, q, :] = np.where(on[:, None], c * rp - sn * rq, rp), np.where(on[:, None], sn * rp + c * rq, rq)
                A[:, p, q] = np.where(on, 0.0, A[:, p, q])
                A[:, q, p] = np.where(on, 0.0, A[:, q, p])
    ev = np.stack([A[:, k, k] for k in range(4)], 1)
    kb = ev.argmax(1)                                                # the first of equal maxima
    return ev, V[np.arange(N.shape[0]), :, kb], kb


def solve_from_m(M: np.ndarray, cS: np.ndarray, cT: np.ndarray):
    """M [H, 3, 3], centroids [H, 3] -> R [H, 3, 3], t [H, 3] = cT - R cS, gap [H] = (lambda_1 - lambda_2) / max |N_ij| (0 for N = 0),
    in the kernels' order of operations"""
    N = horn_n(M)
    ev, q, kb = jacobi_top(N)
    R = quat_to_rot(q)
    t = np.stack([cT[:, a] - ((R[:, a, 0] * cS[:, 0] + R[:, a, 1] * cS[:, 1]) + R[:, a, 2] * cS[:, 2]) for a in range(3)], 1)
    best = ev[np.arange(ev.shape[0]), kb]
    rest = np.where(np.arange(4)[None, :] == kb[:, None], -np.inf, ev).max(1)
    nmax = np.abs(N).max((-1, -2))
    gap = np.divide(best - rest, nmax, out=np.zeros_like(nmax), where=nmax > 0)
    return R, t, gap, best - rest, nmax


def horn_triples(S: np.ndarray, T: np.ndarray):
    """Horn with unit weights on triples S, T [H, 3, 3] as the scoring kernel forms it: centroids ((x0 + x1) + x2) / 3, M summed in
    the triple's order -> R, t, gap, degenerate bool [H] (the kernel's rule: not (lambda_1 - lambda_2 > 1e-9 max |N_ij|))"""
    S, T = np.asarray(S, dtype=np.float64), np.asarray(T, dtype=np.float64)
    cS, cT = ((S[:, 0] + S[:, 1]) + S[:, 2]) / 3.0, ((T[:, 0] + T[:, 1]) + T[:, 2]) / 3.0
    a, b = S - cS[:, None, :], T - cT[:, None, :]
    M = (a[:, 0, :, None] * b[:, 0, None, :] + a[:, 1, :, None] * b[:, 1, None, :]) + a[:, 2, :, None] * b[:, 2, None, :]
    R, t, gap, diff, nmax = solve_from_m(M, cS, cT)
    return R, t, gap, ~(diff > GAP_DEGENERATE * nmax)


def horn(S: np.ndarray, T: np.ndarray):
    """horn_87 with unit weights (W = 1 on the diagonal) in float64, without its final rounding, on S, T [n, 3] or [H, n, 3]
    -> R [..., 3, 3], t [..., 3], gap [...]"""
    S, T = np.asarray(S, dtype=np.float64), np.asarray(T, dtype=np.float64)
    single = S.ndim == 2
    if single:
        S, T = S[None], T[None]
    cS, cT = S.mean(-2), T.mean(-2)
    M = np.swapaxes(S - cS[:, None, :], -1, -2) @ (T - cT[:, None, :])
    R, t, gap, _, _ = solve_from_m(M, cS, cT)
    return (R[0], t[0], gap[0]) if single else (R, t, gap)


def horn_inputs():
    """the golden's seeded triples: S, T float64 [HORN_TRIPLES, 3, 3]; T is a rigid image of S plus noise"""
    rng = np.random.default_rng(HORN_SEED)
    S = rng.uniform(-0.5, 0.5, (HORN_TRIPLES, 3, 3))
    T = np.stack([s @ rotation(rng).T + rng.uniform(-1, 1, 3) for s in S]) + 0.01 * rng.normal(size=S.shape)
    return S, T


# ------------------------------------------------------------------------------------------------------------------ the procedure
def ransac_reference(pts, pair, corr, n_hyp: int, *, e: int = 0, seed: int = 0, max_dist: float = MAX_DIST, refine: bool = False) -> dict:
    """one pair.  pts [R, 3] (float32 values), pair = (source offset, target offset), corr int [M, 2]
    -> triples [H, 3], counts [H] (-1 degenerate), sumsq [H], gap [H], aside bool [H] (too close to a decision to compare), R64 [H, 3,
    3] / t64 [H, 3] (every hypothesis's pose), best_h, count, sumsq_best, status, R, t (the winner's pose, refined if asked and
    possible), n_refined"""
    pts = np.asarray(pts, dtype=np.float64)
    corr = np.asarray(corr, dtype=np.int64)
    S, T = pts[pair[0] + corr[:, 0]], pts[pair[1] + corr[:, 1]]
    M = corr.shape[0]
    tri = draw_triples(M, np.arange(n_hyp), e, seed)
    R, t, gap, deg = horn_triples(S[tri], T[tri])
    # | R S_k + t - T_k |^2 and the inliers' sum in correspondence order, in the kernel's order of operations
    d = [(((R[:, a, 0, None] * S[None, :, 0] + R[:, a, 1, None] * S[None, :, 1]) + R[:, a, 2, None] * S[None, :, 2]) + t[:, a, None]) - T[None, :, a]
         for a in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]                                               # [H, M]
    inl = d2 < max_dist ** 2
    counts = np.where(deg, -1, inl.sum(1))
    sumsq = np.where(deg, 0.0, np.cumsum(np.where(inl, d2, 0.0), 1)[:, -1])
    aside = (gap < GAP_ASIDE) | (np.abs(d2 - max_dist ** 2) < D2_ASIDE).any(1)
    out = {"triples": tri, "counts": counts, "sumsq": sumsq, "gap": gap, "aside": aside, "R64": R, "t64": t, "S": S, "T": T, "n_refined": 0}
    if counts.max() < 0:
        out.update(best_h=-1, count=-1, sumsq_best=0.0, status=0, R=np.eye(3), t=T.mean(0) - S.mean(0))
        return out
    order = np.lexsort((np.arange(n_hyp), sumsq, -counts))
    h = int(order[0])
    out.update(best_h=h, count=int(counts[h]), sumsq_best=float(sumsq[h]), status=1, R=R[h], t=t[h])
    if refine:
        out.update(refine_pose(S, T, R[h], t[h], max_dist))
    return out


def refine_pose(S, T, R, t, max_dist: float = MAX_DIST) -> dict:
    """one more Horn over the inliers of (R, t); the pose is kept when fewer than three or a degenerate N"""
    inl = (((S @ R.T) + t - T) ** 2).sum(-1) < max_dist ** 2
    out = {"n_refined": int(inl.sum()), "status": 1, "R": R, "t": t}
    if inl.sum() >= 3:
        R2, t2, gap = horn(S[inl], T[inl])
        if gap > GAP_DEGENERATE:
            out.update(status=3, R=R2, t=t2)
    return out


def planted_case(M: int, *, seed: int, outliers: float = 0.3, noise: float = 0.0, pad: int = 0) -> dict:
    """M correspondences under a planted pose: T = R0 S + t0 in float64, rounded to float32; a fraction of the targets displaced
    by sigma = 0.3; `pad` unrelated rows in front of each piece (non-zero row offsets) and the correspondences shuffled
    -> pts float32 [2 (pad + M), 3], pair, corr int64 [M, 2], R0, t0, inlier bool [M]"""
    rng = np.random.default_rng([seed, M])
    S = rng.uniform(-0.5, 0.5, (M, 3)).astype(np.float32)
    R0, t0 = rotation(rng), rng.uniform(-1, 1, 3)
    T = S.astype(np.float64) @ R0.T + t0 + noise * rng.normal(size=(M, 3))
    bad = np.zeros(M, dtype=bool)
    bad[rng.permutation(M)[:int(round(outliers * M))]] = True
    if M <= 4:
        bad[:] = False
    T[bad] += 0.3 * rng.normal(size=(int(bad.sum()), 3))
    ps, pt = rng.permutation(M), rng.permutation(M)                   # row order inside the two pieces
    src, tgt = np.zeros((M, 3), dtype=np.float32), np.zeros((M, 3), dtype=np.float32)
    src[ps], tgt[pt] = S, T.astype(np.float32)
    filler = rng.uniform(-2, 2, (2, pad, 3)).astype(np.float32)
    pts = np.concatenate([filler[0], src, filler[1], tgt])
    return {"pts": pts, "pair": (pad, 2 * pad + M), "corr": np.stack([ps, pt], 1).astype(np.int64), "R0": R0, "t0": t0, "inlier": ~bad}


# ------------------------------------------------------------------------------------------------------------------ pose graphs
def rigid4(rng) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(rng), rng.uniform(-1, 1, 3)
    return T


def graph_cases() -> dict:
    """name -> (v_num, edges int64 [m, 2], transformations [m, 4, 4], uncertainty [m]): the golden's graphs.  `dense` has equal
    weights on all 190 edges of 20 vertices (Kruskal's tie rule and the search order decide the tree), `two_components` needs the
    hub (vertices 0, 2, 5 and 1, 3, 4, 6: the larger component does not hold vertex 0), `chain` is listed out of order with
    unequal weights, `star` has its centre at vertex 3, `cycle` has a heavy edge the tree must leave out and one edge given twice"""
    rng = np.random.default_rng(53)
    out = {}

    def add(name, v, edges, u):
        edges = np.asarray(edges, dtype=np.int64)
        out[name] = (v, edges, np.stack([rigid4(rng) for _ in edges]), np.asarray(u, dtype=np.float64))

    add("chain", 6, [(3, 2), (1, 0), (5, 4), (2, 1), (4, 3)], [0.25, 0.5, 0.125, 1.0, 1 / 3])
    add("star", 7, [(3, 0), (1, 3), (3, 2), (4, 3), (3, 5), (6, 3)], [0.2, 0.1, 0.3, 0.1, 0.5, 0.25])
    add("dense", 20, [(j, i) for i in range(20) for j in range(i + 1, 20)], np.full(190, 0.125))
    add("two_components", 7, [(2, 0), (5, 2), (3, 1), (4, 3), (6, 4), (6, 1)], [0.5, 0.25, 0.2, 0.2, 0.2, 0.2])
    add("cycle", 5, [(1, 0), (2, 1), (3, 2), (4, 3), (4, 0), (2, 1), (3, 0)], [0.1, 0.9, 0.1, 0.1, 0.1, 0.05, 1.0])
    return out


def quat_wxyz(R: np.ndarray) -> np.ndarray:
    """a rotation matrix's quaternion (w, x, y, z), w >= 0, for rotations away from half a turn"""
    w = np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 0.0)) / 2
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def quat_rmat(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def make_puzzle(sizes, links, *, seed: int, shared: int = 12, N: int = None, cut=None) -> dict:
    """a synthetic puzzle: piece p has sizes[p] points, of which `shared` per link (p, q) are exact copies of the other piece's
    (fracture points: true matches exist).  gt = R_gt part + t_gt with t_gt the piece's centroid and R_gt a seeded rotation.
    The assignment is the ground truth's: the block (p, q), p < q, of the dense 0 / 1 matrix.  cut = (p, q, keep): only `keep`
    matches of that link stay in the assignment.  Arrays are padded to N points and 1 puzzle (leading axis)"""
    rng = np.random.default_rng([seed, len(sizes)])
    P = len(sizes)
    gt = [rng.uniform(-0.5, 0.5, (n, 3)) + 0.3 * rng.normal(size=3) for n in sizes]
    used = [0] * P
    crit = [[] for _ in range(P)]
    match = []
    for p, q in links:
        pts = rng.uniform(-0.5, 0.5, (shared, 3))
        rp, rq = np.arange(shared) + used[p], np.arange(shared) + used[q]
        gt[p][rp], gt[q][rq] = pts, pts
        match.append((p, q, len(crit[p]) + np.arange(shared), len(crit[q]) + np.arange(shared)))
        crit[p] += rp.tolist(); crit[q] += rq.tolist()
        used[p] += shared; used[q] += shared
    n_crit = np.array([len(c) for c in crit])
    c0 = np.cumsum(n_crit) - n_crit
    perm = np.zeros((n_crit.sum(), n_crit.sum()))
    for p, q, a, b in match:
        keep = cut[2] if cut is not None and cut[:2] == (p, q) else shared
        perm[c0[p] + a[:keep], c0[q] + b[:keep]] = 1
    N = N or int(sum(sizes))
    part, quat, trans, crit_idx = np.zeros((N, 3)), np.zeros((P, 4)), np.zeros((P, 3)), np.zeros(N, dtype=np.int64)
    at = 0
    for p in range(P):
        Rg, tg = rotation(rng), gt[p].mean(0)
        q = quat_wxyz(Rg)
        Rg = quat_rmat(q)
        part[at:at + sizes[p]] = (gt[p] - tg) @ Rg                     # R_gt^T (gt - t_gt)
        quat[p], trans[p] = q, tg
        crit_idx[at:at + n_crit[p]] = crit[p]
        at += sizes[p]
    part32 = part.astype(np.float32)
    gt_all = np.zeros((N, 3))
    at = 0
    for p in range(P):
        gt_all[at:at + sizes[p]] = part32[at:at + sizes[p]].astype(np.float64) @ quat_rmat(quat[p].astype(np.float32)).T + trans[p].astype(np.float32)
        at += sizes[p]
    return {"part_pcs": part32[None], "gt_pcs": gt_all.astype(np.float32)[None], "n_pcs": np.asarray(sizes, dtype=np.int64)[None],
            "part_valids": np.ones((1, P), dtype=np.float32), "part_quat": quat.astype(np.float32)[None], "part_trans": trans.astype(np.float32)[None],
            "n_critical_pcs": n_crit[None], "critical_pcs_idx": crit_idx[None], "perm_mat": [perm]}


def stack_puzzles(items) -> dict:
    """puzzles of make_puzzle (same N) -> one batch; pieces padded to the largest P"""
    P = max(x["n_pcs"].shape[1] for x in items)
    pad = lambda a: np.concatenate([a, np.zeros((1, P - a.shape[1]) + a.shape[2:], dtype=a.dtype)], 1)
    out = {k: np.concatenate([pad(x[k]) if k in ("n_pcs", "part_valids", "part_quat", "part_trans", "n_critical_pcs") else x[k] for x in items])
           for k in items[0] if k != "perm_mat"}
    out["perm_mat"] = [x["perm_mat"][0] for x in items]
    return out


def lexico_iter(lex):
    import itertools

    return itertools.combinations(lex, 2)


def global_transformation_reference(data: dict, edge_pose, global_alignment) -> dict:
    """compute_global_transformation (matching_base_model.py:274-454), loop for loop in float64, with its two outside calls as
    arguments: edge_pose(b, k, idx1, idx2, src, tgt, corr) -> 4 x 4 (k = the edge's number in its puzzle) stands for get_trans_from_mat's RANSAC, global_alignment(v_num, edges,
    transformations, uncertainty) for the global alignment -> rot [B, P, 3, 3], trans [B, P, 3], pivots, edges (per puzzle, with
    their transformations and uncertainties)"""
    match_mat, gt_pcs, part_pcs = data["perm_mat"], data["gt_pcs"], np.asarray(data["part_pcs"], dtype=np.float64)
    n_critical_pcs, critical_pcs_idx, n_pcs = data["n_critical_pcs"], data["critical_pcs_idx"], data["n_pcs"]
    n_valid = data["part_valids"].sum(1).astype(np.int32)
    part_quat, part_trans = np.asarray(data["part_quat"], dtype=np.float64), np.asarray(data["part_trans"], dtype=np.float64)
    B, P = n_pcs.shape
    n_critical_pcs_cumsum, n_pcs_cumsum = np.cumsum(n_critical_pcs, axis=-1), np.cumsum(n_pcs, axis=-1)
    pred = {"rot": np.zeros((B, P, 3, 3)), "trans": np.zeros((B, P, 3)), "pivots": [], "graphs": []}
    for b in range(B):
        piece_connections = np.zeros(n_valid[b])
        sum_full_matched = np.sum(match_mat[b])
        edges, transformations, uncertainty = [], [], []

        def ranges(idx1, idx2):
            cri_st1 = 0 if idx1 == 0 else n_critical_pcs_cumsum[b, idx1 - 1]
            cri_st2 = 0 if idx2 == 0 else n_critical_pcs_cumsum[b, idx2 - 1]
            pc_st1 = 0 if idx1 == 0 else n_pcs_cumsum[b, idx1 - 1]
            pc_st2 = 0 if idx2 == 0 else n_pcs_cumsum[b, idx2 - 1]
            return cri_st1, n_critical_pcs_cumsum[b, idx1], cri_st2, n_critical_pcs_cumsum[b, idx2], pc_st1, n_pcs_cumsum[b, idx1], pc_st2, n_pcs_cumsum[b, idx2]

        def block(cri_st1, cri_ed1, cri_st2, cri_ed2):
            mat = match_mat[b][cri_st1:cri_ed1, cri_st2:cri_ed2]
            mat_s = np.sum(mat).astype(np.int32)
            mat2 = match_mat[b][cri_st2:cri_ed2, cri_st1:cri_ed1]
            mat_s2 = np.sum(mat2).astype(np.int32)
            if mat_s < mat_s2:
                mat, mat_s = mat2.transpose(1, 0), mat_s2
            return mat, mat_s

        for idx1, idx2 in lexico_iter(np.arange(n_valid[b])):
            cri_st1, cri_ed1, cri_st2, cri_ed2, pc_st1, pc_ed1, pc_st2, pc_ed2 = ranges(idx1, idx2)
            n1, n2 = n_critical_pcs[b, idx1], n_critical_pcs[b, idx2]
            if n1 == 0 or n2 == 0:
                continue
            mat, mat_s = block(cri_st1, cri_ed1, cri_st2, cri_ed2)
            if n_valid[b] > 2 and mat_s == 0 and sum_full_matched > 0:
                continue
            if np.count_nonzero(mat) < 3:
                continue
            pc1, pc2 = part_pcs[b, pc_st1:pc_ed1], part_pcs[b, pc_st2:pc_ed2]
            src = pc1[critical_pcs_idx[b, pc_st1: pc_st1 + n1]]
            tgt = pc2[critical_pcs_idx[b, pc_st2: pc_st2 + n2]]
            corr = np.vstack(mat.nonzero()).transpose(1, 0)
            edges.append(np.array([idx2, idx1]))
            transformations.append(edge_pose(b, len(edges) - 1, idx1, idx2, src, tgt, corr))
            uncertainty.append(1.0 / mat_s)
            piece_connections[idx1] += 1
            piece_connections[idx2] += 1
        n_ransac = len(edges)
        for idx1, idx2 in lexico_iter(np.arange(n_valid[b])):
            if piece_connections[idx1] > 0 and piece_connections[idx2] > 0:
                continue
            if piece_connections[idx1] == 0 and piece_connections[idx2] == 0:
                continue
            cri_st1, cri_ed1, cri_st2, cri_ed2, pc_st1, pc_ed1, pc_st2, pc_ed2 = ranges(idx1, idx2)
            n1, n2 = n_critical_pcs[b, idx1], n_critical_pcs[b, idx2]
            pc1, pc2 = part_pcs[b, pc_st1:pc_ed1], part_pcs[b, pc_st2:pc_ed2]
            trans_mat = np.eye(4)
            if n1 == 0 or n2 == 0:
                if n2 > 0:
                    trans_mat[:3, 3] = [critical_pcs_idx[b, pc_st2]] - np.sum(pc1, axis=0)
                elif n1 > 0:
                    trans_mat[:3, 3] = np.sum(pc2, axis=0) - pc1[critical_pcs_idx[b, pc_st1]]
                else:
                    trans_mat[:3, 3] = np.sum(pc2, axis=0) - np.sum(pc1, axis=0)
            else:
                mat, mat_s = block(cri_st1, cri_ed1, cri_st2, cri_ed2)
                src = pc1[critical_pcs_idx[b, pc_st1: pc_st1 + n1]]
                tgt = pc2[critical_pcs_idx[b, pc_st2: pc_st2 + n2]]
                matching1, matching2 = np.nonzero(mat)
                trans_mat[:3, 3] = np.sum(tgt[matching2], axis=0) - np.sum(src[matching1], axis=0)
            edges.append(np.array([idx2, idx1]))
            transformations.append(trans_mat)
            uncertainty.append(1)
            piece_connections[idx1] += 1
            piece_connections[idx2] += 1
        if len(edges) > 0:
            g = global_alignment(n_valid[b], np.stack(edges), np.stack(transformations), np.array(uncertainty, dtype=np.float64))
            pivot = 1
            for idx in range(n_valid[b]):
                if n_pcs[b, idx] > n_pcs[b, pivot]:
                    pivot = idx
        else:
            g = np.repeat(np.eye(4).reshape((1, 4, 4)), n_valid[b], axis=0)
            pivot = 0
        to_gt = np.eye(4)
        to_gt[:3, :3] = quat_rmat(part_quat[b, pivot])
        to_gt[:3, 3] = part_trans[b, pivot]
        offset = to_gt @ np.linalg.inv(g[pivot])
        g = np.stack([offset @ x for x in g])
        pred["rot"][b, :n_valid[b]], pred["trans"][b, :n_valid[b]] = g[:, :3, :3], g[:, :3, 3]
        pred["pivots"].append(pivot)
        pred["graphs"].append({"edges": np.asarray(edges).reshape(-1, 2), "transformations": np.asarray(transformations).reshape(-1, 4, 4),
                               "uncertainty": np.asarray(uncertainty, dtype=np.float64), "n_ransac": n_ransac})
    return pred


def euler_xyz_deg(R: np.ndarray) -> np.ndarray:
    """pytorch3d's matrix_to_euler_angles(R, "XYZ") in degrees on [..., 3, 3]"""
    return np.degrees(np.stack([np.arctan2(-R[..., 1, 2], R[..., 2, 2]), np.arcsin(np.clip(R[..., 0, 2], -1, 1)), np.arctan2(-R[..., 0, 1], R[..., 0, 0])], -1))


def pose_metrics_reference(data: dict, pred: dict) -> dict:
    """trans_metrics / rot_metrics of eval_utils.py:250-304 in float64, averaged over the batch as calc_metric does"""
    valids = data["part_valids"].astype(np.float64)
    gt_rot = np.stack([[quat_rmat(q) if np.any(q) else np.eye(3) for q in row] for row in np.asarray(data["part_quat"], dtype=np.float64)])
    dt = pred["trans"] - np.asarray(data["part_trans"], dtype=np.float64)
    gap = np.abs(euler_xyz_deg(pred["rot"]) - euler_xyz_deg(gt_rot))
    dr = np.minimum(gap, 360.0 - gap)
    out = {}
    for name, d in (("trans", dt), ("rot", dr)):
        per = {"mse": (d ** 2).mean(-1), "rmse": (d ** 2).mean(-1) ** 0.5, "mae": np.abs(d).mean(-1)}
        for m, v in per.items():
            out[f"{name}_{m}"] = float(((v * valids).sum(1) / valids.sum(1)).mean())
    return out
