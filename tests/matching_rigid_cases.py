"""Seeded inputs and the float64 reference of the rigid term of the matcher's training loss (no test in here).

The reference of record is `rigid_reference`: a float64 torch restatement of rigid_loss (Jigsaw_matching/utils/loss.py:59-142) and
horn_87 (utils/pairwise_alignment.py:11-79), run under autograd on the CPU, and `head_rigid_train_reference`, the head's whole
training step (matching_train_cases.head_train_reference) with the term added.  tools/make_matching_rigid_goldens.py feeds the same
inputs to the reference's own code and stores what it returns in tests/golden/matching_rigid.npz; tests/test_matching_rigid_host.py
pins the restatement to that file.  Inputs are regenerated here from seeds, so the fixture holds results only.

Conventions (also the engine's).  A puzzle's critical rows are in piece order; `counts` are the rows per piece, `pts` the critical
points of part_pcs in row order.  A pair p < q is listed when both pieces own rows; its status is 1 (kept), 0 (skipped by
loss.py:98) or -1 (the reference divides 0 by 0: mat_s == 0 and not skipped).  Where the reference's result is not finite - a status
of -1 anywhere in the batch, or no kept pair - the term is reported as 0 with zero gradient.  `poses=(R [k, 3, 3], t [k, 3])` imposes
the poses (the GPU's, or the reference's float32 ones) instead of Horn's own, which the reference rounds to float32 and detaches."""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("matching_train_cases", Path(__file__).resolve().parent / "matching_train_cases.py")
_tc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_tc)

BATCHES = tuple(_tc.BATCHES)             # main, one_owner, empty_puzzle: the whole-step batches, here with a part_pcs
PART_PCS_SEED = 23                       # the pieces' rotations; tools/make_matching_rigid_goldens.py asserts the eigen-gap they give
GAP_MIN = 0.02                           # poses are compared on pairs whose relative eigen-gap is at least this
SAMPLE = 37                              # stride of the stored samples of large tensors
make_batch, head_state_dict = _tc.make_batch, _tc.head_state_dict

# name -> puzzles, each a list of critical points per piece (all pieces valid)
KERNEL_CASES = {
    "edges": [[0, 1, 2, 3, 63, 64, 65]],                       # one under, on and over a tile / a wave; an empty piece; single points
    "two_piece": [[5, 7]],
    "twenty": [[3, 4, 5, 6, 7, 8, 9, 3, 4, 5, 6, 7, 8, 9, 3, 4, 5, 6, 7, 8]],      # 190 pairs
    "large": [[207, 206, 207, 206, 207]],                      # n = 1033: several column tiles per piece, 17 row tiles
    "zero_block": [[6, 5, 7]],                                 # blocks (0, 2) and (2, 0) exactly zero: skipped
    "two_piece_zero": [[4, 6]],                                # mat_s == 0 in a two-piece puzzle: 0 / 0 in t
    "nothing_kept": [[4, 3, 5]],                               # every off-diagonal block zero: all skipped, n_sum == 0
    "two_puzzles": [[4, 6, 5], [7, 3]],                        # two puzzles in one pose launch
}
ZEROED = {"zero_block": [(0, 0, 2)], "two_piece_zero": [(0, 0, 1)], "nothing_kept": [(0, 0, 1), (0, 0, 2), (0, 1, 2)]}


def rotation(rng) -> np.ndarray:
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def kernel_case(name: str, seed: int = 7) -> dict:
    """-> ds_mat (list of float32 [n, n]), pts (list of float32 [n, 3]), counts (list of lists), n_valid (list), row_piece (list of
    int32 [n]).  Every piece samples the same seeded base shape under its own rigid motion, so corresponding points (same base index)
    of any two pieces really are related by one; ds_mat is positive noise plus planted weights on those correspondences."""
    out = {"ds_mat": [], "pts": [], "counts": [], "n_valid": [], "row_piece": []}
    for b, counts in enumerate(KERNEL_CASES[name]):
        rng = np.random.default_rng([seed, sorted(KERNEL_CASES).index(name), b])
        n, P = int(sum(counts)), len(counts)
        off = np.concatenate([[0], np.cumsum(counts)])
        base = rng.uniform(-0.5, 0.5, (max(counts), 3))
        pts = np.zeros((n, 3))
        for p, c in enumerate(counts):
            Rp, tp = rotation(rng), rng.uniform(-1, 1, 3)
            pts[off[p]:off[p + 1]] = (base[:c] + 0.003 * rng.normal(size=(c, 3))) @ Rp.T + tp
        ds = rng.uniform(0.0005, 0.004, (n, n))
        for p in range(P):
            for q in range(P):
                if p != q:
                    k = np.arange(min(counts[p], counts[q]))
                    ds[off[p] + k, off[q] + k] += rng.uniform(0.05, 0.4, k.size) / max(P - 1, 1)
        for (zb, p, q) in ZEROED.get(name, []):
            if zb == b:
                ds[off[p]:off[p + 1], off[q]:off[q + 1]] = 0
                ds[off[q]:off[q + 1], off[p]:off[p + 1]] = 0
        out["ds_mat"].append(ds.astype(np.float32)); out["pts"].append(pts.astype(np.float32)); out["counts"].append(list(counts))
        out["n_valid"].append(P); out["row_piece"].append(np.repeat(np.arange(P), counts).astype(np.int32))
    return out


def make_part_pcs(batch: dict, seed: int = PART_PCS_SEED) -> np.ndarray:
    """part_pcs float32 [B, N_sum, 3] of a matching_train_cases batch: every piece's gt_pcs recentred and turned by a seeded rotation"""
    gt = np.asarray(batch["gt_pcs"], dtype=np.float64)
    out = np.zeros_like(gt)
    for b in range(gt.shape[0]):
        rng = np.random.default_rng([seed, b])
        start = 0
        for c in np.asarray(batch["n_pcs"])[b]:
            c = int(c)
            if c:
                x = gt[b, start:start + c]
                out[b, start:start + c] = (x - x.mean(0)) @ rotation(rng).T
            start += c
    return out.astype(np.float32)


def batch_rigid_inputs(batch: dict) -> dict:
    """the rigid term's view of a whole-step batch: counts / n_valid / row_piece per puzzle and the critical rows' indices"""
    labels = np.asarray(batch["critical_label"]) != 0
    n_pcs = np.asarray(batch["n_pcs"]).astype(np.int64)
    nv = np.asarray(batch["part_valids"]).sum(1).astype(np.int64)
    counts, pieces = [], []
    for b in range(labels.shape[0]):
        piece = np.repeat(np.arange(n_pcs.shape[1]), n_pcs[b])
        pieces.append(piece[labels[b]].astype(np.int32))
        counts.append(np.bincount(piece[labels[b]], minlength=int(nv[b]))[:int(nv[b])].tolist())
    return {"counts": counts, "n_valid": [int(v) for v in nv], "row_piece": pieces, "labels": labels}


# ------------------------------------------------------------------------------------------------------------------ float64 pieces
def horn_n(M: np.ndarray) -> np.ndarray:
    """pairwise_alignment.py:20-47"""
    return np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                     [M[1, 2] - M[2, 1], M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[0, 2] + M[2, 0]],
                     [M[2, 0] - M[0, 2], M[0, 1] + M[1, 0], M[1, 1] - M[0, 0] - M[2, 2], M[1, 2] + M[2, 1]],
                     [M[0, 1] - M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1], M[2, 2] - M[0, 0] - M[1, 1]]])


def quat_to_rot(q: np.ndarray) -> np.ndarray:
    """pairwise_alignment.py:52-70"""
    return np.array([[q[0] ** 2 + q[1] ** 2 - q[2] ** 2 - q[3] ** 2, 2 * (q[1] * q[2] - q[0] * q[3]), 2 * (q[1] * q[3] + q[0] * q[2])],
                     [2 * (q[2] * q[1] + q[0] * q[3]), q[0] ** 2 - q[1] ** 2 + q[2] ** 2 - q[3] ** 2, 2 * (q[2] * q[3] - q[0] * q[1])],
                     [2 * (q[3] * q[1] - q[0] * q[2]), 2 * (q[3] * q[2] + q[0] * q[1]), q[0] ** 2 - q[1] ** 2 - q[2] ** 2 + q[3] ** 2]])


def horn(S: np.ndarray, T: np.ndarray, W: np.ndarray):
    """horn_87 in the dtype of its arguments, without its final rounding to float32 -> (R [3, 3], t [3], eigenvalues ascending [4], N)"""
    S, T = S.T, T.T
    cS, cT = S.mean(axis=1), T.mean(axis=1)
    Sc, Tc = S - cS.reshape(-1, 1), T - cT.reshape(-1, 1)
    N = horn_n(Sc @ W @ Tc.T)
    v, u = np.linalg.eigh(N)
    R = quat_to_rot(u[:, v.argmax()])
    S2, T2 = Sc + cS.reshape(-1, 1), Tc + cT.reshape(-1, 1)
    t = (W @ T2.T).T - (np.sum(W, axis=-1).reshape((-1, 1)) * (R @ S2).T).T
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sum(t, axis=-1) / np.sum(W)
    return R, t, v, N


def eigen_gap(v: np.ndarray) -> float:
    """(lambda_1 - lambda_2) / max |lambda| of ascending eigenvalues; 0 for a zero matrix"""
    m = float(np.abs(v).max())
    return float(v[-1] - v[-2]) / m if m > 0 else 0.0


def pair_list(counts, n_valid):
    return [(b, p, q) for b, c in enumerate(counts) for p in range(n_valid[b]) for q in range(p + 1, n_valid[b]) if c[p] > 0 and c[q] > 0]


def rigid_reference(ds_mats, pts, counts, n_valid, *, poses=None, w_rig: float = 1.0, dtype=torch.float64) -> dict:
    """rigid_loss over a batch.  ds_mats: list of [n, n] (arrays or tensors; a tensor that requires grad is used as it is, so the
    term can sit inside a larger graph), pts: list of [n, 3].
    -> pairs [(b, p, q)], status [k], R [k, 3, 3] / t [k, 3] (the poses used: Horn's rounded to float32, or the imposed ones), R64 /
    t64 (Horn's own, unrounded), eig [k, 4], gap [k], mat_s [k], pair_loss [k], n_sum, numerator, finite, term (the graph's
    w_rig-free loss tensor: numerator / n_sum, or a zero where the reference is not finite), rig_loss (its value), and, unless a
    ds_mat came with a graph of its own, dP: list of d(w_rig rig_loss) / d ds_mat"""
    own = not any(torch.is_tensor(m) and m.requires_grad for m in ds_mats)
    mats = [m if torch.is_tensor(m) and m.requires_grad else torch.as_tensor(np.asarray(m)).to(dtype).clone().requires_grad_(True) for m in ds_mats]
    X = [torch.as_tensor(np.asarray(x)).to(dtype) for x in pts]
    pairs = pair_list(counts, n_valid)
    k = len(pairs)
    out = {"pairs": pairs, "status": np.zeros(k, dtype=np.int32), "R": np.zeros((k, 3, 3)), "t": np.zeros((k, 3)), "R64": np.zeros((k, 3, 3)),
           "t64": np.zeros((k, 3)), "eig": np.zeros((k, 4)), "gap": np.zeros(k), "mat_s": np.zeros(k), "pair_loss": np.zeros(k)}
    loss = torch.zeros((), dtype=dtype)
    n_sum = 0
    for idx, (b, p, q) in enumerate(pairs):
        off = np.concatenate([[0], np.cumsum(counts[b])])
        i0, i1, j0, j1 = off[p], off[p + 1], off[q], off[q + 1]
        mat = mats[b][i0:i1, j0:j1] + mats[b][j0:j1, i0:i1].transpose(1, 0)
        mat_s = mat.sum()
        out["mat_s"][idx] = float(mat_s.detach())
        S, T = X[b][i0:i1], X[b][j0:j1]
        R64, t64, v, _ = horn(S.numpy().astype(np.float64), T.numpy().astype(np.float64), mat.detach().numpy().astype(np.float64))
        out["R64"][idx], out["t64"][idx], out["eig"][idx], out["gap"][idx] = R64, t64, v, eigen_gap(v)
        if n_valid[b] > 2 and float(mat_s.detach()) == 0 and float(mats[b].detach().sum()) > 0:       # loss.py:98
            continue
        if float(mat_s.detach()) == 0:                                                          # 0 / 0 in horn_87's t
            out["status"][idx] = -1
            continue
        out["status"][idx] = 1
        if poses is None:
            R, t = R64.astype(np.float32).astype(np.float64), t64.astype(np.float32).astype(np.float64)   # pairwise_alignment.py:79
        else:
            R, t = np.asarray(poses[0][idx], dtype=np.float64), np.asarray(poses[1][idx], dtype=np.float64)
        out["R"][idx], out["t"][idx] = R, t
        src = (torch.as_tensor(R).to(dtype) @ S.transpose(1, 0)).transpose(1, 0) + torch.as_tensor(t).to(dtype)
        src = src * mat.sum(-1).reshape(-1, 1)
        tgt = mat @ T
        pair_loss = (src ** 2 + tgt ** 2 - 2 * src * tgt).sum()
        out["pair_loss"][idx] = float(pair_loss.detach())
        n_sum += int(i1 - i0)
        loss = loss + pair_loss * mat_s
    finite = n_sum > 0 and not (out["status"] < 0).any()
    term = loss / n_sum if finite else sum((m * 0).sum() for m in mats) if mats else loss
    out.update(n_sum=n_sum, numerator=float(loss.detach()), finite=finite, term=term, rig_loss=float(term.detach()))
    if own:
        if finite:
            (w_rig * term).backward()
        out["dP"] = [m.grad if m.grad is not None else torch.zeros_like(m) for m in mats]
    return out


def scatter_poses(called, R, t):
    """poses stored per CALL of the reference's pairwise_alignment (the pairs it does not skip) -> poses per listed pair"""
    called = np.asarray(called) != 0
    Rf, tf = np.zeros((called.size, 3, 3)), np.zeros((called.size, 3))
    Rf[called], tf[called] = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), np.asarray(t, dtype=np.float64).reshape(-1, 3)
    return Rf, tf


def rigid_closed_form(ds_mats, pts, counts, n_valid, poses, w_rig: float = 1.0):
    """the kernels' formulas in float64 numpy: r_i = sum_j W_ij, b_i = sum_j W_ij T_j, e_i = r_i A_i - b_i, pair_loss = sum |e_i|^2,
    d(pair_loss mat_s) / dW_ij = 2 mat_s e_i . (A_i - T_j) + pair_loss -> (rig_loss, list of dP, pair_loss [k], mat_s [k])"""
    pairs = pair_list(counts, n_valid)
    mats = [np.asarray(m, dtype=np.float64) for m in ds_mats]
    grads = [np.zeros_like(m) for m in mats]
    pl, ms, kept = np.zeros(len(pairs)), np.zeros(len(pairs)), np.zeros(len(pairs), dtype=bool)
    bad, n_sum = False, 0
    parts = []
    for idx, (b, p, q) in enumerate(pairs):
        off = np.concatenate([[0], np.cumsum(counts[b])])
        i0, i1, j0, j1 = off[p], off[p + 1], off[q], off[q + 1]
        W = mats[b][i0:i1, j0:j1] + mats[b][j0:j1, i0:i1].T
        S, T = np.asarray(pts[b], dtype=np.float64)[i0:i1], np.asarray(pts[b], dtype=np.float64)[j0:j1]
        ms[idx] = W.sum()
        if ms[idx] == 0:
            bad |= not (n_valid[b] > 2 and mats[b].sum() > 0)
            continue
        kept[idx] = True
        A = S @ np.asarray(poses[0][idx], dtype=np.float64).T + np.asarray(poses[1][idx], dtype=np.float64)
        r, bb = W.sum(1), W @ T
        e = r[:, None] * A - bb
        pl[idx] = (e ** 2).sum()
        n_sum += i1 - i0
        dW = 2 * ms[idx] * ((e * A).sum(1)[:, None] - e @ T.T) + pl[idx]
        parts.append((b, i0, i1, j0, j1, dW))
    if bad or n_sum == 0:
        return 0.0, grads, pl, ms
    for b, i0, i1, j0, j1, dW in parts:
        grads[b][i0:i1, j0:j1] = dW * (w_rig / n_sum)
        grads[b][j0:j1, i0:i1] = dW.T * (w_rig / n_sum)
    return float((pl * ms)[kept].sum() / n_sum), grads, pl, ms


def pair_sums_reference(ds_mat, pts, counts):
    """float64 numpy: rb [n, P, 4] = (r_i, b_i) of every row against every later piece (other slots 0), and the sums of the terms'
    magnitudes in the same layout (for the reordering bound)"""
    ds, X = np.asarray(ds_mat, dtype=np.float64), np.asarray(pts, dtype=np.float64)
    P, off = len(counts), np.concatenate([[0], np.cumsum(counts)])
    rb, mag = np.zeros((ds.shape[0], P, 4)), np.zeros((ds.shape[0], P, 4))
    for p in range(P):
        for q in range(p + 1, P):
            W = ds[off[p]:off[p + 1], off[q]:off[q + 1]] + ds[off[q]:off[q + 1], off[p]:off[p + 1]].T
            T = X[off[q]:off[q + 1]]
            rb[off[p]:off[p + 1], q, 0], rb[off[p]:off[p + 1], q, 1:] = W.sum(1), W @ T
            mag[off[p]:off[p + 1], q, 0], mag[off[p]:off[p + 1], q, 1:] = np.abs(W).sum(1), np.abs(W) @ np.abs(T)
    return rb, mag


# ------------------------------------------------------------------------------------------------------------------ the whole step
def head_rigid_train_reference(sd: dict, batch: dict, part_pcs, *, w_cls: float = 1.0, w_mat: float = 1.0, w_rig: float = 1.0, relu_masks=None,
                               poses=None, dtype=torch.float64, tau: float = _tc.TAU, max_iter: int = _tc.MAX_ITER) -> dict:
    """matching_train_cases.head_train_reference with loss = w_cls cls_loss + w_mat mat_loss + w_rig rig_loss (w_mat != 0): the same
    forward, the rigid term on the step's own ds_mat inside the graph.  -> its keys plus rig_loss and `rigid` (rigid_reference's dict)"""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype) if not torch.is_tensor(a) else a.detach().to(dtype)
    p = {k: t(sd[k]).clone().requires_grad_(True) for k in _tc.PARAMS}
    buf = {k: t(sd[k]) for k in _tc.BUFFERS}
    x = t(batch["part_feats"])
    B, N_sum, F = x.shape
    feats = x.reshape(B * N_sum, F).clone().requires_grad_(True)
    ri = batch_rigid_inputs(batch)
    labels = ri["labels"]
    out = {"buffers": {}}
    yc, out["buffers"]["pc_classifier.0.running_mean"], out["buffers"]["pc_classifier.0.running_var"] = _tc.bn_train(
        feats, p["pc_classifier.0.weight"], p["pc_classifier.0.bias"], buf["pc_classifier.0.running_mean"], buf["pc_classifier.0.running_var"])
    hc = torch.relu(yc) if relu_masks is None else yc * torch.as_tensor(relu_masks[0]).to(dtype)
    logits = hc @ p["pc_classifier.2.weight"].reshape(-1) + p["pc_classifier.2.bias"].reshape(())
    gt = torch.from_numpy(labels.reshape(-1))
    cls_loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, gt.to(dtype))
    out.update(cls_loss=cls_loss.detach(), logits=logits.detach(), pre_cls=yc.detach())
    n_sum = labels.sum(1)
    N_ = int(n_sum.max())
    gtp, pp = t(batch["gt_pcs"]), t(part_pcs)
    crit = torch.cat([torch.cat([feats[b * N_sum:(b + 1) * N_sum][torch.from_numpy(labels[b])],
                                 torch.zeros(N_ - int(n_sum[b]), F, dtype=dtype)]) for b in range(B)])
    ya, out["buffers"]["affinity_extractor.0.running_mean"], out["buffers"]["affinity_extractor.0.running_var"] = _tc.bn_train(
        crit, p["affinity_extractor.0.weight"], p["affinity_extractor.0.bias"], buf["affinity_extractor.0.running_mean"],
        buf["affinity_extractor.0.running_var"])
    ha = torch.relu(ya) if relu_masks is None else ya * torch.as_tensor(relu_masks[1]).to(dtype)
    af = ha @ p["affinity_extractor.2.weight"].reshape(512, 128).T + p["affinity_extractor.2.bias"]
    af = torch.cat([torch.nn.functional.normalize(af[:, :256], p=2, dim=-1), torch.nn.functional.normalize(af[:, 256:], p=2, dim=-1)], -1)
    total = torch.zeros((), dtype=dtype)
    out["targets"], out["ds_mat"] = [], []
    mats = []
    for b in range(B):
        n = int(n_sum[b])
        fb = af[b * N_:b * N_ + n]
        s = (fb[:, :256] @ p["affinity_layer.A"]) @ fb[:, 256:].T
        P = torch.exp(_tc.sinkhorn_log(s, tau, max_iter))
        tgt = _tc.gt_targets(gtp[b][torch.from_numpy(labels[b])], ri["row_piece"][b])
        total = total + _tc.perm_loss_sum(P, tgt)
        out["targets"].append(tgt); out["ds_mat"].append(P.detach()); mats.append(P)
    n_all = int(n_sum.sum())
    mat_loss = total / n_all if n_all else total
    rig = rigid_reference(mats, [pp[b][torch.from_numpy(labels[b])] for b in range(B)], ri["counts"], ri["n_valid"], poses=poses, dtype=dtype)
    loss = w_cls * cls_loss + w_mat * mat_loss + w_rig * rig["term"]
    loss.backward()
    rig["term"] = rig["term"].detach()
    out.update(mat_loss=mat_loss.detach(), rig_loss=rig["term"], rigid=rig, N_=N_, pre_aff=ya.detach(), loss=loss.detach(),
               grads={k: v.grad for k, v in p.items()}, d_part_feats=feats.grad, params={k: v.detach() for k, v in p.items()})
    return out
