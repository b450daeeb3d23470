"""Seeded inputs and the float64 reference of the matcher head's training step (no test in here).

The reference of record is `head_train_reference`: a float64 torch restatement of the training-time forward of
JointSegmentationAlignmentModel behind part_feats (joint_seg_align_model.py:164-268 in .train()) and of _loss_function (:280-426),
run under autograd on the CPU.  tools/make_matching_train_goldens.py feeds the same inputs to the reference's own code and stores
what it returns in tests/golden/matching_train.npz; tests/test_matching_train_host.py pins the restatement to that file.  The inputs
are regenerated here from seeds, so the fixture holds results only.

Inputs.  The head's weights are matching_cases.head_state_dict().  A batch is B puzzles of EQUAL point count (the reference stacks
them to [B, N_sum, .]) and unequal numbers of critical points, so the zero padding of critical_feats up to the largest N' enters the
affinity extractor's BatchNorm statistics.  Descriptors are built like matching_cases.build_puzzle's, but with match cosines of
0.15 - 0.35: near-saturated matrices (entries of 1 - 1e-6) make the BCE gradient 1 / (1 - P) and the reference's own fp32 run then
misses float64 by percents, so a bar derived from it would mean nothing.  Every ds_mat entry stays at or below 0.97 (asserted by the
fixture tool)."""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("matching_cases", Path(__file__).resolve().parent / "matching_cases.py")
_mc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mc)

TAU, MAX_ITER = 0.05, 20
EPS = 1e-5
MOMENTUM = 0.1
P_MAX = 20
SAMPLE = 37                # stride of the stored gradient samples of the whole step (flattened tensor)
SINKHORN_SAMPLE = {3: 1, 65: 7, 257: 53, 1033: 997}          # the same for the n x n matrices of the Sinkhorn cases
DS_MAX = 0.97              # every ds_mat entry of every case stays at or below this
head_state_dict = _mc.head_state_dict

# name -> per puzzle (points per piece, critical points per piece); the puzzles of a batch have the same number of points
BATCHES = {
    # unequal N' (41 and 29): 12 zero rows enter the extractor's BatchNorm; piece 2 of puzzle 0 has no critical point
    "main": [([60, 50, 40, 30], [16, 14, 0, 11]), ([70, 60, 50], [11, 10, 8])],
    # puzzle 1: one piece owns every critical point: all its targets are -1, its loss is sum -log(1 - P)
    "one_owner": [([70, 60, 50], [12, 9, 7]), ([90, 90], [13, 0])],
    # puzzle 1 has no critical point: it contributes nothing (its 23 rows of the padded buffer are all zero rows)
    "empty_puzzle": [([80, 60, 40], [10, 8, 5]), ([100, 80], [0, 0])],
}


def make_batch_without_critical_points() -> dict:
    """`main` with every label 0: no puzzle has a critical point (the fixture holds the reference's classifier phase on it, the only
    part of the step that is defined there)"""
    b = make_batch("main")
    return dict(b, critical_label=np.zeros_like(b["critical_label"]))
SINKHORN_SIZES = (3, 65, 257, 1033)
SINKHORN_ITERS = (1, 2, 7, 20)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_batch(name: str, seed: int = 11) -> dict:
    """-> part_feats float32 [B, N_sum, 128], gt_pcs float32 [B, N_sum, 3], n_pcs int64 [B, 20], part_valids float32 [B, 20],
    critical_label int64 [B, N_sum], thresholds float32 [B, N_sum] (not used by the fixture: the labels are given)"""
    spec = BATCHES[name]
    sd = head_state_dict()
    g, b_, m, v = (sd[f"affinity_extractor.0.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    out = {k: [] for k in ("part_feats", "gt_pcs", "n_pcs", "part_valids", "critical_label", "thresholds")}
    L = _mc.LATENT
    for b, (sizes, ncrit) in enumerate(spec):
        rng = np.random.default_rng([seed, sorted(BATCHES).index(name), b])
        N = sum(sizes)
        start = np.cumsum(sizes) - np.asarray(sizes)
        piece = np.repeat(np.arange(len(sizes)), sizes)
        zp, zd = _unit(rng.normal(size=(N, L))), _unit(rng.normal(size=(N, L)))
        critical = np.zeros(N, dtype=bool)
        for p, (n, c) in enumerate(zip(sizes, ncrit)):
            critical[start[p] + rng.permutation(n)[:c]] = True
        gt = rng.uniform(0, 0.3, (N, 3))
        gt[:, 0] += 0.3 * piece
        # a soft match: the dual descriptor of the nearest critical point of another piece leans towards the row's primal one
        rows = np.nonzero(critical)[0]
        for i in rows:
            other = rows[piece[rows] != piece[i]]
            if other.size:
                j = other[np.argmin(((gt[other] - gt[i]) ** 2).sum(1))]
                c = rng.uniform(0.15, 0.35)
                zd[j] = _unit(zd[j] + c * zp[i])
        y = np.empty((N, 128))
        y[:, 0:L], y[:, L:2 * L], y[:, 2 * L:3 * L], y[:, 3 * L:4 * L] = zp, -zp, zd, -zd
        t = rng.uniform(0.2, 1.0, N)
        flip = rng.uniform(size=N) < 0.15                      # the classifier is wrong on some points: all four confusion counts occur
        seen = critical ^ flip
        y[:, 124] = np.where(seen, t, -0.5)
        y[:, 125] = np.where(seen, -0.5, t)
        y[:, 126:] = 0.05 * rng.normal(size=(N, 2))
        x = (y - b_) * np.sqrt(v + EPS) / g + m
        n_pcs = np.zeros(P_MAX, dtype=np.int64)
        n_pcs[:len(sizes)] = sizes
        pv = np.zeros(P_MAX, dtype=np.float32)
        pv[:len(sizes)] = 1
        out["part_feats"].append(x.astype(np.float32)); out["gt_pcs"].append(gt.astype(np.float32)); out["n_pcs"].append(n_pcs)
        out["part_valids"].append(pv); out["critical_label"].append(critical.astype(np.int64))
        out["thresholds"].append(rng.uniform(0.02, 0.08, N).astype(np.float32))
    return {k: np.stack(v) for k, v in out.items()}


def sinkhorn_case(n: int, seed: int = 5):
    """-> s float32 [n, n] (affinities: noise plus one planted entry per row, scaled down for tiny n so that nothing saturates),
    tgt int32 [n] (the planted column; every seventh row -1)"""
    rng = np.random.default_rng([seed, n])
    noise, lo, hi = (0.02, 0.08, 0.12) if n < 16 else (0.05, 0.12, 0.26)
    s = noise * rng.normal(size=(n, n))
    tgt = rng.permutation(n)
    s[np.arange(n), tgt] += rng.uniform(lo, hi, n)
    tgt = tgt.astype(np.int32)
    tgt[::7] = -1
    return s.astype(np.float32), tgt


# ------------------------------------------------------------------------------------------------------------------ float64 pieces
def sinkhorn_log(s: torch.Tensor, tau: float = TAU, max_iter: int = MAX_ITER) -> torch.Tensor:
    """the per-sample branch of utils/linear_solvers.py:188-207 for a full (unpadded, unmasked) matrix: log of ds_mat"""
    log_s = s / tau
    for i in range(max_iter):
        log_s = log_s - torch.logsumexp(log_s, 1 if i % 2 == 0 else 0, keepdim=True)
    return log_s


def perm_loss_rows(P: torch.Tensor, tgt) -> torch.Tensor:
    """the rows' shares of F.binary_cross_entropy(P, gt_perm, reduction='sum') (utils/loss.py:51) for gt_perm[i, tgt_i] = 1
    (tgt_i >= 0), both logs clamped at -100: [n]"""
    tgt = torch.as_tensor(np.asarray(tgt), dtype=torch.int64)
    y = torch.zeros_like(P)
    rows = torch.nonzero(tgt >= 0).reshape(-1)
    y[rows, tgt[rows]] = 1
    return -(y * torch.log(P).clamp_min(-100) + (1 - y) * torch.log(1 - P).clamp_min(-100)).sum(1)


def perm_loss_sum(P: torch.Tensor, tgt) -> torch.Tensor:
    return perm_loss_rows(P, tgt).sum()


def sinkhorn_loss_and_grad(s, tgt, tau: float = TAU, max_iter: int = MAX_ITER, g: float = 1.0, dtype=torch.float64):
    """autograd of g * perm_loss_sum(exp(sinkhorn_log(s))) -> (ds_mat, loss (unscaled), dLoss / ds)"""
    s = torch.as_tensor(np.asarray(s)).to(dtype).requires_grad_(True)
    P = torch.exp(sinkhorn_log(s, tau, max_iter))
    loss = perm_loss_sum(P, tgt)
    (loss * g).backward()
    return P.detach(), loss.detach(), s.grad


def sinkhorn_closed_form(s, tgt, tau: float = TAU, max_iter: int = MAX_ITER, g: float = 1.0):
    """the recurrence the kernels run, in float64: potentials kept per step, G = dLoss / d log P updated in place
    -> (ds_mat, loss, dLoss / ds)"""
    s = torch.as_tensor(np.asarray(s)).to(torch.float64)
    tgt = torch.as_tensor(np.asarray(tgt), dtype=torch.int64)
    n = s.shape[0]
    L = s / tau
    u, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pots = []
    for i in range(max_iter):
        X = (L - u[:, None]) - v[None, :]
        if i % 2 == 0:
            u = u + torch.logsumexp(X, 1)
        else:
            v = v + torch.logsumexp(X, 0)
        pots.append((u.clone(), v.clone()))
    P = torch.exp((L - u[:, None]) - v[None, :])
    y = torch.zeros_like(P)
    rows = torch.nonzero(tgt >= 0).reshape(-1)
    y[rows, tgt[rows]] = 1
    loss = perm_loss_sum(P, tgt)
    G = (P - y) * P / (P * (1 - P)).clamp_min(1e-12) * g
    for i in range(max_iter - 1, -1, -1):
        ui, vi = pots[i]
        Pi = torch.exp((L - ui[:, None]) - vi[None, :])
        G = G - Pi * (G.sum(1, keepdim=True) if i % 2 == 0 else G.sum(0, keepdim=True))
    return P, loss, G / tau


def gt_targets(gt_crit: torch.Tensor, piece_of_row: np.ndarray, return_gap: bool = False):
    """joint_seg_align_model.py:333-364 for one puzzle in the dtype of gt_crit [n, 3]: the column of the nearest critical point of
    another piece (-1 when there is none); gap = (second smallest - smallest) distance per row, to tell near-ties"""
    n = gt_crit.shape[0]
    if n == 0:
        return (np.zeros(0, np.int32), np.zeros(0)) if return_gap else np.zeros(0, np.int32)
    d = -2 * gt_crit @ gt_crit.T
    d = d + (gt_crit ** 2).sum(-1)[:, None]
    d = d + (gt_crit ** 2).sum(-1)[None, :]
    d = d.clamp_min(1e-12)
    same = torch.from_numpy(piece_of_row[:, None] == piece_of_row[None, :])
    d = d.masked_fill(same, float("inf"))
    tgt = torch.argmin(d, 1).numpy().astype(np.int32)
    none = same.all(1).numpy()
    tgt[none] = -1
    if not return_gap:
        return tgt
    top = torch.topk(d, min(2, n), dim=1, largest=False).values
    gap = (top[:, -1] - top[:, 0]).numpy() if n > 1 else np.full(n, np.inf)
    return tgt, gap


def bn_train(x, gamma, beta, running_mean, running_var):
    """nn.BatchNorm1d in .train(): batch statistics over the rows; -> (y, new running_mean, new running_var (unbiased))"""
    n = x.shape[0]
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    y = (x - mean) / torch.sqrt(var + EPS) * gamma + beta
    with torch.no_grad():
        rm = (1 - MOMENTUM) * running_mean + MOMENTUM * mean
        rv = (1 - MOMENTUM) * running_var + MOMENTUM * var * (n / max(n - 1, 1))
    return y, rm, rv


PARAMS = ("pc_classifier.0.weight", "pc_classifier.0.bias", "pc_classifier.2.weight", "pc_classifier.2.bias", "affinity_extractor.0.weight",
          "affinity_extractor.0.bias", "affinity_extractor.2.weight", "affinity_extractor.2.bias", "affinity_layer.A")
BUFFERS = ("pc_classifier.0.running_mean", "pc_classifier.0.running_var", "affinity_extractor.0.running_mean",
           "affinity_extractor.0.running_var")


def head_train_reference(sd: dict, batch: dict, *, w_cls: float = 1.0, w_mat: float = 1.0, relu_masks=None, dtype=torch.float64,
                         tau: float = TAU, max_iter: int = MAX_ITER) -> dict:
    """one training forward + loss + backward of the head.  sd: name -> array / tensor (the reference's names); batch: make_batch's
    dict (labels given).  relu_masks = (classifier mask bool [B N_sum, 128], extractor mask bool [B N'_max, 128]): the ReLUs take
    these instead of their own sign test (a float64 run fed the GPU's masks).
    -> loss, cls_loss, mat_loss, counts (tp, fp, tn, fn), N_, targets (list per puzzle), ds_mat (list), grads {name: tensor},
    d_part_feats [B N_sum, 128], buffers {name: tensor}, pre-activations (the two BatchNorm outputs, for the mask margin)"""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype) if not torch.is_tensor(a) else a.detach().to(dtype)
    p = {k: t(sd[k]).clone().requires_grad_(True) for k in PARAMS}
    buf = {k: t(sd[k]) for k in BUFFERS}
    x = t(batch["part_feats"])
    B, N_sum, F = x.shape
    feats = x.reshape(B * N_sum, F).clone().requires_grad_(True)
    labels = np.asarray(batch["critical_label"]).reshape(B, N_sum) != 0
    n_pcs = np.asarray(batch["n_pcs"]).astype(np.int64)
    out = {"buffers": {}}
    # ---- classifier over all B N_sum points
    yc, out["buffers"]["pc_classifier.0.running_mean"], out["buffers"]["pc_classifier.0.running_var"] = bn_train(
        feats, p["pc_classifier.0.weight"], p["pc_classifier.0.bias"], buf["pc_classifier.0.running_mean"], buf["pc_classifier.0.running_var"])
    hc = torch.relu(yc) if relu_masks is None else yc * torch.as_tensor(relu_masks[0]).to(dtype)
    logits = hc @ p["pc_classifier.2.weight"].reshape(-1) + p["pc_classifier.2.bias"].reshape(())
    gt = torch.from_numpy(labels.reshape(-1))
    cls_loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, gt.to(dtype))
    pred = torch.sigmoid(logits.detach()) > 0.5
    out["counts"] = np.asarray([int((pred & gt).sum()), int((pred & ~gt).sum()), int((~pred & ~gt).sum()), int((~pred & gt).sum())], dtype=np.int64)
    out.update(cls_loss=cls_loss.detach(), logits=logits.detach(), pre_cls=yc.detach())
    if w_mat == 0:                                   # joint_seg_align_model.py:221-223, :325-327: the classifier phase
        loss = cls_loss
        out.update(mat_loss=None, N_=None, targets=None, ds_mat=None, pre_aff=None)
    else:
        n_sum = labels.sum(1)
        N_ = int(n_sum.max())
        gtp = t(batch["gt_pcs"])
        crit = torch.cat([torch.cat([feats[b * N_sum:(b + 1) * N_sum][torch.from_numpy(labels[b])],
                                     torch.zeros(N_ - int(n_sum[b]), F, dtype=dtype)]) for b in range(B)])       # [B N_, F] with the zero rows
        ya, out["buffers"]["affinity_extractor.0.running_mean"], out["buffers"]["affinity_extractor.0.running_var"] = bn_train(
            crit, p["affinity_extractor.0.weight"], p["affinity_extractor.0.bias"], buf["affinity_extractor.0.running_mean"],
            buf["affinity_extractor.0.running_var"])
        ha = torch.relu(ya) if relu_masks is None else ya * torch.as_tensor(relu_masks[1]).to(dtype)
        af = ha @ p["affinity_extractor.2.weight"].reshape(512, 128).T + p["affinity_extractor.2.bias"]
        af = torch.cat([torch.nn.functional.normalize(af[:, :256], p=2, dim=-1), torch.nn.functional.normalize(af[:, 256:], p=2, dim=-1)], -1)
        total = torch.zeros((), dtype=dtype)
        out["targets"], out["ds_mat"] = [], []
        for b in range(B):
            n = int(n_sum[b])
            fb = af[b * N_:b * N_ + n]
            s = (fb[:, :256] @ p["affinity_layer.A"]) @ fb[:, 256:].T
            P = torch.exp(sinkhorn_log(s, tau, max_iter))
            piece = np.repeat(np.arange(n_pcs.shape[1]), n_pcs[b])[labels[b]]
            tgt = gt_targets(gtp[b][torch.from_numpy(labels[b])], piece)
            total = total + perm_loss_sum(P, tgt)
            out["targets"].append(tgt); out["ds_mat"].append(P.detach())
        n_all = int(n_sum.sum())
        mat_loss = total / n_all if n_all else total          # the reference divides 0 by 0 there; the engine reports 0
        loss = w_cls * cls_loss + w_mat * mat_loss
        out.update(mat_loss=mat_loss.detach(), N_=N_, pre_aff=ya.detach())
    loss.backward()
    out["loss"] = loss.detach()
    out["grads"] = {k: (v.grad if v.grad is not None else None) for k, v in p.items()}
    out["d_part_feats"] = feats.grad
    out["params"] = {k: v.detach() for k, v in p.items()}
    return out


def adam_steps(params: dict, grads_per_step, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
    """torch.optim.Adam (weight_decay 0) in float64 over a list of gradient dicts -> list of parameter dicts after each step; a
    parameter whose gradient is None is left alone, as the optimizer leaves it"""
    p = {k: v.clone().double() for k, v in params.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    s = {k: torch.zeros_like(v) for k, v in p.items()}
    steps = {k: 0 for k in p}
    outs = []
    for grads in grads_per_step:
        for k, g in grads.items():
            if g is None:
                continue
            g = g.double()
            steps[k] += 1
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g
            s[k] = betas[1] * s[k] + (1 - betas[1]) * g * g
            denom = s[k].sqrt() / np.sqrt(1 - betas[1] ** steps[k]) + eps
            p[k] = p[k] - lr / (1 - betas[0] ** steps[k]) * m[k] / denom
        outs.append({k: v.clone() for k, v in p.items()})
    return outs
