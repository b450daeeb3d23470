"""Inputs and the torch restatement of the matcher's encoder TRAINING tests (no test in here).  The weights, puzzles and sampling
starts are those of tests/matching_encoder_cases.py, loaded by path and left untouched; here are the extra case `solo`, the seeded
dout of loss = sum(out dout), the indices of a call computed on the CPU with the semantics of the golden tool's stand-ins, and
`restate`: PointNet2PTMSGDynamic in .train() (Jigsaw_matching/model/modules/encoder/pointnet2_pointwise/pointnet2_msg.py:67-94,
pointnet2_dynamic_utils.py:105-157 and :171-223) written out in torch under autograd, in a given dtype, on GIVEN indices.

The restatement can be handed the ReLU patterns and the max-pool winners of another run (the GPU's float32 one) in place of its own
decisions, and `mutate` names deliberate misreadings that the host test shows to leave the fixture:
  "dup16"       the statistics of a K = 16 scale taken over a pool of 32 rows (each row twice, the eval path's fill-up);
  "unbiased"    the unbiased variance in the normalisation;
  "drop_padded" the padded interpolation slots (j >= count) dropped from the backward;
  "drop_points1" the gradient path of l2_points through fp3's points1 dropped.
Pool ties: exact duplicates among a pool's rows tie exactly and which one wins changes no gradient, so the restatement takes the first."""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("matching_encoder_cases", Path(__file__).resolve().parent / "matching_encoder_cases.py")
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

NSAMPLE = base.NSAMPLE
SOLO_LENGTHS = (200,)
# the seeds of the puzzles that are not the base file's: chosen so that the reference's float32 run differs from its float64 run in
# at most FLIP_CAP of a layer's ReLU signs and pool winners (tools/make_matching_encoder_train_goldens.py prints the share)
POINT_SEED = {(100, 20, 340): 213, SOLO_LENGTHS: 214}
_PUZZLES = {}
# name -> list of puzzles (lists of piece lengths); "both" = small + second in one call
CASES = {"small": [base.CASES["small"][0]], "second": [base.CASES["second"][0]], "solo": [list(SOLO_LENGTHS)],
         "both": [base.CASES["small"][0], base.CASES["second"][0]]}
FIXTURE_CASES = ("small", "second", "solo")
DOUT_SEED = {"small": 301, "second": 302, "solo": 303, "both": 304}
MUTATIONS = ("dup16", "unbiased", "drop_padded", "drop_points1")
FLIP_CAP = 1e-4                      # at most 1 differing ReLU sign (pool winner) per 10,000 per layer: the cap of DESIGN.md 5.9


def make_case(name: str) -> list:
    """the puzzles of a case: dicts of points float32 [N, 3], lengths int64 [P], start int64 [4, P].  `small` is the base file's puzzle;
    the others have their own seed (POINT_SEED) and are built with the base file's patch generator, by make_puzzle's statements"""
    out = []
    for lengths in CASES[name]:
        key = tuple(int(n) for n in lengths)
        if key not in POINT_SEED:
            out.append(base.make_puzzle(key))
            continue
        if key not in _PUZZLES:
            rng = np.random.default_rng([23, POINT_SEED[key]])
            pts = [base._patch(rng, n) for n in key]
            for p in pts:
                assert base.min_pairwise_distance(p) >= base.MIN_DIST
            counts = base.level_counts(key)
            start = np.stack([np.where(counts[l] > 1, rng.integers(1, np.maximum(counts[l], 2)), 0) for l in range(4)]).astype(np.int64)
            _PUZZLES[key] = {"points": np.concatenate(pts), "lengths": np.asarray(key, dtype=np.int64), "start": start}
        out.append(_PUZZLES[key])
    return out


def flat_case(name: str):
    """-> (points float32 [N, 3], lengths int64 [P], start int64 [P, 4]) of the whole call"""
    pz = make_case(name)
    return (np.concatenate([p["points"] for p in pz]), np.concatenate([p["lengths"] for p in pz]),
            np.ascontiguousarray(np.concatenate([p["start"] for p in pz], 1).T))


def make_dout(name: str, n: int) -> np.ndarray:
    return np.random.default_rng([29, DOUT_SEED[name]]).normal(0, 1, (n, base.FEAT_OUT)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ indices on the CPU
def _d2(q, p):
    d = q[:, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def cpu_indices(points: np.ndarray, lengths: np.ndarray, start: np.ndarray) -> dict:
    """the index results of a call in float32, with the semantics the golden tool's stand-ins state (farthest points from `start`
    [P, 4], k nearest of the same piece ascending with ties to the lower index, missing slots = the first): per level l = 0 .. 3
    cen[l] int64 [S] (into level l), knn[l] int64 [S, 32] (into level l), back[l] = (idx int64 [N_l, 3] into level l + 1, count) or None
    when level l + 1 has one point in the whole call"""
    counts = base.level_counts(lengths)
    xyz = [points.astype(np.float32)]
    out = {"cen": [], "knn": [], "back": [], "counts": counts}
    for l in range(4):
        lo = np.concatenate([[0], np.cumsum(counts[l])])
        cen = []
        for p in range(len(lengths)):
            q = xyz[l][lo[p]:lo[p + 1]]
            dist = np.full(len(q), np.inf, dtype=np.float32)
            cur = int(start[p, l])
            for _ in range(int(counts[l + 1][p])):
                cen.append(lo[p] + cur)
                d = q - q[cur]
                dist = np.minimum(dist, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                cur = int(np.argmax(dist))
        cen = np.asarray(cen, dtype=np.int64)
        out["cen"].append(cen)
        xyz.append(xyz[l][cen])
    for l in range(4):
        lo, lo2 = np.concatenate([[0], np.cumsum(counts[l])]), np.concatenate([[0], np.cumsum(counts[l + 1])])
        knn = np.zeros((int(counts[l + 1].sum()), 32), dtype=np.int64)
        back = np.zeros((int(counts[l].sum()), 3), dtype=np.int64)
        cnt = np.zeros(int(counts[l].sum()), dtype=np.int64)
        for p in range(len(lengths)):
            pts, ctr = xyz[l][lo[p]:lo[p + 1]], xyz[l + 1][lo2[p]:lo2[p + 1]]
            order = np.argsort(_d2(ctr, pts), axis=1, kind="stable")[:, :32] + lo[p]
            knn[lo2[p]:lo2[p + 1]] = np.concatenate([order, np.repeat(order[:, :1], 32 - order.shape[1], 1)], 1)
            order = np.argsort(_d2(pts, ctr), axis=1, kind="stable")[:, :3] + lo2[p]
            back[lo[p]:lo[p + 1]] = np.concatenate([order, np.repeat(order[:, :1], 3 - order.shape[1], 1)], 1)
            cnt[lo[p]:lo[p + 1]] = order.shape[1]
        out["knn"].append(knn)
        out["back"].append((back, cnt) if counts[l + 1].sum() > 1 else None)
    return out


# ------------------------------------------------------------------------------------------------------------------ the restatement
def layer_names() -> list:
    """[(name, conv prefix, BatchNorm prefix)] of the 33 convolutions in front of a BatchNorm, in forward order"""
    out = []
    for name, _, scales in base.SA:
        for k, widths in enumerate(scales):
            out += [(f"{name}.{k}.{j}", f"{name}.conv_blocks.{k}.{j}", f"{name}.bn_blocks.{k}.{j}") for j in range(len(widths))]
    for name, _, widths in base.FP:
        out += [(f"{name}.{j}", f"{name}.mlp_convs.{j}", f"{name}.mlp_bns.{j}") for j in range(len(widths))]
    return out


POOLED = tuple(f"{name}.{k}.2" for name, _, _ in base.SA for k in range(2))


def restate(sd: dict, points: np.ndarray, idx: dict, dout: np.ndarray, dtype=torch.float64, relu: dict = None, winner: dict = None,
            mutate: str = None) -> dict:
    """one training forward + backward of loss = sum(out dout).  sd: numpy state dict under the reference's names; idx: cpu_indices' layout
    (numpy or torch, any device's values); relu: name -> bool [rows, C] pattern (for a pooled layer [S, C], of the pooled output),
    winner: name -> int [S, C] (-1 = none positive) replacing the restatement's own decisions.  -> {"out", "l1_points" .. "l4_points",
    "grad": {parameter: gradient}, "buffers": {running_mean / running_var / num_batches_tracked after the step}, "relu", "winner"}"""
    assert mutate in (None,) + MUTATIONS
    t = lambda a: torch.as_tensor(np.asarray(a))
    prm = {k: t(v).to(dtype).requires_grad_(True) for k, v in sd.items() if k.rsplit(".", 1)[1] in ("weight", "bias")}
    buffers, pat_relu, pat_win = {}, {}, {}
    eps, mom = 1e-5, 0.1

    def layer(name, cp, bp, a, K=0, stat_rows=None):
        """a [rows, C_in] -> relu(bn(conv)) [rows, C_out], or its max over groups of K rows.  stat_rows: the rows the statistics see"""
        w = prm[cp + ".weight"]
        y = a @ w.reshape(w.shape[0], -1).t() + prm[cp + ".bias"]
        ys = y if stat_rows is None else y[stat_rows]
        n = ys.shape[0]
        mean, var = ys.mean(0), ys.var(0, unbiased=False)
        norm_var = var * n / (n - 1) if mutate == "unbiased" else var
        z = (y - mean) / torch.sqrt(norm_var + eps) * prm[bp + ".weight"] + prm[bp + ".bias"]
        buffers[bp + ".running_mean"] = ((1 - mom) * t(sd[bp + ".running_mean"]).to(dtype) + mom * mean).detach()
        buffers[bp + ".running_var"] = ((1 - mom) * t(sd[bp + ".running_var"]).to(dtype) + mom * var * n / (n - 1)).detach()
        buffers[bp + ".num_batches_tracked"] = t(sd[bp + ".num_batches_tracked"]) + 1
        if not K:
            if relu is not None:
                m = t(relu[name]).to(torch.bool)
                pat_relu[name] = m
                return z * m.to(dtype)
            h = torch.relu(z)
            pat_relu[name] = (h > 0).detach()
            return h
        zg = z.reshape(-1, K, z.shape[1])
        if winner is not None:
            win = t(winner[name]).long()
            sel = torch.gather(zg, 1, win.clamp(min=0)[:, None, :])[:, 0]
            m = t(relu[name]).to(torch.bool)
            pat_relu[name], pat_win[name] = m, win
            return sel * m.to(dtype)
        hg = torch.relu(zg)
        win = hg.argmax(1)                                   # the first of the maximal rows
        pooled = torch.gather(hg, 1, win[:, None, :])[:, 0]
        pat_relu[name] = (pooled > 0).detach()
        pat_win[name] = torch.where(pooled > 0, win, torch.full_like(win, -1))
        return pooled

    x = t(points).to(dtype)
    xyz, feats = [x], [x]
    cen = [t(c).long() for c in idx["cen"]]
    for l in range(4):
        xyz.append(xyz[l][cen[l]])
    for l, (name, _, scales) in enumerate(base.SA):
        outs = []
        g32 = t(idx["knn"][l]).long()
        for k, K in enumerate(NSAMPLE):
            g = g32[:, :K]
            stat_rows = None
            if mutate == "dup16" and K == 16:                # a pool of 32 rows per centroid, slot j reads neighbour j mod 16
                g = torch.cat([g, g], 1)
            rows = torch.cat([feats[l][g], xyz[l][g] - xyz[l + 1][:, None, :]], -1).reshape(-1, feats[l].shape[1] + 3)
            a = rows
            for j in range(3):
                nm = f"{name}.{k}.{j}"
                kk = g.shape[1] if j == 2 else 0
                if mutate == "dup16" and K == 16 and (relu is not None or winner is not None):
                    raise ValueError("dup16 runs on the restatement's own decisions")
                a = layer(nm, f"{name}.conv_blocks.{k}.{j}", f"{name}.bn_blocks.{k}.{j}", a, kk, stat_rows)
            outs.append(a)
        feats.append(torch.cat(outs, 1))
    up = feats[4]
    levels = {f"l{l}_points": feats[l].detach() for l in range(1, 5)}
    for l, (name, _, widths) in zip((3, 2, 1, 0), base.FP):
        p1 = feats[l] if l > 0 else None
        if mutate == "drop_points1" and name == "fp3":
            p1 = p1.detach()
        if idx["back"][l] is None:
            interp = up.repeat(xyz[l].shape[0], 1)
        else:
            b3, cnt = t(idx["back"][l][0]).long(), t(idx["back"][l][1]).long()
            a_, b_ = xyz[l][:, None, :], xyz[l + 1][b3]
            d = (a_ ** 2 + b_ ** 2 - 2 * a_ * b_).sum(-1)
            real = torch.arange(3)[None, :] < cnt[:, None]
            d = torch.where(real, d, torch.full_like(d, 1e8))
            r = 1.0 / (d + 1e-8)
            w = r / r.sum(1, keepdim=True)
            src = up[b3]
            if mutate == "drop_padded":
                src = torch.where(real[:, :, None], src, src.detach())
            interp = (src * w[:, :, None]).sum(1)
        a = interp if p1 is None else torch.cat([p1, interp], 1)
        for j in range(len(widths)):
            a = layer(f"{name}.{j}", f"{name}.mlp_convs.{j}", f"{name}.mlp_bns.{j}", a)
        up = a
        levels[f"{name}_out"] = up.detach()
    w1 = prm["conv1.weight"]
    out = up @ w1.reshape(w1.shape[0], -1).t() + prm["conv1.bias"]
    loss = (out * t(dout).to(dtype)).sum()
    loss.backward()
    return {"out": out.detach(), **levels, "grad": {k: v.grad for k, v in prm.items()}, "buffers": buffers, "relu": pat_relu, "winner": pat_win,
            "loss": loss.detach()}


# ------------------------------------------------------------------------------------------------------------------ the fixture's samples
STEP = 3


def sample(a: np.ndarray) -> dict:
    """what the fixture keeps of a float64 tensor: of a vector every 3rd element; of a matrix every 3rd row sum and column sum (each sum
    runs over ALL elements of its row / column) and every 3rd element of every n-th row with n = the row count, that is of row 0.  The
    1.9 M parameter gradients of three cases do not fit a fixture in float64, not even their 5,864-channel vectors in full: the step
    keeps the file under 600 KB"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim <= 1:
        return {"full": a.reshape(-1)[::STEP]}
    a = a.reshape(a.shape[0], -1)
    return {"rowsum": a.sum(1)[::STEP], "colsum": a.sum(0)[::STEP], "rows": a[::a.shape[0], ::STEP]}


def fixture_tensors(res: dict) -> dict:
    """name -> array of everything a run is compared on: the descriptors, the level outputs, the gradients and the running buffers"""
    out = {"out": res["out"], **{k: res[k] for k in ("l1_points", "l2_points", "l3_points", "l4_points")}}
    out.update({"grad." + k: v for k, v in res["grad"].items()})
    out.update({"buf." + k: v for k, v in res["buffers"].items() if not k.endswith("num_batches_tracked")})
    return {k: np.asarray(v.detach().double().numpy() if torch.is_tensor(v) else v, dtype=np.float64) for k, v in out.items()}


def pack_samples(tensors: dict) -> dict:
    """{tensor: array} -> the three arrays a case's samples are stored as: keys "tensor/kind", their sizes and the values end to end
    (one archive member per sample would cost more than the samples)"""
    keys, sizes, data = [], [], []
    for name in sorted(tensors):
        for kind, arr in sample(tensors[name]).items():
            keys.append(f"{name}/{kind}")
            sizes.append(arr.size)
            data.append(arr.reshape(-1))
    return {"keys": np.asarray(keys), "sizes": np.asarray(sizes, dtype=np.int64), "data": np.concatenate(data)}


def load_fixture(case: str) -> dict:
    """-> {"samples": {"tensor/kind": float64 array}, "refdev": {tensor: float}, "max": {tensor: float}, "flips": {layer: (differing,
    elements)}, "winflips": {pooled layer: (differing, elements)}}"""
    z = np.load(Path(__file__).resolve().parent / "golden" / "matching_encoder_train.npz")
    assert int(z["step"]) == STEP
    ends = np.cumsum(z[f"{case}_sizes"])
    data = z[f"{case}_data"]
    samples = {str(k): data[e - n:e] for k, n, e in zip(z[f"{case}_keys"], z[f"{case}_sizes"], ends)}
    tensors = [str(t) for t in z[f"{case}_tensors"]]
    return {"samples": samples, "refdev": dict(zip(tensors, z[f"{case}_refdev"].tolist())), "max": dict(zip(tensors, z[f"{case}_max"].tolist())),
            "flips": {str(n): tuple(int(v) for v in r) for n, r in zip(z["layers"], z[f"{case}_flips"])},
            "winflips": {str(n): tuple(int(v) for v in r) for n, r in zip(z["pooled"], z[f"{case}_winflips"])}}
