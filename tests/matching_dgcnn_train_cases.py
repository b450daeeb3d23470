"""Cases of the DGCNN encoder's training step (pfpp_hip/matching_dgcnn_train.py, csrc/dgcnn_train.hip): seeded inputs and the
restatements the tests compare against.  Loaded by path from the tests and from tools/make_matching_dgcnn_train_goldens.py; imports
nothing of the product (the forward case file tests/matching_dgcnn_cases.py is loaded by path for the weights and the search).

* case_arrays / dout_array: points of a few pieces and the seeded d loss / d out of loss = sum(out * dout).
* train_step: the reference's DGCNNDynamic in .train() at any dtype, forward + backward + the moved running buffers, in two forms:
  "direct" builds [N, 20, 2 C] and runs under autograd (the reference's own graph); "decomposed" is the arithmetic the kernels compute,
  written out by hand (level_forward / level_backward), with no autograd and nothing of size [N, 20, 2 C].  Both accept given
  neighbour lists and given winners.
* stats_extremum_f32 / apply_f32: pfpp_dgcnn_edge_stats' e, winner and sums and pfpp_dgcnn_bn_leaky_apply in numpy, operation by operation.
* stats_case / gather_lists: inputs of the kernel tests (a padded 0 that wins both extrema, a piece of one point, a first-slot tie;
  a star-shaped piece whose centre is in every list).
"""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location("matching_dgcnn_cases", Path(__file__).resolve().parent / "matching_dgcnn_cases.py")
fwd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fwd)

K, WIDTHS, COL, CAT, FEAT, SLOPE, BN_EPS = fwd.K, fwd.WIDTHS, fwd.COL, fwd.CAT, fwd.FEAT, fwd.SLOPE, fwd.BN_EPS
MOMENTUM = 0.1
MIN_STEP = fwd.MIN_STEP
PARAMS = tuple([f"bn{l}.{leaf}" for l in range(1, 6) for leaf in ("weight", "bias")] + [f"conv{l}.0.weight" for l in range(1, 6)])
BUFFERS = tuple(f"bn{l}.{leaf}" for l in range(1, 6) for leaf in ("running_mean", "running_var"))

# tiny: a piece shorter than K, one that spans two query workgroups, a single point.  small: K - 1, K and K + 1 points next to 1 and 3.
LENGTHS = {"tiny": (5, 23, 70, 1), "small": (1, 3, 19, 20, 21, 70)}
# the seeds tools/make_matching_dgcnn_train_goldens.py settled on: the first from 0 upwards at which the reference's float32 and float64
# .train() runs pick the same neighbour sets at all four levels, no 20th / 21st key pair is closer than MIN_STEP, and both runs pick
# the same winner for every (point, channel) at every level
SEEDS = {"tiny": 2, "small": 0}


def case_arrays(name: str, seed=None):
    """-> (x float32 [N, 3], lengths int64 [P]): every piece a cloud around its own centre"""
    lengths = np.asarray(LENGTHS[name], dtype=np.int64)
    rng = np.random.default_rng([int(SEEDS[name] if seed is None else seed), len(lengths), int(lengths.sum()), 17])
    pieces = [rng.uniform(-0.5, 0.5, (1, 3)) + rng.uniform(-0.25, 0.25, (int(n), 3)) * rng.uniform(0.5, 1.0, (1, 3)) for n in lengths]
    return np.concatenate(pieces).astype(np.float32), lengths


def dout_array(name: str, seed=None, feat_dim: int = FEAT) -> np.ndarray:
    N = int(np.sum(LENGTHS[name]))
    rng = np.random.default_rng([int(SEEDS[name] if seed is None else seed), N, 23])
    return rng.standard_normal((N, feat_dim)).astype(np.float32)


state_dict = fwd.state_dict
feat_knn = fwd.feat_knn


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _leaky(y):
    return torch.where(y > 0, y, y * SLOPE)


# ------------------------------------------------------------------------------------------------------------------ one level, by hand
def level_forward(uv, idx, gamma, beta, eps: float = BN_EPS, winner=None) -> dict:
    """uv float64 tensor [N, 2 C] = [u | v], idx int64 array [N, K] (N = the padded slot) -> the level's train-mode forward:
    z_ij = u[idx_ij] + v[i] (0 for a padded slot), mean / var over all K N rows of z (biased), a = gamma rstd, b = beta - mean a,
    e = max_j z where gamma >= 0 and min_j z where gamma < 0 (the first slot that attains it; `winner` [N, C] overrides the choice),
    x = LeakyReLU(e a + b)"""
    N, C = uv.shape[0], uv.shape[1] // 2
    u, v = uv[:, :C], uv[:, C:]
    it = torch.from_numpy(np.asarray(idx).astype(np.int64))
    real = it != N
    up = torch.cat([u, torch.zeros((1, C), dtype=uv.dtype)], 0)
    z = torch.where(real[..., None], up[it.reshape(-1)].reshape(N, K, C) + v[:, None, :], torch.zeros((), dtype=uv.dtype))     # [N, K, C]
    R = N * K
    mean = z.sum((0, 1)) / R
    var = (z * z).sum((0, 1)) / R - mean * mean
    rstd = 1.0 / torch.sqrt(var + eps)
    a = gamma * rstd
    b = beta - mean * a
    if winner is None:
        zn = z.numpy()
        w = np.where(gamma.numpy()[None, :] >= 0, zn.argmax(1), zn.argmin(1))          # numpy: the first occurrence
    else:
        w = np.asarray(winner).astype(np.int64)
    wt = torch.from_numpy(w)
    e = z.gather(1, wt[:, None, :])[:, 0, :]
    return {"z": z, "real": real, "mean": mean, "var": var, "rstd": rstd, "a": a, "b": b, "e": e, "winner": w, "x": _leaky(e * a + b), "R": R}


def level_backward(uv, idx, fw: dict, g) -> dict:
    """the issue's backward of one level in float64, written out: g = d loss / d x [N, C] -> du, dv [N, C], dgamma, dbeta [C]"""
    N, C = uv.shape[0], uv.shape[1] // 2
    u, v = uv[:, :C], uv[:, C:]
    it = torch.from_numpy(np.asarray(idx).astype(np.int64))
    real, a, mean, rstd, R = fw["real"], fw["a"], fw["mean"], fw["rstd"], fw["R"]
    y = fw["e"] * a + fw["b"]
    h = g * torch.where(y > 0, torch.ones((), dtype=uv.dtype), torch.full((), SLOPE, dtype=uv.dtype))
    dbeta = h.sum(0)
    dgamma = (h * (fw["e"] - mean) * rstd).sum(0)
    m1, m2 = dbeta / R, dgamma / R
    wt = torch.from_numpy(fw["winner"])
    n = real.sum(1).to(uv.dtype)[:, None]                                             # real slots of i
    w_idx = it.gather(1, wt)                                                          # [N, C]: the index in the winning slot
    w_real = w_idx != N
    up = torch.cat([u, torch.zeros((1, C), dtype=uv.dtype)], 0)
    su = up[it.reshape(-1)].reshape(N, K, C).sum(1)                                   # sum over the real slots (padded rows are 0)
    dv = a * (h * w_real.to(uv.dtype) - n * m1 - m2 * rstd * (su + n * (v - mean)))
    # du: scatter over the lists
    cnt = torch.bincount(it.reshape(-1), minlength=N + 1)[:N].to(uv.dtype)[:, None]   # c_p
    hw = torch.zeros((N + 1, C), dtype=uv.dtype)
    hw.index_put_((w_idx.reshape(-1), torch.arange(C).repeat(N)), h.reshape(-1), accumulate=True)
    sv = torch.zeros((N + 1, C), dtype=uv.dtype)
    sv.index_add_(0, it.reshape(-1), v[:, None, :].expand(N, K, C).reshape(N * K, C))
    du = a * (hw[:N] - cnt * m1 - m2 * rstd * (cnt * (u - mean) + sv[:N]))
    return {"du": du, "dv": dv, "dgamma": dgamma, "dbeta": dbeta, "h": h, "m1": m1, "m2": m2}


def split_weight(W):
    """[W_a | W_b] [C, 2 C_in] -> [W_a ; W_b - W_a] [2 C, C_in]"""
    c_in = W.shape[1] // 2
    return torch.cat([W[:, :c_in], W[:, c_in:] - W[:, :c_in]], 0)


# ------------------------------------------------------------------------------------------------------------------ the whole step
def train_step(sd: dict, x, lengths, dout, dtype=torch.float64, indices=None, winners=None, form: str = "direct") -> dict:
    """one .train() forward + backward of DGCNNDynamic(feat_dim, False, 3) with loss = sum(out * dout).  indices: four [N, K] arrays to
    use instead of searching (feat_knn at the dtype's precision); winners: four [N, C_l] slot arrays to use instead of the extremum.
    -> {"knn", "winner" (four slot arrays), "x1" .. "x4", "out", "grads" {15 names}, "buffers" {10 names: the values after the step}}"""
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    X = _t(x, dtype)
    N = X.shape[0]
    G = _t(dout, dtype)
    res = {"knn": [], "winner": [], "grads": {}, "buffers": {}}
    P = {k: _t(sd[k], dtype).clone().requires_grad_(form == "direct") for k in PARAMS}

    def moved(l, mean, var, R):
        rm, rv = _t(sd[f"bn{l}.running_mean"], dtype), _t(sd[f"bn{l}.running_var"], dtype)
        res["buffers"][f"bn{l}.running_mean"] = (rm + MOMENTUM * (mean.detach() - rm)).numpy()
        res["buffers"][f"bn{l}.running_var"] = (rv + MOMENTUM * (var.detach() * R / (R - 1) - rv)).numpy()

    feats, kept = [], []
    for l in range(1, 5):
        idx = np.asarray(indices[l - 1]).astype(np.int64) if indices is not None else feat_knn(X.detach().numpy(), lengths, K, np_dtype)[0]
        res["knn"].append(idx)
        W, gamma, beta = P[f"conv{l}.0.weight"][:, :, 0], P[f"bn{l}.weight"], P[f"bn{l}.bias"]
        given = None if winners is None else winners[l - 1]
        if form == "direct":
            it = torch.from_numpy(idx)
            real = it != N
            c_in = X.shape[1]
            Xp = torch.cat([X, torch.zeros((1, c_in), dtype=dtype)], 0)
            nb = Xp[it.reshape(-1)].reshape(N, K, c_in)
            own = X[:, None, :].expand(N, K, c_in)
            f = torch.cat([nb - own, own], -1) * real[..., None].to(dtype)             # [N, K, 2 C_in]
            z = f @ W.t()                                                             # [N, K, C]
            R = N * K
            mean = z.sum((0, 1)) / R
            var = (z * z).sum((0, 1)) / R - mean * mean
            y = _leaky((z - mean) / torch.sqrt(var + BN_EPS) * gamma + beta)
            if given is None:
                zn = z.detach().numpy()
                w = np.where(gamma.detach().numpy()[None, :] >= 0, zn.argmax(1), zn.argmin(1))
            else:
                w = np.asarray(given).astype(np.int64)
            Xn = y.gather(1, torch.from_numpy(w)[:, None, :])[:, 0, :]
        elif form == "decomposed":
            uv = X @ split_weight(W).t()
            fw = level_forward(uv, idx, gamma, beta, BN_EPS, given)
            mean, var, R, w, Xn = fw["mean"], fw["var"], fw["R"], fw["winner"], fw["x"]
            kept.append((X, uv, fw))
        else:
            raise ValueError(form)
        moved(l, mean, var, R)
        res["winner"].append(w)
        res[f"x{l}"] = Xn.detach()
        feats.append(Xn)
        X = Xn
    cat = torch.cat(feats, 1)
    W5, g5, b5 = P["conv5.0.weight"][:, :, 0], P["bn5.weight"], P["bn5.bias"]
    z5 = cat @ W5.t()
    mean5 = z5.sum(0) / N
    var5 = (z5 * z5).sum(0) / N - mean5 * mean5
    rstd5 = 1.0 / torch.sqrt(var5 + BN_EPS)
    y5 = (z5 - mean5) * rstd5 * g5 + b5
    out = _leaky(y5)
    moved(5, mean5, var5, N)
    res["out"] = out.detach()
    if form == "direct":
        (out * G).sum().backward()
        res["grads"] = {k: P[k].grad.numpy() for k in PARAMS}
        return res
    # ---- the backward by hand
    gr = res["grads"]
    h5 = G * torch.where(y5 > 0, torch.ones((), dtype=dtype), torch.full((), SLOPE, dtype=dtype))
    xh = (z5 - mean5) * rstd5
    gr["bn5.bias"], gr["bn5.weight"] = h5.sum(0), (h5 * xh).sum(0)
    dz5 = g5 * rstd5 * (h5 - gr["bn5.bias"] / N - xh * gr["bn5.weight"] / N)
    gr["conv5.0.weight"] = (dz5.t() @ cat)[:, :, None]
    dcat = dz5 @ W5
    dx_next = None
    for l in (4, 3, 2, 1):
        Xl, uv, fw = kept[l - 1]
        C = WIDTHS[l - 1]
        g = dcat[:, COL[l - 1]:COL[l - 1] + C] + (dx_next if dx_next is not None else 0)
        bw = level_backward(uv, res["knn"][l - 1], fw, g)
        gr[f"bn{l}.weight"], gr[f"bn{l}.bias"] = bw["dgamma"], bw["dbeta"]
        duv = torch.cat([bw["du"], bw["dv"]], 1)
        dW2 = duv.t() @ Xl
        gr[f"conv{l}.0.weight"] = torch.cat([dW2[:C] - dW2[C:], dW2[C:]], 1)[:, :, None]
        dx_next = duv @ split_weight(P[f"conv{l}.0.weight"][:, :, 0])
    res["grads"] = {k: gr[k].numpy() for k in PARAMS}
    return res


# ------------------------------------------------------------------------------------------------------------------ the kernels, bit by bit
def stats_extremum_f32(uv: np.ndarray, idx: np.ndarray, gamma: np.ndarray):
    """pfpp_dgcnn_edge_stats in numpy: z_j = u[idx_j] + v as ONE float32 add (0 for a padded slot: anything outside [0, N)); the extremum
    by comparisons in slot order (a later slot must be strictly larger, resp. smaller: the first slot wins a tie), max where gamma >= 0
    and min where gamma < 0.  -> (e float32 [N, C], winner uint8 [N, C], z float32 [N, K, C])"""
    uv = np.asarray(uv, dtype=np.float32)
    N, C = uv.shape[0], uv.shape[1] // 2
    u, v = uv[:, :C], uv[:, C:]
    z = np.zeros((N, idx.shape[1], C), dtype=np.float32)
    hi = lo = ahi = alo = None
    for j in range(idx.shape[1]):
        ok = (idx[:, j] >= 0) & (idx[:, j] < N)
        zj = np.where(ok[:, None], u[np.where(ok, idx[:, j], 0)] + v, np.float32(0.0)).astype(np.float32)
        z[:, j] = zj
        if j == 0:
            hi, lo = zj, zj
            ahi, alo = np.zeros((N, C), dtype=np.uint8), np.zeros((N, C), dtype=np.uint8)
        else:
            ahi, hi = np.where(zj > hi, np.uint8(j), ahi), np.where(zj > hi, zj, hi)
            alo, lo = np.where(zj < lo, np.uint8(j), alo), np.where(zj < lo, zj, lo)
    up = np.asarray(gamma, dtype=np.float32)[None, :] >= 0
    return np.where(up, hi, lo).astype(np.float32), np.where(up, ahi, alo).astype(np.uint8), z


def apply_f32(y: np.ndarray, a: np.ndarray, b: np.ndarray, slope: float = SLOPE) -> np.ndarray:
    """pfpp_dgcnn_bn_leaky_apply in numpy float32: t = y a (rounded) + b (rounded); t > 0 ? t : t slope"""
    t = (np.asarray(y, np.float32) * np.asarray(a, np.float32)[None, :]).astype(np.float32) + np.asarray(b, np.float32)[None, :]
    assert t.dtype == np.float32
    return np.where(t > 0, t, (t * np.float32(slope)).astype(np.float32)).astype(np.float32)


def stats_case(c_out: int, N: int = 300, seed: int = 3):
    """inputs of the statistics pass alone: (uv float32 [N, 2 c_out], idx int32 [N, K], gamma, beta float32 [c_out]).  The forward
    case file's edge_case (points 0 .. 2: a piece of three whose padded 0 wins the max in the even channels and the min in the odd ones;
    channels 0, 1, 2 (mod 8) have negative, zero and positive gamma) with, in addition, point 3 a piece of its own (one real slot) and
    the rows 10 and 11 of u identical, first and second in the list of point 12 and far above (below in the odd channels) every other
    row: a tie that the first slot must win."""
    uv, idx, gamma, beta = fwd.edge_case(c_out, N, seed)
    idx[3] = N
    idx[3, 0] = 3
    sign = np.where(np.arange(c_out) % 2 == 0, 1.0, -1.0).astype(np.float32)
    uv[10, :c_out] = 50.0 * sign
    uv[11, :c_out] = uv[10, :c_out]
    idx[12, 0], idx[12, 1] = 11, 10
    return uv, idx, gamma, beta


GATHER_LENGTHS = (1, 3, 20, 21, 65, 130)


def gather_lists(seed: int = 11):
    """int32 [240, K] lists for the backward gathers: pieces of 1, 3, 20, 21 and 65 points with random lists of their own rows (the
    first min(K, n) slots real, distinct rows, the point itself first), and a star-shaped piece of 130 points whose first row is in
    every other point's list: its inverse list has 130 entries, longer than a wave and longer than K."""
    rng = np.random.default_rng(seed)
    N = int(np.sum(GATHER_LENGTHS))
    idx = np.full((N, K), N, dtype=np.int32)
    lo = 0
    for n in GATHER_LENGTHS:
        kk = min(K, n)
        for i in range(n):
            others = np.setdiff1d(np.arange(n), [i])
            pick = rng.permutation(others)[:kk - 1]
            if n == 130 and i > 0 and 0 not in pick:
                pick[rng.integers(0, kk - 1)] = 0
            idx[lo + i, :kk] = lo + np.concatenate([[i], pick])
        lo += n
    return idx
