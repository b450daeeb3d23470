"""Cases of the matcher's DGCNN encoder (pfpp_hip/matching_dgcnn.py, csrc/dgcnn.hip): seeded inputs and weights, and the restatements the
tests compare against.  Loaded by path from the tests and from tools/make_matching_dgcnn_goldens.py; imports nothing of the product.

* case_arrays / state_dict: points of a few pieces and the 55 tensors of DGCNNDynamic(128, False, 3) with random BatchNorm statistics,
  about 30 % negative gammas and nonzero betas (a negative gamma turns the max over the slots into a min of the pre-activation).
* feat_knn: the bit-defined search of pfpp_dgcnn_knn in numpy (float32), and the same search on float64 keys.
* edge_max_f32: the arithmetic of pfpp_dgcnn_edge_max in numpy float32, operation by operation.
* restate: the whole layer in torch at any dtype, in the reference's form ("direct": gather [N, 20, 2 C], convolution, BatchNorm,
  LeakyReLU, max) and in the form the kernels compute ("split").
"""
from __future__ import annotations

import numpy as np
import torch

K = 20
WIDTHS = (64, 64, 128, 256)
COL = (0, 64, 128, 256)
CAT = 512
FEAT = 128
SLOPE = 0.2
BN_EPS = 1e-5
WEIGHT_SEED = 20240611

# name -> piece lengths.  tiny: one piece spans two query workgroups (70), one is shorter than K (5), one is a single point.
# mixed: a piece whose four runs are uneven and that spans three query workgroups, next to pieces of K - 1, K and K + 1 points.
LENGTHS = {"tiny": (5, 23, 70, 1), "mixed": (19, 130, 20, 21)}
# the seeds tools/make_matching_dgcnn_goldens.py settled on (the first from 0 upwards at which the reference's float32 and float64 runs
# pick the same neighbour sets at all four levels and no 20th / 21st key pair is closer than MIN_STEP, relative); the fixture records them
SEEDS = {"tiny": 0, "mixed": 7}
MIN_STEP = 1e-4


# ------------------------------------------------------------------------------------------------------------------ inputs and weights
def case_arrays(name: str, seed=None):
    """-> (x float32 [N, 3], lengths int64 [P]): every piece a cloud around its own centre"""
    lengths = np.asarray(LENGTHS[name], dtype=np.int64)
    rng = np.random.default_rng([int(SEEDS[name] if seed is None else seed), len(lengths), int(lengths.sum())])
    pieces = [rng.uniform(-0.5, 0.5, (1, 3)) + rng.uniform(-0.25, 0.25, (int(n), 3)) * rng.uniform(0.5, 1.0, (1, 3)) for n in lengths]
    return np.concatenate(pieces).astype(np.float32), lengths


def state_dict_spec(feat_dim: int = FEAT, in_feat_dim: int = 3):
    """names and shapes of DGCNNDynamic(feat_dim, False, in_feat_dim).state_dict() in its order: bn1 .. bn5, then conv1 .. conv5 with the
    same BatchNorms seen through the Sequential"""
    widths = WIDTHS + (feat_dim,)
    bn = lambda prefix, c: [(f"{prefix}.weight", (c,)), (f"{prefix}.bias", (c,)), (f"{prefix}.running_mean", (c,)), (f"{prefix}.running_var", (c,)),
                            (f"{prefix}.num_batches_tracked", ())]
    spec = []
    for l, c in enumerate(widths, 1):
        spec += bn(f"bn{l}", c)
    c_in = in_feat_dim
    for l, c in enumerate(widths, 1):
        spec.append((f"conv{l}.0.weight", (c, 2 * c_in if l < 5 else CAT, 1)))
        spec += bn(f"conv{l}.1", c)
        c_in = c
    return spec


def state_dict(feat_dim: int = FEAT, seed: int = WEIGHT_SEED) -> dict:
    rng = np.random.default_rng(seed)
    sd = {}
    for l, c in enumerate(WIDTHS + (feat_dim,), 1):
        gamma = rng.uniform(0.5, 1.5, c) * np.where(rng.random(c) < 0.3, -1.0, 1.0)
        sd[f"bn{l}.weight"] = gamma.astype(np.float32)
        sd[f"bn{l}.bias"] = (0.2 * rng.standard_normal(c)).astype(np.float32)
        sd[f"bn{l}.running_mean"] = (0.2 * rng.standard_normal(c)).astype(np.float32)
        sd[f"bn{l}.running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        sd[f"bn{l}.num_batches_tracked"] = np.asarray(100 + l, dtype=np.int64)
    c_in = 3
    for l, c in enumerate(WIDTHS + (feat_dim,), 1):
        k = 2 * c_in if l < 5 else CAT
        sd[f"conv{l}.0.weight"] = (rng.standard_normal((c, k, 1)) * (1.5 / np.sqrt(k))).astype(np.float32)
        for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            sd[f"conv{l}.1.{leaf}"] = sd[f"bn{l}.{leaf}"]
        c_in = c
    order = [k for k, _ in state_dict_spec(feat_dim)]
    assert sorted(order) == sorted(sd)
    return {k: sd[k] for k in order}


# ------------------------------------------------------------------------------------------------------------------ the search
def feat_knn(rows: np.ndarray, lengths, k: int = K, dtype=np.float32):
    """per piece, for every row the min(k, n) nearest rows of the piece (itself included) by d = 0; for c in order: t = a_c - b_c;
    d = d + t t (every operation rounded to dtype), ascending by (bits of d, index); the slots behind them hold N.  With float32 this is
    pfpp_dgcnn_knn bit for bit.  -> (idx int64 [N, k], step float64 [N]: (d_21 - d_20) / d_21 between the k-th and the (k + 1)-th key,
    inf where the piece has no (k + 1)-th row)"""
    a_all = np.ascontiguousarray(rows, dtype=dtype)
    N, C = a_all.shape
    out = np.full((N, k), N, dtype=np.int64)
    step = np.full(N, np.inf)
    lo = 0
    for n in np.asarray(lengths, dtype=np.int64):
        a = a_all[lo:lo + n]
        d = np.zeros((n, n), dtype=dtype)
        for c in range(C):
            t = a[:, None, c] - a[None, :, c]
            d = d + t * t
        assert d.dtype == dtype
        order = np.argsort(d.view(np.uint32 if dtype == np.float32 else np.uint64), axis=1, kind="stable")
        kk = min(k, n)
        out[lo:lo + n, :kk] = order[:, :kk] + lo
        if n > k:
            srt = np.take_along_axis(d, order[:, k - 1:k + 1], 1).astype(np.float64)
            step[lo:lo + n] = (srt[:, 1] - srt[:, 0]) / np.maximum(srt[:, 1], 1e-300)
        lo += n
    return out, step


def knn_rows(C: int, lengths, seed: int) -> np.ndarray:
    """float32 [N, C] rows for the search alone: every piece a cloud of its own"""
    rng = np.random.default_rng([seed, C])
    return np.concatenate([rng.standard_normal((1, C)) + 0.5 * rng.standard_normal((int(n), C)) for n in lengths]).astype(np.float32)


TIE_LENGTHS = (7, 100)


def knn_tie_rows(C: int, seed: int = 5) -> np.ndarray:
    """float32 [107, C], pieces of 7 and 100 rows.  In the second piece (runs of 25 rows per wave) the local rows 0 .. 18 are a tight
    cluster, the local rows 24, 25 and 60 are one and the same row at distance ~1 from it, everything else is far away.  For the 19
    cluster rows the three copies are exact ties for the 20th place, one at the end of the first wave's run, one at the start of the
    second's and one in the third's: the lowest index must win.  For the copies themselves the first three keys are 0, 0, 0."""
    rng = np.random.default_rng([seed, C])
    a = 10.0 + 3.0 * rng.standard_normal((107, C))
    a[7:7 + 19] = 0.02 * rng.standard_normal((19, C))
    copy = np.zeros(C)
    copy[:3] = (0.6, -0.5, 0.4)
    for r in (24, 25, 60):
        a[7 + r] = copy
    return a.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the edge extremum
def edge_max_f32(uv: np.ndarray, idx: np.ndarray, scale: np.ndarray, shift: np.ndarray, slope: float = SLOPE) -> np.ndarray:
    """pfpp_dgcnn_edge_max in numpy float32: uv [N, 2 C] = [u | v], idx [N, K] (anything outside [0, N) is the padded slot) ->
    [N, C].  z_j = u[idx_j] + v for a real slot and 0 for a padded one; the extremum by comparisons in slot order (e = z_0; e = z_j > e
    ? z_j : e, resp. <); max where scale >= 0, min where scale < 0; y = e scale + shift as one multiply and one add; LeakyReLU."""
    uv = np.asarray(uv, dtype=np.float32)
    N, C = uv.shape[0], uv.shape[1] // 2
    u, v = uv[:, :C], uv[:, C:]
    scale, shift = np.asarray(scale, dtype=np.float32), np.asarray(shift, dtype=np.float32)
    hi = lo = None
    for j in range(idx.shape[1]):
        ok = (idx[:, j] >= 0) & (idx[:, j] < N)
        z = np.where(ok[:, None], u[np.where(ok, idx[:, j], 0)] + v, np.float32(0.0)).astype(np.float32)
        if j == 0:
            hi, lo = z, z
        else:
            hi, lo = np.where(z > hi, z, hi), np.where(z < lo, z, lo)
    e = np.where(scale[None, :] >= 0, hi, lo).astype(np.float32)
    y = (e * scale[None, :]).astype(np.float32) + shift[None, :]
    assert y.dtype == np.float32
    return np.where(y > 0, y, (y * np.float32(slope)).astype(np.float32)).astype(np.float32)


def edge_case(c_out: int, N: int = 300, seed: int = 3):
    """inputs of the edge extremum alone: (uv float32 [N, 2 c_out], idx int32 [N, K], scale, shift float32 [c_out]).  Channels 0, 1, 2
    (mod 8) have negative, zero and positive scale whatever the draw.  The first three points are a piece of their own with 17 padded
    slots: their u + v is negative in the even channels and positive in the odd ones, so the padded slot's 0 wins the max in the even
    channels and the min in the odd ones.  The other points have full lists of random rows."""
    rng = np.random.default_rng([seed, c_out])
    uv = rng.standard_normal((N, 2 * c_out)).astype(np.float32)
    sign = np.where(np.arange(c_out) % 2 == 0, -1.0, 1.0)
    uv[:3, :c_out] = (sign * rng.uniform(2.0, 3.0, (3, c_out))).astype(np.float32)
    uv[:3, c_out:] = (sign * rng.uniform(0.1, 1.0, (3, c_out))).astype(np.float32)
    idx = rng.integers(3, N, (N, K)).astype(np.int32)
    idx[:3] = N
    idx[:3, :3] = np.asarray([[0, 1, 2], [1, 0, 2], [2, 1, 0]])
    scale = (rng.uniform(0.5, 1.5, c_out) * np.where(rng.random(c_out) < 0.3, -1.0, 1.0)).astype(np.float32)
    scale[0::8], scale[1::8], scale[2::8] = -np.abs(scale[0::8]), 0.0, np.abs(scale[2::8])
    shift = (0.3 * rng.standard_normal(c_out)).astype(np.float32)
    return uv, idx, scale, shift


# ------------------------------------------------------------------------------------------------------------------ the whole layer
def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _leaky(y):
    return torch.where(y > 0, y, y * SLOPE)


def restate(sd: dict, x, lengths, dtype=torch.float64, indices=None, form: str = "direct") -> dict:
    """DGCNNDynamic(feat_dim, False, 3).forward in eval mode.  indices: four [N, K] arrays to use instead of searching (the search
    is feat_knn at the dtype's precision).  form "direct" is the reference's: the [N, K, 2 C] tensor of cat(x_j - x_i, x_i) times the
    mask, the convolution on it, BatchNorm, LeakyReLU, max over the slots.  form "split" is what the kernels compute: u = X W_a^T,
    v = X (W_b - W_a)^T, the extremum of u[j] + v[i] (0 for a padded slot) by the sign of the BatchNorm scale, then the affine and
    LeakyReLU.  -> {"knn": [4 x int64 [N, K]], "x1" .. "x4", "out"} as torch tensors of dtype"""
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    X = _t(x, dtype)
    N = X.shape[0]
    res = {"knn": []}
    feats = []
    for l in range(1, 5):
        idx = np.asarray(indices[l - 1]).astype(np.int64) if indices is not None else feat_knn(X.numpy(), lengths, K, np_dtype)[0]
        res["knn"].append(idx)
        it = torch.from_numpy(idx)
        real = (it != N)
        W = _t(sd[f"conv{l}.0.weight"], dtype)[:, :, 0]
        gamma, beta = _t(sd[f"bn{l}.weight"], dtype), _t(sd[f"bn{l}.bias"], dtype)
        mean, var = _t(sd[f"bn{l}.running_mean"], dtype), _t(sd[f"bn{l}.running_var"], dtype)
        c_in = X.shape[1]
        if form == "direct":
            Xp = torch.cat([X, torch.zeros((1, c_in), dtype=dtype)], 0)
            nb = Xp[it.reshape(-1)].reshape(N, K, c_in)
            own = X[:, None, :].expand(N, K, c_in)
            f = torch.cat([nb - own, own], -1) * real[..., None].to(dtype)
            z = f @ W.t()                                                            # [N, K, C_out]
            y = _leaky((z - mean) / torch.sqrt(var + BN_EPS) * gamma + beta)
            X = y.max(1)[0]
        elif form == "split":
            wa, wb = W[:, :c_in], W[:, c_in:]
            u, v = X @ wa.t(), X @ (wb - wa).t()
            up = torch.cat([u, torch.zeros((1, u.shape[1]), dtype=dtype)], 0)
            z = torch.where(real[..., None], up[it.reshape(-1)].reshape(N, K, -1) + v[:, None, :], torch.zeros((), dtype=dtype))
            s = gamma / torch.sqrt(var + BN_EPS)
            t = beta - mean * s
            e = torch.where(s >= 0, z.max(1)[0], z.min(1)[0])
            X = _leaky(e * s + t)
        else:
            raise ValueError(form)
        feats.append(X)
        res[f"x{l}"] = X
    cat = torch.cat(feats, 1)
    W = _t(sd["conv5.0.weight"], dtype)[:, :, 0]
    z = cat @ W.t()
    res["cat"] = cat
    res["out"] = _leaky((z - _t(sd["bn5.running_mean"], dtype)) / torch.sqrt(_t(sd["bn5.running_var"], dtype) + BN_EPS)
                        * _t(sd["bn5.weight"], dtype) + _t(sd["bn5.bias"], dtype))
    return res


def conv5_f64(sd: dict, cat: np.ndarray) -> np.ndarray:
    """conv5 + bn5 + LeakyReLU of given rows [N, 512] in float64"""
    c = torch.from_numpy(np.asarray(cat)).double()
    z = c @ _t(sd["conv5.0.weight"], torch.float64)[:, :, 0].t()
    y = (z - _t(sd["bn5.running_mean"], torch.float64)) / torch.sqrt(_t(sd["bn5.running_var"], torch.float64) + BN_EPS) \
        * _t(sd["bn5.weight"], torch.float64) + _t(sd["bn5.bias"], torch.float64)
    return _leaky(y).numpy()
