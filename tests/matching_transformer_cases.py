"""Seeded inputs and restatements for the tests of the matcher's point-transformer and cross-attention layers (no test in here).

* Weights of PointTransformerLayer(128, 128, 8, 16) and CrossAttentionLayer(128, 8) under the reference's parameter and buffer names
  (Jigsaw_matching/model/jigsaw/attention_layer.py), regenerated from a seed and never stored; the BatchNorm running statistics and
  affine terms are non-trivial.  A seeded head classifier for the end-to-end test.
* The input cases: points, input features and piece lengths of `tiny` (one puzzle) and `pair` (`tiny` plus a second puzzle), and the
  attention-only cases (packed q | k | v rows and sequence lengths).
* A restatement of both layers in torch that takes the dtype and the neighbour indices as arguments, and the numpy float32
  restatement of the bit-defined neighbour key.  tools/make_matching_transformer_goldens.py runs the REFERENCE's two modules on
  these inputs and stores what they return in tests/golden/matching_transformer.npz; tests/test_matching_transformer_host.py pins the
  restatement to that fixture, so the GPU tests may lean on it (in float64, on any indices).

numpy and torch only: the golden tool runs in a process that must not import the product."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

FEAT, NSAMPLE, HEADS, HEAD_DIM = 128, 16, 8, 16
BN_EPS, LN_EPS = 1e-5, 1e-6

# name -> list of puzzles, each a list of piece lengths.  tiny: fewer than K, exactly K, K + 1 (with two identical input rows: an
# exact tie), wave edges 64 / 65, several query blocks (200).  pair: two sequence lengths, neither a multiple of 32, the first > 128.
CASES = {"tiny": [[5, 16, 17, 64, 65, 200]], "pair": [[5, 16, 17, 64, 65, 200], [33, 100, 31]]}
PUZZLE_SEED = {(5, 16, 17, 64, 65, 200): 201, (33, 100, 31): 202}
TIE_PIECE, TIE_ROWS = 2, (3, 11)            # the 17-point piece: local rows 3 and 11 carry the same input features

# attention-only cases: name -> (sequence lengths of one launch, standard deviation of q and k, seed).  `many` has 64 sequences, the
# first across two blocks of 512 queries: enough workgroups for the kernel's two-queries-per-lane form, which the others do not reach.
ATTN_CASES = {"edges_a": ((1, 31, 32, 33), 1.0, 0), "edges_b": ((127, 128, 129, 300), 1.0, 1), "wide": ((300, 77), 3.9, 2),
              "many": ((600,) + (9,) * 63, 1.0, 3)}


# ------------------------------------------------------------------------------------------------------------------ weights
def _bn(prefix: str, c: int) -> list:
    return [(f"{prefix}.weight", (c,)), (f"{prefix}.bias", (c,)), (f"{prefix}.running_mean", (c,)), (f"{prefix}.running_var", (c,)),
            (f"{prefix}.num_batches_tracked", ())]


def ptf_state_dict_spec() -> list:
    """[(name, shape)] of PointTransformerLayer(128, 128, 8, 16).state_dict() in the reference's order"""
    w = FEAT // HEADS
    spec = []
    for n in ("linear_q", "linear_k", "linear_v"):
        spec += [(f"{n}.weight", (FEAT, FEAT)), (f"{n}.bias", (FEAT,))]
    spec += [("linear_p.0.weight", (3, 3)), ("linear_p.0.bias", (3,))] + _bn("linear_p.1", 3) + [("linear_p.3.weight", (FEAT, 3)), ("linear_p.3.bias", (FEAT,))]
    spec += _bn("linear_w.0", FEAT) + [("linear_w.2.weight", (w, FEAT)), ("linear_w.2.bias", (w,))] + _bn("linear_w.3", w)
    spec += [("linear_w.5.weight", (w, w)), ("linear_w.5.bias", (w,))]
    return spec


def cross_state_dict_spec() -> list:
    """[(name, shape)] of CrossAttentionLayer(128, 8).state_dict() in the reference's order"""
    return [("attn.w_qs.weight", (FEAT, FEAT)), ("attn.w_ks.weight", (FEAT, FEAT)), ("attn.w_vs.weight", (FEAT, FEAT)), ("attn.fc.weight", (FEAT, FEAT)),
            ("attn.layer_norm.weight", (FEAT,)), ("attn.layer_norm.bias", (FEAT,)), ("pos_ffn.w_1.weight", (2 * FEAT, FEAT)),
            ("pos_ffn.w_1.bias", (2 * FEAT,)), ("pos_ffn.w_2.weight", (FEAT, 2 * FEAT)), ("pos_ffn.w_2.bias", (FEAT,)),
            ("pos_ffn.layer_norm.weight", (FEAT,)), ("pos_ffn.layer_norm.bias", (FEAT,))]


def _fill(spec, seed: int, gain: dict) -> dict:
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in spec:
        leaf = name.rsplit(".", 1)[1]
        norm = "layer_norm" in name or name.startswith(("linear_p.1", "linear_w.0", "linear_w.3"))
        if leaf == "num_batches_tracked":
            sd[name] = np.asarray(0, dtype=np.int64)
        elif leaf == "running_mean":
            sd[name] = rng.normal(0, 0.2, shape).astype(np.float32)
        elif leaf == "running_var":
            sd[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif norm and leaf == "weight":
            sd[name] = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif norm and leaf == "bias":
            sd[name] = rng.normal(0.1, 0.1, shape).astype(np.float32)
        elif leaf == "weight":
            sd[name] = (gain.get(name, 1.0) * rng.normal(0, np.sqrt(1.0 / shape[1]), shape)).astype(np.float32)
        else:
            sd[name] = rng.normal(0, 0.05, shape).astype(np.float32)
    return sd


def ptf_state_dict(seed: int = 31) -> dict:
    # linear_p sees offsets of a few tenths: its first layer is scaled up so that the ReLU behind the BatchNorm is active on both sides
    return _fill(ptf_state_dict_spec(), seed, {"linear_p.0.weight": 6.0, "linear_w.2.weight": 1.5, "linear_w.5.weight": 2.0})


def cross_state_dict(seed: int = 32) -> dict:
    return _fill(cross_state_dict_spec(), seed, {"attn.w_qs.weight": 2.0, "attn.w_ks.weight": 2.0})


def classifier_state_dict(seed: int = 33) -> dict:
    """pc_classifier.* of the head (BatchNorm1d(128), ReLU, Conv1d(128, 1, 1)) for the end-to-end test: dense weights, so the logits of
    LayerNorm-ed descriptors spread over several units and none lies within rounding of 0 (the test counts them in float64)"""
    rng = np.random.default_rng(seed)
    C = FEAT
    return {"pc_classifier.0.weight": rng.uniform(0.8, 1.2, C).astype(np.float32), "pc_classifier.0.bias": rng.normal(0.1, 0.1, C).astype(np.float32),
            "pc_classifier.0.running_mean": rng.normal(0, 0.2, C).astype(np.float32), "pc_classifier.0.running_var": rng.uniform(0.5, 1.5, C).astype(np.float32),
            "pc_classifier.0.num_batches_tracked": np.asarray(0, dtype=np.int64),
            "pc_classifier.2.weight": rng.normal(0, 0.4, (1, C, 1)).astype(np.float32), "pc_classifier.2.bias": np.asarray([0.1], dtype=np.float32)}


# ------------------------------------------------------------------------------------------------------------------ inputs
_PUZZLES = {}


def make_puzzle(lengths) -> dict:
    """-> points float32 [N, 3], feats float32 [N, 128], lengths int64 [P].  The features are a smooth function of the coordinates
    plus noise with the first three channels scaled up: the distances between projected rows are spread out and far above the
    denormal range.  In the 17-point piece two rows carry the same features (at different coordinates)."""
    key = tuple(int(n) for n in lengths)
    if key in _PUZZLES:
        return _PUZZLES[key]
    rng = np.random.default_rng([29, PUZZLE_SEED[key]])
    pts = np.concatenate([rng.normal(0, 0.5, 3) + 0.2 * rng.normal(size=(n, 3)) for n in key]).astype(np.float32)
    freq, phase = rng.normal(0, 3.0, (3, FEAT)), rng.uniform(0, 2 * np.pi, FEAT)
    x = np.sin(pts.astype(np.float64) @ freq + phase) + 0.3 * rng.normal(size=(len(pts), FEAT))
    x[:, :3] *= 4.0
    x = x.astype(np.float32)
    if len(key) > TIE_PIECE and key[TIE_PIECE] == 17:
        base = int(np.sum(key[:TIE_PIECE]))
        x[base + TIE_ROWS[1]] = x[base + TIE_ROWS[0]]
    _PUZZLES[key] = {"points": pts, "feats": x, "lengths": np.asarray(key, dtype=np.int64)}
    return _PUZZLES[key]


def make_case(name: str) -> list:
    return [make_puzzle(lengths) for lengths in CASES[name]]


def case_arrays(name: str):
    """-> (points [N, 3], feats [N, 128], piece lengths [P], puzzle point counts [B]) of the whole case, flat"""
    pzs = make_case(name)
    return (np.concatenate([z["points"] for z in pzs]), np.concatenate([z["feats"] for z in pzs]), np.concatenate([z["lengths"] for z in pzs]),
            np.asarray([int(z["lengths"].sum()) for z in pzs], dtype=np.int64))


def attn_case(name: str):
    """-> (qkv float32 [rows, 384] = q | k | v for 8 heads of 16, sequence lengths int64)"""
    lengths, sigma, seed = ATTN_CASES[name]
    rng = np.random.default_rng([37, seed])
    rows = int(np.sum(lengths))
    qkv = rng.normal(size=(rows, 3 * FEAT))
    qkv[:, :2 * FEAT] *= sigma
    return qkv.astype(np.float32), np.asarray(lengths, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------ the neighbour key
def feat_knn_f32(rows: np.ndarray, lengths, K: int = NSAMPLE):
    """the bit-defined search of pfpp_feat_knn in numpy float32: per piece, for every row the min(K, n) nearest rows of the piece by
    d = 0; for c in order: t = a_c - b_c; d = d + t t (every operation rounded to float32), ascending by (bits of d, index); the
    slots behind them hold N.  -> (idx int64 [N, K], gap float64 [N]: the smallest relative step between two consecutive DIFFERENT
    distances among a row's first min(K, n - 1) + 1, i.e. how far the list is from another order)"""
    a_all = np.ascontiguousarray(rows, dtype=np.float32)
    N, C = a_all.shape
    out = np.full((N, K), N, dtype=np.int64)
    gap = np.full(N, np.inf)
    lo = 0
    for n in np.asarray(lengths, dtype=np.int64):
        a = a_all[lo:lo + n]
        d = np.zeros((n, n), dtype=np.float32)
        for c in range(C):
            t = a[:, None, c] - a[None, :, c]
            d = d + t * t
        assert d.dtype == np.float32
        order = np.argsort(d.view(np.uint32), axis=1, kind="stable")
        k = min(K, n)
        out[lo:lo + n, :k] = order[:, :k] + lo
        srt = np.take_along_axis(d, order[:, :min(k + 1, n)], 1).astype(np.float64)
        if srt.shape[1] > 1:
            step = np.diff(srt, axis=1) / np.maximum(srt[:, 1:], 1e-300)
            gap[lo:lo + n] = np.where(step > 0, step, np.inf).min(1)
        lo += n
    return out, gap


# ------------------------------------------------------------------------------------------------------------------ restatements
def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _bn1d(x, sd, prefix, dtype):
    """the reference's LayerNorm1d on [N, k, C]: BatchNorm1d over C of the transposed tensor, eval mode"""
    y = F.batch_norm(x.transpose(1, 2).contiguous(), _t(sd[f"{prefix}.running_mean"], dtype), _t(sd[f"{prefix}.running_var"], dtype),
                     _t(sd[f"{prefix}.weight"], dtype), _t(sd[f"{prefix}.bias"], dtype), False, 0.1, BN_EPS)
    return y.transpose(1, 2).contiguous()


def ptf_restate(sd: dict, p, x, lengths, dtype=torch.float64, indices=None, projections=None) -> dict:
    """PointTransformerLayer.forward (attention_layer.py:190-225) restated.  indices = (idx_k, idx_v) int [N, 16] (N = pad) or None:
    then they are feat_knn_f32 of this run's own x_k / x_v (float32 only: the key is defined on float32 rows).  projections = (x_q,
    x_k, x_v) replaces the three linear layers.  -> dict of torch tensors: x_q, x_k, x_v, idx_k, idx_v, p_r, w, out"""
    p, x = _t(p, dtype), _t(x, dtype)
    N = x.shape[0]
    lin = lambda v, name: F.linear(v, _t(sd[f"{name}.weight"], dtype), _t(sd[f"{name}.bias"], dtype))
    if projections is None:
        x_q, x_k, x_v = lin(x, "linear_q"), lin(x, "linear_k"), lin(x, "linear_v")
    else:
        x_q, x_k, x_v = (_t(a, dtype) for a in projections)
    if indices is None:
        assert dtype == torch.float32, "the neighbour key is defined on float32 rows"
        idx_k, idx_v = feat_knn_f32(x_k.numpy(), lengths)[0], feat_knn_f32(x_v.numpy(), lengths)[0]
    else:
        idx_k, idx_v = (np.asarray(i).astype(np.int64) for i in indices)
    ik, iv = torch.from_numpy(idx_k), torch.from_numpy(idx_v)
    pad = lambda a: torch.cat([a, torch.zeros(1, a.shape[1], dtype=dtype)], 0)
    g_k, g_v = pad(x_k)[ik], pad(x_v)[iv]                                             # [N, 16, 128]; index N = the appended zero row
    g_p = (pad(p)[ik] - p[:, None, :]) * (ik < N).to(dtype)[..., None]                # exactly 0 for the padded slots
    h = torch.relu(_bn1d(lin(g_p, "linear_p.0"), sd, "linear_p.1", dtype))
    p_r = lin(h, "linear_p.3")
    r = g_k - x_q[:, None, :] + p_r
    h = torch.relu(_bn1d(r, sd, "linear_w.0", dtype))
    h = torch.relu(_bn1d(lin(h, "linear_w.2"), sd, "linear_w.3", dtype))
    w = torch.softmax(lin(h, "linear_w.5"), dim=1)                                    # over the 16 neighbours, padded slots included
    out = torch.einsum("ntsi,nti->nsi", (g_v + p_r).reshape(N, NSAMPLE, HEADS, HEAD_DIM), w).reshape(N, FEAT)
    return {"x_q": x_q, "x_k": x_k, "x_v": x_v, "idx_k": idx_k, "idx_v": idx_v, "p_r": p_r, "w": w, "out": out}


def attention_restate(qkv, lengths, dtype=torch.float64, scale: float = 0.25):
    """unmasked attention per sequence and head from packed rows [rows, 384] = q | k | v -> [rows, 128]"""
    qkv = _t(qkv, dtype)
    out, lo = [], 0
    for n in np.asarray(lengths, dtype=np.int64):
        q, k, v = (qkv[lo:lo + n, i * FEAT:(i + 1) * FEAT].reshape(n, HEADS, HEAD_DIM).transpose(0, 1) for i in range(3))
        a = torch.softmax(torch.matmul(q * scale, k.transpose(1, 2)), dim=-1)
        out.append(torch.matmul(a, v).transpose(0, 1).reshape(n, FEAT))
        lo += n
    return torch.cat(out, 0)


def cross_restate(sd: dict, x, seq_lengths, dtype=torch.float64) -> dict:
    """CrossAttentionLayer.forward (attention_layer.py:47-115) restated per puzzle -> dict: att (before fc), ln1, out"""
    x = _t(x, dtype)
    W = lambda name: _t(sd[name], dtype)
    qkv = torch.cat([F.linear(x, W("attn.w_qs.weight")), F.linear(x, W("attn.w_ks.weight")), F.linear(x, W("attn.w_vs.weight"))], 1)
    att = attention_restate(qkv, seq_lengths, dtype, 1.0 / (HEAD_DIM ** 0.5))
    y = F.layer_norm(F.linear(att, W("attn.fc.weight")) + x, (FEAT,), W("attn.layer_norm.weight"), W("attn.layer_norm.bias"), LN_EPS)
    z = F.linear(torch.relu(F.linear(y, W("pos_ffn.w_1.weight"), W("pos_ffn.w_1.bias"))), W("pos_ffn.w_2.weight"), W("pos_ffn.w_2.bias")) + y
    out = F.layer_norm(z, (FEAT,), W("pos_ffn.layer_norm.weight"), W("pos_ffn.layer_norm.bias"), LN_EPS)
    return {"att": att, "ln1": y, "out": out}


def classifier_logits(sd: dict, feats, dtype=torch.float64):
    """pc_classifier of the head on [N, 128] descriptors -> logits [N]"""
    x = _t(feats, dtype)
    scale = _t(sd["pc_classifier.0.weight"], dtype) / torch.sqrt(_t(sd["pc_classifier.0.running_var"], dtype) + BN_EPS)
    h = torch.relu((x - _t(sd["pc_classifier.0.running_mean"], dtype)) * scale + _t(sd["pc_classifier.0.bias"], dtype))
    return h @ _t(sd["pc_classifier.2.weight"], dtype).reshape(-1) + _t(sd["pc_classifier.2.bias"], dtype)[0]
