"""Seeded inputs and the restatement for the tests of the cross-attention layer's backward (no test in here).

* The inputs are the `tiny` and `pair` cases and the cross_state_dict() of tests/matching_transformer_cases.py (loaded by path, left
  untouched): x = the case's feats, dout = default_rng([41, 0]).normal(size=x.shape), loss = sum(out * dout).
* cross_train_restate: CrossAttentionLayer.forward (attention_layer.py:47-115) under torch autograd in a given dtype, with an optional
  ReLU pattern that replaces the sign test of F.relu (:91) — the GPU tests hand the float64 run the pattern the GPU used, so that an
  entry within rounding of 0 does not count as an error of the gradients.
* sample / GRAD_NAMES: what tools/make_matching_cross_train_goldens.py stores of the reference's float64 gradients in
  tests/golden/matching_cross_train.npz (vectors in full; of matrices and dx the row sums, the column sums and every 8th row);
  tests/test_matching_cross_train_host.py pins the restatement to that fixture.

numpy and torch only: the golden tool runs in a process that must not import the product."""
from __future__ import annotations

import importlib.util
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location("matching_transformer_cases", Path(__file__).resolve().parent / "matching_transformer_cases.py")
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

FEAT, HEADS, HEAD_DIM, LN_EPS = base.FEAT, base.HEADS, base.HEAD_DIM, base.LN_EPS
CASES = ("tiny", "pair")
ROW_STEP = 8                                   # every 8th row of a matrix is stored
GRAD_NAMES = tuple(k for k, _ in base.cross_state_dict_spec())       # the layer's 12 parameters under the reference's names
TENSORS = ("dx",) + GRAD_NAMES


def case_inputs(name: str):
    """-> (x float32 [N, 128], puzzle point counts int64 [B], dout float64 [N, 128])"""
    _, x, _, puz = base.case_arrays(name)
    dout = np.random.default_rng([41, 0]).normal(size=x.shape)
    return x, puz, dout


def sample(a: np.ndarray) -> dict:
    """what the fixture keeps of a float64 gradient: a vector in full; of a matrix the row sums, the column sums and every 8th row"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return {"full": a}
    return {"rowsum": a.sum(1), "colsum": a.sum(0), "rows": a[::ROW_STEP]}


def cross_train_restate(sd: dict, x, seq_lengths, dout, dtype=torch.float64, relu_mask=None) -> dict:
    """the layer on the flat rows x [N, 128] (attention per puzzle) and the gradients of sum(out * dout) by autograd ->
    dict: out, pre (the input of the ReLU, [N, 256]), dx, and one entry per parameter name.  relu_mask (bool [N, 256]): h = pre where
    the mask is set, 0 elsewhere, instead of relu(pre).  The parameter gradients are the sums over the puzzles."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    W = {k: t(sd[k]).requires_grad_(True) for k in GRAD_NAMES}
    xt = t(x).requires_grad_(True)
    qkv = torch.cat([F.linear(xt, W["attn.w_qs.weight"]), F.linear(xt, W["attn.w_ks.weight"]), F.linear(xt, W["attn.w_vs.weight"])], 1)
    att, lo = [], 0
    for n in np.asarray(seq_lengths, dtype=np.int64):
        q, k, v = (qkv[lo:lo + n, i * FEAT:(i + 1) * FEAT].reshape(n, HEADS, HEAD_DIM).transpose(0, 1) for i in range(3))
        a = torch.softmax(torch.matmul(q / (HEAD_DIM ** 0.5), k.transpose(1, 2)), dim=-1)
        att.append(torch.matmul(a, v).transpose(0, 1).reshape(n, FEAT))
        lo += n
    att = torch.cat(att, 0)
    y = F.layer_norm(F.linear(att, W["attn.fc.weight"]) + xt, (FEAT,), W["attn.layer_norm.weight"], W["attn.layer_norm.bias"], LN_EPS)
    pre = F.linear(y, W["pos_ffn.w_1.weight"], W["pos_ffn.w_1.bias"])
    h = torch.relu(pre) if relu_mask is None else pre * torch.as_tensor(np.asarray(relu_mask)).to(dtype)
    z = F.linear(h, W["pos_ffn.w_2.weight"], W["pos_ffn.w_2.bias"]) + y
    out = F.layer_norm(z, (FEAT,), W["pos_ffn.layer_norm.weight"], W["pos_ffn.layer_norm.bias"], LN_EPS)
    (out * t(dout)).sum().backward()
    res = {"out": out.detach(), "pre": pre.detach(), "dx": xt.grad}
    res.update({k: W[k].grad for k in GRAD_NAMES})
    return res


def attention_grads(qkv, lengths, dout, dtype=torch.float64, scale: float = 0.25):
    """base.attention_restate's statement under autograd (it takes arrays, not tensors that require a gradient), with the gradients
    of sum(out * dout): -> (out, lse [rows, 8] of the scaled scores, dqkv), all in dtype"""
    q = torch.from_numpy(np.asarray(qkv)).to(dtype).requires_grad_(True)
    outs, lses, lo = [], [], 0
    for n in np.asarray(lengths, dtype=np.int64):
        a, b, c = (q[lo:lo + n, i * FEAT:(i + 1) * FEAT].reshape(n, HEADS, HEAD_DIM).transpose(0, 1) for i in range(3))
        s = torch.matmul(a * scale, b.transpose(1, 2))
        lses.append(torch.logsumexp(s, dim=-1).transpose(0, 1))
        outs.append(torch.matmul(torch.softmax(s, dim=-1), c).transpose(0, 1).reshape(n, FEAT))
        lo += n
    out = torch.cat(outs, 0)
    (out * torch.from_numpy(np.asarray(dout)).to(dtype)).sum().backward()
    return out.detach(), torch.cat(lses, 0).detach(), q.grad
