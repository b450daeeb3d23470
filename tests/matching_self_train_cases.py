"""Seeded inputs and the restatement for the tests of the point-transformer layer's training step (no test in here).

* The inputs are the `tiny` and `pair` cases, the ptf_state_dict() and feat_knn_f32 of tests/matching_transformer_cases.py (loaded by
  path, left untouched): p, x = the case's points and feats, the whole case as ONE flat batch, dout = default_rng([43, i]).normal(...),
  loss = sum(out * dout).
* self_train_restate: PointTransformerLayer.forward (attention_layer.py:190-225) in .train() under torch autograd in a given dtype on
  given neighbour lists: the three LayerNorm1d are F.batch_norm(..., training=True) over all 16 N rows (padded slots included), the
  running buffers are returned.  Optionally three boolean ReLU masks replace the sign tests (relu(x) = x * mask): the GPU tests hand
  the float64 run the patterns the GPU used, so that an entry within rounding of 0 does not count as an error of the gradients.
  `mutate` names one deliberate misreading of the layer (tests/test_matching_self_train_host.py shows that each leaves the fixture).
* sample / TENSORS: what tools/make_matching_self_train_goldens.py stores of the reference's float64 results in
  tests/golden/matching_self_train.npz (vectors in full; of matrices, out and dx the row sums, the column sums and every 8th row).

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

FEAT, NSAMPLE, HEADS, HEAD_DIM, BN_EPS = base.FEAT, base.NSAMPLE, base.HEADS, base.HEAD_DIM, base.BN_EPS
BN_MOMENTUM = 0.1
CASES = ("tiny", "pair")
ROW_STEP = 8                                   # every 8th row of a matrix is stored
BN = ("linear_p.1", "linear_w.0", "linear_w.3")                      # the three BatchNorms, in the order of the ReLUs behind them
BUFFER_NAMES = tuple(f"{b}.{s}" for b in BN for s in ("running_mean", "running_var"))
GRAD_NAMES = tuple(k for k, _ in base.ptf_state_dict_spec() if k.rsplit(".", 1)[1] in ("weight", "bias"))        # the 20 parameters
ZERO_GRADS = ("linear_p.0.bias", "linear_w.2.bias")                  # in front of a batch-statistics BatchNorm
# Two more gradients are sums that vanish in exact arithmetic: linear_w.5.bias (the softmax over the slots does not see a shift of its
# logits: the logit gradients of a (point, channel) sum to 0) and linear_q.bias (x_q enters every row of BatchNorm(128)'s input with the
# same sign, and the input gradient of a batch-statistics BatchNorm sums to 0 over the batch).  Their float64 values are ~1e-14, so
# "relative to the tensor's largest magnitude" has no meaning for them; the restatement returns the sum of the |terms| of the worst
# channel instead (zero_sum_scale), the magnitude a rounding error of such a sum is relative to.
ZERO_SUMS = ("linear_q.bias", "linear_w.5.bias")
# linear_k.bias is a third when no slot of idx_k is padded: every row gradient of BatchNorm(128)'s input then lands in some row of dx_k.
TENSORS = ("out", "dx") + GRAD_NAMES + BUFFER_NAMES
MUTATIONS = ("stats_without_padded", "unbiased_variance", "softmax_masks_padded", "no_dxq")


def case_inputs(name: str):
    """-> (p float32 [N, 3], x float32 [N, 128], piece lengths int64 [P], dout float64 [N, 128])"""
    p, x, lengths, _ = base.case_arrays(name)
    dout = np.random.default_rng([43, CASES.index(name)]).normal(size=x.shape)
    return p, x, lengths, dout


def sample(a: np.ndarray) -> dict:
    """what the fixture keeps of a float64 tensor: a vector in full; of a matrix the row sums, the column sums and every 8th row"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return {"full": a}
    return {"rowsum": a.sum(1), "colsum": a.sum(0), "rows": a[::ROW_STEP]}


def self_train_restate(sd: dict, p, x, dout, indices, dtype=torch.float64, masks=None, mutate=None) -> dict:
    """the layer in .train() on the flat batch (p [N, 3], x [N, 128]) with the lists indices = (idx_k, idx_v) int [N, 16] (N = the padded
    slot) and the gradients of sum(out * dout) by autograd -> dict of torch tensors: out, pre = (the inputs of the three ReLUs: [N, 16, 3],
    [N, 16, 128], [N, 16, 16]), dx, one entry per parameter name, the six running buffers after the step, num_batches_tracked, zero_sum_scale (see ZERO_SUMS), padded_slots, dqkv [N, 384].
    masks = three bool arrays of pre's shapes: relu(v) = v * mask.  mutate: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    W = {k: t(sd[k]).requires_grad_(True) for k in GRAD_NAMES}
    buf = {k: t(sd[k]).clone() for k in BUFFER_NAMES}
    pt, xt = t(p), t(x).requires_grad_(True)
    N = xt.shape[0]
    lin = lambda v, name: F.linear(v, W[f"{name}.weight"], W[f"{name}.bias"])
    x_q, x_k, x_v = lin(xt, "linear_q"), lin(xt, "linear_k"), lin(xt, "linear_v")
    for a in (x_q, x_k, x_v):
        a.retain_grad()
    ik, iv = (torch.from_numpy(np.asarray(i).astype(np.int64)) for i in indices)
    valid = ik < N
    pad = lambda a: torch.cat([a, torch.zeros(1, a.shape[1], dtype=dtype)], 0)
    g_k, g_v = pad(x_k)[ik], pad(x_v)[iv]                                             # [N, 16, 128]; index N = the appended zero row
    g_p = (pad(pt)[ik] - pt[:, None, :]) * valid.to(dtype)[..., None]                 # exactly 0 for the padded slots
    pre = []

    def bn(v, prefix):
        """LayerNorm1d in .train(): BatchNorm1d over the last axis of [N, 16, C] with the statistics of all 16 N rows"""
        rows = v.reshape(-1, v.shape[-1])
        if mutate in ("stats_without_padded", "unbiased_variance"):
            sel = rows[valid.reshape(-1)] if mutate == "stats_without_padded" else rows
            mean, var = sel.mean(0), sel.var(0, unbiased=mutate == "unbiased_variance")
            y = (rows - mean) / torch.sqrt(var + BN_EPS) * W[f"{prefix}.weight"] + W[f"{prefix}.bias"]
        else:
            y = F.batch_norm(rows, buf[f"{prefix}.running_mean"], buf[f"{prefix}.running_var"], W[f"{prefix}.weight"], W[f"{prefix}.bias"], True,
                             BN_MOMENTUM, BN_EPS)
        return y.reshape(v.shape)

    def relu(v):
        pre.append(v.detach())
        return torch.relu(v) if masks is None else v * torch.as_tensor(np.asarray(masks[len(pre) - 1])).to(dtype)

    p_r = lin(relu(bn(lin(g_p, "linear_p.0"), "linear_p.1")), "linear_p.3")
    r = g_k - (x_q.detach() + 0 * x_q if mutate == "no_dxq" else x_q)[:, None, :] + p_r      # no_dxq: the value without the gradient
    h = relu(bn(r, "linear_w.0"))
    h = relu(bn(lin(h, "linear_w.2"), "linear_w.3"))
    lg = lin(h, "linear_w.5")
    lg.retain_grad()
    lg0 = lg
    if mutate == "softmax_masks_padded":
        lg = lg.masked_fill(~valid[..., None], float("-inf"))
    w = torch.softmax(lg, dim=1)                                                      # over the 16 neighbours, padded slots included
    out = torch.einsum("ntsi,nti->nsi", (g_v + p_r).reshape(N, NSAMPLE, HEADS, HEAD_DIM), w).reshape(N, FEAT)
    (out * t(dout)).sum().backward()
    res = {"out": out.detach(), "pre": tuple(pre), "dx": xt.grad, "num_batches_tracked": int(np.asarray(sd[f"{BN[0]}.num_batches_tracked"])) + 1}
    res.update({k: W[k].grad for k in GRAD_NAMES})
    res["padded_slots"] = int((~valid).sum())
    res["zero_sum_scale"] = {"linear_q.bias": float(x_q.grad.abs().sum(0).max()), "linear_k.bias": float(x_k.grad.abs().sum(0).max()),
                             "linear_w.5.bias": float(lg0.grad.abs().sum((0, 1)).max())}
    res["dqkv"] = torch.cat([x_q.grad, x_k.grad, x_v.grad], 1)                        # dx_q | dx_k | dx_v: what the projection GEMMs are handed
    res.update(buf)
    return res
