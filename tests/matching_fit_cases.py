"""Inputs and numpy / float64 restatements for the tests of pfpp_hip/matching_fit.py (tests/test_matching_fit_host.py without a GPU,
tests/test_gpu_matching_fit.py with one).  Nothing here imports the product's kernels: the restatements are the yardsticks."""
from __future__ import annotations

import numpy as np

# ------------------------------------------------------------------------------------------------ multi-tensor Adam
ADAM_SIZES = (1, 3, 255, 256, 257, 4096, 4097, 70_001)         # under a wave, around a pass of 256 threads, around half a chunk, 9 chunks


def blocks_of_plan(plan, sizes, chunk, max_tensors, max_blocks):
    """walk a plan of plan_adam_multi the way the C entry fills its launches -> per launch the list of (tensor, chunk) workgroups;
    asserts both capacities.  Written from the entry's contract (include/pfpp.h), not from the function under test."""
    chunks = [-(-n // chunk) for n in sizes]
    out = []
    for first_t, first_c, nb in plan:
        assert 1 <= nb <= max_blocks
        t, c, blocks, tensors = first_t, first_c, [], set()
        while len(blocks) < nb:
            assert t < len(sizes), "a launch runs past the list"
            if c >= chunks[t]:
                t, c = t + 1, 0
                continue
            blocks.append((t, c))
            tensors.add(t)
            c += 1
        assert len(tensors) <= max_tensors
        out.append(blocks)
    return out


def coverage(plan, sizes, chunk, max_tensors, max_blocks):
    """how often every element of every tensor is covered by the plan's workgroups -> list of int arrays"""
    seen = [np.zeros(n, dtype=np.int64) for n in sizes]
    for blocks in blocks_of_plan(plan, sizes, chunk, max_tensors, max_blocks):
        for t, c in blocks:
            seen[t][c * chunk:min((c + 1) * chunk, sizes[t])] += 1
    return seen


def adam_case(sizes, seed, offset=0):
    """parameters, gradients of three steps (float32) for tensors of these sizes; gradients span magnitudes and hold exact zeros"""
    rng = np.random.default_rng([seed, len(sizes)])
    p = [rng.standard_normal(n + offset).astype(np.float32) for n in sizes]
    g = [[(rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, size=n) * (rng.random(n) > 0.05)).astype(np.float32) for n in sizes] for _ in range(3)]
    return p, g


def adam64(p, grads, steps0, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, g_scale=1.0):
    """torch.optim.AdamW (Adam when weight_decay is 0) in float64 over consecutive gradients of ONE tensor, the step count starting
    at steps0 -> the parameter after every step"""
    p = np.asarray(p, dtype=np.float64).copy()
    m, v, outs = np.zeros_like(p), np.zeros_like(p), []
    for i, g in enumerate(grads):
        t = steps0 + i + 1
        g = np.asarray(g, dtype=np.float64) * g_scale
        p = p * (1.0 - lr * weight_decay)
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        p = p - lr / (1 - betas[0] ** t) * m / (np.sqrt(v) / np.sqrt(1 - betas[1] ** t) + eps)
        outs.append(p.copy())
    return outs


# ------------------------------------------------------------------------------------------------ validation metrics
VAL_SIZES = (1, 2, 63, 64, 65, 257)          # one row, one pair, around a wave of columns and 16 x 4 rows, more than one pass of both


def val_case(n, seed=0):
    """a masked doubly-stochastic-like matrix float32 [n, n] with same-piece blocks of exact zeros, entries exactly 1 and exactly 0,
    targets with -1 rows, an assignment that hits the target on some rows only"""
    rng = np.random.default_rng([seed, n])
    piece = np.sort(rng.integers(0, max(2, min(5, n)), size=n))
    ds = rng.random((n, n)).astype(np.float32) ** 4
    ds[piece[:, None] == piece[None, :]] = 0.0
    tgt = rng.integers(0, n, size=n).astype(np.int32)
    tgt[rng.random(n) < 0.25] = -1
    if n > 2:
        tgt[0], tgt[1] = -1, 1 if n > 1 else 0
    col = rng.permutation(n).astype(np.int64)
    hit = (rng.random(n) < 0.5) & (tgt >= 0)
    col[hit] = tgt[hit]                                      # not a permutation any more: the kernel does not need one
    if n >= 4:
        ds[2, :] = 0.0; ds[2, 3] = 1.0                       # an exact 1 off the target (clamped log(0)) ...
        tgt[2] = 0
        ds[3, :] = 0.0; ds[3, 1] = 1.0; tgt[3] = 1           # ... and on it (log(1) = 0), with an exact 0 on a target in row 2
    return ds, tgt, col


def val_reference(ds, tgt, col):
    """float64: (sum_ij BCE(ds_ij, [j == tgt_i]) with both logs clamped at -100, (tp, fp, fn))"""
    n = ds.shape[0]
    p = ds.astype(np.float64)
    y = np.zeros((n, n), dtype=bool)
    rows = np.nonzero(tgt >= 0)[0]
    y[rows, tgt[rows]] = True
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log(np.maximum(1.0 - p, 0.0)), -100.0)
    loss = float(-(np.where(y, lp, lq)).sum())
    tp = int(((col == tgt) & (tgt >= 0)).sum())
    return loss, (tp, n - tp, int((tgt >= 0).sum()) - tp)
