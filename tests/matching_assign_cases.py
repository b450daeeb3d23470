"""Seeded inputs of the assignment tests (tests/test_matching_assign_host.py, tests/test_gpu_matching_assign.py): square float32
matrices as the matcher's Sinkhorn writes them, and the edge cases of the device solver (pfpp_hip/matching_assign.py).

A case is built once per process and so is its restatement result (reference()): the GPU tests and the host tests share both and
leave them unchanged."""
from __future__ import annotations

import functools
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np

DESC_DIM = 16


class Case(NamedTuple):
    c: np.ndarray                          # float32 [n, n]
    pieces: Optional[Tuple[int, ...]]      # critical points per piece (Sinkhorn-like cases), else None
    by_weight: bool                        # exact ties: any optimum is accepted by its weight


def sinkhorn_like(pieces, noise: float, weak: float, seed: int, tau: float = 0.05, iters: int = 20) -> np.ndarray:
    """unit descriptors with a planted partner permutation, per-coordinate noise and a share `weak` of rows whose descriptor is
    replaced by an unrelated one; L = s / tau, same-piece blocks masked, `iters` alternating log-space normalisations (rows first),
    exp, float32, masked entries exactly 0"""
    rng = np.random.default_rng(seed)
    n = int(sum(pieces))
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    x = unit(rng.standard_normal((n, DESC_DIM)))
    partner = rng.permutation(n)
    y = np.empty_like(x)
    y[partner] = unit(x + noise * rng.standard_normal((n, DESC_DIM)))
    weak_rows = rng.random(n) < weak
    x[weak_rows] = unit(rng.standard_normal((int(weak_rows.sum()), DESC_DIM)))
    piece = np.repeat(np.arange(len(pieces)), pieces)
    same = piece[:, None] == piece[None, :]
    L = np.where(same, -np.inf, (x @ y.T) / tau)
    for it in range(iters):
        ax = 1 if it % 2 == 0 else 0
        m = L.max(axis=ax, keepdims=True)
        L = L - (m + np.log(np.exp(L - m).sum(axis=ax, keepdims=True)))
    out = np.exp(L).astype(np.float32)
    out[same] = 0.0
    return out


def uniform(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((n, n), dtype=np.float32)


def dominated(n: int, seed: int) -> np.ndarray:
    """column 0 is every row's best: the initialisation gives it to row 0 and leaves n - 1 rows free"""
    c = uniform(n, seed)
    c[:, 0] += 2.0
    return c


def identity_like(n: int, seed: int) -> np.ndarray:
    c = uniform(n, seed) * np.float32(0.0999)
    c[np.arange(n), np.arange(n)] = 0.9
    return c


def chain(n: int, seed: int) -> np.ndarray:
    """one free row whose search scans every column.  Before the shuffle: row i < n - 1 has 1 on the diagonal (its initial column)
    and 1 - 2^-8 on column i + 1; the last row has its 1 on column 0, which row 0 keeps, and column n - 1 is the only free one.
    From the last row the direct way to column n - 1 costs 1, the way along the chain k 2^-8 up to column k: the search walks
    all n columns ((n - 1) / 256 < 1) and augments along n - 1 hops.  Every number is exact in float32 and every sum in float64."""
    assert 2 <= n <= 256
    c = np.zeros((n, n), dtype=np.float32)
    i = np.arange(n - 1)
    c[i, i] = 1.0
    c[i, i + 1] = 1.0 - 2.0 ** -8
    c[n - 1, 0] = 1.0
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(c[rng.permutation(n)][:, rng.permutation(n)])


def quarters(n: int, seed: int) -> np.ndarray:
    return (np.random.default_rng(seed).integers(0, 5, (n, n)) / 4.0).astype(np.float32)


_S = lambda pieces, noise, weak, seed: (lambda: Case(sinkhorn_like(pieces, noise, weak, seed), tuple(pieces), False))
_P = lambda fn, *a, by_weight=False: (lambda: Case(fn(*a), None, by_weight))

BUILDERS: Dict[str, Callable[[], Case]] = {
    # group 1: Sinkhorn-like
    "sk_30_33": _S((30, 33), 0.10, 0.2, 11),
    "sk_30_35": _S((30, 35), 0.10, 0.3, 12),
    "sk_40_1_30_17_9": _S((40, 1, 30, 17, 9), 0.10, 0.4, 13),
    "sk_200_20_30": _S((200, 20, 30), 0.10, 0.3, 14),           # 150 rows of the first piece can only take exact zeros
    "sk_100_100_57": _S((100, 100, 57), 0.10, 0.25, 15),
    "sk_150x4": _S((150,) * 4, 0.10, 0.35, 16),
    "sk_all_weak_64x3": _S((64, 64, 64), 0.10, 1.0, 17),
    # group 2: uniform random
    "uniform_1": _P(uniform, 1, 21), "uniform_2": _P(uniform, 2, 22), "uniform_3": _P(uniform, 3, 23),
    "uniform_64": _P(uniform, 64, 24), "uniform_65": _P(uniform, 65, 25),
    "uniform_1025": _P(uniform, 1025, 26),                       # the first size with more columns than a workgroup has threads
    # groups 3-6
    "dominated_65": _P(dominated, 65, 31),
    "identity_257": _P(identity_like, 257, 41),
    "chain_130": _P(chain, 130, 51),
    "quarters_64": _P(quarters, 64, 61, by_weight=True),
    "zeros_5": lambda: Case(np.zeros((5, 5), dtype=np.float32), None, True),
    # group 7: one size of the workload
    "workload_2492": _S((312, 311) * 4, 0.15, 0.3, 71),
}
NAMES = tuple(BUILDERS)
SINKHORN_LIKE = tuple(k for k in NAMES if k.startswith(("sk_", "workload_")))


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = BUILDERS[name]()
    c.c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """assign_reference of the case with the default budget"""
    from pfpp_hip.matching_assign import assign_reference

    out = assign_reference(case(name).c)
    for a in (out.col, out.u, out.v):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scipy_col(name: str) -> np.ndarray:
    from scipy.optimize import linear_sum_assignment

    row, col = linear_sum_assignment(-case(name).c.astype(np.float64))
    assert (row == np.arange(row.size)).all()
    return col.astype(np.int64)


def bits(a: np.ndarray) -> np.ndarray:
    """float64 -> its bit patterns, for comparisons that tell -0.0 from 0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
