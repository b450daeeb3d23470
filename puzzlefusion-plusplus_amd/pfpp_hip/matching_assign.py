"""The matcher's optimal assignment on the device (csrc/matching_assign.hip, include/pfpp.h "matcher, assignment").

The reference hands every puzzle's Sinkhorn output to scipy.optimize.linear_sum_assignment on the host, one puzzle after the other
(Jigsaw_matching/utils/linear_solvers.py:279-340).  Here:

* assign_batch: all puzzles of a call in one launch (one workgroup per puzzle), nothing copied to the host.
* assign_reference: the numpy float64 restatement of the kernels, operation for operation: the parity target of the kernels (bitwise)
  and itself pinned against scipy on the CPU (tests/test_matching_assign_host.py).
* plan_assign: the launches pfpp_match_assign issues for a list of sizes, restated.

The algorithm (maximise sum_i c[i, col_i]; duals and path lengths in float64 on cost = -(double)c; additions, subtractions and
comparisons only):

(a) u_i = min_j cost_ij, v = 0; j*(i) = the lowest column attaining the minimum; column j goes to the lowest row i with j*(i) = j.
(b) the rows left free, in ascending order, each by one shortest augmenting path.  A step relaxes every unscanned column j from the
    current row i, r = ((minv + cost_ij) - u_i) - v_j, dist_j = r and path_j = i where r < dist_j; then scans the unscanned column
    with the smallest (dist, assigned, index), lexicographic: among equal dist an unassigned column first, then the lowest index.
    minv = its dist; an unassigned column is the sink, otherwise the search goes on from the column's row.  At the sink
    u[cur] += minv, u[row4col[j]] += minv - dist_j for every scanned column but the sink, v_j -= minv - dist_j for every scanned
    column, and the assignment is flipped along path.
(c) max_steps bounds the steps of a puzzle over all its searches: when it is used up, status = 1 and col is unspecified.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

MAX_N, MAX_PUZZLES = 8192, 64            # PFPP_MATCH_ASSIGN_MAX_N / _MAX_PUZZLES of include/pfpp.h
# default step budget = BUDGET_FACTOR n.  A step costs 4.2 us at n = 5,000: 32 n bounds a launch there at 0.67 s (64 n: 1.34 s), and
# is 4.8 x the steps of the hardest workload input measured (6.7 n)
BUDGET_FACTOR = 32


class AssignOutput(NamedTuple):
    col: list            # per puzzle int64 [n]: the column of every row
    u: list              # per puzzle float64 [n]
    v: list              # per puzzle float64 [n]
    status: object       # int32 [B]: 0 solved; 1 the step budget ran out, 2 NaN or infinite entries (col of that puzzle is unspecified)
    steps: object        # int64 [B] search steps
    augmentations: object  # int64 [B] searches = rows the initialisation left free


def default_budget(n: int) -> int:
    return max(1, BUDGET_FACTOR * int(n))


def workgroup_shape(n_max: int) -> Tuple[int, int]:
    """(threads, columns per thread) of the solver's workgroups in a launch whose largest puzzle has n_max rows: a function of the
    sizes alone (launch ladder of pfpp_match_assign)"""
    for cap in (64, 128, 256, 512, 1024):
        if n_max <= cap:
            return cap, 1
    for k in (2, 3, 4, 6, 8):
        if n_max <= 1024 * k:
            return 1024, k
    raise ValueError(f"n = {n_max} is beyond the solver's {MAX_N}")


def plan_assign(sizes: Sequence[int]) -> List[Tuple[int, int, int, int]]:
    """the launches of pfpp_match_assign for puzzles of the given sizes (all >= 1): [(first puzzle, count, threads, columns per
    thread)], puzzles in order, MAX_PUZZLES to a launch"""
    sizes = [int(n) for n in sizes]
    plan = []
    for b0 in range(0, len(sizes), MAX_PUZZLES):
        chunk = sizes[b0:b0 + MAX_PUZZLES]
        plan.append((b0, len(chunk), *workgroup_shape(max(chunk))))
    return plan


def _budgets(sizes: Sequence[int], max_steps) -> List[int]:
    if max_steps is None:
        return [default_budget(n) for n in sizes]
    if isinstance(max_steps, (int, np.integer)):
        return [int(max_steps)] * len(sizes)
    if len(max_steps) != len(sizes):
        raise ValueError("max_steps: one budget per puzzle")
    return [default_budget(n) if m is None else int(m) for n, m in zip(sizes, max_steps)]


def assign_batch(ds_list, *, max_steps: Union[None, int, Sequence[Optional[int]]] = None) -> AssignOutput:
    """ds_list: float32 [n_b, n_b] matrices on one GPU (contiguous; empty ones pass through as empty results with status 0).
    max_steps: None = BUDGET_FACTOR n per puzzle, one int for all, or one entry per puzzle (None = its default).  Everything
    returned lives on the device; nothing is read back here."""
    import torch

    from . import _lib, ops
    from ._lib import check

    ds_list = list(ds_list)
    if not ds_list:
        raise ValueError("assign_batch: no matrices")
    for k, ds in enumerate(ds_list):
        if not isinstance(ds, torch.Tensor):
            raise TypeError(f"ds_list[{k}]: expected a torch.Tensor")
        if not ds.is_cuda:
            raise ValueError(f"ds_list[{k}]: must live on the GPU (got {ds.device}); there is no CPU path")
        if ds.dtype != torch.float32 or ds.dim() != 2 or ds.shape[0] != ds.shape[1]:
            raise ValueError(f"ds_list[{k}]: expected a square float32 matrix, got {ds.dtype} {tuple(ds.shape)}")
        if ds.shape[0] > MAX_N:
            raise ValueError(f"ds_list[{k}]: n = {ds.shape[0]} is outside what the kernels are built for (1..{MAX_N})")
    dev = ds_list[0].device
    sizes_all = [int(ds.shape[0]) for ds in ds_list]
    budgets_all = _budgets(sizes_all, max_steps)
    live = [k for k, n in enumerate(sizes_all) if n > 0]
    mats = [ds_list[k].contiguous() for k in live]
    sizes = [sizes_all[k] for k in live]
    budgets = [budgets_all[k] for k in live]
    if any(m < 1 for m in budgets):
        raise ValueError("max_steps: a budget must be at least 1")
    B, total = len(ds_list), sum(sizes)
    col = torch.empty(total, dtype=torch.int64, device=dev)
    u = torch.empty(total, dtype=torch.float64, device=dev)
    v = torch.empty(total, dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    steps = torch.zeros(B, dtype=torch.int64, device=dev)
    augs = torch.zeros(B, dtype=torch.int64, device=dev)
    if live:
        lib = _lib.load()
        L = len(live)
        n_arr = (C.c_int64 * L)(*sizes)
        ws_bytes = lib.pfpp_match_assign_workspace(L, n_arr)
        if ws_bytes < 0:
            raise ValueError("assign_batch: sizes outside what the kernels are built for")
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        st, sp, ag = (torch.empty(L, dtype=t.dtype, device=dev) for t in (status, steps, augs))
        check(lib.pfpp_match_assign(L, (C.c_void_p * L)(*[m.data_ptr() for m in mats]), n_arr, (C.c_int64 * L)(*budgets), C.c_void_p(col.data_ptr()),
                                    C.c_void_p(u.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(sp.data_ptr()),
                                    C.c_void_p(ag.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, ops._stream()), "pfpp_match_assign")
        if L == B:
            status, steps, augs = st, sp, ag
        else:
            at = torch.tensor(live, dtype=torch.int64, device=dev)
            status[at], steps[at], augs[at] = st, sp, ag
    split = lambda t: list(torch.split(t, sizes_all))
    return AssignOutput(split(col), split(u), split(v), status, steps, augs)


def assign_reference(c, max_steps: Optional[int] = None) -> AssignOutput:
    """the kernels' arithmetic in numpy float64, in their order of operations and with their tie rule: c float32 (or anything numpy
    converts) [n, n] -> AssignOutput of host arrays (col int64, u and v float64, status / steps / augmentations Python ints)"""
    c = np.asarray(c)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"assign_reference: expected a square matrix, got {c.shape}")
    n = c.shape[0]
    budget = default_budget(n) if max_steps is None else int(max_steps)
    if budget < 1:
        raise ValueError("max_steps: a budget must be at least 1")
    cost = -c.astype(np.float64)
    v = np.zeros(n, dtype=np.float64)
    if n == 0:
        return AssignOutput(np.zeros(0, np.int64), v.copy(), v, 0, 0, 0)
    jstar = cost.argmin(1)                                  # the first (lowest) column attaining the minimum
    u = cost[np.arange(n), jstar].copy()
    row4col = np.full(n, -1, dtype=np.int64)
    col4row = np.full(n, -1, dtype=np.int64)
    for i in range(n):                                      # ascending rows: a column keeps the lowest row that asks for it
        if row4col[jstar[i]] < 0:
            row4col[jstar[i]] = i
            col4row[i] = jstar[i]
    steps = augs = status = 0
    inf = np.inf
    for cur in range(n):
        if col4row[cur] >= 0:
            continue
        dist = np.full(n, inf)
        path = np.full(n, -1, dtype=np.int64)
        scanned = np.zeros(n, dtype=bool)
        i, minv, sink = cur, 0.0, -1
        while sink < 0:
            if steps == budget:
                status = 1
                break
            steps += 1
            open_ = ~scanned
            r = ((minv + cost[i]) - u[i]) - v
            better = open_ & (r < dist)
            dist[better] = r[better]
            path[better] = i
            d = np.where(open_, dist, inf)
            cand = open_ & (d == d.min())
            free = cand & (row4col < 0)
            j = int(np.argmax(free)) if free.any() else int(np.argmax(cand))
            minv = dist[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        if status:
            break
        u[cur] = u[cur] + minv
        delta = minv - dist[scanned]
        inner = scanned.copy()
        inner[sink] = False
        u[row4col[inner]] = u[row4col[inner]] + (minv - dist[inner])
        v[scanned] = v[scanned] - delta
        j = sink
        while True:
            r_ = int(path[j])
            row4col[j] = r_
            col4row[r_], j = j, int(col4row[r_])
            if r_ == cur:
                break
        augs += 1
    return AssignOutput(col4row, u, v, status, steps, augs)
