"""The matcher's edges and correspondences on the device (csrc/matching_edges.hip, include/pfpp.h "matcher, edges and correspondences").

The reference turns every puzzle's assignment into `edges` and per-edge correspondence lists on the host
(Jigsaw_matching/model/modules/matching_base_model.py:298-359; here pfpp_hip.matching.match_edges), writes them to
matching_data/<id>.npz, and the assembly loop flattens the lists again and uploads them (AutoAgglomerative.prepare_matching,
puzzlefusion_plusplus/auto_aggl.py:92-126).  With the assignment solved on the device (MatchingHead.forward(solver="device")) that
pair rule is the only reason the matches leave the GPU.  Here:

* match_edges_batch: all puzzles of a batch in one launch of pfpp_match_edges -> DeviceMatches.  One small read-back (status, the kept
  flags and the offsets: (2 T + 2) words per puzzle, T = P (P - 1) / 2); no correspondence passes through the host.
* DeviceMatches.files(b): what match_edges returns, for the file.  DeviceMatches.prepared(b): what prepare_matching returns, as views
  of the kernel's outputs, for AutoAgglomerative (data_dict["matching_prepared"]).
* DeviceMatches.batch_prepared() -> BatchMatches: the same for the whole batch as one set of tensors (data_dict["matching_batch"] =
  (object, b)); the loop then builds the verifier input of all its puzzles with one pfpp_edge_features_batch launch.
* pack_matches_reference: the kernel's output arrays in numpy, built from match_edges and prepare_matching: the parity target.
* match_edges_launch: the entry on caller-allocated tensors (tests place canaries around them).
"""
from __future__ import annotations

import ctypes as C
import itertools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_P, MAX_ROWS, MAX_PUZZLES = 32, 65535, 65535          # PFPP_MATCH_EDGES_MAX_P / _MAX_ROWS / _MAX_PUZZLES of include/pfpp.h
STATUS_TEXT = {1: "the assignment is not injective on its matched rows",
               2: "an entry of the assignment lies outside [-1, N'), or the puzzle's sizes contradict each other"}


def triangle_pairs(P: int) -> np.ndarray:
    """int64 [P (P - 1) / 2, 2]: (idx1, idx2), idx1 < idx2, in the row-major order of the verifier's edge slots"""
    return np.asarray(list(itertools.combinations(range(P), 2)), dtype=np.int64).reshape(-1, 2)


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


# ------------------------------------------------------------------------------------------------------------------ the oracle
def pack_matches_reference(perm: Sequence, n_critical_pcs, n_valid, n_pcs, critical_pcs_idx, *, fill: int = -1) -> Dict[str, np.ndarray]:
    """pfpp_match_edges' outputs in numpy from pfpp_hip.matching.match_edges and AutoAgglomerative.prepare_matching (host data only).
    perm: per puzzle the assignment as int [N'_b] (-1 = unmatched; empty = no rows); n_critical_pcs, n_pcs [B, P]; n_valid [B];
    critical_pcs_idx: per puzzle int [sum n_pcs[b]] (or longer).  -> counts [B, P, P], edge_off [B, T + 1], kept [B, T], corr [R, 2],
    idx_a, idx_b [R], status [B] (all int32) and row_off int64 [B + 1]; entries of corr / idx_a / idx_b behind a puzzle's last
    correspondence hold `fill` (the kernel leaves them alone)"""
    import torch

    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative

    from .matching import match_edges

    perm = [_host(p).astype(np.int64).reshape(-1) for p in perm]
    nc, n_pcs = _host(n_critical_pcs).astype(np.int64), _host(n_pcs).astype(np.int64)
    n_valid = _host(n_valid).astype(np.int64).reshape(-1)
    B, P = n_pcs.shape
    nc = nc.reshape(B, P)
    T = P * (P - 1) // 2
    tri = triangle_pairs(P)
    row_off = np.concatenate([[0], np.cumsum([p.size for p in perm])]).astype(np.int64)
    R = int(row_off[-1])
    out = {"counts": np.zeros((B, P, P), np.int32), "edge_off": np.zeros((B, T + 1), np.int32), "kept": np.zeros((B, T), np.int32),
           "corr": np.full((R, 2), fill, np.int32), "idx_a": np.full(R, fill, np.int32), "idx_b": np.full(R, fill, np.int32),
           "status": np.zeros(B, np.int32), "row_off": row_off}
    for b in range(B):
        col, n = perm[b], perm[b].size
        if not 0 <= n_valid[b] <= P or (nc[b] < 0).any() or (nc[b] > n_pcs[b]).any() or n > nc[b].sum() or ((col < -1) | (col >= n)).any():
            out["status"][b] = 2
            continue
        rows = np.nonzero(col >= 0)[0]
        if np.unique(col[rows]).size != rows.size:
            out["status"][b] = 1
            continue
        piece = np.repeat(np.arange(P), nc[b])
        np.add.at(out["counts"][b], (piece[rows], piece[col[rows]]), 1)
        edges, corr = match_edges(col, nc[b], int(n_valid[b]))
        crit = _host(critical_pcs_idx[b]).astype(np.int64).reshape(-1)
        prep = AutoAgglomerative.prepare_matching({"n_pcs": torch.from_numpy(n_pcs[b:b + 1]), "critical_pcs_idx": torch.from_numpy(crit[None]),
                                                   "edges": torch.from_numpy(edges[None]), "correspondences": corr}, "cpu")
        pos = prep["pair_pos"].numpy()
        assert edges.shape[0] == 0 or (np.diff(pos) > 0).all()            # match_edges walks the pairs in the slots' order
        m = np.zeros(T, np.int64)
        m[pos] = np.diff(prep["edge_off"].numpy())
        out["kept"][b, pos] = 1
        out["edge_off"][b, 1:] = np.cumsum(m)
        M, r0 = int(m.sum()), int(row_off[b])
        assert M <= n
        if M:
            out["corr"][r0:r0 + M] = np.concatenate(corr, 0)
            out["idx_a"][r0:r0 + M], out["idx_b"][r0:r0 + M] = prep["idx_a"].numpy(), prep["idx_b"].numpy()
    return out


# ------------------------------------------------------------------------------------------------------------------ the launch
def match_edges_launch(col, row_off, n_critical_pcs, n_valid, piece_off, critical_pcs_idx, *, B: int, P: int, max_rows: int,
                       total_rows: int, total_points: int, counts, edge_off, kept, corr, idx_a, idx_b, status) -> None:
    """pfpp_match_edges on tensors the caller allocated (shapes and dtypes of include/pfpp.h; col may be a slice of a larger
    allocation).  Raises pfpp_hip._lib.PfppError when the entry refuses the call."""
    import torch

    from . import _lib, ops
    from ._lib import check

    lib = _lib.load()
    ws_bytes = lib.pfpp_match_edges_workspace(int(total_rows))
    if ws_bytes < 0:
        raise ValueError("match_edges_launch: negative total_rows")
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=status.device)
    p = lambda t: C.c_void_p(0 if t is None or t.numel() == 0 else t.data_ptr())
    check(lib.pfpp_match_edges(p(col), p(row_off), p(n_critical_pcs), p(n_valid), p(piece_off), p(critical_pcs_idx), int(B), int(P),
                               int(max_rows), int(total_rows), int(total_points), p(counts), p(edge_off), p(kept), p(corr), p(idx_a),
                               p(idx_b), p(status), C.c_void_p(ws.data_ptr()), ws_bytes, ops._stream()), "pfpp_match_edges")


class DeviceMatches:
    """pfpp_match_edges' outputs for a batch (device tensors) and the small part of them the host holds (status, kept, offsets)"""

    def __init__(self, *, n_pcs: np.ndarray, row_off: np.ndarray, counts, edge_off, kept, corr, idx_a, idx_b, status,
                 host: Optional[np.ndarray] = None):
        self.n_pcs, self.row_off = n_pcs, row_off
        self.B, self.P = n_pcs.shape
        self.T = self.P * (self.P - 1) // 2
        self.counts, self.edge_off, self.kept, self.corr, self.idx_a, self.idx_b, self.status = counts, edge_off, kept, corr, idx_a, idx_b, status
        B, T = self.B, self.T
        if host is None:                                  # status | kept | edge_off, as match_edges_batch reads them back in one copy
            host = np.concatenate([_host(status).reshape(-1), _host(kept).reshape(-1), _host(edge_off).reshape(-1)])
        self.status_host = host[:B]
        self.kept_host = host[B:B + B * T].reshape(B, T)
        self.edge_off_host = host[B + B * T:].reshape(B, T + 1)
        self._tri = triangle_pairs(self.P)

    @classmethod
    def from_arrays(cls, out: dict, n_pcs) -> "DeviceMatches":
        """from a dict of the entry's arrays (pack_matches_reference's, or tensors a test launched into): files() works on either,
        prepared() needs device tensors"""
        return cls(n_pcs=_host(n_pcs).astype(np.int64), row_off=_host(out["row_off"]).astype(np.int64),
                   **{k: out[k] for k in ("counts", "edge_off", "kept", "corr", "idx_a", "idx_b", "status")})

    def n_correspondences(self, b: int) -> int:
        return int(self.edge_off_host[b, self.T])

    def files(self, b: int) -> Tuple[np.ndarray, List[np.ndarray]]:
        """(edges int64 [E, 2] = (idx2, idx1), [int64 [M, 2]]) of puzzle b: what pfpp_hip.matching.match_edges returns"""
        slots = np.nonzero(self.kept_host[b])[0]
        r0, off = int(self.row_off[b]), self.edge_off_host[b]
        corr = _host(self.corr[r0:r0 + self.n_correspondences(b)]).astype(np.int64)
        return (np.ascontiguousarray(self._tri[slots][:, ::-1]).reshape(-1, 2),
                [corr[int(off[s]):int(off[s + 1])] for s in slots])

    def prepared(self, b: int) -> dict:
        """AutoAgglomerative.prepare_matching's dict for puzzle b (same keys, dtypes and values): idx_a / idx_b are views of the
        kernel's outputs, edge_off one index_select of its offsets; `pairs`, `max_m` and `pair_pos` come from the kept flags and
        offsets the host already holds.  pair_pos counts in the P slots of THIS batch: the assembly loop needs P = its max_num_part."""
        import torch

        dev = self.idx_a.device
        slots = np.nonzero(self.kept_host[b])[0]
        r0, M, off = int(self.row_off[b]), self.n_correspondences(b), self.edge_off_host[b]
        sel = torch.from_numpy(np.concatenate([slots, [self.T]]).astype(np.int64)).to(dev)
        point_part = np.repeat(np.arange(self.P), self.n_pcs[b]).astype(np.int32)
        return {"idx_a": self.idx_a[r0:r0 + M], "idx_b": self.idx_b[r0:r0 + M], "edge_off": self.edge_off[b].index_select(0, sel),
                "max_m": int((off[slots + 1] - off[slots]).max()) if slots.size else 0,
                "pairs": [(int(i1), int(i2)) for i1, i2 in self._tri[slots]],
                "point_part": torch.from_numpy(point_part).to(dev), "pair_pos": sel[:-1]}

    def batch_prepared(self) -> "BatchMatches":
        """what the assembly loop needs of ALL puzzles of the batch as one set of tensors (data_dict["matching_batch"] = (this, b)):
        one upload, no tensor work per puzzle; the kernel's outputs are used as they are"""
        return BatchMatches(self)


class BatchMatches:
    """The matches of a DeviceMatches batch as AutoAgglomerative.test_batch takes them: every puzzle b travels as
    data_dict["matching_batch"] = (this object, b).

    idx_a, idx_b, edge_off [B, T + 1]: the kernel's outputs (no copy); row_off, pt_off int64 [B + 1]: the puzzles' first rows / first
    by-area points; point_part int32 [sum N]: the piece of every point; pivot int32 [B, P], arange(P) per puzzle: the loop's pivots
    (a merge writes them through its puzzle's view); pts float32 [sum N, 3]: the by-area points of the batch in the pieces' current
    frames (every puzzle's state fills its slice and a merge rewrites it through its view); max_m: the longest slot of the batch.
    The four index arrays come from ONE upload.  A deep copy is the object itself: a dataset sample that carries it is deep-copied
    per __getitem__, and the states of one call must share one object."""

    def __init__(self, dm: DeviceMatches):
        import torch

        dev = dm.idx_a.device
        B, P, T = dm.B, dm.P, dm.T
        self.dm, self.B, self.P, self.T = dm, B, P, T
        n_pcs = np.asarray(dm.n_pcs, dtype=np.int64)
        self.n_points = n_pcs.sum(1)
        self.pt_off_host = np.concatenate([[0], np.cumsum(self.n_points)]).astype(np.int64)
        self.row_off_host = np.ascontiguousarray(dm.row_off, dtype=np.int64)
        total = int(self.pt_off_host[-1])
        slot = np.tile(np.arange(P, dtype=np.int32), B)
        point_part = np.repeat(slot, n_pcs.reshape(-1))
        # index of a point's pivot in the flat [B P] pivot table
        point_slot = point_part + np.repeat(np.arange(B, dtype=np.int32) * P, self.n_points)
        # the int64 offsets first (8-byte aligned), then the int32 arrays: pt_off | row_off | pivot | point_part | point_slot
        blob = torch.from_numpy(np.concatenate([self.pt_off_host.view(np.int32), self.row_off_host.view(np.int32), slot, point_part,
                                                point_slot])).to(dev)
        n64 = 2 * (B + 1)
        off64 = blob[:2 * n64].view(torch.int64)
        self.pt_off, self.row_off = off64[:B + 1], off64[B + 1:]
        self.pivot = blob[2 * n64:2 * n64 + B * P].view(B, P)
        self.point_part = blob[2 * n64 + B * P:2 * n64 + B * P + total]
        self.point_slot = blob[2 * n64 + B * P + total:]
        self.idx_a, self.idx_b, self.edge_off = dm.idx_a, dm.idx_b, dm.edge_off
        self.max_m = int(np.diff(dm.edge_off_host, axis=1).max()) if T else 0
        self.pts = torch.zeros((total, 3), dtype=torch.float32, device=dev)

    def __deepcopy__(self, memo):
        return self

    def points(self, b: int):
        """puzzle b's slice of pts, [N_b, 3] (a view)"""
        return self.pts[int(self.pt_off_host[b]):int(self.pt_off_host[b + 1])]


def _flat(ts):
    """the 1-D tensors one behind the other: without a copy when they are consecutive slices of one allocation (what torch.split
    returns: the head's critical_pcs_idx, the device solver's col), torch.cat otherwise"""
    import torch

    first, off = ts[0], ts[0].storage_offset()
    for t in ts:
        if t.untyped_storage().data_ptr() != first.untyped_storage().data_ptr() or not t.is_contiguous() or t.storage_offset() != off:
            return torch.cat(ts)
        off += t.numel()
    return first.as_strided((off - first.storage_offset(),), (1,))


def match_edges_batch(perm, n_critical_pcs, n_valid, layout_or_n_pcs, critical_pcs_idx) -> DeviceMatches:
    """perm: the perm_mat list of a HeadOutput made with dense_perm=False (per puzzle int64 [N'_b] on the GPU, empty = no rows), or
    an AssignOutput; n_critical_pcs int64 [B, P] (device, as the head returns it); n_valid [B] (host); layout_or_n_pcs: the head's
    Layout or n_pcs [B, P]; critical_pcs_idx: per puzzle int64 [N_b] or flat [sum N] (device).  Raises ValueError for a dense perm
    and for a puzzle whose status is not 0."""
    import torch

    from .matching import Layout, make_layout

    perm = list(perm.col if hasattr(perm, "col") else perm)
    if not perm:
        raise ValueError("match_edges_batch: no puzzles")
    for b, c in enumerate(perm):
        if not isinstance(c, torch.Tensor):
            raise TypeError(f"perm[{b}]: expected a torch.Tensor")
        if c.dim() == 2:
            raise ValueError(f"perm[{b}]: a dense permutation matrix {tuple(c.shape)}; pass dense_perm=False to the head (one column per row)")
        if c.dim() != 1 or c.dtype != torch.int64:
            raise ValueError(f"perm[{b}]: expected int64 [N'], got {c.dtype} {tuple(c.shape)}")
        if c.numel() and not c.is_cuda:
            raise ValueError(f"perm[{b}]: must live on the GPU (got {c.device}); there is no CPU path")
    if not isinstance(n_critical_pcs, torch.Tensor) or not n_critical_pcs.is_cuda or n_critical_pcs.dtype != torch.int64:
        raise ValueError("n_critical_pcs: expected an int64 tensor on the GPU")
    dev = n_critical_pcs.device
    layout = layout_or_n_pcs if isinstance(layout_or_n_pcs, Layout) else make_layout(layout_or_n_pcs, dev)
    B, P = layout.n_pcs.shape
    if len(perm) != B or n_critical_pcs.numel() != B * P:
        raise ValueError(f"match_edges_batch: {len(perm)} assignments and n_critical_pcs of {n_critical_pcs.numel()} entries for n_pcs {B} x {P}")
    n_valid = _host(n_valid).astype(np.int64).reshape(-1)
    if n_valid.size != B:
        raise ValueError("n_valid: one count per puzzle")
    crit = _flat(list(critical_pcs_idx)) if isinstance(critical_pcs_idx, (list, tuple)) else critical_pcs_idx.reshape(-1)
    if not crit.is_cuda or crit.dtype != torch.int64 or crit.numel() != int(layout.puz_points.sum()):
        raise ValueError("critical_pcs_idx: expected int64 on the GPU, one entry per point of the batch")
    sizes = [int(c.numel()) for c in perm]
    if not 1 <= P <= MAX_P or max(sizes) > MAX_ROWS or B > MAX_PUZZLES:
        raise ValueError(f"match_edges_batch: P = {P}, {max(sizes)} rows, {B} puzzles: outside what the kernel is built for "
                         f"(P <= {MAX_P}, rows <= {MAX_ROWS}, puzzles <= {MAX_PUZZLES})")
    live = [c for c in perm if c.numel()]
    col = _flat(live) if live else torch.empty(0, dtype=torch.int64, device=dev)
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    R, T = int(row_off[-1]), P * (P - 1) // 2
    meta = torch.from_numpy(np.concatenate([row_off, n_valid])).to(dev)                 # one upload: row_off | n_valid
    small = torch.empty(B + B * T + B * (T + 1), dtype=torch.int32, device=dev)         # one read-back: status | kept | edge_off
    status, kept, edge_off = small[:B], small[B:B + B * T].view(B, T), small[B + B * T:].view(B, T + 1)
    counts = torch.empty((B, P, P), dtype=torch.int32, device=dev)
    corr = torch.empty((R, 2), dtype=torch.int32, device=dev)
    idx_a, idx_b = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    match_edges_launch(col.contiguous(), meta[:B + 1], n_critical_pcs.contiguous(), meta[B + 1:], layout.piece_off, crit.contiguous(), B=B, P=P,
                       max_rows=max(sizes), total_rows=R, total_points=crit.numel(), counts=counts, edge_off=edge_off, kept=kept, corr=corr,
                       idx_a=idx_a, idx_b=idx_b, status=status)
    host = small.cpu().numpy()
    bad = np.nonzero(host[:B])[0]
    if bad.size:
        raise ValueError("match_edges_batch: " + "; ".join(f"puzzle {int(b)}: status {int(host[b])} ({STATUS_TEXT.get(int(host[b]), '?')})" for b in bad))
    return DeviceMatches(n_pcs=layout.n_pcs, row_off=row_off, counts=counts, edge_off=edge_off, kept=kept, corr=corr, idx_a=idx_a, idx_b=idx_b,
                         status=status, host=host)
