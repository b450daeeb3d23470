"""The rigid term of the matcher's training loss on the GPU (csrc/matching_rigid.hip, include/pfpp.h "the rigid term").

The reference's rigid_loss (Jigsaw_matching/utils/loss.py:59-142) loops over the piece pairs of every puzzle in Python, copies each
block of ds_mat to the host and solves Horn's eigenproblem in numpy (utils/pairwise_alignment.py).  Here:

* RigidBatch: the tables of one batch (pieces' row ranges, the pair list) and the four launches: pair_sums per puzzle, pose_and_fold
  for the batch, grad per puzzle.  Nothing is read back: n_sum depends on which pairs have mat_s == 0 and stays on the device.
* rigid_pairs: RigidBatch on given matrices, for the kernel-level tests.
* MatchingHeadRigidTrainEngine: MatchingHeadTrainEngine with the term (loss_and_grads takes part_pcs) and the reference's
  training_epoch_end switch of the loss weights.

Where the reference's result is not finite - a kept pair with mat_s == 0 (0 / 0 in its translation: a two-piece puzzle, or an
all-zero matrix), or no kept pair in the whole batch (0 / 0 in the mean) - the term is reported as 0 and has zero gradient, the
convention the engine has for its other degenerate inputs."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .matching import _flatten, _gpu, _p, make_layout
from .matching_train import MatchingHeadTrainEngine

MAX_PIECES = 64          # RG_PMAX of csrc/matching_rigid.hip
STATS = 8                # doubles per pair record


class RigidBatch:
    """counts int [B, >= max n_valid]: critical rows per piece; n_valid int [B]; row_off int64 [B + 1]: the puzzles' first rows in
    pts float32 [R, 3] (the critical points of part_pcs, puzzle by puzzle in piece order).  cache (a dict the caller keeps): the
    device tables of the last layout, so that steps over the same layout copy nothing to the device"""

    def __init__(self, counts: np.ndarray, n_valid: Sequence[int], row_off: np.ndarray, pts: torch.Tensor, device, cache: Optional[dict] = None):
        counts = np.asarray(counts, dtype=np.int64)
        n_valid = np.asarray(n_valid, dtype=np.int64).reshape(-1)
        B = n_valid.shape[0]
        P = int(max(n_valid.max(initial=1), 1))
        if P > MAX_PIECES:
            raise ValueError(f"{P} pieces in one puzzle: the rigid kernels are built for at most {MAX_PIECES}")
        self.B, self.P, self.dev = B, P, device
        self.row_off = np.asarray(row_off, dtype=np.int64)
        R = int(self.row_off[-1])
        _gpu(pts, torch.float32, "pts")
        if pts.shape != (R, 3):
            raise ValueError(f"pts: expected [{R}, 3], got {tuple(pts.shape)}")
        self.pts = pts.contiguous()
        cnt = np.zeros((B, P), dtype=np.int64)
        for b in range(B):
            nv = int(n_valid[b])
            cnt[b, :nv] = counts[b, :nv]
            if int(cnt[b].sum()) != int(self.row_off[b + 1] - self.row_off[b]):
                raise ValueError(f"puzzle {b}: the pieces' critical points do not add up to its rows")
        key = (str(device), cnt.tobytes(), n_valid.tobytes(), cnt.shape)
        if cache is not None and cache.get("key") == key:
            tables = cache["tables"]
        else:
            piece_off = np.zeros((B, P + 1), dtype=np.int32)
            piece_off[:, 1:] = np.cumsum(cnt, 1)
            pairs, pair_index = [], np.full((B, P, P), -1, dtype=np.int32)
            for b in range(B):
                for p in range(int(n_valid[b])):
                    for q in range(p + 1, int(n_valid[b])):
                        if cnt[b, p] > 0 and cnt[b, q] > 0:            # utils/loss.py:87-88
                            pair_index[b, p, q] = len(pairs)
                            pairs.append((b, p, q, 0))
            pairs_host = np.asarray(pairs, dtype=np.int32).reshape(-1, 4)
            i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            tables = {"pairs_host": pairs_host, "piece_off_host": piece_off, "piece_off": i32(piece_off), "pair_index": i32(pair_index),
                      "pairs": i32(pairs_host), "n_valid": i32(n_valid.astype(np.int32)), "puz_row_off": torch.from_numpy(self.row_off).to(device)}
            if cache is not None:
                cache.update(key=key, tables=tables)
        self.pairs_host, self.piece_off_host, self.counts_host = tables["pairs_host"], tables["piece_off_host"], cnt
        self.npairs = self.pairs_host.shape[0]
        self.piece_off, self.pair_index, self.pairs = tables["piece_off"], tables["pair_index"], tables["pairs"]
        self.n_valid, self.puz_row_off = tables["n_valid"], tables["puz_row_off"]
        f64 = dict(dtype=torch.float64, device=device)
        self.rb = torch.zeros((max(R, 1), P, 4), **f64)
        self.any_pos = torch.zeros(B, dtype=torch.int32, device=device)
        k = max(self.npairs, 1)
        self.R = torch.zeros((k, 3, 3), dtype=torch.float32, device=device)
        self.t = torch.zeros((k, 3), dtype=torch.float32, device=device)
        self.stats = torch.zeros((k, STATS), **f64)
        self.status = torch.zeros(k, dtype=torch.int32, device=device)
        self.fold = torch.zeros(4, **f64)

    def n(self, b: int) -> int:
        return int(self.row_off[b + 1] - self.row_off[b])

    def pair_sums(self, b: int, ds_mat: torch.Tensor) -> None:
        """(r_i, b_i) of puzzle b's rows against every later piece, from ds_mat float32 [n, n] (rows may be strided)"""
        n = self.n(b)
        _gpu(ds_mat, torch.float32, "ds_mat")
        if ds_mat.shape != (n, n) or (n and ds_mat.stride(1) != 1):
            raise ValueError(f"ds_mat: expected [{n}, {n}] with contiguous rows, got {tuple(ds_mat.shape)}")
        if n == 0:
            return
        r0 = int(self.row_off[b])
        check(_lib.load().pfpp_rigid_pair_sums(_p(ds_mat), ds_mat.stride(0), n, _p(self.pts[r0:]), _p(self.piece_off[b]), self.P, _p(self.rb[r0:]),
                                               _p(self.any_pos[b:]), ops._stream()), "pfpp_rigid_pair_sums")

    def pose_and_fold(self, w_rig_loss: float) -> None:
        """every pair's pose and loss, then fold = (rig_loss, w_rig_loss / n_sum, n_sum, numerator) on the device"""
        lib = _lib.load()
        if self.npairs:
            check(lib.pfpp_rigid_pair_pose(self.npairs, _p(self.pairs), _p(self.puz_row_off), _p(self.piece_off), self.P, _p(self.n_valid),
                                           _p(self.any_pos), _p(self.rb), _p(self.pts), _p(self.R), _p(self.t), _p(self.stats), _p(self.status),
                                           ops._stream()), "pfpp_rigid_pair_pose")
        check(lib.pfpp_rigid_fold(self.npairs, _p(self.stats), _p(self.status), float(w_rig_loss), _p(self.fold), ops._stream()), "pfpp_rigid_fold")

    def grad(self, b: int) -> torch.Tensor:
        """d(w_rig_loss rig_loss) / d ds_mat of puzzle b -> float32 [n, (n + 3) & ~3], zero padding columns: the seed of
        sinkhorn_train_bwd"""
        n = self.n(b)
        ldg = (n + 3) & ~3
        dP = torch.empty((n, ldg), dtype=torch.float32, device=self.dev)
        if n == 0:
            return dP
        if ldg > n:
            dP[:, n:].zero_()
        r0 = int(self.row_off[b])
        check(_lib.load().pfpp_rigid_grad(n, _p(self.pts[r0:]), _p(self.piece_off[b]), self.P, _p(self.rb[r0:]), _p(self.pair_index[b]), _p(self.R),
                                          _p(self.t), _p(self.stats), _p(self.status), _p(self.fold), _p(dP), ldg, ops._stream()), "pfpp_rigid_grad")
        return dP

    def records(self) -> dict:
        """the pair records, one row per pair in pair order (puzzle, p, q)"""
        k = self.npairs
        return {"rigid": self, "rigid_pairs": self.pairs_host[:, :3].copy(), "R": self.R[:k], "t": self.t[:k], "mat_s": self.stats[:k, 0],
                "pair_loss": self.stats[:k, 1], "eigenvalues": self.stats[:k, 2:6], "kept": self.status[:k] == 1, "pair_status": self.status[:k],
                "rig_n_sum": self.fold[2], "rig_scale": self.fold[1]}


def _as_list(x) -> list:
    return list(x) if isinstance(x, (list, tuple)) else [x]


def rigid_pairs(ds_mat, pts, row_piece, n_valid=None, *, w_rig_loss: float = 1.0, need_grad: bool = True) -> dict:
    """the rigid term of given matrices.  ds_mat: float32 [n, n] on the GPU, or a list of them (one per puzzle); pts float32 [n, 3]
    likewise: the critical points in row order; row_piece: the piece of every row (non-decreasing; host or device integers);
    n_valid: pieces per puzzle (default: the last row's piece + 1).
    -> the pair records of RigidBatch.records(), rb (list: fp64 [n, P, 4]), rig_loss / n_sum / scale (0-dim fp64), dP (list of
    float32 [n, n]: d(w_rig_loss rig_loss) / d ds_mat)"""
    mats, points, pieces = _as_list(ds_mat), _as_list(pts), _as_list(row_piece)
    if not (len(mats) == len(points) == len(pieces)):
        raise ValueError("rigid_pairs: one pts and one row_piece per ds_mat")
    for m in mats:
        _gpu(m, torch.float32, "ds_mat")
    dev = mats[0].device
    rp = [np.asarray(p.detach().cpu().numpy() if torch.is_tensor(p) else p, dtype=np.int64).reshape(-1) for p in pieces]
    for b, (m, r) in enumerate(zip(mats, rp)):
        if r.shape[0] != m.shape[0] or (r.size and (np.diff(r) < 0).any()) or (r.size and r[0] < 0):
            raise ValueError(f"puzzle {b}: row_piece needs one non-decreasing piece index per row")
    nv = [int(r[-1]) + 1 if r.size else 0 for r in rp] if n_valid is None else [int(v) for v in _as_list(n_valid)]
    P = max(max(nv), 1)
    counts = np.zeros((len(mats), P), dtype=np.int64)
    for b, r in enumerate(rp):
        if r.size and r[-1] >= nv[b]:
            raise ValueError(f"puzzle {b}: a row of piece {int(r[-1])} but only {nv[b]} valid pieces")
        counts[b, :nv[b]] = np.bincount(r, minlength=nv[b])[:nv[b]] if r.size else 0
    row_off = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    for p_ in points:
        _gpu(p_, torch.float32, "pts")
    all_pts = torch.cat([p_.reshape(-1, 3) for p_ in points]) if points else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    rb = RigidBatch(counts, nv, row_off, all_pts, dev)
    for b, m in enumerate(mats):
        rb.pair_sums(b, m)
    rb.pose_and_fold(w_rig_loss)
    out = rb.records()
    out.update(rb=[rb.rb[int(row_off[b]):int(row_off[b + 1])] for b in range(len(mats))], rig_loss=rb.fold[0], n_sum=rb.fold[2], scale=rb.fold[1],
               numerator=rb.fold[3])
    if need_grad:
        out["dP"] = [rb.grad(b)[:, :m.shape[0]] for b, m in enumerate(mats)]
    return out


class MatchingHeadRigidTrainEngine(MatchingHeadTrainEngine):
    """MatchingHeadTrainEngine with the reference's third loss term: loss = w_cls_loss cls_loss + w_mat_loss mat_loss + w_rig_loss
    rig_loss (joint_seg_align_model.py:379-392).  With the term active (w_mat_loss != 0 and w_rig_loss != 0) loss_and_grads needs
    part_pcs, the network's input points; loss_dict gains rig_loss (fp64) and `saved` the pair records (R, t, mat_s, pair_loss, kept,
    eigenvalues, one row per pair in the order of saved["rigid_pairs"] = (puzzle, p, q)).  With w_mat_loss == 0 the reference returns
    before the term is reached (:221-223, :325-327) and so does this; with w_rig_loss == 0 the step is the base class's, launch for
    launch."""

    _RIGID = True

    def __init__(self, head, *, w_cls_loss: float = 1.0, w_mat_loss: float = 0.0, w_rig_loss: float = 0.0):
        super().__init__(head, w_cls_loss=w_cls_loss, w_mat_loss=w_mat_loss, w_rig_loss=w_rig_loss)
        self._rigid_tables: dict = {}          # RigidBatch's device tables of the last layout

    def loss_and_grads(self, part_feats, gt_pcs, n_pcs, part_valids, *, critical_label_thresholds=None, critical_label=None, part_pcs=None):
        """as MatchingHeadTrainEngine.loss_and_grads; part_pcs float32 [B, N, 3] (or a list / flat, like gt_pcs) on the GPU"""
        if self.w_rig_loss == 0 or self.w_mat_loss == 0:
            return self._step(part_feats, gt_pcs, n_pcs, part_valids, critical_label_thresholds, critical_label, None)
        if part_pcs is None:
            raise ValueError("part_pcs is needed while w_rig_loss is not 0: the rigid term aligns the network's input points")
        pfirst = part_pcs[0] if isinstance(part_pcs, (list, tuple)) else part_pcs
        _gpu(pfirst, torch.float32, "part_pcs")
        layout = make_layout(n_pcs, pfirst.device)
        flat = _flatten(part_pcs, layout, 3, "part_pcs")
        make = lambda counts, n_valid, row_off, src, dev: RigidBatch(counts, n_valid, row_off, flat.index_select(0, src), dev, cache=self._rigid_tables)
        return self._step(part_feats, gt_pcs, n_pcs, part_valids, critical_label_thresholds, critical_label, make)

    def on_epoch_end(self, epoch: int, mat_epoch: int = 9, rig_epoch: int = 199) -> None:
        """the reference's training_epoch_end (:453-463): a weight that is 0 becomes 1.0 once epoch >= its epoch"""
        if self.w_mat_loss == 0 and epoch >= mat_epoch:
            self.w_mat_loss = 1.0
        if self.w_rig_loss == 0 and epoch >= rig_epoch:
            self.w_rig_loss = 1.0
