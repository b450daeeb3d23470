"""The matcher's back end: per-point descriptors -> matching_data (csrc/matching.hip, include/pfpp.h "matcher back end").

The test-time path of the reference's Jigsaw_matching/model/jigsaw/joint_seg_align_model.py:164-278 behind the descriptor network,
and model/modules/matching_base_model.py:298-361, 614-640 up to the file:

* MatchingHead: fracture-point classifier, critical points, affinity features, dual affinity, same-piece mask, Sinkhorn (on the
  GPU, ragged over the puzzles of a batch) and the optimal assignment (scipy on the host, overlapped with the next puzzle's GPU work;
  with solver="device" the exact batched solver of pfpp_hip/matching_assign.py instead).
* sinkhorn / fracture_labels: the two kernels on their own.
* match_edges: the piece-pair rule that turns the assignment into `edges` and `correspondence` (host: O(N') integer work on an
  array the host already holds for the assignment; pfpp_hip.matching_edges runs the same rule on the device for an assignment
  that was solved there).
* write_matching_data: the file, through io.save_matching_data; an existing file is left alone, as in the reference.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
import types
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check
from .io import save_matching_data

PC_FEAT_DIM = 128
AFF_FEAT_DIM = 512
HEAD_PREFIXES = ("pc_classifier.", "affinity_extractor.", "affinity_layer.")


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _gpu(t: torch.Tensor, dtype: torch.dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    return t


class Layout(NamedTuple):
    """CSR description of a ragged batch: pieces in slot order, empty slots as empty ranges"""

    n_pcs: np.ndarray            # int64 [B, P] (host)
    piece_off: torch.Tensor      # int64 [B P + 1] point offsets of the pieces (device)
    puz_piece_off: torch.Tensor  # int64 [B + 1]
    piece_slot: torch.Tensor     # int32 [B P]
    puz_points: np.ndarray       # int64 [B] (host)


def make_layout(n_pcs, device, total_points: Optional[int] = None) -> Layout:
    n = np.asarray(n_pcs.detach().cpu().numpy() if torch.is_tensor(n_pcs) else n_pcs).astype(np.int64)
    if n.ndim != 2 or (n < 0).any():
        raise ValueError("n_pcs: expected non-negative [B, P]")
    B, P = n.shape
    off = np.concatenate([[0], np.cumsum(n.reshape(-1))]).astype(np.int64)
    if total_points is not None and int(off[-1]) != total_points:
        raise ValueError(f"n_pcs sums to {int(off[-1])} points, the batch has {total_points}")
    dev = torch.device(device)
    return Layout(n, torch.from_numpy(off).to(dev), torch.arange(0, (B + 1) * P, P, dtype=torch.int64, device=dev),
                  torch.arange(P, dtype=torch.int32, device=dev).repeat(B), n.sum(1))


def _flatten(x, layout: Layout, width: int, name: str) -> torch.Tensor:
    """[B, N, w], a list of [N_b, w] or flat [sum N, w] -> contiguous flat [sum N, w] whose puzzle sizes match the layout"""
    if isinstance(x, (list, tuple)):
        sizes = [int(t.shape[0]) for t in x]
        x = torch.cat(list(x), 0) if len(x) != 1 else x[0]
    elif x.dim() == 3:
        sizes = [int(x.shape[1])] * int(x.shape[0])
        x = x.reshape(-1, x.shape[-1])
    else:
        sizes = None
    if x.dim() != 2 or x.shape[1] != width:
        raise ValueError(f"{name}: expected [..., {width}], got {tuple(x.shape)}")
    if sizes is not None and sizes != layout.puz_points.tolist():
        raise ValueError(f"{name}: puzzles of {sizes} points, n_pcs sums to {layout.puz_points.tolist()}")
    if x.shape[0] != int(layout.puz_points.sum()):
        raise ValueError(f"{name}: {x.shape[0]} points, n_pcs sums to {int(layout.puz_points.sum())}")
    return x.contiguous()


# ------------------------------------------------------------------------------------------------------------------ kernels
def critical_points(labels: torch.Tensor, layout: Layout) -> Tuple[torch.Tensor, torch.Tensor]:
    """get_critical_pcs_from_label of given labels (uint8 [N]) -> (critical_pcs_idx int64 [N], n_critical_pcs int64 [B P])"""
    _gpu(labels, torch.uint8, "labels")
    labels = labels.contiguous()
    dev = labels.device
    Pt = layout.piece_slot.numel()
    crit = torch.empty(labels.numel(), dtype=torch.int64, device=dev)
    n_crit = torch.empty(Pt, dtype=torch.int64, device=dev)
    check(_lib.load().pfpp_match_classify_compact(None, None, None, None, 0.0, _p(labels), _p(layout.piece_off), Pt, PC_FEAT_DIM, None,
                                                  None, _p(crit), _p(n_crit), ops._stream()), "pfpp_match_classify_compact")
    return crit, n_crit


def sinkhorn(s: torch.Tensor, piece_of_row: torch.Tensor, *, tau: float = 0.05, max_iter: int = 20, check_pieces: bool = True) -> torch.Tensor:
    """masked log-domain Sinkhorn of one puzzle: s float32 [n, n] (rows may be strided), piece_of_row int32 [n] -> ds_mat [n, n];
    entries whose row and column belong to one piece are exactly 0.  At least two pieces must own rows: with one piece every entry
    is masked, which is refused (check_pieces reads two numbers back from the device; a caller that knows the counts turns it off)."""
    _gpu(s, torch.float32, "s")
    _gpu(piece_of_row, torch.int32, "piece_of_row")
    if s.dim() != 2 or s.shape[0] != s.shape[1] or s.stride(1) != 1 or s.shape[0] < 1:
        raise ValueError(f"s: expected a square matrix with contiguous rows, got {tuple(s.shape)}")
    n = s.shape[0]
    if piece_of_row.shape != (n,):
        raise ValueError("piece_of_row: one piece id per row")
    piece = piece_of_row.contiguous()
    if check_pieces and int(piece.min()) == int(piece.max()):
        raise ValueError("sinkhorn: all rows belong to one piece, every entry is masked (the caller skips such a puzzle)")
    lib = _lib.load()
    ws_bytes = lib.pfpp_sinkhorn_workspace(n)
    if ws_bytes < 0:
        raise ValueError(f"sinkhorn: n = {n} is outside what the kernels are built for")
    dev = s.device
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=dev)
    uv = torch.empty((2, n), dtype=torch.float64, device=dev)
    ds = torch.empty((n, n), dtype=torch.float32, device=dev)
    check(lib.pfpp_sinkhorn_masked(_p(s), s.stride(0), _p(piece), n, float(tau), int(max_iter), _p(uv[0]), _p(uv[1]),
                                   _p(ds), _p(ws), ws.numel() * 4, ops._stream()), "pfpp_sinkhorn_masked")
    return ds


def fracture_labels(gt_pcs, n_pcs, thresholds, *, return_dist: bool = False):
    """compute_label (joint_seg_align_model.py:465-484): gt_pcs [B, N, 3] (or flat / a list), n_pcs [B, P], thresholds [B, N] ->
    labels int64 of thresholds' shape: 1 where the nearest point of ANOTHER piece of the puzzle is closer than the threshold"""
    first = gt_pcs[0] if isinstance(gt_pcs, (list, tuple)) else gt_pcs
    _gpu(first, torch.float32, "gt_pcs")
    layout = make_layout(n_pcs, first.device)
    pts = _flatten(gt_pcs, layout, 3, "gt_pcs")
    thr = torch.cat([t.reshape(-1) for t in thresholds]) if isinstance(thresholds, (list, tuple)) else thresholds
    _gpu(thr, torch.float32, "thresholds")
    if thr.numel() != pts.shape[0]:
        raise ValueError("thresholds: one per point")
    shape = thr.shape
    thr = thr.reshape(-1).contiguous()
    lab = torch.empty(pts.shape[0], dtype=torch.uint8, device=pts.device)
    dist = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
    B = layout.n_pcs.shape[0]
    check(_lib.load().pfpp_fracture_labels(_p(pts), _p(layout.piece_off), _p(layout.puz_piece_off), _p(thr), B,
                                           int(layout.puz_points.max(initial=0)), _p(dist), _p(lab), ops._stream()), "pfpp_fracture_labels")
    lab = lab.to(torch.int64).reshape(shape)
    return (lab, dist.reshape(shape)) if return_dist else lab


# ------------------------------------------------------------------------------------------------------------------ host side
def match_edges(perm, n_critical_pcs, n_valid: int) -> Tuple[np.ndarray, List[np.ndarray]]:
    """matching_base_model.py:298-359 up to the _save_data call.  perm: the assignment as one column index per row (int [N'], -1 =
    unmatched) or the dense 0/1 matrix; n_critical_pcs [P]; n_valid pieces.  -> (edges int64 [E, 2] = (idx2, idx1), correspondence =
    list of int64 [M, 2] (row-major nonzero of the pair's block))"""
    perm = np.asarray(perm.detach().cpu().numpy() if torch.is_tensor(perm) else perm)
    if perm.ndim == 2:
        rows, cols = np.nonzero(perm)
    else:
        rows = np.nonzero(perm >= 0)[0]
        cols = perm[rows].astype(np.int64)
    nc = np.asarray(n_critical_pcs.detach().cpu().numpy() if torch.is_tensor(n_critical_pcs) else n_critical_pcs).astype(np.int64).reshape(-1)
    n_valid = int(n_valid)
    start = np.cumsum(nc) - nc
    piece = np.repeat(np.arange(nc.size), nc)
    edges, corr = [], []
    if rows.size and (rows.max() >= piece.size or cols.max() >= piece.size):
        raise ValueError("match_edges: the assignment is larger than sum(n_critical_pcs)")
    pr, pc = piece[rows], piece[cols]
    counts = np.zeros((nc.size, nc.size), dtype=np.int64)
    np.add.at(counts, (pr, pc), 1)
    total = int(rows.size)
    for idx1 in range(n_valid):
        for idx2 in range(idx1 + 1, n_valid):
            if nc[idx1] == 0 or nc[idx2] == 0:
                continue
            mat_s, mat_s2 = counts[idx1, idx2], counts[idx2, idx1]
            if mat_s < mat_s2:          # the transposed opposite block wins (ties keep the first)
                sel = (pr == idx2) & (pc == idx1)
                c = np.stack([cols[sel] - start[idx1], rows[sel] - start[idx2]], 1)
                mat_s = mat_s2
            else:
                sel = (pr == idx1) & (pc == idx2)
                c = np.stack([rows[sel] - start[idx1], cols[sel] - start[idx2]], 1)
            if n_valid > 2 and mat_s == 0 and total > 0:
                continue
            if c.shape[0] < 3:
                continue
            c = c[np.lexsort((c[:, 1], c[:, 0]))]
            edges.append([idx2, idx1])
            corr.append(c.astype(np.int64))
    return np.asarray(edges, dtype=np.int64).reshape(-1, 2), corr


def write_matching_data(out_dir: str, data_id: int, *, edges, correspondence: Sequence[np.ndarray], gt_pcs, critical_pcs_idx, n_pcs,
                        n_critical_pcs) -> Optional[str]:
    """_save_data (matching_base_model.py:614-640): <out_dir>/<data_id>.npz; None when the file exists (it is left alone)"""
    path = os.path.join(out_dir, f"{int(data_id)}.npz")
    if os.path.exists(path):
        return None
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return save_matching_data(out_dir, int(data_id), edges=host(edges), correspondence=[host(c) for c in correspondence], gt_pcs=host(gt_pcs),
                              critical_pcs_idx=host(critical_pcs_idx).astype(np.int64), n_pcs=host(n_pcs).astype(np.int64),
                              n_critical_pcs=host(n_critical_pcs).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------------ the head
class _Opaque(dict):
    """stands for an object of a checkpoint whose class cannot be imported here (the matcher's `hyper_parameters` hold its cfg, an
    easydict.EasyDict: matching_base_model.py:19-22).  Takes whatever its pickle hands it and is never looked at."""

    def __init__(self, *args, **kwargs):
        super().__init__()

    def __setstate__(self, state):
        pass

    def __call__(self, *args, **kwargs):
        return _Opaque()


class _TolerantUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            return _Opaque


_tolerant_pickle = types.SimpleNamespace(__name__="pickle", Unpickler=_TolerantUnpickler,
                                         load=lambda f, **kw: _TolerantUnpickler(f, **kw).load())


def load_checkpoint_state_dict(path: str) -> dict:
    """the `state_dict` of a Lightning checkpoint, or the file's content when it is a bare state_dict.  A file of tensors and plain
    containers loads with weights_only=True.  A real Jigsaw checkpoint also carries `hyper_parameters` with an EasyDict, which that
    mode refuses: such a file is unpickled in full (like the other Lightning files of this tree, pfpp_hip/launch.py), with classes
    that are not installed here replaced by a placeholder, and only the state_dict is kept."""
    return _state_dict_of(_read_checkpoint(path), path)


def _read_checkpoint(path: str):
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        try:
            return torch.load(path, map_location="cpu", weights_only=False, pickle_module=_tolerant_pickle)
        except Exception as e:
            raise RuntimeError(f"{path}: not a checkpoint this loader can read ({type(e).__name__}: {e})") from e


def _state_dict_of(ckpt, path: str) -> dict:
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    if not isinstance(sd, dict) or not all(torch.is_tensor(v) for v in sd.values()):
        raise RuntimeError(f"{path}: no state_dict of tensors found (top-level keys: {list(ckpt)[:8] if isinstance(ckpt, dict) else type(ckpt).__name__})")
    return sd


def checkpoint_encoder_arch(ckpt, sd: dict) -> str:
    """which encoder a matcher checkpoint was trained with: MODEL.ENCODER of its `hyper_parameters` (directly, or under `cfg` as
    Lightning's save_hyperparameters() files it: matching_base_model.py:19-22) when the file has it and it is a string; otherwise
    "dgcnn.dynamic" when the state_dict holds encoder.conv5.0.weight, which only that family has, and the default encoder when not"""
    hp = ckpt.get("hyper_parameters") if isinstance(ckpt, dict) and "state_dict" in ckpt else None
    for cfg in (hp, hp.get("cfg") if isinstance(hp, dict) else None):
        model = cfg.get("MODEL") if isinstance(cfg, dict) else None
        arch = model.get("ENCODER") if isinstance(model, dict) else None
        if isinstance(arch, str):
            return arch
    return "dgcnn.dynamic" if "encoder.conv5.0.weight" in sd else DEFAULT_ENCODER


class _AffinityDual(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.A = nn.Parameter(torch.eye(d // 2))


class HeadOutput(NamedTuple):
    cls_logits: List[torch.Tensor]         # per puzzle float32 [N_b, 1]
    cls_pred: List[torch.Tensor]           # per puzzle int64 [N_b]
    critical_pcs_idx: List[torch.Tensor]   # per puzzle int64 [N_b]
    n_critical_pcs: torch.Tensor           # int64 [B, P]
    ds_mat: List[torch.Tensor]             # per puzzle float32 [N'_b, N'_b] ([0, 0] when fewer than two pieces have critical points)
    perm_mat: List[torch.Tensor]           # per puzzle 0/1 float32 [N'_b, N'_b], or int64 [N'_b] column per row with dense_perm=False
    timings: dict


class MatchingHead(nn.Module):
    """pc_classifier, affinity_extractor and affinity_layer of JointSegmentationAlignmentModel with the reference's parameter names,
    and its test-time forward behind part_feats.  gemm_mode: arithmetic of the three products, "f32" (exact fp32 matrix
    instructions, the default: log_s = s / tau multiplies the product's error by 20) or "f16x3" (split-f16)."""

    def __init__(self, tau: float = 0.05, max_iter: int = 20, gemm_mode: str = "f32"):
        super().__init__()
        self.pc_classifier = nn.Sequential(nn.BatchNorm1d(PC_FEAT_DIM), nn.ReLU(inplace=True), nn.Conv1d(PC_FEAT_DIM, 1, 1))
        self.affinity_extractor = nn.Sequential(nn.BatchNorm1d(PC_FEAT_DIM), nn.ReLU(inplace=True), nn.Conv1d(PC_FEAT_DIM, AFF_FEAT_DIM, 1))
        self.affinity_layer = _AffinityDual(AFF_FEAT_DIM)
        self.tau, self.max_iter, self.gemm_mode = float(tau), int(max_iter), gemm_mode
        self.eval()

    @classmethod
    def from_checkpoint(cls, path: str, **kw) -> "MatchingHead":
        """the head's entries of a Jigsaw checkpoint (a Lightning file with a `state_dict`, or a bare state_dict); the rest is ignored"""
        sd = load_checkpoint_state_dict(path)
        head = cls(**kw)
        head.load_state_dict({k: v for k, v in sd.items() if k.startswith(HEAD_PREFIXES)}, strict=True)
        return head

    @staticmethod
    def _fold(bn: nn.BatchNorm1d) -> Tuple[torch.Tensor, torch.Tensor]:
        scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
        return scale.contiguous(), (bn.bias.detach() - bn.running_mean * scale).contiguous()

    @torch.no_grad()
    def classify(self, feats: torch.Tensor, layout: Layout):
        """-> (logits float32 [N], labels uint8 [N], critical_pcs_idx int64 [N], n_critical_pcs int64 [B P])"""
        dev = feats.device
        N, Pt = feats.shape[0], layout.piece_slot.numel()
        scale, shift = self._fold(self.pc_classifier[0])
        conv = self.pc_classifier[2]
        w = conv.weight.detach().reshape(-1).contiguous()
        logits = torch.empty(N, dtype=torch.float32, device=dev)
        labels = torch.empty(N, dtype=torch.uint8, device=dev)
        crit = torch.empty(N, dtype=torch.int64, device=dev)
        n_crit = torch.empty(Pt, dtype=torch.int64, device=dev)
        check(_lib.load().pfpp_match_classify_compact(_p(feats), _p(scale), _p(shift), _p(w), float(conv.bias.detach().item()), None,
                                                      _p(layout.piece_off), Pt, PC_FEAT_DIM, _p(logits), _p(labels), _p(crit), _p(n_crit),
                                                      ops._stream()), "pfpp_match_classify_compact")
        return logits, labels, crit, n_crit

    @torch.no_grad()
    def affinity_features(self, feats: torch.Tensor, layout: Layout, crit: torch.Tensor, crit_off: torch.Tensor, R: int):
        """-> (normalised affinity features float32 [R, 512], piece slot of every row int32 [R])"""
        dev = feats.device
        scale, shift = self._fold(self.affinity_extractor[0])
        g = torch.empty((R, PC_FEAT_DIM), dtype=torch.float32, device=dev)
        row_piece = torch.empty(R, dtype=torch.int32, device=dev)
        if R == 0:
            return torch.empty((0, AFF_FEAT_DIM), dtype=torch.float32, device=dev), row_piece
        lib = _lib.load()
        check(lib.pfpp_match_gather_rows(_p(feats), _p(scale), _p(shift), _p(crit), _p(layout.piece_off), _p(crit_off), _p(layout.piece_slot),
                                         layout.piece_slot.numel(), R, PC_FEAT_DIM, _p(g), _p(row_piece), ops._stream()),
              "pfpp_match_gather_rows")
        conv = self.affinity_extractor[2]
        f = ops.linear(g, conv.weight.detach().reshape(AFF_FEAT_DIM, PC_FEAT_DIM).contiguous(), conv.bias.detach().contiguous(),
                       mode=self.gemm_mode)
        check(lib.pfpp_match_normalize_halves(_p(f), R, AFF_FEAT_DIM, ops._stream()), "pfpp_match_normalize_halves")
        return f, row_piece

    @torch.no_grad()
    def affinity(self, f: torch.Tensor, r0: int, r1: int, primal_a: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dual affinity of the rows [r0, r1) of the normalised features: s = (X[:, :256] A) X[:, 256:]^T, float32 [n, n] (row
        stride rounded up to 4 floats).  primal_a: X[:, :256] A of all rows when the caller computed it once for the batch."""
        h = AFF_FEAT_DIM // 2
        if primal_a is None:
            primal_a = self.primal_times_a(f)
        n = r1 - r0
        ld = (n + 3) & ~3
        s = torch.empty((n, ld), dtype=torch.float32, device=f.device)
        ops.gemm(primal_a, f, M=n, N=n, K=h, lda=h, ldw=AFF_FEAT_DIM, a_off=r0 * h, w_off=r0 * AFF_FEAT_DIM + h, out=s, ldc=ld,
                 mode=self.gemm_mode)
        return s[:, :n]

    @torch.no_grad()
    def primal_times_a(self, f: torch.Tensor) -> torch.Tensor:
        h = AFF_FEAT_DIM // 2
        a_t = self.affinity_layer.A.detach().t().contiguous()         # the GEMM reads both operands K-contiguous: W = A^T
        return ops.gemm(f, a_t, M=f.shape[0], N=h, K=h, lda=AFF_FEAT_DIM, mode=self.gemm_mode)

    @torch.no_grad()
    def forward(self, part_feats, n_pcs, part_valids, *, dense_perm: bool = True, overlap: bool = True, assign: bool = True,
                solver: str = "host", max_steps=None) -> HeadOutput:
        """part_feats: float32 [B, N, 128], a list of [N_b, 128] or flat [sum N, 128]; n_pcs int [B, P]; part_valids [B, P].
        solver: "host" = scipy on the host, overlapped with the next puzzle's GPU work; "device" = one batched launch of the exact
        device solver over all puzzles behind their Sinkhorn (pfpp_hip.matching_assign.assign_batch; no pinned buffers, no copy stream,
        no download of ds_mat).  max_steps: that solver's step budget (None = its default); a puzzle whose budget runs out is solved
        on the host, with one warning."""
        import time
        import warnings

        from scipy.optimize import linear_sum_assignment

        first = part_feats[0] if isinstance(part_feats, (list, tuple)) else part_feats
        _gpu(first, torch.float32, "part_feats")
        if solver not in ("host", "device"):
            raise ValueError(f"solver: expected 'host' or 'device', got {solver!r}")
        dev = first.device
        layout = make_layout(n_pcs, dev)
        feats = _flatten(part_feats, layout, PC_FEAT_DIM, "part_feats")
        B, P = layout.n_pcs.shape
        pv = np.asarray(part_valids.detach().cpu().numpy() if torch.is_tensor(part_valids) else part_valids)
        n_valid = pv.reshape(B, P).sum(1).astype(np.int64)
        for b in range(B):
            if layout.n_pcs[b, n_valid[b]:].any():
                raise ValueError(f"puzzle {b}: points in a slot behind its {n_valid[b]} valid pieces")
        t0 = time.perf_counter()
        logits, labels, crit, n_crit = self.classify(feats, layout)
        crit_off = torch.zeros(B * P + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n_crit, 0, out=crit_off[1:])
        nc = n_crit.cpu().numpy().reshape(B, P)                       # the one read-back: the matrices are allocated from it
        rows = np.concatenate([[0], np.cumsum(nc.sum(1))]).astype(np.int64)
        f, row_piece = self.affinity_features(feats, layout, crit, crit_off, int(rows[-1]))
        pa = self.primal_times_a(f) if rows[-1] else None
        ds_list: List[torch.Tensor] = []
        perm_list: List[Optional[torch.Tensor]] = [None] * B
        copy_stream = torch.cuda.Stream(dev) if solver == "host" else None
        # Two pinned buffers sized to the largest puzzle, taken in turn by the jobs SUBMITTED (n_jobs; skipped puzzles do not count).
        # Invariant: at most one job is pending, and job k is solved before job k + 1 becomes pending, so when job k + 2 takes the
        # buffer of job k that job's assignment has been read out of it.
        n_big = max((int(rows[b + 1] - rows[b]) for b in range(B) if (nc[b] > 0).sum() >= 2), default=0) if assign and solver == "host" else 0
        pinned = [torch.empty(n_big * n_big, dtype=torch.float32, pin_memory=True) for _ in range(2 if n_big else 0)]
        host_s = copy_s = device_s = 0.0
        pending = None
        n_jobs = 0
        device_jobs: List[int] = []           # solver == "device": the puzzles behind their Sinkhorn, solved in one call after the loop
        fallback: List[int] = []

        def solve(job):
            nonlocal host_s, copy_s
            b, buf, ev = job
            t = time.perf_counter()
            ev.synchronize()
            t1 = time.perf_counter()
            _, col = linear_sum_assignment(-buf.numpy())
            host_s += time.perf_counter() - t1
            copy_s += t1 - t
            perm_list[b] = torch.from_numpy(col.astype(np.int64))

        for b in range(B):
            r0, r1 = int(rows[b]), int(rows[b + 1])
            if (nc[b] > 0).sum() < 2:        # every entry masked: no Sinkhorn, no assignment, no edges (the reference finds no pair either)
                ds_list.append(torch.empty((0, 0), dtype=torch.float32, device=dev))
                perm_list[b] = torch.empty(0, dtype=torch.int64)
                continue
            s = self.affinity(f, r0, r1, pa)
            ds = sinkhorn(s, row_piece[r0:r1], tau=self.tau, max_iter=self.max_iter, check_pieces=False)       # counted above
            ds_list.append(ds)
            if not assign:
                perm_list[b] = torch.empty(0, dtype=torch.int64)
                continue
            if solver == "device":
                device_jobs.append(b)
                continue
            n = r1 - r0
            buf = pinned[n_jobs % 2][:n * n].view(n, n)
            n_jobs += 1
            copy_stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(copy_stream):
                buf.copy_(ds, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            ds.record_stream(copy_stream)
            job = (b, buf, ev)
            if not overlap:
                solve(job)
            else:                               # the GPU works on puzzle b while the host solves puzzle b - 1
                if pending is not None:
                    solve(pending)
                pending = job
        if pending is not None:
            solve(pending)
        if device_jobs:
            from .matching_assign import assign_batch

            t1 = time.perf_counter()
            res = assign_batch([ds_list[b] for b in device_jobs], max_steps=max_steps)
            status = res.status.cpu().numpy()                 # B words: the one wait for the launch
            device_s = time.perf_counter() - t1
            for k, b in enumerate(device_jobs):
                if status[k] == 0:
                    perm_list[b] = res.col[k]
                    continue
                fallback.append(b)
                t1 = time.perf_counter()
                _, col = linear_sum_assignment(-ds_list[b].cpu().numpy())
                host_s += time.perf_counter() - t1
                perm_list[b] = torch.from_numpy(col.astype(np.int64))
            if fallback:
                warnings.warn(f"device assignment: the step budget (max_steps = {'the default' if max_steps is None else max_steps}) ran out for "
                              f"puzzle(s) {fallback} of the batch; solved on the host instead")
        torch.cuda.current_stream(dev).synchronize()
        wall = time.perf_counter() - t0
        perms = []
        for b in range(B):
            col = perm_list[b].to(dev)
            if dense_perm:
                n = ds_list[b].shape[0]
                m = torch.zeros((n, n), dtype=torch.float32, device=dev)
                if col.numel():
                    m[torch.arange(n, device=dev), col] = 1.0
                perms.append(m)
            else:
                perms.append(col)
        sizes = layout.puz_points.tolist()
        return HeadOutput([t.reshape(-1, 1) for t in torch.split(logits, sizes)], list(torch.split(labels.to(torch.int64), sizes)),
                          list(torch.split(crit, sizes)), n_crit.reshape(B, P), ds_list, perms,
                          {"wall_s": wall, "host_assignment_s": host_s, "wait_for_copy_s": copy_s, "device_assignment_s": device_s,
                           "fallback_puzzles": len(fallback)})


# ------------------------------------------------------------------------------------------------------------------ the descriptor network
from .matching_dgcnn import DGCNN, DGCNNDynamic                              # noqa: E402  (the matcher's modules are re-exported here)
from .matching_encoder import PointNet2PTMSGDynamic                          # noqa: E402
from .matching_transformer import CrossAttentionLayer, PointTransformerLayer  # noqa: E402

DESCRIPTOR_PREFIXES = ("encoder.", "tf_self1.", "tf_cross1.")
DEFAULT_ENCODER = "pointnet2_pt.msg.dynamic"


def build_encoder(arch: str, feat_dim: int, global_feat: bool = False, in_feat_dim: int = 3, gemm_mode: str = "f32") -> nn.Module:
    """build_encoder of the reference (model/modules/encoder/__init__.py:1-39) for its arch strings ('xxx.xxx.x', any case):
    'pointnet2_pt.msg.dynamic' -> PointNet2PTMSGDynamic(in_feat_dim, feat_dim), 'dgcnn.dynamic' -> DGCNNDynamic(feat_dim, global_feat,
    in_feat_dim).  The dense families ('pointnet2_pt.msg', 'dgcnn'), global_feat=True and every other string raise NotImplementedError."""
    if not isinstance(arch, str):
        raise TypeError(f"arch: expected a string such as {DEFAULT_ENCODER!r}, got {type(arch).__name__}")
    archs = arch.lower().split(".")
    if "pointnet2_pt" in archs:
        if global_feat:
            raise NotImplementedError(f"{arch}: the point-wise PointNet++ encoder has no global feature (the reference asserts the same)")
        if "msg" not in archs:
            raise NotImplementedError(f"{arch} not supported")
        if "dynamic" not in archs:
            raise NotImplementedError(f"{arch}: the dense PointNet2PTMSG is not built, only 'pointnet2_pt.msg.dynamic'")
        if isinstance(feat_dim, (list, tuple)):
            in_feat_dim, feat_dim = feat_dim
        return PointNet2PTMSGDynamic(in_feat_dim, feat_dim, gemm_mode=gemm_mode)
    if "dgcnn" in archs:
        if "dynamic" not in archs:
            return DGCNN(feat_dim, global_feat)                              # raises: the dense DGCNN is not built
        return DGCNNDynamic(feat_dim, global_feat, in_feat_dim, gemm_mode=gemm_mode)
    raise NotImplementedError(f"{arch} is not supported")


class DescriptorNetwork(nn.Module):
    """encoder, tf_self1 and tf_cross1 of JointSegmentationAlignmentModel (joint_seg_align_model.py:38-50, 56-64, 146-162) with the
    reference's parameter names: the points of several puzzles -> flat per-point descriptors [sum N, 128] in the layout
    MatchingHead.forward takes.  encoder: the reference's MODEL.ENCODER string, "pointnet2_pt.msg.dynamic" (the default) or
    "dgcnn.dynamic".  Everything between the upload of the points and the descriptors runs on the device; the piece lengths are host data."""

    def __init__(self, gemm_mode: str = "f32", encoder: str = DEFAULT_ENCODER):
        super().__init__()
        self.gemm_mode = gemm_mode
        self.encoder = build_encoder(encoder, PC_FEAT_DIM, global_feat=False, in_feat_dim=3, gemm_mode=gemm_mode)
        self.tf_self1 = PointTransformerLayer(PC_FEAT_DIM, PC_FEAT_DIM, n_heads=8, nsampmle=16, gemm_mode=gemm_mode)
        self.tf_cross1 = CrossAttentionLayer(PC_FEAT_DIM, 8, gemm_mode=gemm_mode)
        super().train(False)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("DescriptorNetwork runs in eval mode only: matcher training goes through pfpp_hip.matching_fit (MatcherTrainer / fit, "
                                      "python -m pfpp_hip.train_matching), whose engines step this module's parameters")
        return super().train(False)

    @classmethod
    def from_checkpoint(cls, path: str, **kw) -> "DescriptorNetwork":
        """the `encoder.*`, `tf_self1.*` and `tf_cross1.*` entries of a Jigsaw checkpoint (strict); the rest is ignored.  The encoder
        family is the file's own (checkpoint_encoder_arch) unless `encoder=` names one."""
        ckpt = _read_checkpoint(path)
        sd = _state_dict_of(ckpt, path)
        kw.setdefault("encoder", checkpoint_encoder_arch(ckpt, sd))
        net = cls(**kw)
        net.load_state_dict({k: v for k, v in sd.items() if k.startswith(DESCRIPTOR_PREFIXES)}, strict=True)
        return net

    @torch.no_grad()
    def forward(self, part_pcs, n_pcs, part_valids, start=None, seed: Optional[int] = None) -> torch.Tensor:
        """part_pcs: float32 [B, N, 3], a list of [N_b, 3] or flat [sum N, 3] on the GPU; n_pcs int [B, P]; part_valids [B, P];
        start / seed: the encoder's sampling starts ([number of non-empty pieces, 4]) or the seed they are drawn from"""
        first = part_pcs[0] if isinstance(part_pcs, (list, tuple)) else part_pcs
        _gpu(first, torch.float32, "part_pcs")
        layout = make_layout(n_pcs, first.device)
        pts = _flatten(part_pcs, layout, 3, "part_pcs")
        B, P = layout.n_pcs.shape
        pv = np.asarray(part_valids.detach().cpu().numpy() if torch.is_tensor(part_valids) else part_valids)
        n_valid = pv.reshape(B, P).sum(1).astype(np.int64)
        for b in range(B):
            if layout.n_pcs[b, n_valid[b]:].any() or (layout.n_pcs[b, :n_valid[b]] < 1).any():
                raise ValueError(f"puzzle {b}: its {n_valid[b]} valid pieces must be the first slots and hold at least one point each")
        lengths = layout.n_pcs.reshape(-1)
        lengths = lengths[lengths > 0]                    # get_batch_length_from_part_points: the valid pieces of all puzzles in order
        if isinstance(self.encoder, DGCNNDynamic):        # no sampling in this family: start / seed have nothing to act on
            feats = self.encoder(pts, lengths)
        else:
            feats = self.encoder(pts, lengths, start=start, seed=seed)
        feats = self.tf_self1(pts, feats, lengths)
        return self.tf_cross1(feats, layout.puz_points)
