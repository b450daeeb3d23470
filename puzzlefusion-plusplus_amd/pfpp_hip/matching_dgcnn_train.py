"""Training of the matcher's DGCNN encoder (csrc/dgcnn_train.hip; include/pfpp.h "DGCNN encoder in .train()").

The reference's DGCNNDynamic (Jigsaw_matching/model/modules/encoder/dgcnn.py:130-213) in .train(): each of the four edge-convolution
levels normalises with the statistics of ALL R = 20 N slot rows of the call, padded all-zero rows included, and conv5's BatchNorm with
those of the N rows; every BatchNorm moves its running buffers.  The decomposition of matching_dgcnn carries over: with
uv = X [W_a ; W_b - W_a]^T and z_ij = u[idx_ij] + v[i] (0 for a padded slot)

    forward   mean, var over all R rows of z (fp64 sums);  a = gamma rstd,  b = beta - mean a
              e_i = max_j z_ij (gamma >= 0) or min_j z_ij (gamma < 0), w_i = the winning slot;  x_l[i] = LeakyReLU(e_i a + b)
    backward  h_i = g_i (e_i a + b > 0 ? 1 : 0.2);  dbeta = sum_i h_i;  dgamma = sum_i h_i (e_i - mean) rstd;  m1 = dbeta / R, m2 = dgamma / R
              dv[i] = a (h_i [w_i real] - n_i m1 - m2 rstd (sum_{j real} u[idx_ij] + n_i (v[i] - mean)))
              du[p] = a (sum_{idx_ij = p} h_i [w_i = j] - c_p m1 - m2 rstd (c_p (u[p] - mean) + sum_{idx_ij = p} v[i]))
              dX = [du | dv] [W_a ; W_b - W_a],  dW2 = [du | dv]^T X,  d conv.weight = [dW2_top - dW2_bot | dW2_bot]

so nothing of size [N, 20, .] exists in either direction: a level keeps uv [N, 2 C], e [N, C] and one byte per entry for the winner.

* dgcnn_edge_stats / dgcnn_bn_leaky_apply / dgcnn_bn_leaky_bwd / dgcnn_edge_bwd_dv / dgcnn_edge_bwd_du: the five entries on their own;
  dgcnn_inverse_lists: the CSR lists du walks (plumbing in torch; the padded index N gets no list).
* DGCNNTrainEngine: forward(x, batch_length) of an eval-mode DGCNNDynamic with batch statistics (the module's 10 running buffers and
  five num_batches_tracked move), backward(dout) with the gradients in the .grad of its 15 parameters, optimizer_step() = torch.optim.Adam
  through pfpp_adamw.  The searches are the eval path's kernel; every product (forward, dX, dW) is the exact-fp32 GEMM.
* DGCNNFunction: the engine as a torch.autograd.Function; it chains with matching_transformer_train.PointTransformerFunction.
* DGCNNDescriptorTrainEngine: encoder, tf_self1 and tf_cross1 of a matching.DescriptorNetwork(encoder="dgcnn.dynamic") under one
  loss.backward().
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .matching_dgcnn import CAT, COL, EDGE_WIDTHS, K_NEIGHBOURS, MAX_PIECE, SLOPE, WIDTHS, DGCNNDynamic, _p, dgcnn_knn
from .matching_encoder_train import ragged_bn_stats
from .matching_transformer_train import (PTF_DW_CHUNK_ROWS, CrossAttentionFunction, CrossAttentionTrainEngine, PointTransformerFunction,
                                         PointTransformerTrainEngine, _dweight)

DGCNN_TRAIN_MAX_WG = 1024                                  # PFPP_DGCNN_TRAIN_MAX_WG (include/pfpp.h)
DGCNN_TRAIN_WS_DOUBLES = DGCNN_TRAIN_MAX_WG * 512 + 1024   # PFPP_DGCNN_TRAIN_WS_DOUBLES
MAX_C = 1024
ONE_VALUE = "Expected more than 1 value per channel when training"        # torch's own words for a BatchNorm over one row


def _f32(t: torch.Tensor, name: str, rows: Optional[int] = None, cols: Optional[int] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{name}: expected a float32 tensor on the GPU")
    if t.dim() != 2 or t.stride(1) != 1 or (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name}: expected [{'rows' if rows is None else rows}, {'C' if cols is None else cols}] with contiguous rows, "
                         f"got {tuple(t.shape)}")
    if t.stride(0) % 4 or t.data_ptr() % 16:
        raise ValueError(f"{name}: rows of a multiple of 4 floats, 16-byte aligned")
    return t


def _vec(t: torch.Tensor, name: str, n: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.shape != (n,) or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous float32 [{n}] on the GPU")
    return t


def _edge_width(c_out: int, what: str) -> None:
    if c_out not in EDGE_WIDTHS:
        raise ValueError(f"{what}: the kernel is built for {EDGE_WIDTHS} output channels (got {c_out})")


def _idx(idx: torch.Tensor) -> int:
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype != torch.int32:
        raise ValueError("idx: expected an int32 tensor on the GPU")
    if idx.dim() != 2 or idx.shape[1] != K_NEIGHBOURS or not idx.is_contiguous():
        raise ValueError(f"idx: expected contiguous int32 [N, {K_NEIGHBOURS}], got {tuple(idx.shape)}")
    return idx.shape[0]


def _uv(uv: torch.Tensor, N: int, c_out: int) -> torch.Tensor:
    _f32(uv, "uv", N)
    if uv.shape[1] < 2 * c_out:
        raise ValueError(f"uv: expected [N, >= {2 * c_out}] = [u | v], got {tuple(uv.shape)}")
    return uv


def _winner(w: torch.Tensor, N: int, c_out: int) -> torch.Tensor:
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dtype != torch.uint8 or w.shape != (N, c_out) or not w.is_contiguous():
        raise ValueError(f"winner: expected contiguous uint8 [{N}, {c_out}] on the GPU")
    return w


def train_workspace(device) -> torch.Tensor:
    """the fp64 workspace of the entries that reduce over rows (4 MB, whatever the sizes are)"""
    return torch.empty(DGCNN_TRAIN_WS_DOUBLES, dtype=torch.float64, device=device)


def _ws(ws: Optional[torch.Tensor], device) -> torch.Tensor:
    if ws is None:
        return train_workspace(device)
    if not isinstance(ws, torch.Tensor) or ws.dtype != torch.float64 or not ws.is_cuda or ws.numel() < DGCNN_TRAIN_WS_DOUBLES or not ws.is_contiguous():
        raise ValueError(f"workspace: expected at least {DGCNN_TRAIN_WS_DOUBLES} contiguous float64 on the GPU")
    return ws


# ------------------------------------------------------------------------------------------------------------------ kernels
def dgcnn_edge_stats(uv: torch.Tensor, idx: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, momentum: float = 0.1,
                     running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None, *, c_out: int,
                     ws: Optional[torch.Tensor] = None, want_sums: bool = False):
    """uv float32 [N, >= 2 c_out] = [u | v], idx int32 [N, 20] (N = the padded slot) -> (e float32 [N, c_out], winner uint8 [N, c_out],
    coef float32 [4, c_out] = a | b | mean | rstd) of the level's BatchNorm on the statistics of all 20 N slot rows; the running buffers,
    when given, move by `momentum`.  want_sums: also float64 [2, c_out] = sum z | sum z^2."""
    _edge_width(c_out, "dgcnn_edge_stats")
    N = _idx(idx)
    if N < 1:
        raise ValueError("dgcnn_edge_stats: no points")
    _uv(uv, N, c_out)
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        _vec(t, nm, c_out)
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var go together")
    for t, nm in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _vec(t, nm, c_out)
    if not (eps >= 0.0 and 0.0 <= momentum <= 1.0):
        raise ValueError("eps >= 0 and momentum in [0, 1]")
    ws = _ws(ws, uv.device)
    e = torch.empty((N, c_out), dtype=torch.float32, device=uv.device)
    winner = torch.empty((N, c_out), dtype=torch.uint8, device=uv.device)
    coef = torch.empty((4, c_out), dtype=torch.float32, device=uv.device)
    check(_lib.load().pfpp_dgcnn_edge_stats(_p(uv), uv.stride(0), _p(idx), _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean),
                                            _p(running_var), N, c_out, K_NEIGHBOURS, _p(e), _p(winner), _p(coef), _p(ws), ops._stream()),
          "pfpp_dgcnn_edge_stats")
    for t in (running_mean, running_var):
        if t is not None:
            torch.autograd.graph.increment_version(t)      # written through a raw pointer: the module's pack cache watches _version
    if want_sums:
        return e, winner, coef, ws[DGCNN_TRAIN_MAX_WG * 512:DGCNN_TRAIN_MAX_WG * 512 + 2 * c_out].clone().reshape(2, c_out)
    return e, winner, coef


def dgcnn_bn_leaky_apply(y: torch.Tensor, coef: torch.Tensor, out: Optional[torch.Tensor] = None, c_off: int = 0,
                         slope: float = SLOPE) -> torch.Tensor:
    """LeakyReLU(y a + b) (one multiply, one add) of y float32 [rows, C] with coef [4, C]; out / c_off: write into the columns
    [c_off, c_off + C) of a wider tensor"""
    _f32(y, "y")
    rows, C_ = y.shape
    if C_ % 4 or not 4 <= C_ <= MAX_C:
        raise ValueError(f"C = {C_}: a multiple of 4, at most {MAX_C}")
    _f32(coef, "coef", 4, C_)
    if not coef.is_contiguous():
        raise ValueError("coef: contiguous [4, C]")
    if out is None:
        out, c_off = torch.empty((rows, C_), dtype=torch.float32, device=y.device), 0
    else:
        _f32(out, "out", rows)
        if c_off % 4 or c_off < 0 or c_off + C_ > out.shape[1]:
            raise ValueError("out: the columns [c_off, c_off + C) must exist and start at a multiple of 4")
    check(_lib.load().pfpp_dgcnn_bn_leaky_apply(_p(y), rows, C_, y.stride(0), _p(coef), float(slope), _p(out, 4 * c_off), out.stride(0),
                                                ops._stream()), "pfpp_dgcnn_bn_leaky_apply")
    return out


def dgcnn_bn_leaky_bwd(y: torch.Tensor, g1: torch.Tensor, coef: torch.Tensor, *, g2: Optional[torch.Tensor] = None, count: Optional[int] = None,
                       want_dy: bool = False, slope: float = SLOPE, ws: Optional[torch.Tensor] = None):
    """backward of LeakyReLU(BN_train(.)) at y float32 [rows, C]: g1 (+ g2) = d loss / d output (column slices of wider tensors are
    fine) -> (h [rows, C], dgamma, dbeta, means [2, C] = dbeta / count | dgamma / count).  count: the rows the BatchNorm saw (rows by
    default; 20 N for a level, whose y is the extremum e).  want_dy: h is replaced by dy = a ((h - m1) - x_hat m2)."""
    _f32(y, "y")
    rows, C_ = y.shape
    if C_ % 4 or not 4 <= C_ <= MAX_C:
        raise ValueError(f"C = {C_}: a multiple of 4, at most {MAX_C}")
    if rows < 1:
        raise ValueError("dgcnn_bn_leaky_bwd: no rows")
    _f32(coef, "coef", 4, C_)
    _f32(g1, "g1", rows, C_)
    if g2 is not None:
        _f32(g2, "g2", rows, C_)
    count = rows if count is None else int(count)
    if count < rows:
        raise ValueError(f"count = {count}: the BatchNorm saw at least the {rows} rows given")
    ws = _ws(ws, y.device)
    h = torch.empty((rows, C_), dtype=torch.float32, device=y.device)
    dgamma = torch.empty(C_, dtype=torch.float32, device=y.device)
    dbeta, means = torch.empty_like(dgamma), torch.empty((2, C_), dtype=torch.float32, device=y.device)
    check(_lib.load().pfpp_dgcnn_bn_leaky_bwd(_p(y), y.stride(0), _p(g1), g1.stride(0), _p(g2), 0 if g2 is None else g2.stride(0), rows, C_,
                                              _p(coef), float(slope), float(count), _p(h), _p(dgamma), _p(dbeta), _p(means),
                                              _p(h if want_dy else None), _p(ws), ops._stream()), "pfpp_dgcnn_bn_leaky_bwd")
    return h, dgamma, dbeta, means


def dgcnn_inverse_lists(idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """idx int32 [N, 20] with the padded slots holding N -> (off int64 [N + 1], ent int32 [20 N]): the flat positions e = 20 i + j whose
    index is p are ent[off[p] : off[p + 1]], ascending (a stable sort).  The padded slots sort behind every list: ent[off[N]:] is
    theirs and no list names them.  Plumbing in torch, no kernel."""
    N = _idx(idx)
    flat = idx.reshape(-1).long().clamp_(max=N)            # anything behind N is a padded slot, as in the kernels; bincount refuses < 0
    ent = torch.sort(flat, stable=True).indices.to(torch.int32)
    off = torch.zeros(N + 1, dtype=torch.int64, device=idx.device)
    off[1:] = torch.cumsum(torch.bincount(flat, minlength=N + 1)[:N], 0)
    return off, ent.contiguous()


def _edge_bwd_args(uv, winner, h, coef, means, c_out: int, N: int, what: str) -> None:
    _edge_width(c_out, what)
    _uv(uv, N, c_out)
    _winner(winner, N, c_out)
    _f32(h, "h", N, c_out)
    _f32(coef, "coef", 4, c_out)
    _f32(means, "means", 2, c_out)
    if not h.is_contiguous() or not coef.is_contiguous() or not means.is_contiguous():
        raise ValueError("h / coef / means: contiguous")


def _duv(duv: Optional[torch.Tensor], N: int, c_out: int, device) -> torch.Tensor:
    if duv is None:
        return torch.zeros((N, 2 * c_out), dtype=torch.float32, device=device)
    _f32(duv, "duv", N, 2 * c_out)
    if not duv.is_contiguous():
        raise ValueError("duv: contiguous [N, 2 c_out]")
    return duv


def dgcnn_edge_bwd_dv(uv: torch.Tensor, idx: torch.Tensor, winner: torch.Tensor, h: torch.Tensor, coef: torch.Tensor, means: torch.Tensor, *,
                      c_out: int, duv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the forward-list gather of a level's backward: writes dv into the columns [c_out, 2 c_out) of duv float32 [N, 2 c_out]"""
    N = _idx(idx)
    _edge_bwd_args(uv, winner, h, coef, means, c_out, N, "dgcnn_edge_bwd_dv")
    duv = _duv(duv, N, c_out, uv.device)
    check(_lib.load().pfpp_dgcnn_edge_bwd_dv(_p(uv), uv.stride(0), _p(idx), _p(winner), _p(h), _p(coef), _p(means), N, c_out, K_NEIGHBOURS,
                                             _p(duv), ops._stream()), "pfpp_dgcnn_edge_bwd_dv")
    return duv


def dgcnn_edge_bwd_du(uv: torch.Tensor, off: torch.Tensor, ent: torch.Tensor, winner: torch.Tensor, h: torch.Tensor, coef: torch.Tensor,
                      means: torch.Tensor, *, c_out: int, duv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the inverse-list gather of a level's backward: (off, ent) = dgcnn_inverse_lists(idx); writes du into the columns [0, c_out) of duv"""
    if not isinstance(off, torch.Tensor) or not isinstance(ent, torch.Tensor) or off.dtype != torch.int64 or ent.dtype != torch.int32 \
            or not off.is_cuda or not ent.is_cuda:
        raise ValueError("off / ent: int64 offsets and int32 entries on the GPU")
    N = off.numel() - 1
    if off.dim() != 1 or N < 0 or ent.shape != (K_NEIGHBOURS * N,) or not off.is_contiguous() or not ent.is_contiguous():
        raise ValueError(f"off / ent: expected [N + 1] and [{K_NEIGHBOURS} N], got {tuple(off.shape)} and {tuple(ent.shape)}")
    _edge_bwd_args(uv, winner, h, coef, means, c_out, N, "dgcnn_edge_bwd_du")
    duv = _duv(duv, N, c_out, uv.device)
    check(_lib.load().pfpp_dgcnn_edge_bwd_du(_p(uv), uv.stride(0), _p(off), _p(ent), ent.numel(), _p(winner), _p(h), _p(coef), _p(means), N, c_out,
                                             K_NEIGHBOURS, _p(duv), ops._stream()), "pfpp_dgcnn_edge_bwd_du")
    return duv


# ------------------------------------------------------------------------------------------------------------------ the engine
class DGCNNTrainEngine:
    """one training step of a DGCNNDynamic (the module itself stays in eval mode; what is here is the reference's .train() arithmetic).
    forward() normalises the five BatchNorms with the statistics of the whole flat call (the levels over all 20 N slot rows), writes the
    module's 10 running buffers and bumps the five num_batches_tracked; per level it keeps uv [N, 2 C], the extremum e [N, C], the winning
    slot (one byte per entry), the lists and their inverses, plus cat [N, 512] and conv5's product.  backward(dout) OVERWRITES the .grad
    of all 15 parameters; the points get no gradient.  optimizer_step() is torch.optim.Adam (weight decay 0) through pfpp_adamw."""

    def __init__(self, encoder: DGCNNDynamic):
        if not isinstance(encoder, DGCNNDynamic):
            raise TypeError("DGCNNTrainEngine: expected a DGCNNDynamic")
        if encoder.gemm_mode != "f32":
            raise NotImplementedError("the DGCNN encoder's training runs in the exact-fp32 GEMM mode only")
        self.encoder = encoder
        self.params: Dict[str, torch.nn.Parameter] = dict(encoder.named_parameters())
        assert len(self.params) == 15, list(self.params)
        self.state: Dict[str, Tuple[torch.Tensor, torch.Tensor, int]] = {}
        self.saved: dict = {}
        self._wsp: Optional[torch.Tensor] = None
        self.leaf: Optional[torch.Tensor] = None       # what DGCNNFunction hangs on: the points carry no gradient
        self.stage_events: Optional[list] = None       # set to a list to get (stage name, HIP event) pairs from forward() and backward()

    _mark = CrossAttentionTrainEngine._mark
    optimizer_step = CrossAttentionTrainEngine.optimizer_step      # Adam over self.params / self.state: the same statement

    def _workspace(self, device) -> torch.Tensor:
        if self._wsp is None or self._wsp.device != device:
            self._wsp = train_workspace(device)
        return self._wsp

    def autograd_leaf(self, device) -> torch.Tensor:
        if self.leaf is None or self.leaf.device != device:
            self.leaf = torch.zeros(1, dtype=torch.float32, device=device, requires_grad=True)
        return self.leaf

    @staticmethod
    def _split_weight(conv) -> torch.Tensor:
        """[W_a | W_b] -> [W_a ; W_b - W_a] with the input columns padded to a multiple of 4 (DGCNNDynamic._packed's operand)"""
        w = conv.weight.detach().reshape(conv.weight.shape[0], -1)
        c_in = w.shape[1] // 2
        w2 = torch.zeros((2 * w.shape[0], (c_in + 3) & ~3), dtype=torch.float32, device=w.device)
        w2[:w.shape[0], :c_in] = w[:, :c_in]
        w2[w.shape[0]:, :c_in] = w[:, c_in:] - w[:, :c_in]
        return w2

    # ---- forward
    @torch.no_grad()
    def forward(self, x: torch.Tensor, batch_length, keep_activations: bool = False) -> torch.Tensor:
        """x float32 [N_sum, 3] on the GPU, batch_length: the piece lengths -> the descriptors [N_sum, feat_dim] of the reference's
        .train() forward.  keep_activations (tests): saved["levels"][l] also holds the level's output x_l."""
        enc = self.encoder
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"x: must live on the GPU (got {getattr(x, 'device', type(x).__name__)}); there is no CPU path")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != enc.in_feat_dim:
            raise ValueError(f"x: expected float32 [N_sum, {enc.in_feat_dim}], got {x.dtype} {tuple(x.shape)}")
        if enc.conv5[0].weight.device != x.device:
            raise ValueError(f"the module lives on {enc.conv5[0].weight.device}, x on {x.device}")
        lengths = np.asarray(batch_length.detach().cpu().numpy() if torch.is_tensor(batch_length) else batch_length).astype(np.int64).reshape(-1)
        if lengths.size == 0 or (lengths < 1).any():
            raise ValueError("batch_length: every piece needs at least one point")
        if int(lengths.sum()) != x.shape[0]:
            raise ValueError(f"batch_length sums to {int(lengths.sum())} points, x has {x.shape[0]}")
        max_piece = int(lengths.max())
        if max_piece > MAX_PIECE:
            raise ValueError(f"a piece of {max_piece} points: the search kernel holds at most {MAX_PIECE}")
        dev, N = x.device, x.shape[0]
        if N < 2:
            raise ValueError(f"bn5: a batch-statistics BatchNorm over {N} row; torch refuses it too: {ONE_VALUE}")
        f32 = dict(dtype=torch.float32, device=dev)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
        ws = self._workspace(dev)
        x = x.contiguous()
        xp = torch.zeros((N, 4), **f32)                    # level 1's operand: three columns padded to four
        xp[:, :3] = x
        cat = torch.empty((N, CAT), **f32)
        levels: List[dict] = []
        self._mark("begin")
        for l, c_out in enumerate(WIDTHS):
            conv, bn = getattr(enc, f"conv{l + 1}")[0], getattr(enc, f"bn{l + 1}")
            w2 = self._split_weight(conv)
            if l == 0:
                idx = dgcnn_knn(x, off, max_piece)
                a, a_off, lda, k = xp, 0, 4, enc.in_feat_dim
            else:
                idx = dgcnn_knn(cat, off, max_piece, col=COL[l - 1], width=WIDTHS[l - 1])
                a, a_off, lda, k = cat, COL[l - 1], CAT, WIDTHS[l - 1]
            self._mark(f"search{l + 1}")
            inv = dgcnn_inverse_lists(idx)
            self._mark(f"inverse_lists{l + 1}")
            uv = ops.gemm(a, w2, M=N, N=2 * c_out, K=k, lda=lda, ldw=w2.shape[1], a_off=a_off, out=torch.empty((N, 2 * c_out), **f32),
                          ldc=2 * c_out, mode="f32")
            self._mark(f"product{l + 1}")
            e, winner, coef = dgcnn_edge_stats(uv, idx, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, bn.running_mean,
                                               bn.running_var, c_out=c_out, ws=ws)
            self._mark(f"stats{l + 1}")
            dgcnn_bn_leaky_apply(e, coef, out=cat, c_off=COL[l])
            bn.num_batches_tracked.add_(1)
            self._mark(f"apply{l + 1}")
            levels.append({"idx": idx, "inv": inv, "uv": uv, "e": e, "winner": winner, "coef": coef, "w2": w2, "k": k})
            if keep_activations:
                levels[-1]["x"] = cat[:, COL[l]:COL[l] + c_out]
        bn5 = enc.bn5
        w5 = enc.conv5[0].weight.detach().reshape(enc.feat_dim, CAT).contiguous()
        y5 = ops.gemm(cat, w5, M=N, N=enc.feat_dim, K=CAT, lda=CAT, ldw=CAT, mode="f32")
        coef5 = ragged_bn_stats(y5, bn5.weight.detach(), bn5.bias.detach(), bn5.eps, bn5.momentum, bn5.running_mean, bn5.running_var,
                                ws)                         # the two workspaces have one size
        out = dgcnn_bn_leaky_apply(y5, coef5)
        bn5.num_batches_tracked.add_(1)
        self._mark("conv5")
        self.saved = {"N": N, "xp": xp, "cat": cat, "levels": levels, "w5": w5, "y5": y5, "coef5": coef5}
        return out

    # ---- backward
    @torch.no_grad()
    def backward(self, dout: torch.Tensor) -> None:
        """dout = d loss / d (the last forward's descriptors) [N_sum, feat_dim]; the gradients go to the .grad of the parameters"""
        s, enc = self.saved, self.encoder
        if not s:
            raise RuntimeError("backward() before forward()")
        N, F = s["N"], enc.feat_dim
        if not isinstance(dout, torch.Tensor) or not dout.is_cuda or dout.dtype != torch.float32 or dout.shape != (N, F):
            raise ValueError(f"dout: expected float32 {(N, F)} on the GPU")
        dout = dout.contiguous()
        dev = dout.device
        f32 = dict(dtype=torch.float32, device=dev)
        ws = self._workspace(dev)
        grads: Dict[str, torch.Tensor] = {}
        cat = s["cat"]
        self._mark("begin")
        # ---- conv5 + bn5 + LeakyReLU (dgcnn.py:158-160, :208-210)
        dy5, grads["bn5.weight"], grads["bn5.bias"], _ = dgcnn_bn_leaky_bwd(s["y5"], dout, s["coef5"], want_dy=True, ws=ws)
        grads["conv5.0.weight"] = _dweight(dy5, cat, F, CAT, PTF_DW_CHUNK_ROWS)
        dcat = ops.gemm(dy5, s["w5"], M=N, N=CAT, K=F, lda=F, ldw=CAT, out=torch.empty((N, CAT), **f32), ldc=CAT, w_kmajor=True, mode="f32")
        self._mark("conv5_bwd")
        # ---- the levels, 4 .. 1: x_l feeds conv5 (its columns of dcat) and, below level 4, level l + 1 (its dX)
        dx_next: Optional[torch.Tensor] = None
        for l in (3, 2, 1, 0):
            lv, c_out = s["levels"][l], WIDTHS[l]
            h, dgamma, dbeta, means = dgcnn_bn_leaky_bwd(lv["e"], dcat[:, COL[l]:COL[l] + c_out], lv["coef"], g2=dx_next, count=K_NEIGHBOURS * N,
                                                         ws=ws)
            grads[f"bn{l + 1}.weight"], grads[f"bn{l + 1}.bias"] = dgamma, dbeta
            duv = torch.empty((N, 2 * c_out), **f32)
            dgcnn_edge_bwd_dv(lv["uv"], lv["idx"], lv["winner"], h, lv["coef"], means, c_out=c_out, duv=duv)
            dgcnn_edge_bwd_du(lv["uv"], lv["inv"][0], lv["inv"][1], lv["winner"], h, lv["coef"], means, c_out=c_out, duv=duv)
            self._mark(f"gathers{l + 1}")
            kp = lv["w2"].shape[1]                          # the row length of the level's input, padding included
            xl = s["xp"] if l == 0 else cat[:, COL[l - 1]:COL[l - 1] + kp].contiguous()
            dw2 = _dweight(duv, xl, 2 * c_out, kp, PTF_DW_CHUNK_ROWS)[:, :lv["k"]]
            grads[f"conv{l + 1}.0.weight"] = torch.cat([dw2[:c_out] - dw2[c_out:], dw2[c_out:]], 1)
            if l > 0:
                dx_next = ops.gemm(duv, lv["w2"], M=N, N=kp, K=2 * c_out, lda=2 * c_out, ldw=kp, out=torch.empty((N, kp), **f32), ldc=kp,
                                   w_kmajor=True, mode="f32")
            self._mark(f"products{l + 1}_bwd")
        for k, p in self.params.items():
            p.grad = grads[k].reshape(p.shape).contiguous()


class DGCNNFunction(torch.autograd.Function):
    """out = DGCNNFunction.apply(engine.autograd_leaf(device), engine, x, batch_length): the engine's forward.  The points carry no
    gradient, so the node hangs on a one-element leaf the engine owns; backward() runs engine.backward on the incoming gradient, which
    OVERWRITES the .grad of the encoder's parameters.  One application per optimizer step."""

    @staticmethod
    def forward(ctx, leaf, engine, x, batch_length):
        out = engine.forward(x.detach(), batch_length)
        ctx.engine, ctx.token = engine, engine.saved
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.engine.saved is not ctx.token:
            raise RuntimeError("DGCNNFunction: the engine ran another forward since this application")
        ctx.engine.backward(grad_out.contiguous())
        return torch.zeros(1, dtype=grad_out.dtype, device=grad_out.device), None, None, None


class DGCNNDescriptorTrainEngine:
    """the three trainable stages of a matching.DescriptorNetwork(encoder="dgcnn.dynamic") (eval mode; its train() keeps raising):
    forward() takes DescriptorNetwork.forward's arguments without start / seed (this family samples nothing) and returns part_feats
    connected to autograd, so that a loss on it and .backward() fill the .grad of every parameter; optimizer_step() steps the three
    engines."""

    def __init__(self, net):
        from .matching import DescriptorNetwork

        if not isinstance(net, DescriptorNetwork):
            raise TypeError("DGCNNDescriptorTrainEngine: expected a DescriptorNetwork")
        if not isinstance(net.encoder, DGCNNDynamic):
            raise TypeError("DGCNNDescriptorTrainEngine: expected a DescriptorNetwork with a DGCNN encoder (encoder='dgcnn.dynamic'); the "
                            "PointNet++ family trains through matching_encoder_train.DescriptorTrainEngine")
        if net.gemm_mode != "f32":
            raise NotImplementedError("matcher training runs in the exact-fp32 GEMM mode only")
        self.net = net
        self.encoder = DGCNNTrainEngine(net.encoder)
        self.tf_self1 = PointTransformerTrainEngine(net.tf_self1)
        self.tf_cross1 = CrossAttentionTrainEngine(net.tf_cross1)

    def forward(self, part_pcs, n_pcs, part_valids) -> torch.Tensor:
        from .matching import _flatten, _gpu, make_layout

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
        lengths = lengths[lengths > 0]
        feats = DGCNNFunction.apply(self.encoder.autograd_leaf(pts.device), self.encoder, pts, lengths)
        feats = PointTransformerFunction.apply(pts, feats, self.tf_self1, lengths)
        return CrossAttentionFunction.apply(feats, self.tf_cross1, layout.puz_points)

    def optimizer_step(self, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
        for eng in (self.encoder, self.tf_self1, self.tf_cross1):
            eng.optimizer_step(lr, betas, eps)
