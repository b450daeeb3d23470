"""Training of the matcher's ragged PointNet++ encoder (csrc/pointnet_ragged_train.hip; include/pfpp.h "matcher front end, training").

The reference's PointNet2PTMSGDynamic (Jigsaw_matching/model/modules/encoder/pointnet2_pointwise/pointnet2_msg.py:48-94) in .train():
each of its 33 convolutions in front of conv1 is followed by a BatchNorm that normalises with the statistics of ALL rows of the call and moves its running
buffers, so the training forward is not the eval forward of matching_encoder.PointNet2PTMSGDynamic (which folds the BatchNorms).

* ragged_bn_stats / ragged_bn_apply / ragged_pool_bwd / ragged_bn_relu_bwd / ragged_group_bwd / ragged_interp_bwd: the six entries on
  their own; inverse_lists_of: the CSR lists the two gathers' backwards walk (plumbing in torch).
* EncoderTrainEngine: forward(x, batch_length) of an eval-mode PointNet2PTMSGDynamic with batch statistics (the module's 66 running
  buffers and num_batches_tracked are updated), backward(dout) with the gradients in the .grad of its 134 parameters, optimizer_step()
  = torch.optim.Adam through pfpp_adamw.  Sampling, search, grouping and interpolation are the eval path's kernels; every product
  (forward, dX, dW) is the exact-fp32 GEMM.
* EncoderFunction: the engine as a torch.autograd.Function; it chains with matching_transformer_train.PointTransformerFunction.
* DescriptorTrainEngine: encoder, tf_self1 and tf_cross1 of a matching.DescriptorNetwork under one loss.backward().
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import train_ops as T
from ._lib import check
from .matching_encoder import (MAX_PIECE, NSAMPLE, PointNet2PTMSGDynamic, _p, level_counts, ragged_fps, ragged_group, ragged_interp,
                               ragged_knn)
from .matching_transformer_train import (PTF_DW_CHUNK_ROWS, CrossAttentionFunction, CrossAttentionTrainEngine, PointTransformerFunction,
                                         PointTransformerTrainEngine, _dweight)

RAGGED_TRAIN_WS_DOUBLES = 256 * 2 * 1024 + 1024      # PFPP_RAGGED_TRAIN_WS_DOUBLES (include/pfpp.h)
MAX_C = 1024
SA_NAMES, FP_NAMES = ("sa1", "sa2", "sa3", "sa4"), ("fp4", "fp3", "fp2", "fp1")


def _f32(t: torch.Tensor, name: str, rows: Optional[int] = None, cols: Optional[int] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{name}: expected a float32 tensor on the GPU")
    if t.dim() != 2 or t.stride(1) != 1 or (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name}: expected [{'rows' if rows is None else rows}, {'C' if cols is None else cols}] with contiguous rows, "
                         f"got {tuple(t.shape)}")
    return t


def _width(C_: int) -> None:
    if C_ % 4 or not 4 <= C_ <= MAX_C:
        raise ValueError(f"C = {C_}: a multiple of 4, at most {MAX_C}")


def train_workspace(device) -> torch.Tensor:
    """the fp64 workspace of the entries that reduce over rows (4 MB, whatever the sizes are)"""
    return torch.empty(RAGGED_TRAIN_WS_DOUBLES, dtype=torch.float64, device=device)


def _ws(ws: Optional[torch.Tensor], device) -> torch.Tensor:
    if ws is None:
        return train_workspace(device)
    if ws.dtype != torch.float64 or not ws.is_cuda or ws.numel() < RAGGED_TRAIN_WS_DOUBLES or not ws.is_contiguous():
        raise ValueError(f"workspace: expected at least {RAGGED_TRAIN_WS_DOUBLES} contiguous float64 on the GPU")
    return ws


# ------------------------------------------------------------------------------------------------------------------ kernels
def ragged_bn_stats(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, momentum: float = 0.1,
                    running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                    ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y float32 [rows, C] (row stride a multiple of 4) -> coef float32 [4, C] = a | b | mean | rstd of BatchNorm on the statistics of
    all rows (biased variance); the running buffers, when given, move by `momentum` (unbiased variance)"""
    _f32(y, "y")
    rows, C_ = y.shape
    _width(C_)
    if rows < 2:
        raise ValueError(f"a batch-statistics BatchNorm over {rows} row: it needs at least 2 (torch refuses it too)")
    if y.stride(0) % 4 or y.data_ptr() % 16:
        raise ValueError("y: rows of a multiple of 4 floats, 16-byte aligned")
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.shape != (C_,) or not t.is_contiguous()):
            raise ValueError(f"{nm}: expected contiguous float32 [{C_}] on the GPU")
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var go together")
    coef = torch.empty((4, C_), dtype=torch.float32, device=y.device)
    check(_lib.load().pfpp_ragged_bn_stats(_p(y), rows, C_, y.stride(0), _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean),
                                           _p(running_var), _p(coef), _p(_ws(ws, y.device)), ops._stream()), "pfpp_ragged_bn_stats")
    for t in (running_mean, running_var):
        if t is not None:
            torch.autograd.graph.increment_version(t)      # written through a raw pointer: the module's pack cache watches _version
    return coef


def ragged_bn_apply(y: torch.Tensor, coef: torch.Tensor, pool: int = 0, out: Optional[torch.Tensor] = None, c_off: int = 0,
                    want_winner: bool = False):
    """h = relu(y a + b) [rows, C]; with pool the max over each `pool` consecutive rows [rows / pool, C] (and the first row that attains
    it, int32, -1 where no row is positive).  out / c_off: write into the columns [c_off, c_off + C) of a wider tensor."""
    _f32(y, "y")
    rows, C_ = y.shape
    _width(C_)
    _f32(coef, "coef", 4, C_)
    if pool < 0 or (pool and rows % pool):
        raise ValueError(f"pool = {pool} does not divide the {rows} rows")
    out_rows = rows // pool if pool else rows
    if out is None:
        out, c_off = torch.empty((out_rows, C_), dtype=torch.float32, device=y.device), 0
    else:
        _f32(out, "out", out_rows)
        if c_off % 4 or c_off < 0 or c_off + C_ > out.shape[1] or out.stride(0) % 4:
            raise ValueError("out: the columns [c_off, c_off + C) must exist and start at a multiple of 4")
    winner = torch.empty((out_rows, C_), dtype=torch.int32, device=y.device) if want_winner else None
    check(_lib.load().pfpp_ragged_bn_apply(_p(y), rows, C_, y.stride(0), _p(coef), C.c_void_p(out.data_ptr() + 4 * c_off), out.stride(0),
                                           int(pool), _p(winner), ops._stream()), "pfpp_ragged_bn_apply")
    return (out, winner) if want_winner else out


def ragged_pool_bwd(y: torch.Tensor, coef: torch.Tensor, pool: int, dout: torch.Tensor, c_off: int = 0) -> torch.Tensor:
    """backward of ragged_bn_apply's max: dh [rows, C] = dout[g, c_off + c] on the winning row of group g, 0 elsewhere"""
    _f32(y, "y")
    rows, C_ = y.shape
    _width(C_)
    _f32(coef, "coef", 4, C_)
    if pool < 1 or rows % pool:
        raise ValueError(f"pool = {pool} does not divide the {rows} rows")
    _f32(dout, "dout", rows // pool)
    if c_off < 0 or c_off + C_ > dout.shape[1]:
        raise ValueError("dout: the columns [c_off, c_off + C) must exist")
    dh = torch.empty((rows, C_), dtype=torch.float32, device=y.device)
    check(_lib.load().pfpp_ragged_pool_bwd(_p(y), rows // pool, int(pool), C_, y.stride(0), _p(coef), C.c_void_p(dout.data_ptr() + 4 * c_off),
                                           dout.stride(0), _p(dh), ops._stream()), "pfpp_ragged_pool_bwd")
    return dh


def ragged_bn_relu_bwd(y: torch.Tensor, dh: torch.Tensor, coef: torch.Tensor, gamma: torch.Tensor, ws: Optional[torch.Tensor] = None,
                       dy: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """backward of h = relu(BN_train(y)): dh = d loss / d h [rows, C] contiguous -> (dy, dgamma, dbeta); dy None: in place over dh"""
    _f32(y, "y")
    rows, C_ = y.shape
    _width(C_)
    _f32(coef, "coef", 4, C_)
    _f32(dh, "dh", rows, C_)
    dy = dh if dy is None else _f32(dy, "dy", rows, C_)
    if not dh.is_contiguous() or not dy.is_contiguous() or rows < 1:
        raise ValueError("dh / dy: contiguous [rows, C] with at least one row")
    if gamma.shape != (C_,) or gamma.dtype != torch.float32 or not gamma.is_cuda or not gamma.is_contiguous():
        raise ValueError(f"gamma: expected contiguous float32 [{C_}] on the GPU")
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    check(_lib.load().pfpp_ragged_bn_relu_bwd(_p(y), _p(dh), rows, C_, y.stride(0), _p(coef), _p(gamma), _p(dgamma), _p(dbeta), _p(dy),
                                              _p(_ws(ws, y.device)), ops._stream()), "pfpp_ragged_bn_relu_bwd")
    return dy, dgamma, dbeta


def inverse_lists_of(idx: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """idx int32 [M, K] with values in [0, n) -> (off int64 [n + 1], ent int32 [M K]): the flat positions e = row K + slot whose index is
    p are ent[off[p] : off[p + 1]], ascending (a stable sort).  matching_transformer_train.inverse_lists for a table whose rows are
    not the points it indexes.  Plumbing in torch, no kernel."""
    flat = idx.reshape(-1).long()
    ent = torch.sort(flat, stable=True).indices.to(torch.int32)
    off = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
    off[1:] = torch.cumsum(torch.bincount(flat, minlength=n)[:n], 0)
    return off, ent.contiguous()


def _lists(off: torch.Tensor, ent: torch.Tensor, n: int, n_ent: int) -> None:
    if off.dtype != torch.int64 or ent.dtype != torch.int32 or not off.is_cuda or not ent.is_cuda:
        raise ValueError("off / ent: int64 offsets and int32 entries on the GPU")
    if off.shape != (n + 1,) or ent.shape != (n_ent,) or not off.is_contiguous() or not ent.is_contiguous():
        raise ValueError(f"off / ent: expected [{n + 1}] and [{n_ent}], got {tuple(off.shape)} and {tuple(ent.shape)}")


def ragged_group_bwd(dA: torch.Tensor, D: int, off: torch.Tensor, ent: torch.Tensor, K: int, pool: int, dfeats: torch.Tensor,
                     accumulate: bool = False) -> torch.Tensor:
    """backward of ragged_group's feature columns: dfeats[p, :D] (=, or +=) the sum of dA's rows whose neighbour index is p, in list
    order; (off, ent) = inverse_lists_of(idx[:, :K], number of points).  The coordinate columns of dA get no gradient."""
    _f32(dA, "dA")
    _f32(dfeats, "dfeats")
    if pool < K or dA.shape[0] % pool or D < 1 or D > dA.shape[1] or D > dfeats.shape[1]:
        raise ValueError(f"dA {tuple(dA.shape)}: rows in groups of pool = {pool} >= K = {K}, at least D = {D} columns on both sides")
    S, Np = dA.shape[0] // pool, dfeats.shape[0]
    _lists(off, ent, Np, S * K)
    check(_lib.load().pfpp_ragged_group_bwd(_p(dA), dA.stride(0), int(D), _p(off), _p(ent), S, int(K), int(pool), Np, _p(dfeats),
                                            dfeats.stride(0), int(accumulate), ops._stream()), "pfpp_ragged_group_bwd")
    return dfeats


def ragged_interp_bwd(dout: torch.Tensor, D1: int, D2: int, weights: Optional[torch.Tensor], off: Optional[torch.Tensor],
                      ent: Optional[torch.Tensor], S: int, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """backward of ragged_interp towards points2: dout [N, >= D1 + D2] -> dpoints2 [S, D2]; weights [N, 3] = the forward's, (off, ent) =
    inverse_lists_of(idx [N, 3], S).  S == 1: the column sums of dout[:, D1 : D1 + D2] (weights and lists unused)."""
    _f32(dout, "dout")
    N = dout.shape[0]
    if D1 < 0 or D2 < 1 or D1 + D2 > dout.shape[1] or S < 1:
        raise ValueError(f"dout {tuple(dout.shape)}: needs D1 + D2 = {D1 + D2} columns; S >= 1")
    dp2 = torch.empty((S, D2), dtype=torch.float32, device=dout.device)
    if S == 1:
        if D2 > MAX_C:
            raise ValueError(f"one centroid: at most {MAX_C} channels")
        weights = off = ent = None
    else:
        _f32(weights, "weights", N, 3)
        if not weights.is_contiguous():
            raise ValueError("weights: contiguous [N, 3]")
        _lists(off, ent, S, 3 * N)
    check(_lib.load().pfpp_ragged_interp_bwd(_p(dout), dout.stride(0), int(D1), int(D2), _p(weights), _p(off), _p(ent), N, int(S), _p(dp2),
                                             _p(_ws(ws, dout.device)), ops._stream()), "pfpp_ragged_interp_bwd")
    return dp2


# ------------------------------------------------------------------------------------------------------------------ the engine
class _Conv:
    """one convolution + BatchNorm of the encoder: the modules, their parameter names and what the last forward kept"""
    __slots__ = ("name", "conv", "bn", "cname", "bname", "K", "N", "w", "a", "y", "coef", "h", "pool", "winner")

    def __init__(self, name: str, cname: str, bname: str, conv, bn):
        self.name, self.cname, self.bname, self.conv, self.bn = name, cname, bname, conv, bn
        self.N, self.K = conv.weight.shape[0], conv.weight.shape[1]
        self.w = self.a = self.y = self.coef = self.h = self.winner = None
        self.pool = 0


class EncoderTrainEngine:
    """one training step of a PointNet2PTMSGDynamic (the module itself stays in eval mode; what is here is the reference's .train()
    arithmetic).  forward() normalises the 33 BatchNorms with the statistics of the whole flat call, writes the module's 66 running
    buffers and bumps num_batches_tracked; it keeps, per convolution, its input rows, its output y before the BatchNorm and the four
    coefficient vectors (the grouped operands are kept, not re-gathered), plus the interpolation weights and the inverse lists, which
    depend on the coordinates only and are built once per forward.  backward(dout) OVERWRITES the .grad of all 134 parameters (the 33
    convolution biases sit in front of a batch-statistics BatchNorm: exact zeros); sa1's input gradient is not computed.
    optimizer_step() is torch.optim.Adam (weight decay 0) through pfpp_adamw."""

    def __init__(self, encoder: PointNet2PTMSGDynamic):
        if not isinstance(encoder, PointNet2PTMSGDynamic):
            raise TypeError("EncoderTrainEngine: expected a PointNet2PTMSGDynamic")
        if encoder.gemm_mode != "f32":
            raise NotImplementedError("the encoder's training runs in the exact-fp32 GEMM mode only")
        self.encoder = encoder
        self.params: Dict[str, torch.nn.Parameter] = dict(encoder.named_parameters())
        self.sa: List[List[List[_Conv]]] = []
        for name in SA_NAMES:
            m = getattr(encoder, name)
            self.sa.append([[_Conv(f"{name}.{k}.{j}", f"{name}.conv_blocks.{k}.{j}", f"{name}.bn_blocks.{k}.{j}", c, b)
                             for j, (c, b) in enumerate(zip(convs, bns))] for k, (convs, bns) in enumerate(zip(m.conv_blocks, m.bn_blocks))])
        self.fp: List[List[_Conv]] = []
        for name in FP_NAMES:
            m = getattr(encoder, name)
            self.fp.append([_Conv(f"{name}.{j}", f"{name}.mlp_convs.{j}", f"{name}.mlp_bns.{j}", c, b)
                            for j, (c, b) in enumerate(zip(m.mlp_convs, m.mlp_bns))])
        self.convs: List[_Conv] = [ly for lvl in self.sa for sc in lvl for ly in sc] + [ly for lvl in self.fp for ly in lvl]
        self.state: Dict[str, Tuple[torch.Tensor, torch.Tensor, int]] = {}
        self.saved: dict = {}
        self._wsp: Optional[torch.Tensor] = None
        self.leaf: Optional[torch.Tensor] = None       # what EncoderFunction hangs on: the points carry no gradient
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

    # ---- forward
    def _layer(self, ly: _Conv, a: torch.Tensor, ws, *, pool: int = 0, out=None, c_off: int = 0, keep: bool = False) -> torch.Tensor:
        rows = a.shape[0]
        if rows < 2:
            raise ValueError(f"{ly.bname}: a batch-statistics BatchNorm over {rows} row (a level of this call has one point); torch refuses "
                             "it too: Expected more than 1 value per channel when training")
        w = torch.zeros((ly.N, a.shape[1]), dtype=torch.float32, device=a.device)        # the raw weights, K padded with zeros like the A operand
        w[:, :ly.K] = ly.conv.weight.detach().reshape(ly.N, ly.K)
        # the bias stays in y: it moves the running mean (the normalised value does not see it)
        y = ops.gemm(a, w, M=rows, N=ly.N, K=ly.K, lda=a.shape[1], ldw=w.shape[1], bias=ly.conv.bias.detach(), mode="f32")
        bn = ly.bn
        coef = ragged_bn_stats(y, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, bn.running_mean, bn.running_var, ws)
        res = ragged_bn_apply(y, coef, pool, out, c_off, want_winner=keep and pool > 0)
        h, ly.winner = res if keep and pool > 0 else (res, None)
        bn.num_batches_tracked.add_(1)
        ly.w, ly.a, ly.y, ly.coef, ly.pool = w, a, y, coef, pool
        ly.h = h if (keep or not pool) and out is None else None
        return h

    @torch.no_grad()
    def forward(self, x: torch.Tensor, batch_length, start=None, seed: Optional[int] = None, keep_activations: bool = False) -> torch.Tensor:
        """x float32 [N_sum, feat_in] (coordinates first) on the GPU, batch_length: the piece lengths, start / seed as in
        PointNet2PTMSGDynamic.forward -> the descriptors [N_sum, feat_out] of the reference's .train() forward.  keep_activations
        (tests): saved["relu"][name] = every ReLU's output, saved["winner"][name] = every pool's winning row."""
        enc = self.encoder
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"x: must live on the GPU (got {getattr(x, 'device', type(x).__name__)}); there is no CPU path")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != enc.feat_in:
            raise ValueError(f"x: expected float32 [N_sum, {enc.feat_in}], got {x.dtype} {tuple(x.shape)}")
        if enc.conv1.weight.device != x.device:
            raise ValueError(f"the module lives on {enc.conv1.weight.device}, x on {x.device}")
        lengths = np.asarray(batch_length.detach().cpu().numpy() if torch.is_tensor(batch_length) else batch_length).astype(np.int64).reshape(-1)
        if lengths.size == 0 or (lengths < 1).any():
            raise ValueError("batch_length: every piece needs at least one point")
        if int(lengths.sum()) != x.shape[0]:
            raise ValueError(f"batch_length sums to {int(lengths.sum())} points, x has {x.shape[0]}")
        if int(lengths.max()) > MAX_PIECE:
            raise ValueError(f"a piece of {int(lengths.max())} points: the sampling kernel holds at most {MAX_PIECE}")
        dev, P = x.device, lengths.size
        counts = level_counts(lengths)
        off_h = np.zeros((5, P + 1), dtype=np.int64)
        np.cumsum(counts, 1, out=off_h[:, 1:])
        totals = off_h[:, -1]
        if int(totals[:4].min()) < 2:               # a set-abstraction level has 16 / 32 rows per centroid; a propagation level one per point
            l = int(np.argmin(totals[:4]))
            raise ValueError(f"level {l} of this call has {int(totals[l])} point: the BatchNorms of {FP_NAMES[3 - l]} would see 1 row per "
                             "channel, which torch refuses in training (Expected more than 1 value per channel when training)")
        off = torch.from_numpy(off_h).to(dev)
        if start is None:
            g = torch.Generator(device=dev)
            g.manual_seed(int(seed) if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))
            cnt_d = (off[:4, 1:] - off[:4, :-1])
            st = torch.minimum((torch.rand((4, P), generator=g, device=dev, dtype=torch.float64) * cnt_d).to(torch.int64), cnt_d - 1)
        else:
            st_h = np.asarray(start.detach().cpu().numpy() if torch.is_tensor(start) else start).astype(np.int64)
            if st_h.shape != (P, 4):
                raise ValueError(f"start: expected [P, 4] = ({P}, 4), got {st_h.shape}")
            if (st_h < 0).any() or (st_h.T >= counts[:4]).any():
                raise ValueError("start: an index outside its piece at that level")
            st = torch.from_numpy(np.ascontiguousarray(st_h.T)).to(dev)
        ws = self._workspace(dev)
        x = x.contiguous()
        xyz0 = x if enc.feat_in == 3 else x[:, :3].contiguous()
        self._mark("begin")
        # ---- geometry: the eval path's kernels, call for call (matching_encoder.PointNet2PTMSGDynamic.forward)
        cen_all, xyz_all = ragged_fps(xyz0, off, st.contiguous(), int(lengths.max()), int(totals[1:].sum()))
        base = np.concatenate([[0], np.cumsum(totals[1:])])
        xyz = [xyz0] + [xyz_all[base[l]:base[l + 1]] for l in range(4)]
        cen = [cen_all[base[l]:base[l + 1]] for l in range(4)]
        nbr = [ragged_knn(xyz[l], off[l], xyz[l + 1], off[l + 1], NSAMPLE[1]) for l in range(4)]
        back = [ragged_knn(xyz[l + 1], off[l + 1], xyz[l], off[l], 3, want_count=True) if totals[l + 1] > 1 else (None, None) for l in range(4)]
        self._mark("geometry")
        # ---- the inverse lists of both gathers: they depend on the coordinates only (level 0's grouping gets no gradient)
        ginv = [[inverse_lists_of(nbr[l][:, :K], int(totals[l])) if l > 0 else None for K in NSAMPLE] for l in range(4)]
        iinv = [inverse_lists_of(back[l][0], int(totals[l + 1])) if back[l][0] is not None else None for l in range(4)]
        self._mark("inverse_lists")
        # ---- set abstraction: a K = 16 scale is grouped with pool = 16 (the eval path's fill-up duplicates must not enter the statistics)
        feats = [x]
        for l, name in enumerate(SA_NAMES):
            S = int(totals[l + 1])
            ctot = getattr(enc, name).out_channels
            out = torch.empty((S, ctot), dtype=torch.float32, device=dev)
            c_off = 0
            for layers, K in zip(self.sa[l], NSAMPLE):
                a = ragged_group(feats[l], xyz[l], xyz[l + 1], nbr[l], K, pool=K)
                for j, ly in enumerate(layers):
                    last = j + 1 == len(layers)
                    a = self._layer(ly, a, ws, pool=K if last else 0, out=out if last else None, c_off=c_off if last else 0, keep=keep_activations)
                c_off += layers[-1].N
            feats.append(out)
        self._mark("set_abstraction")
        # ---- feature propagation
        up, interp_w = feats[4], {}
        for l, layers in zip((3, 2, 1, 0), self.fp):
            idx3, cnt3 = back[l]
            a, interp_w[l] = ragged_interp(xyz[l], xyz[l + 1], idx3, cnt3, up, feats[l] if l > 0 else None, want_weights=True)
            for ly in layers:
                a = self._layer(ly, a, ws, keep=keep_activations)
            up = a
        w1 = enc.conv1.weight.detach().reshape(enc.feat_out, -1).contiguous()
        y = ops.linear(up, w1, enc.conv1.bias.detach().contiguous(), mode="f32")
        self._mark("propagation")
        self.saved = {"totals": totals, "counts": counts, "feats": feats, "up": up, "w1": w1, "interp_w": interp_w, "ginv": ginv, "iinv": iinv,
                      "cen": cen, "nbr": nbr, "back": back, "start": st, "N": x.shape[0]}
        if keep_activations:
            self.saved["relu"] = {ly.name: (ly.h if ly.h is not None else None) for ly in self.convs}
            for l, name in enumerate(SA_NAMES):      # a pooled layer's ReLU output is its slice of the level's output
                c_off = 0
                for layers in self.sa[l]:
                    self.saved["relu"][layers[-1].name] = feats[l + 1][:, c_off:c_off + layers[-1].N]
                    c_off += layers[-1].N
            self.saved["winner"] = {ly.name: ly.winner for ly in self.convs if ly.winner is not None}
        return y

    # ---- backward
    def _layer_bwd(self, ly: _Conv, dh: torch.Tensor, ws, grads: dict, need_dx: bool) -> Optional[torch.Tensor]:
        """dh = the gradient at the ReLU's output [rows, C] (consumed: dy is written over it) -> the gradient of the layer's input rows"""
        dy, dgamma, dbeta = ragged_bn_relu_bwd(ly.y, dh, ly.coef, ly.bn.weight.detach(), ws)
        kp = ly.w.shape[1]                          # = the row length of the layer's input, padding included
        dw = _dweight(dy, ly.a, ly.N, kp, PTF_DW_CHUNK_ROWS)
        grads[ly.cname + ".weight"] = dw[:, :ly.K]
        grads[ly.cname + ".bias"] = torch.zeros(ly.N, dtype=torch.float32, device=dh.device)     # in front of a batch-statistics BatchNorm
        grads[ly.bname + ".weight"], grads[ly.bname + ".bias"] = dgamma, dbeta
        if not need_dx:
            return None
        rows = dy.shape[0]
        return ops.gemm(dy, ly.w, M=rows, N=kp, K=ly.N, lda=ly.N, ldw=kp, out=torch.empty((rows, kp), dtype=torch.float32, device=dh.device),
                        ldc=kp, w_kmajor=True, mode="f32")

    @torch.no_grad()
    def backward(self, dout: torch.Tensor) -> None:
        """dout = d loss / d (the last forward's descriptors) [N_sum, feat_out]; the gradients go to the .grad of the parameters"""
        s, enc = self.saved, self.encoder
        if not s:
            raise RuntimeError("backward() before forward()")
        if not isinstance(dout, torch.Tensor) or not dout.is_cuda or dout.dtype != torch.float32 or dout.shape != (s["N"], enc.feat_out):
            raise ValueError(f"dout: expected float32 {(s['N'], enc.feat_out)} on the GPU")
        dout = dout.contiguous()
        dev, totals, feats = dout.device, s["totals"], s["feats"]
        f32 = dict(dtype=torch.float32, device=dev)
        ws = self._workspace(dev)
        grads: Dict[str, torch.Tensor] = {}
        self._mark("begin")
        # ---- conv1 (pointnet2_msg.py:93)
        N, C1 = s["N"], s["up"].shape[1]
        grads["conv1.weight"] = _dweight(dout, s["up"], enc.feat_out, C1, PTF_DW_CHUNK_ROWS)
        grads["conv1.bias"] = T.colsum(dout, torch.zeros(enc.feat_out, **f32))
        d = ops.gemm(dout, s["w1"], M=N, N=C1, K=enc.feat_out, lda=enc.feat_out, ldw=C1, out=torch.empty((N, C1), **f32), ldc=C1, w_kmajor=True,
                     mode="f32")
        self._mark("conv1_bwd")
        # ---- feature propagation, fp1 .. fp4: the gradient of a level's features arrives from the level that took them as points1 ...
        gfeat: List[Optional[torch.Tensor]] = [None] * 5
        for l, layers in zip((0, 1, 2, 3), reversed(self.fp)):
            for ly in reversed(layers):
                d = self._layer_bwd(ly, d, ws, grads, True)
            D1 = feats[l].shape[1] if l > 0 else 0
            D2 = d.shape[1] - D1
            if l > 0:
                gfeat[l] = d[:, :D1].contiguous()
            inv = s["iinv"][l]
            d = ragged_interp_bwd(d, D1, D2, s["interp_w"][l], None if inv is None else inv[0], None if inv is None else inv[1],
                                  int(totals[l + 1]), ws)
        gfeat[4] = d
        self._mark("propagation_bwd")
        # ---- set abstraction, sa4 .. sa1: ... and from the set-abstraction level above, which adds into the same tensor
        for l in (3, 2, 1, 0):
            c_off = 0
            offs = []
            for layers in self.sa[l]:
                offs.append(c_off)
                c_off += layers[-1].N
            for k, (layers, K) in enumerate(zip(self.sa[l], NSAMPLE)):
                last = layers[-1]
                d = ragged_pool_bwd(last.y, last.coef, K, gfeat[l + 1], offs[k])
                for j in range(len(layers) - 1, -1, -1):
                    d = self._layer_bwd(layers[j], d, ws, grads, need_dx=(l > 0 or j > 0))
                if l > 0:                           # sa1's input is the coordinates
                    inv = s["ginv"][l][k]
                    ragged_group_bwd(d, feats[l].shape[1], inv[0], inv[1], K, K, gfeat[l], accumulate=True)
            self._mark(f"{SA_NAMES[l]}_bwd")
        for k, p in self.params.items():
            p.grad = grads[k].reshape(p.shape).contiguous()
        s["gfeat"] = gfeat


class EncoderFunction(torch.autograd.Function):
    """out = EncoderFunction.apply(engine.autograd_leaf(device), engine, x, batch_length, start, seed): the engine's forward.  The points
    carry no gradient, so the node hangs on a one-element leaf the engine owns; backward() runs engine.backward on the incoming gradient,
    which OVERWRITES the .grad of the encoder's parameters.  One application per optimizer step."""

    @staticmethod
    def forward(ctx, leaf, engine, x, batch_length, start=None, seed=None):
        out = engine.forward(x.detach(), batch_length, start=start, seed=seed)
        ctx.engine, ctx.token = engine, engine.saved
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.engine.saved is not ctx.token:
            raise RuntimeError("EncoderFunction: the engine ran another forward since this application")
        ctx.engine.backward(grad_out.contiguous())
        return torch.zeros(1, dtype=grad_out.dtype, device=grad_out.device), None, None, None, None, None


class DescriptorTrainEngine:
    """the three trainable stages of a matching.DescriptorNetwork (eval mode; its train() keeps raising): forward() takes
    DescriptorNetwork.forward's arguments and returns part_feats connected to autograd, so that a loss on it (MatchingHeadLoss, or any
    torch expression) and .backward() fill the .grad of every parameter; optimizer_step() steps the three engines."""

    def __init__(self, net):
        from .matching import DescriptorNetwork, DGCNNDynamic

        if not isinstance(net, DescriptorNetwork):
            raise TypeError("DescriptorTrainEngine: expected a DescriptorNetwork")
        if isinstance(net.encoder, DGCNNDynamic):
            raise NotImplementedError("a DescriptorNetwork with a DGCNN encoder: its forward in eval mode exists (pfpp_hip.matching_dgcnn), its "
                                      "training step (train-mode BatchNorm over all N x 20 rows and the backward) does not")
        if net.gemm_mode != "f32":
            raise NotImplementedError("matcher training runs in the exact-fp32 GEMM mode only")
        self.net = net
        self.encoder = EncoderTrainEngine(net.encoder)
        self.tf_self1 = PointTransformerTrainEngine(net.tf_self1)
        self.tf_cross1 = CrossAttentionTrainEngine(net.tf_cross1)

    def forward(self, part_pcs, n_pcs, part_valids, start=None, seed: Optional[int] = None) -> torch.Tensor:
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
        feats = EncoderFunction.apply(self.encoder.autograd_leaf(pts.device), self.encoder, pts, lengths, start, seed)
        feats = PointTransformerFunction.apply(pts, feats, self.tf_self1, lengths)
        return CrossAttentionFunction.apply(feats, self.tf_cross1, layout.puz_points)

    def optimizer_step(self, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
        for eng in (self.encoder, self.tf_self1, self.tf_cross1):
            eng.optimizer_step(lr, betas, eps)
