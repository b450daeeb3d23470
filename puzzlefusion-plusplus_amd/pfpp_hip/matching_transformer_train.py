"""Training of the matcher's two middle layers: the cross-attention layer tf_cross1 (csrc/matching_tf_train.hip) and the point-transformer
layer tf_self1 (csrc/matching_ptf_train.hip); include/pfpp.h "matcher middle, training".

The reference's CrossAttentionLayer (Jigsaw_matching/model/jigsaw/attention_layer.py:100-115) has no dropout and normalises with
nn.LayerNorm, so its training-time forward is the eval forward; what is here is its backward and Adam:

* attn_rows16_train / attn_rows16_bwd / layernorm128_bwd / relu_bwd: the kernels on their own.
* CrossAttentionTrainEngine: forward() of an eval-mode CrossAttentionLayer that keeps what the backward reads, backward(dout) -> dx
  with the gradients in the .grad of the layer's 12 parameters, optimizer_step() = torch.optim.Adam through pfpp_adamw.  Every GEMM
  runs in the exact-fp32 mode.  No GEMM of the input-gradient chain splits its contraction: a puzzle's dx does not depend on the
  puzzles next to it.  The weight gradients contract over all rows; from 2,048 rows on they run as equal row chunks in the batch
  dimension of one GEMM and are summed in chunk order (by the row count alone; deterministic).
* CrossAttentionFunction: the engine as a torch.autograd.Function of x; it chains with matching_train.MatchingHeadLoss.

The reference's PointTransformerLayer (:159-225) normalises with three BatchNorm1d (LayerNorm1d): in .train() its forward uses the
statistics of all 16 N rows of the flat call and moves the running buffers, so it is not the eval forward:

* ptf_train_*: the nine entries on their own (four forward passes, the BatchNorm finalise, four backward passes); inverse_lists.
* PointTransformerTrainEngine: forward(p, x, o) of an eval-mode PointTransformerLayer with batch statistics (the module's buffers are
  updated), backward(dout) -> dx with the gradients in the .grad of the layer's 20 parameters, optimizer_step() as above.  It keeps
  qkv, the lists and three [N, 16, 16] tensors; nothing of N 16 128 elements exists.
* PointTransformerFunction: that engine as a torch.autograd.Function of x; it chains with CrossAttentionFunction.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import train_ops as T
from ._lib import check
from .matching_train import _mm, _tpad
from .matching_encoder import MAX_PIECE
from .matching_transformer import (FEAT, HEAD_DIM, NSAMPLE, CrossAttentionLayer, PointTransformerLayer, _gpu, _lengths, _p, feat_knn,
                                   layernorm128)

LN_EPS = 1e-6
LN128_BWD_WS_FLOATS = 256 * 4 * 2 * 128        # PFPP_LAYERNORM128_BWD_WS_FLOATS (include/pfpp.h)
DW_CHUNK_ROWS, DW_MAX_CHUNKS = 1024, 64        # weight gradients: rows per batch of the GEMM (at least) and batches (at most)

PARAM_NAMES = ("attn.w_qs.weight", "attn.w_ks.weight", "attn.w_vs.weight", "attn.fc.weight", "attn.layer_norm.weight", "attn.layer_norm.bias",
               "pos_ffn.w_1.weight", "pos_ffn.w_1.bias", "pos_ffn.w_2.weight", "pos_ffn.w_2.bias", "pos_ffn.layer_norm.weight",
               "pos_ffn.layer_norm.bias")


# ------------------------------------------------------------------------------------------------------------------ kernels
def _check_attn(qkv: torch.Tensor, seq_off: torch.Tensor, seq_len: torch.Tensor, H: int) -> None:
    _gpu(qkv, torch.float32, "qkv")
    _gpu(seq_off, torch.int32, "seq_off")
    _gpu(seq_len, torch.int32, "seq_len")
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * HEAD_DIM or not qkv.is_contiguous():
        raise ValueError(f"qkv: expected contiguous [rows, {3 * H * HEAD_DIM}], got {tuple(qkv.shape)}")
    if seq_off.shape != seq_len.shape or seq_off.dim() != 1 or not seq_off.is_contiguous() or not seq_len.is_contiguous():
        raise ValueError("seq_off / seq_len: one int32 entry per sequence")


def _rows_like(t: torch.Tensor, name: str, rows: int, cols: int) -> torch.Tensor:
    _gpu(t, torch.float32, name, (cols,))
    if t.dim() != 2 or t.shape[0] != rows or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous [{rows}, {cols}], got {tuple(t.shape)}")
    return t


def attn_rows16_train(qkv: torch.Tensor, seq_off: torch.Tensor, seq_len: torch.Tensor, max_len: int, H: int, scale: float
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """matching_transformer.attn_rows16 that also returns lse float32 [rows, H] = log sum_j exp((q scale) . k_j); out is bit for bit
    attn_rows16's.  Rows outside every sequence are not written."""
    _check_attn(qkv, seq_off, seq_len, H)
    out = torch.empty((qkv.shape[0], H * HEAD_DIM), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((qkv.shape[0], H), dtype=torch.float32, device=qkv.device)
    check(_lib.load().pfpp_attn_rows16_train(_p(qkv), _p(out), _p(lse), _p(seq_off), _p(seq_len), seq_off.numel(), int(max_len), H, HEAD_DIM,
                                             float(scale), ops._stream()), "pfpp_attn_rows16_train")
    return out, lse


def attn_rows16_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, seq_off: torch.Tensor, seq_len: torch.Tensor,
                    max_len: int, H: int, scale: float, dqkv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """backward of attn_rows16_train: qkv, out, lse of the forward and dout [rows, H 16] -> dqkv [rows, 3 H 16] = dq | dk | dv.  No
    atomics: two calls agree bitwise.  Rows outside every sequence are not written (a dqkv handed in keeps them)."""
    _check_attn(qkv, seq_off, seq_len, H)
    rows = qkv.shape[0]
    _rows_like(out, "out", rows, H * HEAD_DIM)
    _rows_like(dout, "dout", rows, H * HEAD_DIM)
    _rows_like(lse, "lse", rows, H)
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    else:
        _rows_like(dqkv, "dqkv", rows, 3 * H * HEAD_DIM)
    dvec = torch.empty((rows, H), dtype=torch.float32, device=qkv.device)
    check(_lib.load().pfpp_attn_rows16_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(dvec), _p(dqkv), _p(seq_off), _p(seq_len), seq_off.numel(),
                                           int(max_len), H, HEAD_DIM, float(scale), ops._stream()), "pfpp_attn_rows16_bwd")
    return dqkv


def layernorm128_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, eps: float, *, dx: Optional[torch.Tensor] = None,
                     accumulate: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """backward of matching_transformer.layernorm128 from the rows x [rows, 128] before the normalisation -> (dx, dgamma, dbeta).
    accumulate adds into the dx handed in (a residual branch's gradient) instead of overwriting it."""
    _gpu(x, torch.float32, "x", (FEAT,))
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"x: expected contiguous [rows, {FEAT}], got {tuple(x.shape)}")
    rows = x.shape[0]
    _rows_like(dy, "dy", rows, FEAT)
    _gpu(gamma, torch.float32, "gamma", (FEAT,))
    if gamma.dim() != 1 or not gamma.is_contiguous():
        raise ValueError(f"gamma: expected contiguous [{FEAT}]")
    if dx is None:
        if accumulate:
            raise ValueError("accumulate: needs the dx to add into")
        dx = torch.empty_like(x)
    else:
        _rows_like(dx, "dx", rows, FEAT)
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
    ws = torch.empty(LN128_BWD_WS_FLOATS, dtype=torch.float32, device=x.device)
    check(_lib.load().pfpp_layernorm128_bwd(_p(x), _p(dy), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _p(ws), rows, FEAT, float(eps),
                                            int(accumulate), ops._stream()), "pfpp_layernorm128_bwd")
    return dx, dgamma, dbeta


def relu_bwd(h: torch.Tensor, dh: torch.Tensor) -> torch.Tensor:
    """dh <- dh where h > 0, 0 elsewhere (h = 0 and h = -0 included), in place; both [rows, cols] with contiguous rows of one stride"""
    _gpu(h, torch.float32, "h")
    _gpu(dh, torch.float32, "dh")
    if h.dim() != 2 or h.shape != dh.shape or h.stride(1) != 1 or dh.stride(1) != 1 or h.stride(0) != dh.stride(0):
        raise ValueError(f"h {tuple(h.shape)} and dh {tuple(dh.shape)}: two [rows, cols] tensors of one row stride")
    check(_lib.load().pfpp_relu_bwd(_p(h), _p(dh), h.shape[0], h.shape[1], h.stride(0), ops._stream()), "pfpp_relu_bwd")
    return dh


def _dweight(dy_rows: torch.Tensor, a_rows: torch.Tensor, n_out: int, n_in: int, chunk_rows: int = DW_CHUNK_ROWS) -> torch.Tensor:
    """dW [n_out, n_in] = dy^T a, which contracts over the N rows.  From 2 chunk_rows rows on the rows are cut into equal chunks
    (by N alone) that run as the batches of one exact-fp32 GEMM, the rest as one more call, and the partial matrices are
    summed in chunk order: a few output tiles with a contraction over all points would leave most of the chip idle"""
    N = dy_rows.shape[0]
    f32 = dict(dtype=torch.float32, device=dy_rows.device)
    dy_t = _tpad(dy_rows)
    ld = dy_t.shape[1]
    S = min(DW_MAX_CHUNKS, N // chunk_rows)
    if S < 2:
        return _mm(dy_t, a_rows, torch.empty((n_out, n_in), **f32), M=n_out, N=n_in, K=N, lda=ld, ldw=n_in, ldc=n_in, w_kmajor=True)
    c = (N // S) & ~3                                  # rows per chunk: a multiple of 4 keeps every chunk 16-byte aligned
    rest = N - S * c
    parts = torch.empty((S + (1 if rest else 0), n_out, n_in), **f32)
    ops.gemm(dy_t, a_rows, M=n_out, N=n_in, K=c, lda=ld, ldw=n_in, out=parts, ldc=n_in, w_kmajor=True, batch=S, sA=(c, 0),
             sW=(c * n_in, 0), sC=(n_out * n_in, 0), mode="f32")
    if rest:
        ops.gemm(dy_t, a_rows, M=n_out, N=n_in, K=rest, lda=ld, ldw=n_in, out=parts, ldc=n_in, w_kmajor=True, a_off=S * c,
                 w_off=S * c * n_in, c_off=S * n_out * n_in, mode="f32")
    return parts.sum(0)


# ------------------------------------------------------------------------------------------------------------------ the engine
class CrossAttentionTrainEngine:
    """one training step of a CrossAttentionLayer (eval mode: the layer has no train / eval difference): forward() returns the layer's
    output, bit for bit, and keeps x, qkv, att, lse, the two pre-norm rows, y1 and h in `saved`; backward(dout) returns dx and
    OVERWRITES the .grad of the layer's 12 parameters (MatchingHeadTrainEngine's convention); optimizer_step() is torch.optim.Adam
    (weight decay 0) through pfpp_adamw."""

    def __init__(self, layer: CrossAttentionLayer):
        if not isinstance(layer, CrossAttentionLayer):
            raise TypeError("CrossAttentionTrainEngine: expected a CrossAttentionLayer")
        if layer.gemm_mode != "f32":
            raise NotImplementedError("the cross-attention layer's training runs in the exact-fp32 GEMM mode only")
        self.layer = layer
        self.params: Dict[str, torch.nn.Parameter] = dict(layer.named_parameters())
        if tuple(self.params) != PARAM_NAMES:
            raise ValueError(f"not a CrossAttentionLayer: parameters {list(self.params)}")
        self.state: Dict[str, Tuple[torch.Tensor, torch.Tensor, int]] = {}
        self.saved: dict = {}
        self.stage_events: Optional[list] = None       # set to a list to get (stage name, HIP event) pairs from forward() and backward()

    def _mark(self, name: str) -> None:
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    # ---- forward
    @torch.no_grad()
    def forward(self, x: torch.Tensor, seq_lengths=None) -> torch.Tensor:
        """x: flat float32 [N, 128] with seq_lengths = the puzzles' point counts, or dense [B, N_sum, 128]"""
        layer = self.layer
        _gpu(x, torch.float32, "x", (FEAT,))
        if layer.attn.fc.weight.device != x.device:
            raise ValueError(f"the module lives on {layer.attn.fc.weight.device}, x on {x.device}")
        shape = x.shape
        if x.dim() == 3:
            if seq_lengths is not None:
                raise ValueError("seq_lengths: not with a dense [B, N_sum, 128] input")
            lengths = np.full(shape[0], shape[1], dtype=np.int64)
            x = x.reshape(-1, FEAT)
        elif x.dim() == 2:
            if seq_lengths is None:
                raise ValueError("seq_lengths: needed with a flat [N, 128] input")
            lengths = seq_lengths
        else:
            raise ValueError(f"x: expected [N, 128] or [B, N_sum, 128], got {tuple(shape)}")
        N = x.shape[0]
        lengths = _lengths(lengths, N, "seq_lengths")
        if N >= 2 ** 31:
            raise ValueError("more than 2^31 rows")
        pack = layer._packed()
        x = x.contiguous()
        H = layer.attn.n_head
        scale = 1.0 / layer.attn.attention.temperature
        seq_len = torch.from_numpy(lengths.astype(np.int32)).to(x.device)
        seq_off = torch.from_numpy((np.cumsum(lengths) - lengths).astype(np.int32)).to(x.device)
        max_len = int(lengths.max())
        # the module's forward (matching_transformer.CrossAttentionLayer.forward), call for call
        self._mark("begin")
        qkv = ops.gemm(x, pack["w_qkv"], M=N, N=3 * FEAT, K=FEAT, lda=FEAT, mode="f32")
        att, lse = attn_rows16_train(qkv, seq_off, seq_len, max_len, H, scale)
        y = ops.gemm(att, pack["fc"], M=N, N=FEAT, K=FEAT, lda=FEAT, residual=x, ldr=FEAT, mode="f32")
        y1 = layernorm128(y, pack["g1"], pack["b1"], LN_EPS)
        h = ops.gemm(y1, pack["w1"], M=N, N=2 * FEAT, K=FEAT, lda=FEAT, bias=pack["bw1"], act="relu", mode="f32")
        z = ops.gemm(h, pack["w2"], M=N, N=FEAT, K=2 * FEAT, lda=2 * FEAT, bias=pack["bw2"], residual=y1, ldr=FEAT, mode="f32")
        out = layernorm128(z, pack["g2"], pack["b2"], LN_EPS)
        self._mark("forward")
        self.saved = {"x": x, "qkv": qkv, "att": att, "lse": lse, "y": y, "y1": y1, "h": h, "z": z, "seq_off": seq_off, "seq_len": seq_len,
                      "max_len": max_len, "H": H, "scale": scale, "shape": shape}
        return out.reshape(shape)

    # ---- backward
    @torch.no_grad()
    def backward(self, dout: torch.Tensor) -> torch.Tensor:
        """dout = d loss / d (the last forward's output), in its shape -> d loss / d x in x's shape"""
        s = self.saved
        if not s:
            raise RuntimeError("backward() before forward()")
        _gpu(dout, torch.float32, "dout", (FEAT,))
        if dout.shape != s["shape"]:
            raise ValueError(f"dout: expected {tuple(s['shape'])}, got {tuple(dout.shape)}")
        dout = dout.reshape(-1, FEAT).contiguous()
        pack = self.layer._packed()
        x, qkv, att, y, y1, h, z = s["x"], s["qkv"], s["att"], s["y"], s["y1"], s["h"], s["z"]
        N, C, C2, C3 = x.shape[0], FEAT, 2 * FEAT, 3 * FEAT
        f32 = dict(dtype=torch.float32, device=x.device)

        dweight = _dweight
        self._mark("begin")
        # position-wise feed-forward (:88-97): out = LN2(z), z = relu(y1 W1^T + b1) W2^T + b2 + y1
        dz, dg2, db2 = layernorm128_bwd(z, dout, pack["g2"], LN_EPS)
        dbw2 = T.colsum(dz, torch.zeros(C, **f32))
        dw2 = dweight(dz, h, C, C2)
        dh = _mm(dz, pack["w2"], torch.empty((N, C2), **f32), M=N, N=C2, K=C, lda=C, ldw=C2, ldc=C2, w_kmajor=True)
        relu_bwd(h, dh)
        dbw1 = T.colsum(dh, torch.zeros(C2, **f32))
        dw1 = dweight(dh, y1, C2, C)
        dy1 = ops.gemm(dh, pack["w1"], M=N, N=C, K=C2, lda=C2, ldw=C, out=torch.empty((N, C), **f32), ldc=C, w_kmajor=True, residual=dz, ldr=C,
                       mode="f32")
        self._mark("ffn_bwd")
        # attention block (:47-75): y1 = LN1(y), y = att fc^T + x
        dy, dg1, db1 = layernorm128_bwd(y, dy1, pack["g1"], LN_EPS)
        dfc = dweight(dy, att, C, C)
        datt = _mm(dy, pack["fc"], torch.empty((N, C), **f32), M=N, N=C, K=C, lda=C, ldw=C, ldc=C, w_kmajor=True)
        self._mark("fc_bwd")
        dqkv = attn_rows16_bwd(qkv, att, datt, s["lse"], s["seq_off"], s["seq_len"], s["max_len"], s["H"], s["scale"])
        self._mark("attention_bwd")
        dwqkv = dweight(dqkv, x, C3, C)
        dx = ops.gemm(dqkv, pack["w_qkv"], M=N, N=C, K=C3, lda=C3, ldw=C, out=torch.empty((N, C), **f32), ldc=C, w_kmajor=True, residual=dy, ldr=C,
                      mode="f32")
        self._mark("projection_bwd")
        self._store({"attn.w_qs.weight": dwqkv[:C], "attn.w_ks.weight": dwqkv[C:C2], "attn.w_vs.weight": dwqkv[C2:], "attn.fc.weight": dfc,
                     "attn.layer_norm.weight": dg1, "attn.layer_norm.bias": db1, "pos_ffn.w_1.weight": dw1, "pos_ffn.w_1.bias": dbw1,
                     "pos_ffn.w_2.weight": dw2, "pos_ffn.w_2.bias": dbw2, "pos_ffn.layer_norm.weight": dg2, "pos_ffn.layer_norm.bias": db2})
        return dx.reshape(s["shape"])

    def _store(self, grads: Dict[str, torch.Tensor]) -> None:
        for k, p in self.params.items():
            p.grad = grads[k].reshape(p.shape).contiguous()

    # ---- Adam
    def optimizer_step(self, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
        """torch.optim.Adam (weight decay 0) over the parameters that have a gradient; the layer's pack cache sees the writes"""
        lib = _lib.load()
        versions = {k: p._version for k, p in self.params.items() if p.grad is not None}
        for k, p in self.params.items():
            if p.grad is None:
                continue
            ops._chk(p.data, torch.float32, k)
            m, v, step = self.state.get(k) or (torch.zeros_like(p.data), torch.zeros_like(p.data), 0)
            step += 1
            check(lib.pfpp_adamw(_p(p.data), _p(p.grad), _p(m), _p(v), None, None, p.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                 0.0, 1.0 - betas[0] ** step, 1.0 - betas[1] ** step, 1.0, ops._stream()), "pfpp_adamw")
            torch.autograd.graph.increment_version(p)        # the kernel wrote through a raw pointer: _Packed's key watches _version
            self.state[k] = (m, v, step)
        assert all(self.params[k]._version != v for k, v in versions.items()), "the pack cache would not see the step"


class CrossAttentionFunction(torch.autograd.Function):
    """out = CrossAttentionFunction.apply(x, engine, seq_lengths): the engine's forward as a function of x ([N, 128] with lengths, or
    dense [B, N_sum, 128]).  backward() runs engine.backward on the incoming gradient: it returns dx and OVERWRITES the .grad of the
    layer's parameters.  One application per optimizer step: the engine keeps the tensors of its last forward only."""

    @staticmethod
    def forward(ctx, x, engine, seq_lengths=None):
        out = engine.forward(x.detach(), seq_lengths)
        ctx.engine, ctx.token = engine, engine.saved
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.engine.saved is not ctx.token:
            raise RuntimeError("CrossAttentionFunction: the engine ran another forward since this application")
        return ctx.engine.backward(grad_out.contiguous()), None, None


# ------------------------------------------------------------------------------------------------------------------ tf_self1: kernels
PTF_TRAIN_FLOATS = 3748                        # PFPP_PTF_TRAIN_FLOATS (include/pfpp.h): the training pack
PTF_TRAIN_WS_DOUBLES = 1024 * 2304             # PFPP_PTF_TRAIN_WS_DOUBLES
PTF_BWD_W_SUMS, PTF_BWD_U_SUMS, PTF_BWD_R_SUMS = 304, 2304, 539
# where the caller's raw weights go in the training pack: name -> (offset, floats)
PTF_PACK_SLOTS = {"linear_p.0.weight": (0, 9), "linear_p.0.bias": (12, 3), "linear_p.3.weight": (36, 384), "linear_p.3.bias": (420, 128),
                  "linear_w.2.weight": (1060, 2048), "linear_w.2.bias": (3108, 16), "linear_w.5.weight": (3188, 256), "linear_w.5.bias": (3444, 16)}
PTF_PACK_RSTD = (24, 804, 3156)                # rstd of the three BatchNorms (3 / 128 / 16 floats), written by ptf_train_bn_finalise
PTF_BN = ("linear_p.1", "linear_w.0", "linear_w.3")          # the BatchNorms in the order of `which`
PTF_BN_WIDTH = (3, FEAT, NSAMPLE)
PTF_PARAM_NAMES = ("linear_q.weight", "linear_q.bias", "linear_k.weight", "linear_k.bias", "linear_v.weight", "linear_v.bias",
                   "linear_p.0.weight", "linear_p.0.bias", "linear_p.1.weight", "linear_p.1.bias", "linear_p.3.weight", "linear_p.3.bias",
                   "linear_w.0.weight", "linear_w.0.bias", "linear_w.2.weight", "linear_w.2.bias", "linear_w.3.weight", "linear_w.3.bias",
                   "linear_w.5.weight", "linear_w.5.bias")
PTF_DW_CHUNK_ROWS = 128                        # rows per chunk (at least) of the projection's weight gradient: see PointTransformerTrainEngine.backward
PTF_ZERO_GRADS = ("linear_p.0.bias", "linear_w.2.bias")      # in front of a batch-statistics BatchNorm: zero in exact arithmetic, written as zeros


def _ptf_args(qkv: Optional[torch.Tensor], xyz: torch.Tensor, pack: torch.Tensor, **idx: torch.Tensor) -> int:
    """the checks the ptf_train_* wrappers share -> N (qkv None: the entry reads no descriptors)"""
    _gpu(xyz, torch.float32, "xyz", (3,))
    if qkv is not None:
        _gpu(qkv, torch.float32, "qkv", (3 * FEAT,))
        if qkv.dim() != 2 or not qkv.is_contiguous():
            raise ValueError(f"qkv: expected contiguous [N, {3 * FEAT}], got {tuple(qkv.shape)}")
    N = xyz.shape[0] if qkv is None else qkv.shape[0]
    if xyz.dim() != 2 or xyz.shape[0] != N or not xyz.is_contiguous():
        raise ValueError(f"xyz: expected contiguous [{N}, 3], got {tuple(xyz.shape)}")
    for nm, t in idx.items():
        _gpu(t, torch.int32, nm)
        if t.dim() != 2 or t.shape[1] != NSAMPLE:
            raise ValueError(f"{nm}: expected [N, K] with K = {NSAMPLE} (the kernels are built for 16 neighbours), got {tuple(t.shape)}")
        if t.shape[0] != N or not t.is_contiguous():
            raise ValueError(f"{nm}: expected contiguous [{N}, {NSAMPLE}], got {tuple(t.shape)}")
    _gpu(pack, torch.float32, "pack")
    if pack.numel() != PTF_TRAIN_FLOATS or not pack.is_contiguous():
        raise ValueError(f"pack: expected {PTF_TRAIN_FLOATS} packed floats")
    return N


def _ptf_f64(t: torch.Tensor, name: str, n: int, exact: bool = True) -> torch.Tensor:
    _gpu(t, torch.float64, name)
    if t.dim() != 1 or not t.is_contiguous() or (t.numel() != n if exact else t.numel() < n):
        raise ValueError(f"{name}: expected {'' if exact else 'at least '}{n} contiguous float64, got {tuple(t.shape)}")
    return t


def _ptf_sq(t: torch.Tensor, name: str, N: int) -> torch.Tensor:
    _gpu(t, torch.float32, name, (NSAMPLE, NSAMPLE))
    if t.dim() != 3 or t.shape[0] != N or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous [{N}, {NSAMPLE}, {NSAMPLE}], got {tuple(t.shape)}")
    return t


def _ptf_dump(t: Optional[torch.Tensor], N: int, width: int) -> Optional[torch.Tensor]:
    if t is not None:
        _gpu(t, torch.float32, "pre_dump", (NSAMPLE, width))
        if t.dim() != 3 or t.shape[0] != N or not t.is_contiguous():
            raise ValueError(f"pre_dump: expected contiguous [{N}, {NSAMPLE}, {width}], got {tuple(t.shape)}")
    return t


def ptf_train_workspace(device) -> torch.Tensor:
    """the fp64 workspace every ptf_train_* launch with sums writes its per-workgroup partials to (19 MB, whatever N is)"""
    return torch.empty(PTF_TRAIN_WS_DOUBLES, dtype=torch.float64, device=device)


def ptf_train_bn3_stats(xyz: torch.Tensor, idx_k: torch.Tensor, pack: torch.Tensor, ws: torch.Tensor, sums: torch.Tensor) -> torch.Tensor:
    """sums float64 [6] <- sum a | sum a^2 over all 16 N rows, a = linear_p[0] (bias included) of the masked offsets"""
    N = _ptf_args(None, xyz, pack, idx_k=idx_k)
    _ptf_f64(ws, "ws", PTF_TRAIN_WS_DOUBLES, exact=False)
    _ptf_f64(sums, "sums", 6)
    check(_lib.load().pfpp_ptf_train_bn3_stats(_p(xyz), _p(idx_k), _p(pack), N, NSAMPLE, _p(ws), _p(sums), ops._stream()), "pfpp_ptf_train_bn3_stats")
    return sums


def ptf_train_bn_finalise(sums: torch.Tensor, which: int, rows: int, bn: torch.nn.BatchNorm1d, pack: torch.Tensor) -> None:
    """sums float64 [2 C] = sum x | sum x^2 over `rows` rows -> scale | shift | rstd | -mean rstd of BatchNorm `which` (0: linear_p.1,
    1: linear_w.0, 2: linear_w.3) in the pack (biased variance), and bn's running buffers moved by its momentum (unbiased variance)"""
    if which not in (0, 1, 2):
        raise ValueError("which: 0 (BatchNorm(3)), 1 (BatchNorm(128)) or 2 (BatchNorm(16))")
    Cn = PTF_BN_WIDTH[which]
    _ptf_f64(sums, "sums", 2 * Cn)
    _gpu(pack, torch.float32, "pack")
    if pack.numel() != PTF_TRAIN_FLOATS or not pack.is_contiguous():
        raise ValueError(f"pack: expected {PTF_TRAIN_FLOATS} packed floats")
    if rows < 2:
        raise ValueError("rows: a batch of at least 2 rows")
    for nm in ("weight", "bias", "running_mean", "running_var"):
        t = getattr(bn, nm)
        _gpu(t, torch.float32, f"bn.{nm}")
        if t.shape != (Cn,) or not t.is_contiguous():
            raise ValueError(f"bn.{nm}: expected contiguous [{Cn}], got {tuple(t.shape)}")
    check(_lib.load().pfpp_ptf_train_bn_finalise(_p(sums), which, int(rows), _p(bn.weight.data), _p(bn.bias.data), float(bn.eps), float(bn.momentum),
                                                 _p(bn.running_mean), _p(bn.running_var), _p(pack), ops._stream()), "pfpp_ptf_train_bn_finalise")
    for t in (bn.running_mean, bn.running_var):              # written through raw pointers: the module's pack cache watches _version
        torch.autograd.graph.increment_version(t)


def ptf_train_bn128_stats(qkv, xyz, idx_k, pack, ws, sums, pre_dump=None) -> torch.Tensor:
    """sums float64 [256] <- sum r | sum r^2 per channel, r = x_k[idx_k] - x_q + p_r; pre_dump float32 [N, 16, 3] <- what the ReLU of
    linear_p thresholds"""
    N = _ptf_args(qkv, xyz, pack, idx_k=idx_k)
    _ptf_f64(ws, "ws", PTF_TRAIN_WS_DOUBLES, exact=False)
    _ptf_f64(sums, "sums", 2 * FEAT)
    _ptf_dump(pre_dump, N, 3)
    check(_lib.load().pfpp_ptf_train_bn128_stats(_p(qkv), _p(qkv, 4 * FEAT), 3 * FEAT, _p(xyz), _p(idx_k), _p(pack), N, FEAT, NSAMPLE, _p(ws), _p(sums),
                                                 _p(pre_dump), ops._stream()), "pfpp_ptf_train_bn128_stats")
    return sums


def ptf_train_tile(qkv, xyz, idx_k, pack, u, ws, sums, pre_dump=None) -> torch.Tensor:
    """u float32 [N, 16, 16] <- linear_w[2](relu(bn(r))), sums float64 [32] <- sum u | sum u^2; pre_dump [N, 16, 128]"""
    N = _ptf_args(qkv, xyz, pack, idx_k=idx_k)
    _ptf_sq(u, "u", N)
    _ptf_f64(ws, "ws", PTF_TRAIN_WS_DOUBLES, exact=False)
    _ptf_f64(sums, "sums", 2 * NSAMPLE)
    _ptf_dump(pre_dump, N, FEAT)
    check(_lib.load().pfpp_ptf_train_tile(_p(qkv), _p(qkv, 4 * FEAT), 3 * FEAT, _p(xyz), _p(idx_k), _p(pack), N, FEAT, NSAMPLE, _p(u), _p(ws), _p(sums),
                                          _p(pre_dump), ops._stream()), "pfpp_ptf_train_tile")
    return u


def ptf_train_finish(qkv, xyz, idx_k, idx_v, pack, u, w, pre_dump=None) -> torch.Tensor:
    """w float32 [N, 16, 16] <- softmax over the slots of linear_w[5](relu(bn(u))); -> out float32 [N, 128]; pre_dump [N, 16, 16]"""
    N = _ptf_args(qkv, xyz, pack, idx_k=idx_k, idx_v=idx_v)
    _ptf_sq(u, "u", N)
    _ptf_sq(w, "w", N)
    _ptf_dump(pre_dump, N, NSAMPLE)
    out = torch.empty((N, FEAT), dtype=torch.float32, device=qkv.device)
    check(_lib.load().pfpp_ptf_train_finish(_p(qkv, 8 * FEAT), 3 * FEAT, _p(xyz), _p(idx_k), _p(idx_v), _p(pack), N, FEAT, NSAMPLE, _p(u), _p(w), _p(out),
                                            _p(pre_dump), ops._stream()), "pfpp_ptf_train_finish")
    return out


def _ptf_rows(t: torch.Tensor, name: str, N: int, cols: int) -> torch.Tensor:
    _gpu(t, torch.float32, name, (cols,))
    if t.dim() != 2 or t.shape[0] != N or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous [{N}, {cols}], got {tuple(t.shape)}")
    return t


def ptf_train_bwd_w(dout, w, u, qkv, xyz, idx_k, idx_v, pack, dz2, ws, sums, pre_dump=None) -> torch.Tensor:
    """dz2 float32 [N, 16, 16] <- the gradient at the BatchNorm(16) output behind its ReLU; sums float64 [304] <- dW5 | db5 | dbeta | dgamma
    of that BatchNorm; their means go to the pack"""
    N = _ptf_args(qkv, xyz, pack, idx_k=idx_k, idx_v=idx_v)
    _ptf_rows(dout, "dout", N, FEAT)
    for t, nm in ((w, "w"), (u, "u"), (dz2, "dz2")):
        _ptf_sq(t, nm, N)
    _ptf_f64(ws, "ws", PTF_TRAIN_WS_DOUBLES, exact=False)
    _ptf_f64(sums, "sums", PTF_BWD_W_SUMS)
    _ptf_dump(pre_dump, N, NSAMPLE)
    check(_lib.load().pfpp_ptf_train_bwd_w(_p(dout), _p(w), _p(u), _p(qkv, 8 * FEAT), 3 * FEAT, _p(xyz), _p(idx_k), _p(idx_v), _p(pack), N, FEAT, NSAMPLE,
                                           _p(dz2), _p(ws), _p(sums), _p(pre_dump), ops._stream()), "pfpp_ptf_train_bwd_w")
    return dz2


def ptf_train_bwd_u(qkv, xyz, idx_k, pack, u, du, ws, sums, pre_dump=None) -> torch.Tensor:
    """du float32 [N, 16, 16]: dz2 on entry, the gradient of u on return (in place); sums float64 [2304] <- dW2 | dbeta | dgamma of
    BatchNorm(128); their means go to the pack"""
    N = _ptf_args(qkv, xyz, pack, idx_k=idx_k)
    _ptf_sq(u, "u", N)
    _ptf_sq(du, "du", N)
    _ptf_f64(ws, "ws", PTF_TRAIN_WS_DOUBLES, exact=False)
    _ptf_f64(sums, "sums", PTF_BWD_U_SUMS)
    _ptf_dump(pre_dump, N, FEAT)
    check(_lib.load().pfpp_ptf_train_bwd_u(_p(qkv), _p(qkv, 4 * FEAT), 3 * FEAT, _p(xyz), _p(idx_k), _p(pack), N, FEAT, NSAMPLE, _p(u), _p(du), _p(ws),
                                           _p(sums), _p(pre_dump), ops._stream()), "pfpp_ptf_train_bwd_u")
    return du


def ptf_train_bwd_r(dout, w, du, qkv, xyz, idx_k, pack, dqkv, ws, sums, pre_dump=None) -> torch.Tensor:
    """dqkv float32 [N, 384]: columns [0, 128) <- dx_q; sums float64 [539] <- dW3 | db3 | the 27 moments of the BatchNorm(3) backward"""
    N = _ptf_args(qkv, xyz, pack, idx_k=idx_k)
    _ptf_rows(dout, "dout", N, FEAT)
    _ptf_sq(w, "w", N)
    _ptf_sq(du, "du", N)
    _ptf_rows(dqkv, "dqkv", N, 3 * FEAT)
    _ptf_f64(ws, "ws", PTF_TRAIN_WS_DOUBLES, exact=False)
    _ptf_f64(sums, "sums", PTF_BWD_R_SUMS)
    _ptf_dump(pre_dump, N, 3)
    check(_lib.load().pfpp_ptf_train_bwd_r(_p(dout), _p(w), _p(du), _p(qkv), _p(qkv, 4 * FEAT), 3 * FEAT, _p(xyz), _p(idx_k), _p(pack), N, FEAT, NSAMPLE,
                                           _p(dqkv), 3 * FEAT, _p(ws), _p(sums), _p(pre_dump), ops._stream()), "pfpp_ptf_train_bwd_r")
    return dqkv


def inverse_lists(idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """idx int32 [N, 16] (anything outside [0, N) is the padded slot) -> (off int64 [N + 1], ent int32 [16 N]): the entries
    e = point 16 + slot whose index is m are ent[off[m] : off[m + 1]], ascending (a stable sort).  Plumbing in torch, no kernel."""
    N = idx.shape[0]
    flat = idx.reshape(-1).long()
    key = torch.where((flat < 0) | (flat >= N), torch.full_like(flat, N), flat)
    ent = torch.sort(key, stable=True).indices.to(torch.int32)
    off = torch.zeros(N + 1, dtype=torch.int64, device=idx.device)
    off[1:] = torch.cumsum(torch.bincount(key, minlength=N + 1)[:N], 0)
    return off, ent.contiguous()


def ptf_train_bwd_gather(dout, w, du, qkv, xyz, pack, off_k, ent_k, off_v, ent_v, dqkv) -> torch.Tensor:
    """dqkv columns [128, 256) <- dx_k, [256, 384) <- dx_v by the inverse lists of idx_k and idx_v (inverse_lists): every row is written,
    a row in no list with zeros; each row's sum runs in list order"""
    N = _ptf_args(qkv, xyz, pack)
    _ptf_rows(dout, "dout", N, FEAT)
    _ptf_sq(w, "w", N)
    _ptf_sq(du, "du", N)
    _ptf_rows(dqkv, "dqkv", N, 3 * FEAT)
    for off, ent, nm in ((off_k, ent_k, "k"), (off_v, ent_v, "v")):
        _gpu(off, torch.int64, f"off_{nm}")
        _gpu(ent, torch.int32, f"ent_{nm}")
        if off.shape != (N + 1,) or not off.is_contiguous() or ent.shape != (N * NSAMPLE,) or not ent.is_contiguous():
            raise ValueError(f"off_{nm} / ent_{nm}: expected int64 [{N + 1}] and int32 [{N * NSAMPLE}]")
    check(_lib.load().pfpp_ptf_train_bwd_gather(_p(dout), _p(w), _p(du), _p(qkv), _p(qkv, 4 * FEAT), 3 * FEAT, _p(xyz), _p(pack), N, FEAT, NSAMPLE,
                                                _p(off_k), _p(ent_k), _p(off_v), _p(ent_v), _p(dqkv), 3 * FEAT, ops._stream()),
          "pfpp_ptf_train_bwd_gather")
    return dqkv


# ------------------------------------------------------------------------------------------------------------------ tf_self1: the engine
class PointTransformerTrainEngine:
    """one training step of a PointTransformerLayer (the module itself stays in eval mode; what is here is the reference's .train()
    arithmetic): forward() normalises the three BatchNorms with the statistics of the whole flat batch, moves the module's running
    buffers and num_batches_tracked, and keeps qkv, the lists, u, w, the pack and the batch sums in `saved`; backward(dout) returns dx
    and OVERWRITES the .grad of the layer's 20 parameters (18 computed, the two biases in front of a BatchNorm exact zeros);
    optimizer_step() is torch.optim.Adam (weight decay 0) through pfpp_adamw.  Nothing with N 16 128 elements is allocated."""

    def __init__(self, layer: PointTransformerLayer):
        if not isinstance(layer, PointTransformerLayer):
            raise TypeError("PointTransformerTrainEngine: expected a PointTransformerLayer")
        if layer.gemm_mode != "f32":
            raise NotImplementedError("the point-transformer layer's training runs in the exact-fp32 GEMM mode only")
        self.layer = layer
        self.params: Dict[str, torch.nn.Parameter] = dict(layer.named_parameters())
        if tuple(self.params) != PTF_PARAM_NAMES:
            raise ValueError(f"not a PointTransformerLayer: parameters {list(self.params)}")
        self.bns = [dict(layer.named_modules())[k] for k in PTF_BN]
        self.state: Dict[str, Tuple[torch.Tensor, torch.Tensor, int]] = {}
        self.saved: dict = {}
        self._ws: Optional[torch.Tensor] = None
        self.stage_events: Optional[list] = None       # set to a list to get (stage name, HIP event) pairs from forward() and backward()

    _mark = CrossAttentionTrainEngine._mark
    _store = CrossAttentionTrainEngine._store
    optimizer_step = CrossAttentionTrainEngine.optimizer_step      # Adam over self.params / self.state: the same statement

    def _workspace(self, device) -> torch.Tensor:
        if self._ws is None or self._ws.device != device:
            self._ws = ptf_train_workspace(device)
        return self._ws

    # ---- forward
    @torch.no_grad()
    def forward(self, p: torch.Tensor, x: torch.Tensor, o, *, indices=None, pre_dump: bool = False) -> torch.Tensor:
        """p float32 [N, 3], x float32 [N, 128], o: the piece lengths of the whole flat batch -> out [N, 128].  indices = (idx_k, idx_v)
        int32 [N, 16] replaces the two searches.  pre_dump (tests): saved["pre"] = the three pre-activations the ReLUs threshold."""
        layer = self.layer
        _gpu(p, torch.float32, "p", (3,))
        _gpu(x, torch.float32, "x", (FEAT,))
        if p.dim() != 2 or x.dim() != 2 or p.shape[0] != x.shape[0]:
            raise ValueError(f"p {tuple(p.shape)} and x {tuple(x.shape)}: one row per point")
        if layer.linear_q.weight.device != x.device:
            raise ValueError(f"the module lives on {layer.linear_q.weight.device}, x on {x.device}")
        N = x.shape[0]
        lengths = _lengths(o, N, "o")
        if int(lengths.max()) > MAX_PIECE:
            raise ValueError(f"a piece of {int(lengths.max())} points: the limit is {MAX_PIECE}")
        pack = layer._packed()
        p, x = p.contiguous(), x.contiguous()
        dev, f32, f64 = x.device, dict(dtype=torch.float32, device=x.device), dict(dtype=torch.float64, device=x.device)
        self._mark("begin")
        qkv = ops.gemm(x, pack["w_qkv"], M=N, N=3 * FEAT, K=FEAT, lda=FEAT, bias=pack["b_qkv"], mode="f32")
        self._mark("projection")
        if indices is None:
            off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
            idx_k = feat_knn(qkv, off, int(lengths.max()), col=FEAT)
            idx_v = feat_knn(qkv, off, int(lengths.max()), col=2 * FEAT)
        else:
            idx_k, idx_v = (t.contiguous() for t in indices)
        self._mark("neighbours")
        tw = torch.zeros(PTF_TRAIN_FLOATS, **f32)
        for k, (lo, n) in PTF_PACK_SLOTS.items():
            tw[lo:lo + n] = self.params[k].detach().reshape(-1)
        ws = self._workspace(dev)
        sums = [torch.empty(2 * c, **f64) for c in PTF_BN_WIDTH]
        pre = (torch.empty((N, NSAMPLE, 3), **f32), torch.empty((N, NSAMPLE, FEAT), **f32), torch.empty((N, NSAMPLE, NSAMPLE), **f32)) if pre_dump \
            else (None, None, None)
        rows = N * NSAMPLE
        u, w = torch.empty((N, NSAMPLE, NSAMPLE), **f32), torch.empty((N, NSAMPLE, NSAMPLE), **f32)
        ptf_train_bn3_stats(p, idx_k, tw, ws, sums[0])
        ptf_train_bn_finalise(sums[0], 0, rows, self.bns[0], tw)
        self._mark("bn3_stats")
        ptf_train_bn128_stats(qkv, p, idx_k, tw, ws, sums[1], pre[0])
        ptf_train_bn_finalise(sums[1], 1, rows, self.bns[1], tw)
        self._mark("bn128_stats")
        ptf_train_tile(qkv, p, idx_k, tw, u, ws, sums[2], pre[1])
        ptf_train_bn_finalise(sums[2], 2, rows, self.bns[2], tw)
        self._mark("tile")
        out = ptf_train_finish(qkv, p, idx_k, idx_v, tw, u, w, pre[2])
        for bn in self.bns:
            bn.num_batches_tracked.add_(1)
        self._mark("finish")
        self.saved = {"p": p, "x": x, "qkv": qkv, "idx_k": idx_k, "idx_v": idx_v, "tw": tw, "u": u, "w": w, "sums": sums, "pre": pre}
        return out

    # ---- backward
    @torch.no_grad()
    def backward(self, dout: torch.Tensor, *, pre_dump: bool = False) -> torch.Tensor:
        """dout = d loss / d (the last forward's output) [N, 128] -> d loss / d x [N, 128]; p and the lists get no gradient"""
        s = self.saved
        if not s:
            raise RuntimeError("backward() before forward()")
        p, x, qkv, idx_k, idx_v, tw, u, w = (s[k] for k in ("p", "x", "qkv", "idx_k", "idx_v", "tw", "u", "w"))
        N, C, C3 = x.shape[0], FEAT, 3 * FEAT
        _gpu(dout, torch.float32, "dout", (FEAT,))
        if dout.shape != (N, FEAT):
            raise ValueError(f"dout: expected {(N, FEAT)}, got {tuple(dout.shape)}")
        dout = dout.contiguous()
        pack = self.layer._packed()
        f32, f64 = dict(dtype=torch.float32, device=x.device), dict(dtype=torch.float64, device=x.device)
        ws = self._workspace(x.device)
        sw, su, sr = torch.empty(PTF_BWD_W_SUMS, **f64), torch.empty(PTF_BWD_U_SUMS, **f64), torch.empty(PTF_BWD_R_SUMS, **f64)
        pre = (torch.empty((N, NSAMPLE, 3), **f32), torch.empty((N, NSAMPLE, FEAT), **f32), torch.empty((N, NSAMPLE, NSAMPLE), **f32)) if pre_dump \
            else (None, None, None)
        du = torch.empty((N, NSAMPLE, NSAMPLE), **f32)
        dqkv = torch.empty((N, C3), **f32)
        self._mark("begin")
        ptf_train_bwd_w(dout, w, u, qkv, p, idx_k, idx_v, tw, du, ws, sw, pre[2])
        self._mark("bwd_w")
        ptf_train_bwd_u(qkv, p, idx_k, tw, u, du, ws, su, pre[1])
        self._mark("bwd_u")
        ptf_train_bwd_r(dout, w, du, qkv, p, idx_k, tw, dqkv, ws, sr, pre[0])
        self._mark("bwd_r")
        off_k, ent_k = inverse_lists(idx_k)
        off_v, ent_v = inverse_lists(idx_v)
        self._mark("inverse_lists")
        ptf_train_bwd_gather(dout, w, du, qkv, p, tw, off_k, ent_k, off_v, ent_v, dqkv)
        self._mark("gather")
        # the projection's weight gradient contracts over all N rows on the fp32 matrix instructions, one running sum per entry: the
        # rounding of a chain grows with its length (1.1e-6 of the maximum over 1,150 rows against a bar of 6.7e-7 for linear_v.weight,
        # whose float32 yardstick is a plain gather-and-sum), so chunks start at 2 x 128 rows here, not at 2 x 1,024
        dwqkv = _dweight(dqkv, x, C3, C, PTF_DW_CHUNK_ROWS)
        dbqkv = T.colsum(dqkv, torch.zeros(C3, **f32))
        dx = ops.gemm(dqkv, pack["w_qkv"], M=N, N=C, K=C3, lda=C3, ldw=C, out=torch.empty((N, C), **f32), ldc=C, w_kmajor=True, mode="f32")
        self._mark("projection_bwd")
        # the small gradients are the folded fp64 sums; dW0 is a closed form of the 27 moments (the BatchNorm(3) backward is linear in them)
        rows = float(N * NSAMPLE)
        s0 = s["sums"][0]
        mean0 = s0[:3] / rows
        scale0 = self.params["linear_p.1.weight"].detach().double() / torch.sqrt(s0[3:] / rows - mean0 * mean0 + self.bns[0].eps)
        mom = sr[4 * C:]
        dbeta0, dgamma0, A, X, D = mom[0:3], mom[3:6], mom[6:15].reshape(3, 3), mom[15:24].reshape(3, 3), mom[24:27]
        dw0 = scale0[:, None] * (A - (dbeta0 / rows)[:, None] * D[None, :] - (dgamma0 / rows)[:, None] * X)
        K2 = NSAMPLE * NSAMPLE
        g = {"linear_q.weight": dwqkv[:C], "linear_k.weight": dwqkv[C:2 * C], "linear_v.weight": dwqkv[2 * C:], "linear_q.bias": dbqkv[:C],
             "linear_k.bias": dbqkv[C:2 * C], "linear_v.bias": dbqkv[2 * C:], "linear_p.0.weight": dw0.float(), "linear_p.1.weight": dgamma0.float(),
             "linear_p.1.bias": dbeta0.float(), "linear_p.3.weight": sr[:3 * C].float(), "linear_p.3.bias": sr[3 * C:4 * C].float(),
             "linear_w.0.weight": su[NSAMPLE * C + C:].float(), "linear_w.0.bias": su[NSAMPLE * C:NSAMPLE * C + C].float(),
             "linear_w.2.weight": su[:NSAMPLE * C].float(), "linear_w.3.weight": sw[K2 + 2 * NSAMPLE:].float(),
             "linear_w.3.bias": sw[K2 + NSAMPLE:K2 + 2 * NSAMPLE].float(), "linear_w.5.weight": sw[:K2].float(), "linear_w.5.bias": sw[K2:K2 + NSAMPLE].float()}
        for k in PTF_ZERO_GRADS:
            g[k] = torch.zeros_like(self.params[k])
        self._store(g)
        s["du"], s["dqkv"], s["pre_bwd"] = du, dqkv, pre
        self._mark("small_grads")
        return dx


class PointTransformerFunction(torch.autograd.Function):
    """out = PointTransformerFunction.apply(p, x, engine, o, indices=None): the engine's forward as a function of x.  backward() runs
    engine.backward on the incoming gradient: it returns dx (p and the lists get none) and OVERWRITES the .grad of the layer's
    parameters.  One application per optimizer step: the engine keeps the tensors of its last forward only."""

    @staticmethod
    def forward(ctx, p, x, engine, o, indices=None):
        out = engine.forward(p.detach(), x.detach(), o, indices=indices)
        ctx.engine, ctx.token = engine, engine.saved
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.engine.saved is not ctx.token:
            raise RuntimeError("PointTransformerFunction: the engine ran another forward since this application")
        return None, ctx.engine.backward(grad_out.contiguous()), None, None, None
