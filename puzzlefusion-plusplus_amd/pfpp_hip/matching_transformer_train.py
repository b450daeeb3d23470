"""Training of the matcher's cross-attention layer tf_cross1 (csrc/matching_tf_train.hip, include/pfpp.h "matcher middle, training").

The reference's CrossAttentionLayer (Jigsaw_matching/model/jigsaw/attention_layer.py:100-115) has no dropout and normalises with
nn.LayerNorm, so its training-time forward is the eval forward; what is here is its backward and Adam:

* attn_rows16_train / attn_rows16_bwd / layernorm128_bwd / relu_bwd: the kernels on their own.
* CrossAttentionTrainEngine: forward() of an eval-mode CrossAttentionLayer that keeps what the backward reads, backward(dout) -> dx
  with the gradients in the .grad of the layer's 12 parameters, optimizer_step() = torch.optim.Adam through pfpp_adamw.  Every GEMM
  runs in the exact-fp32 mode.  No GEMM of the input-gradient chain splits its contraction: a puzzle's dx does not depend on the
  puzzles next to it.  The weight gradients contract over all rows; from 2,048 rows on they run as equal row chunks in the batch
  dimension of one GEMM and are summed in chunk order (by the row count alone; deterministic).
* CrossAttentionFunction: the engine as a torch.autograd.Function of x; it chains with matching_train.MatchingHeadLoss.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import train_ops as T
from ._lib import check
from .matching_train import _mm, _tpad
from .matching_transformer import FEAT, HEAD_DIM, CrossAttentionLayer, _gpu, _lengths, _p, layernorm128

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

        def dweight(dy_rows: torch.Tensor, a_rows: torch.Tensor, n_out: int, n_in: int) -> torch.Tensor:
            """dW [n_out, n_in] = dy^T a, which contracts over the rows.  From 2 DW_CHUNK_ROWS rows on the rows are cut into equal chunks
            (by N alone) that run as the batches of one exact-fp32 GEMM, the rest as one more call, and the partial matrices are
            summed in chunk order: a few output tiles with a contraction over all points would leave most of the chip idle"""
            dy_t = _tpad(dy_rows)
            ld = dy_t.shape[1]
            S = min(DW_MAX_CHUNKS, N // DW_CHUNK_ROWS)
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
