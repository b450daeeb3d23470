"""The matcher's two layers between its encoder and its head (csrc/matching_tf.hip, include/pfpp.h "matcher middle").

PointTransformerLayer (tf_self1) and CrossAttentionLayer (tf_cross1) of the reference's Jigsaw_matching/model/jigsaw/attention_layer.py
with its parameter and buffer names, forward only, eval mode only.

* PointTransformerLayer: one GEMM projects the descriptors onto q | k | v; the 16 nearest rows of the same piece are searched twice
  in FEATURE space, once among the k rows and once among the v rows (the reference's two knn_and_group calls: slot t of one list is
  paired with slot t of the other); one launch does linear_p, linear_w, the softmax over the neighbours and the weighted sum.  A piece
  of fewer than 16 points pads its lists with the index N, which stands for an all-zero row at a zero offset and is NOT masked out of
  the softmax (to_dense_batch(fill_value=N) behind an appended zero row).
* CrossAttentionLayer: multi-head self-attention over all points of a puzzle (8 heads of 16, temperature 4, no mask), residual,
  LayerNorm(eps=1e-6), the position-wise feed-forward 128 -> 256 -> 128, residual, LayerNorm(eps=1e-6).

gemm_mode ("f32": exact fp32 matrix instructions, the default; "f16x3": split-f16) reaches only the GEMMs; the three kernels of
csrc/matching_tf.hip have one arithmetic."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check
from .matching_encoder import MAX_PIECE

FEAT = 128            # descriptor width the kernels are built for
NSAMPLE = 16          # neighbours
HEAD_DIM = 16         # width of an attention head / channels that share a weight in the point transformer
PTF_WEIGHT_FLOATS = 3140     # PFPP_PTF_WEIGHT_FLOATS (include/pfpp.h)


def _p(t: Optional[torch.Tensor], byte_offset: int = 0) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr() + byte_offset)


def _gpu(t, dtype: torch.dtype, name: str, shape_tail: Optional[tuple] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if shape_tail is not None and tuple(t.shape[-len(shape_tail):]) != shape_tail:
        raise ValueError(f"{name}: expected [..., {', '.join(map(str, shape_tail))}], got {tuple(t.shape)}")
    return t


def _lengths(o, total: int, name: str) -> np.ndarray:
    n = np.asarray(o.detach().cpu().numpy() if torch.is_tensor(o) else o).astype(np.int64).reshape(-1)
    if n.size == 0 or (n < 1).any():
        raise ValueError(f"{name}: every entry needs at least one point")
    if int(n.sum()) != total:
        raise ValueError(f"{name} sums to {int(n.sum())} points, the input has {total}")
    return n


class LayerNorm1d(nn.BatchNorm1d):
    """the reference's name for a BatchNorm1d over the channel axis of [N, k, C]; in eval mode a per-channel affine (folded at pack time)"""


def _fold(bn: nn.BatchNorm1d, bias: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """BatchNorm in eval mode behind a linear layer with `bias` -> (scale, shift): bn(y + bias) = y scale + shift"""
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    b = bn.running_mean.new_zeros(()) if bias is None else bias.detach()
    return scale, (b - bn.running_mean) * scale + bn.bias.detach()


class _Packed:
    """pack cache of a module: rebuilt when a parameter or buffer was written, replaced or moved since the last pack"""

    def _packed(self) -> dict:
        tensors = list(self.state_dict(keep_vars=True).values())
        key = tuple((t.data_ptr(), t._version, t.device) for t in tensors)
        if self._pack is None or key != self._pack_key:
            with torch.no_grad():
                self._pack, self._pack_key = self._build_pack(), key
        return self._pack


# ------------------------------------------------------------------------------------------------------------------ kernels
def feat_knn(feats: torch.Tensor, piece_off: torch.Tensor, max_piece: int, *, col: int = 0, width: int = FEAT, K: int = NSAMPLE) -> torch.Tensor:
    """the min(K, n_piece) nearest rows of the same piece by squared distance between the columns [col, col + width) of feats
    (float32 [N, ld], searched in place) -> int32 [N, K] global indices, ascending by (distance bits, index); the slots behind them hold N"""
    _gpu(feats, torch.float32, "feats")
    _gpu(piece_off, torch.int64, "piece_off")
    if feats.dim() != 2 or feats.stride(1) != 1 or col < 0 or col + width > feats.shape[1]:
        raise ValueError(f"feats: expected [N, >= {col + width}] with contiguous rows, got {tuple(feats.shape)}")
    if width != FEAT or K != NSAMPLE:
        raise ValueError(f"feat_knn: the kernel is built for rows of {FEAT} channels and K = {NSAMPLE} (got {width}, {K})")
    if max_piece > MAX_PIECE:
        raise ValueError(f"a piece of {max_piece} points: the limit is {MAX_PIECE}")
    N = feats.shape[0]
    idx = torch.empty((N, K), dtype=torch.int32, device=feats.device)
    check(_lib.load().pfpp_feat_knn(_p(feats, 4 * col), feats.stride(0), _p(piece_off.contiguous()), piece_off.numel() - 1, N, width, K,
                                    int(max_piece), _p(idx), ops._stream()), "pfpp_feat_knn")
    return idx


def ptf_aggregate(qkv: torch.Tensor, xyz: torch.Tensor, idx_k: torch.Tensor, idx_v: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """qkv float32 [N, 384] (q | k | v), xyz [N, 3], idx_k / idx_v int32 [N, 16] (N = the zero row), weights: the packed
    linear_p / linear_w of PointTransformerLayer -> float32 [N, 128]"""
    _gpu(qkv, torch.float32, "qkv", (3 * FEAT,))
    N = qkv.shape[0]
    _gpu(xyz, torch.float32, "xyz", (3,))
    for t, nm in ((idx_k, "idx_k"), (idx_v, "idx_v")):
        _gpu(t, torch.int32, nm, (NSAMPLE,))
        if t.shape[0] != N or not t.is_contiguous():
            raise ValueError(f"{nm}: expected contiguous [{N}, {NSAMPLE}], got {tuple(t.shape)}")
    _gpu(weights, torch.float32, "weights")
    if weights.numel() != PTF_WEIGHT_FLOATS or not weights.is_contiguous():
        raise ValueError(f"weights: expected {PTF_WEIGHT_FLOATS} packed floats")
    if xyz.shape[0] != N or not xyz.is_contiguous() or not qkv.is_contiguous():
        raise ValueError("qkv and xyz: contiguous, one row per point")
    out = torch.empty((N, FEAT), dtype=torch.float32, device=qkv.device)
    check(_lib.load().pfpp_ptf_aggregate(_p(qkv), _p(qkv, 4 * FEAT), _p(qkv, 8 * FEAT), 3 * FEAT, _p(xyz), _p(idx_k), _p(idx_v), _p(weights),
                                         N, FEAT, NSAMPLE, _p(out), ops._stream()), "pfpp_ptf_aggregate")
    return out


def attn_rows16(qkv: torch.Tensor, seq_off: torch.Tensor, seq_len: torch.Tensor, max_len: int, H: int, scale: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """unmasked softmax((q scale) k^T) v for 16-wide heads from a packed [rows, 3 H 16] projection; sequences are the row ranges
    [seq_off[s], seq_off[s] + seq_len[s]) (int32), of any length -> [rows, H 16].  Rows outside every sequence are not written."""
    _gpu(qkv, torch.float32, "qkv")
    _gpu(seq_off, torch.int32, "seq_off")
    _gpu(seq_len, torch.int32, "seq_len")
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * HEAD_DIM or not qkv.is_contiguous():
        raise ValueError(f"qkv: expected contiguous [rows, {3 * H * HEAD_DIM}], got {tuple(qkv.shape)}")
    if seq_off.shape != seq_len.shape or seq_off.dim() != 1 or not seq_off.is_contiguous() or not seq_len.is_contiguous():
        raise ValueError("seq_off / seq_len: one int32 entry per sequence")
    if out is None:
        out = torch.empty((qkv.shape[0], H * HEAD_DIM), dtype=torch.float32, device=qkv.device)
    else:
        _gpu(out, torch.float32, "out", (H * HEAD_DIM,))
        if out.shape[0] != qkv.shape[0] or not out.is_contiguous():
            raise ValueError("out: contiguous, one row per row of qkv")
    check(_lib.load().pfpp_attn_rows16(_p(qkv), _p(out), _p(seq_off), _p(seq_len), seq_off.numel(), int(max_len), H, HEAD_DIM, float(scale),
                                       ops._stream()), "pfpp_attn_rows16")
    return out


def layernorm128(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """nn.LayerNorm(128, eps) with weight and bias over the rows of x float32 [rows, 128] (ops.layernorm covers 256, 512 and 1024 channels)"""
    _gpu(x, torch.float32, "x", (FEAT,))
    _gpu(gamma, torch.float32, "gamma", (FEAT,))
    _gpu(beta, torch.float32, "beta", (FEAT,))
    if x.dim() != 2 or not x.is_contiguous() or not gamma.is_contiguous() or not beta.is_contiguous():
        raise ValueError(f"x: expected contiguous [rows, {FEAT}], got {tuple(x.shape)}")
    out = torch.empty_like(x)
    check(_lib.load().pfpp_layernorm128(_p(x), _p(gamma), _p(beta), _p(out), x.shape[0], FEAT, float(eps), ops._stream()), "pfpp_layernorm128")
    return out


def _check_mode(gemm_mode: str) -> str:
    if gemm_mode not in ("f32", "f16x3"):
        raise ValueError("gemm_mode: 'f32' or 'f16x3'")
    return gemm_mode


# ------------------------------------------------------------------------------------------------------------------ tf_self1
class PointTransformerLayer(_Packed, nn.Module):
    """attention_layer.py:159-225 (the argument is spelled `nsampmle` there)"""

    def __init__(self, in_feat: int, out_feat: int, n_heads: int = 8, nsampmle: int = 16, gemm_mode: str = "f32"):
        super().__init__()
        if out_feat != in_feat:
            raise ValueError(f"out_feat ({out_feat}) != in_feat ({in_feat}): the layer is built for equal widths")
        if in_feat != FEAT:
            raise ValueError(f"in_feat = {in_feat}: the kernels are built for {FEAT} channels")
        if nsampmle != NSAMPLE:
            raise ValueError(f"nsampmle = {nsampmle}: the kernels are built for K = {NSAMPLE} neighbours")
        if n_heads < 1 or out_feat % n_heads or out_feat // n_heads != HEAD_DIM:
            raise ValueError(f"n_heads = {n_heads}: out_feat / n_heads must be {HEAD_DIM}")
        self.gemm_mode = _check_mode(gemm_mode)
        self.mid_feat = self.out_feat = out_feat
        self.share_feat, self.n_sample = n_heads, nsampmle
        w = out_feat // n_heads
        self.linear_q = nn.Linear(in_feat, out_feat)
        self.linear_k = nn.Linear(in_feat, out_feat)
        self.linear_v = nn.Linear(in_feat, out_feat)
        self.linear_p = nn.Sequential(nn.Linear(3, 3), LayerNorm1d(3), nn.ReLU(inplace=True), nn.Linear(3, out_feat))
        self.linear_w = nn.Sequential(LayerNorm1d(out_feat), nn.ReLU(inplace=True), nn.Linear(out_feat, w), LayerNorm1d(w), nn.ReLU(inplace=True),
                                      nn.Linear(w, w))
        self.softmax = nn.Softmax(dim=1)
        self._pack, self._pack_key = None, None
        self.stage_events: Optional[list] = None       # set to a list to get (stage name, HIP event) pairs from the next forward
        super().train(False)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("PointTransformerLayer runs in eval mode only: matcher training is not built")
        return super().train(False)

    def _build_pack(self) -> dict:
        dev = self.linear_q.weight.device
        w_qkv = torch.cat([self.linear_q.weight, self.linear_k.weight, self.linear_v.weight], 0).detach().contiguous()
        b_qkv = torch.cat([self.linear_q.bias, self.linear_k.bias, self.linear_v.bias], 0).detach().contiguous()
        wp = torch.zeros(PTF_WEIGHT_FLOATS, dtype=torch.float32, device=dev)
        p0, pbn, p3 = self.linear_p[0], self.linear_p[1], self.linear_p[3]
        wbn0, w2, wbn3, w5 = self.linear_w[0], self.linear_w[2], self.linear_w[3], self.linear_w[5]
        s, t = _fold(pbn, p0.bias)
        wp[0:9], wp[12:15], wp[16:19] = p0.weight.detach().reshape(-1), s, t
        wp[20:404], wp[404:532] = p3.weight.detach().reshape(-1), p3.bias.detach()
        wp[532:660], wp[660:788] = _fold(wbn0)
        wp[788:2836] = w2.weight.detach().reshape(-1)
        wp[2836:2852], wp[2852:2868] = _fold(wbn3, w2.bias)
        wp[2868:3124], wp[3124:3140] = w5.weight.detach().reshape(-1), w5.bias.detach()
        return {"w_qkv": w_qkv, "b_qkv": b_qkv, "wp": wp}

    def _mark(self, name: str) -> None:
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    @torch.no_grad()
    def forward(self, p: torch.Tensor, x: torch.Tensor, o, *, return_indices: bool = False, indices=None):
        """p float32 [N, 3], x float32 [N, 128] on the GPU; o: the piece lengths (host array or tensor; any number of puzzles, flat).
        indices = (idx_k, idx_v) int32 [N, 16] replaces the two searches; return_indices also returns the pair used."""
        _gpu(p, torch.float32, "p", (3,))
        _gpu(x, torch.float32, "x", (FEAT,))
        if p.dim() != 2 or x.dim() != 2 or p.shape[0] != x.shape[0]:
            raise ValueError(f"p {tuple(p.shape)} and x {tuple(x.shape)}: one row per point")
        if self.linear_q.weight.device != x.device:
            raise ValueError(f"the module lives on {self.linear_q.weight.device}, x on {x.device}")
        N = x.shape[0]
        lengths = _lengths(o, N, "o")
        if int(lengths.max()) > MAX_PIECE:
            raise ValueError(f"a piece of {int(lengths.max())} points: the limit is {MAX_PIECE}")
        pack = self._packed()
        p, x = p.contiguous(), x.contiguous()
        self._mark("begin")
        qkv = ops.gemm(x, pack["w_qkv"], M=N, N=3 * FEAT, K=FEAT, lda=FEAT, bias=pack["b_qkv"], mode=self.gemm_mode)
        self._mark("projection")
        if indices is None:
            off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(x.device)
            idx_k = feat_knn(qkv, off, int(lengths.max()), col=FEAT)
            self._mark("neighbours_k")
            idx_v = feat_knn(qkv, off, int(lengths.max()), col=2 * FEAT)
            self._mark("neighbours_v")
        else:
            idx_k, idx_v = (t.contiguous() for t in indices)
        out = ptf_aggregate(qkv, p, idx_k, idx_v, pack["wp"])
        self._mark("aggregate")
        return (out, idx_k, idx_v) if return_indices else out


# ------------------------------------------------------------------------------------------------------------------ tf_cross1
class _ScaledDotProductAttention(nn.Module):
    def __init__(self, temperature: float):
        super().__init__()
        self.temperature = temperature


class _MultiHeadAttention(nn.Module):
    def __init__(self, n_head: int, d_model: int):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_model // n_head, d_model // n_head
        self.w_qs = nn.Linear(d_model, n_head * self.d_k, bias=False)
        self.w_ks = nn.Linear(d_model, n_head * self.d_k, bias=False)
        self.w_vs = nn.Linear(d_model, n_head * self.d_v, bias=False)
        self.fc = nn.Linear(n_head * self.d_v, d_model, bias=False)
        self.attention = _ScaledDotProductAttention(temperature=self.d_k ** 0.5)
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-6)


class _PositionwiseFeedForward(nn.Module):
    def __init__(self, d_in: int, d_hid: int):
        super().__init__()
        self.w_1 = nn.Linear(d_in, d_hid)
        self.w_2 = nn.Linear(d_hid, d_in)
        self.layer_norm = nn.LayerNorm(d_in, eps=1e-6)


class CrossAttentionLayer(_Packed, nn.Module):
    """attention_layer.py:100-115: self-attention over all points of a puzzle, then the position-wise feed-forward"""

    def __init__(self, d_in: int, n_head: int, gemm_mode: str = "f32"):
        super().__init__()
        if d_in != FEAT:
            raise ValueError(f"d_in = {d_in}: the layer is built for {FEAT} channels")
        if n_head < 1 or d_in % n_head or d_in // n_head != HEAD_DIM:
            raise ValueError(f"n_head = {n_head}: d_in / n_head must be {HEAD_DIM} (the attention kernel's head width)")
        self.gemm_mode = _check_mode(gemm_mode)
        self.attn = _MultiHeadAttention(n_head, d_in)
        self.pos_ffn = _PositionwiseFeedForward(d_in, 2 * d_in)
        self._pack, self._pack_key = None, None
        self.stage_events: Optional[list] = None
        super().train(False)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("CrossAttentionLayer runs in eval mode only: matcher training is not built")
        return super().train(False)

    def _build_pack(self) -> dict:
        a, f = self.attn, self.pos_ffn
        c = lambda t: t.detach().contiguous()
        return {"w_qkv": torch.cat([a.w_qs.weight, a.w_ks.weight, a.w_vs.weight], 0).detach().contiguous(), "fc": c(a.fc.weight),
                "g1": c(a.layer_norm.weight), "b1": c(a.layer_norm.bias), "w1": c(f.w_1.weight), "bw1": c(f.w_1.bias), "w2": c(f.w_2.weight),
                "bw2": c(f.w_2.bias), "g2": c(f.layer_norm.weight), "b2": c(f.layer_norm.bias)}

    def _mark(self, name: str) -> None:
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    @torch.no_grad()
    def forward(self, x: torch.Tensor, seq_lengths=None, *, return_stages: bool = False):
        """x: flat float32 [N, 128] with seq_lengths = the puzzles' point counts, or the reference's dense [B, N_sum, 128] (every
        puzzle N_sum points; the result has that shape again).  return_stages also returns (attention output, post-LayerNorm 1)."""
        _gpu(x, torch.float32, "x", (FEAT,))
        if self.attn.fc.weight.device != x.device:
            raise ValueError(f"the module lives on {self.attn.fc.weight.device}, x on {x.device}")
        shape = x.shape
        if x.dim() == 3:
            if seq_lengths is not None:
                raise ValueError("seq_lengths: not with a dense [B, N_sum, 128] input")
            lengths = np.full(shape[0], shape[1], dtype=np.int64)
            x = x.reshape(-1, FEAT)
        elif x.dim() == 2:
            if seq_lengths is None:
                raise ValueError("seq_lengths: needed with a flat [N, 128] input")
            lengths = None
        else:
            raise ValueError(f"x: expected [N, 128] or [B, N_sum, 128], got {tuple(shape)}")
        N = x.shape[0]
        lengths = _lengths(seq_lengths if lengths is None else lengths, N, "seq_lengths")
        if N >= 2 ** 31:
            raise ValueError("more than 2^31 rows")
        pack = self._packed()
        x = x.contiguous()
        H = self.attn.n_head
        seq_len = torch.from_numpy(lengths.astype(np.int32)).to(x.device)
        seq_off = torch.from_numpy((np.cumsum(lengths) - lengths).astype(np.int32)).to(x.device)
        self._mark("begin")
        qkv = ops.gemm(x, pack["w_qkv"], M=N, N=3 * FEAT, K=FEAT, lda=FEAT, mode=self.gemm_mode)
        self._mark("projection")
        att = attn_rows16(qkv, seq_off, seq_len, int(lengths.max()), H, 1.0 / self.attn.attention.temperature)
        self._mark("attention")
        y = ops.gemm(att, pack["fc"], M=N, N=FEAT, K=FEAT, lda=FEAT, residual=x, ldr=FEAT, mode=self.gemm_mode)
        y1 = layernorm128(y, pack["g1"], pack["b1"], 1e-6)
        h = ops.gemm(y1, pack["w1"], M=N, N=2 * FEAT, K=FEAT, lda=FEAT, bias=pack["bw1"], act="relu", mode=self.gemm_mode)
        z = ops.gemm(h, pack["w2"], M=N, N=FEAT, K=2 * FEAT, lda=2 * FEAT, bias=pack["bw2"], residual=y1, ldr=FEAT, mode=self.gemm_mode)
        out = layernorm128(z, pack["g2"], pack["b2"], 1e-6).reshape(shape)
        self._mark("tail")
        return (out, att, y1) if return_stages else out
