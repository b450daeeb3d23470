"""The matcher's DGCNN encoder, forward in eval mode (csrc/dgcnn.hip, include/pfpp.h "DGCNN encoder").

DGCNNDynamic of the reference's Jigsaw_matching/model/modules/encoder/dgcnn.py:130-213 with its module structure and parameter
names: points and piece lengths -> per-point descriptors [N_sum, feat_dim].  Four levels (in -> 64 -> 64 -> 128 -> 256) find the 20
nearest points OF THE SAME PIECE in the current feature space, run a 1x1 convolution without bias over cat(x_j - x_i, x_i), BatchNorm,
LeakyReLU(0.2) and take the maximum over the 20 slots (padded slots of a piece shorter than 20 are all-zero rows that take part);
cat(x1 .. x4) [N, 512] then goes through conv5, bn5 and LeakyReLU(0.2).

The form computed here never builds [N, 20, 2 C_in].  With W = [W_a | W_b] along the input columns, slot j of point i has the
pre-activation W_a x_j + (W_b - W_a) x_i; BatchNorm in eval mode is the per-channel affine s z + t and LeakyReLU is increasing, so

    uv = X [W_a ; W_b - W_a]^T                          one [N, C_in] x [C_in, 2 C_out] product per level (ops.gemm, exact fp32)
    z_ij = u[j] + v[i] for a real slot, 0 for a padded slot
    e_i = max_j z_ij where s >= 0, min_j z_ij where s < 0
    x_l[i] = LeakyReLU(e_i s + t)

Level 1 goes through the same product with its three input columns padded to four with zeros.  x1 .. x4 are written straight into
the [N, 512] operand of conv5.  Eval mode only; global_feat=True and the dense DGCNN are not built."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check

K_NEIGHBOURS = 20
WIDTHS = (64, 64, 128, 256)                    # C_out of the four levels
CAT = sum(WIDTHS)                              # 512: the operand of conv5
COL = (0, 64, 128, 256)                        # where x1 .. x4 start in it
SLOPE = 0.2
MAX_PIECE = 8192
KNN_WIDTHS = (3, 64, 128)
EDGE_WIDTHS = (64, 128, 256)


def _p(t: Optional[torch.Tensor], byte_off: int = 0) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr() + byte_off)


def _gpu(t: torch.Tensor, dtype: torch.dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    return t


# ------------------------------------------------------------------------------------------------------------------ kernels
def dgcnn_knn(feats: torch.Tensor, piece_off: torch.Tensor, max_piece: int, *, col: int = 0, width: Optional[int] = None,
              K: int = K_NEIGHBOURS, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the min(K, n_piece) nearest rows of the same piece (the row itself included) by squared distance between the columns
    [col, col + width) of feats (float32 [N, ld], searched in place) -> int32 [N, K] global indices, ascending by (distance bits, index);
    the slots behind them hold N"""
    _gpu(feats, torch.float32, "feats")
    _gpu(piece_off, torch.int64, "piece_off")
    if feats.dim() != 2 or feats.stride(1) != 1:
        raise ValueError(f"feats: expected [N, ld] with contiguous rows, got {tuple(feats.shape)}")
    width = feats.shape[1] - col if width is None else width
    if col < 0 or col + width > feats.shape[1]:
        raise ValueError(f"feats: columns [{col}, {col + width}) of {feats.shape[1]}")
    if width not in KNN_WIDTHS or K != K_NEIGHBOURS:
        raise ValueError(f"dgcnn_knn: the kernel is built for rows of {KNN_WIDTHS} channels and K = {K_NEIGHBOURS} (got {width}, {K})")
    if max_piece > MAX_PIECE:
        raise ValueError(f"a piece of {max_piece} points: the limit is {MAX_PIECE}")
    N = feats.shape[0]
    if out is None:
        out = torch.empty((N, K), dtype=torch.int32, device=feats.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (N, K) or not out.is_contiguous():
        raise ValueError("out: expected contiguous int32 [N, K]")
    check(_lib.load().pfpp_dgcnn_knn(_p(feats, 4 * col), feats.stride(0), _p(piece_off.contiguous()), piece_off.numel() - 1, N, width, K,
                                     int(max_piece), _p(out), ops._stream()), "pfpp_dgcnn_knn")
    return out


def dgcnn_edge_max(uv: torch.Tensor, idx: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, *, c_out: int, ld: Optional[int] = None,
                   out: Optional[torch.Tensor] = None, c_off: int = 0, slope: float = SLOPE) -> torch.Tensor:
    """uv float32 = [u | v] of N rows with row stride ld (a [N, ld] tensor, or a flat buffer with ld given), idx int32 [N, 20]
    (N = the padded slot), scale / shift float32 [c_out] -> LeakyReLU(extremum_j(u[idx[i, j]] + v[i]) scale + shift), written to the
    columns [c_off, c_off + c_out) of out (float32 [N, ldo]; a fresh [N, c_out] without one)"""
    _gpu(uv, torch.float32, "uv")
    _gpu(idx, torch.int32, "idx")
    _gpu(scale, torch.float32, "scale")
    _gpu(shift, torch.float32, "shift")
    if c_out not in EDGE_WIDTHS:
        raise ValueError(f"dgcnn_edge_max: the kernel is built for {EDGE_WIDTHS} output channels (got {c_out})")
    if idx.dim() != 2 or idx.shape[1] != K_NEIGHBOURS or not idx.is_contiguous():
        raise ValueError(f"idx: expected contiguous int32 [N, {K_NEIGHBOURS}], got {tuple(idx.shape)}")
    N = idx.shape[0]
    if not uv.is_contiguous() or (ld is None and uv.dim() != 2):
        raise ValueError("uv: expected a contiguous [N, ld] tensor, or a contiguous flat buffer with ld given")
    ld = uv.shape[1] if ld is None else int(ld)
    if ld < 2 * c_out or (N and uv.numel() < (N - 1) * ld + 2 * c_out):
        raise ValueError(f"uv: {uv.numel()} floats do not hold {N} rows of {2 * c_out} with stride {ld}")
    if scale.numel() != c_out or shift.numel() != c_out:
        raise ValueError("scale / shift: one per output channel")
    if out is None:
        out = torch.empty((N, c_out), dtype=torch.float32, device=uv.device)
    _gpu(out, torch.float32, "out")
    if out.dim() != 2 or out.shape[0] != N or out.stride(1) != 1 or c_off < 0 or c_off + c_out > out.shape[1]:
        raise ValueError(f"out: expected [N, >= {c_off + c_out}] with contiguous rows, got {tuple(out.shape)}")
    check(_lib.load().pfpp_dgcnn_edge_max(_p(uv), ld, _p(idx), _p(scale.contiguous()), _p(shift.contiguous()), float(slope), N, c_out,
                                          K_NEIGHBOURS, _p(out, 4 * c_off), out.stride(0), ops._stream()), "pfpp_dgcnn_edge_max")
    return out


def leaky_relu_(x: torch.Tensor, slope: float = SLOPE) -> torch.Tensor:
    """x = x > 0 ? x : slope x in place; x float32 [rows, C] with contiguous rows"""
    _gpu(x, torch.float32, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"x: expected [rows, C] with contiguous rows, got {tuple(x.shape)}")
    check(_lib.load().pfpp_leaky_relu(_p(x), x.shape[0], x.shape[1], x.stride(0), float(slope), ops._stream()), "pfpp_leaky_relu")
    return x


# ------------------------------------------------------------------------------------------------------------------ the module
def _not_built(what: str) -> NotImplementedError:
    return NotImplementedError(f"{what} is not built: the DGCNN encoder here is DGCNNDynamic(global_feat=False) in eval mode, forward only")


class DGCNN(nn.Module):
    """the reference's dense DGCNN (dgcnn.py:59-127, arch string "dgcnn"): not built"""

    def __init__(self, *args, **kwargs):
        raise _not_built("the dense (non-dynamic) DGCNN encoder")


class DGCNNDynamic(nn.Module):
    """gemm_mode: arithmetic of the five products; only "f32" (exact fp32 matrix instructions).  The searches of levels 2 - 4 run on
    the products' results, and how often split-f16 products flip a near-tie between the 20th and 21st neighbour is unquantified."""

    def __init__(self, feat_dim: int, global_feat: bool = False, in_feat_dim: int = 3, gemm_mode: str = "f32"):
        super().__init__()
        if global_feat:
            raise _not_built("global_feat=True (the pooled per-piece feature and out_fc)")
        if gemm_mode == "f16x3":
            raise ValueError("gemm_mode='f16x3': refused for the DGCNN encoder (its neighbour searches run on the products' results and "
                             "near-tie flips under split-f16 keys are unquantified); use 'f32'")
        if gemm_mode != "f32":
            raise ValueError("gemm_mode: 'f32'")
        if in_feat_dim != 3:
            raise ValueError(f"in_feat_dim = {in_feat_dim}: the first search is built for rows of 3 channels")
        if feat_dim < 4 or feat_dim % 4:
            raise ValueError("feat_dim: a positive multiple of 4 (rows of the output are 16-byte aligned)")
        self.feat_dim, self.global_feat, self.in_feat_dim, self.gemm_mode = int(feat_dim), False, int(in_feat_dim), gemm_mode
        for l, c in enumerate(WIDTHS + (self.feat_dim,), 1):
            setattr(self, f"bn{l}", nn.BatchNorm1d(c))
        c_in = self.in_feat_dim
        for l, c in enumerate(WIDTHS, 1):
            setattr(self, f"conv{l}", nn.Sequential(nn.Conv1d(2 * c_in, c, kernel_size=1, bias=False), getattr(self, f"bn{l}"),
                                                    nn.LeakyReLU(negative_slope=SLOPE)))
            c_in = c
        self.conv5 = nn.Sequential(nn.Conv1d(CAT, self.feat_dim, kernel_size=1, bias=False), self.bn5, nn.LeakyReLU(negative_slope=SLOPE))
        self._pack, self._pack_key = None, None
        self.stage_events: Optional[list] = None       # set to a list to get (stage name, HIP event) pairs from the next forward
        super().train(False)

    def train(self, mode: bool = True):
        if mode:
            raise _not_built("training a DGCNN encoder (train-mode BatchNorm over all N x 20 rows and the backward)")
        return super().train(False)

    @classmethod
    def from_checkpoint(cls, path: str, **kw) -> "DGCNNDynamic":
        """the `encoder.*` entries of a Jigsaw checkpoint (a Lightning file with a `state_dict`, or a bare state_dict); the rest is
        ignored.  feat_dim is read from encoder.conv5.0.weight unless given."""
        from .matching import load_checkpoint_state_dict

        sd = load_checkpoint_state_dict(path)
        enc_sd = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
        if "feat_dim" not in kw:
            if "conv5.0.weight" not in enc_sd:
                raise KeyError(f"{path}: no encoder.conv5.0.weight (not a DGCNN checkpoint)")
            kw["feat_dim"] = int(enc_sd["conv5.0.weight"].shape[0])
        enc = cls(**kw)
        enc.load_state_dict(enc_sd, strict=True)
        return enc

    # -------------------------------------------------------------------------------------------------------------- packing
    def _packed(self) -> dict:
        """the split and folded weights; rebuilt when a parameter or buffer was written, replaced or moved since the last pack"""
        tensors = list(self.state_dict(keep_vars=True).values())
        key = tuple((t.data_ptr(), t._version, t.device) for t in tensors)
        if self._pack is None or key != self._pack_key:
            pack = {}
            with torch.no_grad():
                for l in range(1, 6):
                    conv, bn = getattr(self, f"conv{l}")[0], getattr(self, f"bn{l}")
                    w = conv.weight.detach().reshape(conv.weight.shape[0], -1)
                    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
                    shift = bn.bias.detach() - bn.running_mean * scale
                    if l < 5:                                         # [W_a | W_b] -> [W_a ; W_b - W_a], input columns padded to 4
                        c_in = w.shape[1] // 2
                        wa, wb = w[:, :c_in], w[:, c_in:]
                        w2 = torch.zeros((2 * w.shape[0], (c_in + 3) & ~3), dtype=torch.float32, device=w.device)
                        w2[:w.shape[0], :c_in] = wa
                        w2[w.shape[0]:, :c_in] = wb - wa
                        w = w2
                    pack[l] = (w.contiguous(), scale.contiguous(), shift.contiguous())
            self._pack, self._pack_key = pack, key
        return self._pack

    def _mark(self, name: str) -> None:
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    # -------------------------------------------------------------------------------------------------------------- forward
    @torch.no_grad()
    def conv5_forward(self, cat: torch.Tensor) -> torch.Tensor:
        """conv5 + bn5 + LeakyReLU of cat(x1 .. x4) float32 [N, 512]: the product with bn5 as the GEMM's scale / shift, then the
        LeakyReLU pass in place (the GEMM kernels have no such activation)"""
        _gpu(cat, torch.float32, "cat")
        if cat.dim() != 2 or cat.shape[1] != CAT or not cat.is_contiguous():
            raise ValueError(f"cat: expected contiguous float32 [N, {CAT}], got {tuple(cat.shape)}")
        w5, scale, shift = self._packed()[5]
        y = ops.gemm(cat, w5, M=cat.shape[0], N=self.feat_dim, K=CAT, lda=CAT, ldw=CAT, scale=scale, shift=shift, act="none", mode=self.gemm_mode)
        return leaky_relu_(y)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, batch_length, return_levels: bool = False):
        """x float32 [N_sum, 3] on the GPU; batch_length: the piece lengths (any number of puzzles, flat).  -> [N_sum, feat_dim];
        with return_levels also a dict: l{1..4}_knn int32 [N, 20] and l{1..4}_points (views of `cat` [N, 512])."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"x: must live on the GPU (got {getattr(x, 'device', type(x).__name__)}); there is no CPU path")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.in_feat_dim:
            raise ValueError(f"x: expected float32 [N_sum, {self.in_feat_dim}], got {x.dtype} {tuple(x.shape)}")
        if self.conv5[0].weight.device != x.device:
            raise ValueError(f"the module lives on {self.conv5[0].weight.device}, x on {x.device}")
        lengths = np.asarray(batch_length.detach().cpu().numpy() if torch.is_tensor(batch_length) else batch_length).astype(np.int64).reshape(-1)
        if lengths.size == 0 or (lengths < 1).any():
            raise ValueError("batch_length: every piece needs at least one point")
        if int(lengths.sum()) != x.shape[0]:
            raise ValueError(f"batch_length sums to {int(lengths.sum())} points, x has {x.shape[0]}")
        max_piece = int(lengths.max())
        if max_piece > MAX_PIECE:
            raise ValueError(f"a piece of {max_piece} points: the search kernel holds at most {MAX_PIECE}")
        dev, N = x.device, x.shape[0]
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
        pack = self._packed()
        x = x.contiguous()
        xp = torch.zeros((N, 4), dtype=torch.float32, device=dev)       # level 1's operand: three columns padded to four
        xp[:, :3] = x
        cat = torch.empty((N, CAT), dtype=torch.float32, device=dev)
        uv = torch.empty(N * 2 * WIDTHS[-1], dtype=torch.float32, device=dev)         # every level's [u | v], row stride 2 C_out
        idx_one = None if return_levels else torch.empty((N, K_NEIGHBOURS), dtype=torch.int32, device=dev)
        levels = {}
        self._mark("begin")
        for l, c_out in enumerate(WIDTHS):
            w2, scale, shift = pack[l + 1]
            if l == 0:
                idx = dgcnn_knn(x, off, max_piece, out=idx_one)
                a, a_off, lda, k = xp, 0, 4, self.in_feat_dim
            else:
                idx = dgcnn_knn(cat, off, max_piece, col=COL[l - 1], width=WIDTHS[l - 1], out=idx_one)
                a, a_off, lda, k = cat, COL[l - 1], CAT, WIDTHS[l - 1]
            self._mark(f"search{l + 1}")
            ops.gemm(a, w2, M=N, N=2 * c_out, K=k, lda=lda, ldw=w2.shape[1], a_off=a_off, out=uv, ldc=2 * c_out, mode=self.gemm_mode)
            self._mark(f"product{l + 1}")
            dgcnn_edge_max(uv, idx, scale, shift, c_out=c_out, ld=2 * c_out, out=cat, c_off=COL[l])
            self._mark(f"extremum{l + 1}")
            if return_levels:
                levels[f"l{l + 1}_knn"], levels[f"l{l + 1}_points"] = idx, cat[:, COL[l]:COL[l] + c_out]
        y = self.conv5_forward(cat)
        self._mark("conv5")
        if not return_levels:
            return y
        levels["cat"] = cat
        return y, levels
