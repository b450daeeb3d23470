"""The matcher's ragged PointNet++ encoder, forward only (csrc/pointnet_ragged.hip, include/pfpp.h "matcher front end").

PointNet2PTMSGDynamic of the reference's Jigsaw_matching/model/modules/encoder/pointnet2_pointwise/pointnet2_msg.py:48-94 with
its parameter names: points and piece lengths -> per-point descriptors [N_sum, 128].  Four set-abstraction levels sample every piece
by a ratio (farthest points), group the 16 / 32 nearest points OF THE SAME PIECE and run two MLPs with a max-pool; four
feature-propagation levels interpolate back from the 3 nearest centroids of the same piece.  Nothing depends on which puzzle a piece
belongs to, so one call takes the pieces of any number of puzzles flat (the reference asserts one puzzle per call).

Sampling and neighbour search depend on the coordinates only: one launch samples all four levels, eight launches find every
neighbourhood, and only then do the features move.  The MLPs run through ops.gemm (BatchNorm folded to scale / shift at pack time,
ReLU and the max-pool in the epilogue).  Eval mode only."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check

RATIOS = (0.15, 0.25, 0.25, 0.25)
NSAMPLE = (16, 32)
POOL = 32
MAX_PIECE = 8192


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def sample_count(n, ratio: float) -> np.ndarray:
    """samples torch_cluster.fps draws from a piece of n points: ceil(ratio n) with the product and the ceiling in float32 (its
    ratio tensor has the points' dtype), which is not exact arithmetic: n = 100, ratio 0.15 -> 16"""
    return np.ceil(np.float32(ratio) * np.asarray(n).astype(np.float32)).astype(np.int64)


def level_counts(lengths) -> np.ndarray:
    """int64 [5, P]: piece lengths at the input and behind each set-abstraction level"""
    out = [np.asarray(lengths, dtype=np.int64).reshape(-1)]
    for r in RATIOS:
        out.append(sample_count(out[-1], r))
    return np.stack(out)


def fold_batchnorm(conv_weight: torch.Tensor, conv_bias: torch.Tensor, bn) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """1x1 convolution followed by BatchNorm in eval mode -> (W [C_out, C_in], scale, shift) with bn(conv(x)) = (W x) scale + shift"""
    w = conv_weight.detach().reshape(conv_weight.shape[0], -1)
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    shift = (conv_bias.detach() - bn.running_mean) * scale + bn.bias.detach()
    return w, scale.contiguous(), shift.contiguous()


def _pad8(n: int) -> int:
    return (n + 7) & ~7


class _SetAbstraction(nn.Module):
    def __init__(self, in_channel: int, mlp_list):
        super().__init__()
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for widths in mlp_list:
            convs, bns, last = nn.ModuleList(), nn.ModuleList(), in_channel + 3
            for c in widths:
                convs.append(nn.Conv2d(last, c, 1))
                bns.append(nn.BatchNorm2d(c))
                last = c
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)
        self.out_channels = sum(w[-1] for w in mlp_list)


class _FeaturePropagation(nn.Module):
    def __init__(self, in_channel: int, mlp):
        super().__init__()
        self.mlp_convs, self.mlp_bns, last = nn.ModuleList(), nn.ModuleList(), in_channel
        for c in mlp:
            self.mlp_convs.append(nn.Conv1d(last, c, 1))
            self.mlp_bns.append(nn.BatchNorm1d(c))
            last = c
        self.in_channel, self.out_channels = in_channel, last


class _Layer:
    __slots__ = ("w", "scale", "shift", "K", "N")

    def __init__(self, w, scale, shift):
        N, K = w.shape
        self.w = torch.zeros((N, _pad8(K)), dtype=torch.float32, device=w.device)       # K padded to 8 with zeros, like the A operand
        self.w[:, :K] = w
        self.scale, self.shift, self.K, self.N = scale, shift, K, N


# ------------------------------------------------------------------------------------------------------------------ kernels
def ragged_fps(xyz: torch.Tensor, level_off: torch.Tensor, start: torch.Tensor, max_n: int, total: int):
    """xyz float32 [N, 3]; level_off int64 [L + 1, P + 1]; start int64 [L, P]; total = samples of all levels -> (idx int64 [total],
    new_xyz float32 [total, 3]), the levels one behind the other"""
    L, P = start.shape
    idx = torch.empty(total, dtype=torch.int64, device=xyz.device)
    new_xyz = torch.empty((total, 3), dtype=torch.float32, device=xyz.device)
    check(_lib.load().pfpp_ragged_fps(_p(xyz), _p(level_off), _p(start), P, L, int(max_n), _p(idx), _p(new_xyz), ops._stream()),
          "pfpp_ragged_fps")
    return idx, new_xyz


def ragged_knn(pts: torch.Tensor, pts_off: torch.Tensor, queries: torch.Tensor, query_off: torch.Tensor, K: int, want_count: bool = False):
    """-> idx int32 [M, K] (global indices into pts; the slots behind min(K, n_piece) repeat the first) and, if asked, the counts"""
    M, P = queries.shape[0], pts_off.numel() - 1
    idx = torch.empty((M, K), dtype=torch.int32, device=pts.device)
    cnt = torch.empty(M, dtype=torch.int32, device=pts.device) if want_count else None
    check(_lib.load().pfpp_ragged_knn(_p(pts), _p(pts_off), _p(queries), _p(query_off), P, M, pts.shape[0], K, _p(idx), _p(cnt),
                                      ops._stream()), "pfpp_ragged_knn")
    return (idx, cnt) if want_count else idx


def ragged_group(feats: torch.Tensor, xyz: torch.Tensor, new_xyz: torch.Tensor, idx: torch.Tensor, K: int, pool: int = POOL) -> torch.Tensor:
    """-> float32 [S pool, pad8(D + 3)]: row (s, j) = [feats[g] | xyz[g] - new_xyz[s] | 0], g = idx[s, j mod K]"""
    S, D = new_xyz.shape[0], feats.shape[1]
    out = torch.empty((S * pool, _pad8(D + 3)), dtype=torch.float32, device=xyz.device)
    check(_lib.load().pfpp_ragged_group(_p(feats), feats.stride(0), D, _p(xyz), _p(new_xyz), _p(idx), idx.stride(0), K, pool, S, _p(out),
                                        out.shape[1], ops._stream()), "pfpp_ragged_group")
    return out


def ragged_interp(xyz1: torch.Tensor, xyz2: torch.Tensor, idx: Optional[torch.Tensor], cnt: Optional[torch.Tensor], points2: torch.Tensor,
                  points1: Optional[torch.Tensor], want_weights: bool = False):
    """-> [N, D1 + D2] = [points1 | interpolated points2] (and the weights float32 [N, 3])"""
    N, S, D2 = xyz1.shape[0], xyz2.shape[0], points2.shape[1]
    D1 = 0 if points1 is None else points1.shape[1]
    out = torch.empty((N, D1 + D2), dtype=torch.float32, device=xyz1.device)
    w = torch.empty((N, 3), dtype=torch.float32, device=xyz1.device) if want_weights else None
    check(_lib.load().pfpp_ragged_interp(_p(xyz1), _p(xyz2), _p(idx), _p(cnt), _p(points2), D2, _p(points1), D1, N, S, _p(out), D1 + D2,
                                         _p(w), ops._stream()), "pfpp_ragged_interp")
    return (out, w) if want_weights else out


# ------------------------------------------------------------------------------------------------------------------ the module
class PointNet2PTMSGDynamic(nn.Module):
    """gemm_mode: arithmetic of the MLPs' products, "f32" (exact fp32 matrix instructions, the default) or "f16x3" (split-f16)"""

    def __init__(self, feat_in: int = 3, feat_out: int = 128, gemm_mode: str = "f32"):
        super().__init__()
        if feat_in < 3:
            raise ValueError("feat_in: the first three channels are the coordinates")
        if gemm_mode not in ("f32", "f16x3"):
            raise ValueError("gemm_mode: 'f32' or 'f16x3'")
        self.feat_in, self.feat_out, self.gemm_mode = feat_in, feat_out, gemm_mode
        self.sa1 = _SetAbstraction(feat_in, [[16, 16, 32], [32, 32, 64]])
        self.sa2 = _SetAbstraction(32 + 64, [[64, 64, 128], [64, 96, 128]])
        self.sa3 = _SetAbstraction(128 + 128, [[128, 196, 256], [128, 196, 256]])
        self.sa4 = _SetAbstraction(256 + 256, [[256, 256, 512], [256, 384, 512]])
        self.fp4 = _FeaturePropagation(512 + 512 + 256 + 256, [256, 256])
        self.fp3 = _FeaturePropagation(128 + 128 + 256, [256, 256])
        self.fp2 = _FeaturePropagation(32 + 64 + 256, [256, 128])
        self.fp1 = _FeaturePropagation(128, [128, 128, 128])
        self.conv1 = nn.Conv1d(128, feat_out, 1)
        self._pack, self._pack_key = None, None
        self.stage_events: Optional[list] = None       # set to a list to get (stage name, HIP event) pairs from the next forward
        super().train(False)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("PointNet2PTMSGDynamic runs in eval mode only: matcher training (train-mode BatchNorm and the "
                                      "backward of the ragged encoder) is not built")
        return super().train(False)

    @classmethod
    def from_checkpoint(cls, path: str, **kw) -> "PointNet2PTMSGDynamic":
        """the `encoder.*` entries of a Jigsaw checkpoint (a Lightning file with a `state_dict`, or a bare state_dict); the rest is ignored"""
        from .matching import load_checkpoint_state_dict

        sd = load_checkpoint_state_dict(path)
        enc = cls(**kw)
        enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=True)
        return enc

    # -------------------------------------------------------------------------------------------------------------- packing
    def _packed(self) -> dict:
        """the folded weights; rebuilt when a parameter or buffer was written, replaced or moved since the last pack"""
        tensors = list(self.state_dict(keep_vars=True).values())
        key = tuple((t.data_ptr(), t._version, t.device) for t in tensors)
        if self._pack is None or key != self._pack_key:
            pack = {}
            with torch.no_grad():
                for name in ("sa1", "sa2", "sa3", "sa4"):
                    sa = getattr(self, name)
                    pack[name] = [[_Layer(*fold_batchnorm(c.weight, c.bias, b)) for c, b in zip(convs, bns)]
                                  for convs, bns in zip(sa.conv_blocks, sa.bn_blocks)]
                for name in ("fp4", "fp3", "fp2", "fp1"):
                    fp = getattr(self, name)
                    pack[name] = [_Layer(*fold_batchnorm(c.weight, c.bias, b)) for c, b in zip(fp.mlp_convs, fp.mlp_bns)]
                w = self.conv1.weight.detach().reshape(self.feat_out, -1).contiguous()
                pack["conv1"] = (w, self.conv1.bias.detach().contiguous())
            self._pack, self._pack_key = pack, key
        return self._pack

    def _mlp(self, a: torch.Tensor, layers: Sequence[_Layer], *, pool: int = 0, out=None, ldc=None, c_off: int = 0) -> torch.Tensor:
        for j, ly in enumerate(layers):
            last = j + 1 == len(layers)
            a = ops.gemm(a, ly.w, M=a.shape[0], N=ly.N, K=ly.K, lda=a.shape[1], ldw=ly.w.shape[1], scale=ly.scale, shift=ly.shift, act="relu",
                         pool=pool if last else 0, out=out if last else None, ldc=ldc if last else None, c_off=c_off if last else 0,
                         mode=self.gemm_mode)
        return a

    def _mark(self, name: str) -> None:
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    # -------------------------------------------------------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, x: torch.Tensor, batch_length, start=None, return_levels: bool = False, seed: Optional[int] = None):
        """x float32 [N_sum, feat_in] (coordinates first) on the GPU; batch_length: the piece lengths (any number of puzzles, flat);
        start int [P, 4]: per piece and level the local index the sampling starts from (the reference draws it at random); with
        None it is drawn on the device from a generator seeded with `seed` (None: a fresh seed).  -> [N_sum, feat_out]; with
        return_levels also a dict of every level's indices and features."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"x: must live on the GPU (got {getattr(x, 'device', type(x).__name__)}); there is no CPU path")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.feat_in:
            raise ValueError(f"x: expected float32 [N_sum, {self.feat_in}], got {x.dtype} {tuple(x.shape)}")
        if self.conv1.weight.device != x.device:
            raise ValueError(f"the module lives on {self.conv1.weight.device}, x on {x.device}")
        lengths = np.asarray(batch_length.detach().cpu().numpy() if torch.is_tensor(batch_length) else batch_length).astype(np.int64).reshape(-1)
        if lengths.size == 0 or (lengths < 1).any():
            raise ValueError("batch_length: every piece needs at least one point")
        if int(lengths.sum()) != x.shape[0]:
            raise ValueError(f"batch_length sums to {int(lengths.sum())} points, x has {x.shape[0]}")
        if int(lengths.max()) > MAX_PIECE:
            raise ValueError(f"a piece of {int(lengths.max())} points: the sampling kernel holds at most {MAX_PIECE}")
        dev, P = x.device, lengths.size
        counts = level_counts(lengths)                                           # [5, P] (host: a pure function of the lengths)
        off_h = np.zeros((5, P + 1), dtype=np.int64)
        np.cumsum(counts, 1, out=off_h[:, 1:])
        totals = off_h[:, -1]
        off = torch.from_numpy(off_h).to(dev)
        if start is None:
            g = torch.Generator(device=dev)
            # no seed: one drawn from torch's default generator, so torch.manual_seed() makes the run repeatable as in the reference
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
        pack = self._packed()
        x = x.contiguous()
        xyz0 = x if self.feat_in == 3 else x[:, :3].contiguous()
        self._mark("begin")
        # ---- sampling: all four levels in one launch
        cen_all, xyz_all = ragged_fps(xyz0, off, st.contiguous(), int(lengths.max()), int(totals[1:].sum()))
        base = np.concatenate([[0], np.cumsum(totals[1:])])
        xyz = [xyz0] + [xyz_all[base[l]:base[l + 1]] for l in range(4)]
        cen = [cen_all[base[l]:base[l + 1]] for l in range(4)]
        self._mark("sampling")
        # ---- neighbours: the K = 16 neighbourhood is the head of the K = 32 one (both ascending); 3 nearest centroids for the way back
        nbr = [ragged_knn(xyz[l], off[l], xyz[l + 1], off[l + 1], NSAMPLE[1]) for l in range(4)]
        back = [ragged_knn(xyz[l + 1], off[l + 1], xyz[l], off[l], 3, want_count=True) if totals[l + 1] > 1 else (None, None) for l in range(4)]
        self._mark("neighbours")
        # ---- set abstraction
        feats = [x]
        for l, name in enumerate(("sa1", "sa2", "sa3", "sa4")):
            S = int(totals[l + 1])
            ctot = getattr(self, name).out_channels
            out = torch.empty((S, ctot), dtype=torch.float32, device=dev)
            c_off = 0
            for layers, K in zip(pack[name], NSAMPLE):
                a = ragged_group(feats[l], xyz[l], xyz[l + 1], nbr[l], K)
                self._mlp(a, layers, pool=POOL, out=out, ldc=ctot, c_off=c_off)
                c_off += layers[-1].N
            feats.append(out)
        self._mark("set_abstraction")
        # ---- feature propagation
        levels: Dict[str, torch.Tensor] = {}
        up = feats[4]
        for l, name in zip((3, 2, 1, 0), ("fp4", "fp3", "fp2", "fp1")):
            idx3, cnt3 = back[l]
            res = ragged_interp(xyz[l], xyz[l + 1], idx3, cnt3, up, feats[l] if l > 0 else None, want_weights=return_levels)
            a = res[0] if return_levels else res
            up = self._mlp(a, pack[name])
            if return_levels:
                levels[f"{name}_in"], levels[f"{name}_w"], levels[f"{name}_out"] = a, res[1], up
                levels[f"{name}_idx"], levels[f"{name}_cnt"] = idx3, cnt3
        w, b = pack["conv1"]
        y = ops.linear(up, w, b, mode=self.gemm_mode)
        self._mark("propagation")
        if not return_levels:
            return y
        for l in range(4):
            levels[f"l{l + 1}_centroids"], levels[f"l{l + 1}_xyz"], levels[f"l{l + 1}_points"] = cen[l], xyz[l + 1], feats[l + 1]
            levels[f"l{l + 1}_knn"] = nbr[l]
        levels["counts"], levels["start"] = torch.from_numpy(counts), st
        return y, levels

    def encode_puzzles(self, puzzles, start=None, seed: Optional[int] = None) -> List[torch.Tensor]:
        """several puzzles in one call: [(points float32 [N_b, feat_in], n_pcs int [P_b] (empty slots = 0)), ...] -> per-puzzle views
        [N_b, feat_out] of one result.  start: [sum of the pieces, 4] in the same order, or None."""
        if not puzzles:
            return []
        lengths, sizes = [], []
        for pts, n_pcs in puzzles:
            n = np.asarray(n_pcs.detach().cpu().numpy() if torch.is_tensor(n_pcs) else n_pcs).astype(np.int64).reshape(-1)
            n = n[n > 0]
            if int(n.sum()) != pts.shape[0]:
                raise ValueError(f"a puzzle of {pts.shape[0]} points whose n_pcs sums to {int(n.sum())}")
            lengths.append(n)
            sizes.append(int(pts.shape[0]))
        x = torch.cat([p for p, _ in puzzles], 0) if len(puzzles) > 1 else puzzles[0][0]
        y = self.forward(x, np.concatenate(lengths), start=start, seed=seed)
        return list(torch.split(y, sizes))
