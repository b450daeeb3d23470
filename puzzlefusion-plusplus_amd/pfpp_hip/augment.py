"""Batch augmentation on the GPU: the arithmetic of GeometryLatentDataset.__getitem__
(denoiser/dataset/dataset.py:165-215) for a whole batch in one kernel, fed by the dataset in `device_augment` mode."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib
from ._lib import check
from .ops import _chk, _ptr, _stream


def fragment_prepare(part_pcs_gt: torch.Tensor, num_parts: torch.Tensor, ref_idx: torch.Tensor, q_global: torch.Tensor,
                     q_part: torch.Tensor):
    """raw pfpp_fragment_prepare -> (part_pcs [B,P,N,3], part_trans [B,P,3], part_scale [B,P,1], init_pose_t [B,3])"""
    _chk(part_pcs_gt, torch.float32, "part_pcs_gt"); _chk(num_parts, torch.int32, "num_parts"); _chk(ref_idx, torch.int32, "ref_idx")
    _chk(q_global, torch.float32, "q_global"); _chk(q_part, torch.float32, "q_part")
    B, P, N, _ = part_pcs_gt.shape
    if q_global.shape != (B, 4) or q_part.shape != (B, P, 4) or num_parts.numel() != B or ref_idx.numel() != B:
        raise ValueError("fragment_prepare: q_global [B,4], q_part [B,P,4], num_parts [B], ref_idx [B] expected")
    dev = part_pcs_gt.device
    pcs = torch.empty_like(part_pcs_gt)
    trans = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
    scale = torch.empty((B, P, 1), dtype=torch.float32, device=dev)
    init_t = torch.empty((B, 3), dtype=torch.float32, device=dev)
    lib = _lib.load()
    ws = torch.empty((int(lib.pfpp_fragment_prepare_workspace(B, P)),), dtype=torch.uint8, device=dev)
    check(lib.pfpp_fragment_prepare(_ptr(part_pcs_gt), _ptr(num_parts), _ptr(ref_idx), _ptr(q_global), _ptr(q_part), _ptr(pcs),
                                    _ptr(trans), _ptr(scale), _ptr(init_t), B, P, N, _ptr(ws), _stream()), "pfpp_fragment_prepare")
    return pcs, trans, scale, init_t


def test_frames(part_pcs_gt: torch.Tensor, num_parts: torch.Tensor, ref_idx: torch.Tensor, q_global: torch.Tensor,
                q_part: torch.Tensor, by_area: torch.Tensor, pt_off: torch.Tensor, n_pcs: torch.Tensor):
    """raw pfpp_test_frames -> (part_pcs [B,P,N,3], part_trans [B,P,3], part_scale [B,P,1], init_pose_t [B,3], by_area_out [M,3]):
    fragment_prepare's four outputs, bit for bit, and the by-area points by_area [M,3] (the puzzles concatenated, pt_off int64 [B+1],
    n_pcs int32 [B,P] points per piece slot) in every piece's initial frame"""
    _chk(part_pcs_gt, torch.float32, "part_pcs_gt"); _chk(num_parts, torch.int32, "num_parts"); _chk(ref_idx, torch.int32, "ref_idx")
    _chk(q_global, torch.float32, "q_global"); _chk(q_part, torch.float32, "q_part"); _chk(by_area, torch.float32, "by_area")
    _chk(pt_off, torch.int64, "pt_off"); _chk(n_pcs, torch.int32, "n_pcs")
    B, P, N, _ = part_pcs_gt.shape
    if q_global.shape != (B, 4) or q_part.shape != (B, P, 4) or num_parts.numel() != B or ref_idx.numel() != B:
        raise ValueError("test_frames: q_global [B,4], q_part [B,P,4], num_parts [B], ref_idx [B] expected")
    if by_area.dim() != 2 or by_area.shape[1] != 3 or pt_off.shape != (B + 1,) or n_pcs.shape != (B, P):
        raise ValueError("test_frames: by_area [M,3], pt_off [B+1], n_pcs [B,P] expected")
    M = by_area.shape[0]
    dev = part_pcs_gt.device
    pcs = torch.empty_like(part_pcs_gt)
    trans = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
    scale = torch.empty((B, P, 1), dtype=torch.float32, device=dev)
    init_t = torch.empty((B, 3), dtype=torch.float32, device=dev)
    out = torch.empty_like(by_area)
    lib = _lib.load()
    ws = torch.empty((int(lib.pfpp_fragment_prepare_workspace(B, P)),), dtype=torch.uint8, device=dev)
    check(lib.pfpp_test_frames(_ptr(part_pcs_gt), _ptr(num_parts), _ptr(ref_idx), _ptr(q_global), _ptr(q_part), _ptr(pcs), _ptr(trans),
                               _ptr(scale), _ptr(init_t), _ptr(by_area), _ptr(pt_off), _ptr(n_pcs), _ptr(out), B, P, N, M, _ptr(ws),
                               _stream()), "pfpp_test_frames")
    return pcs, trans, scale, init_t, out


def random_unit_quaternions(shape, device, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """uniform on SO(3) (normalised Gaussian 4-vectors), like scipy's Rotation.random()"""
    q = torch.randn(*shape, 4, device=device, generator=generator)
    return q / q.norm(dim=-1, keepdim=True)


def _group_views(values, device):
    """one sample key of a whole group -> per sample what default_collate([value]) and a move to `device` make of it.  Arrays and
    numbers of one dtype go up in ONE copy (scalars stacked, arrays joined along their first axis, so ragged lengths are fine) and
    come back as views; anything else (strings, lists) is collated per sample.  -> (the views, the group's tensor or None)"""
    import numpy as np
    from torch.utils.data import default_collate

    plain = all(isinstance(v, (np.ndarray, np.generic, int, float, bool)) for v in values)
    arrs = [np.asarray(v) for v in values] if plain else []
    if not plain or len({(a.dtype, a.ndim, a.shape[1:]) for a in arrs}) != 1 or arrs[0].dtype.kind not in "biuf":
        move = lambda v: v.to(device) if torch.is_tensor(v) else [move(x) for x in v] if isinstance(v, list) else v
        return [move(default_collate([v])) for v in values], None
    if arrs[0].ndim == 0:
        whole = torch.from_numpy(np.stack(arrs)).to(device)
        return [whole[b:b + 1] for b in range(len(arrs))], whole
    whole = torch.from_numpy(np.concatenate(arrs, axis=0)).to(device)
    off = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrs])])
    return [whole[int(off[b]):int(off[b + 1])][None] for b in range(len(arrs))], whole


def test_frames_batch(samples, device, *, q_global=None, q_part=None, generator: Optional[torch.Generator] = None):
    """the test split's initial frames of a whole group in one pfpp_test_frames call.  `samples`: items as
    GeometryLatentDataset(..., "test", device_augment=True) returns them (stored geometry: padded part_pcs_gt [P,N,3], num_parts,
    ref_part, part_valids, ...; and the matching keys gt_pc_by_area [M,3], n_pcs [P], ...).  The rotations are drawn on the device,
    global first and then per part as augment_batch draws them, or given (q_global [B,4], q_part [B,P,4], the stored scalar-first
    quaternions).  -> one batch-of-one dict per sample for AutoAgglomerative.test_batch, views into the group's tensors: the keys,
    shapes and dtypes of assemble.as_batch_of_one(ds[i], device) on the host route, except that init_pose_r / init_pose_t are
    float32; matching_batch / matching_prepared travel as they are."""
    import numpy as np

    samples = list(samples)
    B = len(samples)
    if B == 0:
        return []
    gts = [np.asarray(s["part_pcs_gt"]) for s in samples]
    if any(g.ndim != 3 or g.shape != gts[0].shape or g.shape[2] != 3 for g in gts):
        raise ValueError(f"test_frames_batch: the puzzles of a group share P and N; part_pcs_gt shapes {sorted({g.shape for g in gts})}")
    P, N = gts[0].shape[:2]
    counts = np.zeros((B, P), dtype=np.int64)
    num_parts, ref_idx, lens = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int64)
    for b, s in enumerate(samples):
        did = s.get("data_id", b)
        n = np.asarray(s["n_pcs"]).reshape(-1)
        if n.size != P:
            raise ValueError(f"test_frames_batch: puzzle {did}: n_pcs has {n.size} slots, part_pcs_gt has {P}")
        pv = int(s["num_parts"])
        if not 1 <= pv <= P:
            raise ValueError(f"test_frames_batch: puzzle {did}: num_parts {pv} of {P} slots")
        pts = np.asarray(s["gt_pc_by_area"])
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f"test_frames_batch: puzzle {did}: gt_pc_by_area {pts.shape}, [M, 3] expected")
        if (n < 0).any() or int(n.sum()) != pts.shape[0]:
            raise ValueError(f"test_frames_batch: puzzle {did}: n_pcs sums to {int(n.sum())}, gt_pc_by_area holds {pts.shape[0]} points")
        if n[pv:].any():
            raise ValueError(f"test_frames_batch: puzzle {did}: n_pcs counts points in a slot >= num_parts ({pv})")
        ref = np.asarray(s["ref_part"]).reshape(-1).astype(bool)
        if ref.size != P or int(ref[:pv].sum()) != 1:
            raise ValueError(f"test_frames_batch: puzzle {did}: ref_part needs exactly one true entry among its {pv} valid slots")
        counts[b], num_parts[b], ref_idx[b], lens[b] = n, pv, int(np.argmax(ref[:pv])), pts.shape[0]
    pt_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if pt_off[-1] >= 1 << 31:
        raise ValueError(f"test_frames_batch: {int(pt_off[-1])} by-area points in one group (limit 2^31 - 1)")
    # the kernel's integer operands in one upload, the int64 offsets first so that their view is 8-byte aligned
    packed = torch.from_numpy(np.concatenate([pt_off.view(np.int32), num_parts, ref_idx, counts.astype(np.int32).reshape(-1)])).to(device)
    o = 2 * (B + 1)
    d_off, d_num, d_ref, d_cnt = packed[:o].view(torch.int64), packed[o:o + B], packed[o + B:o + 2 * B], packed[o + 2 * B:].view(B, P)
    keys = list(samples[0].keys())
    if any(set(s.keys()) != set(keys) for s in samples):
        raise ValueError("test_frames_batch: the samples of a group carry different keys")
    travel = ("matching_batch", "matching_prepared")
    views, wholes = {}, {}
    for k in keys:
        if k not in travel:
            views[k], wholes[k] = _group_views([s[k] for s in samples], device)
    # the two big arrays: the group's one upload each, as the dicts' views see it (cast only where a file holds another dtype)
    for k in ("part_pcs_gt", "gt_pc_by_area"):
        if wholes[k] is None:                              # the samples disagree on the dtype
            wholes[k] = torch.cat([v[0].float() for v in views[k]])
    gt = wholes["part_pcs_gt"].view(B, P, N, 3).float().contiguous()
    by_area = wholes["gt_pc_by_area"].float().contiguous()
    q_g = random_unit_quaternions((B,), device, generator).contiguous() if q_global is None else \
        torch.as_tensor(q_global).to(device=device, dtype=torch.float32).reshape(B, 4).contiguous()
    q_p = random_unit_quaternions((B, P), device, generator).contiguous() if q_part is None else \
        torch.as_tensor(q_part).to(device=device, dtype=torch.float32).reshape(B, P, 4).contiguous()
    pcs, trans, scale, init_t, frames = test_frames(gt, d_num.contiguous(), d_ref.contiguous(), q_g, q_p, by_area, d_off, d_cnt.contiguous())
    valid = torch.arange(P, device=device)[None, :] < d_num[:, None]
    rots = q_p * valid[..., None]
    out = []
    for b, s in enumerate(samples):
        a, e = int(pt_off[b]), int(pt_off[b + 1])
        d = {k: views[k][b] for k in views}
        d.update(part_pcs=pcs[b:b + 1], part_trans=trans[b:b + 1], part_scale=scale[b:b + 1], part_rots=rots[b:b + 1],
                 init_pose_r=q_g[b:b + 1], init_pose_t=init_t[b:b + 1], part_pcs_by_area=frames[a:e][None])
        d.update({k: s[k] for k in travel if k in s})
        out.append(d)
    return out


test_frames.__test__ = test_frames_batch.__test__ = False    # library functions, whatever a test module imports them as


def augment_batch(batch: Dict[str, torch.Tensor], device, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """collated `device_augment` samples (part_pcs_gt [B,P,N,3], part_valids, ref_part, num_parts, ...) -> the dict the
    Denoiser consumes, all on `device`"""
    gt = batch["part_pcs_gt"].to(device).float().contiguous()
    B, P = gt.shape[:2]
    num_parts = batch["num_parts"].to(device).to(torch.int32).contiguous()
    ref_part = batch["ref_part"].to(device).bool()
    ref_idx = ref_part.float().argmax(dim=1).to(torch.int32).contiguous()
    q_g = random_unit_quaternions((B,), device, generator).contiguous()
    q_p = random_unit_quaternions((B, P), device, generator).contiguous()
    pcs, trans, scale, init_t = fragment_prepare(gt, num_parts, ref_idx, q_g, q_p)
    valid = (torch.arange(P, device=device)[None, :] < num_parts[:, None])
    out = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    out.update(part_pcs=pcs, part_trans=trans, part_scale=scale, part_rots=q_p * valid[..., None], init_pose_r=q_g,
               init_pose_t=init_t, part_valids=batch["part_valids"].to(device).float(), ref_part=ref_part)
    return out
