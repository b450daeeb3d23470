"""Fracture meshes -> pc_data on the GPU: the per-puzzle work of the reference's vqvae/dataset/dataset.py:GeometryPartDataset
(_get_pcs :154-181, __getitem__ :183-226) over a batch of puzzles (csrc/mesh_sample.hip, include/pfpp.h "pc_data generation").

* read_obj: the OBJ reader (numpy, no per-vertex Python loop).  trimesh.load also merges vertices closer than 1e-8 and does other
  processing; this reader keeps the positions as written and only the referenced vertices (the documented deviation).
* pack: a CSR batch of the puzzles' parts, one pinned host buffer per array and one copy of each to the device.
* face_cdf / sample_surface / vertex_graph: wrappers over the kernels; every failure the kernels record is raised here.
* pc_data_batch: one dict per puzzle with exactly io.PC_DATA_KEYS and the reference's dtypes.
* rng_uniforms: the host restatement of the generated uniforms (pfpp_rng_u64), bit for bit.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from .io import PC_DATA_KEYS

# --------------------------------------------------------------------------------------------------------------- OBJ reader
_REC = re.compile(rb"^([vf])[ \t]+([^\r\n#]*)", re.M)


def _records(rests: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """tokens of a list of record bodies -> (tokens [T], line of each token [T], tokens per line [L])"""
    if rests.size == 0:
        return np.zeros(0, dtype=bytes), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    toks = np.array(b" | ".join(rests).split() + [b"|"])
    sep = toks == b"|"
    line = np.cumsum(sep)[~sep]
    counts = np.bincount(line, minlength=rests.size)
    return toks[~sep], line, counts


def read_obj(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> (vertices float64 [V, 3], faces int32 [F, 3]).  `v` and `f` records only; face tokens i, i/j, i//k or i/j/k, negative
    indices relative to the vertices read so far; polygons fan-triangulated as (0, i, i + 1); unreferenced vertices dropped and
    the faces remapped."""
    with open(path, "rb") as fh:
        data = fh.read()
    recs = np.array(_REC.findall(data), dtype=bytes).reshape(-1, 2)
    is_v = recs[:, 0] == b"v"
    # vertices: the first three numbers of every v record
    vt, vline, vcount = _records(recs[is_v, 1])
    if (vcount < 3).any():
        raise ValueError(f"{path}: a v record with fewer than three coordinates")
    start = np.concatenate([[0], np.cumsum(vcount)[:-1]])
    pos = np.arange(vt.size) - start[vline]
    try:
        verts = vt[pos < 3].astype(np.float64).reshape(-1, 3)
    except ValueError as e:
        raise ValueError(f"{path}: unreadable vertex coordinate ({e})") from None
    nv_before = np.cumsum(is_v)[~is_v]                    # vertices defined before each f record
    ft, fline, fcount = _records(recs[~is_v, 1])
    if (fcount < 3).any():
        raise ValueError(f"{path}: a face with fewer than three vertices")
    try:
        idx = np.char.partition(ft, b"/")[:, 0].astype(np.int64)
    except ValueError as e:
        raise ValueError(f"{path}: unreadable face index ({e})") from None
    if (idx == 0).any():
        raise ValueError(f"{path}: face index 0 (OBJ indices start at 1)")
    idx = np.where(idx > 0, idx - 1, nv_before[fline] + idx)
    if idx.size and (idx.min() < 0 or idx.max() >= len(verts)):
        raise ValueError(f"{path}: face index outside the {len(verts)} vertices")
    # fan triangulation (0, i, i + 1) of every polygon
    ntri = fcount - 2
    fstart = np.concatenate([[0], np.cumsum(fcount)[:-1]])
    tline = np.repeat(np.arange(fcount.size), ntri)
    k = np.arange(tline.size) - np.repeat(np.cumsum(ntri) - ntri, ntri) + 1
    a = fstart[tline]
    tri = np.stack([idx[a], idx[a + k], idx[a + k + 1]], axis=1)
    used = np.unique(tri)
    remap = np.full(len(verts), -1, dtype=np.int64)
    remap[used] = np.arange(used.size)
    return np.ascontiguousarray(verts[used]), remap[tri].astype(np.int32).reshape(-1, 3)


# --------------------------------------------------------------------------------------------------------------- batch packing
@dataclass
class MeshBatch:
    """CSR batch of the parts of B puzzles on the device (include/pfpp.h "pc_data generation")"""

    verts: torch.Tensor          # float64 [V, 3]
    faces: torch.Tensor          # int32 [F, 3], part-local
    vert_off: torch.Tensor       # int64 [Pt + 1]
    face_off: torch.Tensor       # int64 [Pt + 1]
    part_puzzle: torch.Tensor    # int32 [Pt]
    part_slot: torch.Tensor      # int32 [Pt]
    puz_part_off: torch.Tensor   # int64 [B + 1]
    data_id: torch.Tensor        # int64 [B]
    tab_off: torch.Tensor        # int64 [B + 1], hash table regions of the vertex graph
    num_parts: List[int]
    table_slots: int
    graph_ws_bytes: int

    @property
    def B(self) -> int:
        return len(self.num_parts)

    @property
    def Pt(self) -> int:
        return int(self.part_slot.numel())


def _pinned(a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory() if torch.cuda.is_available() else t


def pack(puzzles: Sequence[Sequence[Tuple[np.ndarray, np.ndarray]]], data_ids: Sequence[int], device) -> MeshBatch:
    """puzzles[b] = list of (vertices [V, 3], faces [F, 3]) in slot order -> MeshBatch on `device`"""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"pack: device must be a GPU (got {device}); there is no CPU path")
    parts = [p for pz in puzzles for p in pz]
    nparts = [len(pz) for pz in puzzles]
    if len(data_ids) != len(puzzles):
        raise ValueError("pack: one data_id per puzzle")
    nv = np.array([len(v) for v, _ in parts], dtype=np.int64)
    nf = np.array([len(f) for _, f in parts], dtype=np.int64)
    vert_off = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
    face_off = np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)
    for (v, f), n in zip(parts, nv):
        if f.size and (f.min() < 0 or f.max() >= n):
            raise ValueError("pack: face index outside its part")
    verts = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 3) for v, _ in parts]) if parts else np.zeros((0, 3))
    faces = np.concatenate([np.asarray(f, dtype=np.int32).reshape(-1, 3) for _, f in parts]) if parts else np.zeros((0, 3), np.int32)
    part_puzzle = np.repeat(np.arange(len(puzzles), dtype=np.int32), nparts)
    part_slot = np.concatenate([np.arange(n, dtype=np.int32) for n in nparts]) if parts else np.zeros(0, np.int32)
    puz_part_off = np.concatenate([[0], np.cumsum(nparts)]).astype(np.int64)
    puz_nv = vert_off[puz_part_off[1:]] - vert_off[puz_part_off[:-1]]
    tab_off = np.zeros(len(puzzles) + 1, dtype=np.int64)
    lib = _lib.load()
    ws = lib.pfpp_mesh_vertex_graph_workspace(puz_nv.ctypes.data_as(C.c_void_p), len(puzzles), tab_off.ctypes.data_as(C.c_void_p))
    if ws < 0:
        raise ValueError("pack: bad vertex counts")

    def up(a):
        return _pinned(a).to(device, non_blocking=True)

    return MeshBatch(verts=up(verts), faces=up(faces), vert_off=up(vert_off), face_off=up(face_off), part_puzzle=up(part_puzzle),
                     part_slot=up(part_slot), puz_part_off=up(puz_part_off), data_id=up(np.asarray(data_ids, dtype=np.int64)),
                     tab_off=up(tab_off), num_parts=list(nparts), table_slots=int(tab_off[-1]), graph_ws_bytes=int(ws))


# --------------------------------------------------------------------------------------------------------------- wrappers
def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream(dev: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_batch(mb: MeshBatch) -> None:
    for name in ("verts", "faces", "vert_off", "face_off", "part_puzzle", "part_slot", "puz_part_off", "data_id", "tab_off"):
        t = getattr(mb, name)
        if not t.is_cuda:
            raise ValueError(f"{name}: must live on the GPU (got {t.device}); there is no CPU path")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")


def new_status(dev) -> torch.Tensor:
    """the device status word of the mesh kernels (all ones = no failure)"""
    return torch.full((1,), -1, dtype=torch.int64, device=dev)


def check_status(status: torch.Tensor) -> None:
    """raise the first failure the mesh kernels recorded (waits for the current stream)"""
    check(_lib.load().pfpp_mesh_status(_p(status), _stream(status.device)), "pfpp_mesh_status")


def face_cdf(mb: MeshBatch, status: Optional[torch.Tensor] = None):
    """-> (area [F], cdf [F], total [Pt]) float64.  Without a status word of the caller's, failures are raised here."""
    _check_batch(mb)
    dev = mb.verts.device
    own = status is None
    status = new_status(dev) if own else status
    F = mb.faces.shape[0]
    area = torch.empty(F, dtype=torch.float64, device=dev)
    cdf = torch.empty(F, dtype=torch.float64, device=dev)
    total = torch.empty(mb.Pt, dtype=torch.float64, device=dev)
    check(_lib.load().pfpp_mesh_face_cdf(_p(mb.verts), _p(mb.faces), _p(mb.vert_off), _p(mb.face_off), mb.Pt, _p(area), _p(cdf),
                                         _p(total), _p(status), _stream(dev)), "pfpp_mesh_face_cdf")
    if own:
        check_status(status)
    return area, cdf, total


def sample_surface(mb: MeshBatch, num_points: int, cdf: torch.Tensor, total: torch.Tensor, *, uniforms: Optional[torch.Tensor] = None,
                   seed: int = 0, split: int = 0, max_parts: int = 20):
    """-> (points float64 [Pt, N, 3], face int32 [Pt, N], scale float64 [Pt], ref_slot int32 [B]).  uniforms: float64 [Pt, N, 3] =
    (u0, l0, l1) per sample, or None for the generator keyed by (seed, split, data_id, slot, sample)"""
    _check_batch(mb)
    dev = mb.verts.device
    for name, t in (("cdf", cdf), ("total", total)) + ((("uniforms", uniforms),) if uniforms is not None else ()):
        if not t.is_cuda:
            raise ValueError(f"{name}: must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"{name}: contiguous float64 expected")
    if uniforms is not None and tuple(uniforms.shape) != (mb.Pt, num_points, 3):
        raise ValueError(f"uniforms: shape {tuple(uniforms.shape)}, expected {(mb.Pt, num_points, 3)}")
    if not 0 <= seed < 2 ** 64 or not 0 <= split < 2 ** 32:
        raise ValueError("seed must fit 64 bits and split 32 bits")
    pts = torch.empty((mb.Pt, num_points, 3), dtype=torch.float64, device=dev)
    face = torch.empty((mb.Pt, num_points), dtype=torch.int32, device=dev)
    scale = torch.empty(mb.Pt, dtype=torch.float64, device=dev)
    ref = torch.empty(mb.B, dtype=torch.int32, device=dev)
    check(_lib.load().pfpp_mesh_sample_surface(
        _p(mb.verts), _p(mb.faces), _p(mb.vert_off), _p(mb.face_off), _p(cdf), _p(total), _p(mb.part_puzzle), _p(mb.part_slot),
        _p(mb.data_id), _p(mb.puz_part_off), mb.Pt, mb.B, num_points, _p(uniforms), seed, split, max_parts, _p(pts), _p(face),
        _p(scale), _p(ref), _stream(dev)), "pfpp_mesh_sample_surface")
    return pts, face, scale, ref


def vertex_graph(mb: MeshBatch, max_num_part: int = 20, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> bool [B, max_num_part, max_num_part]: _check_connectivity of every puzzle"""
    _check_batch(mb)
    dev = mb.verts.device
    if max(mb.num_parts, default=0) > max_num_part:
        raise ValueError(f"a puzzle has more than max_num_part = {max_num_part} parts")
    own = status is None
    status = new_status(dev) if own else status
    graph = torch.empty((mb.B, max_num_part, max_num_part), dtype=torch.bool, device=dev)
    ws = torch.empty(max(mb.graph_ws_bytes, 1), dtype=torch.uint8, device=dev)
    check(_lib.load().pfpp_mesh_vertex_graph(
        _p(mb.verts), _p(mb.vert_off), _p(mb.part_puzzle), _p(mb.part_slot), _p(mb.puz_part_off), _p(mb.tab_off), mb.Pt, mb.B,
        mb.verts.shape[0], mb.table_slots, max_num_part, _p(graph), _p(ws), ws.numel(), _p(status), _stream(dev)), "pfpp_mesh_vertex_graph")
    if own:
        check_status(status)
    return graph


def rng_uniforms(seed: int, split: int, data_id: int, slot: int, num_points: int, max_parts: int = 20) -> np.ndarray:
    """host restatement of the generated uniforms of one part: float64 [N, 3] (pfpp_rng_u64 of csrc/pfpp_common.h)"""
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        idx = ((np.uint64(data_id) * np.uint64(max_parts) + np.uint64(slot)) * np.uint64(num_points)
               + np.arange(num_points, dtype=np.uint64))[:, None] * np.uint64(3) + np.arange(3, dtype=np.uint64)[None]
        z = np.full(idx.shape, np.uint64(seed) ^ ((np.uint64(split) * np.uint64(0xD6E8FEB86659FD93)) & M), dtype=np.uint64)
        z = z + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# --------------------------------------------------------------------------------------------------------------- pc_data
def pc_data_batch(puzzles: Sequence[Dict], *, num_points: int = 1000, max_num_part: int = 20, seed: int = 0, split: int = 0,
                  uniforms: Optional[Callable[[Dict], np.ndarray]] = None, device="cuda") -> List[Dict[str, object]]:
    """puzzles: dicts with data_id, mesh_file_path, category and meshes (list of (vertices, faces) in slot order) -> one dict per
    puzzle with exactly io.PC_DATA_KEYS: data_id int, part_valids float32 [max_num_part], num_parts int, mesh_file_path str,
    graph bool [max_num_part, max_num_part], category str, part_pcs_gt float64 [Pv, N, 3], ref_part bool [max_num_part].
    uniforms (test hook): puzzle dict -> float64 [Pv, N, 3] given uniforms instead of the generator."""
    if not puzzles:
        return []
    mb = pack([pz["meshes"] for pz in puzzles], [int(pz["data_id"]) for pz in puzzles], device)
    dev = mb.verts.device
    status = new_status(dev)
    graph = vertex_graph(mb, max_num_part, status=status)
    _, cdf, total = face_cdf(mb, status=status)
    u = None
    if uniforms is not None:
        u = torch.from_numpy(np.concatenate([np.asarray(uniforms(pz), dtype=np.float64) for pz in puzzles])).to(dev)
    pts, _, _, ref = sample_surface(mb, num_points, cdf, total, uniforms=u, seed=seed, split=split, max_parts=max_num_part)
    try:
        check_status(status)
    except _lib.PfppError as e:
        m = re.search(r"(part|puzzle) (\d+)", str(e))
        if m:
            i = int(m.group(2))
            b = int(np.searchsorted(np.cumsum(mb.num_parts), i, side="right")) if m.group(1) == "part" else i
            raise _lib.PfppError(f"{puzzles[b]['mesh_file_path']}: {e}") from None
        raise
    pts_h, graph_h, ref_h = pts.cpu().numpy(), graph.cpu().numpy(), ref.cpu().numpy()
    out, p0 = [], 0
    for b, pz in enumerate(puzzles):
        n = mb.num_parts[b]
        valids = np.zeros(max_num_part, dtype=np.float32)
        valids[:n] = 1.0
        ref_part = np.zeros(max_num_part, dtype=bool)
        ref_part[int(ref_h[b])] = True
        d = {"data_id": int(pz["data_id"]), "part_valids": valids, "num_parts": n, "mesh_file_path": str(pz["mesh_file_path"]),
             "graph": graph_h[b], "category": str(pz["category"]), "part_pcs_gt": pts_h[p0:p0 + n], "ref_part": ref_part}
        assert tuple(d) == PC_DATA_KEYS
        out.append(d)
        p0 += n
    return out
