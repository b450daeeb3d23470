"""The matcher's dataset on one GPU: fracture meshes -> the batches of Jigsaw_matching/dataset/all_piece_matching_dataset.py
(AllPieceMatchingDataset, build_all_piece_matching_dataloader), csrc/matching_dataset.hip, include/pfpp.h "the matcher's training
batches".

The reference re-reads and re-samples every mesh on every item of every epoch; the OBJ parse is by far the larger half of that
(DESIGN.md 5.3).  Here the meshes of a split are parsed once (a process pool, or a saved .npz) into a MeshStore that stays on the
device, and a batch is three kernel launches over a selection of the store's puzzles: piece counts, ragged surface samples, pose.

* MeshStore: the CSR arrays of pfpp_hip.meshes.MeshBatch for a whole split plus cdf / total of one face_cdf call.
* sample_batch: the kernels over a selection; given uniforms / orders / rotations (the parity path) or generated ones.
* AllPieceMatchingDataset: the reference's constructor arguments; batch(indices, epoch) returns its data_dict batched, on the
  device; batches() walks the split.  A puzzle's arrays depend on (seed, split, epoch, data_id) only.
* quat_from_matrix / euler_xyz_matrix: host restatements of scipy's Rotation.from_matrix(m).as_quat() and from_euler("xyz").

Deviations from the reference: the generated mode draws no permutation of a piece's points (its samples are independent and
identically distributed, so their order already is a uniformly random one; `order` exists for parity with _shuffle_pc only); the
random draws are counter-based and seeded instead of the global unseeded generators; shuffle_parts with length shuffles the data
list with the seed; trimesh's 1e-8 vertex merge is not done (pfpp_hip.meshes.read_obj)."""
from __future__ import annotations

import os
import pickle
import types
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, meshes
from ._lib import check as _check
from .meshes import MeshBatch, _p, _stream

SPLITS = {"train": 0, "val": 1}
MAX_WORKERS = 16          # the parse pool is never sized by the machine's CPU count
DATA_DICT_KEYS = ("part_pcs", "gt_pcs", "part_valids", "part_quat", "part_trans", "n_pcs", "data_id", "critical_label_thresholds",
                  "mesh_file_path", "num_parts")
POINT_FILE_KEYS = ("part_pcs", "gt_pcs", "n_pcs", "part_valids", "part_quat", "part_trans")


def split_word(split, epoch: int = 0) -> int:
    """the 32-bit `split` argument of the kernels: (epoch << 1) | (0 train, 1 val)"""
    s = SPLITS[split] if isinstance(split, str) else int(split)
    if s not in (0, 1) or not 0 <= int(epoch) < 2 ** 31:
        raise ValueError("split is 'train' / 'val' (0 / 1) and 0 <= epoch < 2^31")
    return (int(epoch) << 1) | s


# --------------------------------------------------------------------------------------------------------------- rotations (host)
def quat_from_matrix(m: np.ndarray) -> np.ndarray:
    """scipy's Rotation.from_matrix(m).as_quat() restated, scalar-first (w, x, y, z), the sign as scipy leaves it: float64
    [..., 3, 3] -> [..., 4].  The matrices are taken as rotations (scipy orthogonalises others; these are never others)."""
    m = np.asarray(m, dtype=np.float64)
    flat = m.reshape(-1, 3, 3)
    out = np.empty((flat.shape[0], 4), dtype=np.float64)          # scipy's order: x, y, z, w
    for n, a in enumerate(flat):
        dec = np.array([a[0, 0], a[1, 1], a[2, 2], a[0, 0] + a[1, 1] + a[2, 2]])
        ch = int(np.argmax(dec))
        q = out[n]
        if ch != 3:
            i = ch
            j = (i + 1) % 3
            k = (j + 1) % 3
            q[i] = 1 - dec[3] + 2 * a[i, i]
            q[j] = a[j, i] + a[i, j]
            q[k] = a[k, i] + a[i, k]
            q[3] = a[k, j] - a[j, k]
        else:
            q[0] = a[2, 1] - a[1, 2]
            q[1] = a[0, 2] - a[2, 0]
            q[2] = a[1, 0] - a[0, 1]
            q[3] = 1 + dec[3]
        q /= np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return out[:, [3, 0, 1, 2]].reshape(m.shape[:-2] + (4,))


def euler_xyz_matrix(deg: np.ndarray) -> np.ndarray:
    """Rotation.from_euler("xyz", deg, degrees=True).as_matrix(): extrinsic x, y, z = Rz Ry Rx; float64 [..., 3] -> [..., 3, 3]"""
    a = np.deg2rad(np.asarray(deg, dtype=np.float64))
    cx, cy, cz = np.cos(a[..., 0]), np.cos(a[..., 1]), np.cos(a[..., 2])
    sx, sy, sz = np.sin(a[..., 0]), np.sin(a[..., 1]), np.sin(a[..., 2])
    r = np.empty(a.shape[:-1] + (3, 3), dtype=np.float64)
    r[..., 0, 0], r[..., 0, 1], r[..., 0, 2] = cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx
    r[..., 1, 0], r[..., 1, 1], r[..., 1, 2] = sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx
    r[..., 2, 0], r[..., 2, 1], r[..., 2, 2] = -sy, cy * sx, cy * cx
    return r


# --------------------------------------------------------------------------------------------------------------- discovery
def read_data_list(data_dir: str, data_fn: str, category: str = "", min_num_part: int = 2, max_num_part: int = 20) -> List[str]:
    """_read_data (:77-115): the reference's metadata pickle when it exists (read, never written), else the rules of
    puzzlefusion_plusplus.vqvae.dataset.dataset.GeometryPartDataset._read_data, which are the same"""
    from puzzlefusion_plusplus.vqvae.dataset.dataset import GeometryPartDataset

    meta = os.path.join(data_dir, f"all_piece_matching_metadata_{min_num_part}_{max_num_part}_" + data_fn)
    if os.path.exists(meta):
        with open(meta, "rb") as fh:
            return list(pickle.load(fh)["data_list"])
    rules = types.SimpleNamespace(data_dir=data_dir, category=category, min_num_part=min_num_part, max_num_part=max_num_part)
    return GeometryPartDataset._read_data(rules, data_fn)


def parse_puzzle(folder: str) -> List[Tuple[np.ndarray, np.ndarray]]:
    """the piece meshes of one fracture folder, file names in sorted order (_get_pcs :198-208)"""
    names = sorted(os.listdir(folder))
    parts = []
    for name in names:
        path = os.path.join(folder, name)
        try:
            parts.append(meshes.read_obj(path))
        except (OSError, ValueError) as e:
            raise ValueError(f"cannot read mesh {path}: {e}") from None
    return parts


# --------------------------------------------------------------------------------------------------------------- the resident store
class MeshStore:
    """the meshes of a whole split: host CSR arrays, their device copies (a MeshBatch) and cdf / total of one face_cdf call"""

    HOST_KEYS = ("verts", "faces", "vert_off", "face_off", "puz_part_off", "data_id")

    def __init__(self, host: Dict[str, np.ndarray], paths: Sequence[str], device="cuda", check_areas: bool = True):
        self.host = {"verts": np.ascontiguousarray(host["verts"], dtype=np.float64).reshape(-1, 3),
                     "faces": np.ascontiguousarray(host["faces"], dtype=np.int32).reshape(-1, 3),
                     "vert_off": np.ascontiguousarray(host["vert_off"], dtype=np.int64),
                     "face_off": np.ascontiguousarray(host["face_off"], dtype=np.int64),
                     "puz_part_off": np.ascontiguousarray(host["puz_part_off"], dtype=np.int64),
                     "data_id": np.ascontiguousarray(host["data_id"], dtype=np.int64)}
        h = self.host
        self.paths = [str(p) for p in paths]
        self.num_parts = np.diff(h["puz_part_off"])
        S, Pt = len(self.num_parts), len(h["vert_off"]) - 1
        if (len(self.paths) != S or len(h["data_id"]) != S or len(h["face_off"]) != Pt + 1 or S and h["puz_part_off"][-1] != Pt
                or h["puz_part_off"][0] != 0 or (self.num_parts < 1).any() or h["vert_off"][0] != 0 or h["face_off"][0] != 0
                or h["vert_off"][-1] != len(h["verts"]) or h["face_off"][-1] != len(h["faces"])
                or (np.diff(h["vert_off"]) < 0).any() or (np.diff(h["face_off"]) < 0).any()):
            raise ValueError("MeshStore: inconsistent CSR arrays")
        nv = np.repeat(np.diff(h["vert_off"]), np.diff(h["face_off"]))
        if len(h["faces"]) and ((h["faces"] < 0).any() or (h["faces"] >= nv[:, None]).any()):
            raise ValueError("MeshStore: face index outside its part")
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(a).to(self.device)        # noqa: E731
        part_puzzle = np.repeat(np.arange(S, dtype=np.int32), self.num_parts)
        part_slot = (np.arange(Pt, dtype=np.int64) - np.repeat(h["puz_part_off"][:-1], self.num_parts)).astype(np.int32)
        self.batch = MeshBatch(verts=up(h["verts"]), faces=up(h["faces"]), vert_off=up(h["vert_off"]), face_off=up(h["face_off"]),
                               part_puzzle=up(part_puzzle), part_slot=up(part_slot), puz_part_off=up(h["puz_part_off"]),
                               data_id=up(h["data_id"]), tab_off=torch.zeros(S + 1, dtype=torch.int64, device=self.device),
                               num_parts=[int(n) for n in self.num_parts], table_slots=0, graph_ws_bytes=0)
        self.cdf = self.total = None
        if self.device.type == "cuda":          # a store on the CPU can be saved and inspected; sample_batch refuses it
            status = meshes.new_status(self.device)
            _, self.cdf, self.total = meshes.face_cdf(self.batch, status=status)
            if check_areas:
                self._raise_status(status)

    def _raise_status(self, status: torch.Tensor) -> None:
        import re

        try:
            meshes.check_status(status)
        except _lib.PfppError as e:
            m = re.search(r": part (\d+)", str(e))
            if m:
                b = int(np.searchsorted(self.host["puz_part_off"], int(m.group(1)), side="right")) - 1
                raise _lib.PfppError(f"{self.paths[b]}: {e}") from None
            raise

    def __len__(self) -> int:
        return len(self.num_parts)

    @property
    def device_bytes(self) -> int:
        ts = [getattr(self.batch, k) for k in ("verts", "faces", "vert_off", "face_off", "part_puzzle", "part_slot", "puz_part_off",
                                                "data_id", "tab_off")] + [t for t in (self.cdf, self.total) if t is not None]
        return int(sum(t.numel() * t.element_size() for t in ts))

    @classmethod
    def from_meshes(cls, puzzles: Sequence[Sequence[Tuple[np.ndarray, np.ndarray]]], data_ids: Sequence[int], paths: Sequence[str],
                    device="cuda", check_areas: bool = True) -> "MeshStore":
        parts = [p for pz in puzzles for p in pz]
        nparts = [len(pz) for pz in puzzles]
        host = {"verts": np.concatenate([np.asarray(v, np.float64).reshape(-1, 3) for v, _ in parts]) if parts else np.zeros((0, 3)),
                "faces": np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in parts]) if parts else np.zeros((0, 3), np.int32),
                "vert_off": np.concatenate([[0], np.cumsum([len(v) for v, _ in parts])]),
                "face_off": np.concatenate([[0], np.cumsum([len(f) for _, f in parts])]),
                "puz_part_off": np.concatenate([[0], np.cumsum(nparts)]), "data_id": np.asarray(data_ids, dtype=np.int64)}
        return cls(host, paths, device, check_areas)

    @classmethod
    def build(cls, data_dir: str, data_list: Sequence[str], device="cuda", workers: Optional[int] = None) -> "MeshStore":
        """parse every folder of data_list (data_id = its index) with a pool of at most 16 processes; workers = 0 parses here"""
        folders = [os.path.join(data_dir, rel) for rel in data_list]
        n = min(MAX_WORKERS, len(folders)) if workers is None else min(MAX_WORKERS, int(workers))
        if n <= 1:
            puzzles = [parse_puzzle(f) for f in folders]
        else:
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor

            # fresh interpreters: a forked child of a process that has initialised the GPU must not touch it, and does not here
            with ProcessPoolExecutor(n, mp_context=mp.get_context("spawn")) as pool:
                puzzles = list(pool.map(parse_puzzle, folders, chunksize=max(1, len(folders) // (4 * n))))
        return cls.from_meshes(puzzles, list(range(len(folders))), list(data_list), device)

    def save(self, path: str) -> None:
        np.savez(path, paths=np.array(self.paths, dtype=str), **self.host)

    @classmethod
    def load(cls, path: str, device="cuda") -> "MeshStore":
        with np.load(path, allow_pickle=False) as d:
            return cls({k: d[k] for k in cls.HOST_KEYS}, [str(p) for p in d["paths"]], device)


# --------------------------------------------------------------------------------------------------------------- a batch
def _table(t, dtype, shape, name: str, dev) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = torch.as_tensor(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {t.dtype} {tuple(t.shape)}, expected {dtype} {tuple(shape)}")
    return t.to(dev).contiguous()


def sample_batch(store: MeshStore, sel: Sequence[int], num_points: int, min_part_point: int = 30, max_parts: int = 20, *, seed: int = 0,
                 split: int = 0, uniforms=None, order=None, rotations=None, want_faces: bool = False, check: bool = True
                 ) -> Dict[str, torch.Tensor]:
    """the three kernels over the puzzles sel of the store.  uniforms float64 [B, N, 3] (piece order), order int32 [B, N] (row r of
    puzzle b is sample order[b, r] of its piece: a permutation of each piece's 0 .. n - 1) and rotations float64 [B, max_parts, 3, 3]
    are the given tables of the parity path; what is not given is generated from (seed, split, data_id).  `split` is
    split_word(split, epoch).  check = True waits for the stream and raises what the kernels recorded in the status word.
    -> part_pcs, gt_pcs float32 [B, N, 3]; n_pcs int64 [B, max_parts]; part_quat [B, max_parts, 4], part_trans [B, max_parts, 3]
    float32; part_valids float32 [B, max_parts]; piece_off int64 [B max_parts + 1], puz_piece_off int64 [B + 1]; points float64
    [B, N, 3] (the samples in piece order), rot float64 [B, max_parts, 3, 3]; face_idx int32 [B, N] with want_faces; status."""
    if store.device.type != "cuda" or store.cdf is None:
        raise ValueError(f"sample_batch: the store must live on the GPU (got {store.device}); there is no CPU path")
    sel_h = np.asarray(sel, dtype=np.int64).reshape(-1)
    B, S, N, mp = len(sel_h), len(store), int(num_points), int(max_parts)
    if B == 0:
        raise ValueError("sample_batch: an empty selection")
    if (sel_h < 0).any() or (sel_h >= S).any():
        raise ValueError(f"sample_batch: selection outside the store's {S} puzzles")
    if not 1 <= mp <= 32 or N < 1:
        raise ValueError("sample_batch: 1 <= max_parts <= 32 and num_points >= 1")
    if not 0 <= seed < 2 ** 64 or not 0 <= split < 2 ** 32:
        raise ValueError("seed must fit 64 bits and split 32 bits")
    P = store.num_parts[sel_h]
    if (P > mp).any():
        raise ValueError(f"sample_batch: a selected puzzle has more than max_parts = {mp} parts")
    need = P * max(int(min_part_point), 1)
    if (need > N).any():
        b = int(np.argmax(need > N))
        raise ValueError(f"sample_batch: {store.paths[sel_h[b]]}: {P[b]} parts x min_part_point {min_part_point} > num_points {N} "
                         "(the reference's loop never ends)")
    dev, mb = store.device, store.batch
    u = _table(uniforms, torch.float64, (B, N, 3), "uniforms", dev)
    od = _table(order, torch.int32, (B, N), "order", dev)
    rot = _table(rotations, torch.float64, (B, mp, 3, 3), "rotations", dev)
    sel_d = torch.from_numpy(sel_h).to(dev)
    status = meshes.new_status(dev)
    n_pcs = torch.empty((B, mp), dtype=torch.int64, device=dev)
    piece_off = torch.empty(B * mp + 1, dtype=torch.int64, device=dev)
    puz_piece_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    # with a given order a row that is no permutation entry would stay unwritten: zeros, not stale memory
    points = (torch.zeros if od is not None else torch.empty)((B, N, 3), dtype=torch.float64, device=dev)
    gt = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    pcs = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    face = torch.empty((B, N), dtype=torch.int32, device=dev) if want_faces else None
    quat = torch.empty((B, mp, 4), dtype=torch.float32, device=dev)
    trans = torch.empty((B, mp, 3), dtype=torch.float32, device=dev)
    rot_out = torch.empty((B, mp, 3, 3), dtype=torch.float64, device=dev)
    lib, st = _lib.load(), _stream(dev)
    _check(lib.pfpp_mdata_piece_counts(_p(store.total), _p(mb.puz_part_off), _p(sel_d), B, S, N, int(min_part_point), mp, _p(n_pcs),
                                      _p(piece_off), _p(puz_piece_off), _p(status), st), "pfpp_mdata_piece_counts")
    _check(lib.pfpp_mdata_sample(_p(mb.verts), _p(mb.faces), _p(mb.vert_off), _p(mb.face_off), _p(store.cdf), _p(store.total),
                                _p(mb.puz_part_off), _p(mb.data_id), _p(sel_d), _p(piece_off), B, S, N, mp, _p(od), _p(u), seed, split,
                                _p(points), _p(gt), _p(face), _p(status), st), "pfpp_mdata_sample")
    _check(lib.pfpp_mdata_pose(_p(points), _p(piece_off), _p(mb.data_id), _p(sel_d), B, S, N, mp, _p(od), _p(rot), seed, split, _p(pcs),
                              _p(quat), _p(trans), _p(rot_out), st), "pfpp_mdata_pose")
    if rot is not None:          # the kernel leaves part_quat to the caller when the matrices are given
        valid = np.arange(mp)[None] < P[:, None]
        q = np.zeros((B, mp, 4), dtype=np.float32)
        q[valid] = quat_from_matrix(np.swapaxes(torch.as_tensor(rotations).cpu().numpy()[valid], -1, -2)).astype(np.float32)
        quat = torch.from_numpy(q).to(dev)
    valids = torch.from_numpy((np.arange(mp)[None] < P[:, None]).astype(np.float32)).to(dev)
    if check:
        store._raise_status(status)
    out = {"part_pcs": pcs, "gt_pcs": gt, "n_pcs": n_pcs, "part_quat": quat, "part_trans": trans, "part_valids": valids,
           "piece_off": piece_off, "puz_piece_off": puz_piece_off, "points": points, "rot": rot_out, "status": status}
    if want_faces:
        out["face_idx"] = face
    return out


# --------------------------------------------------------------------------------------------------------------- the dataset
class AllPieceMatchingDataset:
    """the reference's AllPieceMatchingDataset over a resident MeshStore.  store: a MeshStore, a path of MeshStore.save (read when it
    exists, written after the parse otherwise) or None; it is parsed / loaded at the first batch, so discovery alone needs no GPU."""

    def __init__(self, data_dir, data_fn, data_keys, category="all", num_points=1000, min_num_part=2, max_num_part=20,
                 shuffle_parts=False, rot_range=-1, overfit=10, length=-1, sample_by="area", min_part_point=30,
                 fracture_label_threshold=0.025, *, seed: int = 0, split: Optional[str] = None, device="cuda", store=None,
                 workers: Optional[int] = None):
        if sample_by != "area":
            raise NotImplementedError("Must sample by area")
        self.category = category if category.lower() != "all" else ""
        self.data_dir, self.data_keys = data_dir, data_keys
        self.num_points, self.min_num_part, self.max_num_part = int(num_points), int(min_num_part), int(max_num_part)
        self.min_part_point, self.shuffle_parts, self.rot_range = int(min_part_point), bool(shuffle_parts), rot_range
        self.sample_by, self.fracture_label_threshold = sample_by, float(fracture_label_threshold)
        self.seed, self.device, self.workers = int(seed), device, workers
        self.split = split if split is not None else ("val" if ".val." in str(data_fn) else "train")
        self.data_list = read_data_list(data_dir, data_fn, self.category, self.min_num_part, self.max_num_part)
        if overfit > 0:
            self.data_list = self.data_list[:overfit]
        if 0 < length < len(self.data_list):
            self.length = int(length)
            if shuffle_parts:          # the reference's random.shuffle of the list, seeded here
                pos = np.random.default_rng([self.seed, 0x6C656E]).permutation(len(self.data_list))
                self.data_list = [self.data_list[i] for i in pos]
        else:
            self.length = len(self.data_list)
        self._store = store if isinstance(store, MeshStore) else None
        self._store_path = store if isinstance(store, (str, os.PathLike)) else None
        if self._store is not None and list(self._store.paths) != list(self.data_list):
            raise ValueError("AllPieceMatchingDataset: the store's puzzles are not this data_list")

    def __len__(self) -> int:
        return self.length

    @property
    def store(self) -> MeshStore:
        if self._store is None:
            if self._store_path is not None and os.path.exists(self._store_path):
                st = MeshStore.load(self._store_path, self.device)
                if list(st.paths) != list(self.data_list):
                    raise ValueError(f"{self._store_path}: the saved store's puzzles are not this data_list")
            else:
                st = MeshStore.build(self.data_dir, self.data_list, self.device, self.workers)
                if self._store_path is not None:
                    st.save(self._store_path)
            self._store = st
        return self._store

    def _rotations(self, ids: np.ndarray, word: int) -> Optional[np.ndarray]:
        """rot_range > 0 (:130-132): the host draws the Euler angles, keyed by (seed, split, epoch, data_id)"""
        if not self.rot_range > 0.0:
            return None
        rot = np.empty((len(ids), self.max_num_part, 3, 3), dtype=np.float64)
        for b, i in enumerate(ids):
            ang = (np.random.default_rng([self.seed, word, int(i)]).random((self.max_num_part, 3)) - 0.5) * 2.0 * self.rot_range
            rot[b] = euler_xyz_matrix(ang)
        return rot

    def batch(self, indices: Sequence[int], epoch: int = 0, check: bool = True) -> Dict[str, object]:
        """the reference's data_dict (:266-277) for the puzzles `indices`, default-collated, on the device: part_pcs / gt_pcs float32
        [B, N, 3], part_valids float32 [B, P], part_quat [B, P, 4], part_trans [B, P, 3], n_pcs int64 [B, P], data_id int64 [B],
        critical_label_thresholds float32 [B, N], mesh_file_path list, num_parts int64 [B]"""
        ids = np.asarray(indices, dtype=np.int64).reshape(-1)
        if (ids < 0).any() or (ids >= self.length).any():
            raise IndexError(f"batch: index outside the dataset's {self.length} puzzles")
        word = split_word(self.split, epoch)
        store = self.store
        out = sample_batch(store, ids, self.num_points, self.min_part_point, self.max_num_part, seed=self.seed, split=word,
                           rotations=self._rotations(ids, word), check=check)
        dev = store.device
        d = {k: out[k] for k in ("part_pcs", "gt_pcs", "part_valids", "part_quat", "part_trans", "n_pcs")}
        d["data_id"] = torch.from_numpy(ids).to(dev)
        d["critical_label_thresholds"] = torch.full((len(ids), self.num_points), self.fracture_label_threshold, dtype=torch.float32, device=dev)
        d["mesh_file_path"] = [self.data_list[i] for i in ids]
        d["num_parts"] = torch.from_numpy(store.num_parts[ids].astype(np.int64)).to(dev)
        assert tuple(d) == DATA_DICT_KEYS
        return d

    def epoch_order(self, epoch: int, shuffle: bool) -> np.ndarray:
        if not shuffle:
            return np.arange(self.length)
        return np.random.default_rng([self.seed, 0x65706F, int(epoch)]).permutation(self.length)

    def batches(self, batch_size: int, epoch: int = 0, shuffle: bool = False, drop_last: bool = False) -> Iterator[Dict[str, object]]:
        idx = self.epoch_order(epoch, shuffle)
        end = len(idx) - (len(idx) % batch_size if drop_last else 0)
        for i in range(0, end, batch_size):
            yield self.batch(idx[i:i + batch_size], epoch)


class MatchingLoader:
    """what build_all_piece_matching_dataloader returns in a DataLoader's place: iterating yields the batches of one epoch"""

    def __init__(self, dataset: AllPieceMatchingDataset, batch_size: int, shuffle: bool, drop_last: bool):
        self.dataset, self.batch_size, self.shuffle, self.drop_last, self.epoch = dataset, int(batch_size), shuffle, drop_last, 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        return self.dataset.batches(self.batch_size, self.epoch, self.shuffle, self.drop_last)


def _get(node, key, *default):
    if isinstance(node, dict):
        return node.get(key, *default) if default else node[key]
    return getattr(node, key, *default)


def build_all_piece_matching_dataloader(cfg, *, seed: int = 0, device="cuda", train_store=None, val_store=None):
    """(train_loader, val_loader) as :281-323 builds them, from the reference's cfg.DATA.*, cfg.BATCH_SIZE and cfg.NUM_WORKERS names
    (attributes or mapping keys).  NUM_WORKERS sizes the parse pool (0: parse in this process), capped at 16."""
    D = _get(cfg, "DATA")
    bs, nw = int(_get(cfg, "BATCH_SIZE")), int(_get(cfg, "NUM_WORKERS", 0))
    args = dict(data_dir=_get(D, "DATA_DIR"), data_fn=_get(D, "DATA_FN").format("train"), data_keys=_get(D, "DATA_KEYS"),
                category=_get(D, "CATEGORY"), num_points=_get(D, "NUM_PC_POINTS"), min_num_part=_get(D, "MIN_NUM_PART"),
                max_num_part=_get(D, "MAX_NUM_PART"), shuffle_parts=_get(D, "SHUFFLE_PARTS"), rot_range=_get(D, "ROT_RANGE"),
                overfit=_get(D, "OVERFIT"), sample_by=_get(D, "SAMPLE_BY"), min_part_point=_get(D, "MIN_PART_POINT"),
                length=_get(D, "LENGTH") * bs, fracture_label_threshold=_get(D, "FRACTURE_LABEL_THRESHOLD"))
    extra = dict(seed=seed, device=device, workers=min(MAX_WORKERS, nw))
    train_set = AllPieceMatchingDataset(**args, split="train", store=train_store, **extra)
    train_loader = MatchingLoader(train_set, bs, shuffle=True, drop_last=True)
    args.update(data_fn=_get(D, "DATA_FN").format("val"), shuffle_parts=False, length=_get(D, "TEST_LENGTH"))
    val_set = AllPieceMatchingDataset(**args, split="val", store=val_store, **extra)
    val_loader = MatchingLoader(val_set, 2, shuffle=False, drop_last=False)
    return train_loader, val_loader
