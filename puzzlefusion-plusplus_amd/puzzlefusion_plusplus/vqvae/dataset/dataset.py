"""GeometryPartDataset (drop-in for vqvae/dataset/dataset.py): the Breaking Bad meshes -> the pc_data batches generate_pc_data.py
writes.

The dataset itself does host work only (discovery, _read_data :57-83, exactly as the reference; per item: list the folder, sort,
optional random.shuffle, read the OBJ files), so DataLoader workers never touch the GPU.  build_geometry_dataloader wraps each
loader so that every batch is finished on the GPU in the main process (pfpp_hip.meshes.pc_data_batch: contact graph, surface
sampling, scale and reference part) and comes out as the reference's batch dict.  With batch size 1 the shapes and dtypes are
what the reference's collate gives (part_pcs_gt [1, Pv, N, 3] float64); with larger batches part_pcs_gt is zero-padded to
max_num_part — the reference cannot collate fragments of different counts at all.

Deviations: the reference draws its uniforms from an unseeded global RNG; here they come from a counter-based generator keyed by
(cfg.data.pc_seed, split, data_id, slot, sample), so a run is reproducible and a puzzle's points do not depend on its batch.
trimesh.load merges vertices closer than 1e-8 and drops unreferenced ones; pfpp_hip.meshes.read_obj only does the latter."""
from __future__ import annotations

import os
import random
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from pfpp_hip import meshes

SPLITS = {"train": 0, "val": 1}


class MeshReadError(RuntimeError):
    pass


class GeometryPartDataset(Dataset):
    def __init__(self, data_dir, data_fn, data_keys, cfg, category="", num_points=1000, min_num_part=2, max_num_part=20,
                 shuffle_parts=False, rot_range=-1, overfit=-1):
        self.cfg = cfg
        self.category = category if category.lower() != "all" else ""
        self.data_dir = data_dir
        self.num_points = num_points
        self.min_num_part = min_num_part
        self.max_num_part = max_num_part
        self.shuffle_parts = shuffle_parts
        self.rot_range = rot_range
        self.data_list = self._read_data(data_fn)
        if overfit > 0:
            self.data_list = self.data_list[:overfit]
        self.data_keys = data_keys

    def _read_data(self, data_fn):
        """dataset.py:57-83: the listed objects (category filter on the path components), their fracture / mode folders in sorted
        order, kept when min_num_part <= (number of entries in the folder) <= max_num_part"""
        with open(os.path.join(self.data_dir, data_fn), "r") as f:
            mesh_list = [line.strip() for line in f.readlines()]
            if self.category:
                mesh_list = [line for line in mesh_list if self.category in line.split("/")]
        data_list = []
        for mesh in mesh_list:
            mesh_dir = os.path.join(self.data_dir, mesh)
            if not os.path.isdir(mesh_dir):
                print(f"{mesh} does not exist")
                continue
            fracs = os.listdir(mesh_dir)
            fracs.sort()
            for frac in fracs:
                if "fractured" not in frac and "mode" not in frac:
                    continue
                frac = os.path.join(mesh, frac)
                num_parts = len(os.listdir(os.path.join(self.data_dir, frac)))
                if self.min_num_part <= num_parts <= self.max_num_part:
                    data_list.append(frac)
        return data_list

    def __getitem__(self, index) -> Dict[str, object]:
        """host half of _get_pcs (:154-171): the part meshes of one puzzle, in the reference's part order"""
        rel = self.data_list[index]
        folder = os.path.join(self.data_dir, rel)
        mesh_files = os.listdir(folder)
        mesh_files.sort()
        if not self.min_num_part <= len(mesh_files) <= self.max_num_part:
            raise ValueError(f"{folder}: {len(mesh_files)} parts")
        if self.shuffle_parts:
            random.shuffle(mesh_files)
        parts = []
        for name in mesh_files:
            path = os.path.join(folder, name)
            try:
                parts.append(meshes.read_obj(path))
            except (OSError, ValueError) as e:
                raise MeshReadError(f"cannot read mesh {path}: {e}") from None
        return {"data_id": index, "mesh_file_path": rel, "category": rel.split("/")[1].lower(), "meshes": parts}

    def __len__(self):
        return len(self.data_list)


def _host_items(items):
    return items


def collate_pc_data(items: List[Dict[str, object]], max_num_part: int) -> Dict[str, object]:
    """the reference's default collate of __getitem__'s dicts (batch size 1), part_pcs_gt zero-padded to max_num_part for more"""
    out: Dict[str, object] = {}
    pcs = [np.asarray(d["part_pcs_gt"]) for d in items]
    if len(items) == 1:
        out["part_pcs_gt"] = torch.from_numpy(pcs[0])[None]
    else:
        pad = np.zeros((len(items), max_num_part) + pcs[0].shape[1:], dtype=np.float64)
        for i, p in enumerate(pcs):
            pad[i, : len(p)] = p
        out["part_pcs_gt"] = torch.from_numpy(pad)
    out["ref_part"] = torch.from_numpy(np.stack([d["ref_part"] for d in items]))
    out["part_valids"] = torch.from_numpy(np.stack([d["part_valids"] for d in items]))
    out["mesh_file_path"] = [d["mesh_file_path"] for d in items]
    out["num_parts"] = torch.tensor([d["num_parts"] for d in items], dtype=torch.int64)
    out["graph"] = torch.from_numpy(np.stack([d["graph"] for d in items]))
    out["category"] = [d["category"] for d in items]
    out["data_id"] = torch.tensor([d["data_id"] for d in items], dtype=torch.int64)
    return out


class PcDataLoader:
    """a DataLoader of GeometryPartDataset items whose batches are finished on the GPU (pfpp_hip.meshes.pc_data_batch)"""

    def __init__(self, dataset: GeometryPartDataset, split: str, batch_size: int, num_workers: int, drop_last: bool, seed: int = 0,
                 device=None, uniforms: Optional[Callable] = None):
        self.dataset = dataset
        self.split = split
        self.seed = int(seed)
        self.device = device          # None: the current GPU, looked up when the first batch is finished
        self.uniforms = uniforms
        self.loader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, drop_last=drop_last,
                                 collate_fn=_host_items, persistent_workers=False)

    def __len__(self):
        return len(self.loader)

    def pc_data(self):
        """yields the per-puzzle pc_data dicts of every batch (io.PC_DATA_KEYS)"""
        hook = None
        if self.uniforms is not None:
            hook = lambda pz: self.uniforms(self.split, pz)        # noqa: E731
        for items in self.loader:          # the workers start before this process touches the GPU
            dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            yield meshes.pc_data_batch(items, num_points=self.dataset.num_points, max_num_part=self.dataset.max_num_part,
                                       seed=self.seed, split=SPLITS.get(self.split, 0), uniforms=hook, device=dev)

    def __iter__(self):
        for batch in self.pc_data():
            yield collate_pc_data(batch, self.dataset.max_num_part)


def _cfg_get(node, key, default):
    if isinstance(node, dict):
        return node.get(key, default)
    return getattr(node, key, default)


def build_geometry_dataloader(cfg, uniforms: Optional[Callable] = None, drop_last_train: bool = True):
    """(train_loader, val_loader) as dataset.py:232-269 builds them; the seed of the generated uniforms is cfg.data.pc_seed
    (default 0).  uniforms (test hook): (split, puzzle item) -> float64 [Pv, N, 3] given uniforms."""
    d = cfg.data
    data_dict = dict(data_dir=d.mesh_data_dir, data_fn=d.data_fn.format("train"), data_keys=d.data_keys, cfg=cfg, category=d.category,
                     num_points=d.num_pc_points, min_num_part=d.min_num_part, max_num_part=d.max_num_part,
                     shuffle_parts=d.shuffle_parts, rot_range=d.rot_range, overfit=d.overfit)
    seed = int(_cfg_get(d, "pc_seed", 0) or 0)
    train_set = GeometryPartDataset(**data_dict)
    train_loader = PcDataLoader(train_set, "train", d.batch_size, d.num_workers, drop_last=drop_last_train, seed=seed, uniforms=uniforms)
    data_dict["data_fn"] = d.data_fn.format("val")
    data_dict["shuffle_parts"] = False
    val_set = GeometryPartDataset(**data_dict)
    val_loader = PcDataLoader(val_set, "val", d.val_batch_size, d.num_workers, drop_last=False, seed=seed, uniforms=uniforms)
    return train_loader, val_loader
