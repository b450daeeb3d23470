"""GeometryPartDataset (drop-in for vqvae/dataset/pc_dataset.py): the autoencoder's training data.

Reads the pc_data npz files (pfpp_hip.io.load_pc_data), keeps puzzles with min_num_part <= num_parts <= max_num_part, and per
sample recentres every fragment, applies a uniformly random rotation (scipy, drawn from numpy's global RNG in fragment order, as the
reference does), zero-pads to max_num_part fragments and divides every fragment by its largest absolute coordinate (1 for the
padding)."""
from __future__ import annotations

import copy
import os

import numpy as np
from torch.utils.data import DataLoader, Dataset

from pfpp_hip import io as pfio


class GeometryPartDataset(Dataset):
    def __init__(self, cfg, data_dir, data_fn, category="", rot_range=-1, overfit=-1):
        self.cfg = cfg
        self.category = category if category.lower() != "all" else ""
        self.data_dir = data_dir
        self.data_fn = data_fn
        self.data_files = sorted(f for f in os.listdir(data_dir) if f.endswith(".npz"))
        self.max_num_part = cfg.data.max_num_part
        self.min_num_part = cfg.data.min_num_part
        if overfit != -1:
            self.data_files = self.data_files[:overfit]
        self.rot_range = rot_range
        self.data_list = []
        for name in self.data_files:
            d = pfio.load_pc_data(os.path.join(data_dir, name))
            num_parts = int(d["num_parts"])
            if num_parts > self.max_num_part or num_parts < self.min_num_part:
                continue
            self.data_list.append({"part_pcs": d["part_pcs_gt"], "data_id": int(d["data_id"]), "part_valids": d["part_valids"],
                                   "mesh_file_path": str(d["mesh_file_path"]), "num_parts": num_parts})

    @staticmethod
    def _recenter_pc(pc):
        centroid = np.mean(pc, axis=0)
        return pc - centroid[None], centroid

    @staticmethod
    def _rotate_pc(pc):
        from scipy.spatial.transform import Rotation as R

        rot = R.random().as_matrix()
        quat = R.from_matrix(rot.T).as_quat()[[3, 0, 1, 2]]        # scalar-first quaternion of the inverse rotation
        return (rot @ pc.T).T, quat

    def _pad_data(self, data):
        data = np.array(data)
        out = np.zeros((self.max_num_part,) + tuple(data.shape[1:]), dtype=np.float32)
        out[: data.shape[0]] = data
        return out

    def __getitem__(self, idx):
        sample = copy.deepcopy(self.data_list[idx])
        pcs = sample["part_pcs"]
        frags = []
        for i in range(sample["num_parts"]):
            pc, _ = self._recenter_pc(pcs[i])
            pc, _ = self._rotate_pc(pc)
            frags.append(pc)
        cur = self._pad_data(np.stack(frags, axis=0))           # [P, N, 3]
        scale = np.max(np.abs(cur), axis=(1, 2), keepdims=True)
        scale[scale == 0] = 1
        sample["part_pcs"] = cur / scale
        return sample

    def __len__(self):
        return len(self.data_list)


def build_geometry_dataloader(cfg):
    args = dict(cfg=cfg, data_dir=cfg.data.data_dir, data_fn="train", category=cfg.data.category, rot_range=cfg.data.rot_range,
                overfit=cfg.data.overfit)
    train_set = GeometryPartDataset(**args)
    workers = cfg.data.num_workers
    train_loader = DataLoader(train_set, batch_size=cfg.data.batch_size, shuffle=True, num_workers=workers, pin_memory=True,
                              drop_last=True, persistent_workers=workers > 0)
    args.update(data_fn="val", data_dir=cfg.data.data_val_dir)
    val_set = GeometryPartDataset(**args)
    val_loader = DataLoader(val_set, batch_size=cfg.data.batch_size, shuffle=False, num_workers=workers, pin_memory=True,
                            drop_last=False, persistent_workers=workers > 0)
    return train_loader, val_loader
