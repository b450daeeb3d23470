"""CPU: stage-1 pre-training surface (vqvae/model/fracture_ae.py, vqvae/dataset/pc_dataset.py, vqvae/data/data_module.py).

The dataset drop-in reads files written by pfpp_hip.io and returns what the reference's GeometryPartDataset returns on the same
files and numpy seed (tests/golden/vqvae_dataset.npz, written from the reference's pc_dataset.py on the files
`tools/make_synthetic_dataset.py <dir> --n 3 --points 64` writes, numpy seed 100 + i per item)."""
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_geometry_part_dataset_equals_the_reference_loader(golden, tmp_path):
    subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_dataset.py"), str(tmp_path), "--n", "3", "--points", "64"],
                   check=True, capture_output=True)
    from puzzlefusion_plusplus.vqvae.dataset.pc_dataset import GeometryPartDataset

    g = golden("vqvae_dataset")
    cfg = NS(data=NS(max_num_part=20, min_num_part=2))
    ds = GeometryPartDataset(cfg, str(tmp_path / "pc_data" / "train"), "train", category="all")
    assert len(ds) == int(g["len"]) >= 2
    for i in range(len(ds)):
        np.random.seed(100 + i)
        item = ds[i]
        for k in ("part_pcs", "num_parts", "data_id", "part_valids"):
            want, got = g[f"{i}_{k}"], np.asarray(item[k])
            assert got.shape == want.shape, (i, k)
            assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-6, (i, k)
        assert item["part_pcs"].dtype == np.float64 or item["part_pcs"].dtype == np.float32


def test_data_module_builds_both_loaders(tmp_path):
    subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_dataset.py"), str(tmp_path), "--n", "3", "--points", "64"],
                   check=True, capture_output=True)
    from pfpp_hip import config
    from puzzlefusion_plusplus.vqvae.data.data_module import DataModule

    d = str(tmp_path / "pc_data" / "train")
    dm = DataModule(config.vqvae_train_config(data=dict(data_dir=d, data_val_dir=d, num_workers=0, batch_size=1)))
    assert len(dm.train_dataloader()) == len(dm.val_dataloader()) >= 2
    batch = next(iter(dm.val_dataloader()))
    assert tuple(batch["part_pcs"].shape) == (1, 20, 64, 3) and batch["num_parts"].shape == (1,)


def test_fracture_ae_layout_and_optimizer_settings():
    from pfpp_hip import config
    from pfpp_hip.lightning_compat import instantiate
    from puzzlefusion_plusplus.vqvae.model.fracture_ae import FractureAE
    from puzzlefusion_plusplus.vqvae.model.modules.pn2 import PN2
    from puzzlefusion_plusplus.vqvae.model.modules.vq_vae import VQVAE
    from oracle import weights

    cfg = config.vqvae_train_config()
    fae = FractureAE(cfg)
    assert isinstance(fae.ae, VQVAE)
    keys = list(fae.state_dict())
    ref = list(weights.vqvae_state_dict())
    assert len(ref) == 72 and sorted(keys) == sorted("ae." + k for k in ref)
    params = list(fae.parameters())
    assert len(params) == 45 and sum(p.numel() for p in params) == 605_688
    assert FractureAE.OPTIM == dict(lr=5e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6)
    opt = torch.optim.AdamW(params, **FractureAE.OPTIM)
    sched = instantiate(cfg.model.lr_scheduler, opt)
    assert isinstance(sched, torch.optim.lr_scheduler.MultiStepLR)
    assert dict(sched.milestones) == {800: 1, 1400: 1} and sched.gamma == 0.5
    pn2_ae = FractureAE(config.vqvae_train_config("PN2")).ae
    assert isinstance(pn2_ae, PN2) and len(list(pn2_ae.parameters())) == 44


def test_fracture_ae_forward_keeps_the_valid_fragments():
    """fracture_ae.py:13-33: part_pcs[b, :num_parts[b]] go to the autoencoder, `iters` is set, the caller's dict comes back"""
    from pfpp_hip import config
    from puzzlefusion_plusplus.vqvae.model.fracture_ae import FractureAE

    fae = FractureAE(config.vqvae_train_config())
    seen = {}

    def fake_ae(d):
        seen.update(d)
        return {"pc_offset": None}

    object.__setattr__(fae, "ae", fake_ae)
    pcs = torch.arange(2 * 4 * 5 * 3, dtype=torch.float32).view(2, 4, 5, 3)
    data = {"part_pcs": pcs, "num_parts": torch.tensor([3, 1])}
    _, orig = fae(data)
    assert torch.equal(seen["part_pcs"], torch.cat([pcs[0, :3], pcs[1, :1]])) and seen["iters"] == 0
    assert orig["part_pcs"] is pcs
