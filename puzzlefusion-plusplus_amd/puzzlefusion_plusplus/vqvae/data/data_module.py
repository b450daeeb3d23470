"""DataModule (drop-in for vqvae/data/data_module.py): the train / val loaders of pc_dataset.build_geometry_dataloader."""
from __future__ import annotations

from pfpp_hip.lightning_compat import HAVE_LIGHTNING
from puzzlefusion_plusplus.vqvae.dataset.pc_dataset import build_geometry_dataloader

if HAVE_LIGHTNING:  # pragma: no cover - depends on the host environment
    import lightning.pytorch as pl

    _Base = pl.LightningDataModule
else:
    _Base = object


class DataModule(_Base):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.train_data, self.val_data = build_geometry_dataloader(cfg)

    def train_dataloader(self):
        return self.train_data

    def val_dataloader(self):
        return self.val_data
