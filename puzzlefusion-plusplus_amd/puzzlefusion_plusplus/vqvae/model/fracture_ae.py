"""FractureAE (drop-in for vqvae/model/fracture_ae.py): stage-1 pre-training of the fragment autoencoder on the HIP path.

forward keeps the valid fragments part_pcs[b, :num_parts[b]] and runs cfg.ae.ae_name (VQVAE, or PN2 without the quantizer);
training_step returns cd_loss + embedding_loss, whose backward is the training engine's (pfpp_hip.vqvae_train); configure_optimizers
returns the fused AdamW over self.parameters() in registration order (a reference optimizer state loads by position) with the
reference's hyper-parameters (fracture_ae.py:82-91) and MultiStepLR from cfg.model.lr_scheduler.  Logged keys are the reference's."""
from __future__ import annotations

import torch

from pfpp_hip.lightning_compat import LightningModule, instantiate


class FractureAE(LightningModule):
    # torch.optim.AdamW(self.parameters(), lr=5e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-08), fracture_ae.py:82-91
    OPTIM = dict(lr=5e-4, betas=(0.95, 0.999), eps=1e-08, weight_decay=1e-6)

    def __init__(self, cfg):
        super().__init__()
        self.ae = instantiate(cfg.ae.ae_name, cfg)
        self.cfg = cfg

    def _global_step(self) -> int:
        trainer = getattr(self, "_trainer", None)
        return int(trainer.global_step) if trainer is not None else 0

    def forward(self, data_dict):
        """fracture_ae.py:13-33 -> (output_dict, the caller's data_dict as it came in)"""
        original_data_dict = dict(data_dict)
        part_pcs = data_dict["part_pcs"]
        num_parts = data_dict["num_parts"]
        B, N = part_pcs.shape[:2]
        mask = torch.arange(N, device=part_pcs.device)[None, :] < num_parts.to(part_pcs.device).reshape(B, 1)
        data_dict["part_pcs"] = part_pcs[mask]
        data_dict["iters"] = self._global_step()
        return self.ae(data_dict), original_data_dict

    def _loss(self, data_dict, output_dict):
        return self.ae.loss(data_dict, output_dict)

    def training_step(self, data_dict, idx):
        output_dict, _ = self(data_dict)
        if "perplexity" in output_dict:
            self.log("train_perplexity", output_dict["perplexity"], on_step=True, on_epoch=False)
        loss_dict = self._loss(data_dict, output_dict)
        total_loss = 0
        for loss_name, loss_value in loss_dict.items():
            total_loss = total_loss + loss_value
            self.log(f"train_loss/{loss_name}", loss_value, on_step=True, on_epoch=False)
        self.log("train_loss/total_loss", total_loss, on_step=True, on_epoch=False)
        return total_loss

    def validation_step(self, data_dict, idx):
        with torch.no_grad():
            output_dict, _ = self(data_dict)
            loss_dict = self._loss(data_dict, output_dict)
        total_loss = 0
        for loss_name, loss_value in loss_dict.items():
            total_loss = total_loss + loss_value
            self.log(f"val_loss/{loss_name}", loss_value, on_step=False, on_epoch=True)
        self.log("val_loss/total_loss", total_loss, on_step=False, on_epoch=True)

    def test_step(self, data_dict, idx):
        with torch.no_grad():
            self(data_dict)

    def on_test_epoch_end(self):
        pass

    def configure_optimizers(self):
        from pfpp_hip.optim import FusedAdamW

        optimizer = FusedAdamW(self.ae.train_engine(), params=list(self.parameters()), **self.OPTIM)
        node = getattr(getattr(self.cfg, "model", None), "lr_scheduler", None)
        if node is None:
            lr_scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[800, 1400], gamma=0.5)
        else:
            lr_scheduler = instantiate(node, optimizer)
        return {"optimizer": optimizer, "lr_scheduler": lr_scheduler}
