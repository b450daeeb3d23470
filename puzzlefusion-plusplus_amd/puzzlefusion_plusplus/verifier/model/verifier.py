"""Verifier shell (drop-in for puzzlefusion_plusplus/verifier/model/verifier.py) on the HIP-backed VerifierTransformer.

`forward(data_dict) -> {"logits"}`, `_loss` (the weighted BCE of verifier.py:20-47: negatives weighted 0.2, mean over the valid
edges, plus torchmetrics' binary accuracy / precision / recall / F1 of sigmoid(logits) > 0.5) and `validation_step` run the
inference kernels.  Training runs on the MI355X too (pfpp_hip.verifier_train): `training_step` evaluates the train-mode forward
and the loss in one pass of the HIP kernels and returns a loss whose backward is the engine's backward (gradients land in the
parameters' .grad); `configure_optimizers` returns the fused AdamW over `self.parameters()` in registration order, so the
optimizer state of a reference Lightning checkpoint loads by position.  Published verifier checkpoints load unchanged (same
state_dict keys)."""
from __future__ import annotations

import torch
from torch.nn import functional as F

from pfpp_hip.lightning_compat import LightningModule
from puzzlefusion_plusplus.verifier.model.modules.verifier_transformer import VerifierTransformer


def _confusion(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(tp, fp, tn, fn) of boolean predictions against 0/1 targets"""
    pos = target > 0.5
    return torch.stack([(pred & pos).sum(), (pred & ~pos).sum(), (~pred & ~pos).sum(), (~pred & pos).sum()])


class Verifier(LightningModule):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.verifier = VerifierTransformer(cfg)
        self.save_hyperparameters()
        self.neg_weight = 0.2

    def forward(self, data_dict):
        logits = self.verifier(data_dict["edge_features"], data_dict["edge_indices"], data_dict["edge_valids"])
        return {"logits": logits}

    def _loss(self, data_dict, output_dict):
        """loss values (no graph): weighted BCE over the valid edges and the reference's metrics, verifier.py:20-47"""
        from pfpp_hip.verifier_train import binary_metrics

        mask = data_dict["edge_valids"].bool()
        logits = output_dict["logits"].squeeze(-1)[mask].detach()
        target = data_dict["cls_gt"].float()[mask]
        weight = torch.where(target > 0.5, torch.ones_like(target), torch.full_like(target, self.neg_weight))
        loss = F.binary_cross_entropy_with_logits(logits, target, weight=weight)
        out = {"bce_loss": loss, "cls_loss": loss}
        out.update(binary_metrics(_confusion(torch.sigmoid(logits) > 0.5, target)))
        return out

    def validation_step(self, data_dict, idx):
        with torch.no_grad():
            loss = self._loss(data_dict, self(data_dict))["bce_loss"]
        self.log("val_loss/bce_loss", loss, on_step=False, on_epoch=True)
        return loss

    def training_step(self, data_dict, idx):
        """verifier.py:49-69: train-mode forward + weighted BCE in one pass of the HIP kernels; returns the loss (its backward is the
        engine's) and logs the reference's keys"""
        from pfpp_hip.verifier_train import binary_metrics

        loss, _logits, stats = self.verifier.train_loss(data_dict["edge_features"], data_dict["edge_indices"],
                                                        data_dict["edge_valids"], data_dict["cls_gt"])
        m = binary_metrics(stats)
        self.log("training/loss", loss, on_step=True, on_epoch=False)
        self.log("training/cls_precision", m["cls_precision"], on_step=False, on_epoch=True)
        self.log("training/cls_recall", m["cls_recall"], on_step=False, on_epoch=True)
        self.log("training/cls_f1_score", m["cls_f1_score"], on_step=False, on_epoch=True)
        self.log("training/cls_acc", m["cls_acc"], on_step=False, on_epoch=True)
        return loss

    def configure_optimizers(self):
        # torch.optim.AdamW(self.parameters(), lr=2e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8), verifier.py:100-107, on the
        # fused kernel over the engine's flat buffer
        from pfpp_hip.optim import FusedAdamW

        return FusedAdamW(self.verifier.train_engine(), lr=2e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6,
                          params=list(self.parameters()))
