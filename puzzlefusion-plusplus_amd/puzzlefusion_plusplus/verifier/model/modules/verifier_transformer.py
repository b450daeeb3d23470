"""VerifierTransformer (drop-in for verifier/model/modules/verifier_transformer.py), HIP-backed.

Owns a torch nn.TransformerEncoder purely as the parameter container (identical state_dict keys:
transformer_encoder.layers.{i}.self_attn.in_proj_weight, ...).  In .eval() forward runs pfpp_hip.verifier; in .train() it runs
the training forward of pfpp_hip.verifier_train (the four dropout sites per layer active) as one autograd node whose backward is
the engine's backward (gradients accumulated straight into the parameters' .grad, views of the engine's flat buffer).
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.nn import TransformerEncoder, TransformerEncoderLayer

from pfpp_hip import verifier as hip_verifier
from pfpp_hip.packing import PackCache
from utils.model_utils import PositionalEncoding


class _TrainFn(torch.autograd.Function):
    """VerifierTransformer.forward in train mode as one autograd node (logits -> engine backward through the head kernel)"""

    @staticmethod
    def forward(ctx, eng, seed, edge_features, edge_indices, mask, grad_anchor):
        # grad_anchor: any parameter that requires grad, so that autograd records this node
        logits, saved = eng.forward(edge_features, edge_indices, mask, seed=seed, train=True)
        ctx.eng, ctx.saved = eng, saved
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        ctx.eng.backward(ctx.saved, dlogit=dlogits.contiguous())
        ctx.saved = None
        return (None,) * 6


class _TrainLossFn(torch.autograd.Function):
    """training forward + Verifier._loss's weighted BCE in the head kernel as one autograd node -> (loss, logits, counts)"""

    @staticmethod
    def forward(ctx, eng, seed, edge_features, edge_indices, mask, cls_gt, grad_anchor):
        logits, saved = eng.forward(edge_features, edge_indices, mask, seed=seed, train=True, cls_gt=cls_gt)
        ctx.eng, ctx.saved = eng, saved
        ctx.mark_non_differentiable(logits, saved.t["stats"])
        return saved.t["loss"].reshape(()), logits, saved.t["stats"]

    @staticmethod
    def backward(ctx, grad_loss, _g_logits, _g_stats):
        ctx.eng.backward(ctx.saved, grad_out=grad_loss)
        ctx.saved = None
        return (None,) * 7


class VerifierTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.model_channels = cfg.model.embed_dim
        self.num_layers = cfg.model.num_layers
        self.num_heads = cfg.model.num_heads
        C = self.model_channels
        layer = TransformerEncoderLayer(d_model=C, nhead=self.num_heads, dim_feedforward=2048, dropout=0.1,
                                        batch_first=True, activation="gelu")
        self.transformer_encoder = TransformerEncoder(layer, num_layers=self.num_layers, enable_nested_tensor=False)
        self.edge_indices_pe = PositionalEncoding(C // 2, max_len=20)
        self.edge_feature_emb = nn.Linear(7, C)
        self.mlp_out = nn.Linear(C, 1)
        self._cache = PackCache()

    def packed(self):
        live = dict(self.named_parameters())
        live.update(dict(self.named_buffers()))
        return self._cache.get(list(live.values()),
                               lambda: hip_verifier.pack_verifier({k: v.detach() for k, v in live.items()},
                                                                  self.num_layers))

    def train_engine(self):
        """the training engine (pfpp_hip.verifier_train.VerifierTrainEngine); created on first use: from then on the parameters
        are views of one flat buffer (same names, shapes and values)"""
        if getattr(self, "_engine", None) is None:
            from pfpp_hip.verifier_train import VerifierTrainEngine

            object.__setattr__(self, "_engine", VerifierTrainEngine(self))
        return self._engine

    @staticmethod
    def _seed() -> int:
        return int(torch.randint(0, 2 ** 62, (1,)).item())          # torch.manual_seed governs the dropout masks

    def forward(self, edge_features, edge_indices, mask):
        """edge_features [B,E,7], edge_indices i64 [B,E,2], mask [B,E] -> logits [B,E,1]"""
        if self.training:
            eng = self.train_engine()
            if torch.is_grad_enabled():
                return _TrainFn.apply(eng, self._seed(), edge_features, edge_indices, mask, self.mlp_out.bias)
            return eng.forward(edge_features, edge_indices, mask, seed=self._seed(), train=True)[0]
        return hip_verifier.verifier_forward(self.packed(), edge_features, edge_indices, mask,
                                             num_layers=self.num_layers, num_heads=self.num_heads)

    def train_loss(self, edge_features, edge_indices, mask, cls_gt):
        """train-mode forward with the weighted BCE of Verifier._loss (verifier.py:20-47) evaluated by the head kernel in the same
        pass -> (loss [] attached to the engine's backward, logits [B,E,1], confusion counts int32 [4] = (tp, fp, tn, fn))"""
        return _TrainLossFn.apply(self.train_engine(), self._seed(), edge_features, edge_indices, mask, cls_gt, self.mlp_out.bias)
