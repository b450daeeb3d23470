"""PointNet++ fragment autoencoder (drop-in for vqvae/model/modules/pn2.py), HIP-backed.

Keeps the reference's parameter tree: sa1/sa2/sa3 (PointNetSetAbstraction), conv6 and the decoder linears fc1-fc3.  encode() is
the Denoiser's feature extractor; forward / decode / loss are stage-1 pre-training with ae_name = PN2 (no quantizer): in .train()
with autograd on, forward is one autograd node of pfpp_hip.vqvae_train (batch-statistics BatchNorm, backward on the HIP kernels,
gradients into the parameters' .grad); in .eval() it is the inference encoder and the decoder.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from pfpp_hip import ops
from utils.pn2_utils import PointNetSetAbstraction


def train_engine_of(module: nn.Module):
    """the training engine of a PN2 / VQVAE (pfpp_hip.vqvae_train.VQVAETrainEngine), created on first use: from then on the
    parameters are views of one flat buffer (same names, shapes and values)"""
    if getattr(module, "_engine", None) is None:
        from pfpp_hip.vqvae_train import VQVAETrainEngine

        object.__setattr__(module, "_engine", VQVAETrainEngine(module))
    return module._engine


def train_forward(module: nn.Module, part_pcs: torch.Tensor):
    """train-mode forward of a PN2 / VQVAE -> (embedding_loss, pc_offset, z_q, perplexity, xyz); one autograd node when autograd is on
    and a parameter requires grad"""
    from pfpp_hip.vqvae_train import _TrainFn

    eng = train_engine_of(module)
    anchor = next((p for p in module.parameters() if p.requires_grad), None)
    if torch.is_grad_enabled() and anchor is not None:
        return _TrainFn.apply(eng, part_pcs, anchor)
    with torch.no_grad():
        out, _ = eng.forward(part_pcs)
    return out["embedding_loss"], out["pc_offset"], out["z_q"], out["perplexity"], out["xyz"]


class PN2(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.num_point = cfg.ae.num_point
        self.num_dim = cfg.ae.num_dim
        self.local_decode_pts = cfg.ae.local_decode_pts
        # pn2.py:16-18
        self.sa1 = PointNetSetAbstraction(256, 0.2, 32, 3, [64, 64, 128], False)
        self.sa2 = PointNetSetAbstraction(128, 0.4, 64, 128 + 3, [128, 128, 256], False)
        self.sa3 = PointNetSetAbstraction(self.num_point, 0.8, 64, 256 + 3, [256, 256, 512], False)
        self.conv6 = nn.Conv1d(512, self.num_dim, kernel_size=1)
        self.fc1 = nn.Linear(self.num_dim, 256)
        self.fc2 = nn.Linear(256, 512)
        self.fc3 = nn.Linear(512, self.local_decode_pts * 3)

    def encode_channels_last(self, pts: torch.Tensor):
        """pts [F,N,3] -> z_e [F,L,num_dim], xyz [F,L,3]"""
        xyz, feats = pts.contiguous(), None
        for sa in (self.sa1, self.sa2, self.sa3):
            xyz, feats = sa.forward_channels_last(xyz, feats)
        F, L, C = feats.shape
        w = self.conv6.weight.detach().reshape(self.num_dim, C)
        z = ops.linear(feats.view(F * L, C), w.contiguous(), self.conv6.bias.detach().contiguous())
        return z.view(F, L, self.num_dim), xyz

    def encode(self, xyz: torch.Tensor):
        """xyz [F,3,N] (channel-first, as the reference passes it) -> (z_e [F,L,C], xyz [F,L,3]) (pn2.py:57-68)"""
        return self.encode_channels_last(xyz.permute(0, 2, 1))

    def train_engine(self):
        return train_engine_of(self)

    def decode(self, global_feat):
        """global_feat [B,L,C] -> pc_offset [B,L,local_decode_pts,3] = fc3(relu(fc2(relu(fc1(.))))) (pn2.py:71-81); values only"""
        B, L, C = global_feat.shape
        x = global_feat.detach().reshape(B * L, C).contiguous().float()
        for k, act in ((1, "relu"), (2, "relu"), (3, "none")):
            fc = getattr(self, f"fc{k}")
            x = ops.linear(x, fc.weight.detach().contiguous(), fc.bias.detach().contiguous(), act=act, mode="f32")
        return x.view(B, self.num_point, self.local_decode_pts, 3)

    def forward(self, data_dict):
        """data_dict["part_pcs"] [F,N,3] -> {"pc_offset", "global_feat", "xyz"} (pn2.py:31-56)"""
        pcs = data_dict["part_pcs"]
        if self.training:
            _, off, feat, _, xyz = train_forward(self, pcs)
            return {"pc_offset": off, "global_feat": feat, "xyz": xyz}
        z_e, xyz = self.encode_channels_last(pcs.float())
        return {"pc_offset": self.decode(z_e), "global_feat": z_e, "xyz": xyz}

    def loss(self, data_dict, output_dict):
        """{"cd_loss"}: chamferdist's bidirectional Chamfer distance of pc_offset + xyz against part_pcs (pn2.py:83-97), a
        differentiable HIP op (gradient to pc_offset)"""
        from pfpp_hip.vqvae_train import chamfer_loss

        return {"cd_loss": chamfer_loss(output_dict["pc_offset"], output_dict["xyz"], data_dict["part_pcs"],
                                        self.num_point * self.local_decode_pts)}
