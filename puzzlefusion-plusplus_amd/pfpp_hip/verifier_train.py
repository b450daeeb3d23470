"""Training step of the VerifierTransformer on the HIP kernels.

Reference: Verifier._loss / training_step / configure_optimizers (verifier/model/verifier.py:20-69, 100-107) around
VerifierTransformer.forward (verifier_transformer.py:45-58) in train mode: six post-norm nn.TransformerEncoderLayer(d_model 256,
nhead 8, dim_feedforward 2048, dropout 0.1, activation gelu, batch_first) with four dropout sites per layer (attention
probabilities, dropout1 before norm1, the dropout after GELU, dropout2 before norm2), key padding mask ~edge_valids.

Layer (forward, what is saved for the backward in brackets):
    [x] -> qkv = x W_in^T + b_in [qkv] -> att, lse = attention with probability dropout [att, lse]
        -> s1 = x + drop1(att W_o^T + b_o) [s1] -> x1 = LN1(s1) [x1] -> z = x1 W_1^T + b_1 [z] -> u = drop(gelu(z)) [u]
        -> s2 = x1 + drop2(u W_2^T + b_2) [s2] -> x2 = LN2(s2)
Kernels: the denoiser's split-f16 GEMMs (ops.gemm / ops.linear), pfpp_dropout_layernorm / pfpp_layernorm_bwd_dropout for both
post-norm sites, pfpp_gemm_grad for dX / dW (operands lifted by the power-of-two grad_scale), pfpp_adamw_guarded; and the
verifier's own csrc/verifier_train.hip: attention with probability dropout (forward + single-launch backward), GELU + dropout,
mlp_out + weighted BCE.  Padded edges are computed like the reference computes them; their rows receive no gradient from the
loss and, as masked keys, none through the attention.

Parameters, gradients, Adam moments and split-f16 planes live in one flat buffer (VerifierFlat, the FlatParams layout rules
with the module's registration order); the module's nn.Parameters are views of it.  Gradient scale and overflow guard are
the denoiser engine's (DenoiserTrainEngine._update_grad_scale / _after_step_overflow), driven by max |dlogit|.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as Fnn

from . import ops
from . import train_ops as T
from .packing import round_up
from .train import DenoiserTrainEngine, FlatParams, TrainContext, _f32c, _pw_view, _u8

DROPOUT = 0.1                 # TransformerEncoderLayer(dropout=0.1), verifier_transformer.py:17-24
NEG_WEIGHT = 0.2              # torch.where(cls_gt == 0, 0.2, 1.0), verifier.py:29
SITES_PER_LAYER = 4           # attention probabilities, dropout1, feed-forward dropout, dropout2


def site(layer: int, k: int) -> int:
    """dropout site of layer `layer`: k = 0 attention probabilities, 1 dropout1, 2 after GELU, 3 dropout2"""
    return 1 + SITES_PER_LAYER * layer + k


class VerifierFlat(FlatParams):
    """flat storage of a VerifierTransformer's parameters (registration order), gradients, Adam moments and split-f16 planes"""

    def __init__(self, module: torch.nn.Module):          # noqa: super().__init__ is the denoiser's layout
        named = dict(module.named_parameters())
        self.module = module
        self.num_layers = module.num_layers
        self.order = list(named)
        dev = next(module.parameters()).device
        if dev.type != "cuda":
            raise ValueError("VerifierFlat: the module must live on the GPU (there is no CPU training path)")
        self.offset: Dict[str, int] = {}
        total = 0
        for n in self.order:
            self.offset[n] = total
            total += round_up(named[n].numel(), 8)          # 16-byte aligned fp16 planes
        self.numel = total
        z = lambda dt: torch.zeros(total, dtype=dt, device=dev)
        self.params, self.grads, self.exp_avg, self.exp_avg_sq = (z(torch.float32) for _ in range(4))
        self.hi, self.lo = z(torch.float16), z(torch.float16)
        self.named = named
        self._clean = False
        with torch.no_grad():
            for n in self.order:
                p = named[n]
                v = self.view(self.params, n, p.shape)
                v.copy_(p.detach())
                p.data = v
        self.attach_grads()
        self._views = None
        self.refresh_planes()

    def operands(self):
        first = self.named[self.order[0]]
        if first.data_ptr() != self.params.data_ptr():
            raise RuntimeError("VerifierFlat: the module's parameters were re-allocated (.to()/.cuda() after the training engine was "
                               "created); build the engine after moving the module")
        if self._versions() != self._seen_version:
            self.refresh_planes()         # load_state_dict / in-place edits of the parameters through torch
        if self._views is None:
            w: Dict[str, object] = {}
            g: Dict[str, torch.Tensor] = {}
            pw = lambda n: _pw_view(*(self.view(f, n) for f in (self.params, self.hi, self.lo)))
            for i in range(self.num_layers):
                p = f"transformer_encoder.layers.{i}"
                for src, dst in (("self_attn.in_proj_weight", "wqkv"), ("self_attn.out_proj.weight", "wo"),
                                 ("linear1.weight", "w1"), ("linear2.weight", "w2")):
                    w[f"{i}.{dst}"] = pw(f"{p}.{src}")
                    g[f"{i}.{dst}"] = self.view(self.grads, f"{p}.{src}")
                for src, dst in (("self_attn.in_proj_bias", "bqkv"), ("self_attn.out_proj.bias", "bo"), ("linear1.bias", "b1"),
                                 ("linear2.bias", "b2"), ("norm1.weight", "g1"), ("norm1.bias", "be1"), ("norm2.weight", "g2"),
                                 ("norm2.bias", "be2")):
                    w[f"{i}.{dst}"] = self.view(self.params, f"{p}.{src}")
                    g[f"{i}.{dst}"] = self.view(self.grads, f"{p}.{src}")
            for key, name in (("feat.w", "edge_feature_emb.weight"), ("feat.b", "edge_feature_emb.bias"), ("out.b", "mlp_out.bias")):
                w[key] = self.view(self.params, name)
                g[key] = self.view(self.grads, name)
            C = w["feat.b"].numel()
            w["out.w"] = self.view(self.params, "mlp_out.weight", (C,))
            g["out.w"] = self.view(self.grads, "mlp_out.weight", (C,))
            self._views = {"w": w, "g": g}
        return self._views

    def after_optimizer_step(self) -> None:
        pass


class VerifierTrainEngine:
    """forward (train mode) / backward / optimizer step of a VerifierTransformer on the HIP kernels"""

    # gradient scale (power of two tracking max |dlogit|, two backward passes late) and overflow guard (AdamW skips and flags
    # non-finite gradients, the scale backs off): the denoiser engine's policy, shared code
    _update_grad_scale = DenoiserTrainEngine._update_grad_scale
    _after_step_overflow = DenoiserTrainEngine._after_step_overflow
    _apply_backoff = DenoiserTrainEngine._apply_backoff

    def __init__(self, module: torch.nn.Module, *, dropout: float = DROPOUT, grad_scale: float = 4096.0):
        self.flat = VerifierFlat(module)
        self.module = module
        self.num_layers = module.num_layers
        self.num_heads = module.num_heads
        self.p = float(dropout)
        if math.log2(grad_scale) % 1 != 0:
            raise ValueError("grad_scale must be a power of two (exact rescaling)")
        self.grad_scale = float(grad_scale)
        self._dyn_gscale = True
        self._amax_ring = None
        self._n_backward = 0
        self.step_count = 0
        dev = self.flat.params.device
        self._overflow = torch.zeros(2, dtype=torch.int32, device=dev)
        self._ovf_ring = None
        self._backoff = 1.0
        self._clean_steps = 0
        self.overflow_steps = 0
        C = module.model_channels
        self._feat_w8 = torch.zeros((C, 8), dtype=torch.float32, device=dev)   # the 7-wide embedding, K padded for the fp32 GEMM
        self._head_ws = T.verifier_head_workspace(dev)

    def tables_state_changed(self) -> None:
        """(FusedAdamW.load_state_dict hook: the verifier has no sparse tables)"""

    def arm_optimizer(self, **_hp) -> None:
        """no optimizer-in-backward here: FusedAdamW.step() does the whole update"""

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, edge_features: torch.Tensor, edge_indices: torch.Tensor, edge_valids: torch.Tensor, *, seed: int = 0,
                train: bool = True, cls_gt: Optional[torch.Tensor] = None):
        """-> (logits [B, E, 1], context).  With cls_gt the loss of Verifier._loss is evaluated by the head kernel in the same pass
        (context "loss", "stats" = (tp, fp, tn, fn), and its gradient is kept for backward()).  train=False disables the dropouts."""
        ops_ = self.flat.operands()
        w = ops_["w"]
        B, E, nf = edge_features.shape
        M = B * E
        C = w["feat.b"].numel()
        H = self.num_heads
        dh = C // H
        p = self.p if train else 0.0
        dev = edge_features.device
        ctx = TrainContext()
        s = ctx.t
        with torch.no_grad():
            self._feat_w8[:, :nf].copy_(w["feat.w"])
        feats = Fnn.pad(_f32c(edge_features).reshape(M, nf), (0, 8 - nf)).contiguous()
        fe = ops.linear(feats, self._feat_w8, w["feat.b"], mode="f32")
        h = ops.verifier_embed(fe, edge_indices.reshape(M, 2).to(torch.int64).contiguous(), self.module.edge_indices_pe.pe[0].contiguous())
        kv = _u8(edge_valids.reshape(B, E).bool())
        scale = 1.0 / math.sqrt(dh)
        layers = []
        for i in range(self.num_layers):
            lay: Dict[str, torch.Tensor] = {"x": h}
            lay["qkv"] = ops.linear(h, w[f"{i}.wqkv"], w[f"{i}.bqkv"])
            lay["att"], lay["lse"] = T.verifier_attn_fwd(lay["qkv"], kv, B, E, H, dh, scale, p, seed, site(i, 0))
            y = ops.gemm(lay["att"], w[f"{i}.wo"], M=M, N=C, K=C, lda=C, ldc=C, bias=w[f"{i}.bo"])
            lay["s1"], lay["x1"] = T.dropout_layernorm(y, h, p, seed, site(i, 1), gamma=w[f"{i}.g1"], beta=w[f"{i}.be1"])
            lay["z"] = ops.linear(lay["x1"], w[f"{i}.w1"], w[f"{i}.b1"])
            lay["u"] = T.verifier_gelu_dropout(lay["z"], p, seed, site(i, 2))
            F_ = lay["u"].shape[1]
            y = ops.gemm(lay["u"], w[f"{i}.w2"], M=M, N=C, K=F_, lda=F_, ldc=C, bias=w[f"{i}.b2"])
            lay["s2"], h = T.dropout_layernorm(y, lay["x1"], p, seed, site(i, 3), gamma=w[f"{i}.g2"], beta=w[f"{i}.be2"])
            layers.append(lay)
        s.update(dict(B=B, E=E, M=M, C=C, H=H, dh=dh, p=p, seed=seed, scale=scale, kv=kv, feats=feats, layers=layers, h6=h))
        g_head = torch.zeros(C + 1, dtype=torch.float32, device=dev)      # the head's dw | db of the fused loss, added in backward()
        amax = torch.empty(1, dtype=torch.float32, device=dev)
        if cls_gt is not None:
            target = _f32c(cls_gt).reshape(M)
            valid = _u8(edge_valids.reshape(M).bool())
            logits, loss, dlogit, dh6, stats = T.verifier_head_bce(h, w["out.w"], w["out.b"], target, valid, g_head[:C], g_head[C:],
                                                                   self._head_ws, neg_weight=NEG_WEIGHT, amax=amax)
            s.update(dict(loss=loss, stats=stats, dlogit=dlogit, dh6=dh6, g_head=g_head, amax=amax, n_valid=valid))
        else:
            logits, _, _, _, _ = T.verifier_head_bce(h, w["out.w"], w["out.b"], None, None, g_head[:C], g_head[C:], self._head_ws,
                                                     need_dh=False)
        return logits.view(B, E, 1), ctx

    # ------------------------------------------------------------------------------------------ backward
    def backward(self, ctx: TrainContext, *, dlogit: Optional[torch.Tensor] = None, grad_out: Optional[torch.Tensor] = None) -> None:
        """accumulate d(loss)/d(parameter) into the flat gradient buffer (= every parameter's .grad).  dlogit: an upstream gradient
        of the logits [B, E, 1]; without it, the gradient of the loss evaluated by forward(cls_gt=...), times grad_out (a device
        scalar, autograd's incoming gradient) when given"""
        self.flat.attach_grads()
        self.flat._clean = False
        ops_ = self.flat.operands()
        w, g = ops_["w"], ops_["g"]
        s = ctx.t
        B, E, M, C, H, dh, p, seed = s["B"], s["E"], s["M"], s["C"], s["H"], s["dh"], s["p"], s["seed"]
        if dlogit is not None:
            amax = torch.empty(1, dtype=torch.float32, device=w["out.b"].device)
            _, _, _, dh_, _ = T.verifier_head_bce(s["h6"], w["out.w"], w["out.b"], None, None, g["out.w"], g["out.b"], self._head_ws,
                                                  dlogit_in=_f32c(dlogit).reshape(M), amax=amax)
        else:
            if "dh6" not in s:
                raise RuntimeError("VerifierTrainEngine.backward: the forward evaluated no loss (cls_gt) and no dlogit was given")
            dh_, g_head, amax = s["dh6"], s["g_head"], s["amax"]
            if grad_out is not None:
                go = grad_out.reshape(1).to(torch.float32)
                dh_.mul_(go)                                   # chain rule of autograd's incoming gradient (on the device)
                g_head.mul_(go)
                amax = amax * go.abs()
            g["out.w"].add_(g_head[:C])
            g["out.b"].add_(g_head[C:])
        self._update_grad_scale(dh_, amax)
        G = self.grad_scale

        def lin_bwd(dy, x, gw, gb):
            T.grad_weight(dy, x, gw, g_scale=G, db=gb)

        def dx_into(dy, wpw, out):
            """out += dy . W  (out already holds the residual gradient)"""
            N_out, K_in = wpw.f32.shape
            T.gemm_grad(dy, wpw.f32, out, M=dy.shape[0], N=K_in, K=N_out, lda=dy.stride(0), ldw=wpw.f32.stride(0), ldc=out.stride(0),
                        w_kmajor=True, a_scale=G, accumulate=True, split_k=1)

        for i in reversed(range(self.num_layers)):
            lay = s["layers"][i]
            # ---- norm2 / dropout2 / linear2 (post-norm: the residual gradient is the LayerNorm's input gradient)
            ds2 = torch.zeros_like(dh_)
            dy2 = T.layernorm_bwd(lay["s2"], dh_, ds2, gamma=w[f"{i}.g2"], group_rows=32, dmult=g[f"{i}.g2"], dadd=g[f"{i}.be2"],
                                  ld_d=0, drop=(p, seed, site(i, 3)))
            lin_bwd(dy2, lay["u"], g[f"{i}.w2"], g[f"{i}.b2"])
            du = T.grad_input(dy2, w[f"{i}.w2"].f32, g_scale=G)
            dz = T.verifier_gelu_dropout_bwd(lay["z"], du, p, seed, site(i, 2), out=du if du.shape == lay["z"].shape else None)
            lin_bwd(dz, lay["x1"], g[f"{i}.w1"], g[f"{i}.b1"])
            dx_into(dz, w[f"{i}.w1"], ds2)                     # d x1 = residual + feed-forward path
            del dz, du
            # ---- norm1 / dropout1 / out-projection / attention / in-projection
            ds1 = torch.zeros_like(dh_)
            dy1 = T.layernorm_bwd(lay["s1"], ds2, ds1, gamma=w[f"{i}.g1"], group_rows=32, dmult=g[f"{i}.g1"], dadd=g[f"{i}.be1"],
                                  ld_d=0, drop=(p, seed, site(i, 1)))
            lin_bwd(dy1, lay["att"], g[f"{i}.wo"], g[f"{i}.bo"])
            datt = T.grad_input(dy1, w[f"{i}.wo"].f32, g_scale=G)
            dqkv = T.verifier_attn_bwd(lay["qkv"], lay["att"], datt, lay["lse"], s["kv"], B, E, H, dh, s["scale"], p, seed, site(i, 0))
            lin_bwd(dqkv, lay["x"], g[f"{i}.wqkv"], g[f"{i}.bqkv"])
            dx_into(dqkv, w[f"{i}.wqkv"], ds1)                 # d x = residual + attention path
            dh_ = ds1
        # ---- embedding: h0 = feats W_e^T + b_e + pe[edge_indices] (pe is a buffer)
        nf = g["feat.w"].shape[1]
        dwe = torch.zeros_like(self._feat_w8)
        T.grad_weight(dh_, s["feats"], dwe, g_scale=G, db=g["feat.b"])
        g["feat.w"].add_(dwe[:, :nf])
        ctx.t = {}

    # ------------------------------------------------------------------------------------------ optimizer
    def optimizer_step(self, *, lr: float = 2e-4, betas=(0.95, 0.999), eps: float = 1e-8, weight_decay: float = 1e-6,
                       zero_grad: bool = False) -> None:
        """one guarded AdamW launch over the flat buffer (configure_optimizers, verifier.py:100-107)"""
        self.step_count += 1
        f = self.flat
        T.adamw(f.params, f.grads, f.exp_avg, f.exp_avg_sq, lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps),
                weight_decay=float(weight_decay), step=self.step_count, hi=f.hi, lo=f.lo, g_scale=1.0, zero_grad=zero_grad,
                overflow=self._overflow)
        f._clean = bool(zero_grad)
        self._after_step_overflow()
        f._seen_version = f._versions()
        cache = getattr(self.module, "_cache", None)
        if cache is not None:
            cache._key = None            # the eval-mode packing of the module is stale now (the kernel bumps no version counter)

    # ------------------------------------------------------------------------------------------ whole step
    def loss_and_grads(self, edge_features, edge_indices, edge_valids, cls_gt, *, seed: int = 0, train: bool = True):
        """forward + Verifier._loss + backward; -> (loss [1], stats int32 [4] = (tp, fp, tn, fn), logits [B, E, 1])"""
        logits, ctx = self.forward(edge_features, edge_indices, edge_valids, seed=seed, train=train, cls_gt=cls_gt)
        loss, stats = ctx.t["loss"], ctx.t["stats"]
        self.backward(ctx)
        return loss, stats, logits


def binary_metrics(stats: torch.Tensor) -> Dict[str, torch.Tensor]:
    """torchmetrics' binary accuracy / precision / recall / F1 (task="binary", threshold on the already-thresholded prediction)
    from the confusion counts (tp, fp, tn, fn), on the device; a zero denominator gives 0:
        acc = (tp + tn) / (tp + fp + tn + fn)   precision = tp / (tp + fp)   recall = tp / (tp + fn)
        f1 = 2 tp / (2 tp + fp + fn)"""
    tp, fp, tn, fn = stats.to(torch.float32).unbind(0)

    def div(a, b):
        return torch.where(b > 0, a / torch.clamp(b, min=1.0), torch.zeros_like(a))

    return {"cls_acc": div(tp + tn, tp + fp + tn + fn), "cls_precision": div(tp, tp + fp), "cls_recall": div(tp, tp + fn),
            "cls_f1_score": div(2 * tp, 2 * tp + fp + fn)}
