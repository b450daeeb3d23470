"""Training step of the VQ-VAE (stage 1: vqvae/model/fracture_ae.py) on the HIP kernels.

Reference: FractureAE.training_step (fracture_ae.py:43-58) around VQVAE.forward / loss (vq_vae.py:24-50, 75-89) and PN2.forward /
loss (pn2.py:31-56, 83-97) with the modules in .train(): BatchNorm2d on batch statistics over all F*S*ns rows of a layer
(running statistics updated once per step), the quantizer's straight-through estimator and commitment loss (quantizer.py:45-67),
and chamferdist's bidirectional Chamfer distance.

Forward (what the backward keeps, in brackets):
    per level: FPS + ball query [ball] -> grouped rows (pfpp_group_gather) -> 3 x [y_i = conv_i(h_{i-1}) [y_i], batch mean / var
    [mean_i, var_i], h_i = relu(BN(y_i))] -> max over the neighbourhood
    conv6 [level-3 output] -> z_e -> codes (pfpp_vq_encode) [codes] -> decoder fc1 / relu / fc2 / relu / fc3 [pre-activations]
Backward: decoder and conv6 by the gradient GEMMs (pfpp_gemm_grad, bias sums through its colsum) and pfpp_act_bwd; the quantizer by
pfpp_vq_train; each level from its last layer down: pfpp_sa_pool_bwd (the row that attains the max), pfpp_bn_relu_bwd (two passes
over the rows), weight gradient dy^T h_{i-1} with h_{i-1} rebuilt by pfpp_bn_apply, dX = dy W; the first layer's rows are rebuilt
by pfpp_group_gather and the feature columns of its dX go back to the previous level's points through pfpp_group_gather_bwd.

Parameters, gradients, Adam moments and split-f16 planes live in one flat buffer (ModuleFlat: the FlatParams layout rules with the
module's registration order); the module's nn.Parameters are views of it.  The gradient GEMMs lift their dY operand by a power of
two per site (the denoiser engine's rule, measured two backward passes late; synchronously in the first two) so small Chamfer
gradients do not underflow fp16; AdamW skips and flags non-finite gradients and the scales back off (the denoiser's guard).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib, ops
from . import train_ops as T
from ._lib import check
from .encoder import SA_LEVELS
from .ops import _chk, _ptr, _stream
from .packing import PW, pack_sa_first, round_up
from .train import DenoiserTrainEngine, FlatParams, TrainContext, _f32c, _pw_view

_f32 = torch.float32
MAX_FRAGMENTS = 2048          # batch statistics need all fragments of a step in one pass (as the train-mode encode)


# ------------------------------------------------------------------------------------------------ tensor-level wrappers
def chamfer_fwd(off: torch.Tensor, ctr: Optional[torch.Tensor], tgt: torch.Tensor):
    """off [F, n, 3] (+ ctr [F, n / rep, 3] broadcast over rep consecutive points), tgt [F, m, 3] -> (d_src [F, n], i_src int32 [F, n],
    d_tgt [F, m], i_tgt int32 [F, m]): squared distance to, and index of, the nearest point of the other cloud (pfpp_chamfer_fwd)"""
    _chk(off, _f32, "off"); _chk(tgt, _f32, "tgt")
    F, n, _ = off.shape
    m = tgt.shape[1]
    rep = 1
    if ctr is not None:
        _chk(ctr, _f32, "ctr")
        if ctr.shape[0] != F or n % ctr.shape[1] != 0:
            raise ValueError("chamfer_fwd: ctr must be [F, n / rep, 3]")
        rep = n // ctr.shape[1]
    if tgt.shape[0] != F or tgt.shape[2] != 3 or off.shape[2] != 3:
        raise ValueError("chamfer_fwd: off [F, n, 3] and tgt [F, m, 3] expected")
    dev = off.device
    d_src = torch.empty((F, n), dtype=_f32, device=dev)
    i_src = torch.empty((F, n), dtype=torch.int32, device=dev)
    d_tgt = torch.empty((F, m), dtype=_f32, device=dev)
    i_tgt = torch.empty((F, m), dtype=torch.int32, device=dev)
    check(_lib.load().pfpp_chamfer_fwd(_ptr(off), _ptr(ctr), rep, _ptr(tgt), _ptr(d_src), _ptr(i_src), _ptr(d_tgt), _ptr(i_tgt), F, n, m,
                                       _stream()), "pfpp_chamfer_fwd")
    return d_src, i_src, d_tgt, i_tgt


def chamfer_reduce(d_src: torch.Tensor, d_tgt: torch.Tensor, scale: float) -> torch.Tensor:
    """scale * (sum d_src + sum d_tgt) -> [1]"""
    out = torch.empty(1, dtype=_f32, device=d_src.device)
    check(_lib.load().pfpp_chamfer_reduce(_ptr(d_src), d_src.numel(), _ptr(d_tgt), d_tgt.numel(), float(scale), _ptr(out), _stream()),
          "pfpp_chamfer_reduce")
    return out


def chamfer_bwd(off, ctr, tgt, i_src, i_tgt, scale: float, gscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d loss / d off [F, n, 3] of loss = scale * (sum d_src + sum d_tgt), times gscale[0] (device scalar) when given"""
    F, n, _ = off.shape
    m = tgt.shape[1]
    rep = n // ctr.shape[1] if ctr is not None else 1
    grad = torch.empty_like(off)
    if gscale is not None:
        gscale = _f32c(gscale.reshape(1))
    check(_lib.load().pfpp_chamfer_bwd(_ptr(off), _ptr(ctr), rep, _ptr(tgt), _ptr(i_src), _ptr(i_tgt), _ptr(grad), F, n, m,
                                       float(scale), _ptr(gscale), _stream()), "pfpp_chamfer_bwd")
    return grad


def vq_train(z: torch.Tensor, codebook: torch.Tensor, codes: torch.Tensor, beta: float, *, g_emb: Optional[torch.Tensor] = None,
             grads: bool = False):
    """z [R, D], codes int32 [R] -> (out [2] = (embedding_loss, perplexity), dz [R, D] or None, dcodebook [K, D] or None)"""
    _chk(z, _f32, "z"); _chk(codebook, _f32, "codebook"); _chk(codes, torch.int32, "codes")
    R, D = z.shape
    K = codebook.shape[0]
    lib = _lib.load()
    ws = torch.empty(int(lib.pfpp_vq_train_workspace(R, K)), dtype=torch.uint8, device=z.device)
    out = torch.empty(2, dtype=_f32, device=z.device)
    dz = torch.empty_like(z) if grads else None
    dcb = torch.empty_like(codebook) if grads else None
    if g_emb is not None:
        g_emb = _f32c(g_emb.reshape(1))
    check(lib.pfpp_vq_train(_ptr(z), _ptr(codebook), _ptr(codes), R, K, D, float(beta), _ptr(g_emb), _ptr(dz), _ptr(dcb), _ptr(out), _ptr(ws),
                            _stream()), "pfpp_vq_train")
    return out, dz, dcb


def sa_pool_bwd(y: torch.Tensor, pool: int, mean, var, gamma, beta, dout: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """dout [rows / pool, C] -> dh [rows, C] routed to the row that attains max_p relu(BN(y_p)) (pfpp_sa_pool_bwd)"""
    _chk(y, _f32, "y"); _chk(dout, _f32, "dout")
    rows, C = y.shape
    dh = torch.empty((rows, C), dtype=_f32, device=y.device)
    check(_lib.load().pfpp_sa_pool_bwd(_ptr(y), rows // pool, pool, C, y.stride(0), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta),
                                       float(eps), _ptr(dout), _ptr(dh), _stream()), "pfpp_sa_pool_bwd")
    return dh


def bn_relu_bwd(y: torch.Tensor, dh: torch.Tensor, mean, var, gamma, beta, dgamma: Optional[torch.Tensor], dbeta: Optional[torch.Tensor],
                eps: float = 1e-5, out: Optional[torch.Tensor] = None, amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """backward of relu(BatchNorm_train(y)): -> dy [rows, C] (into `out`, which may be dh); dgamma / dbeta += ; amax (fp32 [1] on the
    device, optional) <- max |dy| from the same pass (pfpp_bn_relu_bwd)"""
    _chk(y, _f32, "y"); _chk(dh, _f32, "dh")
    rows, C = y.shape
    lib = _lib.load()
    ws = torch.empty(int(lib.pfpp_bn_relu_bwd_workspace(rows, C)), dtype=torch.uint8, device=y.device)
    dy = torch.empty_like(dh) if out is None else out
    check(lib.pfpp_bn_relu_bwd(_ptr(y), _ptr(dh), rows, C, y.stride(0), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), float(eps),
                               _ptr(dgamma), _ptr(dbeta), _ptr(dy), _ptr(amax), _ptr(ws), _stream()), "pfpp_bn_relu_bwd")
    return dy


def group_gather_bwd(dA: torch.Tensor, idx: torch.Tensor, N: int, D: int) -> torch.Tensor:
    """dA [F*S*ns, >= D] (feature columns first, pfpp_group_gather's layout), idx int32 [F, S, ns] -> dfeats [F, N, D]"""
    _chk(dA, _f32, "dA"); _chk(idx, torch.int32, "idx")
    F, S, ns = idx.shape
    out = torch.empty((F, N, D), dtype=_f32, device=dA.device)
    check(_lib.load().pfpp_group_gather_bwd(_ptr(dA), dA.stride(0), _ptr(idx), _ptr(out), F, N, S, ns, D, _stream()),
          "pfpp_group_gather_bwd")
    return out


# ------------------------------------------------------------------------------------------------ autograd nodes
class _ChamferFn(torch.autograd.Function):
    """chamferdist.ChamferDistance(off + ctr, tgt, bidirectional=True) (sum over points, mean over clouds); gradient to `off` only"""

    @staticmethod
    def forward(ctx, off, ctr, tgt):
        d_src, i_src, d_tgt, i_tgt = chamfer_fwd(off, ctr, tgt)
        F = off.shape[0]
        loss = chamfer_reduce(d_src, d_tgt, 1.0 / F).reshape(())
        ctx.save_for_backward(off, ctr, tgt, i_src, i_tgt)
        return loss

    @staticmethod
    def backward(ctx, g):
        off, ctr, tgt, i_src, i_tgt = ctx.saved_tensors
        return chamfer_bwd(off, ctr, tgt, i_src, i_tgt, 1.0 / off.shape[0], gscale=g), None, None


def chamfer_loss(pc_offset: torch.Tensor, xyz: torch.Tensor, part_pcs: torch.Tensor, n_pts: int = 1000) -> torch.Tensor:
    """PN2.loss / VQVAE.loss's cd_loss (pn2.py:83-97): r = (pc_offset + xyz[:, :, None]).reshape(-1, n_pts, 3) against part_pcs"""
    F, L, P, _ = pc_offset.shape
    if L * P != n_pts:
        raise ValueError(f"chamfer_loss: the reconstruction has {L} x {P} points per fragment, the reference reshapes to {n_pts}")
    if part_pcs.shape[0] != F:
        raise ValueError("chamfer_loss: one target cloud per reconstructed fragment expected")
    return _ChamferFn.apply(_f32c(pc_offset).view(F, L * P, 3), _f32c(xyz.detach()), _f32c(part_pcs.detach()))


class _TrainFn(torch.autograd.Function):
    """VQVAE.forward / PN2.forward in train mode as one autograd node: (embedding_loss, pc_offset, z_q, perplexity, xyz); its backward
    takes the gradients of embedding_loss, pc_offset and z_q and accumulates the parameters' .grad (views of the flat buffer)"""

    @staticmethod
    def forward(ctx, eng, part_pcs, grad_anchor):
        out, saved = eng.forward(part_pcs)
        ctx.eng, ctx.saved = eng, saved
        ctx.mark_non_differentiable(out["perplexity"], out["xyz"])
        return out["embedding_loss"], out["pc_offset"], out["z_q"], out["perplexity"], out["xyz"]

    @staticmethod
    def backward(ctx, g_emb, g_off, g_zq, _g_perp, _g_xyz):
        ctx.eng.backward(ctx.saved, g_emb=g_emb, g_off=g_off, g_zq=g_zq)
        ctx.saved = None
        return None, None, None


# ------------------------------------------------------------------------------------------------ flat parameter buffer
class ModuleFlat(FlatParams):
    """flat storage of a module's parameters (registration order), gradients, Adam moments and split-f16 planes"""

    def __init__(self, module: torch.nn.Module):          # noqa: super().__init__ is the denoiser's layout
        named = dict(module.named_parameters())
        self.module = module
        self.order = list(named)
        dev = next(module.parameters()).device
        if dev.type != "cuda":
            raise ValueError("ModuleFlat: the module must live on the GPU (there is no CPU training path)")
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
        self.refresh_planes()

    def check_storage(self) -> None:
        first = self.named[self.order[0]]
        if first.data_ptr() != self.params.data_ptr():
            raise RuntimeError("ModuleFlat: the module's parameters were re-allocated (.to()/.cuda() after the training engine was "
                               "created); build the engine after moving the module")
        if self._versions() != self._seen_version:
            self.refresh_planes()         # load_state_dict / in-place edits of the parameters through torch

    def weight(self, name: str, shape) -> PW:
        """a GEMM weight [N, K] (K % 8 == 0) read from the flat buffer and its split planes"""
        return _pw_view(*(self.view(f, name, shape) for f in (self.params, self.hi, self.lo)))

    def after_optimizer_step(self) -> None:
        pass


# ------------------------------------------------------------------------------------------------ engine
class VQVAETrainEngine:
    """train-mode forward / backward / optimizer step of a VQVAE (or of a PN2 used as the autoencoder, ae_name = PN2) on the HIP
    kernels"""

    _after_step_overflow = DenoiserTrainEngine._after_step_overflow
    _apply_backoff = DenoiserTrainEngine._apply_backoff

    def __init__(self, module: torch.nn.Module):
        self.module = module
        self.pn2 = module.pn2 if hasattr(module, "pn2") else module
        self.vq = getattr(module, "vector_quantization", None)
        self.prefix = "pn2." if self.pn2 is not module else ""
        self.flat = ModuleFlat(module)
        self.step_count = 0
        dev = self.flat.params.device
        self._overflow = torch.zeros(2, dtype=torch.int32, device=dev)
        self._ovf_ring = None
        self._backoff = 1.0
        self._clean_steps = 0
        self.overflow_steps = 0
        self._dyn_gscale = True
        self._rings: Dict[str, list] = {}
        self._n_backward = 0
        self._amax = torch.zeros(1, dtype=torch.float32, device=dev)       # max |dy| of the BatchNorm backward's second pass

    # -------------------------------------------------------------------------------- FusedAdamW protocol
    def tables_state_changed(self) -> None:
        """(FusedAdamW.load_state_dict hook: no sparse tables here)"""

    def arm_optimizer(self, **_hp) -> None:
        """no optimizer-in-backward here: FusedAdamW.step() does the whole update"""

    def optimizer_step(self, *, lr: float = 5e-4, betas=(0.95, 0.999), eps: float = 1e-8, weight_decay: float = 1e-6,
                       zero_grad: bool = False) -> None:
        """one guarded AdamW launch over the flat buffer (configure_optimizers, fracture_ae.py:82-91).  Every parameter of the module
        takes the step, whatever its requires_grad (torch.optim.AdamW skips a parameter whose .grad is None); the reference's stage 1
        freezes nothing, and a frozen parameter's zero gradient still gives it the weight decay here"""
        self.step_count += 1
        f = self.flat
        T.adamw(f.params, f.grads, f.exp_avg, f.exp_avg_sq, lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps),
                weight_decay=float(weight_decay), step=self.step_count, hi=f.hi, lo=f.lo, g_scale=1.0, zero_grad=zero_grad,
                overflow=self._overflow)
        f._clean = bool(zero_grad)
        self._after_step_overflow()
        f._seen_version = f._versions()
        self.invalidate_packs()

    def invalidate_packs(self) -> None:
        """the packed weights of the eval / frozen-train encoder paths are stale after an update of the parameters or of the running
        statistics (the kernels bump no version counter)"""
        for mod in self.module.modules():
            for attr in ("_cache", "_cache_train", "_train_cache"):
                c = getattr(mod, attr, None)
                if c is not None and hasattr(c, "_key"):
                    c._key = None

    # -------------------------------------------------------------------------------- gradient scale per site
    def _scale(self, site: str, t: Optional[torch.Tensor] = None, amax_dev: Optional[torch.Tensor] = None) -> float:
        """power of two that lifts max |t| to [8, 16) for the fp16 planes of the gradient GEMMs: from the same site two backward
        passes ago (no stall), read at once in the first two.  amax_dev: max |t| already on the device (the BatchNorm backward takes
        it in its second pass); otherwise a reduction over t (no temporary of t's size)"""
        ring = self._rings.get(site)
        if ring is None:
            ring = self._rings[site] = [[torch.zeros(1, pin_memory=True), torch.cuda.Event(), False] for _ in range(2)]
        slot = ring[self._n_backward % 2]
        if amax_dev is None:
            amax_dev = torch.linalg.vector_norm(t.detach(), float("inf")).reshape(1)
        if slot[2]:
            slot[1].synchronize()
            amax = float(slot[0][0])
        else:
            amax = float(amax_dev)
        slot[0].copy_(amax_dev, non_blocking=True)
        slot[1].record()
        slot[2] = True
        if not (math.isfinite(amax) and amax > 0.0):
            return 1.0
        return max(1.0, float(2.0 ** min(40, max(0, 3 - math.floor(math.log2(amax))))) * self._backoff)

    # -------------------------------------------------------------------------------- forward
    def _sa_weights(self, name: str, D: int):
        f = self.flat
        p = f"{self.prefix}{name}"
        ws = []
        for i in range(3):
            full = f.named[f"{p}.mlp_convs.{i}.weight"]
            w2 = f.view(f.params, f"{p}.mlp_convs.{i}.weight", (full.shape[0], full.shape[1]))
            ws.append(PW(pack_sa_first(w2.detach(), D).contiguous(), prescale=False) if i == 0
                      else f.weight(f"{p}.mlp_convs.{i}.weight", (full.shape[0], full.shape[1])))
        return ws

    def level_forward(self, name: str, S: int, radius: float, nsample: int, xyz: torch.Tensor, feats: Optional[torch.Tensor]):
        """one set-abstraction level in train mode (pn2_utils.py:190-216): xyz [F, N, 3], feats [F, N, D] or None -> the level's
        context (sampling indices, raw conv outputs y_i with their batch mean / variance, output "out" [F, S, C3], "new_xyz")"""
        f = self.flat
        F = xyz.shape[0]
        sa = getattr(self.pn2, name)
        ops.check_fps_ratio(S, xyz.shape[1])
        _, new_xyz = ops.fps(xyz, S)
        ball = ops.ball_query(xyz, new_xyz, radius, nsample)
        feats = None if feats is None else _f32c(feats)
        D = 0 if feats is None else feats.shape[2]
        ws = self._sa_weights(name, D)
        h = ops.group_gather(xyz, new_xyz, feats, ball)
        lv = {"xyz": xyz, "new_xyz": new_xyz, "feats": feats, "ball": ball, "ws": ws, "ns": nsample, "D": D, "sa": sa, "name": name,
              "y": [], "mean": [], "var": []}
        for i in range(3):
            bn = sa.mlp_bns[i]
            y = ops.linear(h, ws[i], f.view(f.params, f"{self.prefix}{name}.mlp_convs.{i}.bias"))
            mean, var = T.bn_stats(y, bn.running_mean, bn.running_var, momentum=0.1)
            h = T.bn_apply(y, mean, var, bn.weight.detach(), bn.bias.detach(), eps=bn.eps, pool=nsample if i == 2 else 0)
            lv["y"].append(y); lv["mean"].append(mean); lv["var"].append(var)
        torch._foreach_add_([sa.mlp_bns[i].num_batches_tracked for i in range(3)], 1)
        lv["out"] = h.view(F, S, -1)
        return lv

    def forward(self, part_pcs: torch.Tensor):
        """part_pcs [F, N, 3] (the valid fragments) -> (outputs, context); BatchNorm on batch statistics with the running statistics
        updated, as the reference's modules in .train() do"""
        pts = _f32c(part_pcs)
        F, N, _ = pts.shape
        num_point = self.pn2.num_point
        if F > MAX_FRAGMENTS:
            raise ValueError(f"VQ-VAE training step: batch statistics need all fragments in one pass (F <= {MAX_FRAGMENTS}, got {F})")
        n_dec = self.pn2.local_decode_pts
        if N != num_point * n_dec:
            raise ValueError(f"VQ-VAE training step: fragments of {N} points; the decoder reconstructs {num_point} x {n_dec}")
        self.flat.check_storage()
        f = self.flat
        dev = pts.device
        s: Dict[str, object] = {"F": F}
        xyz, feats = pts, None
        levels = []
        for name, npoint, radius, nsample in SA_LEVELS:
            lv = self.level_forward(name, npoint or num_point, radius, nsample, xyz, feats)
            feats, xyz = lv["out"], lv["new_xyz"]
            levels.append(lv)
        s["levels"] = levels
        self.invalidate_packs()           # the running statistics changed under the eval-mode packing
        C3 = feats.shape[2]
        w6 = f.weight(f"{self.prefix}conv6.weight", (self.pn2.num_dim, C3))
        z_e = ops.linear(feats.view(F * num_point, C3), w6, f.view(f.params, f"{self.prefix}conv6.bias"))
        s["w6"] = w6
        out: Dict[str, torch.Tensor] = {"xyz": xyz}
        if self.vq is not None:
            cb = f.view(f.params, "vector_quantization.embedding.weight")
            slot = torch.arange(F, dtype=torch.int32, device=dev)
            z_q, codes = ops.vq_encode(z_e.view(F, num_point, -1), cb, slot, F, return_codes=True)
            e_dim = self.vq.e_dim
            vals, _, _ = vq_train(z_e.view(-1, e_dim), cb, codes.reshape(-1), self.vq.beta)
            out["embedding_loss"] = vals[0].reshape(())
            out["perplexity"] = vals[1].reshape(())
            s["codes"] = codes.reshape(-1)
            z_dec = z_q.view(F * num_point, -1)
        else:
            z_dec = z_e
            out["embedding_loss"] = torch.zeros((), dtype=_f32, device=dev)
            out["perplexity"] = torch.zeros((), dtype=_f32, device=dev)
        s["z_e"] = z_e
        # decoder (pn2.py:71-81): fc3(relu(fc2(relu(fc1(z_q)))))
        p = self.prefix
        wf = [f.weight(f"{p}fc{k}.weight", f.named[f"{p}fc{k}.weight"].shape) for k in (1, 2, 3)]
        a1 = ops.linear(z_dec, wf[0], f.view(f.params, f"{p}fc1.bias"))
        h1 = T.act(a1, "relu")
        a2 = ops.linear(h1, wf[1], f.view(f.params, f"{p}fc2.bias"))
        h2 = T.act(a2, "relu")
        off = ops.linear(h2, wf[2], f.view(f.params, f"{p}fc3.bias"))
        s.update(dict(wf=wf, a1=a1, h1=h1, a2=a2, h2=h2, z_dec=z_dec))
        out["pc_offset"] = off.view(F, num_point, n_dec, 3)
        out["z_q"] = z_dec.view(F, num_point, -1)
        out["z_e"] = z_e.view(F, num_point, -1)
        ctx = TrainContext()
        ctx.t = s
        return out, ctx

    # -------------------------------------------------------------------------------- backward
    def backward(self, ctx: TrainContext, *, g_emb: Optional[torch.Tensor] = None, g_off: Optional[torch.Tensor] = None,
                 g_zq: Optional[torch.Tensor] = None) -> None:
        """accumulate d(loss)/d(parameter) into the flat gradient buffer (= every parameter's .grad) from the gradients of
        embedding_loss (device scalar), pc_offset [F, L, P, 3] and z_q [F, L, C] (each may be None)"""
        f = self.flat
        f.attach_grads()
        f._clean = False
        s = ctx.t
        F = s["F"]
        p = self.prefix
        gv = lambda name, shape=None: f.view(f.grads, name, shape)
        wf = s["wf"]
        rows_dec = s["z_dec"].shape[0]
        dz = torch.zeros((rows_dec, s["z_dec"].shape[1]), dtype=_f32, device=f.params.device)
        if g_off is not None:
            d_off = _f32c(g_off).view(rows_dec, -1)
            G = self._scale("fc3", d_off)
            T.grad_weight(d_off, s["h2"], gv(f"{p}fc3.weight"), g_scale=G, db=gv(f"{p}fc3.bias"))
            dh2 = T.grad_input(d_off, wf[2].f32, g_scale=G)
            da2 = T.act_bwd(s["a2"], dh2, "relu")
            G = self._scale("fc2", da2)
            T.grad_weight(da2, s["h1"], gv(f"{p}fc2.weight"), g_scale=G, db=gv(f"{p}fc2.bias"))
            dh1 = T.grad_input(da2, wf[1].f32, g_scale=G)
            da1 = T.act_bwd(s["a1"], dh1, "relu")
            G = self._scale("fc1", da1)
            T.grad_weight(da1, s["z_dec"], gv(f"{p}fc1.weight"), g_scale=G, db=gv(f"{p}fc1.bias"))
            dz = T.grad_input(da1, wf[0].f32, g_scale=G)
        if g_zq is not None:
            dz = dz + _f32c(g_zq).view(rows_dec, -1)
        if self.vq is not None and g_emb is not None:
            e_dim = self.vq.e_dim
            cb = f.view(f.params, "vector_quantization.embedding.weight")
            _, dz_vq, dcb = vq_train(s["z_e"].view(-1, e_dim), cb, s["codes"], self.vq.beta, g_emb=g_emb, grads=True)
            dz = dz + dz_vq.view(rows_dec, -1)
            gv("vector_quantization.embedding.weight").add_(dcb)
        # conv6 (pn2.py:29)
        lv3 = s["levels"][-1]
        feats3 = lv3["out"].view(rows_dec, -1)
        G = self._scale("conv6", dz)
        C3 = feats3.shape[1]
        T.grad_weight(dz, feats3, gv(f"{p}conv6.weight", (dz.shape[1], C3)), g_scale=G, db=gv(f"{p}conv6.bias"))
        dfeat = T.grad_input(dz, s["w6"].f32, g_scale=G)
        for lv in reversed(s["levels"]):
            dfeat = self.level_backward(lv, dfeat)
        self._n_backward += 1
        ctx.t = {}

    def level_backward(self, lv, dout: torch.Tensor) -> Optional[torch.Tensor]:
        """one set-abstraction level: d(output) [F*S, C3] -> d(input features) [F, N, D] (None for the first level)"""
        f = self.flat
        name, sa, ws, ns, D = lv["name"], lv["sa"], lv["ws"], lv["ns"], lv["D"]
        pre = f"{self.prefix}{name}"
        gv = lambda n, shape=None: f.view(f.grads, n, shape)
        bns = sa.mlp_bns
        dh = sa_pool_bwd(lv["y"][2], ns, lv["mean"][2], lv["var"][2], bns[2].weight.detach(), bns[2].bias.detach(), _f32c(dout).view(-1, ws[2].N),
                         eps=bns[2].eps)
        for i in (2, 1, 0):
            bn = bns[i]
            dy = bn_relu_bwd(lv["y"][i], dh, lv["mean"][i], lv["var"][i], bn.weight.detach(), bn.bias.detach(), gv(f"{pre}.mlp_bns.{i}.weight"),
                             gv(f"{pre}.mlp_bns.{i}.bias"), eps=bn.eps, out=dh, amax=self._amax)
            G = self._scale(f"{name}.{i}", amax_dev=self._amax)
            if i > 0:
                pb = bns[i - 1]
                h_prev = T.bn_apply(lv["y"][i - 1], lv["mean"][i - 1], lv["var"][i - 1], pb.weight.detach(), pb.bias.detach(), eps=pb.eps)
                T.grad_weight(dy, h_prev, gv(f"{pre}.mlp_convs.{i}.weight", (ws[i].N, ws[i].K)), g_scale=G,
                              db=gv(f"{pre}.mlp_convs.{i}.bias"))
                del h_prev
                dh = T.grad_input(dy, ws[i].f32, g_scale=G)
                continue
            # first layer: rows [feats | rel_xyz | 0] rebuilt by the grouping kernel; its weight gradient back in the reference's
            # column order [rel_xyz | feats] (pn2_utils.py:146)
            A = ops.group_gather(lv["xyz"], lv["new_xyz"], lv["feats"], lv["ball"])
            dwp = torch.zeros((ws[0].N, D + 4), dtype=_f32, device=dy.device)
            T.grad_weight(dy, A, dwp, g_scale=G, db=gv(f"{pre}.mlp_convs.0.bias"))
            del A
            gw = gv(f"{pre}.mlp_convs.0.weight", (ws[0].N, D + 3))
            gw[:, :3] += dwp[:, D:D + 3]
            if D:
                gw[:, 3:] += dwp[:, :D]
            if lv["feats"] is None:
                return None
            dA = T.grad_input(dy, ws[0].f32, g_scale=G)
            return group_gather_bwd(dA, lv["ball"], lv["xyz"].shape[1], D)
        return None
