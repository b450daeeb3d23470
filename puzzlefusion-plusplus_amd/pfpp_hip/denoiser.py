"""DenoiserTransformer forward on the HIP kernels.

Host orchestration only.  Per layer: AdaLN (LN kernel with the (scale, shift) of the batched
AdaLN GEMM) -> packed QKV GEMM -> block-diagonal self-attention in one kernel (the [B,T,T]
mask of the reference is never built) -> out-projection GEMM with bias+residual epilogue ->
AdaLN -> QKV GEMM -> per-(puzzle, head) QK^T GEMM, key-masked softmax, P.V GEMM ->
out-projection (+bias, +residual) -> LN -> GEGLU GEMM (gate fused in the epilogue) ->
down-projection (+bias, +residual).
"""
from __future__ import annotations

import dataclasses
import enum
import math
from typing import Dict, Optional

import torch

from . import ops
from .packing import PW, pack_geglu, round_up


def pack_denoiser(sd: Dict[str, torch.Tensor], num_layers: int) -> Dict[str, torch.Tensor]:
    """sd: live tensors of a DenoiserTransformer keyed by state_dict names"""
    pk: Dict[str, torch.Tensor] = {}
    pk["shape.w"] = PW(sd["shape_embedding.weight"])
    pk["shape.b"] = sd["shape_embedding.bias"].contiguous()
    pk["param.w"] = PW(sd["param_fc.weight"])
    pk["param.b"] = sd["param_fc.bias"].contiguous()
    pk["ref_emb"] = sd["ref_part_emb.weight"].contiguous()
    # both embedding layers as ONE weight for the few-token kernel (csrc/embed_small.hip): [W_shape (148) | W_param (147) | 0] [C, 320]
    ws, wp = sd["shape_embedding.weight"], sd["param_fc.weight"]
    if ws.shape[1] == 148 and wp.shape[1] == 147:
        wc = ws.new_zeros((ws.shape[0], 320))
        wc[:, :148] = ws
        wc[:, 148:295] = wp
        pk["embed.w"] = PW(wc)
        pk["embed.b"] = (sd["shape_embedding.bias"] + sd["param_fc.bias"]).contiguous()
    pk["pe"] = sd["pos_encoding.pe"][0].contiguous()
    tabs, lw, lb = [], [], []
    for i in range(num_layers):
        p = f"transformer_layers.{i}"
        for n in ("norm1", "norm2"):
            tabs.append(sd[f"{p}.{n}.emb.weight"])
            lw.append(sd[f"{p}.{n}.linear.weight"])
            lb.append(sd[f"{p}.{n}.linear.bias"])
        for a in ("self_attn", "global_attn"):
            pk[f"{i}.{a}.wqkv"] = PW(torch.cat(
                [sd[f"{p}.{a}.to_q.weight"], sd[f"{p}.{a}.to_k.weight"], sd[f"{p}.{a}.to_v.weight"]], dim=0
            ).contiguous())
            pk[f"{i}.{a}.wo"] = PW(sd[f"{p}.{a}.to_out.0.weight"].contiguous())
            pk[f"{i}.{a}.bo"] = sd[f"{p}.{a}.to_out.0.bias"].contiguous()
        pk[f"{i}.norm3.g"] = sd[f"{p}.norm3.weight"].contiguous()
        pk[f"{i}.norm3.b"] = sd[f"{p}.norm3.bias"].contiguous()
        w1, pk[f"{i}.ff.b1"] = pack_geglu(sd[f"{p}.ff.net.0.proj.weight"], sd[f"{p}.ff.net.0.proj.bias"])
        pk[f"{i}.ff.w1"] = PW(w1)
        pk[f"{i}.ff.w2"] = PW(sd[f"{p}.ff.net.2.weight"].contiguous())
        pk[f"{i}.ff.b2"] = sd[f"{p}.ff.net.2.bias"].contiguous()
    pk["ada.tables"] = torch.stack(tabs, 0).contiguous()   # [2*layers, n_emb, C]
    pk["ada.w"] = PW(torch.stack(lw, 0).contiguous())      # [2*layers, 2C, C]
    pk["ada.b"] = torch.stack(lb, 0).contiguous()          # [2*layers, 2C]
    for h in ("mlp_out_trans", "mlp_out_rot"):
        for j in (0, 2, 4):
            pk[f"{h}.{j}.w"] = PW(sd[f"{h}.{j}.weight"].contiguous())
            pk[f"{h}.{j}.b"] = sd[f"{h}.{j}.bias"].contiguous()
    return pk


# ---- which path an eval / sampler step takes: one plan, chosen by a pure function of the call's facts (no process-wide switch
# selects anything here; the arithmetic modes PFPP_GEMM, PFPP_SPLIT_ACT and ops.SINGLE_PASS are inputs of the choice)
# <= this many tokens: the few-token kernels (LayerNorm inside the next GEMM, pfpp_gemm_small, the one-launch embedding); above it the
# C sequencer takes the weight-direct GEMMs (pfpp_gemm_wd)
EVAL_FEW_TOKEN_MAX_ROWS = 2048


class EvalBlocks(enum.Enum):
    C_SEQUENCED = "c"        # the transformer blocks enqueued by one foreign call (pfpp_tlayers_eval; compact forward only)
    PY_TILED = "py_tiled"    # issued from Python, every linear through the tiled GEMM (any mode, any width; the cross-check)
    PY_WD = "py_wd"          # issued from Python, qkv / out-projection / second feed-forward linear through pfpp_gemm_wd


@dataclasses.dataclass(frozen=True)
class EvalPlan:
    embed_fused: bool        # features, both embedding layers and the combine in one launch (csrc/embed_small.hip)
    blocks: EvalBlocks
    lnlin_max_rows: int      # C_SEQUENCED: up to this many tokens the few-token kernels (0 = never: the launches of the Python sequence)
    wd_gemm: bool            # C_SEQUENCED: above lnlin_max_rows the weight-direct GEMMs (the Python sequences say it in `blocks`)
    heads_fused: bool        # pool -> both output heads in one launch (csrc/heads.hip) instead of the layer-wise GEMMs


def frag_covers_blocks(C: int, inner: int) -> bool:
    """does the fragment-blocked layout (packing.PW.frag: N % 32 == 0 and K % 16 == 0) cover every block weight?  wqkv [3C, C],
    wo [C, C], ff.w1 [2 inner, C], ff.w2 [C, inner]"""
    return C % 32 == 0 and (2 * inner) % 32 == 0 and inner % 16 == 0


def _wd_covers_blocks(C: int, inner: int) -> bool:
    """pfpp_gemm_wd_supported for wqkv, wo and ff.w2: N % 128 == 0, K % 32 == 0"""
    return C % 128 == 0 and inner % 32 == 0


def choose_eval(*, compact: bool, gemm_mode: str, split_act: bool, single_pass: bool, traced: bool, tokens: int, C: int, inner: int,
                L: int, latent_dim: int, embed_packed: bool) -> EvalPlan:
    """the plan of denoiser_forward_compact (compact) / denoiser_forward (all slots) when the caller names none.  traced = bench.py's
    per-launch timing pass (ops.GEMM_TRACE set): it issues the blocks from Python and then takes the weight-direct GEMMs
    pfpp_tlayers_eval takes, so that the roofline object describes the kernels of the timed region.  The all-slots forward never takes
    them by itself: with all 640 slots evaluated (16,000 tokens) the 256 x 128 tiled kernel has enough tiles per CU that its LDS traffic
    is not the bound, 6.756 vs 6.751 ms per sampler step (profiles/r04zw_ab_wd_full.txt) — blocks = PY_WD by argument only."""
    split = gemm_mode == "f16x3" and split_act
    heads_fused = gemm_mode == "f16x3" and C == 512
    if not compact:
        return EvalPlan(embed_fused=False, blocks=EvalBlocks.PY_TILED, lnlin_max_rows=0, wd_gemm=False, heads_fused=heads_fused)
    few = tokens <= EVAL_FEW_TOKEN_MAX_ROWS
    embed_fused = few and embed_packed and split and not single_pass and not traced and L >= 11 and latent_dim == 64 and C % 32 == 0
    if split and not traced and frag_covers_blocks(C, inner):
        return EvalPlan(embed_fused=embed_fused, blocks=EvalBlocks.C_SEQUENCED, lnlin_max_rows=EVAL_FEW_TOKEN_MAX_ROWS, wd_gemm=True,
                        heads_fused=heads_fused)
    wd = traced and split and not single_pass and not few and _wd_covers_blocks(C, inner)
    return EvalPlan(embed_fused=embed_fused, blocks=EvalBlocks.PY_WD if wd else EvalBlocks.PY_TILED, lnlin_max_rows=0, wd_gemm=wd,
                    heads_fused=heads_fused)


def check_plan(plan: EvalPlan, *, compact: bool, gemm_mode: str, split_act: bool, single_pass: bool, traced: bool, tokens: int, C: int,
               inner: int, L: int, latent_dim: int, embed_packed: bool) -> None:
    """ValueError for a plan this call cannot honour (before anything is launched): every kernel a plan names has its own modes and
    widths, and nothing falls back quietly"""
    split = gemm_mode == "f16x3" and split_act
    no = []
    if plan.embed_fused and not (compact and embed_packed and split and not single_pass and L >= 11 and latent_dim == 64 and C % 32 == 0):
        no.append("embed_fused: compact forward, 148 + 147 input features, split-f16 planes without single pass, L >= 11, latent 64, C % 32 == 0")
    if plan.blocks is EvalBlocks.C_SEQUENCED and not (compact and split and not traced and frag_covers_blocks(C, inner)):
        no.append("C_SEQUENCED: compact forward in the split-f16 plane mode, untraced, widths the fragment-blocked layout covers")
    if plan.blocks is EvalBlocks.PY_WD and not (split and not single_pass and _wd_covers_blocks(C, inner)):
        no.append("PY_WD: split-f16 plane mode without single pass, C % 128 == 0, inner % 32 == 0")
    if plan.heads_fused and not (gemm_mode == "f16x3" and C == 512):
        no.append("heads_fused: f16x3 mode at width 512")
    if plan.lnlin_max_rows < 0:
        no.append("lnlin_max_rows >= 0")
    if no:
        raise ValueError(f"EvalPlan not possible here ({gemm_mode}, C = {C}, inner = {inner}, {tokens} tokens) - " + "; ".join(no))


def _plan_for(plan: Optional[EvalPlan], pk, *, compact: bool, tokens: int, C: int, inner: int, L: int, latent_dim: int) -> EvalPlan:
    """the call's facts, gathered once: the default plan, or the caller's after check_plan"""
    facts = dict(compact=compact, gemm_mode=ops.GEMM_MODE, split_act=ops.split_act(), single_pass=ops.SINGLE_PASS,
                 traced=ops.GEMM_TRACE is not None, tokens=tokens, C=C, inner=inner, L=L, latent_dim=latent_dim,
                 embed_packed="embed.w" in pk)
    if plan is None:
        return choose_eval(**facts)
    check_plan(plan, **facts)
    return plan


def _fused_heads(pk, pooled, out, slot32=None) -> None:
    """pool -> both output heads in one launch (csrc/heads.hip): f16x3 mode, width 512 (plan.heads_fused)"""
    from . import train_ops as T

    hp = pk.get("_heads")
    if hp is None:
        hp = pk["_heads"] = tuple(T.head_params(pk[f"{n}.0.w"], pk[f"{n}.2.w"], pk[f"{n}.4.w"].f32, pk[f"{n}.0.b"], pk[f"{n}.2.b"],
                                                pk[f"{n}.4.b"], static=True) for n in ("mlp_out_trans", "mlp_out_rot"))
    T.heads_fwd(pooled, hp[0], hp[1], out, slot=slot32)


def _eval_layers_c(pk, h, mods, lay, L: int, num_layers: int, num_heads: int, att_scale: float, inner: int, plan: EvalPlan) -> None:
    """the transformer blocks of the compact eval forward enqueued from C (pfpp_tlayers_eval, csrc/tlayer.hip): h is updated in place
    (plan.blocks = C_SEQUENCED: the plane mode, widths the fragment-blocked layout covers)"""
    import ctypes as C_

    from . import _lib
    from ._lib import ElayerParams, PlanesC, PwC, TlayersEvalArgs

    st = pk.get("_cseq_eval")
    if st is None:
        layers = (ElayerParams * num_layers)()

        def pw(w):
            fh, fl = w.frag()          # (kept alive by the PW in pk)
            return PwC(w.f32.data_ptr(), w.hi.data_ptr(), w.lo.data_ptr(), w.scale, w.hi.shape[-1], fh.data_ptr(), fl.data_ptr())

        for i in range(num_layers):
            for name, key in (("qkv1", f"{i}.self_attn.wqkv"), ("o1", f"{i}.self_attn.wo"), ("qkv2", f"{i}.global_attn.wqkv"),
                              ("o2", f"{i}.global_attn.wo"), ("ff1", f"{i}.ff.w1"), ("ff2", f"{i}.ff.w2")):
                setattr(layers[i], name, pw(pk[key]))
            for name, key in (("bo1", f"{i}.self_attn.bo"), ("bo2", f"{i}.global_attn.bo"), ("g3", f"{i}.norm3.g"), ("b3", f"{i}.norm3.b"),
                              ("bff1", f"{i}.ff.b1"), ("bff2", f"{i}.ff.b2")):
                setattr(layers[i], name, pk[key].data_ptr())
        args = TlayersEvalArgs()
        args.n_layers, args.layers = num_layers, layers
        st = pk["_cseq_eval"] = (args, layers)
    args = st[0]
    M, C = h.shape
    dev = h.device
    norm, att, u = ops.SplitAct.empty(M, C, dev), ops.SplitAct.empty(M, C, dev), ops.SplitAct.empty(M, inner, dev)
    qkv = torch.empty((M, 3 * C), dtype=torch.float32, device=dev)
    ops._sync_attention_mode()
    args.M, args.C, args.H, args.L, args.inner, args.Fv, args.B = M, C, num_heads, L, inner, lay.Fv, mods.shape[1]
    args.h, args.mods = h.data_ptr(), mods.data_ptr()
    args.frag_b, args.seq_off, args.seq_len = lay.frag_b.data_ptr(), lay.seq_off.data_ptr(), lay.seq_len.data_ptr()
    args.n_seq, args.max_len, args.att_scale = lay.seq_off.numel(), lay.max_len, att_scale
    args.single_pass = int(ops.SINGLE_PASS)
    args.norm, args.att, args.u = (PlanesC(t.hi.data_ptr(), t.lo.data_ptr(), 1.0) for t in (norm, att, u))
    args.qkv = qkv.data_ptr()
    ws = ops._split_workspace(dev)
    args.split_ws, args.split_ws_bytes = ws[0].data_ptr(), ws[0].numel() * 4
    args.split_cnt, args.split_cnt_len = ws[1].data_ptr(), ws[1].numel()
    args.lnlin_max_rows, args.wd_gemm = plan.lnlin_max_rows, int(plan.wd_gemm)
    _lib.check(_lib.load().pfpp_tlayers_eval(C_.byref(args), ops._stream()), "pfpp_tlayers_eval")


def dense_attention(qkv: torch.Tensor, B: int, T: int, H: int, dh: int, key_valid_u8: torch.Tensor,
                    scale: float, out: Optional[torch.Tensor] = None, seq=None) -> torch.Tensor:
    """softmax(Q K^T * scale + key mask) V per (sequence, head) from a packed [rows, 3*H*dh] projection —
    one fused kernel (pfpp_attn_dense).  Shared by the denoiser's global attention (a13) and the verifier
    (a18).  `seq` = (seq_off, seq_len) int32 tensors; default: B sequences of T rows."""
    if seq is None:
        seq = uniform_sequences(B, T, qkv.device)
    return ops.attn_dense(qkv, seq[0], seq[1], T, H, dh, scale, key_valid_u8, out=out)


_SEQ_CACHE = {}


def uniform_sequences(B: int, T: int, device):
    key = (B, T, str(device))
    if key not in _SEQ_CACHE:
        off = (torch.arange(B, dtype=torch.int32) * T).to(device)
        ln = torch.full((B,), T, dtype=torch.int32).to(device)
        _SEQ_CACHE[key] = (off, ln)
    return _SEQ_CACHE[key]


def dense_attention_unfused(qkv: torch.Tensor, B: int, T: int, H: int, dh: int, key_valid_u8: torch.Tensor,
                            scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the three-kernel form (QK^T GEMM -> masked softmax -> P.V GEMM), kept as a cross-check of the fused kernel"""
    C = H * dh
    ld = 3 * C
    Tp = round_up(T, 4)
    S = torch.empty((B * H, T, Tp), dtype=torch.float32, device=qkv.device)
    ops.gemm(qkv, qkv, M=T, N=T, K=dh, lda=ld, ldw=ld, out=S, ldc=Tp, batch=B * H, zdiv=H,
             sA=(T * ld, dh), sW=(T * ld, dh), sC=(H * T * Tp, T * Tp), w_off=C)
    ops.softmax_rows(S, key_valid_u8, H * T, T, scale)
    if out is None:
        out = torch.empty((B * T, C), dtype=torch.float32, device=qkv.device)
    ops.gemm(S, qkv, M=T, N=dh, K=T, lda=Tp, ldw=ld, out=out, ldc=C, w_kmajor=True, batch=B * H, zdiv=H,
             sA=(H * T * Tp, T * Tp), sW=(T * ld, dh), sC=(T * C, dh), w_off=2 * C)
    return out


def ada_mods(pk, timesteps: torch.Tensor, n_ada: int, C: int) -> torch.Tensor:
    """all AdaLN (scale, shift) vectors of a step, [2 * layers, B, 2C] = Linear(SiLU(Embedding(t))) per MyAdaLayerNorm
    (attention.py:21-25), in one table lookup + one batched GEMM.  The sampler loops run every puzzle of a batch at the same timestep
    and tag the tensor with it (`timesteps._pfpp_t`, a python int): the rows then depend on (t, B) and the packed weights only, so
    they are computed once per timestep of the schedule and reused for every later step at it (20 x 12 x 1024
    floats per batch size; the cache lives in the pack, i.e. it is dropped whenever the weights are re-packed)."""
    B = timesteps.numel()
    t_host = getattr(timesteps, "_pfpp_t", None)
    cache = None
    if t_host is not None:
        cache = pk.setdefault("_mods_cache", {})
        # the arithmetic mode is part of the key: the exact-fp32 rerun after a non-finite f16x3 result (ops.exact_fp32) must not
        # reuse rows computed in the mode that overflowed
        key = (int(t_host), B, ops.GEMM_MODE, ops.SINGLE_PASS)
        hit = cache.get(key)
        if hit is not None:
            return hit
    se = ops.silu_embed(pk["ada.tables"], timesteps.to(torch.int64).contiguous())
    mods = torch.empty((n_ada, B, 2 * C), dtype=torch.float32, device=se.device)
    ops.gemm(se, pk["ada.w"], M=B, N=2 * C, K=C, lda=C, out=mods, ldc=2 * C, bias=pk["ada.b"],
             batch=n_ada, sA=(B * C, 0), sW=(2 * C * C, 0), sC=(B * 2 * C, 0), sV=(2 * C, 0))
    if cache is not None and len(cache) < 512:
        cache[key] = mods
    return mods


class CompactLayout:
    """which slots are valid fragments and how their tokens group into per-puzzle sequences — everything the compact
    forward needs that depends on part_valids only.  Building it from a device tensor reads back from the GPU
    (nonzero / max), which drains the stream the caller is on; callers that keep part_valids fixed over many steps
    (the sampler loop, HIP-graph capture) build it once, `layout_of` below remembers it on the tensor, and a data
    loader that still has the batch on the host builds it there (`from_host`) with no device read at all."""

    __slots__ = ("slot", "slot32", "Fv", "frag_b", "frag_p", "seq_len", "seq_off", "max_len", "counts")

    def __init__(self, part_valids: torch.Tensor, L: int):
        B, P = part_valids.shape[:2]
        valid = part_valids.reshape(B * P).to(torch.bool)
        self.slot = torch.nonzero(valid).flatten()
        self._derive(B, P, L)

    def _derive(self, B: int, P: int, L: int) -> None:
        self.slot32 = self.slot.to(torch.int32).contiguous()
        self.Fv = int(self.slot.numel())
        self.frag_b = torch.div(self.slot, P, rounding_mode="floor").to(torch.int32).contiguous()
        self.frag_p = (self.slot - self.frag_b.long() * P).to(torch.int32).contiguous()
        counts = torch.bincount(self.frag_b.long(), minlength=B)
        self.counts = counts
        self.seq_len = (counts * L).to(torch.int32)
        self.seq_off = (torch.cumsum(counts, 0) - counts).mul(L).to(torch.int32)
        self.max_len = (int(counts.max().item()) if self.Fv else 0) * L

    @classmethod
    def from_host(cls, part_valids_host: torch.Tensor, L: int, device) -> "CompactLayout":
        """the same layout from the batch as the data loader holds it (CPU): index arithmetic on the host, one small
        async copy per index array, no device->host read"""
        if part_valids_host.device.type != "cpu":
            raise ValueError("CompactLayout.from_host: part_valids must be a host tensor")
        lay = cls(part_valids_host, L)                       # CPU tensors: .item() is free
        for name in ("slot", "slot32", "frag_b", "frag_p", "seq_len", "seq_off", "counts"):
            setattr(lay, name, getattr(lay, name).to(device, non_blocking=True))
        return lay


def layout_of(part_valids: torch.Tensor, L: int) -> CompactLayout:
    """the CompactLayout of this part_valids tensor, remembered ON the tensor object (it lives and dies with it; an
    in-place write bumps `_version` and invalidates it).  A training / sampling loop that passes the same batch
    tensor again — or a loader hook that attached a `from_host` layout with `attach_layout` — never reads back."""
    tag = getattr(part_valids, "_pfpp_layout", None)
    if tag is not None and tag[0] == part_valids._version and tag[1] == L:
        return tag[2]
    lay = CompactLayout(part_valids, L)
    attach_layout(part_valids, L, lay)
    return lay


def attach_layout(part_valids: torch.Tensor, L: int, layout: CompactLayout) -> None:
    part_valids._pfpp_layout = (part_valids._version, L, layout)


def denoiser_forward_compact(pk, x, timesteps, latent, xyz, part_valids, scale, ref_part, *, num_layers: int,
                             num_heads: int, layout: Optional[CompactLayout] = None, plan: Optional[EvalPlan] = None) -> torch.Tensor:
    """DenoiserTransformer.forward restricted to the VALID fragments.

    In the reference every one of the P = 20 slots is a query (denoiser_transformer.py:173-185) but keys are
    only the valid fragments (gen_mask :163-164) and the self-attention is per fragment (:158-162), so no
    valid token ever depends on a padded one.  Dropping the padded slots therefore leaves the predicted noise of
    every valid fragment unchanged (same GEMM rows, same attention keys) and only replaces the reference's
    don't-care values at padded slots by 0 — at the benchmark's fragment distribution that is 4x fewer tokens.
    Ragged per-puzzle sequences go through pfpp_attn_dense's (seq_off, seq_len).
    plan: which kernels the step takes (None = choose_eval's; one this call cannot honour raises ValueError before any launch)."""
    B, P, L, _ = latent.shape
    C = pk["shape.b"].numel()
    n_slots = B * P
    dh = C // num_heads
    dev = latent.device
    lay = layout if layout is not None else layout_of(part_valids, L)
    slot, Fv, frag_b, frag_p = lay.slot, lay.Fv, lay.frag_b, lay.frag_p
    seq_len, seq_off, max_len = lay.seq_len, lay.seq_off, lay.max_len
    out = torch.zeros((n_slots, 7), dtype=torch.float32, device=dev)
    if Fv == 0:
        return out.view(B, P, 7)
    M = Fv * L
    inner = pk["0.ff.w2"].K
    plan = _plan_for(plan, pk, compact=True, tokens=M, C=C, inner=inner, L=L, latent_dim=latent.shape[-1])
    # the valid-fragment gather of the inputs happens inside the kernels (slot32): no gathered copies
    f32 = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
    rp = ref_part.reshape(n_slots)
    ref_u8 = rp.contiguous().view(torch.uint8) if rp.dtype == torch.bool else (rp if rp.dtype == torch.uint8 else (rp != 0).to(torch.uint8)).contiguous()
    if plan.embed_fused:
        # few tokens: features, both embedding layers and the combine in one launch (csrc/embed_small.hip)
        h = ops.embed_tokens_small(f32(latent).reshape(n_slots, L, -1), f32(xyz).reshape(n_slots, L, 3), f32(scale).reshape(n_slots),
                                   f32(x).reshape(n_slots, 7), lay.slot32, pk["embed.w"], pk["embed.b"], pk["ref_emb"], ref_u8, pk["pe"],
                                   frag_p, Fv, L)
    else:
        sf, pf = ops.token_features(f32(latent).reshape(n_slots, L, -1), f32(xyz).reshape(n_slots, L, 3), f32(scale).reshape(n_slots),
                                    f32(x).reshape(n_slots, 7), slot=lay.slot32)
        shape_emb = ops.linear(sf, pk["shape.w"], pk["shape.b"])
        x_emb = ops.linear(pf, pk["param.w"], pk["param.b"])
        h = ops.token_combine_list(shape_emb, x_emb, pk["ref_emb"], ref_u8, pk["pe"], frag_p, L, slot=lay.slot32)
    n_ada = 2 * num_layers
    mods = ada_mods(pk, timesteps, n_ada, C)
    att_scale = 1.0 / math.sqrt(dh)
    in_c = plan.blocks is EvalBlocks.C_SEQUENCED
    wd = plan.blocks is EvalBlocks.PY_WD
    if in_c:
        _eval_layers_c(pk, h, mods, lay, L, num_layers, num_heads, att_scale, inner, plan)
        norm = att = u_buf = None
    elif ops.split_mode():      # GEMM inputs produced by our own kernels travel as pre-split fp16 planes (see ops.split_mode)
        norm, att, u_buf = (ops.SplitAct.empty(M, C, dev), ops.SplitAct.empty(M, C, dev), ops.SplitAct.empty(M, inner, dev))
    else:
        norm, att, u_buf = torch.empty_like(h), torch.empty_like(h), None

    def lin_res(a_, wkey, bkey, K_):
        if wd:
            return ops.gemm_wd(a_, pk[wkey], bias=pk[bkey], residual=h, out=h)
        return ops.gemm(a_, pk[wkey], M=M, N=C, K=K_, lda=K_, out=h, ldc=C, bias=pk[bkey], residual=h, ldr=C)

    for i in range(0 if in_c else num_layers):
        ops.layernorm_grouped(h, mods[2 * i], frag_b, L, out=norm)
        qkv = ops.gemm_wd(norm, pk[f"{i}.self_attn.wqkv"]) if wd else ops.linear(norm, pk[f"{i}.self_attn.wqkv"])
        ops.attn_blockdiag(qkv, Fv, L, num_heads, dh, att_scale, out=att)
        lin_res(att, f"{i}.self_attn.wo", f"{i}.self_attn.bo", C)
        ops.layernorm_grouped(h, mods[2 * i + 1], frag_b, L, out=norm)
        qkv = ops.gemm_wd(norm, pk[f"{i}.global_attn.wqkv"]) if wd else ops.linear(norm, pk[f"{i}.global_attn.wqkv"])
        ops.attn_dense(qkv, seq_off, seq_len, max_len, num_heads, dh, att_scale, None, out=att)
        lin_res(att, f"{i}.global_attn.wo", f"{i}.global_attn.bo", C)
        ops.layernorm(h, gamma=pk[f"{i}.norm3.g"], beta=pk[f"{i}.norm3.b"], out=norm)
        u = ops.linear(norm, pk[f"{i}.ff.w1"], pk[f"{i}.ff.b1"], act="geglu", out=u_buf)
        lin_res(u, f"{i}.ff.w2", f"{i}.ff.b2", inner)
    pooled = ops.mean_pool(h, Fv, L)
    if plan.heads_fused:
        _fused_heads(pk, pooled, out, lay.slot32)
        return out.view(B, P, 7)
    out_c = torch.empty((Fv, 7), dtype=torch.float32, device=dev)
    for name, c0, width in (("mlp_out_trans", 0, 3), ("mlp_out_rot", 3, 4)):
        v = ops.linear(pooled, pk[f"{name}.0.w"], pk[f"{name}.0.b"], act="silu")
        v = ops.linear(v, pk[f"{name}.2.w"], pk[f"{name}.2.b"], act="silu")
        ops.gemm(v, pk[f"{name}.4.w"], M=Fv, N=width, K=v.shape[1], lda=v.shape[1], out=out_c, ldc=7,
                 bias=pk[f"{name}.4.b"], c_off=c0)
    ops.scatter_rows(out_c, lay.slot32, n_slots, out=out)
    return out.view(B, P, 7)


def denoiser_forward(pk, x, timesteps, latent, xyz, part_valids, scale, ref_part, *, num_layers: int,
                     num_heads: int, capture: Optional[dict] = None, plan: Optional[EvalPlan] = None) -> torch.Tensor:
    """DenoiserTransformer.forward (denoiser_transformer.py:169-203), eval mode.  plan: as in denoiser_forward_compact; the blocks are
    always issued from Python here (PY_TILED by default, PY_WD by argument: bit-identical)."""
    B, P, L, _ = latent.shape
    C = pk["shape.b"].numel()
    n = B * P
    T = P * L
    M = B * T
    dh = C // num_heads
    if P > pk["pe"].shape[0]:
        raise ValueError(f"P={P} fragments exceed PositionalEncoding max_len={pk['pe'].shape[0]}")
    inner = pk["0.ff.w2"].K
    plan = _plan_for(plan, pk, compact=False, tokens=M, C=C, inner=inner, L=L, latent_dim=latent.shape[-1])
    sf, pf = ops.token_features(latent.reshape(n, L, -1).contiguous(), xyz.reshape(n, L, 3).contiguous(),
                                scale.reshape(n).contiguous(), x.reshape(n, 7).contiguous())
    shape_emb = ops.linear(sf, pk["shape.w"], pk["shape.b"])
    x_emb = ops.linear(pf, pk["param.w"], pk["param.b"])
    ref_u8 = ref_part.reshape(n).to(torch.uint8).contiguous()
    h = ops.token_combine(shape_emb, x_emb, pk["ref_emb"], ref_u8, pk["pe"], B, P, L)
    if capture is not None:
        capture["tokens"] = h.clone()
    # all AdaLN (scale, shift) vectors of the step in one batched GEMM: [2*layers, B, 2C]
    n_ada = 2 * num_layers
    mods = ada_mods(pk, timesteps, n_ada, C)
    key_valid = part_valids.reshape(B, P).to(torch.bool).repeat_interleave(L, dim=1).to(torch.uint8).contiguous()
    att_scale = 1.0 / math.sqrt(dh)
    # In the split-f16 mode the GEMM inputs produced by our own kernels (normalised rows, attention
    # outputs, GEGLU activations) travel as pre-split fp16 planes: the big GEMMs then do no conversions.
    split = ops.split_mode()
    if split:
        norm, att, u = (ops.SplitAct.empty(M, C, h.device), ops.SplitAct.empty(M, C, h.device),
                        ops.SplitAct.empty(M, inner, h.device))
    else:
        norm, att, u = torch.empty_like(h), torch.empty_like(h), None
    wd = plan.blocks is EvalBlocks.PY_WD

    def lin_res(a_, wkey, bkey, K_):
        if wd:
            return ops.gemm_wd(a_, pk[wkey], bias=pk[bkey], residual=h, out=h)
        return ops.gemm(a_, pk[wkey], M=M, N=C, K=K_, lda=K_, out=h, ldc=C, bias=pk[bkey], residual=h, ldr=C)

    for i in range(num_layers):
        ops.layernorm(h, mod=mods[2 * i], rows_per_batch=T, out=norm)
        qkv = ops.gemm_wd(norm, pk[f"{i}.self_attn.wqkv"]) if wd else ops.linear(norm, pk[f"{i}.self_attn.wqkv"])
        ops.attn_blockdiag(qkv, n, L, num_heads, dh, att_scale, out=att)
        lin_res(att, f"{i}.self_attn.wo", f"{i}.self_attn.bo", C)
        ops.layernorm(h, mod=mods[2 * i + 1], rows_per_batch=T, out=norm)
        qkv = ops.gemm_wd(norm, pk[f"{i}.global_attn.wqkv"]) if wd else ops.linear(norm, pk[f"{i}.global_attn.wqkv"])
        dense_attention(qkv, B, T, num_heads, dh, key_valid, att_scale, out=att)
        lin_res(att, f"{i}.global_attn.wo", f"{i}.global_attn.bo", C)
        ops.layernorm(h, gamma=pk[f"{i}.norm3.g"], beta=pk[f"{i}.norm3.b"], out=norm)
        u = ops.linear(norm, pk[f"{i}.ff.w1"], pk[f"{i}.ff.b1"], act="geglu", out=u)
        lin_res(u, f"{i}.ff.w2", f"{i}.ff.b2", inner)
        if capture is not None:
            capture[f"layer{i}"] = h.clone()
    pooled = ops.mean_pool(h, n, L)
    out = torch.empty((n, 7), dtype=torch.float32, device=h.device)
    if plan.heads_fused:
        _fused_heads(pk, pooled, out)
        return out.view(B, P, 7)
    for name, c0, width in (("mlp_out_trans", 0, 3), ("mlp_out_rot", 3, 4)):
        v = ops.linear(pooled, pk[f"{name}.0.w"], pk[f"{name}.0.b"], act="silu")
        v = ops.linear(v, pk[f"{name}.2.w"], pk[f"{name}.2.b"], act="silu")
        ops.gemm(v, pk[f"{name}.4.w"], M=n, N=width, K=v.shape[1], lda=v.shape[1], out=out, ldc=7,
                 bias=pk[f"{name}.4.b"], c_off=c0)
    return out.view(B, P, 7)
