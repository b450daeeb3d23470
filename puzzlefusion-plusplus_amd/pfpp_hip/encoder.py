"""Fragment encoder on the HIP kernels: rotate -> 3 x [FPS, ball query, group, SA-MLP, max]
-> conv6 -> VQ -> scatter  (SURVEY.md §8a rows a1-a8).

Host orchestration only; all arithmetic is in libpfpp_hip.so.  Activations are kept
channels-last ([rows, C]) so every 1x1 convolution is one GEMM with the BatchNorm /
ReLU / max-over-nsample epilogue fused in.
"""
from __future__ import annotations

import dataclasses
import enum
from typing import Callable, Dict, Optional

import torch

from . import ops
from .packing import PW, fold_conv_bn, pack_sa_first

# (name, npoint, radius, nsample) — vqvae/model/modules/pn2.py:16-18
SA_LEVELS = (("sa1", 256, 0.2, 32), ("sa2", 128, 0.4, 64), ("sa3", None, 0.8, 64))


def pack_encoder(sd: Dict[str, torch.Tensor], prefix: str = "") -> Dict[str, torch.Tensor]:
    """sd: live tensors of a VQVAE module keyed by state_dict names -> packed kernel weights"""
    out: Dict[str, torch.Tensor] = {}
    for name, _, _, _ in SA_LEVELS:
        for i in range(3):
            p = f"{prefix}pn2.{name}"
            w, s, t = fold_conv_bn(
                sd[f"{p}.mlp_convs.{i}.weight"], sd[f"{p}.mlp_convs.{i}.bias"],
                sd[f"{p}.mlp_bns.{i}.weight"], sd[f"{p}.mlp_bns.{i}.bias"],
                sd[f"{p}.mlp_bns.{i}.running_mean"], sd[f"{p}.mlp_bns.{i}.running_var"],
            )
            if i == 0:
                w = pack_sa_first(w, w.shape[1] - 3)
            out[f"{name}.w{i}"] = PW(w.contiguous(), prescale=False)     # the fused set-abstraction kernels read these planes directly
            out[f"{name}.s{i}"] = s
            out[f"{name}.t{i}"] = t
    w6 = sd[f"{prefix}pn2.conv6.weight"]
    out["conv6.w"] = PW(w6.reshape(w6.shape[0], -1).contiguous())
    out["conv6.b"] = sd[f"{prefix}pn2.conv6.bias"].contiguous()
    out["codebook"] = sd[f"{prefix}vector_quantization.embedding.weight"].contiguous()
    return out


def pack_encoder_train(sd: Dict[str, torch.Tensor], prefix: str = "") -> Dict[str, torch.Tensor]:
    """train-mode packing: raw conv weights/biases (BatchNorm is NOT folded: it runs on batch statistics), the
    BatchNorm affine parameters and the LIVE running-statistics buffers (updated in place by pfpp_bn_stats)"""
    out: Dict[str, torch.Tensor] = {}
    for name, _, _, _ in SA_LEVELS:
        for i in range(3):
            p = f"{prefix}pn2.{name}"
            w = sd[f"{p}.mlp_convs.{i}.weight"]
            w = w.reshape(w.shape[0], -1)
            if i == 0:
                w = pack_sa_first(w, w.shape[1] - 3)
            out[f"{name}.w{i}"] = PW(w.contiguous(), prescale=False)     # the fused set-abstraction kernels read these planes directly
            out[f"{name}.b{i}"] = sd[f"{p}.mlp_convs.{i}.bias"].contiguous()
            out[f"{name}.g{i}"] = sd[f"{p}.mlp_bns.{i}.weight"].contiguous()
            out[f"{name}.be{i}"] = sd[f"{p}.mlp_bns.{i}.bias"].contiguous()
            out[f"{name}.rm{i}"] = sd[f"{p}.mlp_bns.{i}.running_mean"]
            out[f"{name}.rv{i}"] = sd[f"{p}.mlp_bns.{i}.running_var"]
            out[f"{name}.nbt{i}"] = sd[f"{p}.mlp_bns.{i}.num_batches_tracked"]
    w6 = sd[f"{prefix}pn2.conv6.weight"]
    out["conv6.w"] = PW(w6.reshape(w6.shape[0], -1).contiguous())
    out["conv6.b"] = sd[f"{prefix}pn2.conv6.bias"].contiguous()
    out["codebook"] = sd[f"{prefix}vector_quantization.embedding.weight"].contiguous()
    out["train"] = True
    return out


# ----------------------------------------------------------------------------- which path a level takes
# level-2 eval on the rows kernels from this many grouped rows up: one puzzle in flight (65 K rows) is neutral and stays on
# sa_mlp2_table + GEMM (a persistent rows workgroup loads a 140 KB weight slice first)
EVAL_ROWS_MIN_ROWS_128 = 200_000
# padding schedule of the 64-neighbour levels from this many neighbourhoods up (one puzzle in flight: its two launches cost more than they save)
PAD_SCHEDULE_MIN_NEIGHBOURHOODS = 2048
# FPS + ball query of the three levels in one kernel from this many fragments up (a handful of fragments — one puzzle in flight — is
# latency-bound either way; there the per-level kernels' wider ball-query grids win: 171 vs 189 us at F = 8)
SAMPLE_FUSED_MIN_FRAGMENTS = 32


class SaPath(enum.Enum):
    TRAIN_CHAIN = "recomputing chain launches (csrc/sa_train.hip): the [rows, C] activations of the layer-wise form are not written"
    TRAIN_LAYERWISE = "layer-wise GEMMs with the batch statistics in their epilogues and normalise + ReLU in the consumer's A loader"
    TRAIN_UNFUSED = "GEMM, bn_stats, bn_apply per layer"
    EVAL_MLP3 = "grouping + the three folded conv/BN/ReLU + the max in one kernel (ops.sa_mlp3_fused)"
    EVAL_ROWS = "the rows kernels of the train-mode chain with the folded BatchNorm as the layers' affines (_sa_rows_eval)"
    EVAL_MLP2 = "grouping + layers 1 and 2 in one kernel, layer 3 (+ max over nsample) as a GEMM"
    EVAL_TILED = "one GEMM per layer"


@dataclasses.dataclass(frozen=True)
class SaPlan:
    path: SaPath
    # the grouped neighbourhoods [F*S*ns, D+4] are never written out: the first convolution's GEMM gathers its A rows from the level's
    # feature table (pfpp_gemm_args.gather_*); False = materialise them with pfpp_group_gather
    gather_in_gemm: bool
    # first layer of a level with features by linearity: conv1 per POINT once (ops.sa_first_table), its value on a grouped row is
    # U[point] - W_xyz . centroid — the grouped first convolution (42 / 33 GFLOP at levels 2 / 3) is never computed
    table_first: bool
    # 64-neighbour levels: neighbourhoods the ball query padded beyond their first 32 slots are taken as one half (ops.sa_pad_schedule)
    pad_schedule: bool


def choose_sa(*, train: bool, gemm_mode: str, split_act: bool, single_pass: bool, D: int, nsample: int, widths, neighbourhoods: int,
              grouped: bool = True) -> SaPlan:
    """The path of one set-abstraction level, from the facts of the call alone: D input features (0 = none), widths = the three layer
    widths, neighbourhoods = F * npoint, grouped = the caller holds the grouping tuple (False: materialised rows only,
    utils/pn2_utils.py).  tests/test_sa_choice_host.py pins the table."""
    widths = tuple(widths)
    f16x3 = gemm_mode == "f16x3"
    gather = f16x3 and D % 32 == 0
    level = {(0, 32, (64, 64, 128)): 1, (128, 64, (128, 128, 256)): 2, (256, 64, (256, 256, 512)): 3}.get((D, nsample, widths))
    pad = nsample == 64 and neighbourhoods >= PAD_SCHEDULE_MIN_NEIGHBOURHOODS
    if train:
        if f16x3 and grouped and level is not None:
            return SaPlan(SaPath.TRAIN_CHAIN, True, D > 0, D > 0 and pad)
        return SaPlan(SaPath.TRAIN_LAYERWISE if f16x3 else SaPath.TRAIN_UNFUSED, gather and grouped, False, False)
    planes = split_act and f16x3           # activations between the layers as split-f16 planes
    if gather and level == 1:
        return SaPlan(SaPath.EVAL_MLP3, True, False, False)
    if gather and planes and not single_pass and (level == 3 or (level == 2 and neighbourhoods * nsample >= EVAL_ROWS_MIN_ROWS_128)):
        return SaPlan(SaPath.EVAL_ROWS, True, True, pad)
    if gather and D == 128 and nsample == 64 and widths[:2] == (128, 128):
        return SaPlan(SaPath.EVAL_MLP2, True, planes, False)
    return SaPlan(SaPath.EVAL_TILED, gather, gather and planes and nsample == 64 and (D, widths[0]) in ((256, 256), (128, 128)), False)


def fused_sampling(fragments: int, supported: bool) -> bool:
    """ops.sample_levels (the sampling chain of all three levels in one launch) or the per-level kernels"""
    return supported and fragments >= SAMPLE_FUSED_MIN_FRAGMENTS


def sa_plan(pk, name: str, nsample: int, neighbourhoods: int, feats: Optional[torch.Tensor], choose: Callable[..., SaPlan] = choose_sa) -> SaPlan:
    """`choose` on the facts of this call: the numeric mode of ops and the level's shape"""
    return choose(train=bool(pk.get("train", False)), gemm_mode=ops.GEMM_MODE, split_act=ops.split_mode(), single_pass=ops.SINGLE_PASS,
                  D=0 if feats is None else feats.shape[2], nsample=nsample, widths=tuple(pk[f"{name}.w{i}"].N for i in range(3)),
                  neighbourhoods=neighbourhoods)


# Stages of the recomputing chain per level kind (D, table_first): (u_in, y_out, y_in) of stages 1-3, where y_out / y_in name the buffer
# of raw rows ("y1", "y2": that layer's pre-activations [rows, C]) handed over under that argument.  Stage 3 also gets out_max / out_min.
_CHAIN_STAGES = {
    # no features: every stage recomputes from the points, nothing but the sums (and the pooled max / min) is written
    (0, False): ((False, None, None), (False, None, None), (False, None, None)),
    # 128 features: stage 2 writes the raw second-layer rows, stage 3 (its weights resident in LDS) reads them through the same argument
    (128, True): ((True, None, None), (True, "y2", None), (False, "y2", None)),
    (128, False): ((False, None, None), (False, "y2", None), (False, "y2", None)),
    # 256 features: one rows launch per layer (no two weight matrices fit in LDS), the previous layer's raw rows come in as y_in
    (256, True): ((True, None, None), (True, "y2", None), (False, None, "y2")),
    (256, False): ((False, "y1", None), (False, "y2", "y1"), (False, None, "y2")),
}


def _sa_chain_train(pk, name: str, grp, nsample: int, plan: SaPlan) -> torch.Tensor:
    """train-mode level by recomputation (csrc/sa_train.hip): one persistent chain launch per layer; stage k recomputes layers
    1..k-1 in registers and produces layer k's batch statistics — the [rows, C] activations of the layer-wise form are never
    written (level 1) / only the raw second-layer rows are (levels 2 and 3 with the per-point first layer)"""
    from . import train_ops as T

    xyz, new_xyz, feats, ball = grp
    dev = xyz.device
    F, S = ball.shape[:2]
    rows = F * S * nsample
    ws = [pk[f"{name}.w{i}"] for i in range(3)]
    bs = [pk[f"{name}.b{i}"] for i in range(3)]
    affs = []
    utab = ops.sa_first_table(xyz, feats, ws[0], bs[0]) if plan.table_first else None
    # the padding schedule goes to all stages of the level or to none (the raw rows of a skipped half are neither written nor read)
    sched = ops.sa_pad_schedule(ball) if plan.pad_schedule else None
    mx, mn, y = None, None, {}
    for i, (table, y_out, y_in) in enumerate(_CHAIN_STAGES[0 if feats is None else feats.shape[2], plan.table_first]):
        Cout = ws[i].N
        st = pk.get(f"{name}.stats{i}")
        if st is None:
            st = pk[f"{name}.stats{i}"] = T.bn_stats_buffer(Cout, dev)
        if i == 2:
            mx = torch.empty((F * S, Cout), dtype=torch.float32, device=dev)
            mn = torch.empty((F * S, Cout), dtype=torch.float32, device=dev)
        if y_out is not None and y_out not in y:
            y[y_out] = torch.empty((rows, Cout), dtype=torch.float32, device=dev)
        ops.sa_train_stage(i + 1, xyz, new_xyz, feats, ball, ws, bs, affs, st, y_out=y.get(y_out), y_in=y.get(y_in), out_max=mx, out_min=mn,
                           u_in=utab if table else None, sched=sched)
        affs.append(T.bn_finalize(st, rows, pk[f"{name}.g{i}"], pk[f"{name}.be{i}"], pk[f"{name}.rm{i}"], pk[f"{name}.rv{i}"],
                                  momentum=0.1, eps=1e-5))
    torch._foreach_add_([pk[f"{name}.nbt{i}"] for i in range(3)], 1)
    return T.bn_minmax_apply(mx, mn, affs[2][0], affs[2][1])


def _sa_mlp_train(pk, name: str, A: Optional[torch.Tensor], nsample: int, grp=None, plan: Optional[SaPlan] = None) -> torch.Tensor:
    """3 x [1x1 conv -> BatchNorm (batch statistics, running buffers updated) -> ReLU], max over nsample
    (utils/pn2_utils.py:210-216 with the module in .train()).  A = the materialised grouped rows [F*S*ns, D+4], or None with the grouping
    tuple in grp; without a plan (utils/pn2_utils.py: materialised rows only) the mode of ops decides alone"""
    from . import train_ops as T

    if plan is None:
        plan = choose_sa(train=True, gemm_mode=ops.GEMM_MODE, split_act=ops.split_mode(), single_pass=ops.SINGLE_PASS, D=A.shape[1] - 4,
                         nsample=nsample, widths=tuple(pk[f"{name}.w{i}"].N for i in range(3)), neighbourhoods=A.shape[0] // nsample,
                         grouped=False)
    if plan.path is SaPath.TRAIN_CHAIN:
        return _sa_chain_train(pk, name, grp, nsample, plan)
    if plan.path is SaPath.TRAIN_LAYERWISE:
        # fused form: batch statistics come out of the producing GEMM's epilogue, normalise+ReLU is applied by the
        # consuming GEMM while it stages its A tiles, and the last layer emits per-group max AND min instead of
        # its [rows, C] activation (max_p relu(a*y_p + b) = relu(a*(a >= 0 ? max_p y_p : min_p y_p) + b))
        dev = A.device if A is not None else grp[0].device
        rows = A.shape[0] if A is not None else grp[3].numel()
        h, aff = A, None
        for i in range(3):
            Cout = pk[f"{name}.w{i}"].N
            st = pk.get(f"{name}.stats{i}")
            if st is None:                   # allocated (and zeroed) once: pfpp_bn_finalize clears the copies it has summed
                st = pk[f"{name}.stats{i}"] = T.bn_stats_buffer(Cout, dev)
            if i == 0 and A is None:
                h = ops.grouped_linear(*grp, pk[f"{name}.w0"], pk[f"{name}.b0"], stats=st)
            elif i < 2:
                h = ops.linear(h, pk[f"{name}.w{i}"], pk[f"{name}.b{i}"], a_affine=aff, stats=st)
            else:
                mn = torch.empty((rows // nsample, Cout), dtype=torch.float32, device=dev)
                mx = ops.linear(h, pk[f"{name}.w{i}"], pk[f"{name}.b{i}"], a_affine=aff, stats=st, pool=nsample, c_min=mn)
            aff = T.bn_finalize(st, rows, pk[f"{name}.g{i}"], pk[f"{name}.be{i}"], pk[f"{name}.rm{i}"], pk[f"{name}.rv{i}"],
                                momentum=0.1, eps=1e-5)
        torch._foreach_add_([pk[f"{name}.nbt{i}"] for i in range(3)], 1)          # num_batches_tracked of the level: one launch
        return T.bn_minmax_apply(mx, mn, aff[0], aff[1])
    h = A
    for i in range(3):
        y = ops.linear(h, pk[f"{name}.w{i}"], pk[f"{name}.b{i}"])
        mean, var = T.bn_stats(y, pk[f"{name}.rm{i}"], pk[f"{name}.rv{i}"], momentum=0.1)
        pk[f"{name}.nbt{i}"] += 1
        h = T.bn_apply(y, mean, var, pk[f"{name}.g{i}"], pk[f"{name}.be{i}"], eps=1e-5, pool=nsample if i == 2 else 0)
        del y
    return h


def _sa_rows_eval(pk, name: str, grp, nsample: int, plan: SaPlan) -> torch.Tensor:
    """eval-mode level with input features (sa3: 256 + 3 -> 256 -> 256 -> 512; sa2: 128 + 3 -> 128 -> 128 -> 256; 64 neighbours) on the ROWS kernels of the train-mode chain
    (csrc/sa_train.hip sa_wide_train_kernel<256, 2, UG> / <256, 3>: a workgroup keeps a 128-column slice of the layer's weight planes in
    LDS for its lifetime, a wave streams 32 rows at a time) instead of an elementwise pass + two tiled plane GEMMs with their
    [rows, 256] planes in between: 430 instead of 766 us at 154 fragments.  Same entry point as training (pfpp_sa_train_stage) with the
    FOLDED BatchNorm scale / shift as the layers' affines and zero conv biases (the folded shift carries them, pn2_utils.py:210-216 in
    .eval()): layer 1 per point (U[point] - W_xyz . centroid), layer 2 from gathered table rows -> raw y_2, layer 3 -> per-neighbourhood
    max / min of y_3, and max_p relu(s y_p + t) = relu(s (s >= 0 ? max y : min y) + t) exactly (monotone).  The statistics the train
    kernels also accumulate go to a scratch buffer nobody reads."""
    from . import train_ops as T

    xyz, new_xyz, feats, ball = grp
    dev = xyz.device
    F, S = ball.shape[:2]
    rows = F * S * nsample
    ws = [pk[f"{name}.w{i}"] for i in range(3)]
    aff = [(pk[f"{name}.s{i}"], pk[f"{name}.t{i}"]) for i in range(3)]
    sc = pk.get(f"{name}._rows_eval")
    if sc is None:
        sc = pk[f"{name}._rows_eval"] = ([torch.zeros(w.N, dtype=torch.float32, device=dev) for w in ws],
                                         [T.bn_stats_buffer(w.N, dev) for w in ws])
    zb, st = sc
    u = ops.sa_first_table(xyz, feats, ws[0], None)
    y2 = torch.empty((rows, ws[1].N), dtype=torch.float32, device=dev)
    sched = ops.sa_pad_schedule(ball) if plan.pad_schedule else None      # padded second halves add nothing to a max / min
    ops.sa_train_stage(2, xyz, new_xyz, feats, ball, ws, zb, aff[:1], st[1], y_out=y2, u_in=u, sched=sched)
    mx = torch.empty((F * S, ws[2].N), dtype=torch.float32, device=dev)
    mn = torch.empty((F * S, ws[2].N), dtype=torch.float32, device=dev)
    # stage 3 as in _CHAIN_STAGES: 256 features read the previous layer's raw rows as y_in, 128 features through y_out
    y3 = dict(y_in=y2) if feats.shape[2] == 256 else dict(y_out=y2)
    ops.sa_train_stage(3, xyz, new_xyz, feats, ball, ws, zb, aff[:2], st[2], out_max=mx, out_min=mn, sched=sched, **y3)
    return T.bn_minmax_apply(mx, mn, aff[2][0], aff[2][1])


def set_abstraction(pk, name: str, npoint: int, radius: float, nsample: int, xyz: torch.Tensor,
                    feats: Optional[torch.Tensor], capture: Optional[dict] = None, sampled=None, plan: Optional[SaPlan] = None):
    """xyz [F,N,3], feats [F,N,D] or None -> new_xyz [F,S,3], new_feats [F,S,C3].  sampled = (fps_idx, new_xyz, ball_idx) when the
    sampling of all levels was done up front (ops.sample_levels); plan = the path to take (default: choose_sa on this call)"""
    F = xyz.shape[0]
    if sampled is not None:
        fps_idx, new_xyz, ball = sampled
    else:
        ops.check_fps_ratio(npoint, xyz.shape[1])
        fps_idx, new_xyz = ops.fps(xyz, npoint)
        ball = ops.ball_query(xyz, new_xyz, radius, nsample)
    if plan is None:
        plan = sa_plan(pk, name, nsample, F * npoint, feats)
    A = None if plan.gather_in_gemm else ops.group_gather(xyz, new_xyz, feats, ball)
    grp = (xyz, new_xyz, None if feats is None else feats.contiguous(), ball)
    w, s, t = ([pk.get(f"{name}.{k}{i}") for i in range(3)] for k in "wst")
    if plan.path in (SaPath.TRAIN_CHAIN, SaPath.TRAIN_LAYERWISE, SaPath.TRAIN_UNFUSED):
        h = _sa_mlp_train(pk, name, A, nsample, grp, plan)
    elif plan.path is SaPath.EVAL_MLP3:
        h = ops.sa_mlp3_fused(xyz, new_xyz, ball, w[0], w[1], w[2], s[0], t[0], s[1], t[1], s[2], t[2])
    elif plan.path is SaPath.EVAL_ROWS:
        h = _sa_rows_eval(pk, name, grp, nsample, plan)
    elif plan.path is SaPath.EVAL_MLP2:
        # first layer per point (ops.sa_mlp2_table: the grouped first convolution is not computed): the activation then goes to layer 3
        # as split-f16 planes (same bytes as fp32), the LDS-DMA plane GEMM with no conversion work in its loop
        mlp2 = ops.sa_mlp2_table if plan.table_first else ops.sa_mlp2_fused
        h = mlp2(xyz, new_xyz, grp[2], ball, w[0], w[1], s[0], t[0], s[1], t[1])
        h = ops.linear(h, w[2], scale=s[2], shift=t[2], act="relu", pool=nsample)
    else:
        # activations between the layers as split-f16 planes
        planes = (lambda i: ops.SplitAct.empty(F * npoint * nsample, w[i].N, xyz.device)) if ops.split_mode() else (lambda i: None)
        if plan.table_first:
            # first layer per point (linear), then an elementwise pass over the grouped rows (ops.sa_table_planes)
            h = ops.sa_table_planes(*grp, w[0], s[0], t[0])
        elif A is None:
            h = ops.grouped_linear(*grp, w[0], scale=s[0], shift=t[0], act="relu", out=planes(0))
        else:
            h = ops.linear(A, w[0], scale=s[0], shift=t[0], act="relu", out=planes(0))
        del A
        h = ops.linear(h, w[1], scale=s[1], shift=t[1], act="relu", out=planes(1))
        h = ops.linear(h, w[2], scale=s[2], shift=t[2], act="relu", pool=nsample)
    new_feats = h.view(F, npoint, -1)
    if capture is not None:
        capture.update({f"{name}.fps_idx": fps_idx, f"{name}.ball_idx": ball, f"{name}.new_xyz": new_xyz, f"{name}.new_points": new_feats})
    return new_xyz, new_feats


def pn2_encode(pk, pts: torch.Tensor, num_point: int = 25, capture: Optional[dict] = None, choose: Callable[..., SaPlan] = choose_sa):
    """pts [F,N,3] (already rotated) -> z_e [F,L,64], xyz [F,L,3]   (pn2.py:57-68).  choose: choose_sa or a function of the same
    signature (the tests' cross-check paths)"""
    xyz, feats = pts, None
    # the sampling chain of all three levels depends on coordinates only: one launch (FPS x 3 + ball query x 3 per fragment)
    lv = tuple((npoint or num_point, radius, nsample) for _, npoint, radius, nsample in SA_LEVELS)
    sampled = ops.sample_levels(pts, lv) if fused_sampling(pts.shape[0], ops.sample_levels_supported(pts.shape[1], lv)) else (None,) * 3
    for (name, npoint, radius, nsample), smp in zip(SA_LEVELS, sampled):
        npoint = npoint or num_point
        plan = sa_plan(pk, name, nsample, xyz.shape[0] * npoint, feats, choose)
        xyz, feats = set_abstraction(pk, name, npoint, radius, nsample, xyz, feats, capture, sampled=smp, plan=plan)
    F, L, C3 = feats.shape
    z_e = ops.linear(feats.view(F * L, C3), pk["conv6.w"], pk["conv6.b"]).view(F, L, -1)
    return z_e, xyz


def encode_valid(pk, pts: torch.Tensor, num_point: int = 25, max_frag: int = 2048):
    """VQVAE.encode on a dense list of fragments [F,N,3] -> {"z_q": [F,L,64], "xyz": [F,L,3]}"""
    F = pts.shape[0]
    slot = torch.arange(F, dtype=torch.int32, device=pts.device)
    z_q = torch.empty((F, num_point, pk["conv6.w"].N), dtype=torch.float32, device=pts.device)
    xyz_out = torch.empty((F, num_point, 3), dtype=torch.float32, device=pts.device)
    for f0 in range(0, F, max_frag):
        f1 = min(F, f0 + max_frag)
        z_e, xyz = pn2_encode(pk, pts[f0:f1].contiguous(), num_point)
        ops.vq_encode(z_e, pk["codebook"], slot[: f1 - f0].contiguous(), f1 - f0, z_q=z_q[f0:f1])
        xyz_out[f0:f1] = xyz
    return {"z_q": z_q, "xyz": xyz_out}


def extract_features(pk, part_pcs: torch.Tensor, pose: torch.Tensor, slot: torch.Tensor,
                     num_point: int = 25, max_frag: int = 2048, capture: Optional[dict] = None):
    """Denoiser._extract_features (denoiser.py:66-77): part_pcs [B,P,N,3], pose [B,P,7],
    slot = flattened indices of the valid fragments (int32, ascending)
    -> latent [B,P,L,64], xyz [B,P,L,3] with zeros in the padded slots."""
    B, P, N, _ = part_pcs.shape
    n_slots = B * P
    dev = part_pcs.device
    # both padded outputs out of ONE zero fill (one launch instead of two on the one-puzzle-in-flight chain)
    Cz = pk["conv6.w"].N
    n_lat = n_slots * num_point * Cz
    both = torch.zeros(n_lat + n_slots * num_point * 3, dtype=torch.float32, device=dev)
    latent = both[:n_lat].view(n_slots, num_point, Cz)
    xyz_out = both[n_lat:].view(n_slots, num_point, 3)
    pcs_flat = part_pcs.view(n_slots, N, 3)
    pose_flat = pose.reshape(n_slots, 7).contiguous()
    F = slot.numel()
    for f0 in range(0, F, max_frag):
        sl = slot[f0:f0 + max_frag].contiguous()
        rot = ops.se3_rotate_gather(pcs_flat, pose_flat, sl)
        if capture is not None:
            capture["rotated"] = rot
        z_e, xyz = pn2_encode(pk, rot, num_point, capture)
        if capture is not None:
            capture["z_e"] = z_e
        ops.vq_encode(z_e, pk["codebook"], sl, n_slots, z_q=latent)
        ops.scatter_rows(xyz, sl, n_slots, out=xyz_out)
    return latent.view(B, P, num_point, -1), xyz_out.view(B, P, num_point, 3)
