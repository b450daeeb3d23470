"""Time forward + backward of the matcher's ragged PointNet++ encoder through EncoderTrainEngine, per stage by HIP events, next to
PyTorch-ROCm eager fp32 autograd of the same steps on the same GPU and the same indices, the two alternating.

    python tools/matching_encoder_train_bench.py [--repeats 3] [--warmup 2] [--skip-eager] [--out FILE]

Shape: 16 puzzles x 8 pieces x 625 points (80,000 points).  Both sides get the indices of a first, untimed engine
forward (sampling chains, the K = 32 lists whose head is the K = 16 list, the 3 nearest centroids with their counts); the engine's
timed forward computes them again (stage `geometry`), eager does not.  Stages of the engine: geometry, inverse_lists (torch sorts),
set_abstraction, propagation; then conv1_bwd, propagation_bwd and sa4_bwd .. sa1_bwd.  The eager baseline: gathers, F.linear,
F.batch_norm(training=True) over all rows, relu, max, loss = sum(out * dout), loss.backward(); its stages are forward and backward.
Peak device memory of both is reported (inputs and weights are resident in both).  Prints one JSON line (and writes it to --out): ms
per call per stage, medians of `repeats` after `warmup` warm-ups; the relative difference of the descriptors and of the
largest-deviating parameter gradient is reported, not asserted (parity is tests/test_gpu_matching_encoder_train.py's business).
Reads nothing outside the repository."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))
LENGTHS = [625] * (16 * 8)
FWD_STAGES = ("geometry", "inverse_lists", "set_abstraction", "propagation")
BWD_STAGES = ("conv1_bwd", "propagation_bwd", "sa4_bwd", "sa3_bwd", "sa2_bwd", "sa1_bwd")


def eager_forward(enc, x: torch.Tensor, idx: dict) -> torch.Tensor:
    """pointnet2_msg.py:67-94 in .train() on given indices, with the module's own parameters and buffers"""
    def layer(conv, bn, a):
        y = F.linear(a, conv.weight.reshape(conv.weight.shape[0], -1), conv.bias)
        return torch.relu(F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps))

    xyz, feats = [x], [x]
    for l in range(4):
        xyz.append(xyz[l][idx["cen"][l]])
    for l, name in enumerate(("sa1", "sa2", "sa3", "sa4")):
        sa, outs = getattr(enc, name), []
        for k, K in enumerate((16, 32)):
            g = idx["knn"][l][:, :K]
            a = torch.cat([feats[l][g], xyz[l][g] - xyz[l + 1][:, None, :]], -1).reshape(-1, feats[l].shape[1] + 3)
            for conv, bn in zip(sa.conv_blocks[k], sa.bn_blocks[k]):
                a = layer(conv, bn, a)
            outs.append(a.reshape(-1, K, a.shape[1]).max(1)[0])
        feats.append(torch.cat(outs, 1))
    up = feats[4]
    for l, name in zip((3, 2, 1, 0), ("fp4", "fp3", "fp2", "fp1")):
        fp = getattr(enc, name)
        if idx["back"][l] is None:
            interp = up.repeat(xyz[l].shape[0], 1)
        else:
            b3, cnt = idx["back"][l]
            a_, b_ = xyz[l][:, None, :], xyz[l + 1][b3]
            dist = (a_ ** 2 + b_ ** 2 - 2 * a_ * b_).sum(-1)
            dist = torch.where(torch.arange(3, device=x.device)[None, :] < cnt[:, None], dist, torch.full_like(dist, 1e8))
            r = 1.0 / (dist + 1e-8)
            interp = (up[b3] * (r / r.sum(1, keepdim=True))[:, :, None]).sum(1)
        a = interp if l == 0 else torch.cat([feats[l], interp], 1)
        for conv, bn in zip(fp.mlp_convs, fp.mlp_bns):
            a = layer(conv, bn, a)
        up = a
    return F.linear(up, enc.conv1.weight.reshape(enc.conv1.weight.shape[0], -1), enc.conv1.bias)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true", help="time the HIP path only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_encoder_train_bench: no GPU", file=sys.stderr)
        return 2
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic
    from pfpp_hip.matching_encoder_train import EncoderTrainEngine

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rng = np.random.default_rng(5)
    pts = []
    for n in LENGTHS:                                            # a noisy patch of a sphere per piece
        v = rng.normal(size=(n, 3)) + 2.0 * rng.normal(size=3)
        pts.append(0.4 * v / np.linalg.norm(v, axis=1, keepdims=True) * (1 + 0.05 * rng.normal(size=(n, 1))))
    x = torch.from_numpy(np.concatenate(pts).astype(np.float32)).to(dev)
    dout = torch.randn((x.shape[0], 128), device=dev)
    enc = PointNet2PTMSGDynamic(3, 128).to(dev)
    eng = EncoderTrainEngine(enc)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    eng.forward(x, LENGTHS, seed=1)
    s = eng.saved
    idx = {"cen": [c.long() for c in s["cen"]], "knn": [k.long() for k in s["nbr"]],
           "back": [None if b[0] is None else (b[0].long(), b[1].long()) for b in s["back"]]}
    start = s["start"].t().contiguous().cpu().numpy()
    eager_enc = None
    if not args.skip_eager:
        eager_enc = PointNet2PTMSGDynamic(3, 128).to(dev)
        eager_enc.load_state_dict(state)
        for p in eager_enc.parameters():
            p.requires_grad_(True)

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    hip, eager, peak = [], [], {}
    for it in range(args.warmup + args.repeats):
        enc.load_state_dict(state)                               # every call starts from the same buffers
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        eng.stage_events = []
        y = eng.forward(x, LENGTHS, start=start)
        eng.backward(dout)
        torch.cuda.synchronize()
        peak["engine"] = torch.cuda.max_memory_allocated()
        marks, eng.stage_events = eng.stage_events, None
        cut = [i for i, (n, _) in enumerate(marks) if n == "begin"][1]         # forward: begin .. propagation; backward: begin .. sa1_bwd
        row = {marks[i][0]: marks[i - 1][1].elapsed_time(marks[i][1]) for i in range(1, len(marks)) if marks[i][0] != "begin"}
        row["forward"] = marks[0][1].elapsed_time(marks[cut - 1][1])
        row["backward"] = marks[cut][1].elapsed_time(marks[-1][1])
        if it >= args.warmup:
            hip.append(row)
        if eager_enc is None:
            continue
        eager_enc.load_state_dict(state)
        for p in eager_enc.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        e0 = ev()
        with torch.enable_grad():
            ye = eager_forward(eager_enc, x, idx)
            loss = (ye * dout).sum()
        e1 = ev()
        loss.backward()
        e2 = ev()
        torch.cuda.synchronize()
        peak["eager"] = torch.cuda.max_memory_allocated()
        if it >= args.warmup:
            eager.append({"forward": e0.elapsed_time(e1), "backward": e1.elapsed_time(e2)})
    med = lambda rows, k: round(statistics.median(r[k] for r in rows), 4)
    res = {"bench": "matching_encoder_train", "points": int(x.shape[0]), "pieces": len(LENGTHS), "repeats": args.repeats, "warmup": args.warmup,
           "engine_ms": {k: med(hip, k) for k in FWD_STAGES + ("forward",) + BWD_STAGES + ("backward",)},
           "engine_peak_mb": round(peak["engine"] / 2 ** 20, 1)}
    res["engine_ms"]["total"] = round(res["engine_ms"]["forward"] + res["engine_ms"]["backward"], 4)
    if eager:
        res["eager_ms"] = {k: med(eager, k) for k in ("forward", "backward")}
        res["eager_ms"]["total"] = round(res["eager_ms"]["forward"] + res["eager_ms"]["backward"], 4)
        res["eager_peak_mb"] = round(peak["eager"] / 2 ** 20, 1)
        res["engine_over_eager"] = round(res["engine_ms"]["total"] / res["eager_ms"]["total"], 4)
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        res["rel_diff_out"] = rel(y, ye.detach())
        grads = {k: rel(p.grad, dict(eager_enc.named_parameters())[k].grad) for k, p in eng.params.items()
                 if not (k.endswith("bias") and "conv" in k and k != "conv1.bias")}
        worst = max(grads, key=grads.get)
        res["rel_diff_worst_grad"] = {worst: grads[worst]}
        # the yardstick for that figure: the same eager steps in float64 (its own ReLU and pool decisions), against which both float32
        # sides are measured on the tensor where they differ most
        e64 = PointNet2PTMSGDynamic(3, 128).to(dev)
        e64.load_state_dict(state)
        e64 = e64.double()
        for p in e64.parameters():
            p.requires_grad_(True)
        with torch.enable_grad():
            (eager_forward(e64, x.double(), idx) * dout.double()).sum().backward()
        g64 = dict(e64.named_parameters())[worst].grad
        res["rel_diff_worst_grad_to_float64"] = {"engine": rel(eng.params[worst].grad.double(), g64),
                                                 "eager": rel(dict(eager_enc.named_parameters())[worst].grad.double(), g64)}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
