"""Time forward + backward of the matcher's cross-attention layer through CrossAttentionTrainEngine, per stage by HIP events, next to
PyTorch-ROCm eager fp32 autograd of the same layer on the same GPU, the two alternating.

    python tools/matching_cross_train_bench.py [--puzzles 16] [--points 5000] [--repeats 3] [--warmup 2] [--out FILE]
    python tools/matching_cross_train_bench.py --puzzles 1                 # one puzzle of 5,000 points

Stages of the engine: forward, then the backward's feed-forward block (LayerNorm 2, w_2, ReLU, w_1 with their weight gradients),
the fc block (LayerNorm 1, fc), the attention's two passes, and the q | k | v projection (weight gradient and dx).  The eager
baseline: F.linear, per puzzle F.scaled_dot_product_attention (what PyTorch-ROCm dispatches it to is its business), F.layer_norm,
loss = sum(out * dout), loss.backward(); its stages are forward and backward.  Peak device memory of both is reported (the inputs
and weights are resident in both).  Prints one JSON line (and writes it to --out): ms per call per stage, medians of `repeats`
after `warmup` warm-ups; the relative difference of dx and of the largest-deviating parameter gradient is reported, not asserted
(parity is tests/test_gpu_matching_cross_train.py's business)."""
from __future__ import annotations

import argparse
import importlib.util
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))
ENGINE_STAGES = ("forward", "ffn_bwd", "fc_bwd", "attention_bwd", "projection_bwd")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_transformer_cases", ROOT / "tests" / "matching_transformer_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def eager_forward(w: dict, x: torch.Tensor, puzzle_points) -> torch.Tensor:
    qkv = torch.cat([F.linear(x, w["attn.w_qs.weight"]), F.linear(x, w["attn.w_ks.weight"]), F.linear(x, w["attn.w_vs.weight"])], 1)
    att, lo = [], 0
    for n in puzzle_points:
        n = int(n)
        t = qkv[lo:lo + n].reshape(1, n, 3, 8, 16).permute(2, 0, 3, 1, 4)
        att.append(F.scaled_dot_product_attention(t[0], t[1], t[2]).transpose(1, 2).reshape(n, 128))
        lo += n
    att = torch.cat(att, 0)
    y = F.layer_norm(F.linear(att, w["attn.fc.weight"]) + x, (128,), w["attn.layer_norm.weight"], w["attn.layer_norm.bias"], 1e-6)
    z = F.linear(torch.relu(F.linear(y, w["pos_ffn.w_1.weight"], w["pos_ffn.w_1.bias"])), w["pos_ffn.w_2.weight"], w["pos_ffn.w_2.bias"]) + y
    return F.layer_norm(z, (128,), w["pos_ffn.layer_norm.weight"], w["pos_ffn.layer_norm.bias"], 1e-6)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true", help="time the HIP path only (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_cross_train_bench: needs a GPU", file=sys.stderr)
        return 2
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from pfpp_hip.matching_transformer import CrossAttentionLayer
    from pfpp_hip.matching_transformer_train import CrossAttentionTrainEngine

    cases = load_cases()
    dev = torch.device("cuda:0")
    layer = CrossAttentionLayer(128, 8)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.cross_state_dict().items()}, strict=True)
    layer.to(dev)
    eng = CrossAttentionTrainEngine(layer)
    puzzle_points = np.full(args.puzzles, args.points, dtype=np.int64)
    N = int(puzzle_points.sum())
    rng = np.random.default_rng(7)
    # rows of standard deviation 0.5: scaled scores up to 8 among 5,000 keys.  (At 1.0 they reach 32, and one of the 1.3 million ReLU
    # inputs of a puzzle lies within float32 rounding of 0: its sign, and with it that row's dx, then differs between any two orders.)
    x = torch.from_numpy((0.5 * rng.normal(size=(N, 128))).astype(np.float32)).to(dev)
    dout = torch.from_numpy(rng.normal(size=(N, 128)).astype(np.float32)).to(dev)
    w_eager = {k: p.detach().clone().requires_grad_(True) for k, p in eng.params.items()}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        res = fn()
        torch.cuda.synchronize()
        return res, torch.cuda.max_memory_allocated() / 2 ** 20

    def time_engine():
        eng.stage_events = []
        eng.forward(x, puzzle_points)
        dx = eng.backward(dout)
        torch.cuda.synchronize()
        ev, eng.stage_events = eng.stage_events, None
        spans, i = {}, 0
        for name in ENGINE_STAGES:                               # ("begin", e) opens forward and backward
            if ev[i][0] == "begin":
                i += 1
            spans[name] = ev[i - 1][1].elapsed_time(ev[i][1])
            i += 1
        return dx, spans

    def time_eager():
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        xe = x.detach().clone().requires_grad_(True)
        for p in w_eager.values():
            p.grad = None
        e[0].record()
        out = eager_forward(w_eager, xe, puzzle_points)
        e[1].record()
        (out * dout).sum().backward()
        e[2].record()
        torch.cuda.synchronize()
        return xe.grad, {"forward": e[0].elapsed_time(e[1]), "backward": e[1].elapsed_time(e[2])}

    if args.skip_eager:
        time_eager = lambda: (None, {"forward": float("nan"), "backward": float("nan")})
    for _ in range(args.warmup):
        dx_hip, _ = time_engine()
        dx_eager, _ = time_eager()
    agree = None
    if not args.skip_eager:
        worst = max(float((p.grad - w_eager[k].grad).abs().max() / w_eager[k].grad.abs().max()) for k, p in eng.params.items())
        agree = {"dx": float((dx_hip - dx_eager).abs().max() / dx_eager.abs().max()), "worst_parameter_gradient": worst}
        if N <= 5000:                      # small enough for float64 autograd on the device: which of the two is off, and by how much
            w64 = {k: p.detach().double().requires_grad_(True) for k, p in eng.params.items()}
            x64 = x.double().requires_grad_(True)
            (eager_forward(w64, x64, puzzle_points) * dout.double()).sum().backward()
            top = float(x64.grad.abs().max())
            agree["dx_vs_float64"] = {"engine": float((dx_hip.double() - x64.grad).abs().max()) / top,
                                      "eager": float((dx_eager.double() - x64.grad).abs().max()) / top}
            del w64, x64
    del dx_hip, dx_eager
    hip, eag, mem_hip, mem_eag = [], [], [], []
    for _ in range(args.repeats):          # alternating: both see the same clocks and the same neighbours on the machine
        (_, t), m = peak(time_engine)
        hip.append(t), mem_hip.append(m)
        (_, t), m = peak(time_eager)
        eag.append(t), mem_eag.append(m)
    med = lambda runs, k: statistics.median(r[k] for r in runs)
    tot = lambda runs: statistics.median(sum(r.values()) for r in runs)
    pair_flop = 224.0 * 8 * float((puzzle_points.astype(np.float64) ** 2).sum())          # 7 products of 16-wide rows per (query, key, head)
    line = {"bench": "matching_cross_train", "device": torch.cuda.get_device_name(0), "puzzles": args.puzzles, "points_per_puzzle": args.points,
            "points": N, "gemm_mode": "f32", "repeats": args.repeats, "warmup": args.warmup,
            "engine_ms": {**{k: round(med(hip, k), 4) for k in ENGINE_STAGES}, "total": round(tot(hip), 4)},
            "engine_total_ms_runs": [round(sum(r.values()), 3) for r in hip], "engine_peak_mib": round(max(mem_hip), 1),
            "attention_bwd_gflop": round(pair_flop / 1e9, 1), "attention_bwd_floor_ms_at_78.6_tflops": round(pair_flop / 78.6e12 * 1e3, 3)}
    if not args.skip_eager:
        line.update({"eager_ms": {"forward": round(med(eag, "forward"), 4), "backward": round(med(eag, "backward"), 4), "total": round(tot(eag), 4)},
                     "eager_total_ms_runs": [round(sum(r.values()), 3) for r in eag], "eager_peak_mib": round(max(mem_eag), 1),
                     "speedup_total": round(tot(eag) / tot(hip), 2), "eager_attention": "F.scaled_dot_product_attention per puzzle, fp32 autograd",
                     "rel_diff": agree})
    text = json.dumps(line)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
