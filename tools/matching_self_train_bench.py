"""Time forward + backward of the matcher's point-transformer layer through PointTransformerTrainEngine, per stage by HIP events, next
to PyTorch-ROCm eager fp32 autograd of the same layer in .train() on the same GPU, the two alternating.

    python tools/matching_self_train_bench.py [--shape batch16|one] [--repeats 3] [--warmup 2] [--out FILE]

Shapes: batch16 = 16 puzzles x 8 pieces x 625 points (80,000 points), one = one puzzle of 4,970 + 30 points.  Both
sides get the same injected neighbour lists (the engine's two searches of a first, untimed forward; the search is timed once, apart,
as `neighbours_ms`).  Stages of the engine: projection, the three statistics passes of the forward (bn3_stats, bn128_stats, tile) and
its finish pass; then bwd_w, bwd_u, bwd_r, the inverse lists (torch), the gather, the projection's GEMMs and the small gradients.  The
eager baseline: F.linear, the gathers, F.batch_norm(training=True) over all 16 N rows, softmax, einsum, loss = sum(out * dout),
loss.backward(); its stages are forward and backward.  Peak device memory of both is reported (inputs and weights are resident in
both).  Prints one JSON line (and writes it to --out): ms per call per stage, medians of `repeats` after `warmup` warm-ups; the
relative difference of out, dx and of the largest-deviating parameter gradient is reported, not asserted (parity is
tests/test_gpu_matching_self_train.py's business).  Reads nothing outside the repository."""
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
FWD_STAGES = ("projection", "neighbours", "bn3_stats", "bn128_stats", "tile", "finish")
BWD_STAGES = ("bwd_w", "bwd_u", "bwd_r", "inverse_lists", "gather", "projection_bwd", "small_grads")
SHAPES = {"batch16": [625] * (16 * 8), "one": [4970, 30]}
# vanish in exact arithmetic (linear_k.bias: where no slot is padded, as at both shapes): no relative difference to speak of
ZERO_GRADS = ("linear_p.0.bias", "linear_w.2.bias", "linear_q.bias", "linear_k.bias", "linear_w.5.bias")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_transformer_cases", ROOT / "tests" / "matching_transformer_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def eager_forward(w: dict, buf: dict, p: torch.Tensor, x: torch.Tensor, ik: torch.Tensor, iv: torch.Tensor) -> torch.Tensor:
    """attention_layer.py:190-225 in .train() on given lists (int64 [N, 16], N = the appended zero row)"""
    N = x.shape[0]
    lin = lambda v, name: F.linear(v, w[f"{name}.weight"], w[f"{name}.bias"])
    pad = lambda a: torch.cat([a, a.new_zeros(1, a.shape[1])], 0)

    def bn(v, name):
        rows = v.reshape(-1, v.shape[-1])
        return F.batch_norm(rows, buf[f"{name}.running_mean"], buf[f"{name}.running_var"], w[f"{name}.weight"], w[f"{name}.bias"], True, 0.1,
                            1e-5).reshape(v.shape)

    x_q, x_k, x_v = lin(x, "linear_q"), lin(x, "linear_k"), lin(x, "linear_v")
    g_k, g_v = pad(x_k)[ik], pad(x_v)[iv]
    g_p = (pad(p)[ik] - p[:, None, :]) * (ik < N).to(x.dtype)[..., None]
    p_r = lin(torch.relu(bn(lin(g_p, "linear_p.0"), "linear_p.1")), "linear_p.3")
    h = torch.relu(bn(g_k - x_q[:, None, :] + p_r, "linear_w.0"))
    h = torch.relu(bn(lin(h, "linear_w.2"), "linear_w.3"))
    wgt = torch.softmax(lin(h, "linear_w.5"), dim=1)
    return torch.einsum("ntsi,nti->nsi", (g_v + p_r).reshape(N, 16, 8, 16), wgt).reshape(N, 128)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="batch16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true", help="time the HIP path only (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_self_train_bench: needs a GPU", file=sys.stderr)
        return 2
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from pfpp_hip.matching_transformer import PointTransformerLayer
    from pfpp_hip.matching_transformer_train import PointTransformerTrainEngine

    cases = load_cases()
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.ptf_state_dict().items()}
    layer = PointTransformerLayer(128, 128, 8, 16)
    layer.load_state_dict(sd, strict=True)
    layer.to(dev)
    eng = PointTransformerTrainEngine(layer)
    lengths = np.asarray(SHAPES[args.shape], dtype=np.int64)
    N = int(lengths.sum())
    rng = np.random.default_rng(7)
    pts = np.concatenate([rng.normal(0, 0.5, 3) + 0.2 * rng.normal(size=(n, 3)) for n in lengths]).astype(np.float32)
    feats = (np.sin(pts.astype(np.float64) @ rng.normal(0, 3.0, (3, 128)) + rng.uniform(0, 2 * np.pi, 128)) + 0.3 * rng.normal(size=(N, 128))).astype(np.float32)
    p, x = torch.from_numpy(pts).to(dev), torch.from_numpy(feats).to(dev)
    dout = torch.from_numpy(rng.normal(size=(N, 128)).astype(np.float32)).to(dev)
    w_eager = {k: v.detach().clone().requires_grad_(True) for k, v in eng.params.items()}
    buf_eager = {k: v.detach().clone() for k, v in layer.named_buffers() if not k.endswith("num_batches_tracked")}

    # the lists both sides use, and what the two searches cost
    eng.stage_events = []
    eng.forward(p, x, lengths)
    torch.cuda.synchronize()
    ev = dict(eng.stage_events)
    neighbours_ms = ev["projection"].elapsed_time(ev["neighbours"])
    eng.stage_events = None
    lists = (eng.saved["idx_k"], eng.saved["idx_v"])
    ik, iv = (t.long() for t in lists)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        res = fn()
        torch.cuda.synchronize()
        return res, torch.cuda.max_memory_allocated() / 2 ** 20

    def time_engine():
        eng.stage_events = []
        out = eng.forward(p, x, lengths, indices=lists)
        dx = eng.backward(dout)
        torch.cuda.synchronize()
        ev, eng.stage_events = eng.stage_events, None
        spans, i = {}, 0
        for name in FWD_STAGES + BWD_STAGES:                     # ("begin", e) opens forward and backward
            if ev[i][0] == "begin":
                i += 1
            assert ev[i][0] == name, (ev[i][0], name)
            spans[name] = ev[i - 1][1].elapsed_time(ev[i][1])
            i += 1
        return (out, dx), spans

    def time_eager():
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        xe = x.detach().clone().requires_grad_(True)
        for v in w_eager.values():
            v.grad = None
        e[0].record()
        out = eager_forward(w_eager, buf_eager, p, xe, ik, iv)
        e[1].record()
        (out * dout).sum().backward()
        e[2].record()
        torch.cuda.synchronize()
        return (out.detach(), xe.grad), {"forward": e[0].elapsed_time(e[1]), "backward": e[1].elapsed_time(e[2])}

    if args.skip_eager:
        time_eager = lambda: ((None, None), {"forward": float("nan"), "backward": float("nan")})
    for _ in range(args.warmup):
        (out_hip, dx_hip), _ = time_engine()
        (out_eager, dx_eager), _ = time_eager()
    agree = None
    if not args.skip_eager:
        diffs = {k: float((v.grad - w_eager[k].grad).abs().max() / w_eager[k].grad.abs().max()) for k, v in eng.params.items() if k not in ZERO_GRADS}
        worst = max(diffs, key=diffs.get)
        ddx = (dx_hip - dx_eager).abs() / dx_eager.abs().max()
        # a ReLU input within float32 rounding of 0 takes either sign, and the rows it feeds then differ by far more than rounding:
        # the share of dx entries beyond 1e-5 of the maximum says how local the difference is
        agree = {"out": float((out_hip - out_eager).abs().max() / out_eager.abs().max()), "dx": float(ddx.max()),
                 "dx_share_above_1e-5": float((ddx > 1e-5).double().mean()), "worst_parameter_gradient": [worst, diffs[worst]]}
        del ddx
    del out_hip, dx_hip, out_eager, dx_eager
    hip, eag, mem_hip, mem_eag = [], [], [], []
    for _ in range(args.repeats):          # alternating: both see the same clocks and the same neighbours on the machine
        (_, t), m = peak(time_engine)
        hip.append(t), mem_hip.append(m)
        (_, t), m = peak(time_eager)
        eag.append(t), mem_eag.append(m)
    med = lambda runs, k: statistics.median(r[k] for r in runs)
    tot = lambda runs: statistics.median(sum(v for k, v in r.items() if k != "neighbours") for r in runs)
    # the 128-wide work per point: the 16 x 16 x 128 product once in the forward (tile) and three times in the backward (dW2 in bwd_u,
    # dh1 in bwd_u, bwd_r and the gather), 2 FLOP per multiply-add; a guide figure at the plain-FMA rate, not a measurement
    wide_flop = 2.0 * 16 * 16 * 128 * N * 5
    line = {"bench": "matching_self_train", "device": torch.cuda.get_device_name(0), "shape": args.shape, "pieces": len(lengths), "points": N,
            "gemm_mode": "f32", "repeats": args.repeats, "warmup": args.warmup, "neighbours_ms": round(neighbours_ms, 4),
            "engine_ms": {**{k: round(med(hip, k), 4) for k in FWD_STAGES + BWD_STAGES if k != "neighbours"}, "total": round(tot(hip), 4)},
            "engine_total_ms_runs": [round(sum(v for k, v in r.items() if k != "neighbours"), 3) for r in hip], "engine_peak_mib": round(max(mem_hip), 1),
            "wide_passes_gflop": round(wide_flop / 1e9, 2), "wide_passes_floor_ms_at_78.6_tflops": round(wide_flop / 78.6e12 * 1e3, 4)}
    if not args.skip_eager:
        line.update({"eager_ms": {"forward": round(med(eag, "forward"), 4), "backward": round(med(eag, "backward"), 4), "total": round(tot(eag), 4)},
                     "eager_total_ms_runs": [round(sum(r.values()), 3) for r in eag], "eager_peak_mib": round(max(mem_eag), 1),
                     "speedup_total": round(tot(eag) / tot(hip), 2), "rel_diff": agree})
    text = json.dumps(line)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
