"""Time one training step of the matcher's DGCNN encoder on the GPU: forward (batch statistics) + backward + Adam for 16 puzzles of
8 x 625 points in one call (tools/matching_dgcnn_bench.py's batch), per stage by HIP events, next to the reference's form in
PyTorch-ROCm eager fp32 under autograd with torch.optim.Adam on the same GPU, the two alternating in one process.

    python tools/matching_dgcnn_train_bench.py [--puzzles 16] [--pieces 8] [--points 625] [--repeats 5] [--skip-eager]

The eager baseline is written for this batch, whose pieces all have one size: per level cdist + topk(20) per piece (batched, no
gradient), a gather to [N, 20, 2 C] = cat(x_j - x_i, x_i), conv (F.linear), F.batch_norm(training=True) over all N x 20 rows,
LeakyReLU, max over the slots; then conv5 with its BatchNorm over N rows; loss = sum(out * dout); backward; Adam.  Its distances are
summed in another order, so a near-tie may fall the other way; parity is tests/test_gpu_matching_dgcnn_train.py's business.

Prints one JSON line: ms per stage (medians of `repeats` after two warm-up pairs), the inverse-list plumbing as a stage of its own,
the ratio to eager, the train forward's cost over the eval forward measured in the same process, and the peak device memory per point
of one step of either path."""
from __future__ import annotations

import argparse
import importlib.util
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))
FWD = tuple(f"{s}{l}" for l in range(1, 5) for s in ("search", "inverse_lists", "product", "stats", "apply")) + ("conv5",)
BWD = ("conv5_bwd",) + tuple(f"{s}{l}{t}" for l in (4, 3, 2, 1) for s, t in (("gathers", ""), ("products", "_bwd")))
GROUPS = {"searches": [f"search{l}" for l in range(1, 5)], "inverse_lists": [f"inverse_lists{l}" for l in range(1, 5)],
          "forward_products": [f"product{l}" for l in range(1, 5)], "stats_extremum": [f"stats{l}" for l in range(1, 5)],
          "apply": [f"apply{l}" for l in range(1, 5)], "conv5_forward": ["conv5"], "conv5_backward": ["conv5_bwd"],
          "backward_gathers": [f"gathers{l}" for l in range(1, 5)], "backward_products": [f"products{l}_bwd" for l in range(1, 5)], "adam": ["adam"]}


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_dgcnn_cases", ROOT / "tests" / "matching_dgcnn_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Eager(torch.nn.Module):
    """the reference's form in eager PyTorch in .train() for pieces of one size: tensors [P, n, C]"""

    def __init__(self, enc):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(getattr(enc, f"conv{l}")[0].weight.detach()[:, :, 0].clone()) for l in range(1, 6)])
        self.g = torch.nn.ParameterList([torch.nn.Parameter(getattr(enc, f"bn{l}").weight.detach().clone()) for l in range(1, 6)])
        self.b = torch.nn.ParameterList([torch.nn.Parameter(getattr(enc, f"bn{l}").bias.detach().clone()) for l in range(1, 6)])
        for l in range(1, 6):
            self.register_buffer(f"rm{l}", getattr(enc, f"bn{l}").running_mean.detach().clone())
            self.register_buffer(f"rv{l}", getattr(enc, f"bn{l}").running_var.detach().clone())

    def forward(self, x):
        F = torch.nn.functional
        P, n, _ = x.shape
        r3 = torch.arange(P, device=x.device)[:, None, None]
        feats = []
        for l in range(4):
            with torch.no_grad():
                idx = torch.cdist(x, x).topk(20, dim=2, largest=False)[1]            # [P, n, 20]
            nb = x[r3, idx]                                                          # [P, n, 20, C]
            own = x[:, :, None, :].expand_as(nb)
            z = F.linear(torch.cat([nb - own, own], -1), self.w[l])                  # [P, n, 20, C_out]
            z = F.batch_norm(z.reshape(P * n * 20, -1), getattr(self, f"rm{l + 1}"), getattr(self, f"rv{l + 1}"), self.g[l], self.b[l], True, 0.1, 1e-5)
            x = F.leaky_relu(z, 0.2).reshape(P, n, 20, -1).max(2)[0]
            feats.append(x)
        z = F.linear(torch.cat(feats, -1).reshape(P * n, -1), self.w[4])
        return F.leaky_relu(F.batch_norm(z, self.rm5, self.rv5, self.g[4], self.b[4], True, 0.1, 1e-5), 0.2)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--pieces", type=int, default=8)
    ap.add_argument("--points", type=int, default=625)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true", help="time the HIP path only (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_dgcnn_train_bench: needs a GPU", file=sys.stderr)
        return 2
    from pfpp_hip.matching_dgcnn import DGCNNDynamic
    from pfpp_hip.matching_dgcnn_train import DGCNNTrainEngine

    cases = load_cases()
    dev = torch.device("cuda:0")
    enc = DGCNNDynamic(cases.FEAT, False, 3)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.state_dict().items()}, strict=True)
    enc.to(dev)
    eng = DGCNNTrainEngine(enc)
    P, n = args.puzzles * args.pieces, args.points
    N = P * n
    rng = np.random.default_rng(5)
    d = rng.normal(size=(P, n, 3))
    pts = (0.4 * d / np.linalg.norm(d, axis=-1, keepdims=True) * (1 + 0.05 * rng.normal(size=(P, n, 1)))).astype(np.float32)
    x = torch.from_numpy(pts).to(dev)
    flat = x.reshape(-1, 3)
    dout = torch.from_numpy(rng.standard_normal((N, cases.FEAT)).astype(np.float32) / N).to(dev)
    lengths = np.full(P, n, dtype=np.int64)
    eager = Eager(enc).to(dev)
    opt = torch.optim.Adam(eager.parameters(), lr=1e-4)

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def time_hip():
        eng.stage_events = []
        eng.forward(flat, lengths)
        eng.backward(dout)
        eng._mark("pre_adam")
        eng.optimizer_step(lr=1e-4)
        eng._mark("adam")
        torch.cuda.synchronize()
        ev, eng.stage_events = eng.stage_events, None
        names = [name for name, _ in ev]
        assert names == ["begin"] + list(FWD) + ["begin"] + list(BWD) + ["pre_adam", "adam"], names
        t = {name: ev[i][1].elapsed_time(ev[i + 1][1]) for i, name in enumerate(names[1:])}
        t.pop("begin")                                       # the gap between forward() and backward(): host work only
        t.pop("pre_adam")
        return t

    def time_eval():
        a = event()
        enc(flat, lengths)
        b = event()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def time_eager():
        ev = [event()]
        out = eager(x)
        ev.append(event())
        opt.zero_grad(set_to_none=True)
        (out * dout).sum().backward()
        ev.append(event())
        opt.step()
        ev.append(event())
        torch.cuda.synchronize()
        return {k: ev[i].elapsed_time(ev[i + 1]) for i, k in enumerate(("forward", "backward", "adam"))}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - before) / N

    if args.skip_eager:
        time_eager = lambda: {k: float("nan") for k in ("forward", "backward", "adam")}
    for _ in range(args.warmup):
        time_hip()
        time_eager()
    hip, eag, evl = [], [], []
    for _ in range(args.repeats):          # alternating: both see the same clocks and the same neighbours on the machine
        hip.append(time_hip())
        evl.append(time_eval())
        eag.append(time_eager())
    mem_hip = peak(time_hip)
    mem_eager = None if args.skip_eager else peak(time_eager)
    med = lambda runs, k: statistics.median(r[k] for r in runs)
    tot = lambda runs: statistics.median(sum(r.values()) for r in runs)
    groups = {g: round(sum(med(hip, k) for k in ks), 4) for g, ks in GROUPS.items()}
    fwd_ms = statistics.median(sum(r[k] for k in FWD) for r in hip)
    line = {"bench": "matching_dgcnn_train", "device": torch.cuda.get_device_name(0), "puzzles": args.puzzles, "pieces": args.pieces,
            "points_per_piece": n, "points": N, "gemm_mode": "f32", "repeats": args.repeats, "warmup_pairs": args.warmup,
            "hip_ms": {**{k: round(med(hip, k), 4) for k in FWD + BWD + ("adam",)}, "total": round(tot(hip), 4)},
            "hip_ms_by_stage": groups, "dominant_stage": max(groups, key=groups.get),
            "hip_total_ms_runs": [round(sum(r.values()), 3) for r in hip],
            "hip_train_forward_ms": round(fwd_ms, 4), "hip_eval_forward_ms": round(statistics.median(evl), 4),
            "train_forward_over_eval_forward": round(fwd_ms / statistics.median(evl), 3),
            "hip_peak_bytes_per_point": round(mem_hip, 1)}
    if not args.skip_eager:
        line.update({"eager_ms": {**{k: round(med(eag, k), 4) for k in ("forward", "backward", "adam")}, "total": round(tot(eag), 4)},
                     "eager_total_ms_runs": [round(sum(r.values()), 3) for r in eag], "speedup_total": round(tot(eag) / tot(hip), 2),
                     "eager_peak_bytes_per_point": round(mem_eager, 1)})
    text = json.dumps(line)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
