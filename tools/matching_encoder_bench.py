"""Time the matcher's ragged PointNet++ encoder on the GPU: 16 puzzles of 8 x 625 points in one call (tools/matching_bench.py's
batch), per stage by HIP events, next to the same steps in PyTorch-ROCm eager fp32 on the same GPU, the two alternating.

    python tools/matching_encoder_bench.py [--puzzles 16] [--pieces 8] [--points 625] [--repeats 3] [--mode f32]

The eager baseline is written for this batch, whose pieces all have one size: a Python farthest-point loop over all pieces at once
(one iteration per sample), dense cdist + topk per piece (batched), gathers, F.linear with the folded BatchNorm, max / weighted sum.
Its sampling sums the squares in another order, so a chain may fork: the relative difference of the two results is reported, not
asserted (parity is tests/test_gpu_matching_encoder.py's business).  Prints one JSON line: ms per puzzle per stage, medians of `repeats` after a warm-up."""
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
STAGES = ("sampling", "neighbours", "set_abstraction", "propagation")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_encoder_cases", ROOT / "tests" / "matching_encoder_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Eager:
    """the encoder in eager PyTorch for pieces of one size: tensors [P, n, ...]"""

    def __init__(self, enc):
        from pfpp_hip.matching_encoder import fold_batchnorm

        self.sa = [[[fold_batchnorm(c.weight, c.bias, b) for c, b in zip(convs, bns)] for convs, bns in zip(sa.conv_blocks, sa.bn_blocks)]
                   for sa in (enc.sa1, enc.sa2, enc.sa3, enc.sa4)]
        self.fp = [[fold_batchnorm(c.weight, c.bias, b) for c, b in zip(fp.mlp_convs, fp.mlp_bns)] for fp in (enc.fp4, enc.fp3, enc.fp2, enc.fp1)]
        self.conv1 = (enc.conv1.weight.detach().reshape(enc.feat_out, -1), enc.conv1.bias.detach())

    @staticmethod
    def fps(xyz, m, start):
        P, n, _ = xyz.shape
        dist = torch.full((P, n), float("inf"), device=xyz.device)
        cur, out, rows = start.clone(), [], torch.arange(P, device=xyz.device)
        for _ in range(m):
            out.append(cur)
            d = xyz - xyz[rows, cur][:, None, :]
            dist = torch.minimum(dist, (d * d).sum(-1))
            cur = dist.argmax(1)
        return torch.stack(out, 1)

    @staticmethod
    def mlp(a, layers):
        for w, s, t in layers:
            a = torch.relu(torch.nn.functional.linear(a, w) * s + t)
        return a

    def __call__(self, x, counts, start, mark):
        P = x.shape[0]
        rows = torch.arange(P, device=x.device)[:, None]
        xyz = [x]
        for l in range(4):
            c = self.fps(xyz[l], counts[l + 1], start[l])
            xyz.append(xyz[l][rows, c])
        mark("sampling")
        nbr = [torch.cdist(xyz[l + 1], xyz[l]).topk(min(32, counts[l]), dim=2, largest=False)[1] for l in range(4)]
        back = [(torch.cdist(xyz[l], xyz[l + 1]) ** 2).topk(min(3, counts[l + 1]), dim=2, largest=False) for l in range(4)]
        mark("neighbours")
        feats = [x]
        r3 = torch.arange(P, device=x.device)[:, None, None]
        for l in range(4):
            outs = []
            for layers, K in zip(self.sa[l], (16, 32)):
                g = nbr[l][:, :, :K]
                a = torch.cat([feats[l][r3, g], xyz[l][r3, g] - xyz[l + 1][:, :, None, :]], -1)
                outs.append(self.mlp(a, layers).max(2)[0])
            feats.append(torch.cat(outs, -1))
        mark("set_abstraction")
        up = feats[4]
        for l, layers in zip((3, 2, 1, 0), self.fp):
            d, g = back[l]
            r = 1.0 / (d + 1e-8)
            w = r / r.sum(-1, keepdim=True)
            it = (up[r3, g] * w[..., None]).sum(2)
            up = self.mlp(torch.cat([feats[l], it], -1) if l > 0 else it, layers)
        y = torch.nn.functional.linear(up, *self.conv1)
        mark("propagation")
        return y.reshape(-1, y.shape[-1])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--pieces", type=int, default=8)
    ap.add_argument("--points", type=int, default=625)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="f32", choices=("f32", "f16x3"))
    ap.add_argument("--skip-eager", action="store_true", help="time the HIP path only (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_encoder_bench: needs a GPU", file=sys.stderr)
        return 2
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic, level_counts

    cases = load_cases()
    dev = torch.device("cuda:0")
    enc = PointNet2PTMSGDynamic(3, 128, gemm_mode=args.mode)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.encoder_state_dict().items()}, strict=True)
    enc.to(dev)
    P, n = args.puzzles * args.pieces, args.points
    rng = np.random.default_rng(5)
    d = rng.normal(size=(P, n, 3))
    pts = (0.4 * d / np.linalg.norm(d, axis=-1, keepdims=True) * (1 + 0.05 * rng.normal(size=(P, n, 1)))).astype(np.float32)
    x = torch.from_numpy(pts).to(dev)
    lengths = np.full(P, n, dtype=np.int64)
    counts = level_counts(lengths)[:, 0].tolist()
    start = np.zeros((P, 4), dtype=np.int64)
    eager = Eager(enc)
    start_d = [torch.zeros(P, dtype=torch.int64, device=dev) for _ in range(4)]

    def time_hip():
        enc.stage_events = []
        y = enc(x.reshape(-1, 3), lengths, start=start)
        torch.cuda.synchronize()
        ev, enc.stage_events = enc.stage_events, None
        return y, {name: ev[i][1].elapsed_time(ev[i + 1][1]) for i, name in enumerate(STAGES)}

    def time_eager():
        ev = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

        with torch.no_grad():
            mark("begin")
            y = eager(x, counts, start_d, mark)
        torch.cuda.synchronize()
        return y, {name: ev[i].elapsed_time(ev[i + 1]) for i, name in enumerate(STAGES)}

    if args.skip_eager:
        time_eager = lambda: (None, {k: float("nan") for k in STAGES})
    for _ in range(args.warmup):
        y_hip, _ = time_hip()
        y_eager, _ = time_eager()
    agree = None if args.skip_eager else float((y_hip - y_eager).abs().max() / y_eager.abs().max())
    hip, eag = [], []
    for _ in range(args.repeats):          # alternating: both see the same clocks and the same neighbours on the machine
        hip.append(time_hip()[1])
        eag.append(time_eager()[1])
    med = lambda runs, k: statistics.median(r[k] for r in runs) / args.puzzles
    tot = lambda runs: statistics.median(sum(r.values()) for r in runs) / args.puzzles
    line = {"bench": "matching_encoder", "device": torch.cuda.get_device_name(0), "puzzles": args.puzzles, "pieces": args.pieces,
            "points_per_piece": n, "gemm_mode": args.mode, "repeats": args.repeats, "level_counts": counts,
            "hip_ms_per_puzzle": {**{k: round(med(hip, k), 4) for k in STAGES}, "total": round(tot(hip), 4)},
            "hip_total_ms_runs": [round(sum(r.values()), 3) for r in hip]}
    if not args.skip_eager:
        line.update({"eager_ms_per_puzzle": {**{k: round(med(eag, k), 4) for k in STAGES}, "total": round(tot(eag), 4)},
                     "eager_total_ms_runs": [round(sum(r.values()), 3) for r in eag], "speedup_total": round(tot(eag) / tot(hip), 2),
                     "descriptors_rel_diff": agree})
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
