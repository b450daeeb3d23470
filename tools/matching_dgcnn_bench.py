"""Time the matcher's DGCNN encoder (forward, eval mode) on the GPU: 16 puzzles of 8 x 625 points in one call (tools/matching_bench.py's
batch), per stage by HIP events, next to the reference's form in PyTorch-ROCm eager fp32 on the same GPU, the two alternating.

    python tools/matching_dgcnn_bench.py [--puzzles 16] [--pieces 8] [--points 625] [--repeats 5] [--skip-eager]

The eager baseline is written for this batch, whose pieces all have one size: per level cdist + topk(20) per piece (batched), a
gather to [N, 20, 2 C] = cat(x_j - x_i, x_i), F.linear, the folded BatchNorm, LeakyReLU, max over the slots; then conv5.  Its distances
are summed in another order, so a near-tie between the 20th and 21st neighbour may fall the other way: the share of rows whose
neighbour sets differ and the relative difference of the two results are reported, not asserted (parity is
tests/test_gpu_matching_dgcnn.py's business).

Prints one JSON line: ms per puzzle per stage (medians of `repeats` after a warm-up), the ratio to eager, and per kernel family the
work the algorithm needs (computed from the shapes here) over its time: fp32 vector operations per second for the searches (three
unfused operations per channel and pair, against 78.6e12 instructions/s = half the 157.3 TFLOP/s that counts an FMA as two), FLOP/s
for the products (against 157.3e12) and bytes/s for the extremum passes (20 gathered rows of u, one of v, the lists, one row written)."""
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
LEVELS = ((3, 64), (64, 64), (64, 128), (128, 256))        # (C_in, C_out)
STAGES = tuple(f"{s}{l}" for l in range(1, 5) for s in ("search", "product", "extremum")) + ("conv5",)
EAGER_STAGES = tuple(f"level{l}" for l in range(1, 5)) + ("conv5",)
VALU_PEAK, FLOP_PEAK = 78.6e12, 157.3e12


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_dgcnn_cases", ROOT / "tests" / "matching_dgcnn_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Eager:
    """the reference's form in eager PyTorch for pieces of one size: tensors [P, n, C]"""

    def __init__(self, enc):
        self.layers = []
        for l in range(1, 6):
            conv, bn = getattr(enc, f"conv{l}")[0], getattr(enc, f"bn{l}")
            s = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
            self.layers.append((conv.weight.detach()[:, :, 0].contiguous(), s, bn.bias.detach() - bn.running_mean * s))

    def __call__(self, x, mark):
        P, n, _ = x.shape
        r3 = torch.arange(P, device=x.device)[:, None, None]
        feats, lists = [], []
        for l in range(4):
            w, s, t = self.layers[l]
            idx = torch.cdist(x, x).topk(20, dim=2, largest=False)[1]                # [P, n, 20]
            nb = x[r3, idx]                                                          # [P, n, 20, C]
            own = x[:, :, None, :].expand_as(nb)
            f = torch.cat([nb - own, own], -1)
            y = torch.nn.functional.leaky_relu(torch.nn.functional.linear(f, w) * s + t, 0.2)
            x = y.max(2)[0]
            feats.append(x)
            lists.append(idx)
            mark(f"level{l + 1}")
        w, s, t = self.layers[4]
        y = torch.nn.functional.leaky_relu(torch.nn.functional.linear(torch.cat(feats, -1), w) * s + t, 0.2)
        mark("conv5")
        return y.reshape(P * n, -1), lists


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--pieces", type=int, default=8)
    ap.add_argument("--points", type=int, default=625)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true", help="time the HIP path only (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_dgcnn_bench: needs a GPU", file=sys.stderr)
        return 2
    from pfpp_hip.matching_dgcnn import DGCNNDynamic

    cases = load_cases()
    dev = torch.device("cuda:0")
    enc = DGCNNDynamic(cases.FEAT, False, 3)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.state_dict().items()}, strict=True)
    enc.to(dev)
    P, n = args.puzzles * args.pieces, args.points
    N = P * n
    rng = np.random.default_rng(5)
    d = rng.normal(size=(P, n, 3))
    pts = (0.4 * d / np.linalg.norm(d, axis=-1, keepdims=True) * (1 + 0.05 * rng.normal(size=(P, n, 1)))).astype(np.float32)
    x = torch.from_numpy(pts).to(dev)
    lengths = np.full(P, n, dtype=np.int64)
    eager = Eager(enc)

    def time_hip():
        enc.stage_events = []
        y, lv = enc(x.reshape(-1, 3), lengths, return_levels=True)
        torch.cuda.synchronize()
        ev, enc.stage_events = enc.stage_events, None
        assert [name for name, _ in ev[1:]] == list(STAGES)
        return y, lv, {name: ev[i][1].elapsed_time(ev[i + 1][1]) for i, name in enumerate(STAGES)}

    def time_eager():
        ev = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

        with torch.no_grad():
            mark("begin")
            y, lists = eager(x, mark)
        torch.cuda.synchronize()
        return y, lists, {name: ev[i].elapsed_time(ev[i + 1]) for i, name in enumerate(EAGER_STAGES)}

    if args.skip_eager:
        time_eager = lambda: (None, None, {k: float("nan") for k in EAGER_STAGES})
    for _ in range(args.warmup):
        y_hip, lv, _ = time_hip()
        y_eager, lists, _ = time_eager()
    agree = sets = None
    if not args.skip_eager:
        agree = float((y_hip - y_eager).abs().max() / y_eager.abs().max())
        base = (torch.arange(P, device=dev) * n)[:, None, None]
        sets = [float(((lists[l] + base).reshape(N, 20).sort(1)[0] != lv[f"l{l + 1}_knn"].long().sort(1)[0]).any(1).float().mean()) for l in range(4)]
    del y_eager, lists
    hip, eag = [], []
    for _ in range(args.repeats):          # alternating: both see the same clocks and the same neighbours on the machine
        hip.append(time_hip()[2])
        eag.append(time_eager()[2])
    med = lambda runs, k: statistics.median(r[k] for r in runs)
    tot = lambda runs: statistics.median(sum(r.values()) for r in runs)
    # the work the algorithm needs, from the shapes
    rates = {}
    for l, (c_in, c_out) in enumerate(LEVELS, 1):
        ops = 3.0 * N * n * c_in                                                     # sub, mul, add per channel and (query, candidate) pair
        flop = 2.0 * N * c_in * 2 * c_out
        byts = 4.0 * N * (20 * c_out + c_out + 20 + c_out)
        t_s, t_p, t_e = (med(hip, f"{s}{l}") * 1e-3 for s in ("search", "product", "extremum"))
        rates[f"level{l}"] = {"search_valu_ops_per_s": round(ops / t_s, -9), "search_share_of_valu_peak": round(ops / t_s / VALU_PEAK, 4),
                              "product_flop_per_s": round(flop / t_p, -9), "product_share_of_fp32_peak": round(flop / t_p / FLOP_PEAK, 4),
                              "extremum_bytes_per_s": round(byts / t_e, -9)}
    flop5 = 2.0 * N * 512 * cases.FEAT
    rates["conv5"] = {"flop_per_s_with_the_leaky_pass": round(flop5 / (med(hip, "conv5") * 1e-3), -9)}
    line = {"bench": "matching_dgcnn", "device": torch.cuda.get_device_name(0), "puzzles": args.puzzles, "pieces": args.pieces,
            "points_per_piece": n, "gemm_mode": "f32", "repeats": args.repeats,
            "hip_ms_per_puzzle": {**{k: round(med(hip, k) / args.puzzles, 4) for k in STAGES}, "total": round(tot(hip) / args.puzzles, 4)},
            "hip_total_ms_runs": [round(sum(r.values()), 3) for r in hip], "achieved": rates}
    if not args.skip_eager:
        line.update({"eager_ms_per_puzzle": {**{k: round(med(eag, k) / args.puzzles, 4) for k in EAGER_STAGES}, "total": round(tot(eag) / args.puzzles, 4)},
                     "eager_total_ms_runs": [round(sum(r.values()), 3) for r in eag], "speedup_total": round(tot(eag) / tot(hip), 2),
                     "descriptors_rel_diff": agree, "rows_with_another_neighbour_set_per_level": sets})
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
