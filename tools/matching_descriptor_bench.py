"""Time the matcher's point-transformer and cross-attention layers on the GPU, per stage by HIP events, next to the same steps in
PyTorch-ROCm eager fp32 on the same GPU, the two alternating.

    python tools/matching_descriptor_bench.py [--puzzles 16] [--pieces 8] [--points 625] [--repeats 3] [--mode f32]
    python tools/matching_descriptor_bench.py --lengths 4970,30          # one puzzle with the largest piece the workload has

Stages: projection (q | k | v GEMM), the two neighbour searches in feature space, the aggregation, and for the cross layer its
projection, the attention and the dense tail (fc + LayerNorm + feed-forward + LayerNorm).  The eager baseline: F.linear, per group of
equally long pieces a batched squared-distance matrix (torch.cdist) + topk, gathers that materialise the [N, 16, 128] tensors, the
folded BatchNorms, softmax and einsum; per group of equally long puzzles F.scaled_dot_product_attention (what PyTorch-ROCm
dispatches it to is its business), F.linear and F.layer_norm.  Its distances sum in another order, so a neighbour list may differ:
the relative difference of the results is reported, not asserted (parity is tests/test_gpu_matching_transformer.py's business).
Prints one JSON line: ms per call per stage, medians of `repeats` after `warmup` warm-ups."""
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
SELF_STAGES = ("projection", "neighbours_k", "neighbours_v", "aggregate")
CROSS_STAGES = ("projection", "attention", "tail")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_transformer_cases", ROOT / "tests" / "matching_transformer_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def groups(lengths):
    """equal lengths -> (length, row offsets of the members): the eager path batches them"""
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [(int(n), [int(off[i]) for i in np.flatnonzero(lengths == n)]) for n in np.unique(lengths)]


class EagerSelf:
    def __init__(self, layer):
        from pfpp_hip.matching_transformer import _fold

        pack = layer._packed()
        self.w_qkv, self.b_qkv = pack["w_qkv"], pack["b_qkv"]
        p0, pbn, p3 = layer.linear_p[0], layer.linear_p[1], layer.linear_p[3]
        self.p0, self.p_st, self.p3 = p0.weight.detach(), _fold(pbn, p0.bias), (p3.weight.detach(), p3.bias.detach())
        self.w_st0 = _fold(layer.linear_w[0])
        self.w2, self.w_st3 = layer.linear_w[2].weight.detach(), _fold(layer.linear_w[3], layer.linear_w[2].bias)
        self.w5 = (layer.linear_w[5].weight.detach(), layer.linear_w[5].bias.detach())

    def knn(self, rows, lengths):
        idx = torch.empty((rows.shape[0], 16), dtype=torch.int64, device=rows.device)
        for n, offs in groups(lengths):
            a = torch.stack([rows[o:o + n] for o in offs])
            nb = torch.cdist(a, a).topk(16, dim=2, largest=False)[1]
            for g, o in enumerate(offs):
                idx[o:o + n] = nb[g] + o
        return idx

    def __call__(self, p, x, lengths, mark):
        qkv = F.linear(x, self.w_qkv, self.b_qkv)
        xq, xk, xv = qkv[:, :128], qkv[:, 128:256], qkv[:, 256:]
        mark("projection")
        ik = self.knn(xk, lengths)
        mark("neighbours_k")
        iv = self.knn(xv, lengths)
        mark("neighbours_v")
        h = torch.relu(F.linear(p[ik] - p[:, None, :], self.p0) * self.p_st[0] + self.p_st[1])
        p_r = F.linear(h, *self.p3)
        r = xk[ik] - xq[:, None, :] + p_r
        h = torch.relu(r * self.w_st0[0] + self.w_st0[1])
        h = torch.relu(F.linear(h, self.w2) * self.w_st3[0] + self.w_st3[1])
        w = torch.softmax(F.linear(h, *self.w5), dim=1)
        out = torch.einsum("ntsi,nti->nsi", (xv[iv] + p_r).reshape(-1, 16, 8, 16), w).reshape(-1, 128)
        mark("aggregate")
        return out


class EagerCross:
    def __init__(self, layer):
        self.k = layer._packed()

    def __call__(self, x, puzzle_points, mark):
        k = self.k
        qkv = F.linear(x, k["w_qkv"])
        mark("projection")
        att = torch.empty_like(x)
        for n, offs in groups(puzzle_points):
            t = torch.stack([qkv[o:o + n] for o in offs]).reshape(len(offs), n, 3, 8, 16).permute(2, 0, 3, 1, 4)
            o_ = F.scaled_dot_product_attention(t[0], t[1], t[2]).transpose(1, 2).reshape(len(offs), n, 128)
            for g, o in enumerate(offs):
                att[o:o + n] = o_[g]
        mark("attention")
        y = F.layer_norm(F.linear(att, k["fc"]) + x, (128,), k["g1"], k["b1"], 1e-6)
        z = F.linear(torch.relu(F.linear(y, k["w1"], k["bw1"])), k["w2"], k["bw2"]) + y
        out = F.layer_norm(z, (128,), k["g2"], k["b2"], 1e-6)
        mark("tail")
        return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--pieces", type=int, default=8)
    ap.add_argument("--points", type=int, default=625)
    ap.add_argument("--lengths", default=None, help="piece lengths of ONE puzzle, comma separated (instead of --puzzles/--pieces/--points)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="f32", choices=("f32", "f16x3"))
    ap.add_argument("--skip-eager", action="store_true", help="time the HIP path only (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_descriptor_bench: needs a GPU", file=sys.stderr)
        return 2
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from pfpp_hip.matching_transformer import CrossAttentionLayer, PointTransformerLayer

    cases = load_cases()
    dev = torch.device("cuda:0")
    s_layer = PointTransformerLayer(128, 128, n_heads=8, nsampmle=16, gemm_mode=args.mode)
    c_layer = CrossAttentionLayer(128, 8, gemm_mode=args.mode)
    s_layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.ptf_state_dict().items()}, strict=True)
    c_layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.cross_state_dict().items()}, strict=True)
    s_layer.to(dev), c_layer.to(dev)
    if args.lengths:
        lengths = np.asarray([int(v) for v in args.lengths.split(",")], dtype=np.int64)
        puzzle_points = np.asarray([lengths.sum()], dtype=np.int64)
    else:
        lengths = np.full(args.puzzles * args.pieces, args.points, dtype=np.int64)
        puzzle_points = np.full(args.puzzles, args.pieces * args.points, dtype=np.int64)
    if lengths.min() < 16:
        ap.error("the eager baseline is written for pieces of at least 16 points")
    N = int(lengths.sum())
    rng = np.random.default_rng(7)
    centre = np.repeat(rng.normal(0, 0.5, (len(lengths), 3)), lengths, 0)
    pts = (centre + 0.2 * rng.normal(size=(N, 3))).astype(np.float32)
    feats = np.sin(pts.astype(np.float64) @ rng.normal(0, 3.0, (3, 128)) + rng.uniform(0, 6.28, 128)) + 0.3 * rng.normal(size=(N, 128))
    feats[:, :3] *= 4.0
    p, x = torch.from_numpy(pts).to(dev), torch.from_numpy(feats.astype(np.float32)).to(dev)
    e_self, e_cross = EagerSelf(s_layer), EagerCross(c_layer)

    def spans(ev, names, prefix):
        return {f"{prefix}_{n}": ev[i][1].elapsed_time(ev[i + 1][1]) for i, n in enumerate(names)}

    def time_hip():
        s_layer.stage_events, c_layer.stage_events = [], []
        mid = s_layer(p, x, lengths)
        y = c_layer(mid, puzzle_points)
        torch.cuda.synchronize()
        a, b = s_layer.stage_events, c_layer.stage_events
        s_layer.stage_events = c_layer.stage_events = None
        return (mid, y), {**spans(a, SELF_STAGES, "self"), **spans(b, CROSS_STAGES, "cross")}

    def time_eager():
        ev = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((name, e))

        with torch.no_grad():
            mark("begin")
            mid = e_self(p, x, lengths, mark)
            n_self = len(ev)
            mark("begin")
            y = e_cross(mid, puzzle_points, mark)
        torch.cuda.synchronize()
        return (mid, y), {**spans(ev[:n_self], SELF_STAGES, "self"), **spans(ev[n_self:], CROSS_STAGES, "cross")}

    keys = [f"self_{n}" for n in SELF_STAGES] + [f"cross_{n}" for n in CROSS_STAGES]
    if args.skip_eager:
        time_eager = lambda: (None, {k: float("nan") for k in keys})
    for _ in range(args.warmup):
        out_hip, _ = time_hip()
        out_eager, _ = time_eager()
    agree = None if args.skip_eager else [float((a - b).abs().max() / b.abs().max()) for a, b in zip(out_hip, out_eager)]
    hip, eag = [], []
    for _ in range(args.repeats):          # alternating: both see the same clocks and the same neighbours on the machine
        hip.append(time_hip()[1])
        eag.append(time_eager()[1])
    med = lambda runs, k: statistics.median(r[k] for r in runs)
    tot = lambda runs: statistics.median(sum(r.values()) for r in runs)
    line = {"bench": "matching_descriptor", "device": torch.cuda.get_device_name(0), "piece_lengths": sorted(set(lengths.tolist())),
            "pieces": len(lengths), "puzzles": len(puzzle_points), "points": N, "gemm_mode": args.mode, "repeats": args.repeats,
            "hip_ms": {**{k: round(med(hip, k), 4) for k in keys}, "total": round(tot(hip), 4)},
            "hip_total_ms_runs": [round(sum(r.values()), 3) for r in hip]}
    if not args.skip_eager:
        line.update({"eager_ms": {**{k: round(med(eag, k), 4) for k in keys}, "total": round(tot(eag), 4)},
                     "eager_total_ms_runs": [round(sum(r.values()), 3) for r in eag], "speedup_total": round(tot(eag) / tot(hip), 2),
                     "eager_attention": "F.scaled_dot_product_attention per group of equally long puzzles",
                     "rel_diff_self_cross": agree})
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
