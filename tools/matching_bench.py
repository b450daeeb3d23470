"""Measure the matcher back end (pfpp_hip.matching.MatchingHead) on one GPU and print one JSON line.

    python tools/matching_bench.py [--puzzles 16] [--reps 3] [--skip-eager] [--profile]

Workload: `--puzzles` puzzles of 8 pieces x 625 = 5,000 points whose descriptors are built like the tests' (tests/matching_cases.py):
178 symmetric matches between consecutive pieces, so N' = 2,492 critical points per puzzle.  Reported per puzzle (milliseconds, median
of `--reps` after one warm-up): the HIP stages by device events (classify + compact, gather + 128 -> 512 + normalise + primal x A, the
affinity GEMM, Sinkhorn), the Sinkhorn kernels' bytes/s against the 20 N'^2 4 B they must read, the device-to-host copy of ds_mat, the
host assignment, and the wall time of the whole forward with and without overlapping the assignment with the next puzzle's GPU work
(alternating, medians of `--reps` as well).
The comparison is the same steps in PyTorch eager fp32 on the same GPU, restated here the way the reference runs them: per-piece
nonzero loops for the critical points, the two N' x N' mask tensors built in Python loops, s * mask + neg_mask, and the full-matrix
Sinkhorn that rewrites log_s 20 times.  --profile runs only the HIP forward (for rocprofv3 --kernel-trace --stats).

    python tools/matching_bench.py --assignment device [--out FILE]

measures the device assignment solver (pfpp_hip.matching_assign) against the host path instead: the two forwards alternate in one
process on the same batch, and on a second, harder one in which 30 % of the critical points carry the descriptor of an unrelated
point.  Per input: wall per batch and per puzzle of both paths (median of `--reps` after one warm-up each), the solver's launch by
device events for the batch and for its puzzles one at a time, the host solver one puzzle at a time, steps and augmentations per
puzzle, and microseconds per search step (a single puzzle's launch over its steps).  With --profile only the device-path forward
runs."""
from __future__ import annotations

import argparse
import importlib.util
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))

PIECES, PER_PIECE, MATCHES = 8, 625, 178
TAU, ITERS = 0.05, 20


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_cases", ROOT / "tests" / "matching_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, dev):
    """(result, milliseconds by device events)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def hip_stages(head, feats, n_pcs, dev):
    from scipy.optimize import linear_sum_assignment

    from pfpp_hip.matching import make_layout, sinkhorn

    B = n_pcs.shape[0]
    layout = make_layout(n_pcs, dev)
    flat = feats.reshape(-1, 128)
    (logits, labels, crit, n_crit), t_cls = timed(lambda: head.classify(flat, layout), dev)
    crit_off = torch.zeros(n_crit.numel() + 1, dtype=torch.int64, device=dev)
    crit_off[1:] = torch.cumsum(n_crit, 0)
    rows = np.concatenate([[0], np.cumsum(n_crit.cpu().numpy().reshape(B, -1).sum(1))])
    (f, row_piece, pa), t_feat = timed(lambda: (*head.affinity_features(flat, layout, crit, crit_off, int(rows[-1])), None), dev)
    pa, t_pa = timed(lambda: head.primal_times_a(f), dev)
    t_aff = t_sk = t_copy = t_lsa = 0.0
    for b in range(B):
        r0, r1 = int(rows[b]), int(rows[b + 1])
        s, t = timed(lambda: head.affinity(f, r0, r1, pa), dev)
        t_aff += t
        ds, t = timed(lambda: sinkhorn(s, row_piece[r0:r1], tau=TAU, max_iter=ITERS, check_pieces=False), dev)
        t_sk += t
        buf = torch.empty(ds.shape, dtype=torch.float32, pin_memory=True)
        _, t = timed(lambda: buf.copy_(ds, non_blocking=True), dev)
        t_copy += t
        t0 = time.perf_counter()
        linear_sum_assignment(-buf.numpy())
        t_lsa += (time.perf_counter() - t0) * 1e3
    n_prime = [int(rows[b + 1] - rows[b]) for b in range(B)]
    return {"classify_compact": t_cls / B, "gather_features": (t_feat + t_pa) / B, "affinity_gemm": t_aff / B, "sinkhorn": t_sk / B,
            "d2h_copy": t_copy / B, "host_assignment": t_lsa / B}, n_prime


def eager_stages(sd, feats, n_pcs, n_valid, dev):
    """the reference's test-time forward behind part_feats in PyTorch eager fp32, stage by stage"""
    from scipy.optimize import linear_sum_assignment

    F = torch.nn.functional
    B, N, _ = feats.shape
    P = n_pcs.shape[1]
    npc = torch.from_numpy(n_pcs).to(dev)

    def bn_relu(name, x):
        return torch.relu(F.batch_norm(x, sd[f"{name}.0.running_mean"], sd[f"{name}.0.running_var"], sd[f"{name}.0.weight"], sd[f"{name}.0.bias"],
                                       False, 0.0, 1e-5))

    def classify():
        x = feats.transpose(1, 2)
        logits = F.conv1d(bn_relu("pc_classifier", x), sd["pc_classifier.2.weight"], sd["pc_classifier.2.bias"]).transpose(1, 2)
        pred = (torch.sigmoid(logits) > 0.5).to(torch.int64).reshape(B, N)
        cum = torch.cumsum(npc, 1)
        n_crit = torch.zeros_like(npc)
        crit = torch.zeros_like(pred)
        for b in range(B):
            for p in range(P):
                st = 0 if p == 0 else cum[b, p - 1]
                idx = pred[b, st:cum[b, p]].nonzero().reshape(-1)
                n_crit[b, p] = idx.shape[0]
                crit[b, st:st + idx.shape[0]] = idx
        return pred, crit, n_crit

    (pred, crit, n_crit), t_cls = timed(classify, dev)
    n_sum = n_crit.sum(-1)
    n_max = int(n_sum.max())

    def features():
        cf = torch.zeros(B, n_max, 128, device=dev)
        for b in range(B):
            cf[b, :n_sum[b]] = feats[b, pred[b] == 1]
        af = F.conv1d(bn_relu("affinity_extractor", cf.permute(0, 2, 1)), sd["affinity_extractor.2.weight"], sd["affinity_extractor.2.bias"]).permute(0, 2, 1)
        return torch.cat([F.normalize(af[:, :, :256], p=2, dim=-1), F.normalize(af[:, :, 256:], p=2, dim=-1)], -1)

    af, t_feat = timed(features, dev)
    s, t_aff = timed(lambda: torch.matmul(torch.matmul(af[:, :, :256], sd["affinity_layer.A"]), af[:, :, 256:].transpose(1, 2)), dev)

    def mask(pos, neg):
        cum = torch.cumsum(n_crit, -1)
        m = torch.ones(s.shape, device=dev) * neg
        for b in range(B):
            e = cum[b, n_valid[b] - 1]
            m[b, :e, :e] = pos
            for p in range(int(n_valid[b])):
                st = 0 if p == 0 else cum[b, p - 1]
                m[b, st:cum[b, p], st:cum[b, p]] = neg
        return m

    def sinkhorn():
        s_ = s * mask(1, 0) + mask(0, -1e6)
        out = torch.full_like(s_, -float("inf"))
        for b in range(B):
            n = int(n_sum[b])
            log_s = s_[b, :n, :n] / TAU
            for i in range(ITERS):
                log_s = log_s - torch.logsumexp(log_s, 1 if i % 2 == 0 else 0, keepdim=True)
            out[b, :n, :n] = log_s
        return torch.exp(out)

    ds, t_sk = timed(sinkhorn, dev)
    (host, ), t_copy = timed(lambda: (ds.cpu(), ), dev)
    t0 = time.perf_counter()
    for b in range(B):
        n = int(n_sum[b])
        linear_sum_assignment(-host[b, :n, :n].numpy())
    t_lsa = (time.perf_counter() - t0) * 1e3
    return {"classify_compact": t_cls / B, "gather_features": t_feat / B, "affinity_gemm": t_aff / B, "sinkhorn_with_masks": t_sk / B,
            "d2h_copy": t_copy / B, "host_assignment": t_lsa / B}, ds


def weaken(cases, pzs, share: float, seed: int):
    """the harder input: a share of every puzzle's critical points takes the descriptor of a critical point of an unrelated puzzle"""
    rng = np.random.default_rng(seed)
    sym = [(p, p + 1, MATCHES) for p in range(PIECES - 1)]
    out = []
    for k, pz in enumerate(pzs):
        other = cases.build_puzzle([PER_PIECE] * PIECES, sym, [], 5000 + k)
        mine, theirs = np.nonzero(pz["critical"])[0], np.nonzero(other["critical"])[0]
        pick = mine[rng.random(mine.size) < share]
        x = pz["part_feats"].copy()
        x[pick] = other["part_feats"][rng.choice(theirs, pick.size, replace=False)]
        out.append(x)
    return out


def assignment_bench(head, feats, n_pcs, valids, reps: int, dev) -> dict:
    """host and device solver on one batch, alternating"""
    from scipy.optimize import linear_sum_assignment

    from pfpp_hip.matching_assign import assign_batch

    B = n_pcs.shape[0]
    walls = {"host": [], "device": []}
    outs = {}
    for solver in ("host", "device") * (reps + 1):             # the first pair is the warm-up
        t0 = time.perf_counter()
        outs[solver] = head(feats, n_pcs, valids, dense_perm=False, solver=solver)
        torch.cuda.synchronize()
        walls[solver].append((time.perf_counter() - t0) * 1e3)
    ds = outs["device"].ds_mat
    equal_rows = [int((outs["host"].perm_mat[b] == outs["device"].perm_mat[b]).sum()) for b in range(B)]
    weight = lambda o: [float(ds[b].double()[torch.arange(ds[b].shape[0], device=dev), o.perm_mat[b]].sum()) for b in range(B)]
    assign_batch(ds)
    batch_ms = statistics.median(timed(lambda: assign_batch(ds), dev)[1] for _ in range(reps))
    res = assign_batch(ds)
    steps, augs = res.steps.tolist(), res.augmentations.tolist()
    single_ms, host_ms = [], []
    for b in range(B):
        assign_batch([ds[b]])
        single_ms.append(statistics.median(timed(lambda: assign_batch([ds[b]]), dev)[1] for _ in range(reps)))
        a = ds[b].cpu().numpy()
        t0 = time.perf_counter()
        linear_sum_assignment(-a)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    med = lambda v: statistics.median(v[1:])
    return {"n": [int(d.shape[0]) for d in ds], "rows_with_the_hosts_column": equal_rows, "weight_host": weight(outs["host"]),
            "weight_device": weight(outs["device"]), "fallback_puzzles": outs["device"].timings["fallback_puzzles"],
            "host": {"wall_ms_per_batch": med(walls["host"]), "wall_ms_per_puzzle": med(walls["host"]) / B,
                     "solver_ms_per_puzzle_alone": statistics.median(host_ms), "solver_ms_per_puzzle_alone_max": max(host_ms)},
            "device": {"wall_ms_per_batch": med(walls["device"]), "wall_ms_per_puzzle": med(walls["device"]) / B,
                       "solver_ms_per_batch_by_events": batch_ms, "solver_ms_per_puzzle_alone": statistics.median(single_ms),
                       "solver_ms_per_puzzle_alone_max": max(single_ms)},
            "steps_per_puzzle": steps, "augmentations_per_puzzle": augs,
            "us_per_step": statistics.median(1e3 * m / s for m, s in zip(single_ms, steps) if s > 0) if any(steps) else None,
            "us_per_step_in_the_batch": 1e3 * batch_ms / max(steps) if any(steps) else None}


def median_of(runs):
    return {k: statistics.median(r[k] for r in runs) for k in runs[0]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gemm", choices=("f32", "f16x3"), default="f32")
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--profile", action="store_true", help="only the HIP forward, without the assignment (kernel trace)")
    ap.add_argument("--assignment", choices=("host", "device"), default="host", help="device: measure the device solver against the host path")
    ap.add_argument("--out", help="--assignment device: also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_bench: no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    from pfpp_hip.matching import MatchingHead

    cases = load_cases()
    sd_np = cases.head_state_dict()
    head = MatchingHead(gemm_mode=args.gemm)
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    head.to(dev)
    sym = [(p, p + 1, MATCHES) for p in range(PIECES - 1)]
    pzs = [cases.build_puzzle([PER_PIECE] * PIECES, sym, [], 100 + k) for k in range(args.puzzles)]
    feats = torch.from_numpy(np.stack([p["part_feats"] for p in pzs])).to(dev)
    n_pcs = np.stack([p["n_pcs"] for p in pzs])
    valids = np.stack([p["part_valids"] for p in pzs])
    B = args.puzzles
    if args.assignment == "device":
        hard = torch.from_numpy(np.stack(weaken(cases, pzs, 0.3, 0))).to(dev)
        if args.profile:
            for x in (feats, hard) * (1 + args.reps):
                head(x, n_pcs, valids, dense_perm=False, solver="device")
            torch.cuda.synchronize()
            return 0
        line = {"bench": "matching_assign", "puzzles": B, "points": PIECES * PER_PIECE, "gemm": args.gemm, "reps": args.reps,
                "device_name": torch.cuda.get_device_name(dev), "easy": assignment_bench(head, feats, n_pcs, valids, args.reps, dev),
                "weak_30": assignment_bench(head, hard, n_pcs, valids, args.reps, dev)}
        text = json.dumps(line)
        print(text)
        if args.out:
            Path(args.out).write_text(text + "\n")
        return 0
    if args.profile:
        for _ in range(1 + args.reps):
            head(feats, n_pcs, valids, assign=False)
        torch.cuda.synchronize()
        return 0
    hip_stages(head, feats, n_pcs, dev)                      # warm-up of every shape
    runs = [hip_stages(head, feats, n_pcs, dev) for _ in range(args.reps)]
    hip, n_prime = median_of([r[0] for r in runs]), runs[0][1]
    walls, host_overlapped = {True: [], False: []}, []
    for overlap in (True, False) * args.reps:                  # alternating; the same statistic as the stages: the median of --reps
        t0 = time.perf_counter()
        out = head(feats, n_pcs, valids, dense_perm=False, overlap=overlap)
        torch.cuda.synchronize()
        walls[overlap].append((time.perf_counter() - t0) * 1e3 / B)
        if overlap:
            host_overlapped.append(out.timings["host_assignment_s"] * 1e3 / B)
    wall_overlap, wall_serial = statistics.median(walls[True]), statistics.median(walls[False])
    npm = float(np.mean(n_prime))
    line = {"bench": "matching_head", "puzzles": B, "points": PIECES * PER_PIECE, "n_critical_mean": npm, "n_critical_min": min(n_prime),
            "n_critical_max": max(n_prime), "gemm": args.gemm, "hip_ms_per_puzzle": hip,
            "hip_gpu_stages_ms_per_puzzle": hip["classify_compact"] + hip["gather_features"] + hip["affinity_gemm"] + hip["sinkhorn"],
            "sinkhorn_must_read_mb": ITERS * npm * npm * 4 / 1e6,
            "sinkhorn_read_gb_per_s": ITERS * npm * npm * 4 / 1e9 / (hip["sinkhorn"] / 1e3),
            "wall_overlap_ms_per_puzzle": wall_overlap, "wall_serial_ms_per_puzzle": wall_serial,
            "host_assignment_share_of_overlapped_wall": statistics.median(host_overlapped) / wall_overlap,
            "peak_device_mem_mb": torch.cuda.max_memory_allocated(dev) / 2 ** 20}
    if not args.skip_eager:
        sd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd_np.items()}
        n_valid = valids.sum(1).astype(np.int64)
        eager_stages(sd, feats, n_pcs, n_valid, dev)
        eruns = [eager_stages(sd, feats, n_pcs, n_valid, dev) for _ in range(args.reps)]
        eager = median_of([r[0] for r in eruns])
        ds_e = eruns[-1][1]
        dev_max = max(float((out.ds_mat[b] - ds_e[b, :n_prime[b], :n_prime[b]]).abs().max()) for b in range(B))
        line.update({"eager_ms_per_puzzle": eager, "ds_mat_max_abs_diff_vs_eager": dev_max,
                     "eager_gpu_stages_ms_per_puzzle": eager["classify_compact"] + eager["gather_features"] + eager["affinity_gemm"] + eager["sinkhorn_with_masks"],
                     "sinkhorn_speedup_vs_eager": eager["sinkhorn_with_masks"] / hip["sinkhorn"]})
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
