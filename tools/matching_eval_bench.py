"""Measure the pairwise RANSAC of the matcher's evaluation (pfpp_hip.matching_eval.ransac_pairs) on one GPU; print one JSON line.

    python tools/matching_eval_bench.py [--puzzles 2] [--n-hyp 50000] [--host-pairs 4] [--profile] [--out profiles/matching_eval_bench_line.json]

Workload: the other matcher benches' shape: `--puzzles` puzzles of 8 pieces x 625 = 5,000 points.  The assignment is built from the
ground truth, so every one of the 28 piece pairs of a puzzle has matches: 89 matched critical points per pair, a fifth of them wrong
(the target displaced by sigma = 0.3), every piece recentred and turned by a seeded rotation.  One call scores n_hyp hypotheses for all
pairs of the batch; timed by device events around the call, median of 7 after a warm-up, with the tables' upload inside.

The comparison is NOT the code under test and NOT open3d (which the reference calls and which is not available here): it is the
float64 numpy restatement of the same procedure (tests/matching_pose_cases.ransac_reference, vectorised over the hypotheses) on this
machine's CPU at the same n_hyp, timed once over the first `--host-pairs` pairs and reported per pair; its winners must equal the
GPU's.  --profile runs only the GPU calls (for rocprofv3 --kernel-trace --stats)."""
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

PIECES, PER_PIECE, MATCHES, WRONG = 8, 625, 89, 0.2


def load_cases(stem: str):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_batch(puzzles: int, cases):
    """-> pts float32 [puzzles 5000, 3], pairs [(source row, target row)], corr [int64 [MATCHES, 2]]"""
    pts, pairs, corr = [], [], []
    for b in range(puzzles):
        rng = np.random.default_rng([97, b])
        world = [rng.uniform(-0.5, 0.5, (PER_PIECE, 3)) for _ in range(PIECES)]
        for p in range(PIECES):                                       # pieces p < q share MATCHES exact points, at rows of their own
            for q in range(p + 1, PIECES):
                shared = rng.uniform(-0.5, 0.5, (MATCHES, 3))
                rp, rq = np.arange(MATCHES) + (q - 1) * MATCHES, np.arange(MATCHES) + p * MATCHES
                world[p][rp], world[q][rq] = shared, shared
                wrong = rng.permutation(MATCHES)[:int(WRONG * MATCHES)]
                world[q][rq[wrong]] += 0.3 * rng.normal(size=(wrong.size, 3))
                pairs.append(((b * PIECES + p) * PER_PIECE, (b * PIECES + q) * PER_PIECE))
                corr.append(np.stack([rp, rq], 1).astype(np.int64))
        for p in range(PIECES):
            x = world[p]
            pts.append(((x - x.mean(0)) @ cases.rotation(rng).T).astype(np.float32))
    return np.concatenate(pts), pairs, corr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=2)
    ap.add_argument("--n-hyp", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-pairs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pfpp_hip.matching_eval import ransac_pairs

    cases = load_cases("matching_pose_cases")
    pts, pairs, corr = make_batch(args.puzzles, cases)
    dev = torch.device("cuda:0")
    pts_d = torch.from_numpy(pts).to(dev)

    def timed(refine: bool):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = ransac_pairs(pts_d, pairs, corr, n_hyp=args.n_hyp, seed=args.seed, refine=refine)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out

    timed(False)
    times = {False: [], True: []}
    for _ in range(args.reps):
        for refine in (False, True):
            ms, out = timed(refine)
            times[refine].append(ms)
            if not refine:
                got = {k: v.cpu().numpy() for k, v in out.items()}
    if args.profile:
        return
    E, M = len(pairs), MATCHES
    line = {"bench": "matching_eval_ransac", "puzzles": args.puzzles, "points": PIECES * PER_PIECE, "pairs": E, "matches_per_pair": M,
            "n_hyp": args.n_hyp, "poses": E * args.n_hyp, "hip_call_ms": statistics.median(times[False]),
            "hip_call_ms_refine": statistics.median(times[True]), "hip_call_ms_min_max": [min(times[False]), max(times[False])],
            "inliers_found_mean": float(got["count"].mean()), "inliers_planted": M - int(WRONG * M)}
    line["hip_gpose_per_s"] = line["poses"] / line["hip_call_ms"] / 1e6
    n = min(args.host_pairs, E)
    if n:
        t0 = time.perf_counter()
        refs = [cases.ransac_reference(pts, pairs[e], corr[e], args.n_hyp, e=e, seed=args.seed) for e in range(n)]
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(r["best_h"] == got["best_h"][e] and r["count"] == got["count"][e] for e, r in enumerate(refs))
        line.update(host="float64 numpy restatement of the same procedure on the CPU (not the code under test, not open3d)", host_pairs_timed=n,
                    host_ms_per_pair=host_ms / n, hip_ms_per_pair=line["hip_call_ms"] / E, winners_equal_host=bool(same),
                    ratio_per_pair=(host_ms / n) / (line["hip_call_ms"] / E))
    text = json.dumps(line)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
