"""Measure the stretch from the device assignment's `col` to the ready `prepared` dicts of a batch on one GPU; print one JSON line.

    python tools/matching_edges_bench.py [--puzzles 16] [--reps 20] [--out FILE] [--profile]

Input: tools/matching_bench.py's batch (`--puzzles` puzzles of 8 pieces x 625 points, 178 symmetric matches between consecutive
pieces, N' = 2,492 critical points per puzzle) through MatchingHead.forward(solver="device", dense_perm=False) once; its perm_mat,
n_critical_pcs and critical_pcs_idx stay on the device, as a caller of the head holds them.  Two routes alternate in one process
(wall clock around work that ends in a device synchronise; median of `--reps` after one warm-up pair):

* host: per puzzle the download of col, pfpp_hip.matching.match_edges, AutoAgglomerative.prepare_matching (which downloads
  critical_pcs_idx and uploads the index arrays): what a caller does without pfpp_hip.matching_edges;
* device: pfpp_hip.matching_edges.match_edges_batch (one launch and one small read-back for the batch) and DeviceMatches.prepared
  per puzzle.

Also reported: the launch alone by device events, match_edges alone per puzzle on the host, and whether the two routes' dicts are
equal.  --profile runs only the device route (for rocprofv3 --kernel-trace --stats)."""
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


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_cases", ROOT / "tests" / "matching_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--profile", action="store_true", help="only the device route (kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_edges_bench: no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    from pfpp_hip.matching import MatchingHead, make_layout, match_edges
    from pfpp_hip.matching_edges import match_edges_batch, match_edges_launch
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative

    cases = load_cases()
    head = MatchingHead()
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}, strict=True)
    head.to(dev)
    sym = [(p, p + 1, MATCHES) for p in range(PIECES - 1)]
    pzs = [cases.build_puzzle([PER_PIECE] * PIECES, sym, [], 100 + k) for k in range(args.puzzles)]
    feats = torch.from_numpy(np.stack([p["part_feats"] for p in pzs])).to(dev)
    n_pcs = np.stack([p["n_pcs"] for p in pzs])
    valids = np.stack([p["part_valids"] for p in pzs])
    n_valid = valids.sum(1).astype(np.int64)
    B = args.puzzles
    out = head(feats, n_pcs, valids, dense_perm=False, solver="device")
    layout = make_layout(n_pcs, dev)
    n_pcs_dev = torch.from_numpy(n_pcs).to(dev)

    def host_route():
        nc = out.n_critical_pcs.cpu().numpy()
        res = []
        for b in range(B):
            edges, corr = match_edges(out.perm_mat[b], nc[b], int(n_valid[b]))                  # downloads col
            res.append(AutoAgglomerative.prepare_matching({"n_pcs": n_pcs_dev[b:b + 1], "critical_pcs_idx": out.critical_pcs_idx[b][None],
                                                           "edges": torch.from_numpy(edges[None]), "correspondences": corr}, dev))
        return res

    def device_route():
        dm = match_edges_batch(out.perm_mat, out.n_critical_pcs, n_valid, layout, out.critical_pcs_idx)
        return [dm.prepared(b) for b in range(B)], dm

    if args.profile:
        for _ in range(1 + args.reps):
            device_route()
        torch.cuda.synchronize()
        return 0
    walls = {"host": [], "device": []}
    last = {}
    for route in ("host", "device") * (args.reps + 1):                  # the first pair is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last[route] = host_route() if route == "host" else device_route()
        torch.cuda.synchronize()
        walls[route].append((time.perf_counter() - t0) * 1e3)
    prepared, dm = last["device"]
    equal = all(set(h) == set(d) and all(torch.equal(h[k], d[k]) if torch.is_tensor(h[k]) else h[k] == d[k] for k in h)
                for h, d in zip(last["host"], prepared))
    # the launch alone, by device events, into tensors allocated beforehand
    col = torch.cat(list(out.perm_mat))
    sizes = [int(c.numel()) for c in out.perm_mat]
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    R, T = int(row_off[-1]), dm.T
    crit = torch.cat(list(out.critical_pcs_idx))
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    bufs = dict(counts=i32(B, dm.P, dm.P), edge_off=i32(B, T + 1), kept=i32(B, T), corr=i32(R, 2), idx_a=i32(R), idx_b=i32(R), status=i32(B))
    ro, nv = torch.from_numpy(row_off).to(dev), torch.from_numpy(n_valid).to(dev)
    kernel_ms = []
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        match_edges_launch(col, ro, out.n_critical_pcs, nv, layout.piece_off, crit, B=B, P=dm.P, max_rows=max(sizes), total_rows=R,
                           total_points=crit.numel(), **bufs)
        e1.record()
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
    cols, nc = [c.cpu().numpy() for c in out.perm_mat], out.n_critical_pcs.cpu().numpy()
    rule_ms = []
    for b in range(B):
        t0 = time.perf_counter()
        match_edges(cols[b], nc[b], int(n_valid[b]))
        rule_ms.append((time.perf_counter() - t0) * 1e3)
    med = lambda v: statistics.median(v[1:])
    line = {"bench": "matching_edges", "puzzles": B, "points": PIECES * PER_PIECE, "reps": args.reps, "device_name": torch.cuda.get_device_name(dev),
            "n": sizes, "edges_per_puzzle": [int(dm.kept_host[b].sum()) for b in range(B)],
            "correspondences_per_puzzle": [dm.n_correspondences(b) for b in range(B)], "routes_equal": bool(equal),
            "host_route_ms_per_batch": med(walls["host"]), "host_route_ms_per_batch_min": min(walls["host"][1:]),
            "device_route_ms_per_batch": med(walls["device"]), "device_route_ms_per_batch_min": min(walls["device"][1:]),
            "launch_ms_per_batch_by_events": med(kernel_ms), "host_match_edges_alone_ms_per_puzzle": statistics.median(rule_ms)}
    text = json.dumps(line)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
