"""Measure a training batch of the matcher's dataset from the resident mesh store (pfpp_hip.matching_dataset.sample_batch) on one GPU;
print one JSON line.

    python tools/matching_dataset_bench.py [--puzzles 16] [--points 5000] [--min-part-point 30] [--reps 7] [--profile]
                                           [--kernel-stats CSV] [--out profiles/matching_dataset_bench_line.json]

Workload: `tools/make_synthetic_meshes.py --bench 16` (16 puzzles of 20 parts, 1.5k-5k faces each) parsed once into a MeshStore;
a batch is all 16 puzzles at 5,000 points per puzzle.  One call = piece counts + ragged sampling + pose, with the selection's
upload and the output allocations inside, timed by device events around the call, median of 7 after a warm-up.  The per-kernel
times come from a kernel trace, a run of its own: this tool with --profile under `rocprofv3 --kernel-trace --stats`, the trace
summarised by tools/rocprof_summary.py, the CSV passed as --kernel-stats; its per-kernel averages are folded into the line.
Also reported: the store's device bytes, the host OBJ parse per puzzle (pfpp_hip.meshes.read_obj, one process), and the CPU
restatement of the reference's item (all_piece_matching_dataset.py __getitem__ after the loads: np.sum areas, counts, trimesh's
sample_surface per part, mean, a random rotation through scipy when it is installed, shuffle, float32) with the meshes already in
memory, on this machine's CPU."""
from __future__ import annotations

import argparse
import csv
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))
sys.path.insert(0, str(ROOT / "tests"))

KERNELS = ("piece_counts_kernel", "ragged_sample_kernel", "pose_kernel")


def cpu_reference_item(parts, num_points, min_part_point, rng, cases):
    """the reference's __getitem__ after trimesh.load, restated with numpy (the sampling as trimesh 4.0.2 does it)"""
    try:
        from scipy.spatial.transform import Rotation
    except ImportError:          # the matrix of a normalised Gaussian quaternion: the same distribution
        Rotation = None
    tris = [v[f] for v, f in parts]
    face_area = [np.sqrt((np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) ** 2).sum(axis=1)) / 2.0 for t in tris]
    areas = np.array([a.sum() for a in face_area])
    nps = cases.piece_counts(areas, num_points, min_part_point)
    pcs, gts, quats, trans = [], [], [], []
    for (v, f), fa, n in zip(parts, face_area, nps):
        cdf = np.cumsum(fa)
        face = np.searchsorted(cdf, rng.random(n) * cdf[-1])
        o = v[f[:, 0]]
        vec = v[f[:, 1:]].copy() - np.tile(o, (1, 2)).reshape((-1, 2, 3))
        o, vec = o[face], vec[face]
        lengths = rng.random((len(vec), 2, 1))
        lengths[lengths.sum(axis=1).reshape(-1) > 1.0] -= 1.0
        pc = (vec * np.abs(lengths)).sum(axis=1) + o
        c = np.mean(pc, axis=0)
        if Rotation is not None:
            rot = Rotation.random().as_matrix()
            quat = Rotation.from_matrix(rot.T).as_quat()[[3, 0, 1, 2]]
        else:
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            rot, quat = cases.quat_matrix(q), q * np.array([1.0, -1.0, -1.0, -1.0])
        rotated = (rot @ (pc - c[None]).T).T
        order = np.arange(n)
        random.shuffle(order)
        pcs.append(rotated[order])
        gts.append(pc[order])
        quats.append(quat)
        trans.append(c)
    return np.concatenate(pcs).astype(np.float32), np.concatenate(gts).astype(np.float32), np.stack(quats), np.stack(trans)


def pose_alone_us(store, sel, out, num_points, reps, max_parts=20):
    """device events around pfpp_mdata_pose alone, on the workspace and offsets of a finished batch: median of `reps` in microseconds"""
    import torch

    from pfpp_hip import _lib
    from pfpp_hip.meshes import _p, _stream

    dev, B = store.device, len(sel)
    sel_d = torch.tensor(sel, dtype=torch.int64, device=dev)
    pcs = torch.empty((B, num_points, 3), dtype=torch.float32, device=dev)
    quat = torch.empty((B, max_parts, 4), dtype=torch.float32, device=dev)
    trans = torch.empty((B, max_parts, 3), dtype=torch.float32, device=dev)
    lib, times = _lib.load(), []
    for rep in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        _lib.check(lib.pfpp_mdata_pose(_p(out["points"]), _p(out["piece_off"]), _p(store.batch.data_id), _p(sel_d), B, len(store), num_points,
                                       max_parts, None, None, 1, 0, _p(pcs), _p(quat), _p(trans), None, _stream(dev)), "pfpp_mdata_pose")
        ev[1].record()
        torch.cuda.synchronize()
        if rep:
            times.append(ev[0].elapsed_time(ev[1]) * 1e3)
    assert torch.equal(pcs, out["part_pcs"])
    return statistics.median(times)


def kernel_stats(path):
    """tools/rocprof_summary.py's CSV -> {kernel: (calls, average us)} for this unit's kernels"""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row["kernel"]:
                    out[k] = (int(row["calls"]), float(row["avg_us"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--min-part-point", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile", action="store_true", help="only the GPU calls (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default=None, help="CSV of tools/rocprof_summary.py from a --profile run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import matching_dataset_cases as cases
    from pfpp_hip import meshes as Mh
    from pfpp_hip.matching_dataset import MeshStore, sample_batch, split_word

    assert torch.cuda.is_available(), "matching_dataset_bench measures the GPU path: no GPU here"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_meshes.py"), tmp, "--bench", str(a.puzzles)], check=True)
        rels = list(json.load(open(os.path.join(tmp, "truth.json"))))
        t0 = time.perf_counter()
        puzzles = [[Mh.read_obj(os.path.join(tmp, r, f)) for f in sorted(os.listdir(os.path.join(tmp, r)))] for r in rels]
        parse_ms = (time.perf_counter() - t0) * 1e3 / a.puzzles
    store = MeshStore.from_meshes(puzzles, list(range(a.puzzles)), rels, dev)
    sel = list(range(a.puzzles))

    def timed(epoch):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        ev[0].record()
        out = sample_batch(store, sel, a.points, a.min_part_point, seed=1, split=split_word("train", epoch), check=False)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), (time.perf_counter() - w0) * 1e3, out

    timed(0)
    runs = [timed(1 + r) for r in range(a.reps)]
    Mh.check_status(runs[-1][2]["status"])
    if a.profile:
        return
    n_pcs = runs[-1][2]["n_pcs"].cpu().numpy()
    line = {"bench": "matching_dataset_batch", "puzzles": a.puzzles, "parts_per_puzzle": 20, "points": a.points,
            "min_part_point": a.min_part_point, "faces_per_part_mean": float(np.mean([len(f) for pz in puzzles for _, f in pz])),
            "hip_call_ms": statistics.median(r[0] for r in runs), "hip_call_ms_min_max": [min(r[0] for r in runs), max(r[0] for r in runs)],
            "hip_wall_ms": statistics.median(r[1] for r in runs), "store_device_bytes": store.device_bytes,
            "largest_piece_rows": int(n_pcs.max()), "host_parse_ms_per_puzzle": parse_ms}
    line["hip_call_ms_per_puzzle"] = line["hip_call_ms"] / a.puzzles
    if a.kernel_stats:
        for k, (calls, us) in kernel_stats(a.kernel_stats).items():
            line[f"{k}_us"] = us
            line[f"{k}_calls"] = calls
        if all(f"{k}_us" in line for k in KERNELS):
            line["kernels_us_per_batch"] = sum(line[f"{k}_us"] for k in KERNELS)
    # the pose kernel alone (its centroid is a serial chain of one fp64 addition per row): the 20-part batch, and the same meshes as
    # 2-part puzzles, whose largest piece holds most of a puzzle's rows
    two = MeshStore.from_meshes([pz[:2] for pz in puzzles], list(range(a.puzzles)), rels, dev)
    for name, st in (("pose_alone_20_parts", store), ("pose_alone_2_parts", two)):
        out = sample_batch(st, sel, a.points, a.min_part_point, seed=1, split=0)
        us = pose_alone_us(st, sel, out, a.points, a.reps)
        line[name] = {"largest_piece_rows": int(out["n_pcs"].max()), "us": us, "ns_per_row_of_largest_piece": 1e3 * us / int(out["n_pcs"].max())}
    rng = np.random.default_rng(0)
    n_cpu = min(4, a.puzzles)
    t0 = time.perf_counter()
    for pz in puzzles[:n_cpu]:
        cpu_reference_item(pz, a.points, a.min_part_point, rng, cases)
    line["cpu_reference_ms_per_puzzle"] = (time.perf_counter() - t0) * 1e3 / n_cpu
    line["cpu_reference"] = "numpy restatement of the reference's item on this machine's CPU, meshes already in memory (not the code under test)"
    line["ratio_per_puzzle"] = line["cpu_reference_ms_per_puzzle"] / line["hip_call_ms_per_puzzle"]
    text = json.dumps(line)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
