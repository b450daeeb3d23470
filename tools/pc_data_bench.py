"""pc_data generation at bench scale: prints one JSON line.

    python tools/pc_data_bench.py [--puzzles 16] [--batch 16] [--workers 6] [--points 1000] [--reps 5]

Writes `tools/make_synthetic_meshes.py --bench` puzzles (20 parts, 3-4k faces each) to a temporary tree and measures
  * the GPU path per puzzle: upload (pinned host buffers -> device), face cdf, sampling (+ scale / reference part) and contact graph,
    as kernel time (device events around each stage) and as wall time of the whole batch (host clock, synchronised);
  * the host OBJ parse per puzzle (pfpp_hip.meshes.read_obj);
  * the CPU restatement of the reference's per-item work: numpy sample_surface per part plus _check_connectivity's pairwise set
    test, as dataset.py:85-127 / 172-179 do it;
  * files per second through the entry point (python -m pfpp_hip.generate_pc_data) with N loader workers;
  * peak device memory of the GPU path."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))


def cpu_reference_item(parts, N, rng):
    """dataset.py:_get_pcs after the loads: pairwise rounded-vertex sets, then trimesh sample_surface per part (restated)"""
    P = len(parts)
    g = np.zeros((20, 20), dtype=bool)
    for i in range(P):
        for j in range(i + 1, P):
            a = set(map(tuple, np.round(parts[i][0], 5)))
            b = set(map(tuple, np.round(parts[j][0], 5)))
            if len(a.intersection(b)) > 0:
                g[i, j] = g[j, i] = True
    pcs = []
    for v, f in parts:
        t = v[f]
        cr = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        cdf = np.cumsum(np.sqrt((cr ** 2).sum(axis=1)) / 2.0)
        face = np.searchsorted(cdf, rng.random(N) * cdf[-1])
        o = v[f[:, 0]]
        vec = v[f[:, 1:]].copy() - np.tile(o, (1, 2)).reshape((-1, 2, 3))
        o, vec = o[face], vec[face]
        lengths = rng.random((len(vec), 2, 1))
        lengths[lengths.sum(axis=1).reshape(-1) > 1.0] -= 1.0
        pcs.append((vec * np.abs(lengths)).sum(axis=1) + o)
    return np.stack(pcs), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--workers", type=int, default=6)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    import torch

    from pfpp_hip import meshes as Mh

    assert torch.cuda.is_available(), "pc_data_bench measures the GPU path: no GPU here"
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)                      # initialise the device before its memory statistics are reset
    res = {"puzzles": a.puzzles, "batch": a.batch, "parts_per_puzzle": 20, "points": a.points}
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_meshes.py"), tmp, "--bench", str(a.puzzles)], check=True)
        rels = json.load(open(os.path.join(tmp, "truth.json")))
        folders = [os.path.join(tmp, r) for r in rels]
        t0 = time.perf_counter()
        puzzles = [[Mh.read_obj(os.path.join(d, f)) for f in sorted(os.listdir(d))] for d in folders]
        res["host_parse_ms_per_puzzle"] = (time.perf_counter() - t0) * 1e3 / a.puzzles
        res["faces_per_part_mean"] = float(np.mean([len(f) for pz in puzzles for _, f in pz]))
        res["verts_per_part_mean"] = float(np.mean([len(v) for pz in puzzles for v, _ in pz]))

        # CPU restatement of the reference's per-item work
        rng = np.random.default_rng(0)
        n_cpu = min(4, a.puzzles)
        t0 = time.perf_counter()
        for pz in puzzles[:n_cpu]:
            cpu_reference_item(pz, a.points, rng)
        res["cpu_reference_ms_per_puzzle"] = (time.perf_counter() - t0) * 1e3 / n_cpu

        # GPU path, batch of a.batch puzzles
        batch = puzzles[: a.batch]
        ids = list(range(len(batch)))
        torch.cuda.reset_peak_memory_stats(dev)
        stage = {"upload": [], "cdf": [], "sample": [], "graph": []}
        walls = []
        for rep in range(a.reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            ev[0].record()
            mb = Mh.pack(batch, ids, dev)
            ev[1].record()
            st = Mh.new_status(dev)
            _, cdf, total = Mh.face_cdf(mb, status=st)
            ev[2].record()
            pts, _, _, ref = Mh.sample_surface(mb, a.points, cdf, total, seed=1)
            ev[3].record()
            g = Mh.vertex_graph(mb, 20, status=st)
            ev[4].record()
            Mh.check_status(st)
            torch.cuda.synchronize()
            if rep:                                   # the first round warms every shape up
                walls.append(time.perf_counter() - w0)
                for k, name in enumerate(stage):
                    stage[name].append(ev[k].elapsed_time(ev[k + 1]))
        nb = len(batch)
        for name, v in stage.items():
            res[f"gpu_{name}_ms_per_puzzle"] = float(np.median(v)) / nb
        res["gpu_kernels_ms_per_puzzle"] = sum(res[f"gpu_{n}_ms_per_puzzle"] for n in ("cdf", "sample", "graph"))
        res["gpu_wall_ms_per_puzzle"] = float(np.median(walls)) * 1e3 / nb
        res["peak_device_mem_mb"] = torch.cuda.max_memory_allocated(dev) / 2 ** 20

        # the entry point, files per second
        cfgdir = os.path.join(tmp, "cfg")
        os.makedirs(cfgdir)
        with open(os.path.join(cfgdir, "global_config.yaml"), "w") as fh:
            fh.write("defaults:\n  - _self_\n  - data\n")
        with open(os.path.join(cfgdir, "data.yaml"), "w") as fh:
            fh.write(f"data:\n  batch_size: 1\n  val_batch_size: 1\n  num_workers: {a.workers}\n  data_fn: \"everyday.{{}}.txt\"\n"
                     f"  mesh_data_dir: {tmp}\n  rot_range: -1\n  overfit: -1\n  data_keys: ['part_ids']\n  num_pc_points: {a.points}\n"
                     "  min_num_part: 2\n  max_num_part: 20\n  shuffle_parts: False\n  category: all\n")
        env = dict(os.environ)
        env["PYTHONPATH"] = os.pathsep.join([str(ROOT), str(ROOT / "puzzlefusion-plusplus_amd"), env.get("PYTHONPATH", "")])
        r = subprocess.run([sys.executable, "-m", "pfpp_hip.generate_pc_data", "--config-dir", cfgdir,
                            f"+data.save_pc_data_path={os.path.join(tmp, 'out')}", f"data.batch_size={a.batch}"],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("train:")][0]
        res["entry_point_train_line"] = line
        res["entry_point_files_per_s"] = float(line.split("(")[1].split()[0])
        res["entry_point_workers"] = a.workers
    print(json.dumps(res))


if __name__ == "__main__":
    main()
