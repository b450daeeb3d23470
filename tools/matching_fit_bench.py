"""Measure one epoch's pieces of the matcher's fit loop (pfpp_hip.matching_fit) on one GPU; print one JSON line.

    python tools/matching_fit_bench.py [--puzzles 16] [--points 5000] [--reps 6] [--out profiles/matching_fit_bench_line.json]

Workload: `tools/make_synthetic_meshes.py --bench 16` (16 puzzles of 20 parts) in a resident MeshStore, batches of 2 (the reference's
BATCH_SIZE) and of 16 puzzles at 5,000 points, the matching phase of the loss (w_cls_loss = w_mat_loss = 1).  A step is the descriptor
engine's forward, the head's loss, backward and the optimizer.  After every batch ran once on each path the timed steps ALTERNATE between the two
optimizer paths on the same model: the four engines' own optimizer_step (one pfpp_adamw launch and one ctypes call per tensor, 175
of them: the parent's path) and MatcherOptimizer (pfpp_adam_multi).  Both paths compute the same bits, so the alternation does not
change what the next step sees.  Device events stand at the step's start, behind the backward and behind the optimizer; the host
clock around the optimizer call is its enqueue cost.  Reported per batch size: median step time, the optimizer's device time and its
share of the step for both paths, the launches per step.  Then the validation pass (MatcherValidator.step) over the 16 puzzles in
batches of 2: time per puzzle and the host assignment's share of it.  No time is asserted anywhere."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=16)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--min-part-point", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6, help="timed steps per batch size (half of them on each optimizer path)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from pfpp_hip import meshes as Mh
    from pfpp_hip.matching import DescriptorNetwork, MatchingHead
    from pfpp_hip.matching_dataset import AllPieceMatchingDataset, MeshStore
    from pfpp_hip.matching_encoder_train import DescriptorTrainEngine
    from pfpp_hip.matching_fit import MatcherOptimizer, MatcherValidator, plan_adam_multi
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine
    from pfpp_hip.matching_train import MatchingHeadLoss

    assert torch.cuda.is_available(), "matching_fit_bench measures the GPU path: no GPU here"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_meshes.py"), tmp, "--bench", str(a.puzzles)], check=True)
        rels = list(json.load(open(os.path.join(tmp, "truth.json"))))
        puzzles = [[Mh.read_obj(os.path.join(tmp, r, f)) for f in sorted(os.listdir(os.path.join(tmp, r)))] for r in rels]
        store = MeshStore.from_meshes(puzzles, list(range(a.puzzles)), rels, dev)
        ds = AllPieceMatchingDataset(tmp, "everyday.train.txt", [], num_points=a.points, min_part_point=a.min_part_point, overfit=-1, seed=1,
                                     device=dev, store=store)
    torch.manual_seed(0)
    net, head = DescriptorNetwork().to(dev), MatchingHead().to(dev)
    desc = DescriptorTrainEngine(net)
    head_eng = MatchingHeadRigidTrainEngine(head, w_cls_loss=1.0, w_mat_loss=1.0)
    opt = MatcherOptimizer(desc, head_eng)
    sizes = [opt._param(k).numel() for k in opt.names]
    line = {"bench": "matching_fit", "puzzles": a.puzzles, "points": a.points, "parameters": len(sizes), "elements": sum(sizes),
            "launches_per_step_per_tensor": len(sizes), "launches_per_step_multi": len(plan_adam_multi(sizes)), "reps": a.reps}

    def step(d, path, seed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        feats = desc.forward(d["part_pcs"], d["n_pcs"], d["part_valids"], seed=seed)
        loss = MatchingHeadLoss.apply(feats, head_eng, d["gt_pcs"], d["n_pcs"], d["part_valids"], d["critical_label_thresholds"], None, d["part_pcs"])
        loss.backward()
        ev[1].record()
        t0 = time.perf_counter()
        if path == "per_tensor":
            desc.optimizer_step(lr=1e-3)
            head_eng.optimizer_step(lr=1e-3)
        else:
            opt.step(1e-3)
        host_ms = (time.perf_counter() - t0) * 1e3
        ev[2].record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss.detach())), "the loss is not finite"
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), host_ms

    for bs in (2, min(16, a.puzzles)):
        batches = [ds.batch(list(range(i, i + bs)), epoch=0) for i in range(0, a.puzzles - bs + 1, bs)]
        for w, d in enumerate(batches):                                         # every batch of the timed window once on each path
            for path in ("per_tensor", "multi"):
                step(d, path, w)
        rec = {"per_tensor": [], "multi": []}
        for r in range(a.reps):
            path = ("per_tensor", "multi")[r % 2]
            rec[path].append(step(batches[(r // 2) % len(batches)], path, 10 + r // 2))      # both paths see the same batches
        out = {}
        for path, rows in rec.items():
            fb, op, host = (statistics.median(x) for x in zip(*rows))
            out[path] = {"fwd_bwd_ms": round(fb, 3), "optimizer_ms": round(op, 3), "optimizer_host_ms": round(host, 3), "step_ms": round(fb + op, 3),
                         "optimizer_share": round(op / (fb + op), 4), "optimizer_ms_all": [round(x[1], 3) for x in rows]}
        line[f"batch_{bs}"] = out

    val = MatcherValidator(net, head)
    wall, host, n_crit = [], [], []
    for rep in range(2):                                                        # the first pass warms up
        wall, host, n_crit = [], [], []
        for i in range(0, a.puzzles - 1, 2):
            d = ds.batch([i, i + 1], epoch=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val.step(d, seed=i)
            wall.append((time.perf_counter() - t0) * 1e3 / 2)
            host.append(val.timings["host_assignment_s"] * 1e3 / 2)
            n_crit += [int(x) for x in val.saved["n_critical_pcs"].sum(1).tolist()]
    line["validation"] = {"ms_per_puzzle": round(statistics.median(wall), 3), "host_assignment_ms_per_puzzle": round(statistics.median(host), 3),
                          "host_assignment_share": round(statistics.median(host) / statistics.median(wall), 4),
                          "critical_points_per_puzzle_median": statistics.median(n_crit)}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
