"""Measure matcher -> assembly loop over synthetic puzzles on one GPU, three routes alternating in one process; print one JSON line.

    python tools/assemble_bench.py [--puzzles 64] [--in-flight 32] [--reps 5] [--warmup 2] [--out FILE]

Input: `--puzzles` puzzles of tools/make_synthetic_dataset.py (pc_data files, 1000 points per part, 2..20 parts) and for each a
descriptor file built by tests/matching_cases.py's construction (its head weights; 5000 by-area points spread evenly over the parts,
matches between consecutive parts), written to a temporary directory.  The loop runs with random-init weights as bench.py's batched
auto_aggl line does (20 DDPM steps per outer iteration, up to 6 iterations), `--in-flight` puzzles per test_batch call.

* route "files": python -m pfpp_hip.generate_matching_data --assignment device --edges device into a fresh directory, then
  GeometryLatentDataset from that directory and AutoAgglomerative.test_batch per group (prepare_matching and edge_features per puzzle);
* route "assembler": pfpp_hip.assemble.Assembler (matches stay on the device, one edge-feature launch per outer iteration);
* route "assembler_device_frames": the same with frames="device" (a group's initial frames from one pfpp_test_frames call instead of
  the dataset's per-puzzle host arithmetic).  Its rotations come from the device generator, so its loop sees other inputs than the
  two routes above: its records are not compared with theirs.

All routes get the same seeds.  Wall clock per route run, ending in a device synchronise; `--warmup` pairs, then `--reps` pairs,
medians with all values listed.  The edge-feature stage of every outer iteration is bracketed by HIP events, and the calls of the HIP
entries inside it are counted.  On a commit without pfpp_hip.assemble only the "files" route runs (the baseline), with the events
around every per-puzzle edge_features() call.  The frame preparation of a group (Assembler.group_dicts: dataset items to the
batch-of-one dicts on the device) is bracketed by the host clock, ending in a device synchronise, for both Assembler routes."""
from __future__ import annotations

import argparse
import importlib.util
import json
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))
POINTS_BY_AREA = 5000


def load_module(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_inputs(root: Path, n: int):
    """pc_data, descriptor files and the matcher's checkpoint under root -> the data ids"""
    cases = load_module("matching_cases", ROOT / "tests" / "matching_cases.py")
    synth = load_module("make_synthetic_dataset", ROOT / "tools" / "make_synthetic_dataset.py")
    from pfpp_hip import synthetic

    (root / "features").mkdir(parents=True)
    torch.save({"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}}, root / "jigsaw.ckpt")
    ids = []
    for k in range(n):
        pid = 700 + k
        synth.write_puzzle(root, pid, "val")
        pv = int(synthetic.make_puzzle(pid)["num_parts"])
        sizes = [POINTS_BY_AREA // pv] * pv
        per = min(60, sizes[0] // 4)
        pz = cases.build_puzzle(sizes, [(p, p + 1, per) for p in range(pv - 1)], [], pid)
        np.savez(root / "features" / f"{pid}.npz", part_feats=pz["part_feats"], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"])
        ids.append(pid)
    shutil.rmtree(root / "matching_data", ignore_errors=True)               # write_puzzle's synthetic matches are not used
    return ids


class StageTimer:
    """HIP events around the edge-feature stage and counts of the HIP entries called inside it"""

    def __init__(self):
        self.stages, self.launches, self.inside, self.records = [], [], False, []

    def wrap_stage(self, fn):
        def stage(todo):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.launches.append({"puzzles": len(todo)})
            self.inside = True
            e0.record()
            out = fn(todo)
            e1.record()
            self.inside = False
            self.stages.append((e0, e1))
            return out

        return stage

    def wrap_call(self, fn):                              # the parent's stage: one edge_features() call per puzzle
        def call(state):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.launches.append({"puzzles": 1})
            self.inside = True
            e0.record()
            out = fn(state)
            e1.record()
            self.inside = False
            self.stages.append((e0, e1))
            return out

        return call

    def wrap_entry(self, name, fn):
        def entry(*a, **k):
            if self.inside:
                self.launches[-1][name] = self.launches[-1].get(name, 0) + 1
            return fn(*a, **k)

        return entry

    def take(self):
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.stages]
        launches = self.launches
        self.stages, self.launches = [], []
        return ms, launches


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=64)
    ap.add_argument("--in-flight", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("assemble_bench: no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    from pfpp_hip import config, ops
    from pfpp_hip import generate_matching_data as gen
    from puzzlefusion_plusplus import auto_aggl
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative
    from puzzlefusion_plusplus.denoiser.dataset.dataset import GeometryLatentDataset

    try:
        from pfpp_hip import assemble
    except ImportError:
        assemble = None
    root = Path(tempfile.mkdtemp(prefix="assemble_bench_"))
    try:
        ids = write_inputs(root, args.puzzles)
        pc = str(root / "pc_data" / "val")
        cfg = config.auto_aggl_config()
        cfg.denoiser.data = NS(max_num_part=20, data_val_dir=pc, matching_data_path=None)
        torch.manual_seed(4321)
        model = AutoAgglomerative(cfg).to(dev).eval()
        with torch.no_grad():
            model.encoder.vector_quantization.embedding.weight.uniform_(-1.0, 1.0)
        timer = StageTimer()
        if hasattr(AutoAgglomerative, "_edge_features"):
            AutoAgglomerative._edge_features = staticmethod(timer.wrap_stage(AutoAgglomerative._edge_features))
            stage_measure = "one HIP event pair around the edge-feature stage of an outer iteration (host gaps between its launches included)"
        else:
            auto_aggl._PuzzleState.edge_features = timer.wrap_call(auto_aggl._PuzzleState.edge_features)
            stage_measure = "one HIP event pair around every per-puzzle edge_features() call; per outer iteration = mean per call x puzzles in flight"
        for name in ("pose_apply_points", "edge_histogram", "edge_features_batch"):
            if hasattr(ops, name):
                setattr(ops, name, timer.wrap_entry(name, getattr(ops, name)))

        def as_batch(item):
            from torch.utils.data import default_collate

            out = default_collate([item])
            move = lambda v: v.to(dev) if torch.is_tensor(v) else [move(x) for x in v] if isinstance(v, list) else v
            return {k: move(v) for k, v in out.items()}

        def files_route(rep: int):
            mdir = root / f"matching_data_{rep}"
            rc = gen.main(["--features", str(root / "features"), "--checkpoint", str(root / "jigsaw.ckpt"), "--out", str(mdir), "--batch-size",
                           str(args.in_flight), "--assignment", "device", "--edges", "device"])
            assert rc == 0
            cfg.denoiser.data.matching_data_path = str(mdir)
            np.random.seed(0)
            torch.manual_seed(0)
            ds = GeometryLatentDataset(cfg.denoiser, pc, -1, "test")
            index = {s["data_id"]: k for k, s in enumerate(ds.data_list)}
            res = []
            for i in range(0, len(ids), args.in_flight):
                res += model.test_batch([as_batch(ds[index[d]]) for d in ids[i:i + args.in_flight]])
            shutil.rmtree(mdir)
            return [(float(r["metrics"]["part_acc"][0]), r["steps"], r["verifier_calls"], r["merges"]) for r in res]

        frame_s = []                                        # wall clock of every group_dicts call of the route that is running
        with_frames = assemble is not None and hasattr(assemble.Assembler, "group_dicts")
        if with_frames:
            plain_group_dicts = assemble.Assembler.group_dicts

            def timed_group_dicts(self, ds, rows, dev_):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = plain_group_dicts(self, ds, rows, dev_)
                torch.cuda.synchronize()
                frame_s.append(time.perf_counter() - t0)
                return out

            assemble.Assembler.group_dicts = timed_group_dicts

        def assembler_route(rep: int, **kw):
            asm = assemble.Assembler(cfg, model, str(root / "jigsaw.ckpt"), features=str(root / "features"), in_flight=args.in_flight, seed=0, **kw)
            recs = asm.run(None, ids=ids, log=lambda s: None)
            return [(r["part_acc"], r["steps"], r["verifier_calls"], r["merges"]) for r in recs]

        routes = {"files": files_route}
        if assemble is not None:
            routes["assembler"] = assembler_route
        if with_frames:
            routes["assembler_device_frames"] = lambda rep: assembler_route(rep, frames="device")
        walls = {k: [] for k in routes}
        stage_ms = {k: [] for k in routes}
        frames_ms = {k: [] for k in routes}                 # per timed run: the sum over its groups
        launches, last = {}, {}
        import io
        from contextlib import redirect_stdout

        for rep in range(args.warmup + args.reps):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with redirect_stdout(io.StringIO()):
                    last[name] = fn(rep)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ms, counted = timer.take()
                spent, frame_s[:] = list(frame_s), []
                if rep >= args.warmup:
                    walls[name].append(dt)
                    if spent:
                        frames_ms[name].append(1e3 * sum(spent))
                    stage_ms[name] += ms
                    launches[name] = counted
        line = {"bench": "assemble", "puzzles": len(ids), "in_flight": args.in_flight, "reps": args.reps, "warmup_pairs": args.warmup,
                "device_name": torch.cuda.get_device_name(dev), "stage_measure": stage_measure,
                "routes_equal": (last["files"] == last["assembler"]) if assemble is not None else None,
                "ddpm_steps_per_puzzle": sorted({r[1] for r in last["files"]}), "verifier_calls_per_puzzle": sorted({r[2] for r in last["files"]})}
        for name in routes:
            w = walls[name]
            line[name] = {"puzzles_per_s_median": round(len(ids) / statistics.median(w), 2), "puzzles_per_s_all": [round(len(ids) / x, 2) for x in w],
                          "wall_s_all": [round(x, 4) for x in w],
                          "edge_stage_ms_median": round(statistics.median(stage_ms[name]), 4) if stage_ms[name] else None,
                          "edge_stage_ms_min_max": [round(min(stage_ms[name]), 4), round(max(stage_ms[name]), 4)] if stage_ms[name] else None,
                          "edge_stage_events": len(stage_ms[name])}
            if frames_ms[name]:
                f = frames_ms[name]
                line[name]["frames_ms_per_run_median"] = round(statistics.median(f), 3)
                line[name]["frames_ms_per_run_all"] = [round(x, 3) for x in f]
                line[name]["frames_measure"] = "host clock around every group's frame preparation, device synchronise before and after, summed over the groups of a run"
            if launches.get(name):
                full = [c for c in launches[name] if c["puzzles"] == max(x["puzzles"] for x in launches[name])]
                line[name]["hip_entry_calls_per_stage"] = full[0]
                line[name]["hip_entry_calls_per_stage_all_equal"] = all(c == full[0] for c in full)
        text = json.dumps(line)
        print(text)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(text + "\n")
        return 0
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
