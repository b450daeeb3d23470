"""Fragments and checkpoints in, assembled poses out, in one process on one GPU: the reference's test.py with its matcher
(Jigsaw_matching/, test run) in front and no matching_data file in between.

    python -m pfpp_hip.assemble (--points DIR | --features DIR) --matcher CKPT --out DIR [--denoiser CKPT] [--verifier CKPT]
                                [--config-dir DIR [--config-name auto_aggl]] [--pc-data DIR] [--in-flight 32] [--seed 0]
                                [--gemm f32|f16x3] [--frames host|device] [key=value ...]

Per group of --in-flight puzzles (also the matcher's batch size): pfpp_hip.generate_matching_data.head_batches with the device
assignment (one column per row) -> pfpp_hip.matching_edges.match_edges_batch -> DeviceMatches.batch_prepared() -> the join with
pc_data and the initial frames by GeometryLatentDataset(matching=mapping) -> AutoAgglomerative.test_batch, where every puzzle
carries data_dict["matching_batch"] and the verifier input of all puzzles in flight comes from one launch per outer iteration.  The
matches never leave the GPU.  With --frames device the initial frames of a group (the dataset's random rotations, recentring and the
by-area points in every piece's frame) come from one pfpp_hip.augment.test_frames_batch call instead of the dataset's per-puzzle
scipy / numpy pass; the rotations are then drawn by torch's device generator, so a seed fixes the run but not to --frames host's.

--points / --features: the matcher's input files, as generate_matching_data reads them.  The pc_data directory is the config's
(denoiser.data.data_val_dir, as test.py's build_test_dataloader takes it) or --pc-data; a puzzle without a pc_data file is skipped
and named.  The denoiser / verifier checkpoints are the config's denoiser.ckpt_path / verifier.ckpt_path or --denoiser / --verifier,
loaded by the key rules of test.py:24-38.  The config tree is pfpp_hip.config.auto_aggl_config() or, with --config-dir, the yaml
tree as pfpp_hip.launch.compose reads it; key=value overrides apply to either.

Writes OUT/results.jsonl (one line per puzzle: data_id, part_acc, shape_cd, rmse_r, rmse_t, verifier_calls, merges, steps) and,
when the config sets experiment_output_path, the reference's inference files (AutoAgglomerative._save_inference_data)."""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace as NS
from typing import Dict, Iterator, List, Optional

RESULT_KEYS = ("part_acc", "shape_cd", "rmse_r", "rmse_t")
FRAMES = ("host", "device")              # who makes a group's initial frames: the dataset per puzzle, or pfpp_test_frames per group


def load_loop_weights(model, denoiser_ckpt: str, verifier_ckpt: str) -> None:
    """test.py:24-38: `denoiser.` / `encoder.` of the denoiser file, every key of the verifier file with `verifier.` taken out"""
    import torch

    den = torch.load(denoiser_ckpt, map_location="cpu", weights_only=False)["state_dict"]
    model.denoiser.load_state_dict({k.replace("denoiser.", ""): v for k, v in den.items() if k.startswith("denoiser.")})
    model.encoder.load_state_dict({k.replace("encoder.", ""): v for k, v in den.items() if k.startswith("encoder.")})
    ver = torch.load(verifier_ckpt, map_location="cpu", weights_only=False)["state_dict"]
    model.verifier.load_state_dict({k.replace("verifier.", ""): v for k, v in ver.items()})


def as_batch_of_one(item: dict, device) -> dict:
    """a dataset item -> the batch-1 dict test_batch takes (what the reference's loader with batch size 1 and Lightning's transfer
    make of it); the matching_batch entry travels as it is"""
    import torch
    from torch.utils.data import default_collate

    item = dict(item)
    keep = {k: item.pop(k) for k in ("matching_batch", "matching_prepared") if k in item}
    out = default_collate([item])
    move = lambda v: v.to(device) if torch.is_tensor(v) else [move(x) for x in v] if isinstance(v, list) else v
    out = {k: move(v) for k, v in out.items()}
    out.update(keep)
    return out


class Assembler:
    """matcher -> assembly loop over the puzzles of a directory, `in_flight` at a time.  `model` is an AutoAgglomerative on the GPU
    in eval mode with its weights loaded; cfg its config tree (cfg.denoiser.data names max_num_part and the pc_data directory)."""

    def __init__(self, cfg, model, matcher: str, *, points: Optional[str] = None, features: Optional[str] = None,
                 pc_data: Optional[str] = None, in_flight: int = 32, seed: int = 0, gemm: str = "f32", frames: str = "host"):
        if (points is None) == (features is None):
            raise ValueError("Assembler: exactly one of points= and features=")
        if in_flight < 1:
            raise ValueError("Assembler: in_flight must be at least 1")
        if frames not in FRAMES:
            raise ValueError(f"Assembler: frames={frames!r}, one of {FRAMES}")
        self.frames = frames
        self.cfg, self.model, self.matcher = cfg, model, matcher
        self.source, self.points = (points, True) if points is not None else (features, False)
        self.pc_data = pc_data if pc_data is not None else cfg.denoiser.data.data_val_dir
        self.in_flight, self.seed, self.gemm = int(in_flight), int(seed), gemm
        self.P = int(cfg.denoiser.data.max_num_part)

    # ------------------------------------------------------------------------------------------------ the matcher's half
    def matched_groups(self, ids) -> Iterator[tuple]:
        """-> (data ids, {data_id: mapping entry}) per group of in_flight puzzles.  An entry holds what the dataset and the loop
        read of a matching_data file (gt_pc_by_area, n_pcs, critical_pcs_idx, n_critical_pcs) and, in place of its edges and
        correspondences, matching_batch = (the group's BatchMatches, the puzzle's index in it)."""
        import numpy as np
        import torch

        from .generate_matching_data import head_batches
        from .matching_edges import _flat, match_edges_batch

        P = self.P
        for group, items, n_pcs, valids, out in head_batches(self.source, self.points, self.matcher, self.gemm, self.seed, list(ids),
                                                             self.in_flight, dense_perm=False, solver="device"):
            p = n_pcs.shape[1]
            if p > P:
                raise ValueError(f"{self.source}: puzzles of {p} piece slots, the loop's max_num_part is {P}")
            # pair_pos and the pivots count in the LOOP's P: the matcher's batch is padded to it
            n_pcs = np.pad(n_pcs, ((0, 0), (0, P - p)))
            nc = torch.nn.functional.pad(out.n_critical_pcs.reshape(len(group), p), (0, P - p)) if p < P else out.n_critical_pcs
            n_valid = [int(np.asarray(x["part_valids"]).sum()) for x in items]
            dm = match_edges_batch(out.perm_mat, nc, n_valid, n_pcs, out.critical_pcs_idx)
            bo = dm.batch_prepared()
            crit = _flat(list(out.critical_pcs_idx)).cpu().numpy()           # for the sample only: the loop reads idx_a / idx_b
            nc_host = nc.reshape(len(group), P).cpu().numpy()
            mapping = {}
            for b, (d, x) in enumerate(zip(group, items)):
                o = bo.pt_off_host
                mapping[d] = {"gt_pc_by_area": x["gt_pcs"], "n_pcs": n_pcs[b], "critical_pcs_idx": crit[int(o[b]):int(o[b + 1])],
                              "n_critical_pcs": nc_host[b], "matching_batch": (bo, b)}
            yield group, mapping

    # ------------------------------------------------------------------------------------------------ the initial frames
    def group_dicts(self, ds, rows, dev) -> List[dict]:
        """the batch-of-one dicts of a group (dataset rows `rows`, their mapping entries joined): per puzzle by the dataset's host
        arithmetic, or for the whole group by one pfpp_test_frames call (the dataset then returns the stored geometry only)"""
        if self.frames == "device":
            from .augment import test_frames_batch

            return test_frames_batch([ds[k] for k in rows], dev)
        return [as_batch_of_one(ds[k], dev) for k in rows]

    # ------------------------------------------------------------------------------------------------ the whole route
    def run(self, out_dir: Optional[str] = None, ids=None, log=print) -> List[dict]:
        """all puzzles of the source directory (or `ids`) -> one record per assembled puzzle, in the matcher's order; with out_dir,
        OUT/results.jsonl is written as the groups finish"""
        import numpy as np
        import torch

        from puzzlefusion_plusplus.denoiser.dataset.dataset import GeometryLatentDataset

        from .generate_matching_data import list_puzzles

        if ids is None:
            ids, _ = list_puzzles(self.source, os.devnull)          # nothing counts as done: no <data_id>.npz is ever written
        np.random.seed(self.seed)                        # the dataset's scipy rotations draw from numpy's global generator
        torch.manual_seed(self.seed)                     # also the device generator frames="device" draws its rotations from
        dev = next(self.model.parameters()).device
        # pc_data is read ONCE (a dataset per group would read the whole directory per group); the group's mapping entries are
        # joined to its samples below, which is what the dataset's matching= keyword does at construction
        ds = GeometryLatentDataset(self.cfg.denoiser, self.pc_data, -1, "test", device_augment=self.frames == "device",
                                   matching={d: {} for d in ids})
        index = {s["data_id"]: k for k, s in enumerate(ds.data_list)}
        records: List[dict] = []
        fh = None
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            fh = open(os.path.join(out_dir, "results.jsonl"), "w")
        try:
            for group, mapping in self.matched_groups(ids):
                missing = [d for d in group if d not in index]
                if missing:
                    log(f"skipped (no pc_data file in {self.pc_data}): {' '.join(str(d) for d in missing)}")
                todo = [d for d in group if d in index]
                if not todo:
                    continue
                for d in todo:
                    ds.data_list[index[d]].update(mapping[d])
                results = self.model.test_batch(self.group_dicts(ds, [index[d] for d in todo], dev))
                for d, r in zip(todo, results):
                    rec = {"data_id": int(d), **{k: float(r["metrics"][k][0]) for k in RESULT_KEYS},
                           "verifier_calls": int(r["verifier_calls"]), "merges": int(r["merges"]), "steps": int(r["steps"])}
                    records.append(rec)
                    if fh is not None:
                        fh.write(json.dumps(rec) + "\n")
                        fh.flush()
                for d in todo:                           # the group's tensors go with its BatchMatches
                    ds.data_list[index[d]].pop("matching_batch", None)
        finally:
            if fh is not None:
                fh.close()
        return records


def _override(cfg, dotted: str, value) -> None:
    """key=value / +key=value on an attribute tree (Hydra's rule: a new key needs the +)"""
    create = dotted.startswith("+")
    keys = dotted.lstrip("+").split(".")
    node = cfg
    for k in keys[:-1]:
        if not hasattr(node, k):
            if not create:
                raise KeyError(f"override {dotted}: no such key (prefix it with + to add it, as Hydra does)")
            setattr(node, k, NS())
        node = getattr(node, k)
    if not create and not hasattr(node, keys[-1]):
        raise KeyError(f"override {dotted}: no such key (prefix it with + to add it, as Hydra does)")
    setattr(node, keys[-1], value)


def build_config(config_dir: Optional[str], config_name: str, overrides: List[str]):
    from . import config as cfgmod

    if config_dir is not None:
        from .launch import compose

        return cfgmod.to_namespace(compose(config_dir, config_name, overrides))
    import yaml

    cfg = cfgmod.auto_aggl_config()
    for ov in overrides:
        key, _, val = ov.partition("=")
        _override(cfg, key, cfgmod.to_namespace(yaml.safe_load(val)) if val != "" else None)
    return cfg


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m pfpp_hip.assemble", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--points", help="directory of <data_id>.npz point-cloud files (the descriptor network runs in front of the head)")
    src.add_argument("--features", help="directory of <data_id>.npz descriptor files")
    ap.add_argument("--matcher", required=True, help="Jigsaw checkpoint (Lightning file or bare state_dict)")
    ap.add_argument("--denoiser", help="denoiser checkpoint (default: the config's denoiser.ckpt_path)")
    ap.add_argument("--verifier", help="verifier checkpoint (default: the config's verifier.ckpt_path)")
    ap.add_argument("--out", required=True, help="directory of results.jsonl")
    ap.add_argument("--config-dir", help="yaml tree of the reference (config/); default: pfpp_hip.config.auto_aggl_config()")
    ap.add_argument("--config-name", default="auto_aggl")
    ap.add_argument("--pc-data", help="pc_data directory (default: the config's denoiser.data.data_val_dir)")
    ap.add_argument("--in-flight", type=int, default=32, help="puzzles per group: the matcher's batch size and the loop's")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gemm", choices=("f32", "f16x3"), default="f32", help="the matcher's GEMM mode")
    ap.add_argument("--frames", choices=FRAMES, default="host",
                    help="the initial frames of a group: by the dataset per puzzle on the host, or in one launch on the GPU")
    ap.add_argument("overrides", nargs="*", help="key=value overrides of the config tree")
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.in_flight < 1:
        ap.error("--in-flight must be at least 1")
    source, flag = (args.points, "--points") if args.points is not None else (args.features, "--features")
    if not os.path.isdir(source):
        ap.error(f"{flag} {source}: not a directory")
    if not os.path.isfile(args.matcher):
        ap.error(f"--matcher {args.matcher}: no such file")
    try:
        cfg = build_config(args.config_dir, args.config_name, args.overrides)
    except (KeyError, OSError) as e:
        ap.error(str(e))
    if not hasattr(cfg.denoiser, "data"):
        cfg.denoiser.data = NS(max_num_part=20, data_val_dir=None, matching_data_path=None)
    if args.pc_data is not None:
        cfg.denoiser.data.data_val_dir = args.pc_data
    if not getattr(cfg.denoiser.data, "data_val_dir", None) or not os.path.isdir(cfg.denoiser.data.data_val_dir):
        ap.error(f"pc_data directory {getattr(cfg.denoiser.data, 'data_val_dir', None)}: not a directory (--pc-data or denoiser.data.data_val_dir)")
    ckpts = {}
    for name, given in (("denoiser", args.denoiser), ("verifier", args.verifier)):
        ckpts[name] = given if given is not None else getattr(getattr(cfg, name), "ckpt_path", None)
        if ckpts[name] is None or not os.path.isfile(ckpts[name]):
            ap.error(f"--{name} {ckpts[name]}: no such file (--{name} or {name}.ckpt_path)")

    import torch

    if not torch.cuda.is_available():
        print("assemble: no GPU: the matcher and the assembly loop run on the GPU only", file=sys.stderr)
        return 2
    import time

    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative

    model = AutoAgglomerative(cfg)
    load_loop_weights(model, ckpts["denoiser"], ckpts["verifier"])
    model = model.cuda().eval()
    asm = Assembler(cfg, model, args.matcher, points=args.points, features=args.features, in_flight=args.in_flight, seed=args.seed,
                    gemm=args.gemm, frames=args.frames)
    t0 = time.perf_counter()
    records = asm.run(args.out, log=lambda s: print(s, flush=True))
    dt = time.perf_counter() - t0
    acc = sum(r["part_acc"] for r in records) / max(len(records), 1)
    print(f"{len(records)} puzzles -> {os.path.join(args.out, 'results.jsonl')} in {dt:.2f} s ({len(records) / max(dt, 1e-9):.1f} puzzles/s; "
          f"mean part_acc {acc:.4f})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
