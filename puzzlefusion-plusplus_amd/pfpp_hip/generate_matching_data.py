"""matching_data from point clouds or from per-point descriptors on one GPU — the reference's matcher (Jigsaw_matching/, test run)

    python -m pfpp_hip.generate_matching_data (--points DIR | --features DIR) --checkpoint CKPT --out DIR [--batch-size 16]
                                              [--gemm f32|f16x3] [--seed S] [--assignment host|device] [--edges host|device]

--points reads one DIR/<data_id>.npz per puzzle (part_pcs float32 [N_sum, 3]: the pieces' points as the matcher sees them, gt_pcs
float32 [N_sum, 3], n_pcs int64 [P], part_valids [P]) and runs pfpp_hip.matching.DescriptorNetwork (encoder, tf_self1, tf_cross1) in
front of the head; --features reads the descriptors themselves (part_feats float32 [N_sum, 128] in place of part_pcs: the seam
between the two).  Either way pfpp_hip.matching.MatchingHead runs in batches and OUT/<data_id>.npz is written
through pfpp_hip.io.save_matching_data.  A file that exists is left alone and its puzzle is not computed.  --edges device builds
the files' edges and correspondences of a whole batch in one launch (pfpp_hip.matching_edges) instead of per puzzle on the host; the
files hold the same arrays."""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List, Optional

FEATURE_KEYS = ("part_feats", "gt_pcs", "n_pcs", "part_valids")
POINT_KEYS = ("part_pcs", "gt_pcs", "n_pcs", "part_valids")


def list_puzzles(features: str, out: str):
    """-> (data ids still to do, ids skipped because their file exists); a file name that is not <integer>.npz is an error"""
    todo, skipped = [], []
    for name in sorted(os.listdir(features)):
        if not name.endswith(".npz"):
            continue
        stem = name[:-4]
        if not stem.isdigit():
            raise ValueError(f"{os.path.join(features, name)}: feature files are named <data_id>.npz")
        (skipped if os.path.exists(os.path.join(out, f"{int(stem)}.npz")) else todo).append(int(stem))
    return sorted(todo), sorted(skipped)


def load_features(features: str, data_id: int, points: bool = False, extra=()):
    """one puzzle's file: the descriptors (part_feats [N_sum, 128]) or, with points, the point clouds (part_pcs [N_sum, 3]); extra:
    further entries the caller needs (they must be there)"""
    import numpy as np

    keys, first, width = (POINT_KEYS, "part_pcs", 3) if points else (FEATURE_KEYS, "part_feats", 128)
    keys = tuple(keys) + tuple(k for k in extra if k not in keys)
    path = os.path.join(features, f"{data_id}.npz")
    with np.load(path) as d:
        missing = [k for k in keys if k not in d.files]
        if missing:
            raise KeyError(f"{path}: missing entries {missing}")
        x = {k: d[k] for k in keys}
    n = int(np.asarray(x["n_pcs"]).sum())
    if x[first].shape != (n, width) or x["gt_pcs"].shape != (n, 3) or x["n_pcs"].shape != x["part_valids"].shape:
        raise ValueError(f"{path}: {first} {x[first].shape}, gt_pcs {x['gt_pcs'].shape} do not match n_pcs (sum {n})")
    return x


def head_batches(source: str, points: bool, checkpoint: str, gemm: str, seed: int, todo, batch_size: int, extra=(), dense_perm: bool = False,
                 solver: str = "host"):
    """the models of a checkpoint over the puzzles `todo` of a directory, batch by batch: pfpp_hip.matching.DescriptorNetwork in
    front of the head when the files hold points, the head alone when they hold descriptors
    (solver: the head's assignment solver, "host" or "device")
    -> yields (data ids, the puzzles' files, n_pcs [b, P], part_valids [b, P], the head's output)"""
    import numpy as np
    import torch

    from pfpp_hip.matching import DescriptorNetwork, MatchingHead

    head = MatchingHead.from_checkpoint(checkpoint, gemm_mode=gemm).cuda()
    net = DescriptorNetwork.from_checkpoint(checkpoint, gemm_mode=gemm).cuda() if points else None
    for i in range(0, len(todo), batch_size):
        ids = todo[i:i + batch_size]
        items = [load_features(source, d, points=net is not None, extra=extra) for d in ids]
        P = max(x["n_pcs"].shape[0] for x in items)
        pad = lambda a: np.concatenate([np.asarray(a).reshape(-1), np.zeros(P - a.shape[0], dtype=a.dtype)])
        n_pcs, valids = np.stack([pad(x["n_pcs"].astype(np.int64)) for x in items]), np.stack([pad(x["part_valids"].astype(np.float32)) for x in items])
        if net is not None:          # descriptors of the whole batch, flat, as the head takes them
            feats = net([torch.from_numpy(np.ascontiguousarray(x["part_pcs"], dtype=np.float32)).cuda() for x in items], n_pcs, valids,
                        seed=seed + i)
        else:
            feats = [torch.from_numpy(np.ascontiguousarray(x["part_feats"], dtype=np.float32)).cuda() for x in items]
        yield ids, items, n_pcs, valids, head(feats, n_pcs, valids, dense_perm=dense_perm, solver=solver)


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pfpp_hip.generate_matching_data", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--points", help="directory of <data_id>.npz point-cloud files (the descriptor network runs in front of the head)")
    src.add_argument("--features", help="directory of <data_id>.npz descriptor files")
    ap.add_argument("--checkpoint", required=True, help="Jigsaw checkpoint (Lightning file or bare state_dict)")
    ap.add_argument("--out", required=True, help="matching_data directory")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--gemm", choices=("f32", "f16x3"), default="f32")
    ap.add_argument("--seed", type=int, default=0, help="--points: seed of the encoder's sampling starts (the reference draws them at random)")
    ap.add_argument("--assignment", choices=("host", "device"), default="host",
                    help="the optimal assignment: scipy on the host, or the batched exact solver on the GPU (pfpp_hip.matching_assign)")
    ap.add_argument("--edges", choices=("host", "device"), default="host",
                    help="the pair rule that turns the assignment into edges and correspondences: numpy per puzzle on the host, or one "
                         "launch per batch on the GPU (pfpp_hip.matching_edges)")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be at least 1")
    source, flag = (args.points, "--points") if args.points is not None else (args.features, "--features")
    if not os.path.isdir(source):
        ap.error(f"{flag} {source}: not a directory")
    if not os.path.isfile(args.checkpoint):
        ap.error(f"--checkpoint {args.checkpoint}: no such file")
    todo, skipped = list_puzzles(source, args.out)
    if skipped:
        print(f"{len(skipped)} puzzles already in {args.out}: left alone", flush=True)
    if not todo:
        print("nothing to do", flush=True)
        return 0

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        print("generate_matching_data: no GPU: the matching kernels run on the GPU only", file=sys.stderr)
        return 2
    from pfpp_hip.matching import match_edges, write_matching_data
    from pfpp_hip.matching_edges import match_edges_batch

    t0, n, host, device = time.perf_counter(), 0, 0.0, 0.0
    for ids, items, n_pcs, valids, out in head_batches(source, args.points is not None, args.checkpoint, args.gemm, args.seed, todo, args.batch_size,
                                                       solver=args.assignment):
        host += out.timings["host_assignment_s"]
        device += out.timings["device_assignment_s"]
        nc = out.n_critical_pcs.cpu().numpy()
        n_valid = [int(np.asarray(x["part_valids"]).sum()) for x in items]
        dm = match_edges_batch(out.perm_mat, out.n_critical_pcs, n_valid, n_pcs, out.critical_pcs_idx) if args.edges == "device" else None
        for b, (d, x) in enumerate(zip(ids, items)):
            p = x["n_pcs"].shape[0]
            edges, corr = dm.files(b) if dm is not None else match_edges(out.perm_mat[b], nc[b], n_valid[b])
            write_matching_data(args.out, d, edges=edges, correspondence=corr, gt_pcs=x["gt_pcs"], critical_pcs_idx=out.critical_pcs_idx[b],
                                n_pcs=x["n_pcs"], n_critical_pcs=nc[b, :p])
            n += 1
    dt = time.perf_counter() - t0
    print(f"{n} puzzles -> {args.out} in {dt:.2f} s ({n / max(dt, 1e-9):.1f} files/s; host assignment {host:.2f} s" +
          (f", device assignment {device:.2f} s" if args.assignment == "device" else "") + ")", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
