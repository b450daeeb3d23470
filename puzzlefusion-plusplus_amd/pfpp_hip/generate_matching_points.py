"""The matcher's point-cloud files from the Breaking Bad meshes on one GPU

    python -m pfpp_hip.generate_matching_points --data-dir D --data-fn 'everyday.{}.txt' --split val --out DIR
        [--num-points 5000] [--min-part-point 30] [--seed S] [--epoch E] [--batch-size 16] [--store FILE] [--category all]
        [--min-num-part 2] [--max-num-part 20] [--rot-range -1] [--workers 16]

writes DIR/<data_id>.npz with part_pcs, gt_pcs float32 [N, 3], n_pcs int64 [P], part_valids float32 [P], part_quat float32 [P, 4]
and part_trans float32 [P, 3]: the files pfpp_hip.generate_matching_data --points and pfpp_hip.evaluate_matching --points read.  A
file that exists is left alone and its puzzle is not computed.  --store names a file of the parsed meshes (pfpp_hip.matching_dataset
.MeshStore): read when it exists, written after the parse otherwise.  Without a GPU the command ends with status 2."""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List, Optional


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pfpp_hip.generate_matching_points", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--data-fn", required=True, help="the split lists' name with {} for the split, e.g. 'everyday.{}.txt'")
    ap.add_argument("--split", required=True, choices=("train", "val"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--num-points", type=int, default=5000)
    ap.add_argument("--min-part-point", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epoch", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--store", help="file of the parsed meshes: read when it exists, written otherwise")
    ap.add_argument("--category", default="all")
    ap.add_argument("--min-num-part", type=int, default=2)
    ap.add_argument("--max-num-part", type=int, default=20)
    ap.add_argument("--rot-range", type=float, default=-1.0)
    ap.add_argument("--workers", type=int, default=None, help="processes of the parse pool (at most 16; 0 parses in this process)")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be at least 1")

    import numpy as np
    import torch

    from pfpp_hip.matching_dataset import POINT_FILE_KEYS, AllPieceMatchingDataset

    if not torch.cuda.is_available():
        print("generate_matching_points: no GPU: the sampling and pose kernels run on the GPU only", file=sys.stderr)
        return 2
    ds = AllPieceMatchingDataset(args.data_dir, args.data_fn.format(args.split), [], category=args.category, num_points=args.num_points,
                                 min_num_part=args.min_num_part, max_num_part=args.max_num_part, rot_range=args.rot_range, overfit=-1,
                                 min_part_point=args.min_part_point, seed=args.seed, split=args.split, store=args.store, workers=args.workers)
    os.makedirs(args.out, exist_ok=True)
    todo = [i for i in range(len(ds)) if not os.path.exists(os.path.join(args.out, f"{i}.npz"))]
    t0 = time.perf_counter()
    for k in range(0, len(todo), args.batch_size):
        ids = todo[k:k + args.batch_size]
        host = {key: v.cpu().numpy() for key, v in ds.batch(ids, args.epoch).items() if key in POINT_FILE_KEYS}
        for b, i in enumerate(ids):
            tmp = os.path.join(args.out, f".{i}.tmp.npz")
            np.savez(tmp, **{key: host[key][b] for key in POINT_FILE_KEYS})
            os.replace(tmp, os.path.join(args.out, f"{i}.npz"))
    dt = time.perf_counter() - t0
    print(f"{args.split}: {len(todo)} puzzles -> {args.out} in {dt:.2f} s, {len(ds) - len(todo)} existing files left alone", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
