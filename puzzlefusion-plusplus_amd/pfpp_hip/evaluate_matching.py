"""Score a trained matcher over a directory of puzzles on one GPU — the reference's test pass (Jigsaw_matching/, transformation_loss)

    python -m pfpp_hip.evaluate_matching (--points DIR | --features DIR) --checkpoint CKPT [--n-hyp 50000] [--seed S] [--refine]
                                         [--batch-size 16] [--gemm f32|f16x3] [--shape-cd-index reference|corrected]

The files, the checkpoint and the models are pfpp_hip.generate_matching_data's (one DIR/<data_id>.npz per puzzle; --points runs the
descriptor network in front of the head, --features reads the descriptors), with two more entries per file: part_quat float32 [P, 4]
(w, x, y, z) and part_trans float32 [P, 3], the pieces' ground-truth poses (gt = R part + t), and part_pcs [N_sum, 3] also where
the descriptors are given.  Each batch goes through pfpp_hip.matching_eval.MatchingEvaluator: the pairwise RANSAC of the batch in one
launch, global alignment, the pivot anchoring, the metrics.  Puzzles of a batch with different point counts are evaluated one by one.
Printed: one JSON line with the metrics averaged over the puzzles (part_acc, chamfer_distance, trans_{mse,rmse,mae},
rot_{mse,rmse,mae}) and their number."""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import List, Optional

from .generate_matching_data import head_batches, list_puzzles

POSE_KEYS = ("part_pcs", "part_quat", "part_trans")


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pfpp_hip.evaluate_matching", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--points", help="directory of <data_id>.npz point-cloud files (the descriptor network runs in front of the head)")
    src.add_argument("--features", help="directory of <data_id>.npz descriptor files (with part_pcs)")
    ap.add_argument("--checkpoint", required=True, help="Jigsaw checkpoint (Lightning file or bare state_dict)")
    ap.add_argument("--n-hyp", type=int, default=50000, help="RANSAC hypotheses per piece pair")
    ap.add_argument("--seed", type=int, default=0, help="seed of the RANSAC draws (and, with --points, of the encoder's sampling starts)")
    ap.add_argument("--refine", action="store_true", help="one more Horn over the winning hypothesis's inliers")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--gemm", choices=("f32", "f16x3"), default="f32")
    ap.add_argument("--shape-cd-index", choices=("reference", "corrected"), default="reference")
    ap.add_argument("--assignment", choices=("host", "device"), default="host",
                    help="the optimal assignment: scipy on the host, or the batched exact solver on the GPU (pfpp_hip.matching_assign)")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be at least 1")
    if args.n_hyp < 1:
        ap.error("--n-hyp must be at least 1")
    source, flag = (args.points, "--points") if args.points is not None else (args.features, "--features")
    if not os.path.isdir(source):
        ap.error(f"{flag} {source}: not a directory")
    if not os.path.isfile(args.checkpoint):
        ap.error(f"--checkpoint {args.checkpoint}: no such file")
    todo, _ = list_puzzles(source, os.path.join(source, ".none"))
    if not todo:
        print("evaluate_matching: no <data_id>.npz in " + source, file=sys.stderr)
        return 1

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        print("evaluate_matching: no GPU: the matching kernels run on the GPU only", file=sys.stderr)
        return 2
    from .matching_eval import MatchingEvaluator

    ev = MatchingEvaluator(n_hyp=args.n_hyp, seed=args.seed, refine=args.refine, shape_cd_index=args.shape_cd_index)
    for ids, items, n_pcs, valids, out in head_batches(source, args.points is not None, args.checkpoint, args.gemm, args.seed, todo, args.batch_size,
                                                       extra=POSE_KEYS, solver=args.assignment):
        P = n_pcs.shape[1]
        nc = out.n_critical_pcs.cpu().numpy()
        same = len({x["part_pcs"].shape[0] for x in items}) == 1
        for group in ([list(range(len(items)))] if same else [[b] for b in range(len(items))]):
            cuda = lambda key, width: torch.from_numpy(np.stack([np.ascontiguousarray(items[b][key], dtype=np.float32).reshape(-1, width) for b in group])).cuda()
            padp = lambda key, width: torch.from_numpy(np.stack([np.concatenate([np.asarray(items[b][key], dtype=np.float32).reshape(-1, width),
                                                                                 np.zeros((P - items[b]["n_pcs"].shape[0], width), dtype=np.float32)])
                                                                 for b in group])).cuda()
            data = {"part_pcs": cuda("part_pcs", 3), "gt_pcs": cuda("gt_pcs", 3), "n_pcs": n_pcs[group], "part_valids": torch.from_numpy(valids[group]).cuda(),
                    "part_quat": padp("part_quat", 4), "part_trans": padp("part_trans", 3), "n_critical_pcs": nc[group],
                    "critical_pcs_idx": torch.stack([out.critical_pcs_idx[b] for b in group])}
            ev.transformation_metrics(data, {"perm_mat": [out.perm_mat[b] for b in group]})
    line = {k: float(np.concatenate([np.atleast_1d(v) for v in ev.stats[k]]).mean()) for k in ev.KEYS}
    line["puzzles"] = int(sum(np.atleast_1d(v).size for v in ev.stats["part_acc"]))
    line.update(n_hyp=args.n_hyp, seed=args.seed, refine=bool(args.refine))
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
