"""pc_data from the Breaking Bad meshes on one GPU — the reference's step zero (generate_pc_data.py:11-47)

    python -m pfpp_hip.generate_pc_data --config-dir <reference>/config/ae +data.save_pc_data_path=DIR \\
        [data.batch_size=64] [+data.pc_seed=S]

writes DIR/{train,val}/<data_id:05>.npz through pfpp_hip.io.save_pc_data, one progress line per split.  The reference forces batch
size 1; here the batch size is 1 unless data.batch_size is given on the command line, and the files do not depend on it (the
uniforms are keyed by puzzle, part and sample).  An unreadable mesh ends the run with a non-zero exit status naming the file."""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List, Optional


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pfpp_hip.generate_pc_data", description=__doc__.split("\n\n")[0])
    ap.add_argument("--config-dir", required=True, help="the reference's config/ae (or a tree with the same keys)")
    ap.add_argument("--config-name", default="global_config")
    ap.add_argument("overrides", nargs="*", help="Hydra-style overrides: a.b=c, +a.b=c")
    args = ap.parse_args(argv)

    import torch

    from pfpp_hip import io as pfio
    from pfpp_hip.config import to_namespace
    from pfpp_hip.launch import compose
    from puzzlefusion_plusplus.vqvae.dataset.dataset import MeshReadError, build_geometry_dataloader

    tree = compose(args.config_dir, args.config_name, args.overrides)
    given = {ov.lstrip("+").partition("=")[0] for ov in args.overrides}
    data = tree.setdefault("data", {})
    if "data.batch_size" not in given:
        data["batch_size"] = 1
    if "data.val_batch_size" not in given:
        data["val_batch_size"] = data["batch_size"]
    data.setdefault("pc_seed", 0)
    save = data.get("save_pc_data_path")
    if not save:
        ap.error("+data.save_pc_data_path=DIR is required")
    if not torch.cuda.is_available():
        print("generate_pc_data: no GPU: the sampling and contact-graph kernels run on the GPU only", file=sys.stderr)
        return 2
    cfg = to_namespace(tree)
    try:
        train_loader, val_loader = build_geometry_dataloader(cfg, drop_last_train=False)
        for loader, split in ((train_loader, "train"), (val_loader, "val")):
            out = os.path.join(save, split)
            os.makedirs(out, exist_ok=True)
            t0, n = time.perf_counter(), 0
            for batch in loader.pc_data():
                for d in batch:
                    pfio.save_pc_data(out, **d)
                    n += 1
            dt = time.perf_counter() - t0
            print(f"{split}: {n} puzzles -> {out} in {dt:.2f} s ({n / max(dt, 1e-9):.1f} files/s)", flush=True)
    except MeshReadError as e:
        print(f"generate_pc_data: {e}", file=sys.stderr)
        return 1
    except Exception as e:        # an error re-raised from a loader worker keeps the worker's message (MeshReadError names the file)
        if "cannot read mesh" in str(e):
            print(f"generate_pc_data: {e}", file=sys.stderr)
            return 1
        raise
    return 0


if __name__ == "__main__":
    sys.exit(main())
