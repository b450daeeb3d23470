"""python -m pfpp_hip.train_matching --cfg FILE [KEY VALUE ...]: the reference's Jigsaw_matching/train_matching.py on the HIP path.
FILE is one of the reference's experiment yaml files, read over the defaults its utils/config.py, dataset_config.py and
model_config.py set (pfpp_hip.matching_fit.default_config); KEY VALUE pairs override dotted keys as its cfg_from_list does.
One key is this tree's own: VAL_ASSIGNMENT host|device, the validation pass's assignment solver (default host)."""
from __future__ import annotations

import argparse
import sys


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfg", "--config", dest="cfg_file", action="append", default=None, help="an experiment yaml file")
    ap.add_argument("--max-epochs", type=int, default=None, help="stop after this epoch count (a later run resumes)")
    ap.add_argument("overrides", nargs="*", help="KEY VALUE pairs, e.g. TRAIN.NUM_EPOCHS 3")
    args = ap.parse_args(argv)
    from .matching_fit import fit, load_config

    cfg = load_config(args.cfg_file, args.overrides)
    trainer = fit(cfg, max_epochs=args.max_epochs)
    print(f"trained to epoch {trainer.epoch}, {trainer.global_step} steps; log {trainer.log_path}; checkpoints in {trainer.save_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
