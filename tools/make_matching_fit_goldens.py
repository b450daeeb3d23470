"""Generate tests/golden/matching_fit.npz by RUNNING THE REFERENCE's matcher code on the CPU.

    python tools/make_matching_fit_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching (sys.dont_write_bytecode, nothing is copied): utils/lr.py (CosineAnnealingWarmupRestarts),
utils/utils.py (filter_wd_parameters), model/jigsaw/model_config.py and model/jigsaw/joint_seg_align_model.py: the whole
JointSegmentationAlignmentModel is constructed (its __init__ fixes the parameter order) and its eval-mode forward and _loss_function
run behind given part_feats, which is the reference's validation_step (trainer.testing False).  Packages those files import but which
are not installed get the stand-ins of tools/make_matching_goldens.py; LightningModule is torch.nn.Module with a no-op
save_hyperparameters; torchmetrics' four binary metrics are replaced by their definitions on the confusion counts.  The inputs come
from tests/matching_train_cases.py, loaded by path; this process never imports the product.

The fixture holds results only:
* lr_<total>_<warmup ratio>: the rate in force in every epoch of two cycles, recorded by driving the reference's scheduler class the way
  Lightning does (one step() at the end of every epoch) behind configure_optimizers' arguments;
* param_names / state_names: named_parameters() and state_dict() keys of the model in order; no_decay_names / decay_names: the two lists
  of filter_wd_parameters in the order it returns them;
* val_<batch>_*: the loss_dict of the validation step in float64, the deviation of the reference's own float32 run from it (what the GPU
  test's bars are 4 x of), the assignment's columns of the float32 run, n_critical_pcs and (tp, fp, fn).
The tool asserts that the assignment is stable: the same columns after perturbing ds_mat by relative 1e-6 noise."""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[1]

import numpy as np
import torch

SCHEDULES = ((250, 0.0), (10, 0.3), (7, 0.5))          # (NUM_EPOCHS, WARMUP_RATIO); LR 1e-3 and LR_DECAY 100 as in every experiment file
LR, LR_DECAY = 1e-3, 100.0
VAL_BATCHES = ("main", "one_owner")                      # of tests/matching_train_cases.py; one_owner: a puzzle whose critical points one piece owns
LOSS_KEYS = ("cls_loss", "cls_acc", "cls_precision", "cls_recall", "cls_f1", "mat_loss", "loss", "mat_f1", "mat_precision", "mat_recall")


def _load(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class AttrDict(dict):
    """easydict.EasyDict's behaviour as far as the model and its config file use it"""

    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_fit.npz"))
    args = ap.parse_args()
    jig = Path(args.reference) / "Jigsaw_matching"
    if not jig.is_dir():
        ap.error(f"{jig}: not a directory")
    cases = _load("matching_train_cases", ROOT / "tests" / "matching_train_cases.py")
    standins = _load("make_matching_goldens", ROOT / "tools" / "make_matching_goldens.py")
    sys.meta_path.insert(0, standins._Finder())
    sys.path.insert(0, str(jig))
    assert "pfpp_hip" not in sys.modules

    import easydict
    import pytorch_lightning
    import torchmetrics

    class _Lightning(torch.nn.Module):
        device = torch.device("cpu")

        def save_hyperparameters(self, *a, **k):
            pass

    pytorch_lightning.LightningModule = _Lightning
    easydict.EasyDict = AttrDict

    def _counts(pred, gt):
        pred, gt = pred.bool(), gt.bool()
        return (pred & gt).sum().double(), (pred & ~gt).sum().double(), (~pred & ~gt).sum().double(), (~pred & gt).sum().double()

    def _safe(a, b):
        return a / b if float(b) > 0 else torch.zeros((), dtype=torch.float64)

    m4 = lambda f: (lambda p, g, task: f(*_counts(p, g)))
    torchmetrics.functional = types.SimpleNamespace(
        accuracy=m4(lambda tp, fp, tn, fn: _safe(tp + tn, tp + fp + tn + fn)), precision=m4(lambda tp, fp, tn, fn: _safe(tp, tp + fp)),
        recall=m4(lambda tp, fp, tn, fn: _safe(tp, tp + fn)), f1_score=m4(lambda tp, fp, tn, fn: _safe(2 * tp, 2 * tp + fp + fn)))

    import model.jigsaw.joint_seg_align_model as jsam_mod
    from model.jigsaw.model_config import get_model_cfg
    from utils.critical_pcs import get_critical_pcs_from_label
    from utils.linear_solvers import hungarian
    from utils.loss import permutation_loss
    from utils.lr import CosineAnnealingWarmupRestarts
    from utils.utils import filter_wd_parameters

    JSAM = jsam_mod.JointSegmentationAlignmentModel
    torch.set_num_threads(8)
    out = {}

    # ---- the learning rate of every epoch: configure_optimizers' scheduler, stepped once per epoch as Lightning's 'interval': 'epoch' does
    for total, ratio in SCHEDULES:
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=LR, weight_decay=0.0)
        sched = CosineAnnealingWarmupRestarts(opt, total, max_lr=LR, min_lr=LR / LR_DECAY, warmup_steps=int(total * ratio))
        rates = []
        for _ in range(2 * total + 1):
            rates.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        out[f"lr_{total}_{ratio}"] = np.asarray(rates, dtype=np.float64)
        print(f"schedule ({total}, {ratio}): epochs 0-3 {rates[:4]}, restart {rates[total - 1:total + 2]}")

    # ---- parameter order and the weight-decay split
    cfg = AttrDict(STATS="", DATA=AttrDict(MAX_NUM_PART=20), MODEL=get_model_cfg())
    model = JSAM(cfg)
    names = [k for k, _ in model.named_parameters()]
    by_id = {id(p): k for k, p in model.named_parameters()}
    split = filter_wd_parameters(model)
    out.update(param_names=np.asarray(names), param_shapes=np.asarray([",".join(map(str, p.shape)) for p in model.parameters()]),
               state_names=np.asarray(list(model.state_dict())), no_decay_names=np.asarray([by_id[id(p)] for p in split["no_decay"]]),
               decay_names=np.asarray([by_id[id(p)] for p in split["decay"]]))
    assert sorted(out["no_decay_names"].tolist() + out["decay_names"].tolist()) == sorted(names)
    print(f"{len(names)} parameters ({sum(p.numel() for p in model.parameters())} elements), {len(out['state_names'])} state_dict entries, "
          f"{len(split['no_decay'])} not decayed, {len(split['decay'])} decayed")

    # ---- the validation step behind part_feats
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.startswith(("encoder.", "tf_self1.", "tf_cross1.")) for k in missing.missing_keys)
    model.eval()
    model.trainer = types.SimpleNamespace(testing=False)
    jsam_mod.get_batch_length_from_part_points = lambda n_pcs, n_valids=None: torch.zeros(1)      # the only line in front of part_feats that runs

    def perm_loss(pred, gt, ns):
        """utils/loss.py:47-56 without its cast of the prediction to float32 (:38); in float32 it is the reference's, bit for bit"""
        loss = torch.zeros((), dtype=pred.dtype)
        for b in range(pred.shape[0]):
            n = int(ns[b])
            loss = loss + torch.nn.functional.binary_cross_entropy(pred[b, :n, :n], gt[b, :n, :n].to(pred.dtype), reduction="sum")
        res = loss / ns.sum().to(pred.dtype)
        if pred.dtype == torch.float32:
            assert torch.equal(res, permutation_loss(pred, gt.float(), ns, ns)), "perm_loss is not the reference's permutation_loss"
        return res

    class _Fun:
        """torch.nn.functional as the model file sees it; :301 casts the labels to float32, which the float64 run must not"""

        def __getattr__(self, name):
            return getattr(torch.nn.functional, name)

        @staticmethod
        def binary_cross_entropy_with_logits(logits, target):
            return torch.nn.functional.binary_cross_entropy_with_logits(logits, target.to(logits.dtype))

    jsam_mod.fun = _Fun()

    def val_step(batch, dtype):
        model.to(dtype)
        label, n_pcs = torch.from_numpy(batch["critical_label"]), torch.from_numpy(batch["n_pcs"])
        crit_idx, n_crit = get_critical_pcs_from_label(label, n_pcs)
        data = {"part_valids": torch.from_numpy(batch["part_valids"]), "n_pcs": n_pcs, "part_pcs": torch.from_numpy(batch["gt_pcs"]).to(dtype),
                "gt_pcs": torch.from_numpy(batch["gt_pcs"]).to(dtype), "part_feats": torch.from_numpy(batch["part_feats"]).to(dtype),
                "critical_label": label, "critical_pcs_idx": crit_idx, "n_critical_pcs": n_crit}
        seen = {}

        def capture(mat, gt_perm, ns, _):
            seen["gt_perm"] = gt_perm.detach().clone()
            return perm_loss(mat, gt_perm, ns)

        jsam_mod.permutation_loss = capture
        with torch.no_grad():
            res = JSAM.forward(model, data)
            loss_dict = JSAM._loss_function(model, data, res)
        n_sum = n_crit.sum(-1)
        tp = fp = fn = 0
        for b in range(len(n_sum)):
            n = int(n_sum[b])
            pred, gt = res["perm_mat"][b, :n, :n].double(), seen["gt_perm"][b, :n, :n].double()
            tp, fp, fn = tp + int((pred * gt).sum()), fp + int((pred * (1 - gt)).sum()), fn + int(((1 - pred) * gt).sum())
        return {"loss_dict": {k: float(loss_dict[k]) for k in LOSS_KEYS}, "N_": int(loss_dict["N_"]), "batch_size": int(loss_dict["batch_size"]),
                "ds": res["ds_mat"], "perm": res["perm_mat"], "n_crit": n_crit, "counts": (tp, fp, fn), "gt_perm": seen["gt_perm"]}

    rng = np.random.default_rng(2024)
    for name in VAL_BATCHES:
        batch = cases.make_batch(name)
        r32, r64 = val_step(batch, torch.float32), val_step(batch, torch.float64)
        n_crit = r64["n_crit"].numpy()
        assert r32["counts"] == r64["counts"], "the float32 and float64 runs of the reference disagree on the assignment's counts"
        cols, per_puzzle = [], []
        for b in range(n_crit.shape[0]):
            n = int(n_crit[b].sum())
            solved = int((n_crit[b] > 0).sum()) >= 2
            ds = r32["ds"][b, :n, :n]
            col = r32["perm"][b, :n, :n].argmax(-1).numpy()
            bce = float(torch.nn.functional.binary_cross_entropy(r64["ds"][b, :n, :n], r64["gt_perm"][b, :n, :n].double(), reduction="sum"))
            per_puzzle.append(bce)
            if solved:                                     # a tie must not decide a test: the same columns under relative 1e-6 noise
                for _ in range(4):
                    noisy = ds * torch.from_numpy(1.0 + 1e-6 * rng.uniform(-1, 1, (n, n))).float()
                    again = hungarian(noisy[None], torch.tensor([n]), torch.tensor([n]))[0].argmax(-1).numpy()
                    assert np.array_equal(again, col), f"{name} puzzle {b}: the assignment is not stable, choose other inputs"
                assert np.array_equal(col, r64["perm"][b, :n, :n].argmax(-1).numpy()), "float32 and float64 assignments differ"
            else:
                # every entry masked: s is -1e6 everywhere, the Sinkhorn output uniform, the targets all zero
                print(f"{name} puzzle {b}: {n} critical points on fewer than two pieces: ds_mat in [{float(ds.min()):.6g}, {float(ds.max()):.6g}] "
                      f"(1 / n = {1.0 / max(n, 1):.6g}), its share of the BCE sum {bce:.6g}, n (n - 1) log(n / (n - 1)) + ... = "
                      f"{-n * n * np.log1p(-1.0 / n) if n > 1 else 100.0 * n:.6g}")
            cols.append(np.where(solved, col, -1).astype(np.int64))
        out.update({f"val_{name}_{k}": np.asarray(v) for k, v in r64["loss_dict"].items()})
        out.update({f"val_{name}_N_": np.asarray(r64["N_"]), f"val_{name}_batch_size": np.asarray(r64["batch_size"]),
                    f"val_{name}_n_critical_pcs": n_crit, f"val_{name}_cols": np.concatenate(cols), f"val_{name}_counts": np.asarray(r64["counts"]),
                    f"val_{name}_puzzle_bce": np.asarray(per_puzzle)})
        for k in ("cls_loss", "mat_loss", "loss"):
            out[f"val_{name}_dev_{k}"] = np.asarray(abs(r32["loss_dict"][k] - r64["loss_dict"][k]) / abs(r64["loss_dict"][k]))
        for k in ("mat_f1", "mat_precision", "mat_recall"):
            out[f"val_{name}_dev_{k}"] = np.asarray(abs(r32["loss_dict"][k] - r64["loss_dict"][k]))
        print(f"{name}: " + ", ".join(f"{k} {v:.6g}" for k, v in r64["loss_dict"].items()) + f", counts {r64['counts']}, N' {n_crit.sum(1).tolist()}; "
              "ref fp32-fp64: " + ", ".join(f"{k[len(name) + 9:]} {float(v):.3g}" for k, v in out.items() if k.startswith(f"val_{name}_dev_")))
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
