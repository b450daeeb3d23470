"""Generate tests/golden/matching_train.npz by RUNNING THE REFERENCE's matcher code in .train() under autograd on the CPU.

    python tools/make_matching_train_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching (sys.dont_write_bytecode, nothing is copied): utils/linear_solvers.py (sinkhorn),
utils/loss.py (permutation_loss), utils/pc_utils.py (square_distance), utils/critical_pcs.py, model/jigsaw/affinity_layer.py
(AffinityDual) and model/jigsaw/joint_seg_align_model.py (_init_classifier, _init_affinity_extractor,
_get_critical_feats_BNF_from_label, diagonal_square_mask, forward's lines behind part_feats through the module's own `forward`, and
_loss_function itself).  Packages those files import but which are not installed get the stand-ins of tools/make_matching_goldens.py;
torchmetrics' four binary metrics are replaced by their definitions on the confusion counts.  The inputs come from
tests/matching_train_cases.py, loaded by path; this process never imports the product.

The fixture holds results only: losses, confusion counts, targets, strided samples of every gradient in float64, the updated
running statistics, and the reference's own fp32-against-fp64 deviation per tensor (what the GPU tests' bars are 4 x of)."""
from __future__ import annotations

import argparse
import functools
import importlib.util
import os
import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[1]

import numpy as np
import torch


def _load(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel_dev(a32: torch.Tensor, a64: torch.Tensor) -> float:
    """max |fp32 - fp64| over max |fp64|: the deviation of a tensor, relative to its largest entry"""
    den = float(a64.abs().max())
    return float((a32.double() - a64).abs().max()) / den if den > 0 else 0.0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_train.npz"))
    args = ap.parse_args()
    jig = Path(args.reference) / "Jigsaw_matching"
    if not jig.is_dir():
        ap.error(f"{jig}: not a directory")
    cases = _load("matching_train_cases", ROOT / "tests" / "matching_train_cases.py")
    standins = _load("make_matching_goldens", ROOT / "tools" / "make_matching_goldens.py")
    sys.meta_path.insert(0, standins._Finder())
    sys.path.insert(0, str(jig))
    assert "pfpp_hip" not in sys.modules

    import torchmetrics                                                # the stand-in: give it the four metrics _loss_function calls

    def _counts(pred, gt):
        pred, gt = pred.bool(), gt.bool()
        return (pred & gt).sum().double(), (pred & ~gt).sum().double(), (~pred & ~gt).sum().double(), (~pred & gt).sum().double()

    def _safe(a, b):
        return a / b if float(b) > 0 else torch.zeros((), dtype=torch.float64)

    m4 = lambda f: (lambda p, g, task: f(*_counts(p, g)))
    torchmetrics.functional = types.SimpleNamespace(
        accuracy=m4(lambda tp, fp, tn, fn: _safe(tp + tn, tp + fp + tn + fn)), precision=m4(lambda tp, fp, tn, fn: _safe(tp, tp + fp)),
        recall=m4(lambda tp, fp, tn, fn: _safe(tp, tp + fn)), f1_score=m4(lambda tp, fp, tn, fn: _safe(2 * tp, 2 * tp + fp + fn)))

    from model.jigsaw.affinity_layer import AffinityDual
    from model.jigsaw.joint_seg_align_model import JointSegmentationAlignmentModel as JSAM
    from utils.critical_pcs import get_critical_pcs_from_label
    from utils.linear_solvers import Sinkhorn, sinkhorn
    from utils.loss import permutation_loss

    torch.set_num_threads(8)
    sd_np = cases.head_state_dict()

    def perm_loss(pred, gt, ns):
        """utils/loss.py:47-56 without its cast of the prediction to float32 (:38), which would make the float64 run a float32 one;
        in float32 it must return what the reference's permutation_loss returns, bit for bit"""
        loss = torch.zeros((), dtype=pred.dtype)
        for b in range(pred.shape[0]):
            n = int(ns[b])
            loss = loss + torch.nn.functional.binary_cross_entropy(pred[b, :n, :n], gt[b, :n, :n].to(pred.dtype), reduction="sum")
        out = loss / ns.sum().to(pred.dtype)
        if pred.dtype == torch.float32:
            assert torch.equal(out.detach(), permutation_loss(pred.detach(), gt.float(), ns, ns)), "perm_loss is not the reference's permutation_loss"
        return out

    def build(dtype, w_cls, w_mat):
        """a JointSegmentationAlignmentModel without its __init__ (no encoder, no Lightning): the attributes forward's lines behind
        part_feats and _loss_function read, the three head modules from the reference's own constructors, in .train()"""
        fake = types.SimpleNamespace(device=torch.device("cpu"), pc_cls_method="binary", pc_feat_dim=128, aff_feat_dim=512, half_aff_feat_dim=256,
                                     num_classes=2, training=True, w_cls_loss=w_cls, w_mat_loss=w_mat, w_rig_loss=0.0,
                                     trainer=types.SimpleNamespace(testing=False), tf_layers=[],
                                     cfg=types.SimpleNamespace(MODEL=types.SimpleNamespace(TEST_S_MASK=True)))
        fake.pc_classifier, fake.affinity_extractor, fake.affinity_layer = JSAM._init_classifier(fake), JSAM._init_affinity_extractor(fake), AffinityDual(512)
        fake.sinkhorn = Sinkhorn(max_iter=cases.MAX_ITER, tau=cases.TAU)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}
        fake.pc_classifier.load_state_dict({k[len("pc_classifier."):]: v for k, v in sd.items() if k.startswith("pc_classifier.")})
        fake.affinity_extractor.load_state_dict({k[len("affinity_extractor."):]: v for k, v in sd.items() if k.startswith("affinity_extractor.")})
        fake.affinity_layer.load_state_dict({"A": sd["affinity_layer.A"]})
        for m in (fake.pc_classifier, fake.affinity_extractor, fake.affinity_layer):
            m.to(dtype).train()
        for fn in ("_get_critical_feats_BNF_from_label", "diagonal_square_mask", "compute_label"):
            setattr(fake, fn, functools.partial(getattr(JSAM, fn), fake))
        return fake

    def step(batch, dtype, w_cls=1.0, w_mat=1.0):
        fake = build(dtype, w_cls, w_mat)
        part_feats = torch.from_numpy(batch["part_feats"]).to(dtype).requires_grad_(True)
        label = torch.from_numpy(batch["critical_label"])
        n_pcs = torch.from_numpy(batch["n_pcs"])
        crit_idx, n_crit = get_critical_pcs_from_label(label, n_pcs)
        data = {"part_valids": torch.from_numpy(batch["part_valids"]), "n_pcs": n_pcs, "part_pcs": torch.from_numpy(batch["gt_pcs"]).to(dtype),
                "gt_pcs": torch.from_numpy(batch["gt_pcs"]).to(dtype), "part_feats": part_feats, "critical_label": label,
                "critical_pcs_idx": crit_idx, "n_critical_pcs": n_crit}
        # utils.get_batch_length_from_part_points is the only line of forward in front of part_feats that runs: a stand-in namespace
        import model.jigsaw.joint_seg_align_model as jsam_mod

        jsam_mod.get_batch_length_from_part_points = lambda n_pcs, n_valids=None: torch.zeros(1)
        seen = {}

        def capture(mat, gt_perm, ns, _):
            seen["gt_perm"] = gt_perm.detach().clone()
            return perm_loss(mat, gt_perm, ns)

        jsam_mod.permutation_loss = capture

        class _Fun:
            """torch.nn.functional as the model file sees it, with one change: :301 casts the labels to float32, which makes the
            float64 run's classifier loss a float32 number; the labels take the logits' dtype instead (the same thing in float32)"""

            def __getattr__(self, name):
                return getattr(torch.nn.functional, name)

            @staticmethod
            def binary_cross_entropy_with_logits(logits, target):
                res = torch.nn.functional.binary_cross_entropy_with_logits(logits, target.to(logits.dtype))
                if logits.dtype == torch.float32:       # in float32 the lifted line is the reference's, bit for bit
                    assert target.dtype == torch.float32 and torch.equal(res.detach(), torch.nn.functional.binary_cross_entropy_with_logits(logits.detach(), target))
                return res

        jsam_mod.fun = _Fun()
        out = JSAM.forward(fake, data)
        loss_dict = JSAM._loss_function(fake, data, out)
        loss_dict["loss"].backward()
        named = {}
        for prefix, mod in (("pc_classifier", fake.pc_classifier), ("affinity_extractor", fake.affinity_extractor), ("affinity_layer", fake.affinity_layer)):
            for k, v in mod.named_parameters():
                named[f"{prefix}.{k}"] = None if v.grad is None else v.grad.detach().reshape(-1)
            for k, v in mod.named_buffers():
                named[f"buf:{prefix}.{k}"] = v.detach().clone()
        res = {"loss": loss_dict["loss"].detach(), "cls_loss": loss_dict["cls_loss"].detach(), "grads": named,
               "d_part_feats": part_feats.grad.detach().reshape(-1),
               "metrics": [float(loss_dict[k]) for k in ("cls_acc", "cls_precision", "cls_recall", "cls_f1")], "logits": out["cls_logits"].detach().reshape(-1)}
        if w_mat != 0:
            gp = seen["gt_perm"]
            assert ((gp == 0) | (gp == 1)).all() and (gp.sum(-1) <= 1).all()
            res.update(mat_loss=loss_dict["mat_loss"].detach(), N_=int(loss_dict["N_"]), ds=out["ds_mat"].detach(), n_sum=n_crit.sum(-1),
                       tgt=torch.where(gp.sum(-1) > 0, gp.argmax(-1), torch.full(gp.shape[:2], -1)))
        return res

    out = {"sample_stride": np.asarray(cases.SAMPLE)}
    S = cases.SAMPLE
    # ---- Sinkhorn + permutation loss alone, on given matrices and targets
    for n in cases.SINKHORN_SIZES:
        s_np, tgt = cases.sinkhorn_case(n)
        gt = torch.zeros(1, n, n, dtype=torch.float64)
        rows = np.nonzero(tgt >= 0)[0]
        gt[0, rows, tgt[rows]] = 1
        ns = torch.tensor([n])
        for it in cases.SINKHORN_ITERS:
            r = {}
            for dtype in (torch.float32, torch.float64):
                s = torch.from_numpy(s_np).to(dtype)[None].requires_grad_(True)
                ds = sinkhorn(s, ns, ns, max_iter=it, tau=cases.TAU)
                loss = perm_loss(ds, gt, ns) * n                                # the sum: permutation_loss divides by n
                loss.backward()
                rows_l = torch.nn.functional.binary_cross_entropy(ds.detach()[0], gt[0].to(dtype), reduction="none").sum(1)
                r[dtype] = (ds.detach()[0], loss.detach().double(), s.grad[0], rows_l.double())
            (p32, l32, g32, w32), (p64, l64, g64, w64) = r[torch.float32], r[torch.float64]
            assert abs(float(w64.sum()) - float(l64)) <= 1e-12 * float(l64)
            out.update({f"sk_n{n}_t{it}_row_loss": w64.numpy(), f"sk_n{n}_t{it}_dev_row_loss": np.asarray(rel_dev(w32, w64))})
            assert float(p64.max()) <= cases.DS_MAX, (n, it, float(p64.max()))
            key = f"sk_n{n}_t{it}"
            sn = cases.SINKHORN_SAMPLE[n]
            out.update({f"{key}_loss": l64.numpy(), f"{key}_ds_sample": p64.reshape(-1)[::sn].numpy(), f"{key}_grad_sample": g64.reshape(-1)[::sn].numpy(),
                        f"{key}_grad_max": np.asarray(float(g64.abs().max())),
                        f"{key}_dev_ds": np.asarray(float((p32.double() - p64).abs().max())), f"{key}_dev_loss": np.asarray(abs(float(l32) - float(l64)) / abs(float(l64))),
                        f"{key}_dev_grad": np.asarray(rel_dev(g32, g64))})
            print(f"{key}: max ds {float(p64.max()):.3f}, loss {float(l64):.6g}, ref fp32-fp64: ds {out[key + '_dev_ds']:.3g}, loss {out[key + '_dev_loss']:.3g}, "
                  f"row losses / max {out[key + '_dev_row_loss']:.3g}, "
                  f"grad / max {out[key + '_dev_grad']:.3g}")
    # ---- the whole step
    for name in list(cases.BATCHES) + ["nolabel"]:
        batch = cases.make_batch(name) if name != "nolabel" else cases.make_batch_without_critical_points()
        for tag, w_mat in (("", 1.0), ("_phase0", 0.0)):
            if (tag and name not in ("main", "nolabel")) or (not tag and name == "nolabel"):      # nolabel: the classifier phase alone is defined
                continue
            r32, r64 = step(batch, torch.float32, 1.0, w_mat), step(batch, torch.float64, 1.0, w_mat)
            key = name + tag
            out.update({f"{key}_loss": r64["loss"].numpy(), f"{key}_cls_loss": r64["cls_loss"].numpy(), f"{key}_metrics": np.asarray(r64["metrics"]),
                        f"{key}_dev_loss": np.asarray(abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"]))),
                        f"{key}_d_part_feats_sample": r64["d_part_feats"][::S].numpy(), f"{key}_dev_d_part_feats": np.asarray(rel_dev(r32["d_part_feats"], r64["d_part_feats"])),
                        f"{key}_logit_min_abs": np.asarray(float(r64["logits"].abs().min()))})
            assert r32["metrics"] == r64["metrics"], "the fp32 and fp64 runs of the reference disagree on a predicted label"
            for k, g64 in r64["grads"].items():
                g32 = r32["grads"][k]
                if k.startswith("buf:"):
                    out[f"{key}_{k[4:]}"] = g64.numpy()
                    if g64.dtype.is_floating_point:
                        out[f"{key}_dev_{k[4:]}"] = np.asarray(rel_dev(g32, g64))
                elif g64 is None:
                    out[f"{key}_nograd_{k}"] = np.asarray(1)
                else:
                    out[f"{key}_grad_{k}_sample"] = g64[::S].numpy()
                    out[f"{key}_grad_{k}_max"] = np.asarray(float(g64.abs().max()))
                    out[f"{key}_dev_grad_{k}"] = np.asarray(rel_dev(g32, g64))
            line = f"{key}: loss {float(r64['loss']):.6g} (cls {float(r64['cls_loss']):.6g}"
            if w_mat:
                n_sum = r64["n_sum"].numpy()
                ds_max = max((float(r64["ds"][b, :n, :n].max()) for b, n in enumerate(n_sum) if n), default=0.0)
                assert ds_max <= cases.DS_MAX, (key, ds_max)
                assert torch.equal(r32["tgt"], r64["tgt"]), "the fp32 and fp64 runs of the reference disagree on a target"
                out.update({f"{key}_mat_loss": r64["mat_loss"].numpy(), f"{key}_N_": np.asarray(r64["N_"]), f"{key}_n_sum": n_sum,
                            f"{key}_targets": np.concatenate([r64["tgt"][b, :n].numpy() for b, n in enumerate(n_sum)]).astype(np.int32),
                            f"{key}_ds_sample": np.concatenate([r64["ds"][b, :n, :n].reshape(-1)[::S].numpy() for b, n in enumerate(n_sum)]),
                            f"{key}_dev_mat_loss": np.asarray(abs(float(r32["mat_loss"]) - float(r64["mat_loss"])) / max(abs(float(r64["mat_loss"])), 1e-300))})
                line += f", mat {float(r64['mat_loss']):.6g}), N' {n_sum.tolist()}, max ds {ds_max:.3f}"
            devs = {k[len(key) + 5:]: float(v) for k, v in out.items() if k.startswith(f"{key}_dev_")}
            print(line + ", ref fp32-fp64: " + ", ".join(f"{k} {v:.2g}" for k, v in devs.items()))
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
