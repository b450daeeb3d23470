"""Generate tests/golden/matching_rigid.npz by RUNNING THE REFERENCE's rigid_loss and horn_87, alone and inside the matcher's training step.

    python tools/make_matching_rigid_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching (sys.dont_write_bytecode, nothing is copied): utils/loss.py (rigid_loss, permutation_loss),
utils/pairwise_alignment.py (pairwise_alignment, horn_87) and, for the whole step, what tools/make_matching_train_goldens.py imports,
with `forward` and `_loss_function` run at w_rig_loss = 1.  The inputs come from tests/matching_rigid_cases.py, loaded by path; this
process never imports the product.

Every case runs twice, in float32 (the reference as it is) and in float64.  A float64 run needs the reference's float32 casts lifted,
or it is a float32 run (and torch.matmul at loss.py:120 raises on mixed dtypes): the two `.astype(np.float32)` of
pairwise_alignment.py:79 and the `dtype=torch.float32` of loss.py:114-119, plus loss.py:68's float32 accumulators, which `loss +=`
would otherwise round every pair into.  They are lifted by handing the two modules a `np` / `torch` whose float32 and `tensor` follow
the run's dtype; in float32 each lifted line is asserted to return the reference's result bit for bit.  The float64 run of the loss
takes the float32 run's (R, t) - the poses are constants of the loss, like the ReLU patterns of DESIGN.md 5.10 - while Horn's own
float64 poses are recorded beside them.  Per-pair mat_s and pair_loss are read off the module's torch.sum calls; the numerator and
n_sum off its two accumulators.

The fixture holds results only: poses, per-pair sums, losses, strided samples of the gradients in float64, and the reference's own
float32-against-float64 deviation per tensor (what the GPU tests' bars are 4 x of)."""
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


def rel_dev(a32, a64) -> float:
    """max |fp32 - fp64| over max |fp64|: the deviation of a tensor, relative to its largest entry"""
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    if a64.size == 0:
        return 0.0
    den = float(np.abs(a64).max())
    return float(np.abs(a32 - a64).max()) / den if den > 0 else 0.0


class TorchFor:
    """utils/loss.py's `torch` for one run: torch itself, but `tensor` builds in the run's dtype (loss.py:68, :114-119) and the scalar
    `sum` calls and the two accumulators of rigid_loss are remembered"""

    def __init__(self, dtype):
        self.dtype, self.sums, self.created, self.zeros = dtype, [], [], []

    def __getattr__(self, name):
        return getattr(torch, name)

    def tensor(self, data, dtype=None, device=None):
        res = torch.tensor(data, dtype=self.dtype, device=device)
        if self.dtype == torch.float32:                    # the lifted line is the reference's, bit for bit
            ref = torch.tensor(data, dtype=dtype, device=device)
            assert ref.dtype == res.dtype and bool(((ref == res) | (ref.isnan() & res.isnan())).all())
        self.created.append(res)
        return res

    def zeros_like(self, x, **kw):
        res = torch.zeros_like(x, **kw)
        self.zeros.append(res)
        return res

    def sum(self, x, *a, **kw):
        res = torch.sum(x, *a, **kw)
        if not a and not kw:
            self.sums.append(res.detach().clone())
        return res


class NumpyFor:
    """utils/pairwise_alignment.py's `np` for one run: numpy itself, but float32 (the casts of :79) is the run's dtype"""

    def __init__(self, f32):
        self.float32 = f32

    def __getattr__(self, name):
        return getattr(np, name)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_rigid.npz"))
    args = ap.parse_args()
    jig = Path(args.reference) / "Jigsaw_matching"
    if not jig.is_dir():
        ap.error(f"{jig}: not a directory")
    cases = _load("matching_rigid_cases", ROOT / "tests" / "matching_rigid_cases.py")
    tcases = cases._tc
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

    import model.jigsaw.joint_seg_align_model as jsam_mod
    import utils.loss
    import utils.pairwise_alignment
    from model.jigsaw.affinity_layer import AffinityDual
    from utils.critical_pcs import get_critical_pcs_from_label
    from utils.linear_solvers import Sinkhorn

    # the package re-exports a function under the sub-module's name (utils/__init__.py): take the modules themselves
    loss_mod, pa_mod = sys.modules["utils.loss"], sys.modules["utils.pairwise_alignment"]
    JSAM = jsam_mod.JointSegmentationAlignmentModel
    ref_rigid_loss, ref_alignment, ref_perm_loss = loss_mod.rigid_loss, pa_mod.pairwise_alignment, loss_mod.permutation_loss
    torch.set_num_threads(8)

    # ---- the reference's rigid_loss in one dtype, with everything the fixture needs read off it
    def run_rigid(call, dtype, poses32=None):
        """call(rigid_loss): runs code that calls the given rigid_loss exactly once.  -> the call's result and a record: the poses
        pairwise_alignment returned (float32 run) or Horn's own float64 poses (float64 run, which hands poses32 on), per call mat_s
        and pair_loss, the numerator and n_sum"""
        tp = TorchFor(dtype)
        rec = {"R": [], "t": [], "pos": [], "shape": []}

        def alignment(S, T, W, method="horn87"):
            rec["pos"].append(len(tp.sums)); rec["shape"].append((S.shape[0], T.shape[0]))
            with np.errstate(invalid="ignore", divide="ignore"):
                if dtype == torch.float32:
                    R, t = ref_alignment(S, T, W, method)
                    pa_mod.np = NumpyFor(np.float32)
                    R2, t2 = ref_alignment(S, T, W, method)            # the lifted casts are the reference's, bit for bit
                    pa_mod.np = np
                    assert R.dtype == R2.dtype == np.float32 and np.array_equal(R, R2, equal_nan=True) and np.array_equal(t, t2, equal_nan=True)
                    rec["R"].append(R); rec["t"].append(t)
                    return R, t
                assert S.dtype == T.dtype == W.dtype == np.float64
                pa_mod.np = NumpyFor(np.float64)
                R, t = ref_alignment(S, T, W, method)
                pa_mod.np = np
                assert R.dtype == np.float64
                rec["R"].append(R); rec["t"].append(t)
                k = len(rec["R"]) - 1
                return poses32[0][k].astype(np.float64), poses32[1][k].astype(np.float64)

        def entry(*a):                                     # what loss.py's torch saw before rigid_loss began is not the term's
            tp.sums.clear(); tp.created.clear(); tp.zeros.clear()
            return ref_rigid_loss(*a)

        loss_mod.torch, loss_mod.pairwise_alignment = tp, alignment
        try:
            res = call(entry)
        finally:
            loss_mod.torch, loss_mod.pairwise_alignment = torch, ref_alignment
        k = len(rec["R"])
        assert len(tp.created) >= 1 and len(tp.zeros) == 1
        rec.update(R=np.asarray(rec["R"]).reshape(k, 3, 3), t=np.asarray(rec["t"]).reshape(k, 3),
                   mat_s=np.asarray([float(tp.sums[p - 2]) + float(tp.sums[p - 1]) for p in rec["pos"]]),
                   pair_loss=np.asarray([float(tp.sums[p]) for p in rec["pos"]]),
                   numerator=float(tp.created[0].detach()), n_sum=float(tp.zeros[0]))
        return res, rec

    def record(out, key, r32, r64, rec32, rec64, ref):
        """r32 / r64: dicts of the two runs' tensors (rig_loss, dP list, ...); rec*: run_rigid's records; ref: the restatement"""
        called = ref["status"] != 0
        assert int(called.sum()) == len(rec32["shape"]) == len(rec64["shape"]), (key, "the restatement and the reference disagree on the skipped pairs")
        cnt = [(ref["counts"][b][p], ref["counts"][b][q]) for (b, p, q), c in zip(ref["pairs"], called) if c]
        assert cnt == rec32["shape"] == rec64["shape"], key
        assert rec32["n_sum"] == rec64["n_sum"]
        finite = bool(np.isfinite(r64["rig_loss"]))
        assert finite == bool(np.isfinite(r32["rig_loss"]))
        gaps = ref["gap"][ref["status"] == 1]
        firm = ref["gap"][called] >= GAP_MIN                       # poses are compared where the eigenvector is well determined
        out.update({f"{key}_pairs": np.asarray(ref["pairs"], dtype=np.int32).reshape(-1, 3), f"{key}_called": called.astype(np.int32),
                    f"{key}_finite": np.asarray(int(finite)), f"{key}_n_sum": np.asarray(rec64["n_sum"]), f"{key}_numerator": np.asarray(rec64["numerator"]),
                    f"{key}_rig_loss": np.asarray(r64["rig_loss"]), f"{key}_R32": rec32["R"], f"{key}_t32": rec32["t"], f"{key}_R64": rec64["R"],
                    f"{key}_t64": rec64["t"], f"{key}_mat_s": rec64["mat_s"], f"{key}_pair_loss": rec64["pair_loss"]})
        if finite:
            out.update({f"{key}_dev_rig_loss": np.asarray(abs(r32["rig_loss"] - r64["rig_loss"]) / abs(r64["rig_loss"])),
                        f"{key}_dev_mat_s": np.asarray(rel_dev(rec32["mat_s"], rec64["mat_s"])),
                        f"{key}_dev_pair_loss": np.asarray(rel_dev(rec32["pair_loss"], rec64["pair_loss"])),
                        f"{key}_dev_R": np.asarray(float(np.abs(rec32["R"] - rec64["R"])[firm].max(initial=0.0))),
                        f"{key}_dev_t": np.asarray(float((np.abs(rec32["t"] - rec64["t"]) / np.maximum(np.abs(rec64["t"]), 1))[firm].max(initial=0.0)))})
        return finite, gaps

    out = {"sample_stride": np.asarray(cases.SAMPLE)}
    S, GAP_MIN = cases.SAMPLE, cases.GAP_MIN
    # ---- rigid_loss alone, on given matrices: every point of the made-up puzzles is a critical point
    outside = total = 0
    for name in cases.KERNEL_CASES:
        kc = cases.kernel_case(name)
        B = len(kc["ds_mat"])
        n_max, P = max(m.shape[0] for m in kc["ds_mat"]), max(kc["n_valid"])
        ref = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"])
        ref["counts"] = kc["counts"]
        runs, recs = {}, {}
        for dtype in (torch.float32, torch.float64):
            mat = torch.zeros(B, n_max, n_max, dtype=dtype)
            part = torch.zeros(B, n_max, 3, dtype=dtype)
            n_pcs, idx = torch.zeros(B, P, dtype=torch.int64), torch.zeros(B, n_max, dtype=torch.int64)
            for b in range(B):
                n = kc["ds_mat"][b].shape[0]
                mat[b, :n, :n] = torch.from_numpy(kc["ds_mat"][b]).to(dtype)
                part[b, :n] = torch.from_numpy(kc["pts"][b]).to(dtype)
                n_pcs[b, :len(kc["counts"][b])] = torch.tensor(kc["counts"][b])
                idx[b, :n] = torch.cat([torch.arange(c) for c in kc["counts"][b]])
            mat.requires_grad_(True)
            call = lambda rigid_loss: rigid_loss(n_pcs, mat, part, idx, part, torch.tensor(kc["n_valid"]), n_pcs)
            loss, recs[dtype] = run_rigid(call, dtype, None if dtype == torch.float32 else (recs[torch.float32]["R"], recs[torch.float32]["t"]))
            assert loss.dtype == dtype
            if bool(torch.isfinite(loss)):
                loss.backward()
            grad = mat.grad if mat.grad is not None else torch.zeros_like(mat)
            runs[dtype] = {"rig_loss": float(loss.detach()), "dP": [grad[b, :m.shape[0], :m.shape[0]].double().numpy() for b, m in enumerate(kc["ds_mat"])]}
        r32, r64 = runs[torch.float32], runs[torch.float64]
        finite, gaps = record(out, name, r32, r64, recs[torch.float32], recs[torch.float64], ref)
        outside += int((gaps < cases.GAP_MIN).sum()); total += gaps.size
        line = f"{name}: {len(ref['pairs'])} pairs, {int((ref['status'] == 1).sum())} kept, n_sum {ref['n_sum']}, rig_loss {r64['rig_loss']:.6g}"
        if finite:
            g32, g64 = np.concatenate([g.reshape(-1) for g in r32["dP"]]), np.concatenate([g.reshape(-1) for g in r64["dP"]])
            out.update({f"{name}_dP_sample": g64[::S], f"{name}_dP_max": np.asarray(float(np.abs(g64).max())), f"{name}_dev_dP": np.asarray(rel_dev(g32, g64))})
            devs = {k[len(name) + 5:]: float(v) for k, v in out.items() if k.startswith(f"{name}_dev_")}
            line += f", gap {gaps.min():.3g} - {gaps.max():.3g}, ref fp32-fp64: " + ", ".join(f"{k} {v:.2g}" for k, v in devs.items())
        print(line)
    print(f"kernel-level cases: {outside} of {total} kept pairs have an eigen-gap below {cases.GAP_MIN} (the pieces of 1 or 2 points)")

    # ---- the whole step at w_rig_loss = 1 (the harness of tools/make_matching_train_goldens.py)
    sd_np = cases.head_state_dict()

    def perm_loss(pred, gt, ns):
        """utils/loss.py:47-56 without its cast of the prediction to float32 (:38); in float32 it must return the reference's value"""
        loss = torch.zeros((), dtype=pred.dtype)
        for b in range(pred.shape[0]):
            n = int(ns[b])
            loss = loss + torch.nn.functional.binary_cross_entropy(pred[b, :n, :n], gt[b, :n, :n].to(pred.dtype), reduction="sum")
        res = loss / ns.sum().to(pred.dtype)
        if pred.dtype == torch.float32:
            assert torch.equal(res.detach(), ref_perm_loss(pred.detach(), gt.float(), ns, ns)), "perm_loss is not the reference's permutation_loss"
        return res

    def build(dtype):
        fake = types.SimpleNamespace(device=torch.device("cpu"), pc_cls_method="binary", pc_feat_dim=128, aff_feat_dim=512, half_aff_feat_dim=256,
                                     num_classes=2, training=True, w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=1.0,
                                     trainer=types.SimpleNamespace(testing=False), tf_layers=[],
                                     cfg=types.SimpleNamespace(MODEL=types.SimpleNamespace(TEST_S_MASK=True)))
        fake.pc_classifier, fake.affinity_extractor, fake.affinity_layer = JSAM._init_classifier(fake), JSAM._init_affinity_extractor(fake), AffinityDual(512)
        fake.sinkhorn = Sinkhorn(max_iter=tcases.MAX_ITER, tau=tcases.TAU)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}
        fake.pc_classifier.load_state_dict({k[len("pc_classifier."):]: v for k, v in sd.items() if k.startswith("pc_classifier.")})
        fake.affinity_extractor.load_state_dict({k[len("affinity_extractor."):]: v for k, v in sd.items() if k.startswith("affinity_extractor.")})
        fake.affinity_layer.load_state_dict({"A": sd["affinity_layer.A"]})
        for m in (fake.pc_classifier, fake.affinity_extractor, fake.affinity_layer):
            m.to(dtype).train()
        for fn in ("_get_critical_feats_BNF_from_label", "diagonal_square_mask", "compute_label"):
            setattr(fake, fn, functools.partial(getattr(JSAM, fn), fake))
        return fake

    class _Fun:
        """torch.nn.functional as the model file sees it, the labels of :301 in the logits' dtype (the same thing in float32)"""

        def __getattr__(self, name):
            return getattr(torch.nn.functional, name)

        @staticmethod
        def binary_cross_entropy_with_logits(logits, target):
            res = torch.nn.functional.binary_cross_entropy_with_logits(logits, target.to(logits.dtype))
            if logits.dtype == torch.float32:
                assert target.dtype == torch.float32 and torch.equal(res.detach(), torch.nn.functional.binary_cross_entropy_with_logits(logits.detach(), target))
            return res

    jsam_mod.get_batch_length_from_part_points = lambda n_pcs, n_valids=None: torch.zeros(1)
    jsam_mod.permutation_loss = lambda mat, gt_perm, ns, _: perm_loss(mat, gt_perm, ns)
    jsam_mod.fun = _Fun()

    def step(batch, part_pcs, dtype, poses32):
        fake = build(dtype)
        part_feats = torch.from_numpy(batch["part_feats"]).to(dtype).requires_grad_(True)
        label = torch.from_numpy(batch["critical_label"])
        n_pcs = torch.from_numpy(batch["n_pcs"])
        crit_idx, n_crit = get_critical_pcs_from_label(label, n_pcs)
        data = {"part_valids": torch.from_numpy(batch["part_valids"]), "n_pcs": n_pcs, "part_pcs": torch.from_numpy(part_pcs).to(dtype),
                "gt_pcs": torch.from_numpy(batch["gt_pcs"]).to(dtype), "part_feats": part_feats, "critical_label": label,
                "critical_pcs_idx": crit_idx, "n_critical_pcs": n_crit}
        seen = {}

        def call(rigid_loss):
            jsam_mod.rigid_loss = rigid_loss
            fwd = JSAM.forward(fake, data)
            seen["ds"] = fwd["ds_mat"]
            seen["ds"].retain_grad()
            return JSAM._loss_function(fake, data, fwd)

        loss_dict, rec = run_rigid(call, dtype, poses32)
        # d rig_loss / d ds_mat on its own, before the whole loss's backward
        (g_ds,) = torch.autograd.grad(loss_dict["rig_loss"], seen["ds"], retain_graph=True)
        loss_dict["loss"].backward()
        named = {}
        for prefix, mod in (("pc_classifier", fake.pc_classifier), ("affinity_extractor", fake.affinity_extractor), ("affinity_layer", fake.affinity_layer)):
            for k, v in mod.named_parameters():
                named[f"{prefix}.{k}"] = v.grad.detach().reshape(-1)
            for k, v in mod.named_buffers():
                named[f"buf:{prefix}.{k}"] = v.detach().clone()
        n_sum = n_crit.sum(-1).numpy()
        res = {k: float(loss_dict[k].detach()) for k in ("loss", "cls_loss", "mat_loss", "rig_loss")}
        res.update(grads=named, d_part_feats=part_feats.grad.detach().reshape(-1), n_crit=n_sum,
                   ds=[seen["ds"].detach()[b, :n, :n].double().numpy() for b, n in enumerate(n_sum)],
                   dP=[g_ds[b, :n, :n].double().numpy() for b, n in enumerate(n_sum)])
        return res, rec

    for name in cases.BATCHES:
        batch = cases.make_batch(name)
        part_pcs = cases.make_part_pcs(batch)
        r32, rec32 = step(batch, part_pcs, torch.float32, None)
        r64, rec64 = step(batch, part_pcs, torch.float64, (rec32["R"], rec32["t"]))
        ri = cases.batch_rigid_inputs(batch)
        pts = [part_pcs[b][ri["labels"][b]] for b in range(part_pcs.shape[0])]
        ref = cases.rigid_reference(r64["ds"], pts, ri["counts"], ri["n_valid"], poses=None)
        ref["counts"] = ri["counts"]
        key = f"step_{name}"
        finite, gaps = record(out, key, r32, r64, rec32, rec64, ref)
        assert finite and gaps.size and float(gaps.min()) >= cases.GAP_MIN, (key, gaps)
        assert max(float(d.max()) for d in r64["ds"] if d.size) <= tcases.DS_MAX
        for k in ("loss", "cls_loss", "mat_loss"):
            out[f"{key}_{k}"] = np.asarray(r64[k])
            out[f"{key}_dev_{k}"] = np.asarray(abs(r32[k] - r64[k]) / abs(r64[k]))
        g32, g64 = np.concatenate([g.reshape(-1) for g in r32["dP"]]), np.concatenate([g.reshape(-1) for g in r64["dP"]])
        out.update({f"{key}_dP_sample": g64[::S], f"{key}_dP_max": np.asarray(float(np.abs(g64).max())), f"{key}_dev_dP": np.asarray(rel_dev(g32, g64)),
                    f"{key}_ds_sample": np.concatenate([d.reshape(-1) for d in r64["ds"]])[::S],
                    f"{key}_d_part_feats_sample": r64["d_part_feats"][::S].numpy(), f"{key}_d_part_feats_max": np.asarray(float(r64["d_part_feats"].abs().max())),
                    f"{key}_dev_d_part_feats": np.asarray(rel_dev(r32["d_part_feats"].numpy(), r64["d_part_feats"].numpy()))})
        for k, g64_ in r64["grads"].items():
            g32_ = r32["grads"][k]
            if k.startswith("buf:"):
                out[f"{key}_{k[4:]}"] = g64_.numpy()
                if g64_.dtype.is_floating_point:
                    out[f"{key}_dev_{k[4:]}"] = np.asarray(rel_dev(g32_.numpy(), g64_.numpy()))
            else:
                out[f"{key}_grad_{k}_sample"] = g64_[::S].numpy()
                out[f"{key}_grad_{k}_max"] = np.asarray(float(g64_.abs().max()))
                out[f"{key}_dev_grad_{k}"] = np.asarray(rel_dev(g32_.numpy(), g64_.numpy()))
        devs = {k[len(key) + 5:]: float(v) for k, v in out.items() if k.startswith(f"{key}_dev_")}
        print(f"{key}: loss {r64['loss']:.6g} (cls {r64['cls_loss']:.6g}, mat {r64['mat_loss']:.6g}, rig {r64['rig_loss']:.6g}), {int((ref['status'] == 1).sum())} pairs "
              f"kept, n_sum {ref['n_sum']}, gap {gaps.min():.3g} - {gaps.max():.3g}, ref fp32-fp64: " + ", ".join(f"{k} {v:.2g}" for k, v in devs.items()))
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
