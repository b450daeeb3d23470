"""Generate tests/golden/matching_head.npz by RUNNING THE REFERENCE's matcher code on the CPU (build container only).

    python tools/make_matching_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching (sys.dont_write_bytecode, nothing is copied): utils/linear_solvers.py (sinkhorn, hungarian),
utils/critical_pcs.py, model/jigsaw/affinity_layer.py (AffinityDual), model/jigsaw/joint_seg_align_model.py (_init_classifier,
_init_affinity_extractor, compute_label, diagonal_square_mask) and model/modules/matching_base_model.py
(compute_global_transformation, with get_trans_from_mat's RANSAC stubbed and _save_data captured).  Packages those files import
but which are not installed get empty stand-ins.  The matcher's top-level packages are called `model`, `utils` and `dataset`, so this
process never imports the product; the inputs come from tests/matching_cases.py (numpy only), loaded by path.

The fixture holds results only (the tests regenerate the inputs): logits, labels, critical points, a strided sample of the affinity,
row sums / column sums / a strided sample of ds_mat in float32 and float64, the assignment as one column per row, edges,
correspondences, the fracture labels, and the measured deviations that set the tests' bars."""
from __future__ import annotations

import argparse
import functools
import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys
import tempfile
import types
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[1]

import numpy as np
import torch
import torch.nn as nn

STANDINS = ("pytorch_lightning", "torchmetrics", "easydict", "open3d", "gtsam", "trimesh", "chamferdist", "wandb", "pytorch3d",
            "torch_geometric", "matplotlib")
SAMPLE = 7          # stride of the stored samples of s and ds_mat (flattened matrix)


class _Anything(types.ModuleType):
    """a module whose every attribute exists: sub-modules on import, empty classes otherwise"""

    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        value = type(name, (nn.Module,), {}) if name[:1].isupper() else (lambda *a, **k: None)
        setattr(self, name, value)
        return value


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in STANDINS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _Anything(spec.name)
        if spec.name == "pytorch_lightning":
            m.LightningModule = nn.Module
        return m

    def exec_module(self, module):
        pass


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_cases", ROOT / "tests" / "matching_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_head.npz"))
    args = ap.parse_args()
    jig = Path(args.reference) / "Jigsaw_matching"
    if not jig.is_dir():
        ap.error(f"{jig}: not a directory")
    cases = load_cases()
    sys.meta_path.insert(0, _Finder())
    sys.path.insert(0, str(jig))
    assert "pfpp_hip" not in sys.modules

    from model.jigsaw.affinity_layer import AffinityDual
    from model.jigsaw.joint_seg_align_model import JointSegmentationAlignmentModel as JSAM
    from model.modules import matching_base_model as mbm
    from utils.critical_pcs import get_critical_pcs_from_label
    from utils.estimate_transform import get_corr_from_mat
    from utils.linear_solvers import hungarian, sinkhorn

    torch.set_num_threads(8)
    fake = types.SimpleNamespace(device=torch.device("cpu"), pc_cls_method="binary", pc_feat_dim=128, aff_feat_dim=512, num_classes=2)
    fake.diagonal_square_mask = functools.partial(JSAM.diagonal_square_mask, fake)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}
    classifier, extractor, aff = JSAM._init_classifier(fake), JSAM._init_affinity_extractor(fake), AffinityDual(512)
    classifier.load_state_dict({k[len("pc_classifier."):]: v for k, v in sd.items() if k.startswith("pc_classifier.")})
    extractor.load_state_dict({k[len("affinity_extractor."):]: v for k, v in sd.items() if k.startswith("affinity_extractor.")})
    aff.load_state_dict({"A": sd["affinity_layer.A"]})
    for m in (classifier, extractor, aff):
        m.eval()

    captured = {}

    class _Saved(Exception):
        pass

    def save_data(edges, corr_list, gt_pcs, critical_pcs_idx, n_pcs, n_critical_pcs, data_id):
        captured.update(edges=edges, corr=corr_list, gt_pcs=gt_pcs, critical_pcs_idx=critical_pcs_idx, n_pcs=n_pcs,
                        n_critical_pcs=n_critical_pcs, data_id=data_id)
        raise _Saved()

    mbm.get_trans_from_mat = lambda src, tgt, mat: (np.eye(4), get_corr_from_mat(mat))        # RANSAC never reaches the file
    base = types.SimpleNamespace(_save_data=save_data)

    def head(x, n_pcs, part_valids, dtype, s_noise=None):
        """the test-time lines of JointSegmentationAlignmentModel.forward behind part_feats, driven module by module"""
        mods = [m.to(dtype) for m in (classifier, extractor, aff)]
        with torch.no_grad():
            part_feats = torch.from_numpy(x).to(dtype)[None]
            n_valid = torch.from_numpy(part_valids)[None].sum(1).to(torch.long)
            npcs = torch.from_numpy(n_pcs)[None]
            feat = part_feats.transpose(1, 2)
            logits = mods[0](feat).transpose(1, 2)
            pred = (torch.sigmoid(logits) > 0.5).to(torch.int64).reshape(1, -1)
            crit_idx, n_crit = get_critical_pcs_from_label(pred, npcs)
            n_sum = n_crit.sum(-1)
            cf = part_feats[0, pred[0] == 1][None]
            af = mods[1](cf.permute(0, 2, 1)).permute(0, 2, 1)
            af = torch.cat([nn.functional.normalize(af[:, :, :256], p=2, dim=-1), nn.functional.normalize(af[:, :, 256:], p=2, dim=-1)], -1)
            s = mods[2](af, af)
            if s_noise is not None:
                s = s + s_noise
            fake_t = types.SimpleNamespace(device=torch.device("cpu"))
            mask = JSAM.diagonal_square_mask(fake_t, s.shape, n_crit, n_part=n_valid, pos_msk=1, neg_msk=0).to(dtype)
            neg = JSAM.diagonal_square_mask(fake_t, s.shape, n_crit, n_part=n_valid, pos_msk=0, neg_msk=-1e6).to(dtype)
            ds = sinkhorn(s * mask + neg, n_sum, n_sum, max_iter=20, tau=0.05)
            perm = hungarian(ds, n_sum, n_sum)
        for m in (classifier, extractor, aff):
            m.float()
        return dict(logits=logits[0, :, 0], pred=pred[0], crit_idx=crit_idx[0], n_crit=n_crit[0], s=s[0], ds=ds[0], perm=perm[0], n_valid=n_valid)

    out = {"sample_stride": np.asarray(SAMPLE)}
    cwd = os.getcwd()
    for name in cases.CASES:
        pz = cases.make_puzzle(name)
        r32 = head(pz["part_feats"], pz["n_pcs"], pz["part_valids"], torch.float32)
        r64 = head(pz["part_feats"], pz["n_pcs"], pz["part_valids"], torch.float64)
        assert torch.equal(r32["pred"], r64["pred"]) and torch.equal(r32["pred"].bool(), torch.from_numpy(pz["critical"]))
        assert r64["logits"].abs().min() > 0.1, "a logit near the threshold"
        n = r32["ds"].shape[0]
        cols32, cols64 = r32["perm"].argmax(1), r64["perm"].argmax(1)
        assert torch.equal(cols32, cols64), "the fp32 and fp64 runs of the reference disagree on the assignment"
        rows = pz["critical"].nonzero()[0]
        built = np.searchsorted(rows, pz["partner"][rows])
        strong = r64["ds"][torch.arange(n), cols64] > 0.5
        assert np.array_equal(cols64.numpy()[strong.numpy()], built[strong.numpy()]), "a strong row is not the constructed partner"
        # sensitivity: a perturbation of s by eps changes ds_mat by how much, and does the assignment move?
        g = torch.Generator().manual_seed(1)
        sens = {}
        for eps in (1e-6, 1e-5):
            rp = head(pz["part_feats"], pz["n_pcs"], pz["part_valids"], torch.float64,
                      s_noise=eps * (2 * torch.rand(r64["s"].shape, generator=g, dtype=torch.float64) - 1))
            assert torch.equal(rp["perm"].argmax(1), cols64), "the assignment moves under a 1e-5 perturbation of s"
            sens[eps] = float((rp["ds"] - r64["ds"]).abs().max())
        # the file, through the reference's own pair rule and its writer's arguments
        with tempfile.TemporaryDirectory() as td:
            os.chdir(td)
            try:
                mbm.MatchingBaseModel.compute_global_transformation(
                    base, r32["n_crit"][None].numpy(), r32["perm"][None].numpy(), pz["gt_pcs"][None], r32["crit_idx"][None].numpy(),
                    pz["gt_pcs"][None], r32["n_valid"].numpy(), pz["n_pcs"][None], None, None, torch.tensor([pz["data_id"]]), None)
                raise AssertionError("_save_data was not reached")
            except _Saved:
                pass
            finally:
                os.chdir(cwd)
        edges = np.asarray(captured["edges"], dtype=np.int64).reshape(-1, 2)
        corr = [np.asarray(c, dtype=np.int64).reshape(-1, 2) for c in captured["corr"]]
        assert np.array_equal(captured["gt_pcs"], pz["gt_pcs"]) and np.array_equal(captured["n_pcs"], pz["n_pcs"])
        # fracture labels
        thr = torch.from_numpy(pz["thresholds"])[None]
        gt = torch.from_numpy(pz["gt_pcs"])[None]
        lab32 = JSAM.compute_label(fake, gt, torch.from_numpy(pz["n_pcs"])[None], r32["n_valid"], thr)[0]
        lab64 = JSAM.compute_label(fake, gt.double(), torch.from_numpy(pz["n_pcs"])[None], r32["n_valid"], thr.double())[0]
        ds32, ds64 = r32["ds"].numpy(), r64["ds"].numpy()
        out.update({
            f"{name}_logits": r32["logits"].numpy(), f"{name}_cls_pred": r32["pred"].numpy().astype(np.uint8),
            f"{name}_critical_pcs_idx": captured["critical_pcs_idx"].astype(np.int16), f"{name}_n_critical_pcs": captured["n_critical_pcs"],
            f"{name}_s_sample": r64["s"].numpy().reshape(-1)[::SAMPLE], f"{name}_ds_sample": ds64.reshape(-1)[::SAMPLE],
            f"{name}_ds_rowsum": ds64.sum(1), f"{name}_ds_colsum": ds64.sum(0), f"{name}_ds32_sample": ds32.reshape(-1)[::SAMPLE],
            f"{name}_ds_on_perm": ds64[np.arange(n), cols64.numpy()], f"{name}_perm": cols32.numpy().astype(np.int16),
            f"{name}_edges": edges, f"{name}_corr_cat": np.concatenate(corr).astype(np.int16) if corr else np.zeros((0, 2), np.int16),
            f"{name}_corr_len": np.asarray([len(c) for c in corr], dtype=np.int64),
            f"{name}_labels": lab32.numpy().astype(np.uint8), f"{name}_labels64": lab64.numpy().astype(np.uint8),
            f"{name}_ref_ds_dev": np.asarray(float(np.abs(ds32 - ds64).max())), f"{name}_ref_s_dev": np.asarray(float((r32["s"].double() - r64["s"]).abs().max())),
            f"{name}_sens_1e-6": np.asarray(sens[1e-6]), f"{name}_sens_1e-5": np.asarray(sens[1e-5]),
        })
        print(f"{name}: N' = {n}, edges {edges.tolist()}, corr {[len(c) for c in corr]}, strong rows {int(strong.sum())}/{n}, "
              f"ref fp32-fp64 ds {float(np.abs(ds32 - ds64).max()):.3g}, s {float((r32['s'].double() - r64['s']).abs().max()):.3g}, "
              f"sensitivity {sens[1e-6]:.3g} @1e-6 {sens[1e-5]:.3g} @1e-5, labels {int(lab32.sum())} (fp64 differs on {int((lab32 != lab64).sum())})")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
