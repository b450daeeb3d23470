"""Generate tests/golden/matching_encoder_train.npz by RUNNING THE REFERENCE's PointNet2PTMSGDynamic in .train() under autograd on the
CPU (build container only).

    python tools/make_matching_encoder_train_goldens.py --reference <checkout of the reference>

The module is imported from <reference>/Jigsaw_matching exactly as tools/make_matching_encoder_goldens.py imports it (nothing is
copied), with that tool's fps / knn / to_dense_batch stand-ins; the inputs come from tests/matching_encoder_train_cases.py.  Per case
three runs of loss = sum(out dout), loss.backward() on the same indices:
  1. float32;
  2. float64 with its own ReLU and max-pool decisions: the samples the restatement is pinned to;
  3. float64 with run 1's ReLU patterns and pool winners imposed (the module's F.relu and torch.max are given the recorded pattern):
     the float32 run's deviation from it is the reference's own rounding, free of decisions that flipped.
The fixture holds, per case and tensor (descriptors, level outputs, the 134 parameter gradients, the 66 running buffers): the
deviation of run 1 from run 3 relative to the tensor's largest magnitude, that magnitude, and samples of run 2
(matching_encoder_train_cases.sample, stored end to end per case); per layer the number of ReLU signs and pool winners that differ
between runs 1 and 2 and the number of elements.  A case above the cap of 1 differing decision per 10,000 per layer stops the tool:
its seed is changed, not the cap.  Weights and points are regenerated from seeds and never stored."""
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


def load_by_path(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Decisions:
    """what F.relu and torch.max decide inside the reference's module: recorded, or replaced by a recorded list"""

    def __init__(self):
        self.relu, self.win, self.impose, self.pos_r, self.pos_w = [], [], None, 0, 0

    def relu_fn(self, x, *a, **k):
        if self.impose is None:
            out = torch.relu(x)
            self.relu.append((out > 0).detach())
            return out
        m = self.impose.relu[self.pos_r]
        self.pos_r += 1
        self.relu.append(m)
        return x * m.to(x.dtype)

    def max_fn(self, x, dim):
        if self.impose is None:
            val, idx = torch.max(x, dim)
            self.win.append(idx.detach())
            return val, idx
        idx = self.impose.win[self.pos_w]
        self.pos_w += 1
        self.win.append(idx)
        return torch.gather(x, dim, idx.unsqueeze(dim)).squeeze(dim), idx


class _Proxy:
    """a module namespace with a few names replaced"""

    def __init__(self, real, **over):
        self.__dict__["_real"], self.__dict__["_over"] = real, over

    def __getattr__(self, name):
        over = self.__dict__["_over"]
        return over[name] if name in over else getattr(self.__dict__["_real"], name)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_encoder_train.npz"))
    args = ap.parse_args()
    jig = Path(args.reference) / "Jigsaw_matching"
    if not jig.is_dir():
        ap.error(f"{jig}: not a directory")
    ev = load_by_path("make_matching_encoder_goldens", ROOT / "tools" / "make_matching_encoder_goldens.py")      # the stand-ins and their tape
    tc = load_by_path("matching_encoder_train_cases", ROOT / "tests" / "matching_encoder_train_cases.py")
    ev.STATE.cases = tc.base
    ev.install_standins()
    assert "pfpp_hip" not in sys.modules
    pkg_dir = jig / "model" / "modules" / "encoder" / "pointnet2_pointwise"
    pkg = types.ModuleType("pn2_pointwise")
    pkg.__path__ = [str(pkg_dir)]
    sys.modules["pn2_pointwise"] = pkg
    for stem in ("pointnet2_utils", "pointnet2_dynamic_utils", "pointnet2_msg"):
        load_by_path(f"pn2_pointwise.{stem}", pkg_dir / f"{stem}.py")
    du = sys.modules["pn2_pointwise.pointnet2_dynamic_utils"]
    Encoder = sys.modules["pn2_pointwise.pointnet2_msg"].PointNet2PTMSGDynamic
    real_F, real_torch = du.F, du.torch

    torch.set_num_threads(8)
    sd_np = tc.base.encoder_state_dict()
    names = tc.layer_names()
    out = {"step": np.asarray(tc.STEP), "layers": np.asarray([n for n, _, _ in names]), "pooled": np.asarray(tc.POOLED)}

    def run(name, dtype, tape, replay, impose):
        pts, lengths, start = tc.flat_case(name)
        model = Encoder(tc.base.FEAT_IN, tc.base.FEAT_OUT)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
        model.to(dtype).train()
        dec = Decisions()
        dec.impose = impose
        du.F, du.torch = _Proxy(real_F, relu=dec.relu_fn), _Proxy(real_torch, max=dec.max_fn)
        ev.STATE.start, ev.STATE.level, ev.STATE.tape = start.T, 0, tape
        tape.rewind(replay)
        got, hooks = {}, []
        for l, nm in enumerate(("sa1", "sa2", "sa3", "sa4"), 1):
            def sa_hook(mod, a, o, l=l):
                got[f"l{l}_points"] = o[2][0].t().detach()
            hooks.append(getattr(model, nm).register_forward_hook(sa_hook))
        try:
            y = model(torch.from_numpy(pts).to(dtype), [int(n) for n in lengths])
            (y * torch.from_numpy(tc.make_dout(name, len(pts))).to(dtype)).sum().backward()
        finally:
            du.F, du.torch = real_F, real_torch
            for h in hooks:
                h.remove()
        assert len(dec.relu) == len(names) and len(dec.win) == len(tc.POOLED)
        res = {"out": y.detach(), **got, "grad": {k: p.grad for k, p in model.named_parameters()},
               "buffers": {k: v for k, v in model.state_dict().items() if "running" in k or k.endswith("num_batches_tracked")}}
        assert all(int(v) == 1 for k, v in res["buffers"].items() if k.endswith("num_batches_tracked"))
        return tc.fixture_tensors(res), dec

    for name in tc.FIXTURE_CASES:
        tape = ev.Tape()
        t32, d32 = run(name, torch.float32, tape, False, None)
        t64, d64 = run(name, torch.float64, tape, True, None)
        t64i, _ = run(name, torch.float64, tape, True, d32)
        flips = np.asarray([[int((a != b).sum()), a.numel()] for a, b in zip(d32.relu, d64.relu)], dtype=np.int64)
        winflips = np.asarray([[int((a != b).sum()), a.numel()] for a, b in zip(d32.win, d64.win)], dtype=np.int64)
        worst = max(float((flips[:, 0] / flips[:, 1]).max()), float((winflips[:, 0] / winflips[:, 1]).max()))
        print(f"{name}: worst share of differing decisions in a layer {worst:.2e} (cap {tc.FLIP_CAP:.0e})")
        if worst > tc.FLIP_CAP:
            raise SystemExit(f"{name}: above the cap — change the case's seed (matching_encoder_train_cases.POINT_SEED), not the cap")
        tensors = sorted(t64)
        mags = np.asarray([float(np.abs(t64i[k]).max()) for k in tensors])
        out[f"{name}_tensors"] = np.asarray(tensors)
        out[f"{name}_max"] = mags
        out[f"{name}_refdev"] = np.asarray([float(np.abs(t32[k] - t64i[k]).max()) for k in tensors]) / np.maximum(mags, 1e-300)
        out[f"{name}_flips"], out[f"{name}_winflips"] = flips, winflips
        for k, v in tc.pack_samples(t64).items():
            out[f"{name}_{k}"] = v
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
