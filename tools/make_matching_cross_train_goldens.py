"""Generate tests/golden/matching_cross_train.npz by RUNNING THE REFERENCE's CrossAttentionLayer in .train() under autograd on the CPU
(build container only).

    python tools/make_matching_cross_train_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching by path (sys.dont_write_bytecode, nothing is copied): model/jigsaw/attention_layer.py, with
the torch_geometric stand-ins of tools/make_matching_transformer_goldens.py so that the file imports (the cross-attention layer calls
neither).  Inputs and weights come from tests/matching_cross_train_cases.py, loaded by path; this process never imports the product.

Per case (`tiny`, `pair`) the layer runs per puzzle as B = 1 in float32 and in float64 with loss = sum(out * dout); the parameter
gradients are summed over the puzzles.  The fixture holds results only:
  * per tensor (dx and the 12 parameter gradients) the reference's float32-against-float64 deviation over the tensor's largest
    magnitude, and that magnitude;
  * the number of ReLU sign patterns (:91) that differ between the two runs and the smallest float64 |pre-activation|;
  * of the float64 gradients: the vectors in full; of the matrices and dx the float64 row sums, column sums and every 8th row."""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[1]

import numpy as np
import torch


def load(stem: str, path: Path):
    spec = importlib.util.spec_from_file_location(stem, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(layer, x, puzzle_points, dout, dtype) -> dict:
    """the reference's layer per puzzle under autograd -> float64 numpy: dx, the summed parameter gradients, pre (input of the ReLU)"""
    layer.to(dtype)
    layer.zero_grad(set_to_none=True)
    pre, dx, lo = [], [], 0
    hook = layer.pos_ffn.w_1.register_forward_hook(lambda m, a, out: pre.append(out.detach()[0].double().numpy()))
    for n in puzzle_points:                                       # the reference takes puzzles of one size per call: one call each
        xb = torch.from_numpy(x[lo:lo + n]).to(dtype)[None].requires_grad_(True)
        out = layer(xb)
        (out * torch.from_numpy(dout[lo:lo + n]).to(dtype)[None]).sum().backward()         # .grad of the parameters accumulates
        dx.append(xb.grad[0].double().numpy())
        lo += n
    hook.remove()
    got = {"dx": np.concatenate(dx), "pre": np.concatenate(pre)}
    got.update({k: p.grad.double().numpy().copy() for k, p in layer.named_parameters()})
    layer.zero_grad(set_to_none=True)
    layer.float()
    return got


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_cross_train.npz"))
    args = ap.parse_args()
    src = Path(args.reference) / "Jigsaw_matching" / "model" / "jigsaw" / "attention_layer.py"
    if not src.is_file():
        ap.error(f"{src}: no such file")
    cases = load("matching_cross_train_cases", ROOT / "tests" / "matching_cross_train_cases.py")
    load("make_matching_transformer_goldens", ROOT / "tools" / "make_matching_transformer_goldens.py").install_standins()
    assert "pfpp_hip" not in sys.modules
    ref = load("jigsaw_attention_layer", src)

    torch.set_num_threads(8)
    layer = ref.CrossAttentionLayer(d_in=cases.FEAT, n_head=cases.HEADS).train()
    assert layer.training
    names = [k for k, _ in layer.named_parameters()]
    assert tuple(names) == cases.GRAD_NAMES, "the case file's parameter names are not the reference's"
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.base.cross_state_dict().items()}, strict=True)
    out = {"row_step": np.asarray(cases.ROW_STEP), "names": np.asarray(cases.TENSORS)}
    for name in cases.CASES:
        x, puz, dout = cases.case_inputs(name)
        r32, r64 = run(layer, x, puz, dout, torch.float32), run(layer, x, puz, dout, torch.float64)
        flips = int(((r32["pre"] > 0) != (r64["pre"] > 0)).sum())
        out[f"{name}_relu_flips"], out[f"{name}_relu_entries"] = np.asarray(flips), np.asarray(r64["pre"].size)
        out[f"{name}_pre_min_abs"] = np.asarray(float(np.abs(r64["pre"]).min()))
        print(f"{name}: {len(x)} rows in {len(puz)} puzzles; ReLU sign patterns differ in {flips} of {r64['pre'].size} entries, smallest float64 "
              f"|pre-activation| {np.abs(r64['pre']).min():.3g}")
        for key in cases.TENSORS:
            a32, a64 = r32[key], r64[key]
            dev, top = float(np.abs(a32 - a64).max() / np.abs(a64).max()), float(np.abs(a64).max())
            out[f"{name}_{key}_refdev"], out[f"{name}_{key}_max"] = np.asarray(dev), np.asarray(top)
            for part, v in cases.sample(a64).items():
                out[f"{name}_{key}_{part}"] = v
            print(f"{name} {key}: shape {a64.shape}, max |g| {top:.4g}, reference fp32 vs fp64 {dev:.3g} (relative to the maximum)")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
