"""Generate tests/golden/matching_self_train.npz by RUNNING THE REFERENCE's PointTransformerLayer in .train() under autograd on the CPU
(build container only).

    python tools/make_matching_self_train_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching by path (sys.dont_write_bytecode, nothing is copied): model/jigsaw/attention_layer.py, with
the torch_geometric stand-ins of tools/make_matching_transformer_goldens.py; the knn stand-in replays the lists recorded in
tests/golden/matching_transformer.npz (the projections do not depend on the mode, so they are this run's lists too).  Inputs and
weights come from tests/matching_self_train_cases.py, loaded by path; this process never imports the product.

Per case (`tiny`, `pair`) the layer runs on the whole flat batch in one call with loss = sum(out * dout), three times from the same
state dict: in float32, in float64 with its own ReLU signs (only to count how many signs differ), and in float64 with the float32
run's three ReLU patterns imposed (the three nn.ReLU modules of this process's instance are replaced by a masked one), so that the
stored deviation is rounding and not sign flips.  The fixture holds results only:
  * per tensor (out, dx, the 20 parameter gradients, the 6 running buffers) the reference's float32-against-float64 deviation over the
    tensor's largest magnitude, and that magnitude;
  * of the float64 tensors: the vectors in full; of the matrices, out and dx the row sums, column sums and every 8th row;
  * per ReLU the number of differing signs, the entries and the smallest float64 |pre-activation|; the three masks of `tiny` (packbits)."""
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


class TapReLU(torch.nn.Module):
    """stands where an nn.ReLU stood: records its input; with a mask set, relu(x) = x * mask"""

    def __init__(self):
        super().__init__()
        self.pre, self.mask = None, None

    def forward(self, x):
        self.pre = x.detach().double().numpy().copy()
        return torch.relu(x) if self.mask is None else x * torch.from_numpy(self.mask).to(x.dtype)


def run(layer, taps, sd, p, x, lengths, dout, dtype, masks=None) -> dict:
    """the reference's layer in .train() on the flat batch under autograd, from the state dict sd -> float64 numpy"""
    layer.float()
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    layer.to(dtype).train()
    layer.zero_grad(set_to_none=True)
    for i, tap in enumerate(taps):
        tap.mask = None if masks is None else masks[i]
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = layer(torch.from_numpy(p).to(dtype), xt, torch.from_numpy(lengths))
    (out * torch.from_numpy(dout).to(dtype)).sum().backward()
    got = {"out": out.detach().double().numpy(), "dx": xt.grad.double().numpy(), "pre": [tap.pre for tap in taps]}
    got.update({k: v.grad.double().numpy().copy() for k, v in layer.named_parameters()})
    got.update({k: v.double().numpy().copy() for k, v in layer.named_buffers() if not k.endswith("num_batches_tracked")})
    got["num_batches_tracked"] = [int(v) for k, v in layer.named_buffers() if k.endswith("num_batches_tracked")]
    return got


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_self_train.npz"))
    args = ap.parse_args()
    src = Path(args.reference) / "Jigsaw_matching" / "model" / "jigsaw" / "attention_layer.py"
    if not src.is_file():
        ap.error(f"{src}: no such file")
    cases = load("matching_self_train_cases", ROOT / "tests" / "matching_self_train_cases.py")
    standins = load("make_matching_transformer_goldens", ROOT / "tools" / "make_matching_transformer_goldens.py")
    standins.STATE.cases = cases.base
    standins.install_standins()
    assert "pfpp_hip" not in sys.modules
    ref = load("jigsaw_attention_layer", src)
    recorded = np.load(ROOT / "tests" / "golden" / "matching_transformer.npz")

    torch.set_num_threads(8)
    layer = ref.PointTransformerLayer(in_feat=cases.FEAT, out_feat=cases.FEAT, n_heads=cases.HEADS, nsampmle=cases.NSAMPLE)
    assert tuple(k for k, _ in layer.named_parameters()) == cases.GRAD_NAMES, "the case file's parameter names are not the reference's"
    assert all(isinstance(layer.linear_p[2], torch.nn.ReLU) and isinstance(m, torch.nn.ReLU) for m in (layer.linear_w[1], layer.linear_w[4]))
    taps = [TapReLU(), TapReLU(), TapReLU()]
    layer.linear_p[2], layer.linear_w[1], layer.linear_w[4] = taps
    sd = cases.base.ptf_state_dict()
    out = {"row_step": np.asarray(cases.ROW_STEP), "names": np.asarray(cases.TENSORS)}
    for name in cases.CASES:
        p, x, lengths, dout = cases.case_inputs(name)
        N = len(x)
        idx = [recorded[f"{name}_idx_k"].astype(np.int64), recorded[f"{name}_idx_v"].astype(np.int64)]
        rows = np.repeat(np.arange(N), cases.NSAMPLE)
        tape = standins.Tape()
        tape.calls = [torch.from_numpy(np.stack([rows[i.reshape(-1) != N], i.reshape(-1)[i.reshape(-1) != N]])) for i in idx]
        standins.STATE.tape = tape

        def go(dtype, masks=None):
            tape.rewind(replay=True)
            got = run(layer, taps, sd, p, x, lengths, dout, dtype, masks)
            assert tape.pos == 2                                   # knn on x_k, then on x_v
            return got

        r32, r64own = go(torch.float32), go(torch.float64)
        masks = [a > 0 for a in r32["pre"]]
        r64 = go(torch.float64, masks)
        assert r32["num_batches_tracked"] == [1, 1, 1]
        for i, (a32, a64) in enumerate(zip(r32["pre"], r64own["pre"])):
            flips = int(((a32 > 0) != (a64 > 0)).sum())
            out[f"{name}_relu{i}_flips"], out[f"{name}_relu{i}_entries"] = np.asarray(flips), np.asarray(a64.size)
            out[f"{name}_relu{i}_pre_min_abs"] = np.asarray(float(np.abs(a64).min()))
            print(f"{name} ReLU {i}: signs of the float32 run differ from the float64 run's own in {flips} of {a64.size} entries "
                  f"({1e4 * flips / a64.size:.3f} per 10,000); smallest float64 |pre-activation| {np.abs(a64).min():.3g}")
            if name == "tiny":
                out[f"tiny_relu{i}_mask"], out[f"tiny_relu{i}_shape"] = np.packbits(masks[i].reshape(-1)), np.asarray(masks[i].shape)
        for key in cases.TENSORS:
            a32, a64 = r32[key], r64[key]
            top = float(np.abs(a64).max())
            dev = float(np.abs(a32 - a64).max() / top)
            out[f"{name}_{key}_refdev"], out[f"{name}_{key}_max"] = np.asarray(dev), np.asarray(top)
            for part, v in cases.sample(a64).items():
                out[f"{name}_{key}_{part}"] = v
            print(f"{name} {key}: shape {a64.shape}, max |.| {top:.4g}, reference fp32 vs fp64 {dev:.3g} (relative to the maximum)")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
