"""Generate tests/golden/matching_dgcnn_train.npz by RUNNING THE REFERENCE's DGCNNDynamic in .train() on the CPU (build container only).

    python tools/make_matching_dgcnn_train_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching by path (sys.dont_write_bytecode, nothing is copied): model/modules/encoder/dgcnn.py, with
the stand-ins of tools/make_matching_dgcnn_goldens.py for torch_geometric's knn and to_dense_batch (loaded by path; see that file for
what they state).  The inputs, weights and dout come from tests/matching_dgcnn_train_cases.py; this process never imports the product.

Each case runs forward + backward (loss = sum(out * dout)) in float32 and in float64 with INDEPENDENT searches.  A seed is accepted
when (a) both runs pick the same neighbour sets at all four levels, (b) at every level the smallest relative step between the 20th and
the 21st key (float64 run) is at least the case file's MIN_STEP and (c) both runs pick the SAME WINNER of the max over the slots, by
neighbour identity, for every (point, channel) at every level: one flipped winner moves the reference's own float32 gradients by far
more than rounding.  Otherwise the next seed is tried.  A seed other than the case file's SEEDS entry is an error that names the seed
to put there.  The fixture holds results only: the float64 run's lists and winning slots, strided float64 samples of x1 .. x4, out and
the 15 gradients, the 10 running buffers after the step, and per tensor the reference's float32 deviation from its float64 run
relative to the tensor's largest magnitude."""
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

FIXTURE_CASES = ("tiny", "small")
ACT_STRIDE = {"x1": 41, "x2": 41, "x3": 41, "x4": 41, "out": 17}              # element strides of the flattened tensors
GRAD_STRIDE = {"conv1.0.weight": 1, "conv2.0.weight": 13, "conv3.0.weight": 29, "conv4.0.weight": 101, "conv5.0.weight": 101}       # the rest: 1
MAX_SEEDS = 200


def load(name: str, path: Path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(model, sd, fw, x, lengths, dout, dtype) -> dict:
    """one .train() forward + backward of the reference's module from the case file's state"""
    model.float()
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.to(dtype).train()
    model.zero_grad(set_to_none=True)
    fw.STATE.lists, fw.STATE.steps = [], []
    got = {}

    def keep(l):
        def hook(m, a, out):                                 # out [N, C, 20]
            val, slot = out.max(dim=-1)
            got[f"x{l}"], got[f"w{l}"] = val.detach().double().numpy(), slot.numpy()
        return hook

    hooks = [getattr(model, f"conv{l}").register_forward_hook(keep(l)) for l in range(1, 5)]
    out = model(torch.from_numpy(x).to(dtype), torch.from_numpy(lengths))
    for h in hooks:
        h.remove()
    (out * torch.from_numpy(dout).to(dtype)).sum().backward()
    assert len(fw.STATE.lists) == 4
    got["out"] = out.detach().double().numpy()
    got["knn"], got["steps"] = list(fw.STATE.lists), list(fw.STATE.steps)
    got["grads"] = {k: p.grad.detach().double().numpy() for k, p in model.named_parameters()}
    got["buffers"] = {k: b.detach().double().numpy() for k, b in model.named_buffers() if not k.endswith("num_batches_tracked")}
    got["tracked"] = [int(getattr(model, f"bn{l}").num_batches_tracked) for l in range(1, 6)]
    # the winner by neighbour identity (every padded slot is the same all-zero row: N)
    got["who"] = [np.take_along_axis(got["knn"][l], got[f"w{l + 1}"], 1) for l in range(4)]
    return got


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_dgcnn_train.npz"))
    args = ap.parse_args()
    src = Path(args.reference) / "Jigsaw_matching" / "model" / "modules" / "encoder" / "dgcnn.py"
    if not src.is_file():
        ap.error(f"{src}: no such file")
    cases = load("matching_dgcnn_train_cases", ROOT / "tests" / "matching_dgcnn_train_cases.py")
    fw = load("make_matching_dgcnn_goldens", ROOT / "tools" / "make_matching_dgcnn_goldens.py")
    fw.STATE.cases = cases
    fw.install_standins()
    assert "pfpp_hip" not in sys.modules
    ref = load("jigsaw_dgcnn", src)

    torch.set_num_threads(8)
    model = ref.DGCNNDynamic(cases.FEAT, False, 3)
    sd = cases.state_dict()
    assert tuple(k for k, _ in model.named_parameters()) == cases.PARAMS, "the case file's parameter names are not the reference's"
    assert tuple(k for k, _ in model.named_buffers() if not k.endswith("num_batches_tracked")) == cases.BUFFERS
    out = {"param_names": np.asarray(cases.PARAMS), "buffer_names": np.asarray(cases.BUFFERS)}
    for k, v in ACT_STRIDE.items():
        out[f"stride_{k}"] = np.asarray(v)
    for k in cases.PARAMS:
        out[f"stride_{k}"] = np.asarray(GRAD_STRIDE.get(k, 1))
    wrong = []
    for name in FIXTURE_CASES:
        for seed in range(MAX_SEEDS):
            x, lengths = cases.case_arrays(name, seed)
            dout = cases.dout_array(name, seed)
            N = len(x)
            r32, r64 = run(model, sd, fw, x, lengths, dout, torch.float32), run(model, sd, fw, x, lengths, dout, torch.float64)
            same = [bool((np.sort(a, 1) == np.sort(b, 1)).all()) for a, b in zip(r32["knn"], r64["knn"])]
            flips = [int((a != b).sum()) for a, b in zip(r32["who"], r64["who"])]
            ok = all(same) and min(r64["steps"]) >= cases.MIN_STEP and sum(flips) == 0
            print(f"{name} seed {seed}: N = {N}; same neighbour sets per level {same}; smallest 20th/21st step per level "
                  f"{[f'{s:.3g}' for s in r64['steps']]}; winners that differ per level {flips} -> {'accepted' if ok else 'rejected'}")
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed below {MAX_SEEDS} meets the three conditions")
        if seed != cases.SEEDS[name]:
            wrong.append(f"{name}: {seed}")
        assert r64["tracked"] == [int(sd[f"bn{l}.num_batches_tracked"]) + 1 for l in range(1, 6)]
        out[f"{name}_seed"] = np.asarray(seed)
        out[f"{name}_min_step"] = np.asarray(r64["steps"])
        for l in range(4):
            out[f"{name}_l{l + 1}_knn"] = r64["knn"][l].astype(np.int16)
            out[f"{name}_l{l + 1}_winner"] = r64[f"w{l + 1}"].astype(np.uint8)
            padded = int((r64["who"][l] == N).sum())
            print(f"{name} level {l + 1}: {padded} of {r64['who'][l].size} entries won by a padded slot")

        def put(key, a32, a64, stride):
            dev = float(np.abs(a32 - a64).max() / np.abs(a64).max())
            out[f"{name}_{key}_refdev"] = np.asarray(dev)
            out[f"{name}_{key}_max"] = np.asarray(float(np.abs(a64).max()))
            out[f"{name}_{key}"] = a64.reshape(-1)[::stride].astype(np.float64)
            print(f"{name} {key}: shape {a64.shape}, max |x| {np.abs(a64).max():.4g}, reference fp32 vs fp64 {dev:.3g} (relative to the maximum)")

        for key in ("x1", "x2", "x3", "x4", "out"):
            put(key, r32[key], r64[key], ACT_STRIDE[key])
        for key in cases.PARAMS:
            put(f"grad_{key}", r32["grads"][key], r64["grads"][key], GRAD_STRIDE.get(key, 1))
        for key in cases.BUFFERS:
            put(f"buf_{key}", r32["buffers"][key], r64["buffers"][key], 1)
    if wrong:
        raise SystemExit("tests/matching_dgcnn_train_cases.py SEEDS does not hold the accepted seeds; set " + ", ".join(wrong) + " and run again")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
