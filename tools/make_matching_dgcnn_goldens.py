"""Generate tests/golden/matching_dgcnn.npz by RUNNING THE REFERENCE's DGCNNDynamic on the CPU (build container only).

    python tools/make_matching_dgcnn_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching by path (sys.dont_write_bytecode, nothing is copied): model/modules/encoder/dgcnn.py.
The inputs and weights come from tests/matching_dgcnn_cases.py, loaded by path; this process never imports the product.

torch_geometric is not installed where this runs.  Its two functions the module calls get stand-ins that state their semantics:
  * knn(x, y, k, batch_x, batch_y) with x is y: pairs (query, row) grouped by query, the min(k, n_piece) nearest rows of the query's
    piece ascending by the squared distance summed in channel order AT THE PRECISION OF x (the case file's feat_knn: float32 keys in
    the float32 run, float64 keys in the float64 run), lower index first on ties;
  * to_dense_batch(x, batch, fill_value, max_num_nodes).
For these third-party pieces the fixture is circular by necessity.  Everything else is the reference's own code: the appended zero
row, the mask on both halves, the convolutions, BatchNorms, LeakyReLUs, the max over the slots, the concatenation and conv5.

Each case runs in float32 and in float64 with INDEPENDENT searches.  A seed is accepted when (a) both runs pick the same neighbour
sets at all four levels and (b) at every level the smallest relative step between the 20th and the 21st key (float64 run) is at least
the case file's MIN_STEP; otherwise the next seed is tried.  A seed other than the case file's SEEDS entry is an error that names the
seed to put there.  The fixture holds results only: the float64 run's neighbour lists, strided float64 samples of x1 .. x4 and the
output, the state-dict names with shapes, the seed, the smallest step per level, and per tensor the reference's own float32
deviation from its float64 run relative to the tensor's largest magnitude."""
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

FIXTURE_CASES = ("tiny", "mixed")
STRIDE = {"x1": 7, "x2": 7, "x3": 7, "x4": 7, "out": 3}          # element strides of the flattened tensors
MAX_SEEDS = 200


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_dgcnn_cases", ROOT / "tests" / "matching_dgcnn_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


STATE = types.SimpleNamespace(cases=None, lists=[], steps=[])


def knn(x, y, k, batch_x=None, batch_y=None, cosine=False, num_workers=1, batch_size=None):
    assert x is y and batch_x is batch_y
    b = batch_x.numpy()
    assert (np.diff(b) >= 0).all()
    lengths = np.bincount(b)
    lengths = lengths[lengths > 0]
    N = x.shape[0]
    idx, step = STATE.cases.feat_knn(x.detach().numpy(), lengths, k, np.float32 if x.dtype == torch.float32 else np.float64)
    STATE.lists.append(idx)
    STATE.steps.append(float(step.min()))
    flat = idx.reshape(-1)
    rows = np.repeat(np.arange(N), k)[flat != N]
    return torch.from_numpy(np.stack([rows, flat[flat != N]]).astype(np.int64))


def to_dense_batch(x, batch=None, fill_value=0.0, max_num_nodes=None, batch_size=None):
    B = int(batch.max()) + 1
    counts = torch.bincount(batch, minlength=B)
    first = torch.cumsum(counts, 0) - counts
    pos = torch.arange(batch.numel()) - first[batch]
    n_max = int(max_num_nodes if max_num_nodes is not None else counts.max())
    keep = pos < n_max
    dense = torch.full((B, n_max) + tuple(x.shape[1:]), fill_value, dtype=x.dtype)
    dense[batch[keep], pos[keep]] = x[keep]
    mask = torch.zeros((B, n_max), dtype=torch.bool)
    mask[batch[keep], pos[keep]] = True
    return dense, mask


def install_standins():
    tg = types.ModuleType("torch_geometric")
    nn_ = types.ModuleType("torch_geometric.nn")
    utils = types.ModuleType("torch_geometric.utils")
    nn_.knn, utils.to_dense_batch = knn, to_dense_batch
    tg.nn, tg.utils = nn_, utils
    for m in (tg, nn_, utils):
        m.__path__ = []
        sys.modules[m.__name__] = m


def run(model, x, lengths, dtype) -> dict:
    STATE.lists, STATE.steps = [], []
    model.to(dtype)
    got = {}
    hooks = [getattr(model, f"conv{l}").register_forward_hook(
        lambda m, a, out, l=l: got.__setitem__(f"x{l}", out.max(dim=-1)[0].detach().double().numpy())) for l in range(1, 5)]
    with torch.no_grad():
        got["out"] = model(torch.from_numpy(x).to(dtype), torch.from_numpy(lengths)).double().numpy()
    for h in hooks:
        h.remove()
    model.float()
    assert len(STATE.lists) == 4
    got["knn"], got["steps"] = list(STATE.lists), list(STATE.steps)
    return got


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_dgcnn.npz"))
    args = ap.parse_args()
    src = Path(args.reference) / "Jigsaw_matching" / "model" / "modules" / "encoder" / "dgcnn.py"
    if not src.is_file():
        ap.error(f"{src}: no such file")
    cases = load_cases()
    STATE.cases = cases
    install_standins()
    assert "pfpp_hip" not in sys.modules
    spec = importlib.util.spec_from_file_location("jigsaw_dgcnn", src)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    torch.set_num_threads(8)
    model = ref.DGCNNDynamic(cases.FEAT, False, 3).eval()
    names = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert names == [(k, tuple(s)) for k, s in cases.state_dict_spec()], "the case file's names / shapes are not the reference's"
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.state_dict().items()}, strict=True)
    out = {"state_names": np.asarray([k for k, _ in names]), "state_shapes": np.asarray([",".join(map(str, s)) for _, s in names])}
    for k, v in STRIDE.items():
        out[f"stride_{k}"] = np.asarray(v)
    wrong = []
    for name in FIXTURE_CASES:
        for seed in range(MAX_SEEDS):
            x, lengths = cases.case_arrays(name, seed)
            N = len(x)
            r32, r64 = run(model, x, lengths, torch.float32), run(model, x, lengths, torch.float64)
            same = [bool((np.sort(a, 1) == np.sort(b, 1)).all()) for a, b in zip(r32["knn"], r64["knn"])]
            ok = all(same) and min(r64["steps"]) >= cases.MIN_STEP
            print(f"{name} seed {seed}: N = {N}; same neighbour sets per level {same}; smallest 20th/21st step per level "
                  f"{[f'{s:.3g}' for s in r64['steps']]} (float32 run {[f'{s:.3g}' for s in r32['steps']]}) -> {'accepted' if ok else 'rejected'}")
            if ok:
                break
        else:
            raise SystemExit(f"{name}: no seed below {MAX_SEEDS} meets both conditions")
        if seed != cases.SEEDS[name]:
            wrong.append(f"{name}: {seed}")
        pads = int(sum((r64["knn"][0] == N).sum(1).astype(bool)))
        assert pads == int(lengths[lengths < cases.K].sum()), "rows with padded slots: the pieces shorter than K"
        out[f"{name}_seed"] = np.asarray(seed)
        out[f"{name}_min_step"] = np.asarray(r64["steps"])
        for l in range(4):
            out[f"{name}_l{l + 1}_knn"] = r64["knn"][l].astype(np.int16)
        for key in ("x1", "x2", "x3", "x4", "out"):
            a32, a64 = r32[key], r64[key]
            dev = float(np.abs(a32 - a64).max() / np.abs(a64).max())
            out[f"{name}_{key}_refdev"] = np.asarray(dev)
            out[f"{name}_{key}_max"] = np.asarray(float(np.abs(a64).max()))
            out[f"{name}_{key}"] = a64.reshape(-1)[::STRIDE[key]].astype(np.float64)
            print(f"{name} {key}: shape {a64.shape}, max |x| {np.abs(a64).max():.4g}, reference fp32 vs fp64 {dev:.3g} (relative to the maximum)")
    if wrong:
        raise SystemExit("tests/matching_dgcnn_cases.py SEEDS does not hold the accepted seeds; set " + ", ".join(wrong) + " and run again")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
