"""Generate tests/golden/matching_encoder.npz by RUNNING THE REFERENCE's PointNet2PTMSGDynamic on the CPU (build container only).

    python tools/make_matching_encoder_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching (sys.dont_write_bytecode, nothing is copied):
model/modules/encoder/pointnet2_pointwise/pointnet2_msg.py and pointnet2_dynamic_utils.py.  The matcher's top-level packages are
called `model`, `utils` and `dataset`, so this process never imports the product; the inputs come from
tests/matching_encoder_cases.py (numpy only), loaded by path.

torch_geometric is not installed where this runs.  Its three functions the encoder calls get stand-ins that state their semantics:
  * fps(x, batch, ratio): per piece ceil(ratio n) samples with the product and the ceiling in float32, squared distance
    (dx dx + dy dy) + dz dz in float32, running minimum, first argmax; the first index comes from the case file (random_start);
  * knn(x, y, k, batch_x, batch_y): pairs (query, point) grouped by query, ascending by the same squared distance, lower index
    first on ties, at most k per query and only points of the query's piece;
  * to_dense_batch(x, batch, fill_value, max_num_nodes).
For these third-party pieces the fixture is circular by necessity.  Everything else is the reference's own code: grouping, the
fill / group_first handling, the MLPs with BatchNorm, the interpolation arithmetic, the concatenations, conv1.

The fixture holds results only: per level the centroid indices, the sorted neighbour rows, the interpolation weights by centroid,
strided samples of each level's output and of each propagated level, every 3rd row of the descriptors, the state-dict names with
shapes, and per stored tensor the reference's own float32 deviation from the same module run in float64 on the same indices,
relative to the tensor's largest magnitude."""
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

FIXTURE_CASES = ("small", "second")
STRIDE = 5           # stride of the stored samples of the level outputs (flattened [rows, channels])
ROW_STRIDE = 3       # every 3rd row of the final descriptors


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_encoder_cases", ROOT / "tests" / "matching_encoder_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Tape:
    """the index results of the stand-ins: computed and recorded in the float32 run, replayed in the float64 run (same indices)"""

    def __init__(self):
        self.calls, self.pos, self.replay = [], 0, False

    def take(self, compute):
        if self.replay:
            out = self.calls[self.pos]
            self.pos += 1
            return out
        out = compute()
        self.calls.append(out)
        return out

    def rewind(self, replay: bool):
        self.pos, self.replay = 0, replay


STATE = types.SimpleNamespace(tape=Tape(), cases=None, start=None, level=0)


def _pieces(batch: torch.Tensor):
    b = batch.numpy()
    assert (np.diff(b) >= 0).all()
    bounds = np.flatnonzero(np.diff(b)) + 1
    return np.concatenate([[0], bounds]), np.concatenate([bounds, [len(b)]])


def fps(x, batch=None, ratio=0.5, random_start=True, batch_size=None):
    def compute():
        pts = x.detach().to(torch.float32).numpy()
        lo, hi = _pieces(batch)
        out = []
        for p, (a, b) in enumerate(zip(lo, hi)):
            n = b - a
            m = int(STATE.cases.sample_count(n, ratio))
            q = pts[a:b]
            dist = np.full(n, np.inf, dtype=np.float32)
            cur = int(STATE.start[STATE.level, p])
            for _ in range(m):
                out.append(a + cur)
                d = q - q[cur]
                dist = np.minimum(dist, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                cur = int(np.argmax(dist))
        STATE.level += 1
        return torch.from_numpy(np.asarray(out, dtype=np.int64))

    return STATE.tape.take(compute)


def knn(x, y, k, batch_x=None, batch_y=None, cosine=False, num_workers=1, batch_size=None):
    def compute():
        px, py = x.detach().to(torch.float32).numpy(), y.detach().to(torch.float32).numpy()
        lo, hi = _pieces(batch_x)
        piece_of_x = batch_x.numpy()[lo]
        rows, cols = [], []
        by = batch_y.numpy()
        for a, b, pid in zip(lo, hi, piece_of_x):
            qs = np.flatnonzero(by == pid)
            if qs.size == 0:
                continue
            d = py[qs][:, None, :] - px[a:b][None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            order = np.argsort(d2, axis=1, kind="stable")[:, :k]
            rows.append(np.repeat(qs, order.shape[1]))
            cols.append((order + a).reshape(-1))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        o = np.argsort(rows, kind="stable")
        return torch.from_numpy(np.stack([rows[o], cols[o]]).astype(np.int64))

    return STATE.tape.take(compute)


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
    pool = types.ModuleType("torch_geometric.nn.pool")
    utils = types.ModuleType("torch_geometric.utils")
    pool.fps, pool.knn, utils.to_dense_batch = fps, knn, to_dense_batch
    tg.nn, tg.utils, nn_.pool = nn_, utils, pool
    for m in (tg, nn_, pool, utils):
        m.__path__ = []
        sys.modules[m.__name__] = m


class _Captured(Exception):
    pass


def run(model, cases, puzzles, dtype, tape: Tape, replay: bool):
    """one forward of the reference's module over the pieces of `puzzles` (concatenated: nothing in the module looks at puzzles)
    with hooks on every level -> dict of float64 / int arrays"""
    pts = np.concatenate([pz["points"] for pz in puzzles])
    lengths = np.concatenate([pz["lengths"] for pz in puzzles])
    STATE.start = np.concatenate([pz["start"] for pz in puzzles], 1)
    STATE.level, STATE.tape = 0, tape
    tape.rewind(replay)
    model.to(dtype)
    got, hooks = {}, []
    geo = {}
    for l, name in enumerate(("sa1", "sa2", "sa3", "sa4"), 1):
        def sa_hook(mod, args, out, l=l):
            geo[l] = (out[0].detach(), out[1].detach())
            got[f"l{l}_points"] = out[2][0].t().double().numpy()
        hooks.append(getattr(model, name).register_forward_hook(sa_hook))
    for name, d1 in (("fp4", 512), ("fp3", 256), ("fp2", 96), ("fp1", 0)):
        def pre(mod, args, name=name, d1=d1):
            got[f"{name}_interp"] = args[0][0, d1:].t().double().numpy()
        def post(mod, args, out, name=name):
            got[f"{name}_out"] = out[0].t().double().numpy()
        hooks.append(getattr(model, name).mlp_convs[0].register_forward_pre_hook(pre))
        hooks.append(getattr(model, name).register_forward_hook(post))
    x = torch.from_numpy(pts).to(dtype)
    with torch.no_grad():
        got["final"] = model(x, [int(n) for n in lengths]).double().numpy()
    for h in hooks:
        h.remove()
    # the interpolation weights, by the reference's own arithmetic: propagate one-hot features and stop before the MLP
    piece0 = torch.from_numpy(np.repeat(np.arange(len(lengths)), lengths)).reshape(1, 1, -1)
    geo[0] = (x.t()[None], piece0)
    for name, fine, coarse in (("fp4", 3, 4), ("fp3", 2, 3), ("fp2", 1, 2), ("fp1", 0, 1)):
        S = geo[coarse][0].shape[2]
        box = {}

        def stop(mod, args, box=box):
            box["w"] = args[0][0].t().double().numpy()
            raise _Captured()

        h = getattr(model, name).mlp_convs[0].register_forward_pre_hook(stop)
        try:
            with torch.no_grad():
                getattr(model, name)(geo[fine][0], geo[coarse][0], geo[fine][1], geo[coarse][1], None, torch.eye(S, dtype=dtype)[None])
            raise AssertionError("the MLP was reached")
        except _Captured:
            pass
        finally:
            h.remove()
        dense = box["w"]                                         # [N, S]: the weight each centroid carries for each fine point
        order = np.argsort(-dense, axis=1, kind="stable")[:, :3]
        w = np.take_along_axis(dense, order, 1)
        assert (np.count_nonzero(dense, axis=1) <= 3).all()
        got[f"{name}_w_idx"] = np.where(w > 0, order, -1)
        got[f"{name}_w"] = w
    model.float()
    return got


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_encoder.npz"))
    args = ap.parse_args()
    jig = Path(args.reference) / "Jigsaw_matching"
    if not jig.is_dir():
        ap.error(f"{jig}: not a directory")
    cases = load_cases()
    STATE.cases = cases
    install_standins()
    assert "pfpp_hip" not in sys.modules
    # the two files by path under their package names: model/__init__.py would import the whole matcher (Lightning, open3d, ...)
    pkg_dir = jig / "model" / "modules" / "encoder" / "pointnet2_pointwise"
    pkg = types.ModuleType("pn2_pointwise")
    pkg.__path__ = [str(pkg_dir)]
    sys.modules["pn2_pointwise"] = pkg
    for stem in ("pointnet2_utils", "pointnet2_dynamic_utils", "pointnet2_msg"):
        spec = importlib.util.spec_from_file_location(f"pn2_pointwise.{stem}", pkg_dir / f"{stem}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
    Encoder = sys.modules["pn2_pointwise.pointnet2_msg"].PointNet2PTMSGDynamic

    torch.set_num_threads(8)
    model = Encoder(cases.FEAT_IN, cases.FEAT_OUT).eval()
    names = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert names == [(k, tuple(s)) for k, s in cases.state_dict_spec()], "the case file's names / shapes are not the reference's"
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.encoder_state_dict().items()}, strict=True)
    out = {"state_names": np.asarray([k for k, _ in names]), "state_shapes": np.asarray([",".join(map(str, s)) for _, s in names]),
           "stride": np.asarray(STRIDE), "row_stride": np.asarray(ROW_STRIDE),
           "count_n": np.arange(1, 5001, dtype=np.int64),
           "count_015": cases.sample_count(np.arange(1, 5001), 0.15).astype(np.int16),
           "count_025": cases.sample_count(np.arange(1, 5001), 0.25).astype(np.int16)}
    for name in FIXTURE_CASES:
        puzzles = cases.make_case(name)
        tape = Tape()
        r32 = run(model, cases, puzzles, torch.float32, tape, replay=False)
        calls = list(tape.calls)
        r64 = run(model, cases, puzzles, torch.float64, tape, replay=True)
        assert tape.pos == len(calls)
        # tape order of the forward: per SA level fps, knn(16), knn(32); per FP level knn(3); then the four weight passes
        lengths = np.concatenate([pz["lengths"] for pz in puzzles])
        counts = cases.level_counts(lengths)
        for l in range(4):
            cen, k16, k32 = (calls[3 * l + j] for j in range(3))
            assert cen.numel() == counts[l + 1].sum()
            out[f"{name}_l{l + 1}_centroids"] = cen.numpy().astype(np.int16)
            for K, pairs in ((16, k16), (32, k32)):
                dense = to_dense_batch(pairs[1], pairs[0], fill_value=-1, max_num_nodes=K)[0].numpy()
                dense = np.where(dense < 0, dense[:, :1], dense)
                out[f"{name}_l{l + 1}_knn{K}"] = np.sort(dense, axis=1).astype(np.int16)
        for key in sorted(r32):
            a32, a64 = r32[key], r64[key]
            if key.endswith("_w_idx"):
                assert np.array_equal(a32, a64)
                out[f"{name}_{key}"] = a32.astype(np.int16)
                continue
            dev = float(np.abs(a32 - a64).max() / np.abs(a64).max())
            out[f"{name}_{key}_refdev"] = np.asarray(dev)
            out[f"{name}_{key}_max"] = np.asarray(float(np.abs(a64).max()))
            if key == "final":
                out[f"{name}_final"] = a32[::ROW_STRIDE].astype(np.float32)
            elif key.endswith("_w"):
                out[f"{name}_{key}"] = a32.astype(np.float32)
            else:
                out[f"{name}_{key}"] = a32.reshape(-1)[::STRIDE].astype(np.float32)
            print(f"{name} {key}: shape {a32.shape}, max |x| {np.abs(a64).max():.4g}, reference fp32 vs fp64 {dev:.3g} (relative to the maximum)")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
