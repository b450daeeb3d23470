"""Generate tests/golden/matching_transformer.npz by RUNNING THE REFERENCE's PointTransformerLayer and CrossAttentionLayer on the CPU
(build container only).

    python tools/make_matching_transformer_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching by path (sys.dont_write_bytecode, nothing is copied): model/jigsaw/attention_layer.py.
The inputs and weights come from tests/matching_transformer_cases.py, loaded by path; this process never imports the product.

einops is installed where this runs; torch_geometric is not.  Its two functions the layer calls get stand-ins that state their
semantics:
  * knn(x, y, k, batch_x, batch_y) with x is y: pairs (query, row) grouped by query, the min(k, n_piece) nearest rows of the query's
    piece ascending by the bit-defined float32 key of the case file (feat_knn_f32), lower index first on ties;
  * to_dense_batch(x, batch, fill_value, max_num_nodes).
For these third-party pieces the fixture is circular by necessity.  Everything else is the reference's own code: the projections,
the appended zero row, the masked offsets, linear_p, linear_w with its BatchNorms, the softmax over padded slots, the einsum, the
attention, both residuals and LayerNorms.

The index results are recorded in the float32 run and replayed in the float64 run (same indices).  The fixture holds results only:
idx_k and idx_v, strided samples of p_r, w and the self layer's output, of the attention output (before fc), the first LayerNorm
and the cross layer's output, the state-dict names with shapes, and per stored tensor the reference's own float32 deviation from
its float64 run relative to the tensor's largest magnitude."""
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

FIXTURE_CASES = ("tiny", "pair")
STRIDE = {"p_r": 193, "w": 29, "out": 5, "att": 9, "ln1": 9, "cross_out": 5}     # element strides of the flattened tensors


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_transformer_cases", ROOT / "tests" / "matching_transformer_cases.py")
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


STATE = types.SimpleNamespace(tape=Tape(), cases=None, gaps=[])


def knn(x, y, k, batch_x=None, batch_y=None, cosine=False, num_workers=1, batch_size=None):
    def compute():
        assert x is y and batch_x is batch_y
        b = batch_x.numpy()
        assert (np.diff(b) >= 0).all()
        lengths = np.bincount(b)
        lengths = lengths[lengths > 0]
        N = x.shape[0]
        idx, gap = STATE.cases.feat_knn_f32(x.detach().to(torch.float32).numpy(), lengths, k)
        STATE.gaps.append(float(gap.min()))
        rows = np.repeat(np.arange(N), k)[idx.reshape(-1) != N]
        cols = idx.reshape(-1)[idx.reshape(-1) != N]
        return torch.from_numpy(np.stack([rows, cols]).astype(np.int64))

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
    utils = types.ModuleType("torch_geometric.utils")
    nn_.knn, utils.to_dense_batch = knn, to_dense_batch
    tg.nn, tg.utils = nn_, utils
    for m in (tg, nn_, utils):
        m.__path__ = []
        sys.modules[m.__name__] = m


def run_self(layer, p, x, lengths, dtype, tape: Tape, replay: bool) -> dict:
    tape.rewind(replay)
    STATE.tape = tape
    layer.to(dtype)
    got, hooks = {}, []
    hooks.append(layer.linear_p.register_forward_hook(lambda m, a, out: got.__setitem__("p_r", out.detach().double().numpy())))
    hooks.append(layer.softmax.register_forward_hook(lambda m, a, out: got.__setitem__("w", out.detach().double().numpy())))
    with torch.no_grad():
        got["out"] = layer(torch.from_numpy(p).to(dtype), torch.from_numpy(x).to(dtype), torch.from_numpy(lengths)).double().numpy()
    for h in hooks:
        h.remove()
    layer.float()
    return got


def run_cross(layer, x, puzzle_points, dtype) -> dict:
    layer.to(dtype)
    got = {"att": [], "ln1": [], "cross_out": []}
    hooks = [layer.attn.fc.register_forward_pre_hook(lambda m, a: got["att"].append(a[0][0].detach().double().numpy())),
             layer.attn.register_forward_hook(lambda m, a, out: got["ln1"].append(out[0][0].detach().double().numpy()))]
    lo = 0
    with torch.no_grad():
        for n in puzzle_points:                                   # the reference takes puzzles of one size per call: one call each
            got["cross_out"].append(layer(torch.from_numpy(x[lo:lo + n]).to(dtype)[None])[0].double().numpy())
            lo += n
    for h in hooks:
        h.remove()
    layer.float()
    return {k: np.concatenate(v) for k, v in got.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "matching_transformer.npz"))
    args = ap.parse_args()
    src = Path(args.reference) / "Jigsaw_matching" / "model" / "jigsaw" / "attention_layer.py"
    if not src.is_file():
        ap.error(f"{src}: no such file")
    cases = load_cases()
    STATE.cases = cases
    install_standins()
    assert "pfpp_hip" not in sys.modules
    spec = importlib.util.spec_from_file_location("jigsaw_attention_layer", src)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    torch.set_num_threads(8)
    self_layer = ref.PointTransformerLayer(in_feat=cases.FEAT, out_feat=cases.FEAT, n_heads=cases.HEADS, nsampmle=cases.NSAMPLE).eval()
    cross_layer = ref.CrossAttentionLayer(d_in=cases.FEAT, n_head=cases.HEADS).eval()
    out = {}
    for tag, layer, spec_fn, sd_fn in (("self", self_layer, cases.ptf_state_dict_spec, cases.ptf_state_dict),
                                       ("cross", cross_layer, cases.cross_state_dict_spec, cases.cross_state_dict)):
        names = [(k, tuple(v.shape)) for k, v in layer.state_dict().items()]
        assert names == [(k, tuple(s)) for k, s in spec_fn()], f"{tag}: the case file's names / shapes are not the reference's"
        layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_fn().items()}, strict=True)
        out[f"{tag}_state_names"] = np.asarray([k for k, _ in names])
        out[f"{tag}_state_shapes"] = np.asarray([",".join(map(str, s)) for _, s in names])
    for k, v in STRIDE.items():
        out[f"stride_{k}"] = np.asarray(v)
    for name in FIXTURE_CASES:
        p, x, lengths, puzzle_points = cases.case_arrays(name)
        N = len(x)
        tape = Tape()
        STATE.gaps = []
        r32 = run_self(self_layer, p, x, lengths, torch.float32, tape, replay=False)
        calls = list(tape.calls)
        r64 = run_self(self_layer, p, x, lengths, torch.float64, tape, replay=True)
        assert tape.pos == len(calls) == 2                         # knn on x_k, then on x_v
        idx = [to_dense_batch(c[1], c[0], fill_value=N, max_num_nodes=cases.NSAMPLE)[0].numpy() for c in calls]
        differ = float((idx[0] != idx[1]).any(1).mean())
        print(f"{name}: N = {N}; idx_k and idx_v differ in {100 * differ:.1f} % of the rows; smallest relative step between two "
              f"different neighbour distances {min(STATE.gaps):.3g}")
        assert differ > 0.5, "the pairing of slot t of idx_v with slot t of idx_k is not pinned by this case"
        assert (idx[0][:, 0] == np.arange(N)).mean() > 0.99 and int((idx[0] == N).sum()) == 5 * 11      # the 5-point piece pads 11 slots
        out[f"{name}_idx_k"], out[f"{name}_idx_v"] = idx[0].astype(np.int16), idx[1].astype(np.int16)
        out[f"{name}_knn_gap"] = np.asarray(min(STATE.gaps))
        r32.update(run_cross(cross_layer, x, puzzle_points, torch.float32))
        r64.update(run_cross(cross_layer, x, puzzle_points, torch.float64))
        for key in sorted(r32):
            a32, a64 = r32[key], r64[key]
            dev = float(np.abs(a32 - a64).max() / np.abs(a64).max())
            out[f"{name}_{key}_refdev"] = np.asarray(dev)
            out[f"{name}_{key}_max"] = np.asarray(float(np.abs(a64).max()))
            out[f"{name}_{key}"] = a32.reshape(-1)[::STRIDE[key]].astype(np.float32)
            print(f"{name} {key}: shape {a32.shape}, max |x| {np.abs(a64).max():.4g}, reference fp32 vs fp64 {dev:.3g} (relative to the maximum)")
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
