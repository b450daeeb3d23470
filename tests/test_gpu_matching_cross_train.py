"""GPU: the backward of the matcher's cross-attention layer (csrc/matching_tf_train.hip, pfpp_hip/matching_transformer_train.py)
against (a) tests/golden/matching_cross_train.npz, written by tools/make_matching_cross_train_goldens.py from the reference's own
layer under autograd, and (b) the restatements of tests/matching_cross_train_cases.py, which
tests/test_matching_cross_train_host.py pins to that fixture to 1e-12.  Every test prints the figures it measured before it asserts.

Bars (the rule of 5.6 and 5.7).  Per tensor, 4 x the reference's own float32-against-float64 deviation relative to
the tensor's largest magnitude, floor 4 x 2^-23: from the fixture for the engine, from a float32 torch autograd evaluation of the
same inputs computed here for the kernels on their own.  The float64 run of the layer is fed the ReLU pattern the GPU used; that
pattern may differ from float64's own in at most 1 entry per 10,000, each with a float64 pre-activation below 1e-4."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FLOOR = 4.0 * 2.0 ** -23
ATTN_NAMES = ("edges_a", "edges_b", "wide", "many")
RELU_FLIPS_ALLOWED = {"tiny": 9, "pair": 13}         # 1 per 10,000 of 93,952 and 135,936 entries


def load_cases(stem):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases("matching_cross_train_cases")
base = cases.base
_ATTN, _LAYER, _RUN = {}, {}, {}


def rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def bar_of(dev_ref):
    return max(4.0 * dev_ref, FLOOR)


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def fresh_layer(dev):
    from pfpp_hip.matching_transformer import CrossAttentionLayer

    layer = CrossAttentionLayer(128, 8)
    layer.load_state_dict(tensors(base.cross_state_dict()), strict=True)
    return layer.to(dev)


def shared_layer(dev):
    """the layer with the case file's weights; no test writes to it"""
    if "layer" not in _LAYER:
        _LAYER["layer"] = fresh_layer(dev)
    return _LAYER["layer"]


# ------------------------------------------------------------------------------------------------ attention: inputs and references
def attn_ref(name):
    """inputs of an attention-only case, a seeded normal dout, and float64 / float32 torch autograd of both; computed once, left unchanged"""
    if name not in _ATTN:
        qkv, lengths = base.attn_case(name)
        dout = np.random.default_rng([43, ATTN_NAMES.index(name)]).normal(size=(len(qkv), 128)).astype(np.float32)
        r64 = [t.numpy() for t in cases.attention_grads(qkv, lengths, dout, torch.float64)]
        r32 = [t.double().numpy() for t in cases.attention_grads(qkv, lengths, dout, torch.float32)]
        _ATTN[name] = {"qkv": qkv, "lengths": lengths, "dout": dout, "out": r64[0], "lse": r64[1], "dqkv": r64[2],
                       "dev_lse": rel(r32[1], r64[1]), "dev_parts": [rel(r32[2][:, i * 128:(i + 1) * 128], r64[2][:, i * 128:(i + 1) * 128]) for i in range(3)]}
    return _ATTN[name]


def seqs(lengths, dev, skip_before=None):
    """seq_off / seq_len on the device; skip_before = s leaves one unused row in front of sequence s"""
    lengths = np.asarray(lengths, dtype=np.int64)
    off = np.cumsum(lengths) - lengths
    if skip_before is not None:
        off[skip_before:] += 1
    return torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(lengths.astype(np.int32)).to(dev)


def attn_forward(dev, name):
    from pfpp_hip.matching_transformer_train import attn_rows16_train

    r = attn_ref(name)
    qkv = torch.from_numpy(r["qkv"]).to(dev)
    off, ln = seqs(r["lengths"], dev)
    out, lse = attn_rows16_train(qkv, off, ln, int(r["lengths"].max()), 8, 0.25)
    return r, qkv, off, ln, out, lse


@pytest.mark.parametrize("name", ATTN_NAMES)
def test_attn_rows16_train_is_the_forward_bit_for_bit_and_its_lse(dev, hip_lib, name):
    from pfpp_hip.matching_transformer import attn_rows16

    r, qkv, off, ln, out, lse = attn_forward(dev, name)
    plain = attn_rows16(qkv, off, ln, int(r["lengths"].max()), 8, 0.25)
    err, bar = rel(lse.cpu().numpy(), r["lse"]), bar_of(r["dev_lse"])
    print(f"{name}: out == attn_rows16: {torch.equal(out, plain)}; lse {err:.3g} of the maximum {np.abs(r['lse']).max():.3g} "
          f"(float32 torch {r['dev_lse']:.3g}, bar {bar:.3g})")
    assert torch.equal(out, plain)
    assert lse.shape == (len(r["qkv"]), 8) and torch.isfinite(lse).all() and err <= bar


@pytest.mark.parametrize("name", ATTN_NAMES)
def test_attn_rows16_bwd_against_float64_autograd(dev, hip_lib, name):
    from pfpp_hip.matching_transformer_train import attn_rows16_bwd

    r, qkv, off, ln, out, lse = attn_forward(dev, name)
    dout = torch.from_numpy(r["dout"]).to(dev)
    L = int(r["lengths"].max())
    dqkv = attn_rows16_bwd(qkv, out, dout, lse, off, ln, L, 8, 0.25)
    again = attn_rows16_bwd(qkv, out, dout, lse, off, ln, L, 8, 0.25)
    got = dqkv.cpu().numpy()
    errs = [rel(got[:, i * 128:(i + 1) * 128], r["dqkv"][:, i * 128:(i + 1) * 128]) for i in range(3)]
    bars = [bar_of(d) for d in r["dev_parts"]]
    for part, e, d, b in zip(("dq", "dk", "dv"), errs, r["dev_parts"], bars):
        print(f"{name} {part}: {e:.3g} of the maximum (float32 torch autograd {d:.3g}, bar {b:.3g})")
    print(f"{name}: two runs agree bitwise: {torch.equal(dqkv, again)}")
    assert np.isfinite(got).all() and torch.equal(dqkv, again)
    assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)


@pytest.mark.parametrize("name", ["edges_b", "many"])
def test_attn_rows16_bwd_keeps_sequences_apart_and_unused_rows_untouched(dev, hip_lib, name):
    from pfpp_hip.matching_transformer_train import attn_rows16_bwd, attn_rows16_train

    r, qkv, off, ln, out, lse = attn_forward(dev, name)
    lengths = r["lengths"]
    L = int(lengths.max())
    dout = torch.from_numpy(r["dout"]).to(dev)
    want = attn_rows16_bwd(qkv, out, dout, lse, off, ln, L, 8, 0.25)
    # another dout for sequence 1 only: every other sequence's rows keep their bits
    lo, hi = int(lengths[0]), int(lengths[0] + lengths[1])
    other = dout.clone()
    other[lo:hi] = torch.flip(other[lo:hi], dims=(1,)) * 1.5 + 0.25
    got = attn_rows16_bwd(qkv, out, other, lse, off, ln, L, 8, 0.25)
    assert torch.equal(got[:lo], want[:lo]) and torch.equal(got[hi:], want[hi:]) and not torch.equal(got[lo:hi], want[lo:hi])
    # one unused row in front of sequence 1: it keeps the sentinel, forward and backward, and the sequences their results
    keep = torch.cat([torch.arange(lo), torch.arange(lo + 1, len(qkv) + 1)]).to(dev)
    wide = lambda t, fill: torch.full((t.shape[0] + 1, t.shape[1]), fill, dtype=t.dtype, device=dev).index_copy_(0, keep, t)
    off2, _ = seqs(lengths, dev, skip_before=1)
    qkv2 = wide(qkv, float("nan"))                               # whoever reads the unused row spreads NaN
    out2, lse2 = attn_rows16_train(qkv2, off2, ln, L, 8, 0.25)
    assert torch.equal(out2[keep], out) and torch.equal(lse2[keep], lse)
    out2[lo], lse2[lo] = float("nan"), float("nan")
    sentinel = torch.full_like(qkv2, -7.25)
    got2 = attn_rows16_bwd(qkv2, out2, wide(dout, float("nan")), lse2, off2, ln, L, 8, 0.25, dqkv=sentinel)
    assert got2 is sentinel and bool((got2[lo] == -7.25).all()) and torch.equal(got2[keep], want)


@pytest.mark.parametrize("k", [-20, 10])
def test_attn_rows16_bwd_is_linear_in_dout_bit_for_bit(dev, hip_lib, k):
    from pfpp_hip.matching_transformer_train import attn_rows16_bwd

    for name in ("edges_a", "many"):                             # both launch forms
        r, qkv, off, ln, out, lse = attn_forward(dev, name)
        dout = torch.from_numpy(r["dout"]).to(dev)
        L = int(r["lengths"].max())
        one = attn_rows16_bwd(qkv, out, dout, lse, off, ln, L, 8, 0.25)
        scaled = attn_rows16_bwd(qkv, out, dout * 2.0 ** k, lse, off, ln, L, 8, 0.25)
        tiny = float(one.abs()[one != 0].min()) * 2.0 ** k
        print(f"{name}: smallest non-zero |dqkv| 2^{k} = {tiny:.3g} (float32 normal range from 1.2e-38)")
        assert tiny > 1e-30 and torch.equal(scaled, one * 2.0 ** k)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1001])
def test_layernorm128_bwd_against_torch(dev, hip_lib, rows):
    """rows of very different mean and spread and, from 3 rows on, a constant row (variance 0: eps decides), against autograd of
    F.layer_norm in float64; the = and the += form of dx; dgamma / dbeta of two runs agree bitwise"""
    from pfpp_hip.matching_transformer_train import layernorm128_bwd

    rng = np.random.default_rng([59, rows])
    x = (rng.normal(size=(rows, 128)) * rng.uniform(0.01, 30.0, (rows, 1)) + rng.normal(0, 5.0, (rows, 1))).astype(np.float32)
    if rows >= 3:
        x[rows // 2] = 2.5
    dy = rng.normal(size=(rows, 128)).astype(np.float32)
    g = rng.uniform(0.5, 1.5, 128).astype(np.float32)
    init = rng.normal(size=(rows, 128)).astype(np.float32)

    def torch_grads(dt):
        xt, gt, bt = torch.from_numpy(x).to(dt).requires_grad_(True), torch.from_numpy(g).to(dt).requires_grad_(True), torch.zeros(128, dtype=dt, requires_grad=True)
        (torch.nn.functional.layer_norm(xt, (128,), gt, bt, 1e-6) * torch.from_numpy(dy).to(dt)).sum().backward()
        return [t.grad.double().numpy() for t in (xt, gt, bt)]

    want, ref32 = torch_grads(torch.float64), torch_grads(torch.float32)
    d = lambda a: torch.from_numpy(a).to(dev)
    dx, dg, db = layernorm128_bwd(d(x), d(dy), d(g), 1e-6)
    acc = d(init)
    dx2, dg2, db2 = layernorm128_bwd(d(x), d(dy), d(g), 1e-6, dx=acc, accumulate=True)
    for nm, got, w, r32 in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), want, ref32):
        dev_ref = rel(r32, w)
        err, bar = rel(got.cpu().numpy(), w), bar_of(dev_ref)
        print(f"layernorm128_bwd, {rows} rows, {nm}: {err:.3g} of the maximum {np.abs(w).max():.3g} (float32 torch {dev_ref:.3g}, bar {bar:.3g})")
        assert torch.isfinite(got).all() and err <= bar
    dev_acc = rel(ref32[0] + init.astype(np.float64), want[0] + init)
    err_acc = rel(dx2.cpu().numpy(), want[0] + init)
    print(f"layernorm128_bwd, {rows} rows, += form: {err_acc:.3g} (float32 torch {dev_acc:.3g}, bar {bar_of(dev_acc):.3g}); dx2 is the tensor handed in: {dx2 is acc}")
    assert dx2 is acc and err_acc <= bar_of(dev_acc) and torch.equal(dx2, d(init) + dx)
    assert torch.equal(dg, dg2) and torch.equal(db, db2)


# ------------------------------------------------------------------------------------------------ ReLU backward
def test_relu_bwd_is_exact_with_zeros_of_both_signs(dev, hip_lib):
    from pfpp_hip.matching_transformer_train import relu_bwd

    rng = np.random.default_rng(61)
    h = rng.normal(size=(1001, 256)).astype(np.float32)
    h[h < 0] = 0.0                                               # a ReLU's output ...
    h[5, :7], h[6, :7], h[7, :3] = 0.0, -0.0, [1e-30, -1e-30, 3e38]       # ... and what it never produces: -0, negative entries
    dh = rng.normal(size=(1001, 256)).astype(np.float32)
    hd, dd = torch.from_numpy(h).to(dev), torch.from_numpy(dh).to(dev)
    want = torch.where(hd > 0, dd, torch.zeros_like(dd))
    got = relu_bwd(hd, dd.clone())
    assert torch.equal(got, want) and float(got[5, :7].abs().max()) == 0 and float(got[6, :7].abs().max()) == 0
    assert float(got[7, 0]) == float(dh[7, 0]) and float(got[7, 1]) == 0 and float(got[7, 2]) == float(dh[7, 2])
    assert np.array_equal(got.cpu().numpy() != 0, (h > 0) & (dh != 0))
    # a column slice of wider rows: the columns next to it keep their bits
    wide_h, wide_d = torch.from_numpy(h).to(dev), torch.from_numpy(dh).to(dev)
    relu_bwd(wide_h[:, 64:192], wide_d[:, 64:192])
    assert torch.equal(wide_d[:, 64:192], want[:, 64:192]) and torch.equal(wide_d[:, :64], dd[:, :64]) and torch.equal(wide_d[:, 192:], dd[:, 192:])


# ------------------------------------------------------------------------------------------------ the engine
def engine_run(dev, name):
    """one forward + backward of the engine on a case; computed once, left unchanged"""
    from pfpp_hip.matching_transformer_train import CrossAttentionTrainEngine

    if name not in _RUN:
        layer = shared_layer(dev)
        x, puz, dout = cases.case_inputs(name)
        eng = CrossAttentionTrainEngine(layer)
        xd, dd = torch.from_numpy(x).to(dev), torch.from_numpy(dout.astype(np.float32)).to(dev)
        out = eng.forward(xd, puz)
        dx = eng.backward(dd)
        _RUN[name] = {"x": xd, "dout": dd, "puz": puz, "out": out, "dx": dx, "h": eng.saved["h"].clone(),
                      "grads": {k: p.grad.clone() for k, p in eng.params.items()}}
    return _RUN[name]


@pytest.mark.parametrize("name", ["tiny", "pair"])
def test_engine_forward_is_the_modules_and_gradients_stay_within_the_fixtures_bars(dev, hip_lib, golden, name):
    g = golden("matching_cross_train")
    run = engine_run(dev, name)
    layer = shared_layer(dev)
    assert torch.equal(run["out"], layer(run["x"], run["puz"]))
    x, puz, dout = cases.case_inputs(name)
    # the float64 run is fed the ReLU pattern the GPU used; its dout is the fixture's, not rounded to float32
    mask = (run["h"] > 0).cpu().numpy()
    want = cases.cross_train_restate(base.cross_state_dict(), x, puz, dout, torch.float64, relu_mask=mask)
    pre = want["pre"].numpy()
    differ = mask != (pre > 0)
    n_diff, worst_pre = int(differ.sum()), float(np.abs(pre[differ]).max()) if differ.any() else 0.0
    print(f"{name}: the GPU's ReLU pattern differs from float64's own in {n_diff} of {mask.size} entries (allowed {RELU_FLIPS_ALLOWED[name]}), "
          f"largest float64 |pre-activation| among them {worst_pre:.3g} (allowed 1e-4)")
    assert n_diff <= RELU_FLIPS_ALLOWED[name] and worst_pre < 1e-4
    failed = []
    for key in cases.TENSORS:
        got = run["dx"] if key == "dx" else run["grads"][key]
        dev_ref = float(g[f"{name}_{key}_refdev"])
        err, bar = rel(got.cpu().numpy(), want[key].numpy()), bar_of(dev_ref)
        print(f"{name} {key}: {err:.3g} of the maximum (reference fp32 vs fp64 {dev_ref:.3g}, bar {bar:.3g})")
        assert got.shape == want[key].shape and torch.isfinite(got).all()
        if err > bar:
            failed.append(key)
    assert not failed, failed


def test_engine_dx_of_a_puzzle_does_not_depend_on_its_neighbours(dev, hip_lib):
    """pair's dx rows of each puzzle equal, bit for bit, the dx of that puzzle run alone: no GEMM of the input-gradient chain splits K and
    the attention reads its own sequence only; the dense [B, N_sum, 128] form gives the flat form's bits"""
    from pfpp_hip.matching_transformer_train import CrossAttentionTrainEngine

    run = engine_run(dev, "pair")
    eng = CrossAttentionTrainEngine(shared_layer(dev))
    lo = 0
    for n in run["puz"]:
        n = int(n)
        out = eng.forward(run["x"][lo:lo + n].contiguous(), [n])
        dx = eng.backward(run["dout"][lo:lo + n].contiguous())
        assert torch.equal(out, run["out"][lo:lo + n]) and torch.equal(dx, run["dx"][lo:lo + n]), f"puzzle of {n} points"
        lo += n
    n = int(run["puz"][1])
    xb, db = run["x"][-2 * n:].reshape(2, n, 128), run["dout"][-2 * n:].reshape(2, n, 128)
    out_b = eng.forward(xb)
    dx_b = eng.backward(db)
    assert out_b.shape == dx_b.shape == (2, n, 128) and torch.equal(out_b[1], run["out"][-n:]) and torch.equal(dx_b[1], run["dx"][-n:])


@pytest.mark.parametrize("lengths", [(1024, 1024), (1100, 1000)])
def test_engine_weight_gradients_summed_over_row_chunks(dev, hip_lib, lengths):
    """from 2,048 rows on the weight gradients run as row chunks in the batch dimension of one GEMM: 2,048 rows are two chunks of
    1,024, 2,100 rows two of 1,048 and a rest of 4 (the fixture's cases have 367 and 531 rows: one call).  Against the float64
    restatement fed the GPU's ReLU pattern; bar: 4 x the float32 restatement's deviation, floor 4 x 2^-23.  Two runs agree bitwise
    but for the two bias gradients (pfpp_colsum)."""
    from pfpp_hip.matching_transformer_train import DW_CHUNK_ROWS, CrossAttentionTrainEngine

    N = sum(lengths)
    assert N // DW_CHUNK_ROWS == 2
    rng = np.random.default_rng([71, N])
    x = (0.5 * rng.normal(size=(N, 128))).astype(np.float32)
    dout = rng.normal(size=(N, 128)).astype(np.float32)
    eng = CrossAttentionTrainEngine(shared_layer(dev))
    xd, dd = torch.from_numpy(x).to(dev), torch.from_numpy(dout).to(dev)
    eng.forward(xd, lengths)
    dx = eng.backward(dd)
    grads = {k: p.grad.clone() for k, p in eng.params.items()}
    mask = (eng.saved["h"] > 0).cpu().numpy()
    sd = base.cross_state_dict()
    r64, r32 = cases.cross_train_restate(sd, x, lengths, dout, torch.float64), cases.cross_train_restate(sd, x, lengths, dout, torch.float32)
    pre = r64["pre"].numpy()
    differ = mask != (pre > 0)
    n_diff, worst_pre = int(differ.sum()), float(np.abs(pre[differ]).max()) if differ.any() else 0.0
    print(f"{N} rows: the GPU's ReLU pattern differs from float64's own in {n_diff} of {mask.size} entries (allowed {mask.size // 10000}), "
          f"largest float64 |pre-activation| among them {worst_pre:.3g} (allowed 1e-4)")
    assert n_diff <= mask.size // 10000 and worst_pre < 1e-4
    want = r64 if n_diff == 0 else cases.cross_train_restate(sd, x, lengths, dout, torch.float64, relu_mask=mask)
    failed = []
    for key in cases.TENSORS:
        got = dx if key == "dx" else grads[key]
        dev_ref = rel(r32[key].double().numpy(), r64[key].numpy())
        err, bar = rel(got.cpu().numpy(), want[key].numpy()), bar_of(dev_ref)
        print(f"{N} rows {key}: {err:.3g} of the maximum (float32 restatement {dev_ref:.3g}, bar {bar:.3g})")
        if err > bar:
            failed.append(key)
    assert not failed, failed
    eng.forward(xd, lengths)
    assert torch.equal(eng.backward(dd), dx)
    assert all(torch.equal(grads[k], p.grad) for k, p in eng.params.items() if k not in ("pos_ffn.w_1.bias", "pos_ffn.w_2.bias"))


# ------------------------------------------------------------------------------------------------ Adam
def test_optimizer_step_is_adam_and_the_next_forward_uses_the_new_weights(dev, hip_lib):
    """two steps against float64 Adam on the GPU's own gradients, bar 2^-23 |p| + 8e-6 lr; the module's pack is
    rebuilt: the next forward equals a fresh module's that was loaded with the stepped weights"""
    from pfpp_hip.matching_transformer_train import CrossAttentionTrainEngine

    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    layer = fresh_layer(dev)
    eng = CrossAttentionTrainEngine(layer)
    x, puz, dout = cases.case_inputs("tiny")
    xd, dd = torch.from_numpy(x).to(dev), torch.from_numpy(dout.astype(np.float32)).to(dev)
    p64 = {k: p.detach().cpu().double().clone() for k, p in eng.params.items()}
    m64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    v64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    outs = []
    for step in (1, 2):
        outs.append(eng.forward(xd, puz).clone())
        eng.backward(dd)
        pack_before = layer._packed()
        eng.optimizer_step(lr, (b1, b2), eps)
        assert layer._packed() is not pack_before
        worst = 0.0
        for k, p in eng.params.items():
            g = p.grad.detach().cpu().double()
            m64[k] = b1 * m64[k] + (1 - b1) * g
            v64[k] = b2 * v64[k] + (1 - b2) * g * g
            p64[k] = p64[k] - lr * (m64[k] / (1 - b1 ** step)) / ((v64[k] / (1 - b2 ** step)).sqrt() + eps)
            err = (p.detach().cpu().double() - p64[k]).abs()
            bar = 2.0 ** -23 * p64[k].abs() + 8e-6 * lr
            worst = max(worst, float((err / bar).max()))
            assert bool((err <= bar).all()), k
            p64[k] = p.detach().cpu().double().clone()       # the next step starts from the GPU's float32 parameters
        print(f"Adam step {step}: worst error / bar over the 12 parameters {worst:.3g}")
    assert not torch.equal(outs[0], outs[1])
    other = fresh_layer(dev)
    other.load_state_dict(layer.state_dict(), strict=True)
    assert torch.equal(eng.forward(xd, puz), other(xd, puz))


# ------------------------------------------------------------------------------------------------ the chain with the head
def test_chain_with_the_heads_loss_runs_both_backwards(dev, hip_lib):
    """loss = MatchingHeadLoss(CrossAttentionFunction(x)): x.grad is cross_engine.backward of the d_part_feats the head's engine returned
    in that application, bit for bit, and both sets of parameters carry gradients.  The head's fixtures have other layouts than `pair`
    (two puzzles of 180 points), so the labels are given directly"""
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_train import MatchingHeadLoss, MatchingHeadTrainEngine
    from pfpp_hip.matching_transformer_train import CrossAttentionFunction, CrossAttentionTrainEngine

    head_cases = load_cases("matching_train_cases")
    head = MatchingHead()
    head.load_state_dict(tensors(head_cases.head_state_dict()), strict=True)
    head_eng = MatchingHeadTrainEngine(head.to(dev), w_cls_loss=1.0, w_mat_loss=1.0)
    cross_eng = CrossAttentionTrainEngine(shared_layer(dev))
    pts, x, _, puz = base.case_arrays("pair")
    pieces = base.CASES["pair"]
    n_pcs = np.zeros((2, 20), dtype=np.int64)
    valids = np.zeros((2, 20), dtype=np.float32)
    for b, lens in enumerate(pieces):
        n_pcs[b, :len(lens)], valids[b, :len(lens)] = lens, 1
    label = (np.random.default_rng(67).uniform(size=len(x)) < 0.25).astype(np.int64)
    lo = 0
    for lens in pieces:                                          # every piece of four or more points gets a critical point
        for n in lens:
            if n >= 4:
                label[lo] = 1
            lo += n
    gt, lab = torch.from_numpy(pts).to(dev), torch.from_numpy(label).to(dev)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    mid = CrossAttentionFunction.apply(xd, cross_eng, puz)
    mid.retain_grad()
    loss = MatchingHeadLoss.apply(mid, head_eng, gt, n_pcs, valids, None, lab)
    assert torch.equal(mid.detach(), shared_layer(dev)(xd.detach(), puz)) and bool(torch.isfinite(loss))
    loss.backward()
    d_part_feats = mid.grad.clone()                              # what loss_and_grads returned in this application (times 1)
    assert xd.grad is not None and xd.grad.shape == xd.shape and d_part_feats.shape == (len(x), 128)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in list(cross_eng.params.values()) + list(head_eng.params.values()))
    g_chain = {k: p.grad.clone() for k, p in cross_eng.params.items()}
    dx = cross_eng.backward(d_part_feats)
    print(f"chain on pair: loss {float(loss.detach()):.6g}, max |d_part_feats| {float(d_part_feats.abs().max()):.3g}, max |x.grad| {float(xd.grad.abs().max()):.3g}")
    assert torch.equal(xd.grad, dx) and float(xd.grad.abs().max()) > 0
    # the parameter gradients likewise; the two bias gradients go through pfpp_colsum, which adds its row blocks' sums in the order
    # they finish: equal to the order of those additions, as the head's gradients are (2e-6 of the maximum, tests/test_gpu_matching_train.py)
    for k, p in cross_eng.params.items():
        if k in ("pos_ffn.w_1.bias", "pos_ffn.w_2.bias"):
            assert float((g_chain[k] - p.grad).abs().max()) <= 2e-6 * float(p.grad.abs().max()), k
        else:
            assert torch.equal(g_chain[k], p.grad), k
    # a second head step on the same descriptors gives that gradient again, to the order of its BatchNorm reductions
    again = head_eng.loss_and_grads(mid.detach(), gt, n_pcs, valids, critical_label=lab)[1]
    assert float((again - d_part_feats).abs().max()) <= 2e-6 * float(d_part_feats.abs().max())
