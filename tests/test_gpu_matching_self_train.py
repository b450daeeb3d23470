"""GPU: the training step of the matcher's point-transformer layer (csrc/matching_ptf_train.hip, pfpp_hip/matching_transformer_train.py)
against the float64 restatement of tests/matching_self_train_cases.py, which tests/test_matching_self_train_host.py pins to 1e-12 to
tests/golden/matching_self_train.npz (the reference's own layer in .train() under autograd).  Every test prints the figures it measured
before it asserts.

The reference of record is the float64 restatement fed the GPU's own three ReLU patterns (pre_dump).  Bars (the rule of
5.7 and 5.8): per tensor 4 x the reference's own float32-against-float64 deviation relative to the tensor's largest magnitude, floor
4 x 2^-23; the deviation comes from the fixture on `tiny` and `pair`, from a float32 torch evaluation of the same restatement elsewhere.
The GPU's patterns may differ from the float64 restatement's own signs in at most 1 entry per 10,000 per ReLU (a condition).
linear_p.0.bias and linear_w.2.bias get exact zeros.  linear_q.bias and linear_w.5.bias vanish in exact arithmetic as well (ZERO_SUMS of
the case file): their float64 value is ~1e-14, and what the engine returns is the rounding of a sum, so their bar is 4 x 2^-23 of the
sum of the |terms| of the worst channel, which the restatement reports; linear_k.bias is a third such sum where no slot is padded."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FLOOR = 4.0 * 2.0 ** -23
COLSUM = ("linear_q.bias", "linear_k.bias", "linear_v.bias")         # through pfpp_colsum: two runs agree to rounding, not bitwise


def load_cases(stem):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases("matching_self_train_cases")
base = cases.base
_RUN, _REF = {}, {}


def rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def fresh_layer(dev, sd=None):
    from pfpp_hip.matching_transformer import PointTransformerLayer

    layer = PointTransformerLayer(128, 128, 8, 16)
    layer.load_state_dict(tensors(base.ptf_state_dict()) if sd is None else sd, strict=True)
    return layer.to(dev)


def step(dev, p, x, lengths, dout, indices=None):
    """one forward + backward of a fresh layer and engine with both pre_dumps -> everything the tests compare, on the host"""
    from pfpp_hip.matching_transformer_train import PointTransformerTrainEngine

    layer = fresh_layer(dev)
    eng = PointTransformerTrainEngine(layer)
    d = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    ind = None if indices is None else tuple(d(i, torch.int32) for i in indices)
    out = eng.forward(d(p), d(x), lengths, indices=ind, pre_dump=True)
    dx = eng.backward(d(dout), pre_dump=True)
    torch.cuda.synchronize()
    got = {"out": out.cpu().numpy(), "dx": dx.cpu().numpy(), "dqkv": eng.saved["dqkv"].cpu().numpy(),
           "idx": (eng.saved["idx_k"].cpu().numpy(), eng.saved["idx_v"].cpu().numpy()),
           "pre": [a.cpu().numpy() for a in eng.saved["pre"]], "pre_bwd": [a.cpu().numpy() for a in eng.saved["pre_bwd"]],
           "num_batches_tracked": [int(b.num_batches_tracked) for b in eng.bns], "engine": eng, "layer": layer}
    got.update({k: v.grad.cpu().numpy() for k, v in eng.params.items()})
    got.update({k: v.cpu().numpy() for k, v in layer.named_buffers() if not k.endswith("num_batches_tracked")})
    return got


def fixture_lists(golden, name):
    g = golden("matching_transformer")
    return g[f"{name}_idx_k"].astype(np.int64), g[f"{name}_idx_v"].astype(np.int64)


def case_run(dev, golden, name, own_search=False):
    key = (name, own_search)
    if key not in _RUN:
        p, x, lengths, dout = cases.case_inputs(name)
        _RUN[key] = step(dev, p, x, lengths, dout.astype(np.float32), None if own_search else fixture_lists(golden, name))
    return _RUN[key]


def case_ref(golden, name, masks_key, masks):
    """the float64 restatement of a case on the fixture's lists with the given masks (None: its own signs); computed once per pattern"""
    key = (name, masks_key)
    if key not in _REF:
        p, x, _, dout = cases.case_inputs(name)
        _REF[key] = cases.self_train_restate(base.ptf_state_dict(), p, x, dout.astype(np.float32), fixture_lists(golden, name), torch.float64, masks)
    return _REF[key]


def flips(got, own):
    """per ReLU: how many signs of the GPU's pre_dump differ from the float64 restatement's own, and the cap of 1 per 10,000"""
    n = [int(((a > 0) != (b.numpy() > 0)).sum()) for a, b in zip(got["pre"], own["pre"])]
    return n, [a.size // 10000 for a in got["pre"]]


def check(tag, got, want, devs, keys):
    """print error / deviation / bar per tensor, then assert; devs: key -> the reference's own float32 deviation"""
    failed = []
    for key in keys:
        if key in cases.ZERO_GRADS:
            zero = not got[key].any()
            print(f"{tag} {key}: exact zeros: {zero}")
            if not zero:
                failed.append(key)
            continue
        if key in cases.ZERO_SUMS or (key == "linear_k.bias" and want["padded_slots"] == 0):
            scale = want["zero_sum_scale"][key]
            err = float(np.abs(got[key]).max() / scale)
            print(f"{tag} {key}: {err:.3g} of the sum of the |terms| {scale:.4g} (vanishes in exact arithmetic; bar {FLOOR:.3g})")
            if err > FLOOR:
                failed.append(key)
            continue
        err, bar = rel(got[key], want[key].numpy()), max(4.0 * devs[key], FLOOR)
        print(f"{tag} {key}: {err:.3g} of the maximum (reference float32 {devs[key]:.3g}, bar {bar:.3g})")
        if not (err <= bar):
            failed.append(key)
    assert not failed, failed


def check_case(golden, name, got, tag):
    g = golden("matching_self_train")
    own = case_ref(golden, name, "own", None)
    n, cap = flips(got, own)
    print(f"{tag}: the GPU's ReLU patterns differ from float64's own in {n} entries (allowed {cap})")
    assert all(a <= b for a, b in zip(n, cap))
    masks = [a > 0 for a in got["pre"]]
    want = own if not any(n) else case_ref(golden, name, tag, masks)
    assert all(np.array_equal(a, b) for a, b in zip(got["pre"], got["pre_bwd"])), "the backward thresholds other bits than the forward"
    devs = {k: float(g[f"{name}_{k}_refdev"]) for k in cases.TENSORS}
    check(tag, got, want, devs, cases.TENSORS)
    assert got["num_batches_tracked"] == [want["num_batches_tracked"]] * 3


# ------------------------------------------------------------------------------------------------ 1, 2, 3: the fixture's cases
@pytest.mark.parametrize("name", ["tiny", "pair"])
def test_step_on_the_fixtures_lists(dev, hip_lib, golden, name):
    check_case(golden, name, case_run(dev, golden, name), f"{name} (fixture lists)")


@pytest.mark.parametrize("name", ["tiny", "pair"])
def test_step_with_the_engines_own_searches(dev, hip_lib, golden, name):
    got = case_run(dev, golden, name, own_search=True)
    want_k, want_v = fixture_lists(golden, name)
    assert np.array_equal(got["idx"][0], want_k) and np.array_equal(got["idx"][1], want_v)
    check_case(golden, name, got, f"{name} (own searches)")


# ------------------------------------------------------------------------------------------------ 4, 5: other lists and launch sizes
def custom(dev, p, x, lengths, dout, indices, tag, keys=("out", "dqkv", "dx") + cases.GRAD_NAMES + cases.BUFFER_NAMES):
    """a step on inputs of the test's own: reference = the float64 restatement on the lists the GPU used and with the GPU's ReLU
    patterns, yardstick = the float32 torch evaluation of the same restatement -> (got, want)"""
    got = step(dev, p, x, lengths, dout, indices)
    sd = base.ptf_state_dict()
    own = cases.self_train_restate(sd, p, x, dout, got["idx"], torch.float64)
    r32 = cases.self_train_restate(sd, p, x, dout, got["idx"], torch.float32)
    n, cap = flips(got, own)
    print(f"{tag}: the GPU's ReLU patterns differ from float64's own in {n} entries (allowed {cap})")
    assert all(a <= max(b, 0) for a, b in zip(n, cap))
    want = own if not any(n) else cases.self_train_restate(sd, p, x, dout, got["idx"], torch.float64, [a > 0 for a in got["pre"]])
    devs = {k: rel(r32[k].double().numpy(), own[k].numpy()) for k in keys}
    check(tag, got, want, devs, keys)
    return got, want


def piece200():
    p, x, lengths, dout = cases.case_inputs("tiny")
    lo = int(lengths[:-1].sum())
    assert int(lengths[-1]) == 200
    return p[lo:], x[lo:], [200], dout[lo:].astype(np.float32)


def random_lists(seed, N):
    rng = np.random.default_rng([47, seed])
    return [np.stack([rng.permutation(N)[:16] for _ in range(N)]).astype(np.int32) for _ in range(2)]


def test_a_row_in_every_list(dev, hip_lib):
    p, x, lengths, dout = piece200()
    ik, iv = random_lists(0, 200)
    for i in (ik, iv):
        i[i == 7] = 9
    ik[:, 3], iv[:, 5] = 7, 7                                  # in-degree 200: more than a wave
    got, _ = custom(dev, p, x, lengths, dout, (ik, iv), "row 7 in all 200 lists", keys=("dqkv", "dx", "out"))
    assert int((got["idx"][0] == 7).sum()) == 200 and int((got["idx"][1] == 7).sum()) == 200


def test_a_row_in_no_list_gets_zeros_over_a_sentinel(dev, hip_lib):
    from pfpp_hip.matching_transformer_train import inverse_lists, ptf_train_bwd_gather

    p, x, lengths, dout = piece200()
    ik, iv = random_lists(1, 200)
    for i in (ik, iv):
        i[i == 11] = 12
    got, _ = custom(dev, p, x, lengths, dout, (ik, iv), "row 11 in no list", keys=("dqkv", "dx"))
    assert not got["dqkv"][11, 128:].any() and got["dqkv"][11, :128].any()
    s = got["engine"].saved
    filled = torch.full_like(s["dqkv"], 7.5)
    ptf_train_bwd_gather(torch.from_numpy(dout).to(dev), s["w"], s["du"], s["qkv"], s["p"], s["tw"], *inverse_lists(s["idx_k"]), *inverse_lists(s["idx_v"]), filled)
    assert bool((filled[:, :128] == 7.5).all()) and not bool(filled[11, 128:].any())
    assert torch.equal(filled[:, 128:], s["dqkv"][:, 128:])


def test_the_two_lists_are_not_interchangeable(dev, hip_lib):
    p, x, lengths, dout = piece200()
    ik, iv = random_lists(2, 200)
    got, want = custom(dev, p, x, lengths, dout, (ik, iv), "idx_k != idx_v", keys=("dqkv", "dx", "out"))
    swapped = step(dev, p, x, lengths, dout, (iv, ik))
    for key in ("out", "dx"):
        err = rel(swapped[key], want[key].numpy())
        print(f"swapped lists, {key}: {err:.3g} of the maximum of the unswapped result")
        assert err > 1e-2


@pytest.mark.parametrize("lengths", [[1, 2, 3], [1000, 150]])
def test_small_and_large_launches(dev, hip_lib, lengths):
    """6 points: 82 of the 96 slots padded (1 + 4 + 9 = 14 are not), fewer points than any grid.  1,150 points: more than the 1,024 workgroups of the point
    passes (some walk two points), several partials per slice of the fold"""
    N = sum(lengths)
    rng = np.random.default_rng([53, N])
    p = np.concatenate([rng.normal(0, 0.5, 3) + 0.2 * rng.normal(size=(n, 3)) for n in lengths]).astype(np.float32)
    x = (np.sin(p.astype(np.float64) @ rng.normal(0, 3.0, (3, 128))) + 0.3 * rng.normal(size=(N, 128))).astype(np.float32)
    dout = rng.normal(size=(N, 128)).astype(np.float32)
    got, _ = custom(dev, p, x, lengths, dout, None, f"{N} points in {lengths}")
    pads = int((got["idx"][0] == N).sum())
    assert pads == (82 if N == 6 else 0) and got["num_batches_tracked"] == [1, 1, 1]


# ------------------------------------------------------------------------------------------------ 6: reproducibility
def test_two_runs_agree_bitwise_and_the_backward_is_linear_in_powers_of_two(dev, hip_lib, golden):
    a = case_run(dev, golden, "pair")
    p, x, lengths, dout = cases.case_inputs("pair")
    lists = fixture_lists(golden, "pair")
    b = step(dev, p, x, lengths, dout.astype(np.float32), lists)
    exact = ("out", "dx", "dqkv") + tuple(k for k in cases.GRAD_NAMES if k not in COLSUM) + cases.BUFFER_NAMES
    differ = [k for k in exact if not np.array_equal(a[k], b[k])]
    print(f"two runs of pair: tensors that differ in a bit: {differ}")
    assert not differ
    for k in COLSUM[1:]:
        assert float(np.abs(a[k] - b[k]).max()) <= 2e-6 * float(np.abs(a[k]).max()), k
    eng = b["engine"]
    for e in (-10, 10):
        dx = eng.backward(torch.from_numpy(dout.astype(np.float32) * 2.0 ** e).to(dev)).cpu().numpy()
        differ = [k for k in ("dx",) + tuple(k for k in cases.GRAD_NAMES if k not in COLSUM)
                  if not np.array_equal((dx if k == "dx" else eng.params[k].grad.cpu().numpy()), b[k] * np.float32(2.0 ** e))]
        print(f"backward(2^{e} dout) against 2^{e} backward(dout): tensors that differ in a bit: {differ}")
        assert not differ


# ------------------------------------------------------------------------------------------------ 7: Adam
def test_optimizer_step_is_adam_and_the_eval_forward_uses_the_new_weights_and_buffers(dev, hip_lib, golden):
    """two steps against float64 Adam on the GPU's own gradients, bar 2^-23 |p| + 8e-6 lr; the module's eval pack is
    rebuilt: its eval forward equals a fresh module's that was loaded with the stepped weights and the moved buffers"""
    from pfpp_hip.matching_transformer_train import PointTransformerTrainEngine

    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    layer = fresh_layer(dev)
    eng = PointTransformerTrainEngine(layer)
    p, x, lengths, dout = cases.case_inputs("tiny")
    pd, xd, dd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (p, x, dout))
    p64 = {k: v.detach().cpu().double().clone() for k, v in eng.params.items()}
    m64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    v64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    outs, evals = [], [layer(pd, xd, lengths).clone()]
    for n in (1, 2):
        outs.append(eng.forward(pd, xd, lengths).clone())
        eng.backward(dd)
        pack_before = layer._packed()
        eng.optimizer_step(lr, (b1, b2), eps)
        assert layer._packed() is not pack_before
        worst = 0.0
        for k, v in eng.params.items():
            g = v.grad.detach().cpu().double()
            m64[k] = b1 * m64[k] + (1 - b1) * g
            v64[k] = b2 * v64[k] + (1 - b2) * g * g
            p64[k] = p64[k] - lr * (m64[k] / (1 - b1 ** n)) / ((v64[k] / (1 - b2 ** n)).sqrt() + eps)
            err = (v.detach().cpu().double() - p64[k]).abs()
            bar = 2.0 ** -23 * p64[k].abs() + 8e-6 * lr
            worst = max(worst, float((err / bar).max()))
            assert bool((err <= bar).all()), k
            p64[k] = v.detach().cpu().double().clone()       # the next step starts from the GPU's float32 parameters
        print(f"Adam step {n}: worst error / bar over the 20 parameters {worst:.3g}")
        evals.append(layer(pd, xd, lengths).clone())
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(evals[0], evals[1]) and not torch.equal(evals[1], evals[2])
    assert [int(b.num_batches_tracked) for b in eng.bns] == [2, 2, 2]
    other = fresh_layer(dev, layer.state_dict())
    assert torch.equal(layer(pd, xd, lengths), other(pd, xd, lengths))


# ------------------------------------------------------------------------------------------------ 8: the chain of the three engines
def test_chain_of_the_three_functions(dev, hip_lib, golden):
    """loss = MatchingHeadLoss(CrossAttentionFunction(PointTransformerFunction(p, x))) on `pair`: x.grad is, bit for bit, the three
    engines called by hand on the gradients of that application.  The chain that starts at tf_cross1's input, on the same descriptors,
    gives the same forward and loss bit for bit.  Its gradients pass through a second step of the head, whose gradients two runs repeat
    only to the order of its atomic reductions (tests/test_gpu_matching_train.py: 2e-6 of the maximum; on the MI355X one head bias
    differed in a bit in each of two runs, a different one each time, and d_part_feats in none): where the head hands tf_cross1 the same bits, tf_cross1's
    gradients and input gradient are asserted bit for bit (but for its two pfpp_colsum biases), otherwise to that bound"""
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_train import MatchingHeadLoss, MatchingHeadTrainEngine
    from pfpp_hip.matching_transformer import CrossAttentionLayer
    from pfpp_hip.matching_transformer_train import (CrossAttentionFunction, CrossAttentionTrainEngine, PointTransformerFunction,
                                                     PointTransformerTrainEngine)

    head_cases = load_cases("matching_train_cases")
    head = MatchingHead()
    head.load_state_dict(tensors(head_cases.head_state_dict()), strict=True)
    head_eng = MatchingHeadTrainEngine(head.to(dev), w_cls_loss=1.0, w_mat_loss=1.0)
    cross = CrossAttentionLayer(128, 8)
    cross.load_state_dict(tensors(base.cross_state_dict()), strict=True)
    cross_eng = CrossAttentionTrainEngine(cross.to(dev))
    self_eng = PointTransformerTrainEngine(fresh_layer(dev))
    pts, x, lengths, puz = base.case_arrays("pair")
    pieces = base.CASES["pair"]
    n_pcs, valids = np.zeros((2, 20), dtype=np.int64), np.zeros((2, 20), dtype=np.float32)
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
    mid0 = PointTransformerFunction.apply(gt, xd, self_eng, lengths)
    mid0.retain_grad()
    mid1 = CrossAttentionFunction.apply(mid0, cross_eng, puz)
    mid1.retain_grad()
    loss = MatchingHeadLoss.apply(mid1, head_eng, gt, n_pcs, valids, None, lab)
    assert bool(torch.isfinite(loss))
    loss.backward()
    assert xd.grad is not None and xd.grad.shape == xd.shape and float(xd.grad.abs().max()) > 0
    g_self = {k: v.grad.clone() for k, v in self_eng.params.items()}
    g_cross = {k: v.grad.clone() for k, v in cross_eng.params.items()}
    g_head = {k: v.grad.clone() for k, v in head_eng.params.items()}
    d_part_feats, d_mid0 = mid1.grad.clone(), mid0.grad.clone()
    by_hand = cross_eng.backward(d_part_feats)
    dx = self_eng.backward(by_hand)
    print(f"chain on pair: loss {float(loss.detach()):.6g}, max |d_part_feats| {float(d_part_feats.abs().max()):.3g}, max |d tf_self1 out| "
          f"{float(d_mid0.abs().max()):.3g}, max |x.grad| {float(xd.grad.abs().max()):.3g}")
    assert torch.equal(by_hand, d_mid0) and torch.equal(xd.grad, dx)
    assert all(torch.equal(g_self[k], v.grad) for k, v in self_eng.params.items() if k not in COLSUM)
    # the chain that starts at tf_cross1's input, on the same descriptors
    start = mid0.detach().clone().requires_grad_(True)
    mid2 = CrossAttentionFunction.apply(start, cross_eng, puz)
    mid2.retain_grad()
    loss2 = MatchingHeadLoss.apply(mid2, head_eng, gt, n_pcs, valids, None, lab)
    loss2.backward()
    diff_head = [k for k, v in head_eng.params.items() if not torch.equal(g_head[k], v.grad)]
    diff_cross = [k for k, v in cross_eng.params.items() if not torch.equal(g_cross[k], v.grad)]
    head_repeats = torch.equal(mid2.grad, d_part_feats)
    print(f"chain from tf_cross1's input: loss equal bitwise: {torch.equal(loss.detach(), loss2.detach())}; d_part_feats equal bitwise: "
          f"{head_repeats}; head gradients that differ in a bit: {diff_head}; cross gradients that differ in a bit: {diff_cross}")
    assert torch.equal(mid2.detach(), mid1.detach()) and torch.equal(loss.detach(), loss2.detach())
    near = lambda a, c: float((a - c).abs().max()) <= 2e-6 * float(c.abs().max())
    assert all(near(v.grad, g_head[k]) for k, v in head_eng.params.items()) and near(mid2.grad, d_part_feats)
    if head_repeats:                                             # the head handed tf_cross1 the same bits: so does everything below it
        assert not [k for k in diff_cross if k not in ("pos_ffn.w_1.bias", "pos_ffn.w_2.bias")] and torch.equal(start.grad, d_mid0)
    assert all(near(v.grad, g_cross[k]) for k, v in cross_eng.params.items()) and near(start.grad, d_mid0)
