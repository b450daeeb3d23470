"""GPU: the DGCNN encoder's training step (csrc/dgcnn_train.hip, pfpp_hip/matching_dgcnn_train.py) against (a)
tests/golden/matching_dgcnn_train.npz, written by tools/make_matching_dgcnn_train_goldens.py from the reference's own module in
.train(), and (b) the restatements of tests/matching_dgcnn_train_cases.py, which tests/test_matching_dgcnn_train_host.py pins to that
fixture.  Every test prints the figures it measured before it asserts.

Bars.  The statistics pass: e and the winner bit for bit the numpy restatement; the sums against numpy float64 of the
same fp32 z to 1e-12.  Floats elsewhere: the fixture records per tensor the deviation of the reference's own fp32 run from its float64
run relative to the tensor's largest magnitude; the bar is 4 x that, with a floor of 4 x 2^-23.  The gathers take the bar of the
gradient of their level's convolution weight (the smaller of the two fixture cases), which is what du and dv become."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FLOOR = 4.0 * 2.0 ** -23
ACTS = ("x1", "x2", "x3", "x4", "out")


def load_cases(stem="matching_dgcnn_train_cases"):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_STEP = {}


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def fresh_encoder(dev):
    from pfpp_hip.matching_dgcnn import DGCNNDynamic

    enc = DGCNNDynamic(cases.FEAT, False, 3)
    enc.load_state_dict(tensors(cases.state_dict()), strict=True)
    return enc.to(dev)


def bar_of(g, name, key):
    return max(4.0 * float(g[f"{name}_{key}_refdev"]), FLOOR)


def engine_step(name, dev):
    """one forward + backward of the engine on a fixture case from the case file's state, computed once: what it returned and kept"""
    if name not in _STEP:
        from pfpp_hip.matching_dgcnn_train import DGCNNTrainEngine

        enc = fresh_encoder(dev)
        eng = DGCNNTrainEngine(enc)
        x, lengths = cases.case_arrays(name)
        out = eng.forward(torch.from_numpy(x).to(dev), lengths, keep_activations=True)
        eng.backward(torch.from_numpy(cases.dout_array(name)).to(dev))
        torch.cuda.synchronize()
        lv = eng.saved["levels"]
        _STEP[name] = {"out": out.cpu().numpy(), "x": [l["x"].cpu().numpy() for l in lv], "knn": [l["idx"].cpu().numpy().astype(np.int64) for l in lv],
                       "winner": [l["winner"].cpu().numpy().astype(np.int64) for l in lv],
                       "grads": {k: p.grad.cpu().numpy() for k, p in eng.params.items()},
                       "buffers": {k: b.cpu().numpy() for k, b in enc.named_buffers() if not k.endswith("num_batches_tracked")},
                       "tracked": [int(getattr(enc, f"bn{l}").num_batches_tracked) for l in range(1, 6)]}
    return _STEP[name]


# ------------------------------------------------------------------------------------------------ the statistics and extremum pass
@pytest.mark.parametrize("c_out", [64, 128, 256])
def test_statistics_pass_matches_the_restatement_bit_for_bit(dev, hip_lib, c_out):
    from pfpp_hip.matching_dgcnn_train import dgcnn_bn_leaky_apply, dgcnn_edge_stats

    uv, idx, gamma, beta = cases.stats_case(c_out)
    N = len(uv)
    rm0 = np.linspace(-0.3, 0.3, c_out).astype(np.float32)
    rv0 = np.linspace(0.5, 1.5, c_out).astype(np.float32)
    rm, rv = torch.from_numpy(rm0.copy()).to(dev), torch.from_numpy(rv0.copy()).to(dev)
    v0 = rm._version
    e, w, coef, sums = dgcnn_edge_stats(torch.from_numpy(uv).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(gamma).to(dev),
                                        torch.from_numpy(beta).to(dev), cases.BN_EPS, cases.MOMENTUM, rm, rv, c_out=c_out, want_sums=True)
    x = dgcnn_bn_leaky_apply(e, coef)
    torch.cuda.synchronize()
    e_w, w_w, z = cases.stats_extremum_f32(uv, idx, gamma)
    e, w, coef, sums = e.cpu().numpy(), w.cpu().numpy(), coef.cpu().numpy(), sums.cpu().numpy()
    bad_e, bad_w = int((e.view(np.uint32) != e_w.view(np.uint32)).sum()), int((w != w_w).sum())
    print(f"C = {c_out}, N = {N}: {bad_e} extremum entries and {bad_w} winners differ from the restatement; gamma < 0 / == 0 / > 0: "
          f"{int((gamma < 0).sum())} / {int((gamma == 0).sum())} / {int((gamma > 0).sum())}; padded winners {int((np.take_along_axis(idx, w_w.astype(np.int64), 1) == N).sum())}")
    assert e.dtype == np.float32 and w.dtype == np.uint8 and bad_e == 0 and bad_w == 0
    assert (w[12][(np.arange(c_out) % 2 == 0) & (gamma >= 0)] == 0).all()                      # the tie: the first slot
    z64 = z.astype(np.float64).reshape(-1, c_out)
    R = z64.shape[0]
    s_w, q_w, abs_w = z64.sum(0), (z64 * z64).sum(0), np.abs(z64).sum(0)
    err_s, err_q = float((np.abs(sums[0] - s_w) / abs_w).max()), float((np.abs(sums[1] - q_w) / q_w).max())
    print(f"sum z: {err_s:.3g} of sum |z|; sum z^2: {err_q:.3g} of itself (bars 1e-12)")
    assert R == 20 * N and err_s <= 1e-12 and err_q <= 1e-12
    mean = s_w / R
    var = q_w / R - mean * mean
    rstd = 1.0 / np.sqrt(var + cases.BN_EPS)
    a64 = gamma.astype(np.float64) * rstd
    want = {"a": a64, "b": beta - mean * a64.astype(np.float32).astype(np.float64), "mean": mean, "rstd": rstd}
    for i, k in enumerate(want):
        err = float(np.abs(coef[i] - want[k]).max() / np.abs(want[k]).max())
        print(f"coef {k}: {err:.3g} of the maximum (bar 2^-23)")
        assert err <= 2.0 ** -23
    rm_w = (1 - cases.MOMENTUM) * rm0.astype(np.float64) + cases.MOMENTUM * mean
    rv_w = (1 - cases.MOMENTUM) * rv0.astype(np.float64) + cases.MOMENTUM * var * R / (R - 1)
    err_m, err_v = float(np.abs(rm.cpu().numpy() - rm_w).max() / np.abs(rm_w).max()), float(np.abs(rv.cpu().numpy() - rv_w).max() / np.abs(rv_w).max())
    print(f"running_mean {err_m:.3g}, running_var {err_v:.3g} of the maximum against the float64 sums (bar 2^-23)")
    assert err_m <= 2.0 ** -23 and err_v <= 2.0 ** -23 and rm._version > v0
    assert np.array_equal(x.cpu().numpy().view(np.uint32), cases.apply_f32(e, coef[0], coef[1]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ the backward gathers
@pytest.mark.parametrize("level", [1, 3, 4])
def test_backward_gathers_match_the_float64_restatement(dev, hip_lib, golden, level):
    """C = 64, 128, 256 on lists with pieces of 1, 3, 20, 21, 65 points and a star of 130 whose centre sits in 130 lists"""
    from pfpp_hip.matching_dgcnn_train import (dgcnn_bn_leaky_bwd, dgcnn_edge_bwd_du, dgcnn_edge_bwd_dv, dgcnn_edge_stats, dgcnn_inverse_lists)

    g = golden("matching_dgcnn_train")
    C_ = cases.WIDTHS[level - 1]
    bar = min(bar_of(g, n, f"grad_conv{level}.0.weight") for n in ("tiny", "small"))
    idx = cases.gather_lists()
    N = len(idx)
    rng = np.random.default_rng([level, 31])
    uv = rng.standard_normal((N, 2 * C_)).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, C_) * np.where(rng.random(C_) < 0.3, -1.0, 1.0)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C_)).astype(np.float32)
    g1, g2 = rng.standard_normal((N, C_)).astype(np.float32), rng.standard_normal((N, C_)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    uv_d, idx_d = t(uv), t(idx)
    e, w, coef = dgcnn_edge_stats(uv_d, idx_d, t(gamma), t(beta), cases.BN_EPS, c_out=C_)
    wide = torch.zeros((N, 2 * C_), dtype=torch.float32, device=dev)
    wide[:, C_:] = t(g1)                                                                   # a column slice of a wider tensor, as in the engine
    h, dgamma, dbeta, means = dgcnn_bn_leaky_bwd(e, wide[:, C_:], coef, g2=t(g2), count=20 * N)
    off, ent = dgcnn_inverse_lists(idx_d)
    duv = torch.full((N, 2 * C_), float("nan"), dtype=torch.float32, device=dev)
    dgcnn_edge_bwd_dv(uv_d, idx_d, w, h, coef, means, c_out=C_, duv=duv)
    dgcnn_edge_bwd_du(uv_d, off, ent, w, h, coef, means, c_out=C_, duv=duv)
    torch.cuda.synchronize()
    off_h = off.cpu().numpy()
    lens = np.diff(off_h)
    assert lens.max() == 130 and lens.min() == 1 and off_h[-1] == int((idx != N).sum()) and ent.numel() == 20 * N
    # the float64 restatement on the same uv, lists and winners
    uv64 = torch.from_numpy(uv).double()
    fw = cases.level_forward(uv64, idx.astype(np.int64), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), cases.BN_EPS,
                             winner=w.cpu().numpy())
    bw = cases.level_backward(uv64, idx.astype(np.int64), fw, torch.from_numpy(g1.astype(np.float32) + g2.astype(np.float32)).double())
    got = {"du": duv[:, :C_].cpu().numpy(), "dv": duv[:, C_:].cpu().numpy(), "dgamma": dgamma.cpu().numpy(), "dbeta": dbeta.cpu().numpy()}
    padded = int((np.take_along_axis(idx.astype(np.int64), fw["winner"], 1) == N).sum())
    print(f"level {level} (C = {C_}), N = {N}: inverse lists of 1 .. {lens.max()} entries; {padded} entries won by a padded slot; bar {bar:.3g}")
    assert padded > 0
    for k, a in got.items():
        want = bw[k].numpy()
        err = float(np.abs(a - want).max() / np.abs(want).max())
        print(f"  {k}: {err:.3g} of the maximum")
        assert np.isfinite(a).all() and err <= bar


# ------------------------------------------------------------------------------------------------ conv5's LeakyReLU pieces
@pytest.mark.parametrize("rows,C_", [(2, 4), (2, 128), (65, 4), (65, 128)])
def test_conv5_leaky_apply_and_backward(dev, hip_lib, rows, C_):
    from pfpp_hip.matching_dgcnn_train import dgcnn_bn_leaky_apply, dgcnn_bn_leaky_bwd
    from pfpp_hip.matching_encoder_train import ragged_bn_stats

    rng = np.random.default_rng([rows, C_])
    y = rng.standard_normal((rows, C_)).astype(np.float32)
    g = rng.standard_normal((rows, C_)).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, C_) * np.where(rng.random(C_) < 0.3, -1.0, 1.0)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C_)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    y_d = t(y)
    coef = ragged_bn_stats(y_d, t(gamma), t(beta), cases.BN_EPS)
    out = dgcnn_bn_leaky_apply(y_d, coef)
    dy, dgamma, dbeta, _ = dgcnn_bn_leaky_bwd(y_d, t(g), coef, want_dy=True)
    torch.cuda.synchronize()
    c = coef.cpu().numpy()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), cases.apply_f32(y, c[0], c[1]).view(np.uint32))
    Y = torch.from_numpy(y).double().requires_grad_(True)
    G, B = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    o = torch.nn.functional.leaky_relu(torch.nn.functional.batch_norm(Y, None, None, G, B, True, 0.1, cases.BN_EPS), cases.SLOPE)
    (o * torch.from_numpy(g).double()).sum().backward()
    # y a + b = (y - mean) a + beta evaluated as one multiply and one add: its rounding is 2^-24 of the TERMS y a and mean a, which over
    # 2 rows (var as small as the two values are close, a up to gamma / sqrt(eps)) are far larger than the result; the bar is relative
    # to the largest term.  The bits themselves are pinned by the restatement above.
    top = max(float(np.abs(o.detach().numpy()).max()), float(np.abs(y.astype(np.float64) * c[0]).max()))
    err_o = float(np.abs(out.cpu().numpy() - o.detach().numpy()).max() / top)
    # the sign test runs on the fp32 pre-activation: an entry within rounding of 0 may fall the other way (none in these draws)
    pre = (y.astype(np.float64) * c[0] + c[1])
    assert np.abs(pre).min() > 1e-6
    print(f"rows = {rows}, C = {C_}: out {err_o:.3g} of the maximum")
    assert err_o <= 8.0 * 2.0 ** -23
    # a few fp32-rounded operations per element, against float64 autograd: 16 x 2^-23 of the tensor's maximum, or of the channel's
    # largest TERM where that is larger.  x_hat = (y - mean) rstd is formed from a mean that coef holds in fp32, so it carries
    # 2^-24 |mean| rstd: dgamma = sum h x_hat carries that times |dbeta|, and dy = a ((h - m1) - x_hat m2), whose own terms are of size
    # a g, carries it times a m2.  At 65 rows (rstd about 1) these scales are below the maxima; at 2 rows, where rstd reaches
    # 1 / sqrt(eps) and dy cancels to eps / (var + eps) of its terms, no fp32 evaluation passes relative to the result alone.
    amp = c[3] * np.abs(c[2])                                                               # rstd |mean| per channel
    scale = {"dy": np.abs(c[0]) * (np.abs(g).max(0) + amp * np.abs(G.grad.numpy()) / rows), "dgamma": amp * np.abs(B.grad.numpy()),
             "dbeta": np.zeros(C_)}
    for k, a, want in (("dy", dy, Y.grad), ("dgamma", dgamma, G.grad), ("dbeta", dbeta, B.grad)):
        top = np.maximum(np.abs(want.numpy()).max(), scale[k])
        err = float((np.abs(a.cpu().numpy() - want.numpy()) / top).max())
        print(f"  {k}: {err:.3g} of max(the maximum, the channel's largest term) (bar {16 * 2.0 ** -23:.3g})")
        assert err <= 16.0 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the whole engine
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_engine_step_matches_the_reference(dev, hip_lib, golden, name):
    g = golden("matching_dgcnn_train")
    s = engine_step(name, dev)
    x, lengths = cases.case_arrays(name)
    N = len(x)
    sd = cases.state_dict()
    for l in range(4):
        want = g[f"{name}_l{l + 1}_knn"].astype(np.int64)
        bad = int((np.sort(s["knn"][l], 1) != np.sort(want, 1)).any(1).sum())
        print(f"{name} level {l + 1}: {bad} of {N} rows pick another neighbour set than the reference")
        assert bad == 0
    for key, got in list(zip(ACTS, s["x"] + [s["out"]])) + [(f"buf_{k}", s["buffers"][k]) for k in cases.BUFFERS]:
        stride = 1 if key.startswith("buf_") else int(g[f"stride_{key}"])
        err = float(np.abs(got.reshape(-1)[::stride] - g[f"{name}_{key}"]).max() / float(g[f"{name}_{key}_max"]))
        print(f"{name} {key}: {err:.3g} of the maximum (bar {bar_of(g, name, key):.3g})")
        assert err <= bar_of(g, name, key)
    assert s["tracked"] == [int(sd[f"bn{l}.num_batches_tracked"]) + 1 for l in range(1, 6)]
    # winners, by neighbour identity; a differing entry is excused only where the two candidates' z are within twice the level's bar
    fix_w = [g[f"{name}_l{l + 1}_winner"].astype(np.int64) for l in range(4)]
    fix_k = [g[f"{name}_l{l + 1}_knn"].astype(np.int64) for l in range(4)]
    r64 = cases.train_step(sd, x, lengths, cases.dout_array(name), torch.float64, indices=s["knn"], winners=s["winner"], form="decomposed")
    excused_total = 0
    for l in range(4):
        who_fix, who_eng = np.take_along_axis(fix_k[l], fix_w[l], 1), np.take_along_axis(s["knn"][l], s["winner"][l], 1)
        diff = np.argwhere(who_fix != who_eng)
        excused = 0
        if len(diff):
            # z of both candidates in the float64 restatement on the engine's lists
            X = torch.from_numpy(x).double() if l == 0 else r64[f"x{l}"]
            W = torch.from_numpy(np.asarray(sd[f"conv{l + 1}.0.weight"])).double()[:, :, 0]
            uv = X @ cases.split_weight(W).t()
            C_ = cases.WIDTHS[l]
            up = torch.cat([uv[:, :C_], torch.zeros((1, C_), dtype=torch.float64)], 0).numpy()
            v = uv[:, C_:].numpy()
            zmax = float(np.abs(up[s["knn"][l]] + v[:, None, :]).max())
            tol = 2.0 * bar_of(g, name, f"x{l + 1}") * zmax
            for i, c in diff:
                za = up[who_fix[i, c], c] + (v[i, c] if who_fix[i, c] != N else 0.0)
                zb = up[who_eng[i, c], c] + (v[i, c] if who_eng[i, c] != N else 0.0)
                assert abs(za - zb) <= tol, f"level {l + 1} ({i}, {c}): winners {who_fix[i, c]} / {who_eng[i, c]} with z {za} / {zb}"
                excused += 1
        print(f"{name} level {l + 1}: {len(diff)} of {who_fix.size} winners differ from the reference's, {excused} excused as near-ties")
        assert excused <= 1e-3 * who_fix.size
        excused_total += excused
    for k in cases.PARAMS:
        want = r64["grads"][k]
        err = float(np.abs(s["grads"][k] - want).max() / np.abs(want).max())
        stride = int(g[f"stride_{k}"])
        fix = float(np.abs(want.reshape(-1)[::stride] - g[f"{name}_grad_{k}"]).max() / float(g[f"{name}_grad_{k}_max"]))
        print(f"{name} grad {k}: {err:.3g} of the maximum (bar {bar_of(g, name, 'grad_' + k):.3g}); the restatement on the engine's lists and "
              f"winners is {fix:.3g} from the fixture")
        assert s["grads"][k].shape == want.shape and err <= bar_of(g, name, "grad_" + k)
        if excused_total == 0:
            assert fix <= 1e-10


def test_two_runs_are_bitwise_equal_and_eval_sees_the_moved_buffers(dev, hip_lib):
    from pfpp_hip.matching_dgcnn_train import DGCNNTrainEngine

    x, lengths = cases.case_arrays("small")
    x_d, dout = torch.from_numpy(x).to(dev), torch.from_numpy(cases.dout_array("small")).to(dev)
    runs = []
    for _ in range(2):
        enc = fresh_encoder(dev)
        before = enc(x_d, lengths).clone()
        eng = DGCNNTrainEngine(enc)
        out = eng.forward(x_d, lengths)
        eng.backward(dout)
        after = enc(x_d, lengths)
        torch.cuda.synchronize()
        assert not enc.training and not torch.equal(before, after), "the eval forward after a step must see the moved running buffers"
        ref = fresh_encoder(dev)
        ref.load_state_dict(enc.state_dict(), strict=True)
        assert torch.equal(ref(x_d, lengths), after)                                          # and exactly what a fresh pack of them gives
        runs.append([out.clone()] + [p.grad.clone() for p in eng.params.values()] + [b.clone() for b in enc.buffers()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        DGCNNTrainEngine(fresh_encoder(dev)).forward(x_d[:1], [1])


def test_stage_events_cover_every_stage(dev, hip_lib):
    from pfpp_hip.matching_dgcnn_train import DGCNNTrainEngine

    x, lengths = cases.case_arrays("tiny")
    eng = DGCNNTrainEngine(fresh_encoder(dev))
    eng.stage_events = []
    eng.forward(torch.from_numpy(x).to(dev), lengths)
    eng.backward(torch.from_numpy(cases.dout_array("tiny")).to(dev))
    names, eng.stage_events = [n for n, _ in eng.stage_events], None
    assert names == ["begin"] + [f"{s}{l}" for l in range(1, 5) for s in ("search", "inverse_lists", "product", "stats", "apply")] + ["conv5"] \
        + ["begin", "conv5_bwd"] + [f"{s}{l}{t}" for l in (4, 3, 2, 1) for s, t in (("gathers", ""), ("products", "_bwd"))]


def _puzzles(dev):
    """two puzzles of 2 and 3 pieces for the chain"""
    rng = np.random.default_rng(9)
    n_pcs = np.asarray([[40, 30, 0], [25, 33, 22]], dtype=np.int64)
    pts = [torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (1, 3)) + rng.uniform(-0.2, 0.2, (int(n), 3)) for n in row if n]).astype(np.float32)).to(dev)
           for row in n_pcs]
    return pts, n_pcs, (n_pcs > 0)


def test_chain_fills_every_grad_under_one_backward(dev, hip_lib):
    from pfpp_hip.matching import DescriptorNetwork
    from pfpp_hip.matching_dgcnn_train import DGCNNDescriptorTrainEngine

    torch.manual_seed(3)
    net = DescriptorNetwork(encoder="dgcnn.dynamic").to(dev)
    full = DGCNNDescriptorTrainEngine(net)
    pts, n_pcs, valids = _puzzles(dev)
    feats = full.forward(pts, n_pcs, valids)
    target = torch.linspace(-1, 1, feats.numel(), device=dev).reshape(feats.shape)
    loss = ((feats - target) ** 2).mean()
    caught = {}
    orig = full.encoder.backward
    full.encoder.backward = lambda d: (caught.__setitem__("d", d.clone()), orig(d))[1]
    loss.backward()
    torch.cuda.synchronize()
    missing = [k for k, p in net.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    print(f"loss {float(loss.detach()):.4g}; {len(list(net.parameters()))} parameters, {len(missing)} without a finite gradient")
    assert feats.requires_grad and not missing
    assert any(float(p.grad.abs().max()) > 0 for p in net.encoder.parameters())
    got = [p.grad.clone() for p in net.encoder.parameters()]
    orig(caught["d"])                                                                          # the same incoming gradient, on its own
    assert all(torch.equal(a, p.grad) for a, p in zip(got, net.encoder.parameters()))
    with pytest.raises(RuntimeError, match="another forward"):
        f2 = full.forward(pts, n_pcs, valids)
        full.encoder.forward(torch.cat(pts), n_pcs[n_pcs > 0])
        f2.sum().backward()


def test_three_adam_steps_lower_a_fixed_quadratic_loss(dev, hip_lib):
    from pfpp_hip.matching_dgcnn_train import DGCNNTrainEngine

    x, lengths = cases.case_arrays("tiny")
    x_d = torch.from_numpy(x).to(dev)
    target = torch.from_numpy(cases.dout_array("tiny")).to(dev)
    enc = fresh_encoder(dev)
    eng = DGCNNTrainEngine(enc)
    losses = []
    for _ in range(4):
        out = eng.forward(x_d, lengths)
        losses.append(float(((out - target) ** 2).mean()))
        eng.backward(2.0 * (out - target) / out.numel())
        eng.optimizer_step(lr=1e-3)
    print(f"loss over three Adam steps: {[f'{v:.5f}' for v in losses]}")
    assert losses[3] < losses[0] and all(np.isfinite(losses))


def _eager_direct_step(sd, x, lists, dout):
    """the reference's form in eager fp32 under autograd on given lists: [N, 20, 2 C] and three [N, 20, C] tensors per level"""
    F = torch.nn.functional
    N = x.shape[0]
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k in cases.PARAMS}
    X, feats = x, []
    for l in range(1, 5):
        it = lists[l - 1].long()
        real = (it != N)[..., None].to(x.dtype)
        Xp = torch.cat([X, torch.zeros((1, X.shape[1]), dtype=x.dtype, device=x.device)], 0)
        nb = Xp[it.reshape(-1)].reshape(N, cases.K, -1)
        own = X[:, None, :].expand_as(nb)
        f = (torch.cat([nb - own, own], -1) * real).permute(0, 2, 1).contiguous()
        y = F.leaky_relu(F.batch_norm(F.conv1d(f, P[f"conv{l}.0.weight"]), None, None, P[f"bn{l}.weight"], P[f"bn{l}.bias"], True, 0.1, cases.BN_EPS),
                         cases.SLOPE)
        X = y.max(-1)[0]
        feats.append(X)
    z = F.conv1d(torch.cat(feats, 1).t()[None].contiguous(), P["conv5.0.weight"])
    out = F.leaky_relu(F.batch_norm(z, None, None, P["bn5.weight"], P["bn5.bias"], True, 0.1, cases.BN_EPS), cases.SLOPE)[0].t()
    (out * dout).sum().backward()
    return out.detach(), {k: p.grad for k, p in P.items()}


def test_a_step_never_holds_a_tensor_of_20_rows_per_point(dev, hip_lib):
    """N = 4096 (8 pieces of 512).  The decomposed step keeps per point uv (4 KiB over the levels), e (2 KiB), cat (2 KiB), the winners
    (0.5 KiB), lists and their inverses (0.6 KiB), conv5's rows (1 KiB) and in the backward dcat, h, duv and the transposed operand of
    the weight gradient (about 7 KiB at level 4): about 18 KiB.  The reference's form under autograd keeps [N, 20, 2 C_in] and three
    [N, 20, C_out] tensors per level: 80 KiB per point at level 4 alone.  Bar: 32 KiB per point, and a quarter of the eager step."""
    from pfpp_hip.matching_dgcnn_train import DGCNNTrainEngine

    enc = fresh_encoder(dev)
    eng = DGCNNTrainEngine(enc)
    lengths = np.full(8, 512)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (1, 3)) + rng.uniform(-0.2, 0.2, (512, 3)) for _ in lengths]).astype(np.float32)).to(dev)
    dout = torch.from_numpy(rng.standard_normal((4096, cases.FEAT)).astype(np.float32)).to(dev)
    eng.forward(x[:1024], lengths[:2])                      # workspaces exist before the measurement
    eng.backward(dout[:1024])
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    eng.forward(x, lengths)
    eng.backward(dout)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    lists = [lv["idx"] for lv in eng.saved["levels"]]
    out_hip, grads_hip = None, {k: p.grad.clone() for k, p in eng.params.items()}
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out_e, grads_e = _eager_direct_step(sd, x, lists, dout)
    torch.cuda.synchronize()
    growth_e = torch.cuda.max_memory_allocated() - before
    worst = max(float((grads_hip[k] - grads_e[k].reshape(grads_hip[k].shape)).abs().max() / grads_e[k].abs().max()) for k in cases.PARAMS)
    print(f"N = 4096: peak growth of one step {growth / 4096 / 1024:.2f} KiB per point (bar 32) against {growth_e / 4096 / 1024:.2f} KiB per point "
          f"of the eager direct form on the same lists; worst gradient difference between the two fp32 paths {worst:.3g} of the maximum (reported)")
    assert growth < 32 * 1024 * 4096 and 4 * growth < growth_e
