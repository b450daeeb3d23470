"""GPU: the training step of the matcher's ragged PointNet++ encoder (csrc/pointnet_ragged_train.hip, pfpp_hip/matching_encoder_train.py).

The six entries alone against float64 numpy at edge shapes, then the engine against the float64 restatement of
tests/matching_encoder_train_cases.py (which tests/test_matching_encoder_train_host.py pins to tests/golden/matching_encoder_train.npz,
the reference's own module in .train() under autograd) on the GPU's own indices, fed the GPU's ReLU patterns and pool winners.  Every
test prints the figures it measured before it asserts.

Bars (DESIGN.md 5.9's rule): per tensor 4 x the reference's own float32-against-float64 deviation recorded in the fixture, floor
4 x 2^-23, relative to the tensor's largest magnitude.  `both` (small + second in one call) has no fixture entry: its deviation is the
larger of the two cases' (the same layers over the union of their rows).  The 33 convolution biases in front of a BatchNorm get exact
zeros.  Kernel tolerances are worked out from the number formats in each test."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EPS32 = 2.0 ** -24
FLOOR = 4.0 * 2.0 ** -23
COLSUM = ("conv1.bias",)                      # through pfpp_colsum: two runs agree to rounding, not bitwise


def load_cases(stem):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tc = load_cases("matching_encoder_train_cases")
base = tc.base
_RUN = {}


def d(a, dev, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)


def T():
    import pfpp_hip.matching_encoder_train as m

    return m


# ================================================================================================ the kernels alone
def bn_inputs(rows, C, seed):
    rng = np.random.default_rng([41, seed, rows, C])
    y = (rng.normal(0.3, 1.0, (rows, C)) * rng.uniform(0.5, 2.0, C)).astype(np.float32)
    return (y, rng.uniform(0.8, 1.2, C).astype(np.float32), rng.normal(0.1, 0.2, C).astype(np.float32),
            rng.normal(0, 0.1, C).astype(np.float32), rng.uniform(0.5, 1.5, C).astype(np.float32))


# rows: the least torch accepts; one row under and one over the 64 rows a workgroup takes before a second one starts; one over the
# 256 x 64 rows from which a workgroup's share grows beyond 64
@pytest.mark.parametrize("rows,C", [(2, 16), (63, 96), (65, 196), (64, 512), (256 * 64 + 1, 16), (1000, 196)])
def test_statistics_against_float64(dev, hip_lib, rows, C):
    """the sums are fp64 and folded in fp64: every coefficient is one float32 rounding of its float64 value, 2^-24 relative (b is
    formed from the rounded a, as the kernel forms it); the running buffers likewise.  Two runs agree bitwise."""
    y, gamma, beta, rm, rv = bn_inputs(rows, C, 1)
    eps, mom = 1e-5, 0.1
    rmd, rvd = d(rm, dev), d(rv, dev)
    coef = T().ragged_bn_stats(d(y, dev), d(gamma, dev), d(beta, dev), eps, mom, rmd, rvd).cpu().numpy()
    again = T().ragged_bn_stats(d(y, dev), d(gamma, dev), d(beta, dev), eps, mom, d(rm, dev), d(rv, dev)).cpu().numpy()
    y64 = y.astype(np.float64)
    mean, var = y64.mean(0), y64.var(0)
    rs = 1.0 / np.sqrt(var + eps)
    a = (gamma * rs).astype(np.float32)
    want = np.stack([a, beta - mean * a, mean, rs])
    # mean and b cancel: their error is measured against the magnitudes that went in
    scale = np.stack([np.abs(want[0]), np.abs(beta) + np.abs(mean * a), np.abs(y64).mean(0), np.abs(rs)])
    err = float((np.abs(coef - want) / scale).max())
    run = np.stack([0.9 * rm.astype(np.float64) + 0.1 * mean, 0.9 * rv.astype(np.float64) + 0.1 * var * rows / (rows - 1)])
    got_run = np.stack([rmd.cpu().numpy(), rvd.cpu().numpy()])
    err_run = float((np.abs(got_run - run) / (np.abs(run) + np.abs(np.stack([0.1 * mean, 0 * var])))).max())
    print(f"rows {rows} C {C}: coefficients {err / EPS32:.3g} x 2^-24, running buffers {err_run / EPS32:.3g} x 2^-24; bitwise repeat "
          f"{np.array_equal(coef, again)}")
    assert err <= 2 * EPS32 and err_run <= 2 * EPS32 and np.array_equal(coef, again)


def test_statistics_refuse_one_row_and_odd_widths(dev, hip_lib):
    y, gamma, beta, _, _ = bn_inputs(4, 16, 2)
    with pytest.raises(ValueError, match="at least 2"):
        T().ragged_bn_stats(d(y[:1], dev), d(gamma, dev), d(beta, dev), 1e-5)
    with pytest.raises(ValueError, match="multiple of 4"):
        T().ragged_bn_stats(d(np.zeros((4, 18), np.float32), dev), d(np.ones(18, np.float32), dev), d(np.ones(18, np.float32), dev), 1e-5)


@pytest.mark.parametrize("rows,C,pool", [(64, 16, 16), (96, 96, 32), (130 * 16, 196, 16), (64, 512, 32)])
def test_apply_pool_and_their_backward(dev, hip_lib, rows, C, pool):
    """h = max(fma(y, a, b), 0): the float64 value of y a + b is exact to 2^-53, so h is its float32 rounding (or its neighbour where
    the double rounding falls on a tie: 2^-23 relative).  The pooled output is, bit for bit, the maximum of the unpooled rows and the
    winner the first row that attains it; the pool's backward puts dout there and zeros elsewhere, bit for bit."""
    y, gamma, beta, _, _ = bn_inputs(rows, C, 3)
    y[:pool] = -np.abs(y[:pool]) - 5.0                       # group 0: no row positive in the channels whose a > 0
    yd = d(y, dev)
    coef = T().ragged_bn_stats(yd, d(gamma, dev), d(beta, dev), 1e-5)
    h = T().ragged_bn_apply(yd, coef).cpu().numpy()
    wide = torch.full((rows // pool, C + 8), -7.0, device=dev)
    pooled, win = T().ragged_bn_apply(yd, coef, pool, out=wide, c_off=4, want_winner=True)
    c = coef.cpu().numpy().astype(np.float64)
    want = np.maximum(y.astype(np.float64) * c[0] + c[1], 0.0)
    err = float((np.abs(h - want) / np.maximum(np.abs(want), 1e-30)).max())
    hg = h.reshape(-1, pool, C)
    arg = np.where(hg.max(1) > 0, hg.argmax(1), -1)
    wide = wide.cpu().numpy()
    dout = np.random.default_rng(5).normal(size=(rows // pool, C + 4)).astype(np.float32)
    dh = T().ragged_pool_bwd(yd, coef, pool, d(dout, dev), c_off=4).cpu().numpy().reshape(-1, pool, C)
    want_dh = np.where(np.arange(pool)[None, :, None] == arg[:, None, :], dout[:, None, 4:], 0.0).astype(np.float32)
    print(f"rows {rows} C {C} pool {pool}: h off by {err / EPS32:.3g} x 2^-24; groups with no positive row {(arg < 0).sum()}")
    assert err <= 2 * EPS32
    assert np.array_equal(wide[:, 4:4 + C], hg.max(1)) and np.array_equal(win.cpu().numpy(), arg)
    assert (wide[:, :4] == -7.0).all() and (wide[:, 4 + C:] == -7.0).all(), "columns outside [c_off, c_off + C) were written"
    assert (arg < 0).any() and np.array_equal(dh, want_dh)


@pytest.mark.parametrize("rows,C", [(2, 16), (63, 96), (65, 196), (130, 512), (256 * 64 + 1, 16)])
def test_bn_relu_backward_against_float64(dev, hip_lib, rows, C):
    """dz = dh where the forward's h > 0.  dbeta / dgamma: fp64 sums of float32 terms, one rounding of x hat per term and one of the
    result: 4 x 2^-24 of the sum of the |terms|.  dy = g ((dz - m1) - xh m2) in float32, elementwise against the bound
    g (|dz| + |m1| + |xh| mean|dz xh|): m2 = mean(dz xh) inherits the two roundings of xh in EVERY term, so its error is measured by the
    mean of the |terms|, not by |m2|.  The xh m2 term carries the most roundings — xh two (the difference and the product with rstd), m2
    three (xh inside its terms and the rounding of the mean), the product one, the two subtractions two, g one and the last product
    one: ten, so the bar is 12 x 2^-24 of that bound.  Two runs agree bitwise; dy in place over dh gives the same bits."""
    y, gamma, beta, _, _ = bn_inputs(rows, C, 4)
    dh = np.random.default_rng([6, rows, C]).normal(size=(rows, C)).astype(np.float32)
    yd, gd = d(y, dev), d(gamma, dev)
    coef = T().ragged_bn_stats(yd, gd, d(beta, dev), 1e-5)
    h = T().ragged_bn_apply(yd, coef).cpu().numpy()
    dy, dgamma, dbeta = (t.cpu().numpy() for t in T().ragged_bn_relu_bwd(yd, d(dh, dev), coef, gd, dy=torch.empty((rows, C), device=dev)))
    inplace = d(dh, dev)
    dy2, dgamma2, dbeta2 = (t.cpu().numpy() for t in T().ragged_bn_relu_bwd(yd, inplace, coef, gd))
    c = coef.cpu().numpy().astype(np.float64)
    dz = np.where(h > 0, dh, 0.0).astype(np.float64)
    xh = (y.astype(np.float64) - c[2]) * c[3]
    m1, m2 = dz.mean(0), (dz * xh).mean(0)
    g = gamma.astype(np.float64) * c[3]
    want = g * (dz - m1 - xh * m2)
    bound = g * (np.abs(dz) + np.abs(m1) + np.abs(xh) * np.abs(dz * xh).mean(0))
    e_dy = float((np.abs(dy - want) / np.maximum(bound, 1e-30)).max())
    e_b = float((np.abs(dbeta - dz.sum(0)) / np.maximum(np.abs(dz).sum(0), 1e-30)).max())
    e_g = float((np.abs(dgamma - (dz * xh).sum(0)) / np.maximum(np.abs(dz * xh).sum(0), 1e-30)).max())
    print(f"rows {rows} C {C}: dy {e_dy / EPS32:.3g}, dbeta {e_b / EPS32:.3g}, dgamma {e_g / EPS32:.3g} x 2^-24 of their bounds")
    assert e_dy <= 12 * EPS32 and e_b <= 4 * EPS32 and e_g <= 4 * EPS32
    assert np.array_equal(dy, dy2) and np.array_equal(dgamma, dgamma2) and np.array_equal(dbeta, dbeta2)
    assert np.array_equal(inplace.cpu().numpy(), dy)


def test_the_backward_thresholds_the_forwards_bits(dev, hip_lib):
    """the forward's h == 0 pattern is the backward's dz == 0 pattern, bit for bit.  dz is read off dbeta: with dh non-zero in one row
    only, dbeta[c] = dz[row, c].  Half the rows are built to sit on the threshold, y = -b / a to float32 rounding, where y a + b
    rounded twice and the fused form can differ in sign: with the other half's mean m and biased variance v and k = beta / gamma, the
    threshold t = mean - k sqrt(var + eps) of ALL rows is its own fixed point at t = m - u, u^2 (1 - k^2) / 4 = k^2 (v / 2 + eps)."""
    rows, C = 48, 96
    y, gamma, beta, _, _ = bn_inputs(rows, C, 7)
    gd, bd = d(gamma, dev), d(beta, dev)
    odd = y[1::2].astype(np.float64)
    k = beta.astype(np.float64) / gamma.astype(np.float64)
    assert (np.abs(k) < 0.95).all()
    u = np.sign(k) * np.sqrt(k * k * (odd.var(0) / 2 + 1e-5) * 4 / (1 - k * k))
    y[::2] = (odd.mean(0) - u).astype(np.float32)
    yd = d(y, dev)
    coef = T().ragged_bn_stats(yd, gd, bd, 1e-5)
    h = T().ragged_bn_apply(yd, coef).cpu().numpy()
    dz = np.zeros((rows, C), dtype=np.float32)
    for r in range(rows):
        dh = torch.zeros((rows, C), device=dev)
        dh[r] = 1.0
        dz[r] = T().ragged_bn_relu_bwd(yd, dh, coef, gd)[2].cpu().numpy()
    pre = y.astype(np.float64) * coef.cpu().numpy()[0].astype(np.float64) + coef.cpu().numpy()[1].astype(np.float64)
    print(f"h == 0 in {(h == 0).sum()} of {h.size} entries; |y a + b| < 1e-6 in {(np.abs(pre) < 1e-6).sum()}; patterns equal "
          f"{np.array_equal(h == 0, dz == 0)}")
    assert (np.abs(pre) < 1e-6).sum() > rows * C // 4
    assert np.array_equal(h == 0, dz == 0) and set(np.unique(dz)) <= {0.0, 1.0}


def test_group_backward_lists_sentinel_and_accumulate(dev, hip_lib):
    """point 0 is in every centroid's list, point 5 in none; K = 16 of a table of 32 columns; 200 source points so that more than one
    workgroup and a partial one run; D = 96 of lda = 104 columns (the coordinate columns get no gradient) into rows of 100 floats
    whose last four hold a sentinel.  A sum of n float32 terms accumulated in float32: n 2^-24 of the sum of the |terms|."""
    rng = np.random.default_rng(8)
    S, K, Np, D, lda, ldf = 150, 16, 201, 96, 104, 100
    idx = rng.integers(1, Np, (S, 32))
    idx[idx == 5] = 6
    idx[:, 3] = 0
    dA = rng.normal(size=(S * K, lda)).astype(np.float32)
    off, ent = T().inverse_lists_of(d(idx[:, :K], dev, torch.int32), Np)
    dfe = torch.full((Np, ldf), 3.5, device=dev)
    T().ragged_group_bwd(d(dA, dev), D, off, ent, K, K, dfe)
    got = dfe.cpu().numpy()
    want, mag = np.zeros((Np, D)), np.zeros((Np, D))
    np.add.at(want, idx[:, :K].reshape(-1), dA[:, :D].astype(np.float64))
    np.add.at(mag, idx[:, :K].reshape(-1), np.abs(dA[:, :D]).astype(np.float64))
    n = np.bincount(idx[:, :K].reshape(-1), minlength=Np)
    err = float((np.abs(got[:, :D] - want) / np.maximum(mag * np.maximum(n, 1)[:, None], 1e-30)).max())
    print(f"group backward: {err / EPS32:.3g} x 2^-24 of n sum |terms|; lists of {n.min()} .. {n.max()} entries")
    assert n[0] == S and n[5] == 0 and err <= EPS32
    assert (got[5, :D] == 0).all() and (got[:, D:] == 3.5).all()
    again = torch.full((Np, ldf), 3.5, device=dev)
    T().ragged_group_bwd(d(dA, dev), D, off, ent, K, K, again)
    assert torch.equal(again, dfe)
    T().ragged_group_bwd(d(dA, dev), D, off, ent, K, K, again, accumulate=True)          # the second scale of a level adds
    acc = again.cpu().numpy()
    assert np.array_equal(acc[5, :D], got[5, :D]) and float(np.abs(acc[:, :D] - 2 * want).max()) <= 4e-6 * float(np.abs(want).max())


@pytest.mark.parametrize("S", [7, 1])
def test_interpolation_backward(dev, hip_lib, S):
    """S = 7: centroid 2 in no list, point 0 with all three slots equal (a piece with one centroid: two padded slots), weights as the
    forward leaves them; S = 1: the broadcast, column sums over all rows in fp64 (one float32 rounding of the float64 sum).  N = 300 rows
    of 40 + 196 columns: more than one workgroup's share."""
    rng = np.random.default_rng(9)
    N, D1, D2 = 300, 40, 196
    dout = rng.normal(size=(N, D1 + D2)).astype(np.float32)
    if S == 1:
        got = T().ragged_interp_bwd(d(dout, dev), D1, D2, None, None, None, 1).cpu().numpy()
        want = dout[:, D1:].astype(np.float64).sum(0)
        err = float((np.abs(got[0] - want) / np.abs(dout[:, D1:]).astype(np.float64).sum(0)).max())
        print(f"S = 1: {err / EPS32:.3g} x 2^-24 of the sum of the |terms|")
        assert got.shape == (1, D2) and err <= EPS32
        return
    idx = rng.integers(0, S, (N, 3))
    idx[idx == 2] = 3
    idx[0] = 4
    w = rng.uniform(0.05, 1, (N, 3)).astype(np.float32)
    w[0, 1:] = 1e-16
    w /= w.sum(1, keepdims=True)
    off, ent = T().inverse_lists_of(d(idx, dev, torch.int32), S)
    got = T().ragged_interp_bwd(d(dout, dev), D1, D2, d(w, dev), off, ent, S).cpu().numpy()
    want, mag = np.zeros((S, D2)), np.zeros((S, D2))
    terms = w.astype(np.float64)[:, :, None] * dout[:, None, D1:].astype(np.float64)
    np.add.at(want, idx.reshape(-1), terms.reshape(-1, D2))
    np.add.at(mag, idx.reshape(-1), np.abs(terms).reshape(-1, D2))
    n = np.bincount(idx.reshape(-1), minlength=S)
    err = float((np.abs(got - want) / np.maximum(mag * np.maximum(n, 1)[:, None], 1e-30)).max())
    print(f"S = {S}: {err / EPS32:.3g} x 2^-24 of n sum |terms|; lists of {n.min()} .. {n.max()} entries")
    assert n[2] == 0 and (got[2] == 0).all() and err <= EPS32
    assert torch.equal(T().ragged_interp_bwd(d(dout, dev), D1, D2, d(w, dev), off, ent, S).cpu(), torch.from_numpy(got))


# ================================================================================================ the engine
def fresh_encoder(dev, sd=None):
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    enc = PointNet2PTMSGDynamic(3, 128)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in base.encoder_state_dict().items()} if sd is None else sd, strict=True)
    return enc.to(dev)


def collect(eng, out):
    s = eng.saved
    got = {"out": out.cpu().numpy(), **{f"l{l}_points": s["feats"][l].cpu().numpy() for l in range(1, 5)}}
    got.update({"grad." + k: v.grad.cpu().numpy() for k, v in eng.params.items()})
    got.update({"buf." + k: v.cpu().numpy() for k, v in eng.encoder.named_buffers() if not k.endswith("num_batches_tracked")})
    return got


def step(dev, name):
    """one forward (activations kept) + backward of a fresh module -> what the tests compare, on the host"""
    pts, lengths, start = tc.flat_case(name)
    eng = T().EncoderTrainEngine(fresh_encoder(dev))
    dout = tc.make_dout(name, len(pts))
    out = eng.forward(d(pts, dev), lengths, start=start, keep_activations=True)
    eng.backward(d(dout, dev))
    torch.cuda.synchronize()
    s = eng.saved
    got = collect(eng, out)
    got["tracked"] = sorted({int(v) for k, v in eng.encoder.named_buffers() if k.endswith("num_batches_tracked")})
    got["relu"] = {k: (v > 0).cpu().numpy() for k, v in s["relu"].items()}
    got["winner"] = {k: v.cpu().numpy() for k, v in s["winner"].items()}
    got["idx"] = {"cen": [c.cpu().numpy() for c in s["cen"]], "knn": [k.cpu().numpy() for k in s["nbr"]],
                  "back": [None if b[0] is None else (b[0].cpu().numpy(), b[1].cpu().numpy()) for b in s["back"]]}
    got["engine"], got["dout"], got["pts"] = eng, dout, pts
    return got


def case_run(dev, name):
    if name not in _RUN:
        _RUN[name] = step(dev, name)
    return _RUN[name]


def refdev(name):
    if name != "both":
        return tc.load_fixture(name)["refdev"]
    a, b = tc.load_fixture("small")["refdev"], tc.load_fixture("second")["refdev"]
    return {k: max(a[k], b[k]) for k in a}


ZERO_BIAS = tuple("grad." + cp + ".bias" for _, cp, _ in tc.layer_names())


@pytest.mark.parametrize("name", ["small", "second", "solo", "both"])
def test_forward_and_backward_against_the_restatement(dev, hip_lib, name):
    got = case_run(dev, name)
    sd = base.encoder_state_dict()
    host = tc.cpu_indices(*tc.flat_case(name))
    same = all(np.array_equal(a, b) for a, b in zip(got["idx"]["cen"], host["cen"])) and \
        all(np.array_equal(np.sort(a, 1), np.sort(b, 1)) for a, b in zip(got["idx"]["knn"], host["knn"]))
    print(f"{name}: the GPU's sampling chains and neighbour sets equal the host's float32 ones: {same}")
    own = tc.restate(sd, got["pts"], got["idx"], got["dout"])
    n_relu = {k: int((got["relu"][k] != own["relu"][k].numpy()).sum()) for k in got["relu"]}
    n_win = {k: int(((got["winner"][k] != own["winner"][k].numpy()) & got["relu"][k]).sum()) for k in got["winner"]}
    print(f"{name}: ReLU signs that differ from float64's own: {sum(n_relu.values())} of {sum(v.size for v in got['relu'].values())} "
          f"({ {k: v for k, v in n_relu.items() if v} }); pool winners with a positive maximum that differ: {sum(n_win.values())}")
    want = tc.fixture_tensors(tc.restate(sd, got["pts"], got["idx"], got["dout"], relu=got["relu"], winner=got["winner"]))
    devs, failed, worst = refdev(name), [], (0.0, "")
    assert set(want) <= set(got) and len(want) == 5 + 134 + 66
    for key in sorted(want):
        if key in ZERO_BIAS:
            if got[key].any():
                failed.append(key)
            continue
        err = float(np.abs(got[key].reshape(want[key].shape) - want[key]).max() / np.abs(want[key]).max())
        bar = max(4.0 * devs[key], FLOOR)
        worst = max(worst, (err / bar, key))
        if not err <= bar:
            print(f"{name} {key}: {err:.3g} of the maximum (reference float32 {devs[key]:.3g}, bar {bar:.3g})  MISSED")
            failed.append(key)
    print(f"{name}: {len(want)} tensors; worst error / bar {worst[0]:.3g} ({worst[1]}); conv biases exact zeros: "
          f"{not any(got[k].any() for k in ZERO_BIAS)}")
    assert got["tracked"] == [1]
    assert not failed, failed


def test_two_runs_agree_bitwise_and_the_backward_is_linear_in_powers_of_two(dev, hip_lib):
    a, b = case_run(dev, "second"), step(dev, "second")
    keys = [k for k in a if k.startswith(("grad.", "buf.", "out", "l1", "l2", "l3", "l4")) and k[5:] not in COLSUM]
    differ = [k for k in keys if not np.array_equal(a[k], b[k])]
    print(f"two runs of second: tensors that differ in a bit: {differ}")
    assert not differ
    assert float(np.abs(a["grad.conv1.bias"] - b["grad.conv1.bias"]).max()) <= 2e-6 * float(np.abs(a["grad.conv1.bias"]).max())
    eng = b["engine"]
    for e in (-10, 10):
        eng.backward(d(b["dout"] * np.float32(2.0 ** e), dev))
        differ = [k for k, v in eng.params.items() if k not in COLSUM and not np.array_equal(v.grad.cpu().numpy(), b["grad." + k] * np.float32(2.0 ** e))]
        print(f"backward(2^{e} dout) against 2^{e} backward(dout): tensors that differ in a bit: {differ}")
        assert not differ


def test_refusals(dev, hip_lib):
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    eng = T().EncoderTrainEngine(fresh_encoder(dev))
    pts = d(base._patch(np.random.default_rng(3), 30), dev)
    before = {k: v.clone() for k, v in eng.encoder.named_buffers()}
    with pytest.raises(ValueError, match="more than 1 value per channel"):       # 30 -> 5 -> 2 -> 1 -> 1
        eng.forward(pts, [30], seed=0)
    assert all(torch.equal(v, before[k]) for k, v in eng.encoder.named_buffers()), "a refused call moved the buffers"
    with pytest.raises(NotImplementedError, match="exact-fp32"):
        T().EncoderTrainEngine(PointNet2PTMSGDynamic(3, 128, gemm_mode="f16x3"))
    with pytest.raises(NotImplementedError):
        eng.encoder.train()
    with pytest.raises(RuntimeError, match="before forward"):
        T().EncoderTrainEngine(fresh_encoder(dev)).backward(torch.zeros((30, 128), device=dev))


def test_optimizer_step_is_adam_and_the_eval_forward_uses_the_new_state(dev, hip_lib):
    """two steps against float64 Adam on the GPU's own gradients, bar 2^-23 |p| + 8e-6 lr; afterwards the module's
    eval forward equals, bit for bit, a fresh module's that was loaded with the stepped weights and the moved buffers"""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    enc = fresh_encoder(dev)
    eng = T().EncoderTrainEngine(enc)
    pts, lengths, start = tc.flat_case("solo")
    x, dd = d(pts, dev), d(tc.make_dout("solo", len(pts)), dev)
    p64 = {k: v.detach().cpu().double().clone() for k, v in eng.params.items()}
    m64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    v64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    evals = [enc(x, lengths, start=start).clone()]
    for n in (1, 2):
        eng.forward(x, lengths, start=start)
        eng.backward(dd)
        pack_before = enc._packed()
        eng.optimizer_step(lr, (b1, b2), eps)
        assert enc._packed() is not pack_before
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
            p64[k] = v.detach().cpu().double().clone()
        print(f"Adam step {n}: worst error / bar over the {len(eng.params)} parameters {worst:.3g}")
        evals.append(enc(x, lengths, start=start).clone())
    assert not torch.equal(evals[0], evals[1]) and not torch.equal(evals[1], evals[2])
    assert {int(v) for k, v in enc.named_buffers() if k.endswith("num_batches_tracked")} == {2}
    other = fresh_encoder(dev, enc.state_dict())
    assert torch.equal(enc(x, lengths, start=start), other(x, lengths, start=start))


def _matcher_parts(dev):
    sc = load_cases("matching_self_train_cases")
    from pfpp_hip.matching_transformer import CrossAttentionLayer, PointTransformerLayer

    t = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    layer = PointTransformerLayer(128, 128, 8, 16)
    layer.load_state_dict(t(sc.base.ptf_state_dict()), strict=True)
    cross = CrossAttentionLayer(128, 8)
    cross.load_state_dict(t(sc.base.cross_state_dict()), strict=True)
    return layer.to(dev), cross.to(dev), t


def test_chain_of_the_four_functions(dev, hip_lib):
    """loss = MatchingHeadLoss(CrossAttentionFunction(PointTransformerFunction(p, EncoderFunction(...)))) on `small`, then .backward():
    all four backwards run, and the encoder's .grads are, bit for bit, the encoder engine called by hand on the gradient that reached
    its output (conv1.bias, through pfpp_colsum, to rounding)"""
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_train import MatchingHeadLoss, MatchingHeadTrainEngine
    from pfpp_hip.matching_transformer_train import (CrossAttentionFunction, CrossAttentionTrainEngine, PointTransformerFunction,
                                                     PointTransformerTrainEngine)

    layer, cross, t = _matcher_parts(dev)
    head = MatchingHead()
    head.load_state_dict(t(load_cases("matching_train_cases").head_state_dict()), strict=True)
    head_eng = MatchingHeadTrainEngine(head.to(dev), w_cls_loss=1.0, w_mat_loss=1.0)
    self_eng, cross_eng = PointTransformerTrainEngine(layer), CrossAttentionTrainEngine(cross)
    enc_eng = T().EncoderTrainEngine(fresh_encoder(dev))
    pts, lengths, start = tc.flat_case("small")
    n_pcs, valids = np.zeros((1, 20), dtype=np.int64), np.zeros((1, 20), dtype=np.float32)
    n_pcs[0, :len(lengths)], valids[0, :len(lengths)] = lengths, 1
    label = (np.random.default_rng(67).uniform(size=len(pts)) < 0.25).astype(np.int64)
    label[np.cumsum(lengths) - lengths] = 1                     # every piece gets a critical point
    gt, lab = d(pts, dev), torch.from_numpy(label).to(dev)
    feats = T().EncoderFunction.apply(enc_eng.autograd_leaf(dev), enc_eng, gt, lengths, start, None)
    assert feats.requires_grad
    feats.retain_grad()
    mid0 = PointTransformerFunction.apply(gt, feats, self_eng, lengths)
    mid1 = CrossAttentionFunction.apply(mid0, cross_eng, np.asarray([len(pts)]))
    loss = MatchingHeadLoss.apply(mid1, head_eng, gt, n_pcs, valids, None, lab)
    assert bool(torch.isfinite(loss))
    loss.backward()
    g_enc = {k: v.grad.clone() for k, v in enc_eng.params.items()}
    assert all(v.grad is not None for eng in (self_eng, cross_eng, head_eng) for v in eng.params.values())
    print(f"chain on small: loss {float(loss.detach()):.6g}, max |d descriptors| {float(feats.grad.abs().max()):.3g}, largest encoder "
          f"gradient {max(float(v.abs().max()) for v in g_enc.values()):.3g}")
    assert float(feats.grad.abs().max()) > 0
    enc_eng.backward(feats.grad.contiguous())
    differ = [k for k, v in enc_eng.params.items() if k not in COLSUM and not torch.equal(v.grad, g_enc[k])]
    print(f"encoder gradients that differ in a bit from the engine called by hand: {differ}")
    assert not differ
    assert float((enc_eng.params["conv1.bias"].grad - g_enc["conv1.bias"]).abs().max()) <= 2e-6 * float(g_enc["conv1.bias"].abs().max())


def test_descriptor_train_engine_takes_one_full_step(dev, hip_lib):
    from pfpp_hip.matching import DescriptorNetwork

    layer, cross, _ = _matcher_parts(dev)
    net = DescriptorNetwork()
    net.encoder.load_state_dict(fresh_encoder("cpu").state_dict())
    net.tf_self1.load_state_dict(layer.state_dict())
    net.tf_cross1.load_state_dict(cross.state_dict())
    net = net.to(dev)
    eng = T().DescriptorTrainEngine(net)
    pts, lengths, start = tc.flat_case("second")
    n_pcs, valids = np.zeros((1, 20), dtype=np.int64), np.zeros((1, 20), dtype=np.float32)
    n_pcs[0, :len(lengths)], valids[0, :len(lengths)] = lengths, 1
    x = d(pts, dev)
    before = net(x[None], n_pcs, valids, start=start).clone()
    params = {k: v.detach().clone() for k, v in net.named_parameters()}
    part_feats = eng.forward(x[None], n_pcs, valids, start=start)
    assert part_feats.requires_grad and part_feats.shape == before.shape
    (part_feats * d(tc.make_dout("second", len(pts)), dev).reshape(part_feats.shape)).sum().backward()
    missing = [k for k, v in net.named_parameters() if v.grad is None or not bool(torch.isfinite(v.grad).all())]
    assert not missing, missing
    eng.optimizer_step(1e-3)
    still = [k for k, v in net.named_parameters() if torch.equal(v.detach(), params[k]) and bool(v.grad.any())]
    after = net(x[None], n_pcs, valids, start=start)
    print(f"one step of {len(params)} parameters: unchanged with a non-zero gradient {still}; max |change of part_feats| "
          f"{float((after - before).abs().max()):.3g}")
    assert not still and bool(torch.isfinite(after).all()) and not torch.equal(after, before)
    with pytest.raises(NotImplementedError):
        net.train()
