"""GPU: the matcher's point-transformer and cross-attention layers (csrc/matching_tf.hip, pfpp_hip/matching_transformer.py,
pfpp_hip.matching.DescriptorNetwork) against (a) tests/golden/matching_transformer.npz, written by
tools/make_matching_transformer_goldens.py from the reference's own modules, and (b) the restatements of
tests/matching_transformer_cases.py, which tests/test_matching_transformer_host.py pins to that fixture.  Inputs and weights are
regenerated from the case file.  Every test prints the figures it measured before it asserts.

Bars.  Neighbour indices are compared with the numpy float32 restatement of the bit-defined key on the rows the GPU
itself projected, index for index, nothing excused.  Floats: the fixture records, per tensor, the deviation of the reference's own
fp32 run from its float64 run relative to the tensor's largest magnitude; the bar is 4 x that for exact-fp32 products (same
operations, another order) and 16 x for split-f16 projections (22 instead of 24 operand bits), with a floor of 4 x 2^-23.  For the
attention-only cases the reference deviation is that of a float32 torch evaluation of the same inputs, computed here."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MULT = {"f32": 4.0, "f16x3": 16.0}
FLOOR = 4.0 * 2.0 ** -23


def load_cases(stem="matching_transformer_cases"):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_LAYERS, _NET, _R64 = {}, {}, {}


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def layers(dev, mode):
    from pfpp_hip.matching_transformer import CrossAttentionLayer, PointTransformerLayer

    if mode not in _LAYERS:
        s, c = PointTransformerLayer(128, 128, n_heads=8, nsampmle=16, gemm_mode=mode), CrossAttentionLayer(128, 8, gemm_mode=mode)
        s.load_state_dict(tensors(cases.ptf_state_dict()), strict=True)
        c.load_state_dict(tensors(cases.cross_state_dict()), strict=True)
        _LAYERS[mode] = (s.to(dev), c.to(dev))
    return _LAYERS[mode]


def restated64(name, golden):
    """float64 restatement of both layers on the fixture's indices, computed once and left unchanged"""
    if name not in _R64:
        g = golden("matching_transformer")
        p, x, lengths, puz = cases.case_arrays(name)
        idx = (g[f"{name}_idx_k"].astype(np.int64), g[f"{name}_idx_v"].astype(np.int64))
        r = cases.ptf_restate(cases.ptf_state_dict(), p, x, lengths, torch.float64, indices=idx)
        r["swapped"] = cases.ptf_restate(cases.ptf_state_dict(), p, x, lengths, torch.float64, indices=(idx[0], idx[0]))["out"]
        r.update({f"cross_{k}": v for k, v in cases.cross_restate(cases.cross_state_dict(), x, puz, torch.float64).items()})
        _R64[name] = r
    return _R64[name]


def rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------ neighbours in feature space
def check_knn_lists(idx, rows, lengths, label):
    """idx int [N, 16] against the numpy float32 restatement on the same rows: equal index for index; ascending order, fill slots
    and piece membership asserted on their own"""
    N = rows.shape[0]
    want, gap = cases.feat_knn_f32(rows, lengths)
    piece = np.repeat(np.arange(len(lengths)), lengths)
    real = idx != N
    n_real = np.minimum(np.asarray(lengths)[piece], 16)
    assert idx.shape == (N, 16) and ((idx >= 0) & (idx <= N)).all()
    assert (real.sum(1) == n_real).all() and (real == (np.arange(16)[None, :] < n_real[:, None])).all(), f"{label}: fill slots"
    assert (piece[np.where(real, idx, 0)] == piece[:, None])[real].all(), f"{label}: an index outside the row's piece"
    a = rows.astype(np.float32)
    nb = a[np.where(real, idx, 0)]
    d = np.zeros((N, 16), dtype=np.float32)
    for c in range(rows.shape[1]):
        t = a[:, None, c] - nb[:, :, c]
        d = d + t * t
    d = np.where(real, d, np.float32(3e38))
    assert (np.diff(d, axis=1) >= 0).all(), f"{label}: not ascending"
    tie = (np.diff(d, axis=1) == 0) & real[:, 1:]
    assert (np.diff(idx, axis=1)[tie] > 0).all(), f"{label}: a tie not broken towards the lower index"
    bad = int((idx != want).any(1).sum())
    print(f"{label}: {N} rows, {bad} differ from the float32 restatement; {int(tie.sum())} exact ties; smallest relative distance step {gap.min():.3g}")
    assert bad == 0
    return want


def test_feat_knn_equals_the_float32_restatement_index_for_index(dev, hip_lib):
    from pfpp_hip import ops
    from pfpp_hip.matching_transformer import feat_knn

    layer, _ = layers(dev, "f32")
    p, x, lengths, _ = cases.case_arrays("pair")
    N = len(x)
    pack = layer._packed()
    xd = torch.from_numpy(x).to(dev)
    qkv = ops.gemm(xd, pack["w_qkv"], M=N, N=384, K=128, lda=128, bias=pack["b_qkv"], mode="f32")
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
    idx_k = feat_knn(qkv, off, int(lengths.max()), col=128).cpu().numpy().astype(np.int64)
    idx_v = feat_knn(qkv, off, int(lengths.max()), col=256).cpu().numpy().astype(np.int64)
    rows = qkv.cpu().numpy()
    check_knn_lists(idx_k, rows[:, 128:256], lengths, "pair x_k")
    check_knn_lists(idx_v, rows[:, 256:], lengths, "pair x_v")
    # the 5-point piece: five neighbours and eleven times the fill value N; the tie of the 17-point piece, lower index first
    assert (idx_k[:5, :5] < 5).all() and (idx_k[:5, 5:] == N).all() and (idx_v[:5, 5:] == N).all()
    lo, hi = 21 + cases.TIE_ROWS[0], 21 + cases.TIE_ROWS[1]
    assert np.array_equal(rows[lo], rows[hi]), "identical input rows must project to identical rows"
    assert idx_k[lo, :2].tolist() == [lo, hi] and idx_k[hi, :2].tolist() == [lo, hi] and idx_v[hi, :2].tolist() == [lo, hi]
    differ = float((idx_k != idx_v).any(1).mean())
    print(f"idx_k and idx_v differ in {100 * differ:.1f} % of the rows")
    assert differ > 0.5
    # the layer's own searches are these
    out, ik, iv = layer(torch.from_numpy(p).to(dev), xd, lengths, return_indices=True)
    assert ik.dtype == torch.int32 and np.array_equal(ik.cpu().numpy(), idx_k) and np.array_equal(iv.cpu().numpy(), idx_v)


def test_feat_knn_merges_the_four_runs_of_a_large_piece_in_index_order(dev, hip_lib):
    """a piece of 700 rows is walked by four waves in runs of 175 over eleven tiles each; four identical rows, one per run, tie at
    every query and must come out in index order; a second piece of 100 rows shares the launch"""
    from pfpp_hip.matching_transformer import feat_knn

    rng = np.random.default_rng(41)
    lengths = np.asarray([700, 100])
    rows = rng.normal(size=(800, 128)).astype(np.float32)
    dup = [5, 200, 400, 650]
    rows[dup[1:]] = rows[dup[0]]
    wide = np.zeros((800, 384), dtype=np.float32)              # searched in place in the middle third of wider rows
    wide[:, 128:256] = rows
    off = torch.from_numpy(np.asarray([0, 700, 800], dtype=np.int64)).to(dev)
    idx = feat_knn(torch.from_numpy(wide).to(dev), off, 700, col=128).cpu().numpy().astype(np.int64)
    check_knn_lists(idx, rows, lengths, "700 + 100 rows")
    for q in dup:
        assert idx[q, :4].tolist() == dup
    again = feat_knn(torch.from_numpy(wide).to(dev), off, 700, col=128).cpu().numpy()
    assert np.array_equal(again, idx)


# ------------------------------------------------------------------------------------------------ aggregation
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_aggregate_on_the_fixtures_indices_against_float64(dev, hip_lib, golden, mode):
    g = golden("matching_transformer")
    layer, _ = layers(dev, mode)
    p, x, lengths, _ = cases.case_arrays("tiny")
    r = restated64("tiny", golden)
    ik = torch.from_numpy(g["tiny_idx_k"].astype(np.int32)).to(dev)
    iv = torch.from_numpy(g["tiny_idx_v"].astype(np.int32)).to(dev)
    pd, xd = torch.from_numpy(p).to(dev), torch.from_numpy(x).to(dev)
    out = layer(pd, xd, lengths, indices=(ik, iv)).cpu().numpy()
    dev_ref = float(g["tiny_out_refdev"])
    bar = max(MULT[mode] * dev_ref, FLOOR)
    err = rel(out, r["out"].numpy())
    # the pairing of slot t of idx_v with slot t of idx_k: the same kernel fed idx_k in place of idx_v computes something else
    wrong = layer(pd, xd, lengths, indices=(ik, ik)).cpu().numpy()
    miss, own = rel(wrong, r["out"].numpy()), rel(wrong, r["swapped"].numpy())
    print(f"tiny {mode} aggregate on the fixture's indices: {err:.3g} of the maximum (reference {dev_ref:.3g}, bar {bar:.3g}); fed idx_k "
          f"twice: {miss:.3g} from the layer's result ({miss / bar:.0f} bars), {own:.3g} from the float64 restatement of that variant")
    assert np.isfinite(out).all() and err <= bar
    assert miss > 1000 * bar and own <= bar


def test_aggregate_walks_more_points_than_it_has_workgroups(dev, hip_lib):
    """1,150 points: the launch has 1,024 workgroups, so 126 of them take a second point with the weights they already hold.  The
    neighbour lists are the GPU's own (tested above); the float64 restatement runs on them.  Bar: 4 x the deviation of the float32
    restatement from the float64 one on the same lists, floor 4 x 2^-23."""
    layer, _ = layers(dev, "f32")
    rng = np.random.default_rng(47)
    lengths = np.asarray([700, 450])
    N = int(lengths.sum())
    p = (0.3 * rng.normal(size=(N, 3))).astype(np.float32)
    x = rng.normal(size=(N, 128)).astype(np.float32)
    out, ik, iv = layer(torch.from_numpy(p).to(dev), torch.from_numpy(x).to(dev), lengths, return_indices=True)
    idx = (ik.cpu().numpy(), iv.cpu().numpy())
    want = cases.ptf_restate(cases.ptf_state_dict(), p, x, lengths, torch.float64, indices=idx)["out"].numpy()
    ref32 = cases.ptf_restate(cases.ptf_state_dict(), p, x, lengths, torch.float32, indices=idx)["out"].double().numpy()
    dev_ref = rel(ref32, want)
    bar = max(4.0 * dev_ref, FLOOR)
    err = rel(out.cpu().numpy(), want)
    tail = rel(out.cpu().numpy()[1024:], want[1024:])
    print(f"1,150 points: {err:.3g} of the maximum (float32 restatement {dev_ref:.3g}, bar {bar:.3g}); the points past the grid {tail:.3g}")
    assert err <= bar


def test_layernorm128_against_torch(dev, hip_lib):
    """rows of very different mean and spread, a constant row (variance 0: eps decides) and a row count that is no multiple of the 4
    rows of a workgroup, against F.layer_norm in float64.  Bar: 4 x the deviation of torch's float32 layer_norm, floor 4 x 2^-23."""
    from pfpp_hip.matching_transformer import layernorm128

    rng = np.random.default_rng(53)
    x = (rng.normal(size=(1001, 128)) * rng.uniform(0.01, 30.0, (1001, 1)) + rng.normal(0, 5.0, (1001, 1))).astype(np.float32)
    x[7] = 2.5
    g, b = rng.uniform(0.5, 1.5, 128).astype(np.float32), rng.normal(0, 0.3, 128).astype(np.float32)
    t = lambda a, dt: torch.from_numpy(a).to(dt)
    want = torch.nn.functional.layer_norm(t(x, torch.float64), (128,), t(g, torch.float64), t(b, torch.float64), 1e-6).numpy()
    ref32 = torch.nn.functional.layer_norm(t(x, torch.float32), (128,), t(g, torch.float32), t(b, torch.float32), 1e-6).double().numpy()
    got = layernorm128(t(x, torch.float32).to(dev), t(g, torch.float32).to(dev), t(b, torch.float32).to(dev), 1e-6).cpu().numpy()
    dev_ref = rel(ref32, want)
    bar = max(4.0 * dev_ref, FLOOR)
    err = rel(got, want)
    print(f"layernorm128, 1,001 rows: {err:.3g} of the maximum (float32 torch {dev_ref:.3g}, bar {bar:.3g}); constant row max |y - beta| "
          f"{float(np.abs(got[7] - b).max()):.3g}")
    assert np.isfinite(got).all() and err <= bar and np.array_equal(got[7], b)


# ------------------------------------------------------------------------------------------------ attention, 16-wide heads
def run_attention(dev, qkv, lengths):
    from pfpp_hip.matching_transformer import attn_rows16

    seq_len = torch.from_numpy(lengths.astype(np.int32)).to(dev)
    seq_off = torch.from_numpy((np.cumsum(lengths) - lengths).astype(np.int32)).to(dev)
    return attn_rows16(torch.from_numpy(qkv).to(dev), seq_off, seq_len, int(lengths.max()), 8, 0.25).cpu().numpy()


@pytest.mark.parametrize("name", sorted(cases.ATTN_CASES))
def test_attention_rows16_against_float64(dev, hip_lib, name):
    qkv, lengths = cases.attn_case(name)
    want = cases.attention_restate(qkv, lengths, torch.float64).numpy()
    ref32 = cases.attention_restate(qkv, lengths, torch.float32).double().numpy()
    dev_ref = rel(ref32, want)
    bar = max(4.0 * dev_ref, FLOOR)
    got = run_attention(dev, qkv, lengths)
    err = rel(got, want)
    q, k = qkv[:, :128].astype(np.float64), qkv[:, 128:256].astype(np.float64)
    n0 = int(lengths[0])
    span = np.abs(np.einsum("ihd,jhd->hij", q[:n0].reshape(n0, 8, 16), k[:n0].reshape(n0, 8, 16)) * 0.25).max()
    print(f"{name} lengths {lengths.tolist()}: {err:.3g} of the maximum (float32 torch {dev_ref:.3g}, bar {bar:.3g}); largest |score| {span:.1f}")
    assert np.isfinite(got).all() and err <= bar
    if name == "wide":
        assert span > 55.0                                       # the online rescale is exercised
    # rows of different sequences never mix: perturb the first sequence, the others' output is bitwise unchanged
    other = qkv.copy()
    other[:n0] = np.random.default_rng(43).normal(size=(n0, 384)).astype(np.float32)
    got2 = run_attention(dev, other, lengths)
    assert np.array_equal(got2[n0:], got[n0:]) and not np.array_equal(got2[:n0], got[:n0])
    assert np.array_equal(run_attention(dev, qkv, lengths), got)


# ------------------------------------------------------------------------------------------------ the full layers
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_both_layers_against_the_fixture(dev, hip_lib, golden, mode):
    g = golden("matching_transformer")
    s_layer, c_layer = layers(dev, mode)
    p, x, lengths, puz = cases.case_arrays("tiny")
    pd, xd = torch.from_numpy(p).to(dev), torch.from_numpy(x).to(dev)
    out, ik, iv = s_layer(pd, xd, lengths, return_indices=True)
    same = [int((t.cpu().numpy() != g[f"tiny_{k}"]).any(1).sum()) for t, k in ((ik, "idx_k"), (iv, "idx_v"))]
    got = {"out": out.cpu().numpy()}
    y, att, ln1 = c_layer(xd, puz, return_stages=True)
    got.update({"cross_out": y.cpu().numpy(), "att": att.cpu().numpy(), "ln1": ln1.cpu().numpy()})
    dense = c_layer(xd[None])                                    # the reference's dense [B, N_sum, 128] form
    assert dense.shape == (1, len(x), 128) and torch.equal(dense[0], y)
    # The fixture's lists were found on torch's CPU projection, these on the GPU's.  The two differ by the rounding of a 128-term sum
    # in another order (split-f16: 22 operand bits), i.e. by a few 2^-24 of a row's magnitude, which moves a squared distance by at
    # most ~1e-6 of its value (f16x3) while the closest two neighbour distances of `tiny` are 3.9e-6 apart (recorded in the fixture):
    # no list may change.
    print(f"tiny {mode}: rows whose neighbour lists differ from the fixture's (CPU projection): idx_k {same[0]}, idx_v {same[1]}; "
          f"smallest relative step between neighbour distances {float(g['tiny_knn_gap']):.3g}")
    assert same == [0, 0]
    worst = 0.0
    for key in ("out", "att", "ln1", "cross_out"):
        want = g[f"tiny_{key}"].astype(np.float64)
        dev_ref, scale = float(g[f"tiny_{key}_refdev"]), float(g[f"tiny_{key}_max"])
        err = float(np.abs(got[key].reshape(-1)[::int(g[f"stride_{key}"])].astype(np.float64) - want).max() / scale)
        bar = max(MULT[mode] * dev_ref, FLOOR)
        worst = max(worst, err / bar)
        print(f"tiny {mode} {key}: {err:.3g} of the maximum {scale:.4g} (reference {dev_ref:.3g}, bar {bar:.3g})")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the descriptor network
def network(dev, mode="f32"):
    from pfpp_hip.matching import DescriptorNetwork

    if mode not in _NET:
        enc_cases = load_cases("matching_encoder_cases")
        sd = {f"encoder.{k}": v for k, v in enc_cases.encoder_state_dict().items()}
        sd.update({f"tf_self1.{k}": v for k, v in cases.ptf_state_dict().items()})
        sd.update({f"tf_cross1.{k}": v for k, v in cases.cross_state_dict().items()})
        net = DescriptorNetwork(gemm_mode=mode)
        net.load_state_dict(tensors(sd), strict=True)
        _NET[mode] = net.to(dev)
    return _NET[mode]


def pair_batch(dev):
    pzs = cases.make_case("pair")
    P = 8
    n_pcs = np.stack([np.concatenate([z["lengths"], np.zeros(P - len(z["lengths"]), np.int64)]) for z in pzs])
    valids = (n_pcs > 0).astype(np.float32)
    return [torch.from_numpy(z["points"]).to(dev) for z in pzs], n_pcs, valids


def test_descriptor_network_batch_equals_puzzles_alone_and_repeats_bitwise(dev, hip_lib):
    net = network(dev)
    pts, n_pcs, valids = pair_batch(dev)
    n_pieces = (n_pcs > 0).sum(1)
    start = np.zeros((int(n_pieces.sum()), 4), dtype=np.int64)
    both = net(pts, n_pcs, valids, start=start)
    again = net(pts, n_pcs, valids, start=start)
    n0 = pts[0].shape[0]
    a = net(pts[:1], n_pcs[:1], valids[:1], start=start[:n_pieces[0]])
    b = net(pts[1:], n_pcs[1:], valids[1:], start=start[n_pieces[0]:])
    flat = net(torch.cat(pts), n_pcs, valids, start=start)
    print(f"pair: {both.shape[0]} descriptors; batch vs alone max |diff| {float((both[:n0] - a).abs().max()):.3g} / {float((both[n0:] - b).abs().max()):.3g}")
    assert both.shape == (n0 + pts[1].shape[0], 128) and bool(torch.isfinite(both).all())
    assert torch.equal(both, again) and torch.equal(both, flat)
    assert torch.equal(both[:n0], a) and torch.equal(both[n0:], b)
    seeded = net(pts, n_pcs, valids, seed=3)
    assert torch.equal(seeded, net(pts, n_pcs, valids, seed=3))
    with pytest.raises(ValueError, match="valid pieces"):
        net(pts, n_pcs, np.ones_like(valids))


def test_descriptor_network_feeds_the_head_end_to_end(dev, hip_lib):
    """DescriptorNetwork -> MatchingHead on `pair` labels the same critical points as the head fed with the float64 restatement of
    the two layers (run on the encoder's descriptors, downloaded, with the neighbour lists the GPU found on them).  A point whose float64 logit lies within the bar of the
    descriptors (16 x 2^-23 of the largest logit: two layers behind one another) could flip and would be excused; the seeded
    classifier of the case file leaves none there."""
    from pfpp_hip.matching import MatchingHead

    enc_cases = load_cases("matching_cases")
    net = network(dev)
    pts, n_pcs, valids = pair_batch(dev)
    lengths = n_pcs[n_pcs > 0]
    puz = n_pcs.sum(1)
    start = np.zeros((len(lengths), 4), dtype=np.int64)
    head = MatchingHead()
    sd = enc_cases.head_state_dict()
    sd.update(cases.classifier_state_dict())
    head.load_state_dict(tensors(sd), strict=True)
    head = head.to(dev)
    flat = torch.cat(pts)
    feats = net(pts, n_pcs, valids, start=start)
    enc_out = net.encoder(flat, lengths, start=start)
    _, ik, iv = net.tf_self1(flat, enc_out, lengths, return_indices=True)          # the discrete stage has its own test above
    mid = cases.ptf_restate(cases.ptf_state_dict(), flat.cpu().numpy(), enc_out.cpu().numpy(), lengths, torch.float64,
                            indices=(ik.cpu().numpy(), iv.cpu().numpy()))["out"]
    want = cases.cross_restate(cases.cross_state_dict(), mid.numpy(), puz, torch.float64)["out"]
    logits = cases.classifier_logits(cases.classifier_state_dict(), want.numpy(), torch.float64).numpy()
    margin = 16.0 * 2.0 ** -23 * float(np.abs(logits).max())
    excused = np.abs(logits) < margin
    got = head(feats, n_pcs, valids, assign=False)
    ref = head(want.to(torch.float32).to(dev), n_pcs, valids, assign=False)
    err = rel(feats.cpu().numpy(), want.numpy())
    labels_got, labels_ref = torch.cat(got.cls_pred).cpu().numpy(), torch.cat(ref.cls_pred).cpu().numpy()
    flips = int(((labels_got != labels_ref) & ~excused).sum())
    print(f"pair end to end: descriptors {err:.3g} of the maximum from the float64 restatement; {int(labels_ref.sum())} of {len(logits)} points "
          f"critical; smallest |logit| {np.abs(logits).min():.3g} (margin {margin:.3g}); {int(excused.sum())} points excused; {flips} labels differ")
    assert int(excused.sum()) == 0 and flips == 0
    assert 0 < int(labels_ref.sum()) < len(logits)
    assert torch.equal(got.n_critical_pcs, ref.n_critical_pcs)
    assert all(torch.equal(a, b) for a, b in zip(got.critical_pcs_idx, ref.critical_pcs_idx))
    assert np.array_equal((logits > 0).astype(np.int64), labels_ref)
