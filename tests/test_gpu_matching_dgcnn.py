"""GPU: the matcher's DGCNN encoder (csrc/dgcnn.hip, pfpp_hip/matching_dgcnn.py, the encoder selection of pfpp_hip.matching) against
(a) tests/golden/matching_dgcnn.npz, written by tools/make_matching_dgcnn_goldens.py from the reference's own module, and (b) the
restatements of tests/matching_dgcnn_cases.py, which tests/test_matching_dgcnn_host.py pins to that fixture.  Inputs and weights are
regenerated from the case file.  Every test prints the figures it measured before it asserts.

Bars.  The search is compared with the numpy float32 restatement of the bit-defined key index for index, the edge
extremum and the LeakyReLU pass with theirs bit for bit.  The whole encoder must pick the fixture's neighbour SETS at all four levels,
no row excused: the fixture's seeds were accepted only where the reference's float32 and float64 runs agree on every set and no
20th / 21st key pair is closer than 1e-4 relative.  Floats: the fixture records per tensor the deviation of the reference's own fp32
run from its float64 run relative to the tensor's largest magnitude; the bar is 4 x that, with a floor of 4 x 2^-23."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FLOOR = 4.0 * 2.0 ** -23
KEYS = ("x1", "x2", "x3", "x4", "out")


def load_cases(stem="matching_dgcnn_cases"):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_ENC, _R64 = {}, {}


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def encoder(dev):
    from pfpp_hip.matching_dgcnn import DGCNNDynamic

    if "enc" not in _ENC:
        enc = DGCNNDynamic(cases.FEAT, False, 3)
        enc.load_state_dict(tensors(cases.state_dict()), strict=True)
        _ENC["enc"] = enc.to(dev)
    return _ENC["enc"]


def restated64(name, golden):
    """float64 restatement in the reference's form on the fixture's lists, computed once and left unchanged"""
    if name not in _R64:
        g = golden("matching_dgcnn")
        x, lengths = cases.case_arrays(name)
        idx = [g[f"{name}_l{l + 1}_knn"].astype(np.int64) for l in range(4)]
        _R64[name] = cases.restate(cases.state_dict(), x, lengths, torch.float64, indices=idx)
    return _R64[name]


def offsets(lengths, dev):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)


# ------------------------------------------------------------------------------------------------ the search
def check_knn_lists(idx, rows, lengths, label):
    """idx int [N, 20] against the numpy float32 restatement on the same rows: equal index for index; the fill value N behind short
    pieces and piece membership asserted on their own"""
    N, K = rows.shape[0], cases.K
    want, step = cases.feat_knn(rows, lengths)
    piece = np.repeat(np.arange(len(lengths)), lengths)
    real = idx != N
    n_real = np.minimum(np.asarray(lengths)[piece], K)
    assert idx.shape == (N, K) and ((idx >= 0) & (idx <= N)).all()
    assert (real == (np.arange(K)[None, :] < n_real[:, None])).all(), f"{label}: fill slots"
    assert (piece[np.where(real, idx, 0)] == piece[:, None])[real].all(), f"{label}: an index outside the row's piece"
    bad = int((idx != want).any(1).sum())
    print(f"{label}: {N} rows in pieces of {list(map(int, lengths))}, {bad} differ from the float32 restatement; {int((~real).sum())} fill slots; "
          f"smallest relative 20th/21st step {step.min():.3g}")
    assert bad == 0


KNN_LENGTHS = (1, 5, 19, 20, 21, 63, 64, 65, 257)


@pytest.mark.parametrize("C", [3, 64, 128])
def test_search_equals_the_float32_restatement_index_for_index(dev, hip_lib, C):
    from pfpp_hip.matching_dgcnn import dgcnn_knn

    lengths = np.asarray(KNN_LENGTHS)
    rows = cases.knn_rows(C, lengths, seed=11)
    # rows of 64 / 128 channels are searched in place inside a wider buffer (as x1 .. x3 are inside the [N, 512] operand of conv5)
    col, ld = (0, 3) if C == 3 else (64, 512)
    buf = torch.full((len(rows), ld), 7.0, dtype=torch.float32, device=dev)
    buf[:, col:col + C] = torch.from_numpy(rows).to(dev)
    off = offsets(lengths, dev)
    idx = dgcnn_knn(buf, off, int(lengths.max()), col=col, width=C)
    again = dgcnn_knn(buf, off, int(lengths.max()), col=col, width=C)
    assert idx.dtype == torch.int32 and torch.equal(idx, again)
    check_knn_lists(idx.cpu().numpy().astype(np.int64), rows, lengths, f"C = {C}")


@pytest.mark.parametrize("C", [3, 64, 128])
def test_search_breaks_exact_ties_towards_the_lower_index_across_runs(dev, hip_lib, C):
    from pfpp_hip.matching_dgcnn import dgcnn_knn

    lengths = np.asarray(cases.TIE_LENGTHS)
    rows = cases.knn_tie_rows(C)
    x = torch.from_numpy(rows).to(dev)
    off = offsets(lengths, dev)
    idx = dgcnn_knn(x, off, int(lengths.max()))
    assert torch.equal(idx, dgcnn_knn(x, off, int(lengths.max())))
    got = idx.cpu().numpy().astype(np.int64)
    check_knn_lists(got, rows, lengths, f"ties, C = {C}")
    for q in range(7, 7 + 19):                              # the three copies tie for the 20th place: the one in the first run wins
        assert got[q, 19] == 7 + 24 and 7 + 25 not in got[q] and 7 + 60 not in got[q]
    for q in (7 + 24, 7 + 25, 7 + 60):
        assert list(got[q, :3]) == [7 + 24, 7 + 25, 7 + 60]


# ------------------------------------------------------------------------------------------------ the edge extremum
@pytest.mark.parametrize("c_out", [64, 128, 256])
def test_edge_extremum_equals_the_numpy_restatement_bit_for_bit(dev, hip_lib, c_out):
    from pfpp_hip.matching_dgcnn import dgcnn_edge_max

    N = 300
    uv, idx, scale, shift = cases.edge_case(c_out, N)
    want = cases.edge_max_f32(uv, idx, scale, shift)
    c_off = {64: 64, 128: 128, 256: 256}[c_out]
    out = torch.full((N, 512), -7.5, dtype=torch.float32, device=dev)
    d = lambda a: torch.from_numpy(a).to(dev)
    # uv handed over as a flat buffer with a row stride wider than [u | v]
    ld = 2 * c_out + 8
    buf = torch.full((N, ld), 9.0, dtype=torch.float32, device=dev)
    buf[:, :2 * c_out] = d(uv)
    dgcnn_edge_max(buf.reshape(-1), d(idx), d(scale), d(shift), c_out=c_out, ld=ld, out=out, c_off=c_off)
    got = out.cpu().numpy()
    tight = dgcnn_edge_max(d(uv), d(idx), d(scale), d(shift), c_out=c_out).cpu().numpy()
    y = got[:, c_off:c_off + c_out]
    n_bad = int((y.view(np.uint32) != want.view(np.uint32)).sum())
    even_pos, odd_neg = (np.arange(c_out) % 2 == 0) & (scale > 0), (np.arange(c_out) % 2 == 1) & (scale < 0)
    print(f"C_out = {c_out}: {n_bad} of {y.size} outputs differ in bits; scales < 0 / == 0 / > 0: {int((scale < 0).sum())} / {int((scale == 0).sum())} / "
          f"{int((scale > 0).sum())}; the padded slot wins the max in {int(even_pos.sum())} channels and the min in {int(odd_neg.sum())}")
    assert (scale < 0).any() and (scale == 0).any() and (scale > 0).any() and even_pos.any() and odd_neg.any()
    assert n_bad == 0 and np.array_equal(tight.view(np.uint32), want.view(np.uint32))
    act = lambda t: np.where(t > 0, t, t * np.float32(0.2))
    assert np.array_equal(y[:3][:, even_pos], np.broadcast_to(act(shift[even_pos]), (3, int(even_pos.sum()))))
    assert np.array_equal(y[:3][:, odd_neg], np.broadcast_to(act(shift[odd_neg]), (3, int(odd_neg.sum()))))
    other = np.ones(512, dtype=bool)
    other[c_off:c_off + c_out] = False
    assert (got[:, other] == -7.5).all(), "columns outside [c_off, c_off + C_out) were written"


# ------------------------------------------------------------------------------------------------ LeakyReLU and conv5
def test_leaky_relu_pass_in_place_bit_for_bit(dev, hip_lib):
    from pfpp_hip.matching_dgcnn import leaky_relu_

    rng = np.random.default_rng(2)
    a = rng.standard_normal((301, 136)).astype(np.float32)
    a[0, :6] = [0.0, -0.0, 1e-30, -1e-30, 3e38, -3e38]
    buf = torch.from_numpy(a).to(dev)
    view = buf[:, :128]                                     # rows of 128 inside rows of 136: the last 8 columns stay
    assert leaky_relu_(view) is view
    got = buf.cpu().numpy()
    want = np.where(a[:, :128] > 0, a[:, :128], (a[:, :128] * np.float32(0.2)).astype(np.float32))
    assert np.array_equal(got[:, :128].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[:, 128:], a[:, 128:])


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_conv5_on_the_fixtures_levels_against_float64(dev, hip_lib, golden, name):
    g = golden("matching_dgcnn")
    r = restated64(name, golden)
    cat32 = r["cat"].to(torch.float32)
    want = cases.conv5_f64(cases.state_dict(), cat32.numpy())                  # float64 on the float32 rows the GPU is given
    got = encoder(dev).conv5_forward(cat32.to(dev).contiguous()).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    bar = max(4.0 * float(g[f"{name}_out_refdev"]), FLOOR)
    print(f"{name} conv5 + bn5 + LeakyReLU: {err:.3g} of the maximum (bar {bar:.3g}); {int((want < 0).sum())} of {want.size} outputs negative")
    assert err <= bar and (want < 0).any() and (want > 0).any()


# ------------------------------------------------------------------------------------------------ the whole encoder
@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_encoder_against_the_fixture(dev, hip_lib, golden, name):
    g = golden("matching_dgcnn")
    x, lengths = cases.case_arrays(name)
    N = len(x)
    enc = encoder(dev)
    xd = torch.from_numpy(x).to(dev)
    y, lv = enc(xd, lengths, return_levels=True)
    y2 = enc(xd, torch.from_numpy(lengths))
    assert y.shape == (N, cases.FEAT) and torch.equal(y, y2)
    for l in range(4):
        got = lv[f"l{l + 1}_knn"].cpu().numpy().astype(np.int64)
        want = g[f"{name}_l{l + 1}_knn"].astype(np.int64)
        rows_off = int((np.sort(got, 1) != np.sort(want, 1)).any(1).sum())
        print(f"{name} level {l + 1}: {rows_off} of {N} rows pick another neighbour set than the reference (smallest 20th/21st step "
              f"{float(g[f'{name}_min_step'][l]):.3g}); {int((got == N).sum())} fill slots")
        assert rows_off == 0
    got_all = {f"x{l + 1}": lv[f"l{l + 1}_points"] for l in range(4)}
    got_all["out"] = y
    for key in KEYS:
        want = g[f"{name}_{key}"]
        got = got_all[key].contiguous().cpu().numpy().astype(np.float64).reshape(-1)[::int(g[f"stride_{key}"])]
        err = float(np.abs(got - want).max() / float(g[f"{name}_{key}_max"]))
        bar = max(4.0 * float(g[f"{name}_{key}_refdev"]), FLOOR)
        print(f"{name} {key}: {err:.3g} of the maximum from the reference's float64 run (bar {bar:.3g}; the reference's own float32 run "
              f"{float(g[f'{name}_{key}_refdev']):.3g})")
        assert got.shape == want.shape and err <= bar
    assert torch.equal(lv["cat"][:, 256:], lv["l4_points"])


def test_encoder_never_holds_a_tensor_of_20_rows_per_point(dev, hip_lib):
    """N = 4096 (8 pieces of 512): the decomposed form needs about 4.7 KiB per point (the 512-wide operand, a 512-wide product, one
    list and the output); the reference's form needs 41 KiB per point at level 4 alone"""
    enc = encoder(dev)
    lengths = np.full(8, 512)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(np.concatenate([rng.uniform(-0.5, 0.5, (1, 3)) + rng.uniform(-0.2, 0.2, (512, 3)) for _ in lengths]).astype(np.float32)).to(dev)
    enc(x[:1024], lengths[:2])                              # workspaces and the pack exist before the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = enc(x, lengths)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"N = {len(x)}: peak growth {growth} bytes = {growth / len(x) / 1024:.2f} KiB per point (bar 8)")
    assert y.shape == (4096, cases.FEAT) and bool(torch.isfinite(y).all())
    assert growth < 8 * 1024 * len(x)


def test_stage_events_cover_every_stage(dev, hip_lib):
    enc = encoder(dev)
    x, lengths = cases.case_arrays("tiny")
    enc.stage_events = []
    enc(torch.from_numpy(x).to(dev), lengths)
    names, enc.stage_events = [n for n, _ in enc.stage_events], None
    assert names == ["begin"] + [f"{s}{l}" for l in range(1, 5) for s in ("search", "product", "extremum")] + ["conv5"]


# ------------------------------------------------------------------------------------------------ wiring
def descriptor_state_dict():
    tf = load_cases("matching_transformer_cases")
    sd = {f"encoder.{k}": v for k, v in cases.state_dict().items()}
    sd.update({f"tf_self1.{k}": v for k, v in tf.ptf_state_dict().items()})
    sd.update({f"tf_cross1.{k}": v for k, v in tf.cross_state_dict().items()})
    return tensors(sd)


def two_puzzles():
    """-> (points per puzzle, n_pcs [2, 8], part_valids [2, 8])"""
    xa, la = cases.case_arrays("mixed")
    lb = np.asarray([40, 25, 64])
    rng = np.random.default_rng(9)
    xb = np.concatenate([rng.uniform(-0.5, 0.5, (1, 3)) + rng.uniform(-0.2, 0.2, (int(n), 3)) for n in lb]).astype(np.float32)
    n_pcs = np.stack([np.concatenate([l, np.zeros(8 - len(l), np.int64)]) for l in (la, lb)])
    return [xa, xb], n_pcs, (n_pcs > 0).astype(np.float32)


def test_descriptor_network_with_a_dgcnn_encoder_is_the_composition_of_its_modules(dev, hip_lib):
    from pfpp_hip.matching import DescriptorNetwork
    from pfpp_hip.matching_dgcnn import DGCNNDynamic

    net = DescriptorNetwork(encoder="dgcnn.dynamic")
    net.load_state_dict(descriptor_state_dict(), strict=True)
    net = net.to(dev)
    pts, n_pcs, valids = two_puzzles()
    pts = [torch.from_numpy(p).to(dev) for p in pts]
    feats = net(pts, n_pcs, valids)
    again = net(pts, n_pcs, valids, seed=5)                 # this family draws nothing: the seed has nothing to act on
    flat, lengths = torch.cat(pts), n_pcs[n_pcs > 0]
    e = net.encoder(flat, lengths)
    want = net.tf_cross1(net.tf_self1(flat, e, lengths), n_pcs.sum(1))
    print(f"two puzzles, {flat.shape[0]} points: descriptors {tuple(feats.shape)}, max |x| {float(feats.abs().max()):.3g}")
    assert isinstance(net.encoder, DGCNNDynamic) and feats.shape == (flat.shape[0], 128) and bool(torch.isfinite(feats).all())
    assert torch.equal(feats, want) and torch.equal(feats, again)


def test_generate_matching_data_reads_a_dgcnn_checkpoint(dev, hip_lib, tmp_path):
    from pfpp_hip import generate_matching_data as gen
    from pfpp_hip import io as pfio

    tf, mc = load_cases("matching_transformer_cases"), load_cases("matching_cases")
    sd = descriptor_state_dict()
    head = mc.head_state_dict()
    head.update(tf.classifier_state_dict())
    pts, n_pcs, valids = two_puzzles()
    # the seeded weights of this network give descriptors whose classifier logits all fall on one side of 0.  The classifier's bias is
    # set to minus the median of the logits of the descriptors themselves, so that about half the points are critical and the affinity,
    # the Sinkhorn sweeps and the assignment behind this encoder work on real matrices
    from pfpp_hip.matching import DescriptorNetwork

    net = DescriptorNetwork(encoder="dgcnn.dynamic")
    net.load_state_dict(sd, strict=True)
    f = net.to(dev)([torch.from_numpy(p).to(dev) for p in pts], n_pcs, valids).cpu().double().numpy()
    s = head["pc_classifier.0.weight"].astype(np.float64) / np.sqrt(head["pc_classifier.0.running_var"].astype(np.float64) + 1e-5)
    h = np.maximum(f * s + (head["pc_classifier.0.bias"] - head["pc_classifier.0.running_mean"] * s), 0.0)
    logits = h @ head["pc_classifier.2.weight"].astype(np.float64).reshape(-1)
    print(f"logits without the bias: {logits.min():.4g} .. {logits.max():.4g}, median {np.median(logits):.4g}")
    head["pc_classifier.2.bias"] = np.asarray([-np.median(logits)], dtype=np.float32)
    sd.update(tensors(head))
    torch.save({"state_dict": sd, "hyper_parameters": {"cfg": {"MODEL": {"ENCODER": "dgcnn.dynamic"}}}}, tmp_path / "dgcnn.ckpt")
    points = tmp_path / "points"
    points.mkdir()
    for d, (p, n, v) in enumerate(zip(pts, n_pcs, valids), 41):
        np.savez(points / f"{d}.npz", part_pcs=p, gt_pcs=p, n_pcs=n, part_valids=v)
    assert gen.main(["--points", str(points), "--checkpoint", str(tmp_path / "dgcnn.ckpt"), "--out", str(tmp_path / "out"), "--batch-size", "2"]) == 0
    total = 0
    for d, (p, n) in enumerate(zip(pts, n_pcs), 41):
        m = pfio.load_matching_data(str(tmp_path / "out" / f"{d}.npz"))
        n_crit = np.asarray(m["n_critical_pcs"])
        total += int(n_crit.sum())
        print(f"{d}.npz: {np.asarray(m['edges']).shape[0]} edges, critical points per piece {n_crit.tolist()}")
        assert np.array_equal(np.asarray(m["n_pcs"]), n) and np.asarray(m["gt_pc_by_area"]).shape == p.shape
        assert np.asarray(m["critical_pcs_idx"]).shape == (len(p),) and (n_crit <= n).all() and np.asarray(m["edges"]).shape[1:] == (2,)
    assert 0.25 * len(logits) < total < 0.75 * len(logits)
