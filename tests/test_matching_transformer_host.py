"""CPU: the host side of the matcher's point-transformer and cross-attention layers (pfpp_hip/matching_transformer.py,
pfpp_hip.matching.DescriptorNetwork) and the test-side oracle of tests/matching_transformer_cases.py against
tests/golden/matching_transformer.npz, which tools/make_matching_transformer_goldens.py wrote from the reference's own modules.

The restatement in float32 must equal the fixture's reference outputs within 4 x the recorded deviation of the reference's float32
run from its float64 run (the rule of DESIGN.md 5.4 / 5.5: the same operations in another order) and reproduce its neighbour
indices exactly.  The smallest relative step between two different neighbour distances of the cases is 1.7e-6 (recorded in the
fixture): the float32 projections in front of the search are those of torch's CPU linear layer here and there.  Every test prints
what it measured before it asserts."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("pfpp_feat_knn", "pfpp_ptf_aggregate", "pfpp_attn_rows16", "pfpp_layernorm128")
FLOOR = 4.0 * 2.0 ** -23


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_transformer_cases", ROOT / "tests" / "matching_transformer_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_R32 = {}


def restated32(name):
    """the float32 restatement of both layers on a case, computed once and left unchanged"""
    if name not in _R32:
        p, x, lengths, puz = cases.case_arrays(name)
        r = cases.ptf_restate(cases.ptf_state_dict(), p, x, lengths, torch.float32)
        r.update({f"cross_{k}" if k == "out" else k: v for k, v in cases.cross_restate(cases.cross_state_dict(), x, puz, torch.float32).items()})
        _R32[name] = r
    return _R32[name]


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.mark.parametrize("name", ["tiny", "pair"])
def test_restatement_in_float32_equals_the_reference(golden, name):
    g = golden("matching_transformer")
    r = restated32(name)
    N = r["out"].shape[0]
    for key in ("idx_k", "idx_v"):
        same = np.array_equal(r[key], g[f"{name}_{key}"].astype(np.int64))
        print(f"{name} {key}: restated {'==' if same else '!='} the reference's ({N} rows; smallest distance step {float(g[f'{name}_knn_gap']):.3g})")
        assert same
    for key in ("p_r", "w", "out", "att", "ln1", "cross_out"):
        want = g[f"{name}_{key}"].astype(np.float64)
        got = r[key].double().numpy().reshape(-1)[::int(g[f"stride_{key}"])]
        dev, scale = float(g[f"{name}_{key}_refdev"]), float(g[f"{name}_{key}_max"])
        err = float(np.abs(got - want).max() / scale)
        bar = max(4.0 * dev, FLOOR)
        print(f"{name} {key}: restatement vs reference {err:.3g} of the maximum, reference fp32 vs fp64 {dev:.3g}, bar {bar:.3g}")
        assert got.shape == want.shape and err <= bar


def test_restated_key_reproduces_padding_order_and_tie(golden):
    g = golden("matching_transformer")
    p, x, lengths, _ = cases.case_arrays("tiny")
    N = len(x)
    r = restated32("tiny")
    off = np.concatenate([[0], np.cumsum(lengths)])
    for key, rows in (("idx_k", r["x_k"].numpy()), ("idx_v", r["x_v"].numpy())):
        idx, gap = cases.feat_knn_f32(rows, lengths)
        want = g[f"tiny_{key}"].astype(np.int64)
        assert np.array_equal(idx, want)
        # the 5-point piece: five neighbours, eleven slots of the fill value N
        assert (want[:5, :5] < 5).all() and (want[:5, 5:] == N).all() and int((want == N).sum()) == 55
        assert all(sorted(want[i, :5]) == list(range(5)) for i in range(5))
        # every index stays inside the row's piece; ascending by the float32 key
        piece = np.repeat(np.arange(len(lengths)), lengths)
        real = want != N
        assert (piece[np.where(real, want, 0)] == piece[:, None])[real].all()
        a = rows.astype(np.float32)
        d = np.zeros((N, 16), dtype=np.float32)
        nb = a[np.where(real, want, 0)]
        for c in range(128):
            t = a[:, None, c] - nb[:, :, c]
            d = d + t * t
        d = np.where(real, d, np.float32(3e38))                # the fill slots come last
        assert (np.diff(d, axis=1) >= 0).all()
        # the tie: two identical rows of the 17-point piece are at distance exactly 0 from each other; the lower index comes first
        lo, hi = off[cases.TIE_PIECE] + cases.TIE_ROWS[0], off[cases.TIE_PIECE] + cases.TIE_ROWS[1]
        assert np.array_equal(rows[lo], rows[hi]) and d[lo, 1] == 0 and d[hi, 1] == 0
        assert want[lo, :2].tolist() == [lo, hi] and want[hi, :2].tolist() == [lo, hi]
        self_first = float((want[:, 0] == np.arange(N)).mean())
        print(f"tiny {key}: slot 0 is the row itself for {100 * self_first:.1f} % of the rows (all but the upper row of the tie); "
              f"smallest step {gap.min():.3g}")
        assert int((want[:, 0] != np.arange(N)).sum()) == 1
    differ = float((g["tiny_idx_k"] != g["tiny_idx_v"]).any(1).mean())
    print(f"idx_k and idx_v differ in {100 * differ:.1f} % of the rows")
    assert differ > 0.5


def test_state_dict_names_and_shapes_are_the_references(golden):
    from pfpp_hip.matching import CrossAttentionLayer, DescriptorNetwork, PointTransformerLayer

    g, ge = golden("matching_transformer"), golden("matching_encoder")
    shapes = lambda names, shp: [(str(k), tuple(int(v) for v in str(s).split(",") if v)) for k, s in zip(names, shp)]
    want_self, want_cross = shapes(g["self_state_names"], g["self_state_shapes"]), shapes(g["cross_state_names"], g["cross_state_shapes"])
    want_enc = shapes(ge["state_names"], ge["state_shapes"])
    got = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got(PointTransformerLayer(128, 128, n_heads=8, nsampmle=16)) == want_self == [(k, tuple(s)) for k, s in cases.ptf_state_dict_spec()]
    assert got(CrossAttentionLayer(128, 8)) == want_cross == [(k, tuple(s)) for k, s in cases.cross_state_dict_spec()]
    assert "linear_p.1.running_var" in dict(want_self) and "linear_w.3.num_batches_tracked" in dict(want_self)
    want_net = ([(f"encoder.{k}", s) for k, s in want_enc] + [(f"tf_self1.{k}", s) for k, s in want_self]
                + [(f"tf_cross1.{k}", s) for k, s in want_cross])
    assert got(DescriptorNetwork()) == want_net
    PointTransformerLayer(128, 128).load_state_dict(tensors(cases.ptf_state_dict()), strict=True)
    CrossAttentionLayer(128, 8).load_state_dict(tensors(cases.cross_state_dict()), strict=True)


def descriptor_state_dict():
    spec = importlib.util.spec_from_file_location("matching_encoder_cases", ROOT / "tests" / "matching_encoder_cases.py")
    enc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(enc)
    sd = {f"encoder.{k}": v for k, v in enc.encoder_state_dict().items()}
    sd.update({f"tf_self1.{k}": v for k, v in cases.ptf_state_dict().items()})
    sd.update({f"tf_cross1.{k}": v for k, v in cases.cross_state_dict().items()})
    return tensors(sd)


def test_from_checkpoint_round_trips_a_synthetic_checkpoint(tmp_path):
    from pfpp_hip.matching import DescriptorNetwork

    sd = descriptor_state_dict()
    full = dict(sd)
    full.update({"pc_classifier.0.weight": torch.zeros(128), "affinity_layer.A": torch.eye(4)})
    torch.save({"state_dict": full, "epoch": 3}, tmp_path / "jigsaw.ckpt")
    torch.save(full, tmp_path / "bare.pt")
    for f in ("jigsaw.ckpt", "bare.pt"):
        net = DescriptorNetwork.from_checkpoint(str(tmp_path / f), gemm_mode="f16x3")
        assert net.gemm_mode == net.encoder.gemm_mode == net.tf_self1.gemm_mode == net.tf_cross1.gemm_mode == "f16x3"
        assert not net.training and all(torch.equal(net.state_dict()[k], v) for k, v in sd.items())
    torch.save({"state_dict": {k: v for k, v in full.items() if k != "tf_self1.linear_w.3.running_var"}}, tmp_path / "short.ckpt")
    with pytest.raises(RuntimeError, match="tf_self1.linear_w.3.running_var"):
        DescriptorNetwork.from_checkpoint(str(tmp_path / "short.ckpt"))


def test_packing_folds_the_batchnorms_and_is_rebuilt_after_a_write():
    from pfpp_hip.matching_transformer import PTF_WEIGHT_FLOATS, CrossAttentionLayer, PointTransformerLayer

    sd = cases.ptf_state_dict()
    layer = PointTransformerLayer(128, 128)
    layer.load_state_dict(tensors(sd), strict=True)
    pack = layer._packed()
    assert pack is layer._packed() and pack["wp"].shape == (PTF_WEIGHT_FLOATS,) and pack["w_qkv"].shape == (384, 128)
    assert torch.equal(pack["w_qkv"][128:256], layer.linear_k.weight) and torch.equal(pack["b_qkv"][256:], layer.linear_v.bias)
    wp = pack["wp"].double().numpy()
    # the folded linear_w[2] + BatchNorm(16) against torch in float64
    x = torch.randn(7, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    lw = PointTransformerLayer(128, 128)
    lw.load_state_dict(tensors(sd), strict=True)
    lw.double()
    with torch.no_grad():
        want = lw.linear_w[3](lw.linear_w[2](x)[:, :, None])[:, :, 0].numpy()
        want_p = lw.linear_p[1](lw.linear_p[0](x[:, :3])[:, :, None])[:, :, 0].numpy()
    got = (x.numpy() @ wp[788:2836].reshape(16, 128).T) * wp[2836:2852] + wp[2852:2868]
    got_p = (x.numpy()[:, :3] @ wp[0:9].reshape(3, 3).T) * wp[12:15] + wp[16:19]
    err = max(float(np.abs(got - want).max()), float(np.abs(got_p - want_p).max()))
    print(f"folded BatchNorms of linear_w / linear_p vs torch (float64 of the float32 pack): {err:.3g}")
    assert err < 1e-5
    assert np.array_equal(wp[3124:3140].astype(np.float32), sd["linear_w.5.bias"]) and np.array_equal(wp[404:532].astype(np.float32), sd["linear_p.3.bias"])
    with torch.no_grad():
        layer.linear_w[3].running_var.mul_(2.0)                 # an in-place write to a buffer
    pack2 = layer._packed()
    assert pack2 is not pack and not torch.equal(pack2["wp"][2836:2852], pack["wp"][2836:2852]) and torch.equal(pack2["wp"][:2836], pack["wp"][:2836])
    cross = CrossAttentionLayer(128, 8)
    cross.load_state_dict(tensors(cases.cross_state_dict()), strict=True)
    c1 = cross._packed()
    assert c1 is cross._packed() and torch.equal(c1["w_qkv"][256:], cross.attn.w_vs.weight)
    before = c1["bw2"].clone()
    with torch.no_grad():
        cross.pos_ffn.w_2.bias.add_(1.0)
    c2 = cross._packed()
    assert c2 is not c1 and torch.equal(c2["bw2"], before + 1.0)


def test_eval_mode_only_unsupported_configurations_and_no_cpu_path():
    from pfpp_hip.matching import DescriptorNetwork
    from pfpp_hip.matching_transformer import CrossAttentionLayer, PointTransformerLayer, attn_rows16, feat_knn, ptf_aggregate

    for m in (PointTransformerLayer(128, 128), CrossAttentionLayer(128, 8), DescriptorNetwork()):
        assert not m.training and m.eval() is m and m.train(False) is m
        with pytest.raises(NotImplementedError, match="matcher training"):
            m.train()
        with pytest.raises(NotImplementedError):
            m.train(True)
    for args, what in (((64, 64), "128"), ((128, 64), "out_feat"), ((128, 128, 4), "n_heads"), ((128, 128, 8, 8), "nsampmle")):
        with pytest.raises(ValueError, match=what):
            PointTransformerLayer(*args)
    for args, what in (((64, 4), "d_in"), ((128, 4), "n_head")):
        with pytest.raises(ValueError, match=what):
            CrossAttentionLayer(*args)
    with pytest.raises(ValueError, match="gemm_mode"):
        PointTransformerLayer(128, 128, gemm_mode="bf16")
    with pytest.raises(ValueError, match="gemm_mode"):
        CrossAttentionLayer(128, 8, gemm_mode="bf16")
    with pytest.raises(ValueError, match="GPU"):
        PointTransformerLayer(128, 128)(torch.zeros(8, 3), torch.zeros(8, 128), [8])
    with pytest.raises(ValueError, match="GPU"):
        CrossAttentionLayer(128, 8)(torch.zeros(8, 128), [8])
    with pytest.raises(ValueError, match="GPU"):
        DescriptorNetwork()(torch.zeros(8, 3), np.asarray([[8]]), np.asarray([[1.0]]))
    with pytest.raises(ValueError, match="GPU"):
        feat_knn(torch.zeros(8, 128), torch.zeros(2, dtype=torch.int64), 8)
    with pytest.raises(ValueError, match="GPU"):
        ptf_aggregate(torch.zeros(8, 384), torch.zeros(8, 3), torch.zeros(8, 16, dtype=torch.int32), torch.zeros(8, 16, dtype=torch.int32), torch.zeros(3140))
    with pytest.raises(ValueError, match="GPU"):
        attn_rows16(torch.zeros(8, 384), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 8, 8, 0.25)


def test_header_declares_the_entries_and_arguments_are_checked_before_a_launch(hip_lib):
    from pfpp_hip import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pfpp.h").read_text(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} not declared in include/pfpp.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.pfpp_version() == 2 and "#define PFPP_PTF_WEIGHT_FLOATS 3140" in text
    one = C.c_void_p(4096)            # a non-null, 16-byte aligned address that is never dereferenced on these paths
    f = C.c_float
    # pfpp_feat_knn(feats, ld, piece_off, P, N, C, K, max_n, idx, stream)
    assert lib.pfpp_feat_knn(one, 384, one, 3, 0, 128, 16, 0, one, None) == 0                        # no row: nothing to do
    assert lib.pfpp_feat_knn(None, 384, one, 3, 100, 128, 16, 50, one, None) == -1 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_feat_knn(one, 384, one, 3, 100, 64, 16, 50, one, None) == -2 and b"128" in lib.pfpp_last_error()
    assert lib.pfpp_feat_knn(one, 384, one, 3, 100, 128, 32, 50, one, None) == -2 and b"K must be 16" in lib.pfpp_last_error()
    assert lib.pfpp_feat_knn(one, 384, one, 3, 10000, 128, 16, 9000, one, None) == -2 and b"8192" in lib.pfpp_last_error()
    assert lib.pfpp_feat_knn(one, 126, one, 3, 100, 128, 16, 50, one, None) == -1                    # row stride below the width
    assert lib.pfpp_feat_knn(C.c_void_p(4100), 384, one, 3, 100, 128, 16, 50, one, None) == -1       # rows not 16-byte aligned
    assert lib.pfpp_feat_knn(one, 384, one, 3, 100, 128, 16, 200, one, None) == -1                   # a piece larger than the whole
    assert lib.pfpp_feat_knn(one, 384, one, 70000, 100000, 128, 16, 50, one, None) == -2 and b"65536" in lib.pfpp_last_error()
    # pfpp_ptf_aggregate(q, k, v, ld, xyz, idx_k, idx_v, weights, N, C, K, out, stream)
    assert lib.pfpp_ptf_aggregate(one, one, one, 384, one, one, one, one, 0, 128, 16, one, None) == 0
    assert lib.pfpp_ptf_aggregate(one, one, one, 384, one, one, None, one, 10, 128, 16, one, None) == -1 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_ptf_aggregate(one, one, one, 384, one, one, one, one, 10, 96, 16, one, None) == -2
    assert lib.pfpp_ptf_aggregate(one, one, one, 384, one, one, one, one, 10, 128, 8, one, None) == -2
    assert lib.pfpp_ptf_aggregate(one, one, one, 100, one, one, one, one, 10, 128, 16, one, None) == -1
    assert lib.pfpp_ptf_aggregate(one, one, one, 384, one, one, one, one, -1, 128, 16, one, None) == -1
    # pfpp_attn_rows16(qkv, out, seq_off, seq_len, n_seq, max_len, H, dh, scale, stream)
    assert lib.pfpp_attn_rows16(one, one, one, one, 0, 10, 8, 16, f(0.25), None) == 0
    assert lib.pfpp_attn_rows16(one, one, one, one, 2, 10, 8, 32, f(0.25), None) == -2 and b"16" in lib.pfpp_last_error()
    assert lib.pfpp_attn_rows16(one, None, one, one, 2, 10, 8, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16(one, one, one, one, 2, 0, 8, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16(C.c_void_p(4104), one, one, one, 2, 10, 8, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16(one, one, one, one, 70000, 10, 8, 16, f(0.25), None) == -2
    # pfpp_layernorm128(x, gamma, beta, out, rows, C, eps, stream); the existing LayerNorm keeps its widths
    assert lib.pfpp_layernorm128(one, one, one, one, 0, 128, f(1e-6), None) == 0
    assert lib.pfpp_layernorm128(one, one, one, one, 10, 256, f(1e-6), None) == -2 and b"128" in lib.pfpp_last_error()
    assert lib.pfpp_layernorm128(one, None, one, one, 10, 128, f(1e-6), None) == -1
    assert lib.pfpp_layernorm128(one, one, one, one, 10, 128, f(-1.0), None) == -1
    assert lib.pfpp_layernorm(one, one, None, 0, one, one, 10, 128, 1, f(1e-6), None) == -2
    # the existing dense attention keeps refusing 16-wide heads
    assert lib.pfpp_attn_dense(one, one, one, one, None, 0, 2, 10, 8, 16, f(0.25), None) == -2


def test_generate_matching_data_takes_points_or_features_not_both(tmp_path, capsys):
    from pfpp_hip import generate_matching_data as G

    (tmp_path / "in").mkdir()
    ckpt = tmp_path / "c.ckpt"
    ckpt.write_bytes(b"")
    base = ["--checkpoint", str(ckpt), "--out", str(tmp_path / "out")]
    for argv, what in ((base, "one of the arguments --points --features is required"),
                       (["--points", str(tmp_path / "in"), "--features", str(tmp_path / "in")] + base, "not allowed with argument"),
                       (["--points", str(tmp_path / "missing")] + base, "--points"), (["--features", str(tmp_path / "missing")] + base, "--features")):
        with pytest.raises(SystemExit) as e:
            G.main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and what in err, err
    # an empty directory: nothing to do, whichever kind it is (no GPU is touched)
    assert G.main(["--points", str(tmp_path / "in")] + base) == 0 and G.main(["--features", str(tmp_path / "in")] + base) == 0
    np.savez(tmp_path / "in" / "7.npz", part_pcs=np.zeros((5, 3), np.float32), gt_pcs=np.zeros((5, 3), np.float32), n_pcs=np.asarray([3, 2]),
             part_valids=np.ones(2, np.float32))
    x = G.load_features(str(tmp_path / "in"), 7, points=True)
    assert x["part_pcs"].shape == (5, 3)
    with pytest.raises(KeyError, match="part_feats"):
        G.load_features(str(tmp_path / "in"), 7)
    assert G.list_puzzles(str(tmp_path / "in"), str(tmp_path / "out")) == ([7], [])
