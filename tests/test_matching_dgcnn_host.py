"""CPU: the host side of the matcher's DGCNN encoder (pfpp_hip/matching_dgcnn.py, build_encoder and DescriptorNetwork's encoder
selection in pfpp_hip/matching.py) and the test-side oracle of tests/matching_dgcnn_cases.py against tests/golden/matching_dgcnn.npz,
which tools/make_matching_dgcnn_goldens.py wrote from the reference's own module.

The float64 restatement in the reference's form must reproduce the fixture (its neighbour sets exactly, its float64 values to 1e-12
of the maximum: the same operations in another order at 2^-53), and the decomposed form the kernels compute must equal the direct one
in float64 to 1e-13 of the maximum on the same lists (the algebra, padded slots and negative scales included).  Every test prints what
it measured before it asserts."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("pfpp_dgcnn_knn", "pfpp_dgcnn_edge_max", "pfpp_leaky_relu")
KEYS = ("x1", "x2", "x3", "x4", "out")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_dgcnn_cases", ROOT / "tests" / "matching_dgcnn_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_R64 = {}


def restated64(name):
    """the float64 restatement in the reference's form with its own search, computed once and left unchanged"""
    if name not in _R64:
        x, lengths = cases.case_arrays(name)
        _R64[name] = (cases.restate(cases.state_dict(), x, lengths, torch.float64), x, lengths)
    return _R64[name]


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_restatement_in_float64_equals_the_reference(golden, name):
    g = golden("matching_dgcnn")
    r, x, lengths = restated64(name)
    N = len(x)
    assert int(g[f"{name}_seed"]) == cases.SEEDS[name] and N == int(np.sum(cases.LENGTHS[name]))
    steps = g[f"{name}_min_step"]
    print(f"{name}: N = {N}, seed {int(g[f'{name}_seed'])}; smallest 20th/21st key step per level {steps}")
    assert steps.shape == (4,) and (steps >= cases.MIN_STEP).all()
    for l in range(4):
        want = g[f"{name}_l{l + 1}_knn"].astype(np.int64)
        assert want.shape == (N, cases.K)
        same = np.array_equal(np.sort(r["knn"][l], 1), np.sort(want, 1))
        print(f"{name} level {l + 1}: restated neighbour sets {'==' if same else '!='} the reference's; {int((want == N).sum())} padded slots")
        assert same
        short = np.repeat(np.asarray(cases.LENGTHS[name]), cases.LENGTHS[name])
        assert np.array_equal((want == N).sum(1), np.maximum(cases.K - short, 0))
    for key in KEYS:
        want = g[f"{name}_{key}"]
        got = r[key].numpy().reshape(-1)[::int(g[f"stride_{key}"])]
        err = float(np.abs(got - want).max() / float(g[f"{name}_{key}_max"]))
        print(f"{name} {key}: restated float64 vs the reference's float64 {err:.3g} of the maximum (bar 1e-12)")
        assert want.dtype == np.float64 and got.shape == want.shape and err <= 1e-12


@pytest.mark.parametrize("name", ["tiny", "mixed"])
def test_decomposed_form_equals_the_direct_form_in_float64(golden, name):
    g = golden("matching_dgcnn")
    direct, x, lengths = restated64(name)
    idx = [g[f"{name}_l{l + 1}_knn"].astype(np.int64) for l in range(4)]
    sd = cases.state_dict()
    a = cases.restate(sd, x, lengths, torch.float64, indices=idx, form="direct")
    b = cases.restate(sd, x, lengths, torch.float64, indices=idx, form="split")
    neg = [int((sd[f"bn{l}.weight"] < 0).sum()) for l in range(1, 5)]
    print(f"{name}: negative BatchNorm scales per level {neg} of {cases.WIDTHS}")
    assert all(0.15 * c < n < 0.45 * c for n, c in zip(neg, cases.WIDTHS))
    for key in KEYS:
        top = float(a[key].abs().max())
        err = float((a[key] - b[key]).abs().max()) / top
        print(f"{name} {key}: decomposed vs direct {err:.3g} of the maximum (bar 1e-13)")
        assert err <= 1e-13
        assert float((a[key] - direct[key]).abs().max()) / top <= 1e-12


def test_numpy_search_orders_ties_by_index_and_fills_short_pieces():
    rows = cases.knn_tie_rows(64)
    idx, _ = cases.feat_knn(rows, cases.TIE_LENGTHS)
    N = len(rows)
    assert (idx[:7, :7].min() >= 0) and (idx[:7, :7].max() < 7) and (idx[:7, 7:] == N).all()
    for q in range(7, 7 + 19):
        assert set(idx[q, :19]) == set(range(7, 7 + 19)) and idx[q, 19] == 7 + 24, idx[q]
    for q in (7 + 24, 7 + 25, 7 + 60):
        assert list(idx[q, :3]) == [7 + 24, 7 + 25, 7 + 60]


def test_numpy_edge_extremum_covers_both_padded_winners():
    uv, idx, scale, shift = cases.edge_case(64)
    y = cases.edge_max_f32(uv, idx, scale, shift)
    N = len(uv)
    assert (scale < 0).any() and (scale == 0).any() and (scale > 0).any() and (idx[:3, 3:] == N).all()
    even_pos, odd_neg = (np.arange(64) % 2 == 0) & (scale > 0), (np.arange(64) % 2 == 1) & (scale < 0)
    assert even_pos.any() and odd_neg.any()
    act = lambda t: np.where(t > 0, t, t * np.float32(0.2))
    # the padded slot's 0 wins: the output is LeakyReLU(0 scale + shift) = LeakyReLU(shift)
    assert np.array_equal(y[:3][:, even_pos], np.broadcast_to(act(shift[even_pos]), (3, int(even_pos.sum()))))
    assert np.array_equal(y[:3][:, odd_neg], np.broadcast_to(act(shift[odd_neg]), (3, int(odd_neg.sum()))))
    assert np.array_equal(y[:, scale == 0], np.broadcast_to(act(shift[scale == 0]), (N, int((scale == 0).sum()))))


def test_state_dict_has_the_references_names_and_shapes(golden):
    from pfpp_hip.matching_dgcnn import DGCNNDynamic

    g = golden("matching_dgcnn")
    want = list(zip(g["state_names"].tolist(), g["state_shapes"].tolist()))
    spec = [(k, ",".join(map(str, s))) for k, s in cases.state_dict_spec()]
    enc = DGCNNDynamic(128, False, 3)
    got = [(k, ",".join(map(str, v.shape))) for k, v in enc.state_dict().items()]
    print(f"{len(got)} state-dict entries")
    assert len(want) == 55 and spec == want and got == want
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.state_dict().items()}
    enc.load_state_dict(sd, strict=True)
    assert not enc.training and enc.conv3[1] is enc.bn3 and torch.equal(enc.bn4.running_var, sd["conv4.1.running_var"])
    # the pack follows the parameters: a write is seen, an untouched module keeps its pack
    p0 = enc._packed()
    assert enc._packed() is p0
    with torch.no_grad():
        enc.conv2[0].weight.mul_(2.0)
    p1 = enc._packed()
    assert p1 is not p0 and torch.equal(p1[2][0], 2.0 * p0[2][0]) and p1[1][0].shape == (128, 4) and p1[4][0].shape == (512, 128)
    wa, wb = sd["conv1.0.weight"][:, :3, 0], sd["conv1.0.weight"][:, 3:, 0]
    assert torch.equal(p1[1][0][:64, :3], wa) and torch.equal(p1[1][0][64:, :3], wb - wa) and (p1[1][0][:, 3] == 0).all()


def test_refusals_of_what_is_not_built():
    from pfpp_hip.matching_dgcnn import DGCNN, DGCNNDynamic

    with pytest.raises(NotImplementedError, match="global_feat=True"):
        DGCNNDynamic(128, True, 3)
    with pytest.raises(NotImplementedError, match="dense"):
        DGCNN(128, False)
    with pytest.raises(ValueError, match="f16x3.*unquantified"):
        DGCNNDynamic(128, gemm_mode="f16x3")
    enc = DGCNNDynamic(128)
    with pytest.raises(NotImplementedError, match="training a DGCNN encoder"):
        enc.train()
    assert enc.eval() is enc and not enc.training
    with pytest.raises(ValueError, match="GPU"):
        enc(torch.zeros(5, 3), [5])


def test_build_encoder_parses_the_references_arch_strings():
    from pfpp_hip.matching import DescriptorNetwork, build_encoder
    from pfpp_hip.matching_dgcnn import DGCNNDynamic
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    a = build_encoder("pointnet2_pt.msg.dynamic", 128)
    assert isinstance(a, PointNet2PTMSGDynamic) and (a.feat_in, a.feat_out) == (3, 128)
    b = build_encoder("PointNet2_PT.MSG.Dynamic", [6, 64])
    assert isinstance(b, PointNet2PTMSGDynamic) and (b.feat_in, b.feat_out) == (6, 64)
    for arch in ("dgcnn.dynamic", "DGCNN.Dynamic"):
        d = build_encoder(arch, 128, global_feat=False, in_feat_dim=3)
        assert isinstance(d, DGCNNDynamic) and d.feat_dim == 128 and d.gemm_mode == "f32"
    for arch, kw, msg in (("dgcnn", {}, "dense"), ("dgcnn.dynamic", {"global_feat": True}, "global_feat=True"),
                          ("pointnet2_pt.msg", {}, "dense"), ("pointnet2_pt.ssg.dynamic", {}, "not supported"),
                          ("pointnet2_pt.msg.dynamic", {"global_feat": True}, "global feature"), ("kpconv", {}, "is not supported")):
        with pytest.raises(NotImplementedError, match=msg):
            build_encoder(arch, 128, **kw)
    with pytest.raises(ValueError, match="f16x3"):
        build_encoder("dgcnn.dynamic", 128, gemm_mode="f16x3")
    assert isinstance(DescriptorNetwork().encoder, PointNet2PTMSGDynamic)                       # the default does not change
    net = DescriptorNetwork(encoder="dgcnn.dynamic")
    assert isinstance(net.encoder, DGCNNDynamic) and not net.training and len([k for k in net.state_dict() if k.startswith("encoder.")]) == 55
    with pytest.raises(ValueError, match="f16x3"):
        DescriptorNetwork(gemm_mode="f16x3", encoder="dgcnn.dynamic")


def _seeded(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in net.state_dict().values():
            if v.dtype.is_floating_point:
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    return {k: v.clone() for k, v in net.state_dict().items()}


def test_descriptor_network_chooses_the_encoder_from_the_checkpoint(tmp_path):
    import sys
    import types

    from pfpp_hip.matching import DescriptorNetwork, checkpoint_encoder_arch
    from pfpp_hip.matching_dgcnn import DGCNNDynamic
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    sd_dg = _seeded(DescriptorNetwork(encoder="dgcnn.dynamic"), 1)
    sd_pn = _seeded(DescriptorNetwork(), 2)
    head = {"affinity_layer.A": torch.eye(4)}                                   # the rest of the matcher is ignored
    hp = lambda arch: {"cfg": {"MODEL": {"ENCODER": arch, "PC_FEAT_DIM": 128}, "GPUS": [0]}}
    files = {
        "dg_bare.pt": ({**sd_dg, **head}, DGCNNDynamic, sd_dg),                                                   # by encoder.conv5.0.weight
        "dg_plain.ckpt": ({"state_dict": {**sd_dg, **head}, "epoch": 1}, DGCNNDynamic, sd_dg),
        "dg_hyper.ckpt": ({"state_dict": {**sd_dg, **head}, "hyper_parameters": hp("dgcnn.dynamic")}, DGCNNDynamic, sd_dg),
        "dg_flat_hyper.ckpt": ({"state_dict": {**sd_dg, **head}, "hyper_parameters": hp("DGCNN.dynamic")["cfg"]}, DGCNNDynamic, sd_dg),
        "pn_bare.pt": ({**sd_pn, **head}, PointNet2PTMSGDynamic, sd_pn),
        "pn_hyper.ckpt": ({"state_dict": {**sd_pn, **head}, "hyper_parameters": hp("pointnet2_pt.msg.dynamic")}, PointNet2PTMSGDynamic, sd_pn),
    }
    for name, (content, cls, sd) in files.items():
        torch.save(content, tmp_path / name)
        net = DescriptorNetwork.from_checkpoint(str(tmp_path / name))
        print(f"{name}: {type(net.encoder).__name__}")
        assert isinstance(net.encoder, cls) and not net.training
        assert all(torch.equal(net.state_dict()[k], v) for k, v in sd.items())
    # the file's own statement wins over the keys: a DGCNN state_dict filed under the other name dies in the strict load, and so does
    # an explicit encoder= that contradicts the file
    torch.save({"state_dict": sd_dg, "hyper_parameters": hp("pointnet2_pt.msg.dynamic")}, tmp_path / "lying.ckpt")
    with pytest.raises(RuntimeError, match="encoder"):
        DescriptorNetwork.from_checkpoint(str(tmp_path / "lying.ckpt"))
    with pytest.raises(RuntimeError, match="encoder"):
        DescriptorNetwork.from_checkpoint(str(tmp_path / "dg_bare.pt"), encoder="pointnet2_pt.msg.dynamic")
    assert checkpoint_encoder_arch({"state_dict": {}, "hyper_parameters": {"cfg": {"MODEL": {}}}}, {}) == "pointnet2_pt.msg.dynamic"
    # a real Jigsaw file holds an EasyDict whose class may not be importable here: the placeholder it loads as still answers
    class EasyDictLike(dict):
        pass

    mod = types.ModuleType("easydict_like_for_dgcnn_test")
    EasyDictLike.__module__, EasyDictLike.__qualname__, mod.EasyDictLike = mod.__name__, "EasyDictLike", EasyDictLike
    sys.modules[mod.__name__] = mod
    try:
        cfg = EasyDictLike(MODEL=EasyDictLike(ENCODER="dgcnn.dynamic"))
        torch.save({"state_dict": {**sd_pn, **head}, "hyper_parameters": EasyDictLike(cfg=cfg)}, tmp_path / "easy.ckpt")
    finally:
        del sys.modules[mod.__name__]
    with pytest.raises(RuntimeError, match="conv5"):                              # chosen by the cfg (DGCNN), so the PointNet++ keys are refused
        DescriptorNetwork.from_checkpoint(str(tmp_path / "easy.ckpt"))
    from pfpp_hip.matching_dgcnn import DGCNNDynamic as D

    enc = D.from_checkpoint(str(tmp_path / "dg_hyper.ckpt"))
    assert enc.feat_dim == 128 and all(torch.equal(enc.state_dict()[k[len("encoder."):]], v) for k, v in sd_dg.items() if k.startswith("encoder."))
    with pytest.raises(KeyError, match="not a DGCNN checkpoint"):
        D.from_checkpoint(str(tmp_path / "pn_bare.pt"))


def test_training_keeps_refusing_a_dgcnn_encoder():
    from pfpp_hip.matching import DescriptorNetwork
    from pfpp_hip.matching_encoder_train import DescriptorTrainEngine
    from pfpp_hip.matching_fit import MatcherTrainer, default_config

    with pytest.raises(NotImplementedError, match="forward in eval mode exists.*training step.*does not"):
        DescriptorTrainEngine(DescriptorNetwork(encoder="dgcnn.dynamic"))
    cfg = default_config()
    cfg["MODEL"]["ENCODER"] = "dgcnn.dynamic"
    with pytest.raises(NotImplementedError, match="forward in eval mode exists.*training step does not"):
        MatcherTrainer(cfg)


def test_header_declares_the_entries_and_arguments_are_checked_before_a_launch(hip_lib):
    from pfpp_hip import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pfpp.h").read_text(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} not declared in include/pfpp.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.pfpp_version() == 2
    n_entries = len(re.findall(r"^(?:int|int64_t|const char\*|unsigned)\s+pfpp_\w+\s*\(", text, flags=re.M))
    readme = (ROOT / "README.md").read_text()
    print(f"{n_entries} entry points declared")
    assert f"{n_entries} entry points" in readme
    one = C.c_void_p(4096)            # a non-null, 16-byte aligned address that is never dereferenced on these paths
    odd = C.c_void_p(4100)
    f = C.c_float
    # pfpp_dgcnn_knn(feats, ld, piece_off, P, N, C, K, max_n, idx, stream)
    knn = lib.pfpp_dgcnn_knn
    assert knn(one, 512, one, 3, 0, 128, 20, 0, one, None) == 0                                   # no row: nothing to do
    assert knn(None, 512, one, 3, 100, 128, 20, 50, one, None) == -1 and b"null" in lib.pfpp_last_error()
    assert knn(one, 512, None, 3, 100, 64, 20, 50, one, None) == -1 and knn(one, 512, one, 3, 100, 3, 20, 50, None, None) == -1
    for c in (2, 4, 32, 256):
        assert knn(one, 512, one, 3, 100, c, 20, 50, one, None) == -2 and b"3, 64 or 128" in lib.pfpp_last_error()
    for k in (16, 19, 21, 32):
        assert knn(one, 512, one, 3, 100, 64, k, 50, one, None) == -2 and b"K must be 20" in lib.pfpp_last_error()
    assert knn(one, 512, one, 3, 10000, 128, 20, 8193, one, None) == -2 and b"8192" in lib.pfpp_last_error()
    assert knn(one, 512, one, 70000, 100000, 128, 20, 50, one, None) == -2 and b"65536" in lib.pfpp_last_error()
    assert knn(one, 512, one, 3, (1 << 31) // 20, 3, 20, 50, one, None) == -2 and b"int32" in lib.pfpp_last_error()
    assert knn(one, 62, one, 3, 100, 64, 20, 50, one, None) == -1 and knn(one, 2, one, 3, 100, 3, 20, 50, one, None) == -1      # stride below the width
    assert knn(odd, 512, one, 3, 100, 64, 20, 50, one, None) == -1 and knn(one, 66, one, 3, 100, 64, 20, 50, one, None) == -1   # rows not 16-byte aligned
    assert knn(one, 512, one, 3, 100, 128, 20, 200, one, None) == -1                              # a piece larger than the whole
    assert knn(one, 512, one, 3, 100, 64, 20, 50, odd, None) == -1                                # idx rows not 16-byte aligned
    # pfpp_dgcnn_edge_max(uv, ld, idx, scale, shift, slope, N, C_out, K, out, ldo, stream)
    edge = lib.pfpp_dgcnn_edge_max
    assert edge(one, 512, one, one, one, f(0.2), 0, 256, 20, one, 512, None) == 0
    for bad in range(5):
        ptrs = [one] * 5
        ptrs[bad] = None
        assert edge(ptrs[0], 512, ptrs[1], ptrs[2], ptrs[3], f(0.2), 10, 256, 20, ptrs[4], 512, None) == -1 and b"null" in lib.pfpp_last_error()
    for c in (3, 32, 96, 512):
        assert edge(one, 1024, one, one, one, f(0.2), 10, c, 20, one, 512, None) == -2 and b"64, 128 or 256" in lib.pfpp_last_error()
    assert edge(one, 512, one, one, one, f(0.2), 10, 64, 16, one, 512, None) == -2 and b"K must be 20" in lib.pfpp_last_error()
    assert edge(one, 510, one, one, one, f(0.2), 10, 256, 20, one, 512, None) == -1               # uv rows narrower than [u | v]
    assert edge(one, 512, one, one, one, f(0.2), 10, 256, 20, one, 128, None) == -1               # out rows narrower than C_out
    assert edge(one, 130, one, one, one, f(0.2), 10, 64, 20, one, 512, None) == -1                # strides that break 16-byte rows
    assert edge(one, 512, one, one, one, f(0.2), 10, 64, 20, odd, 512, None) == -1 and edge(odd, 512, one, one, one, f(0.2), 10, 64, 20, one, 512, None) == -1
    assert edge(one, 512, one, one, one, f(0.2), (1 << 31) // 20, 64, 20, one, 512, None) == -2
    # pfpp_leaky_relu(x, rows, C, ld, slope, stream)
    leaky = lib.pfpp_leaky_relu
    assert leaky(one, 0, 128, 128, f(0.2), None) == 0 and leaky(None, 0, 128, 128, f(0.2), None) == 0
    assert leaky(None, 5, 128, 128, f(0.2), None) == -1 and b"null" in lib.pfpp_last_error()
    assert leaky(one, 5, 126, 128, f(0.2), None) == -1 and leaky(one, 5, 128, 124, f(0.2), None) == -1 and leaky(odd, 5, 128, 128, f(0.2), None) == -1
    assert leaky(one, -1, 128, 128, f(0.2), None) == -1
