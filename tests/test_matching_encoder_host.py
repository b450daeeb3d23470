"""CPU: the host side of the matcher's ragged PointNet++ encoder (pfpp_hip/matching_encoder.py): the state_dict layout and the
sample-count rule against tests/golden/matching_encoder.npz (written by tools/make_matching_encoder_goldens.py from the reference's
module), BatchNorm folding against torch, the eval-only contract, the checkpoint reader and the new entries of include/pfpp.h."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("pfpp_ragged_fps", "pfpp_ragged_knn", "pfpp_ragged_group", "pfpp_ragged_interp")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_encoder_cases", ROOT / "tests" / "matching_encoder_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()


def test_state_dict_names_and_shapes_are_the_references(golden):
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    g = golden("matching_encoder")
    want = [(str(k), tuple(int(v) for v in str(s).split(",") if v)) for k, s in zip(g["state_names"], g["state_shapes"])]
    enc = PointNet2PTMSGDynamic(3, 128)
    got = [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    assert got == want
    assert got == [(k, tuple(s)) for k, s in cases.state_dict_spec()]
    assert "sa1.conv_blocks.0.0.weight" in dict(got) and "sa1.bn_blocks.0.0.running_mean" in dict(got)
    assert dict(got)["fp4.mlp_convs.0.weight"] == (256, 1536, 1) and dict(got)["conv1.weight"] == (128, 128, 1)
    n_par = sum(int(np.prod(s)) for k, s in got if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
    assert 1.8e6 < n_par < 2.0e6


def test_strict_load_and_checkpoint_reader(tmp_path):
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.encoder_state_dict().items()}
    enc = PointNet2PTMSGDynamic()
    enc.load_state_dict(sd, strict=True)
    assert not enc.training and torch.equal(enc.sa3.conv_blocks[1][1].weight, sd["sa3.conv_blocks.1.1.weight"])
    with pytest.raises(RuntimeError, match="conv1.bias"):
        PointNet2PTMSGDynamic().load_state_dict({k: v for k, v in sd.items() if k != "conv1.bias"}, strict=True)
    full = {f"encoder.{k}": v for k, v in sd.items()}
    full.update({"pc_classifier.0.weight": torch.zeros(128), "tf_self1.linear_q.weight": torch.zeros(8, 8)})
    torch.save({"state_dict": full, "epoch": 3}, tmp_path / "jigsaw.ckpt")
    torch.save(full, tmp_path / "bare.pt")
    for f in ("jigsaw.ckpt", "bare.pt"):
        e = PointNet2PTMSGDynamic.from_checkpoint(str(tmp_path / f), gemm_mode="f16x3")
        assert e.gemm_mode == "f16x3" and all(torch.equal(e.state_dict()[k], v) for k, v in sd.items())
    torch.save({"state_dict": {k: v for k, v in full.items() if k != "encoder.fp1.mlp_bns.2.running_var"}}, tmp_path / "short.ckpt")
    with pytest.raises(RuntimeError, match="fp1.mlp_bns.2.running_var"):
        PointNet2PTMSGDynamic.from_checkpoint(str(tmp_path / "short.ckpt"))


def test_sample_counts_follow_the_float32_rule(golden):
    from pfpp_hip.matching_encoder import level_counts, sample_count

    g = golden("matching_encoder")
    n = g["count_n"]
    assert np.array_equal(sample_count(n, 0.15), g["count_015"].astype(np.int64))
    assert np.array_equal(sample_count(n, 0.25), g["count_025"].astype(np.int64))
    assert sample_count(100, 0.15) == 16 and sample_count(200, 0.15) == 31 and sample_count(20, 0.15) == 3 and sample_count(340, 0.15) == 52
    exact = -(-(n * 15) // 100)                                  # ceil(0.15 n) in exact arithmetic
    assert int((sample_count(n, 0.15) != exact).sum()) == 81     # the float32 product lands above an integer 81 times up to 5000
    lc = level_counts([30, 33, 64, 65, 200, 417])
    assert lc.tolist() == [[30, 33, 64, 65, 200, 417], [5, 5, 10, 10, 31, 63], [2, 2, 3, 3, 8, 16], [1, 1, 1, 1, 2, 4], [1, 1, 1, 1, 1, 1]]
    assert level_counts([4970, 30])[1].tolist() == [746, 5]
    for name in ("small", "second"):
        lengths = np.concatenate([pz["lengths"] for pz in cases.make_case(name)])
        for l in range(4):
            assert g[f"{name}_l{l + 1}_centroids"].size == level_counts(lengths)[l + 1].sum()


def test_batchnorm_folding_equals_torch():
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic, fold_batchnorm

    enc = PointNet2PTMSGDynamic()
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.encoder_state_dict().items()}, strict=True)
    enc.double()
    g = torch.Generator().manual_seed(0)
    for conv, bn, shape in ((enc.sa2.conv_blocks[1][0], enc.sa2.bn_blocks[1][0], (2, 99, 5, 7)), (enc.fp3.mlp_convs[0], enc.fp3.mlp_bns[0], (2, 512, 9))):
        x = torch.randn(shape, generator=g, dtype=torch.float64)
        with torch.no_grad():
            want = bn(conv(x))
        w, scale, shift = fold_batchnorm(conv.weight, conv.bias, bn)
        rows = x.movedim(1, -1).reshape(-1, shape[1])
        got = (rows @ w.t()) * scale + shift
        err = float((got - want.movedim(1, -1).reshape(-1, w.shape[0])).abs().max())
        print(f"folded BatchNorm vs torch (float64): {err:.3g}")
        assert err < 1e-12


def test_eval_mode_only_and_no_cpu_path():
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    enc = PointNet2PTMSGDynamic()
    assert not enc.training and enc.eval() is enc and enc.train(False) is enc
    with pytest.raises(NotImplementedError, match="matcher training"):
        enc.train()
    with pytest.raises(ValueError, match="GPU"):
        enc(torch.zeros(8, 3), [8])
    with pytest.raises(ValueError):
        PointNet2PTMSGDynamic(gemm_mode="bf16")


def test_case_points_keep_their_distance():
    """the reference's interpolation distance cancels; the cases keep every pair of a piece at least 1e-3 apart so that it never
    comes near its 1e-8 guard"""
    for name in ("small", "second"):
        for pz in cases.make_case(name):
            off = np.concatenate([[0], np.cumsum(pz["lengths"])])
            for a, b in zip(off[:-1], off[1:]):
                assert cases.min_pairwise_distance(pz["points"][a:b]) >= cases.MIN_DIST
            assert pz["points"].dtype == np.float32 and 0.3 < np.linalg.norm(pz["points"], axis=1).mean() < 0.5
            assert (pz["start"][0] > 0).all()


def test_header_declares_the_ragged_entries_and_arguments_are_checked_before_a_launch(hip_lib):
    from pfpp_hip import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pfpp.h").read_text(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} not declared in include/pfpp.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.pfpp_version() == 2
    one = C.c_void_p(16)            # a non-null, 16-byte aligned address that is never dereferenced
    assert lib.pfpp_ragged_fps(one, one, one, 0, 4, 100, one, one, None) == 0                       # no piece: nothing to do
    assert lib.pfpp_ragged_fps(None, one, one, 2, 4, 100, one, one, None) == -1
    assert lib.pfpp_ragged_fps(one, one, one, 2, 4, 9000, one, one, None) == -2                     # a piece beyond 8192 points
    assert b"8192" in lib.pfpp_last_error()
    assert lib.pfpp_ragged_knn(one, one, one, one, 2, 10, 10, 5, one, None, None) == -2             # K
    assert lib.pfpp_ragged_knn(one, one, one, one, 2, 0, 10, 16, one, None, None) == 0
    assert lib.pfpp_ragged_knn(one, None, one, one, 2, 10, 10, 16, one, None, None) == -1
    assert lib.pfpp_ragged_group(one, 96, 96, one, one, one, 32, 16, 32, 4, one, 99, None) == -1    # ldo not a multiple of 4
    assert lib.pfpp_ragged_group(one, 96, 96, one, one, one, 32, 16, 24, 4, one, 104, None) == -1   # pool % K
    assert lib.pfpp_ragged_group(one, 96, 96, one, one, one, 32, 16, 32, 0, one, 104, None) == 0
    assert lib.pfpp_ragged_interp(one, one, one, one, one, 130, None, 0, 4, 2, one, 132, None, None) == -1     # D2 % 4
    assert lib.pfpp_ragged_interp(one, one, None, None, one, 128, None, 0, 4, 2, one, 128, None, None) == -1   # S > 1 needs idx
    assert lib.pfpp_ragged_interp(one, one, one, one, one, 128, None, 0, 4, 0, one, 128, None, None) == -1     # no centroid
    assert lib.pfpp_ragged_interp(one, one, one, one, one, 128, None, 0, 0, 2, one, 128, None, None) == 0
