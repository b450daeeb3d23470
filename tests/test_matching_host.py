"""CPU: the matcher back end's host side — exported symbols and argument checks, the piece-pair rule and the file against the
reference's own output (tests/golden/matching_head.npz, written by tools/make_matching_goldens.py), the head's state_dict layout and
the generator script's argument handling.  Inputs are regenerated from tests/matching_cases.py; the fixture holds results only."""
import ctypes as C
import importlib.util
import re
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("pfpp_match_classify_compact", "pfpp_match_gather_rows", "pfpp_match_normalize_halves", "pfpp_sinkhorn_workspace",
               "pfpp_sinkhorn_masked", "pfpp_fracture_labels")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_cases", ROOT / "tests" / "matching_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()


def fixture_corr(g, name):
    cat, lens = g[f"{name}_corr_cat"].astype(np.int64), g[f"{name}_corr_len"]
    return np.split(cat, np.cumsum(lens)[:-1]) if len(lens) else []


def test_library_exports_the_matching_symbols_and_checks_arguments_before_a_launch(hip_lib):
    from pfpp_hip import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pfpp.h").read_text(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} not declared in include/pfpp.h"
        assert hasattr(lib, s) and (s in _lib.SIGNATURES or s in _lib.PLAIN)
    assert lib.pfpp_version() == 2
    # every check below returns before anything touches the device (there is none here)
    one = C.c_void_p(16)            # a non-null, 16-byte aligned address that is never dereferenced
    assert lib.pfpp_sinkhorn_workspace(-1) == -1 and lib.pfpp_sinkhorn_workspace(70000) == -1
    assert lib.pfpp_sinkhorn_workspace(0) == 0 and lib.pfpp_sinkhorn_workspace(130) == 3 * 130 * (8 + 4)
    assert lib.pfpp_sinkhorn_masked(None, 4, one, 4, 0.05, 20, one, one, one, one, 1 << 20, None) == -1                # null s
    assert lib.pfpp_sinkhorn_masked(one, 3, one, 4, 0.05, 20, one, one, one, one, 1 << 20, None) == -1                 # ld < n
    assert lib.pfpp_sinkhorn_masked(one, 4, one, 4, 0.0, 20, one, one, one, one, 1 << 20, None) == -1                  # tau
    assert lib.pfpp_sinkhorn_masked(one, 4, one, 4, 0.05, 20, one, one, one, one, 8, None) == -1                       # workspace too small
    assert b"workspace" in lib.pfpp_last_error()
    assert lib.pfpp_sinkhorn_masked(one, 70000, one, 70000, 0.05, 20, one, one, one, one, 1 << 40, None) == -2         # unsupported n
    assert lib.pfpp_match_classify_compact(one, one, one, one, 0.0, None, one, 4, 64, one, one, one, one, None) == -2  # C != 128
    assert lib.pfpp_match_classify_compact(None, None, None, None, 0.0, None, one, 4, 128, None, None, one, one, None) == -1
    assert lib.pfpp_match_classify_compact(one, one, one, one, 0.0, None, one, 0, 128, one, one, one, one, None) == 0  # nothing to do
    assert lib.pfpp_match_gather_rows(one, one, one, one, one, one, one, 4, 8, 96, one, one, None) == -2
    assert lib.pfpp_match_gather_rows(C.c_void_p(20), one, one, one, one, one, one, 4, 8, 128, one, one, None) == -1   # misaligned feats
    assert lib.pfpp_match_gather_rows(one, one, one, one, one, one, one, 4, 0, 128, one, one, None) == 0
    assert lib.pfpp_match_normalize_halves(one, 8, 256, None) == -2 and lib.pfpp_match_normalize_halves(None, 8, 512, None) == -1
    assert lib.pfpp_fracture_labels(one, one, one, None, 1, 100, None, one, None) == -1
    assert lib.pfpp_fracture_labels(one, one, one, one, 70000, 100, None, one, None) == -2
    assert lib.pfpp_fracture_labels(one, one, one, one, 0, 100, None, one, None) == 0


def test_wrappers_have_no_cpu_path(hip_lib):
    from pfpp_hip import matching

    with pytest.raises(ValueError, match="GPU"):
        matching.sinkhorn(torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        matching.fracture_labels(torch.zeros(1, 8, 3), np.array([[4, 4]]), torch.zeros(1, 8))
    with pytest.raises(ValueError, match="GPU"):
        matching.MatchingHead()(torch.zeros(1, 8, 128), np.array([[4, 4]]), np.ones((1, 2)))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_match_edges_and_file_equal_the_reference(golden, tmp_path, name):
    """the reference's compute_global_transformation on the fixture's assignment: edges and every correspondence array exactly,
    order included; the file round-trips through io.load_matching_data"""
    from pfpp_hip import io as pfio
    from pfpp_hip.matching import match_edges, write_matching_data

    g = golden("matching_head")
    pz = cases.make_puzzle(name)
    perm = g[f"{name}_perm"].astype(np.int64)
    nc = g[f"{name}_n_critical_pcs"]
    n_valid = int(pz["part_valids"].sum())
    edges, corr = match_edges(perm, nc, n_valid)
    want = fixture_corr(g, name)
    assert edges.dtype == np.int64 and np.array_equal(edges, g[f"{name}_edges"])
    assert len(corr) == len(want) and all(np.array_equal(a, b) for a, b in zip(corr, want))
    # the dense 0/1 matrix is accepted as well and gives the same
    dense = np.zeros((perm.size, perm.size), dtype=np.float32)
    dense[np.arange(perm.size), perm] = 1
    e2, c2 = match_edges(torch.from_numpy(dense), torch.from_numpy(nc), n_valid)
    assert np.array_equal(e2, edges) and all(np.array_equal(a, b) for a, b in zip(c2, corr))
    crit = g[f"{name}_critical_pcs_idx"].astype(np.int64)
    path = write_matching_data(str(tmp_path), pz["data_id"], edges=edges, correspondence=corr, gt_pcs=pz["gt_pcs"], critical_pcs_idx=crit,
                               n_pcs=pz["n_pcs"], n_critical_pcs=nc)
    assert Path(path).name == f"{pz['data_id']}.npz"
    with np.load(path, allow_pickle=True) as d:
        assert tuple(d.files) == pfio.MATCHING_KEYS
    back = pfio.load_matching_data(path)
    assert np.array_equal(back["edges"], edges) and np.array_equal(back["critical_pcs_idx"], crit)
    assert np.array_equal(back["n_pcs"], pz["n_pcs"]) and np.array_equal(back["n_critical_pcs"], nc)
    assert np.array_equal(back["gt_pc_by_area"], pz["gt_pcs"])
    assert len(back["correspondences"]) == len(corr) and all(np.array_equal(a, b) for a, b in zip(back["correspondences"], corr))
    # an existing file is left alone (the reference's _save_data returns early)
    before = Path(path).read_bytes()
    assert write_matching_data(str(tmp_path), pz["data_id"], edges=edges[:0], correspondence=[], gt_pcs=pz["gt_pcs"], critical_pcs_idx=crit,
                               n_pcs=pz["n_pcs"], n_critical_pcs=nc) is None
    assert Path(path).read_bytes() == before


def test_the_fixture_covers_the_cases_of_the_pair_rule(golden):
    g = golden("matching_head")
    nc = g["five_n_critical_pcs"]
    assert nc[4] == 0 and (nc[:4] > 0).all()                                                    # a piece with no predicted critical point
    edges = g["five_edges"].tolist()
    assert [3, 1] not in edges and [4, 0] not in edges                                          # fewer than 3 matches; an empty side
    k = edges.index([3, 0])
    c = fixture_corr(g, "five")[k]
    assert len(c) == 8 and (np.diff(c[:, 0]) > 0).all()                                         # the transposed block won: 2 + 6 matches
    # Pairs with critical points on both sides and no match reach the `mat_s == 0` rule.  Nothing here (or in any data) can tell whether
    # match_edges applies it: a pair with mat_s == 0 has no non-zero, so the `fewer than 3 non-zeros` rule behind it drops the pair anyway.
    assert g["two_edges"].tolist() == [[1, 0]] and g["split_edges"].tolist() == [[1, 0], [3, 2]]


def test_match_edges_degenerate_and_unmatched_rows():
    from pfpp_hip.matching import match_edges

    e, c = match_edges(np.zeros(0, dtype=np.int64), np.array([5, 0, 0]), 3)
    assert e.shape == (0, 2) and e.dtype == np.int64 and c == []
    # rows without a column (-1) are not matches; with two pieces a pair with no match at all is still dropped by the count
    e, c = match_edges(np.array([3, 4, 5, -1, -1, -1]), np.array([3, 3]), 2)
    assert e.tolist() == [[1, 0]] and c[0].tolist() == [[0, 0], [1, 1], [2, 2]]
    e, c = match_edges(np.full(6, -1), np.array([3, 3]), 2)
    assert e.shape == (0, 2) and c == []


def test_written_file_feeds_the_denoiser_dataset_in_test_mode(golden, tmp_path):
    from pfpp_hip import io as pfio
    from pfpp_hip.matching import match_edges, write_matching_data
    from puzzlefusion_plusplus.denoiser.dataset.dataset import GeometryLatentDataset

    g = golden("matching_head")
    pz = cases.make_puzzle("five")
    edges, corr = match_edges(g["five_perm"].astype(np.int64), g["five_n_critical_pcs"], 5)
    mdir = tmp_path / "matching_data"
    write_matching_data(str(mdir), pz["data_id"], edges=edges, correspondence=corr, gt_pcs=pz["gt_pcs"],
                        critical_pcs_idx=g["five_critical_pcs_idx"].astype(np.int64), n_pcs=pz["n_pcs"], n_critical_pcs=g["five_n_critical_pcs"])
    rng = np.random.default_rng(0)
    valids = pz["part_valids"]
    graph = np.zeros((20, 20), dtype=bool)
    ref = np.zeros(20, dtype=bool)
    ref[0] = True
    pfio.save_pc_data(str(tmp_path / "pc_data"), data_id=pz["data_id"], part_valids=valids, num_parts=5, mesh_file_path="a/b", graph=graph,
                      category="everyday", part_pcs_gt=rng.normal(size=(5, 64, 3)), ref_part=ref)
    cfg = NS(data=NS(max_num_part=20, matching_data_path=str(mdir)), model=NS(multiple_ref_parts=False))
    ds = GeometryLatentDataset(cfg, str(tmp_path / "pc_data"), -1, "test")
    assert len(ds) == 1
    item = ds[0]
    assert np.array_equal(item["edges"], edges) and len(item["correspondences"]) == len(corr)
    assert all(np.array_equal(a, b) for a, b in zip(item["correspondences"], corr))
    assert np.array_equal(item["n_critical_pcs"], g["five_n_critical_pcs"]) and item["part_pcs_by_area"].shape == pz["gt_pcs"].shape


def test_matching_head_takes_the_reference_state_dict(tmp_path):
    from pfpp_hip.matching import MatchingHead

    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}
    want = {"pc_classifier.0.weight": (128,), "pc_classifier.0.running_var": (128,), "pc_classifier.2.weight": (1, 128, 1), "pc_classifier.2.bias": (1,),
            "affinity_extractor.0.bias": (128,), "affinity_extractor.2.weight": (512, 128, 1), "affinity_extractor.2.bias": (512,),
            "affinity_layer.A": (256, 256)}
    head = MatchingHead()
    assert set(head.state_dict()) == set(sd) and all(tuple(head.state_dict()[k].shape) == s for k, s in want.items())
    head.load_state_dict(sd, strict=True)
    assert not head.training and torch.equal(head.affinity_layer.A, sd["affinity_layer.A"])
    with pytest.raises(RuntimeError):
        MatchingHead().load_state_dict({k: v for k, v in sd.items() if k != "affinity_layer.A"}, strict=True)
    # a Lightning file: the head's entries among the rest of the matcher's
    full = dict(sd)
    full.update({"encoder.sa1.conv.weight": torch.zeros(4, 4), "tf_self1.linear_q.weight": torch.zeros(8, 8), "tf_cross1.w_qs.weight": torch.zeros(8, 8)})
    torch.save({"state_dict": full, "epoch": 3}, tmp_path / "jigsaw.ckpt")
    torch.save(full, tmp_path / "bare.pt")
    for f in ("jigsaw.ckpt", "bare.pt"):
        h = MatchingHead.from_checkpoint(str(tmp_path / f), gemm_mode="f16x3")
        assert h.gemm_mode == "f16x3" and all(torch.equal(h.state_dict()[k], v) for k, v in sd.items())
    torch.save({"state_dict": {k: v for k, v in full.items() if not k.startswith("affinity_layer.")}}, tmp_path / "short.ckpt")
    with pytest.raises(RuntimeError, match="affinity_layer.A"):
        MatchingHead.from_checkpoint(str(tmp_path / "short.ckpt"))


def test_from_checkpoint_reads_a_lightning_file_with_hyper_parameters(tmp_path):
    """The reference's matcher calls save_hyperparameters() with its cfg, an EasyDict: a real Jigsaw checkpoint holds a dict subclass
    under `hyper_parameters`, which torch.load(weights_only=True) refuses.  The head's entries must load from such a file whether
    the class can be imported (easydict installed) or not."""
    import pickle
    import sys
    import types

    from pfpp_hip.matching import MatchingHead, load_checkpoint_state_dict

    class EasyDictLike(dict):
        def __init__(self, d=None):
            super().__init__()
            for k, v in (d or {}).items():
                setattr(self, k, v)

        def __setattr__(self, k, v):
            v = EasyDictLike(v) if isinstance(v, dict) and not isinstance(v, EasyDictLike) else v
            super().__setattr__(k, v)
            super().__setitem__(k, v)

        __setitem__ = __setattr__

    mod = types.ModuleType("easydict_like_for_test")
    EasyDictLike.__module__, EasyDictLike.__qualname__, mod.EasyDictLike = mod.__name__, "EasyDictLike", EasyDictLike
    sys.modules[mod.__name__] = mod
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}
    full = dict(sd)
    full["encoder.sa1.conv.weight"] = torch.zeros(4, 4)
    path = tmp_path / "jigsaw.ckpt"
    try:
        torch.save({"state_dict": full, "epoch": 3, "hyper_parameters": {"cfg": EasyDictLike({"MODEL": {"SINKHORN_TAU": 0.05}, "GPUS": [0]})},
                    "optimizer_states": [{"state": {}, "param_groups": [{"lr": 1e-3}]}]}, path)
        with pytest.raises(pickle.UnpicklingError):
            torch.load(path, map_location="cpu", weights_only=True)          # the layout really is one the strict mode refuses
        h = MatchingHead.from_checkpoint(str(path))
        assert all(torch.equal(h.state_dict()[k], v) for k, v in sd.items())
    finally:
        del sys.modules[mod.__name__]
    h = MatchingHead.from_checkpoint(str(path))                              # the class is gone: a placeholder stands in
    assert all(torch.equal(h.state_dict()[k], v) for k, v in sd.items())
    assert set(load_checkpoint_state_dict(str(path))) == set(full)
    torch.save({"hyper_parameters": {"cfg": 1}, "epoch": 3}, tmp_path / "empty.ckpt")
    with pytest.raises(RuntimeError, match="no state_dict"):
        MatchingHead.from_checkpoint(str(tmp_path / "empty.ckpt"))
    (tmp_path / "junk.ckpt").write_bytes(b"not a checkpoint")
    with pytest.raises(Exception):
        MatchingHead.from_checkpoint(str(tmp_path / "junk.ckpt"))


def test_generate_matching_data_arguments_and_skip_if_exists(tmp_path, capsys):
    from pfpp_hip import generate_matching_data as gen

    feats, out = tmp_path / "features", tmp_path / "matching_data"
    feats.mkdir()
    out.mkdir()
    ckpt = tmp_path / "head.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}, ckpt)
    for argv in ([], ["--features", str(feats), "--out", str(out)], ["--features", str(tmp_path / "nope"), "--checkpoint", str(ckpt), "--out", str(out)],
                 ["--features", str(feats), "--checkpoint", str(tmp_path / "nope.pt"), "--out", str(out)],
                 ["--features", str(feats), "--checkpoint", str(ckpt), "--out", str(out), "--batch-size", "0"],
                 ["--features", str(feats), "--checkpoint", str(ckpt), "--out", str(out), "--gemm", "bf16"]):
        with pytest.raises(SystemExit) as e:
            gen.main(argv)
        assert e.value.code == 2
    capsys.readouterr()
    assert gen.main(["--features", str(feats), "--checkpoint", str(ckpt), "--out", str(out)]) == 0
    assert "nothing to do" in capsys.readouterr().out
    pz = cases.make_puzzle("two")
    for d in (12, 15):
        np.savez(feats / f"{d}.npz", part_feats=pz["part_feats"], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"])
    (feats / "notes.txt").write_text("ignored")
    (out / "12.npz").write_bytes(b"kept")
    assert gen.list_puzzles(str(feats), str(out)) == ([15], [12])
    (out / "15.npz").write_bytes(b"kept too")
    assert gen.main(["--features", str(feats), "--checkpoint", str(ckpt), "--out", str(out)]) == 0      # everything exists: no GPU needed
    assert "2 puzzles already" in capsys.readouterr().out and (out / "12.npz").read_bytes() == b"kept"
    x = gen.load_features(str(feats), 15)
    assert x["part_feats"].shape == (400, 128) and x["n_pcs"].shape == (20,)
    np.savez(feats / "16.npz", part_feats=pz["part_feats"][:-1], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"])
    with pytest.raises(ValueError, match="do not match"):
        gen.load_features(str(feats), 16)
    np.savez(feats / "17.npz", part_feats=pz["part_feats"])
    with pytest.raises(KeyError, match="missing"):
        gen.load_features(str(feats), 17)
    (feats / "x1.npz").write_bytes(b"")
    with pytest.raises(ValueError, match="<data_id>.npz"):
        gen.list_puzzles(str(feats), str(out))
