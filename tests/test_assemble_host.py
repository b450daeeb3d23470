"""Host (no GPU): the batched edge-feature entry (pfpp_edge_features_batch, csrc/edgefeat.hip) is declared, bound, counted and checks
its arguments before any launch; the front end (pfpp_hip.assemble) refuses what it cannot run."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_entry_is_declared_bound_and_counted(hip_lib):
    from pfpp_hip import _lib, ops

    raw = (ROOT / "include" / "pfpp.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bint pfpp_edge_features_batch\s*\(", text)
    assert "node_merge_utils.py:62-89" in raw and "auto_aggl.py:193-201" in raw and "auto_aggl.py:385-389" in raw
    assert "pfpp_edge_features_batch" in _lib.SIGNATURES and hasattr(lib, "pfpp_edge_features_batch")
    assert len(_lib.SIGNATURES["pfpp_edge_features_batch"]) == 13 and callable(ops.edge_features_batch)
    assert lib.pfpp_version() == 2
    n_entries = len(re.findall(r"^(?:int|int64_t|const char\*|unsigned)\s+pfpp_\w+\s*\(", text, flags=re.M))
    print(f"{n_entries} entry points declared")
    assert f"{n_entries} entry points" in (ROOT / "README.md").read_text()


def test_arguments_are_checked_before_any_launch(hip_lib):
    from pfpp_hip import _lib

    lib = _lib.load()
    fn = lib.pfpp_edge_features_batch
    one = C.c_void_p(4096)                  # a non-null, aligned address that is never dereferenced on these paths
    # (pts, pt_off, idx_a, idx_b, row_off, edge_off, puz, out, nb, B, P, max_m, stream)
    good = [one] * 8 + [2, 3, 20, 600, None]
    for k in range(8):
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, f"null pointer in position {k}"
        assert "null pointer" in lib.pfpp_last_error().decode()
    args = list(good)
    args[11] = 6001
    assert fn(*args) == -2 and "6000" in lib.pfpp_last_error().decode()
    args = list(good)
    args[10] = 33
    assert fn(*args) == -2 and "32" in lib.pfpp_last_error().decode()
    args = list(good)
    args[8] = 0
    assert fn(*args) == 0                   # no puzzle in the call: nothing to do
    args[10], args[8] = 1, 2
    assert fn(*args) == 0                   # one piece: no slot


def test_main_without_a_gpu_returns_2_and_a_missing_matcher_is_an_argparse_error(tmp_path, capsys, monkeypatch):
    from pfpp_hip import assemble

    for d in ("features", "pc_data"):
        (tmp_path / d).mkdir()
    for f in ("jigsaw.ckpt", "denoiser.ckpt", "verifier.ckpt"):
        (tmp_path / f).write_bytes(b"")
    common = ["--features", str(tmp_path / "features"), "--pc-data", str(tmp_path / "pc_data"), "--out", str(tmp_path / "out"),
              "--denoiser", str(tmp_path / "denoiser.ckpt"), "--verifier", str(tmp_path / "verifier.ckpt")]
    with pytest.raises(SystemExit) as e:
        assemble.main(common + ["--matcher", str(tmp_path / "nowhere.ckpt")])
    assert e.value.code == 2 and "no such file" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        assemble.main(common)                                       # --matcher is required
    capsys.readouterr()
    with pytest.raises(SystemExit):
        assemble.main(common + ["--matcher", str(tmp_path / "jigsaw.ckpt"), "verifier.no_such_key=1"])
    assert "no such key" in capsys.readouterr().err
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert assemble.main(common + ["--matcher", str(tmp_path / "jigsaw.ckpt"), "verifier.threshold=0.5"]) == 2
    assert "no GPU" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_batch_object_survives_the_datasets_deep_copy():
    import copy

    from pfpp_hip.matching_edges import BatchMatches

    bo = BatchMatches.__new__(BatchMatches)
    sample = {"matching_batch": (bo, 3), "n_pcs": np.arange(4)}
    again = copy.deepcopy(sample)
    assert again["matching_batch"][0] is bo and again["matching_batch"][1] == 3 and again["n_pcs"] is not sample["n_pcs"]
