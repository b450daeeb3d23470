"""Host (no GPU): the restatement of the by-area transform (tests/frames_cases.py) against the reference's own test-split outputs
(tests/golden/dataset.npz); pfpp_test_frames (csrc/augment.hip) is declared, bound, counted and checks its arguments before any
launch; pfpp_hip.augment.test_frames_batch and the front end's --frames refuse what they cannot run."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest

import frames_cases as FC

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("i", [0, 1])
def test_restatement_equals_the_reference_dataset_golden(golden, i):
    """with the recorded float64 global rotation, the golden's float64 init_pose_t and its float32 part_trans / part_rots the
    restatement IS dataset.py:86-109: equal bit for bit.  With the global quaternion rounded to float32 (what the kernel gets) and
    with c_ref / t recomputed from the stored fragments: below the 2e-6 of test_fragment_prepare_vs_reference_dataset_golden."""
    it = FC.golden_item(golden("dataset"), i)
    want = it["want"]
    assert np.array_equal(want["init_pose_r"], it["q_global"]) and len(it["by_area"]) == 5000 == int(it["n_pcs"].sum())
    got = FC.by_area_frames(it["by_area"], it["n_pcs"], it["num_parts"], it["q_global"], want["init_pose_t"], want["part_trans"], want["part_rots"])
    d = np.abs(got.astype(np.float64) - want["part_pcs_by_area"]).max()
    print(f"test{i}: float64 global quaternion: max difference {d:.1e}")
    assert got.dtype == want["part_pcs_by_area"].dtype and np.array_equal(got, want["part_pcs_by_area"])
    q32 = it["q_global"].astype(np.float32)
    got = FC.by_area_frames(it["by_area"], it["n_pcs"], it["num_parts"], q32, want["init_pose_t"], want["part_trans"], want["part_rots"])
    d = np.abs(got.astype(np.float64) - want["part_pcs_by_area"]).max()
    print(f"test{i}: float32 global quaternion: max difference {d:.1e}")
    assert d < 2e-6
    whole = FC.restate(dict(it, q_global=q32, q_part=it["q_part"].astype(np.float32)))
    d = np.abs(whole.astype(np.float64) - want["part_pcs_by_area"]).max()
    print(f"test{i}: float32 quaternions, c_ref and t from the stored fragments: max difference {d:.1e}")
    assert d < 2e-6


def test_hand_puzzles_hold_the_cases_they_were_built_for():
    for N in (7, 64):
        A, B, Cc = (FC.hand_puzzle(n, N) for n in "ABC")
        assert A["n_pcs"].tolist()[:2] == [1, 257] and A["num_parts"] == 2 and A["ref"] == 1
        assert B["num_parts"] == FC.P_HAND == 5 and B["n_pcs"].tolist() == [255, 256, 1, 30, 300] and int(B["n_pcs"].sum()) % 256
        assert np.cumsum(B["n_pcs"])[:2].tolist() == [255, 511] and np.cumsum(B["n_pcs"])[2] == 512
        assert Cc["num_parts"] == 3 and Cc["n_pcs"].tolist() == [40, 0, 7, 0, 0]
        assert len({len(p["by_area"]) for p in (A, B, Cc)}) == 3
        for p in (A, B, Cc):
            assert p["part_pcs_gt"].shape == (5, N, 3) and len(p["by_area"]) == int(p["n_pcs"].sum())
            norms = np.linalg.norm(np.concatenate([p["q_global"][None], p["q_part"]]), axis=1)
            assert (np.abs(norms - 1) > 1e-3).all()                         # non-unit quaternions
            want = FC.restate(p)
            assert want.dtype == np.float32 and 0 < np.abs(want).max() < 2  # the range the GPU test's one-ulp bar is stated for


# ------------------------------------------------------------------------------------------------ the library entry
def test_entry_is_declared_bound_and_counted(hip_lib):
    from pfpp_hip import _lib, augment

    raw = (ROOT / "include" / "pfpp.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bint pfpp_test_frames\s*\(", text)
    assert "dataset.py:86-109" in raw and ":165-215" in raw
    assert "pfpp_test_frames" in _lib.SIGNATURES and hasattr(lib, "pfpp_test_frames")
    assert len(_lib.SIGNATURES["pfpp_test_frames"]) == 19 and callable(augment.test_frames) and callable(augment.test_frames_batch)
    assert lib.pfpp_version() == 2
    n_entries = len(re.findall(r"^(?:int|int64_t|const char\*|unsigned)\s+pfpp_\w+\s*\(", text, flags=re.M))
    assert f"{n_entries} entry points" in (ROOT / "README.md").read_text()


def test_arguments_are_checked_before_any_launch(hip_lib):
    from pfpp_hip import _lib

    lib = _lib.load()
    fn = lib.pfpp_test_frames
    one = C.c_void_p(4096)                  # a non-null, aligned address that is never dereferenced on these paths
    # (part_pcs_gt, num_parts, ref_idx, q_global, q_part, part_pcs, part_trans, part_scale, init_pose_t, by_area, pt_off, n_pcs,
    #  by_area_out, B, P, N, M, workspace, stream)
    good = [one] * 13 + [2, 20, 64, 10000, one, None]
    for k in list(range(13)) + [17]:
        args = list(good)
        args[k] = None
        assert fn(*args) == -1, f"null pointer in position {k}"
        assert "null pointer" in lib.pfpp_last_error().decode()
    for pos, value, word in ((14, 33, "32"), (15, 2049, "2048"), (13, 65536, "65535"), (16, 1 << 31, "2^31")):
        args = list(good)
        args[pos] = value
        assert fn(*args) == -2 and word in lib.pfpp_last_error().decode(), (pos, value)
    args = list(good)
    args[16] = -1
    assert fn(*args) == -1
    args = list(good)
    args[13] = 0
    assert fn(*args) == 0                   # no puzzle in the call: nothing to do


# ------------------------------------------------------------------------------------------------ test_frames_batch
def sample_of(p: dict) -> dict:
    """a hand-built puzzle as GeometryLatentDataset(..., "test", device_augment=True) returns an item"""
    valid = (np.arange(FC.P_HAND) < p["num_parts"]).astype(np.float32)
    return {"data_id": ord(p["name"]), "part_valids": valid, "num_parts": p["num_parts"], "mesh_file_path": "a/" + p["name"],
            "graph": np.zeros((FC.P_HAND, FC.P_HAND), dtype=bool), "part_pcs_gt": p["part_pcs_gt"], "ref_part": p["ref_part"],
            "gt_pc_by_area": p["by_area"], "n_pcs": p["n_pcs"], "critical_pcs_idx": np.zeros(len(p["by_area"]), dtype=np.int64),
            "n_critical_pcs": np.zeros(FC.P_HAND, dtype=np.int64)}


def test_frames_batch_refuses_inconsistent_samples_before_any_launch(monkeypatch):
    from pfpp_hip import augment

    monkeypatch.setattr(augment, "test_frames", lambda *a, **k: pytest.fail("the kernel wrapper was reached"))
    A, B = sample_of(FC.hand_puzzle("A", 7)), sample_of(FC.hand_puzzle("B", 7))
    assert augment.test_frames_batch([], "cpu") == []
    with pytest.raises(ValueError, match="n_pcs sums to 258.*257 points"):
        augment.test_frames_batch([B, dict(A, gt_pc_by_area=A["gt_pc_by_area"][:-1])], "cpu")
    moved = A["n_pcs"].copy()
    moved[1], moved[3] = 250, 7
    with pytest.raises(ValueError, match="slot >= num_parts"):
        augment.test_frames_batch([dict(A, n_pcs=moved)], "cpu")
    none, two, outside = (np.zeros(FC.P_HAND, dtype=bool) for _ in range(3))
    two[:2] = True
    outside[3] = True                                                      # the only true entry is no valid slot of A
    for ref in (none, two, outside):
        with pytest.raises(ValueError, match="ref_part"):
            augment.test_frames_batch([B, dict(A, ref_part=ref)], "cpu")
    with pytest.raises(ValueError, match="share P and N"):
        augment.test_frames_batch([A, sample_of(FC.hand_puzzle("B", 64))], "cpu")
    wide = dict(A, part_pcs_gt=np.zeros((6, 7, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="share P and N"):
        augment.test_frames_batch([B, wide], "cpu")
    with pytest.raises(ValueError, match="n_pcs has 5 slots"):
        augment.test_frames_batch([wide], "cpu")


# ------------------------------------------------------------------------------------------------ the front end
def test_frames_option_parses_defaults_to_host_and_refuses_other_words(capsys):
    from pfpp_hip import assemble

    common = ["--features", "f", "--matcher", "m", "--out", "o"]
    ap = assemble.build_parser()
    assert ap.parse_args(common).frames == "host"
    assert ap.parse_args(common + ["--frames", "device"]).frames == "device"
    assert ap.parse_args(common + ["--frames", "host"]).frames == "host"
    with pytest.raises(SystemExit) as e:
        ap.parse_args(common + ["--frames", "gpu"])
    assert e.value.code == 2 and "--frames" in capsys.readouterr().err
    cfg = NS(denoiser=NS(data=NS(max_num_part=20, data_val_dir="pc")))
    assert assemble.Assembler(cfg, None, "m", features="f").frames == "host"
    assert assemble.Assembler(cfg, None, "m", features="f", frames="device").frames == "device"
    with pytest.raises(ValueError, match="frames"):
        assemble.Assembler(cfg, None, "m", features="f", frames="gpu")
