"""CPU: the matcher's dataset (pfpp_hip/matching_dataset.py, csrc/matching_dataset.hip) — the numpy restatement of the kernels
(tests/matching_dataset_cases.py) against tests/golden/matching_dataset.npz, which tools/make_matching_dataset_goldens.py wrote by
running the reference's all_piece_matching_dataset.py with recorded draws; the summation order of np.sum; the host rotations;
discovery."""
import numpy as np
import pytest

import matching_dataset_cases as MC


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return MC.make_tree(tmp_path_factory.mktemp("meshes"))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("matching_dataset")


@pytest.fixture(scope="module")
def restated(tree, gold):
    """every golden item restated from its recorded draws, once"""
    out = {}
    for N, mpp in MC.SETTINGS:
        for split, i, p in MC.golden_items(gold, N):
            parts = MC.folder_meshes(tree, str(gold[p + "mesh_file_path"]))
            out[p] = MC.item(parts, gold[p + "areas"], i, N, mpp, uniforms=gold[p + "uniforms"], order=gold[p + "order"], rot=gold[p + "rot"])
    return out


def test_np_sum_order_is_numpys():
    rng = np.random.default_rng(5)
    bad = 0
    for n in range(2, 21):
        for _ in range(200):
            a = rng.random(n) * 10.0 ** rng.integers(-3, 4, n)
            bad += MC.np_sum_order(a) != np.sum(a)
    assert bad == 0


def test_counts_equal_the_reference(gold, restated):
    for N, mpp in MC.SETTINGS:
        for split, i, p in MC.golden_items(gold, N):
            assert np.array_equal(restated[p]["n_pcs"], gold[p + "n_pcs"]), p
            assert restated[p]["n_pcs"].sum() == N
            assert np.array_equal(restated[p]["part_valids"], gold[p + "part_valids"])
    # the two puzzles the issue names, (251, 20)
    val, train = [str(s) for s in gold["val_data_list"]], [str(s) for s in gold["train_data_list"]]
    mug = f"n251_val_{val.index('everyday/Mug/obj002/fractured_0')}_n_pcs"
    bowl = f"n251_train_{train.index('everyday/Bowl/obj001/fractured_2')}_n_pcs"
    assert gold[mug][:12].tolist() == [20, 20, 20, 20, 20, 23, 20, 25, 23, 20, 20, 20]
    assert gold[bowl][:8].tolist() == [51, 40, 40, 20, 40, 20, 20, 20]


def test_restatement_reproduces_the_reference_items(gold, restated):
    for N, _ in MC.SETTINGS:
        for split, i, p in MC.golden_items(gold, N):
            r = restated[p]
            assert np.array_equal(r["gt_pcs"], gold[p + "gt_pcs"]), p
            assert np.array_equal(r["part_trans"], gold[p + "part_trans"]), p
            assert r["part_pcs"].dtype == np.float32 and gold[p + "part_pcs"].dtype == np.float32
            MC.assert_blas_rounding(r["part_pcs"], gold[p + "part_pcs"], p + "part_pcs")
            # the stored quaternion is float32 of scipy's: equal up to the cast of a 1e-15 difference
            assert np.abs(r["part_quat"] - gold[p + "part_quat"]).max() <= 2.0 ** -23, p
            assert int(gold[p + "data_id"]) == i and int(gold[p + "num_parts"]) == int(r["part_valids"].sum())
            assert np.array_equal(gold[p + "critical_label_thresholds"], np.full(N, 0.025, dtype=np.float32))


def test_quat_from_matrix_is_scipys(gold):
    st = pytest.importorskip("scipy.spatial.transform")
    from pfpp_hip.matching_dataset import euler_xyz_matrix, quat_from_matrix

    mats = np.concatenate([gold[k] for k in gold if k.endswith("_rot")])
    mats = np.concatenate([mats, np.swapaxes(mats, -1, -2), euler_xyz_matrix(np.random.default_rng(1).uniform(-180, 180, (200, 3)))])
    want = st.Rotation.from_matrix(mats).as_quat()[:, [3, 0, 1, 2]]
    assert np.abs(quat_from_matrix(mats) - want).max() <= 1e-15
    ang = np.random.default_rng(2).uniform(-180, 180, (50, 3))
    assert np.abs(euler_xyz_matrix(ang) - st.Rotation.from_euler("xyz", ang, degrees=True).as_matrix()).max() <= 1e-15


def test_marsaglia_quaternions_are_unit_and_their_matrices_rotations():
    worst_q = worst_r = 0.0
    used = 0
    for data_id in range(40):
        for slot in range(20):
            q, n = MC.marsaglia_quat(9, 3, data_id, slot)
            used = max(used, n)
            R = MC.quat_matrix(q)
            worst_q = max(worst_q, abs(float(q @ q) - 1.0))
            worst_r = max(worst_r, float(np.abs(R @ R.T - np.eye(3)).max()))
            assert np.linalg.det(R) > 0.999
    print(f"| |q|^2 - 1 | <= {worst_q:.2e}, |R R^T - 1| <= {worst_r:.2e}, at most {used} attempts")
    assert worst_q <= 4 * 2.0 ** -52 and worst_r <= 1e-14 and 1 < used < 64
    # no attempt inside the disc: the identity
    q, n = MC.marsaglia_quat(9, 3, 0, 0, attempts=0)
    assert q.tolist() == [1.0, 0.0, 0.0, 0.0]


def test_infeasible_min_part_point_is_refused():
    with pytest.raises(ValueError):
        MC.piece_counts(np.ones(12), 251, 21)
    assert MC.piece_counts(np.ones(12), 252, 21).tolist() == [21] * 12
    assert MC.piece_counts(np.array([5.0, 1.0, 1.0]), 64, 1).sum() == 64


def test_discovery_equals_the_reference(tree, gold):
    from pfpp_hip.matching_dataset import AllPieceMatchingDataset, read_data_list

    for split, fn in MC.SPLIT_FILES.items():
        assert read_data_list(str(tree), fn) == [str(s) for s in gold[f"{split}_data_list"]]
    ds = AllPieceMatchingDataset(str(tree), "everyday.train.txt", ["part_ids"], overfit=-1)
    assert ds.data_list == [str(s) for s in gold["train_data_list"]] and len(ds) == 5 and ds.split == "train"
    assert len(AllPieceMatchingDataset(str(tree), "everyday.train.txt", [], overfit=2).data_list) == 2
    assert len(AllPieceMatchingDataset(str(tree), "everyday.train.txt", [], overfit=-1, length=3)) == 3
    bowls = AllPieceMatchingDataset(str(tree), "everyday.train.txt", [], category="Bowl", overfit=-1).data_list
    assert bowls == [s for s in ds.data_list if "/Bowl/" in s] and len(bowls) == 2
    assert AllPieceMatchingDataset(str(tree), "everyday.train.txt", [], overfit=-1, max_num_part=6).data_list == \
        [s for s in ds.data_list if "fractured_2" not in s]
    with pytest.raises(NotImplementedError):
        AllPieceMatchingDataset(str(tree), "everyday.train.txt", [], sample_by="point")
    # nothing was written next to the meshes (the reference would have left its metadata pickle)
    assert not list(tree.glob("all_piece_matching_metadata*"))


def test_metadata_pickle_is_read_when_it_exists(tmp_path):
    import pickle

    from pfpp_hip.matching_dataset import read_data_list

    (tmp_path / "all_piece_matching_metadata_2_20_x.val.txt").write_bytes(pickle.dumps({"data_list": ["a/b/fractured_0"]}))
    assert read_data_list(str(tmp_path), "x.val.txt") == ["a/b/fractured_0"]


def test_command_line_without_a_gpu_ends_with_status_2(tree, tmp_path, monkeypatch, capsys):
    import torch

    from pfpp_hip.generate_matching_points import main

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    rc = main(["--data-dir", str(tree), "--data-fn", "everyday.{}.txt", "--split", "val", "--out", str(tmp_path / "out")])
    assert rc == 2 and "no GPU" in capsys.readouterr().err and not (tmp_path / "out").exists()


def test_entry_points_check_their_arguments(hip_lib):
    """they return before a launch: null pointers, sizes, more than 32 part slots"""
    import ctypes as C

    from pfpp_hip import _lib

    lib = _lib.load()
    one = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.pfpp_mdata_piece_counts(None, one, one, 1, 1, 64, 3, 20, one, one, one, one, None) != 0 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_mdata_piece_counts(one, one, one, 1, 1, 64, 3, 33, one, one, one, one, None) != 0 and b"unsupported" in lib.pfpp_last_error()
    assert lib.pfpp_mdata_piece_counts(one, one, one, 1, 1, 0, 3, 20, one, one, one, one, None) != 0 and b"sizes" in lib.pfpp_last_error()
    assert lib.pfpp_mdata_piece_counts(one, one, one, 0, 1, 64, 3, 20, one, one, one, one, None) == 0          # an empty batch launches nothing
    args = [one] * 10 + [1, 1, 64, 20, None, None, 0, 0]
    assert lib.pfpp_mdata_sample(*args, one, None, None, one, None) != 0 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_mdata_sample(*args[:13], 40, None, None, 0, 0, one, one, None, one, None) != 0 and b"unsupported" in lib.pfpp_last_error()
    pose = [one, one, one, one, 1, 1, 64, 20, None, None, 0, 0]
    assert lib.pfpp_mdata_pose(*pose, one, None, one, None, None) != 0 and b"part_quat" in lib.pfpp_last_error()
    assert lib.pfpp_mdata_pose(*pose[:4], -1, 1, 64, 20, None, None, 0, 0, one, one, one, None, None) != 0 and b"sizes" in lib.pfpp_last_error()


def test_store_round_trip_and_loader_on_the_host(tree, tmp_path):
    """a store on the CPU can be built, saved and loaded (parsed by two workers here); sampling from it is refused"""
    from pfpp_hip.matching_dataset import MeshStore, build_all_piece_matching_dataloader, read_data_list, sample_batch

    dl = read_data_list(str(tree), "everyday.val.txt")
    a = MeshStore.build(str(tree), dl, device="cpu", workers=0)
    b = MeshStore.build(str(tree), dl, device="cpu", workers=2)
    a.save(str(tmp_path / "store.npz"))
    c = MeshStore.load(str(tmp_path / "store.npz"), device="cpu")
    for k in MeshStore.HOST_KEYS:
        assert np.array_equal(a.host[k], b.host[k]) and np.array_equal(a.host[k], c.host[k]), k
    assert a.paths == c.paths == dl and a.num_parts.tolist() == [12, 3, 2, 4, 6] and a.device_bytes > 0
    with pytest.raises(ValueError, match="GPU"):
        sample_batch(c, [0], 251, 20)
    cfg = {"BATCH_SIZE": 2, "NUM_WORKERS": 0,
           "DATA": dict(DATA_DIR=str(tree), DATA_FN="everyday.{}.txt", DATA_KEYS=[], CATEGORY="all", NUM_PC_POINTS=251, MIN_NUM_PART=2,
                        MAX_NUM_PART=20, SHUFFLE_PARTS=False, ROT_RANGE=-1, OVERFIT=-1, SAMPLE_BY="area", MIN_PART_POINT=20, LENGTH=-1,
                        TEST_LENGTH=3, FRACTURE_LABEL_THRESHOLD=0.025)}
    train, val = build_all_piece_matching_dataloader(cfg)
    assert (len(train), train.batch_size, train.shuffle, train.drop_last) == (2, 2, True, True)
    assert (len(val), val.batch_size, val.shuffle, val.drop_last, len(val.dataset)) == (2, 2, False, False, 3)
    assert sorted(train.dataset.epoch_order(1, True).tolist()) == list(range(5))
    assert not np.array_equal(train.dataset.epoch_order(1, True), train.dataset.epoch_order(2, True))
