"""GPU: the matcher's dataset (csrc/matching_dataset.hip, pfpp_hip/matching_dataset.py, pfpp_hip/generate_matching_points.py).

Yardsticks: tests/golden/matching_dataset.npz, written by the reference's own all_piece_matching_dataset.py with recorded draws
(tools/make_matching_dataset_goldens.py), and the float64 numpy restatement of the kernels in tests/matching_dataset_cases.py, which
tests/test_matching_dataset_host.py checks against the same golden without a GPU.  The restatement takes the store's cdf and total,
the kernels' own inputs."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import matching_dataset_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return MC.make_tree(tmp_path_factory.mktemp("meshes"))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("matching_dataset")


class Host:
    """a store and the host copies the restatement needs"""

    def __init__(self, store):
        self.store = store
        h = store.host
        self.cdf, self.total = store.cdf.cpu().numpy(), store.total.cpu().numpy()
        self.parts = [(h["verts"][h["vert_off"][p]:h["vert_off"][p + 1]], h["faces"][h["face_off"][p]:h["face_off"][p + 1]])
                      for p in range(len(h["vert_off"]) - 1)]

    def puzzle(self, s):
        p0, p1 = self.store.host["puz_part_off"][s:s + 2]
        fo = self.store.host["face_off"]
        return dict(parts=self.parts[p0:p1], areas=self.total[p0:p1], cdfs=[self.cdf[fo[p]:fo[p + 1]] for p in range(p0, p1)],
                    totals=self.total[p0:p1], data_id=int(self.store.host["data_id"][s]))

    def item(self, s, N, mpp, **kw):
        pz = self.puzzle(s)
        return MC.item(pz["parts"], pz["areas"], pz["data_id"], N, mpp, cdfs=pz["cdfs"], totals=pz["totals"], **kw)


@pytest.fixture(scope="module")
def stores(dev, hip_lib, tree, gold):
    from pfpp_hip.matching_dataset import MeshStore

    return {split: Host(MeshStore.build(str(tree), [str(s) for s in gold[f"{split}_data_list"]], dev, workers=0)) for split in ("train", "val")}


def _grid(dims, seed, widths=None, h=0.25):
    sys.path.insert(0, str(MC.ROOT / "tools"))
    import make_synthetic_meshes as ms

    R, t = ms.rotation(seed), np.array([0.3, -0.25, 0.5])
    widths = widths or [[6] + [2] * (d - 1) for d in dims]
    breaks = [np.concatenate([[0], np.cumsum(w)]).astype(int) for w in widths]
    out = []
    for c in itertools.product(*[range(d) for d in dims]):
        v, f = ms.box_surface([int(breaks[a][c[a]]) for a in range(3)], [int(breaks[a][c[a] + 1]) for a in range(3)], h)
        out.append((ms.transform(v * h, R, t), f.astype(np.int32)))
    return out


@pytest.fixture(scope="module")
def edge_store(dev, hip_lib):
    """puzzles of 2, 20 and 3 parts, in memory; data ids that are not the positions"""
    from pfpp_hip.matching_dataset import MeshStore

    puzzles = [_grid((2, 1, 1), 3), _grid((5, 2, 2), 4), _grid((3, 1, 1), 5, widths=[[9, 1, 3], [4], [4]])]
    return Host(MeshStore.from_meshes(puzzles, [11, 5, 40], ["two", "twenty", "three"], dev))


def _np(t):
    return t.cpu().numpy()


def _assert_item(out, b, want, N, keys, what):
    for k in keys:
        got = _np(out[k][b])
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k, got.dtype, got.shape, want[k].dtype, want[k].shape)
        assert np.array_equal(got, want[k]), (what, k, int((got != want[k]).sum()))


ALL_KEYS = ("n_pcs", "part_valids", "gt_pcs", "part_pcs", "part_trans", "part_quat", "points", "rot", "face_idx")


def test_counts_equal_the_restatement_and_the_reference(stores, gold):
    from pfpp_hip.matching import make_layout
    from pfpp_hip.matching_dataset import sample_batch

    for N, mpp in MC.SETTINGS:
        for split in ("train", "val"):
            H = stores[split]
            out = sample_batch(H.store, range(5), N, mpp)
            n_pcs = _np(out["n_pcs"])
            for i in range(5):
                areas = H.puzzle(i)["areas"]
                want = np.zeros(20, dtype=np.int64)
                want[:len(areas)] = MC.piece_counts(areas, N, mpp)
                assert np.array_equal(n_pcs[i], want) and np.array_equal(n_pcs[i], gold[f"n{N}_{split}_{i}_n_pcs"]), (N, split, i, n_pcs[i])
            lay = make_layout(n_pcs, out["n_pcs"].device)
            assert torch.equal(out["piece_off"], lay.piece_off) and torch.equal(out["puz_piece_off"], lay.puz_piece_off)
            assert (n_pcs.sum(1) == N).all() and out["n_pcs"].dtype == torch.int64


def test_given_draws_reproduce_the_reference(stores, gold):
    from pfpp_hip.matching_dataset import sample_batch

    for N, mpp in MC.SETTINGS:
        for split in ("train", "val"):
            H = stores[split]
            pre = [f"n{N}_{split}_{i}_" for i in range(5)]
            rot = np.zeros((5, 20, 3, 3))
            for i, p in enumerate(pre):
                rot[i, :len(gold[p + "rot"])] = gold[p + "rot"]
            u, order = np.stack([gold[p + "uniforms"] for p in pre]), np.stack([gold[p + "order"] for p in pre]).astype(np.int32)
            out = sample_batch(H.store, range(5), N, mpp, uniforms=u, order=order, rotations=rot, want_faces=True)
            for i, p in enumerate(pre):
                for k in ("gt_pcs", "part_trans", "n_pcs", "part_valids"):
                    assert np.array_equal(_np(out[k][i]), gold[p + k]), (p, k)
                want = H.item(i, N, mpp, uniforms=gold[p + "uniforms"], order=gold[p + "order"], rot=gold[p + "rot"])
                _assert_item(out, i, want, N, ("part_pcs", "gt_pcs", "part_trans", "part_quat", "points", "face_idx"), p)
                MC.assert_blas_rounding(_np(out["part_pcs"][i]), gold[p + "part_pcs"], p + "part_pcs")
                assert np.abs(_np(out["part_quat"][i]) - gold[p + "part_quat"]).max() <= 2.0 ** -23


def test_generated_mode_is_the_restatement_bit_for_bit(stores):
    from pfpp_hip.matching_dataset import sample_batch, split_word

    H, N, mpp, seed = stores["val"], 251, 20, 0x1234567890ABCDEF
    word = split_word("val", 3)
    out = sample_batch(H.store, range(5), N, mpp, seed=seed, split=word, want_faces=True)
    want = [H.item(i, N, mpp, seed=seed, split=word) for i in range(5)]
    for i in range(5):
        _assert_item(out, i, want[i], N, ALL_KEYS, f"puzzle {i}")
    # a puzzle does not depend on its batch or its position in it; a repeated index is allowed
    for sel in ([2], [2, 0, 1], [4, 3, 2], [2, 2, 0]):
        o = sample_batch(H.store, sel, N, mpp, seed=seed, split=word, want_faces=True)
        for b, s in enumerate(sel):
            _assert_item(o, b, want[s], N, ALL_KEYS, f"sel {sel} position {b}")
    again = sample_batch(H.store, range(5), N, mpp, seed=seed, split=word, want_faces=True)
    assert all(torch.equal(out[k], again[k]) for k in ALL_KEYS + ("piece_off", "puz_piece_off"))
    other = sample_batch(H.store, range(5), N, mpp, seed=seed, split=split_word("val", 4))
    assert torch.equal(other["n_pcs"], out["n_pcs"])
    for k in ("gt_pcs", "part_pcs", "part_quat", "part_trans"):
        assert not torch.equal(other[k], out[k]), k
    assert not torch.equal(sample_batch(H.store, range(5), N, mpp, seed=seed, split=split_word("train", 3))["gt_pcs"], out["gt_pcs"])


def _on_face_residual(H, s, want, points, face_idx):
    """largest distance of a sample from the triangle its face index names (fp64), barycentric coordinates allowed 1e-12 outside"""
    worst, o = 0.0, 0
    for (v, f), n in zip(H.puzzle(s)["parts"], want["n_pcs"]):
        p, fc = points[o:o + n], face_idx[o:o + n]
        a, e1, e2 = v[f[fc, 0]], v[f[fc, 1]] - v[f[fc, 0]], v[f[fc, 2]] - v[f[fc, 0]]
        d = p - a
        g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
        det = g11 * g22 - g12 * g12
        l0, l1 = (r1 * g22 - r2 * g12) / det, (r2 * g11 - r1 * g12) / det
        res = np.linalg.norm(d - l0[:, None] * e1 - l1[:, None] * e2, axis=1)
        out = np.maximum.reduce([-l0, -l1, l0 + l1 - 1.0, np.zeros_like(l0)])
        worst = max(worst, float(res.max()), float(out.max()))
        o += n
    return worst


@pytest.mark.parametrize("N,mpp", [(64, 3), (251, 12), (256, 12), (257, 12), (1000, 30), (257, 1)])
def test_kernel_edges(edge_store, N, mpp):
    from pfpp_hip.matching_dataset import sample_batch

    H = edge_store
    out = sample_batch(H.store, [0, 1, 2], N, mpp, seed=5, split=1, want_faces=True)
    n_pcs = _np(out["n_pcs"])
    assert (n_pcs.sum(1) == N).all() and ((n_pcs > 0).sum(1) == [2, 20, 3]).all()
    worst = 0.0
    for s in range(3):
        want = H.item(s, N, mpp, seed=5, split=1)
        _assert_item(out, s, want, N, ALL_KEYS, f"N {N} puzzle {s}")
        worst = max(worst, _on_face_residual(H, s, want, _np(out["points"][s]), _np(out["face_idx"][s])))
        assert np.array_equal(_np(out["gt_pcs"][s]), _np(out["points"][s]).astype(np.float32))
    print(f"N {N}, min_part_point {mpp}: counts of the 20-part puzzle {n_pcs[1].tolist()}, on-face residual {worst:.2e}")
    assert worst <= 1e-12
    if mpp > 1:          # pieces of exactly min_part_point in the 20-part puzzle
        assert (n_pcs[1] == mpp).any()
    ends = np.cumsum(n_pcs, axis=1)
    if N > 256:          # a piece whose rows straddle the first block of 256 threads
        assert ((ends - n_pcs < 256) & (ends > 256) & (n_pcs > 0)).any(1).all()


def test_refusals(stores, edge_store, dev):
    from pfpp_hip import _lib
    from pfpp_hip.matching_dataset import MeshStore, sample_batch

    st = stores["val"].store
    for sel in ([5], [-1], [0, 7]):
        with pytest.raises(ValueError, match="selection"):
            sample_batch(st, sel, 251, 20)
    with pytest.raises(ValueError, match="min_part_point"):
        sample_batch(st, [0], 251, 21)          # 12 parts x 21 > 251: the reference's loop would never end
    with pytest.raises(ValueError, match="max_parts"):
        sample_batch(st, [0], 251, 20, max_parts=8)
    with pytest.raises(ValueError, match="uniforms"):
        sample_batch(st, [0], 251, 20, uniforms=np.zeros((1, 250, 3)))
    cpu = MeshStore(st.host, st.paths, device="cpu")
    with pytest.raises(ValueError, match="GPU"):
        sample_batch(cpu, [0], 251, 20)
    # a part without area: three collinear vertices
    flat = (np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]]), np.array([[0, 1, 2]], dtype=np.int32))
    good = edge_store.puzzle(0)["parts"]
    with pytest.raises(_lib.PfppError, match="broken.*areas sum to zero"):
        MeshStore.from_meshes([good, [good[0], flat]], [0, 1], ["fine", "broken"], dev)
    bad = MeshStore.from_meshes([good, [good[0], flat]], [0, 1], ["fine", "broken"], dev, check_areas=False)
    assert sample_batch(bad, [0], 64, 3)["n_pcs"].sum() == 64
    with pytest.raises(_lib.PfppError, match="broken.*areas sum to zero"):
        sample_batch(bad, [0, 1], 64, 3)
    order = np.tile(np.arange(64, dtype=np.int32), (1, 1))
    with pytest.raises(_lib.PfppError, match="order"):
        sample_batch(edge_store.store, [0], 64, 3, order=order)          # row 63 of the puzzle asks for sample 63 of its piece


def _rotate_back(d, b):
    """part_quat (scalar first) applied to part_pcs, plus part_trans, per piece: should give gt_pcs"""
    n_pcs, q, t = _np(d["n_pcs"][b]), _np(d["part_quat"][b]).astype(np.float64), _np(d["part_trans"][b]).astype(np.float64)
    pcs, gt, worst, o = _np(d["part_pcs"][b]).astype(np.float64), _np(d["gt_pcs"][b]).astype(np.float64), 0.0, 0
    for k, n in enumerate(n_pcs):
        if n:
            assert abs(float(q[k] @ q[k]) - 1.0) < 1e-6
            worst = max(worst, float(np.abs(pcs[o:o + n] @ MC.quat_matrix(q[k]).T + t[k] - gt[o:o + n]).max()))
        o += n
    return worst


def test_dataset_batches_and_store_round_trip(tree, stores, dev, tmp_path):
    from pfpp_hip.matching_dataset import DATA_DICT_KEYS, AllPieceMatchingDataset, MeshStore

    path = str(tmp_path / "val_store.npz")
    kw = dict(num_points=251, min_part_point=20, overfit=-1, seed=3, device=dev, workers=0, fracture_label_threshold=0.025)
    ds = AllPieceMatchingDataset(str(tree), "everyday.val.txt", ["part_ids"], store=path, **kw)
    d = ds.batch([1, 4], epoch=2)
    assert tuple(d) == DATA_DICT_KEYS and os.path.exists(path)
    shapes = {"part_pcs": (2, 251, 3), "gt_pcs": (2, 251, 3), "part_valids": (2, 20), "part_quat": (2, 20, 4), "part_trans": (2, 20, 3),
              "n_pcs": (2, 20), "data_id": (2,), "critical_label_thresholds": (2, 251), "num_parts": (2,)}
    for k, s in shapes.items():
        assert tuple(d[k].shape) == s and d[k].is_cuda and d[k].dtype == (torch.int64 if k in ("n_pcs", "data_id", "num_parts") else torch.float32), k
    assert d["data_id"].tolist() == [1, 4] and d["num_parts"].tolist() == [3, 6] and d["mesh_file_path"] == [ds.data_list[1], ds.data_list[4]]
    assert bool((d["critical_label_thresholds"] == 0.025).all()) and d["part_valids"].sum(1).tolist() == [3.0, 6.0]
    print(f"generated rotations: part_quat takes part_pcs back to gt_pcs within {max(_rotate_back(d, 0), _rotate_back(d, 1)):.2e}")
    assert max(_rotate_back(d, 0), _rotate_back(d, 1)) < 5e-6
    # the saved store gives the same batches, and so does the store parsed for the other tests
    for other in (AllPieceMatchingDataset(str(tree), "everyday.val.txt", [], store=path, **kw),
                  AllPieceMatchingDataset(str(tree), "everyday.val.txt", [], store=stores["val"].store, **kw)):
        e = other.batch([1, 4], epoch=2)
        assert all(torch.equal(d[k], e[k]) for k in shapes)
    assert isinstance(MeshStore.load(path, dev), MeshStore)
    # one epoch: every puzzle once, each as in any other batch of that epoch
    got = list(ds.batches(2, epoch=2, shuffle=True, drop_last=False))
    assert sorted(i for g in got for i in g["data_id"].tolist()) == list(range(5)) and [len(g["data_id"]) for g in got] == [2, 2, 1]
    for g in got:
        for b, i in enumerate(g["data_id"].tolist()):
            if i in (1, 4):
                assert torch.equal(g["part_pcs"][b], d["part_pcs"][[1, 4].index(i)])
    assert len(list(ds.batches(2, epoch=2, drop_last=True))) == 2
    # rot_range > 0: the host draws Euler angles; the quaternion still takes the points back
    r = AllPieceMatchingDataset(str(tree), "everyday.val.txt", [], store=stores["val"].store, rot_range=30.0, **kw).batch([1, 4], epoch=2)
    assert torch.equal(r["gt_pcs"], d["gt_pcs"]) and torch.equal(r["part_trans"], d["part_trans"]) and not torch.equal(r["part_pcs"], d["part_pcs"])
    assert max(_rotate_back(r, 0), _rotate_back(r, 1)) < 5e-6
    w = _np(r["part_quat"])[:, :3, 0]
    assert (np.abs(w) >= np.cos(np.deg2rad(30.0 * 3 / 2)) - 1e-6).all()          # three angles of at most 30 degrees each


def test_command_line_writes_the_point_files(tree, stores, dev, tmp_path, capsys):
    from pfpp_hip.evaluate_matching import POSE_KEYS
    from pfpp_hip.generate_matching_data import list_puzzles, load_features
    from pfpp_hip.generate_matching_points import main
    from pfpp_hip.matching_dataset import AllPieceMatchingDataset

    out = str(tmp_path / "points")
    argv = ["--data-dir", str(tree), "--data-fn", "everyday.{}.txt", "--split", "val", "--out", out, "--num-points", "251", "--min-part-point",
            "20", "--seed", "3", "--epoch", "2", "--batch-size", "2", "--workers", "0", "--store", str(tmp_path / "s.npz")]
    assert main(argv) == 0
    todo, _ = list_puzzles(out, str(tmp_path / "none"))
    assert todo == [0, 1, 2, 3, 4]
    ds = AllPieceMatchingDataset(str(tree), "everyday.val.txt", [], num_points=251, min_part_point=20, overfit=-1, seed=3, device=dev,
                                 store=stores["val"].store)
    d = ds.batch(range(5), epoch=2)
    for i in todo:
        x = load_features(out, i, points=True, extra=POSE_KEYS)
        for k in ("part_pcs", "gt_pcs", "n_pcs", "part_valids", "part_quat", "part_trans"):
            assert np.array_equal(x[k], _np(d[k][i])) and x[k].dtype == _np(d[k]).dtype, (i, k)
    stamp = os.stat(os.path.join(out, "3.npz")).st_mtime_ns
    os.remove(os.path.join(out, "1.npz"))
    assert main(argv) == 0 and "4 existing files left alone" in capsys.readouterr().out
    assert os.stat(os.path.join(out, "3.npz")).st_mtime_ns == stamp and os.path.exists(os.path.join(out, "1.npz"))


def test_one_training_step_fed_from_the_dataset(tree, stores, dev):
    """two puzzles of 64 points (every piece at least 8), the descriptor network's engine, the head's loss from the dataset's
    thresholds, backward: the loss and every gradient are finite"""
    from pfpp_hip.matching import DescriptorNetwork, MatchingHead
    from pfpp_hip.matching_dataset import AllPieceMatchingDataset
    from pfpp_hip.matching_encoder_train import DescriptorTrainEngine
    from pfpp_hip.matching_train import MatchingHeadLoss, MatchingHeadTrainEngine

    torch.manual_seed(0)
    ds = AllPieceMatchingDataset(str(tree), "everyday.val.txt", [], num_points=64, min_part_point=8, overfit=-1, seed=1, device=dev,
                                 store=stores["val"].store, fracture_label_threshold=0.25)
    d = ds.batch([2, 3], epoch=0)          # 2 and 4 pieces in contact
    net = DescriptorNetwork().to(dev)
    head_eng = MatchingHeadTrainEngine(MatchingHead().to(dev), w_cls_loss=1.0, w_mat_loss=1.0)
    eng = DescriptorTrainEngine(net)
    feats = eng.forward(d["part_pcs"], d["n_pcs"], d["part_valids"], seed=0)
    loss = MatchingHeadLoss.apply(feats, head_eng, d["gt_pcs"], d["n_pcs"], d["part_valids"], d["critical_label_thresholds"])
    assert bool(torch.isfinite(loss))
    loss.backward()
    grads = [(k, v.grad) for k, v in net.named_parameters()] + [(k, v.grad) for k, v in head_eng.params.items()]
    bad = [k for k, g in grads if g is None or not bool(torch.isfinite(g).all())]
    print(f"loss {float(loss.detach()):.6g}, {len(grads)} gradients, largest {max(float(g.abs().max()) for _, g in grads if g is not None):.3g}")
    assert not bad, bad
