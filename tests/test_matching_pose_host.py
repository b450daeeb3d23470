"""CPU: the float64 restatement of the matcher's pairwise RANSAC (tests/matching_pose_cases.py) - its Philox rounds and draw against a
second, independent implementation and Random123's published known answers, its Horn against the reference's own horn_87
(tests/golden/matching_pose.npz) - the spanning tree and the global poses of pfpp_hip.matching_eval against the reference's
spanning_tree_alignment.py and pose_graph_utils.py on the golden's graphs, the translation-only edges and the pivot rule against the
loop-for-loop restatement of compute_global_transformation, and the argument checks of pfpp_hip.matching_eval, of the command line and
of the new entry points, all of which return before a launch."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

_spec = importlib.util.spec_from_file_location("matching_pose_cases", Path(__file__).resolve().parent / "matching_pose_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


def test_philox_rounds_match_the_published_known_answers_and_each_other():
    # Random123's kat_vectors, philox4x32 10 rounds
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert cases.philox4x32_10_scalar(*ctr, *key) == want
        assert tuple(int(v) for v in cases.philox4x32_10(np.array([ctr], dtype=np.uint64), key)[0]) == want
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, (200, 4), dtype=np.uint64)
    key = (int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)))
    got = cases.philox4x32_10(ctr, key)
    for row, g in zip(ctr, got):
        assert cases.philox4x32_10_scalar(*(int(v) for v in row), *key) == tuple(int(v) for v in g)


@pytest.mark.parametrize("M", [3, 4, 5, 1000])
def test_draw_gives_distinct_triples_in_range_and_both_implementations_agree(M):
    seed = 0x9e3779b97f4a7c15
    hs = np.arange(4096)
    tri = cases.draw_triples(M, hs, 2, seed)
    assert tri.shape == (4096, 3) and tri.min() >= 0 and tri.max() < M
    assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 0] != tri[:, 2]).all() and (tri[:, 1] != tri[:, 2]).all()
    for h in list(range(64)) + [4095]:
        assert cases.draw_triple_scalar(M, h, 2, seed) == tuple(int(v) for v in tri[h])
    if M <= 5:          # every ordered triple turns up: M (M - 1) (M - 2) <= 60 of them in 4096 draws
        assert len({tuple(t) for t in tri.tolist()}) == M * (M - 1) * (M - 2)
    assert not np.array_equal(tri, cases.draw_triples(M, hs, 3, seed))           # the pair and the seed both move the stream
    assert not np.array_equal(tri, cases.draw_triples(M, hs, 2, seed + 1))


def test_horn_restatement_equals_the_reference_on_triples(golden):
    g = golden("matching_pose")
    S, T = cases.horn_inputs()
    R, t, gap = cases.horn(S, T)
    print("max |R - ref|", np.abs(R - g["horn_R"]).max(), "max |t - ref|", np.abs(t - g["horn_t"]).max(), "least gap", gap.min())
    assert gap.min() > 1e-3            # eigh's vector is determined to 1e-16 / gap
    assert np.abs(R - g["horn_R"]).max() <= 1e-12 and np.abs(t - g["horn_t"]).max() <= 1e-12
    assert np.array_equal(g["horn_R"].astype(np.float32), g["horn_R32"]) and np.array_equal(g["horn_t"].astype(np.float32), g["horn_t32"])


def test_reference_procedure_finds_the_planted_pose_and_orders_winners():
    k = cases.planted_case(64, seed=3, pad=5)
    r = cases.ransac_reference(k["pts"], k["pair"], k["corr"], 512, seed=11)
    h = r["best_h"]
    assert r["count"] == r["counts"].max() == int(k["inlier"].sum())
    tied = np.nonzero(r["counts"] == r["count"])[0]
    assert r["sumsq"][h] == r["sumsq"][tied].min() and h == tied[r["sumsq"][tied] == r["sumsq"][h]].min()
    assert np.abs(r["R"] - k["R0"]).max() < 1e-5
    # collinear: every hypothesis degenerate, the stated fallback
    line = np.outer(np.arange(3.0), [0.25, -0.5, 0.125]).astype(np.float32)
    pts = np.concatenate([line, line + np.float32(0.5)])
    r = cases.ransac_reference(pts, (0, 3), np.stack([np.arange(3)] * 2, 1), 16)
    assert r["status"] == 0 and r["best_h"] == -1 and (r["counts"] == -1).all()
    assert np.array_equal(r["R"], np.eye(3)) and np.allclose(r["t"], 0.5)


def test_wrappers_refuse_bad_arguments_before_any_launch(hip_lib):
    from pfpp_hip import matching_eval as me

    pts = torch.zeros((8, 3))
    good = [np.array([[0, 0], [1, 1], [2, 2]])]
    with pytest.raises(ValueError, match="GPU"):
        me.ransac_pairs(pts, [[0, 4]], good)
    with pytest.raises(ValueError, match="GPU"):
        me.nn_dist_ragged(pts, [0, 8], pts, [0, 8])
    with pytest.raises(TypeError):
        me.ransac_pairs(pts.numpy(), [[0, 4]], good)
    # everything else is checked before the device is: these raise on CPU tensors with their own message
    bad_calls = [
        (dict(pts=torch.zeros((8, 2))), r"\[R, 3\]"),
        (dict(corr=[]), "correspondence lists"),
        (dict(corr=[good[0][:2]]), "M >= 3"),
        (dict(corr=[np.zeros((3, 3), dtype=np.int64)]), "M >= 3"),
        (dict(corr=[np.array([[0, 0], [1, 1], [2, 4]])]), "outside pts"),
        (dict(corr=[np.array([[0, 0], [1, 1], [-1, 2]])]), "outside pts"),
        (dict(pairs=[[0, 6]]), "outside pts"),
        (dict(corr=[good[0].astype(np.float64)]), "integers"),
        (dict(n_hyp=0), "n_hyp"),
        (dict(n_hyp=1 << 31), "n_hyp"),
        (dict(max_dist=0.0), "max_dist"),
        (dict(max_dist=float("nan")), "max_dist"),
        (dict(seed=-1), "seed"),
        (dict(seed=1 << 64), "seed"),
    ]
    for kw, msg in bad_calls:
        a = dict(dict(pts=pts, pairs=[[0, 4]], corr=good), **kw)
        with pytest.raises((ValueError, TypeError), match=msg):
            me.ransac_pairs(a.pop("pts"), a.pop("pairs"), a.pop("corr"), **a)
    for kw, msg in [(dict(src=torch.zeros((8, 2))), "expected"), (dict(so=[0, 4], do=[0, 4, 8]), "one entry per segment"), (dict(so=[0, 9]), "src_off"),
                    (dict(do=[4, 2]), "dst_off"), (dict(so=[-1, 8]), "src_off")]:
        a = dict(dict(src=pts, so=[0, 8], dst=pts, do=[0, 8]), **kw)
        with pytest.raises(ValueError, match=msg):
            me.nn_dist_ragged(a["src"], a["so"], a["dst"], a["do"])


def test_entry_points_refuse_bad_arguments_before_any_launch(hip_lib):
    from pfpp_hip import _lib

    lib = _lib.load()
    assert lib.pfpp_ransac_pairs_workspace(3, 257) == 3 * 2 * 16 and lib.pfpp_ransac_pairs_workspace(0, 1) == 0
    assert lib.pfpp_ransac_pairs_workspace(-1, 1) == -1 and lib.pfpp_ransac_pairs_workspace(1, 0) == -1
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(pts=p, R=8, E=1, pair_off=p, corr=p, corr_off=p, H=16, max_dist=0.05, seed=0, refine=0, Rout=p, tout=p, stats=p, info=p, counts=None,
              ws=p, ws_bytes=16)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pfpp_ransac_pairs(a["pts"], a["R"], a["E"], a["pair_off"], a["corr"], a["corr_off"], a["H"], a["max_dist"], a["seed"], a["refine"],
                                     a["Rout"], a["tout"], a["stats"], a["info"], a["counts"], a["ws"], a["ws_bytes"], None)

    assert call(E=0) == 0                                            # nothing to do, nothing launched
    for bad in (dict(H=0), dict(E=-1), dict(max_dist=0.0), dict(max_dist=-1.0), dict(pts=None), dict(corr=None), dict(Rout=None), dict(ws=None),
                dict(ws_bytes=8), dict(R=0), dict(ws=C.c_void_p(p.value + 4))):
        assert call(**bad) == -1, bad                                # PFPP_EINVAL
        assert b"pfpp_ransac_pairs" in lib.pfpp_last_error()
    for bad in (dict(E=65536, ws_bytes=1 << 30), dict(H=0x7fffff01, ws_bytes=1 << 40)):
        assert call(**bad) == -2, bad                                # PFPP_EUNSUPPORTED
    nn = lambda **kw: lib.pfpp_nn_dist_ragged(kw.get("src", p), kw.get("so", p), kw.get("dst", p), kw.get("do", p), kw.get("out", p),
                                              kw.get("S", 1), kw.get("max_n", 4), None)
    assert nn(S=0) == 0 and nn(max_n=0) == 0
    for bad in (dict(S=-1), dict(max_n=-1), dict(src=None), dict(do=None), dict(out=None)):
        assert nn(**bad) == -1, bad
    assert nn(S=65536) == -2


# ------------------------------------------------------------------------------------------------------------------ pose graphs
@pytest.mark.parametrize("name", ["chain", "star", "dense", "two_components", "cycle"])
def test_spanning_tree_and_global_poses_equal_the_reference(golden, name):
    from pfpp_hip import matching_eval as me

    g = golden("matching_pose")
    v, edges, T, u = cases.graph_cases()[name]
    aux = me.connect_graph(v, edges)
    assert np.array_equal(aux, g[f"graph_{name}_aux"])
    order, pred = me.minimum_spanning_tree(v + 1, np.concatenate([edges, aux]), np.concatenate([u, np.ones(len(aux))]))
    assert list(order) == g[f"graph_{name}_order"].tolist()                 # Kruskal's tie rule and the search order
    assert [pred.get(k, -1) for k in range(v + 1)] == g[f"graph_{name}_pred"].tolist()
    poses = me.global_alignment(v, edges, T, u)
    dev = np.abs(poses - g[f"graph_{name}_poses"]).max()
    print(name, "max |pose - reference|", dev)
    assert dev <= 1e-12 and np.array_equal(poses[0], np.eye(4))
    if name == "two_components":                                             # the hub is no leaf: identity auxiliaries tie the components
        assert len(aux) == 2 and aux[0, 1] == 1 and aux[1, 1] == 0           # the larger component first
        assert np.allclose(poses[1], np.eye(4), atol=1e-12)
    with pytest.raises(ValueError, match="not connected"):
        me.spanning_tree_alignment(3, np.array([[1, 0]]), T[:1], u[:1])


def host_pipeline(data, poses_of):
    """the module's host stages around given edge poses: match_edges, the translation-only edges, global alignment, the anchoring"""
    from pfpp_hip import matching_eval as me
    from pfpp_hip.matching import match_edges

    rot, trans, pivots, graphs = np.zeros(data["n_pcs"].shape + (3, 3)), np.zeros(data["n_pcs"].shape + (3,)), [], []
    for b in range(data["n_pcs"].shape[0]):
        nv = int(data["part_valids"][b].sum())
        edges, corr = match_edges(data["perm_mat"][b], data["n_critical_pcs"][b], nv)
        conn = np.zeros(nv)
        for idx2, idx1 in edges.tolist():
            conn[idx1] += 1
            conn[idx2] += 1
        T = np.asarray([poses_of(b, k) for k in range(len(edges))], dtype=np.float64).reshape(-1, 4, 4)
        ee, eT = me.translation_edges(data["perm_mat"][b], data["n_critical_pcs"][b], data["critical_pcs_idx"][b], data["part_pcs"][b], data["n_pcs"][b],
                                      nv, conn)
        graph = {"edges": np.concatenate([edges, np.asarray(ee, dtype=np.int64).reshape(-1, 2)]),
                 "transformations": np.concatenate([T, np.asarray(eT, dtype=np.float64).reshape(-1, 4, 4)]),
                 "uncertainty": np.concatenate([1.0 / np.array([c.shape[0] for c in corr], dtype=np.float64), np.ones(len(ee))]), "n_ransac": len(edges)}
        poses, pivot = me.anchor_poses(graph, data["n_pcs"][b], nv, data["part_quat"][b], data["part_trans"][b])
        rot[b, :nv], trans[b, :nv] = poses[:, :3, :3], poses[:, :3, 3]
        pivots.append(pivot)
        graphs.append(graph)
    return rot, trans, pivots, graphs


CHAIN5 = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)]
HOST_PUZZLES = {
    "full": dict(sizes=[200, 210, 190, 205, 195], links=CHAIN5),                                  # pivot moves from 1 to ... 1 (210 is the largest)
    "first_largest": dict(sizes=[230, 210, 190, 205, 195], links=CHAIN5),                         # pivot 0
    "later_larger": dict(sizes=[200, 190, 195, 205, 210], links=CHAIN5),                          # pivot 1 -> 0 -> 3 -> 4 as written
    "cut": dict(sizes=[200, 210, 190, 205, 195], links=[(0, 1), (1, 2), (2, 3), (3, 4)], cut=(3, 4, 2)),      # piece 4 keeps 2 matches
    "no_critical": dict(sizes=[200, 210, 190, 60], links=[(0, 1), (1, 2), (0, 2)]),               # piece 3 owns no critical point
    "two_pieces": dict(sizes=[200, 210], links=[(0, 1)]),
}


@pytest.mark.parametrize("name", sorted(HOST_PUZZLES))
def test_translation_edges_and_pivot_equal_the_restatement(name):
    from pfpp_hip import matching_eval as me

    data = cases.make_puzzle(seed=61, **HOST_PUZZLES[name])
    rng = np.random.default_rng(67)
    fake = [cases.rigid4(rng) for _ in range(16)]
    ref = cases.global_transformation_reference(data, lambda b, k, *a: fake[k], me.global_alignment)
    rot, trans, pivots, graphs = host_pipeline(data, lambda b, k: fake[k])
    g, w = graphs[0], ref["graphs"][0]
    print(name, "edges", g["edges"].tolist(), "ransac", g["n_ransac"], "pivot", pivots)
    assert np.array_equal(g["edges"], w["edges"]) and g["n_ransac"] == w["n_ransac"] and pivots == ref["pivots"]
    assert np.array_equal(g["uncertainty"], w["uncertainty"])
    assert np.abs(g["transformations"] - w["transformations"]).max() <= 1e-12
    assert np.abs(rot - ref["rot"]).max() <= 1e-12 and np.abs(trans - ref["trans"]).max() <= 1e-12
    want_pivot = {"full": 1, "first_largest": 0, "later_larger": 4, "cut": 1, "no_critical": 1, "two_pieces": 1}[name]
    assert pivots == [want_pivot]
    if name in ("cut", "no_critical"):                                       # the translation-only path ran
        assert len(g["edges"]) > g["n_ransac"] and (g["uncertainty"][g["n_ransac"]:] == 1).all()
        assert np.array_equal(g["transformations"][g["n_ransac"]:, :3, :3], np.broadcast_to(np.eye(3), (len(g["edges"]) - g["n_ransac"], 3, 3)))


def test_puzzle_without_any_match_gets_identity_poses_and_pivot_zero():
    from pfpp_hip import matching_eval as me

    data = cases.make_puzzle(seed=61, sizes=[200, 210, 190], links=[(0, 1), (1, 2)])
    data["perm_mat"] = [np.zeros_like(data["perm_mat"][0])]
    ref = cases.global_transformation_reference(data, lambda *a: np.eye(4), me.global_alignment)
    rot, trans, pivots, graphs = host_pipeline(data, lambda b, k: np.eye(4))
    assert len(graphs[0]["edges"]) == 0 and pivots == ref["pivots"] == [0]
    assert np.abs(rot - ref["rot"]).max() <= 1e-12 and np.abs(trans - ref["trans"]).max() <= 1e-12
    # identity poses moved by the pivot's ground truth: every piece gets piece 0's pose
    assert np.allclose(rot[0], cases.quat_rmat(data["part_quat"][0, 0])) and np.allclose(trans[0], data["part_trans"][0, 0])


def test_evaluator_refuses_bad_arguments():
    from pfpp_hip import matching_eval as me

    with pytest.raises(ValueError, match="shape_cd_index"):
        me.MatchingEvaluator(shape_cd_index="other")
    with pytest.raises(ValueError, match="GPU"):
        me.pose_graph([np.zeros((2, 2))], [[1, 1]], np.zeros((1, 8), dtype=np.int64), torch.zeros((1, 8, 3)), [[4, 4]], [2])


def test_evaluate_matching_arguments(tmp_path, capsys):
    from pfpp_hip import evaluate_matching as cli

    (tmp_path / "d").mkdir()
    (tmp_path / "ckpt").write_bytes(b"x")
    for argv in (["--checkpoint", "c"], ["--points", str(tmp_path / "d"), "--features", str(tmp_path / "d"), "--checkpoint", "c"],
                 ["--points", str(tmp_path / "missing"), "--checkpoint", str(tmp_path / "ckpt")],
                 ["--points", str(tmp_path / "d"), "--checkpoint", str(tmp_path / "missing")],
                 ["--points", str(tmp_path / "d"), "--checkpoint", str(tmp_path / "ckpt"), "--n-hyp", "0"],
                 ["--points", str(tmp_path / "d"), "--checkpoint", str(tmp_path / "ckpt"), "--shape-cd-index", "other"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    capsys.readouterr()
    assert cli.main(["--points", str(tmp_path / "d"), "--checkpoint", str(tmp_path / "ckpt")]) == 1          # an empty directory
    assert "no <data_id>.npz" in capsys.readouterr().err
