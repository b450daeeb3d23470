"""No GPU: pfpp_hip.matching_edges.pack_matches_reference, the numpy statement of pfpp_match_edges' outputs built from match_edges and
AutoAgglomerative.prepare_matching, against the reference's own compute_global_transformation (tests/golden/matching_head.npz); the
properties the seeded cases were built for; the dataset's `matching=` keyword; and the argument checks of the two new entry points,
all of which return before a launch."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matching_cases as cases
import matching_edges_cases as EC

ROOT = Path(__file__).resolve().parents[1]


def reference(batch: EC.Batch, **kw):
    from pfpp_hip.matching_edges import pack_matches_reference

    return pack_matches_reference(batch.perm, batch.n_critical_pcs, batch.n_valid, batch.n_pcs, batch.critical_pcs_idx, **kw)


@pytest.mark.parametrize("names", [("five",), ("two",), ("split",), ("five", "two", "split")])
def test_packed_reference_reproduces_the_fixture(golden, names):
    """pack_matches_reference -> DeviceMatches.files(b) = *_edges, *_corr_cat and *_corr_len of the fixture, alone and in a batch"""
    from pfpp_hip.matching_edges import DeviceMatches

    g = golden("matching_head")
    batch = EC.fixture_batch(g, names)
    out = reference(batch)
    assert (out["status"] == 0).all() and all(out[k].dtype == np.int32 for k in ("counts", "edge_off", "kept", "corr", "idx_a", "idx_b", "status"))
    dm = DeviceMatches.from_arrays(out, batch.n_pcs)
    for b, name in enumerate(names):
        edges, corr = dm.files(b)
        assert edges.dtype == np.int64 and np.array_equal(edges, g[f"{name}_edges"])
        assert [c.shape[0] for c in corr] == g[f"{name}_corr_len"].tolist() and all(c.dtype == np.int64 for c in corr)
        assert np.array_equal(np.concatenate(corr, 0), g[f"{name}_corr_cat"].astype(np.int64))
        n, M = batch.perm[b].size, dm.n_correspondences(b)
        r0 = int(out["row_off"][b])
        assert 0 < M <= n and (out["corr"][r0 + M:r0 + n] == -1).all() and (out["idx_a"][r0 + M:r0 + n] == -1).all()
        # idx_a / idx_b as get_distance_for_matching_pts forms them
        start = np.cumsum(batch.n_pcs[b]) - batch.n_pcs[b]
        crit = batch.critical_pcs_idx[b]
        s1, s2 = start[np.repeat(edges[:, 1], [c.shape[0] for c in corr])], start[np.repeat(edges[:, 0], [c.shape[0] for c in corr])]
        cat = np.concatenate(corr, 0)
        assert np.array_equal(out["idx_a"][r0:r0 + M], s1 + crit[s1 + cat[:, 0]]) and np.array_equal(out["idx_b"][r0:r0 + M], s2 + crit[s2 + cat[:, 1]])


def test_seeded_cases_hold_what_they_were_built_for():
    from pfpp_hip.matching import match_edges
    from pfpp_hip.matching_edges import DeviceMatches, triangle_pairs

    batch = EC.seeded_batch()
    out = reference(batch, fill=EC.CANARY)
    dm = DeviceMatches.from_arrays(out, batch.n_pcs)
    assert batch.n_critical_pcs[0].tolist() == [63, 64, 65, 257, 0, 1, 130, 1025] and (out["status"] == 0).all()
    p0 = batch.perm[0]
    piece = np.repeat(np.arange(8), batch.n_critical_pcs[0])
    rows = np.nonzero(p0 >= 0)[0]
    assert 0.03 < (p0 < 0).mean() < 0.07 and (piece[rows] == piece[p0[rows]]).sum() > 100        # unmatched rows; same-piece matches
    assert out["kept"][0].sum() >= 10 and int(out["edge_off"][0, -1]) < p0.size
    # the rule puzzle, by hand
    e, c = dm.files(1)
    by_pair = {(int(i1), int(i2)): x.tolist() for (i2, i1), x in zip(e, c)}
    cnt = out["counts"][1]
    assert (cnt[0, 1], cnt[1, 0]) == (2, 1) and (0, 1) not in by_pair                            # exactly 2: dropped
    assert (cnt[0, 2], cnt[2, 0]) == (3, 0) and by_pair[(0, 2)] == [[2, 5], [3, 1], [4, 7]]      # exactly 3: kept
    assert (cnt[1, 2], cnt[2, 1]) == (3, 3) and by_pair[(1, 2)] == [[1, 0], [2, 2], [3, 3]]      # a tie: the first block
    assert (cnt[0, 3], cnt[3, 0]) == (2, 4) and by_pair[(0, 3)] == [[1, 3], [3, 2], [7, 1], [9, 0]]   # transposed, in column order
    assert cnt[6, 6] == 3 and by_pair[(6, 7)] == [[4, 0], [5, 1], [6, 2], [7, 3]] and sorted(by_pair) == [(0, 2), (0, 3), (1, 2), (6, 7)]
    # n_valid = 2: one pair is looked at although four pieces have matches
    assert batch.n_valid[2] == 2 and (out["counts"][2][2:4, :4] > 0).any() and dm.files(2)[0].tolist() == [[1, 0]]
    for b in (3, 5):                                                                              # no rows: nothing
        assert batch.perm[b].size == 0 and not out["kept"][b].any() and not out["counts"][b].any() and not out["edge_off"][b].any()
    assert batch.n_critical_pcs[3].sum() > 0 and batch.n_critical_pcs[5].sum() == 0
    assert batch.perm[6].size == 100 < batch.n_critical_pcs[6].sum() and dm.files(6)[0].tolist() == [[1, 0]]      # fewer rows than critical points
    # every puzzle: what match_edges says, and offsets over the triangle slots in row-major order
    tri = triangle_pairs(8)
    assert tri[:8].tolist() == [[0, k] for k in range(1, 8)] + [[1, 2]]
    for b in range(len(batch.perm)):
        e0, c0 = match_edges(batch.perm[b], batch.n_critical_pcs[b], int(batch.n_valid[b]))
        e1, c1 = dm.files(b)
        assert np.array_equal(e0, e1) and len(c0) == len(c1) and all(np.array_equal(x, y) for x, y in zip(c0, c1))
        assert np.array_equal(np.diff(out["edge_off"][b])[out["kept"][b] == 1], [x.shape[0] for x in c0])
        assert (np.diff(out["edge_off"][b])[out["kept"][b] == 0] == 0).all()
    # all pairs
    ap = EC.all_pairs_batch()
    oa = reference(ap)
    assert oa["kept"].sum() == 190 and int(oa["edge_off"][0, -1]) == 570 and ap.perm[0].size == 1140
    assert (oa["counts"][0] == 3 * (1 - np.eye(20, dtype=np.int32))).all() and (np.diff(oa["edge_off"][0]) == 3).all()


@pytest.mark.parametrize("kind,status", [("duplicate", 1), ("too_large", 2), ("negative", 2)])
def test_reference_status_of_bad_input(kind, status):
    bad = EC.bad_batch(kind)
    out = reference(bad, fill=EC.CANARY)
    assert out["status"].tolist() == [0, status, 0]
    r0, r1 = int(out["row_off"][1]), int(out["row_off"][2])
    assert not out["kept"][1].any() and not out["counts"][1].any() and not out["edge_off"][1].any() and (out["corr"][r0:r1] == EC.CANARY).all()
    assert out["kept"][0].any() and out["kept"][2].any()
    good = EC.bad_batch(kind)
    good.perm[1][good.perm[1] < -1] = -1
    good.perm[1][good.perm[1] >= good.perm[1].size] = -1
    if kind == "duplicate":
        rows = np.nonzero(good.perm[1] >= 0)[0]
        good.perm[1][rows[7]] = -1
    assert reference(good)["kept"][1].any()                   # without the broken entry the puzzle has edges


def test_dataset_takes_matching_from_a_mapping(golden, tmp_path):
    """GeometryLatentDataset(matching=mapping) gives the item the directory of files gives, and skips a puzzle the mapping lacks"""
    from pfpp_hip import io as pfio
    from pfpp_hip.matching import match_edges, write_matching_data
    from puzzlefusion_plusplus.denoiser.dataset.dataset import GeometryLatentDataset

    g = golden("matching_head")
    pz = cases.make_puzzle("five")
    edges, corr = match_edges(g["five_perm"].astype(np.int64), g["five_n_critical_pcs"], 5)
    mdir = tmp_path / "matching_data"
    path = write_matching_data(str(mdir), pz["data_id"], edges=edges, correspondence=corr, gt_pcs=pz["gt_pcs"],
                               critical_pcs_idx=g["five_critical_pcs_idx"].astype(np.int64), n_pcs=pz["n_pcs"], n_critical_pcs=g["five_n_critical_pcs"])
    rng = np.random.default_rng(0)
    ref = np.zeros(20, dtype=bool)
    ref[0] = True
    for did in (pz["data_id"], 99):
        pfio.save_pc_data(str(tmp_path / "pc_data"), data_id=did, part_valids=pz["part_valids"], num_parts=5, mesh_file_path="a/b",
                          graph=np.zeros((20, 20), dtype=bool), category="everyday", part_pcs_gt=rng.normal(size=(5, 64, 3)), ref_part=ref)
    cfg = NS(data=NS(max_num_part=20, matching_data_path=str(mdir)), model=NS(multiple_ref_parts=False))
    mapping = {pz["data_id"]: dict(pfio.load_matching_data(path), matching_prepared={"max_m": 3})}
    from_dir = GeometryLatentDataset(cfg, str(tmp_path / "pc_data"), -1, "test")
    from_map = GeometryLatentDataset(NS(data=NS(max_num_part=20, matching_data_path="/nowhere"), model=cfg.model), str(tmp_path / "pc_data"), -1,
                                     "test", matching=mapping)
    assert len(from_dir) == len(from_map) == 1
    np.random.seed(4)
    a = from_dir[0]
    np.random.seed(4)
    b = from_map[0]
    assert b.pop("matching_prepared") == {"max_m": 3} and set(a) == set(b)
    for k in a:
        if k == "correspondences":
            assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    with pytest.raises(ValueError, match="test split"):
        GeometryLatentDataset(cfg, str(tmp_path / "pc_data"), -1, "train", matching=mapping)


def test_wrapper_refuses_what_it_cannot_run():
    from pfpp_hip.matching_edges import match_edges_batch

    nc = torch.zeros((1, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="dense_perm=False"):
        match_edges_batch([torch.zeros((4, 4))], nc, [2], np.array([[3, 3]]), [torch.zeros(6, dtype=torch.int64)])
    with pytest.raises(ValueError, match="GPU"):
        match_edges_batch([torch.zeros(4, dtype=torch.int64)], nc, [2], np.array([[3, 3]]), [torch.zeros(6, dtype=torch.int64)])
    with pytest.raises(ValueError, match="no puzzles"):
        match_edges_batch([], nc, [], np.zeros((0, 2)), [])


def test_new_entries_are_declared_bound_counted_and_refuse_bad_arguments_before_a_launch(hip_lib):
    from pfpp_hip import _lib, build
    from pfpp_hip.matching_edges import MAX_P, MAX_PUZZLES, MAX_ROWS

    raw = (ROOT / "include" / "pfpp.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    assert "int pfpp_match_edges(" in text and "int64_t pfpp_match_edges_workspace(" in text
    assert "matching_base_model.py:298-359" in raw and "auto_aggl.py:92-126" in raw
    assert "pfpp_match_edges" in _lib.SIGNATURES and hasattr(lib, "pfpp_match_edges")
    # the query returns int64, so it is bound in the table of entries that do not return int (as pfpp_match_assign_workspace is)
    assert "pfpp_match_edges_workspace" in _lib.PLAIN and hasattr(lib, "pfpp_match_edges_workspace")
    assert "matching_edges.hip" in build.SOURCES and lib.pfpp_version() == 2
    n_entries = len(re.findall(r"^(?:int|int64_t|const char\*|unsigned)\s+pfpp_\w+\s*\(", text, flags=re.M))
    assert f"{n_entries} entry points" in (ROOT / "README.md").read_text()
    for name, value in (("MAX_P", MAX_P), ("MAX_ROWS", MAX_ROWS), ("MAX_PUZZLES", MAX_PUZZLES)):
        assert int(re.search(rf"#define PFPP_MATCH_EDGES_{name} (\d+)", raw).group(1)) == value
    assert len(_lib.SIGNATURES["pfpp_match_edges"]) == 21

    assert lib.pfpp_match_edges_workspace(0) == 0 and lib.pfpp_match_edges_workspace(2492 * 16) == 4 * 2492 * 16
    assert lib.pfpp_match_edges_workspace(-1) == -1
    one = C.c_void_p(4096)                                  # a non-null, aligned address that is never dereferenced on these paths
    ptrs = ["col", "row_off", "n_crit", "n_valid", "piece_off", "crit", "counts", "edge_off", "kept", "corr", "idx_a", "idx_b", "status", "ws"]

    def call(B=2, P=8, max_rows=100, total_rows=150, total_points=400, ws_bytes=600, **null):
        p = {k: (None if k in null else one) for k in ptrs}
        p.update({k: v for k, v in null.items() if v is not None})
        return lib.pfpp_match_edges(p["col"], p["row_off"], p["n_crit"], p["n_valid"], p["piece_off"], p["crit"], B, P, max_rows, total_rows,
                                    total_points, p["counts"], p["edge_off"], p["kept"], p["corr"], p["idx_a"], p["idx_b"], p["status"], p["ws"],
                                    ws_bytes, None)

    for k in ptrs:
        assert call(**{k: None}) == -1 and b"null" in lib.pfpp_last_error(), k
    for P in (0, 33, -1):
        assert call(P=P) == -2 and b"unsupported" in lib.pfpp_last_error(), P
    assert call(max_rows=65536, total_rows=70000, ws_bytes=280000) == -2 and b"65535 rows" in lib.pfpp_last_error()
    assert call(B=65536) == -2 and b"65535 puzzles" in lib.pfpp_last_error()
    assert call(B=0) == 0 and call(B=0, col=None, ws=None, status=None) == 0            # nothing to do
    assert call(B=0, P=33) == -2                                                            # the ranges hold for an empty batch too
    assert call(B=-1) == -1 and call(max_rows=151) == -1 and call(total_points=-1) == -1
    assert call(ws_bytes=599) == -1 and b"workspace" in lib.pfpp_last_error()
    assert call(ws=C.c_void_p(4098)) == -1 and call(corr=C.c_void_p(4100)) == -1 and b"aligned" in lib.pfpp_last_error()
