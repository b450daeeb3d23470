"""CPU: the host half of pc_data generation (pfpp_hip/meshes.py read_obj, vqvae/dataset/dataset.py discovery) and the mesh fixture.

tests/golden/mesh_pc_data.npz was written by tools/make_mesh_goldens.py from the reference's own dataset.py over the tree
`tools/make_synthetic_meshes.py DIR` writes."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

OBJ_TEXT = """# hand-written
v 0 0 0
v 1 0 0
v 1 1 0   # trailing comment
v 0 1 0
v 9 9 9
vn 0 0 1
vt 0.5 0.5
v 0.5 0.5 1 1.0
v 2 0 0
f 1/1 2/1 3/1 4/1
f -4//1 -6//1 -7//1
o name
f 2/1/1 7/1/1 3/1/1
f 1 2 7 6 4
l 1 2
"""


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    d = tmp_path_factory.mktemp("meshes")
    subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_meshes.py"), str(d)], check=True, capture_output=True)
    return d


def test_read_obj_records_slashes_negative_indices_polygons_and_unreferenced_vertices(tmp_path):
    from pfpp_hip.meshes import read_obj

    p = tmp_path / "m.obj"
    p.write_text(OBJ_TEXT)
    v, f = read_obj(str(p))
    # vertex 5 (9, 9, 9) is never referenced: dropped, the later ones move down by one
    want_v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1], [2, 0, 0]], dtype=np.float64)
    # quad -> (0,1,2), (0,2,3); "-4 -6 -7" after seven vertices -> 4, 2, 1 (1-based); pentagon fan (0, i, i + 1)
    want_f = np.array([[0, 1, 2], [0, 2, 3], [3, 1, 0], [1, 5, 2], [0, 1, 5], [0, 5, 4], [0, 4, 3]], dtype=np.int32)
    assert v.dtype == np.float64 and f.dtype == np.int32
    np.testing.assert_array_equal(v, want_v)
    np.testing.assert_array_equal(f, want_f)


def test_read_obj_refuses_bad_indices(tmp_path):
    from pfpp_hip.meshes import read_obj

    p = tmp_path / "bad.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError, match="outside"):
        read_obj(str(p))


def test_discovery_equals_the_reference_data_list(tree, golden, monkeypatch):
    import torch

    from puzzlefusion_plusplus.vqvae.dataset.dataset import GeometryPartDataset

    touched = []
    monkeypatch.setattr(torch.cuda, "init", lambda: touched.append(1))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: touched.append(1))
    g = golden("mesh_pc_data")
    for split in ("train", "val"):
        ds = GeometryPartDataset(str(tree), f"everyday.{split}.txt", ["part_ids"], None, category="all", num_points=50)
        assert ds.data_list == [str(x) for x in g[f"{split}_data_list"]]
        item = ds[0]                                        # host work only
        assert item["mesh_file_path"] == ds.data_list[0] and len(item["meshes"]) >= 2
    ds = GeometryPartDataset(str(tree), "everyday.train.txt", ["part_ids"], None, category="Bowl")
    assert ds.data_list == [str(x) for x in g["train_data_list"] if "/Bowl/" in str(x)]
    assert GeometryPartDataset(str(tree), "everyday.train.txt", ["part_ids"], None, category="bowl").data_list == []   # case-sensitive
    assert not touched


def _set_graph(meshes):
    """_are_meshes_connected (dataset.py:85-107) restated: sets of np.round(., 5) vertex tuples"""
    P = len(meshes)
    g = np.zeros((P, P), dtype=bool)
    sets = [set(map(tuple, np.round(v, 5))) for v, _ in meshes]
    for i in range(P):
        for j in range(i + 1, P):
            g[i, j] = g[j, i] = len(sets[i] & sets[j]) > 0
    return g


def test_fixture_chebyshev_truth_equals_the_set_restatement(tree):
    from pfpp_hip.meshes import read_obj

    truth = json.loads((tree / "truth.json").read_text())
    n_grid = 0
    for rel, t in truth.items():
        d = tree / rel
        meshes = [read_obj(str(d / f)) for f in sorted(os.listdir(d))]
        g = _set_graph(meshes)
        if t is not None:
            np.testing.assert_array_equal(g, np.array(t), err_msg=rel)
            n_grid += 1
    assert n_grid >= 8
