"""Generate tests/golden/matching_pose.npz by RUNNING THE REFERENCE's horn_87 on the seeded point triples of tests/matching_pose_cases.py.

    python tools/make_matching_pose_goldens.py --reference <checkout of the reference>

Imported from <reference>/Jigsaw_matching (sys.dont_write_bytecode, nothing is copied): utils/pairwise_alignment.py, as a file - the
package's __init__ is not needed.  Every triple runs twice: as the reference is (its result is float32, pairwise_alignment.py:79)
and with the two `.astype(np.float32)` of that line lifted by handing the module an `np` whose float32 is float64; the lifted run is
asserted to round to the reference's own result.  The weight is the 3 x 3 identity: unit weights, what the RANSAC's pose uses.
Also imported, as the two files of a package stub so that utils/global_alignment/__init__.py (which pulls in gtsam) never runs:
utils/global_alignment/pose_graph_utils.py (connect_graph, minimum_spanning_tree; networkx) and spanning_tree_alignment.py.  For every
graph of matching_pose_cases.graph_cases() the tool does what global_alignment(method='spanning_tree') does around them - the hub's
auxiliary edges of uncertainty 1, here with identity transformations (the reference's commented-out line 25), the alignment over
v_num + 1 vertices, re-referencing to vertex 0 - and asserts that connect_graph joined the hub to the smallest vertex of every
component, the rule pfpp_hip.matching_eval.connect_graph fixes.
The fixture holds results only: horn_R [n, 3, 3], horn_t [n, 3] (float64), horn_R32, horn_t32 (the reference as it is); per graph
graph_<name>_aux (the auxiliary edges), graph_<name>_order / _pred (the tree's preorder and predecessors over v_num + 1 vertices) and
graph_<name>_poses [v_num, 4, 4]."""
import argparse
import importlib.util
import sys
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class NumpyFor:
    """numpy itself, but float32 (the casts of pairwise_alignment.py:79) is the run's dtype"""

    def __init__(self, f32):
        self.float32 = f32

    def __getattr__(self, name):
        return getattr(np, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds Jigsaw_matching/)")
    args = ap.parse_args()
    cases = load("matching_pose_cases", ROOT / "tests" / "matching_pose_cases.py")
    pa = load("ref_pairwise_alignment", Path(args.reference) / "Jigsaw_matching" / "utils" / "pairwise_alignment.py")
    S, T = cases.horn_inputs()
    out = {k: [] for k in ("horn_R", "horn_t", "horn_R32", "horn_t32")}
    for s, t in zip(S, T):
        pa.np = np
        R32, t32 = pa.horn_87(s, t, np.eye(3))
        pa.np = NumpyFor(np.float64)
        R64, t64 = pa.horn_87(s, t, np.eye(3))
        assert R32.dtype == np.float32 and R64.dtype == np.float64
        assert np.array_equal(R64.astype(np.float32), R32) and np.array_equal(t64.astype(np.float32), t32)
        for k, v in zip(out, (R64, t64, R32, t32)):
            out[k].append(v)
    pa.np = np
    import types

    ga_dir = Path(args.reference) / "Jigsaw_matching" / "utils" / "global_alignment"
    stub = types.ModuleType("ref_global_alignment")
    stub.__path__ = [str(ga_dir)]
    sys.modules["ref_global_alignment"] = stub
    import importlib

    pgu = importlib.import_module("ref_global_alignment.pose_graph_utils")
    sta = importlib.import_module("ref_global_alignment.spanning_tree_alignment")
    graphs = {}
    for name, (v, edges, T, u) in cases.graph_cases().items():
        aux = pgu.connect_graph(v, edges)
        comp_min = sorted(set(int(a[1]) for a in aux))
        label = list(range(v))
        for a, b in edges.tolist():
            la, lb = label[a], label[b]
            label = [min(la, lb) if x in (la, lb) else x for x in label]
        assert comp_min == sorted(set(label)), (name, aux, "connect_graph did not pick the smallest vertex of a component")
        all_e = np.concatenate([edges, aux], axis=0).astype(np.int32)
        all_T = np.concatenate([T, np.repeat(np.eye(4)[np.newaxis], aux.shape[0], axis=0)], axis=0)
        all_u = np.concatenate([u, np.ones(aux.shape[0])])
        order, pred = pgu.minimum_spanning_tree(v + 1, all_e, all_u)
        poses, _ = sta.spanning_tree_alignment(v + 1, all_e, all_T, all_u)
        for i in range(v):
            poses[v - i - 1] = np.linalg.inv(poses[0]) @ poses[v - i - 1]
        graphs[f"graph_{name}_aux"] = np.asarray(aux, dtype=np.int64)
        graphs[f"graph_{name}_order"] = np.asarray(order, dtype=np.int64)
        graphs[f"graph_{name}_pred"] = np.asarray([pred.get(k, -1) for k in range(v + 1)], dtype=np.int64)
        graphs[f"graph_{name}_poses"] = poses[:v]
    path = ROOT / "tests" / "golden" / "matching_pose.npz"
    np.savez_compressed(path, **{k: np.stack(v) for k, v in out.items()}, **graphs)
    print(path, {k: np.stack(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
