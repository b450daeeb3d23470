"""Write tests/golden/matching_dataset.npz by RUNNING THE REFERENCE's Jigsaw_matching/dataset/all_piece_matching_dataset.py (build
container only).

    python tools/make_matching_dataset_goldens.py      # needs /root/reference; writes tests/golden/matching_dataset.npz

The reference's AllPieceMatchingDataset is imported verbatim (sys.dont_write_bytecode, nothing is copied) over the small tree of
tools/make_synthetic_meshes.py, with the stand-in for trimesh of tools/make_mesh_goldens.py (not installed): load(..., force="mesh"),
.area = area_faces.sum() and .sample(n, return_index=True) = trimesh 4.0.2's sample_surface, driven by a seeded generator.  Three
kinds of draws are recorded so that the GPU path can be fed the same ones: the uniforms (u0, l0, l1) of every sample, the
permutation of every random.shuffle (_shuffle_pc) and every rotation matrix (R.random()).
Settings: (num_points, min_part_point) = (251, 20) and (997, 30).  Per setting and split: data_list; per item: every key of the
reference's data_dict, areas [P], uniforms [N, 3] and order [N] (piece after piece), rot [P, 3, 3].
The tool asserts what makes the fixture robust against the last-bit differences between numpy's sums and the kernels' (areas N /
total at least 1e-6 away from an integer, no face pick within 1e-12 total of a cdf value) and that both branches of the reference's
`while delta > 0` loop ran; when an assertion on the draws fails it reseeds."""
from __future__ import annotations

import importlib.util
import random as pyrandom
import subprocess
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import make_mesh_goldens as mmg  # noqa: E402  (the trimesh stand-in: _Mesh, _load, _Sampler)

REF = Path("/root/reference")
GOLD = ROOT / "tests" / "golden" / "matching_dataset.npz"
SETTINGS = ((251, 20), (997, 30))
SEED = 20261020


class _Draws:
    """the three seeded sources and what they gave"""

    def __init__(self, seed):
        self.sampler = mmg._Sampler(seed)
        self.shuffler = pyrandom.Random(seed + 1)
        self.rot_rng = np.random.default_rng(seed + 2)
        self.orders, self.rots, self.picks = [], [], []

    def clear(self):
        self.sampler.draws.clear()
        self.orders.clear()
        self.rots.clear()

    def sample(self, mesh, count, return_index=False):
        pts, face = self.sampler.sample_surface(mesh, int(count))
        cdf = np.cumsum(mesh.area_faces)
        pick = self.sampler.draws[-1][:, 0] * cdf[-1]
        self.picks.append(float(np.abs(pick[:, None] - cdf[None]).min() / cdf[-1]))
        return (pts, face) if return_index else pts

    def shuffle(self, x):
        self.shuffler.shuffle(x)
        self.orders.append(np.array(x, dtype=np.int32))

    def random_rotation(self):
        r = Rotation.random(random_state=self.rot_rng)
        self.rots.append(r.as_matrix())
        return r


def _loop_branches(nps, num_points, min_part_point):
    """the `while delta > 0` loop of sample_reweighted_points_by_areas on the ceil counts -> (raised, one_step, clamp, result)"""
    nps = np.array(nps, dtype=np.int64)
    raised = one = clamp = 0
    delta = 0
    for i in range(len(nps)):
        if nps[i] < min_part_point:
            delta += min_part_point - nps[i]
            nps[i] = min_part_point
            raised += 1
    while delta > 0:
        k = np.argmax(nps)
        if nps[k] - delta >= min_part_point:
            nps[k] -= delta
            delta = 0
            one += 1
        else:
            delta -= nps[k] - min_part_point
            nps[k] = min_part_point
            clamp += 1
    return raised, one, clamp, nps


def generate(ref, tmp, seed):
    draws = _Draws(seed)

    class _Mesh(mmg._Mesh):
        @property
        def area(self):
            return self.area_faces.sum()

        def sample(self, count, return_index=False):
            return draws.sample(self, count, return_index)

    def load(path, force=None):
        assert force == "mesh"
        m = mmg._load(path)
        return _Mesh(m.vertices, m.faces)

    ref.trimesh.load = load
    ref.random = types.SimpleNamespace(shuffle=draws.shuffle)
    ref.R = types.SimpleNamespace(random=draws.random_rotation, from_euler=Rotation.from_euler, from_matrix=Rotation.from_matrix)
    out, branches, margin = {}, np.zeros(3, dtype=np.int64), np.inf
    for num_points, min_part_point in SETTINGS:
        for split in ("train", "val"):
            ds = ref.AllPieceMatchingDataset(tmp, f"everyday.{split}.txt", ["part_ids"], category="all", num_points=num_points,
                                             min_num_part=2, max_num_part=20, shuffle_parts=False, rot_range=-1, overfit=-1, length=-1,
                                             sample_by="area", min_part_point=min_part_point, fracture_label_threshold=0.025)
            out[f"{split}_data_list"] = np.array(ds.data_list)
            for i in range(len(ds)):
                draws.clear()
                d = ds[i]
                p = f"n{num_points}_{split}_{i}_"
                P = int(d["num_parts"])
                for k in ("data_id", "num_parts"):
                    out[p + k] = np.int64(d[k])
                out[p + "mesh_file_path"] = np.array(d["mesh_file_path"])
                for k in ("part_pcs", "gt_pcs", "part_valids", "part_quat", "part_trans", "n_pcs", "critical_label_thresholds"):
                    out[p + k] = np.asarray(d[k])
                folder = Path(tmp) / d["mesh_file_path"]
                areas = np.array([load(str(folder / f), force="mesh").area for f in sorted(f.name for f in folder.iterdir())])
                out[p + "areas"] = areas
                out[p + "uniforms"] = np.concatenate(draws.sampler.draws)
                out[p + "order"] = np.concatenate(draws.orders)
                out[p + "rot"] = np.stack(draws.rots)
                assert len(draws.rots) == P and out[p + "uniforms"].shape == (num_points, 3) and out[p + "order"].shape == (num_points,)
                x = areas * num_points / np.sum(areas)
                margin = min(margin, float(np.abs(x - np.round(x)).min()))
                first = ref.AllPieceMatchingDataset.sample_points_by_areas(areas, num_points)
                r, one, clamp, nps = _loop_branches(first, num_points, min_part_point)
                assert np.array_equal(nps, d["n_pcs"][:P]), (p, nps, d["n_pcs"])
                branches += (r, one, clamp)
    assert margin > 1e-6, f"areas N / total within {margin} of an integer"
    assert branches.min() > 0, f"loop branches (raised, one step, clamp) = {branches}"
    pick = min(draws.picks)
    if not pick > 1e-12:
        raise RuntimeError(f"a face pick lies within {pick} total of a cdf value")
    print(f"seed {seed}: count margin {margin:.4f}, face pick margin {pick:.2e} total, loop (raised, one step, clamp) = {branches.tolist()}")
    return out


def main():
    if not REF.exists():
        sys.exit("make_matching_dataset_goldens: the reference checkout is not here")
    sys.modules["trimesh"] = types.ModuleType("trimesh")
    spec = importlib.util.spec_from_file_location("ref_all_piece_matching_dataset", REF / "Jigsaw_matching/dataset/all_piece_matching_dataset.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_meshes.py"), tmp], check=True)
        for attempt in range(16):
            try:
                out = generate(ref, tmp, SEED + 10 * attempt)
                break
            except RuntimeError as e:          # only the draws can be helped by another seed
                print(f"reseeding: {e}")
        else:
            sys.exit("make_matching_dataset_goldens: no seed passed the margins")
    GOLD.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLD, **out)
    print(f"wrote {GOLD} ({GOLD.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
