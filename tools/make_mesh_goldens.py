"""Write tests/golden/mesh_pc_data.npz by RUNNING THE REFERENCE's vqvae/dataset/dataset.py (build container only).

    python tools/make_mesh_goldens.py            # needs /root/reference; writes tests/golden/mesh_pc_data.npz

The reference's GeometryPartDataset is imported verbatim (sys.dont_write_bytecode, nothing is copied) over the small tree of
tools/make_synthetic_meshes.py, with a stand-in for trimesh (not installed): `load` is a minimal OBJ reader written here (v / f
records, fan triangulation, unreferenced vertices dropped), `sample.sample_surface` is trimesh 4.0.2's algorithm restated
(cumsum of the face areas, searchsorted of N uniforms times the total, N x 2 uniforms folded into the triangle), driven by a
seeded numpy Generator whose draws are recorded so that the GPU path can be fed the same uniforms.
Per split: data_list; per item: data_id, mesh_file_path, category, num_parts, part_valids, graph, ref_part, part_pcs_gt and the
uniforms [Pv, N, 3] = (u0, l0, l1)."""
from __future__ import annotations

import importlib.util
import subprocess
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parents[1]
REF = Path("/root/reference")
GOLD = ROOT / "tests" / "golden" / "mesh_pc_data.npz"
NUM_POINTS = 50


class _Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces

    @property
    def area_faces(self):
        t = self.vertices[self.faces]
        u, v = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        c0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        c1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        c2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        return np.sqrt((c0 * c0 + c1 * c1) + c2 * c2) / 2.0


def _load(path):
    verts, faces = [], []
    with open(path) as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                idx = [int(t.split("/")[0]) for t in tok[1:]]
                idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                faces += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    v, f = np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)
    used = np.unique(f)
    remap = np.full(len(v), -1)
    remap[used] = np.arange(len(used))
    return _Mesh(v[used], remap[f])


class _Sampler:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.draws = []

    def sample_surface(self, mesh, count):
        cdf = np.cumsum(mesh.area_faces)
        u0 = self.rng.random(count)
        face = np.searchsorted(cdf, u0 * cdf[-1])
        origins = mesh.vertices[mesh.faces[:, 0]]
        vectors = mesh.vertices[mesh.faces[:, 1:]].copy()
        vectors -= np.tile(origins, (1, 2)).reshape((-1, 2, 3))
        origins, vectors = origins[face], vectors[face]
        lengths = self.rng.random((len(vectors), 2, 1))
        self.draws.append(np.stack([u0, lengths[:, 0, 0], lengths[:, 1, 0]], axis=1))
        test = lengths.sum(axis=1).reshape(-1) > 1.0
        lengths[test] -= 1.0
        lengths = np.abs(lengths)
        return (vectors * lengths).sum(axis=1) + origins, face


def main():
    if not REF.exists():
        sys.exit("make_mesh_goldens: the reference checkout is not here")
    sampler = _Sampler(20261016)
    tm = types.ModuleType("trimesh")
    tm.load = _load
    tm.sample = types.SimpleNamespace(sample_surface=sampler.sample_surface)
    sys.modules["trimesh"] = tm
    spec = importlib.util.spec_from_file_location("ref_vqvae_dataset", REF / "puzzlefusion_plusplus/vqvae/dataset/dataset.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_meshes.py"), tmp], check=True)
        for split in ("train", "val"):
            ds = ref.GeometryPartDataset(tmp, f"everyday.{split}.txt", ["part_ids"], None, category="all", num_points=NUM_POINTS,
                                         min_num_part=2, max_num_part=20, shuffle_parts=False)
            out[f"{split}_data_list"] = np.array(ds.data_list)
            for i in range(len(ds)):
                sampler.draws.clear()
                d = ds[i]
                p = f"{split}_{i}_"
                for k in ("data_id", "num_parts"):
                    out[p + k] = np.int64(d[k])
                for k in ("mesh_file_path", "category"):
                    out[p + k] = np.array(d[k])
                for k in ("part_valids", "graph", "ref_part", "part_pcs_gt"):
                    out[p + k] = np.asarray(d[k])
                out[p + "uniforms"] = np.stack(sampler.draws)
    GOLD.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(GOLD, **out)
    print(f"wrote {GOLD} ({GOLD.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
