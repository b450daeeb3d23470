"""Write a deterministic tree of fracture meshes shaped like the Breaking Bad dataset (the input of pfpp_hip.generate_pc_data):

    python tools/make_synthetic_meshes.py DIR              # the small tree of the tests and tests/golden/mesh_pc_data.npz
    python tools/make_synthetic_meshes.py DIR --bench 16   # 16 puzzles of 20 parts, ~2-8k faces per part (tools/pc_data_bench.py)

DIR/everyday.{train,val}.txt list objects; DIR/everyday/<Category>/<id>/{fractured_<k>,mode_0}/piece_<i>.obj hold the parts.
Fragments are the cells of an nx x ny x nz box grid whose surfaces are triangulated on one shared lattice (touching cells share
bit-identical vertices), the whole assembly under one rigid transform; the first cell is clearly the largest.  Ground truth:
cells at Chebyshev distance 1 share a vertex.  Cases for discovery to reject or skip: a folder that is neither "fractured" nor
"mode", a 1-part and a 21-part fracture, a listed object that does not exist.  Rounding cases: a cell shifted by 3e-5
(disconnected), vertices at and one ulp around 5-decimal rounding midpoints, +0 / -0 coordinates.  DIR/truth.json holds the
expected contact graph of every folder."""
from __future__ import annotations

import argparse
import itertools
import json
import os

import numpy as np

FMT = "%.17g"


def rotation(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def transform(p: np.ndarray, R: np.ndarray, t: np.ndarray) -> np.ndarray:
    """R p + t written out per element, so equal inputs give bit-identical outputs whatever the array they sit in"""
    out = np.empty_like(p)
    for a in range(3):
        out[:, a] = ((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a]
    return out


def box_surface(lo, hi, h):
    """triangulated surface of the integer-lattice box [lo, hi] (lattice units of h): vertices [V, 3] (integers), faces [F, 3]"""
    verts, faces, index = [], [], {}

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for ax in range(3):
        u, v = [a for a in range(3) if a != ax]
        for side in (lo[ax], hi[ax]):
            for i in range(lo[u], hi[u]):
                for j in range(lo[v], hi[v]):
                    q = []
                    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[ax], p[u], p[v] = side, i + du, j + dv
                        q.append(vid(tuple(p)))
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


def write_obj(path, verts, faces):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("# synthetic fragment\n")
        for v in verts:
            fh.write("v " + " ".join(FMT % float(c) for c in v) + "\n")
        for f in faces:
            fh.write("f " + " ".join(str(int(i) + 1) for i in f) + "\n")


def grid_puzzle(folder, dims, widths, h, R, t, shift=None):
    """cells of a grid; widths[a] = cell widths (lattice units) along axis a.  -> ground-truth graph in sorted file-name order"""
    breaks = [np.concatenate([[0], np.cumsum(w)]).astype(int) for w in widths]
    cells = list(itertools.product(*[range(d) for d in dims]))
    for n, c in enumerate(cells):
        lo = [int(breaks[a][c[a]]) for a in range(3)]
        hi = [int(breaks[a][c[a] + 1]) for a in range(3)]
        v, f = box_surface(lo, hi, h)
        p = transform(v * h, R, t)
        if shift is not None and n == shift:
            p = p + 3e-5
        write_obj(os.path.join(folder, f"piece_{n}.obj"), p, f)
    P = len(cells)
    g = [[False] * P for _ in range(P)]
    for i, j in itertools.combinations(range(P), 2):
        if max(abs(a - b) for a, b in zip(cells[i], cells[j])) == 1 and shift not in (i, j):
            g[i][j] = g[j][i] = True
    order = sorted(range(P), key=lambda n: f"piece_{n}.obj")       # the loaders' part order: sorted file names
    return [[g[a][b] for b in order] for a in order]


def tetra(apex, base_shift):
    b = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.3, 0.0]]) + base_shift
    return np.vstack([b, apex]), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])


def rounding_puzzles(root, truth):
    """hand-placed tetrahedra: shared apexes at 5-decimal midpoints and one ulp around them, and at +0 / -0"""
    mids = [0.000125, 1.234565]
    parts = []
    for k, m in enumerate(mids):
        for m2 in (m, np.nextafter(m, np.inf), np.nextafter(m, -np.inf)):
            parts.append(((m, 1.0 + k, 2.0), (m2, 1.0 + k, 2.0)))
    folder = os.path.join(root, "everyday/Mug/obj002/fractured_0")
    n = 0
    for a, b in parts:
        for apex, sh in ((a, -1.0), (b, 1.0)):
            v, f = tetra(np.array(apex), np.array([sh * (1 + 0.4 * n), 1.2 * n, 0.0]))     # the puzzle spans < 20.97 units
            write_obj(os.path.join(folder, f"piece_{n:02d}.obj"), v, f)
            n += 1
    truth[os.path.relpath(folder, root)] = None          # no grid truth: the set restatement decides
    folder = os.path.join(root, "everyday/Mug/obj002/fractured_1")
    for n, z in enumerate((0.0, -0.0, 0.0)):
        v, f = tetra(np.array([z, -0.0 if n == 1 else 0.0, 3.0]), np.array([2.0 * n - 2.0, 4.0 * n + 1.0, -1.0]))
        write_obj(os.path.join(folder, f"piece_{n}.obj"), v, f)
    truth[os.path.relpath(folder, root)] = [[False, True, True], [True, False, True], [True, True, False]]


def small_tree(root):
    truth = {}
    R, t = rotation(7), np.array([0.25, -0.5, 0.125])
    big = lambda n: [6] + [2] * (n - 1)                      # noqa: E731 — the first cell 3x the others (lattice 0.25)
    h = 0.25

    def grid(rel, dims, shift=None):
        folder = os.path.join(root, rel)
        truth[rel] = grid_puzzle(folder, dims, [big(d) for d in dims], h, R, t, shift)

    grid("everyday/BeerBottle/obj000/fractured_0", (2, 1, 1))
    grid("everyday/BeerBottle/obj000/fractured_1", (2, 2, 1))
    grid("everyday/BeerBottle/obj000/mode_0", (3, 2, 1))
    grid("everyday/BeerBottle/obj000/pieces_extra", (2, 1, 1))          # neither "fractured" nor "mode": ignored
    grid("everyday/Bowl/obj001/fractured_0", (1, 1, 1))                 # 1 part: filtered by min_num_part
    grid("everyday/Bowl/obj001/fractured_1", (7, 3, 1))                 # 21 parts: filtered by max_num_part
    grid("everyday/Bowl/obj001/fractured_2", (2, 2, 2), shift=5)        # one cell shifted by 3e-5
    grid("everyday/Bowl/obj001/mode_1", (3, 1, 2))
    rounding_puzzles(root, truth)
    with open(os.path.join(root, "everyday.train.txt"), "w") as fh:
        fh.write("everyday/BeerBottle/obj000\neveryday/Missing/obj999\neveryday/Bowl/obj001\n")
    with open(os.path.join(root, "everyday.val.txt"), "w") as fh:
        fh.write("everyday/Mug/obj002\neveryday/BeerBottle/obj000\n")
    return truth


def bench_tree(root, n):
    truth = {}
    h = 1.0 / 16
    objs = []
    for k in range(n):
        R, t = rotation(100 + k), np.array([0.1 * k, -0.2, 0.3])
        rel = f"everyday/Bench/obj{k:03d}/fractured_0"
        widths = [[24, 16, 16, 16, 16], [16, 16], [16, 16]]       # 5 x 2 x 2 = 20 parts, 1.5k-5k faces each
        truth[rel] = grid_puzzle(os.path.join(root, rel), (5, 2, 2), widths, h, R, t)
        objs.append(os.path.dirname(rel))
    for split in ("train", "val"):
        with open(os.path.join(root, f"everyday.{split}.txt"), "w") as fh:
            fh.write("\n".join(objs if split == "train" else objs[:1]) + "\n")
    return truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--bench", type=int, default=0, help="write N bench puzzles (20 parts) instead of the small tree")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    truth = bench_tree(a.out, a.bench) if a.bench else small_tree(a.out)
    with open(os.path.join(a.out, "truth.json"), "w") as fh:
        json.dump(truth, fh)


if __name__ == "__main__":
    main()
