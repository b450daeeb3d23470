"""float64 numpy restatement of csrc/matching_dataset.hip in the kernels' own order (piece counts, ragged surface samples, centroid,
rotation, Marsaglia quaternions), the shared fixtures of tests/test_matching_dataset_host.py and tests/test_gpu_matching_dataset.py,
and the conditions both files apply.  Nothing here needs a GPU."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
SETTINGS = ((251, 20), (997, 30))
SPLIT_FILES = {"train": "everyday.train.txt", "val": "everyday.val.txt"}
ROT_SEED = 0xA5B85C5E198ED849
MAX_PARTS = 20


def make_tree(path) -> Path:
    subprocess.run([sys.executable, str(ROOT / "tools" / "make_synthetic_meshes.py"), str(path)], check=True, capture_output=True)
    return Path(path)


def folder_meshes(tree, rel):
    from pfpp_hip.meshes import read_obj

    d = Path(tree) / rel
    return [read_obj(str(d / f)) for f in sorted(os.listdir(d))]


def face_areas(v, f):
    t = v[f]
    u, w = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    c0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    c1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    c2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return np.sqrt((c0 * c0 + c1 * c1) + c2 * c2) / 2.0


# ------------------------------------------------------------------------------------------------------------------- piece counts
def np_sum_order(a) -> float:
    """np.sum of 1..128 float64 values, addition by addition (numpy's pairwise_sum below its block size)"""
    a = [np.float64(x) for x in a]
    n = len(a)
    if n < 8:
        tot = np.float64(0.0)
        for x in a:
            tot = tot + x
        return tot
    r = a[:8]
    i = 8
    while i < n - n % 8:
        r = [r[j] + a[i + j] for j in range(8)]
        i += 8
    tot = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        tot = tot + a[i]
        i += 1
    return tot


def piece_counts(areas, num_points: int, min_part_point: int) -> np.ndarray:
    """sample_reweighted_points_by_areas (:164-193) in fp64 and int32, as piece_counts_kernel does it"""
    areas = np.asarray(areas, dtype=np.float64)
    P = len(areas)
    if P * max(min_part_point, 1) > num_points:
        raise ValueError("infeasible: parts x min_part_point > num_points")
    tot = np_sum_order(areas)
    nps = np.array([np.int32(np.ceil(a * np.float64(num_points) / tot)) for a in areas], dtype=np.int32)
    nps[int(np.argmax(nps))] -= np.int32(int(nps.astype(np.int64).sum()) - num_points)
    if min_part_point > 1:
        delta = 0
        for k in range(P):
            if nps[k] < min_part_point:
                delta += min_part_point - int(nps[k])
                nps[k] = min_part_point
        while delta > 0:
            k = int(np.argmax(nps))
            if nps[k] - delta >= min_part_point:
                nps[k] -= delta
                delta = 0
            else:
                delta -= int(nps[k]) - min_part_point
                nps[k] = min_part_point
    return nps.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------- generators
def uniform53(seed: int, split: int, idx) -> np.ndarray:
    """(pfpp_rng_u64(seed, split, idx) >> 11) 2^-53 (csrc/pfpp_common.h)"""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.full(idx.shape, np.uint64(seed) ^ (np.uint64(split) * np.uint64(0xD6E8FEB86659FD93)), dtype=np.uint64)
        z = z + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def sample_uniforms(seed, split, data_id, slot, n, num_points, max_parts=MAX_PARTS) -> np.ndarray:
    """the generated (u0, l0, l1) of samples 0 .. n - 1 of a piece: key ((data_id max_parts + slot) num_points + s) 3 + k"""
    with np.errstate(over="ignore"):
        key = ((np.uint64(data_id) * np.uint64(max_parts) + np.uint64(slot)) * np.uint64(num_points)
               + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(3) + np.arange(3, dtype=np.uint64)[None]
    return uniform53(seed, split, key)


def quat_matrix(q) -> np.ndarray:
    w, x, y, z = (np.float64(c) for c in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def marsaglia_quat(seed, split, data_id, slot, max_parts=MAX_PARTS, attempts=64):
    """-> (q float64 [4] = (w, x, y, z), attempts used); the identity when a pair finds no attempt inside the disc"""
    base = (data_id * max_parts + slot) * attempts
    u = 2.0 * uniform53(seed ^ ROT_SEED, split, (np.uint64(base) + np.arange(attempts, dtype=np.uint64))[:, None] * np.uint64(4)
                        + np.arange(4, dtype=np.uint64)[None]) - 1.0
    s1 = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]
    s2 = u[:, 2] * u[:, 2] + u[:, 3] * u[:, 3]
    ok1, ok2 = s1 < 1.0, (s2 > 0.0) & (s2 < 1.0)
    if not ok1.any() or not ok2.any():
        return np.array([1.0, 0.0, 0.0, 0.0]), attempts
    a, b = int(np.argmax(ok1)), int(np.argmax(ok2))
    f = np.sqrt((1.0 - s1[a]) / s2[b])
    return np.array([u[a, 0], u[a, 1], u[b, 2] * f, u[b, 3] * f]), max(a, b) + 1


# ------------------------------------------------------------------------------------------------------------------- one item
def sample_part(v, f, cdf, total, u):
    """sample_point of csrc/mesh_common.h for the rows of u [n, 3] -> (points float64 [n, 3], face [n])"""
    face = np.minimum(np.searchsorted(cdf, u[:, 0] * total, side="left"), len(f) - 1)
    l = u[:, 1:3].copy()
    fold = l[:, 0] + l[:, 1] > 1.0
    l[fold] = l[fold] - 1.0
    l = np.abs(l)
    a = v[f[face, 0]]
    return ((v[f[face, 1]] - a) * l[:, :1] + (v[f[face, 2]] - a) * l[:, 1:2]) + a, face


def centroid(pc) -> np.ndarray:
    """np.mean(pc, axis = 0) addition by addition: the rows in row order, one division"""
    acc = pc[0].copy()
    for i in range(1, len(pc)):
        acc = acc + pc[i]
    return acc / np.float64(len(pc))


def rotate32(pc, R) -> np.ndarray:
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    return np.stack([(R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z for k in range(3)], axis=1).astype(np.float32)


def item(parts, areas, data_id, num_points, min_part_point, *, cdfs=None, totals=None, seed=0, split=0, uniforms=None, order=None,
         rot=None, max_parts=MAX_PARTS):
    """one puzzle as the three kernels compute it.  parts: [(verts, faces)] in slot order; areas: what the counts take (the store's
    total); cdfs / totals: the parts' cdf and total (np.cumsum of the face areas when not given); uniforms [N, 3] and order [N]
    piece after piece, rot [P, 3, 3]: the given tables, else the generated mode."""
    from pfpp_hip.matching_dataset import quat_from_matrix

    P = len(parts)
    nps = piece_counts(areas, num_points, min_part_point)
    out = {"n_pcs": np.zeros(max_parts, dtype=np.int64), "part_valids": (np.arange(max_parts) < P).astype(np.float32),
           "part_quat": np.zeros((max_parts, 4), dtype=np.float32), "part_trans": np.zeros((max_parts, 3), dtype=np.float32),
           "rot": np.zeros((max_parts, 3, 3))}
    out["n_pcs"][:P] = nps
    pts, gts, pcs, faces, o = [], [], [], [], 0
    for k, (v, f) in enumerate(parts):
        n = int(nps[k])
        cdf = np.cumsum(face_areas(v, f)) if cdfs is None else cdfs[k]
        total = cdf[-1] if totals is None else totals[k]
        u = uniforms[o:o + n] if uniforms is not None else sample_uniforms(seed, split, data_id, k, n, num_points, max_parts)
        p, face = sample_part(v, f, cdf, total, u)
        od = np.asarray(order[o:o + n], dtype=np.int64) if order is not None else np.arange(n)
        if rot is not None:
            R = np.asarray(rot[k], dtype=np.float64)
            q = quat_from_matrix(R.T)
        else:
            w = marsaglia_quat(seed, split, data_id, k, max_parts)[0]
            R = quat_matrix(w)
            q = np.array([w[0], -w[1], -w[2], -w[3]])
        c = centroid(p)
        out["part_trans"][k], out["part_quat"][k], out["rot"][k] = c.astype(np.float32), q.astype(np.float32), R
        pts.append(p)
        gts.append(p[od].astype(np.float32))
        pcs.append(rotate32(p - c[None], R)[od])
        faces.append(face[od].astype(np.int32))
        o += n
    out.update(points=np.concatenate(pts), gt_pcs=np.concatenate(gts), part_pcs=np.concatenate(pcs), face_idx=np.concatenate(faces))
    return out


# ------------------------------------------------------------------------------------------------------------------- conditions
def ulp_mismatch(a, b):
    """float32 arrays -> (number of elements that differ, the largest difference in float32 ulps)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    return int((d != 0).sum()), int(d.max(initial=0))


def assert_blas_rounding(got, want, what=""):
    """part_pcs against the reference's BLAS product: at most 0.1 % of the elements may differ, each by one float32 ulp"""
    n, worst = ulp_mismatch(got, want)
    print(f"{what}: {n} of {np.asarray(got).size} elements differ, worst {worst} ulp")
    assert worst <= 1 and n <= 0.001 * np.asarray(got).size, (what, n, worst)


def golden_items(gold, num_points):
    """-> [(split, index, prefix)] of every item of one setting"""
    return [(split, i, f"n{num_points}_{split}_{i}_") for split in ("train", "val") for i in range(len(gold[f"{split}_data_list"]))]
