"""The test split's initial frames (pfpp_test_frames, pfpp_hip.augment.test_frames_batch): a float64 numpy restatement of the by-area
transform, written from the formulas of include/pfpp.h and the reference's dataset.py:86-109 (not from the kernel), and the hand-built
puzzles the GPU tests run.

    a = R(q_global)^T x - c_ref;   c = a - (double)(float) t[p];   y = R(q_part[p])^T c,  stored as float32

with R(q) the rotation of the scalar-first quaternion q / |q| (scipy normalises, the kernel's two_s does)."""
import numpy as np


def rot_t(q) -> np.ndarray:
    """R(q)^T in float64 for a scalar-first quaternion that need not be unit"""
    r, i, j, k = (float(v) for v in np.asarray(q, dtype=np.float64))
    s = 2.0 / (r * r + i * i + j * j + k * k)
    R = np.array([[1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)],
                  [s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r)],
                  [s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)]], dtype=np.float64)
    return R.T


def apply(M: np.ndarray, x: np.ndarray) -> np.ndarray:
    """rows of x times M, every product and sum written out in float64 (no BLAS: the order is this line's)"""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([M[r, 0] * x[:, 0] + M[r, 1] * x[:, 1] + M[r, 2] * x[:, 2] for r in range(3)], axis=1)


def by_area_frames(x, n_pcs, num_parts: int, q_global, c_ref, trans, q_part) -> np.ndarray:
    """by-area points x [M, 3] of the assembled shape -> every piece's initial frame, float32 [M, 3].  c_ref float64 [3] (init_pose_t),
    trans [P, 3] (part_trans: rounded to float32 before use, as the host subtracts its float32 cur_trans), q_global [4], q_part [P, 4]"""
    a = apply(rot_t(q_global), x) - np.asarray(c_ref, dtype=np.float64)
    out = np.zeros((len(a), 3), dtype=np.float32)
    off = 0
    for p in range(int(num_parts)):
        n = int(n_pcs[p])
        c = a[off:off + n] - np.asarray(trans[p]).astype(np.float32).astype(np.float64)
        out[off:off + n] = apply(rot_t(q_part[p]), c).astype(np.float32)
        off += n
    return out


def frame_shifts(part_pcs_gt, num_parts: int, ref: int, q_global):
    """-> (c_ref float64 [3], t float64 [P, 3]): the reference part's centroid after the global rotation and every valid part's
    centroid relative to it, from float64 means of the stored fragments"""
    gt = np.asarray(part_pcs_gt, dtype=np.float64)
    Rg = rot_t(q_global)
    cent = apply(Rg, gt.mean(axis=1))
    t = np.zeros((gt.shape[0], 3))
    t[:num_parts] = cent[:num_parts] - cent[ref]
    return cent[ref], t


def restate(puzzle: dict) -> np.ndarray:
    """the by-area output of a hand-built puzzle from its float32 inputs"""
    c_ref, t = frame_shifts(puzzle["part_pcs_gt"], puzzle["num_parts"], puzzle["ref"], puzzle["q_global"])
    return by_area_frames(puzzle["by_area"], puzzle["n_pcs"], puzzle["num_parts"], puzzle["q_global"], c_ref, t, puzzle["q_part"])


# ---- the hand-built puzzles: (name, num_parts, by-area counts per slot, reference slot), all of P = 5 slots
P_HAND = 5
HAND = {
    "A": (2, (1, 257, 0, 0, 0), 1),               # 2 pieces of 1 and 257 points; the reference piece is slot 1, not slot 0
    "B": (5, (255, 256, 1, 30, 300), 3),          # piece boundaries on and beside a 256-thread boundary; 842 is no multiple of 256
    "C": (3, (40, 0, 7, 0, 0), 0),                # a valid piece without a by-area point
}


def hand_puzzle(name: str, N: int) -> dict:
    """float32 inputs of one hand-built puzzle with N points per fragment; non-unit quaternions (|q| between 0.5 and 1.6), padded
    fragments zero, coordinates after the transform below 2"""
    pv, counts, ref = HAND[name]
    rng = np.random.default_rng([ord(name), N])
    gt = np.zeros((P_HAND, N, 3), dtype=np.float32)
    centres = rng.normal(0, 0.35, size=(pv, 1, 3))
    gt[:pv] = (centres + rng.normal(0, 0.15, size=(pv, N, 3))).astype(np.float32)
    pts = [centres[p] + rng.normal(0, 0.15, size=(counts[p], 3)) for p in range(pv)]
    q = rng.normal(size=(1 + P_HAND, 4))
    q *= rng.uniform(0.5, 1.6, size=(1 + P_HAND, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    ref_part = np.zeros(P_HAND, dtype=bool)
    ref_part[ref] = True
    return {"name": name, "num_parts": pv, "ref": ref, "ref_part": ref_part, "n_pcs": np.asarray(counts, dtype=np.int64),
            "part_pcs_gt": gt, "by_area": np.concatenate(pts).astype(np.float32), "q_global": q[0].astype(np.float32),
            "q_part": q[1:].astype(np.float32)}


def pack(puzzles) -> dict:
    """the operands of one pfpp_test_frames call (numpy, in the entry's dtypes: float64 quaternions are rounded to float32) for a
    list of puzzles in hand_puzzle's layout"""
    lens = [len(p["by_area"]) for p in puzzles]
    f32 = lambda key, join: join([p[key] for p in puzzles]).astype(np.float32)
    return {"part_pcs_gt": f32("part_pcs_gt", np.stack), "num_parts": np.array([p["num_parts"] for p in puzzles], dtype=np.int32),
            "ref_idx": np.array([p["ref"] for p in puzzles], dtype=np.int32), "q_global": f32("q_global", np.stack),
            "q_part": f32("q_part", np.stack), "by_area": f32("by_area", np.concatenate),
            "pt_off": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), "n_pcs": np.stack([p["n_pcs"] for p in puzzles]).astype(np.int32)}


def golden_item(g: dict, i: int) -> dict:
    """test item i of tests/golden/dataset.npz (what the reference's own __getitem__ took and returned) in hand_puzzle's layout, the
    recorded float64 rotations kept as they are"""
    k = f"test{i}_"
    q = g[k + "drawn_quats_f64"]
    P = g[k + "part_pcs_gt"].shape[0]
    qp = np.zeros((P, 4))
    qp[:, 0] = 1.0
    qp[:len(q) - 1] = q[1:]
    return {"name": k, "num_parts": int(g[k + "num_parts"]), "ref": int(np.argmax(g[k + "ref_part"])), "ref_part": g[k + "ref_part"],
            "n_pcs": g[k + "n_pcs"], "part_pcs_gt": g[k + "part_pcs_gt"], "by_area": g[k + "gt_pc_by_area"], "q_global": q[0], "q_part": qp,
            "want": {n: g[k + n] for n in ("part_pcs_by_area", "part_rots", "part_trans", "init_pose_t", "init_pose_r")}}
