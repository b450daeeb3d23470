"""Evaluating the matcher on the GPU: piece-pair poses by RANSAC and the ragged nearest distance (csrc/matching_pose.hip,
include/pfpp.h "matcher, evaluation").

The reference's test pass (Jigsaw_matching/model/modules/matching_base_model.py:298-359) hands every piece pair with at least three
matched critical points to open3d's correspondence RANSAC on the host (utils/estimate_transform.py:8-66: three-point poses, 50,000
draws at most, 0.05 inlier distance), one pair at a time.  Here:

* ransac_pairs: all hypotheses of all pairs of a batch in one launch.  The procedure is fixed: counter-based draws
  (Philox4x32-10), every hypothesis scored, no early stop; tests/matching_pose_cases.py restates it in float64 numpy.
* nn_dist_ragged: ops.nn_dist over segments of unequal sizes, bit for bit its arithmetic: the per-part and whole-shape chamfer terms
  of utils/eval_utils.py without padding the pieces to one size.
* pose_graph, translation_edges: the reference's pose graph of every puzzle of a batch (:285-434), its RANSAC edges from ONE
  ransac_pairs call, its translation-only edges as written.
* connect_graph, minimum_spanning_tree, spanning_tree_alignment, global_alignment: utils/global_alignment/ (the spanning-tree
  method) in numpy and plain Python, with networkx's order rules restated; pinned to the reference's files by a golden.
* anchor_poses, MatchingEvaluator: the pivot anchoring (:431-453) and calc_metric (:144-218): part_acc, chamfer_distance,
  trans_{mse,rmse,mae}, rot_{mse,rmse,mae}, pred_dict, stats.  python -m pfpp_hip.evaluate_matching runs it over a directory.

Argument errors are raised before any launch."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .matching import _gpu, _p

TILE = 1024              # PFPP_RANSAC_TILE: correspondences the scoring kernel stages per step
MAX_PAIRS = 65535        # pairs (and ragged segments) per launch
STATUS_OK = 1            # bit 0 of a pair's status: a non-degenerate hypothesis won
STATUS_REFINED = 2       # bit 1: the pose is Horn's over the winner's inliers


def _host_int(x, name: str) -> np.ndarray:
    a = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name}: expected integers, got {a.dtype}")
    return a.astype(np.int64)


def ransac_pairs(pts: torch.Tensor, pairs, corr: Sequence, *, n_hyp: int = 50000, max_dist: float = 0.05, seed: int = 0, refine: bool = False,
                 return_counts: bool = False) -> dict:
    """pts float32 [R, 3] on the GPU; pairs int [E, 2] (host): the first rows of every pair's source and target piece in pts; corr:
    one int [M_e, 2] array per pair (host), M_e >= 3: correspondence k matches pts[pairs[e, 0] + corr[e][k, 0]] to pts[pairs[e, 1] +
    corr[e][k, 1]].  n_hyp hypotheses per pair (the reference's 50,000), max_dist the inlier distance, seed a 64-bit integer.
    -> R float32 [E, 3, 3], t float32 [E, 3] (the pose maps source to target), best_h int32 [E], count int32 [E], sumsq float64 [E]
    (of the winning three-point pose), status int32 [E] (STATUS_OK | STATUS_REFINED; 0: every hypothesis was degenerate - R = 1, t =
    the difference of the matched points' centroids, best_h = count = -1), n_refined float64 [E] (the inliers the refinement used);
    with return_counts also counts int32 [E, n_hyp] (-1 = degenerate).  refine=True replaces the winner's pose by Horn's over its
    inliers."""
    if not isinstance(pts, torch.Tensor):
        raise TypeError("pts: expected a torch.Tensor")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"pts: expected [R, 3], got {tuple(pts.shape)}")
    R = int(pts.shape[0])
    pairs_h = _host_int(pairs, "pairs")
    if pairs_h.size % 2:
        raise ValueError(f"pairs: expected [E, 2], got {tuple(pairs_h.shape)}")
    pairs_h = pairs_h.reshape(-1, 2)
    E = pairs_h.shape[0]
    corr = list(corr)
    if len(corr) != E:
        raise ValueError(f"ransac_pairs: {E} pairs but {len(corr)} correspondence lists")
    if E > MAX_PAIRS:
        raise ValueError(f"ransac_pairs: {E} pairs in one call, at most {MAX_PAIRS}")
    n_hyp = int(n_hyp)
    if not 1 <= n_hyp <= 0x7fffff00:
        raise ValueError(f"n_hyp: {n_hyp} is outside [1, 2^31 - 256]")
    if not (float(max_dist) > 0.0 and np.isfinite(max_dist)):
        raise ValueError(f"max_dist: {max_dist} must be positive and finite")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed: expected an unsigned 64-bit integer")
    lists = []
    for e, c in enumerate(corr):
        c = _host_int(c, f"corr[{e}]")
        if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 3:
            raise ValueError(f"corr[{e}]: expected [M, 2] with M >= 3 (a pose needs three correspondences), got {tuple(c.shape)}")
        rows = c + pairs_h[e][None, :]
        if rows.min() < 0 or rows.max() >= R or c.min() < 0:
            raise ValueError(f"corr[{e}]: a correspondence points outside pts ({R} rows)")
        lists.append(c)
    _gpu(pts, torch.float32, "pts")
    dev = pts.device
    out = {"R": torch.zeros((E, 3, 3), dtype=torch.float32, device=dev), "t": torch.zeros((E, 3), dtype=torch.float32, device=dev)}
    info = torch.zeros((E, 3), dtype=torch.int32, device=dev)
    stats = torch.zeros((E, 2), dtype=torch.float64, device=dev)
    counts = torch.empty((E, n_hyp), dtype=torch.int32, device=dev) if return_counts else None
    if E:
        corr_off = np.concatenate([[0], np.cumsum([c.shape[0] for c in lists])]).astype(np.int64)
        corr_d = torch.from_numpy(np.ascontiguousarray(np.concatenate(lists).astype(np.int32))).to(dev)
        off_d = torch.from_numpy(corr_off).to(dev)
        pairs_d = torch.from_numpy(np.ascontiguousarray(pairs_h)).to(dev)
        lib = _lib.load()
        ws_bytes = int(lib.pfpp_ransac_pairs_workspace(E, n_hyp))
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=dev)
        check(lib.pfpp_ransac_pairs(_p(pts.contiguous()), R, E, _p(pairs_d), _p(corr_d), _p(off_d), n_hyp, float(max_dist), seed, int(bool(refine)),
                                    _p(out["R"]), _p(out["t"]), _p(stats), _p(info), _p(counts), _p(ws), ws.numel() * 8, ops._stream()),
              "pfpp_ransac_pairs")
    out.update(best_h=info[:, 0], count=info[:, 1], status=info[:, 2], sumsq=stats[:, 0], n_refined=stats[:, 1])
    if return_counts:
        out["counts"] = counts
    return out


def nn_dist_ragged(src: torch.Tensor, src_off, dst: torch.Tensor, dst_off) -> torch.Tensor:
    """src float32 [Ns, 3], dst float32 [Nd, 3] on the GPU; src_off, dst_off int [S + 1] (host): segment s owns src[src_off[s] :
    src_off[s + 1]] and dst[dst_off[s] : dst_off[s + 1]].  -> float32 [Ns]: out[i] = min_j |src_i - dst_j|^2 over the segment's own
    targets, in ops.nn_dist's arithmetic (inf where the segment has no target).  Rows of src outside every segment are left 0."""
    if not (isinstance(src, torch.Tensor) and isinstance(dst, torch.Tensor)):
        raise TypeError("nn_dist_ragged: src and dst must be torch.Tensors")
    if src.dim() != 2 or src.shape[1] != 3 or dst.dim() != 2 or dst.shape[1] != 3:
        raise ValueError("nn_dist_ragged: src [Ns, 3] and dst [Nd, 3] expected")
    so, do = _host_int(src_off, "src_off").reshape(-1), _host_int(dst_off, "dst_off").reshape(-1)
    if so.size < 1 or so.shape != do.shape:
        raise ValueError("nn_dist_ragged: src_off and dst_off need one entry per segment plus one")
    for off, n, name in ((so, src.shape[0], "src_off"), (do, dst.shape[0], "dst_off")):
        if off[0] < 0 or off[-1] > n or (np.diff(off) < 0).any():
            raise ValueError(f"{name}: offsets must be non-decreasing and within the {n} rows")
    S = so.size - 1
    if S > MAX_PAIRS:
        raise ValueError(f"nn_dist_ragged: {S} segments in one call, at most {MAX_PAIRS}")
    _gpu(src, torch.float32, "src")
    _gpu(dst, torch.float32, "dst")
    out = torch.zeros(src.shape[0], dtype=torch.float32, device=src.device)
    max_n = int(np.diff(so).max(initial=0))
    if S and max_n:
        so_d, do_d = torch.from_numpy(so).to(src.device), torch.from_numpy(do).to(src.device)
        check(_lib.load().pfpp_nn_dist_ragged(_p(src.contiguous()), _p(so_d), _p(dst.contiguous()), _p(do_d), _p(out), S, max_n, ops._stream()),
              "pfpp_nn_dist_ragged")
    return out


# ------------------------------------------------------------------------------------------------------------------ global alignment
def connect_graph(v_num: int, edges: np.ndarray) -> np.ndarray:
    """pose_graph_utils.py:5-20: one auxiliary edge (hub = v_num, vertex) per connected component, the components in the order of
    their sizes (largest first; equal sizes in the order of their smallest vertex).  The vertex is the component's SMALLEST: the
    reference takes `list(component)[0]` of a Python set, whose order follows CPython's hash table (deviations)"""
    label = np.arange(v_num)
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2):
        la, lb = label[a], label[b]
        if la != lb:
            label[label == max(la, lb)] = min(la, lb)                  # a component is named by its smallest vertex
    roots = np.unique(label)
    sizes = np.array([(label == r).sum() for r in roots])
    order = np.argsort(-sizes, kind="stable")
    return np.stack([np.array([v_num, roots[k]]) for k in order]).astype(np.int64)


def minimum_spanning_tree(v_num: int, edges: np.ndarray, weights: np.ndarray):
    """pose_graph_utils.py:23-31 without networkx, with its order rules: the graph's edge list runs over the vertices in index
    order and, per vertex, over its neighbours in the order their edges first appeared (an edge given twice keeps its place and takes
    the later weight); Kruskal takes that list sorted by weight, stably, so equal weights keep it; the tree's adjacency lists are in
    the order Kruskal accepted the edges; the depth-first search from vertex 0 follows them
    -> (the vertices in preorder, {vertex: its predecessor})"""
    adj = [dict() for _ in range(v_num)]
    for (a, b), w in zip(np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist(), np.asarray(weights, dtype=np.float64).tolist()):
        adj[a][b] = w
        adj[b][a] = w
    listed, done = [], set()
    for a in range(v_num):
        for b, w in adj[a].items():
            if b not in done:
                listed.append((w, a, b))
        done.add(a)
    listed.sort(key=lambda x: x[0])                                    # stable
    parent = list(range(v_num))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tree = [[] for _ in range(v_num)]
    for w, a, b in listed:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            if b not in tree[a]:
                tree[a].append(b)
            if a not in tree[b]:
                tree[b].append(a)
    order, pred, seen = [0], {}, {0}
    stack = [(0, iter(tree[0]))]
    while stack:
        v, it = stack[-1]
        for c in it:
            if c not in seen:
                seen.add(c)
                order.append(c)
                pred[c] = v
                stack.append((c, iter(tree[c])))
                break
        else:
            stack.pop()
    return order, pred


def spanning_tree_alignment(v_num: int, edges: np.ndarray, transformations: np.ndarray, uncertainty: np.ndarray) -> np.ndarray:
    """spanning_tree_alignment.py:6-22: global poses [v_num, 4, 4] along the minimum spanning tree from vertex 0 (the identity);
    transformations[i] belongs to the directed edge (edges[i, 0], edges[i, 1]), its inverse to the reversed one; a pair of vertices
    given twice keeps the later transformation.  Every vertex must be reachable from vertex 0"""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    order, pred = minimum_spanning_tree(v_num, edges, uncertainty)
    if len(order) != v_num:
        raise ValueError("spanning_tree_alignment: the graph is not connected (global_alignment adds the hub vertex)")
    between = {}
    for (a, b), T in zip(edges.tolist(), np.asarray(transformations, dtype=np.float64)):
        between[(a, b)] = T
        between[(b, a)] = np.linalg.inv(T)
    out = np.zeros((v_num, 4, 4))
    out[0] = np.eye(4)
    for y in order[1:]:
        x = pred[y]
        out[y] = out[x] @ between[(x, y)]
    return out


def global_alignment(v_num: int, edges: np.ndarray, transformations: np.ndarray, uncertainty: np.ndarray) -> np.ndarray:
    """global_alignment/__init__.py:9-47 with method='spanning_tree' (never Shonan averaging): a hub vertex joined to one vertex of
    every component by an edge of uncertainty 1 whose transformation is the identity (the reference's commented-out line 25; its
    line 21-22 draws them at random), the spanning-tree poses, re-referenced to vertex 0 -> [v_num, 4, 4]"""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    aux = connect_graph(v_num, edges)
    all_edges = np.concatenate([edges, aux])
    all_T = np.concatenate([np.asarray(transformations, dtype=np.float64).reshape(-1, 4, 4), np.repeat(np.eye(4)[None], len(aux), 0)])
    all_u = np.concatenate([np.asarray(uncertainty, dtype=np.float64).reshape(-1), np.ones(len(aux))])
    poses = spanning_tree_alignment(v_num + 1, all_edges, all_T, all_u)
    for i in range(v_num):
        poses[v_num - i - 1] = np.linalg.inv(poses[0]) @ poses[v_num - i - 1]
    return poses[:v_num]


# ------------------------------------------------------------------------------------------------------------------ the pose graph
def _assignment(perm):
    perm = np.asarray(perm.detach().cpu().numpy() if torch.is_tensor(perm) else perm)
    if perm.ndim == 2:
        return np.nonzero(perm)
    rows = np.nonzero(perm >= 0)[0]
    return rows, perm[rows].astype(np.int64)


def translation_edges(perm, n_critical_pcs, critical_pcs_idx, part_pcs, n_pcs, n_valid: int, connections: np.ndarray):
    """matching_base_model.py:372-429, as written: the pieces that no RANSAC edge reaches are tied to a connected piece by a
    translation-only edge of uncertainty 1.  part_pcs float [N, 3] (host) of one puzzle; connections float [n_valid]: edges per
    piece so far, updated in place -> (edges [(idx2, idx1)], transformations [4, 4])"""
    rows, cols = _assignment(perm)
    nc, npc = np.asarray(n_critical_pcs, dtype=np.int64).reshape(-1), np.asarray(n_pcs, dtype=np.int64).reshape(-1)
    cri0, pc0 = np.cumsum(nc) - nc, np.cumsum(npc) - npc
    piece = np.repeat(np.arange(nc.size), nc)
    pr, pc = piece[rows], piece[cols]
    crit = np.asarray(critical_pcs_idx, dtype=np.int64).reshape(-1)
    pts = np.asarray(part_pcs, dtype=np.float64)
    edges, mats = [], []
    for idx1 in range(n_valid):
        for idx2 in range(idx1 + 1, n_valid):
            if (connections[idx1] > 0) == (connections[idx2] > 0):
                continue
            n1, n2 = int(nc[idx1]), int(nc[idx2])
            pc1, pc2 = pts[pc0[idx1]:pc0[idx1] + npc[idx1]], pts[pc0[idx2]:pc0[idx2] + npc[idx2]]
            T = np.eye(4)
            if n1 == 0 or n2 == 0:
                if n2 > 0:                                             # :398: the INDEX of the first critical point, not the point
                    T[:3, 3] = float(crit[pc0[idx2]]) - pc1.sum(0)
                elif n1 > 0:
                    T[:3, 3] = pc2.sum(0) - pc1[crit[pc0[idx1]]]
                else:
                    T[:3, 3] = pc2.sum(0) - pc1.sum(0)
            else:
                fwd, bwd = (pr == idx1) & (pc == idx2), (pr == idx2) & (pc == idx1)
                if fwd.sum() < bwd.sum():                              # the transposed opposite block (ties keep the first)
                    m1, m2 = cols[bwd] - cri0[idx1], rows[bwd] - cri0[idx2]
                else:
                    m1, m2 = rows[fwd] - cri0[idx1], cols[fwd] - cri0[idx2]
                src = pc1[crit[pc0[idx1]:pc0[idx1] + n1]]
                tgt = pc2[crit[pc0[idx2]:pc0[idx2] + n2]]
                T[:3, 3] = tgt[m2].sum(0) - src[m1].sum(0)
            edges.append([idx2, idx1])
            mats.append(T)
            connections[idx1] += 1
            connections[idx2] += 1
    return edges, mats


def pose_graph(perm, n_critical_pcs, critical_pcs_idx, part_pcs, n_pcs, n_valid, **ransac) -> list:
    """the pose graphs of a batch (matching_base_model.py:285-434).  perm: per puzzle the assignment (pfpp_hip.matching.match_edges'
    forms); n_critical_pcs, n_pcs int [B, P]; critical_pcs_idx int [B, N] (piece-local indices, the first n_critical of every piece's
    slots); part_pcs float32 [B, N, 3] on the GPU; n_valid int [B]; **ransac goes to ransac_pairs (n_hyp, max_dist, seed, refine).
    The RANSAC edges of ALL puzzles are one ransac_pairs call; their uncertainty is 1 / (matches of the pair)
    -> per puzzle a dict: edges int64 [E, 2] = (idx2, idx1), transformations [E, 4, 4], uncertainty [E], n_ransac (the first
    n_ransac edges are RANSAC's), ransac (ransac_pairs' outputs for them, host arrays)"""
    from .matching import match_edges

    _gpu(part_pcs, torch.float32, "part_pcs")
    if part_pcs.dim() != 3 or part_pcs.shape[2] != 3:
        raise ValueError(f"part_pcs: expected [B, N, 3], got {tuple(part_pcs.shape)}")
    B, N = part_pcs.shape[:2]
    nc_all, np_all = _host_int(n_critical_pcs, "n_critical_pcs").reshape(B, -1), _host_int(n_pcs, "n_pcs").reshape(B, -1)
    crit_all = _host_int(critical_pcs_idx, "critical_pcs_idx").reshape(B, -1)
    nv = _host_int(n_valid, "n_valid").reshape(-1)
    if len(perm) != B or nv.size != B or crit_all.shape[1] != N or (np_all.sum(1) > N).any():
        raise ValueError("pose_graph: one assignment, n_valid and N critical_pcs_idx slots per puzzle, n_pcs within the N points")
    per, pairs, corr = [], [], []
    for b in range(B):
        edges, cs = match_edges(perm[b], nc_all[b], int(nv[b]))
        pc0 = np.cumsum(np_all[b]) - np_all[b]
        for (idx2, idx1), c in zip(edges.tolist(), cs):
            i1 = crit_all[b, pc0[idx1]:pc0[idx1] + nc_all[b, idx1]]
            i2 = crit_all[b, pc0[idx2]:pc0[idx2] + nc_all[b, idx2]]
            pairs.append((b * N + pc0[idx1], b * N + pc0[idx2]))
            corr.append(np.stack([i1[c[:, 0]], i2[c[:, 1]]], 1))
        per.append((edges, [c.shape[0] for c in cs]))
    res = {k: v.cpu().numpy() for k, v in ransac_pairs(part_pcs.reshape(-1, 3), np.asarray(pairs, dtype=np.int64).reshape(-1, 2), corr, **ransac).items()}
    host_pts = part_pcs.cpu().numpy()
    out, at = [], 0
    for b in range(B):
        edges, ms = per[b]
        k = len(ms)
        T = np.repeat(np.eye(4)[None], k, 0)
        T[:, :3, :3], T[:, :3, 3] = res["R"][at:at + k], res["t"][at:at + k]
        conn = np.zeros(int(nv[b]))
        for idx2, idx1 in edges.tolist():
            conn[idx1] += 1
            conn[idx2] += 1
        extra_e, extra_T = translation_edges(perm[b], nc_all[b], crit_all[b], host_pts[b], np_all[b], int(nv[b]), conn)
        out.append({"edges": np.concatenate([edges, np.asarray(extra_e, dtype=np.int64).reshape(-1, 2)]),
                    "transformations": np.concatenate([T, np.asarray(extra_T, dtype=np.float64).reshape(-1, 4, 4)]),
                    "uncertainty": np.concatenate([1.0 / np.asarray(ms, dtype=np.float64), np.ones(len(extra_e))]), "n_ransac": k,
                    "ransac": {key: v[at:at + k] for key, v in res.items()}})
        at += k
    return out


def quat_to_rmat(q: np.ndarray) -> np.ndarray:
    """(w, x, y, z), normalised first, -> [3, 3]: scipy's Rotation.from_quat(q[[1, 2, 3, 0]]).as_matrix() of :446"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def anchor_poses(graph: dict, n_pcs, n_valid: int, part_quat, part_trans):
    """matching_base_model.py:431-453: the global poses of one puzzle, moved so that the pivot piece sits at its ground-truth pose.
    The pivot starts at piece 1 and moves to the first piece with more points than it (:436-440, as written); with no edge at all
    the poses are the identity and the pivot is piece 0 -> (poses [n_valid, 4, 4], pivot)"""
    npc = np.asarray(n_pcs, dtype=np.int64).reshape(-1)
    if len(graph["edges"]):
        poses = global_alignment(n_valid, graph["edges"], graph["transformations"], graph["uncertainty"])
        pivot = 1
        for idx in range(n_valid):
            if npc[idx] > npc[pivot]:
                pivot = idx
    else:
        poses, pivot = np.repeat(np.eye(4)[None], n_valid, 0), 0
    to_gt = np.eye(4)
    to_gt[:3, :3] = quat_to_rmat(np.asarray(part_quat)[pivot])
    to_gt[:3, 3] = np.asarray(part_trans, dtype=np.float64)[pivot]
    offset = to_gt @ np.linalg.inv(poses[pivot])
    return np.stack([offset @ p for p in poses]), pivot


def rmat_to_quat(R: np.ndarray) -> np.ndarray:
    """[..., 3, 3] -> (w, x, y, z) [..., 4] through scipy (the metrics' Euler angles do not depend on the sign)"""
    from scipy.spatial.transform import Rotation

    q = Rotation.from_matrix(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)).as_quat()
    return q[:, [3, 0, 1, 2]].reshape(*np.shape(R)[:-2], 4)


class MatchingEvaluator:
    """the reference's test pass behind the network (matching_base_model.py:144-454: transformation_loss ->
    compute_global_transformation -> calc_metric) on the GPU where it has a hot path: the pairwise RANSAC of the whole batch in one
    launch and the chamfer terms through the ragged nearest distance.  Deviations: DESIGN.md 5.12.
    shape_cd_index: "reference" advances calc_shape_cd's read position by n_pcs[0][i] (eval_utils.py:141, as written), "corrected"
    by the puzzle's own n_pcs[b][i]"""

    KEYS = ("part_acc", "chamfer_distance", "trans_mse", "trans_rmse", "trans_mae", "rot_mse", "rot_rmse", "rot_mae")

    def __init__(self, *, n_hyp: int = 50000, max_dist: float = 0.05, seed: int = 0, refine: bool = False, shape_cd_index: str = "reference"):
        if shape_cd_index not in ("reference", "corrected"):
            raise ValueError('shape_cd_index: "reference" or "corrected"')
        self.ransac = dict(n_hyp=n_hyp, max_dist=max_dist, seed=seed, refine=refine)
        self.shape_cd_index = shape_cd_index
        self.stats = {k: [] for k in self.KEYS + ("pred_trans", "gt_trans", "pred_rot", "gt_rot", "part_valids")}
        self.pred_dict, self.graphs, self.pivots = None, None, None

    def global_transformation(self, data_dict, out_dict) -> dict:
        """compute_global_transformation: pred_dict rot [B, P, 3, 3], trans [B, P, 3] (float64, host), after the pivot anchoring"""
        valids = np.asarray(data_dict["part_valids"].detach().cpu().numpy())
        n_valid = valids.sum(1).astype(np.int64)
        n_pcs = _host_int(data_dict["n_pcs"], "n_pcs")
        B, P = n_pcs.shape
        part_pcs = data_dict["part_pcs"][..., :3].contiguous()
        self.graphs = pose_graph(out_dict["perm_mat"], data_dict["n_critical_pcs"], data_dict["critical_pcs_idx"], part_pcs, n_pcs, n_valid,
                                 **self.ransac)
        quat, trans = data_dict["part_quat"].detach().cpu().numpy(), data_dict["part_trans"].detach().cpu().numpy()
        pred = {"rot": np.zeros((B, P, 3, 3)), "trans": np.zeros((B, P, 3))}
        self.pivots = []
        for b in range(B):
            poses, pivot = anchor_poses(self.graphs[b], n_pcs[b], int(n_valid[b]), quat[b], trans[b])
            pred["rot"][b, :n_valid[b]], pred["trans"][b, :n_valid[b]] = poses[:, :3, :3], poses[:, :3, 3]
            self.pivots.append(pivot)
        self.pred_dict = pred
        return pred

    def calc_metric(self, data_dict, pred_dict) -> dict:
        """calc_metric (:144-218).  part_acc's per-part chamfer distance runs over each piece's own points, once (the reference
        resamples N_sum indices per piece with replacement, :171-185)"""
        from puzzlefusion_plusplus.denoiser.evaluation.evaluator import rot_metrics, trans_metrics

        part_pcs = data_dict["part_pcs"][..., :3].contiguous()
        dev = part_pcs.device
        B, N = part_pcs.shape[:2]
        n_pcs = _host_int(data_dict["n_pcs"], "n_pcs")
        P = n_pcs.shape[1]
        valids = data_dict["part_valids"].to(dev)
        f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)
        pred_rot, pred_trans = f32(pred_dict["rot"]), f32(pred_dict["trans"])
        gt_trans = data_dict["part_trans"].to(dev).float()
        gt_quat = data_dict["part_quat"].to(dev).float()
        gt_rot = f32(np.stack([[quat_to_rmat(q) if np.any(q) else np.eye(3) for q in row] for row in gt_quat.cpu().numpy()]))       # padded parts: 1
        flat = part_pcs.reshape(-1, 3)
        piece_of = torch.from_numpy(np.concatenate([np.concatenate([np.repeat(np.arange(P), n_pcs[b]), np.zeros(N - n_pcs[b].sum(), dtype=np.int64)])
                                                    + b * P for b in range(B)])).to(dev)
        place = lambda rot, trans: torch.einsum("nij,nj->ni", rot.reshape(-1, 3, 3)[piece_of], flat) + trans.reshape(-1, 3)[piece_of]
        mine, truth = place(pred_rot, pred_trans), place(gt_rot, gt_trans)
        off = np.concatenate([[0], np.cumsum(np.concatenate([n_pcs, (N - n_pcs.sum(1))[:, None]], 1).reshape(-1))])      # pieces, then the rest
        d12, d21 = nn_dist_ragged(mine, off, truth, off), nn_dist_ragged(truth, off, mine, off)
        seg = torch.from_numpy(np.repeat(np.arange(off.size - 1), np.diff(off))).to(dev)
        sums = torch.zeros(off.size - 1, dtype=torch.float64, device=dev).index_add_(0, seg, (d12 + d21).double())
        cnt = torch.from_numpy(np.diff(off).reshape(B, P + 1)[:, :P]).to(dev)
        cd = (sums.reshape(B, P + 1)[:, :P] / cnt.clamp(min=1)).float()
        real = valids == 1
        part_acc = ((cd < 0.01) & real).sum(-1) / real.sum(-1)
        # the whole shape against gt_pcs (eval_utils.py:124-151)
        gt_pcs = data_dict["gt_pcs"][..., :3].to(dev).float().contiguous()
        gather, rot_i, segs = [], [], [0]
        for b in range(B):
            index, total = 0, 0
            for i in range(int(real[b].sum())):
                c = int(n_pcs[b, i])
                rows = np.arange(index, min(index + c, N)) + b * N
                gather.append(rows)
                rot_i.append(np.full(rows.size, b * P + i))
                total += rows.size
                index += int(n_pcs[0, i] if self.shape_cd_index == "reference" else c)
            segs.append(segs[-1] + total)
        gi, ri = torch.from_numpy(np.concatenate(gather)).to(dev), torch.from_numpy(np.concatenate(rot_i)).to(dev)
        final = torch.einsum("nij,nj->ni", pred_rot.reshape(-1, 3, 3)[ri], flat[gi]) + pred_trans.reshape(-1, 3)[ri]
        goff = np.arange(B + 1) * N
        a, c2 = nn_dist_ragged(final, segs, gt_pcs.reshape(-1, 3), goff), nn_dist_ragged(gt_pcs.reshape(-1, 3), goff, final, segs)
        sizes = torch.from_numpy(np.diff(segs)).to(dev)
        sa = torch.zeros(B, dtype=torch.float64, device=dev).index_add_(0, torch.from_numpy(np.repeat(np.arange(B), np.diff(segs))).to(dev), a.double())
        shape_cd = (sa / sizes.clamp(min=1) + c2.reshape(B, N).double().mean(1)).float()
        metric = {"part_acc": part_acc.mean(), "chamfer_distance": shape_cd.mean()}
        rot_host = np.array(pred_dict["rot"], dtype=np.float64)
        rot_host[~real.cpu().numpy()] = np.eye(3)                      # padded parts carry no pose; they are masked out below
        pred_q, gt_q = f32(rmat_to_quat(rot_host)), gt_quat
        for m in ("mse", "rmse", "mae"):
            tm, rm = trans_metrics(pred_trans, gt_trans, valids, m), rot_metrics(pred_q, gt_q, valids, m)
            metric[f"trans_{m}"], metric[f"rot_{m}"] = tm.mean(), rm.mean()
            self.stats[f"trans_{m}"].append(tm.cpu().numpy())
            self.stats[f"rot_{m}"].append(rm.cpu().numpy())
        for k, v in (("part_acc", part_acc), ("chamfer_distance", shape_cd), ("pred_trans", pred_trans), ("gt_trans", gt_trans), ("pred_rot", pred_rot),
                     ("gt_rot", gt_rot), ("part_valids", valids)):
            self.stats[k].append(v.cpu().numpy())
        self.part_cd = cd
        return metric

    def transformation_metrics(self, data_dict, out_dict) -> dict:
        """transformation_loss (:223-272) -> the reference's metric keys (0-dim tensors) and pred_dict"""
        pred = self.global_transformation(data_dict, out_dict)
        metric = self.calc_metric(data_dict, pred)
        metric["pred_dict"] = pred
        return metric
