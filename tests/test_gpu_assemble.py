"""GPU: the batched verifier input (pfpp_edge_features_batch through ops.edge_features_batch), the batch-level matches
(DeviceMatches.batch_prepared), their use in AutoAgglomerative.test_batch (data_dict["matching_batch"]) and the front end
(pfpp_hip.assemble).

The yardstick everywhere is the existing per-puzzle route on the same device: ops.pose_apply_points + ops.edge_histogram + the scatter
by pair_pos + normalise_edge_hist (what _PuzzleState.edge_features does), and for the loop and the front end the runs that use it.
Every comparison is torch.equal / exact."""
import itertools
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import matching_cases as cases
import matching_edges_cases as EC

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY = -12345.0
# the loop test's verifier threshold.  The verifier carries seeded random weights: its sigmoid outputs hardly depend on the edge
# features, they are about 0.7533 (2 parts), 0.7686 .. 0.7690 (4 parts) and 0.7850 .. 0.7861 (6 parts), ordered by the edge's
# indices.  In the 6-part puzzle edge (2, 3) leads with 0.78608 before (0, 2) with 0.78576; the threshold sits between the two, so
# with part 0 as the reference part exactly the non-reference edge (2, 3) is accepted and merged in the first outer iteration.
# (With the reference part the generator chose, 2, every threshold promotes an edge's ends to reference parts before it could merge.)
LOOP_THRESHOLD = 0.78592


# ------------------------------------------------------------------------------------------------ the kernel
def hand_batch(P: int, seed: int = 3):
    """three puzzles as pfpp_match_edges leaves them (numpy): 0 holds slots of 1, 255, 256, 257 and 600 rows, its first and its last
    slot; 1 has no rows at all; 2 holds a slot of coincident matched points, a slot whose far rows (piece 3 sits 30 away) are dropped,
    and rows allocated behind its last correspondence"""
    rng = np.random.default_rng(seed)
    T = P * (P - 1) // 2
    tri = list(itertools.combinations(range(P), 2))
    n_pcs = np.zeros((3, P), dtype=np.int64)
    n_pcs[0, :P] = rng.integers(40, 90, P)
    n_pcs[1, :3] = (50, 0, 61)
    n_pcs[2, :5] = (70, 66, 1, 45, 33)
    start = np.cumsum(n_pcs, 1) - n_pcs
    m = np.zeros((3, T), dtype=np.int64)
    for s, rows in zip((0, 1, 3, 4, 6, T - 1), (1, 255, 256, 257, 600, 3)):
        m[0, s] = rows
    m[2, tri.index((0, 1))], m[2, tri.index((0, 4))], m[2, tri.index((1, 3))], m[2, tri.index((3, 4))] = 37, 30, 12, 5
    slack = (5, 17, 9)                                           # rows of the puzzle's slice behind its last correspondence
    row_off = np.concatenate([[0], np.cumsum(m.sum(1) + slack)]).astype(np.int64)
    edge_off = np.zeros((3, T + 1), dtype=np.int32)
    edge_off[:, 1:] = np.cumsum(m, 1)
    idx_a = np.full(int(row_off[-1]), -7777, dtype=np.int32)    # the entries behind a puzzle's last row keep a canary: never read
    idx_b = idx_a.copy()
    for b in range(3):
        for s, (i, j) in enumerate(tri):
            if m[b, s]:
                o = int(row_off[b] + edge_off[b, s])
                idx_a[o:o + m[b, s]] = start[b, i] + rng.integers(0, n_pcs[b, i], m[b, s])
                idx_b[o:o + m[b, s]] = start[b, j] + (rng.integers(0, n_pcs[b, j], m[b, s]) if (b, i, j) != (2, 1, 3) else
                                                      rng.choice(n_pcs[b, j], m[b, s], replace=False))      # distinct: they become copies
    # puzzle 2, slot (0, 4): 20 rows between pieces 0 and 4, then 10 rows whose a-point lies in the far piece 3
    o = int(row_off[2] + edge_off[2, tri.index((0, 4))])
    o13 = int(row_off[2] + edge_off[2, tri.index((1, 3))])
    shifted = np.setdiff1d(start[2, 3] + np.arange(n_pcs[2, 3]), idx_b[o13:o13 + 12])       # piece 3 without slot (1, 3)'s copies
    idx_a[o + 20:o + 30] = rng.choice(shifted, 10)
    o34 = int(row_off[2] + edge_off[2, tri.index((3, 4))])
    idx_a[o34:o34 + 5] = rng.choice(shifted, 5)                                              # slot (3, 4): every row is far
    pt_off = np.concatenate([[0], np.cumsum(n_pcs.sum(1))]).astype(np.int64)
    scale = np.repeat([1.0, 1.0, 0.25], n_pcs.sum(1))[:, None]
    pts = rng.uniform(-0.5, 0.5, (int(pt_off[-1]), 3)) * scale
    # a matched b-point is its a-point plus noise of 10^-3.5 .. 10^-0.5 (a point matched twice keeps its last partner, the earlier
    # rows then see an unrelated point): with the nearly equal poses below the distances spread over all six bins
    for b in (0, 2):
        for s in np.nonzero(m[b])[0]:
            o = int(row_off[b] + edge_off[b, s])
            ia, ib = pt_off[b] + idx_a[o:o + m[b, s]], pt_off[b] + idx_b[o:o + m[b, s]]
            pts[ib] = pts[ia] + rng.normal(0, 1, (ia.size, 3)) * 10 ** rng.uniform(-3.5, -0.5, (ia.size, 1))
    pts = pts.astype(np.float32)
    # puzzle 2, slot (1, 3): the matched points coincide after the poses (pieces 1 and 3 share a pose below, the points are copies)
    o = int(row_off[2] + edge_off[2, tri.index((1, 3))])
    pts[pt_off[2] + idx_b[o:o + 12]] = pts[pt_off[2] + idx_a[o:o + 12]]
    # non-unit quaternions (|q|^2 about 1.3: quaternion_apply without normalisation scales by it), a slightly different pose per piece
    quat = np.concatenate([1.15 * (1 + rng.normal(0, 0.002, (3, P, 1))), rng.normal(0, 0.01, (3, P, 3))], -1)
    pose = np.concatenate([rng.normal(0, 0.01, (3, P, 3)), quat], -1).astype(np.float32)
    pose[2, 3] = pose[2, 1]
    far = {"puzzle": 2, "slot": tri.index((0, 4)), "rows": 30}
    return {"P": P, "T": T, "n_pcs": n_pcs, "m": m, "row_off": row_off, "edge_off": edge_off, "idx_a": idx_a, "idx_b": idx_b,
            "pt_off": pt_off, "pts": pts, "pose": pose, "far": far, "coincident": {"puzzle": 2, "slot": tri.index((1, 3))}}


def shift_far_piece(hb) -> None:
    """piece 3 of puzzle 2 sits 30 away in the by-area points themselves (its pose stays piece 1's), except the copies of slot (1, 3)"""
    n_pcs, pt_off = hb["n_pcs"], hb["pt_off"]
    start = int(pt_off[2] + n_pcs[2, :3].sum())
    o = int(hb["row_off"][2] + hb["edge_off"][2, hb["coincident"]["slot"]])
    copies = set((pt_off[2] + hb["idx_b"][o:o + 12]).tolist())
    for k in range(start, start + int(n_pcs[2, 3])):
        if k not in copies:
            hb["pts"][k] += 30.0


def guarded(dev, values: np.ndarray, guard_value):
    flat = np.ascontiguousarray(values).reshape(-1)
    big = torch.full((flat.size + 2 * GUARD,), guard_value, dtype=torch.from_numpy(flat).dtype, device=dev)
    view = big[GUARD:GUARD + flat.size]
    view.copy_(torch.from_numpy(flat))
    return big, view


def per_puzzle_features(dev, hb, b: int):
    """the existing route for puzzle b: (edge features [T, 7], the six counts [T, 6])"""
    from pfpp_hip import ops
    from puzzlefusion_plusplus.auto_aggl import normalise_edge_hist

    P, T = hb["P"], hb["T"]
    a, e = int(hb["pt_off"][b]), int(hb["pt_off"][b + 1])
    part = torch.from_numpy(np.repeat(np.arange(P), hb["n_pcs"][b]).astype(np.int32)).to(dev)
    pts_t = ops.pose_apply_points(torch.from_numpy(hb["pts"][a:e]).to(dev), part, torch.from_numpy(hb["pose"][b]).to(dev), normalise=False)
    slots = np.nonzero(hb["m"][b])[0]
    r0, M = int(hb["row_off"][b]), int(hb["m"][b].sum())
    off = torch.from_numpy(hb["edge_off"][b][np.concatenate([slots, [T]])]).to(dev)
    ef = torch.zeros(1, T, 6, dtype=torch.int32, device=dev)
    if slots.size:
        hist = ops.edge_histogram(pts_t, torch.from_numpy(hb["idx_a"][r0:r0 + M]).to(dev), torch.from_numpy(hb["idx_b"][r0:r0 + M]).to(dev),
                                  off.contiguous(), int(hb["m"][b].max()))
        ef[0, torch.from_numpy(slots).to(dev)] = hist
    return normalise_edge_hist(ef)[0], ef[0]


def batched_features(dev, hb, puz):
    """one pose-apply over the whole batch and one pfpp_edge_features_batch launch for the puzzles `puz`; every operand sits
    between guard zones that must come back intact, the inputs unchanged -> [len(puz), T, 7]"""
    from pfpp_hip import ops

    P, T, B = hb["P"], hb["T"], 3
    slot_base = np.zeros(B, dtype=np.int32)
    for k, b in enumerate(puz):
        slot_base[b] = k * P
    part = np.concatenate([np.repeat(np.arange(P), hb["n_pcs"][b]) + slot_base[b] for b in range(B)]).astype(np.int32)
    pose = torch.from_numpy(np.concatenate([hb["pose"][b] for b in puz])).to(dev)
    pts_t = ops.pose_apply_points(torch.from_numpy(hb["pts"]).to(dev), torch.from_numpy(part).to(dev), pose, normalise=False)
    ins = {"pts": guarded(dev, pts_t.cpu().numpy(), 1e30), "pt_off": guarded(dev, hb["pt_off"], 1 << 40), "idx_a": guarded(dev, hb["idx_a"], 1 << 30),
           "idx_b": guarded(dev, hb["idx_b"], 1 << 30), "row_off": guarded(dev, hb["row_off"], 1 << 40),
           "edge_off": guarded(dev, hb["edge_off"], 1 << 30), "puz": guarded(dev, np.asarray(puz, dtype=np.int32), 1 << 30)}
    assert torch.equal(ins["pts"][1].view(-1, 3), pts_t)
    before = {k: big.clone() for k, (big, _) in ins.items()}
    big, out = guarded(dev, np.full((len(puz), T, 7), CANARY, dtype=np.float32), CANARY - 1)
    got = ops.edge_features_batch(ins["pts"][1].view(-1, 3), ins["pt_off"][1], ins["idx_a"][1], ins["idx_b"][1], ins["row_off"][1],
                                  ins["edge_off"][1].view(B, T + 1), ins["puz"][1], int(hb["m"].max()), out=out)
    torch.cuda.synchronize()
    for k, (whole, _) in ins.items():
        assert torch.equal(whole, before[k]), f"input {k} was written"
    assert (big[:GUARD] == CANARY - 1).all() and (big[GUARD + out.numel():] == CANARY - 1).all(), "guard zone of out written"
    assert not (out == CANARY).any(), "a slot of a listed puzzle was not written"
    return got.view(len(puz), T, 7).clone()


@pytest.fixture(scope="module", params=[5, 20], ids=["P5", "P20"])
def hand(request, dev, hip_lib):
    hb = hand_batch(request.param)
    shift_far_piece(hb)
    return hb, [per_puzzle_features(dev, hb, b) for b in range(3)]


def test_input_has_the_cases_it_was_built_for(hand):
    hb, want = hand
    T = hb["T"]
    assert {1, 255, 256, 257, 600} <= set(hb["m"][0].tolist()) and hb["m"][0, 0] and hb["m"][0, T - 1] and not hb["m"][1].any()
    feats, counts = want[2]
    far, co = hb["far"], hb["coincident"]
    kept = int(counts[far["slot"]].sum())
    print(f"far slot: {kept} of {far['rows']} rows counted; coincident slot: {counts[co['slot']].tolist()}")
    assert 0 < kept < far["rows"] and float(feats[far["slot"], 6]) == kept            # d >= 100 dropped: the seventh feature is not m
    assert counts[co["slot"]].tolist() == [12, 0, 0, 0, 0, 0]                           # d = 0
    assert not want[1][0].any() and want[1][0].shape == (T, 7)
    filled = sum(int((torch.cat([c for _, c in want]).sum(0) > 0)[k]) for k in range(6))
    print(f"bins populated: {filled} of 6")
    assert filled >= 4
    for b in (0, 2):
        sums = want[b][1].sum(1).cpu().numpy()
        assert (sums[hb["m"][b] == 0] == 0).all() and (sums <= hb["m"][b]).all()
    assert (want[0][1].sum(1).cpu().numpy() == hb["m"][0]).all()                        # puzzle 0: nothing dropped
    lost = hb["m"][2] > 0
    lost &= want[2][1].sum(1).cpu().numpy() == 0
    assert lost.sum() == 1 and not want[2][0][lost].any()                               # slot (3, 4): rows, all dropped: seven zeros


@pytest.mark.parametrize("puz", [(0, 1, 2), (2, 0), (1,)], ids=lambda p: "puz" + "".join(map(str, p)))
def test_batched_features_equal_the_per_puzzle_route(dev, hand, puz):
    hb, want = hand
    got = batched_features(dev, hb, puz)
    assert got.dtype == torch.float32
    for k, b in enumerate(puz):
        bad = (got[k] != want[b][0]).nonzero()[:5].tolist()
        assert torch.equal(got[k], want[b][0]), (b, bad)


def test_two_runs_agree_bitwise(dev, hand):
    hb, _ = hand
    assert torch.equal(batched_features(dev, hb, (0, 1, 2)), batched_features(dev, hb, (0, 1, 2)))


# ------------------------------------------------------------------------------------------------ batch_prepared
def device_matches(dev, batch: EC.Batch):
    from pfpp_hip.matching_edges import match_edges_batch

    return match_edges_batch([torch.from_numpy(p).to(dev) for p in batch.perm], torch.from_numpy(batch.n_critical_pcs).to(dev), batch.n_valid,
                             batch.n_pcs, [torch.from_numpy(c).to(dev) for c in batch.critical_pcs_idx])


@pytest.mark.parametrize("which", ["seeded", "fixture"])
def test_batch_prepared_implies_what_prepared_returns(hip_lib, dev, golden, which, monkeypatch):
    from pfpp_hip.matching_edges import BatchMatches, triangle_pairs

    batch = EC.seeded_batch() if which == "seeded" else EC.fixture_batch(golden("matching_head"), ("five", "two", "split"))
    dm = device_matches(dev, batch)
    uploads = []
    plain = torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: uploads.append(a.size) or plain(a))
    bo = dm.batch_prepared()
    monkeypatch.undo()
    assert isinstance(bo, BatchMatches) and len(uploads) == 1                           # one upload for the whole batch
    B, P, T = dm.B, dm.P, dm.T
    tri = triangle_pairs(P)
    assert bo.pivot.dtype == torch.int32 and torch.equal(bo.pivot.cpu(), torch.arange(P, dtype=torch.int32).repeat(B, 1))
    assert bo.pt_off.dtype == torch.int64 and bo.pt_off.cpu().tolist() == np.concatenate([[0], np.cumsum(batch.n_pcs.sum(1))]).tolist()
    assert bo.row_off.cpu().tolist() == dm.row_off.tolist()
    assert bo.idx_a is dm.idx_a and bo.idx_b is dm.idx_b and bo.edge_off is dm.edge_off   # the kernel's outputs, as they are
    assert tuple(bo.pts.shape) == (int(batch.n_pcs.sum()), 3) and bo.pts.dtype == torch.float32
    pt_off, row_off, edge_off = bo.pt_off.cpu().numpy(), bo.row_off.cpu().numpy(), bo.edge_off.cpu().numpy()
    max_m = []
    for b in range(B):
        want = dm.prepared(b)
        m = np.diff(edge_off[b])
        slots = np.nonzero(m)[0]
        r0 = int(row_off[b])
        assert [(int(i), int(j)) for i, j in tri[slots]] == want["pairs"]
        assert torch.equal(torch.from_numpy(slots).to(dev), want["pair_pos"])
        assert torch.equal(bo.edge_off[b][torch.from_numpy(np.concatenate([slots, [T]])).to(dev)], want["edge_off"])
        for k in ("idx_a", "idx_b"):
            assert torch.equal(getattr(bo, k)[r0:r0 + int(edge_off[b, T])], want[k]), (b, k)
        part = bo.point_part[int(pt_off[b]):int(pt_off[b + 1])]
        assert part.dtype == want["point_part"].dtype and torch.equal(part, want["point_part"])
        assert torch.equal(bo.point_slot[int(pt_off[b]):int(pt_off[b + 1])], part + b * P)
        assert (int(m.max()) if slots.size else 0) == want["max_m"]
        max_m.append(want["max_m"])
    assert bo.max_m == max(max_m) and isinstance(bo.max_m, int)


# ------------------------------------------------------------------------------------------------ the loop
def loop_model(weights_sd, dev, threshold, steps=3, iters=3):
    from pfpp_hip import config
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative

    cfg = config.auto_aggl_config()
    cfg.denoiser.model.num_inference_steps = steps
    cfg.verifier.max_iters = iters
    cfg.verifier.threshold = threshold
    model = AutoAgglomerative(cfg)
    model.encoder.load_state_dict(weights_sd("vqvae")); model.denoiser.load_state_dict(weights_sd("denoiser"))
    model.verifier.load_state_dict(weights_sd("verifier"))
    return model.to(dev).eval()


def loop_puzzles(dev):
    """three synthetic puzzles of 2, 4 and 6 parts with a random assignment each, matched in ONE pfpp_match_edges batch
    -> (per puzzle the dict without matching, the DeviceMatches, per puzzle x_init, per puzzle the noises)"""
    from pfpp_hip import synthetic
    from pfpp_hip.matching_edges import match_edges_batch

    bases, perms, crits, n_pcs, nc = [], [], [], [], []
    for k, parts in enumerate((2, 4, 6)):
        base = {k_: v.to(dev) for k_, v in synthetic.make_batch(70 + k, 1, num_points=1000, num_parts=parts).items()}
        md = synthetic.make_matching(base, seed=20 + k)
        tot = int(md["n_pcs"].sum())
        rng = np.random.default_rng(30 + k)
        col = rng.permutation(int(md["n_critical_pcs"].sum())).astype(np.int64)
        col[rng.random(col.size) < 0.05] = -1
        base.update({k_: md[k_] for k_ in ("part_pcs_by_area", "critical_pcs_idx", "n_pcs", "n_critical_pcs")})
        if parts == 6:                                            # see LOOP_THRESHOLD
            base["ref_part"] = torch.zeros_like(base["ref_part"])
            base["ref_part"][0, 0] = True
        if parts == 2:                                            # a fragment below the loop's size rule (0.05): the puzzle is complete
            other = int(torch.where(~base["ref_part"][0, :2])[0][0])      # after its first verifier call and leaves the batch early
            base["part_scale"][0, other] = 0.04
        assert base["part_pcs_by_area"].shape[1] == tot
        bases.append(base)
        perms.append(torch.from_numpy(col).to(dev))
        crits.append(md["critical_pcs_idx"][0, :tot].contiguous())
        n_pcs.append(md["n_pcs"][0].cpu().numpy())
        nc.append(md["n_critical_pcs"][0])
    dm = match_edges_batch(perms, torch.stack(nc).to(dev), [2, 4, 6], np.stack(n_pcs), crits)
    g = torch.Generator(device=dev).manual_seed(8)
    x0 = [torch.randn(1, 20, 7, device=dev, generator=g) for _ in range(3)]
    nz = [[torch.randn(1, 20, 7, device=dev, generator=g) for _ in range(9)] for _ in range(3)]
    return bases, dm, x0, nz


def run_loop(model, dicts, x0, nz, monkeypatch, batch_route: bool):
    """test_batch with the verifier inputs of every outer iteration recorded -> (results, [inputs per verifier call])"""
    from pfpp_hip import matching_edges, ops
    from puzzlefusion_plusplus import auto_aggl
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative

    seen = []
    plain = model.verifier.forward

    def recording(ef, *a, **kw):
        seen.append(ef.clone())
        return plain(ef, *a, **kw)

    monkeypatch.setattr(model.verifier, "forward", recording)
    events = []                                           # (parts of the puzzle, merges before, merges after) per after_verify call
    after = auto_aggl._PuzzleState.after_verify

    def noting(self, logits):
        n = self.n_merges
        after(self, logits)
        events.append((self.n_nodes, n, self.n_merges))

    monkeypatch.setattr(auto_aggl._PuzzleState, "after_verify", noting)
    if batch_route:
        monkeypatch.setattr(ops, "edge_histogram", lambda *a, **k: pytest.fail("ops.edge_histogram was called"))
        monkeypatch.setattr(AutoAgglomerative, "prepare_matching", staticmethod(lambda *a: pytest.fail("prepare_matching was called")))
        monkeypatch.setattr(matching_edges.DeviceMatches, "prepared", lambda *a: pytest.fail("DeviceMatches.prepared was called"))
    torch.manual_seed(5)                                  # a merge draws its first sampled point from torch's generator
    out = model.test_batch(dicts, x0, nz)
    monkeypatch.undo()
    return out, seen, events


def assert_same_results(a, b, what):
    for k in ("pred_trans", "pred_rots", "x", "trajectory", "ref_part"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert a["verifier_calls"] == b["verifier_calls"] and a["merges"] == b["merges"] and a["steps"] == b["steps"], what


def test_loop_with_matching_batch_equals_the_per_puzzle_route(weights_sd, dev, hip_lib, monkeypatch):
    model = loop_model(weights_sd, dev, LOOP_THRESHOLD)
    bases, dm, x0, nz = loop_puzzles(dev)
    per_puzzle = [dict(b, matching_prepared=dm.prepared(k)) for k, b in enumerate(bases)]
    first, seen_first, events = run_loop(model, per_puzzle, x0, nz, monkeypatch, batch_route=False)
    bo = dm.batch_prepared()
    batched = [dict(b, matching_batch=(bo, k)) for k, b in enumerate(bases)]
    second, seen_second, events_second = run_loop(model, batched, x0, nz, monkeypatch, batch_route=True)
    print("verifier_calls", [r["verifier_calls"] for r in first], "merges", [r["merges"] for r in first], "steps", [r["steps"] for r in first])
    assert len(seen_first) == len(seen_second) >= 2
    for i, (a, b) in enumerate(zip(seen_first, seen_second)):
        assert a.shape == b.shape and torch.equal(a, b), f"verifier input of outer iteration {i}"
    assert float(seen_first[0].abs().sum()) > 0
    for k in range(3):
        assert_same_results(first[k], second[k], k)
    # what the run has to exercise: a merge, a merge followed by a further outer iteration of its puzzle (the write-through of pivot
    # and of the by-area points reaches the next launch), and a puzzle that finishes before the others (the subset path)
    assert any(r["merges"] >= 1 for r in first)
    print("after_verify (parts, merges before, merges after):", events)
    assert events == events_second
    assert any(e[2] > e[1] and any(l[0] == e[0] for l in events[i + 1:]) for i, e in enumerate(events))
    assert len({r["steps"] for r in first}) > 1
    assert [s.shape[0] for s in seen_first] != [3] * len(seen_first)
    # the pivots of a merged puzzle were written through the view into the batch object
    merged = [k for k, r in enumerate(second) if r["merges"]]
    assert any(not torch.equal(bo.pivot[k], torch.arange(20, dtype=torch.int32, device=dev)) for k in merged)
    # one mixed call: puzzle 1 with its own prepared dict, the others through the batch object
    bo2 = dm.batch_prepared()
    mixed = [dict(b, matching_batch=(bo2, k)) if k != 1 else dict(b, matching_prepared=dm.prepared(1)) for k, b in enumerate(bases)]
    third, seen_third, _ = run_loop(model, mixed, x0, nz, monkeypatch, batch_route=False)
    assert len(seen_third) == len(seen_first) and all(torch.equal(a, b) for a, b in zip(seen_first, seen_third))
    for k in range(3):
        assert_same_results(first[k], third[k], ("mixed", k))


def test_matching_batch_refuses_a_contradicting_puzzle(weights_sd, dev, hip_lib):
    model = loop_model(weights_sd, dev, 0.9, iters=1)
    bases, dm, x0, nz = loop_puzzles(dev)
    bo = dm.batch_prepared()
    with pytest.raises(ValueError, match="matching_batch"):
        model.test_batch([dict(bases[0], matching_batch=(bo, 3))])                     # the batch holds puzzles 0..2
    short = dict(bases[0], part_pcs_by_area=bases[0]["part_pcs_by_area"][:, :-1].contiguous())
    with pytest.raises(ValueError, match="matching_batch.*points"):
        model.test_batch([dict(short, matching_batch=(bo, 0))])
    with pytest.raises(ValueError, match="matching_batch"):
        model.test_batch([dict(bases[0], matching_batch=(bo, 0), matching_prepared=dm.prepared(0))])


# ------------------------------------------------------------------------------------------------ the front end
def test_assemble_equals_the_route_through_matching_data_files(weights_sd, dev, hip_lib, tmp_path, capsys):
    from pfpp_hip import assemble, config
    from pfpp_hip import generate_matching_data as gen
    from pfpp_hip import io as pfio
    from puzzlefusion_plusplus.auto_aggl import AutoAgglomerative
    from puzzlefusion_plusplus.denoiser.dataset.dataset import GeometryLatentDataset

    feats, pc = tmp_path / "features", tmp_path / "pc_data"
    feats.mkdir()
    torch.save({"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}}, tmp_path / "jigsaw.ckpt")
    torch.save({"state_dict": {**{"denoiser." + k: v for k, v in weights_sd("denoiser").items()},
                               **{"encoder." + k: v for k, v in weights_sd("vqvae").items()}}}, tmp_path / "denoiser.ckpt")
    torch.save({"state_dict": {"verifier." + k: v for k, v in weights_sd("verifier").items()}}, tmp_path / "verifier.ckpt")
    puzzles = [cases.make_puzzle(n) for n in ("five", "two", "split")] + [cases.build_puzzle(*cases.CASES["two"], 14)]
    rng = np.random.default_rng(1)
    for pz in puzzles:
        np.savez(feats / f"{pz['data_id']}.npz", part_feats=pz["part_feats"], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"])
        if pz["data_id"] == 14:
            continue                                                                    # the puzzle without pc_data
        pv = int(pz["part_valids"].sum())
        ref = np.zeros(20, dtype=bool)
        ref[0] = True
        gt = rng.normal(0, 0.2, size=(pv, 1000, 3)) + rng.normal(0, 0.5, size=(pv, 1, 3))
        pfio.save_pc_data(str(pc), data_id=pz["data_id"], part_valids=pz["part_valids"], num_parts=pv, mesh_file_path=f"a/{pz['data_id']}",
                          graph=np.zeros((20, 20), dtype=bool), category="everyday", part_pcs_gt=gt.astype(np.float32), ref_part=ref)
    ids, seed = [11, 12, 13], 3
    # ---- the front end
    rc = assemble.main(["--features", str(feats), "--matcher", str(tmp_path / "jigsaw.ckpt"), "--denoiser", str(tmp_path / "denoiser.ckpt"),
                        "--verifier", str(tmp_path / "verifier.ckpt"), "--pc-data", str(pc), "--out", str(tmp_path / "out"), "--in-flight", "2",
                        "--seed", str(seed), "denoiser.model.num_inference_steps=3", "verifier.max_iters=2",
                        f"+experiment_output_path={tmp_path / 'exp_a'}"])
    said = capsys.readouterr().out
    assert rc == 0 and "skipped" in said and " 14" in said.split("skipped")[1].splitlines()[0]
    lines = [json.loads(l) for l in (tmp_path / "out" / "results.jsonl").read_text().splitlines()]
    assert [l["data_id"] for l in lines] == ids
    assert sorted(os.listdir(tmp_path / "out")) == ["results.jsonl"]                    # no matching_data file
    assert not [f for _, _, fs in os.walk(tmp_path / "exp_a") for f in fs if f.endswith(".npz")]
    # ---- the route through files: the matcher in the same batches, the dataset from the directory, test_batch in the same groups
    mdir = tmp_path / "matching_data"
    assert gen.main(["--features", str(feats), "--checkpoint", str(tmp_path / "jigsaw.ckpt"), "--out", str(mdir), "--batch-size", "2",
                     "--assignment", "device", "--edges", "device"]) == 0
    cfg = config.auto_aggl_config()
    cfg.denoiser.model.num_inference_steps, cfg.verifier.max_iters = 3, 2
    cfg.experiment_output_path = str(tmp_path / "exp_b")
    cfg.denoiser.data = NS(max_num_part=20, data_val_dir=str(pc), matching_data_path=str(mdir))
    model = AutoAgglomerative(cfg)
    assemble.load_loop_weights(model, str(tmp_path / "denoiser.ckpt"), str(tmp_path / "verifier.ckpt"))
    model = model.to(dev).eval()
    np.random.seed(seed)
    torch.manual_seed(seed)
    ds = GeometryLatentDataset(cfg.denoiser, str(pc), -1, "test")
    assert [s["data_id"] for s in ds.data_list] == ids
    results = []
    for group in ([0, 1], [2]):
        results += model.test_batch([assemble.as_batch_of_one(ds[i], dev) for i in group])
    for line, r in zip(lines, results):
        for k in assemble.RESULT_KEYS:
            assert line[k] == float(r["metrics"][k][0]), (line["data_id"], k)
        assert (line["verifier_calls"], line["merges"], line["steps"]) == (r["verifier_calls"], r["merges"], r["steps"])
        assert line["verifier_calls"] >= 1
        a, b = (tmp_path / e / "inference" / "results" / str(line["data_id"]) for e in ("exp_a", "exp_b"))
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == 4
        for f in os.listdir(a):
            if f.endswith(".npy"):
                assert np.array_equal(np.load(a / f), np.load(b / f)), (line["data_id"], f)
