"""GPU: the device assignment solver (csrc/matching_assign.hip through pfpp_hip/matching_assign.py) and the code paths that take it.

Yardstick of the kernels: pfpp_hip.matching_assign.assign_reference, the numpy float64 restatement, BITWISE: col, steps,
augmentations, status, u and v.  The arithmetic is add, subtract and compare in fp64 with a stated order and a total tie rule, so
this is the bar and not a tolerance; the restatement itself is pinned against scipy in tests/test_matching_assign_host.py.
Yardstick of the callers (MatchingHead, MatcherValidator, generate_matching_data): their own host-solver path."""
import warnings

import numpy as np
import pytest
import torch

import matching_assign_cases as AC
import matching_cases as cases

pytestmark = pytest.mark.gpu


def solve(dev, names, **kw):
    from pfpp_hip.matching_assign import assign_batch

    out = assign_batch([torch.from_numpy(np.array(AC.case(k).c)).to(dev) if k is not None else torch.empty((0, 0), device=dev) for k in names], **kw)
    torch.cuda.synchronize()
    return out


def assert_equals_reference(out, k, name):
    ref = AC.reference(name)
    got = (int(out.status[k]), int(out.steps[k]), int(out.augmentations[k]))
    assert got == (ref.status, ref.steps, ref.augmentations), (name, got, (ref.status, ref.steps, ref.augmentations))
    assert out.col[k].dtype == torch.int64 and np.array_equal(out.col[k].cpu().numpy(), ref.col), name
    for what, mine, want in (("u", out.u[k], ref.u), ("v", out.v[k], ref.v)):
        assert mine.dtype == torch.float64
        assert np.array_equal(AC.bits(mine.cpu().numpy()), AC.bits(want)), (name, what, np.abs(mine.cpu().numpy() - want).max())


def assert_same(a, ka, b, kb):
    assert int(a.status[ka]) == int(b.status[kb]) and int(a.steps[ka]) == int(b.steps[kb])
    assert int(a.augmentations[ka]) == int(b.augmentations[kb])
    assert torch.equal(a.col[ka], b.col[kb])
    for x, y in ((a.u, b.u), (a.v, b.v)):
        assert np.array_equal(AC.bits(x[ka].cpu().numpy()), AC.bits(y[kb].cpu().numpy()))


@pytest.mark.parametrize("name", AC.NAMES)
def test_bitwise_parity_with_the_restatement(hip_lib, dev, name):
    out = solve(dev, [name])
    assert_equals_reference(out, 0, name)
    assert_same(out, 0, solve(dev, [name]), 0)                      # two runs agree bitwise


def test_batch_of_different_sizes_with_an_empty_matrix(hip_lib, dev):
    """63, 1,025, 5 and 257 rows in one launch (workgroups of 1,024 threads, shaped by the largest), an empty matrix among them: each
    puzzle comes out as in its own call, whose workgroup its own size shapes"""
    names = ["sk_30_33", "uniform_1025", None, "zeros_5", "identity_257"]
    out = solve(dev, names)
    assert out.status.shape == (5,) and out.col[2].numel() == 0 and out.u[2].numel() == 0 and int(out.status[2]) == 0 and int(out.steps[2]) == 0
    for k, name in enumerate(names):
        if name is not None:
            assert_equals_reference(out, k, name)
            assert_same(out, k, solve(dev, [name]), 0)


def test_more_puzzles_than_one_launch_holds(hip_lib, dev):
    """MAX_PUZZLES + 6 puzzles: two launches by the plan, the second shaped by its own largest puzzle; every puzzle as in its own call"""
    from pfpp_hip.matching_assign import MAX_PUZZLES, plan_assign

    pool = ["uniform_3", "zeros_5", "uniform_64", "uniform_2", "uniform_65", "sk_30_33", "uniform_1"]
    names = [pool[k % len(pool)] for k in range(MAX_PUZZLES)] + ["uniform_2", "sk_all_weak_64x3", "uniform_1", "chain_130", "dominated_65", "quarters_64"]
    plan = plan_assign([AC.case(k).c.shape[0] for k in names])
    assert plan == [(0, MAX_PUZZLES, 128, 1), (MAX_PUZZLES, 6, 256, 1)]
    out = solve(dev, names)
    for first, count, _, _ in plan:                                 # walk the plan: every puzzle of every launch
        for k in range(first, first + count):
            assert_equals_reference(out, k, names[k])


def test_budget_of_one_stops_one_puzzle_and_leaves_its_neighbours(hip_lib, dev):
    names = ["uniform_64", "sk_30_35", "sk_100_100_57"]
    out = solve(dev, names, max_steps=[None, 1, None])
    assert int(out.status[1]) == 1 and int(out.steps[1]) == 1 and int(out.augmentations[1]) == 0
    for k in (0, 2):
        assert_equals_reference(out, k, names[k])
    exact = solve(dev, ["sk_30_35"], max_steps=AC.reference("sk_30_35").steps)
    assert_equals_reference(exact, 0, "sk_30_35")
    short = solve(dev, ["sk_30_35"], max_steps=AC.reference("sk_30_35").steps - 1)
    assert int(short.status[0]) == 1
    identity = solve(dev, ["identity_257"], max_steps=1)            # no search: the budget is never touched
    assert_equals_reference(identity, 0, "identity_257")


# ------------------------------------------------------------------------------------------------ MatchingHead
@pytest.fixture(scope="module")
def head(dev, hip_lib):
    from pfpp_hip.matching import MatchingHead

    h = MatchingHead()
    h.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}, strict=True)
    return h.to(dev)


def head_inputs(dev, with_degenerate: bool):
    pzs = [cases.make_puzzle(n) for n in ("five", "two", "split")]
    feats = [p["part_feats"] for p in pzs]
    if with_degenerate:                                             # piece 1 of "two" without a critical point: no Sinkhorn, no assignment
        two = cases.make_puzzle("two")
        x = two["part_feats"].copy()
        x[220:] = x[~two["critical"]][0]
        pzs.insert(1, two)
        feats.insert(1, x)
    return pzs, [torch.from_numpy(f).to(dev) for f in feats], np.stack([p["n_pcs"] for p in pzs]), np.stack([p["part_valids"] for p in pzs])


def assert_head_outputs_equal(pzs, host, device, rows_above_half: bool = True):
    from pfpp_hip.matching import match_edges

    assert torch.equal(host.n_critical_pcs, device.n_critical_pcs)
    nc = host.n_critical_pcs.cpu().numpy()
    for b, pz in enumerate(pzs):
        assert torch.equal(host.cls_pred[b], device.cls_pred[b]) and torch.equal(host.critical_pcs_idx[b], device.critical_pcs_idx[b])
        assert torch.equal(host.ds_mat[b], device.ds_mat[b])
        h, d = host.perm_mat[b], device.perm_mat[b]
        assert d.device == host.ds_mat[b].device and d.dtype == torch.int64 and torch.equal(h, d), b
        if h.numel() and rows_above_half:
            assert bool((host.ds_mat[b][torch.arange(h.numel(), device=h.device), h] > 0.5).all())       # the fixture: no row sits on a zero
        eh, ch = match_edges(h, nc[b], int(pz["part_valids"].sum()))
        ed, cd = match_edges(d, nc[b], int(pz["part_valids"].sum()))
        assert np.array_equal(eh, ed) and len(ch) == len(cd) and all(np.array_equal(x, y) for x, y in zip(ch, cd))


@pytest.mark.parametrize("with_degenerate", [False, True])
def test_head_with_the_device_solver_equals_the_host_path(dev, head, with_degenerate):
    pzs, feats, n_pcs, valids = head_inputs(dev, with_degenerate)
    host = head(feats, n_pcs, valids, dense_perm=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        device = head(feats, n_pcs, valids, dense_perm=False, solver="device")
    assert_head_outputs_equal(pzs, host, device)
    if with_degenerate:
        assert device.perm_mat[1].numel() == 0 and device.ds_mat[1].shape == (0, 0)
    t = device.timings
    assert t["fallback_puzzles"] == 0 and t["device_assignment_s"] > 0 and t["host_assignment_s"] == 0 and t["wait_for_copy_s"] == 0
    assert host.timings["fallback_puzzles"] == 0 and host.timings["device_assignment_s"] == 0 and host.timings["host_assignment_s"] > 0
    dense = head(feats, n_pcs, valids, solver="device")
    assert all(torch.equal(a, b) for a, b in zip(dense.perm_mat, head(feats, n_pcs, valids).perm_mat))
    with pytest.raises(ValueError, match="solver"):
        head(feats, n_pcs, valids, solver="gpu")


def test_head_falls_back_to_the_host_when_the_budget_runs_out(dev, head):
    """The fixture's puzzles come out of the initialisation complete (every row's largest entry is its match), so a budget never
    matters for them.  One more puzzle is "two" with five critical points of piece 0 pulled towards five others of that piece
    (x -> 0.3 x + 0.7 x', an affine mix, so the latents mix the same way): both rows of such a pair want the same column and one of
    them has to search.  With a budget of 1 that puzzle goes to the host solver; the others do not."""
    from pfpp_hip.matching_assign import assign_batch

    pzs, feats, n_pcs, valids = head_inputs(dev, True)
    two = cases.make_puzzle("two")
    x = two["part_feats"].copy()
    crit0 = np.nonzero(two["critical"][:220])[0]
    x[crit0[5:10]] = 0.3 * x[crit0[5:10]] + 0.7 * x[crit0[0:5]]
    pzs.append(two)
    feats.append(torch.from_numpy(x).to(dev))
    n_pcs, valids = np.concatenate([n_pcs, two["n_pcs"][None]]), np.concatenate([valids, two["part_valids"][None]])
    host = head(feats, n_pcs, valids, dense_perm=False)
    live = [b for b in range(len(pzs)) if host.ds_mat[b].numel()]
    steps = assign_batch([host.ds_mat[b] for b in live]).steps.tolist()
    over = [b for b, s in zip(live, steps) if s > 1]               # a budget of 1 allows one step
    assert over == [len(pzs) - 1], (live, steps)
    with pytest.warns(UserWarning, match=r"max_steps = 1\).*puzzle\(s\)") as rec:
        device = head(feats, n_pcs, valids, dense_perm=False, solver="device", max_steps=1)
    assert len(rec) == 1 and str(over) in str(rec[0].message)
    assert_head_outputs_equal(pzs, host, device, rows_above_half=False)
    assert device.timings["fallback_puzzles"] == 1 and device.timings["host_assignment_s"] > 0
    full = head(feats, n_pcs, valids, dense_perm=False, solver="device")          # and with the default budget the device solves it
    assert full.timings["fallback_puzzles"] == 0
    assert_head_outputs_equal(pzs, host, full, rows_above_half=False)


# ------------------------------------------------------------------------------------------------ MatcherValidator
@pytest.mark.parametrize("name", ["main", "one_owner"])
def test_validator_with_the_device_solver_equals_the_host_path(dev, hip_lib, name):
    import matching_train_cases as TC
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_fit import MatcherValidator

    h = MatchingHead(tau=TC.TAU, max_iter=TC.MAX_ITER)
    h.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in TC.head_state_dict().items()}, strict=True)
    h = h.to(dev)
    b = TC.make_batch(name)
    d = {k: torch.from_numpy(b[k]).to(dev) for k in ("gt_pcs", "part_valids")}
    d.update(n_pcs=b["n_pcs"], part_pcs=d["gt_pcs"])
    run = lambda val: val.step_from_feats(torch.from_numpy(b["part_feats"]).to(dev), d, critical_label=torch.from_numpy(b["critical_label"]).to(dev))
    vh, vd = MatcherValidator(None, h), MatcherValidator(None, h, solver="device")
    oh, od = run(vh), run(vd)
    assert torch.equal(vh.saved["n_critical_pcs"], vd.saved["n_critical_pcs"]) and vh.saved["counts"].tolist() == vd.saved["counts"].tolist()
    for k in ("mat_f1", "mat_precision", "mat_recall", "cls_loss", "mat_loss", "loss"):
        assert np.array_equal(AC.bits(np.float64(float(oh[k])).reshape(1)), AC.bits(np.float64(float(od[k])).reshape(1))), k
    for ds, ch, cd in zip(vh.saved["ds_mat"], vh.saved["cols"], vd.saved["cols"]):
        assert (ch is None) == (cd is None)
        if ch is not None:
            on_positive = ds[torch.arange(ch.numel(), device=ch.device), ch] > 0
            assert torch.equal(ch[on_positive], cd[on_positive]) and sorted(cd.tolist()) == list(range(cd.numel()))
    assert vd.timings["fallback_puzzles"] == 0 and vd.timings["host_assignment_s"] == 0 and vd.timings["device_assignment_s"] > 0
    with pytest.raises(ValueError, match="solver"):
        MatcherValidator(None, h, solver="gpu")


# ------------------------------------------------------------------------------------------------ generate_matching_data
def test_generate_matching_data_with_the_device_solver_writes_the_host_runs_files(dev, hip_lib, tmp_path):
    from pfpp_hip import generate_matching_data as gen
    from pfpp_hip import io as pfio

    feats = tmp_path / "features"
    feats.mkdir()
    torch.save({"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in cases.head_state_dict().items()}}, tmp_path / "jigsaw.ckpt")
    for name in ("five", "split"):
        pz = cases.make_puzzle(name)
        np.savez(feats / f"{pz['data_id']}.npz", part_feats=pz["part_feats"], gt_pcs=pz["gt_pcs"], n_pcs=pz["n_pcs"], part_valids=pz["part_valids"])
    common = ["--features", str(feats), "--checkpoint", str(tmp_path / "jigsaw.ckpt"), "--batch-size", "2"]
    assert gen.main(common + ["--out", str(tmp_path / "host")]) == 0
    assert gen.main(common + ["--out", str(tmp_path / "device"), "--assignment", "device"]) == 0
    for name in ("five", "split"):
        h = pfio.load_matching_data(str(tmp_path / "host" / f"{cases.DATA_ID[name]}.npz"))
        d = pfio.load_matching_data(str(tmp_path / "device" / f"{cases.DATA_ID[name]}.npz"))
        assert set(h) == set(d) and h["edges"].shape[0] >= 1
        for k in h:
            if k == "correspondences":
                assert len(h[k]) == len(d[k]) and all(np.array_equal(x, y) for x, y in zip(h[k], d[k]))
            else:
                assert np.array_equal(h[k], d[k]), k
