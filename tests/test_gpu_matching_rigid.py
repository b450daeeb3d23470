"""GPU: the rigid term of the matcher's training loss (csrc/matching_rigid.hip, the seeded Sinkhorn backward of csrc/matching_train.hip,
pfpp_hip/matching_rigid.py) against the float64 reference of tests/matching_rigid_cases.py, which tests/test_matching_rigid_host.py
pins to the reference's own code (tests/golden/matching_rigid.npz).  Every test prints the figures it measured before it asserts.

Bars.
* Pair sums: fp64 sums of exact fp64 terms in another order than numpy's: n 2^-52 sum |terms| per output.
* Poses, on pairs whose relative eigen-gap (lambda_1 - lambda_2) / max |lambda| is at least 0.02: R within 2^-24 and t within 2^-24
  max(|t|, 1) of float64 eigh on the same W (the one rounding to fp32 is 2^-25; the fp64 Jacobi's own error over the gap is orders
  below).  On every pair, kept or not, R is orthonormal to 4 x 2^-24 with det > 0 and its quaternion attains lambda_max of the float64 N to
  1e-6 |N|; eigenvalues within 1e-12 |N|.
* Loss, per-pair pair_loss and mat_s, dP: against the float64 restatement FED THE GPU's (R, t) - the poses are constants of the loss -
  with 4 x the reference's own float32-against-float64 deviation of that tensor (the fixture's `*_dev_*`), floor 4 x 2^-23 of the
  tensor's maximum.
* Seeded Sinkhorn backward: the ds bars of tests/test_gpu_matching_train.py (4 x the fixture's deviation of the same size and step count).
* Whole step: 4 x the fixture's deviations of the reference's step at weights (1, 1, 1), without a floor, the float64 restatement fed
  the GPU's ReLU masks and poses, for two consecutive steps (the second held to the first step's deviations): loss, rig_loss, every
  gradient, d_part_feats, the running statistics, and mat_loss, pair_loss and mat_s.  cls_loss, which the step's table does not list,
  is checked too, but not against the fixture: the deviation of one scalar is a single draw (1.7e-8 on `one_owner`, a third of a
  float32 rounding; the same kernel's cls_loss is 8.1e-8 off float64 in that batch's second step), so its bar comes from the format:
  the loss is a mean of positive per-element terms that pfpp_match_cls_bce, like torch, forms in float32 with four roundings each
  (expf, log1pf, two additions; the sum is fp64): 4 x 2^-24 relative."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("matching_rigid_cases", Path(__file__).resolve().parent / "matching_rigid_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)
tcases = cases._tc

BAR = 4.0
FLOOR = 4 * 2.0 ** -23
MASK_MARGIN = 2e-5          # tests/test_gpu_matching_train.py
LR = 1e-3
U24 = 2.0 ** -24
CLS_LOSS_BAR = 4 * U24      # see the module docstring


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("matching_rigid")


@pytest.fixture(scope="module")
def train_fixture(golden):
    return golden("matching_train")


_runs = {}


def kernel_run(dev, name):
    """the kernels on a kernel-level case, twice; ds_mat is handed over with a row stride and poison behind every row"""
    if name not in _runs:
        from pfpp_hip.matching_rigid import rigid_pairs

        kc = cases.kernel_case(name)
        mats = []
        for m in kc["ds_mat"]:
            buf = torch.full((m.shape[0], m.shape[0] + 3), 3.0e4, dtype=torch.float32, device=dev)
            buf[:, :m.shape[0]] = torch.from_numpy(m).to(dev)
            mats.append(buf[:, :m.shape[0]])
        pts = [torch.from_numpy(p).to(dev) for p in kc["pts"]]
        outs = [rigid_pairs(mats, pts, kc["row_piece"], kc["n_valid"], w_rig_loss=1.0) for _ in range(2)]
        host = lambda o: {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in o.items() if k in
                          ("rb", "R", "t", "mat_s", "pair_loss", "eigenvalues", "pair_status", "rig_loss", "n_sum", "scale", "numerator", "dP")}
        ref = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"])
        _runs[name] = (kc, host(outs[0]), host(outs[1]), ref)
    return _runs[name]


def rot_to_quat(R):
    """the unit quaternion (scalar first) of pairwise_alignment.py:52-70's R, by the largest of the four squared components"""
    t = np.trace(R)
    sq = np.array([1 + t, 1 + 2 * R[0, 0] - t, 1 + 2 * R[1, 1] - t, 1 + 2 * R[2, 2] - t]) / 4
    k = int(sq.argmax())
    q = np.zeros(4)
    q[k] = np.sqrt(sq[k])
    d = 4 * q[k]
    if k == 0:
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) / d, (R[0, 2] - R[2, 0]) / d, (R[1, 0] - R[0, 1]) / d
    elif k == 1:
        q[0], q[2], q[3] = (R[2, 1] - R[1, 2]) / d, (R[0, 1] + R[1, 0]) / d, (R[0, 2] + R[2, 0]) / d
    elif k == 2:
        q[0], q[1], q[3] = (R[0, 2] - R[2, 0]) / d, (R[0, 1] + R[1, 0]) / d, (R[1, 2] + R[2, 1]) / d
    else:
        q[0], q[1], q[2] = (R[1, 0] - R[0, 1]) / d, (R[0, 2] + R[2, 0]) / d, (R[1, 2] + R[2, 1]) / d
    return q / np.linalg.norm(q)


# ------------------------------------------------------------------------------------------------ the kernels on given matrices
@pytest.mark.parametrize("name", list(cases.KERNEL_CASES))
def test_pair_sums_against_float64(dev, hip_lib, name):
    """(r_i, b_i) of every row against every later piece: pieces of 0, 1, 2, 3, 63, 64, 65 rows (under, on and over a tile), 20
    pieces, n = 1033 (several column tiles per piece), zero blocks, two puzzles; two runs bitwise equal"""
    kc, got, again, _ = kernel_run(dev, name)
    for b, m in enumerate(kc["ds_mat"]):
        want, mag = cases.pair_sums_reference(m, kc["pts"][b], kc["counts"][b])
        P = want.shape[1]
        rb = got["rb"][b].numpy()[:, :P]
        err = np.abs(rb - want)
        bound = m.shape[0] * 2.0 ** -52 * mag
        worst = float((err / np.maximum(bound, 1e-300)).max(initial=0.0))
        print(f"{name} puzzle {b}: n {m.shape[0]}, {P} pieces, largest |error| {float(err.max(initial=0.0)):.3g}, largest error / bound {worst:.3g}")
        assert (err <= bound).all()
        assert not got["rb"][b].numpy()[:, P:].any()
        assert torch.equal(got["rb"][b], again["rb"][b])


@pytest.mark.parametrize("name", list(cases.KERNEL_CASES))
def test_poses_against_float64_eigh(dev, hip_lib, name):
    kc, got, again, ref = kernel_run(dev, name)
    R, t, ev, status = got["R"].numpy().astype(np.float64), got["t"].numpy().astype(np.float64), got["eigenvalues"].numpy(), got["pair_status"].numpy()
    assert np.array_equal(status, ref["status"]), (status, ref["status"])
    assert all(torch.equal(got[k], again[k]) for k in ("R", "t", "eigenvalues", "pair_status", "mat_s", "pair_loss"))
    worst = {"R": 0.0, "t": 0.0, "orth": 0.0, "lam": 0.0, "eig": 0.0}
    firm = 0
    for k, (b, p, q) in enumerate(ref["pairs"]):
        off = np.concatenate([[0], np.cumsum(kc["counts"][b])])
        W = kc["ds_mat"][b].astype(np.float64)
        W = W[off[p]:off[p + 1], off[q]:off[q + 1]] + W[off[q]:off[q + 1], off[p]:off[p + 1]].T
        X = kc["pts"][b].astype(np.float64)
        R64, t64, v, N = cases.horn(X[off[p]:off[p + 1]], X[off[q]:off[q + 1]], W)
        norm = float(np.abs(v).max())
        worst["eig"] = max(worst["eig"], float(np.abs(ev[k] - v).max()) / norm if norm > 0 else float(np.abs(ev[k]).max()))
        assert float(np.abs(ev[k] - v).max()) <= 1e-12 * norm, (name, k)
        if 1 in (kc["counts"][b][p], kc["counts"][b][q]):
            assert norm == 0 and np.array_equal(R[k], np.eye(3)), (name, k, "a single point gives N = 0 and the identity")
        orth = float(np.abs(R[k] @ R[k].T - np.eye(3)).max())              # every pair, the skipped and the 0 / 0 ones included
        qk = rot_to_quat(R[k])
        lam = float(v[-1] - qk @ N @ qk)
        worst["orth"], worst["lam"] = max(worst["orth"], orth), max(worst["lam"], lam / norm if norm > 0 else 0.0)
        assert orth <= 4 * U24 and np.linalg.det(R[k]) > 0 and lam <= 1e-6 * norm, (name, k, orth, lam)
        if status[k] != 1:
            assert not t[k].any()                                          # no translation where mat_s == 0
            continue
        if cases.eigen_gap(v) >= cases.GAP_MIN:
            firm += 1
            eR, et = float(np.abs(R[k] - R64).max()), float((np.abs(t[k] - t64) / np.maximum(np.abs(t64), 1)).max())
            worst["R"], worst["t"] = max(worst["R"], eR), max(worst["t"], et)
            assert eR <= U24 and et <= U24, (name, k, eR, et)
    print(f"{name}: {len(ref['pairs'])} pairs, {int((status == 1).sum())} kept, {firm} with a gap of {cases.GAP_MIN} or more: R {worst['R']:.3g}, t {worst['t']:.3g} "
          f"(bar {U24:.3g}); |R R^T - 1| {worst['orth']:.3g}, lambda_max - q N q {worst['lam']:.3g} |N|, eigenvalues {worst['eig']:.3g} |N|")


@pytest.mark.parametrize("name", list(cases.KERNEL_CASES))
def test_loss_and_gradient_against_float64_fed_the_gpu_poses(dev, hip_lib, fixture, name):
    kc, got, again, _ = kernel_run(dev, name)
    ref = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"], poses=(got["R"].numpy(), got["t"].numpy()))
    status = got["pair_status"].numpy()
    assert np.array_equal(status, ref["status"])
    dP = [d.double().numpy() for d in got["dP"]]
    assert all(torch.equal(a, b) for a, b in zip(got["dP"], again["dP"])) and torch.equal(got["rig_loss"], again["rig_loss"])
    # exact zeros: diagonal blocks and the pairs that are not kept
    for b, g in enumerate(dP):
        off = np.concatenate([[0], np.cumsum(kc["counts"][b])])
        for p in range(len(off) - 1):
            assert not g[off[p]:off[p + 1], off[p]:off[p + 1]].any()
        for k, (pb, p, q) in enumerate(ref["pairs"]):
            if pb == b and status[k] != 1:
                assert not g[off[p]:off[p + 1], off[q]:off[q + 1]].any() and not g[off[q]:off[q + 1], off[p]:off[p + 1]].any()
    if not ref["finite"]:
        print(f"{name}: the reference is not finite here ({np.isnan(float(fixture[name + '_rig_loss']))}); rig_loss {float(got['rig_loss'])}, scale {float(got['scale'])}")
        assert float(got["rig_loss"]) == 0.0 and float(got["scale"]) == 0.0 and all(not g.any() for g in dP)
        return
    bar = lambda q: max(BAR * float(fixture[f"{name}_dev_{q}"]), FLOOR)
    kept = status == 1
    assert float(got["n_sum"]) == ref["n_sum"] == float(fixture[f"{name}_n_sum"])
    e_loss = abs(float(got["rig_loss"]) - ref["rig_loss"]) / abs(ref["rig_loss"])
    e_ms = float(np.abs(got["mat_s"].numpy() - ref["mat_s"]).max()) / float(np.abs(ref["mat_s"]).max())
    e_pl = float(np.abs(got["pair_loss"].numpy() - ref["pair_loss"])[kept].max()) / float(np.abs(ref["pair_loss"]).max())
    want = np.concatenate([g.numpy().reshape(-1) for g in ref["dP"]])
    e_dp = float(np.abs(np.concatenate([g.reshape(-1) for g in dP]) - want).max()) / float(np.abs(want).max())
    print(f"{name}: rig_loss {float(got['rig_loss']):.7g}: {e_loss:.3g} (bar {bar('rig_loss'):.3g}), mat_s {e_ms:.3g} (bar {bar('mat_s'):.3g}), "
          f"pair_loss {e_pl:.3g} (bar {bar('pair_loss'):.3g}), dP / max {e_dp:.3g} (bar {bar('dP'):.3g})")
    assert e_loss <= bar("rig_loss") and e_ms <= bar("mat_s") and e_pl <= bar("pair_loss") and e_dp <= bar("dP")
    assert abs(float(got["scale"]) - 1.0 / ref["n_sum"]) <= 1e-15


@pytest.mark.parametrize("n", (3, 65, 257))
def test_seeded_sinkhorn_backward(dev, hip_lib, train_fixture, n):
    """a zero seed gives pfpp_sinkhorn_train_bwd's result bit for bit; a random seed the float64 autograd of g BCE + <seed, P>, for
    step counts whose first pass runs in the row layout and in the column layout"""
    from pfpp_hip.matching_train import sinkhorn_train_bwd, sinkhorn_train_fwd

    s_np, tgt_np = tcases.sinkhorn_case(n)
    s, tgt = torch.from_numpy(s_np).to(dev), torch.from_numpy(tgt_np).to(dev)
    ldg = (n + 3) & ~3
    g = 0.37
    seed_np = np.zeros((n, ldg), dtype=np.float32)
    seed_np[:, :n] = np.random.default_rng([3, n]).normal(size=(n, n)) * 0.5
    for it in tcases.SINKHORN_ITERS:
        ds_mat, _, pots = sinkhorn_train_fwd(s, tgt, tau=tcases.TAU, max_iter=it)
        plain = sinkhorn_train_bwd(s, tgt, pots, ds_mat, g=g, tau=tcases.TAU, max_iter=it, padded=True)
        zero = sinkhorn_train_bwd(s, tgt, pots, ds_mat, g=g, tau=tcases.TAU, max_iter=it, padded=True, seed=torch.zeros((n, ldg), dtype=torch.float32, device=dev))
        assert torch.equal(plain, zero), f"n {n}, {it} steps: a zero seed changes the result"
        runs = [sinkhorn_train_bwd(s, tgt, pots, ds_mat, g=g, tau=tcases.TAU, max_iter=it, padded=True, seed=torch.from_numpy(seed_np).to(dev)).cpu()
                for _ in range(2)]
        assert torch.equal(runs[0], runs[1]) and not runs[0][:, n:].any()
        s64 = torch.from_numpy(s_np).double().requires_grad_(True)
        P = torch.exp(tcases.sinkhorn_log(s64, tcases.TAU, it))
        (g * tcases.perm_loss_sum(P, tgt_np) + (torch.from_numpy(seed_np[:, :n]).double() * P).sum()).backward()
        err = float((runs[0][:, :n].double() - s64.grad).abs().max()) / float(s64.grad.abs().max())
        bar = BAR * float(train_fixture[f"sk_n{n}_t{it}_dev_grad"])
        print(f"n {n} steps {it}: seeded ds / max {err:.3g} (bar {bar:.3g})")
        assert err <= bar, (n, it)


def test_ordered_column_sums(dev, hip_lib):
    """the bias gradients' column sums: 1, 64, 65 and 360 rows (one block, one past it, six), 4, 512 and 13 columns behind a row
    stride; fp64 partials rounded once: 2^-24 of the sum plus the fp64 reordering bound; two runs bitwise equal"""
    from pfpp_hip.matching_train import colsum_ordered

    gen = torch.Generator().manual_seed(1)
    for rows, cols in ((1, 4), (64, 512), (65, 13), (360, 4), (360, 512), (0, 4)):
        buf = torch.randn(rows, cols + 3, generator=gen) * 3
        x = buf.to(dev)[:, :cols]
        got, again = colsum_ordered(x), colsum_ordered(x)
        want, mag = buf[:, :cols].double().sum(0), buf[:, :cols].double().abs().sum(0)
        err = (got.cpu().double() - want).abs()
        bound = U24 * want.abs() + rows * 2.0 ** -52 * mag
        print(f"colsum_ordered [{rows}, {cols}]: largest error / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}")
        assert got.shape == (cols,) and (err <= bound).all() and torch.equal(got, again)


# ------------------------------------------------------------------------------------------------ the whole step
def head_on(dev, sd=None):
    from pfpp_hip.matching import MatchingHead

    head = MatchingHead()
    head.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in (sd or cases.head_state_dict()).items()}, strict=True)
    return head.to(dev)


def batch_on(dev, name):
    b = cases.make_batch(name)
    b["part_pcs"] = cases.make_part_pcs(b)
    return b, {k: torch.from_numpy(b[k]).to(dev) for k in ("part_feats", "gt_pcs", "critical_label", "part_pcs")}


def engine_step(eng, t, b, rigid=True):
    kw = {"part_pcs": t["part_pcs"]} if rigid else {}
    loss_dict, d = eng.loss_and_grads(t["part_feats"], t["gt_pcs"], b["n_pcs"], b["part_valids"], critical_label=t["critical_label"], **kw)
    grads = {k: p.grad.detach().clone() for k, p in eng.params.items()}
    masks = (eng.saved["h_cls"].cpu() > 0, eng.saved["h_aff"].cpu() > 0)
    return loss_dict, d.clone(), grads, masks


def state64(head):
    return {k: v.detach().cpu().double().clone() for k, v in head.state_dict().items()}


@pytest.mark.parametrize("name", list(cases.BATCHES))
def test_whole_step_with_the_rigid_term(dev, hip_lib, fixture, name):
    """weights (1, 1, 1) on the three batches of the head's tests, two consecutive steps with an Adam step between: the three
    losses, every gradient, d_part_feats and the running statistics against float64 fed the GPU's ReLU masks and poses"""
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine

    head = head_on(dev)
    eng = MatchingHeadRigidTrainEngine(head, w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=1.0)
    b, t = batch_on(dev, name)
    key = f"step_{name}"
    dev_of = lambda q: CLS_LOSS_BAR if q == "cls_loss" else BAR * float(fixture[f"{key}_dev_{q}"])
    for step in (1, 2):
        sd = state64(head)
        loss_dict, d, grads, masks = engine_step(eng, t, b)
        after = state64(head)
        poses = (eng.saved["R"].cpu().numpy(), eng.saved["t"].cpu().numpy())
        ref = cases.head_rigid_train_reference(sd, b, b["part_pcs"], relu_masks=masks, poses=poses)
        rig = ref["rigid"]
        assert np.array_equal(eng.saved["rigid_pairs"], np.asarray(rig["pairs"]).reshape(-1, 3)) and np.array_equal(eng.saved["pair_status"].cpu().numpy(), rig["status"])
        assert float(eng.saved["rig_n_sum"]) == rig["n_sum"] == float(fixture[f"{key}_n_sum"])
        for nm, pre, mask in (("classifier", ref["pre_cls"], masks[0]), ("extractor", ref["pre_aff"], masks[1])):
            diff = (pre > 0) != mask
            margin = float(pre[diff].abs().max()) if diff.any() else 0.0
            print(f"{name} step {step} {nm} ReLU: {int(diff.sum())} of {diff.numel()} signs differ from float64's, largest |pre-activation| there {margin:.3g}")
            assert margin <= MASK_MARGIN
        if step == 1:                                  # the masks and the GPU's poses moved nothing that matters
            assert abs(float(ref["loss"]) - float(fixture[f"{key}_loss"])) <= 1e-5 * float(ref["loss"])
        for k in ("loss", "mat_loss", "rig_loss", "cls_loss"):
            e = abs(float(loss_dict[k]) - float(ref[k])) / abs(float(ref[k]))
            print(f"{name} step {step} {k} {float(loss_dict[k]):.7g}: {e:.3g} (bar {dev_of(k):.3g})")
            assert e <= dev_of(k), k
        kept = rig["status"] == 1
        e_pl = float(np.abs(eng.saved["pair_loss"].cpu().numpy() - rig["pair_loss"])[kept].max()) / float(np.abs(rig["pair_loss"]).max())
        e_ms = float(np.abs(eng.saved["mat_s"].cpu().numpy() - rig["mat_s"]).max()) / float(np.abs(rig["mat_s"]).max())
        print(f"{name} step {step} pair_loss {e_pl:.3g} (bar {dev_of('pair_loss'):.3g}), mat_s {e_ms:.3g} (bar {dev_of('mat_s'):.3g})")
        assert e_pl <= dev_of("pair_loss") and e_ms <= dev_of("mat_s")
        for k in tcases.PARAMS:
            want = ref["grads"][k]
            e = float((grads[k].cpu().double() - want.reshape(grads[k].shape)).abs().max()) / float(want.abs().max())
            print(f"{name} step {step} grad {k}: {e:.3g} (bar {dev_of('grad_' + k):.3g})")
            assert e <= dev_of("grad_" + k), k
        e = float((d.cpu().double() - ref["d_part_feats"]).abs().max()) / float(ref["d_part_feats"].abs().max())
        print(f"{name} step {step} d_part_feats: {e:.3g} (bar {dev_of('d_part_feats'):.3g})")
        assert e <= dev_of("d_part_feats")
        for k, want in ref["buffers"].items():
            e = float((after[k] - want).abs().max()) / float(want.abs().max())
            print(f"{name} step {step} {k}: {e:.3g} (bar {dev_of(k):.3g})")
            assert e <= dev_of(k), k
        eng.optimizer_step(lr=LR)


def test_without_the_rigid_weight_the_step_is_the_base_engines(dev, hip_lib):
    """w_rig_loss = 0: the base class's launches in the base class's order; gradients, buffers and d_part_feats bit for bit; with
    w_mat_loss = 0 the classifier phase, whatever w_rig_loss is"""
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine
    from pfpp_hip.matching_train import MatchingHeadTrainEngine

    b, t = batch_on(dev, "main")
    base_head, new_head = head_on(dev), head_on(dev)
    base = MatchingHeadTrainEngine(base_head, w_cls_loss=1.0, w_mat_loss=1.0)
    new = MatchingHeadRigidTrainEngine(new_head, w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=0.0)
    la, da, ga, _ = engine_step(base, t, b, rigid=False)
    lb, db, gb, _ = engine_step(new, t, b, rigid=True)               # part_pcs given and not used
    worst = max(float((ga[k] - gb[k]).abs().max()) / float(ga[k].abs().max()) for k in ga)
    print(f"w_rig_loss = 0 against the base engine: largest gradient difference / max {worst:.3g}, d_part_feats {float((da - db).abs().max()):.3g}")
    assert "rig_loss" not in lb and float(la["loss"]) == float(lb["loss"])
    assert torch.equal(da, db) and all(torch.equal(ga[k], gb[k]) for k in ga)
    sa, sb = base_head.state_dict(), new_head.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    phase0 = MatchingHeadRigidTrainEngine(head_on(dev), w_cls_loss=1.0, w_mat_loss=0.0, w_rig_loss=1.0)
    l0, _ = phase0.loss_and_grads(t["part_feats"], t["gt_pcs"], b["n_pcs"], b["part_valids"], critical_label=t["critical_label"])
    assert "mat_loss" not in l0 and "rig_loss" not in l0 and float(l0["loss"]) == float(l0["cls_loss"])


def test_two_runs_agree_and_the_weight_scales_the_rigid_part(dev, hip_lib):
    """two runs of the whole step agree bitwise; loss_and_grads at 2 w_rig_loss doubles the rigid part of dP bitwise"""
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine

    b, t = batch_on(dev, "main")
    runs = []
    for w in (1.0, 1.0, 2.0):
        eng = MatchingHeadRigidTrainEngine(head_on(dev), w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=w)
        loss_dict, d, grads, _ = engine_step(eng, t, b)
        rigid = eng.saved["rigid"]
        runs.append({"loss": loss_dict, "d": d, "grads": grads, "dP": [rigid.grad(k).clone() for k in range(2)], "ds": [m.clone() for m in eng.saved["ds_mat"]]})
    a, c, twice = runs
    worst = max(float((a["grads"][k] - c["grads"][k]).abs().max()) / float(a["grads"][k].abs().max()) for k in a["grads"])
    print(f"two runs: largest gradient difference / max {worst:.3g}, d_part_feats {float((a['d'] - c['d']).abs().max()):.3g}, "
          f"ds_mat equal {all(torch.equal(x, y) for x, y in zip(a['ds'], c['ds']))}, dP_rig equal {all(torch.equal(x, y) for x, y in zip(a['dP'], c['dP']))}")
    assert all(torch.equal(x, 2.0 * y) for x, y in zip(twice["dP"], a["dP"])) and float(a["dP"][0].abs().max()) > 0
    assert float(twice["loss"]["rig_loss"]) == float(a["loss"]["rig_loss"])
    assert all(torch.equal(x, y) for x, y in zip(a["dP"], c["dP"])) and float(a["loss"]["rig_loss"]) == float(c["loss"]["rig_loss"])
    assert torch.equal(a["d"], c["d"]) and all(torch.equal(a["grads"][k], c["grads"][k]) for k in a["grads"])


def test_chain_behind_the_cross_attention_layer(dev, hip_lib):
    """MatchingHeadLoss with part_pcs behind CrossAttentionFunction: the head's gradients are bitwise those of the engine called by
    hand on the same descriptors, and x.grad is the cross-attention engine's backward of the d_part_feats of that application"""
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine
    from pfpp_hip.matching_train import MatchingHeadLoss
    from pfpp_hip.matching_transformer import CrossAttentionLayer
    from pfpp_hip.matching_transformer_train import CrossAttentionFunction, CrossAttentionTrainEngine

    b, t = batch_on(dev, "main")
    spec = importlib.util.spec_from_file_location("matching_transformer_cases", Path(__file__).resolve().parent / "matching_transformer_cases.py")
    tf_cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tf_cases)
    layer = CrossAttentionLayer(128, 8)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tf_cases.cross_state_dict().items()}, strict=True)
    cross_eng = CrossAttentionTrainEngine(layer.to(dev))
    puz = np.full(2, t["part_feats"].shape[1], dtype=np.int64)           # the puzzles' point counts
    x = (t["part_feats"].reshape(-1, 128)).clone().requires_grad_(True)
    eng = MatchingHeadRigidTrainEngine(head_on(dev), w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=1.0)
    mid = CrossAttentionFunction.apply(x, cross_eng, puz)
    mid.retain_grad()
    loss = MatchingHeadLoss.apply(mid, eng, t["gt_pcs"], b["n_pcs"], b["part_valids"], None, t["critical_label"], t["part_pcs"])
    assert "rig_loss" in eng.last_loss_dict and float(eng.last_loss_dict["rig_loss"]) > 0
    loss.backward()
    chain = {k: p.grad.clone() for k, p in eng.params.items()}
    d_chain = mid.grad.clone()
    assert torch.equal(x.grad, cross_eng.backward(d_chain)) and float(x.grad.abs().max()) > 0
    by_hand = MatchingHeadRigidTrainEngine(head_on(dev), w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=1.0)
    ld, d = by_hand.loss_and_grads(mid.detach(), t["gt_pcs"], b["n_pcs"], b["part_valids"], critical_label=t["critical_label"], part_pcs=t["part_pcs"])
    worst = max(float((chain[k] - p.grad).abs().max()) / float(p.grad.abs().max()) for k, p in by_hand.params.items())
    print(f"chain: loss {float(loss.detach()):.6g} (rig {float(eng.last_loss_dict['rig_loss']):.4g}); against the engine by hand: largest gradient "
          f"difference / max {worst:.3g}, d_part_feats {float((d_chain.reshape(-1, 128) - d).abs().max()):.3g}")
    assert float(loss.detach()) == float(ld["loss"].float())
    assert all(torch.equal(chain[k], p.grad) for k, p in by_hand.params.items()) and torch.equal(d_chain.reshape(-1, 128), d)
