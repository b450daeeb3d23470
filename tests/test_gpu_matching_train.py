"""GPU: training of the matcher's head (csrc/matching_train.hip, pfpp_hip/matching_train.py) against the float64 reference of
tests/matching_train_cases.py, which tests/test_matching_train_host.py pins to the reference's own code (tests/golden/matching_train.npz).
Every test prints the figures it measured before it asserts.

Bars.  The bar of a tensor is 4 x the deviation of the reference's own fp32 run from its float64 run on the same
inputs, as the fixture records it (`*_dev_*`): max |fp32 - fp64| for ds_mat, relative for a loss, and max |fp32 - fp64| / max |fp64|
for a gradient, each per case (size and step count).  The loss of a Sinkhorn case is compared through its rows: the kernel hands out
the per-row losses it folds, and their bar is 4 x the reference's deviation of the same vector (max over the rows / largest row: not
the single draw that the deviation of one number is); the reported loss must be the fp64 sum of those rows (1e-13) and is printed
against float64 (it cannot be off by more than the rows' bar allows: n bar max_row / loss).
The whole step compares the gradients of each of two consecutive steps with the float64 reference evaluated at the parameters,
running statistics and ReLU sign patterns the GPU had at that step, and the two Adam updates with float64 Adam on the GPU's own
gradients (Adam's first steps are lr g / (|g| + eps): on an element whose gradient is within its error of zero they amplify that
error to the full lr, so parameters after a step are only comparable through the same gradients).  The Adam bar per step is
2^-23 |p| + ADAM_REL lr: the parameter is rounded to fp32 once per step, and the update, at most lr, is formed in fp32 from fp32
hyper-parameters, as pfpp_adamw's ABI takes them: 1 - fl32(0.999) is 1.29e-5 (relative) below 0.001 and reaches the update through the
square root of the second moment as 6.45e-6, 1 - fl32(0.9) adds 2.4e-7, the square root, the divisions and the bias corrections about
1e-6: ADAM_REL = 8e-6.  MASK_MARGIN: a ReLU whose sign differs from float64's must have a pre-activation this close to 0; the
BatchNorm outputs are O(1) and carry a few fp32 roundings of that size."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("matching_train_cases", Path(__file__).resolve().parent / "matching_train_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

BAR = 4.0
MASK_MARGIN = 2e-5
ADAM_REL = 8e-6
LR = 1e-3


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("matching_train")


def head_on(dev, sd=None):
    from pfpp_hip.matching import MatchingHead

    head = MatchingHead()
    head.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in (sd or cases.head_state_dict()).items()}, strict=True)
    return head.to(dev)


def batch_on(dev, name):
    b = cases.make_batch(name)
    return b, {k: torch.from_numpy(b[k]).to(dev) for k in ("part_feats", "gt_pcs", "critical_label", "thresholds")}


# ------------------------------------------------------------------------------------------------ Sinkhorn: forward, loss, backward
@pytest.mark.parametrize("n", cases.SINKHORN_SIZES)
def test_sinkhorn_train_forward_loss_backward(dev, hip_lib, fixture, n):
    """n = 3 (under a wave), 65 (one past the 64-row and 64-column blocks), 257 (one past four columns per lane), 1033 (ragged, many
    blocks); max_iter 1, 2, 7, 20 (the last step a row step or a column step); a row stride that is no multiple of anything, with
    poison behind every row; rows with target -1; two runs bitwise equal"""
    from pfpp_hip.matching_train import sinkhorn_train_bwd, sinkhorn_train_fwd

    s_np, tgt_np = cases.sinkhorn_case(n)
    assert (tgt_np == -1).any() and (tgt_np >= 0).any()
    buf = torch.full((n, n + 5), 3.0e4, dtype=torch.float32, device=dev)
    buf[:, :n] = torch.from_numpy(s_np).to(dev)
    s, tgt = buf[:, :n], torch.from_numpy(tgt_np).to(dev)
    g = 0.37
    for it in cases.SINKHORN_ITERS:
        bars = {q: BAR * float(fixture[f"sk_n{n}_t{it}_dev_{q}"]) for q in ("ds", "row_loss", "grad")}
        P64, loss64, grad64 = cases.sinkhorn_loss_and_grad(s_np, tgt_np, max_iter=it, g=g)
        rows64 = cases.perm_loss_rows(P64, tgt_np)
        runs = []
        for _ in range(2):
            rows = torch.empty(n, dtype=torch.float64, device=dev)
            ds_mat, loss, pots = sinkhorn_train_fwd(s, tgt, tau=cases.TAU, max_iter=it, row_loss=rows)
            ds = sinkhorn_train_bwd(s, tgt, pots, ds_mat, g=g, tau=cases.TAU, max_iter=it)
            runs.append((ds_mat.cpu(), loss.cpu(), ds.cpu().contiguous(), rows.cpu()))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), f"n {n}, {it} steps: two runs differ"
        ds_mat, loss, ds, rows = runs[0]
        e_ds = float((ds_mat.double() - P64).abs().max())
        e_rows = float((rows - rows64).abs().max()) / float(rows64.abs().max())
        e_fold = abs(float(loss) - float(rows.sum())) / float(rows.sum())
        e_loss = abs(float(loss) - float(loss64)) / abs(float(loss64))
        loss_bound = n * bars["row_loss"] * float(rows64.abs().max()) / float(loss64) + 1e-13      # what the rows' bar allows their sum
        e_grad = float((ds.double() - grad64).abs().max()) / float(grad64.abs().max())
        print(f"n {n} steps {it}: ds_mat {e_ds:.3g} (bar {bars['ds']:.3g}), row losses / max {e_rows:.3g} (bar {bars['row_loss']:.3g}), "
              f"loss {e_loss:.3g} (fold of the rows {e_fold:.3g}), ds / max {e_grad:.3g} (bar {bars['grad']:.3g})")
        assert torch.isfinite(ds).all() and e_ds <= bars["ds"] and e_rows <= bars["row_loss"] and e_grad <= bars["grad"], (n, it)
        assert e_fold <= 1e-13 and e_loss <= loss_bound, (n, it)
    assert float(buf[:, n:].min()) == 3.0e4 == float(buf[:, n:].max())


# ------------------------------------------------------------------------------------------------ targets
def test_gt_targets_equal_the_float64_argmin(dev, hip_lib):
    """four puzzles in one launch: 1300 rows over five pieces of which one has none (more than one LDS tile of columns, several
    workgroups of rows), 40 rows owned by a single piece (all -1), none, and 3 rows; an exact tie goes to the lowest column"""
    from pfpp_hip.matching_train import gt_targets

    rng = np.random.default_rng(9)          # a draw without a natural near-tie: the closest pair of candidates of any row is 5.7e-6 apart
    spec =[[400, 350, 0, 300, 250], [40], [], [1, 1, 1]]
    pts, piece, off, want, gaps = [], [], [0], [], []
    for b, counts in enumerate(spec):
        n = sum(counts)
        p = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        pc = np.repeat(np.arange(len(counts)), counts)
        if b == 0:
            p[700] = p[900] = p[5] + np.float32(0.001)          # rows 700 (piece 1) and 900 (piece 3): the same point next to row 5 (piece 0)
        t, gap = cases.gt_targets(torch.from_numpy(p).double(), pc, return_gap=True)
        pts.append(p); piece.append(pc + 10 * b); off.append(off[-1] + n); want.append(t); gaps.append(gap)
    pts, want, gaps = np.concatenate(pts), np.concatenate(want), np.concatenate(gaps)
    # the rows as a scattered subset of a larger cloud, in order
    N = 4000
    src = np.sort(rng.permutation(N)[:off[-1]])
    cloud = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    cloud[src] = pts
    got = gt_targets(torch.from_numpy(cloud).to(dev), torch.from_numpy(src).to(dev), torch.from_numpy(np.concatenate(piece).astype(np.int32)).to(dev),
                     torch.tensor(off, dtype=torch.int64, device=dev), max(sum(c) for c in spec)).cpu().numpy()
    # coordinates in [0, 1]: -2 a.b + |a|^2 + |b|^2 has terms up to 6 and three roundings, 7e-7 per distance; a row whose two nearest
    # candidates are closer together than 2e-6 is a near-tie.  The inputs have none but the exact tie built at row 5
    near = (gaps < 2e-6) & (want >= 0)
    print(f"rows {len(want)}, near-ties {int(near.sum())} (the exact tie built at row 5 of puzzle 0), -1 rows {int((want < 0).sum())}")
    assert near.sum() == 1 and near[5]
    assert np.array_equal(got[~near], want[~near])
    assert got[5] == 700 and (got[off[1]:off[2]] == -1).all() and (got[off[3]:] >= 0).all()


# ------------------------------------------------------------------------------------------------ the small kernels on their own
def test_normalize_halves_bwd_and_cls_bce(dev, hip_lib):
    """F.normalize's backward on 37 rows (a ragged last workgroup) with an all-zero half (the eps branch) against float64 autograd;
    the classifier loss over 300,001 strided logits (the grid-stride path: more than 1024 workgroups' worth) against float64"""
    from pfpp_hip.matching_train import cls_bce, normalize_halves_bwd

    gen = torch.Generator().manual_seed(0)
    x = torch.randn(37, 512, generator=gen) * torch.logspace(-3, 2, 37)[:, None]
    x[5, 256:] = 0
    dy = torch.randn(37, 512, generator=gen)
    x64 = x.double().requires_grad_(True)
    y = torch.cat([torch.nn.functional.normalize(x64[:, :256], dim=-1), torch.nn.functional.normalize(x64[:, 256:], dim=-1)], -1)
    y.backward(dy.double())
    got = normalize_halves_bwd(x.to(dev), dy.to(dev)).cpu().double()
    ok = torch.ones(37, 512, dtype=torch.bool)
    ok[5, 256:] = False                                      # dy / 1e-12 there: compared relative to itself
    err = float(((got - x64.grad).abs() / x64.grad.abs().amax(1, keepdim=True))[ok].max())
    err0 = float(((got - x64.grad).abs() / x64.grad.abs().clamp_min(1e-300))[~ok].max())
    print(f"normalize_halves_bwd: {err:.3g} of the row's largest entry; eps branch {err0:.3g} relative")
    assert err <= 2e-6 and err0 <= 1e-6

    N = 300_001
    logits = torch.randn(N, 3, generator=gen) * 4
    labels = (torch.rand(N, generator=gen) < 0.3).to(torch.uint8)
    loss, dlogit, counts = cls_bce(logits.to(dev)[:, 1], labels.to(dev), g=0.5)
    l64 = logits[:, 1].double()
    want = torch.nn.functional.binary_cross_entropy_with_logits(l64, labels.double())
    dwant = (torch.sigmoid(l64) - labels.double()) * 0.5 / N
    pred = (torch.sigmoid(logits[:, 1]) > 0.5)
    lab = labels.bool()
    cw = [int((pred & lab).sum()), int((pred & ~lab).sum()), int((~pred & ~lab).sum()), int((~pred & lab).sum())]
    e_loss = abs(float(loss) - float(want)) / float(want)
    e_d = float((dlogit.cpu().double() - dwant).abs().max() / dwant.abs().max())
    print(f"cls_bce: loss {e_loss:.3g}, dlogit {e_d:.3g}, counts {counts.tolist()} (float64 {cw})")
    near = int(((torch.sigmoid(l64) - 0.5).abs() < 1e-6).sum())
    assert e_loss <= 1e-7 and e_d <= 1e-6 and sum(abs(a - b) for a, b in zip(counts.tolist(), cw)) <= 2 * near and sum(counts.tolist()) == N


# ------------------------------------------------------------------------------------------------ the whole step
def engine_step(dev, eng, t, b, **kw):
    loss_dict, d = eng.loss_and_grads(t["part_feats"], t["gt_pcs"], b["n_pcs"], b["part_valids"], critical_label=t["critical_label"], **kw)
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().double().clone()) for k, p in eng.params.items()}
    masks = (eng.saved["h_cls"].cpu() > 0, eng.saved["h_aff"].cpu() > 0 if "h_aff" in eng.saved else None)
    return loss_dict, d.cpu().double(), grads, masks


def state64(head):
    return {k: v.detach().cpu().double().clone() for k, v in head.state_dict().items()}


def check_step(fixture, name, key, got, ref, masks, missing_as_zeros=False):
    """one step's loss, gradients, d_part_feats and running statistics against the float64 run `ref` that was fed the GPU's masks;
    the bars are 4 x the fixture's deviations of case `key`.  A parameter the reference gives no gradient has none here either
    (zeros with missing_as_zeros: the batch without critical points)"""
    loss_dict, d, grads, buffers = got
    dev_of = lambda q: BAR * float(fixture[f"{key}_dev_{q}"])
    for nm, pre, mask in (("classifier", ref["pre_cls"], masks[0]), ("extractor", ref["pre_aff"], masks[1])):
        if pre is not None:
            diff = (pre > 0) != mask
            margin = float(pre[diff].abs().max()) if diff.any() else 0.0
            print(f"{name} {nm} ReLU: {int(diff.sum())} of {diff.numel()} signs differ from float64's, largest |pre-activation| there {margin:.3g}")
            assert margin <= MASK_MARGIN
    e = abs(float(loss_dict["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    print(f"{name} loss {float(loss_dict['loss']):.7g}: {e:.3g} (bar {dev_of('loss'):.3g})")
    assert e <= dev_of("loss")
    for k in cases.PARAMS:
        if ref["grads"][k] is None:
            assert (grads[k] is not None and float(grads[k].abs().max()) == 0.0) if missing_as_zeros else grads[k] is None, k
            continue
        e = float((grads[k] - ref["grads"][k].reshape(grads[k].shape)).abs().max()) / float(ref["grads"][k].abs().max())
        print(f"{name} grad {k}: {e:.3g} (bar {dev_of('grad_' + k):.3g})")
        assert e <= dev_of("grad_" + k), k
    e = float((d - ref["d_part_feats"]).abs().max()) / float(ref["d_part_feats"].abs().max())
    print(f"{name} d_part_feats: {e:.3g} (bar {dev_of('d_part_feats'):.3g})")
    assert e <= dev_of("d_part_feats")
    for k, want in ref["buffers"].items():
        e = float((buffers[k] - want).abs().max()) / float(want.abs().max())
        print(f"{name} {k}: {e:.3g} (bar {dev_of(k):.3g})")
        assert e <= dev_of(k), k


@pytest.mark.parametrize("name", list(cases.BATCHES))
def test_whole_step_against_float64(dev, hip_lib, fixture, name):
    """two puzzles of unequal N' (the zero rows of the padded critical_feats count in the extractor's BatchNorm), a piece without
    critical points; a puzzle whose critical points one piece owns; a puzzle without any.  Two steps: loss, metrics, targets, every
    gradient, d_part_feats, running statistics, and the parameters after each Adam step"""
    from pfpp_hip.matching_train import MatchingHeadTrainEngine

    head = head_on(dev)
    eng = MatchingHeadTrainEngine(head, w_cls_loss=1.0, w_mat_loss=1.0)
    b, t = batch_on(dev, name)
    sd = state64(head)
    gpu_grads = []
    for step in (1, 2):
        loss_dict, d, grads, masks = engine_step(dev, eng, t, b)
        after = state64(head)
        ref = cases.head_train_reference(sd, b, relu_masks=masks)
        check_step(fixture, f"{name} step {step}", name, (loss_dict, d, grads, after), ref, masks)
        if step == 1:
            assert abs(float(ref["loss"]) - float(fixture[f"{name}_loss"])) <= 1e-6 * float(ref["loss"])      # the masks moved nothing that matters
            tp, fp, tn, fn = (float(c) for c in ref["counts"])
            want = [(tp + tn) / (tp + fp + tn + fn), tp / (tp + fp), tp / (tp + fn), 2 * tp / (2 * tp + fp + fn)]
            got = [float(loss_dict[k]) for k in ("cls_acc", "cls_precision", "cls_recall", "cls_f1")]
            assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)
            assert int(loss_dict["N_"]) == ref["N_"] == int(fixture[f"{name}_N_"]) and loss_dict["batch_size"] == 2
            assert np.array_equal(eng.saved["targets"].cpu().numpy(), fixture[f"{name}_targets"])
            assert abs(float(loss_dict["mat_loss"]) - float(ref["mat_loss"])) <= BAR * float(fixture[f"{name}_dev_mat_loss"]) * float(ref["mat_loss"])
        assert int(after["pc_classifier.0.num_batches_tracked"]) == step == int(after["affinity_extractor.0.num_batches_tracked"])
        gpu_grads.append(grads)
        eng.optimizer_step(lr=LR)
        sd = state64(head)
        want_p = cases.adam_steps({k: state64(head_on(dev))[k] for k in cases.PARAMS}, gpu_grads, lr=LR)[-1]
        for k in cases.PARAMS:
            err = (sd[k] - want_p[k].reshape(sd[k].shape)).abs()
            bar = step * (2.0 ** -23 * want_p[k].reshape(sd[k].shape).abs() + ADAM_REL * LR)
            print(f"{name} after Adam step {step}, {k}: largest error {float(err.max()):.3g}, largest error / bar {float((err / bar).max()):.3g}")
            assert (err <= bar).all(), k


def test_classifier_phase(dev, hip_lib, fixture):
    """w_mat_loss = 0: the loss is the classifier's alone (unweighted), the extractor and the affinity get no gradient, their
    statistics and parameters stay, Adam leaves them alone"""
    from pfpp_hip.matching_train import MatchingHeadTrainEngine

    head = head_on(dev)
    eng = MatchingHeadTrainEngine(head, w_cls_loss=0.25, w_mat_loss=0.0)
    b, t = batch_on(dev, "main")
    sd = state64(head)
    loss_dict, d, grads, masks = engine_step(dev, eng, t, b)
    ref = cases.head_train_reference(sd, b, w_cls=0.25, w_mat=0.0, relu_masks=masks)
    check_step(fixture, "classifier phase", "main_phase0", (loss_dict, d, grads, state64(head)), ref, masks)
    assert "mat_loss" not in loss_dict and float(loss_dict["loss"]) == float(loss_dict["cls_loss"])
    eng.optimizer_step(lr=LR)
    after = state64(head)
    for k in sd:
        same = torch.equal(after[k], sd[k])
        assert same == (not k.startswith("pc_classifier")), k


def test_batch_without_critical_points(dev, hip_lib, fixture):
    """no puzzle has a critical point: the reference divides 0 by 0; here mat_loss is 0, the extractor's and the affinity's gradients are
    zeros, their statistics stay, and the classifier's step is the usual one: it is held to 4 x the deviations of the reference's
    classifier phase on the same batch and labels (`nolabel_phase0` in the fixture), the part of the step the reference defines there"""
    from pfpp_hip.matching_train import MatchingHeadTrainEngine

    head = head_on(dev)
    eng = MatchingHeadTrainEngine(head, w_cls_loss=1.0, w_mat_loss=1.0)
    b = cases.make_batch_without_critical_points()
    t = {k: torch.from_numpy(b[k]).to(dev) for k in ("part_feats", "gt_pcs", "critical_label")}
    sd = state64(head)
    loss_dict, d, grads, masks = engine_step(dev, eng, t, b)
    ref = cases.head_train_reference(sd, b, w_mat=0.0, relu_masks=masks)
    assert float(loss_dict["mat_loss"]) == 0.0 and int(loss_dict["N_"]) == 0 and torch.isfinite(d).all()
    check_step(fixture, "no critical points", "nolabel_phase0", (loss_dict, d, grads, state64(head)), ref, masks, missing_as_zeros=True)
    after = state64(head)
    assert torch.equal(after["affinity_extractor.0.running_var"], sd["affinity_extractor.0.running_var"])
    assert int(after["affinity_extractor.0.num_batches_tracked"]) == 0 and int(after["pc_classifier.0.num_batches_tracked"]) == 1


def test_loss_function_and_label_paths_equal_loss_and_grads(dev, hip_lib):
    """MatchingHeadLoss through loss.backward(), behind an eager stand-in for the descriptor network, hands over loss_and_grads'
    d_part_feats (times the incoming gradient) and leaves the same parameter gradients; labels computed from thresholds by
    fracture_labels give what the same labels give when passed in; a ragged list input equals the stacked one"""
    from pfpp_hip.matching import fracture_labels
    from pfpp_hip.matching_train import MatchingHeadLoss, MatchingHeadTrainEngine

    b, t = batch_on(dev, "main")
    # two runs of one step agree to the order of the BatchNorm reductions: far below any bar above
    near = lambda a, c: float((a - c).abs().max()) <= 2e-6 * float(c.abs().max())

    eng2 = MatchingHeadTrainEngine(head_on(dev), w_cls_loss=1.0, w_mat_loss=1.0)
    raw = t["part_feats"].clone().requires_grad_(True)
    scale = torch.tensor(1.5, device=dev, requires_grad=True)
    loss = MatchingHeadLoss.apply(raw * scale, eng2, t["gt_pcs"], b["n_pcs"], b["part_valids"], None, t["critical_label"])
    (2.0 * loss).backward(retain_graph=True)
    g15 = {k: p.grad.clone() for k, p in eng2.params.items()}
    first = raw.grad.clone()
    raw.grad = scale.grad = None
    (2.0 * loss).backward()                   # a second backward over the retained graph sets the same gradients, not scaled twice
    assert torch.equal(raw.grad, first) and all(torch.equal(g15[k], p.grad) for k, p in eng2.params.items())
    d15 = eng2.loss_and_grads(t["part_feats"] * 1.5, t["gt_pcs"], b["n_pcs"], b["part_valids"], critical_label=t["critical_label"])[1]
    assert loss.dtype == torch.float32 and float(loss) == float(eng2.last_loss_dict["loss"].float())
    assert near(raw.grad.reshape(-1, 128), 2.0 * d15 * 1.5)
    assert all(near(g15[k], 2.0 * p.grad) for k, p in eng2.params.items())
    assert abs(float(scale.grad) - float((2.0 * d15 * t["part_feats"].reshape(-1, 128)).sum())) <= 1e-4 * float((d15 * t["part_feats"].reshape(-1, 128)).abs().sum())

    eng3 = MatchingHeadTrainEngine(head_on(dev), w_cls_loss=1.0, w_mat_loss=1.0)
    labels = fracture_labels(t["gt_pcs"], b["n_pcs"], t["thresholds"])
    assert 0 < int(labels.sum()) < labels.numel()
    ld_a, d_a = eng3.loss_and_grads(t["part_feats"], t["gt_pcs"], b["n_pcs"], b["part_valids"], critical_label_thresholds=t["thresholds"])
    ga = {k: p.grad.clone() for k, p in eng3.params.items()}
    eng4 = MatchingHeadTrainEngine(head_on(dev), w_cls_loss=1.0, w_mat_loss=1.0)
    ld_b, d_b = eng4.loss_and_grads(list(t["part_feats"]), list(t["gt_pcs"]), b["n_pcs"], b["part_valids"], critical_label=list(labels))
    assert abs(float(ld_a["loss"]) - float(ld_b["loss"])) <= 2e-7 * float(ld_b["loss"]) and near(d_a, d_b)
    assert all(near(ga[k], p.grad) for k, p in eng4.params.items())
