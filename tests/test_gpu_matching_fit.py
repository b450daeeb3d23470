"""GPU: fitting the matcher (pfpp_hip/matching_fit.py; pfpp_adam_multi in csrc/train_ops.hip, pfpp_match_val_metrics in
csrc/matching_train.hip).  Every test prints the figures it measured before it asserts.

Yardsticks.  pfpp_adam_multi: per-tensor pfpp_adamw on clones, bitwise, and once float64 Adam at the bar tests/test_gpu_matching_train.py
uses for its optimizer check (per step 2^-23 |p| + ADAM_REL lr, ADAM_REL = 8e-6: derived in that file's docstring).
pfpp_match_val_metrics: the float64 restatement of tests/matching_fit_cases.py on the same fp32 matrix.  The kernel takes the fp64 log of
every fp32 entry and adds the terms in fp64, a lane's chain of at most ceil(n / 16) ceil(n / 64) terms and then two trees: the sum of
the non-negative terms is off by at most (chain + 10) 2^-53 plus the logs' few ulp, below 1e-13 (relative) for every n here; 1e-13 is
also what tests/test_gpu_matching_train.py asks of pfpp_sinkhorn_train_fwd's fold of its fp64 row losses, the same sum with the same clamp.
MatcherOptimizer: the engines' own optimizer_step on an identical copy, bitwise."""
import numpy as np
import pytest
import torch

import matching_fit_cases as FC

pytestmark = pytest.mark.gpu

ADAM_REL = 8e-6          # tests/test_gpu_matching_train.py
LR = 1e-3


# ------------------------------------------------------------------------------------------------ pfpp_adam_multi
def _per_tensor(p, g, m, v, step, lr, wd, g_scale, betas=(0.9, 0.999), eps=1e-8):
    from pfpp_hip import _lib, ops
    from pfpp_hip.matching import _p

    _lib.check(_lib.load().pfpp_adamw(_p(p), _p(g), _p(m), _p(v), None, None, p.numel(), lr, betas[0], betas[1], eps, wd, 1.0 - betas[0] ** step,
                                      1.0 - betas[1] ** step, g_scale, ops._stream()), "pfpp_adamw")


def _run_both(dev, sizes, *, steps0=None, wd=0.0, g_scale=1.0, offset=0, n_steps=3, seed=0):
    """n_steps steps of adam_multi and of per-tensor pfpp_adamw on clones; offset: the parameters (and moments) are views that start
    `offset` floats into their allocations.  -> per step (multi, single) lists of (p, m, v) on the host"""
    from pfpp_hip.matching_fit import adam_multi

    p_np, g_np = FC.adam_case(sizes, seed, offset)
    steps0 = steps0 or [0] * len(sizes)
    view = lambda a: torch.from_numpy(a.copy()).to(dev)[offset:]
    state = {}
    for which in ("multi", "single"):
        state[which] = ([view(a) for a in p_np], [view(np.zeros_like(a)) for a in p_np], [view(np.zeros_like(a)) for a in p_np])
    out = []
    for s in range(n_steps):
        g = [torch.from_numpy(a).to(dev) for a in g_np[s]]
        g_before = [t.clone() for t in g]
        steps = [k + s + 1 for k in steps0]
        adam_multi(*state["multi"][:1], g, *state["multi"][1:], steps, lr=LR, weight_decay=wd, g_scale=g_scale)
        for i in range(len(sizes)):
            if sizes[i]:
                _per_tensor(state["single"][0][i], g[i], state["single"][1][i], state["single"][2][i], steps[i], LR, wd, g_scale)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(g, g_before)), "a gradient was written"
        out.append(tuple([[t.cpu().clone() for t in state[w][q]] for q in range(3)] for w in ("multi", "single")))
    return out, p_np, g_np


def _assert_bitwise(out, check_steps=(0, 2)):
    for s in check_steps:
        multi, single = out[s]
        for q, name in enumerate(("p", "m", "v")):
            bad = [i for i, (a, b) in enumerate(zip(multi[q], single[q])) if not torch.equal(a, b)]
            assert not bad, f"step {s + 1}: {name} of tensors {bad[:8]} differs from pfpp_adamw's"


@pytest.mark.parametrize("wd,g_scale", [(0.0, 1.0), (0.01, 1.0), (0.0, 0.5)])
def test_adam_multi_equals_pfpp_adamw_bitwise(dev, hip_lib, wd, g_scale):
    """sizes 1 .. 70,001 in one list (the last one 9 chunks), with a zero-length tensor between them; steps 1 and 3; the gradients stay"""
    sizes = list(FC.ADAM_SIZES[:4]) + [0] + list(FC.ADAM_SIZES[4:])
    out, _, _ = _run_both(dev, sizes, wd=wd, g_scale=g_scale)
    _assert_bitwise(out)
    assert not torch.equal(out[0][0][0][-1], out[2][0][0][-1])          # it did step


def test_adam_multi_capacities_views_and_step_counts(dev, hip_lib):
    """lists of capacity - 1, capacity and capacity + 1 tensors; a tensor spanning two launches (more chunks than a launch has
    blocks); parameters and moments that are views at an odd float offset; per-tensor step counts 1 and 11"""
    from pfpp_hip.matching_fit import CHUNK, MAX_BLOCKS, MAX_TENSORS, plan_adam_multi

    for n in (MAX_TENSORS - 1, MAX_TENSORS, MAX_TENSORS + 1):
        sizes = [1 + (37 * i) % 300 for i in range(n)]
        out, _, _ = _run_both(dev, sizes, offset=3, steps0=[0 if i % 2 else 10 for i in range(n)], seed=n)
        _assert_bitwise(out)
        assert len(plan_adam_multi(sizes)) == (2 if n > MAX_TENSORS else 1)
    long = MAX_BLOCKS * CHUNK + 4097                                         # 385 chunks behind a small tensor: cut after 383
    sizes = [5, long, 257]
    assert [nb for _, _, nb in plan_adam_multi(sizes)] == [MAX_BLOCKS, 3]
    out, _, _ = _run_both(dev, sizes, offset=1, seed=7)              # steps 1 and 3: at step 3 the continuation launch reads non-zero moments
    _assert_bitwise(out)


def test_adam_multi_no_ops_and_refusals(dev, hip_lib):
    from pfpp_hip import _lib
    from pfpp_hip.matching_fit import adam_multi

    adam_multi([], [], [], [], [], lr=LR)                                     # an empty list
    e = torch.empty(0, dtype=torch.float32, device=dev)
    adam_multi([e], [e], [e], [e], [1], lr=LR)                                # a zero-length tensor
    torch.cuda.synchronize()
    t = torch.zeros(4, dtype=torch.float32, device=dev)
    with pytest.raises(_lib.PfppError, match="bias corrections"):
        adam_multi([t], [t.clone()], [t.clone()], [t.clone()], [1], lr=LR, betas=(1.0, 0.999))
    assert float(t.abs().max()) == 0.0


def test_adam_multi_is_adam_in_float64(dev, hip_lib):
    """the arithmetic pfpp_adam_multi shares with pfpp_adamw is Adam's: three steps against float64 Adam on the same gradients, step
    counts starting at 0 and at 10, at test_gpu_matching_train.py's bar per step"""
    sizes, steps0 = [257, 4097], [0, 10]
    out, p_np, g_np = _run_both(dev, sizes, steps0=steps0)
    for i in range(len(sizes)):
        want = FC.adam64(p_np[i], [g_np[s][i] for s in range(3)], steps0[i], LR)
        for s in range(3):
            err = np.abs(out[s][0][0][i].numpy().astype(np.float64) - want[s])
            bar = (s + 1) * (2.0 ** -23 * np.abs(want[s]) + ADAM_REL * LR)
            print(f"tensor {i} step {s + 1}: largest error {err.max():.3g}, largest error / bar {(err / bar).max():.3g}")
            assert (err <= bar).all()


# ------------------------------------------------------------------------------------------------ pfpp_match_val_metrics
@pytest.mark.parametrize("n", FC.VAL_SIZES)
def test_val_metrics_against_float64(dev, hip_lib, n):
    from pfpp_hip.matching_fit import val_metrics

    ds, tgt, col = FC.val_case(n)
    want_loss, want_counts = FC.val_reference(ds, tgt, col)
    t = [torch.from_numpy(a).to(dev) for a in (ds, tgt, col)]
    runs = [tuple(x.cpu() for x in val_metrics(*t)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two runs differ"
    loss, counts = float(runs[0][0]), tuple(runs[0][1].tolist())
    e = abs(loss - want_loss) / max(abs(want_loss), 1e-300)
    print(f"n {n}: loss {loss:.12g} (float64 {want_loss:.12g}, relative {e:.3g}), counts {counts} (restatement {want_counts}), "
          f"{int((tgt < 0).sum())} rows without a target, {int((ds == 0).sum())} zeros, {int((ds == 1).sum())} ones")
    assert counts == want_counts
    assert e <= 1e-13 if want_loss else loss == 0.0


# ------------------------------------------------------------------------------------------------ MatcherValidator
BAR = 4.0          # x the reference's own fp32-against-fp64 deviation, as tests/golden/matching_train.npz's bars are taken


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("matching_fit")


@pytest.mark.parametrize("name", ["main", "one_owner"])
def test_validator_against_the_reference_validation_step(dev, hip_lib, fixture, name):
    """the reference's eval-mode forward + _loss_function behind given part_feats (tools/make_matching_fit_goldens.py), head weights of
    tests/matching_cases.py.  one_owner's second puzzle has critical points on one piece only: the masked-everything case.
    Bars: the three losses 4 x the fixture's own fp32-against-fp64 deviation (relative); the three mat_* ratios the same (the reference
    forms them in float32 in both runs, so the deviation and the bar are 0: equal to the last bit); the four cls_* ratios are float32
    quotients of integer counts against the float64 quotient of the same counts, 2^-24 relative, asked at 1e-6."""
    import matching_train_cases as TC
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_fit import MatcherValidator

    head = MatchingHead(tau=TC.TAU, max_iter=TC.MAX_ITER)
    head.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in TC.head_state_dict().items()}, strict=True)
    head = head.to(dev)
    b = TC.make_batch(name)
    d = {k: torch.from_numpy(b[k]).to(dev) for k in ("gt_pcs", "part_valids")}
    d.update(n_pcs=b["n_pcs"], part_pcs=d["gt_pcs"])
    val = MatcherValidator(None, head)
    out = val.step_from_feats(torch.from_numpy(b["part_feats"]).to(dev), d, critical_label=torch.from_numpy(b["critical_label"]).to(dev))
    key = f"val_{name}_"
    n_crit = fixture[key + "n_critical_pcs"]
    assert np.array_equal(val.saved["n_critical_pcs"].cpu().numpy(), n_crit)
    cols = np.concatenate([(c.cpu().numpy() if c is not None else np.full(int(n_crit[i].sum()), -1)) for i, c in enumerate(val.saved["cols"])])
    assert np.array_equal(cols, fixture[key + "cols"]), "the assignment's columns are not the reference's"
    assert val.saved["counts"].tolist() == fixture[key + "counts"].tolist()
    assert int(out["N_"]) == int(fixture[key + "N_"]) and out["batch_size"] == int(fixture[key + "batch_size"])
    if name == "one_owner":
        assert (n_crit[1] > 0).sum() == 1 and val.saved["cols"][1] is None
    failures = []
    for k in ("cls_loss", "mat_loss", "loss"):
        want, bar = float(fixture[key + k]), BAR * float(fixture[key + "dev_" + k])
        e = abs(float(out[k]) - want) / abs(want)
        print(f"{name} {k}: {float(out[k]):.9g} (reference float64 {want:.9g}), relative {e:.3g}, bar {bar:.3g}")
        failures += [k] if e > bar else []
    for k in ("mat_f1", "mat_precision", "mat_recall", "cls_acc", "cls_precision", "cls_recall", "cls_f1"):
        want = float(fixture[key + k])
        bar = BAR * float(fixture[key + "dev_" + k]) if k.startswith("mat_") else 1e-6
        e = abs(float(out[k]) - want)
        print(f"{name} {k}: {float(out[k]):.9g} (reference {want:.9g}), difference {e:.3g}, bar {bar:.3g}")
        failures += [k] if e > bar else []
    assert not failures, failures
    again = val.step_from_feats(torch.from_numpy(b["part_feats"]).to(dev), d, critical_label=torch.from_numpy(b["critical_label"]).to(dev))
    assert all(float(again[k]) == float(out[k]) for k in out if k != "batch_size"), "two runs differ"
    mean = MatcherValidator.epoch_end([dict(out), dict(again, batch_size=6)])
    assert mean["val/loss"] == float(out["loss"]) and set(mean) == {f"val/{k}" for k in out if k != "batch_size"}


# ------------------------------------------------------------------------------------------------ MatcherOptimizer
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import matching_dataset_cases as MC

    return MC.make_tree(tmp_path_factory.mktemp("meshes"))


def _config(tree, out, extra=()):
    from pfpp_hip.matching_fit import load_config

    return load_config(None, ["DATA.DATA_DIR", str(tree), "DATA.NUM_PC_POINTS", "64", "DATA.MIN_PART_POINT", "8", "DATA.MAX_NUM_PART", "8",
                              "DATA.FRACTURE_LABEL_THRESHOLD", "0.25", "BATCH_SIZE", "2", "NUM_WORKERS", "0", "TRAIN.NUM_EPOCHS", "3",
                              "TRAIN.VAL_EVERY", "1", "MODEL.LOSS.mat_epoch", "0", "MODEL.LOSS.rig_epoch", "1", "OUTPUT_PATH", str(out),
                              "MODEL_SAVE_PATH", str(out / "model_save"), *extra])


def test_matcher_optimizer_equals_the_engines_own_steps_bitwise(dev, hip_lib, tree, tmp_path):
    """two identical model copies, three steps on one batch; the second a classifier-phase step (w_mat_loss 0), so the affinity
    parameters skip a step and their count stays behind.  Copy A steps through the four engines' optimizer_step (175 launches), copy B
    through MatcherOptimizer.  The gradients are computed once per step, on A, and handed to B as clones: a few bias gradients of the
    engines end in float atomics (pfpp_colsum) and two backward passes need not agree in their last bit, which is not this test's
    subject.  All 175 parameters, both moments and the step counts must be equal; then the roles swap for one step (state written by
    one path is continued by the other)."""
    from pfpp_hip.matching import DescriptorNetwork, MatchingHead
    from pfpp_hip.matching_encoder_train import DescriptorTrainEngine
    from pfpp_hip.matching_fit import MatcherOptimizer, MatcherTrainer
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine

    tr = MatcherTrainer(_config(tree, tmp_path), device=dev)
    a_desc, a_head, opt_a = tr.descriptor_engine, tr.head_engine, tr.optimizer
    net_b, head_b = DescriptorNetwork().to(dev), MatchingHead().to(dev)
    net_b.load_state_dict(tr.net.state_dict()); head_b.load_state_dict(tr.head.state_dict())
    b_desc, b_head = DescriptorTrainEngine(net_b), MatchingHeadRigidTrainEngine(head_b, w_cls_loss=1.0, w_mat_loss=1.0)
    opt_b = MatcherOptimizer(b_desc, b_head)
    assert opt_a.names == opt_b.names and len(opt_b.names) == 175
    tr.train_loader.set_epoch(0)
    batch = next(iter(tr.train_loader))
    from pfpp_hip.matching_train import MatchingHeadLoss

    def compare(what):
        bad = []
        for name in opt_a.names:
            (ea, ka), (eb, kb) = opt_a.entries[name], opt_b.entries[name]
            if not torch.equal(ea.params[ka].data, eb.params[kb].data):
                bad.append(name + " (parameter)")
            sa, sb = ea.state.get(ka), eb.state.get(kb)
            if (sa is None) != (sb is None) or (sa is not None and (sa[2] != sb[2] or not torch.equal(sa[0], sb[0]) or not torch.equal(sa[1], sb[1]))):
                bad.append(name + " (state)")
        assert not bad, (what, bad[:6])

    for step, (w_mat, own_on_a) in enumerate([(1.0, True), (0.0, True), (1.0, True), (1.0, False)]):
        a_head.w_mat_loss = w_mat
        feats = a_desc.forward(batch["part_pcs"], batch["n_pcs"], batch["part_valids"], seed=step)
        loss = MatchingHeadLoss.apply(feats, a_head, batch["gt_pcs"], batch["n_pcs"], batch["part_valids"], batch["critical_label_thresholds"], None,
                                      batch["part_pcs"])
        loss.backward()
        for name in opt_a.names:
            (ea, ka), (eb, kb) = opt_a.entries[name], opt_b.entries[name]
            g = ea.params[ka].grad
            eb.params[kb].grad = None if g is None else g.clone()
        # the running statistics moved on A only; B's forward is never run, its buffers are not compared
        if own_on_a:
            a_desc.optimizer_step(lr=LR); a_head.optimizer_step(lr=LR); opt_b.step(LR)
        else:
            opt_a.step(LR); b_desc.optimizer_step(lr=LR); b_head.optimizer_step(lr=LR)
        torch.cuda.synchronize()
        compare(f"step {step + 1}")
    steps = {name: opt_b.entries[name][0].state[opt_b.entries[name][1]][2] for name in opt_b.names}
    assert steps["affinity_layer.A"] == 3 == steps["affinity_extractor.2.weight"] and steps["pc_classifier.2.weight"] == 4 == steps["encoder.conv1.bias"]
    print(f"MatcherOptimizer: {opt_b.last_launches} launches for 175 tensors; step counts {sorted(set(steps.values()))}")
    assert opt_b.last_launches <= 7
    sd = opt_b.state_dict(LR)
    assert sorted(sd["state"]) == list(range(175)) and float(sd["state"][opt_b.names.index("affinity_layer.A")]["step"]) == 3.0
    opt_a.load_state_dict(sd)
    compare("after load_state_dict")


# ------------------------------------------------------------------------------------------------ the loop
def _read_log(path):
    import json

    return [json.loads(line) for line in open(path)]


def test_fit_loop_phases_checkpoints_resume_and_command_line(dev, hip_lib, tree, tmp_path):
    """3 epochs, validation every epoch, mat_epoch 0 and rig_epoch 1: epoch 0 is the classifier phase, epoch 1 adds the matching loss,
    epoch 2 the rigid term.  One run in this process; then `python -m pfpp_hip.train_matching` in a fresh child for 2 epochs and in another
    that resumes from last.ckpt for the third: the final state_dict, the moments and the validation loss_dict must equal the single run's
    bit for bit.  (A few bias gradients of the engines end in pfpp_colsum's float atomics, one per block of 64 rows.  A batch here has
    128 rows, so a column receives two addends and their order cannot matter; at the reference's 5,000 points per puzzle it can, in
    the last bit of those gradients.)"""
    import subprocess
    import sys

    import matching_dataset_cases as MC
    from pfpp_hip.matching import DescriptorNetwork, MatchingHead
    from pfpp_hip.matching_eval import MatchingEvaluator
    from pfpp_hip.matching_fit import MatcherTrainer, cosine_warmup_lr, fit

    one = tmp_path / "one"
    cfg = _config(tree, one)
    tr = fit(cfg, device=dev)
    log = _read_log(tr.log_path)
    epochs = [r for r in log if r["kind"] == "epoch"]
    steps = [r for r in log if r["kind"] == "step"]
    assert [r["epoch"] for r in epochs] == [0, 1, 2] and len(steps) == tr.global_step == 3 * len(tr.train_loader) > 0
    assert [r["lr"] for r in epochs] == [cosine_warmup_lr(e, 3, 1e-3, 100.0, 0.0) for e in range(3)]
    assert [(r["w_mat_loss"], r["w_rig_loss"]) for r in epochs] == [(1.0, 0.0), (1.0, 1.0), (1.0, 1.0)]
    per_epoch = [[s for s in steps if s["epoch"] == e] for e in range(3)]
    assert "train/mat_loss" not in per_epoch[0][0] and "train/mat_loss" in per_epoch[1][0] and "train/rig_loss" in per_epoch[2][0]
    for r in log:
        bad = [k for k, v in r.items() if isinstance(v, float) and not np.isfinite(v)]
        assert not bad, (r["kind"], r["epoch"], bad)
    # validation runs before the epoch's weight switch, as Lightning runs it before training_epoch_end: none at epoch == rig_epoch yet
    assert all("val/loss" in r and "val/mat_f1" in r for r in epochs) and "val/rig_loss" not in epochs[1] and "val/rig_loss" in epochs[2]
    save = one / "model_save"
    assert sorted(p.name for p in save.iterdir()) == ["last.ckpt", "model_epoch=000.ckpt", "model_epoch=001.ckpt", "model_epoch=002.ckpt"]
    last = str(save / "last.ckpt")
    net, head = DescriptorNetwork.from_checkpoint(last).to(dev), MatchingHead.from_checkpoint(last).to(dev)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(net.state_dict().values(), tr.net.state_dict().values()))
    # the test pass on one validation batch with the trained weights
    tr.val_loader.set_epoch(0)
    d = next(iter(tr.val_loader))
    out = head(net(d["part_pcs"], d["n_pcs"], d["part_valids"], seed=0), d["n_pcs"], d["part_valids"])
    ev = MatchingEvaluator(n_hyp=2000, seed=0)
    data = dict(d, n_critical_pcs=out.n_critical_pcs.cpu().numpy(), critical_pcs_idx=torch.stack(list(out.critical_pcs_idx)))
    metrics = ev.transformation_metrics(data, {"perm_mat": list(out.perm_mat)})
    flat = {k: np.asarray(metrics[k].detach().cpu() if torch.is_tensor(metrics[k]) else metrics[k], dtype=np.float64) for k in ev.KEYS}
    print("evaluator on the trained checkpoint:", {k: v.tolist() for k, v in flat.items()})
    assert flat and all(np.isfinite(v).all() for v in flat.values())

    # ---- the command line: 2 epochs in one child, the third in another that resumes
    two = tmp_path / "two"
    import os

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(MC.ROOT / "puzzlefusion-plusplus_amd"), os.environ.get("PYTHONPATH", "")]))
    args = [sys.executable, "-m", "pfpp_hip.train_matching"]
    over = ["DATA.DATA_DIR", str(tree), "DATA.NUM_PC_POINTS", "64", "DATA.MIN_PART_POINT", "8", "DATA.MAX_NUM_PART", "8", "DATA.FRACTURE_LABEL_THRESHOLD",
            "0.25", "BATCH_SIZE", "2", "NUM_WORKERS", "0", "TRAIN.NUM_EPOCHS", "3", "TRAIN.VAL_EVERY", "1", "MODEL.LOSS.mat_epoch", "0",
            "MODEL.LOSS.rig_epoch", "1", "OUTPUT_PATH", str(two), "MODEL_SAVE_PATH", str(two / "model_save")]
    for extra in (["--max-epochs", "2"], []):
        r = subprocess.run(args + extra + over, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(p.name for p in (two / "model_save").iterdir()) == sorted(p.name for p in save.iterdir())
    a = torch.load(last, map_location="cpu", weights_only=True)
    b = torch.load(str(two / "model_save" / "last.ckpt"), map_location="cpu", weights_only=True)
    assert a["epoch"] == b["epoch"] == 2 and a["global_step"] == b["global_step"]
    diff = {k: float((a["state_dict"][k].double() - b["state_dict"][k].double()).abs().max()) for k in a["state_dict"]
            if not torch.equal(a["state_dict"][k], b["state_dict"][k])}
    sa, sb = a["optimizer_states"][0]["state"], b["optimizer_states"][0]["state"]
    diff_m = [i for i in sa if not (torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"])
                                    and float(sa[i]["step"]) == float(sb[i]["step"]))]
    log2 = [r for r in _read_log(two / "train_log.jsonl") if r["kind"] == "epoch"]
    val_a = {k: v for k, v in epochs[2].items() if k.startswith("val/")}
    val_b = {k: v for k, v in log2[2].items() if k.startswith("val/")}
    print(f"single run against 2 + 1 epochs in two children: {len(diff)} of {len(a['state_dict'])} state_dict tensors differ "
          f"(largest difference {max(diff.values(), default=0.0):.3g}: {sorted(diff, key=diff.get)[-3:]}), {len(diff_m)} of {len(sa)} optimizer states differ; "
          f"validation {val_a} against {val_b}")
    assert [r["epoch"] for r in log2] == [0, 1, 2] and sorted(sa) == sorted(sb)
    assert not diff and not diff_m and val_a == val_b
