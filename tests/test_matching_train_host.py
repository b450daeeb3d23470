"""CPU: the reference of record of the matcher head's training step.  tests/matching_train_cases.py's float64 restatement against
tests/golden/matching_train.npz (the reference's own code under autograd in float64, tools/make_matching_train_goldens.py), the
closed-form Sinkhorn backward the kernels run against autograd, and the argument checks of the new entry points and of the engine
(all of which return before a launch).

Two of the tests here run no product code and therefore pass without the feature: test_closed_form_sinkhorn_backward_equals_autograd
and test_cases_cover_the_degenerate_puzzles pin the reference of record itself (the recurrence the kernels implement is the one
autograd gives; the cases hold the degenerate puzzles the GPU tests rely on).  The fixture tests need the new golden file, the
argument-check and engine tests the new entry points and module."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

_spec = importlib.util.spec_from_file_location("matching_train_cases", Path(__file__).resolve().parent / "matching_train_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

REL = 1e-12


def close(got, want, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max()) if scale is None else scale
    return float(np.abs(got - want).max()) <= REL * max(scale, 1e-300)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("matching_train")


@pytest.mark.parametrize("n", cases.SINKHORN_SIZES)
def test_sinkhorn_restatement_equals_the_reference(fixture, n):
    """ds_mat, the loss and d loss / d s of the reference's sinkhorn + permutation_loss in float64, strided samples"""
    s, tgt = cases.sinkhorn_case(n)
    sn = cases.SINKHORN_SAMPLE[n]
    for it in cases.SINKHORN_ITERS:
        key = f"sk_n{n}_t{it}"
        P, loss, grad = cases.sinkhorn_loss_and_grad(s, tgt, max_iter=it)
        assert float(P.max()) <= cases.DS_MAX
        assert close(loss, fixture[f"{key}_loss"]), key
        assert close(cases.perm_loss_rows(P, tgt), fixture[f"{key}_row_loss"]), key
        assert close(P.reshape(-1)[::sn], fixture[f"{key}_ds_sample"], 1.0), key
        assert close(grad.reshape(-1)[::sn], fixture[f"{key}_grad_sample"], float(fixture[f"{key}_grad_max"])), key
        assert close(float(grad.abs().max()), fixture[f"{key}_grad_max"]), key


@pytest.mark.parametrize("n", (3, 37, 65, 150, 257))
def test_closed_form_sinkhorn_backward_equals_autograd(n):
    """the recurrence of csrc/matching_train.hip — potentials kept per step, G <- G - P_i rowsum(G) / colsum(G) from the last step down,
    ds = G_0 / tau — in float64 against autograd of the rewrite form, for odd and even step counts and rows without a target"""
    rng = np.random.default_rng(n)
    s, tgt = (cases.sinkhorn_case(n) if n in cases.SINKHORN_SIZES else
              ((0.05 * rng.normal(size=(n, n))).astype(np.float32), np.where(rng.uniform(size=n) < 0.2, -1, rng.integers(0, n, n)).astype(np.int32)))
    for it in (1, 2, 3, 7, 20):
        P, loss, grad = cases.sinkhorn_loss_and_grad(s, tgt, max_iter=it, g=0.37)
        P2, loss2, grad2 = cases.sinkhorn_closed_form(s, tgt, max_iter=it, g=0.37)
        assert close(P2, P, 1.0) and close(loss2, loss)
        assert float((grad2 - grad).abs().max()) <= 1e-12 * float(grad.abs().max()), (n, it)


@pytest.mark.parametrize("name", list(cases.BATCHES))
def test_head_restatement_equals_the_reference(fixture, name):
    """the whole step in float64: loss, metrics, targets (exact), every parameter's gradient, d_part_feats, the running statistics"""
    sd, batch = cases.head_state_dict(), cases.make_batch(name)
    r = cases.head_train_reference(sd, batch)
    S = cases.SAMPLE
    assert close(r["loss"], fixture[f"{name}_loss"]) and close(r["cls_loss"], fixture[f"{name}_cls_loss"]) and close(r["mat_loss"], fixture[f"{name}_mat_loss"])
    tp, fp, tn, fn = (float(c) for c in r["counts"])
    ratio = lambda a, b: a / b if b > 0 else 0.0
    assert [ratio(tp + tn, tp + fp + tn + fn), ratio(tp, tp + fp), ratio(tp, tp + fn), ratio(2 * tp, 2 * tp + fp + fn)] == fixture[f"{name}_metrics"].tolist()
    assert min(tp, fp, tn, fn) > 0
    assert r["N_"] == int(fixture[f"{name}_N_"]) and [len(t) for t in r["targets"]] == fixture[f"{name}_n_sum"].tolist()
    assert np.array_equal(np.concatenate(r["targets"]), fixture[f"{name}_targets"])
    assert close(np.concatenate([p.reshape(-1)[::S].numpy() for p in r["ds_mat"]]), fixture[f"{name}_ds_sample"], 1.0)
    for k in cases.PARAMS:
        g = r["grads"][k].reshape(-1)
        assert close(g[::S], fixture[f"{name}_grad_{k}_sample"], float(fixture[f"{name}_grad_{k}_max"])), k
    assert close(r["d_part_feats"].reshape(-1)[::S], fixture[f"{name}_d_part_feats_sample"], float(r["d_part_feats"].abs().max()))
    for k in cases.BUFFERS:
        assert close(r["buffers"][k], fixture[f"{name}_{k}"]), k
    assert int(fixture[f"{name}_pc_classifier.0.num_batches_tracked"]) == 1 == int(fixture[f"{name}_affinity_extractor.0.num_batches_tracked"])


def test_head_restatement_classifier_phase(fixture):
    """w_mat_loss = 0 (the reference's first epochs): only the classifier runs; the extractor and the affinity get no gradient and the
    extractor's running statistics stay"""
    sd, batch = cases.head_state_dict(), cases.make_batch("main")
    r = cases.head_train_reference(sd, batch, w_mat=0.0)
    S = cases.SAMPLE
    assert close(r["loss"], fixture["main_phase0_loss"]) and r["mat_loss"] is None
    for k in cases.PARAMS:
        if k.startswith("pc_classifier"):
            assert close(r["grads"][k].reshape(-1)[::S], fixture[f"main_phase0_grad_{k}_sample"], float(fixture[f"main_phase0_grad_{k}_max"])), k
        else:
            assert r["grads"][k] is None and f"main_phase0_nograd_{k}" in fixture
    assert close(r["d_part_feats"].reshape(-1)[::S], fixture["main_phase0_d_part_feats_sample"], float(r["d_part_feats"].abs().max()))
    assert np.array_equal(fixture["main_phase0_affinity_extractor.0.running_mean"], sd["affinity_extractor.0.running_mean"])
    assert int(fixture["main_phase0_affinity_extractor.0.num_batches_tracked"]) == 0


def test_head_restatement_without_critical_points(fixture):
    """every label 0: the reference's classifier phase is the part of the step that is defined; the restatement equals it"""
    r = cases.head_train_reference(cases.head_state_dict(), cases.make_batch_without_critical_points(), w_mat=0.0)
    S = cases.SAMPLE
    assert close(r["loss"], fixture["nolabel_phase0_loss"]) and r["counts"][0] == 0 == r["counts"][3]
    for k in cases.PARAMS[:4]:
        assert close(r["grads"][k].reshape(-1)[::S], fixture[f"nolabel_phase0_grad_{k}_sample"], float(fixture[f"nolabel_phase0_grad_{k}_max"])), k
    assert close(r["d_part_feats"].reshape(-1)[::S], fixture["nolabel_phase0_d_part_feats_sample"], float(r["d_part_feats"].abs().max()))


def test_cases_cover_the_degenerate_puzzles():
    """a piece without critical points, a puzzle where one piece owns them all (every target -1), a puzzle with none"""
    sd = cases.head_state_dict()
    main = cases.head_train_reference(sd, cases.make_batch("main"))
    assert main["N_"] == 41 and [len(t) for t in main["targets"]] == [41, 29] and all((t >= 0).all() for t in main["targets"])
    one = cases.head_train_reference(sd, cases.make_batch("one_owner"))
    assert (one["targets"][1] == -1).all() and len(one["targets"][1]) == 13 and (one["targets"][0] >= 0).all()
    empty = cases.head_train_reference(sd, cases.make_batch("empty_puzzle"))
    assert len(empty["targets"][1]) == 0 and empty["ds_mat"][1].numel() == 0


def test_training_entry_points_refuse_bad_arguments_before_any_launch(hip_lib):
    """null pointers, n outside [1, 65535], a workspace smaller than pfpp_sinkhorn_train_workspace(n), widths the kernels are not built
    for: error code and message through pfpp_last_error, no launch (no GPU needed)"""
    from pfpp_hip import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)                        # any non-null, 16-byte aligned address: never dereferenced on these paths
    tau = C.c_float(0.05)
    assert lib.pfpp_sinkhorn_train_workspace(-1) == -1 and lib.pfpp_sinkhorn_train_workspace(65536) == -1
    assert lib.pfpp_sinkhorn_train_workspace(65535) > 0 and lib.pfpp_sinkhorn_train_workspace(0) == 0
    n = 100
    need = lib.pfpp_sinkhorn_train_workspace(n)
    assert need == 2 * n * (8 + 4) + 2 * n * 8
    fwd = lambda **k: lib.pfpp_sinkhorn_train_fwd(k.get("s", one), k.get("ld", n), k.get("n", n), k.get("tau", tau), k.get("it", 20), k.get("tgt", one),
                                                  k.get("pots", one), k.get("ds", one), k.get("loss", one), k.get("rows", None), k.get("ws", one), k.get("bytes", need), None)
    bwd = lambda **k: lib.pfpp_sinkhorn_train_bwd(k.get("s", one), k.get("ld", n), k.get("n", n), k.get("tau", tau), k.get("it", 20), k.get("tgt", one),
                                                  k.get("pots", one), k.get("P", one), C.c_float(1.0), k.get("ds", one), k.get("ldg", n), k.get("ws", one),
                                                  k.get("bytes", need), None)
    for call in (fwd, bwd):
        for null in ("s", "tgt", "pots", "ds", "ws"):
            assert call(**{null: None}) != 0, null
        assert call(s=None) != 0 and b"null" in lib.pfpp_last_error()
        assert call(n=0) != 0 and call(n=65536, ld=65536, ldg=65536, bytes=1 << 40) != 0 and b"65535" in lib.pfpp_last_error()
        assert call(ld=n - 1) != 0 and call(it=-1) != 0 and call(tau=C.c_float(0.0)) != 0
        assert call(bytes=need - 1) != 0 and b"workspace" in lib.pfpp_last_error()
    assert fwd(loss=None) != 0 and bwd(P=None) != 0 and bwd(ldg=n - 1) != 0
    assert lib.pfpp_match_gt_targets(None, 10, one, one, one, 1, 4, one, None) != 0 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_match_gt_targets(one, 10, one, one, one, 1, 65536, one, None) != 0 and b"65535" in lib.pfpp_last_error()
    assert lib.pfpp_match_gt_targets(one, 0, one, one, one, 1, 4, one, None) != 0
    assert lib.pfpp_match_normalize_halves_bwd(one, None, one, 4, 512, None) != 0
    assert lib.pfpp_match_normalize_halves_bwd(one, one, one, 4, 256, None) != 0 and b"unsupported" in lib.pfpp_last_error()
    assert lib.pfpp_match_normalize_halves_bwd(C.c_void_p(4100), one, one, 4, 512, None) != 0 and b"aligned" in lib.pfpp_last_error()
    cws = lib.pfpp_match_cls_bce_workspace()
    assert cws == 1024 * 40
    assert lib.pfpp_match_cls_bce(one, 1, None, 8, C.c_float(1.0), one, one, 1, one, one, cws, None) != 0 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_match_cls_bce(one, 1, one, 0, C.c_float(1.0), one, one, 1, one, one, cws, None) != 0
    assert lib.pfpp_match_cls_bce(one, 1, one, 8, C.c_float(1.0), one, one, 1, one, None, cws, None) != 0
    assert lib.pfpp_match_cls_bce(one, 1, one, 8, C.c_float(1.0), one, one, 1, one, one, cws - 1, None) != 0 and b"workspace" in lib.pfpp_last_error()
    assert lib.pfpp_match_gather_raw(one, None, 8, 4, 128, one, None) != 0 and lib.pfpp_match_gather_raw(one, one, 8, 4, 64, one, None) != 0
    assert lib.pfpp_match_scatter_raw(one, one, 8, 4, 128, 1, None, None) != 0 and lib.pfpp_match_scatter_raw(one, one, 8, 4, 64, 1, one, None) != 0
    assert lib.pfpp_match_gather_raw(one, one, 8, 0, 128, one, None) == 0                    # nothing to do is not an error


def test_engine_refuses_cpu_tensors_and_the_rigid_loss(hip_lib):
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_train import MatchingHeadTrainEngine, gather_raw, sinkhorn_train_fwd

    head = MatchingHead()
    with pytest.raises(NotImplementedError, match="rigid_loss"):
        MatchingHeadTrainEngine(head, w_rig_loss=1.0)
    with pytest.raises(NotImplementedError, match="fp32"):
        MatchingHeadTrainEngine(MatchingHead(gemm_mode="f16x3"))
    eng = MatchingHeadTrainEngine(head, w_mat_loss=1.0)
    b = cases.make_batch("main")
    with pytest.raises(ValueError, match="GPU"):
        eng.loss_and_grads(torch.from_numpy(b["part_feats"]), torch.from_numpy(b["gt_pcs"]), b["n_pcs"], b["part_valids"],
                           critical_label=torch.from_numpy(b["critical_label"]))
    with pytest.raises(ValueError, match="GPU"):
        sinkhorn_train_fwd(torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        gather_raw(torch.zeros(4, 128), torch.zeros(2, dtype=torch.int64))
    assert all(p.grad is None for p in head.parameters())
