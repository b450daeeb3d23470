"""CPU: the reference of record of the rigid term of the matcher's training loss.  tests/matching_rigid_cases.py's float64 restatement
against tests/golden/matching_rigid.npz (the reference's own rigid_loss / horn_87 / training step in float64,
tools/make_matching_rigid_goldens.py), the closed-form gradient the kernels compute against autograd, the identity-on-zero-N rule, and
the argument checks of the new entry points and of the new engine (all of which return before a launch).

test_closed_form_gradient_equals_autograd runs no product code and passes without the feature: it pins the formula the gradient
kernel implements.  The fixture tests need the new golden file, the others the new entry points, module and class."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

_spec = importlib.util.spec_from_file_location("matching_rigid_cases", Path(__file__).resolve().parent / "matching_rigid_cases.py")
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)
tcases = cases._tc

REL = 1e-12
ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("pfpp_rigid_pair_sums", "pfpp_rigid_pair_pose", "pfpp_rigid_fold", "pfpp_rigid_grad", "pfpp_sinkhorn_train_bwd_seeded",
           "pfpp_match_colsum_ordered")


def close(got, want, scale=None, rel=REL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max(initial=0.0)) if scale is None else scale
    return float(np.abs(got - want).max(initial=0.0)) <= rel * max(scale, 1e-300)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("matching_rigid")


def check_rigid(fixture, key, ref):
    """a rigid_reference result (fed the fixture's float32 poses) against the reference's float64 run of the same inputs"""
    called = fixture[f"{key}_called"] != 0
    assert np.array_equal(np.asarray(ref["pairs"], dtype=np.int32).reshape(-1, 3), fixture[f"{key}_pairs"])
    assert np.array_equal(ref["status"] != 0, called), "the kept flags differ"
    assert bool(ref["finite"]) == bool(fixture[f"{key}_finite"])
    assert close(ref["mat_s"][called], fixture[f"{key}_mat_s"])
    firm = ref["gap"][called] >= cases.GAP_MIN                # Horn's own float64 poses, where the eigenvector is determined
    assert close(ref["R64"][called][firm], fixture[f"{key}_R64"][firm], 1.0) and close(ref["t64"][called][firm], fixture[f"{key}_t64"][firm])
    if not ref["finite"]:
        assert np.isnan(float(fixture[f"{key}_rig_loss"])) and ref["rig_loss"] == 0.0
        return
    assert ref["n_sum"] == int(fixture[f"{key}_n_sum"])
    assert (ref["status"] >= 0).all()
    assert close(ref["pair_loss"][called], fixture[f"{key}_pair_loss"])
    assert close(ref["numerator"], fixture[f"{key}_numerator"]) and close(ref["rig_loss"], fixture[f"{key}_rig_loss"])


@pytest.mark.parametrize("name", list(cases.KERNEL_CASES))
def test_rigid_restatement_equals_the_reference(fixture, name):
    """rigid_loss alone on given matrices: kept flags and n_sum exactly, per-pair mat_s and pair_loss, the loss and its gradient"""
    kc = cases.kernel_case(name)
    poses = cases.scatter_poses(fixture[f"{name}_called"], fixture[f"{name}_R32"], fixture[f"{name}_t32"])
    ref = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"], poses=poses)
    check_rigid(fixture, name, ref)
    grad = np.concatenate([g.numpy().reshape(-1) for g in ref["dP"]])
    if ref["finite"]:
        assert close(grad[::cases.SAMPLE], fixture[f"{name}_dP_sample"], float(fixture[f"{name}_dP_max"]))
        assert close(np.abs(grad).max(), fixture[f"{name}_dP_max"])
    else:
        assert not grad.any()
    # the poses the restatement finds on its own are the reference's float64 ones rounded: within a float32 ulp of its float32 ones
    own = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"])
    firm = (own["gap"] >= cases.GAP_MIN) & (own["status"] == 1)
    assert float(np.abs(own["R"] - poses[0])[firm].max(initial=0.0)) <= 4 * max(float(fixture.get(f"{name}_dev_R", 0.0)), 2.0 ** -24)


@pytest.mark.parametrize("name", list(cases.BATCHES))
def test_step_restatement_equals_the_reference(fixture, name):
    """the whole step at weights (1, 1, 1) in float64: the three losses, the rigid records, every gradient, the running statistics"""
    key = f"step_{name}"
    sd, batch = cases.head_state_dict(), cases.make_batch(name)
    poses = cases.scatter_poses(fixture[f"{key}_called"], fixture[f"{key}_R32"], fixture[f"{key}_t32"])
    r = cases.head_rigid_train_reference(sd, batch, cases.make_part_pcs(batch), poses=poses)
    S = cases.SAMPLE
    check_rigid(fixture, key, r["rigid"])
    assert float(r["rigid"]["gap"][r["rigid"]["status"] == 1].min()) >= cases.GAP_MIN
    for k in ("loss", "cls_loss", "mat_loss"):
        assert close(r[k], fixture[f"{key}_{k}"]), k
    assert close(r["rig_loss"], fixture[f"{key}_rig_loss"])
    assert close(np.concatenate([p.reshape(-1).numpy() for p in r["ds_mat"]])[::S], fixture[f"{key}_ds_sample"], 1.0)
    for k in tcases.PARAMS:
        assert close(r["grads"][k].reshape(-1)[::S], fixture[f"{key}_grad_{k}_sample"], float(fixture[f"{key}_grad_{k}_max"])), k
    assert close(r["d_part_feats"].reshape(-1)[::S], fixture[f"{key}_d_part_feats_sample"], float(fixture[f"{key}_d_part_feats_max"]))
    for k in tcases.BUFFERS:
        assert close(r["buffers"][k], fixture[f"{key}_{k}"]), k


@pytest.mark.parametrize("name", list(cases.KERNEL_CASES))
def test_closed_form_gradient_equals_autograd(name):
    """r_i, b_i, e_i = r_i A_i - b_i, pair_loss = sum |e_i|^2 and d(pair_loss mat_s) / dW_ij = 2 mat_s e_i . (A_i - T_j) + pair_loss,
    to both blocks of the pair, against autograd of the reference's lines"""
    kc = cases.kernel_case(name)
    ref = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"], w_rig=0.7)
    loss, grads, pl, ms = cases.rigid_closed_form(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"], (ref["R"], ref["t"]), w_rig=0.7)
    assert close(loss, ref["rig_loss"]) and close(ms, ref["mat_s"])
    assert close(pl[ref["status"] == 1], ref["pair_loss"][ref["status"] == 1])
    want = np.concatenate([g.numpy().reshape(-1) for g in ref["dP"]])
    assert close(np.concatenate([g.reshape(-1) for g in grads]), want)
    if ref["finite"]:
        assert np.abs(want).max() > 0


def test_zero_n_gives_the_identity(fixture):
    """a piece with a single critical point centres to exactly 0, so Horn's N is the zero matrix: the reference's horn_87 returns the
    identity there (LAPACK's eigenvectors of a zero matrix, argmax takes the first), in float32 and in float64, and so does the
    restatement"""
    kc = cases.kernel_case("edges")
    ref = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"])
    counts = kc["counts"][0]
    single = np.asarray([counts[p] == 1 or counts[q] == 1 for (_, p, q) in ref["pairs"]])
    assert single.sum() == 5 and (ref["status"] == 1).all()
    eye = np.eye(3)
    for k in np.nonzero(single)[0]:
        assert not ref["eig"][k].any()
        assert np.array_equal(ref["R64"][k], eye) and np.array_equal(fixture["edges_R32"][k], eye) and np.array_equal(fixture["edges_R64"][k], eye)


def test_cases_cover_the_degenerate_inputs():
    shapes = cases.KERNEL_CASES
    assert sorted(shapes["edges"][0]) == [0, 1, 2, 3, 63, 64, 65]
    assert len(shapes["two_piece"][0]) == 2 and len(shapes["twenty"][0]) == 20 and all(3 <= c <= 9 for c in shapes["twenty"][0])
    assert len(cases.pair_list(shapes["twenty"], [20])) == 190
    assert len(shapes["large"][0]) == 5 and sum(shapes["large"][0]) == 1033 and len(shapes["two_puzzles"]) == 2
    for name, want in (("zero_block", [1, 0, 1]), ("two_piece_zero", [-1]), ("nothing_kept", [0, 0, 0])):
        kc = cases.kernel_case(name)
        ref = cases.rigid_reference(kc["ds_mat"], kc["pts"], kc["counts"], kc["n_valid"])
        assert ref["status"].tolist() == want and ref["finite"] == (name == "zero_block")


def test_rigid_entry_points_are_declared_exported_and_refuse_bad_arguments(hip_lib):
    """declared in include/pfpp.h under the reference lines they replace, mirrored in pfpp_hip/_lib.py, exported; null pointers, n
    outside [0, 65535], more pieces than the kernels are built for and a short workspace return an error and a message before any
    launch (no GPU needed); nothing to do is not an error"""
    from pfpp_hip import _lib

    header = (ROOT / "include" / "pfpp.h").read_text()
    assert "utils/loss.py:59-142" in header and "pairwise_alignment.py:11-79" in header
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "pfpp_match_colsum_ordered_workspace" in _lib.PLAIN
    one = C.c_void_p(4096)
    sums = lambda **k: lib.pfpp_rigid_pair_sums(k.get("ds", one), k.get("ld", 10), k.get("n", 10), k.get("pts", one), k.get("off", one), k.get("P", 3),
                                                k.get("rb", one), k.get("pos", one), None)
    for null in ("ds", "pts", "off", "rb", "pos"):
        assert sums(**{null: None}) != 0 and b"null" in lib.pfpp_last_error(), null
    assert sums(n=-1) != 0 and sums(ld=9) != 0 and sums(P=0) != 0
    assert sums(n=65536, ld=65536) != 0 and b"65535" in lib.pfpp_last_error()
    assert sums(P=65) != 0 and b"64 pieces" in lib.pfpp_last_error()
    assert sums(rb=C.c_void_p(4100)) != 0 and b"aligned" in lib.pfpp_last_error()
    assert sums(n=0, ld=0) == 0
    pose = lambda **k: lib.pfpp_rigid_pair_pose(k.get("npairs", 2), k.get("pairs", one), one, one, k.get("P", 3), one, one, k.get("rb", one), one, one, one,
                                                one, k.get("status", one), None)
    assert pose(pairs=None) != 0 and b"null" in lib.pfpp_last_error()
    assert pose(rb=None) != 0 and pose(status=None) != 0 and pose(npairs=-1) != 0 and pose(P=65) != 0
    assert pose(npairs=0, pairs=None) == 0
    fold = lambda **k: lib.pfpp_rigid_fold(k.get("npairs", 2), k.get("stats", one), one, C.c_double(1.0), k.get("out", one), None)
    assert fold(out=None) != 0 and fold(stats=None) != 0 and fold(npairs=-1) != 0
    grad = lambda **k: lib.pfpp_rigid_grad(k.get("n", 10), k.get("pts", one), one, k.get("P", 3), k.get("rb", one), one, one, one, one, one, k.get("fold", one),
                                           k.get("dP", one), k.get("ldg", 12), None)
    for null in ("pts", "rb", "fold", "dP"):
        assert grad(**{null: None}) != 0 and b"null" in lib.pfpp_last_error(), null
    assert grad(ldg=9) != 0 and grad(n=-1) != 0 and grad(P=65) != 0
    assert grad(n=65536, ldg=65536) != 0 and b"65535" in lib.pfpp_last_error()
    assert grad(n=0) == 0
    n = 100
    need = lib.pfpp_sinkhorn_train_workspace(n)
    seeded = lambda **k: lib.pfpp_sinkhorn_train_bwd_seeded(k.get("s", one), k.get("ld", n), k.get("n", n), C.c_float(0.05), k.get("it", 20), k.get("tgt", one),
                                                            k.get("pots", one), k.get("P", one), C.c_float(1.0), k.get("ds", one), k.get("ldg", n),
                                                            k.get("ws", one), k.get("bytes", need), None)
    for null in ("s", "tgt", "pots", "P", "ds", "ws"):
        assert seeded(**{null: None}) != 0, null
    assert seeded(s=None) != 0 and b"pfpp_sinkhorn_train_bwd_seeded: null" in lib.pfpp_last_error()
    assert seeded(n=0) != 0 and seeded(n=65536, ld=65536, ldg=65536, bytes=1 << 40) != 0 and b"65535" in lib.pfpp_last_error()
    assert seeded(ldg=n - 1) != 0 and seeded(it=-1) != 0
    assert seeded(bytes=need - 1) != 0 and b"workspace" in lib.pfpp_last_error()
    assert lib.pfpp_match_colsum_ordered_workspace(-1, 4) == -1 == lib.pfpp_match_colsum_ordered_workspace(4, 0)
    assert lib.pfpp_match_colsum_ordered_workspace(65, 4) == 2 * 4 * 8 and lib.pfpp_match_colsum_ordered_workspace(0, 4) == 0
    ordered = lambda **k: lib.pfpp_match_colsum_ordered(k.get("x", one), k.get("ld", 4), k.get("rows", 65), k.get("cols", 4), k.get("out", one),
                                                        k.get("ws", one), k.get("bytes", 64), None)
    assert ordered(x=None) != 0 and b"null" in lib.pfpp_last_error()
    assert ordered(out=None) != 0 and ordered(ld=3) != 0 and ordered(rows=-1) != 0 and ordered(cols=0, ld=0) != 0
    assert ordered(bytes=63) != 0 and b"workspace" in lib.pfpp_last_error()
    assert ordered(ws=None) != 0 and ordered(ws=C.c_void_p(4100)) != 0 and b"aligned" in lib.pfpp_last_error()


def test_rigid_engine_refusals(hip_lib):
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine, rigid_pairs
    from pfpp_hip.matching_train import MatchingHeadTrainEngine

    head = MatchingHead()
    with pytest.raises(NotImplementedError, match="MatchingHeadRigidTrainEngine"):          # the base class still refuses, and says where to go
        MatchingHeadTrainEngine(head, w_rig_loss=1.0)
    with pytest.raises(NotImplementedError, match="fp32"):
        MatchingHeadRigidTrainEngine(MatchingHead(gemm_mode="f16x3"), w_mat_loss=1.0, w_rig_loss=1.0)
    eng = MatchingHeadRigidTrainEngine(head, w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=1.0)
    assert (eng.w_cls_loss, eng.w_mat_loss, eng.w_rig_loss) == (1.0, 1.0, 1.0)
    b = cases.make_batch("main")
    args = (torch.from_numpy(b["part_feats"]), torch.from_numpy(b["gt_pcs"]), b["n_pcs"], b["part_valids"])
    label = torch.from_numpy(b["critical_label"])
    with pytest.raises(ValueError, match="part_pcs"):
        eng.loss_and_grads(*args, critical_label=label)
    with pytest.raises(ValueError, match="GPU"):
        eng.loss_and_grads(*args, critical_label=label, part_pcs=torch.from_numpy(cases.make_part_pcs(b)))
    with pytest.raises(ValueError, match="GPU"):
        MatchingHeadRigidTrainEngine(head, w_mat_loss=1.0).loss_and_grads(*args, critical_label=label)
    with pytest.raises(ValueError, match="GPU"):
        rigid_pairs(torch.zeros(4, 4), torch.zeros(4, 3), np.array([0, 0, 1, 1]))
    assert all(p.grad is None for p in head.parameters())


def test_on_epoch_end_switches_the_weights_like_the_reference(hip_lib):
    """training_epoch_end (joint_seg_align_model.py:453-463): a weight that is 0 becomes 1.0 once epoch >= its epoch, and only from 0"""
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine

    eng = MatchingHeadRigidTrainEngine(MatchingHead())
    assert (eng.w_cls_loss, eng.w_mat_loss, eng.w_rig_loss) == (1.0, 0.0, 0.0)
    for epoch in range(0, 9):
        eng.on_epoch_end(epoch)
        assert (eng.w_mat_loss, eng.w_rig_loss) == (0.0, 0.0)
    eng.on_epoch_end(9)
    assert (eng.w_mat_loss, eng.w_rig_loss) == (1.0, 0.0)
    eng.on_epoch_end(198)
    assert eng.w_rig_loss == 0.0
    eng.on_epoch_end(199)
    assert (eng.w_mat_loss, eng.w_rig_loss) == (1.0, 1.0)
    eng2 = MatchingHeadRigidTrainEngine(MatchingHead(), w_mat_loss=0.5, w_rig_loss=0.25)
    eng2.on_epoch_end(250)
    assert (eng2.w_mat_loss, eng2.w_rig_loss) == (0.5, 0.25)
    eng3 = MatchingHeadRigidTrainEngine(MatchingHead())
    eng3.on_epoch_end(3, mat_epoch=2, rig_epoch=4)
    assert (eng3.w_mat_loss, eng3.w_rig_loss) == (1.0, 0.0)
