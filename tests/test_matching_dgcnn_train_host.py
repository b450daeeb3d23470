"""CPU: the host side of the DGCNN encoder's training step (pfpp_hip/matching_dgcnn_train.py) and the test-side restatement of
tests/matching_dgcnn_train_cases.py against tests/golden/matching_dgcnn_train.npz, which tools/make_matching_dgcnn_train_goldens.py
wrote from the reference's own module in .train().

The float64 restatement in the reference's form must reproduce the fixture (neighbour sets and winners exactly, values, the 15
gradients and the 10 moved running buffers to 1e-10 of each tensor's maximum), and the decomposed form the kernels compute, written
out by hand without autograd, must equal the direct form under autograd to 1e-12 on the same lists and winners: negative gammas and
padded winners included.  Every test prints what it measured before it asserts."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("pfpp_dgcnn_edge_stats", "pfpp_dgcnn_bn_leaky_apply", "pfpp_dgcnn_bn_leaky_bwd", "pfpp_dgcnn_edge_bwd_dv", "pfpp_dgcnn_edge_bwd_du")
ACTS = ("x1", "x2", "x3", "x4", "out")
CASES = ("tiny", "small")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_dgcnn_train_cases", ROOT / "tests" / "matching_dgcnn_train_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_R64 = {}


def restated64(name):
    """the float64 restatement in the reference's form with its own search and its own winners, computed once and left unchanged"""
    if name not in _R64:
        x, lengths = cases.case_arrays(name)
        _R64[name] = (cases.train_step(cases.state_dict(), x, lengths, cases.dout_array(name), torch.float64), x, lengths)
    return _R64[name]


@pytest.mark.parametrize("name", CASES)
def test_restatement_in_float64_equals_the_reference(golden, name):
    g = golden("matching_dgcnn_train")
    r, x, lengths = restated64(name)
    N = len(x)
    assert int(g[f"{name}_seed"]) == cases.SEEDS[name] and N == int(np.sum(cases.LENGTHS[name]))
    assert tuple(g["param_names"].tolist()) == cases.PARAMS and tuple(g["buffer_names"].tolist()) == cases.BUFFERS
    assert (g[f"{name}_min_step"] >= cases.MIN_STEP).all()
    for l in range(4):
        want = g[f"{name}_l{l + 1}_knn"].astype(np.int64)
        assert np.array_equal(np.sort(r["knn"][l], 1), np.sort(want, 1)), f"level {l + 1}: neighbour sets"
        who_want = np.take_along_axis(want, g[f"{name}_l{l + 1}_winner"].astype(np.int64), 1)
        who_got = np.take_along_axis(r["knn"][l], r["winner"][l], 1)
        diff = int((who_want != who_got).sum())
        print(f"{name} level {l + 1}: {diff} of {who_want.size} winners differ from the reference's; {int((who_want == N).sum())} won by a padded slot")
        assert diff == 0
    worst = 0.0
    for key, got in [(k, r[k].numpy()) for k in ACTS] + [(f"grad_{k}", r["grads"][k]) for k in cases.PARAMS] + \
                    [(f"buf_{k}", r["buffers"][k]) for k in cases.BUFFERS]:
        stride = int(g[f"stride_{key[5:] if key.startswith('grad_') else key}"]) if not key.startswith("buf_") else 1
        want = g[f"{name}_{key}"]
        err = float(np.abs(got.reshape(-1)[::stride] - want).max() / float(g[f"{name}_{key}_max"]))
        worst = max(worst, err)
        print(f"{name} {key}: restated float64 vs the reference's float64 {err:.3g} of the maximum (bar 1e-10)")
        assert want.dtype == np.float64 and err <= 1e-10
    print(f"{name}: worst {worst:.3g}")


@pytest.mark.parametrize("name", CASES)
def test_decomposed_form_equals_the_direct_form_in_float64(golden, name):
    g = golden("matching_dgcnn_train")
    direct, x, lengths = restated64(name)
    sd = cases.state_dict()
    N = len(x)
    dec = cases.train_step(sd, x, lengths, cases.dout_array(name), torch.float64, indices=direct["knn"], winners=direct["winner"], form="decomposed")
    neg = [int((sd[f"bn{l}.weight"] < 0).sum()) for l in range(1, 5)]
    padded = [int((np.take_along_axis(direct["knn"][l], direct["winner"][l], 1) == N).sum()) for l in range(4)]
    print(f"{name}: negative gammas per level {neg} of {cases.WIDTHS}; entries won by a padded slot per level {padded}")
    assert all(n > 0 for n in neg) and all(p > 0 for p in padded)
    # the decomposed form picks the same winners on its own (no ties in these cases)
    own = cases.train_step(sd, x, lengths, cases.dout_array(name), torch.float64, indices=direct["knn"], form="decomposed")
    assert all(np.array_equal(a, b) for a, b in zip(own["winner"], direct["winner"]))
    for key, a, b in [(k, direct[k].numpy(), dec[k].numpy()) for k in ACTS] + [(f"grad {k}", direct["grads"][k], dec["grads"][k]) for k in cases.PARAMS] \
            + [(f"buffer {k}", direct["buffers"][k], dec["buffers"][k]) for k in cases.BUFFERS]:
        err = float(np.abs(a - b).max() / np.abs(a).max())
        print(f"{name} {key}: decomposed vs direct {err:.3g} of the maximum (bar 1e-12)")
        assert a.shape == b.shape and err <= 1e-12


def test_numpy_statistics_pass_covers_padded_winners_one_point_and_a_first_slot_tie():
    uv, idx, gamma, beta = cases.stats_case(64)
    e, w, z = cases.stats_extremum_f32(uv, idx, gamma)
    N = len(uv)
    assert (gamma < 0).any() and (gamma == 0).any() and (gamma > 0).any()
    even_pos, odd_neg = (np.arange(64) % 2 == 0) & (gamma >= 0), (np.arange(64) % 2 == 1) & (gamma < 0)
    # points 0 .. 2: the padded 0 wins the max in the even channels and the min in the odd ones, at the first padded slot (3)
    assert (e[:3][:, even_pos] == 0).all() and (w[:3][:, even_pos] == 3).all()
    assert (e[:3][:, odd_neg] == 0).all() and (w[:3][:, odd_neg] == 3).all()
    assert (idx[3, 1:] == N).all() and set(np.unique(w[3])) <= {0, 1}                   # a piece of one point: its own row or the first padded slot
    assert np.array_equal(z[12, 0], z[12, 1]) and (w[12][even_pos] == 0).all() and (w[12][odd_neg] == 0).all()      # the tie: slot 0, not slot 1
    y = cases.apply_f32(e, np.ones(64, np.float32), np.zeros(64, np.float32))
    assert np.array_equal(y, np.where(e > 0, e, e * np.float32(0.2)))


def test_gather_lists_hold_a_hub():
    idx = cases.gather_lists()
    N = len(idx)
    assert N == sum(cases.GATHER_LENGTHS) == 240
    counts = np.bincount(idx.reshape(-1), minlength=N + 1)
    hub = N - 130
    print(f"inverse list lengths: hub {counts[hub]}, others at most {np.delete(counts[:N], hub).max()}, padded slots {counts[N]}")
    assert counts[hub] == 130 and counts[0] == 1 and counts[N] == 19 + 3 * 17
    assert (idx[:, 0] == np.arange(N)).all()


def test_header_declares_the_entries_and_arguments_are_checked_before_a_launch(hip_lib):
    from pfpp_hip import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pfpp.h").read_text(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} not declared in include/pfpp.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.pfpp_version() == 2
    assert "PFPP_DGCNN_TRAIN_WS_DOUBLES (PFPP_DGCNN_TRAIN_MAX_WG * 512 + 1024)" in text
    one, odd, d, f = C.c_void_p(4096), C.c_void_p(4100), C.c_double, C.c_float
    # pfpp_dgcnn_edge_stats(uv, ld, idx, gamma, beta, eps, momentum, rmean, rvar, N, C_out, K, e, winner, coef, workspace, stream)
    st = lib.pfpp_dgcnn_edge_stats
    ok = lambda **kw: dict(dict(uv=one, ld=512, idx=one, gamma=one, beta=one, eps=d(1e-5), mom=d(0.1), rm=one, rv=one, N=10, C=256, K=20, e=one,
                                w=one, coef=one, ws=one), **kw)
    call = lambda a: st(a["uv"], a["ld"], a["idx"], a["gamma"], a["beta"], a["eps"], a["mom"], a["rm"], a["rv"], a["N"], a["C"], a["K"], a["e"],
                        a["w"], a["coef"], a["ws"], None)
    for nm in ("uv", "idx", "gamma", "beta", "e", "w", "coef", "ws"):
        assert call(ok(**{nm: None})) == -1 and b"null" in lib.pfpp_last_error(), nm
    assert call(ok(N=0)) == -1 and call(ok(rm=None)) == -1 and call(ok(ld=510)) == -1 and call(ok(uv=odd)) == -1 and call(ok(mom=d(1.5))) == -1
    assert call(ok(w=C.c_void_p(4098))) == -1
    for c in (32, 96, 512):
        assert call(ok(C=c, ld=2048)) == -2 and b"64, 128 or 256" in lib.pfpp_last_error()
    assert call(ok(K=16)) == -2 and b"K must be 20" in lib.pfpp_last_error()
    assert call(ok(N=(1 << 31) // 20)) == -2
    # pfpp_dgcnn_bn_leaky_apply(y, rows, C, ld, coef, slope, out, ldo, stream)
    ap = lib.pfpp_dgcnn_bn_leaky_apply
    assert ap(one, 0, 128, 128, one, f(0.2), one, 128, None) == 0
    assert ap(None, 5, 128, 128, one, f(0.2), one, 128, None) == -1 and b"null" in lib.pfpp_last_error()
    assert ap(one, 5, 128, 128, None, f(0.2), one, 128, None) == -1 and ap(one, 5, 128, 128, one, f(0.2), None, 128, None) == -1
    assert ap(one, 5, 126, 128, one, f(0.2), one, 128, None) == -2 and ap(one, 5, 2048, 2048, one, f(0.2), one, 2048, None) == -2
    assert ap(one, 5, 128, 124, one, f(0.2), one, 128, None) == -1 and ap(one, 5, 128, 128, one, f(0.2), one, 64, None) == -1
    assert ap(odd, 5, 128, 128, one, f(0.2), one, 128, None) == -1 and ap(one, 5, 128, 128, one, f(0.2), odd, 128, None) == -1
    # pfpp_dgcnn_bn_leaky_bwd(y, ld, g1, ldg1, g2, ldg2, rows, C, coef, slope, count, h, dgamma, dbeta, means, dy, workspace, stream)
    bw = lib.pfpp_dgcnn_bn_leaky_bwd
    base = [one, 128, one, 128, None, 0, 5, 128, one, f(0.2), d(5.0), one, one, one, one, None, one, None]

    def bwd(**kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return bw(*a)

    for i in (0, 2, 8, 11, 12, 13, 14, 16):
        assert bwd(**{f"a{i}": None}) == -1 and b"null" in lib.pfpp_last_error(), i
    assert bwd(a6=0) == -1 and bwd(a7=126) == -2 and bwd(a3=64) == -1 and bwd(a4=one, a5=64) == -1 and bwd(a2=odd) == -1 and bwd(a15=odd) == -1
    assert bwd(a10=d(0.0)) == -1
    # pfpp_dgcnn_edge_bwd_dv(uv, ld, idx, winner, h, coef, means, N, C_out, K, duv, stream)
    dv = lib.pfpp_dgcnn_edge_bwd_dv
    assert dv(one, 512, one, one, one, one, one, 0, 256, 20, one, None) == 0
    for bad in range(7):
        p = [one] * 7
        p[bad] = None
        assert dv(p[0], 512, p[1], p[2], p[3], p[4], p[5], 10, 256, 20, p[6], None) == -1 and b"null" in lib.pfpp_last_error()
    assert dv(one, 512, one, one, one, one, one, 10, 96, 20, one, None) == -2 and dv(one, 512, one, one, one, one, one, 10, 256, 19, one, None) == -2
    assert dv(one, 508, one, one, one, one, one, 10, 256, 20, one, None) == -1 and dv(one, 512, one, one, one, one, one, 10, 256, 20, odd, None) == -1
    # pfpp_dgcnn_edge_bwd_du(uv, ld, off, ent, n_ent, winner, h, coef, means, N, C_out, K, duv, stream)
    du = lib.pfpp_dgcnn_edge_bwd_du
    assert du(one, 512, one, one, 0, one, one, one, one, 0, 256, 20, one, None) == 0
    for bad in range(8):
        p = [one] * 8
        p[bad] = None
        assert du(p[0], 512, p[1], p[2], 200, p[3], p[4], p[5], p[6], 10, 256, 20, p[7], None) == -1 and b"null" in lib.pfpp_last_error()
    assert du(one, 512, one, one, 201, one, one, one, one, 10, 256, 20, one, None) == -1 and b"more entries" in lib.pfpp_last_error()
    assert du(one, 512, one, one, 200, one, one, one, one, 10, 32, 20, one, None) == -2 and du(one, 130, one, one, 200, one, one, one, one, 10, 64, 20, one, None) == -1


def test_wrappers_and_engines_refuse_bad_arguments_before_a_launch():
    from pfpp_hip import matching_dgcnn_train as M
    from pfpp_hip.matching import DescriptorNetwork
    from pfpp_hip.matching_dgcnn import DGCNNDynamic
    from pfpp_hip.matching_encoder import PointNet2PTMSGDynamic

    cpu = torch.zeros(10, 128)
    idx = torch.zeros(10, 20, dtype=torch.int32)
    with pytest.raises(ValueError, match="64, 128, 256"):
        M.dgcnn_edge_stats(cpu, idx, cpu[0], cpu[0], 1e-5, c_out=96)
    with pytest.raises(ValueError, match="idx"):
        M.dgcnn_edge_stats(cpu, idx, cpu[0], cpu[0], 1e-5, c_out=64)
    with pytest.raises(ValueError, match="GPU"):
        M.dgcnn_bn_leaky_apply(cpu, cpu[:4])
    with pytest.raises(ValueError, match="GPU"):
        M.dgcnn_bn_leaky_bwd(cpu, cpu, cpu[:4])
    with pytest.raises(ValueError, match="idx"):
        M.dgcnn_edge_bwd_dv(cpu, idx, cpu, cpu, cpu, cpu, c_out=64)
    with pytest.raises(ValueError, match="off / ent"):
        M.dgcnn_edge_bwd_du(cpu, idx, idx, cpu, cpu, cpu, cpu, c_out=64)
    with pytest.raises(ValueError, match="idx"):
        M.dgcnn_inverse_lists(torch.zeros(10, 16, dtype=torch.int32))
    with pytest.raises(TypeError, match="DGCNNDynamic"):
        M.DGCNNTrainEngine(PointNet2PTMSGDynamic(3, 128))
    with pytest.raises(TypeError, match="DescriptorNetwork"):
        M.DGCNNDescriptorTrainEngine(DGCNNDynamic(128))
    with pytest.raises(TypeError, match="DGCNN encoder"):
        M.DGCNNDescriptorTrainEngine(DescriptorNetwork())
    enc = DGCNNDynamic(128)
    eng = M.DGCNNTrainEngine(enc)
    assert tuple(eng.params) == cases.PARAMS and not enc.training and eng.saved == {} and eng.stage_events is None
    with pytest.raises(ValueError, match="GPU"):
        eng.forward(torch.zeros(5, 3), [5])
    with pytest.raises(RuntimeError, match="before forward"):
        eng.backward(torch.zeros(5, 128))
    full = M.DGCNNDescriptorTrainEngine(DescriptorNetwork(encoder="dgcnn.dynamic"))
    assert isinstance(full.encoder, M.DGCNNTrainEngine) and not full.net.training
    assert issubclass(M.DGCNNFunction, torch.autograd.Function)
    assert M.DGCNN_TRAIN_WS_DOUBLES == 1024 * 512 + 1024 and M.ONE_VALUE == "Expected more than 1 value per channel when training"


def test_the_three_old_refusals_still_raise():
    from pfpp_hip.matching import DescriptorNetwork
    from pfpp_hip.matching_dgcnn import DGCNNDynamic
    from pfpp_hip.matching_encoder_train import DescriptorTrainEngine
    from pfpp_hip.matching_fit import MatcherTrainer, default_config

    with pytest.raises(NotImplementedError, match="training a DGCNN encoder"):
        DGCNNDynamic(128).train()
    with pytest.raises(NotImplementedError, match="forward in eval mode exists.*training step.*does not"):
        DescriptorTrainEngine(DescriptorNetwork(encoder="dgcnn.dynamic"))
    cfg = default_config()
    cfg["MODEL"]["ENCODER"] = "dgcnn.dynamic"
    with pytest.raises(NotImplementedError, match="forward in eval mode exists.*training step does not"):
        MatcherTrainer(cfg)
