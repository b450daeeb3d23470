"""CPU: the host side of the point-transformer layer's training (pfpp_hip/matching_transformer_train.py) and the test-side oracle of
tests/matching_self_train_cases.py against tests/golden/matching_self_train.npz, which tools/make_matching_self_train_goldens.py wrote
from the reference's own PointTransformerLayer in .train() under autograd (whole flat batch in one call).

The restatement in float64, fed the fixture's three ReLU patterns, must equal the fixture's float64 results (out, dx, 20 gradients, 6
running buffers) to 1e-12 of each tensor's largest magnitude, so the GPU tests may lean on it.  The four gradients that vanish in
exact arithmetic are ~1e-14 in the fixture and are compared on the scale their rounding is relative to (ZERO_GRADS, ZERO_SUMS of the
case file).  Every test prints what it measured before it asserts."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("pfpp_ptf_train_bn3_stats", "pfpp_ptf_train_bn_finalise", "pfpp_ptf_train_bn128_stats", "pfpp_ptf_train_tile",
               "pfpp_ptf_train_finish", "pfpp_ptf_train_bwd_w", "pfpp_ptf_train_bwd_u", "pfpp_ptf_train_bwd_r", "pfpp_ptf_train_bwd_gather")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_self_train_cases", ROOT / "tests" / "matching_self_train_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()
_RESTATED = {}


def fixture_lists(golden, name):
    g = golden("matching_transformer")
    return g[f"{name}_idx_k"].astype(np.int64), g[f"{name}_idx_v"].astype(np.int64)


def fixture_masks(g):
    return [np.unpackbits(g[f"tiny_relu{i}_mask"])[:int(np.prod(g[f"tiny_relu{i}_shape"]))].reshape(g[f"tiny_relu{i}_shape"]).astype(bool) for i in range(3)]


def restated(golden, name, mutate=None):
    """the float64 restatement of a case on the fixture's lists (with the fixture's masks where it stores them), computed once"""
    if (name, mutate) not in _RESTATED:
        p, x, _, dout = cases.case_inputs(name)
        masks = fixture_masks(golden("matching_self_train")) if name == "tiny" else None
        _RESTATED[name, mutate] = cases.self_train_restate(cases.base.ptf_state_dict(), p, x, dout, fixture_lists(golden, name), torch.float64, masks, mutate)
    return _RESTATED[name, mutate]


def deviation(g, name, key, value) -> float:
    """largest deviation of what the fixture keeps of a tensor, over the fixture's largest magnitude (a row or column sum: times its length)"""
    top = float(g[f"{name}_{key}_max"])
    worst = 0.0
    for part, got in cases.sample(value).items():
        want = g[f"{name}_{key}_{part}"]
        assert got.shape == want.shape and want.dtype == np.float64
        worst = max(worst, float(np.abs(got - want).max() / (top * (1 if part in ("full", "rows") else max(value.shape)))))
    return worst


def bar(g, name, key) -> float:
    return 4 * max(float(g[f"{name}_{key}_refdev"]), 2.0 ** -23)


@pytest.mark.parametrize("name", ["tiny", "pair"])
def test_restatement_in_float64_equals_the_reference_to_1e_12(golden, name):
    g = golden("matching_self_train")
    assert [str(k) for k in g["names"]] == list(cases.TENSORS) and int(g["row_step"]) == cases.ROW_STEP
    r = restated(golden, name)
    for i in range(3):
        flips, entries = int(g[f"{name}_relu{i}_flips"]), int(g[f"{name}_relu{i}_entries"])
        print(f"{name} ReLU {i}: the reference's float32 and float64 signs differ in {flips} of {entries} entries; smallest float64 "
              f"|pre-activation| {float(g[f'{name}_relu{i}_pre_min_abs']):.3g} (restated: {float(r['pre'][i].abs().min()):.3g})")
        assert flips * 10000 <= entries and entries == r["pre"][i].numel()               # the cap of the GPU test holds for the reference itself
        assert abs(float(r["pre"][i].abs().min()) - float(g[f"{name}_relu{i}_pre_min_abs"])) <= 1e-12
    assert r["num_batches_tracked"] == 1
    worst = 0.0
    for key in cases.TENSORS:
        v = r[key].numpy()
        if key in cases.ZERO_GRADS + cases.ZERO_SUMS:
            continue
        err = deviation(g, name, key, v)
        worst = max(worst, err)
        assert err <= 1e-12, (key, err)
        assert 0 < float(g[f"{name}_{key}_refdev"]) < 1e-5
    print(f"{name}: restatement vs the reference's float64 results, worst tensor {worst:.3g} of the maximum (bar 1e-12)")


@pytest.mark.parametrize("name", ["tiny", "pair"])
def test_the_gradients_that_vanish_in_exact_arithmetic_are_rounding_in_the_fixture(golden, name):
    g = golden("matching_self_train")
    r = restated(golden, name)
    for key, rel in (("linear_p.0.bias", "linear_p.0.weight"), ("linear_w.2.bias", "linear_w.2.weight")):
        got, scale = float(np.abs(g[f"{name}_{key}_full"]).max()), float(g[f"{name}_{rel}_max"])
        print(f"{name} {key}: the reference's float64 gradient is at most {got:.3g}, {got / scale:.3g} of the largest entry of {rel}")
        assert got <= 1e-12 * scale and float(r[key].abs().max()) <= 1e-12 * scale        # writing zeros is right
    for key in cases.ZERO_SUMS:
        got, scale = float(np.abs(g[f"{name}_{key}_full"]).max()), r["zero_sum_scale"][key]
        print(f"{name} {key}: the reference's float64 gradient is at most {got:.3g}, {got / scale:.3g} of the sum of its |terms| ({scale:.4g})")
        assert scale > 1 and got <= 1e-12 * scale and float(r[key].abs().max()) <= 1e-12 * scale


def test_masks_of_the_fixture_are_the_restatements_own_and_a_flipped_entry_shows(golden):
    p, x, _, dout = cases.case_inputs("tiny")
    sd, lists = cases.base.ptf_state_dict(), fixture_lists(golden, "tiny")
    own = cases.self_train_restate(sd, p, x, dout, lists, torch.float64)
    masks = fixture_masks(golden("matching_self_train"))
    assert all(np.array_equal(m, (a > 0).numpy()) for m, a in zip(masks, own["pre"]))
    r = restated(golden, "tiny")
    assert all(torch.allclose(own[k], r[k], rtol=0, atol=1e-12 * float(own[k].abs().max()) + 1e-300) for k in cases.TENSORS)
    i = np.unravel_index(np.argmax(own["pre"][1].numpy()), masks[1].shape)                # the most active entry switched off
    masks[1][i] = False
    f = cases.self_train_restate(sd, p, x, dout, lists, torch.float64, masks)
    assert not torch.equal(r["dx"], f["dx"]) and not torch.equal(r["linear_w.2.weight"], f["linear_w.2.weight"])


@pytest.mark.parametrize("mutate", cases.MUTATIONS)
def test_a_misreading_of_the_layer_leaves_the_fixtures_bar_by_a_wide_margin(golden, mutate):
    g = golden("matching_self_train")
    m = restated(golden, "tiny", mutate)
    over = {k: deviation(g, "tiny", k, m[k].numpy()) / bar(g, "tiny", k) for k in cases.TENSORS if k not in cases.ZERO_GRADS + cases.ZERO_SUMS}
    key = max(over, key=over.get)
    print(f"{mutate}: {sum(v > 1 for v in over.values())} of {len(over)} tensors outside their bar; worst {key} at {over[key]:.3g} bars, out at "
          f"{over['out']:.3g}, dx at {over['dx']:.3g}")
    assert over[key] >= 20 and over["dx"] >= 20
    if mutate == "no_dxq":
        assert float(m["linear_q.weight"].abs().max()) == 0.0 and over["out"] <= 1e-6     # the forward is untouched, linear_q gets nothing


def test_header_declares_the_entries_and_arguments_are_checked_before_a_launch(hip_lib):
    from pfpp_hip import _lib
    from pfpp_hip import matching_transformer_train as MT

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pfpp.h").read_text(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} not declared in include/pfpp.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.pfpp_version() == 2
    for macro, value in (("PFPP_PTF_TRAIN_FLOATS", MT.PTF_TRAIN_FLOATS), ("PFPP_PTF_TRAIN_BWD_W_SUMS", MT.PTF_BWD_W_SUMS),
                         ("PFPP_PTF_TRAIN_BWD_U_SUMS", MT.PTF_BWD_U_SUMS), ("PFPP_PTF_TRAIN_BWD_R_SUMS", MT.PTF_BWD_R_SUMS),
                         ("PFPP_PTF_TRAIN_MAX_WG", 1024)):
        assert f"#define {macro} {value}" in text, macro
    assert MT.PTF_TRAIN_WS_DOUBLES == 1024 * MT.PTF_BWD_U_SUMS and "PFPP_PTF_TRAIN_WS_DOUBLES (PFPP_PTF_TRAIN_MAX_WG * PFPP_PTF_TRAIN_BWD_U_SUMS)" in text
    hi = max(lo + n for lo, n in MT.PTF_PACK_SLOTS.values())
    assert hi <= MT.PTF_TRAIN_FLOATS and sorted(MT.PTF_PACK_SLOTS) == sorted(k for k in cases.GRAD_NAMES if k.startswith(("linear_p.0", "linear_p.3", "linear_w.2", "linear_w.5")))
    one = C.c_void_p(4096)            # a non-null, 16-byte aligned address that is never dereferenced on these paths
    f = C.c_float
    # (entry, arguments with N = 10, C = 128, K = 16; positions of N, C (or None), K; the pointers that may be null)
    table = {
        "pfpp_ptf_train_bn3_stats": ([one, one, one, 10, 16, one, one, None], 3, None, 4, ()),
        "pfpp_ptf_train_bn128_stats": ([one, one, 384, one, one, one, 10, 128, 16, one, one, None, None], 6, 7, 8, (11,)),
        "pfpp_ptf_train_tile": ([one, one, 384, one, one, one, 10, 128, 16, one, one, one, None, None], 6, 7, 8, (12,)),
        "pfpp_ptf_train_finish": ([one, 384, one, one, one, one, 10, 128, 16, one, one, one, None, None], 6, 7, 8, (12,)),
        "pfpp_ptf_train_bwd_w": ([one, one, one, one, 384, one, one, one, one, 10, 128, 16, one, one, one, None, None], 9, 10, 11, (15,)),
        "pfpp_ptf_train_bwd_u": ([one, one, 384, one, one, one, 10, 128, 16, one, one, one, one, None, None], 6, 7, 8, (13,)),
        "pfpp_ptf_train_bwd_r": ([one, one, one, one, one, 384, one, one, one, 10, 128, 16, one, 384, one, one, None, None], 9, 10, 11, (16,)),
        "pfpp_ptf_train_bwd_gather": ([one, one, one, one, one, 384, one, one, 10, 128, 16, one, one, one, one, one, 384, None], 8, 9, 10, ()),
    }
    for name, (args, iN, iC, iK, nullable) in table.items():
        fn = getattr(lib, name)
        assert len(args) == len(_lib.SIGNATURES[name]), name
        zero = list(args)
        zero[iN] = 0
        assert fn(*zero) == 0, name                                                      # no point: nothing to do
        bad = list(args)
        bad[iK] = 8
        assert fn(*bad) == -2 and b"16" in lib.pfpp_last_error(), name
        if iC is not None:
            bad = list(args)
            bad[iC] = 64
            assert fn(*bad) == -2 and b"128" in lib.pfpp_last_error(), name
        bad = list(args)
        bad[iN] = -1
        assert fn(*bad) == -1, name
        for hole, a in enumerate(args[:-1]):                                             # every pointer but the stream and pre_dump
            if a is one and hole not in nullable:
                bad = list(args)
                bad[hole] = None
                assert fn(*bad) == -1 and b"null" in lib.pfpp_last_error(), (name, hole)
    # pfpp_ptf_train_bn_finalise(sums, which, rows, gamma, beta, eps, momentum, running_mean, running_var, pack, stream)
    fin = lib.pfpp_ptf_train_bn_finalise
    assert fin(one, 3, 160, one, one, f(1e-5), f(0.1), one, one, one, None) == -1
    assert fin(one, 0, 1, one, one, f(1e-5), f(0.1), one, one, one, None) == -1              # the unbiased variance needs two rows
    assert fin(one, 0, 160, one, one, f(1e-5), f(1.5), one, one, one, None) == -1
    assert fin(None, 0, 160, one, one, f(1e-5), f(0.1), one, one, one, None) == -1 and b"null" in lib.pfpp_last_error()
    # the eval entry keeps its refusals
    assert lib.pfpp_ptf_aggregate(one, one, one, 384, one, one, one, one, 10, 128, 8, one, None) == -2


def test_engine_refuses_split_f16_and_cpu_tensors_and_the_module_still_refuses_train():
    from pfpp_hip import matching_transformer_train as MT
    from pfpp_hip.matching_transformer import CrossAttentionLayer, PointTransformerLayer

    assert MT.PTF_PARAM_NAMES == cases.GRAD_NAMES and MT.PTF_ZERO_GRADS == cases.ZERO_GRADS and MT.PTF_BN == cases.BN
    with pytest.raises(NotImplementedError, match="exact-fp32"):
        MT.PointTransformerTrainEngine(PointTransformerLayer(128, 128, 8, 16, gemm_mode="f16x3"))
    with pytest.raises(TypeError):
        MT.PointTransformerTrainEngine(CrossAttentionLayer(128, 8))
    layer = PointTransformerLayer(128, 128, 8, 16)
    eng = MT.PointTransformerTrainEngine(layer)
    assert tuple(eng.params) == MT.PTF_PARAM_NAMES and eng.layer is layer and not layer.training and len(eng.bns) == 3
    with pytest.raises(NotImplementedError, match="matcher training"):
        layer.train()
    p, x = torch.zeros(8, 3), torch.zeros(8, 128)
    with pytest.raises(ValueError, match="GPU"):
        eng.forward(p, x, [8])
    with pytest.raises(ValueError, match="GPU"):
        MT.PointTransformerFunction.apply(p, x.clone().requires_grad_(True), eng, [8])
    with pytest.raises(RuntimeError, match="before forward"):
        eng.backward(torch.zeros(8, 128))
    qkv, idx, pack = torch.zeros(8, 384), torch.zeros(8, 16, dtype=torch.int32), torch.zeros(MT.PTF_TRAIN_FLOATS)
    sq, d = torch.zeros(8, 16, 16), torch.zeros(1, dtype=torch.float64)
    for call in (lambda: MT.ptf_train_bn3_stats(p, idx, pack, d, d), lambda: MT.ptf_train_bn128_stats(qkv, p, idx, pack, d, d),
                 lambda: MT.ptf_train_tile(qkv, p, idx, pack, sq, d, d), lambda: MT.ptf_train_finish(qkv, p, idx, idx, pack, sq, sq),
                 lambda: MT.ptf_train_bwd_w(x, sq, sq, qkv, p, idx, idx, pack, sq, d, d), lambda: MT.ptf_train_bwd_u(qkv, p, idx, pack, sq, sq, d, d),
                 lambda: MT.ptf_train_bwd_r(x, sq, sq, qkv, p, idx, pack, qkv, d, d),
                 lambda: MT.ptf_train_bwd_gather(x, sq, sq, qkv, p, pack, idx, idx, idx, idx, qkv),
                 lambda: MT.ptf_train_bn_finalise(d, 0, 128, layer.linear_p[1], pack)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="which"):
        MT.ptf_train_bn_finalise(d, 3, 128, layer.linear_p[1], pack)
