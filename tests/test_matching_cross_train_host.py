"""CPU: the host side of the cross-attention layer's training (pfpp_hip/matching_transformer_train.py) and the test-side oracle of
tests/matching_cross_train_cases.py against tests/golden/matching_cross_train.npz, which tools/make_matching_cross_train_goldens.py
wrote from the reference's own CrossAttentionLayer in .train() under autograd.

The restatement in float64 must equal the fixture's float64 gradients to 1e-12 of each tensor's largest magnitude (the same
operations in the same precision) with no ReLU sign pattern differing, so the GPU tests may lean on it.  Every test prints what it
measured before it asserts."""
import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("pfpp_attn_rows16_train", "pfpp_attn_rows16_bwd", "pfpp_layernorm128_bwd", "pfpp_relu_bwd")


def load_cases():
    spec = importlib.util.spec_from_file_location("matching_cross_train_cases", ROOT / "tests" / "matching_cross_train_cases.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = load_cases()


@pytest.mark.parametrize("name", ["tiny", "pair"])
def test_restatement_in_float64_equals_the_reference_to_1e_12(golden, name):
    g = golden("matching_cross_train")
    x, puz, dout = cases.case_inputs(name)
    assert [str(k) for k in g["names"]] == list(cases.TENSORS) and int(g["row_step"]) == cases.ROW_STEP
    r = cases.cross_train_restate(cases.base.cross_state_dict(), x, puz, dout, torch.float64)
    flips, entries = int(g[f"{name}_relu_flips"]), int(g[f"{name}_relu_entries"])
    print(f"{name}: the reference's float32 and float64 ReLU patterns differ in {flips} of {entries} entries; smallest float64 "
          f"|pre-activation| {float(g[f'{name}_pre_min_abs']):.3g} (restated: {float(r['pre'].abs().min()):.3g})")
    assert flips == 0 and entries == r["pre"].numel()
    assert abs(float(r["pre"].abs().min()) - float(g[f"{name}_pre_min_abs"])) <= 1e-12
    worst = 0.0
    for key in cases.TENSORS:
        top = float(g[f"{name}_{key}_max"])
        for part, got in cases.sample(r[key].numpy()).items():
            want = g[f"{name}_{key}_{part}"]
            scale = top * (1 if part in ("full", "rows") else max(r[key].shape))         # a sum of n entries
            err = float(np.abs(got - want).max() / scale)
            worst = max(worst, err)
            assert got.shape == want.shape and want.dtype == np.float64 and err <= 1e-12, (key, part, err)
        assert 0 < float(g[f"{name}_{key}_refdev"]) < 2e-6
    print(f"{name}: restatement vs the reference's float64 gradients, worst of {len(cases.TENSORS)} tensors {worst:.3g} of the maximum (bar 1e-12)")


def test_restatement_with_its_own_relu_pattern_is_itself_and_a_flipped_entry_shows():
    x, puz, dout = cases.case_inputs("tiny")
    sd = cases.base.cross_state_dict()
    r = cases.cross_train_restate(sd, x, puz, dout, torch.float64)
    mask = (r["pre"] > 0).numpy()
    m = cases.cross_train_restate(sd, x, puz, dout, torch.float64, relu_mask=mask)
    assert all(torch.equal(r[k], m[k]) for k in cases.TENSORS)
    i, j = np.unravel_index(np.argmax(r["pre"].numpy()), mask.shape)                     # the most active entry switched off
    mask[i, j] = False
    f = cases.cross_train_restate(sd, x, puz, dout, torch.float64, relu_mask=mask)
    assert not torch.equal(r["dx"], f["dx"]) and not torch.equal(r["pos_ffn.w_2.weight"], f["pos_ffn.w_2.weight"])


def test_header_declares_the_entries_and_arguments_are_checked_before_a_launch(hip_lib):
    from pfpp_hip import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pfpp.h").read_text(), flags=re.S)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", text), f"{s} not declared in include/pfpp.h"
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.pfpp_version() == 2 and "#define PFPP_LAYERNORM128_BWD_MAX_WG 256" in text
    from pfpp_hip import matching_transformer_train as MT

    assert MT.LN128_BWD_WS_FLOATS == 256 * 4 * 2 * 128 and "PFPP_LAYERNORM128_BWD_WS_FLOATS (PFPP_LAYERNORM128_BWD_MAX_WG * 4 * 2 * 128)" in text
    one = C.c_void_p(4096)            # a non-null, 16-byte aligned address that is never dereferenced on these paths
    f = C.c_float
    # pfpp_attn_rows16_train(qkv, out, lse, seq_off, seq_len, n_seq, max_len, H, dh, scale, stream)
    assert lib.pfpp_attn_rows16_train(one, one, one, one, one, 0, 10, 8, 16, f(0.25), None) == 0                 # no sequence: nothing to do
    assert lib.pfpp_attn_rows16_train(one, one, one, one, one, 2, 10, 8, 32, f(0.25), None) == -2 and b"16" in lib.pfpp_last_error()
    assert lib.pfpp_attn_rows16_train(one, one, None, one, one, 2, 10, 8, 16, f(0.25), None) == -1 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_attn_rows16_train(one, None, one, one, one, 2, 10, 8, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16_train(one, one, one, one, one, 2, 0, 8, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16_train(C.c_void_p(4104), one, one, one, one, 2, 10, 8, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16_train(one, one, one, one, one, 70000, 10, 8, 16, f(0.25), None) == -2
    # pfpp_attn_rows16_bwd(qkv, out, dout, lse, dvec, dqkv, seq_off, seq_len, n_seq, max_len, H, dh, scale, stream)
    assert lib.pfpp_attn_rows16_bwd(one, one, one, one, one, one, one, one, 0, 10, 8, 16, f(0.25), None) == 0
    assert lib.pfpp_attn_rows16_bwd(one, one, one, one, one, one, one, one, 2, 10, 8, 32, f(0.25), None) == -2 and b"16" in lib.pfpp_last_error()
    assert lib.pfpp_attn_rows16_bwd(one, one, one, one, one, one, one, one, 2, 10, 8, 64, f(0.25), None) == -2
    for hole in range(8):             # every pointer
        args = [one] * 8
        args[hole] = None
        assert lib.pfpp_attn_rows16_bwd(*args, 2, 10, 8, 16, f(0.25), None) == -1 and b"null" in lib.pfpp_last_error(), hole
    assert lib.pfpp_attn_rows16_bwd(one, one, C.c_void_p(4100), one, one, one, one, one, 2, 10, 8, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16_bwd(one, one, one, one, one, one, one, one, 2, 10, 0, 16, f(0.25), None) == -1
    assert lib.pfpp_attn_rows16_bwd(one, one, one, one, one, one, one, one, 2, 10, 70000, 16, f(0.25), None) == -2
    # pfpp_layernorm128_bwd(x, dy, gamma, dx, dgamma, dbeta, workspace, rows, C, eps, accumulate_dx, stream)
    assert lib.pfpp_layernorm128_bwd(one, one, one, one, one, one, one, 0, 128, f(1e-6), 0, None) == 0
    assert lib.pfpp_layernorm128_bwd(one, one, one, one, one, one, one, 10, 256, f(1e-6), 0, None) == -2 and b"128" in lib.pfpp_last_error()
    assert lib.pfpp_layernorm128_bwd(one, one, one, one, one, one, one, 10, 64, f(1e-6), 1, None) == -2
    for hole in range(7):
        args = [one] * 7
        args[hole] = None
        assert lib.pfpp_layernorm128_bwd(*args, 10, 128, f(1e-6), 0, None) == -1 and b"null" in lib.pfpp_last_error(), hole
    assert lib.pfpp_layernorm128_bwd(one, one, one, one, one, one, one, 10, 128, f(-1.0), 0, None) == -1
    assert lib.pfpp_layernorm128_bwd(one, one, one, one, one, one, one, -1, 128, f(1e-6), 0, None) == -1
    # pfpp_relu_bwd(h, dh, rows, cols, ld, stream)
    assert lib.pfpp_relu_bwd(one, one, 0, 256, 256, None) == 0
    assert lib.pfpp_relu_bwd(None, one, 4, 256, 256, None) == -1 and b"null" in lib.pfpp_last_error()
    assert lib.pfpp_relu_bwd(one, None, 4, 256, 256, None) == -1
    assert lib.pfpp_relu_bwd(one, one, 4, 256, 128, None) == -1                                                  # row stride below the width
    # the forward entries and the dense backward keep their refusals
    assert lib.pfpp_attn_rows16(one, one, one, one, 2, 10, 8, 32, f(0.25), None) == -2
    assert lib.pfpp_attn_dense_bwd(one, one, one, one, one, one, one, one, None, 0, 2, 10, 8, 16, f(0.25), None) == -2


def test_engine_refuses_split_f16_and_cpu_tensors_and_the_module_still_refuses_train():
    from pfpp_hip.matching_transformer import CrossAttentionLayer
    from pfpp_hip.matching_transformer_train import (PARAM_NAMES, CrossAttentionFunction, CrossAttentionTrainEngine, attn_rows16_bwd,
                                                     attn_rows16_train, layernorm128_bwd, relu_bwd)

    assert PARAM_NAMES == cases.GRAD_NAMES
    with pytest.raises(NotImplementedError, match="exact-fp32"):
        CrossAttentionTrainEngine(CrossAttentionLayer(128, 8, gemm_mode="f16x3"))
    with pytest.raises(TypeError):
        CrossAttentionTrainEngine(torch.nn.Linear(4, 4))
    layer = CrossAttentionLayer(128, 8)
    eng = CrossAttentionTrainEngine(layer)
    assert tuple(eng.params) == PARAM_NAMES and eng.layer is layer and not layer.training
    with pytest.raises(NotImplementedError, match="matcher training"):
        layer.train()
    with pytest.raises(NotImplementedError):
        layer.train(True)
    with pytest.raises(ValueError, match="GPU"):
        eng.forward(torch.zeros(8, 128), [8])
    with pytest.raises(ValueError, match="GPU"):
        CrossAttentionFunction.apply(torch.zeros(8, 128, requires_grad=True), eng, [8])
    with pytest.raises(RuntimeError, match="before forward"):
        eng.backward(torch.zeros(8, 128))
    i32 = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        attn_rows16_train(torch.zeros(8, 384), i32, i32, 8, 8, 0.25)
    with pytest.raises(ValueError, match="GPU"):
        attn_rows16_bwd(torch.zeros(8, 384), torch.zeros(8, 128), torch.zeros(8, 128), torch.zeros(8, 8), i32, i32, 8, 8, 0.25)
    with pytest.raises(ValueError, match="GPU"):
        layernorm128_bwd(torch.zeros(8, 128), torch.zeros(8, 128), torch.ones(128), 1e-6)
    with pytest.raises(ValueError, match="GPU"):
        relu_bwd(torch.zeros(8, 256), torch.zeros(8, 256))
