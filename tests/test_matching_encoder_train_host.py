"""CPU: the float64 restatement of the encoder's training step (tests/matching_encoder_train_cases.py) against
tests/golden/matching_encoder_train.npz, which holds what the reference's own PointNet2PTMSGDynamic returned in .train() under autograd
(tools/make_matching_encoder_train_goldens.py).  The GPU tests compare the engine with this restatement; here it is pinned to the
reference, each deliberate misreading is shown to leave the fixture, and the fixture's own conditions are checked."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def load_cases(stem):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tc = load_cases("matching_encoder_train_cases")
base = tc.base
_REF = {}
PIN = 1e-11          # float64 rounding through some forty layers and sums over up to 13,000 rows, relative to a tensor's maximum


def restated(name, mutate=None):
    key = (name, mutate)
    if key not in _REF:
        pts, lengths, start = tc.flat_case(name)
        res = tc.restate(base.encoder_state_dict(), pts, tc.cpu_indices(pts, lengths, start), tc.make_dout(name, len(pts)), mutate=mutate)
        _REF[key] = (tc.fixture_tensors(res), res)
    return _REF[key]


def vanishing(fx):
    """the tensors that are rounding noise in the reference itself: its float32 run deviates from its float64 run by more than the
    tensor's largest magnitude.  They vanish in exact arithmetic: in `solo` the one centroid of level 4 is broadcast to fp4's two
    rows, whose BatchNorm removes what the rows share, so no gradient reaches sa4; and the rows of a BatchNorm's input gradient sum to
    zero, so the beta of a pooled layer all of whose maxima are positive gets none."""
    return {k for k, v in fx["refdev"].items() if v >= 1.0}


def allowed(fx, key):
    """the pin of a tensor, relative to its largest magnitude: PIN, or 64 x the float64 noise that the reference's own float32 noise
    predicts (float64 carries 29 more bits) where that is more — `solo` normalises over 2 to 32 rows and its float32 run is 3 % off"""
    return max(PIN, 64.0 * 2.0 ** -29 * fx["refdev"][key])


def distance(name, tensors):
    """per tensor: the largest deviation of its samples from the fixture's, relative to the tensor's largest magnitude (a sum's
    relative to that times its number of terms)"""
    fx = tc.load_fixture(name)
    out = {}
    for key, arr in tensors.items():
        worst = 0.0
        mag = fx["max"][key]
        for kind, got in tc.sample(arr).items():
            want = fx["samples"][f"{key}/{kind}"]
            assert want.shape == got.reshape(-1).shape, (key, kind)
            scale = mag * (1 if kind in ("full", "rows") else arr.reshape(arr.shape[0], -1).shape[1 if kind == "rowsum" else 0])
            worst = max(worst, float(np.abs(got.reshape(-1) - want).max() / max(scale, 1e-300)))
        out[key] = worst
    return out


def conv_biases():
    return ["grad." + cp + ".bias" for _, cp, _ in tc.layer_names()]


@pytest.mark.parametrize("name", tc.FIXTURE_CASES)
def test_restatement_equals_the_reference_in_float64(name):
    tensors, _ = restated(name)
    fx = tc.load_fixture(name)
    assert len(tensors) == 5 + 134 + 66 and set(fx["refdev"]) == set(tensors)
    dist = {k: v / allowed(fx, k) for k, v in distance(name, {k: v for k, v in tensors.items() if k not in conv_biases()}).items()}
    worst = max(dist, key=dist.get)
    print(f"{name}: {len(dist)} tensors ({len(vanishing(fx))} vanish in exact arithmetic), worst {dist[worst]:.3g} of its pin ({worst}, pin "
          f"{allowed(fx, worst):.3g} of the maximum)")
    assert dist[worst] <= 1.0


@pytest.mark.parametrize("mutate", tc.MUTATIONS)
def test_each_misreading_leaves_the_fixture(mutate):
    """on `small`: some tensor is further from the fixture than 1,000 x the bar the GPU tests use for it.  Not so for the padded
    interpolation slots: a padded slot's weight is 1e-8 / (sum of 1 / d), about 1e-8 of the real ones, so dropping it moves the
    worst gradient by 1e-8 of its maximum — below every float32 bar, and 1,000 x this file's float64 pin, which is what is asserted"""
    fx = tc.load_fixture("small")
    tensors, _ = restated("small", mutate)
    dist = distance("small", {k: v for k, v in tensors.items() if k not in conv_biases() and k not in vanishing(fx)})
    bars = max(dist[k] / max(4 * fx["refdev"][k], 4 * 2.0 ** -23) for k in dist)
    pins = max(dist[k] / allowed(fx, k) for k in dist)
    print(f"{mutate}: worst tensor at {bars:.3g} float32 bars, {pins:.3g} float64 pins")
    assert pins >= 300.0 if mutate == "drop_padded" else bars >= 1000.0


@pytest.mark.parametrize("name", tc.FIXTURE_CASES)
def test_conv_bias_gradients_vanish_in_the_reference(name):
    """the 33 convolution biases sit in front of a batch-statistics BatchNorm: in the reference's float64 run their gradients are at
    rounding level against the weight gradient of the same convolution (the engine writes exact zeros)"""
    fx = tc.load_fixture(name)
    worst = max(float(np.abs(fx["samples"][k + "/full"]).max()) / fx["max"][k[:-len("bias")] + "weight"] for k in conv_biases())
    _, res = restated(name)
    mine = max(float(res["grad"][k[5:]].abs().max()) / fx["max"][k[:-len("bias")] + "weight"] for k in conv_biases())
    print(f"{name}: largest conv-bias gradient / largest weight gradient of its layer: reference {worst:.3g}, restatement {mine:.3g}")
    assert worst <= 1e-10 and mine <= 1e-10
    assert abs(fx["max"]["grad.conv1.bias"]) > 1e-3          # conv1 has no BatchNorm behind it: its bias gradient is real


def test_solo_shrinks_to_one_centroid_with_two_rows_in_fp4():
    counts = base.level_counts(np.asarray(tc.SOLO_LENGTHS))[:, 0].tolist()
    assert counts == [200, 31, 8, 2, 1]
    assert base.level_counts(np.asarray([30]))[:, 0].tolist() == [30, 5, 2, 1, 1]
    pts, lengths, start = tc.flat_case("solo")
    idx = tc.cpu_indices(pts, lengths, start)
    assert idx["back"][3] is None and idx["back"][2] is not None


@pytest.mark.parametrize("name", tc.FIXTURE_CASES)
def test_the_references_own_float32_run_stays_under_the_flip_cap(name):
    """in the fixture the reference's float32 run differs from its float64 run in at most 1 ReLU sign per 10,000 per layer, and in at
    most 1 pool winner per 10,000 per pool (DESIGN.md 5.9's cap): the deviations the bars are built from are rounding, not decisions"""
    fx = tc.load_fixture(name)
    assert len(fx["flips"]) == 33 and len(fx["winflips"]) == 8
    worst = max((n / size, k) for k, (n, size) in {**fx["flips"], **{"pool " + k: v for k, v in fx["winflips"].items()}}.items())
    print(f"{name}: worst share of differing decisions {worst[0]:.3g} ({worst[1]}); cap {tc.FLIP_CAP:.0e}")
    assert worst[0] <= tc.FLIP_CAP


def test_the_case_files_are_consistent():
    assert [n for n, _, _ in tc.layer_names()] == [str(s) for s in np.load(ROOT / "tests" / "golden" / "matching_encoder_train.npz")["layers"]]
    assert tc.make_case("small")[0] is base.make_puzzle(base.CASES["small"][0])          # the base file's puzzle, untouched
    assert (ROOT / "tests" / "golden" / "matching_encoder_train.npz").stat().st_size < 600 * 1024
