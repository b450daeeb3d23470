"""GPU (-m gpu): the row-wise normalisation, reduction and element-wise kernels of csrc/transformer_ops.hip, csrc/train_ops.hip and
csrc/bn_train.hip at their row, channel and magnitude edges, inside guarded allocations, against the float64 references of
tests/rowop_cases.py, whose docstring defines the buffers, the units, the bounds and the cases.  Every test prints the figures it
measured before it asserts (`rowops ...` lines); profiles/rowops_errors.txt is that output for the whole table.  Every output,
plane pairs, statistics, loss and masks included, is written into a guarded allocation of the case; plane pairs also keep the bare
plane contract against the fp32 value of the same launch or of the fp32 form on the same inputs; L and D hold both of their bounds."""
import importlib.util
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("rowop_cases", ROOT / "tests" / "rowop_cases.py")
    mod = sys.modules.setdefault("rowop_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclasses look themselves up)
    if not hasattr(mod, "CASES"):
        spec.loader.exec_module(mod)
    return mod


rc = load_cases()


def _run(dev, name):
    c = rc.CASES[name]
    rep, flags = rc.run(c, dev)
    print(rc.describe(rep, flags))
    assert rep["guards_ok"], (name, "a guard row or column was written")
    assert rep["untouched_ok"], (name, "a row of dmult / dadd that no group refers to was written")
    for tag, e, bound in rep["lines"]:
        assert e <= bound, (name, c.entry, tag, e, bound)
    assert rep["bits_ok"], (name, "an output that is fixed bit for bit differs")
    for k, v in flags.items():
        assert v is not False, (name, k)
    return rep, flags


@pytest.mark.parametrize("name", rc.GROUPS["L"])
def test_l_layernorm_forward(dev, name):
    """pfpp_layernorm(_split) / pfpp_layernorm_grouped(_split): C in {256, 512, 1024}, 1 .. 37 rows around the 4-row workgroup, no
    affine / gamma, beta / mod with a last batch of one row / grouped with truncated last groups and an unused NaN row of mod,
    ld_mod = 2C + 8, rows far from zero mean, of zero variance and with one outlier; fp32 and split output; repeat launch"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True


@pytest.mark.parametrize("name", rc.GROUPS["D"])
def test_d_dropout_layernorm(dev, name):
    """pfpp_dropout_layernorm(_p): h has the bits of res + x keep / (1 - p) in float32 under the restated mask (p = 0 without a
    residual: the bits of y), n is the float64 LayerNorm of that h within the bound; every form of L once; repeat launch"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True


@pytest.mark.parametrize("name", rc.GROUPS["B"])
def test_b_layernorm_backward(dev, name):
    """pfpp_layernorm_bwd(_dropout, _p): group_rows 1 .. 33 (1 to 5 slices per group, slices shorter than 4 rows, empty slices of a
    truncated last group), several groups adding into one non-zero row of dmult / dadd, an unused row that keeps its bits, uniform
    batches, gamma with ld_d = 0, no multipliers; the fused dropout in bits from the returned dx; the plane outputs; dx repeats in bits"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True
    if rc.CASES[name].o("drop") is not None:
        assert flags["drop_bits"] is True


@pytest.mark.parametrize("name", rc.GROUPS["S"])
def test_s_column_sums_and_plane_split(dev, name):
    """pfpp_colsum on both kernels at the 64-row chunk and 256-column block edges, batched with sx / so, accumulate on and off,
    cols % 4 == 0 with ld % 4 != 0; pfpp_colsum_planes around its 16 rows per block and at 8200 x 8; pfpp_split_planes around the
    1024-element workgroup"""
    _run(dev, name)


@pytest.mark.parametrize("name", rc.GROUPS["G"])
def test_g_geglu_activations_dropout(dev, name):
    """pfpp_geglu(_p) / pfpp_geglu_bwd(_p) with gates in the tails of erff and expf, pfpp_act / pfpp_act_bwd, pfpp_dropout with
    n % 4 != 0 tails and p = 0 (a bit-exact copy-add), pfpp_dropout_mask against the restated generator; repeat launch"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True


@pytest.mark.parametrize("name", rc.GROUPS["N"])
def test_n_batchnorm(dev, name):
    """pfpp_bn_stats at the 2048-row slab edge, below the row phases, at one row, ld > C, |mean| / sigma up to 1000 and a constant
    channel; pfpp_bn_apply with ld, ldy > C and pooling; pfpp_bn_finalize; pfpp_bn_minmax_apply with negative, zero and positive
    multipliers; repeat launch"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True


@pytest.mark.parametrize("name", rc.GROUPS["P"])
def test_p_softmax_and_pooling(dev, name):
    """pfpp_softmax_rows (T around 64, ld in {T, T + 3}, masks, a fully masked batch, s scale up to +-80; every live row sums to 1
    within 64 2^-24), pfpp_mean_pool and pfpp_mean_pool_bwd; repeat launch"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True
    if rc.CASES[name].kind == "softmax":
        assert flags["row_sums"] is True


@pytest.mark.parametrize("name", rc.GROUPS["M"])
def test_m_loss(dev, name):
    """pfpp_mse_loss / pfpp_mse_loss_masked on both sides of the 1024 threads of the single workgroup; no / every / one / 20 % of the
    rows selected, NaN in every row that is not; the masked form equals the sel form in bits, amax is max |dpred| in bits"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True
    if rc.CASES[name].o("masked"):
        assert flags["same_bits_as_sel"] is True and flags["amax_bits"] is True


@pytest.mark.parametrize("name", rc.GROUPS["A"])
def test_a_adamw(dev, name):
    """pfpp_adamw / pfpp_adamw_guarded: three steps against float64 AdamW around the 256-element workgroup, planes, zero_grad,
    g_scale = 1 / 4096; non-finite gradients at both ends and at the workgroup edge keep p, m, v in bits, overflow = [1, count],
    every other element has the bits of the unguarded run"""
    _, flags = _run(dev, name)
    assert flags["repeat_bits"] is True
    if rc.CASES[name].o("guarded"):
        assert flags["same_bits_as_unguarded"] is True and flags["skipped_kept"] is True
