"""CPU: which path a set-abstraction level takes (pfpp_hip.encoder.choose_sa) and when the sampling chain is fused, as a table.
The expected plans are written out from the conditions of the encoder as it was while the paths were picked by module-level
switches (all at their defaults), not computed from the function."""
import pytest

L1 = dict(D=0, nsample=32, widths=(64, 64, 128))          # neighbourhoods = 256 per fragment
L2 = dict(D=128, nsample=64, widths=(128, 128, 256))      # 128 per fragment, 8,192 grouped rows
L3 = dict(D=256, nsample=64, widths=(256, 256, 512))      # 25 per fragment
PER_FRAGMENT = {0: 256, 128: 128, 256: 25}


def _cases():
    # (train, gemm_mode, split_act, single_pass, level, fragments, extra) -> (path, gather_in_gemm, table_first, pad_schedule)
    T, F_ = True, False
    rows = []

    def add(want, level, fragments, train=False, mode="f16x3", split=True, single=False, **extra):
        rows.append((dict(train=train, gemm_mode=mode, split_act=split and mode == "f16x3", single_pass=single,
                          neighbourhoods=fragments * PER_FRAGMENT[level["D"]], **{**level, **extra}), want))

    # ---- train mode: the chain on the three known shapes in split-f16 mode, whatever the activation format / pass count
    for split, single in ((True, False), (False, False), (True, True)):
        add(("TRAIN_CHAIN", T, F_, F_), L1, 154, train=True, split=split, single=single)
        add(("TRAIN_CHAIN", T, T, T), L2, 154, train=True, split=split, single=single)
        add(("TRAIN_CHAIN", T, T, T), L3, 154, train=True, split=split, single=single)
    add(("TRAIN_CHAIN", T, F_, F_), L1, 1, train=True)
    # the padding schedule on the table-fed 64-neighbour levels from 2,048 neighbourhoods up
    add(("TRAIN_CHAIN", T, T, F_), L2, 15, train=True)          # 1,920
    add(("TRAIN_CHAIN", T, T, T), L2, 16, train=True)           # 2,048
    add(("TRAIN_CHAIN", T, T, F_), L3, 81, train=True)          # 2,025
    add(("TRAIN_CHAIN", T, T, T), L3, 82, train=True)           # 2,050
    # other split-f16 calls: layer-wise fused-BatchNorm GEMMs, the first one gathering where the feature width allows
    add(("TRAIN_LAYERWISE", T, F_, F_), L2, 154, train=True, widths=(128, 128, 128))
    add(("TRAIN_LAYERWISE", T, F_, F_), L1, 154, train=True, nsample=64)
    add(("TRAIN_LAYERWISE", T, F_, F_), L3, 154, train=True, nsample=32)
    add(("TRAIN_LAYERWISE", F_, F_, F_), L2, 154, train=True, D=130)
    # materialised rows without the grouping tuple (utils/pn2_utils.py)
    add(("TRAIN_LAYERWISE", F_, F_, F_), L2, 154, train=True, grouped=False)
    add(("TRAIN_LAYERWISE", F_, F_, F_), L1, 154, train=True, grouped=False)
    add(("TRAIN_UNFUSED", F_, F_, F_), L2, 154, train=True, mode="f32", grouped=False)
    # exact fp32: bn_stats / bn_apply on materialised rows
    for lvl in (L1, L2, L3):
        add(("TRAIN_UNFUSED", F_, F_, F_), lvl, 154, train=True, mode="f32")

    # ---- eval mode
    for split, single in ((True, False), (False, False), (True, True)):
        add(("EVAL_MLP3", T, F_, F_), L1, 154, split=split, single=single)
    add(("EVAL_MLP3", T, F_, F_), L1, 1)
    # level 3 on the rows kernels always, with the schedule from 2,048 neighbourhoods up
    add(("EVAL_ROWS", T, T, F_), L3, 1)
    add(("EVAL_ROWS", T, T, F_), L3, 81)
    add(("EVAL_ROWS", T, T, T), L3, 82)
    add(("EVAL_ROWS", T, T, T), L3, 154)
    # level 2 on them from 200,000 grouped rows up
    add(("EVAL_MLP2", T, T, F_), L2, 1)
    add(("EVAL_MLP2", T, T, F_), L2, 24)            # 196,608 rows
    add(("EVAL_ROWS", T, T, T), L2, 25)             # 204,800 rows, 3,200 neighbourhoods
    add(("EVAL_ROWS", T, T, T), L2, 154)
    # fp32 activations between the kernels: no rows kernels, no per-point table
    add(("EVAL_MLP2", T, F_, F_), L2, 154, split=False)
    add(("EVAL_TILED", T, F_, F_), L3, 154, split=False)
    # single pass: no rows kernels, the table stays
    add(("EVAL_MLP2", T, T, F_), L2, 154, single=True)
    add(("EVAL_TILED", T, T, F_), L3, 154, single=True)
    # exact fp32: materialised rows, one GEMM per layer
    for lvl in (L1, L2, L3):
        add(("EVAL_TILED", F_, F_, F_), lvl, 154, mode="f32")
    # a feature width that is no multiple of 32: materialised rows
    add(("EVAL_TILED", F_, F_, F_), L2, 154, D=130)
    add(("EVAL_TILED", F_, F_, F_), L3, 154, D=250)
    # other shapes
    add(("EVAL_MLP2", T, T, F_), L2, 154, widths=(128, 128, 128))       # only the first two widths matter to sa_mlp2
    add(("EVAL_TILED", T, T, F_), L3, 154, widths=(256, 128, 128))      # table-fed first layer: (D, C1) = (256, 256) or (128, 128), 64 neighbours
    add(("EVAL_TILED", T, T, F_), L2, 154, widths=(128, 64, 128))
    add(("EVAL_TILED", T, F_, F_), L3, 154, widths=(128, 128, 128))
    add(("EVAL_TILED", T, F_, F_), L2, 154, nsample=32)
    add(("EVAL_TILED", T, F_, F_), L2, 154, D=64, widths=(64, 64, 128))
    add(("EVAL_TILED", T, F_, F_), L1, 154, nsample=64)
    add(("EVAL_TILED", T, F_, F_), L1, 154, widths=(64, 64, 64))
    return rows


@pytest.mark.parametrize("i", range(len(_cases())))
def test_set_abstraction_path_table(i):
    from pfpp_hip.encoder import SaPath, SaPlan, choose_sa

    kw, (path, gather, table, pad) = _cases()[i]
    assert choose_sa(**kw) == SaPlan(SaPath[path], gather, table, pad), kw


def test_thresholds_are_the_measured_ones():
    from pfpp_hip import encoder

    assert (encoder.EVAL_ROWS_MIN_ROWS_128, encoder.PAD_SCHEDULE_MIN_NEIGHBOURHOODS, encoder.SAMPLE_FUSED_MIN_FRAGMENTS) == (200_000, 2048, 32)


@pytest.mark.parametrize("fragments,supported,want", [(31, True, False), (32, True, True), (154, True, True), (32, False, False),
                                                      (154, False, False), (1, True, False)])
def test_fused_sampling_rule(fragments, supported, want):
    from pfpp_hip.encoder import fused_sampling

    assert fused_sampling(fragments, supported) is want
