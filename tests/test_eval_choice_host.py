"""CPU: which kernels an eval / sampler step of the denoiser takes (pfpp_hip.denoiser.choose_eval), as a table, and which explicit
plans a call refuses (check_plan).  The expected plans are written out from the conditions of denoiser.py as it was while the step was
steered by environment switches (PFPP_HEADS_FUSED, PFPP_EVAL_CSEQ, PFPP_EVAL_LNLIN_ROWS, PFPP_EVAL_WD, PFPP_EMBED_FUSED,
PFPP_EVAL_WD_FULL, all at their defaults), not computed from the function:
  embedding in one launch   tokens <= 2048 and the packed [C, 320] weight exists and split-f16 planes and not single pass and not traced
                            and L >= 11 and latent width 64 (compact forward only)
  blocks from C             split-f16 planes and not traced and every block weight has N % 32 == 0, K % 16 == 0 (compact forward only);
                            the call then passes lnlin_max_rows = 2048, wd_gemm = 1
  else from Python          weight-direct GEMMs iff traced and split-f16 planes and not single pass and tokens > 2048 and C % 128 == 0
  fused heads               f16x3 mode and width 512
  all-slots forward         embedding layer-wise, blocks from Python on the tiled GEMM, fused heads as above
A plan for blocks issued from Python carries lnlin_max_rows = 0 and wd_gemm = (blocks is PY_WD): that sequence has no few-token kernels."""
import dataclasses
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BASE = dict(compact=True, gemm_mode="f16x3", split_act=True, single_pass=False, traced=False, tokens=500, C=512, inner=2048, L=25,
            latent_dim=64, embed_packed=True)


def _cases():
    # facts that differ from BASE -> (embed_fused, blocks, lnlin_max_rows, wd_gemm, heads_fused)
    T, F_ = True, False
    rows = []

    def add(want, **facts):
        rows.append(({**BASE, **facts}, want))

    # ---- compact forward, parity arithmetic: both sides of the few-token range
    add((T, "C_SEQUENCED", 2048, T, T))
    add((T, "C_SEQUENCED", 2048, T, T), tokens=25)
    add((T, "C_SEQUENCED", 2048, T, T), tokens=2048)
    add((F_, "C_SEQUENCED", 2048, T, T), tokens=2049)
    add((F_, "C_SEQUENCED", 2048, T, T), tokens=3850)
    # ---- the traced pass: blocks from Python, weight-direct above the few-token range only; the one-launch embedding is never traced
    add((F_, "PY_TILED", 0, F_, T), traced=True)
    add((F_, "PY_TILED", 0, F_, T), traced=True, tokens=2048)
    add((F_, "PY_WD", 0, T, T), traced=True, tokens=2049)
    add((F_, "PY_TILED", 0, F_, T), traced=True, tokens=2049, single_pass=True)
    add((F_, "PY_TILED", 0, F_, T), traced=True, tokens=2049, split_act=False)
    add((F_, "PY_WD", 0, T, F_), traced=True, tokens=2049, C=384)
    add((F_, "PY_TILED", 0, F_, F_), traced=True, tokens=2049, C=320)
    # ---- exact fp32 and fp32 hand-over between the kernels: no planes, so neither the sequencer nor the one-launch embedding
    add((F_, "PY_TILED", 0, F_, F_), gemm_mode="f32")
    add((F_, "PY_TILED", 0, F_, F_), gemm_mode="f32", tokens=2049)
    add((F_, "PY_TILED", 0, F_, F_), gemm_mode="f32", tokens=2049, traced=True)
    add((F_, "PY_TILED", 0, F_, F_), gemm_mode="f32", split_act=False)
    add((F_, "PY_TILED", 0, F_, T), split_act=False)
    add((F_, "PY_TILED", 0, F_, T), split_act=False, tokens=2049)
    # ---- single pass: the sequencer (it passes the mode on), the layer-wise embedding
    add((F_, "C_SEQUENCED", 2048, T, T), single_pass=True)
    add((F_, "C_SEQUENCED", 2048, T, T), single_pass=True, tokens=2049)
    # ---- widths: the heads kernel is the 512-wide one; the fragment-blocked layout needs N % 32 == 0 and K % 16 == 0
    add((T, "C_SEQUENCED", 2048, T, F_), C=384)
    add((F_, "C_SEQUENCED", 2048, T, F_), C=384, tokens=2049)
    add((T, "PY_TILED", 0, F_, T), inner=2056)
    add((F_, "PY_TILED", 0, F_, T), inner=2056, tokens=2049)
    # ---- the one-launch embedding's own limits
    add((F_, "C_SEQUENCED", 2048, T, T), L=10)
    add((T, "C_SEQUENCED", 2048, T, T), L=11)
    add((F_, "C_SEQUENCED", 2048, T, T), latent_dim=32)
    add((F_, "C_SEQUENCED", 2048, T, T), embed_packed=False)
    # ---- all slots evaluated: never the sequencer, the one-launch embedding or (by itself) the weight-direct GEMMs
    add((F_, "PY_TILED", 0, F_, T), compact=False, tokens=16000)
    add((F_, "PY_TILED", 0, F_, T), compact=False, tokens=500)
    add((F_, "PY_TILED", 0, F_, T), compact=False, tokens=16000, traced=True)
    add((F_, "PY_TILED", 0, F_, T), compact=False, tokens=16000, single_pass=True)
    add((F_, "PY_TILED", 0, F_, T), compact=False, tokens=16000, split_act=False)
    add((F_, "PY_TILED", 0, F_, F_), compact=False, tokens=16000, gemm_mode="f32")
    add((F_, "PY_TILED", 0, F_, F_), compact=False, tokens=16000, C=384)
    return rows


@pytest.mark.parametrize("i", range(len(_cases())))
def test_eval_plan_table(i):
    from pfpp_hip.denoiser import EvalBlocks, EvalPlan, check_plan, choose_eval

    facts, (embed, blocks, rows, wd, heads) = _cases()[i]
    plan = choose_eval(**facts)
    assert plan == EvalPlan(embed, EvalBlocks[blocks], rows, wd, heads), facts
    check_plan(plan, **facts)                                   # the library's own choice is always one the call can honour


def test_widths_a_kernel_refuses_are_not_chosen():
    """the rows that are NOT the former conditions': there the former code named a kernel and the step then raised in the middle.
    Traced, above the few-token range, a feed-forward width that is no multiple of 32: the former condition (C % 128 == 0 alone) said
    weight-direct and PW.frag / pfpp_gemm_wd refused the second feed-forward linear; the choice now reads pfpp_gemm_wd_supported's
    whole rule and the step runs tiled.  A width that is no multiple of 32: the former condition had no clause on C for the one-launch
    embedding, whose kernel needs C % 32 == 0; the step now embeds layer-wise."""
    from pfpp_hip.denoiser import EvalBlocks, EvalPlan, choose_eval

    assert choose_eval(**{**BASE, "C": 400}) == EvalPlan(False, EvalBlocks.PY_TILED, 0, False, False)               # 400 % 32 = 16
    assert choose_eval(**{**BASE, "traced": True, "tokens": 2049, "inner": 2056}).blocks is EvalBlocks.PY_TILED
    assert choose_eval(**{**BASE, "traced": True, "tokens": 2049, "inner": 2064}).blocks is EvalBlocks.PY_TILED      # K % 16 == 0, K % 32 != 0
    assert choose_eval(**{**BASE, "traced": True, "tokens": 2049, "inner": 2080}).blocks is EvalBlocks.PY_WD


def test_few_token_range_is_the_measured_one():
    from pfpp_hip import denoiser

    assert denoiser.EVAL_FEW_TOKEN_MAX_ROWS == 2048


@pytest.mark.parametrize("C,inner,want", [(512, 2048, True), (384, 1536, True), (400, 2048, False), (512, 2056, False), (512, 2064, True),
                                          (32, 16, True)])
def test_fragment_blocked_layout_predicate(C, inner, want):
    from pfpp_hip.denoiser import frag_covers_blocks

    assert frag_covers_blocks(C, inner) is want


def _refusals():
    # (changes to the default plan of BASE + facts, facts)
    return [
        (dict(heads_fused=True), dict(C=384)),
        (dict(heads_fused=True), dict(gemm_mode="f32")),
        (dict(blocks="C_SEQUENCED"), dict(gemm_mode="f32")),
        (dict(blocks="C_SEQUENCED"), dict(split_act=False)),
        (dict(blocks="C_SEQUENCED"), dict(traced=True)),
        (dict(blocks="C_SEQUENCED"), dict(inner=2056)),
        (dict(blocks="C_SEQUENCED"), dict(compact=False, tokens=16000)),
        (dict(blocks="PY_WD"), dict(single_pass=True)),
        (dict(blocks="PY_WD"), dict(gemm_mode="f32")),
        (dict(blocks="PY_WD"), dict(C=320)),
        (dict(blocks="PY_WD"), dict(inner=2064)),
        (dict(embed_fused=True), dict(compact=False, tokens=16000)),
        (dict(embed_fused=True), dict(L=10)),
        (dict(embed_fused=True), dict(C=400)),
        (dict(embed_fused=True), dict(latent_dim=32)),
        (dict(embed_fused=True), dict(embed_packed=False)),
        (dict(embed_fused=True), dict(single_pass=True)),
        (dict(embed_fused=True), dict(gemm_mode="f32")),
        (dict(lnlin_max_rows=-1), dict()),
    ]


@pytest.mark.parametrize("i", range(len(_refusals())))
def test_check_plan_refuses_what_the_call_cannot_honour(i):
    from pfpp_hip.denoiser import EvalBlocks, check_plan, choose_eval

    change, delta = _refusals()[i]
    facts = {**BASE, **delta}
    if "blocks" in change:
        change = dict(change, blocks=EvalBlocks[change["blocks"]])
    plan = dataclasses.replace(choose_eval(**facts), **change)
    with pytest.raises(ValueError, match="EvalPlan not possible"):
        check_plan(plan, **facts)


def test_check_plan_accepts_the_cross_check_plans():
    """what the GPU tests pass: layer-wise heads, the Python sequence on the tiled GEMM, the sequencer without few-token kernels, and
    the weight-direct GEMMs with all slots evaluated (by argument only)"""
    from pfpp_hip.denoiser import EvalBlocks, check_plan, choose_eval

    default = choose_eval(**BASE)
    for change in (dict(heads_fused=False), dict(embed_fused=False), dict(lnlin_max_rows=0, embed_fused=False, blocks=EvalBlocks.PY_TILED),
                   dict(lnlin_max_rows=0, embed_fused=False), dict(wd_gemm=False), dict(blocks=EvalBlocks.PY_WD)):
        check_plan(dataclasses.replace(default, **change), **BASE)
    full = {**BASE, "compact": False, "tokens": 16000}
    check_plan(dataclasses.replace(choose_eval(**full), blocks=EvalBlocks.PY_WD), **full)
    with pytest.raises(dataclasses.FrozenInstanceError):
        default.heads_fused = False


def test_the_step_reads_no_environment():
    src = (ROOT / "puzzlefusion-plusplus_amd" / "pfpp_hip" / "denoiser.py").read_text()
    assert "environ" not in src and "getenv" not in src
    for name in ("gemm_wd.hip", "gemm_small.hip"):
        assert "getenv" not in (ROOT / "puzzlefusion-plusplus_amd" / "csrc" / name).read_text(), name
