"""GPU (-m gpu): the set-abstraction stage kernels of csrc/sa_train.hip (every launch statement behind pfpp_sa_train_stage, the
padding schedule) and their eval-mode siblings of csrc/sa_fused.hip, one launch per case inside guarded allocations, against the
float64 references of tests/sa_stage_cases.py, whose docstring defines the cases, the buffers, the units and the bounds.  Every test
prints the figures it measured before it asserts (`sa_stage ...` lines); profiles/sa_stage_errors.txt is that output for the whole
table."""
import importlib.util
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def load_cases():
    spec = importlib.util.spec_from_file_location("sa_stage_cases", ROOT / "tests" / "sa_stage_cases.py")
    mod = sys.modules.setdefault("sa_stage_cases", importlib.util.module_from_spec(spec))      # (registered: its dataclasses look themselves up)
    if not hasattr(mod, "CASES"):
        spec.loader.exec_module(mod)
    return mod


sc = load_cases()


def _run(dev, name):
    c = sc.CASES[name]
    rep, kernel = sc.run(c, dev)
    print(sc.describe(c, rep, kernel))
    for tag, e, bound in rep["lines"]:
        assert e <= bound, (name, tag, e, bound)
    for k, v in rep["flags"].items():
        assert v is True, (name, k)
    return rep, kernel


@pytest.mark.parametrize("name", sc.GROUPS["T"])
def test_t_train_stage(dev, name):
    """ops.sa_train_stage, every enumerator of SaKern: G = F S from 1 to 33 against grid caps from 1 workgroup to more than there is
    work, N in {33, 48, 64}, live-slot counts on both sides of 16 / 32 / 48 / 64 and lists in which slot 0 reappears, class mixes at
    the wrap points of the padding-aware walk, with a schedule and without; sums (over the copies, from non-zero starts), raw rows,
    max and min against float64 in units and at 2e-5 of the largest value; unwritten rows keep the sentinel; the reported kernel
    name; a second launch, another grid cap and the unscheduled twin reproduce rows, max and min bit for bit"""
    rep, kernel = _run(dev, name)
    c = sc.CASES[name]
    assert kernel == sc.KERN[c.kern].name
    assert rep["flags"]["repeat_bits"] and rep["flags"]["other_grid_bits"] and rep["flags"]["other_grid_stats"]
    if c.sched:
        assert any(k.startswith("schedule_keeps") for k in rep["flags"])


@pytest.mark.parametrize("name", sc.GROUPS["P"])
def test_p_pad_schedule(dev, name):
    """ops.sa_pad_schedule in bits against the numpy reference: one neighbourhood, around the 1024 threads of the scatter, at and
    above 32,768 neighbourhoods (more than 32 per thread: the scatter's second path)"""
    rep, _ = _run(dev, name)
    assert rep["flags"]["sched_bits"] and rep["flags"]["repeat_bits"]


@pytest.mark.parametrize("name", sc.GROUPS["E"])
def test_e_eval_forms(dev, name):
    """ops.sa_mlp3_fused, ops.sa_mlp2_fused (fp32 and planes), ops.sa_mlp2_table, ops.sa_table_planes into guarded outputs against
    the float64 grouped chain; the planes of sa_mlp2_fused keep the plane contract against the fp32 form's output"""
    rep, _ = _run(dev, name)
    assert rep["flags"]["repeat_bits"]
    if sc.CASES[name].kern == "mlp2_p":
        assert rep["flags"]["plane_contract"]


@pytest.mark.parametrize("ns,D", [(16, 0), (32, 128), (64, 64)])
def test_widths_the_abi_rejects_launch_nothing(dev, ns, D):
    """a neighbour count or feature width outside the three level shapes: PFPP_EUNSUPPORTED (code -2) and no kernel reported"""
    import torch
    from pfpp_hip import _lib, ops

    F, N, S, C1 = 1, 16, 2, 128 if D else 64
    xyz = torch.rand(F, N, 3, device=dev)
    feats = torch.randn(F, N, D, device=dev) if D else None
    idx = torch.zeros(F, S, ns, dtype=torch.int32, device=dev)
    planes = torch.zeros(C1, D + 8, dtype=torch.float16, device=dev)
    w = sc.gc._pw_shim(planes, planes.clone(), C1, D + 8)
    stats = torch.zeros(1, 2, C1, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.PfppError, match=r"code -2"):
        ops.sa_train_stage(1, xyz, xyz[:, :S].contiguous(), feats, idx, [w], [torch.zeros(C1, device=dev)], [], stats)
    assert _lib.load().pfpp_last_gemm_kernel().decode() == ""
    assert not bool(stats.any())
