"""Case table, float64 reference, CPU yardstick and error report of the set-abstraction stage kernels (no test in here; importable
without a GPU).  tests/test_sa_stage_cases_host.py checks the table itself on the CPU, tests/test_gpu_sa_stage_edges.py runs it
through the HIP kernels, `python tests/sa_stage_cases.py --yardstick` prints the yardstick figures behind K and
`python tests/sa_stage_cases.py --report` (GPU) prints one line per case (profiles/sa_stage_errors.txt).

One case is ONE launch through a wrapper of pfpp_hip.ops.
  T  ops.sa_train_stage: every launch statement behind pfpp_sa_train_stage (KERN: the 13 enumerators of SaKern in csrc/sa_train.hip),
     the schedule-taking ones with and without a schedule; each case asserts the reported kernel name.
  P  ops.sa_pad_schedule, G up to 40,000 (the scatter's per > PER_REG path), against a numpy reference, in bits.
  E  the eval forms: ops.sa_mlp3_fused, ops.sa_mlp2_fused (fp32 and planes), ops.sa_mlp2_table, ops.sa_table_planes.

Shapes.  The widths are fixed by the ABI; F, N, S, the index lists and ops.PERSISTENT_WGS vary (PAIRS: G = F S in {1, 3, 4, 5, 8, 9,
15, 33} against grid caps {None, 1, 2, 3, 8, 9, 17, 40}; grids() restates persistent_grid / rows_grid, so the host test can show
that the table has one workgroup per slice, workgroups without work and G on both sides of a round).  N in {33, 48, 64}; every
case's index tensor contains 0 and N - 1 and never NAN_ROW = N - 2, the point row that holds NaN.  64-neighbour levels: live-slot
counts LIVE_SET, the tail filled with slot 0 as the ball query fills it, two lists in which slot 0's index reappears inside the live
part (the count is by definition 1 + the highest slot that differs from slot 0: live_counts()), and class mixes n2 in {0, G, 1,
stride - 1, stride, stride + 1} (the wrap arithmetic of PadWalk) for the stride of the launch; every such list is run with the
schedule and without.

Operands (profiles).  Weights are random in every channel and K position, biases non-zero.  Finalised affines by channel c % 4:
positive multiplier, negative multiplier, multiplier exactly 0, add -1e3 (dead after ReLU).  "span": rows of every weight matrix
(and the biases) are scaled by a permutation of logspace(-3, 2) and the multipliers by the inverse, so that the pre-activations of
every layer span 1e-3 .. 1e2 (inside the split-f16 range of DESIGN.md section 5.0).  "offset": the fragment sits at 4 +- 0.3, so
that the cancellation in U[p] - W_xyz . c is inside the unit.  Coordinates otherwise in [-1, 1].

Buffers (rules and constants of tests/gemm_cases.py).  Every input and output lives in a taller allocation of its own.  Input
guards hold NaN, idx guards NAN_ROW, output guards SENTINEL (planes: SENTINEL_F16, the schedule: SENTINEL_I32) and must keep their
bits; inputs must keep all their bits.  Operands the wrapper wants but the launch must not read (the earlier layers' planes and
biases of a rows stage) are NaN throughout.  stats starts from non-zero values of the size of what is added, copies in {1, 3, 64};
the check is on the sum over copies.  Raw rows of slots >= live are never written under a schedule: they keep SENTINEL after
stage 2, and hold NaN when fed to rows8 and wide stages 2 / 3 (without a schedule they hold row 0's values, as an unscheduled
stage 2 writes them).  The schedule a T case is given is the numpy reference's, not the kernel's (group P pins that).

Reference: float64 from the values the operands stand for ((hi + lo) of a weight plane, the fp32 values otherwise): gather, conv +
bias, relu(y a_mul + a_add) per finalised layer, then sum(y), sum(y^2) over all F S ns rows (copies included), the raw rows, the
per-neighbourhood max and min.  The table-fed forms are judged against the same grouped convolution; the table a T case is given
is the fp32 rounding of the float64 per-point convolution.

Units (first-order forward error, from the reference's float64 intermediates only):
  u(y) = 2^-20 sum_k |a_k||w_k| + sum_k |w_k| u(a_k);   u(a) = |a_mul| u(y_prev) + 2^-24 (|y_prev a_mul| + |a_add|), and 0 where
  the normalised value is below -1024 u (ReLU returns an exact 0);  gathered coordinates: u = 2^-24 |q - c|;  table forms:
  + 2^-24 (|U[p]| + |W_xyz . c|) on the first layer (E: + 2^-20 sum |a||w| of the per-point GEMM that makes U);  sums:
  sum_rows u(y), sum_rows 2 |y| u(y);  max / min: the largest unit of the neighbourhood.  Plane outputs: + 2^-20 |value| + 1.3e-7
  (the split's allowance), and |lo| <= 2^-11 |hi| + 2^-25 (lo is the fp16 of a remainder of at most half an ulp of hi); the
  planes of sa_mlp2_fused also keep the bare plane contract against the fp32 output of the fp32 form on the same inputs.
The bound of a group is K[group] units.  K is not from a GPU result: emulate() computes the same chain on the CPU (operands split
with split_cpu, the products lo.hi, hi.lo, hi.hi per 16-deep step, float32 accumulation, sums in float32 per half and float64
beyond); K = its largest error in units rounded up to a power of two, times YARD_SPARE.  The project's whole-output bound of 2e-5
max |ref| is checked on raw rows, max and min (and the E outputs) as well: the yardstick passes it with the factor 8 to spare in
every group, so it is kept everywhere.
Bits: a second launch, and a launch under another PERSISTENT_WGS, reproduce raw rows, max and min; the sums under another grid
agree within 2^-40 sum |y| / 2^-40 sum y^2; with and without a schedule max, min and the live raw rows are identical.
No element is left out of a comparison; every reference value is finite."""
from __future__ import annotations

import importlib.util
import math
import sys
import zlib
from dataclasses import dataclass
from functools import lru_cache
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]


def _load_gemm_cases():
    spec = importlib.util.spec_from_file_location("gemm_cases", ROOT / "tests" / "gemm_cases.py")
    mod = sys.modules.setdefault("gemm_cases", importlib.util.module_from_spec(spec))
    if not hasattr(mod, "CASES"):
        spec.loader.exec_module(mod)
    return mod


gc = _load_gemm_cases()
SENTINEL, SENTINEL_F16, NAN, TOP, YARD_SPARE = gc.SENTINEL, gc.SENTINEL_F16, gc.NAN, gc.TOP, gc.YARD_SPARE
Buf, split_cpu, _bits = gc.Buf, gc.split_cpu, gc._bits
SENTINEL_I32 = -1234
U24, U20 = 2.0 ** -24, 2.0 ** -20
WHOLE_BOUND = 2e-5
_GUARD_FILL = [NAN]
f32, f16, f64 = torch.float32, torch.float16, torch.float64

LIVE_SET = (1, 2, 16, 17, 31, 32, 33, 34, 47, 48, 49, 63, 64)
G_SET = (1, 3, 4, 5, 8, 9, 15, 33)
WGS_SET = (None, 1, 2, 3, 8, 9, 17, 40)
N_SET = (33, 48, 64)
FS_OF_G = {1: (1, 1), 3: (3, 1), 4: (2, 2), 5: (1, 5), 8: (2, 4), 9: (3, 3), 15: (3, 5), 33: (3, 11)}
PAIRS = ((15, None), (15, 1), (15, 2), (15, 3), (15, 8), (15, 9), (15, 17), (15, 40), (1, None), (3, 1), (4, 1), (5, 2), (8, 2),
         (9, 3), (33, 1), (33, 8), (33, None))
COPIES = (1, 3, 64)      # 64 = train_ops.BN_STAT_COPIES, bn_stats_buffer's default (the host test pins the number)

# K[group]: the bound in units.  Measured yardstick maximum in the comment (python tests/sa_stage_cases.py --yardstick); K = 8 * that
# rounded up to a power of two.
K = {
    "T": 4.0,      # yardstick 0.475 (raw rows of wide stage 2, span profile; max / min 0.418, sums 0.162; whole-output 3.8e-7 of max |ref|)
    "E": 2.0,      # yardstick 0.126 (planes of sa_table_planes; fp32 rows 0.031, pooled 0.031; whole-output 4.0e-7 of max |ref|)
}


@dataclass(frozen=True)
class Kern:
    name: str            # what pfpp_last_gemm_kernel() reports ("" for the eval entry points, which do not report)
    enum: str            # SaKern enumerator / eval entry point
    D: int
    ns: int
    widths: Tuple[int, int, int]
    stage: int
    src: str             # gather | rows | table
    grid: str            # p4 | p8 | light | rows:<n_total> | e4 | etab | eplanes
    sched_ok: bool = False
    outs: Tuple[str, ...] = ("stats",)


_W0, _W2, _W3 = (64, 64, 128), (128, 128, 256), (256, 256, 512)
_WIDE = "sa_wide_train_kernel"
KERN = {
    "sa1_1": Kern("sa1_train_kernel<64, 64, 128, 1>", "Sa1Stage1", 0, 32, _W0, 1, "gather", "p4"),
    "sa1_2": Kern("sa1_train_kernel<64, 64, 128, 2>", "Sa1Stage2", 0, 32, _W0, 2, "gather", "p4"),
    "sa1_3": Kern("sa1_train_kernel<64, 64, 128, 3>", "Sa1Stage3", 0, 32, _W0, 3, "gather", "p4", outs=("stats", "max", "min")),
    "sa2_1": Kern("sa2_train_kernel<128, 128, 128, 1>", "Sa2Stage1", 128, 64, _W2, 1, "gather", "p4"),
    "sa2_2": Kern("sa2_train_kernel<128, 128, 128, 2>", "Sa2Stage2", 128, 64, _W2, 2, "gather", "p4", outs=("stats", "rows")),
    "rows8": Kern("sa_rows8_train_kernel<128, 256>", "Rows8", 128, 64, _W2, 3, "rows", "p8", True, ("stats", "max", "min")),
    "fs128": Kern("sa_first_stats_kernel<128>", "FirstStats128", 128, 64, _W2, 1, "table", "light"),
    "fs256": Kern("sa_first_stats_kernel<256>", "FirstStats256", 256, 64, _W3, 1, "table", "light"),
    "tab128": Kern(f"{_WIDE}<128, 2, true, false>", "Table128", 128, 64, _W2, 2, "table", "rows:128", True, ("stats", "rows")),
    "tab256": Kern(f"{_WIDE}<256, 2, true, false>", "Table256", 256, 64, _W3, 2, "table", "rows:256", True, ("stats", "rows")),
    "wide1": Kern(f"{_WIDE}<256, 1, false, false>", "Wide1", 256, 64, _W3, 1, "gather", "rows:256", outs=("stats", "rows")),
    "wide2": Kern(f"{_WIDE}<256, 2, false, false>", "Wide2", 256, 64, _W3, 2, "rows", "rows:256", True, ("stats", "rows")),
    "wide3": Kern(f"{_WIDE}<256, 3, false, false>", "Wide3", 256, 64, _W3, 3, "rows", "rows:512", True, ("stats", "max", "min")),
    # eval forms (s / t = folded BatchNorm scale / shift, no bias)
    "mlp3": Kern("", "pfpp_sa_mlp3_fused", 0, 32, _W0, 3, "gather", "e4", outs=("pool",)),
    "mlp2": Kern("", "pfpp_sa_mlp2_fused", 128, 64, _W2, 2, "gather", "e4", outs=("act",)),
    "mlp2_p": Kern("", "pfpp_sa_mlp2_fused_p", 128, 64, _W2, 2, "gather", "e4", outs=("planes",)),
    "mlp2_tab": Kern("", "pfpp_sa_mlp2_table_p", 128, 64, _W2, 2, "table", "etab", outs=("planes",)),
    "tp128": Kern("", "pfpp_sa_table_planes", 128, 64, _W2, 1, "table", "eplanes", outs=("planes",)),
    "tp256": Kern("", "pfpp_sa_table_planes", 256, 64, _W3, 1, "table", "eplanes", outs=("planes",)),
}
T_KERNS = tuple(k for k, v in KERN.items() if v.name)
E_KERNS = tuple(k for k, v in KERN.items() if not v.name)
EVAL_ENTRIES = ("pfpp_sa_mlp3_fused", "pfpp_sa_mlp2_fused", "pfpp_sa_mlp2_fused_p", "pfpp_sa_mlp2_table_p", "pfpp_sa_table_planes")


@dataclass(frozen=True)
class Case:
    name: str
    group: str                 # T P E
    kern: str                  # key of KERN ("sched" for P)
    F: int = 3
    S: int = 5
    N: int = 48
    wgs: Optional[int] = None  # ops.PERSISTENT_WGS of the launch
    sched: bool = False
    lives: str = "set"         # "set": LIVE_SET and the two reappearing lists round-robin; "n2=<k>": k two-half neighbourhoods; "rand"
    profile: str = "unit"      # unit | span | offset
    copies: int = 64
    G_p: int = 0               # group P: the number of neighbourhoods

    @property
    def G(self):
        return self.G_p or self.F * self.S


def _ceil(a, b):
    return -(-a // b)


def grids(kern: str, G: int, wgs: Optional[int]):
    """-> (workgroups, workgroups per column slice, neighbourhoods per round = the stride of the walk): persistent_grid and
    rows_grid of csrc/sa_train.hip and the grid lines of the eval entry points, restated"""
    k = KERN[kern]
    cap = wgs or 256
    if k.grid == "p4":
        g = min(_ceil(G, 4), cap)
        return g, g, 4 * g
    if k.grid == "p8":
        g = min(_ceil(G, 8), cap)
        return g, g, 8 * g
    if k.grid == "light":
        g = min(_ceil(G, 4), 4 * cap)
        return g, g, 4 * g
    if k.grid.startswith("rows:"):
        n_sl = int(k.grid[5:]) // 128
        g = max(cap // (8 * n_sl) * (8 * n_sl), n_sl)
        return g, g // n_sl, 4 * (g // n_sl)
    if k.grid == "e4":
        g = min(_ceil(G, 4), 256)
        return g, g, 4 * g
    if k.grid == "etab":
        g = min(_ceil(G, 4), max(cap // 8 * 8, 1))
        return g, g, 4 * g
    g = min(_ceil(G, 4), 2048)
    return g, g, 4 * g


def _nm(kern, G, wgs, N=48, extra=""):
    return f"{kern}_g{G}_w{'all' if wgs is None else wgs}" + (f"_n{N}" if N != 48 else "") + extra


def _table_t():
    t = []
    i = 0
    for kern in T_KERNS:
        k = KERN[kern]
        for G, wgs in PAIRS:
            F, S = FS_OF_G[G]
            i += 1
            t.append(Case("T_" + _nm(kern, G, wgs), "T", kern, F, S, 48, wgs, False, "set" if k.ns == 64 else "rand", "unit", COPIES[i % 3]))
            if k.sched_ok:
                t.append(Case("T_" + _nm(kern, G, wgs, extra="_sched"), "T", kern, F, S, 48, wgs, True, "set", "unit", COPIES[i % 3]))
        for N in (33, 64):
            i += 1
            t.append(Case("T_" + _nm(kern, 15, None, N), "T", kern, 3, 5, N, None, False, "set" if k.ns == 64 else "rand", "unit", COPIES[i % 3]))
            if k.sched_ok:
                t.append(Case("T_" + _nm(kern, 15, None, N, "_sched"), "T", kern, 3, 5, N, None, True, "set", "unit", COPIES[i % 3]))
        for prof in ("span", "offset"):
            i += 1
            for sc in ((False, True) if k.sched_ok else (False,)):
                t.append(Case("T_" + _nm(kern, 15, 2, extra=f"_{prof}" + ("_sched" if sc else "")), "T", kern, 3, 5, 48, 2, sc,
                              "set" if k.ns == 64 else "rand", prof, COPIES[i % 3]))
        if k.sched_ok:
            # class mixes: the wrap arithmetic of PadWalk at the stride of the launch (4 row_wgs, rows8: 8 grid)
            for G, wgs in ((15, 1), (33, 2 if k.grid == "p8" else (8 if k.grid == "rows:128" else (16 if k.grid == "rows:256" else 32)))):
                stride = grids(kern, G, wgs)[2]
                for n2 in sorted({0, G, 1, stride - 1, stride, stride + 1}):
                    if 0 <= n2 <= G:
                        i += 1
                        F, S = FS_OF_G[G]
                        for sc in (True, False):
                            t.append(Case("T_" + _nm(kern, G, wgs, extra=f"_mix{n2}" + ("_sched" if sc else "")), "T", kern, F, S, 48, wgs, sc,
                                          f"n2={n2}", "unit", COPIES[i % 3]))
    return t


P_SIZES = (1, 1023, 1024, 1025, 32768, 32769, 40000)


def _table_p():
    return [Case(f"P_sched_g{G}", "P", "sched", N=48, lives="rand", G_p=G) for G in P_SIZES]


def _table_e():
    t = []
    for kern in E_KERNS:
        pairs = PAIRS if kern == "mlp2_tab" else tuple((G, None) for G in G_SET)
        for G, wgs in pairs:
            F, S = FS_OF_G[G]
            t.append(Case("E_" + _nm(kern, G, wgs), "E", kern, F, S, 48, wgs, False, "set" if KERN[kern].ns == 64 else "rand"))
        for N in (33, 64):
            t.append(Case("E_" + _nm(kern, 15, None, N), "E", kern, 3, 5, N, None, False, "set" if KERN[kern].ns == 64 else "rand"))
        for prof in ("span", "offset"):
            t.append(Case("E_" + _nm(kern, 15, None, extra="_" + prof), "E", kern, 3, 5, 48, None, False,
                          "set" if KERN[kern].ns == 64 else "rand", prof))
    return t


CASES = {c.name: c for c in _table_t() + _table_p() + _table_e()}
GROUPS = {g: [n for n, c in CASES.items() if c.group == g] for g in "TPE"}
assert len(CASES) == sum(len(v) for v in GROUPS.values())


def alt_wgs(c: Case):
    """another grid cap for the bit comparison: one that changes the partition"""
    return 1 if c.wgs != 1 else 9


def nosched_twin(c: Case) -> Case:
    return CASES[c.name[:-len("_sched")]]


# ------------------------------------------------------------------------------------------------------------ index lists
def _stem(c: Case) -> bytes:
    """what seeds a case: its name without the parts that must not change the inputs (a case and its unscheduled twin, the fp32 and
    the plane form of sa_mlp2_fused)"""
    return c.name.replace("_sched", "").replace("mlp2_p", "mlp2").encode()


def _gen(c: Case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(_stem(c)) + salt)


def live_counts(idx: np.ndarray) -> np.ndarray:
    """[G, 64] -> [G]: 1 + the highest slot that differs from slot 0 (the kernels' definition)"""
    diff = idx != idx[:, :1]
    return np.where(diff.any(1), 64 - np.argmax(diff[:, ::-1], 1), 1).astype(np.int32)


def sched_ref(idx: np.ndarray) -> np.ndarray:
    """the schedule of pfpp_sa_pad_schedule: int32 [3G + 1]"""
    live = live_counts(idx)
    two = live > 32
    order = np.concatenate([np.nonzero(two)[0], np.nonzero(~two)[0]]).astype(np.int32)
    return np.concatenate([order, np.array([two.sum()], np.int32), live, live[order]]).astype(np.int32)


REAPPEAR = ((41, 5), (20, 5))      # (live count, a slot inside the live part that repeats slot 0's index)


def wanted_lives(c: Case):
    """-> [(live, reappearing slot or None)] per neighbourhood"""
    G = c.G
    if c.lives == "set":
        pool = [(v, None) for v in LIVE_SET] + list(REAPPEAR)
        rot = zlib.crc32(_stem(c)) % len(pool)
        want = [pool[(rot + 4 * i) % len(pool)] for i in range(G)]      # (4 and 15 are coprime: every entry comes once in 15)
        if max(v for v, _ in want) < 4:                                  # (room for the indices 0 and N - 1)
            want[0] = (17, None)
        return want
    n2 = int(c.lives[3:])
    g = _gen(c, 7)
    two = set(torch.randperm(G, generator=g)[:n2].tolist())
    hi, lo = (33, 34, 47, 48, 49, 63, 64), (1, 2, 16, 17, 31, 32)
    return [((hi[i % 7] if i in two else lo[i % 6]), None) for i in range(G)]


def make_idx(c: Case) -> torch.Tensor:
    """int32 [G, ns]: in range, never NAN_ROW, containing 0 and N - 1"""
    g = _gen(c, 1)
    ns = 64 if c.group == "P" else KERN[c.kern].ns
    G, N = c.G, c.N
    pool = torch.tensor([v for v in range(N) if v != N - 2], dtype=torch.int32)
    idx = pool[torch.randint(0, len(pool), (G, ns), generator=g)]
    if ns == 32 or c.lives == "rand":
        if c.group == "P":
            live = torch.tensor(LIVE_SET)[torch.randint(0, len(LIVE_SET), (G,), generator=g)]
            idx = torch.where(torch.arange(64)[None] < live[:, None], idx, idx[:, :1])
            idx[0, :3] = torch.tensor([5, 0, N - 1], dtype=torch.int32)
        else:
            idx[0, 1], idx[0, 2] = 0, N - 1
        return idx.contiguous()
    want = wanted_lives(c)
    big = max(range(G), key=lambda i: want[i][0])
    for i, (live, rep) in enumerate(want):
        if i == big and live >= 4:
            idx[i, 1], idx[i, 2] = 0, N - 1
        if live > 1 and idx[i, live - 1] == idx[i, 0]:
            idx[i, live - 1] = pool[(int(torch.nonzero(pool == idx[i, 0])[0]) + 1) % len(pool)]
        if rep is not None:
            idx[i, rep] = idx[i, 0]
        idx[i, live:] = idx[i, 0]
    return idx.contiguous()


# ------------------------------------------------------------------------------------------------------------ operands
def _dense(rows, cols, dtype, fill, data=None):
    return Buf(rows, cols, dtype, fill, left=0, right=0, align=1, data=data)


def _vec(n, dtype, fill, data=None):
    return Buf(1, n, dtype, fill, left=16, right=8, align=16, data=data)


def _fill16():
    v = _GUARD_FILL[0]
    return v if v != v else max(-65504.0, min(65504.0, v))


def _affine(C, g):
    m = torch.rand(C, generator=g) + 0.5
    a = torch.randn(C, generator=g) * 0.3
    m[1::4] *= -1.0
    a[1::4] += 0.5
    m[2::4] = 0.0
    a[2::4] = a[2::4].abs() + 0.1
    a[6::8] *= -1.0
    a[3::4] = -1e3
    return m, a


def _operands(c: Case):
    """the fp32 / fp16 operand values of a case (no buffers yet)"""
    k = KERN[c.kern]
    g = _gen(c, 2)
    F, N, S, G, D, ns = c.F, c.N, c.S, c.G, k.D, k.ns
    off, rad = (4.0, 0.3) if c.profile == "offset" else (0.0, 1.0)
    o = dict(xyz=off + rad * (torch.rand(F * N, 3, generator=g) * 2 - 1), ctr=off + rad * (torch.rand(G, 3, generator=g) * 2 - 1))
    if D:
        o["feats"] = torch.randn(F * N, D, generator=g)
    o["idx"] = make_idx(c)
    kin = (D + 3, k.widths[0], k.widths[1])
    kpad = (D + 8, k.widths[0], k.widths[1])
    for i in range(k.stage):
        C = k.widths[i]
        w = torch.zeros(C, kpad[i])
        w[:, :kin[i]] = torch.randn(C, kin[i], generator=g) / math.sqrt(kin[i])
        b = torch.randn(C, generator=g) * 0.5
        m, a = _affine(C, g)
        if c.profile == "span":
            s = torch.logspace(-3, 2, C)[torch.randperm(C, generator=g)]
            w, b, m = w * s[:, None], b * s, m / s
        o[f"w{i}"], o[f"b{i}"], o[f"m{i}"], o[f"a{i}"] = w, b, m, a
    o["nan_rows"] = torch.arange(F) * N + (N - 2)
    for key in ("xyz", "feats"):
        if key in o:
            o[key][o["nan_rows"]] = _GUARD_FILL[0]
    return o


def _wval(o, i):
    hi, lo = split_cpu(o[f"w{i}"])
    return hi, lo, hi.double() + lo.double()


def _gather(c: Case, o):
    """the grouped first-layer input in float64 [R, D + 8] and its unit, the global point row of every grouped row"""
    k = KERN[c.kern]
    G, ns, D = c.G, k.ns, k.D
    frag = torch.arange(G) // c.S
    rows = (frag[:, None] * c.N + o["idx"].long()).reshape(-1)            # [R]
    diff = o["xyz"].double()[rows] - o["ctr"].double().repeat_interleave(ns, 0)
    X = torch.zeros(G * ns, D + 8, dtype=f64)
    Ux = torch.zeros_like(X)
    if D:
        X[:, :D] = o["feats"].double()[rows]
    X[:, D:D + 3] = diff
    Ux[:, D:D + 3] = U24 * diff.abs()
    return X, Ux, rows


def _layer(a, ua, W, b):
    y = a @ W.t() + (b.double() if b is not None else 0.0)
    u = U20 * (a.abs() @ W.abs().t()) + ua @ W.abs().t()
    return y, u


def _act(y, u, m, a):
    m, a = m.double(), a.double()
    v = y * m + a
    uv = m.abs() * u + U24 * ((y * m).abs() + a.abs())
    return torch.relu(v), torch.where(v < -1024.0 * uv, torch.zeros((), dtype=f64), uv)


def _y_prev(c: Case, o, g):
    """the raw rows a rows stage reads: random live rows, the slots >= live equal to row 0 (what an unscheduled stage writes)"""
    k = KERN[c.kern]
    Kp = k.widths[k.stage - 2]
    y = torch.randn(c.G, 64, Kp, generator=g) * 1.5
    live = torch.from_numpy(live_counts(o["idx"].numpy())).long()
    copy = torch.arange(64)[None] >= live[:, None]
    y = torch.where(copy[:, :, None], y[:, :1], y)
    return y.reshape(c.G * 64, Kp), copy.reshape(-1)


@lru_cache(maxsize=6)
def built(c: Case):
    return _build(c)


def built_with_guards(c: Case, fill: float):
    _GUARD_FILL[0] = fill
    try:
        return _build(c)
    finally:
        _GUARD_FILL[0] = NAN


def _build(c: Case):
    if c.group == "P":
        idx = make_idx(c)
        bufs = {"idx": _dense(c.G, 64, torch.int32, c.N - 2, data=idx), "sched": _vec(3 * c.G + 1, torch.int32, SENTINEL_I32)}
        return dict(bufs=bufs, ref={"sched": torch.from_numpy(sched_ref(idx.numpy()))[None]}, unit={}, o=dict(idx=idx), outs=("sched",),
                    inputs=("idx",))
    k = KERN[c.kern]
    o = _operands(c)
    fill = _GUARD_FILL[0]
    G, ns, D, st = c.G, k.ns, k.D, k.stage
    R = G * ns
    live = live_counts(o["idx"].numpy()) if ns == 64 else np.full(G, 32, np.int32)
    bufs = {"xyz": _dense(c.F * c.N, 3, f32, fill, data=o["xyz"]), "ctr": _dense(G, 3, f32, fill, data=o["ctr"]),
            "idx": _dense(G, ns, torch.int32, c.N - 2, data=o["idx"])}
    if D:
        bufs["feats"] = _dense(c.F * c.N, D, f32, fill, data=o["feats"])
    W = {}
    for i in range(st):
        hi, lo, W[i] = _wval(o, i)
        o[f"w{i}h"], o[f"w{i}l"] = hi, lo
    ref, unit = {}, {}
    # ---- the chain in float64
    evalf = c.group == "E"
    first = 0
    if k.src == "rows":
        g = _gen(c, 3)
        yp, copy = _y_prev(c, o, g)
        o["y_prev"], o["copy_rows"] = yp, copy
        a, ua = _act(yp.double(), torch.zeros(R, yp.shape[1], dtype=f64), o[f"m{st - 2}"], o[f"a{st - 2}"])
        first = st - 1
        fed = yp.clone()
        if c.sched:
            fed[copy] = fill
        bufs["y_prev"] = _dense(R, yp.shape[1], f32, fill, data=fed)
    else:
        X, Ux, prow = _gather(c, o)
        o["prow"] = prow
        a, ua = X, Ux
    y = u = None
    for i in range(first, st):
        y, u = _layer(a, ua, W[i], None if evalf else o[f"b{i}"])
        if i == 0 and k.src == "table":
            pts = torch.zeros(c.F * c.N, D + 8, dtype=f64)
            pts[:, :D], pts[:, D:D + 3] = o["feats"].double(), o["xyz"].double()
            ok = torch.ones(c.F * c.N, dtype=torch.bool)
            ok[o["nan_rows"]] = False
            U64 = torch.zeros(c.F * c.N, k.widths[0], dtype=f64)
            U64[ok] = pts[ok] @ W[0].t() + (0.0 if evalf else o["b0"].double())
            wc = (o["ctr"].double() @ W[0][:, D:D + 3].t()).repeat_interleave(ns, 0)
            u = u + U24 * (U64[prow].abs() + wc.abs())
            if evalf:
                u = u + U20 * (pts[ok].abs() @ W[0].abs().t())[torch.cumsum(ok, 0) - 1][prow]
            else:
                U32 = U64.float()
                U32[~ok] = fill
                o["u_in"] = U32
                bufs["u_in"] = _dense(c.F * c.N, k.widths[0], f32, fill, data=U32)
        if i + 1 < st or evalf:
            a, ua = _act(y, u, o[f"m{i}"], o[f"a{i}"])
    Cs = k.widths[st - 1]
    # ---- operand buffers the launch reads (and NaN stand-ins for what the wrapper wants but the kernel must not read)
    read_w = set(range(first, st)) | ({0} if k.src == "table" else set())
    if k.src == "table" and st == 1 and not evalf:
        read_w = {0}
    for i in range(st):
        if i in read_w:
            bufs[f"w{i}h"], bufs[f"w{i}l"] = _dense(*W[i].shape, f16, _fill16(), data=o[f"w{i}h"]), _dense(*W[i].shape, f16, _fill16(), data=o[f"w{i}l"])
        if evalf or i < st - 1:
            if evalf or i >= first - 1:
                bufs[f"m{i}"], bufs[f"a{i}"] = _vec(k.widths[i], f32, fill, data=o[f"m{i}"]), _vec(k.widths[i], f32, fill, data=o[f"a{i}"])
        if not evalf and i >= first and not (k.src == "table" and i == 0):
            bufs[f"b{i}"] = _vec(k.widths[i], f32, fill, data=o[f"b{i}"])
    # ---- outputs
    written = torch.ones(R, dtype=torch.bool)
    if c.sched and "rows" in k.outs:
        written = (torch.arange(64)[None] < torch.from_numpy(live).long()[:, None]).reshape(-1)
    if "stats" in k.outs:
        g = _gen(c, 4)
        mag = torch.stack([y.abs().sum(0), (y * y).sum(0)])                                     # [2, C]
        s0 = (torch.rand(c.copies, 2, Cs, generator=g, dtype=f64) * 2 - 1) * mag[None] / c.copies
        bufs["stats"] = _dense(c.copies * 2, Cs, f64, SENTINEL, data=s0.reshape(c.copies * 2, Cs))
        ref["stats"] = s0.sum(0) + torch.stack([y.sum(0), (y * y).sum(0)])
        unit["stats"] = torch.stack([u.sum(0), (2 * y.abs() * u).sum(0)])
        o["stats_mag"] = mag
    if "rows" in k.outs:
        bufs["rows"] = _dense(R, Cs, f32, SENTINEL)
        ref["rows"], unit["rows"] = y, u
    if "max" in k.outs:
        y3, u3 = y.view(G, ns, Cs), u.view(G, ns, Cs)
        bufs["max"], bufs["min"] = _dense(G, Cs, f32, SENTINEL), _dense(G, Cs, f32, SENTINEL)
        ref["max"], ref["min"] = y3.amax(1), y3.amin(1)
        unit["max"] = unit["min"] = u3.amax(1)
    if "pool" in k.outs:
        bufs["pool"] = _dense(G, Cs, f32, SENTINEL)
        ref["pool"], unit["pool"] = a.view(G, ns, Cs).amax(1), ua.view(G, ns, Cs).amax(1)
    if "act" in k.outs:
        bufs["act"] = _dense(R, Cs, f32, SENTINEL)
        ref["act"], unit["act"] = a, ua
    if "planes" in k.outs:
        bufs["hi"], bufs["lo"] = _dense(R, Cs, f16, SENTINEL_F16), _dense(R, Cs, f16, SENTINEL_F16)
        ref["planes"], unit["planes"] = a, ua + U20 * a.abs() + 1.3e-7
    if c.sched:
        bufs["sched"] = _vec(3 * G + 1, torch.int32, SENTINEL_I32, data=torch.from_numpy(sched_ref(o["idx"].numpy())))
    o["live"], o["written"] = live, written
    outs = tuple(n for n in ("stats", "rows", "max", "min", "pool", "act", "hi", "lo") if n in bufs)
    return dict(bufs=bufs, ref=ref, unit=unit, o=o, outs=outs, inputs=tuple(n for n in bufs if n not in outs))


# ------------------------------------------------------------------------------------------------------------ the yardstick
def fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def mm3(a32, wh, wl, drop=None):
    """split-f16 contraction: a split with split_cpu, per 16-deep step the products lo.hi, hi.lo, hi.hi, float32 accumulation"""
    Kd = wh.shape[1]
    Kp = _ceil(Kd, 16) * 16
    ah, al = split_cpu(a32)
    pad = lambda t: torch.nn.functional.pad(t.float(), (0, Kp - t.shape[1]))
    ah, al, wh, wl = pad(ah), pad(al), pad(wh), pad(wl)
    acc = torch.zeros(a32.shape[0], wh.shape[0], dtype=f32)
    for k0 in range(0, Kp, 16):
        for j, (x, w) in enumerate(((al, wh), (ah, wl), (ah, wh))):
            if j != drop:
                acc = acc + x[:, k0:k0 + 16] @ w[:, k0:k0 + 16].t()
    return acc


def walk_visits(G, n2, stride, order, wrap_bug=False):
    """how often PadWalk (csrc/sa_train.hip) hands out each neighbourhood over the waves k = 0 .. stride - 1"""
    cnt = np.zeros(G, np.int64)
    for k in range(stride):
        r = n2 % stride
        ib = n2 + (k - r if k >= r else k - r + stride)
        if wrap_bug:      # (the "+ stride" of the waves below the wrap point forgotten: they fall back into the first class)
            ib = n2 + k - r
        i = k if k < n2 else ib
        jumped = k >= n2
        while 0 <= i < G:
            cnt[order[i]] += 1
            j = i + stride
            i, jumped = (ib, True) if (not jumped and i < n2 and j >= n2) else (j, jumped)      # (jumped: a wrong ib must not loop here)
    return cnt


MUTATIONS = ("drop_lo_hi", "drop_hi_lo", "row_left_out", "live33_one_half", "copies31", "copies33", "copies_row1", "maxmin_swapped",
             "channels_swapped", "half1_rows_in_half0", "visited_twice", "skip_wrap", "wrap_bug", "wrong_fragment")


def emulate(c: Case, mut: Optional[str] = None, b=None):
    """the launch on the CPU in the kernels' arithmetic -> {output: tensor}; `mut` makes it wrong in one of the ways of MUTATIONS"""
    b = b or built(c)
    o = b["o"]
    if c.group == "P":
        return {"sched": b["ref"]["sched"].clone()}
    k = KERN[c.kern]
    G, ns, D, st = c.G, k.ns, k.D, k.stage
    R = G * ns
    evalf = c.group == "E"
    drop = {"drop_lo_hi": 0, "drop_hi_lo": 1}.get(mut)
    live = torch.from_numpy(o["live"]).long()
    # the schedule as the launch sees it
    use = c.sched and k.sched_ok
    sch = sched_ref(o["idx"].numpy()) if use else None
    order = sch[:G] if use else np.arange(G)
    n2 = int(sch[G]) if use else G
    cnt = live.clone() if use else torch.full((G,), 64 if ns == 64 else 32)
    if mut == "live33_one_half":
        cnt = torch.where(cnt == 33, torch.full_like(cnt, 32), cnt)
    one = (cnt <= 32) & (ns == 64) & use
    stride = grids(c.kern, G, c.wgs)[2]
    visits = torch.from_numpy(walk_visits(G, n2, stride, order, mut == "wrap_bug"))
    edge = int(order[min(n2, G - 1)])
    if mut == "visited_twice":
        visits[edge] = 2
    if mut == "skip_wrap":
        visits[edge] = 0
    # ---- the chain in float32
    first = 0
    if k.src == "rows":
        yp = o["y_prev"].view(G, 64, -1)
        j = torch.arange(64)[None].expand(G, 64)
        src = torch.where(j < cnt[:, None], j, torch.zeros_like(j))                       # j < live ? j : 0
        x = torch.gather(yp, 1, src[:, :, None].expand_as(yp)).reshape(R, -1)
        a = torch.relu(fma32(x, o[f"m{st - 2}"], o[f"a{st - 2}"]))
        first = st - 1
    else:
        frag = torch.arange(G) // c.S
        if mut == "wrong_fragment":
            frag = torch.where((torch.arange(G) % c.S == 0) & (torch.arange(G) > 0), frag - 1, frag)
        prow = (frag[:, None] * c.N + o["idx"].long()).reshape(-1)
    y = None
    for i in range(first, st):
        if i == 0 and k.src == "table":
            wx = (o["w0h"].float() + o["w0l"].float())[:, D:D + 3]                         # [C1, 3]
            cx = o["ctr"]
            v = fma32(wx[None, :, 2], cx[:, 2:3], fma32(wx[None, :, 1], cx[:, 1:2], (wx[None, :, 0].double() * cx[:, 0:1].double()).float()))
            v = v.repeat_interleave(ns, 0)                                                  # [R, C1]
            if evalf:
                ok = torch.ones(c.F * c.N, dtype=torch.bool)
                ok[o["nan_rows"]] = False
                pts = torch.zeros(c.F * c.N, D + 8)
                pts[:, :D], pts[:, D:D + 3] = o["feats"], o["xyz"]
                U32 = torch.zeros(c.F * c.N, k.widths[0])
                U32[ok] = mm3(pts[ok], o["w0h"], o["w0l"], drop)
            else:
                U32 = o["u_in"]
            if st == 1 and not evalf:
                y = U32[prow] - v
            else:
                a = torch.relu(fma32(U32[prow], o["m0"][None], fma32(-o["m0"][None], v, o["a0"][None])))
                y = None
            continue
        if i == 0:
            X = torch.zeros(R, D + 8)
            if D:
                X[:, :D] = o["feats"][prow]
            X[:, D:D + 3] = o["xyz"][prow] - o["ctr"].repeat_interleave(ns, 0)
            a = X
        acc = mm3(a, o[f"w{i}h"], o[f"w{i}l"], drop)
        if evalf:
            a = torch.relu(fma32(acc, o[f"m{i}"][None], o[f"a{i}"][None]))
        else:
            y = acc + o[f"b{i}"][None]
            if i + 1 < st:
                a = torch.relu(fma32(y, o[f"m{i}"][None], o[f"a{i}"][None]))
    Cs = k.widths[st - 1]
    out = {}
    if evalf:
        if mut == "channels_swapped":
            a = a.clone()
            a[:, [2, 3]] = a[:, [3, 2]]
        vis = (visits > 0).repeat_interleave(ns)
        if "pool" in k.outs:
            out["pool"] = torch.where(visits[:, None] > 0, a.view(G, ns, Cs).amax(1), torch.full((), SENTINEL))
        if "act" in k.outs:
            out["act"] = torch.where(vis[:, None], a, torch.full((), SENTINEL))
        if "planes" in k.outs:
            hi, lo = split_cpu(a)
            out["hi"] = torch.where(vis[:, None], hi, torch.full((), SENTINEL_F16, dtype=f16))
            out["lo"] = torch.where(vis[:, None], lo, torch.full((), SENTINEL_F16, dtype=f16))
        return out
    if mut == "channels_swapped":
        y = y.clone()
        y[:, [2, 3]] = y[:, [3, 2]]
    y3 = y.view(G, ns, Cs)
    # ---- sums: float32 per half, float64 beyond; a one-half neighbourhood adds 32 y_0 and 32 y_0^2 for its second half
    mask = torch.ones(G, ns, dtype=torch.bool)
    mask[one, 32:] = False
    if mut == "row_left_out":
        mask[G - 1, 7] = False
    ym = torch.where(mask[:, :, None], y3, torch.zeros(()))
    hs = ym.view(G, ns // 32, 32, Cs).sum(2).double().sum(1)                                # [G, C]
    hq = (ym * ym).view(G, ns // 32, 32, Cs).sum(2).double().sum(1)
    ncopy = {"copies31": 31.0, "copies33": 33.0}.get(mut, 32.0)
    y0 = y3[:, 1 if mut == "copies_row1" else 0].double()
    hs = hs + torch.where(one[:, None], ncopy * y0, torch.zeros((), dtype=f64))
    hq = hq + torch.where(one[:, None], ncopy * y0 * y0, torch.zeros((), dtype=f64))
    vz = visits.double()[:, None]
    if "stats" in k.outs:
        s0 = b["bufs"]["stats"].view.reshape(c.copies, 2, Cs).sum(0)
        out["stats"] = s0 + torch.stack([(hs * vz).sum(0), (hq * vz).sum(0)])
    if "rows" in k.outs:
        wr = (torch.arange(ns)[None] < (cnt[:, None] if use else ns)) & (visits[:, None] > 0)
        rows = torch.where(wr[:, :, None], y3, torch.full((), SENTINEL))
        if mut == "half1_rows_in_half0":
            two = (~one) & (visits > 0)
            rows[two, :32] = torch.where(wr[two, 32:, None], y3[two, 32:], rows[two, :32])
            rows[two, 32:] = SENTINEL
        out["rows"] = rows.reshape(R, Cs)
    if "max" in k.outs:
        ylive = torch.where(mask[:, :, None], y3, y3[:, :1])
        mx, mn = ylive.amax(1), ylive.amin(1)
        if mut == "maxmin_swapped":
            mx, mn = mn, mx
        out["max"] = torch.where(visits[:, None] > 0, mx, torch.full((), SENTINEL))
        out["min"] = torch.where(visits[:, None] > 0, mn, torch.full((), SENTINEL))
    return out


# ------------------------------------------------------------------------------------------------------------ evaluation
def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def evaluate(c: Case, got: dict, b=None):
    """got: {output: the data region} -> dict(lines=[(tag, error, bound)], flags={name: bool}); every element is compared"""
    b = b or built(c)
    lines, flags = [], {}
    ref, unit = b["ref"], b["unit"]
    if c.group == "P":
        flags["sched_bits"] = same_bits(got["sched"].reshape(-1), ref["sched"].reshape(-1))
        return dict(lines=lines, flags=flags)
    Kb = K[c.group]

    def units(tag, g, r, u, sel=None):
        g = g.double()
        err = (g - r).abs()
        if sel is not None:
            err, r, u = err[sel], r[sel], u[sel]
        e = torch.where(err == 0, torch.zeros((), dtype=f64), err / u.clamp_min(1e-300))
        e = torch.where(torch.isfinite(e), e, torch.full((), float("inf"), dtype=f64))
        lines.append((tag, float(e.max()) if e.numel() else 0.0, Kb))
        if tag != "stats" and tag != "planes" and e.numel():
            w = float(err.max() / r.abs().max().clamp_min(1e-300)) if bool(torch.isfinite(err).all()) else float("inf")
            lines.append((tag + "_whole", w, WHOLE_BOUND))

    if "stats" in ref:
        units("stats", got["stats"], ref["stats"], unit["stats"])
    if "rows" in ref:
        wr = b["o"]["written"]
        units("rows", got["rows"], ref["rows"], unit["rows"], wr)
        flags["unwritten_rows_keep_sentinel"] = bool((got["rows"][~wr] == SENTINEL).all())
    for tag in ("max", "min", "pool", "act"):
        if tag in ref:
            units(tag, got[tag], ref[tag], unit[tag])
    if "planes" in ref:
        hi, lo = got["hi"], got["lo"]
        val = hi.double() + lo.double()
        units("planes", val, ref["planes"], unit["planes"])
        w = float((val - ref["planes"]).abs().max() / ref["planes"].abs().max().clamp_min(1e-300))
        lines.append(("planes_whole", w if math.isfinite(w) else float("inf"), WHOLE_BOUND))
        flags["lo_within_half_an_ulp_of_hi"] = bool((lo.double().abs() <= 2.0 ** -11 * hi.double().abs() + 2.0 ** -25).all())
    return dict(lines=lines, flags=flags)


def planes_contract(x32, hi, lo) -> bool:
    """the project's plane contract of fp32 values x: |hi + lo - x| <= 2^-20 |x| + 1.3e-7 and hi within half an fp16 ulp of x"""
    x = x32.double()
    ok = ((hi.double() + lo.double() - x).abs() <= U20 * x.abs() + 1.3e-7).all()
    return bool(ok) and same_bits(x32.half(), hi)


def passes(rep) -> bool:
    return all(e <= bound for _, e, bound in rep["lines"]) and all(rep["flags"].values())


def describe(c: Case, rep: dict, kernel: str = "") -> str:
    parts = [f"{tag} {e:.3g}{'' if e <= bound else ' OVER'}" for tag, e, bound in rep["lines"]]
    bad = [k for k, v in rep["flags"].items() if not v]
    what = kernel or (KERN[c.kern].enum if c.kern in KERN else "pfpp_sa_pad_schedule")
    return f"sa_stage {c.name:<40} {what:<46} " + "  ".join(parts) + \
        ("  FAILED: " + ", ".join(bad) if bad else "  flags ok" if rep["flags"] else "")


def yardstick(c: Case):
    return evaluate(c, emulate(c))


# ------------------------------------------------------------------------------------------------------------ GPU runs
def _last_kernel():
    from pfpp_hip import _lib
    return _lib.load().pfpp_last_gemm_kernel().decode()


def launch(c: Case, dev, wgs="case", b=None):
    """one launch of the case on fresh copies of its buffers -> (allocations after the launch {name: cpu tensor}, kernel name)"""
    from pfpp_hip import ops
    b = b or built(c)
    bufs = b["bufs"]
    t = {n: v.alloc.to(dev) for n, v in bufs.items()}

    def d(n):
        v = bufs[n]
        x = t[n][v.top:v.top + v.rows, v.left:v.left + v.cols]
        return x[0] if v.rows == 1 and v.left else x
    prev, ops.PERSISTENT_WGS = ops.PERSISTENT_WGS, (c.wgs if wgs == "case" else wgs)
    try:
        if c.group == "P":
            ops.sa_pad_schedule(d("idx").view(c.G, 1, 64), out=d("sched"))
            torch.cuda.synchronize()
            return {n: v.cpu() for n, v in t.items()}, ""
        k = KERN[c.kern]
        G, ns, st = c.G, k.ns, k.stage
        nanp = lambda n, kk: torch.full((n, kk), NAN, dtype=f16, device=dev)
        kpad = (k.D + 8, k.widths[0], k.widths[1])
        ws = [gc._pw_shim(d(f"w{i}h"), d(f"w{i}l"), k.widths[i], kpad[i]) if f"w{i}h" in bufs
              else gc._pw_shim(nanp(k.widths[i], kpad[i]), nanp(k.widths[i], kpad[i]), k.widths[i], kpad[i]) for i in range(st)]
        vec = lambda n, i: d(n) if n in bufs else torch.full((k.widths[i],), NAN, dtype=f32, device=dev)
        xyz, ctr, idx = d("xyz").view(c.F, c.N, 3), d("ctr").view(c.F, c.S, 3), d("idx").view(c.F, c.S, ns)
        feats = d("feats").view(c.F, c.N, k.D) if k.D else None
        if c.group == "E":
            aff = [vec(f"{m}{i}", i) for i in range(st) for m in "ma"]
            if c.kern == "mlp3":
                ops.sa_mlp3_fused(xyz, ctr, idx, ws[0], ws[1], ws[2], *aff, out=d("pool"))
            elif c.kern == "mlp2":
                ops.sa_mlp2_fused(xyz, ctr, feats, idx, ws[0], ws[1], *aff, out=d("act"))
            elif c.kern == "mlp2_p":
                ops.sa_mlp2_fused(xyz, ctr, feats, idx, ws[0], ws[1], *aff, as_planes=True, out=(d("hi"), d("lo")))
            elif c.kern == "mlp2_tab":
                ops.sa_mlp2_table(xyz, ctr, feats, idx, ws[0], ws[1], *aff, out=(d("hi"), d("lo")))
            else:
                ops.sa_table_planes(xyz, ctr, feats, idx, ws[0], *aff, out=(d("hi"), d("lo")))
            torch.cuda.synchronize()
            return {n: v.cpu() for n, v in t.items()}, ""
        kw = {}
        if k.src == "table":
            kw["u_in"] = d("u_in")
        if c.sched:
            kw["sched"] = d("sched")
        if k.src == "rows":
            kw["y_out" if c.kern == "rows8" else "y_in"] = d("y_prev")
        if "rows" in bufs:
            kw["y_out"] = d("rows")
        if "max" in bufs:
            kw["out_max"], kw["out_min"] = d("max"), d("min")
        biases = [vec(f"b{i}", i) for i in range(st)]
        affs = [(vec(f"m{i}", i), vec(f"a{i}", i)) for i in range(st - 1)]
        Cs = k.widths[st - 1]
        ops.sa_train_stage(st, xyz, ctr, feats, idx, ws, biases, affs, d("stats").view(c.copies, 2, Cs), **kw)
        torch.cuda.synchronize()
        return {n: v.cpu() for n, v in t.items()}, _last_kernel()
    finally:
        ops.PERSISTENT_WGS = prev


def data_of(b, allocs):
    """{output: data region} of the allocations a launch left (stats: summed over the copies)"""
    got = {}
    for n in b["outs"]:
        v = b["bufs"][n]
        x = allocs[n][v.top:v.top + v.rows, v.left:v.left + v.cols]
        got[n] = x.reshape(-1, 2, v.cols).sum(0) if n == "stats" else x
    return got


def guards_ok(b, allocs) -> bool:
    """every guard keeps its bits and every input keeps all of them"""
    ok = True
    for n, v in b["bufs"].items():
        m = v.guard_mask() if n in b["outs"] else torch.ones(v.alloc.shape, dtype=torch.bool)
        ok &= bool(torch.equal(_bits(allocs[n])[m], _bits(v.alloc)[m]))
    return ok


def run(c: Case, dev):
    """-> (report of evaluate() with the flags of the guard and bit checks added, kernel name)"""
    b = built(c)
    allocs, kernel = launch(c, dev)
    got = data_of(b, allocs)
    rep = evaluate(c, got)
    fl = rep["flags"]
    fl["guards_and_inputs_keep_their_bits"] = guards_ok(b, allocs)
    if c.group == "T":
        fl["kernel_name"] = kernel == KERN[c.kern].name
    fixed = [n for n in b["outs"] if n not in ("stats",)]
    again = data_of(b, launch(c, dev)[0])
    fl["repeat_bits"] = all(same_bits(again[n], got[n]) for n in fixed)
    if c.group == "T" or c.kern == "mlp2_tab":
        other = data_of(b, launch(c, dev, wgs=alt_wgs(c))[0])
        fl["other_grid_bits"] = all(same_bits(other[n], got[n]) for n in fixed)
        if "stats" in got:
            tol = 2.0 ** -40 * b["o"]["stats_mag"]
            fl["other_grid_stats"] = bool(((other["stats"] - got["stats"]).abs() <= tol).all())
    if c.sched:
        tw = nosched_twin(c)
        bt = built(tw)
        plain = data_of(bt, launch(tw, dev)[0])
        if "max" in got:
            fl["schedule_keeps_max_min_bits"] = same_bits(plain["max"], got["max"]) and same_bits(plain["min"], got["min"])
        if "rows" in got:
            wr = b["o"]["written"]
            fl["schedule_keeps_live_row_bits"] = same_bits(plain["rows"][wr], got["rows"][wr])
    if c.kern == "mlp2_p":
        tw = CASES[c.name.replace("mlp2_p", "mlp2", 1)]
        x32 = data_of(built(tw), launch(tw, dev)[0])["act"]
        fl["plane_contract"] = planes_contract(x32, got["hi"], got["lo"])
    return rep, kernel


def yardstick_main() -> int:
    worst = {}
    for c in CASES.values():
        for tag, e, bound in yardstick(c)["lines"]:
            key = (c.group, "whole" if tag.endswith("_whole") else tag)
            if e > worst.get(key, (-1.0, ""))[0]:
                worst[key] = (e, c.name)
    for (g, tag), (e, name) in sorted(worst.items()):
        print(f"yardstick {g} {tag:<8} {e:.3g}  ({name})")
    return 0


def report_main() -> int:
    sys.path[:0] = [str(ROOT), str(ROOT / "puzzlefusion-plusplus_amd")]
    dev = torch.device("cuda:0")
    bad = 0
    for c in CASES.values():
        rep, kernel = run(c, dev)
        print(describe(c, rep, kernel))
        bad += not passes(rep)
    print(f"sa_stage {len(CASES)} cases, {bad} failing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(yardstick_main() if "--yardstick" in sys.argv else report_main() if "--report" in sys.argv else 0)
