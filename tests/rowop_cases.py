"""Case table, float64 reference and error report of the row-wise training kernels (no test in here; importable without a GPU).
tests/test_rowop_cases_host.py checks the table itself on the CPU, tests/test_gpu_rowop_edges.py runs it through the HIP kernels, and
`python tests/rowop_cases.py --report` prints one line per case (profiles/rowops_errors.txt).

One case is ONE launch (AdamW: three steps) through a Python wrapper of pfpp_hip.ops / train_ops / planes of an entry point named in
FAMILY: the normalisation, reduction and element-wise kernels of csrc/transformer_ops.hip, csrc/train_ops.hip and csrc/bn_train.hip.
Groups: L LayerNorm forward, D dropout + LayerNorm, B LayerNorm backward, S column sums and the plane split, G GEGLU / activations /
dropout, N train-mode BatchNorm, P softmax and pooling, M the loss, A AdamW.  (pfpp_adamw has no wrapper of its own: its cases go
through the ctypes handle the wrappers use.)

Buffers (the rules and constants of tests/gemm_cases.py).  Every input and every output lives inside a
taller allocation of its own (TOP guard rows above and below); where the entry point takes a leading dimension (ld, ldy, ld_mod,
ld_d, sx, so) the allocation is wider than the data as well.  Output guards hold SENTINEL (-1234 in fp16 planes) and must keep their
bits, input guards hold NaN (uint8 selections: 1, so that a row past the end drags a NaN row in; group_batch: the index of a `mod` row
that is NaN).  Kernels that add into their output (dx, dmult / dadd, colsum) start from non-zero values of the size of what they add,
and the reference includes them.  Rows of mod that no group refers to hold NaN; rows of dmult / dadd that no group refers to must
keep their bits.  pfpp_softmax_rows writes the columns T .. ld as zero (its contract), so S has guard rows only.  The keep mask (uint8) is guarded
with SENTINEL_U8; the fp64 accumulators of bn_finalize, which the kernel clears, with SENTINEL.  No output is left to a wrapper to
allocate: the wrappers take `out` arguments for every result.

Dropout.  The keep mask is a pure function of (seed, site, element index): keep_mask() restates the generator of csrc/pfpp_common.h, so
every reference is known on the CPU; the pfpp_dropout_mask cases pin the restatement to the device's mask bit for bit.

Row profiles (LayerNorm-like cases, row r -> profile r % 8): standard normal; offset 100; offset 1e4; 1 + 1e-3 N(0,1); 1e3 N(0,1);
constant 3.0; all zero; standard normal with one element at 1e4.  Channel profiles (BatchNorm, column sums, column c -> c % 4):
|mean| / sigma in {0, 32, 1000} and a constant channel (3.0).

Errors.  The reference is float64 evaluated from the float32 inputs.  Each check has a unit per element, the first-order forward error
of the operation in float32, built from the reference's own float64 intermediates (never from the result under test):
  L, D  2^-24 kappa (1 + |multiplier|) + 2^-24 |shift|,  kappa = 1 + |row mean| / sqrt(var + eps); and, on top of it, a second
        bound KX units of 2^-24 (kappa + |xhat|) (1 + |multiplier|) + 2^-24 |shift| (the rounding of rstd is relative to xhat: the
        first unit has no term for it, so one outlier element with |xhat| = 32 sets its K for every row; both bounds must hold)
  B     dx: 2^-24 kappa rstd max_c |dy multiplier|;  dmult: 2^-24 sum_rows |dy| (|xhat| + kappa) (xhat inherits the rounding of
        the row mean: with kappa = 1 this is 2^-24 sum_rows |dy xhat| of a centred row; without the kappa term the float32 yardstick
        itself is 3e5 units off on the rows whose mean is 1e4 sigma);  dadd: 2^-24 sum_rows |dy|
  S     2^-24 sum_rows |x| (times out_scale for planes);  split_planes: the plane contract alone
  G     2^-24 |value| max(|gate|, |gelu(gate)|), the derivative in place of gelu for the gate gradient; activations the same with
        value = 1 (backward: value = dy)
  N     bn_apply / bn_minmax_apply: 2^-24 (|x a| + |mean a| + |beta| + 1);  statistics: 2^-24 (|mean| + sigma) and
        2^-24 (var + |mean| sigma);  running statistics: the momentum-weighted sum of the two terms' units;  a_mul: 2^-24 |a|,
        a_add: 2^-24 (|beta| + |mean a|)
  P     softmax: 2^-24 p (1 + |s scale - max|) + 2^-126 (the smallest normal float);  pooling: 2^-24 sum |x| / L
  M     loss: 2^-24 loss;  gradient: 2^-24 |dpred|
  A     2^-24 (|p| + |step|), 2^-24 (|m| + |g|), 2^-24 (|v| + g^2) accumulated over the steps taken
The bound of a group is K[group] units.  K was not chosen from a GPU result: the same formula evaluated with torch float32 ops on the
CPU (the yardstick) gives the largest error in units per group; that, rounded up to a power of two, times YARD_SPARE = 8 (the room the
GEMM table gives a different but legitimate summation order) is K.  Plane outputs are judged twice.  Against float64: (hi + lo) / scale
within the bound plus the split's allowance (2^-20 |value| + 1.3e-7).  And by the project's plane contract alone, with no allowance of
the table's: |hi + lo - scale x| <= 2^-20 |scale x| + 1.3e-7 and hi within half an fp16 ulp of scale x, where x is the float32 value
the kernel itself computed: the fp32 output of the same launch where there is one (dx, the dropped-out gradient, AdamW's p, the input
of the split), else the output of the fp32 form launched on the same inputs (a case and its plane twin share their seed).  Elements a
guarded AdamW step skips keep SENTINEL_F16 in both planes, in bits.  Where a result is fixed bit
for bit (dropout's copy-add, the dropped-out gradient, masked against selected loss, amax, guarded against unguarded AdamW) the
check is equality of bits.  At most MAX_EXCLUDED = 2 % of a check's elements may be left out of a comparison, and only elements whose
float64 reference is not finite."""
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
SENTINEL, SENTINEL_F16, NAN, TOP, GCOL, YARD_SPARE = gc.SENTINEL, gc.SENTINEL_F16, gc.NAN, gc.TOP, gc.GCOL, gc.YARD_SPARE
Buf, split_cpu = gc.Buf, gc.split_cpu


def _bits(t: torch.Tensor):
    return t.contiguous() if t.element_size() == 1 else gc._bits(t)


SENTINEL_U8 = 0xA5          # guard of the uint8 keep mask
U = 2.0 ** -24
TINY = 2.0 ** -126
MAX_EXCLUDED = 0.02
EPS = 1e-5
_GUARD_FILL = [NAN]        # what the NaN guards hold (built_with_guards swaps it: no reference may depend on it)

FAMILY = ("pfpp_layernorm", "pfpp_layernorm_split", "pfpp_layernorm_grouped", "pfpp_layernorm_grouped_split",
          "pfpp_dropout_layernorm", "pfpp_dropout_layernorm_p", "pfpp_layernorm_bwd", "pfpp_layernorm_bwd_dropout",
          "pfpp_layernorm_bwd_p", "pfpp_colsum", "pfpp_colsum_planes", "pfpp_split_planes", "pfpp_dropout", "pfpp_dropout_mask",
          "pfpp_geglu", "pfpp_geglu_p", "pfpp_geglu_bwd", "pfpp_geglu_bwd_p", "pfpp_act", "pfpp_act_bwd", "pfpp_bn_stats",
          "pfpp_bn_apply", "pfpp_bn_finalize", "pfpp_bn_minmax_apply", "pfpp_softmax_rows", "pfpp_mean_pool", "pfpp_mean_pool_bwd",
          "pfpp_mse_loss", "pfpp_mse_loss_masked", "pfpp_adamw", "pfpp_adamw_guarded")

# K[group]: the bound in units.  Measured float32 yardstick maximum of the group in the comment (python tests/rowop_cases.py --yardstick);
# K = 8 * that rounded up to a power of two.
K = {
    "L": 512.0,    # yardstick 42.3 (the row with one element at 1e4: |xhat| = 32 there, which the unit does not carry; 6.4 on the other rows)
    "D": 256.0,    # yardstick 26.5 (the same row profile at C = 512)
    "B": 128.0,    # yardstick 8.2
    "S": 64.0,     # yardstick 4.0
    "G": 32.0,     # yardstick 3.1
    "N": 32.0,     # yardstick 3.4
    "P": 32.0,     # yardstick 3.6
    "M": 32.0,     # yardstick 2.5
    "A": 32.0,     # yardstick 2.8
}
# KX[group]: the second bound of L and D, in units that carry |xhat| (see "Errors"); measured and rounded like K
KX = {
    "L": 32.0,     # yardstick 2.42
    "D": 16.0,     # yardstick 1.64
}
# groups whose kernels use no atomics: a second launch on the same inputs must give the same bits (B: dx and what follows it only)
REPEATABLE = "LDGNPMAB"


@dataclass(frozen=True)
class Case:
    name: str
    group: str             # L D B S G N P M A
    entry: str             # the C entry point the launch reaches (a name of FAMILY)
    kind: str              # builder / runner key
    opts: Tuple = ()       # sorted (key, value) pairs

    def o(self, key, default=None):
        return dict(self.opts).get(key, default)


def _case(name, group, entry, kind, **opts):
    return Case(name, group, entry, kind, tuple(sorted(opts.items())))


@dataclass
class Check:
    """one compared output of a launch"""
    tag: str
    out: object                      # Buf name, (hi name, lo name) of a plane pair, or "ret:<key>" of what the runner returns
    ref: torch.Tensor                # float64 (bound / planes) or the expected bits (bits)
    unit: Optional[torch.Tensor] = None
    yard: Optional[torch.Tensor] = None
    kind: str = "bound"              # bound | bits | planes
    scale: float = 1.0               # planes
    atomic: bool = False             # the output is finished with atomics: not part of the repeat-launch comparison
    unit_x: Optional[torch.Tensor] = None    # L, D: the second unit (bound KX[group])
    x32: Optional[str] = None        # planes: where the float32 value they carry is: a Buf of this launch, or "twin:<Buf>" of the fp32 form
    skip: Optional[torch.Tensor] = None      # planes: elements the kernel must leave alone (they keep SENTINEL_F16 in bits)


# ------------------------------------------------------------------------------------------------------------ the table
GB_PATTERN = (2, 0, 2, 1)            # group -> row of mod; row 3 is referred to by nobody
LN_FORMS = (("plain", 1, {}), ("plain", 3, {}), ("affine", 4, {}), ("affine", 37, {}), ("mod", 5, dict(rpb=2)), ("mod", 37, dict(rpb=12)),
            ("grp", 5, dict(gr=1)), ("grp", 37, dict(gr=5)), ("grp", 37, dict(gr=25)))


def _ln_entry(form, split):
    return ("pfpp_layernorm_grouped" if form == "grp" else "pfpp_layernorm") + ("_split" if split else "")


def _table_l():
    t = []
    for C in (256, 512, 1024):
        for split in (False, True):
            for form, rows, o in LN_FORMS:
                nm = f"L_c{C}_{'pl' if split else 'f32'}_{form}_r{rows}" + "".join(f"_{k}{v}" for k, v in o.items())
                t.append(_case(nm, "L", _ln_entry(form, split), "ln", C=C, rows=rows, form=form, split=split, **o))
    return t


def _table_d():
    t = []
    forms = (("plain", 1, {}), ("affine", 5, {}), ("mod", 37, dict(rpb=12)), ("grp", 37, dict(gr=5)))
    i = 0
    for C in (256, 512):
        for planes in (False, True):
            for form, rows, o in forms:
                for p in (0.0, 0.2):
                    res = bool(i % 2) if p else (form != "plain")       # p = 0 without a residual: the plain form (h is y in bits)
                    i += 1
                    nm = f"D_c{C}_{'pl' if planes else 'f32'}_{form}_r{rows}_p{int(p * 10)}{'_res' if res else ''}"
                    t.append(_case(nm, "D", "pfpp_dropout_layernorm" + ("_p" if planes else ""), "dln", C=C, rows=rows, form=form,
                                   planes=planes, p=p, res=res, seed=1234 + i, site=i % 7, **o))
        t.append(_case(f"D_c{C}_f32_plain_r5_p2_res", "D", "pfpp_dropout_layernorm", "dln", C=C, rows=5, form="plain", planes=False,
                       p=0.2, res=True, seed=99, site=3))
        t.append(_case(f"D_c{C}_f32_plain_r37_p2", "D", "pfpp_dropout_layernorm", "dln", C=C, rows=37, form="plain", planes=False,
                       p=0.2, res=False, seed=98, site=2))
    return t


LNB_GROUP_ROWS = (1, 3, 8, 9, 25, 32, 33)


def lnb_rows(form, gr):
    if form == "grp":
        return 4 * gr + (gr + 1) // 2                                 # five groups, the last one truncated
    if form == "uni":
        return 5 * gr                                                 # rows_per_batch = 2 gr: batches of 2, 2 and 1 groups
    return 70 if gr == 33 else 2 * gr + 1                             # last group of 1 row (4 rows at 33): its later slices are empty


def _table_b():
    t = []
    for C in (256, 512):
        for gr in LNB_GROUP_ROWS:
            for form in ("grp", "uni", "gamma", "none"):
                t.append(_case(f"B_c{C}_{form}_g{gr}", "B", "pfpp_layernorm_bwd", "lnb", C=C, gr=gr, form=form, rows=lnb_rows(form, gr)))
        t.append(_case(f"B_c{C}_grp_g25_drop", "B", "pfpp_layernorm_bwd_dropout", "lnb", C=C, gr=25, form="grp", rows=lnb_rows("grp", 25),
                       drop=(0.2, 4321, 5)))
        t.append(_case(f"B_c{C}_gamma_g9_drop", "B", "pfpp_layernorm_bwd_dropout", "lnb", C=C, gr=9, form="gamma", rows=19,
                       drop=(0.2, 4322, 1)))
        t.append(_case(f"B_c{C}_grp_g9_planes", "B", "pfpp_layernorm_bwd_p", "lnb", C=C, gr=9, form="grp", rows=lnb_rows("grp", 9),
                       planes=True))
        t.append(_case(f"B_c{C}_uni_g33_planes_drop", "B", "pfpp_layernorm_bwd_p", "lnb", C=C, gr=33, form="uni", rows=lnb_rows("uni", 33),
                       planes=True, drop=(0.2, 4323, 2)))
    return t


def _table_s():
    t = []
    i = 0
    for cols in (4, 252, 256, 260):
        for rows in (1, 3, 4, 63, 64, 65, 129):
            t.append(_case(f"S_colsum_c{cols}_r{rows}", "S", "pfpp_colsum", "colsum", cols=cols, rows=rows, batch=3, acc=bool(i % 2), pad=4))
            i += 1
    for cols in (1, 3, 7):
        for rows in (1, 63, 64, 65):
            t.append(_case(f"S_colsum_narrow_c{cols}_r{rows}", "S", "pfpp_colsum", "colsum", cols=cols, rows=rows, batch=2, acc=bool(i % 2),
                           pad=2, x_off=3))
            i += 1
    for rows in (1, 65):
        t.append(_case(f"S_colsum_c8_ld9_r{rows}", "S", "pfpp_colsum", "colsum", cols=8, rows=rows, batch=2, acc=True, pad=1))
    for cols in (4, 256, 260):
        for rows in (1, 15, 16, 17, 129):
            t.append(_case(f"S_colsum_planes_c{cols}_r{rows}", "S", "pfpp_colsum_planes", "colsum_planes", cols=cols, rows=rows))
    t.append(_case("S_colsum_planes_c8_r8200", "S", "pfpp_colsum_planes", "colsum_planes", cols=8, rows=8200))
    for n in (4, 1020, 1024, 1028):
        for scale in (1.0, 4096.0):
            t.append(_case(f"S_split_n{n}_x{int(scale)}", "S", "pfpp_split_planes", "split", n=n, scale=scale))
    return t


GATE_VALUES = (0.0, -0.0, 1e-3, -1e-3, 1.0, -1.0, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0, 1e4, -1e4, 3.5, -3.5)
ACT_VALUES = GATE_VALUES + (100.0, -100.0)


def _table_g():
    t = []
    i = 0
    for rows, inner in ((1, 4), (3, 344), (1, 1024), (5, 12), (2, 2048)):
        for p in (0.0, 0.1):
            for planes in (False, True):
                i += 1
                sfx = f"r{rows}_i{inner}_p{int(p * 10)}_{'pl' if planes else 'f32'}"
                t.append(_case(f"G_geglu_{sfx}", "G", "pfpp_geglu" + ("_p" if planes else ""), "geglu", rows=rows, inner=inner, p=p,
                               planes=planes, seed=500 + i, site=i % 5))
                t.append(_case(f"G_geglu_bwd_{sfx}", "G", "pfpp_geglu_bwd" + ("_p" if planes else ""), "geglu_bwd", rows=rows, inner=inner,
                               p=p, planes=planes, seed=500 + i, site=i % 5))
    for act in ("none", "relu", "silu", "gelu"):
        for n in (1, 255, 256, 257):
            t.append(_case(f"G_act_{act}_n{n}", "G", "pfpp_act", "act", act=act, n=n, bwd=False))
            t.append(_case(f"G_act_bwd_{act}_n{n}", "G", "pfpp_act_bwd", "act", act=act, n=n, bwd=True))
    for n in (1, 5, 1023, 1024, 1025):
        for res in (False, True):
            for p in (0.0, 0.2):
                i += 1
                t.append(_case(f"G_dropout_n{n}_p{int(p * 10)}{'_res' if res else ''}", "G", "pfpp_dropout", "dropout", n=n, res=res, p=p,
                               seed=700 + i, site=i % 3))
    for n, p in ((1, 0.2), (255, 0.0), (1025, 0.2), (1025, 0.1)):
        t.append(_case(f"G_dropout_mask_n{n}_p{int(p * 10)}", "G", "pfpp_dropout_mask", "dropout_mask", n=n, p=p, seed=800 + n, site=4))
    return t


def _table_n():
    t = []
    pairs = ((64, 15), (64, 16), (64, 17), (64, 2047), (128, 2), (128, 2048), (256, 1), (256, 3), (256, 2049), (512, 1), (512, 4097),
             (1024, 1), (1024, 2), (1024, 2048))
    for i, (C, rows) in enumerate(pairs):
        t.append(_case(f"N_stats_c{C}_r{rows}", "N", "pfpp_bn_stats", "bn_stats", C=C, rows=rows, running=bool(i % 2) or rows == 1))
    for C, pool, orows in ((4, 0, 65), (4, 32, 1), (36, 0, 3), (36, 64, 3), (64, 0, 1), (64, 32, 65), (1024, 0, 3), (1024, 64, 1),
                           (1024, 32, 3)):
        t.append(_case(f"N_apply_c{C}_p{pool}_r{orows}", "N", "pfpp_bn_apply", "bn_apply", C=C, pool=pool, orows=orows))
    for copies in (1, 64):
        for C in (64, 300):
            t.append(_case(f"N_finalize_k{copies}_c{C}", "N", "pfpp_bn_finalize", "bn_finalize", copies=copies, C=C, rows=77,
                           running=copies == 64))
    for rows, C in ((1, 4), (3, 36), (5, 260)):
        t.append(_case(f"N_minmax_r{rows}_c{C}", "N", "pfpp_bn_minmax_apply", "bn_minmax", rows=rows, C=C))
    return t


def _table_p():
    t = []
    masks = ("none", "trailing", "scattered", "batch_masked")
    shapes = ((1, 1), (5, 1), (5, 5), (13, 5), (13, 13), (13, 1))                 # (rows_total, rows_per_batch)
    i = 0
    for T in (1, 63, 64, 65, 200):
        for pad in (0, 3):
            for mask in masks:
                rt, rpb = shapes[i % len(shapes)]
                if mask == "batch_masked" and rt // rpb < 2:
                    rt, rpb = 13, 5
                i += 1
                t.append(_case(f"P_softmax_t{T}_ld{T + pad}_{mask}_r{rt}_b{rpb}", "P", "pfpp_softmax_rows", "softmax", T=T, ld=T + pad,
                               mask=mask, rows=rt, rpb=rpb))
    for n in (1, 3):
        for L in (1, 25, 32):
            for C in (4, 260, 512):
                t.append(_case(f"P_mean_pool_n{n}_l{L}_c{C}", "P", "pfpp_mean_pool", "mean_pool", n=n, L=L, C=C, bwd=False))
                t.append(_case(f"P_mean_pool_bwd_n{n}_l{L}_c{C}", "P", "pfpp_mean_pool_bwd", "mean_pool", n=n, L=L, C=C, bwd=True))
    return t


def _table_m():
    t = []
    i = 0
    for n in (1, 63, 1023, 1024, 1025, 2049):
        for sel in ("none", "all", "one", "random"):
            go = (1.0, 4096.0)[i % 2]
            i += 1
            t.append(_case(f"M_mse_n{n}_{sel}_g{int(go)}", "M", "pfpp_mse_loss", "mse", n=n, sel=sel, grad_out=go, masked=False))
            t.append(_case(f"M_mse_masked_n{n}_{sel}_g{int(go)}", "M", "pfpp_mse_loss_masked", "mse", n=n, sel=sel, grad_out=go, masked=True))
    return t


def _table_a():
    t = []
    for i, n in enumerate((1, 255, 256, 257, 1000)):
        t.append(_case(f"A_adamw_n{n}", "A", "pfpp_adamw", "adamw", n=n, planes=bool(i % 2), zero_grad=False, g_scale=1.0, guarded=False,
                       direct=True))
        t.append(_case(f"A_adamw_zero_n{n}", "A", "pfpp_adamw_guarded", "adamw", n=n, planes=not i % 2, zero_grad=True, g_scale=1.0 / 4096,
                       guarded=False))
        t.append(_case(f"A_adamw_guarded_n{n}", "A", "pfpp_adamw_guarded", "adamw", n=n, planes=bool(i % 2), zero_grad=bool(i % 2),
                       g_scale=1.0 / 4096, guarded=True))
    return t


CASES = {c.name: c for c in _table_l() + _table_d() + _table_b() + _table_s() + _table_g() + _table_n() + _table_p() + _table_m()
         + _table_a()}
GROUPS = {g: [n for n, c in CASES.items() if c.group == g] for g in "LDBSGNPMA"}
assert len(CASES) == sum(len(v) for v in GROUPS.values())


# ------------------------------------------------------------------------------------------------------------ helpers (CPU)
f32, f16 = torch.float32, torch.float16


def _gen(c: Case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + salt)


def _dense(rows, cols, dtype, fill, data=None):
    """[rows, cols] with no leading dimension (the entry point has none): guard rows only"""
    return Buf(rows, cols, dtype, fill, left=0, right=0, align=1, data=data)


def _flat(n, dtype, fill, data=None):
    """n elements in a row, guard elements on either side and guard rows around it; the data starts 16-byte aligned"""
    return Buf(1, n, dtype, fill, left=16, right=GCOL, align=16, data=data)


def _wide(rows, cols, dtype, fill, pad, data=None):
    """[rows, cols] at the start of rows of cols + pad elements (ld > cols), guard rows above and below"""
    return Buf(rows, cols, dtype, fill, left=0, right=pad, align=1, data=data)


def _in(kind, *a, data=None):
    """an fp32 input: kind(rows, cols[, pad]) / _flat(n, None) with the guard fill of the moment"""
    fill = _GUARD_FILL[0]
    if kind is _flat:
        return _flat(a[0], f32, fill, data=data)
    return kind(*a[:2], f32, fill, *a[2:], data=data)


def keep_mask(n: int, p: float, seed: int, site: int) -> torch.Tensor:
    """uint8 [n]: the counter-based keep mask of csrc/pfpp_common.h (splitmix64 finaliser of (seed, site, index), keep iff the
    upper 32 bits are >= p 2^32 with p rounded to float32)"""
    t = float(np.float32(p)) * 4294967296.0
    thresh = 0 if t <= 0.0 else (4294967295 if t >= 4294967295.0 else int(t))
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (np.uint64(site) * np.uint64(0xD6E8FEB86659FD93))
        z = z + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return torch.from_numpy(((z >> np.uint64(32)) >= np.uint64(thresh)).astype(np.uint8))


def inv_keep32(p: float) -> torch.Tensor:
    """1.0f / (1.0f - p) as the launchers compute it"""
    return torch.tensor(1.0, dtype=f32) / (torch.tensor(1.0, dtype=f32) - torch.tensor(p, dtype=f32))


def row_profiles(rows, C, g):
    x = torch.randn(rows, C, generator=g)
    for r in range(rows):
        k = r % 8
        if k == 1:
            x[r] += 100.0
        elif k == 2:
            x[r] += 1e4
        elif k == 3:
            x[r] = 1.0 + 1e-3 * x[r]
        elif k == 4:
            x[r] *= 1e3
        elif k == 5:
            x[r] = 3.0
        elif k == 6:
            x[r] = 0.0
        elif k == 7:
            x[r, (37 * r) % C] = 1e4
    return x


def channel_profiles(rows, C, g):
    x = torch.randn(rows, C, generator=g)
    for k, off in ((1, 32.0), (2, 1000.0)):
        x[:, k::4] += off
    x[:, 3::4] = 3.0
    return x


def ln_stats(x, dt):
    x = x.to(dt)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    var = (xc * xc).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return mean, rstd, xc * rstd


def ln_eval(x, a, b, one, dt):
    _, _, y = ln_stats(x, dt)
    if a is not None:
        y = y * ((1.0 + a.to(dt)) if one else a.to(dt)) + b.to(dt)
    return y


def ln_unit(x, a, b, one):
    """-> (the unit, the unit with kappa + |xhat| in place of kappa)"""
    mean, rstd, xh = ln_stats(x, torch.float64)
    kappa = 1.0 + mean.abs() * rstd
    mult = torch.ones(1, 1, dtype=torch.float64) if a is None else ((1.0 + a.double()) if one else a.double())
    shift = torch.zeros(1, 1, dtype=torch.float64) if b is None else b.double()
    return ((U * kappa * (1.0 + mult.abs()) + U * shift.abs()).expand(x.shape).clone(),
            (U * (kappa + xh.abs()) * (1.0 + mult.abs()) + U * shift.abs()).expand(x.shape).clone())


def _both(fn):
    return fn(torch.float64), fn(torch.float32)


def _ln_operands(c: Case, g, rows, C, bufs):
    """the (a, b, one, kwargs description) of a LayerNorm form; adds mod / gamma / beta / group_batch to bufs"""
    form = c.o("form")
    info = dict(form=form)
    if form == "plain":
        return None, None, False, info
    if form == "affine":
        gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.5
        bufs["gamma"], bufs["beta"] = _in(_flat, C, None, data=gamma), _in(_flat, C, None, data=beta)
        return gamma[None], beta[None], False, info
    if form == "mod":
        rpb = c.o("rpb")
        bidx = torch.arange(rows) // rpb
        B = int(bidx.max()) + 1
        info["rpb"] = rpb
    else:
        gr = c.o("gr")
        ng = (rows + gr - 1) // gr
        gb = torch.tensor([GB_PATTERN[i % 4] for i in range(ng)], dtype=torch.int32)
        bidx = gb[torch.arange(rows) // gr].long()
        B = 4
        bufs["gb"] = _flat(ng, torch.int32, 3, data=gb)                # guard: the NaN row of mod
        info["gr"] = gr
    mod = torch.randn(B, 2 * C, generator=g) * 0.5
    used = torch.zeros(B, dtype=torch.bool)
    used[bidx] = True
    mod[~used] = _GUARD_FILL[0]
    bufs["mod"] = _in(_wide, B, 2 * C, 8, data=mod)                     # ld_mod = 2C + 8
    info["bidx"], info["B"], info["used"] = bidx, B, used
    return mod[bidx, :C], mod[bidx, C:], True, info


# ------------------------------------------------------------------------------------------------------------ builders (CPU)
def _build_ln(c: Case):
    g = _gen(c)
    C, rows = c.o("C"), c.o("rows")
    x = row_profiles(rows, C, g)
    bufs = {"x": _in(_dense, rows, C, data=x)}
    a, b, one, info = _ln_operands(c, g, rows, C, bufs)
    ref, yard = _both(lambda dt: ln_eval(x, a, b, one, dt))
    unit, unit_x = ln_unit(x, a, b, one)
    if c.o("split"):
        bufs["out_hi"], bufs["out_lo"] = _dense(rows, C, f16, SENTINEL_F16), _dense(rows, C, f16, SENTINEL_F16)
        checks = [Check("y", ("out_hi", "out_lo"), ref, unit, yard, kind="planes", unit_x=unit_x, x32="twin:out")]
    else:
        bufs["out"] = _dense(rows, C, f32, SENTINEL)
        checks = [Check("y", "out", ref, unit, yard, unit_x=unit_x)]
    return dict(bufs=bufs, checks=checks, info=info)


def dropout32(x, res, keep, p):
    """(res or 0) + x keep / (1 - p) in float32, the arithmetic of pfpp_dropout"""
    v = torch.where(keep.bool().view(x.shape), x * inv_keep32(p), torch.zeros((), dtype=f32))
    return (res if res is not None else torch.zeros_like(x)) + v


def _build_dln(c: Case):
    g = _gen(c)
    C, rows, p = c.o("C"), c.o("rows"), c.o("p")
    y = row_profiles(rows, C, g)
    res = torch.randn(rows, C, generator=g) if c.o("res") else None
    bufs = {"y": _in(_dense, rows, C, data=y)}
    if res is not None:
        bufs["res"] = _in(_dense, rows, C, data=res)
    a, b, one, info = _ln_operands(c, g, rows, C, bufs)
    keep = keep_mask(rows * C, p, c.o("seed"), c.o("site"))
    h = dropout32(y, res, keep, p)
    ref, yard = _both(lambda dt: ln_eval(h, a, b, one, dt))
    unit, unit_x = ln_unit(h, a, b, one)
    checks = [Check("h", "y", h, kind="bits")]
    if c.o("planes"):
        bufs["n_hi"], bufs["n_lo"] = _dense(rows, C, f16, SENTINEL_F16), _dense(rows, C, f16, SENTINEL_F16)
        checks.append(Check("n", ("n_hi", "n_lo"), ref, unit, yard, kind="planes", unit_x=unit_x, x32="twin:n"))
    else:
        bufs["n"] = _dense(rows, C, f32, SENTINEL)
        checks.append(Check("n", "n", ref, unit, yard, unit_x=unit_x))
    info["keep"] = keep
    return dict(bufs=bufs, checks=checks, info=info)


def _build_lnb(c: Case):
    g = _gen(c)
    C, gr, rows, form = c.o("C"), c.o("gr"), c.o("rows"), c.o("form")
    x, dy = row_profiles(rows, C, g), torch.randn(rows, C, generator=g)
    bufs = {"x": _in(_dense, rows, C, data=x), "dy": _in(_dense, rows, C, data=dy)}
    info = dict(form=form)
    ng = (rows + gr - 1) // gr
    mult32 = None
    if form in ("grp", "uni"):
        if form == "grp":
            gb = torch.tensor([(2, 0, 2, 1, 0)[i % 5] for i in range(ng)], dtype=torch.int32)
            bidx = gb[torch.arange(rows) // gr].long()
            B = 4
            bufs["gb"] = _flat(ng, torch.int32, 3, data=gb)
        else:
            bidx = torch.arange(rows) // (2 * gr)
            B = int(bidx.max()) + 1
        mod = torch.randn(B, 2 * C, generator=g) * 0.5
        used = torch.zeros(B, dtype=torch.bool)
        used[bidx] = True
        mod[~used] = _GUARD_FILL[0]
        bufs["mod"] = _in(_wide, B, 2 * C, 8, data=mod)
        mult32, one = mod[bidx, :C], True
        info.update(B=B, used=used)
    elif form == "gamma":
        gamma = torch.randn(C, generator=g) * 0.5 + 1.0
        bufs["gamma"] = _in(_flat, C, None, data=gamma)
        mult32, one = gamma[None].expand(rows, C), False
        bidx, B = torch.zeros(rows, dtype=torch.long), 1

    def mult_of(dt):
        if mult32 is None:
            return torch.ones(1, 1, dtype=dt)
        return (1.0 + mult32.to(dt)) if one else mult32.to(dt)

    def parts(dt):
        _, rstd, xh = ln_stats(x, dt)
        gg = dy.to(dt) * mult_of(dt)
        inc = rstd * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
        return rstd, xh, gg, inc
    mean64, rstd64, xh64 = ln_stats(x, torch.float64)
    kappa = 1.0 + mean64.abs() * rstd64
    gmax = (dy.double() * mult_of(torch.float64)).abs().amax(-1, keepdim=True)
    mag_dx = (kappa * rstd64 * gmax)                                    # [rows, 1]
    # the running gradient the kernel adds to: of the size of what is added (the unit has no term for it)
    dx0 = ((torch.rand(rows, C, generator=g).double() * 2 - 1) * (rstd64 * gmax)).float()
    bufs["dx"] = _dense(rows, C, f32, SENTINEL, data=dx0)
    ref, yard = _both(lambda dt: dx0.to(dt) + parts(dt)[3])
    unit_dx = (U * mag_dx).expand(rows, C).clone()
    checks = [Check("dx", "dx", ref, unit_dx, yard)]
    drop = c.o("drop")
    if drop is not None:
        p, seed, site = drop
        keep = keep_mask(rows * C, p, seed, site).bool().view(rows, C)
        ik = float(inv_keep32(p))
        zero = torch.zeros((), dtype=torch.float64)
        dref = torch.where(keep, ref * ik, zero)
        dyard = torch.where(keep, yard * inv_keep32(p), torch.zeros((), dtype=f32))
        dunit = torch.where(keep, unit_dx * ik, zero)
        info["keep"], info["p"] = keep, p
    if drop is not None:
        bufs["drop"] = _dense(rows, C, f32, SENTINEL)
        checks.append(Check("drop", "drop", dref, dunit, dyard))
    if c.o("planes"):
        sc = 4.0
        for k in ("dx_hi", "dx_lo", "ret_hi", "ret_lo"):
            bufs[k] = _dense(rows, C, f16, SENTINEL_F16)
        checks.append(Check("dx_planes", ("dx_hi", "dx_lo"), ref, unit_dx, yard, kind="planes", scale=sc, x32="dx"))
        if drop is not None:
            checks.append(Check("ret_planes", ("ret_hi", "ret_lo"), dref, dunit, dyard, kind="planes", scale=sc, x32="drop"))
        else:
            checks.append(Check("ret_planes", ("ret_hi", "ret_lo"), ref, unit_dx, yard, kind="planes", scale=sc, x32="dx"))
        info["scale"] = sc
    if form != "none":
        sel = torch.nn.functional.one_hot(bidx, B).double()            # [rows, B]
        # dmult: xhat itself carries 2^-24 (kappa + |xhat|) (the rounding of the row mean, times rstd), which the sum over the rows
        # inherits; with kappa = 1 this is the 2^-24 sum |dy xhat| of a well-centred row
        mag_m = sel.t() @ (dy.double().abs() * (xh64.abs() + kappa))   # [B, C]
        mag_a = sel.t() @ dy.double().abs()
        d0 = torch.rand(B, 2 * C, generator=g) * 2 - 1
        d0[:, :C] = (d0[:, :C].double() * mag_m).float()
        d0[:, C:] = (d0[:, C:].double() * mag_a).float()
        untouched = mag_a.sum(1) == 0                                   # batch rows no group refers to: any value, must keep its bits
        d0[untouched] = torch.randn(int(untouched.sum()), 2 * C, generator=g)
        bufs["dmods"] = Buf(B, 2 * C, f32, SENTINEL, left=0, right=8 if form != "gamma" else 0, align=1, data=d0)
        rm, ym = _both(lambda dt: d0[:, :C].to(dt) + sel.to(dt).t() @ (dy.to(dt) * parts(dt)[1]))
        ra, ya = _both(lambda dt: d0[:, C:].to(dt) + sel.to(dt).t() @ dy.to(dt))
        checks.append(Check("dmult", "dmods:lo", rm, U * mag_m, ym, atomic=True))
        checks.append(Check("dadd", "dmods:hi", ra, U * mag_a, ya, atomic=True))
        info["untouched"] = untouched
    return dict(bufs=bufs, checks=checks, info=info)


def _build_colsum(c: Case):
    g = _gen(c)
    cols, rows, batch, pad = c.o("cols"), c.o("rows"), c.o("batch"), c.o("pad")
    x_off = c.o("x_off", 0)
    xs = [channel_profiles(rows, cols, g) for _ in range(batch)]
    R = rows + 2 * TOP
    # batch slices stacked with their own guard rows; x_off shifts the data off the 16-byte grid (narrow kernel)
    xb = Buf(batch * R - 2 * TOP, cols, f32, _GUARD_FILL[0], left=x_off, right=pad, align=1)
    for z in range(batch):
        xb.alloc[TOP + z * R:TOP + z * R + rows, x_off:x_off + cols] = xs[z]
    xb.holes = [(TOP + z * R + rows, TOP + (z + 1) * R) for z in range(batch - 1)]
    mag = torch.stack([v.double().abs().sum(0) for v in xs])           # [batch, cols]
    o0 = ((torch.rand(batch, cols, generator=g).double() * 2 - 1) * mag).float()
    ob = Buf(batch, cols, f32, SENTINEL, left=GCOL, right=GCOL, align=1, data=o0)        # so = ld of this buffer
    acc = c.o("acc")
    ref, yard = _both(lambda dt: (o0.to(dt) if acc else 0.0) + torch.stack([v.to(dt).sum(0) for v in xs]))
    return dict(bufs={"x": xb, "out": ob}, checks=[Check("colsum", "out", ref, U * mag, yard, atomic=True)], info=dict(R=R))


def _build_colsum_planes(c: Case):
    g = _gen(c)
    cols, rows = c.o("cols"), c.o("rows")
    x = channel_profiles(rows, cols, g)
    scale = 4.0                                                         # out_scale = 1 / scale = 0.25
    hi, lo = split_cpu(x, 1.0)
    fill16 = max(-65504.0, min(65504.0, _GUARD_FILL[0])) if _GUARD_FILL[0] == _GUARD_FILL[0] else NAN    # (fp16: 1e30 -> the largest finite value)
    mk = lambda d: Buf(rows, cols, f16, fill16, left=0, right=8, align=1, data=d)
    val = hi.double() + lo.double()
    mag = val.abs().sum(0)[None] / scale
    o0 = ((torch.rand(1, cols, generator=g).double() * 2 - 1) * mag).float()
    ob = Buf(1, cols, f32, SENTINEL, left=GCOL, right=GCOL, align=1, data=o0)
    ref, yard = _both(lambda dt: o0.to(dt) + (hi.to(dt) + lo.to(dt)).sum(0)[None] / scale)
    return dict(bufs={"hi": mk(hi), "lo": mk(lo), "out": ob}, checks=[Check("colsum", "out", ref, U * mag, yard, atomic=True)],
                info=dict(scale=scale))


def _build_split(c: Case):
    g = _gen(c)
    n, scale = c.o("n"), c.o("scale")
    x = torch.randn(n, generator=g) * torch.logspace(-3, 3, n) / scale   # scale x spans the magnitudes of the plane-contract test
    bufs = {"x": _in(_flat, n, None, data=x), "hi": _flat(n, f16, SENTINEL_F16), "lo": _flat(n, f16, SENTINEL_F16)}
    ref = x.double()[None]
    return dict(bufs=bufs, checks=[Check("planes", ("hi", "lo"), ref, torch.zeros_like(ref), x[None].clone(), kind="planes", scale=scale, x32="x")],
                info={})


def gelu_t(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))


def gelu_grad_t(v):
    return 0.5 * (1.0 + torch.erf(v * 0.7071067811865476)) + v * 0.3989422804014327 * torch.exp(-0.5 * v * v)


def silu_t(v):
    return v / (1.0 + torch.exp(-v))


def silu_grad_t(v):
    s = 1.0 / (1.0 + torch.exp(-v))
    return s * (1.0 + v * (1.0 - s))


def _geglu_z(c, g):
    rows, inner = c.o("rows"), c.o("inner")
    z = torch.randn(rows, 2 * inner, generator=g)
    vals = torch.tensor(GATE_VALUES, dtype=f32)
    nlist = min(inner, max(16, inner // 2))                             # gate column c < nlist: the value c % 16 of the list; the rest normal
    z[:, inner:inner + nlist] = vals[torch.arange(nlist) % 16][None].expand(rows, nlist)
    return z


def _build_geglu(c: Case):
    g = _gen(c)
    rows, inner, p = c.o("rows"), c.o("inner"), c.o("p")
    z = _geglu_z(c, g)
    keep = keep_mask(rows * inner, p, c.o("seed"), c.o("site")).bool().view(rows, inner)
    ik = float(inv_keep32(p))
    bufs = {"z": _in(_dense, rows, 2 * inner, data=z)}
    bwd = c.kind == "geglu_bwd"
    v64, g64 = z[:, :inner].double(), z[:, inner:].double()
    if not bwd:
        def f(dt):
            o = z[:, :inner].to(dt) * gelu_t(z[:, inner:].to(dt))
            return torch.where(keep, o * (inv_keep32(p).to(dt) if p else 1.0), torch.zeros((), dtype=dt))
        ref, yard = _both(f)
        unit = torch.where(keep, U * ik * v64.abs() * torch.maximum(g64.abs(), gelu_t(g64).abs()), torch.zeros((), dtype=torch.float64))
        scale = 1.0
    else:
        du = torch.randn(rows, inner, generator=g) * 1e-2
        bufs["du"] = _in(_dense, rows, inner, data=du)

        def f(dt):
            d = torch.where(keep, du.to(dt) * (inv_keep32(p).to(dt) if p else 1.0), torch.zeros((), dtype=dt))
            gg, vv = z[:, inner:].to(dt), z[:, :inner].to(dt)
            return torch.cat([d * gelu_t(gg), d * vv * gelu_grad_t(gg)], 1)
        ref, yard = _both(f)
        d64 = torch.where(keep, du.double() * ik, torch.zeros((), dtype=torch.float64)).abs()
        unit = U * torch.cat([d64 * torch.maximum(g64.abs(), gelu_t(g64).abs()),
                              d64 * v64.abs() * torch.maximum(g64.abs(), gelu_grad_t(g64).abs())], 1)
        scale = 64.0
    if c.o("planes"):
        bufs["out_hi"], bufs["out_lo"] = _dense(rows, ref.shape[1], f16, SENTINEL_F16), _dense(rows, ref.shape[1], f16, SENTINEL_F16)
        checks = [Check("u", ("out_hi", "out_lo"), ref, unit, yard, kind="planes", scale=scale, x32="twin:out")]
    else:
        bufs["out"] = _dense(rows, ref.shape[1], f32, SENTINEL)
        checks = [Check("u", "out", ref, unit, yard)]
    return dict(bufs=bufs, checks=checks, info=dict(scale=scale))


ACT_FWD = {"none": lambda v: v, "relu": torch.relu, "silu": silu_t, "gelu": gelu_t}
ACT_BWD = {"none": lambda v: torch.ones_like(v), "relu": lambda v: (v > 0).to(v.dtype), "silu": silu_grad_t, "gelu": gelu_grad_t}


def _build_act(c: Case):
    g = _gen(c)
    n, act, bwd = c.o("n"), c.o("act"), c.o("bwd")
    vals = torch.tensor(ACT_VALUES, dtype=f32)
    pre = torch.randn(n, generator=g)
    k = min(n, len(ACT_VALUES))
    pre[:k] = vals[(torch.arange(k) + n) % len(ACT_VALUES)]
    bufs = {"pre": _in(_flat, n, None, data=pre), "out": _flat(n, f32, SENTINEL)}
    p64 = pre.double()
    if bwd:
        dy = torch.randn(n, generator=g)
        bufs["dy"] = _in(_flat, n, None, data=dy)
        ref, yard = _both(lambda dt: dy.to(dt) * ACT_BWD[act](pre.to(dt)))
        unit = U * dy.double().abs() * torch.maximum(p64.abs(), ACT_BWD[act](p64).abs())
    else:
        ref, yard = _both(lambda dt: ACT_FWD[act](pre.to(dt)))
        unit = U * torch.maximum(p64.abs(), ACT_FWD[act](p64).abs())
    return dict(bufs=bufs, checks=[Check("out", "out", ref[None], unit[None], yard[None])], info={})


def _build_dropout(c: Case):
    g = _gen(c)
    n, p = c.o("n"), c.o("p")
    x = torch.randn(n, generator=g)
    res = torch.randn(n, generator=g) if c.o("res") else None
    keep = keep_mask(n, p, c.o("seed"), c.o("site"))
    bufs = {"x": _in(_flat, n, None, data=x), "out": _flat(n, f32, SENTINEL)}
    if res is not None:
        bufs["res"] = _in(_flat, n, None, data=res)
    want = dropout32(x, res, keep, p)
    return dict(bufs=bufs, checks=[Check("out", "out", want[None], kind="bits")], info=dict(keep=keep))


def _build_dropout_mask(c: Case):
    keep = keep_mask(c.o("n"), c.o("p"), c.o("seed"), c.o("site"))
    bufs = {"keep": _flat(c.o("n"), torch.uint8, SENTINEL_U8)}
    return dict(bufs=bufs, checks=[Check("keep", "keep", keep[None], kind="bits")], info={})


def _build_bn_stats(c: Case):
    g = _gen(c)
    C, rows = c.o("C"), c.o("rows")
    x = channel_profiles(rows, C, g)
    bufs = {"x": _in(_wide, rows, C, 4, data=x), "mean": _flat(C, f32, SENTINEL), "var": _flat(C, f32, SENTINEL)}
    x64 = x.double()
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)                                   # biased
    sig = var.sqrt()
    u_m, u_v = U * (mean.abs() + sig), U * (var + mean.abs() * sig)
    ym = x.mean(0)
    yv = ((x - ym) ** 2).mean(0)
    checks = [Check("mean", "mean", mean[None], u_m[None], ym[None]), Check("var", "var", var[None], u_v[None], yv[None])]
    if c.o("running"):
        mom = 0.1
        r0m, r0v = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        bufs["rmean"], bufs["rvar"] = _flat(C, f32, SENTINEL, data=r0m), _flat(C, f32, SENTINEL, data=r0v)
        unb = var * rows / (rows - 1) if rows > 1 else var              # the kernel's rule for one row (torch refuses that input)
        yunb = yv * rows / (rows - 1) if rows > 1 else yv
        checks.append(Check("running_mean", "rmean", ((1 - mom) * r0m.double() + mom * mean)[None],
                            (U * (1 - mom) * r0m.double().abs() + mom * u_m)[None], ((1 - mom) * r0m + mom * ym)[None]))
        checks.append(Check("running_var", "rvar", ((1 - mom) * r0v.double() + mom * unb)[None],
                            (U * (1 - mom) * r0v.double().abs() + mom * u_v * (rows / max(rows - 1, 1)))[None],
                            ((1 - mom) * r0v + mom * yunb)[None]))
    return dict(bufs=bufs, checks=checks, info={})


def _bn_affine(C, g):
    gamma = torch.randn(C, generator=g) * 0.5 + 1.0
    gamma[1::8] *= -1.0
    beta = torch.randn(C, generator=g) * 0.5
    return gamma, beta


def _build_bn_apply(c: Case):
    g = _gen(c)
    C, pool, orows = c.o("C"), c.o("pool"), c.o("orows")
    rows = orows * (pool or 1)
    x = channel_profiles(rows, C, g)
    x64 = x.double()
    mean, var = x64.mean(0).float(), ((x64 - x64.mean(0)) ** 2).mean(0).float()
    gamma, beta = _bn_affine(C, g)
    beta[0] = -10.0                                                     # a channel (and so every pool group of it) that is negative throughout
    bufs = {"x": _in(_wide, rows, C, 4, data=x), "out": Buf(orows, C, f32, SENTINEL, left=0, right=8, align=1)}
    for k, v in (("mean", mean), ("var", var), ("gamma", gamma), ("beta", beta)):
        bufs[k] = _in(_flat, C, None, data=v)

    def pooled(v):
        return v.view(orows, pool, C).amax(1) if pool else v
    a64 = gamma.double() / torch.sqrt(var.double() + EPS)
    ref = pooled(torch.relu((x64 - mean.double()) * a64 + beta.double()))
    a32 = gamma * (1.0 / torch.sqrt(var + EPS))
    yard = pooled(torch.relu(x * a32 + (beta - mean * a32)))
    unit = pooled(U * ((x64 * a64).abs() + (mean.double() * a64).abs() + beta.double().abs() + 1.0))
    return dict(bufs=bufs, checks=[Check("y", "out", ref, unit, yard)], info=dict(rows=rows))


def _build_bn_finalize(c: Case):
    g = _gen(c)
    copies, C, rows = c.o("copies"), c.o("C"), c.o("rows")
    x = channel_profiles(rows, C, g).double()
    # (no constant channel here: E[x^2] - mean^2 of one is all cancellation, in the reference as much as in the kernel)
    x[:, 3::4] = 0.5 + 0.1 * torch.randn(rows, len(range(3, C, 4)), generator=g).double()
    s, q = x.sum(0), (x * x).sum(0)
    w = torch.rand(copies, 1, generator=g).double() + 0.1
    w = w / w.sum()
    stats = torch.stack([w * s[None], w * q[None]], 1)                  # [copies, 2, C]
    gamma, beta = _bn_affine(C, g)
    bufs = {"stats": Buf(copies * 2, C, torch.float64, SENTINEL, left=0, right=0, align=1, data=stats.view(copies * 2, C)),
            "gamma": _in(_flat, C, None, data=gamma), "beta": _in(_flat, C, None, data=beta)}
    for k in ("a_mul", "a_add", "mean", "var"):
        bufs[k] = _flat(C, f32, SENTINEL)
    st = bufs["stats"].view.view(copies, 2, C)                          # (as stored: the sums the kernel will see)
    s, q = st[:, 0].sum(0), st[:, 1].sum(0)
    mean = s / rows
    var = (q / rows - mean * mean).clamp_min(0.0)
    sig = var.sqrt()
    u_m, u_v = U * (mean.abs() + sig), U * (var + mean.abs() * sig)
    a = gamma.double() / torch.sqrt(var + EPS)
    b = beta.double() - mean * a
    m32, v32 = mean.float(), var.float()
    a32 = gamma * (1.0 / torch.sqrt(v32 + EPS))
    checks = [Check("mean", "mean", mean[None], u_m[None], m32[None]), Check("var", "var", var[None], u_v[None], v32[None]),
              Check("a_mul", "a_mul", a[None], (U * a.abs())[None], a32[None]),
              Check("a_add", "a_add", b[None], (U * (beta.double().abs() + (mean * a).abs()))[None], (beta - m32 * a32)[None]),
              Check("stats_cleared", "stats", torch.zeros(copies * 2, C, dtype=torch.float64), kind="bits")]
    if c.o("running"):
        mom = 0.1
        r0m, r0v = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        bufs["rmean"], bufs["rvar"] = _flat(C, f32, SENTINEL, data=r0m), _flat(C, f32, SENTINEL, data=r0v)
        unb = var * rows / (rows - 1)
        checks.append(Check("running_mean", "rmean", ((1 - mom) * r0m.double() + mom * mean)[None],
                            (U * (1 - mom) * r0m.double().abs() + mom * u_m)[None], ((1 - mom) * r0m + mom * m32)[None]))
        checks.append(Check("running_var", "rvar", ((1 - mom) * r0v.double() + mom * unb)[None],
                            (U * (1 - mom) * r0v.double().abs() + mom * u_v * rows / (rows - 1))[None],
                            ((1 - mom) * r0v + mom * v32 * rows / (rows - 1))[None]))
    return dict(bufs=bufs, checks=checks, info={})


def _build_bn_minmax(c: Case):
    g = _gen(c)
    rows, C, pool = c.o("rows"), c.o("C"), 8
    x = torch.randn(rows, pool, C, generator=g) * 2.0
    a = torch.randn(C, generator=g)
    a[0::3] = -a[0::3].abs()
    a[1::3] = a[1::3].abs()
    a[2::6] = 0.0
    b = torch.randn(C, generator=g)
    mx, mn = x.amax(1), x.amin(1)
    bufs = {"mx": _in(_dense, rows, C, data=mx), "mn": _in(_dense, rows, C, data=mn), "a": _in(_flat, C, None, data=a),
            "b": _in(_flat, C, None, data=b), "out": _dense(rows, C, f32, SENTINEL)}
    ref, yard = _both(lambda dt: torch.relu(a.to(dt) * x.to(dt) + b.to(dt)).amax(1))
    unit = (U * ((a.double() * x.double()).abs() + b.double().abs() + 1.0)).amax(1)
    return dict(bufs=bufs, checks=[Check("y", "out", ref, unit, yard)], info={})


def _build_softmax(c: Case):
    g = _gen(c)
    T, ld, rows, rpb, mask = c.o("T"), c.o("ld"), c.o("rows"), c.o("rpb"), c.o("mask")
    scale = 0.125
    s = torch.randn(rows, T, generator=g) * 8.0
    big = torch.rand(rows, T, generator=g)
    s[big < 0.05] = 640.0
    s[big > 0.95] = -640.0
    nb = (rows + rpb - 1) // rpb
    kv = torch.ones(nb, T, dtype=torch.uint8)
    if mask == "trailing":
        kv[:, (T + 1) // 2:] = 0
    elif mask in ("scattered", "batch_masked"):
        kv = (torch.rand(nb, T, generator=g) < 0.6).to(torch.uint8)
        kv[:, 0] = 1
        if mask == "batch_masked":
            kv[1] = 0
    S = torch.full((rows, ld), 5.0)                                    # the pad columns T .. ld hold a finite non-zero value: the launch zeroes them
    S[:, :T] = s
    bufs = {"S": _dense(rows, ld, f32, SENTINEL, data=S)}
    if mask != "none":
        bufs["kv"] = Buf(nb, T, torch.uint8, 1, left=0, right=0, align=1, data=kv)
    valid = kv[torch.arange(rows) // rpb].bool()

    def f(dt):
        a = s.to(dt) * scale
        a = torch.where(valid, a, torch.full((), -float("inf"), dtype=dt))
        m = a.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros((), dtype=dt))
        e = torch.where(valid, torch.exp(a - m), torch.zeros((), dtype=dt))
        den = e.sum(-1, keepdim=True)
        p = torch.where(den > 0, e / den, torch.zeros((), dtype=dt))
        out = torch.zeros(rows, ld, dtype=dt)
        out[:, :T] = p
        return out, a - m
    (ref, arg), (yard, _) = f(torch.float64), f(torch.float32)
    unit = torch.zeros(rows, ld, dtype=torch.float64)
    unit[:, :T] = torch.where(valid, U * ref[:, :T] * (1.0 + arg.abs()) + TINY, torch.zeros((), dtype=torch.float64))
    return dict(bufs=bufs, checks=[Check("p", "S", ref, unit, yard)], info=dict(scale=scale, live=valid.any(-1)))


def _build_mean_pool(c: Case):
    g = _gen(c)
    n, L, C = c.o("n"), c.o("L"), c.o("C")
    if c.o("bwd"):
        dp = torch.randn(n, C, generator=g)
        bufs = {"dp": _in(_dense, n, C, data=dp), "out": _dense(n * L, C, f32, SENTINEL)}
        ref, yard = _both(lambda dt: (dp.to(dt) / L)[:, None].expand(n, L, C).reshape(n * L, C))
        return dict(bufs=bufs, checks=[Check("dx", "out", ref, U * ref.abs(), yard)], info={})
    x = row_profiles(n * L, C, g)
    bufs = {"x": _in(_dense, n * L, C, data=x), "out": _dense(n, C, f32, SENTINEL)}
    ref, yard = _both(lambda dt: x.to(dt).view(n, L, C).sum(1) / L)
    return dict(bufs=bufs, checks=[Check("pooled", "out", ref, U * x.double().abs().view(n, L, C).sum(1) / L, yard)], info={})


def _build_mse(c: Case):
    gname = Case(c.name.replace("_masked", ""), c.group, c.entry, c.kind, c.opts)       # the masked case has the inputs of its sel twin
    g = _gen(gname)
    n, W, sel_kind, go = c.o("n"), 7, c.o("sel"), c.o("grad_out")
    pred, target = torch.randn(n, W, generator=g), torch.randn(n, W, generator=g)
    sel = torch.zeros(n, dtype=torch.bool)
    if sel_kind == "all":
        sel[:] = True
    elif sel_kind == "one":
        sel[(n * 2) // 3] = True
    elif sel_kind == "random":
        sel = torch.rand(n, generator=g) < 0.2
        sel[n - 1] = True
    fill = _GUARD_FILL[0]
    bufs = {"pred": _in(_dense, n, W, data=pred), "target": _in(_dense, n, W, data=target), "loss": _flat(1, f32, SENTINEL),
            "dpred": _dense(n, W, f32, SENTINEL)}
    pred_, target_ = pred.clone(), target.clone()
    pred_[~sel] = fill                                                  # rows that are not selected are never read: they hold the guard value too
    bufs["pred"].view[...] = pred_
    if c.o("masked"):
        ref_u8 = ((torch.arange(n) % 3 == 0) & ~sel).to(torch.uint8)
        valid = (sel | (ref_u8 != 0)).float() * 2.5                      # any non-zero value counts
        bufs["valid"], bufs["ref"] = _flat(n, f32, 1.0, data=valid), _flat(n, torch.uint8, 0, data=ref_u8)
        bufs["amax"] = _flat(1, f32, SENTINEL, data=torch.full((1,), -1.0))
    else:
        bufs["sel"] = _flat(n, torch.uint8, 1, data=sel.to(torch.uint8))
    cnt = int(sel.sum())

    def f(dt):
        d = torch.where(sel[:, None], pred.to(dt) - target.to(dt), torch.zeros((), dtype=dt))
        if cnt == 0:
            return torch.full((1,), float("nan"), dtype=dt), torch.zeros(n, W, dtype=dt)
        loss = (d[sel] ** 2).mean().reshape(1)
        k = torch.tensor(go, dtype=dt) * 2.0 / torch.tensor(cnt * float(W), dtype=dt)
        return loss, k * d
    (rl, rg), (yl, yg) = f(torch.float64), f(torch.float32)
    if cnt == 0:                                                        # NaN loss (0 / 0 like torch's mean over nothing), gradient exactly zero
        checks = [Check("loss", "loss", torch.full((1, 1), float("nan")), kind="bits"), Check("dpred", "dpred", torch.zeros(n, W), kind="bits")]
    else:
        checks = [Check("loss", "loss", rl[None], U * rl.abs()[None], yl[None]), Check("dpred", "dpred", rg, U * rg.abs(), yg)]
    return dict(bufs=bufs, checks=checks, info=dict(sel=sel, cnt=cnt))


ADAM = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
ADAM_STEPS = 3


def adam_bad_positions(n):
    """(index, value) of the non-finite gradients of a guarded case: element 0, the last one, both sides of the first workgroup edge"""
    pos = {0: float("inf"), n - 1: float("-inf")}
    if n > 256:
        pos[255], pos[256] = float("nan"), float("inf")
    elif n > 255:
        pos[254] = float("nan")
    if n - 1 in pos and n == 1:
        pos = {0: float("nan")}
    return pos


def _build_adamw(c: Case):
    g = _gen(c)
    n, gs = c.o("n"), c.o("g_scale")
    p0, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    grads = [torch.randn(n, generator=g) * (10.0 ** (i - 1)) / gs for i in range(ADAM_STEPS)]
    bad = adam_bad_positions(n) if c.o("guarded") else {}
    for gr_ in grads:
        for i, v in bad.items():
            gr_[i] = v
    bufs = {"p": _flat(n, f32, SENTINEL, data=p0), "m": _flat(n, f32, SENTINEL, data=m0), "v": _flat(n, f32, SENTINEL, data=v0)}
    for i, gr_ in enumerate(grads):
        bufs[f"g{i}"] = _flat(n, f32, SENTINEL, data=gr_)
    if c.o("planes"):
        bufs["hi"], bufs["lo"] = _flat(n, f16, SENTINEL_F16), _flat(n, f16, SENTINEL_F16)
    ok = torch.ones(n, dtype=torch.bool)
    ok[list(bad)] = False
    h = {k: float(np.float32(v)) for k, v in ADAM.items()}              # the float32 values the entry point receives

    def f(dt):
        p, m, v = p0.to(dt), m0.to(dt), v0.to(dt)
        up, um = torch.zeros(n, dtype=dt), m0.to(dt).abs()
        T = lambda val: torch.tensor(val, dtype=dt)
        for t, gr_ in enumerate(grads, 1):
            gg = torch.where(ok, gr_.to(dt) * T(gs), torch.zeros((), dtype=dt))
            bc1, bc2 = float(np.float32(1.0 - ADAM["beta1"] ** t)), float(np.float32(1.0 - ADAM["beta2"] ** t))
            if dt == f32:                                              # torch.optim.AdamW's single-tensor order of operations
                p2 = p * (T(1.0) - T(h["lr"]) * T(h["weight_decay"]))
                m2 = m + (T(1.0) - T(h["beta1"])) * (gg - m)
                v2 = v * T(h["beta2"]) + (T(1.0) - T(h["beta2"])) * (gg * gg)
                den = v2.sqrt() / T(math.sqrt(bc2)) + T(h["eps"])
                step = T(h["lr"] / bc1) * (m2 / den)
            else:
                p2 = p * (1.0 - h["lr"] * h["weight_decay"])
                m2 = h["beta1"] * m + (1.0 - h["beta1"]) * gg
                v2 = h["beta2"] * v + (1.0 - h["beta2"]) * gg * gg
                den = v2.sqrt() / math.sqrt(bc2) + h["eps"]
                step = (h["lr"] / bc1) * m2 / den
            # magnitudes of the terms summed: m is a sum of terms of either sign, so the step carries |terms of m| / den, not |m| / den
            um = torch.where(ok, h["beta1"] * um + (1.0 - h["beta1"]) * gg.abs(), um)
            up = up + torch.where(ok, p2.abs() + (h["lr"] / bc1) * um / den, torch.zeros((), dtype=dt))
            p, m, v = torch.where(ok, p2 - step, p), torch.where(ok, m2, m), torch.where(ok, v2, v)
        return p, m, v, up, um, v.abs()
    (rp, rm, rv, up, um, uv), (yp, ym, yv, _, _, _) = f(torch.float64), f(torch.float32)
    okd = ok.double()                                                   # (skipped elements: unit 0, they keep their bits)
    checks = [Check("p", "p", rp[None], (U * up * okd)[None], yp[None]), Check("m", "m", rm[None], (U * um * okd)[None], ym[None]),
              Check("v", "v", rv[None], (U * uv * okd)[None], yv[None])]
    if c.o("planes"):                                                   # (skipped elements: the planes keep the sentinel, in bits)
        checks.append(Check("planes", ("hi", "lo"), rp[None], (U * up * okd)[None], yp[None].clone(), kind="planes", x32="p",
                            skip=(~ok)[None] if bad else None))
    if c.o("zero_grad"):
        for i in range(ADAM_STEPS):
            checks.append(Check(f"g{i}_cleared", f"g{i}", torch.zeros(1, n), kind="bits"))
    if c.o("guarded"):
        checks.append(Check("overflow", "ret:overflow", torch.tensor([1, ADAM_STEPS * len(bad)], dtype=torch.int32), kind="bits"))
    return dict(bufs=bufs, checks=checks, info=dict(bad=bad, ok=ok, grads=grads))


_BUILDERS = dict(ln=_build_ln, dln=_build_dln, lnb=_build_lnb, colsum=_build_colsum, colsum_planes=_build_colsum_planes, split=_build_split,
                 geglu=_build_geglu, geglu_bwd=_build_geglu, act=_build_act, dropout=_build_dropout, dropout_mask=_build_dropout_mask,
                 bn_stats=_build_bn_stats, bn_apply=_build_bn_apply, bn_finalize=_build_bn_finalize, bn_minmax=_build_bn_minmax,
                 softmax=_build_softmax, mean_pool=_build_mean_pool, mse=_build_mse, adamw=_build_adamw)


@lru_cache(maxsize=4)
def built(c: Case):
    """CPU side of a case: bufs {name: Buf}, checks [Check], info; cached: treat as read-only"""
    return _BUILDERS[c.kind](c)


def built_with_guards(c: Case, fill: float):
    """the case built again (not cached) with `fill` instead of NaN in every input guard"""
    _GUARD_FILL[0] = fill
    try:
        return _BUILDERS[c.kind](c)
    finally:
        _GUARD_FILL[0] = NAN


# ------------------------------------------------------------------------------------------------------------ layout rules
def check_layout(c: Case):
    """the alignment and divisibility rules of the entry point (its PFPP_REQUIRE lines) on the case's buffers"""
    b = built(c)["bufs"]
    a16 = lambda k: (b[k].off * b[k].alloc.element_size()) % 16 == 0
    a8 = lambda k: (b[k].off * b[k].alloc.element_size()) % 8 == 0
    e = c.entry
    if e.startswith(("pfpp_layernorm", "pfpp_dropout_layernorm")):
        bwd = "bwd" in e
        assert c.o("C") in ((256, 512) if (bwd or "dropout" in e) else (256, 512, 1024))
        assert all(a16(k) for k in b if k != "gb"), c.name
        if "mod" in b:
            assert b["mod"].ld % 4 == 0 and b["mod"].ld > 2 * c.o("C")
        if bwd:
            assert c.o("rows") > (c.o("rows") - 1) // c.o("gr") * c.o("gr")        # (the last group has at least one row)
        if "dmods" in b and c.o("form") != "gamma":
            assert b["dmods"].ld == 2 * c.o("C") + 8
    elif e == "pfpp_colsum":
        vec = c.o("cols") % 4 == 0 and b["x"].ld % 4 == 0 and a16("x") and (built(c)["info"]["R"] * b["x"].ld) % 4 == 0
        assert vec == (c.o("cols") % 4 == 0 and c.o("pad") % 4 == 0), c.name
        assert b["x"].ld >= c.o("cols") and (c.o("pad") == 4) <= vec
    elif e == "pfpp_colsum_planes":
        assert c.o("cols") % 4 == 0 and b["hi"].ld % 4 == 0 and b["hi"].ld > c.o("cols") and a8("hi") and a8("lo")
    elif e == "pfpp_split_planes":
        assert c.o("n") % 4 == 0 and a16("x") and a8("hi") and a8("lo")
    elif e.startswith("pfpp_geglu"):
        assert c.o("inner") % 4 == 0 and all(a16(k) for k in b)
    elif e == "pfpp_dropout":
        assert all(a16(k) for k in b)
    elif e == "pfpp_bn_stats":
        assert c.o("C") in (64, 128, 256, 512, 1024) and b["x"].ld % 4 == 0 and b["x"].ld > c.o("C") and a16("x")
    elif e == "pfpp_bn_apply":
        assert c.o("C") % 4 == 0 and c.o("C") <= 1024 and b["x"].ld % 4 == 0 and b["out"].ld % 4 == 0
        assert b["x"].ld > c.o("C") and b["out"].ld > c.o("C") and all(a16(k) for k in b)
    elif e == "pfpp_mean_pool_bwd":
        assert c.o("C") % 4 == 0 and all(a16(k) for k in b)
    elif e == "pfpp_softmax_rows":
        assert c.o("ld") >= c.o("T") >= 1
    elif e.startswith("pfpp_adamw") and c.o("planes"):
        assert a8("hi") and a8("lo")


# ------------------------------------------------------------------------------------------------------------ evaluation
def _data_of(b: dict, key: str, alloc: torch.Tensor):
    """the data region of buffer `key` (or of one half of dmods) inside an allocation"""
    name, _, half = key.partition(":")
    buf = b["bufs"][name]
    v = alloc[buf.top:buf.top + buf.rows, buf.left:buf.left + buf.cols]
    if half:
        C = buf.cols // 2
        v = v[:, :C] if half == "lo" else v[:, C:]
    return v


def _got(b: dict, ch: Check, outs: dict, rets: dict):
    def one(key):
        return rets[key[4:]] if key.startswith("ret:") else _data_of(b, key, outs[key.partition(":")[0]])
    if isinstance(ch.out, tuple):
        return one(ch.out[0]), one(ch.out[1])
    return one(ch.out)


def _live(ch: Check):
    """the elements of a plane check that are compared: finite reference, not skipped by the kernel"""
    ok = torch.isfinite(ch.ref)
    return ok if ch.skip is None else ok & ~ch.skip


def planes_error(ch: Check, hi: torch.Tensor, lo: torch.Tensor, group: str):
    """worst |hi + lo - scale ref| over its allowance: the bound of the group (both units where there are two) plus the split's own
    2^-20 |value| + 1.3e-7"""
    ok = _live(ch)
    x = (ch.ref * ch.scale)[ok]
    h, l = hi.double().reshape(ch.ref.shape)[ok], lo.double().reshape(ch.ref.shape)[ok]
    slack = K[group] * ch.unit[ok]
    if ch.unit_x is not None:
        slack = torch.minimum(slack, KX[group] * ch.unit_x[ok])
    allow = ch.scale * slack + x.abs() * 2.0 ** -20 + 1.3e-7
    e = float((((h + l) - x).abs() / allow).max()) if x.numel() else 0.0
    return e if math.isfinite(e) else math.inf


def planes_contract(ch: Check, x32: torch.Tensor, hi: torch.Tensor, lo: torch.Tensor):
    """the plane contract of the project on its own (tests/test_gpu_train_ops.py, _assert_planes_carry), for the float32 value x32 that
    the kernel itself computed -> (worst |hi + lo - scale x| over 2^-20 |scale x| + 1.3e-7, worst |scale x - hi| over half an fp16
    ulp of hi); both must be <= 1.  Elements of ch.skip are left out (they are compared in bits elsewhere)"""
    x = x32.double().reshape(ch.ref.shape) * ch.scale
    ok = torch.isfinite(x)
    if float(ok.double().mean()) < 1.0 - MAX_EXCLUDED:
        return math.inf, math.inf
    if ch.skip is not None:
        ok = ok & ~ch.skip
    x = x[ok]
    h, l = hi.double().reshape(ch.ref.shape)[ok], lo.double().reshape(ch.ref.shape)[ok]
    if x.numel() == 0:
        return 0.0, 0.0
    e1 = float((((h + l) - x).abs() / (x.abs() * 2.0 ** -20 + 1.3e-7)).max())
    ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -14))) - 10), torch.tensor(2.0 ** -24, dtype=torch.float64))
    e2 = float(((x - h).abs() / (0.5 * ulp * (1 + 2.0 ** -10) + 1e-12)).max())
    if not (math.isfinite(e1) and math.isfinite(e2)):
        return math.inf, math.inf
    return e1, e2


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    """equal dtype and bits; a NaN matches a NaN whatever its payload (the empty-selection loss)"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not want.dtype.is_floating_point:
        return bool(torch.equal(got, want))
    n = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), n)) and bool(torch.equal(_bits(got[~n]), _bits(want[~n])))


def units_error(ch: Check, got: torch.Tensor, second: bool = False):
    """worst |got - ref| / unit (second: / unit_x) over the elements with a finite reference (unit 0: the result must be exact);
    non-finite -> inf"""
    ok = torch.isfinite(ch.ref)
    d = (got.double().reshape(ch.ref.shape) - ch.ref).abs()[ok]
    u = (ch.unit_x if second else ch.unit)[ok]
    if d.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(d).all()):
        return math.inf
    r = torch.where(d == 0, torch.zeros_like(d), d / u)                # (x / 0 = inf for x > 0)
    return float(r.max())


def excluded_fraction(ch: Check) -> float:
    if ch.kind == "bits":
        return 0.0
    return 1.0 - float(torch.isfinite(ch.ref).double().mean())


def yardstick(c: Case, second: bool = False):
    """[(tag, error of the float32 CPU evaluation in units)] of the case's bounded checks (second: in the units of KX)"""
    res = []
    for ch in built(c)["checks"]:
        if ch.kind == "bits" or c.kind == "split" or (second and ch.unit_x is None):
            continue
        res.append((ch.tag, units_error(ch, ch.yard, second)))
    return res


def twin_of(c: Case) -> Case:
    """the fp32 form of a plane-producing case on the same inputs (the seed is the name's, which the two share); not in the table"""
    o = dict(c.opts)
    o["split" if "split" in o else "planes"] = False
    return Case(c.name, c.group, c.entry, c.kind, tuple(sorted(o.items())))


def needs_twin(c: Case) -> bool:
    return any(ch.kind == "planes" and ch.x32.startswith("twin:") for ch in built(c)["checks"])


def evaluate(c: Case, outs: dict, rets: dict, twin_outs: Optional[dict] = None):
    """outs {buffer: allocation after the launch (CPU)}, rets {key: tensor the wrapper returned (CPU)}, twin_outs: the allocations
    after the launch of twin_of(c), where the case needs it ->
    dict(case, entry, lines [(tag, error in units, bound in units)], guards_ok, untouched_ok, bits_ok, ok)"""
    b = built(c)
    k = K[c.group]
    lines, bits_ok = [], True
    guards = True
    for name, after in outs.items():
        buf = b["bufs"][name]
        m = buf.guard_mask()
        guards &= bool(torch.equal(_bits(after[m]), _bits(buf.alloc[m])))
    untouched = True
    if "untouched" in b["info"] and "dmods" in outs:
        rows = b["info"]["untouched"]
        buf = b["bufs"]["dmods"]
        untouched = bool(torch.equal(_bits(outs["dmods"][buf.top:buf.top + buf.rows][rows]), _bits(buf.alloc[buf.top:buf.top + buf.rows][rows])))
    for ch in b["checks"]:
        got = _got(b, ch, outs, rets)
        if ch.kind == "bits":
            same = same_bits(got.reshape(ch.ref.shape), ch.ref)
            bits_ok &= same
            lines.append((ch.tag + " (bits)", 0.0 if same else math.inf, 0.0))
        elif ch.kind == "planes":
            lines.append((ch.tag + " (hi + lo against float64)", planes_error(ch, got[0], got[1], c.group), 1.0))
            if ch.x32.startswith("twin:"):
                x32 = _data_of(built(twin_of(c)), ch.x32[5:], twin_outs[ch.x32[5:]])
            else:
                x32 = _data_of(b, ch.x32, outs[ch.x32])
            e1, e2 = planes_contract(ch, x32, got[0], got[1])
            lines.append((ch.tag + " (contract: hi + lo)", e1, 1.0))
            lines.append((ch.tag + " (contract: hi nearest)", e2, 1.0))
            if ch.skip is not None:
                sk = ch.skip.reshape(ch.ref.shape)
                want = torch.full((int(sk.sum()),), SENTINEL_F16, dtype=f16)
                same = all(same_bits(t.reshape(ch.ref.shape)[sk], want) for t in got)
                bits_ok &= same
                lines.append((ch.tag + " (skipped: sentinel bits)", 0.0 if same else math.inf, 0.0))
        else:
            lines.append((ch.tag, units_error(ch, got), k))
            if ch.unit_x is not None:
                lines.append((ch.tag + " (xhat unit)", units_error(ch, got, True), KX[c.group]))
    ok = guards and untouched and bits_ok and all(e <= bnd for _, e, bnd in lines)
    return dict(case=c.name, entry=c.entry, lines=lines, guards_ok=guards, untouched_ok=untouched, bits_ok=bits_ok, ok=ok)


def worst_line(rep: dict):
    """(fraction of the bound, tag, error in units) of the worst output compared with float64.  The lines of the plane contract have
    an allowance of their own (the split's, not the table's): asserted, and shown apart by describe(), unless one of them fails"""
    return max(((e / bnd if bnd else e), tag, e) for tag, e, bnd in rep["lines"] if not ("(contract: " in tag and e <= bnd))


def describe(rep: dict, flags: Optional[dict] = None) -> str:
    worst = worst_line(rep)
    out = (f"rowops {rep['case']:<44} {rep['entry']:<30} worst {worst[2]:9.3e} units ({worst[1]}) = {worst[0]:9.3e} of the bound, "
           f"guards {'intact' if rep['guards_ok'] else 'WRITTEN'}, untouched rows {'kept' if rep['untouched_ok'] else 'WRITTEN'}")
    con = [(tag, e) for tag, e, _ in rep["lines"] if "(contract: " in tag]
    if con:     # (hi nearest: the largest |value - hi| over half an fp16 ulp tends to 1 by construction)
        out += (f", plane contract hi + lo {max(e for t, e in con if t.endswith('hi + lo)')):.3f}, "
                f"hi nearest {max(e for t, e in con if t.endswith('hi nearest)')):.3f} (each at most 1)")
    if flags:
        out += "".join(f", {k} {v}" for k, v in flags.items() if v is not None)
    return out + ("" if rep["ok"] else "  NOT OK")


# ------------------------------------------------------------------------------------------------------------ GPU runs
class _Dev:
    """the case's allocations on the device, and views of their data as the wrappers want them"""

    def __init__(self, c: Case, dev):
        self.b = built(c)
        self.dev = dev
        self.t = {k: v.alloc.to(dev) for k, v in self.b["bufs"].items()}

    def buf(self, k):
        return self.b["bufs"][k]

    def has(self, k):
        return k in self.t

    def rows(self, k):
        """[rows, ld] from the first data row on (contiguous; the data starts at column 0)"""
        bf = self.buf(k)
        assert bf.left == 0
        return self.t[k][bf.top:bf.top + bf.rows]

    def flat(self, k):
        bf = self.buf(k)
        return self.t[k].view(-1)[bf.off:bf.off + bf.cols]

    def get(self, k, how="flat"):
        if not self.has(k):
            return None
        return self.flat(k) if how == "flat" else self.rows(k)

    def outs(self):
        return {k: v.cpu() for k, v in self.t.items()}


def _ln_kwargs(c, d):
    form = c.o("form")
    if form == "affine":
        return dict(gamma=d.flat("gamma"), beta=d.flat("beta"))
    if form == "mod":
        return dict(mod=d.rows("mod"), rows_per_batch=c.o("rpb"), ld_mod=d.buf("mod").ld)
    if form == "grp":
        return dict(mod=d.rows("mod"), group_batch=d.flat("gb"), group_rows=c.o("gr"), ld_mod=d.buf("mod").ld)
    return {}


def run_ln(c, d):
    from pfpp_hip import ops
    out = ops.SplitAct(d.rows("out_hi"), d.rows("out_lo")) if c.o("split") else d.rows("out")
    kw = _ln_kwargs(c, d)
    if c.o("form") == "grp":
        ops.layernorm_grouped(d.rows("x"), kw["mod"], kw["group_batch"], kw["group_rows"], out=out, ld_mod=kw["ld_mod"])
    else:
        ops.layernorm(d.rows("x"), out=out, **kw)
    return {}


def run_dln(c, d):
    from pfpp_hip import train_ops as T
    kw = _ln_kwargs(c, d)
    res = d.get("res", "rows")
    if c.o("planes"):
        from pfpp_hip import planes as P
        T.dropout_layernorm_planes(d.rows("y"), res, c.o("p"), c.o("seed"), c.o("site"), n_out=P.Planes(d.rows("n_hi"), d.rows("n_lo")), **kw)
        return {}
    T.dropout_layernorm(d.rows("y"), res, c.o("p"), c.o("seed"), c.o("site"), n_out=d.rows("n"), **kw)
    return {}


def run_lnb(c, d):
    from pfpp_hip import train_ops as T
    form, C = c.o("form"), c.o("C")
    kw = dict(group_rows=c.o("gr"))
    if form in ("grp", "uni"):
        kw["mod"] = d.rows("mod")
        if form == "grp":
            kw["group_batch"] = d.flat("gb")
        else:
            kw["rows_per_batch"] = 2 * c.o("gr")
    elif form == "gamma":
        kw["gamma"] = d.flat("gamma")
    if d.has("dmods"):
        dm = d.rows("dmods")
        kw.update(dmult=dm[:, :C], dadd=dm[:, C:], ld_d=d.buf("dmods").ld if form != "gamma" else 0)
    drop = c.o("drop")
    if c.o("planes"):
        from pfpp_hip import planes as P
        sc = d.b["info"]["scale"]
        T.layernorm_bwd_planes(d.rows("x"), d.rows("dy"), d.rows("dx"), sc, drop=drop, want_ret=True, want_dx=True,
                               ret_fp32=drop is not None, ret_out=P.Planes(d.rows("ret_hi"), d.rows("ret_lo"), sc),
                               dx_out=P.Planes(d.rows("dx_hi"), d.rows("dx_lo"), sc), drop_out=d.get("drop", "rows"), **kw)
        return {}
    T.layernorm_bwd(d.rows("x"), d.rows("dy"), d.rows("dx"), drop=drop, drop_out=d.get("drop", "rows"), **kw)
    return {}


def run_colsum(c, d):
    from pfpp_hip import train_ops as T
    xb, ob = d.buf("x"), d.buf("out")
    T.colsum(d.t["x"], d.t["out"], rows=c.o("rows"), cols=c.o("cols"), ld=xb.ld, batch=c.o("batch"), sx=d.b["info"]["R"] * xb.ld, so=ob.ld,
             accumulate=c.o("acc"), x_off=xb.off, o_off=ob.off)
    return {}


def run_colsum_planes(c, d):
    from pfpp_hip import planes as P
    P.colsum(P.Planes(d.rows("hi"), d.rows("lo"), d.b["info"]["scale"]), d.flat("out"), cols=c.o("cols"))
    return {}


def run_split(c, d):
    from pfpp_hip import planes as P
    P.split(d.flat("x"), c.o("scale"), out=P.Planes(d.flat("hi"), d.flat("lo"), c.o("scale")))
    return {}


def run_geglu(c, d):
    from pfpp_hip import planes as P, train_ops as T
    a = (c.o("p"), c.o("seed"), c.o("site"))
    sc = d.b["info"]["scale"]
    if c.kind == "geglu":
        if c.o("planes"):
            T.geglu_planes(d.rows("z"), *a, out=P.Planes(d.rows("out_hi"), d.rows("out_lo"), sc))
        else:
            T.geglu(d.rows("z"), *a, out=d.rows("out"))
    else:
        if c.o("planes"):
            T.geglu_bwd_planes(d.rows("z"), d.rows("du"), *a, sc, out=P.Planes(d.rows("out_hi"), d.rows("out_lo"), sc))
        else:
            T.geglu_bwd(d.rows("z"), d.rows("du"), *a, out=d.rows("out"))
    return {}


def run_act(c, d):
    from pfpp_hip import train_ops as T
    if c.o("bwd"):
        T.act_bwd(d.flat("pre"), d.flat("dy"), c.o("act"), out=d.flat("out"))
    else:
        T.act(d.flat("pre"), c.o("act"), out=d.flat("out"))
    return {}


def run_dropout(c, d):
    from pfpp_hip import train_ops as T
    T.dropout(d.flat("x"), c.o("p"), c.o("seed"), c.o("site"), res=d.get("res"), out=d.flat("out"))
    return {}


def run_dropout_mask(c, d):
    from pfpp_hip import train_ops as T
    T.dropout_mask(c.o("n"), c.o("p"), c.o("seed"), c.o("site"), d.dev, out=d.flat("keep"))
    return {}


def run_bn_stats(c, d):
    from pfpp_hip import train_ops as T
    T.bn_stats(d.rows("x"), d.get("rmean"), d.get("rvar"), 0.1, cols=c.o("C"), out=(d.flat("mean"), d.flat("var")))
    return {}


def run_bn_apply(c, d):
    from pfpp_hip import train_ops as T
    T.bn_apply(d.rows("x"), d.flat("mean"), d.flat("var"), d.flat("gamma"), d.flat("beta"), EPS, c.o("pool"), cols=c.o("C"),
               out=d.rows("out"), ldy=d.buf("out").ld)
    return {}


def run_bn_finalize(c, d):
    from pfpp_hip import train_ops as T
    st = d.rows("stats").view(c.o("copies"), 2, c.o("C"))
    T.bn_finalize(st, c.o("rows"), d.flat("gamma"), d.flat("beta"), d.get("rmean"), d.get("rvar"), 0.1, EPS, want_stats=True,
                  out=(d.flat("a_mul"), d.flat("a_add"), d.flat("mean"), d.flat("var")))
    return {}


def run_bn_minmax(c, d):
    from pfpp_hip import train_ops as T
    T.bn_minmax_apply(d.rows("mx"), d.rows("mn"), d.flat("a"), d.flat("b"), out=d.rows("out"))
    return {}


def run_softmax(c, d):
    from pfpp_hip import ops
    ops.softmax_rows(d.rows("S"), d.get("kv", "rows"), c.o("rpb"), c.o("T"), d.b["info"]["scale"])
    return {}


def run_mean_pool(c, d):
    from pfpp_hip import ops, train_ops as T
    if c.o("bwd"):
        T.mean_pool_bwd(d.rows("dp"), c.o("L"), out=d.rows("out"))
    else:
        ops.mean_pool(d.rows("x"), c.o("n"), c.o("L"), out=d.rows("out"))
    return {}


def run_mse(c, d):
    from pfpp_hip import train_ops as T
    o = dict(loss_out=d.flat("loss"), dpred_out=d.rows("dpred"))
    if c.o("masked"):
        T.mse_loss_masked(d.rows("pred"), d.rows("target"), d.flat("valid"), d.flat("ref"), c.o("grad_out"), amax=d.flat("amax"), **o)
    else:
        T.mse_loss(d.rows("pred"), d.rows("target"), d.flat("sel"), c.o("grad_out"), **o)
    return {}


def run_adamw(c, d):
    from pfpp_hip import _lib, ops, train_ops as T
    h = ADAM
    ovf = torch.zeros(2, dtype=torch.int32, device=d.dev) if c.o("guarded") else None
    for t in range(1, ADAM_STEPS + 1):
        g = d.flat(f"g{t - 1}")
        if c.o("direct"):                                              # pfpp_adamw has no wrapper of its own: the handle train_ops.adamw uses
            _lib.check(_lib.load().pfpp_adamw(ops._ptr(d.flat("p")), ops._ptr(g), ops._ptr(d.flat("m")), ops._ptr(d.flat("v")),
                                              ops._ptr(d.get("hi")), ops._ptr(d.get("lo")), c.o("n"), h["lr"], h["beta1"], h["beta2"],
                                              h["eps"], h["weight_decay"], 1.0 - h["beta1"] ** t, 1.0 - h["beta2"] ** t, c.o("g_scale"),
                                              ops._stream()), "pfpp_adamw")
        else:
            T.adamw(d.flat("p"), g, d.flat("m"), d.flat("v"), step=t, hi=d.get("hi"), lo=d.get("lo"), g_scale=c.o("g_scale"),
                    zero_grad=c.o("zero_grad"), overflow=ovf, **h)
    return dict(overflow=ovf) if ovf is not None else {}


_RUNNERS = dict(ln=run_ln, dln=run_dln, lnb=run_lnb, colsum=run_colsum, colsum_planes=run_colsum_planes, split=run_split, geglu=run_geglu,
                geglu_bwd=run_geglu, act=run_act, dropout=run_dropout, dropout_mask=run_dropout_mask, bn_stats=run_bn_stats,
                bn_apply=run_bn_apply, bn_finalize=run_bn_finalize, bn_minmax=run_bn_minmax, softmax=run_softmax, mean_pool=run_mean_pool,
                mse=run_mse, adamw=run_adamw)


def _launch(c: Case, dev):
    d = _Dev(c, dev)
    rets = _RUNNERS[c.kind](c, d)
    torch.cuda.synchronize()
    return d, d.outs(), {k: v.cpu() for k, v in rets.items()}


def _twin_flags(c: Case, dev, d, outs, rets):
    """the bit-identities that need a second, different launch"""
    from pfpp_hip import train_ops as T
    flags = {}
    b = d.b
    if c.kind == "mse":
        if c.o("masked"):
            sel = b["info"]["sel"].to(torch.uint8).to(dev)
            loss, dpred = T.mse_loss(d.rows("pred"), d.rows("target"), sel, c.o("grad_out"))
            torch.cuda.synchronize()
            got_l, got_d, got_a = (_data_of(b, k, outs[k]) for k in ("loss", "dpred", "amax"))
            flags["same_bits_as_sel"] = bool(torch.equal(_bits(loss.cpu()), _bits(got_l.reshape(1)))) and bool(torch.equal(_bits(dpred.cpu()), _bits(got_d)))
            flags["amax_bits"] = bool(torch.equal(_bits(got_a.reshape(1)), _bits(got_d.abs().max().reshape(1))))
    elif c.kind == "adamw" and c.o("guarded"):
        # the unguarded run on the same inputs with the non-finite gradients replaced by 0: every other element has the same bits
        d2 = _Dev(c, dev)
        for t in range(ADAM_STEPS):
            g = d2.flat(f"g{t}")
            g[list(b["info"]["bad"])] = 0.0
        for t in range(1, ADAM_STEPS + 1):
            T.adamw(d2.flat("p"), d2.flat(f"g{t - 1}"), d2.flat("m"), d2.flat("v"), step=t, hi=d2.get("hi"), lo=d2.get("lo"),
                    g_scale=c.o("g_scale"), zero_grad=c.o("zero_grad"), overflow=None, **ADAM)
        torch.cuda.synchronize()
        ok = b["info"]["ok"]
        bad = ~ok
        same, kept = True, True
        for k in ("p", "m", "v"):
            buf = b["bufs"][k]
            a1, a2 = outs[k][buf.top, buf.left:buf.left + buf.cols], d2.flat(k).cpu()
            same &= bool(torch.equal(_bits(a1[ok]), _bits(a2[ok])))
            kept &= bool(torch.equal(_bits(a1[bad]), _bits(buf.view[0][bad])))
        flags["same_bits_as_unguarded"], flags["skipped_kept"] = same, kept
    elif c.kind == "lnb" and c.o("drop") is not None:
        # the dropped-out gradient is the returned dx times 1 / (1 - p) under the mask, in float32
        dx = _data_of(b, "dx", outs["dx"])
        want = torch.where(b["info"]["keep"], dx * inv_keep32(b["info"]["p"]), torch.zeros((), dtype=f32))
        flags["drop_bits"] = bool(torch.equal(_bits(_data_of(b, "drop", outs["drop"])), _bits(want)))
    if c.kind == "softmax":
        buf = b["bufs"]["S"]
        p = outs["S"][buf.top:buf.top + buf.rows, :c.o("T")].double()
        live = b["info"]["live"]
        flags["row_sums"] = bool(((p.sum(-1) - 1.0).abs()[live] <= 64 * U).all()) and bool((p[~live] == 0).all())
    return flags


def run(c: Case, dev):
    """-> (report of evaluate(), flags: the bit-identities of a second launch; every value must be True or None)"""
    d, outs, rets = _launch(c, dev)
    twin_outs = _launch(twin_of(c), dev)[1] if needs_twin(c) else None
    rep = evaluate(c, outs, rets, twin_outs)
    flags = _twin_flags(c, dev, d, outs, rets)
    if c.group in REPEATABLE:
        _, outs2, rets2 = _launch(c, dev)
        atomic = {ch.out.partition(":")[0] for ch in built(c)["checks"] if ch.atomic and isinstance(ch.out, str)}
        same = all(torch.equal(_bits(outs[k]), _bits(outs2[k])) for k in outs if k not in atomic)
        same &= all(torch.equal(_bits(rets[k]), _bits(rets2[k])) for k in rets)
        flags["repeat_bits"] = bool(same)
    return rep, flags


def flags_ok(flags: dict) -> bool:
    return all(v is not False for v in flags.values())


def yardstick_main() -> int:
    worst = {}
    for name, c in CASES.items():
        for tag, e in yardstick(c):
            if e > worst.get(c.group, (0.0,))[0]:
                worst[c.group] = (e, name, tag)
    for g, (e, name, tag) in worst.items():
        p2 = 2.0 ** math.ceil(math.log2(e)) if e > 0 else 1.0
        print(f"group {g}: yardstick max {e:.3f} units ({name}, {tag}) -> K = {YARD_SPARE * max(p2, 1.0):g}; table has {K[g]:g}")
    for g in KX:
        e, name = max((e, n) for n in GROUPS[g] for _, e in yardstick(CASES[n], True))
        print(f"group {g}: yardstick max {e:.3f} xhat units ({name}) -> KX = {YARD_SPARE * 2.0 ** math.ceil(math.log2(e)):g}; table has {KX[g]:g}")
    return 0


def bn_apply_sweep(dev):
    """not a case: the absolute error of pfpp_bn_apply's folded affine (a = gamma rstd, b = beta - mean a) over |mean| / sigma, for the
    paragraph of DESIGN.md that says where its 1e-5 absolute bound holds"""
    from pfpp_hip import train_ops as T
    ratios = (0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1000)
    g = torch.Generator().manual_seed(5)
    rows, C = 4096, 96
    x = torch.randn(rows, C, generator=g) + torch.tensor([float(ratios[c % 12]) for c in range(C)])
    x64 = x.double()
    mean, var = x64.mean(0).float(), ((x64 - x64.mean(0)) ** 2).mean(0).float()
    gamma, beta = torch.ones(C), torch.full((C,), 0.5)
    ref = torch.relu((x64 - mean.double()) * (gamma.double() / torch.sqrt(var.double() + EPS)) + beta.double())
    got = T.bn_apply(x.to(dev), mean.to(dev), var.to(dev), gamma.to(dev), beta.to(dev), EPS).cpu().double()
    a32 = gamma * (1.0 / torch.sqrt(var + EPS))
    cpu = torch.relu(x * a32 + (beta - mean * a32)).double()
    d, dc = (got - ref).abs(), (cpu - ref).abs()
    for k, r in enumerate(ratios):
        print(f"rowops bn_apply folded affine, |mean|/sigma {r:>4}: max abs error {float(d[:, k::12].max()):.2e} on the GPU, "
              f"{float(dc[:, k::12].max()):.2e} float32 on the CPU (outputs up to {float(ref[:, k::12].max()):.1f})", flush=True)


def report_main() -> int:
    sys.path[:0] = [str(ROOT), str(ROOT / "puzzlefusion-plusplus_amd")]
    from pfpp_hip._lib import PfppError
    dev = torch.device("cuda:0")
    bad = 0
    worst = {}
    for name, c in CASES.items():
        try:
            rep, flags = run(c, dev)
        except (ValueError, TypeError, PfppError) as e:               # a call the wrapper or the entry point rejects is a line of the record too
            print(f"rowops {name:<44} ERROR {type(e).__name__}: {str(e)[:200]}", flush=True)
            bad += 1
            continue
        except Exception as e:                                       # anything else (a HIP error): nothing more is launched
            print(f"rowops {name:<44} STOPPED {type(e).__name__}: {str(e)[:200]}", flush=True)
            return 2
        print(describe(rep, flags), flush=True)
        frac = worst_line(rep)[0]
        worst[c.group] = max(worst.get(c.group, 0.0), frac)
        bad += not rep["ok"] or not flags_ok(flags)
    for g, f in worst.items():
        print(f"rowops group {g}: worst fraction of the bound {f:.3f} (K = {K[g]:g} units" + (f", KX = {KX[g]:g}" if g in KX else "") + ")")
    bn_apply_sweep(dev)
    print(f"rowops {len(CASES)} cases, {bad} not ok", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    if "--report" in sys.argv:
        sys.exit(report_main())
    if "--yardstick" in sys.argv:
        sys.exit(yardstick_main())
    print(f"{len(CASES)} cases: " + ", ".join(f"{g} {len(v)}" for g, v in GROUPS.items()))
