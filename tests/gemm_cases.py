"""Case table, float64 reference and error report of the GEMM edge tests (no test in here; importable without a GPU).
tests/test_gemm_cases_host.py checks the table itself on the CPU, tests/test_gpu_gemm_edges.py runs it through the HIP kernels, and
`python tests/gemm_cases.py --report` prints case, kernel, band and error, one line each (profiles/gemm_edges_errors.txt).

One case is ONE launch through a Python wrapper of the GEMM family (csrc/gemm.hip, gemm_pl.hip, gemm_grad.hip, gemm_wd.hip,
gemm_small.hip): ops.gemm, planes.gemm, planes.dw_group, train_ops.gemm_grad / grad_weight_group, ops.gemm_wd / planes.gemm_wd,
ops.gemm_small.  Groups: A pfpp_gemm_planes (forced variants x forms nt / nn / tn), B pfpp_gemm with a pre-split A, C pfpp_gemm's
register-staged, fp32-MFMA, fp32-A plane, split-K and fused-grouping launches, D pfpp_gemm batched, E pfpp_gemm_grad(_group),
F pfpp_gemm_dw_group, G pfpp_gemm_wd / pfpp_gemm_small.  K is 32 unless the case is about K.
Where two entry points accept the same call, a second launch through the other one into a twin allocation must give the same bits:
pfpp_gemm_planes (nt, non-accumulating, no K split) against pfpp_gemm in groups A and B (planes_twin: all but GEGLU and plane
output), pfpp_gemm_wd against the tiled plane GEMM in group G.

Buffers.  Every operand and every output lives in a taller and wider allocation of its own; the launch gets a pointer into it
(element offsets / row or column slices) and the allocation's row length as the leading dimension.
  * outputs: >= 8 guard columns on either side (ldc > N) and 2 guard rows above and below, pre-filled with SENTINEL (-1234.5625,
    exactly representable; -1234 in fp16 output planes); after the launch every guard element must still hold those bits;
  * operands: guard rows and columns of NaN (fp32 NaN, fp16 NaN in planes), which includes the K .. lda pad of a row-major fp32
    operand and the rows after row K of a k-major one ("rows beyond K are never read");
  * guards are part of the same torch allocation as the data: a wrong kernel fails the test, it does not leave the process's memory.
Contract pads (stay as the ABI wants them, they are NOT guards): the ldw pad of a pre-split weight (packing.PW: K rounded up to 8,
zero filled); pfpp_gemm_dw_group has no leading dimensions at all (lda = M, ldw = ldc = N), so its operands carry guard rows only;
the A operand of the fused grouping has lda = D.

Reference: act(alpha * A.W + bias or scale/shift) + residual in float64, or C0 + alpha * A.W with accumulate, from the values the
operands stand for: (hi + lo) / scale for planes, the fp32 values for fp32 operands (a packed weight stands for its fp32 tensor),
hi / scale alone in the single-pass fp16 mode.  Pooling is the row-group max (min for c_min), GEGLU value * gelu(gate) on the
unpacked weight.

Error, per band.  The result is split at the launched tile's last full row boundary (M // BM * BM) and last full column boundary
into interior, right strip, bottom strip and corner; BM x BN comes from the kernel name the launch reports.  Per band:
max |got - ref| / max |ref| over the band <= BAND_BOUND = 2e-5 (the project's forward bound, without max(1, .)): dropping one of
the three split-f16 products costs 2^-11 = 5e-4, a missing 32-deep K tile of 3,850 about 9 %; rounding stays below 2.3e-6 (float64
emulation of the three-product arithmetic on a 1 x 8 corner at K = 3,850).  Over the whole matrix the entry point's own bound holds
as well, against the global max |ref|: 2e-5 forward, 2e-6 plane dX / dW, grad_input, gemm_wd and gemm_small, 5e-6 pfpp_gemm_grad.
The float32 CPU evaluation of the same formula (the yardstick) has to pass the band bounds with a factor 8 to spare: the bounds
are not set by the inputs."""
from __future__ import annotations

import math
import sys
import zlib
from dataclasses import dataclass
from functools import lru_cache
from pathlib import Path
from typing import Tuple

import torch

SENTINEL = -1234.5625
SENTINEL_F16 = -1234.0
BAND_BOUND = 2e-5
YARD_SPARE = 8.0
WHOLE_FWD, WHOLE_PLANE_GRAD, WHOLE_GRAD = 2e-5, 2e-6, 5e-6
NAN = float("nan")
TOP = 2                    # guard rows above and below an output
GCOL = 8                   # guard columns left and right of an output
KTAIL = 40                 # NaN rows after row K of a k-major operand (more than one 32-deep K tile)
_TAIL_FILL = [NAN]         # what those rows hold (built_with_tail swaps it: no reference may depend on it)


@dataclass(frozen=True)
class Case:
    name: str
    group: str             # A .. G
    entry: str             # planes | gemm | grad | grad_group | dw_group | wd | small
    M: int = 0
    N: int = 0
    K: int = 32
    form: str = "nt"       # nt: A [M,K] W [N,K]; nn: W [K,N]; tn: A [K,M] W [K,N]
    jobs: Tuple = ()       # grouped launches: ((M, N, K), ...)
    opts: Tuple = ()       # sorted (key, value) pairs

    def o(self, key, default=None):
        return dict(self.opts).get(key, default)


def _case(name, group, entry, M=0, N=0, K=32, form="nt", jobs=(), **opts):
    return Case(name, group, entry, M, N, K, form, tuple(jobs), tuple(sorted(opts.items())))


# ------------------------------------------------------------------------------------------------------------ the table
PL_TILE = {"nt": {1: (256, 256), 2: (256, 128), 3: (128, 128), 6: (128, 64), 11: (64, 32)},
           "nn": {1: (256, 128), 2: (256, 128), 3: (128, 128), 6: (128, 64), 11: (128, 64)},
           "tn": {1: (256, 128), 2: (256, 128), 3: (128, 128), 6: (128, 64), 11: (128, 64)}}
PL_VARIANTS = (1, 2, 3, 6, 11)


def _table_a():
    t = []
    for form in ("nt", "nn", "tn"):
        for v in PL_VARIANTS:
            bm, bn = PL_TILE[form][v]
            dm = 8 if form == "tn" else 1                        # k-major A: M % 8 == 0
            dn = 1 if form == "nt" else 8                        # k-major W: N % 8 == 0
            ks = (1, 33, 97) if form == "tn" else (32, 96, 32)
            for i, s in enumerate((-1, 0, 1)):
                # the nt form takes any N: one side of the tile at +-1, the other at +-8 (a float4-wide store at N % 4 != 0)
                n = bn + s * (8 if (form == "nt" and v in (2, 6)) else dn)
                t.append(_case(f"A_{form}_v{v}_{'m0p'[i]}", "A", "planes", bm + s * dm, n, ks[i], form, variant=v, splits=1))
    t.append(_case("A_tn_v3_k31", "A", "planes", 136, 120, 31, "tn", variant=3, splits=1, colsum=True, accumulate=True))
    for form in ("nt", "nn", "tn"):                              # K splits at K = 352 (11 K-tiles: chunks of 4, 4, 3)
        k = 352
        t.append(_case(f"A_{form}_split3_ws", "A", "planes", 136, 136, k, form, variant=3, splits=3))
        t.append(_case(f"A_{form}_split3_ws_acc", "A", "planes", 136, 136, k, form, variant=3, splits=3, accumulate=True))
        t.append(_case(f"A_{form}_split3_atomic", "A", "planes", 136, 136, k, form, variant=3, splits=3, accumulate=True, use_ws=False))
        t.append(_case(f"A_{form}_split1_acc", "A", "planes", 136, 136, k, form, variant=3, splits=1, accumulate=True))
    for v in (2, 3, 6):
        t.append(_case(f"A_tn_v{v}_colsum", "A", "planes", 264, 136, 97, "tn", variant=v, splits=1, colsum=True, accumulate=True))
    t.append(_case("A_tn_colsum_split3_ws", "A", "planes", 136, 136, 352, "tn", variant=3, splits=3, colsum=True, accumulate=True))
    t.append(_case("A_tn_colsum_split3_atomic", "A", "planes", 136, 136, 352, "tn", variant=3, splits=3, colsum=True, accumulate=True,
                   use_ws=False))
    t.append(_case("A_tn_colsum_split3_ws_k353", "A", "planes", 136, 136, 353, "tn", variant=3, splits=3, colsum=True, accumulate=True))
    for form in ("nt", "nn", "tn"):
        t.append(_case(f"A_{form}_alpha", "A", "planes", 136, 72, 96, form, variant=6, splits=1, alpha=0.37))
        t.append(_case(f"A_{form}_bias_res", "A", "planes", 136, 72, 96, form, variant=6, splits=1, bias=True, residual=True))
    for act in ("relu", "silu", "gelu"):
        t.append(_case(f"A_nt_{act}", "A", "planes", 129, 136, 32, "nt", variant=3, splits=1, act=act, bias=True))
    for v in (1, 2, 3, 6):
        bm, bn = PL_TILE["nt"][v]
        t.append(_case(f"A_nt_x1_v{v}", "A", "planes", bm + 1, bn + 8, 96, "nt", variant=v, splits=1, single_pass=True))
    return t


def _table_b():
    t = []
    for m0 in (256, 3840, 16384):                                # 200, 3850 and 16385 rows' tiles: 256 is a multiple of every BM, BN
        for i, s in enumerate((-1, 0, 1)):
            t.append(_case(f"B_m{m0}_{'m0p'[i]}", "B", "gemm", m0 + s, 256 + 8 * s, 32, a="planes", w="pw"))
    for i, s in enumerate((-1, 0, 1)):                           # above 16,384 rows the tile-count rule picks 256 x 128 from 160 such tiles on
        t.append(_case(f"B_m16640_{'m0p'[i]}", "B", "gemm", 16640 + s, 384 + 8 * s, 32, a="planes", w="pw"))
    t.append(_case("B_200", "B", "gemm", 200, 520, 32, a="planes", w="pw", bias=True))
    t.append(_case("B_3850", "B", "gemm", 3850, 520, 32, a="planes", w="pw", bias=True, residual=True))
    t.append(_case("B_16385", "B", "gemm", 16385, 520, 32, a="planes", w="pw", alpha=0.37))
    t.append(_case("B_planes_out", "B", "gemm", 257, 264, 32, a="planes", w="pw", out_planes=True, bias=True))
    t.append(_case("B_planes_out_3850", "B", "gemm", 3850, 520, 32, a="planes", w="pw", out_planes=True))
    for n in (128, 192):
        t.append(_case(f"B_geglu_n{n}", "B", "gemm", 257, n, 32, a="planes", w="pw", act="geglu", bias=True))
    t.append(_case("B_geglu_planes_out", "B", "gemm", 129, 192, 32, a="planes", w="pw", act="geglu", bias=True, out_planes=True))
    t.append(_case("B_x1", "B", "gemm", 257, 264, 96, a="planes", w="pw", single_pass=True, bias=True))
    return t


def _table_c():
    t = []
    g = lambda name, M, N, K=32, **o: t.append(_case("C_" + name, "C", "gemm", M, N, K, a="f32", **o))
    g("pre256x256", 8193, 1032, w="pw", bias=True)
    g("pre256x256_m", 8447, 1024, w="pw")
    g("pre256x128pf2", 8193, 136, w="pw", act="relu", bn=True)
    g("pre256x128pf2_m", 8447, 120, w="pw")
    g("pre256x128pf2_aff", 8193, 136, w="pw", affine=True)
    for m in (1, 63, 65):
        g(f"deep64x64_m{m}", m, 72, w="pw", bias=True)
        g(f"deep64x128_geglu_m{m}", m, 192, w="pw", act="geglu", bias=True)
    g("deep64x64_k96", 65, 56, 96, w="pw", act="gelu", bias=True)
    g("pre128x64pf2_1008_tiles", 8000, 1930, w="pw")
    g("pre128x128pf2_1024_tiles", 8100, 1930, w="pw", bias=True)
    g("pre128x128_2048_tiles", 8100, 3970, w="pw")
    g("pre128x128pf2_pool64", 192, 136, w="pw", pool=64, act="relu", bn=True)
    g("pre128x64pf2_pool32", 2080, 56, w="pw", pool=32, act="relu", bn=True)
    g("pre128x64_stats", 4097, 136, 64, w="pw", stats=True, bias=True)
    g("pre128x128_stats_pool64", 4160, 136, 64, w="pw", stats=True, pool=64, c_min=True, bias=True)
    for k in (7, 33, 132):
        g(f"plain128x128_k{k}", 129, 136, k, w="f32", act="relu", bn=True)
        g(f"plain128x64_k{k}", 127, 56, k, w="f32", bias=True)
    g("plain128x64_n3", 129, 3, 33, w="f32")
    g("f32_128x128", 129, 136, w="f32", mode="f32", bias=True, residual=True)
    g("f32_128x64", 127, 56, 36, w="f32", mode="f32", act="silu", bias=True)
    g("f32k_128x128", 129, 136, w="kmajor", mode="f32", alpha=0.37)
    g("f32k_128x64", 127, 56, 36, w="kmajor", mode="f32", bias=True)
    g("af32_n72", 65537, 72, w="pw", bias=True)
    g("af32_n56", 65537, 56, w="pw", act="relu", bn=True)
    g("af32_n136_affine_stats", 65537, 136, 64, w="pw", affine=True, stats=True, bias=True)
    g("af32_pool32_cmin", 65568, 136, 64, w="pw", pool=32, c_min=True, stats=True, bias=True)
    g("split_k_ws", 125, 520, 2048, w="pw", bias=True, residual=True)
    g("split_k_no_ws", 125, 520, 2048, w="pw", bias=True, residual=True, lend_ws=False)
    for d in (0, 32):
        g(f"gather_d{d}", 192, 72, d + 4, w="pw", gather=d, bias=True, act="relu")
    return t


def _table_d():
    t = []
    for m in (7, 33):
        t.append(_case(f"D_f16x3_m{m}", "D", "gemm", m, 72, 36, a="f32", w="f32", batch=6, zdiv=2, bias=True, alpha=0.37))
        t.append(_case(f"D_f32k_m{m}", "D", "gemm", m, 72, 36, a="f32", w="kmajor", mode="f32", batch=6, zdiv=2, bias=True, alpha=0.37))
    return t


def _table_e():
    t = []
    g = lambda name, M, N, K, form, **o: t.append(_case("E_" + name, "E", "grad", M, N, K, form, **o))
    # nt: 128 x 64 (split_k = 1), 128 x 128 (split_k = 0, N > 64); nn: 128 x 64, 256 x 128 (>= 384 such tiles);
    # tn: 128 x 128 (split_k = 0 without accumulate), 128 x 64 (accumulate, < 40 tiles)
    for i, s in enumerate((-4, 4)):
        sg = "mp"[i]
        g(f"nt_128x64_{sg}", 128 + s, 64 + s, (31, 148)[i], "nt", split_k=1)
        g(f"nt_128x128_{sg}", 128 + s, 128 + s, (1, 353)[i], "nt", split_k=0)
        g(f"nn_128x64_{sg}", 128 + s, 64 + s, (148, 31)[i], "nn", split_k=1)
        g(f"tn_128x128_{sg}", 128 + s, 128 + s, (353, 1)[i], "tn", split_k=0)
        g(f"tn_128x64_{sg}", 128 + s, 64 + s, (31, 148)[i], "tn", split_k=1, accumulate=True)
    g("nn_256x128_m", 384 * 256 - 4, 124, 32, "nn", split_k=1)
    g("nn_256x128_p", 192 * 256 - 252, 132, 32, "nn", split_k=1)
    for sk in (0, 1, 3):
        g(f"tn_split{sk}_acc", 132, 132, 353, "tn", split_k=sk, accumulate=True)
        g(f"nn_split{sk}_acc", 132, 132, 353, "nn", split_k=sk, accumulate=True)
    g("nt_split3_acc", 132, 132, 353, "nt", split_k=3, accumulate=True)
    g("tn_colsum", 132, 68, 148, "tn", split_k=1, accumulate=True, colsum=True)
    g("tn_colsum_split3", 132, 132, 353, "tn", split_k=3, accumulate=True, colsum=True)
    g("nn_scales", 132, 68, 148, "nn", split_k=1, a_scale=4096.0, w_scale=0.25, alpha=0.37)
    g("tn_scales", 132, 132, 353, "tn", split_k=0, a_scale=4096.0, w_scale=4.0)
    t.append(_case("E_group", "E", "grad_group", jobs=((4, 260, 353), (8, 8, 31), (132, 124, 148), (124, 132, 1), (260, 4, 353),
                                                      (128, 128, 32), (68, 260, 97), (256, 132, 353))))
    return t


def _table_f():
    t = []
    jobs = ((8, 8), (72, 136), (264, 120), (136, 264))
    for v, k in zip((0, 3, 6, 7), (385, 97, 33, 1)):
        t.append(_case(f"F_v{v}_k{k}", "F", "dw_group", K=k, jobs=jobs, variant=v))
    t.append(_case("F_v3_k385", "F", "dw_group", K=385, jobs=jobs, variant=3))
    t.append(_case("F_v6_k97", "F", "dw_group", K=97, jobs=jobs, variant=6))
    return t


def _table_g():
    t = []
    for m in (1, 31, 33, 127, 129):
        t.append(_case(f"G_wd_m{m}", "G", "wd", m, 128, 32, kind="wd", bias=True, residual=True))
        t.append(_case(f"G_small_m{m}", "G", "small", m, 32, 512, bias=True, residual=True))
    t.append(_case("G_wd_plain", "G", "wd", 65, 256, 64, kind="wd"))
    # the 128 x 256 tile (N % 256 == 0 and at least 240 such tiles): 31 x 8 = 248 tiles, one row past the tile grid
    t.append(_case("G_wd_big", "G", "wd", 3841, 2048, 32, kind="wd", bias=True, residual=True))
    t.append(_case("G_wd_big_f16", "G", "wd", 3839, 2048, 32, kind="f16", bias=True, residual=True))
    t.append(_case("G_wd_f16", "G", "wd", 65, 128, 32, kind="f16", bias=True, residual=True))
    t.append(_case("G_wd_transposed", "G", "wd", 65, 128, 64, "nn", kind="t", bias=True, residual=True))
    t.append(_case("G_wd_transposed_m129", "G", "wd", 129, 128, 64, "nn", kind="t"))
    t.append(_case("G_small_plain", "G", "small", 33, 160, 512))
    t.append(_case("G_small_k2048", "G", "small", 33, 32, 2048, bias=True, residual=True))
    return t


CASES = {c.name: c for c in _table_a() + _table_b() + _table_c() + _table_d() + _table_e() + _table_f() + _table_g()}
GROUPS = {g: [n for n, c in CASES.items() if c.group == g] for g in "ABCDEFG"}


# ------------------------------------------------------------------------------------------------------------ buffers
def _up(x, m):
    return (x + m - 1) // m * m


class Buf:
    """a [rows, cols] matrix inside a taller and wider allocation of its own filled with `fill`: .alloc [top + rows + bottom, ld],
    .view = the data, .off = element offset of the data, .ld"""

    def __init__(self, rows, cols, dtype, fill, *, top=TOP, bottom=TOP, left=GCOL, right=GCOL, align=4, data=None):
        self.rows, self.cols, self.top, self.left = rows, cols, top, left
        self.holes = []        # (first row, end row) of the allocation inside the data rows that are guards too (between batch slices)
        self.ld = _up(left + cols + right, align)
        self.alloc = torch.full((top + rows + bottom, self.ld), fill, dtype=dtype)
        if bottom == KTAIL:
            self.alloc[top + rows:] = _TAIL_FILL[0]
        self.off = top * self.ld + left
        if data is not None:
            self.view[...] = data

    @property
    def view(self):
        return self.alloc[self.top:self.top + self.rows, self.left:self.left + self.cols]

    def guard_mask(self):
        m = torch.ones(self.alloc.shape, dtype=torch.bool)
        m[self.top:self.top + self.rows, self.left:self.left + self.cols] = False
        for r0, r1 in self.holes:
            m[r0:r1] = True
        return m


def _operand32(data, bottom=TOP):
    return Buf(data.shape[0], data.shape[1], torch.float32, NAN, left=4, right=4, bottom=bottom, align=4, data=data)


def split_cpu(x, scale=1.0):
    """hi = f16(scale x), lo = f16(scale x - hi): what pfpp_split_planes writes"""
    xs = x.float() * scale
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return hi, lo


def _operand16(x, scale=1.0, bottom=TOP):
    """-> (hi Buf, lo Buf, float64 value (hi + lo) / scale, float64 value hi / scale)"""
    hi, lo = split_cpu(x, scale)
    mk = lambda d: Buf(x.shape[0], x.shape[1], torch.float16, NAN, left=8, right=8, bottom=bottom, align=8, data=d)
    return mk(hi), mk(lo), (hi.double() + lo.double()) / scale, hi.double() / scale


def _out32(rows, cols, c0=None, left=GCOL):
    return Buf(rows, cols, torch.float32, SENTINEL, left=left, align=4, data=c0)


@dataclass
class Problem:
    """one output matrix of a launch: where it lives, what it must hold, how to band it"""
    tag: str
    out: str               # key of the output Buf in built["bufs"] (or a (hi key, lo key) pair: plane output)
    ref: torch.Tensor      # float64 [R, C]
    yard: torch.Tensor     # the same formula in float32 on the CPU
    M: int                 # launch rows / columns: the band boundaries are (M // BM * BM) // row_div, (N // BN * BN) // col_div
    N: int
    row_div: int = 1
    col_div: int = 1
    whole: float = WHOLE_FWD
    banded: bool = True
    sub: int = -1          # >= 0: the problem is this one row of the buffer's data


ACT = {"none": lambda v: v, "relu": torch.relu, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu}


def _gen(c: Case, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + salt)


def _both(fn):
    """evaluate fn(dtype) in float64 (reference) and float32 (yardstick)"""
    return fn(torch.float64), fn(torch.float32)


# ------------------------------------------------------------------------------------------------------------ builders (CPU)
def _build_planes(c: Case):
    g = _gen(c)
    M, N, K, form = c.M, c.N, c.K, c.form
    sA = 1.0 if form == "nt" else 4096.0
    a32 = torch.randn((K, M) if form == "tn" else (M, K), generator=g) * (1.0 if form == "nt" else 1e-2)
    w32 = torch.randn((N, K) if form == "nt" else (K, N), generator=g) / math.sqrt(K)
    ahi, alo, av, avh = _operand16(a32, sA, bottom=KTAIL if form == "tn" else TOP)
    whi, wlo, wv, wvh = _operand16(w32, 1.0, bottom=KTAIL if form != "nt" else TOP)
    if c.o("single_pass"):
        av, wv = avh, wvh
    av = av.t() if form == "tn" else av
    wv = wv if form != "nt" else wv.t()                          # [K, N]
    alpha = c.o("alpha", 1.0)
    bias = torch.randn(N, generator=g) + (0.5 if c.o("act") == "relu" else 0.0) if c.o("bias") else None
    bufs = dict(a_hi=ahi, a_lo=alo, w_hi=whi, w_lo=wlo)
    c0 = torch.randn(M, N, generator=g) * float(av.abs().max()) if c.o("accumulate") else None
    bufs["out"] = _out32(M, N, c0)
    res = None
    if c.o("residual"):
        res = torch.randn(M, N, generator=g) * float(av.abs().max())
        bufs["res"] = Buf(M, N, torch.float32, NAN, left=4, right=8, align=4, data=res)       # ldr != ldc
        assert bufs["res"].ld != bufs["out"].ld
    act = ACT[c.o("act", "none")]

    def f(dt):
        v = alpha * (av.to(dt) @ wv.to(dt))
        if bias is not None:
            v = v + bias.to(dt)
        v = act(v)
        if res is not None:
            v = v + res.to(dt)
        if c0 is not None:
            v = v + c0.to(dt)
        return v
    ref, yard = _both(f)
    whole = WHOLE_FWD if form == "nt" else WHOLE_PLANE_GRAD
    probs = [Problem("C", "out", ref, yard, M, N, whole=whole)]
    if c.o("colsum"):
        cs0 = torch.randn(1, M, generator=g) * float(av.abs().max())
        bufs["colsum"] = Buf(1, M, torch.float32, SENTINEL, top=0, bottom=0, left=8, right=8, data=cs0)
        r2, y2 = _both(lambda dt: (cs0.to(dt) + av.to(dt).sum(1)[None]).t())
        probs.append(Problem("colsum", "colsum", r2, y2, M, 1, whole=whole))
    return dict(bufs=bufs, problems=probs, bias=bias, alpha=alpha, sA=sA)


def _build_gemm(c: Case):
    from_pack = _import_packing()
    g = _gen(c)
    M, N, K = c.M, c.N, c.K
    batch, zdiv = c.o("batch", 1), c.o("zdiv", 1)
    nb = batch // zdiv
    act, pool = c.o("act", "none"), c.o("pool", 0)
    geglu = act == "geglu"
    alpha = c.o("alpha", 1.0)
    bufs, extra = {}, {}
    gather = c.o("gather")
    if gather is not None:
        F, S, ns, Np, D = 2, 3, 32, 40, gather
        assert M == F * S * ns and K == D + 4
        xyz, ctr = torch.rand(F, Np, 3, generator=g), torch.rand(F, S, 3, generator=g)
        idx = torch.randint(0, Np, (F, S, ns), generator=g, dtype=torch.int32)
        feats = torch.randn(F, Np, D, generator=g) if D else None
        fi = torch.arange(F)[:, None, None].expand(F, S, ns)
        rel = xyz[fi, idx.long()] - ctr[:, :, None, :]
        cols = ([feats[fi, idx.long()]] if D else []) + [rel, torch.zeros(F, S, ns, 1)]
        a_all = torch.cat(cols, -1).reshape(1, M, K)
        extra.update(xyz=xyz, ctr=ctr, idx=idx, feats=feats)
    else:
        a_all = torch.randn(batch, M, K, generator=g)
    w_all = torch.randn(batch, N, K, generator=g) / math.sqrt(K)
    bias_all = torch.randn(batch, N, generator=g) + (0.5 if act == "relu" else 0.0)
    scale_all = torch.rand(batch, N, generator=g) + 0.5
    a_val = a_all.double()
    single = bool(c.o("single_pass"))
    # ---- A
    if c.o("a") == "planes":
        assert batch == 1
        bufs["a_hi"], bufs["a_lo"], v, vh = _operand16(a_all[0])
        a_val = (vh if single else v)[None]
    elif gather is None:
        # slices z = 0 .. batch-1 stacked with their own guard rows: slice z starts (TOP + M + TOP) rows after slice z - 1
        b = Buf(batch * (M + 2 * TOP) - 2 * TOP, K, torch.float32, NAN, left=4, right=4, align=4)
        for z in range(batch):
            b.alloc[TOP + z * (M + 2 * TOP):TOP + z * (M + 2 * TOP) + M, 4:4 + K] = a_all[z]
        bufs["a"] = b
    aff = None
    if c.o("affine"):
        aff = (torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.5)
        extra["affine"] = aff
    # ---- W: slice index w(z) = (z % zdiv) * nb + z // zdiv (sW0 = one slice, sW1 = nb slices)
    widx = [(z % zdiv) * nb + z // zdiv for z in range(batch)]
    w_val = w_all.double()
    wk = c.o("w")
    if wk == "pw":
        assert batch == 1
        w_dev = w_all[0]
        if geglu:
            w_dev, bias_p = from_pack.pack_geglu(w_all[0], bias_all[0])
            extra["bias_packed"] = bias_p
        extra["w_pw"] = w_dev.contiguous()
        if single:
            sc = from_pack.plane_scale(w_all[0])
            w_val = ((w_all[0] * sc).half().double() / sc)[None]
    elif wk == "f32":
        b = Buf(batch * (N + 2 * TOP) - 2 * TOP, K, torch.float32, NAN, left=4, right=4, align=4)
        for z in range(batch):
            r0 = TOP + widx[z] * (N + 2 * TOP)
            b.alloc[r0:r0 + N, 4:4 + K] = w_all[z]
        bufs["w"] = b
    else:                                                        # kmajor: [K, N] per slice, ldw > N
        b = Buf(batch * (K + 2 * TOP) - 2 * TOP, N, torch.float32, NAN, left=4, right=4, align=4)
        for z in range(batch):
            r0 = TOP + widx[z] * (K + 2 * TOP)
            b.alloc[r0:r0 + K, 4:4 + N] = w_all[z].t()
        bufs["w"] = b
    # ---- per-column vectors, slice index as W's
    vec = torch.zeros(batch, N)
    if c.o("bias") or c.o("bn"):
        for z in range(batch):
            vec[widx[z]] = bias_all[z]
        extra["bias_vec"] = vec
    if c.o("bn"):
        sv = torch.zeros(batch, N)
        for z in range(batch):
            sv[widx[z]] = scale_all[z]
        extra["scale_vec"] = sv
    # ---- outputs
    rows = M // pool if pool else M
    n_out = N // 2 if geglu else N
    R = rows + 2 * TOP
    res_all = torch.randn(batch, rows, n_out, generator=g) if c.o("residual") else None
    if c.o("out_planes"):
        mk = lambda: Buf(rows, n_out, torch.float16, SENTINEL_F16, left=8, right=8, align=8)
        bufs["out_hi"], bufs["out_lo"] = mk(), mk()
    else:
        bufs["out"] = Buf(batch * R - 2 * TOP, n_out, torch.float32, SENTINEL, align=4)
        bufs["out"].holes = [(TOP + z * R + rows, TOP + (z + 1) * R) for z in range(batch - 1)]
    if res_all is not None:
        b = Buf(batch * R - 2 * TOP, n_out, torch.float32, NAN, left=4, right=8, align=4)       # own allocation, ldr != ldc
        for z in range(batch):
            b.alloc[TOP + z * R:TOP + z * R + rows, 4:4 + n_out] = res_all[z]
        bufs["res"] = b
        assert b.ld != bufs["out"].ld
    if c.o("c_min"):
        bufs["c_min"] = Buf(rows, n_out, torch.float32, SENTINEL, left=0, right=bufs["out"].ld - n_out, align=4)
        assert bufs["c_min"].ld == bufs["out"].ld
    if c.o("stats"):
        bufs["stats"] = Buf(2, N, torch.float64, 0.0, top=0, bottom=0, left=0, right=0, align=1)
    actf = ACT[act if not geglu else "none"]
    probs = []
    pre_all = {}

    def f(z, dt, what="out"):
        a = a_val[z if gather is None else 0].to(dt)
        if aff is not None:
            a = torch.relu(a * aff[0].to(dt) + aff[1].to(dt))
        v = alpha * (a @ w_val[z].to(dt).t())
        if c.o("bn"):
            v = v * scale_all[z].to(dt) + bias_all[z].to(dt)
        elif c.o("bias"):
            v = v + bias_all[z].to(dt)
        if what == "pre":
            return v
        if geglu:
            h, gg = v.chunk(2, -1)
            v = h * torch.nn.functional.gelu(gg)
        else:
            v = actf(v)
        if pool:
            grp = v.view(M // pool, pool, N)
            v = grp.min(1)[0] if what == "min" else grp.max(1)[0]
        if res_all is not None:
            v = v + res_all[z].to(dt)
        return v
    for z in range(batch):
        r, y = _both(lambda dt: f(z, dt))
        key = ("out_hi", "out_lo") if c.o("out_planes") else "out"
        probs.append(Problem(f"z{z}" if batch > 1 else "C", key, r, y, M, N, row_div=pool or 1, col_div=2 if geglu else 1))
    if c.o("c_min"):
        r, y = _both(lambda dt: f(0, dt, "min"))
        probs.append(Problem("c_min", "c_min", r, y, M, N, row_div=pool))
    if c.o("stats"):
        def st(dt):
            v = f(0, dt, "pre")
            return torch.stack((v.sum(0), (v * v).sum(0)))
        r, y = _both(st)
        probs.append(Problem("st_sum", "stats", r[0:1], y[0:1], 1, N, banded=False, sub=0))
        probs.append(Problem("st_sq", "stats", r[1:2], y[1:2], 1, N, banded=False, sub=1))
    return dict(bufs=bufs, problems=probs, extra=extra, alpha=alpha, widx=widx, R=R)


def _build_grad(c: Case):
    g = _gen(c)
    M, N, K, form = c.M, c.N, c.K, c.form
    a32 = torch.randn((K, M) if form == "tn" else (M, K), generator=g)
    w32 = torch.randn((N, K) if form == "nt" else (K, N), generator=g) / math.sqrt(K)
    bufs = dict(a=_operand32(a32, bottom=KTAIL if form == "tn" else TOP), w=_operand32(w32, bottom=KTAIL if form != "nt" else TOP))
    av = a32.t() if form == "tn" else a32
    wv = w32.t() if form == "nt" else w32
    alpha = c.o("alpha", 1.0)
    c0 = torch.randn(M, N, generator=g) if c.o("accumulate") else None
    bufs["out"] = _out32(M, N, c0)

    def f(dt):
        v = alpha * (av.to(dt) @ wv.to(dt))
        return v if c0 is None else v + c0.to(dt)
    r, y = _both(f)
    whole = WHOLE_PLANE_GRAD if form == "nn" else WHOLE_GRAD
    probs = [Problem("C", "out", r, y, M, N, whole=whole)]
    if c.o("colsum"):
        cs0 = torch.randn(1, M, generator=g)
        bufs["colsum"] = Buf(1, M, torch.float32, SENTINEL, top=0, bottom=0, left=8, right=8, data=cs0)
        r2, y2 = _both(lambda dt: (cs0.to(dt) + av.to(dt).sum(1)[None]).t())
        probs.append(Problem("colsum", "colsum", r2, y2, M, 1, whole=whole))
    return dict(bufs=bufs, problems=probs, alpha=alpha)


def _build_grad_group(c: Case):
    g = _gen(c)
    bufs, probs = {}, []
    for j, (M, N, K) in enumerate(c.jobs):                       # dW [M = out, N = in] += dY [K, M]^T . X [K, N]
        dy, x = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g) / math.sqrt(K)
        c0 = torch.randn(M, N, generator=g)
        bufs[f"a{j}"], bufs[f"w{j}"] = _operand32(dy, bottom=KTAIL), _operand32(x, bottom=KTAIL)
        bufs[f"out{j}"] = _out32(M, N, c0)
        r, y = _both(lambda dt: c0.to(dt) + dy.to(dt).t() @ x.to(dt))
        probs.append(Problem(f"job{j}", f"out{j}", r, y, M, N, whole=WHOLE_GRAD))
    return dict(bufs=bufs, problems=probs)


def _build_dw_group(c: Case):
    g = _gen(c)
    K = c.K
    bufs, probs = {}, []
    for j, (M, N) in enumerate(c.jobs):
        dy, x = torch.randn(K, M, generator=g) * 1e-2, torch.randn(K, N, generator=g) / math.sqrt(K)
        # no leading dimensions in this ABI (contract: lda = M, ldw = ldc = N): guard rows only
        mk = lambda d, fill, dt_, bottom: Buf(d.shape[0], d.shape[1], dt_, fill, left=0, right=0, bottom=bottom, align=1, data=d)
        hi, lo = split_cpu(dy, 4096.0)
        bufs[f"a_hi{j}"], bufs[f"a_lo{j}"] = mk(hi, NAN, torch.float16, KTAIL), mk(lo, NAN, torch.float16, KTAIL)
        dv = (hi.double() + lo.double()) / 4096.0
        hi, lo = split_cpu(x, 1.0)
        bufs[f"w_hi{j}"], bufs[f"w_lo{j}"] = mk(hi, NAN, torch.float16, KTAIL), mk(lo, NAN, torch.float16, KTAIL)
        xv = hi.double() + lo.double()
        c0 = torch.randn(M, N, generator=g) * 1e-2
        bufs[f"out{j}"] = mk(c0, SENTINEL, torch.float32, TOP)
        r, y = _both(lambda dt: c0.to(dt) + dv.to(dt).t() @ xv.to(dt))
        probs.append(Problem(f"gw{j}", f"out{j}", r, y, M, N, whole=WHOLE_PLANE_GRAD))
        if j != 1:                                               # gb = None on job 1
            b0 = torch.randn(1, M, generator=g) * 1e-2
            bufs[f"gb{j}"] = Buf(1, M, torch.float32, SENTINEL, top=0, bottom=0, left=8, right=8, data=b0)
            r, y = _both(lambda dt: (b0.to(dt) + dv.to(dt).sum(0)[None]).t())
            probs.append(Problem(f"gb{j}", f"gb{j}", r, y, M, 1, whole=WHOLE_PLANE_GRAD))
    return dict(bufs=bufs, problems=probs)


def _build_wd(c: Case):
    """wd / small: A planes [M, K] with guards, the weight a packing.PW built on the device (kind t: planes of W as stored [K, N]),
    bias, residual ALIASING the output (ldc > N)"""
    g = _gen(c)
    M, N, K = c.M, c.N, c.K
    kind = c.o("kind", "small")
    a32 = torch.randn(M, K, generator=g)
    w32 = torch.randn(N, K, generator=g) / math.sqrt(K)
    ahi, alo, av, avh = _operand16(a32)
    bufs = dict(a_hi=ahi, a_lo=alo)
    extra = {}
    if kind == "t":
        whi, wlo, wv, _ = _operand16(w32.t().contiguous())       # [K, N]
        bufs["w_hi"], bufs["w_lo"] = whi, wlo
        wv = wv.t()
    else:
        pk = _import_packing()
        sc = pk.plane_scale(w32)
        hi, lo = split_cpu(w32, sc)
        wv = (hi.double() if kind == "f16" else hi.double() + lo.double()) / sc
        extra["w_pw"] = w32
    if kind == "f16":
        av = avh
    bias = torch.randn(N, generator=g) * 0.1 if c.o("bias") else None
    res = torch.randn(M, N, generator=g) if c.o("residual") else None
    bufs["out"] = _out32(M, N, res)

    def f(dt):
        v = av.to(dt) @ wv.to(dt).t()
        if bias is not None:
            v = v + bias.to(dt)
        return v if res is None else v + res.to(dt)
    r, y = _both(f)
    return dict(bufs=bufs, problems=[Problem("C", "out", r, y, M, N, whole=WHOLE_FWD if kind == "f16" else WHOLE_PLANE_GRAD)],
                bias=bias, extra=extra)


def _import_packing():
    root = Path(__file__).resolve().parents[1]
    for p in (str(root), str(root / "puzzlefusion-plusplus_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from pfpp_hip import packing
    return packing


_BUILDERS = dict(planes=_build_planes, gemm=_build_gemm, grad=_build_grad, grad_group=_build_grad_group, dw_group=_build_dw_group,
                 wd=_build_wd, small=_build_wd)


@lru_cache(maxsize=2)
def built(c: Case):
    """CPU side of a case: bufs {name: Buf}, problems [Problem], and what the runner needs; cached: treat as read-only"""
    return _BUILDERS[c.entry](c)


def built_with_tail(c: Case, fill: float):
    """the case built again (not cached) with `fill` instead of NaN in the rows after row K of its k-major operands"""
    _TAIL_FILL[0] = fill
    try:
        return _BUILDERS[c.entry](c)
    finally:
        _TAIL_FILL[0] = NAN


def read_reference(c: Case, b: dict, extra_rows: int = 0):
    """the product A^T . W of a weight-gradient case restated from the ALLOCATIONS a launch reads (planes: (hi + lo) / scale), over
    rows 0 .. K - 1 + extra_rows of the k-major operands -> {job: float64 [M, N]}"""
    jobs = [(j, jb[2] if len(jb) > 2 else c.K) for j, jb in enumerate(c.jobs)] if c.jobs else [("", c.K)]
    res = {}
    for j, K in jobs:
        def val(stem):
            if f"{stem}_hi{j}" in b["bufs"]:
                hi, lo = b["bufs"][f"{stem}_hi{j}"], b["bufs"][f"{stem}_lo{j}"]
                rows = lambda bf: bf.alloc[bf.top:bf.top + K + extra_rows, bf.left:bf.left + bf.cols].double()
                return rows(hi) + rows(lo)
            bf = b["bufs"][f"{stem}{j}"]
            return bf.alloc[bf.top:bf.top + K + extra_rows, bf.left:bf.left + bf.cols].double()
        res[j] = val("a").t() @ val("w")
    return res


# ------------------------------------------------------------------------------------------------------------ layout rules
def check_layout(c: Case):
    """the guard layout against the entry point's alignment rules (the PFPP_REQUIRE lines of the entry points); raises AssertionError"""
    b = built(c)["bufs"]
    for name, buf in b.items():
        es = buf.alloc.element_size()
        if name.startswith(("gb", "colsum", "stats")):
            assert (buf.off * es) % 4 == 0
            continue
        assert (buf.off * es) % 16 == 0, (c.name, name, "16-byte aligned operands")
        if buf.alloc.dtype == torch.float16 and c.entry != "dw_group":
            assert buf.ld % 8 == 0, (c.name, name, "plane leading dimensions % 8 == 0")
        elif buf.alloc.dtype == torch.float32 and c.entry != "dw_group":
            assert buf.ld % 4 == 0, (c.name, name)
        if name.startswith("out") and c.entry != "dw_group":
            assert buf.left >= GCOL and buf.ld >= buf.left + buf.cols + GCOL and buf.top >= TOP, (c.name, name, "output guards")
    if c.entry == "dw_group":
        for M, N in c.jobs:
            assert M % 8 == 0 and N % 8 == 0
    if c.entry == "planes":
        assert c.K % 32 == 0 or c.form == "tn"
        assert c.form != "tn" or c.M % 8 == 0
        assert c.form == "nt" or c.N % 8 == 0
        if c.o("splits", 1) > 1 and c.o("use_ws", True):          # the slab path: N % 4, ldc % 4 (else the launcher falls back to atomics)
            assert c.N % 4 == 0 and b["out"].ld % 4 == 0
    if c.entry == "grad":
        assert c.form != "tn" or c.M % 4 == 0
        assert c.form == "nt" or c.N % 4 == 0
    if c.entry == "grad_group":
        assert all(M % 4 == 0 and N % 4 == 0 for M, N, _ in c.jobs) and len(c.jobs) <= 8
    if c.entry == "gemm":
        if c.o("a") == "planes":
            assert c.K % 32 == 0 and (c.N > 64 or c.o("act") == "geglu")
        if c.o("act") == "geglu":
            assert c.N % 64 == 0
        if c.o("pool"):
            assert c.M % c.o("pool") == 0
    if c.entry == "wd":
        assert c.N % 128 == 0 and c.K % 32 == 0 and (c.o("kind") != "t" or c.K % 64 == 0)
    if c.entry == "small":
        assert c.N % 32 == 0 and c.K % 512 == 0


# ------------------------------------------------------------------------------------------------------------ error report
def tile_of(kernel: str):
    """BM, BN of a kernel name as pfpp_last_gemm_kernel reports it (template arguments in the order of the csrc/ definitions)"""
    name, _, rest = kernel.partition("<")
    f = [x.strip() for x in rest.split(">")[0].split(",")] if rest else []
    if name in ("gemm_pl_kernel", "gemm_pl_dwgroup_kernel", "gemm_grad_kernel", "gemm_grad_group_kernel", "gemm_f16x3_deep_kernel"):
        return 32 * int(f[0]) * int(f[2]), 32 * int(f[1]) * int(f[3])          # <MT, NT, WM, WN, ...>
    if name == "gemm_f16x3_kernel":
        return 32 * int(f[0]) * int(f[3]), 32 * int(f[1]) * int(f[4])          # <MT, NT, WPRE, WM, WN, ...>
    if name == "gemm_f32_mfma_kernel":
        return 64 * int(f[0]), 64 * int(f[1])
    if name == "gemm_wd_kernel":
        return 32 * int(f[0]), 128 * int(f[1])
    if name == "gemm_small_kernel":
        return 32, 128
    if name == "gemm_small_ks_kernel":
        return 32, 32                                                          # its grid: one workgroup per 32 x 32 output unit
    raise ValueError(f"no tile known for kernel {kernel!r}")


def bands(p: Problem, BM: int, BN: int):
    """-> {band: (row slice, column slice)} of the problem's [R, C] result; empty bands left out"""
    R, C = p.ref.shape
    if not p.banded:
        return {"all": (slice(0, R), slice(0, C))}
    rb = min(R, (p.M // BM * BM) // p.row_div)
    cb = min(C, (p.N // BN * BN) // p.col_div)
    res = {"interior": (slice(0, rb), slice(0, cb)), "right": (slice(0, rb), slice(cb, C)),
           "bottom": (slice(rb, R), slice(0, cb)), "corner": (slice(rb, R), slice(cb, C))}
    return {k: v for k, v in res.items() if v[0].stop > v[0].start and v[1].stop > v[1].start}


def band_errors(p: Problem, got: torch.Tensor, BM: int, BN: int):
    """{band: max |got - ref| / max |ref| over the band}, and the whole-matrix figure under "whole" """
    res = {}
    d = (got.double() - p.ref).abs()
    for k, (rs, cs) in bands(p, BM, BN).items():
        e, den = float(d[rs, cs].max()), float(p.ref[rs, cs].abs().max())
        res[k] = e / den if math.isfinite(e) and den > 0 else math.inf
    e = float(d.max())
    res["whole"] = e / float(p.ref.abs().max()) if math.isfinite(e) else math.inf
    return res


def evaluate(c: Case, outs: dict, kernel: str):
    """outs: {buffer name: allocation after the launch (CPU)} -> dict(case, kernel, finite, guards_ok, lines [(tag, band, err, bound)], ok)"""
    b = built(c)
    BM, BN = tile_of(kernel.split("+")[0])
    lines, finite, guards = [], True, True
    for name, after in outs.items():
        buf = b["bufs"][name]
        m = buf.guard_mask()
        guards &= bool(torch.equal(_bits(after[m]), _bits(buf.alloc[m])))
    for p in b["problems"]:
        if isinstance(p.out, tuple):
            got = _view_of(c, p, outs[p.out[0]], p.out[0]).double() + _view_of(c, p, outs[p.out[1]], p.out[1]).double()
        else:
            got = _view_of(c, p, outs[p.out], p.out)
        finite &= bool(torch.isfinite(got).all())
        for band, e in band_errors(p, got, BM, BN).items():
            lines.append((p.tag, band, e, p.whole if band == "whole" else BAND_BOUND))
    ok = finite and guards and all(e <= bnd for _, _, e, bnd in lines)
    return dict(case=c.name, kernel=kernel, finite=finite, guards_ok=guards, lines=lines, ok=ok)


def _bits(t: torch.Tensor):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _view_of(c: Case, p: Problem, alloc: torch.Tensor, name: str):
    """the problem's [R, C] data inside an output allocation"""
    buf = built(c)["bufs"][name]
    R, C = p.ref.shape
    if p.tag.startswith("z") and c.o("batch", 1) > 1:             # batched C: slice z, guard rows in between
        z = int(p.tag[1:])
        r0 = TOP + z * built(c)["R"]
        return alloc[r0:r0 + R, buf.left:buf.left + C]
    v = alloc[buf.top:buf.top + buf.rows, buf.left:buf.left + buf.cols]
    if p.sub >= 0:
        return v[p.sub:p.sub + 1]
    return v.t() if v.shape != (R, C) else v                     # (column sums live in a row)


def yardstick(c: Case, BM: int, BN: int):
    """[(tag, band, error of the float32 CPU evaluation against float64)]"""
    res = []
    for p in built(c)["problems"]:
        for band, e in band_errors(p, p.yard, BM, BN).items():
            res.append((p.tag, band, e, p.whole if band == "whole" else BAND_BOUND))
    return res


def describe(rep: dict) -> str:
    out = []
    for tag, band, e, bnd in rep["lines"]:
        out.append(f"gemm_edges {rep['case']:<32} {rep['kernel']:<78} {tag:<7} {band:<8} err {e:.3e} bound {bnd:.0e} {'ok  ' if e <= bnd else 'OVER'}")
    if not rep["finite"] or not rep["guards_ok"]:
        out.append(f"gemm_edges {rep['case']:<32} finite {rep['finite']} guards_intact {rep['guards_ok']}")
    return "\n".join(out)


# ------------------------------------------------------------------------------------------------------------ GPU runs
class _Dev:
    """the case's allocations on the device"""

    def __init__(self, c: Case, dev):
        self.b = built(c)
        self.t = {}
        for k, v in self.b["bufs"].items():
            self.t[k] = v.alloc.to(dev)

    def buf(self, k):
        return self.b["bufs"][k]

    def outs(self, keys):
        return {k: self.t[k].cpu() for k in keys}


def _out_keys(c: Case):
    return [k for k in built(c)["bufs"] if k.startswith(("out", "colsum", "gb", "c_min", "stats"))]


def _last_kernel():
    from pfpp_hip import _lib
    return _lib.load().pfpp_last_gemm_kernel().decode()


def _pw_shim(hi, lo, N, K, scale=1.0):
    """a packing.PW around existing plane allocations (pfpp_gemm on the very planes pfpp_gemm_planes read)"""
    from pfpp_hip.packing import PW
    w = PW.__new__(PW)
    w.f32 = torch.zeros(4, dtype=torch.float32, device=hi.device)
    w.hi, w.lo, w.N, w.K, w.scale, w._frag = hi, lo, N, K, scale, None
    return w


def run_planes(c: Case, dev):
    from pfpp_hip import ops, planes as P
    d = _Dev(c, dev)
    b = d.b
    A = P.Planes(d.t["a_hi"], d.t["a_lo"], b["sA"])
    W = P.Planes(d.t["w_hi"], d.t["w_lo"], 1.0)
    bias = None if b["bias"] is None else b["bias"].to(dev)
    kw = dict(M=c.M, N=c.N, K=c.K, a_kmajor=c.form == "tn", w_kmajor=c.form != "nt", bias=bias, act=c.o("act", "none"),
              accumulate=bool(c.o("accumulate")), splits=c.o("splits", 0), variant=c.o("variant", 0), alpha=b["alpha"] / b["sA"],
              use_ws=c.o("use_ws", True), single_pass=bool(c.o("single_pass")),
              lda=d.buf("a_hi").ld, ldw=d.buf("w_hi").ld, ldc=d.buf("out").ld, a_off=d.buf("a_hi").off, w_off=d.buf("w_hi").off,
              c_off=d.buf("out").off)
    if c.o("residual"):
        kw.update(residual=d.t["res"], ldr=d.buf("res").ld, r_off=d.buf("res").off)
    if c.o("colsum"):
        kw["colsum"] = d.t["colsum"].view(-1)[d.buf("colsum").off:d.buf("colsum").off + c.M]
    P.gemm(A, W, d.t["out"], **kw)
    kernel = _last_kernel()
    torch.cuda.synchronize()
    same = None
    if c.form == "nt" and not c.o("accumulate") and c.o("splits", 0) == 1 and c.N > 64:
        # pfpp_gemm on the same planes, into a second allocation prepared the same way: the same bits (include/pfpp.h)
        twin = d.buf("out").alloc.to(dev)
        prev = ops.SINGLE_PASS
        try:
            ops.SINGLE_PASS = bool(c.o("single_pass"))
            ops.gemm(ops.SplitAct(d.t["a_hi"], d.t["a_lo"]), _pw_shim(d.t["w_hi"], d.t["w_lo"], c.N, c.K), M=c.M, N=c.N, K=c.K,
                     lda=d.buf("a_hi").ld, ldw=d.buf("w_hi").ld, out=twin, ldc=d.buf("out").ld, bias=bias, act=c.o("act", "none"),
                     residual=d.t.get("res"), ldr=d.buf("res").ld if c.o("residual") else 0,
                     r_off=d.buf("res").off if c.o("residual") else None, alpha=b["alpha"] / b["sA"],
                     a_off=d.buf("a_hi").off, w_off=d.buf("w_hi").off, c_off=d.buf("out").off, mode="f16x3")
        finally:
            ops.SINGLE_PASS = prev
        torch.cuda.synchronize()
        same = bool(torch.equal(twin, d.t["out"]))
    return d.outs(_out_keys(c)), kernel, dict(same_bits=same)


def run_gemm(c: Case, dev):
    from pfpp_hip import ops, planes as P
    from pfpp_hip.packing import PW
    d = _Dev(c, dev)
    b, ex = d.b, d.b["extra"]
    M, N, K = c.M, c.N, c.K
    batch, zdiv = c.o("batch", 1), c.o("zdiv", 1)
    nb = batch // zdiv
    pool, geglu = c.o("pool", 0), c.o("act") == "geglu"
    rows = M // pool if pool else M
    kw = dict(M=M, N=N, K=K, act=c.o("act", "none"), pool=pool, alpha=b["alpha"], mode=c.o("mode", "f16x3"), batch=batch, zdiv=zdiv)
    gather = c.o("gather")
    if c.o("a") == "planes":
        A = ops.SplitAct(d.t["a_hi"], d.t["a_lo"])
        kw.update(lda=d.buf("a_hi").ld, a_off=d.buf("a_hi").off)
    elif gather is not None:
        A = None if ex["feats"] is None else ex["feats"].to(dev).view(-1, gather)
        kw.update(lda=gather, gather=(ex["idx"].to(dev), ex["xyz"].to(dev), ex["ctr"].to(dev)))
    else:
        A = d.t["a"]
        SA = (M + 2 * TOP) * d.buf("a").ld
        kw.update(lda=d.buf("a").ld, a_off=d.buf("a").off, sA=(zdiv * SA, SA) if batch > 1 else (0, 0))
    wk = c.o("w")
    if wk == "pw":
        W = PW(ex["w_pw"].to(dev))
    else:
        W = d.t["w"]
        SW = ((K if wk == "kmajor" else N) + 2 * TOP) * d.buf("w").ld
        kw.update(ldw=d.buf("w").ld, w_off=d.buf("w").off, w_kmajor=wk == "kmajor", sW=(SW, nb * SW) if batch > 1 else (0, 0))
    if c.o("bn"):
        kw.update(scale=ex["scale_vec"].to(dev), shift=ex["bias_vec"].to(dev))
    elif c.o("bias"):
        kw["bias"] = (ex["bias_packed"] if geglu else ex["bias_vec"]).to(dev).contiguous()
    if batch > 1:
        kw["sV"] = (N, nb * N)
    if c.o("out_planes"):
        out = ops.SplitAct(d.t["out_hi"], d.t["out_lo"])
        ob = d.buf("out_hi")
    else:
        out, ob = d.t["out"], d.buf("out")
    SC = b["R"] * ob.ld
    kw.update(out=out, ldc=ob.ld, c_off=ob.off, sC=(zdiv * SC, SC) if batch > 1 else (0, 0))
    if c.o("residual"):
        kw.update(residual=d.t["res"], ldr=d.buf("res").ld, r_off=d.buf("res").off)
    if c.o("affine"):
        kw["a_affine"] = (ex["affine"][0].to(dev), ex["affine"][1].to(dev))
    if c.o("stats"):
        kw["stats"] = d.t["stats"].view(1, 2, N)
    if c.o("c_min"):
        kw["c_min"] = d.t["c_min"][d.buf("c_min").top:]
    old_ws, old_sp = ops._split_workspace, ops.SINGLE_PASS
    if not c.o("lend_ws", True):
        ops._split_workspace = lambda device: None
    ops.SINGLE_PASS = bool(c.o("single_pass"))
    try:
        ops.gemm(A, W, **kw)
    finally:
        ops._split_workspace, ops.SINGLE_PASS = old_ws, old_sp
    kernel = _last_kernel()
    torch.cuda.synchronize()
    same = None
    if planes_twin(c):
        # pfpp_gemm_planes (non-accumulating, no K split, its own choice of tile) on the same A planes and the packed weight's planes,
        # into a second allocation prepared the same way: the same bits (include/pfpp.h)
        twin = ob.alloc.to(dev)
        pk = dict(residual=d.t["res"], ldr=d.buf("res").ld, r_off=d.buf("res").off) if c.o("residual") else {}
        P.gemm(P.Planes(d.t["a_hi"], d.t["a_lo"]), P.Planes(W.hi, W.lo), twin, M=M, N=N, K=K, bias=kw.get("bias"), act=c.o("act", "none"),
               splits=1, alpha=b["alpha"] / W.scale, single_pass=bool(c.o("single_pass")), lda=d.buf("a_hi").ld, ldc=ob.ld,
               a_off=d.buf("a_hi").off, c_off=ob.off, **pk)
        torch.cuda.synchronize()
        same = bool(torch.equal(twin, d.t["out"]))
    return d.outs(_out_keys(c)), kernel, dict(same_bits=same)


def planes_twin(c: Case) -> bool:
    """does pfpp_gemm_planes accept this pfpp_gemm call?  nt form, both operands pre-split, fp32 output, bias / residual / an
    activation it knows (no GEGLU, scale / shift, pooling, batch)"""
    return (c.entry == "gemm" and c.o("a") == "planes" and c.o("w") == "pw" and c.o("act", "none") != "geglu" and not c.o("out_planes")
            and not c.o("bn") and not c.o("pool") and c.o("batch", 1) == 1)


def run_grad(c: Case, dev):
    from pfpp_hip import train_ops as TO
    d = _Dev(c, dev)
    kw = {}
    if c.o("colsum"):
        kw["colsum"] = d.t["colsum"].view(-1)[d.buf("colsum").off:d.buf("colsum").off + c.M]
    TO.gemm_grad(d.t["a"], d.t["w"], d.t["out"], M=c.M, N=c.N, K=c.K, lda=d.buf("a").ld, ldw=d.buf("w").ld, ldc=d.buf("out").ld,
                 a_kmajor=c.form == "tn", w_kmajor=c.form != "nt", accumulate=bool(c.o("accumulate")), split_k=c.o("split_k", 0),
                 a_scale=c.o("a_scale", 1.0), w_scale=c.o("w_scale", 1.0), alpha=d.b["alpha"], a_off=d.buf("a").off,
                 w_off=d.buf("w").off, c_off=d.buf("out").off, **kw)
    kernel = _last_kernel()
    torch.cuda.synchronize()
    return d.outs(_out_keys(c)), kernel, {}


def run_grad_group(c: Case, dev):
    from pfpp_hip import train_ops as TO
    d = _Dev(c, dev)
    sl = lambda k: d.t[k][d.buf(k).top:d.buf(k).top + d.buf(k).rows, d.buf(k).left:d.buf(k).left + d.buf(k).cols]
    TO.grad_weight_group([(sl(f"a{j}"), sl(f"w{j}"), sl(f"out{j}")) for j in range(len(c.jobs))])
    kernel = _last_kernel()
    torch.cuda.synchronize()
    return d.outs(_out_keys(c)), kernel, {}


def run_dw_group(c: Case, dev):
    from pfpp_hip import planes as P
    d = _Dev(c, dev)
    probs = []
    for j, (M, N) in enumerate(c.jobs):
        top = d.buf(f"a_hi{j}").top
        dy = P.Planes(d.t[f"a_hi{j}"][top:], d.t[f"a_lo{j}"][top:], 4096.0)        # rows K .. are the NaN tail
        x = P.Planes(d.t[f"w_hi{j}"][top:], d.t[f"w_lo{j}"][top:], 1.0)
        gw = d.t[f"out{j}"][TOP:TOP + M]
        gb = None
        if f"gb{j}" in d.t:
            o = d.buf(f"gb{j}").off
            gb = d.t[f"gb{j}"].view(-1)[o:o + M]
        probs.append((dy, x, gw, gb))
    P.dw_group(probs, c.K, c.o("variant", 0))
    kernel = _last_kernel()
    torch.cuda.synchronize()
    return d.outs(_out_keys(c)), kernel, {}


def run_wd(c: Case, dev):
    """gemm_wd / gemm_small in place over the residual, and (wd) the tiled plane GEMM on the same operands into a twin allocation"""
    from pfpp_hip import ops, planes as P
    from pfpp_hip.packing import PW
    d = _Dev(c, dev)
    b = d.b
    M, N, K = c.M, c.N, c.K
    kind = c.o("kind", "small")
    view = lambda k: d.t[k][d.buf(k).top:d.buf(k).top + d.buf(k).rows, d.buf(k).left:d.buf(k).left + d.buf(k).cols]
    bias = None if b["bias"] is None else b["bias"].to(dev)
    out = view("out")
    res = out if c.o("residual") else None
    twin = d.buf("out").alloc.to(dev)
    ob = d.buf("out")
    same = None
    if kind == "t":
        # planes.gemm_wd takes no offsets: a flat view from the first data element on, re-cut into rows of the allocation's length
        def shifted(k, rows):
            bf = d.buf(k)
            return d.t[k].view(-1)[bf.off:bf.off + (rows + 1) * bf.ld].view(rows + 1, bf.ld)
        Af = P.Planes(shifted("a_hi", M), shifted("a_lo", M))
        Wf = P.Planes(shifted("w_hi", K), shifted("w_lo", K))
        P.gemm_wd(Af, Wf, out, M=M, N=N, K=K, bias=bias, residual=res, transposed=True)
        kernel = _last_kernel()
        P.gemm(P.Planes(d.t["a_hi"], d.t["a_lo"]), P.Planes(d.t["w_hi"], d.t["w_lo"]), twin, M=M, N=N, K=K, w_kmajor=True, bias=bias,
               residual=twin if res is not None else None, splits=1, lda=d.buf("a_hi").ld, ldw=d.buf("w_hi").ld, ldc=ob.ld, ldr=ob.ld,
               a_off=d.buf("a_hi").off, w_off=d.buf("w_hi").off, c_off=ob.off, r_off=ob.off)
        torch.cuda.synchronize()
        same = bool(torch.equal(twin, d.t["out"]))
    else:
        a = ops.SplitAct(view("a_hi"), view("a_lo"))
        pw = PW(b["extra"]["w_pw"].to(dev))
        if kind == "small":
            ops.gemm_small(a, pw, bias=bias, residual=res, out=out)
            kernel = _last_kernel()
        else:
            ops.gemm_wd(a, pw, bias=bias, residual=res, out=out, single_pass=kind == "f16")
            kernel = _last_kernel()
            prev = ops.SINGLE_PASS
            try:
                ops.SINGLE_PASS = kind == "f16"
                ops.gemm(ops.SplitAct(d.t["a_hi"], d.t["a_lo"]), pw, M=M, N=N, K=K, lda=d.buf("a_hi").ld, a_off=d.buf("a_hi").off,
                         out=twin, ldc=ob.ld, c_off=ob.off, bias=bias, residual=twin if res is not None else None, ldr=ob.ld)
            finally:
                ops.SINGLE_PASS = prev
            torch.cuda.synchronize()
            same = bool(torch.equal(twin, d.t["out"]))
    torch.cuda.synchronize()
    return d.outs(_out_keys(c)), kernel, dict(same_bits=same)


_RUNNERS = dict(planes=run_planes, gemm=run_gemm, grad=run_grad, grad_group=run_grad_group, dw_group=run_dw_group, wd=run_wd,
                small=run_wd)


def run(c: Case, dev):
    """-> (report of evaluate(), flags)"""
    outs, kernel, flags = _RUNNERS[c.entry](c, dev)
    return evaluate(c, outs, kernel), flags


def report_main() -> int:
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root), str(root / "puzzlefusion-plusplus_amd")]
    from pfpp_hip._lib import PfppError
    dev = torch.device("cuda:0")
    bad = 0
    for name, c in CASES.items():
        try:
            rep, flags = run(c, dev)
        except (ValueError, TypeError, PfppError) as e:          # a call the wrapper or the entry point rejects is a line of the record too
            print(f"gemm_edges {name:<32} ERROR {type(e).__name__}: {str(e)[:200]}", flush=True)
            bad += 1
            continue
        except Exception as e:                                   # anything else (a HIP error): nothing more is launched
            print(f"gemm_edges {name:<32} STOPPED {type(e).__name__}: {str(e)[:200]}", flush=True)
            return 2
        print(describe(rep), flush=True)
        if flags.get("same_bits") is not None:
            print(f"gemm_edges {name:<32} same bits as the other entry point: {flags['same_bits']}", flush=True)
        bad += not rep["ok"] or flags.get("same_bits") is False
    print(f"gemm_edges {len(CASES)} cases, {bad} not ok", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    if "--report" in sys.argv:
        sys.exit(report_main())
    print(f"{len(CASES)} cases: " + ", ".join(f"{g} {len(v)}" for g, v in GROUPS.items()))
