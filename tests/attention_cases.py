"""Case table, float64 reference and error report of the attention edge tests (no test in here; importable without a GPU).
tests/test_attention_cases_host.py checks the table itself on the CPU, tests/test_gpu_attention_edges.py runs it through the HIP
kernels, once more per CROSS_CHECKS setting for the kernels that the defaults never pick.

Both attentions read a packed projection qkv [rows, 3 H dh] = (q | k | v) and ragged groups (off, len) of rows: the sequences of the
dense attention (csrc/attention.hip, attention_bwd.hip: 32-key tiles inside 128-row workgroups, optional key mask), the fragments
of the block-diagonal one (L <= 32 rows each).  `reference` restates softmax(q k^T scale + mask) v per (group, head) in torch and
takes dqkv from autograd; in float64 it is the reference of every comparison, in float32 it is the yardstick (below).

The error is reported per BLOCK = (group, head, part) with part in out / dq / dk / dv: max |got - ref| over the block divided by
max |ref| over the same block, so that a wrong tail row of a long sequence cannot hide behind the larger gradients of a short one in
the same launch, nor a wrong dk behind a larger dv.  Two kinds of block have a reference that is identically zero, dq and dk of a
group of length 1 (the softmax of one logit has no gradient: dS = P (dP - D) = 0): they are divided by the size of the terms that
cancel, scale max|dO . v| max|k| (dq) and scale max|dO . v| max|q| (dk), which is what a kernel's rounding of dP against D is
relative to.  lse and D = rowsum(dO . out) are compared per (group, head) as max |got - ref| / max(1, |ref|).

Bounds.  The floors are the project's bounds for these operations, now per block: 1e-5 (out), 2e-5 (dqkv), 3e-6 max(1, |ref|) (the
block-diagonal forward, an absolute error).  The `hard` cases (the logit-range sweep E, gradients of 1e-6) are not given a number
in advance: their yardstick is the same block's error under torch float32 CPU autograd of the same formula, and the bound is
max(floor, 8 yardstick + max|lse| 2^-22): 8 for the three-product split-f16 arithmetic (22 bits per operand) and the hardware exp2,
the lse term for the cancellation in exp(S - lse), which a backward that recomputes P from lse has and a max-subtracting softmax
does not.  lse and D, for which the project had no bound, get max(1e-5, 8 yardstick) everywhere (lse is the logarithm of the sum
that `out` divides by; D inherits out's error times dh terms of dO, which the float32 yardstick measures).

A sequence with no valid key is outside the contract of the dense attention (its reference is NaN: a softmax over nothing), so the
mask patterns that would empty a sequence run on the lengths they leave a key in; every generator here keeps key 0 or names the
key it keeps."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, replace
from functools import lru_cache
from typing import Optional, Tuple

import torch

EDGE_LENS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
FLOOR_OUT, FLOOR_GRAD, FLOOR_BD_OUT, FLOOR_STAT = 1e-5, 2e-5, 3e-6, 1e-5
YARD_FACTOR, LSE_TERM = 8.0, 2.0 ** -22
SENTINEL = -1234.5625          # exactly representable; no kernel output of these cases comes near it
AB_GS, AB_DS, F16_MAX = 4096.0, 16384.0, 65504.0      # csrc/attention_bwd.hip: the lifts of dO and dS before the fp16 split
G_PLANES = 4096.0
MASKS = ("rand", "key0", "last", "no_last_tile", "no_first_tile")


@dataclass(frozen=True)
class Case:
    name: str
    lens: Tuple[int, ...]
    H: int = 2
    dh: int = 64
    mask: Optional[str] = None      # one of MASKS
    gap: int = 0                    # rows that belong to no sequence: before, between and after the sequences
    permute: bool = False           # sequence order != row order (seq_off not monotonic)
    max_len: Optional[int] = None   # None: max(lens)
    do: Tuple[str, float] = ("normal", 1e-3)      # dO ~ g N(0, 1) or uniform in [-g, g]
    shift: int = 0                  # m: q += |m| / 8 per dim, k += sign(m) |m| / 8 (m < 0: all logits negative)
    mult: float = 1.0               # q, k *= mult
    hard: bool = False
    blockdiag: bool = False         # lens = (L,) * n_frag

    @property
    def scale(self) -> float:
        return 1.0 / math.sqrt(self.dh)

    @property
    def T(self) -> int:
        return self.max_len or max(self.lens)


def with_path(c: Case, path: str) -> Case:
    """the four dense kernel paths: dh64 (unmasked: split-f16), dh64m, dh32, dh32m (exact fp32)"""
    dh = 64 if path.startswith("dh64") else 32
    mask = c.mask or ("rand" if path.endswith("m") else None)
    return replace(c, name=f"{c.name}-{path}", dh=dh, mask=mask)


DENSE_PATHS = ("dh64", "dh64m", "dh32", "dh32m")


def _e_variants():
    """(suffix, fields): the logit-range sweep"""
    v = [(f"neg{m}", dict(shift=-m)) for m in (8, 10, 12)] + [(f"pos{m}", dict(shift=m)) for m in (8, 12)]
    v.append(("x4", dict(mult=4.0)))
    v.append(("neg6_do1", dict(shift=-6, do=("normal", 1.0))))
    return v


def _d_variants():
    return [(f"g{g:g}", dict(do=("uniform", g), hard=g < 1e-4)) for g in (1e-6, 1e-3, 1.0, 15.0)]


def _dense_table():
    t = {}
    a = [Case("A", EDGE_LENS), Case("A_h3", (33, 1, 129), H=3)]
    b = [Case("B", EDGE_LENS, gap=5, permute=True, max_len=384)]
    d = [Case(f"D_{s}", (33, 129, 257), **f) for s, f in _d_variants()]
    e = [Case(f"E_{s}", (50, 129), hard=True, **f) for s, f in _e_variants()]
    for c in a + b + d + e:
        for p in DENSE_PATHS:
            cp = with_path(c, p)
            t[cp.name] = cp
    for m in MASKS:                 # C: the masked form of A, on the lengths the pattern leaves a valid key in
        lens = tuple(n for n in EDGE_LENS if n > 32) if m in ("no_last_tile", "no_first_tile") else EDGE_LENS
        for dh in (64, 32):
            t[f"C_{m}-dh{dh}m"] = Case(f"C_{m}-dh{dh}m", lens, dh=dh, mask=m)
    return t


BD_LS = (1, 2, 7, 8, 9, 16, 17, 25, 31, 32)


def _bd_table():
    t = {}
    for L in BD_LS:                 # I: 6 pairs (not a multiple of the mfma kernel's 4 per workgroup) and a single pair
        t[f"I_L{L}_f3h2"] = Case(f"I_L{L}_f3h2", (L,) * 3, H=2, blockdiag=True)
        t[f"I_L{L}_f1h1"] = Case(f"I_L{L}_f1h1", (L,), H=1, blockdiag=True)
    for L in (7, 32):               # J: the magnitude and logit sweeps
        for s, f in _d_variants():
            t[f"J_L{L}_{s}"] = Case(f"J_L{L}_{s}", (L,) * 3, blockdiag=True, **f)
        for s, f in _e_variants():
            t[f"J_L{L}_{s}"] = Case(f"J_L{L}_{s}", (L,) * 3, blockdiag=True, hard=True, **f)
    return t


DENSE = _dense_table()
BLOCKDIAG = _bd_table()
F_CASES = ("A-dh64", "E_neg12-dh64")        # parts and planes: the split-f16 path
K_LS = (1, 17, 32)
CHILD_DENSE = [n for n in DENSE if n[0] in "AC"]
CHILD_BD = [n for n in BLOCKDIAG if n[0] == "I"]
CROSS_CHECKS = (("DENSE_F32", "BD_F32"),          # ops.attention_cross_check names: dense fp32 <64> unmasked, block-diagonal fp32 mfma
                ("BD_F32", "BD_SCALAR"))          # block-diagonal scalar kernels


# ------------------------------------------------------------------------------------------------------------ inputs
def layout(c: Case):
    """-> rows, seq_off (list, in sequence order), inside (bool [rows]: the row belongs to a sequence)"""
    n = len(c.lens)
    order = list(range(n))
    if c.permute:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(n + 17)).tolist()
        assert order != sorted(order)
    off, row = [0] * n, c.gap
    for s in order:                 # physical order of the sequences
        off[s] = row
        row += c.lens[s] + c.gap
    inside = torch.zeros(row, dtype=torch.bool)
    for s in range(n):
        inside[off[s]:off[s] + c.lens[s]] = True
    return row, off, inside


def make_mask(c: Case, g: torch.Generator) -> Optional[torch.Tensor]:
    """bool [n_seq, T]; columns at and past a sequence's length carry random values (nothing may depend on them)"""
    if c.mask is None:
        return None
    kv = torch.rand(len(c.lens), c.T, generator=g) < 0.5
    for s, n in enumerate(c.lens):
        if c.mask == "rand":
            kv[s, :n] = torch.rand(n, generator=g) < 0.6
            kv[s, 0] = True
        elif c.mask == "key0":
            kv[s, :n] = False
            kv[s, 0] = True
        elif c.mask == "last":
            kv[s, :n] = False
            kv[s, n - 1] = True
        elif c.mask == "no_last_tile":
            kv[s, :n] = True
            kv[s, 32 * ((n - 1) // 32):n] = False
        elif c.mask == "no_first_tile":
            kv[s, :n] = True
            kv[s, :32] = False
        else:
            raise ValueError(c.mask)
        assert bool(kv[s, :n].any()), (c.name, s)
    return kv


@lru_cache(maxsize=None)
def inputs(c: Case):
    """-> dict: qkv float32 [rows, 3 H dh], dout float32 [rows, H dh], groups [(off, len)], inside, key_valid (bool or None).
    Cached: treat as read-only."""
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    rows, off, inside = layout(c)
    C = c.H * c.dh
    qkv = torch.randn(rows, 3 * C, generator=g)
    qkv[:, :2 * C] *= c.mult
    if c.shift:
        a = abs(c.shift) / 8.0
        qkv[:, :C] += a
        qkv[:, C:2 * C] += a if c.shift > 0 else -a
    kind, gmag = c.do
    dout = torch.randn(rows, C, generator=g) * gmag if kind == "normal" else (torch.rand(rows, C, generator=g) * 2 - 1) * gmag
    return dict(qkv=qkv, dout=dout, groups=list(zip(off, c.lens)), inside=inside, key_valid=make_mask(c, g))


def reference(c: Case, dtype=torch.float64):
    """softmax(q k^T scale + key mask) v per (group, head) and its gradients by autograd, computed in `dtype` from the float32 inputs
    -> dict: out [rows, C], lse [rows, H], D [rows, H], dqkv [rows, 3C] (zero outside the groups), unc {(part, group): [H]}"""
    inp = inputs(c)
    H, dh, C = c.H, c.dh, c.H * c.dh
    x = inp["qkv"].to(dtype).clone().requires_grad_(True)
    g = inp["dout"].to(dtype)
    rows = x.shape[0]
    out = torch.zeros(rows, C, dtype=dtype)
    lse = torch.zeros(rows, H, dtype=dtype)
    unc = {}
    loss = x.sum() * 0
    for s, (o, n) in enumerate(inp["groups"]):
        q, k, v = (x[o:o + n, i * C:(i + 1) * C].reshape(n, H, dh).transpose(0, 1) for i in range(3))       # [H, n, dh]
        sc = q @ k.transpose(1, 2) * c.scale
        if inp["key_valid"] is not None:
            sc = sc.masked_fill(~inp["key_valid"][s, :n][None, None, :], -math.inf)
        l = torch.logsumexp(sc, -1)
        og = (torch.exp(sc - l[..., None]) @ v).transpose(0, 1).reshape(n, C)
        loss = loss + (og * g[o:o + n]).sum()
        out[o:o + n] = og.detach()
        lse[o:o + n] = l.detach().t()
        gh = g[o:o + n].reshape(n, H, dh).transpose(0, 1)
        dp = (gh @ v.detach().transpose(1, 2)).abs().amax((1, 2)) * c.scale
        unc["dq", s] = dp * k.detach().abs().amax((1, 2))
        unc["dk", s] = dp * q.detach().abs().amax((1, 2))
    loss.backward()
    D = (g * out).reshape(rows, H, dh).sum(-1)
    return dict(out=out, lse=lse, D=D, dqkv=x.grad.detach(), unc=unc)


@lru_cache(maxsize=None)
def refs(c: Case):
    """(float64 reference, float32 yardstick run); cached: treat as read-only"""
    return reference(c, torch.float64), reference(c, torch.float32)


# ------------------------------------------------------------------------------------------------------------ error report
PARTS = ("out", "dq", "dk", "dv")


def block_errors(c: Case, got: dict, ref: dict):
    """got: tensors under out / dqkv / lse / D (any subset) -> {(quantity, group, head): relative error as the docstring defines it}"""
    H, dh, C = c.H, c.dh, c.H * c.dh
    res = {}
    for s, (o, n) in enumerate(inputs(c)["groups"]):
        blocks = []
        for name in ("out", "fwd"):          # fwd: the inference forward of the same attention, against the same reference
            if name in got:
                blocks.append((name, got[name][o:o + n], ref["out"][o:o + n]))
        if "dqkv" in got:
            for i, part in enumerate(("dq", "dk", "dv")):
                blocks.append((part, got["dqkv"][o:o + n, i * C:(i + 1) * C], ref["dqkv"][o:o + n, i * C:(i + 1) * C]))
        for part, a, b in blocks:
            b = b.double().reshape(n, H, dh)
            err = (a.double().reshape(n, H, dh) - b).abs().amax((0, 2))
            den = b.abs().amax((0, 2))
            if part in ("out", "fwd") and c.blockdiag:
                den = den.clamp_min(1.0)              # the block-diagonal forward's bound is 3e-6 max(1, |ref|)
            if part in ("dq", "dk"):
                den = torch.where(den > 0, den, ref["unc"][part, s].double())
            for h in range(H):
                res[part, s, h] = float(err[h] / den[h]) if math.isfinite(float(err[h])) else math.inf
        for stat in ("lse", "D"):
            if stat in got:
                b = ref[stat][o:o + n].double()
                err = ((got[stat][o:o + n].double() - b).abs() / b.abs().clamp_min(1.0)).amax(0)
                for h in range(H):
                    res[stat, s, h] = float(err[h]) if math.isfinite(float(err[h])) else math.inf
    return res


def floor_of(c: Case, quantity: str) -> float:
    if quantity in ("lse", "D"):
        return FLOOR_STAT
    if quantity == "out":
        return FLOOR_BD_OUT if c.blockdiag else FLOOR_OUT
    return FLOOR_GRAD


def yardstick(c: Case):
    """{block: error of the float32 CPU autograd run against float64}"""
    r64, r32 = refs(c)
    return block_errors(c, {"out": r32["out"], "dqkv": r32["dqkv"], "lse": r32["lse"], "D": r32["D"]}, r64)


def bounds(c: Case):
    """{block: bound}: the floor, and for the hard cases (and lse / D everywhere) what the yardstick allows"""
    r64 = refs(c)[0]
    yard = yardstick(c)
    res = {}
    for (quantity, s, h), y in yard.items():
        fl = floor_of(c, quantity)
        if quantity in ("lse", "D"):
            res[quantity, s, h] = max(fl, YARD_FACTOR * y)
        elif c.hard:
            o, n = inputs(c)["groups"][s]
            res[quantity, s, h] = max(fl, YARD_FACTOR * y + float(r64["lse"][o:o + n, h].abs().max()) * LSE_TERM)
        else:
            res[quantity, s, h] = fl
    return res


def report(c: Case, got: dict):
    """-> dict: finite (every tensor in got), worst {quantity: dict(block, err, yard, bound)} (the block with the largest err / bound),
    ok (every block within its bound)"""
    r64 = refs(c)[0]
    finite = all(bool(torch.isfinite(t[inputs(c)["inside"]]).all()) for t in got.values())
    errs, yard, bnd = block_errors(c, got, r64), yardstick(c), bounds(c)
    worst = {}
    for blk, e in errs.items():
        w = worst.get(blk[0])
        key = ("out",) + blk[1:] if blk[0] == "fwd" else blk
        if w is None or e / bnd[key] > w["err"] / w["bound"]:
            worst[blk[0]] = dict(block=f"{blk[0]}[group {blk[1]} (len {c.lens[blk[1]]}), head {blk[2]}]", err=e, yard=yard[key], bound=bnd[key])
    return dict(case=c.name, finite=finite, worst=worst, ok=finite and all(w["err"] <= w["bound"] for w in worst.values()))


def describe(rep: dict) -> str:
    """one line per quantity: the figures a test prints before it asserts (and profiles/attn_edges_errors.txt records)"""
    lines = []
    for qn, w in rep["worst"].items():
        ratio = w["err"] / max(w["yard"], 2.0 ** -24)
        lines.append(f"attn_edges {rep['case']:<22} {qn:<4} err {w['err']:.3e} yard {w['yard']:.3e} ratio {ratio:8.2f} bound {w['bound']:.3e}"
                     f" {'ok  ' if w['err'] <= w['bound'] else 'OVER'} worst {w['block']}")
    return "\n".join(lines)


def overflow_margin(c: Case):
    """largest lifted dS that ab_dq_f16_body (csrc/attention_bwd.hip) forms for a zero-staged pad key, over the query rows:
    exp(-lse_q) |v_{T-1} . dO_q - D_q| scale 2^14, float64 from the reference -> (max over all queries, fraction of queries at or
    over the fp16 overflow threshold 65520)"""
    inp, r = inputs(c), refs(c)[0]
    H, dh, C = c.H, c.dh, c.H * c.dh
    vals = []
    for o, n in inp["groups"]:
        if n % 32 == 0:
            continue
        v_last = inp["qkv"][o + n - 1, 2 * C:].double().reshape(H, dh)
        dp = (inp["dout"][o:o + n].double().reshape(n, H, dh) * v_last[None]).sum(-1)
        vals.append((torch.exp(-r["lse"][o:o + n]) * (dp - r["D"][o:o + n]).abs() * c.scale * AB_DS).reshape(-1))
    vals = torch.cat(vals)
    return float(vals.max()), float((vals >= 65520.0).double().mean())


# ------------------------------------------------------------------------------------------------------------ GPU runs
def _device_mask(kv: Optional[torch.Tensor], dev):
    """uint8 key_valid as a column slice of a wider tensor (row stride > max_len); what lies outside the slice is 'valid'"""
    if kv is None:
        return None
    wide = torch.ones(kv.shape[0], kv.shape[1] + 19, dtype=torch.uint8, device=dev)
    sl = wide[:, 3:3 + kv.shape[1]]
    sl.copy_(kv.to(torch.uint8))
    assert sl.stride(0) > kv.shape[1]
    return sl


def run_dense(c: Case, dev):
    """forward (training form) and backward through the wrappers, into sentinel-filled buffers
    -> got (CPU tensors out, fwd, lse, D, dqkv), flags (fwd_equal, outside_kept, masked_zero), dev (the GPU tensors, for F / G)"""
    from pfpp_hip import ops, train_ops as T

    inp = inputs(c)
    H, dh, C = c.H, c.dh, c.H * c.dh
    qkv, dout = inp["qkv"].to(dev), inp["dout"].to(dev)
    rows = qkv.shape[0]
    so = torch.tensor([o for o, _ in inp["groups"]], dtype=torch.int32, device=dev)
    sl = torch.tensor(c.lens, dtype=torch.int32, device=dev)
    kv = _device_mask(inp["key_valid"], dev)

    def filled(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)

    out, lse = T.attn_dense_train(qkv, so, sl, c.T, H, dh, c.scale, key_valid=kv, out=filled(rows, C), lse=filled(rows, H))
    # the inference forward: as dispatched (launches of <= 64 workgroups at dh 64 go to attn_dense_short_kernel, which splits the keys
    # over the waves and so sums in another order: other bits by design, held to the bound of `out`), and with that kernel switched
    # off for the call (NO_SHORT, on top of what the caller has set), where it is the training forward's kernel and must give its bits
    fwd = ops.attn_dense(qkv, so, sl, c.T, H, dh, c.scale, kv, out=filled(rows, C))
    with ops.attention_cross_check("NO_SHORT"):
        walk = ops.attn_dense(qkv, so, sl, c.T, H, dh, c.scale, kv, out=filled(rows, C))
    dvec = filled(rows, H)
    dqkv = T.attn_dense_bwd(qkv, out, dout, lse, so, sl, c.T, H, dh, c.scale, key_valid=kv, out=filled(rows, 3 * C), dvec=dvec)
    torch.cuda.synchronize()
    outside = ~inp["inside"].to(dev)
    flags = dict(fwd_equal=torch.equal(out, walk),
                 outside_kept=all(bool((t[outside] == SENTINEL).all()) for t in (out, fwd, walk, lse, dvec, dqkv)), masked_zero=True)
    if kv is not None:
        for s, (o, n) in enumerate(inp["groups"]):
            bad = ~inp["key_valid"][s, :n].to(dev)
            flags["masked_zero"] &= bool((dqkv[o:o + n, C:][bad] == 0.0).all())
    got = dict(out=out.cpu(), fwd=fwd.cpu(), lse=lse.cpu(), D=dvec.cpu(), dqkv=dqkv.cpu())
    return got, flags, dict(qkv=qkv, dout=dout, out=out, lse=lse, dvec=dvec, dqkv=dqkv, so=so, sl=sl)


def run_blockdiag(c: Case, dev):
    from pfpp_hip import ops, train_ops as T

    inp = inputs(c)
    qkv, dout = inp["qkv"].to(dev), inp["dout"].to(dev)
    L, n_frag = c.lens[0], len(c.lens)
    out = ops.attn_blockdiag(qkv, n_frag, L, c.H, c.dh, c.scale)
    dqkv = T.attn_blockdiag_bwd(qkv, dout, n_frag, L, c.H, c.dh, c.scale)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), dqkv=dqkv.cpu()), dict(qkv=qkv, dout=dout, dqkv=dqkv)
