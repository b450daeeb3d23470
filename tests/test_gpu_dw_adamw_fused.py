"""GPU (-m gpu): AdamW in the epilogue of the grouped weight-gradient launch (pfpp_gemm_dw_group with pfpp_dw_update blocks,
csrc/gemm_pl.hip) and the remainder launch pfpp_adamw_ranges (csrc/train_ops.hip), through the C entry points, against today's
sequence: the plain grouped launch onto a zeroed gradient buffer followed by pfpp_adamw_guarded(zero_grad=1) per matrix.

Shapes: contraction lengths (token rows) {1, 31, 33, 97} around the 32-deep contraction step; matrices (n_out, n_in) in
{(8, 8), (256, 128), (264, 136), (520, 72)}: smaller than, equal to, one 8-wide group beyond and several tiles of the 256 x 128
tile; two to six jobs per launch; zero and non-zero moments; step 1 and step 7.  Every comparison is in bits.

The sign of a zero gradient.  The plain job stores ((acc * alpha) + 0.0f) + 0.0f (no bias, then the zeroed residual); the update
epilogue forms the same expression, so a zero gradient is +0 on both sides ((-0) + (+0) = +0 under round-to-nearest) and there
is no representable difference left to argue about.  Even if one side did keep a -0: with g = -0 against g = +0 and m, v >= 0
from a previous step, g * g = +0 both times (v equal); g - m = -m for m > 0 (equal), and for m = +0 it is -0 against +0, but
fma(w1, d, +0) = +0 for d = +-0 (m equal); p sees g only through m and v.  So it could not reach p, m or v either way.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

HP = dict(lr=2e-4, beta1=0.95, beta2=0.999, eps=1e-8, weight_decay=1e-2)      # (a weight decay that does not round 1 - lr wd to 1)
GUARD = 64                      # sentinel elements in front of and behind every matrix of every buffer
# share of updated parameters whose bits must differ from before.  An update leaves p where it was only if the Adam step cancels the
# weight decay to within half an ulp of p: a window of ~6e-8 |p| in a step spread over ~6e-5 (lr x m / sqrt(v) of the moments used
# here), i.e. about one element in a thousand; ten times that is allowed.  (Equality with today's sequence is the actual check; this
# only says that both sides did something.)
MOVED = 0.99
G_DY = 1024.0                   # scale of the dY planes (a power of two, as the engine's gradient scale)
MATS = {"a": (8, 8), "b": (256, 128), "c": (264, 136), "d": (520, 72)}
# name -> (contraction length, matrices, moments non-zero, optimizer step)
CASES = {
    "k1_two_jobs_step1": (1, "ab", False, 1),
    "k31_three_jobs_step7": (31, "cda", True, 7),
    "k33_four_jobs_step1": (33, "bcda", True, 1),
    "k97_six_jobs_step7": (97, "abcdab", False, 7),
    "k97_five_jobs_step7": (97, "dcbad", True, 7),
}


def _planes(t, scale):
    v = t * scale
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    return hi, lo


class State:
    """one flat buffer per role, the matrices GUARD elements apart; dY / X planes with two NaN rows behind the contraction"""

    def __init__(self, dev, K, mats, nonzero, seed, bad=None):
        g = torch.Generator().manual_seed(seed)
        self.K, self.shapes = K, [MATS[c] for c in mats]
        self.off, pos = [], GUARD
        for M, N in self.shapes:
            self.off.append(pos)
            pos += (M * N + GUARD + 7) // 8 * 8
        self.total = pos
        self.p = torch.randn(pos, generator=g).to(dev)
        self.m = (torch.randn(pos, generator=g) * 1e-3 if nonzero else torch.zeros(pos)).to(dev)
        self.v = (torch.rand(pos, generator=g) * 1e-5 if nonzero else torch.zeros(pos)).to(dev)
        self.hi, self.lo = _planes(self.p, 1.0)
        self.gw = torch.zeros(pos, device=dev)
        self.gb = torch.zeros(pos, device=dev)          # bias sums of job j at off[j] (M of them)
        self.ovf = torch.zeros(2, dtype=torch.int32, device=dev)
        self.dy, self.x = [], []
        for j, (M, N) in enumerate(self.shapes):
            dy = torch.randn(K + 2, M, generator=g) * 3e-3
            x = torch.randn(K + 2, N, generator=g)
            dh, dl = _planes(dy, G_DY)
            xh, xl = _planes(x, 1.0)
            if bad is not None and bad[0] == j:
                dh[bad[1], bad[2]] = float("inf")
            for pl in (dh, dl, xh, xl):
                pl[K:] = float("nan")
            self.dy.append((dh.to(dev), dl.to(dev)))
            self.x.append((xh.to(dev), xl.to(dev)))

    def roles(self):
        return dict(p=self.p, m=self.m, v=self.v, hi=self.hi, lo=self.lo, gw=self.gw, gb=self.gb, ovf=self.ovf)


def _launch(st, step, fused, gw_fill=None):
    """the grouped launch (+ today's AdamW launches when not fused) on `st`, in place"""
    from pfpp_hip import _lib
    from pfpp_hip._lib import DwJob, DwUpdate, PlanesC

    lib = _lib.load()
    n = len(st.shapes)
    jobs, upd = (DwJob * n)(), (DwUpdate * n)()
    bc1, bc2 = 1.0 - HP["beta1"] ** step, 1.0 - HP["beta2"] ** step
    if gw_fill is not None:
        st.gw.fill_(gw_fill)
    for j, (M, N) in enumerate(st.shapes):
        o = st.off[j]
        gb = st.gb[o:o + M].data_ptr() if j != 1 else None          # one job without bias sums
        jobs[j] = DwJob(PlanesC(st.dy[j][0].data_ptr(), st.dy[j][1].data_ptr(), G_DY), PlanesC(st.x[j][0].data_ptr(), st.x[j][1].data_ptr(), 1.0),
                        st.gw[o:].data_ptr(), gb, M, N)
        if fused:
            upd[j] = DwUpdate(st.p[o:].data_ptr(), st.m[o:].data_ptr(), st.v[o:].data_ptr(), st.hi[o:].data_ptr(), st.lo[o:].data_ptr(),
                              HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], bc1, bc2, 1.0, st.ovf.data_ptr())
            jobs[j].upd = C.pointer(upd[j])
    _lib.check(lib.pfpp_gemm_dw_group(jobs, n, st.K, 0, None), "pfpp_gemm_dw_group")
    name = lib.pfpp_last_gemm_kernel().decode()
    if not fused:
        for j, (M, N) in enumerate(st.shapes):
            o = st.off[j]
            _lib.check(lib.pfpp_adamw_guarded(st.p[o:].data_ptr(), st.gw[o:].data_ptr(), st.m[o:].data_ptr(), st.v[o:].data_ptr(),
                                              st.hi[o:].data_ptr(), st.lo[o:].data_ptr(), M * N, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                                              HP["weight_decay"], bc1, bc2, 1.0, 1, st.ovf.data_ptr(), None), "pfpp_adamw_guarded")
    torch.cuda.synchronize()
    return name


@functools.lru_cache(maxsize=None)
def _pair(case, bad=None):
    """(initial state, unfused result, fused result, fused result of a repeat launch) of a case; computed once, never modified"""
    dev = torch.device("cuda:0")
    K, mats, nonzero, step = CASES[case]
    mk = lambda: State(dev, K, mats, nonzero, seed=len(case) + K, bad=bad)
    init, ref, fus, rep = mk(), mk(), mk(), mk()
    assert _launch(ref, step, False) == "gemm_pl_dwgroup_kernel<2, 2, 4, 2, 3>"
    assert _launch(fus, step, True, gw_fill=123.0) == "gemm_pl_dwgroup_kernel<2, 2, 4, 2, 3, true>"
    _launch(rep, step, True, gw_fill=123.0)
    return init, ref, fus, rep


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32), b.view(torch.int16 if b.dtype == torch.float16 else torch.int32))


def _matrix_mask(st, dev):
    mask = torch.zeros(st.total, dtype=torch.bool, device=dev)
    for o, (M, N) in zip(st.off, st.shapes):
        mask[o:o + M * N] = True
    return mask


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_update_equals_grouped_launch_then_adamw_in_bits(dev, hip_lib, case):
    """p, m, v, hi, lo after the fused launch == after the plain grouped launch onto a zeroed g followed by pfpp_adamw_guarded(zero_grad),
    in bits; so are the bias sums; the parameters moved; a repeat launch from the same state gives the same bits"""
    init, ref, fus, rep = _pair(case)
    for role in ("p", "m", "v", "hi", "lo", "gb", "ovf"):
        assert _same_bits(ref.roles()[role], fus.roles()[role]), (case, role)
        assert _same_bits(rep.roles()[role], fus.roles()[role]), (case, role, "repeat launch")
    mask = _matrix_mask(fus, dev)
    assert float((fus.p[mask] != init.p[mask]).float().mean()) > MOVED and float((fus.v[mask] > 0).float().mean()) > MOVED
    assert int(fus.ovf[0]) == 0 and int(fus.ovf[1]) == 0
    assert float(ref.gw.abs().max()) == 0.0                     # (today's path: accumulated, consumed and cleared)


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_update_leaves_the_gradient_buffer_and_the_guards_alone(dev, hip_lib, case):
    """the gw ranges (filled with a sentinel before the launch) are neither read into the result nor written; the GUARD elements in
    front of and behind every matrix of p, m, v, hi, lo keep their bits; bias sums land in their M elements only"""
    init, ref, fus, _ = _pair(case)
    assert bool((fus.gw == 123.0).all())
    guard = ~_matrix_mask(fus, dev)
    for role in ("p", "m", "v", "hi", "lo"):
        assert _same_bits(fus.roles()[role][guard], init.roles()[role][guard]), (case, role)
    bias = torch.zeros(fus.total, dtype=torch.bool, device=dev)
    for j, (o, (M, N)) in enumerate(zip(fus.off, fus.shapes)):
        if j != 1:
            bias[o:o + M] = True
    assert float(fus.gb[~bias].abs().max()) == 0.0 and bool((fus.gb[bias] != 0).any())


@pytest.mark.parametrize("case,bad", [("k33_four_jobs_step1", (1, 17, 259)), ("k97_five_jobs_step7", (0, 96, 519)), ("k31_three_jobs_step7", (2, 0, 7))])
def test_one_non_finite_dy_element_skips_exactly_its_parameters(dev, hip_lib, case, bad):
    """dY[k, c] = inf in job j makes row c of that job's gradient non-finite (inf or NaN, n_in elements): exactly those parameters keep
    p, m, v and their planes, the flag is raised with that count, every other element is updated as in the clean launch - and all of
    it equals today's sequence on the same input in bits"""
    init, ref, fus, _ = _pair(case, bad)
    _, _, clean, _ = _pair(case)
    j, _, c = bad
    M, N = fus.shapes[j]
    o = fus.off[j]
    hit = torch.zeros(fus.total, dtype=torch.bool, device=dev)
    hit[o + c * N: o + (c + 1) * N] = True
    for role in ("p", "m", "v", "hi", "lo"):
        got, was, want = fus.roles()[role], init.roles()[role], clean.roles()[role]
        assert _same_bits(got[hit], was[hit]), (case, role, "a skipped element changed")
        assert _same_bits(got[~hit], want[~hit]), (case, role, "an element outside the row differs from the clean launch")
        assert _same_bits(got, ref.roles()[role]), (case, role, "differs from today's sequence")
    assert fus.ovf.tolist() == [1, N] and ref.ovf.tolist() == [1, N]


def test_jobs_with_and_without_an_update_block_share_a_launch(dev, hip_lib):
    """a job without the update block behaves as today next to jobs that carry one: its gradient is accumulated (onto a non-zero
    buffer here) and its parameters are not touched"""
    from pfpp_hip import _lib
    from pfpp_hip._lib import DwJob, DwUpdate, PlanesC

    lib = _lib.load()
    K, mats, step = 33, "cb", 7
    mixed, want_gw1 = State(dev, K, mats, True, 5), State(dev, K, mats, True, 5)      # want_gw1: both jobs plain, for job 1's gradient
    for st in (mixed, want_gw1):
        st.gw.fill_(0.25)
    n = 2
    jobs, upd = (DwJob * n)(), (DwUpdate * n)()
    bc1, bc2 = 1.0 - HP["beta1"] ** step, 1.0 - HP["beta2"] ** step
    for st, with_upd in ((want_gw1, (False, False)), (mixed, (True, False))):
        for j, (M, N) in enumerate(st.shapes):
            o = st.off[j]
            jobs[j] = DwJob(PlanesC(st.dy[j][0].data_ptr(), st.dy[j][1].data_ptr(), G_DY), PlanesC(st.x[j][0].data_ptr(), st.x[j][1].data_ptr(), 1.0),
                            st.gw[o:].data_ptr(), None, M, N)
            if with_upd[j]:
                upd[j] = DwUpdate(st.p[o:].data_ptr(), st.m[o:].data_ptr(), st.v[o:].data_ptr(), st.hi[o:].data_ptr(), st.lo[o:].data_ptr(),
                                  HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], bc1, bc2, 1.0, st.ovf.data_ptr())
                jobs[j].upd = C.pointer(upd[j])
        _lib.check(lib.pfpp_gemm_dw_group(jobs, n, K, 0, None), "pfpp_gemm_dw_group")
        torch.cuda.synchronize()
    o1, (M1, N1) = mixed.off[1], mixed.shapes[1]
    init = State(dev, K, mats, True, 5)
    assert _same_bits(mixed.gw[o1:o1 + M1 * N1], want_gw1.gw[o1:o1 + M1 * N1]) and bool((mixed.gw[o1:o1 + M1 * N1] != 0.25).any())
    for role in ("p", "m", "v", "hi", "lo"):
        assert _same_bits(mixed.roles()[role][o1:], init.roles()[role][o1:]), role
    o0, (M0, N0) = mixed.off[0], mixed.shapes[0]
    assert bool((mixed.gw[:o1] == 0.25).all()) and float((mixed.p[o0:o0 + M0 * N0] != init.p[o0:o0 + M0 * N0]).float().mean()) > MOVED


def test_update_blocks_of_one_launch_must_agree(dev, hip_lib):
    """refused before any launch: update blocks with different hyper-parameters, a block without p"""
    from pfpp_hip import _lib
    from pfpp_hip._lib import DwJob, DwUpdate, PlanesC

    lib = _lib.load()
    st = State(dev, 8, "aa", False, 1)
    jobs, upd = (DwJob * 2)(), (DwUpdate * 2)()
    for j in range(2):
        o = st.off[j]
        jobs[j] = DwJob(PlanesC(st.dy[j][0].data_ptr(), st.dy[j][1].data_ptr(), G_DY), PlanesC(st.x[j][0].data_ptr(), st.x[j][1].data_ptr(), 1.0),
                        None, None, 8, 8)
        upd[j] = DwUpdate(st.p[o:].data_ptr(), st.m[o:].data_ptr(), st.v[o:].data_ptr(), None, None, 2e-4 * (1 + j), 0.9, 0.99, 1e-8, 0.0, 0.1, 0.01,
                          1.0, None)
        jobs[j].upd = C.pointer(upd[j])
    assert lib.pfpp_gemm_dw_group(jobs, 2, 8, 0, None) != 0 and b"share" in lib.pfpp_last_error()
    upd[1].lr = upd[0].lr
    upd[1].p = None
    assert lib.pfpp_gemm_dw_group(jobs, 2, 8, 0, None) != 0
    torch.cuda.synchronize()
    init = State(dev, 8, "aa", False, 1)
    assert _same_bits(st.p, init.p)


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_remainder_launch_equals_adamw_guarded_over_the_same_ranges(dev, hip_lib, zero_grad):
    """pfpp_adamw_ranges over a table of (offset, length) ranges - one element, odd lengths, more than one workgroup, an empty range,
    unaligned offsets - == pfpp_adamw_guarded over each range, in bits: p, m, v, planes, the gradient buffer (cleared inside the ranges
    with zero_grad, untouched outside), the flag and the count with a NaN and an inf gradient inside the ranges and one outside"""
    from pfpp_hip import _lib

    lib = _lib.load()
    ranges = [(3, 1), (16, 513), (600, 0), (777, 4097), (5000, 8)]
    total = 5100
    step = 7
    bc1, bc2 = 1.0 - HP["beta1"] ** step, 1.0 - HP["beta2"] ** step

    def mk():
        g = torch.Generator().manual_seed(11)
        p = torch.randn(total, generator=g).to(dev)
        gr = (torch.randn(total, generator=g) * 1e-2)
        gr[20], gr[900], gr[700] = float("nan"), float("inf"), float("nan")           # 700 lies outside every range
        m = (torch.randn(total, generator=g) * 1e-3).to(dev)
        v = (torch.rand(total, generator=g) * 1e-5).to(dev)
        hi, lo = _planes(p, 1.0)
        return dict(p=p, g=gr.to(dev), m=m, v=v, hi=hi, lo=lo, ovf=torch.zeros(2, dtype=torch.int32, device=dev))

    init, ref, got = mk(), mk(), mk()
    for o, n in ranges:
        if n:
            _lib.check(lib.pfpp_adamw_guarded(ref["p"][o:].data_ptr(), ref["g"][o:].data_ptr(), ref["m"][o:].data_ptr(), ref["v"][o:].data_ptr(),
                                              ref["hi"][o:].data_ptr(), ref["lo"][o:].data_ptr(), n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                                              HP["weight_decay"], bc1, bc2, 0.5, zero_grad, ref["ovf"].data_ptr(), None), "pfpp_adamw_guarded")
    off = (C.c_int64 * len(ranges))(*[o for o, _ in ranges])
    ln = (C.c_int64 * len(ranges))(*[n for _, n in ranges])
    _lib.check(lib.pfpp_adamw_ranges(got["p"].data_ptr(), got["g"].data_ptr(), got["m"].data_ptr(), got["v"].data_ptr(), got["hi"].data_ptr(),
                                     got["lo"].data_ptr(), off, ln, len(ranges), HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"],
                                     bc1, bc2, 0.5, zero_grad, got["ovf"].data_ptr(), None), "pfpp_adamw_ranges")
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool, device=dev)
    for o, n in ranges:
        inside[o:o + n] = True
    for role in ("p", "g", "m", "v", "hi", "lo", "ovf"):
        assert _same_bits(got[role], ref[role]), role
    for role in ("p", "g", "m", "v", "hi", "lo"):
        assert _same_bits(got[role][~inside], init[role][~inside]), role
    assert got["ovf"].tolist() == [1, 2]
    moved = inside.clone()
    moved[20] = moved[900] = False
    assert float((got["p"][moved] != init["p"][moved]).float().mean()) > MOVED and _same_bits(got["p"][[20, 900]], init["p"][[20, 900]])
    if zero_grad:
        assert float(got["g"][inside].abs().max()) == 0.0
    # the same table without the guard (overflow = NULL) == pfpp_adamw_zero per range
    ref2, got2 = mk(), mk()
    for st in (ref2, got2):
        st["g"].nan_to_num_(0.0, 0.0, 0.0)
    for o, n in ranges:
        if n:
            _lib.check(lib.pfpp_adamw_zero(ref2["p"][o:].data_ptr(), ref2["g"][o:].data_ptr(), ref2["m"][o:].data_ptr(), ref2["v"][o:].data_ptr(),
                                           ref2["hi"][o:].data_ptr(), ref2["lo"][o:].data_ptr(), n, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"],
                                           HP["weight_decay"], bc1, bc2, 0.5, zero_grad, None), "pfpp_adamw_zero")
    _lib.check(lib.pfpp_adamw_ranges(got2["p"].data_ptr(), got2["g"].data_ptr(), got2["m"].data_ptr(), got2["v"].data_ptr(), got2["hi"].data_ptr(),
                                     got2["lo"].data_ptr(), off, ln, len(ranges), HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"],
                                     bc1, bc2, 0.5, zero_grad, None, None), "pfpp_adamw_ranges")
    torch.cuda.synchronize()
    for role in ("p", "g", "m", "v", "hi", "lo"):
        assert _same_bits(got2[role], ref2[role]), role


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _batch(kind, dev):
    """-> (engine inputs, noise, latent points per fragment).  "golden": the golden batch, 2 puzzles, 28 fragments of 25 points, 700
    tokens.  "tiny": 2 puzzles of 2 fragments of 4 points, 16 tokens, seeded - the size at which the armed step is reproducible in bits:
    the LayerNorm backward adds one partial sum per workgroup with fp32 atomics, and here no target receives more than two of them
    (AdaLN rows: one workgroup per fragment, two fragments per puzzle; norm3's affine: workgroups of 8 rows, 16 rows), and two
    addends onto zero give the same sum in either order"""
    import numpy as np

    if kind == "golden":
        root = __import__("pathlib").Path(__file__).resolve().parent / "golden"
        g, t = np.load(root / "denoiser.npz"), np.load(root / "train.npz")
        inp = [torch.from_numpy(np.asarray(g[k])).to(dev) for k in ("x", "timesteps", "latent", "xyz", "part_valids", "scale", "ref_part")]
        return inp, torch.from_numpy(np.asarray(t["noise"])).to(dev), 25
    g = torch.Generator().manual_seed(3)
    B, P, L = 2, 2, 4
    ref = torch.zeros(B, P, dtype=torch.bool)
    ref[:, 0] = True
    inp = [torch.randn(B, P, 7, generator=g), torch.tensor([17, 801]), torch.randn(B, P, L, 64, generator=g),
           torch.randn(B, P, L, 3, generator=g) * 0.3, torch.ones(B, P), torch.rand(B, P, 1, generator=g) + 0.5, ref]
    return [v.to(dev) for v in inp], torch.randn(B, P, 7, generator=g).to(dev), L


@functools.lru_cache(maxsize=None)
def _engine_runs(kind):
    """three armed steps (zero_grad=True) of a 2-layer, width-256 engine (the narrowest the row-wise kernels take) on _batch(kind)
    with fused_update on and off, from the same state.  Asserted on the way: the fused engine really took the fused form and the
    other one did not, every layer's slice went early, the gradient buffer is all zero after each step either way, the overflow flag
    stays down.  -> ({fused: [(loss, params, exp_avg, exp_avg_sq, hi, lo) per step]}, the engine's FlatParams)"""
    from pfpp_hip.train import DenoiserTrainEngine
    from puzzlefusion_plusplus.denoiser.model.modules.denoiser_transformer import DenoiserTransformer

    dev = torch.device("cuda:0")
    inp, noise, L = _batch(kind, dev)
    cfg = _NS(model=_NS(embed_dim=256, out_channels=7, num_layers=2, num_heads=4, num_dim=64, num_point=L))
    torch.manual_seed(7)
    sd = DenoiserTransformer(cfg).state_dict()
    res = {}
    for fused in (True, False):
        m = DenoiserTransformer(cfg)
        m.load_state_dict(sd)
        eng = DenoiserTrainEngine(m.to(dev), dropout=0.0, token_dropout=0.0)
        f = eng.flat
        snaps = []
        for step in range(3):
            f.zero_grad()
            eng.arm_optimizer(lr=2e-4, zero_grad=True, fused_update=fused)
            loss = eng.loss_and_grads(*inp, noise, seed=100 + step, train=True)
            args, _ = eng._cseq_static
            assert bool(args.opt_fused_dw) == fused
            assert set(f.layer_ranges) <= set(eng._early)
            eng.optimizer_step(lr=2e-4, zero_grad=True)
            torch.cuda.synchronize()
            assert f._clean and f._zero and float(f.grads.abs().max()) == 0.0
            snaps.append((float(loss), f.params.clone(), f.exp_avg.clone(), f.exp_avg_sq.clone(), f.hi.clone(), f.lo.clone()))
        assert eng.overflow_steps == 0
        res[fused] = snaps
    return res, f


# parameters whose gradient is summed with floating-point atomics by the LayerNorm backward (the AdaLN rows dmods and norm3's affine):
# the AdaLN tables and linears, which take their gradients from dmods, and norm3.  Their bits differ between two runs of the SAME form
NOISY = (".norm1.emb.weight", ".norm2.emb.weight", ".norm1.linear.weight", ".norm2.linear.weight", ".norm1.linear.bias",
         ".norm2.linear.bias", ".norm3.weight", ".norm3.bias")


def test_first_armed_engine_step_agrees_in_bits_where_the_step_is_reproducible(dev, hip_lib):
    """the golden batch (700 tokens: three row tiles of contraction steps, every matrix several tiles), after the first armed step
    from the same state, fused_update on against off: the loss, and parameter, both moments and both
    planes of EVERY parameter whose gradient the step computes reproducibly - all six matrices of both blocks, which the fused form
    updates in the weight-gradient launch's epilogue, their biases, which go through the remainder launch, the embeddings and the
    output heads - are equal in bits, and they all moved.  Left out: the parameters named in NOISY, whose gradients the LayerNorm
    backward sums with atomics at this size: two UNFUSED runs differ there as well (measured on one MI355X, 5,002,128 parameters:
    unfused against unfused 5,712 parameters and 380,554 first moments differ, fused against unfused 5,731 / 391,031, in both
    comparisons only parameters named in NOISY), which is why the three-step test below runs at the size where the step is
    reproducible"""
    res, f = _engine_runs("golden")
    a, b = res[True][0], res[False][0]
    assert a[0] == b[0]
    checked = 0
    for n in f.order:
        if n.endswith(NOISY):
            continue
        o, k = f.offset[n], f.named[n].numel()
        for what, x, y in zip(("params", "exp_avg", "exp_avg_sq", "hi", "lo"), a[1:], b[1:]):
            assert _same_bits(x[o:o + k], y[o:o + k]), (n, what, int((x[o:o + k] != y[o:o + k]).sum()))
        checked += k
    mats = [n for n in f.order if n.startswith("transformer_layers.") and n.endswith(".weight") and f.named[n].dim() == 2 and not n.endswith(NOISY)]
    assert len(mats) >= 12, mats
    for n in mats:
        o, k = f.offset[n], f.named[n].numel()
        assert float(a[3][o:o + k].max()) > 0.0, n                 # a second moment: the gradient arrived
    assert checked > f.numel // 2


def test_three_armed_engine_steps_fused_and_unfused_agree_in_bits(dev, hip_lib):
    """2 puzzles, 2 layers, width 256: three armed steps with fused_update on and off from the same state - the loss, and EVERY
    parameter, both moments and both planes, equal in bits after every step.  On the tiny batch of _batch(), where the armed step
    reproduces itself in bits run to run (at 700 tokens the parent does not: the order of the LayerNorm backward's atomics
    varies, and from the second step on every bit follows), so that a difference here is the fused form's.  The contraction of the
    weight gradients is 16 token rows, half a contraction step; the matrices are the width-256 blocks' ([768, 256] ... [256, 1024])."""
    res, f = _engine_runs("tiny")
    for step, (a, b) in enumerate(zip(res[True], res[False])):
        assert a[0] == b[0], (step, a[0], b[0])
        for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "hi", "lo"), a[1:], b[1:]):
            assert _same_bits(x, y), (step, name, int((x != y).sum()))
    for n in f.order:                    # every parameter of the blocks went on moving from step to step
        if n.startswith("transformer_layers.") and ".emb." not in n:
            o, k = f.offset[n], f.named[n].numel()
            assert not torch.equal(res[True][2][1][o:o + k], res[True][0][1][o:o + k]), n
