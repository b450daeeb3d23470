"""GPU: stage-1 pre-training of the VQ-VAE on the HIP kernels (pfpp_hip.vqvae_train, vqvae/model/fracture_ae.py).

Yardstick: float64 torch autograd on the oracle's restatements (set_abstraction(train=True) through pn2_encode, chamferdist's
bidirectional Chamfer distance) plus float64 restatements of quantizer.py:45-67 (both .detach()s) and of the decoder (pn2.py:71-81)
in this file.  The GPU's discrete choices (VQ codes, nearest-neighbour indices, the row that attains each neighbourhood's max) are fed into
the float64 run; every code that differs from float64's own choice must be a near-tie (gap < 1e-4).
"""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

pytestmark = pytest.mark.gpu

BETA = 0.25


def _fragments(n_puzzles=2, num_parts=6, first=0):
    from pfpp_hip import synthetic

    b = synthetic.make_batch(first, n_puzzles, num_points=1000, num_parts=num_parts)
    pv = b["part_valids"].bool()
    return b["part_pcs"][pv].contiguous(), b


def _model(kind, dev, sd):
    from pfpp_hip import config
    from puzzlefusion_plusplus.vqvae.model.modules.pn2 import PN2
    from puzzlefusion_plusplus.vqvae.model.modules.vq_vae import VQVAE

    cfg = config.vqvae_train_config(kind)
    if kind == "VQVAE":
        m = VQVAE(cfg)
        m.load_state_dict(sd)
    else:
        m = PN2(cfg)
        m.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("pn2.")})
    return m.to(dev).train()


def _lv_choices(lv):
    """the GPU's discrete choices of one train-mode level: the neighbourhood row that attains each channel's max (first nonzero row of
    pfpp_sa_pool_bwd with dout = 1; 0 where the max is 0 and no gradient passes) and the ReLU masks of the first two layers"""
    from pfpp_hip import train_ops as T
    from pfpp_hip import vqvae_train as V

    with torch.no_grad():
        y, bn = lv["y"][2], lv["sa"].mlp_bns[2]
        ones = torch.ones((y.shape[0] // lv["ns"], y.shape[1]), dtype=torch.float32, device=y.device)
        dh = V.sa_pool_bwd(y, lv["ns"], lv["mean"][2], lv["var"][2], bn.weight.detach(), bn.bias.detach(), ones)
        route = (dh.view(-1, lv["ns"], y.shape[1]) != 0).to(torch.uint8).argmax(1).cpu()
        masks = []
        for i in range(2):
            b = lv["sa"].mlp_bns[i]
            h = T.bn_apply(lv["y"][i], lv["mean"][i], lv["var"][i], b.weight.detach(), b.bias.detach())
            masks.append((h > 0).cpu())
    return route, masks


def _gpu_routes(eng, pcs):
    """the GPU's discrete choices of a train-mode forward: per level (_lv_choices), and the VQ codes"""
    with torch.no_grad():
        out, ctx = eng.forward(pcs)
        routes = [_lv_choices(lv) for lv in ctx.t["levels"]]
        codes = ctx.t.get("codes")
    return out, routes, (codes.cpu() if codes is not None else None)


def _sa64(sd64, pre, S, radius, nsample, xyz, pts, choice=None, gaps=None):
    """PointNetSetAbstraction.forward in float64 with train-mode BatchNorm (oracle.set_abstraction's arithmetic).  choice = the GPU's
    (route, masks): the ReLU masks of the first two layers and the neighbourhood max are taken from it, and `gaps` records how far
    each differing choice is from float64's own (|value| where a mask differs, max - value at the GPU's row)"""
    from oracle import pfpp_oracle as O

    new_xyz, new_points, _, _ = O.sample_and_group(S, radius, nsample, xyz, pts)
    h = new_points.permute(0, 3, 2, 1)
    Fn = h.shape[0]
    for i in range(3):
        h = Fnn.conv2d(h, sd64[f"{pre}.mlp_convs.{i}.weight"], sd64[f"{pre}.mlp_convs.{i}.bias"])
        h = Fnn.batch_norm(h, sd64[f"{pre}.mlp_bns.{i}.running_mean"], sd64[f"{pre}.mlp_bns.{i}.running_var"],
                           sd64[f"{pre}.mlp_bns.{i}.weight"], sd64[f"{pre}.mlp_bns.{i}.bias"], True, 0.1, 1e-5)
        sd64[f"{pre}.mlp_bns.{i}.num_batches_tracked"] += 1
        if choice is not None and i < 2:          # rows (f, s, k) -> [F, C, ns, S]
            m = choice[1][i].view(Fn, S, nsample, -1).permute(0, 3, 2, 1)
            if gaps is not None:
                diff = m != (h.detach() > 0)
                gaps["relu"] = max(gaps.get("relu", 0.0), h.detach()[diff].abs().max().item() if diff.any() else 0.0)
                gaps["relu_flips"] = gaps.get("relu_flips", 0) + int(diff.sum())
            h = h * m.to(h.dtype)
        else:
            h = Fnn.relu(h)
    if choice is None:
        out = torch.max(h, 2)[0]
    else:
        r = choice[0].view(Fn, S, h.shape[1]).permute(0, 2, 1)[:, :, None, :].long()
        out = torch.gather(h, 2, r).squeeze(2)
        if gaps is not None:
            gaps["max"] = max(gaps.get("max", 0.0), (h.detach().max(2)[0] - out.detach()).max().item())
    return new_xyz, out.permute(0, 2, 1)


def _pn2_encode64(sd64, pcs64, routes=None, gaps=None):
    """PN2.encode in float64 (choices from the GPU when `routes` is given, float64's own otherwise)"""
    from oracle import pfpp_oracle as O

    xyz, pts = pcs64, None
    for k, (name, npoint, radius, nsample) in enumerate(O.SA_CFG):
        xyz, pts = _sa64(sd64, f"pn2.{name}", npoint or 25, radius, nsample, xyz, pts, None if routes is None else routes[k], gaps)
    g = Fnn.conv1d(pts.permute(0, 2, 1), sd64["pn2.conv6.weight"], sd64["pn2.conv6.bias"])
    return g.permute(0, 2, 1), xyz


def _sd64(sd):
    return {k: (v.double().clone().requires_grad_(True) if (v.is_floating_point() and "running_" not in k) else v.clone().double()
                if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def _nearest64(src, dst):
    """float64 squared distances [F, n, m] per fragment -> (own nearest index [F, n], the distance matrix list)"""
    out = []
    for f in range(src.shape[0]):
        d = ((src[f][:, None, :] - dst[f][None, :, :]) ** 2).sum(-1)
        out.append(d)
    return out


def _f64_loss(sd64, pcs64, codes=None, nn=None, vq=True, routes=None, gaps=None):
    """total_loss of VQVAE / PN2 in float64 -> (total, cd, emb, perplexity, z_e).  codes / nn = (i_src, i_tgt) / routes: the GPU's
    choices (recorded in `gaps` against float64's own), or None for float64's own"""
    z_e, xyz = _pn2_encode64(sd64, pcs64, routes, gaps)
    Fn = pcs64.shape[0]
    emb = perp = None
    if vq:
        cb = sd64["vector_quantization.embedding.weight"]
        z = z_e.reshape(-1, cb.shape[1])
        if codes is None:
            with torch.no_grad():
                codes = ((z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * z @ cb.t()).argmin(1)
        e = cb[codes.long().reshape(-1)]
        emb = torch.mean((e.detach() - z) ** 2) + BETA * torch.mean((e - z.detach()) ** 2)
        counts = torch.bincount(codes.long().reshape(-1), minlength=cb.shape[0]).double() / z.shape[0]
        perp = torch.exp(-torch.sum(counts * torch.log(counts + 1e-10)))
        z_dec = (z + (e - z).detach()).reshape(Fn, 25, -1)
    else:
        z_dec = z_e
    x = Fnn.relu(Fnn.linear(z_dec, sd64["pn2.fc1.weight"], sd64["pn2.fc1.bias"]))
    x = Fnn.relu(Fnn.linear(x, sd64["pn2.fc2.weight"], sd64["pn2.fc2.bias"]))
    off = Fnn.linear(x, sd64["pn2.fc3.weight"], sd64["pn2.fc3.bias"]).reshape(Fn, 25, 40, 3)
    r = (off + xyz[:, :, None]).reshape(Fn, 1000, 3)
    p = pcs64
    with torch.no_grad():
        dmat = _nearest64(r.detach(), p)
        own_src = torch.stack([d.argmin(1) for d in dmat])
        own_tgt = torch.stack([d.argmin(0) for d in dmat])
        if nn is None:
            nn = (own_src, own_tgt)
        elif gaps is not None:
            g_src = max((d.gather(1, nn[0][f].long()[:, None]).squeeze(1) - d.min(1)[0]).max().item() for f, d in enumerate(dmat))
            g_tgt = max((d.gather(0, nn[1][f].long()[None, :]).squeeze(0) - d.min(0)[0]).max().item() for f, d in enumerate(dmat))
            gaps["nn"] = max(g_src, g_tgt)
            gaps["nn_flips"] = int((nn[0].long() != own_src).sum() + (nn[1].long() != own_tgt).sum())
    bi = torch.arange(Fn)[:, None]
    d1 = ((r - p[bi, nn[0].long()]) ** 2).sum(-1).sum(1)
    d2 = ((p - r[bi, nn[1].long()]) ** 2).sum(-1).sum(1)
    cd = (d1 + d2).mean()
    total = cd + (emb if vq else 0.0)
    return total, cd, emb, perp, z_e


def _f64_step(sd, pcs, codes, nn_src, nn_tgt, vq=True, routes=None, gaps=None):
    """float64 autograd of total_loss for state dict `sd` (VQVAE keys) with the GPU's discrete choices
    -> (cd, emb, perplexity, grads by name, sd64 after the step, z_e)"""
    sd64 = _sd64(sd)
    total, cd, emb, perp, z_e = _f64_loss(sd64, pcs.double(), codes, (nn_src, nn_tgt), vq, routes, gaps)
    total.backward()
    grads = {k: v.grad for k, v in sd64.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    return cd.detach(), (emb.detach() if vq else None), (perp if vq else None), grads, sd64, z_e.detach()


def _assert_near_ties(gaps):
    """every GPU choice that differs from float64's own is a near-tie: a ReLU mask only where |BN(y)| < 1e-4, a neighbourhood-max row
    within 1e-4 of the float64 max, a nearest neighbour within 1e-4 of the float64 nearest distance"""
    for key in ("relu", "max", "nn"):
        assert gaps.get(key, 0.0) < 1e-4, gaps


# Bar of the gradient comparisons, calibrated on an MI355X with the choices above fed in: worst deviation 4.2e-5 of a tensor's
# max over the step tests (2e-6 .. 4e-6 for one level on its own) (the conv biases in front of a BatchNorm excluded, see _check_grads).  Without the fed ReLU masks and
# max rows the set-abstraction gradients deviate by 1e-3 .. 1e-2: the BatchNorm backward makes them sums with heavy cancellation,
# so one mask of a value within rounding of zero moves them visibly.
GRAD_BAR = 2e-4


def _check_grads(named_grads, want, prefix=""):
    """every gradient within GRAD_BAR of the tensor's max; the conv biases in front of a train-mode BatchNorm (zero in exact
    arithmetic) bounded by 1e-3 of their layer's weight-gradient scale"""
    worst, bad = 0.0, []
    for name, g in named_grads.items():
        key = prefix + name
        w = want[key]
        if ".mlp_convs." in key and key.endswith(".bias"):
            scale = want[key[:-4] + "weight"].abs().max().item()
            if not g.abs().max().item() <= 1e-3 * scale + 1e-12:
                bad.append((key, g.abs().max().item(), scale))
            continue
        rel = (g.double().cpu() - w).abs().max().item() / (w.abs().max().item() + 1e-30)
        worst = max(worst, rel)
        if not rel < GRAD_BAR:
            bad.append((key, rel))
    assert not bad, bad
    return worst


def _gpu_step(model, pcs):
    out = model({"part_pcs": pcs})
    losses = model.loss({"part_pcs": pcs}, out)
    total = sum(losses.values())
    total.backward()
    return out, losses


def test_chamfer_matches_float64_autograd_and_nn_dist(dev):
    from pfpp_hip import ops
    from pfpp_hip import vqvae_train as V

    g = torch.Generator().manual_seed(0)
    for F, L, P, m in ((3, 25, 40, 1000), (2, 7, 13, 333), (1, 1, 1, 5)):
        off = (torch.randn(F, L * P, 3, generator=g) * 0.1).to(dev)
        ctr = torch.rand(F, L, 3, generator=g).to(dev)
        tgt = torch.rand(F, m, 3, generator=g).to(dev)
        tgt[:, -1] = tgt[:, 0]                          # an exact duplicate target: the lower index wins
        d_src, i_src, d_tgt, i_tgt = V.chamfer_fwd(off, ctr, tgt)
        r = (off.view(F, L, P, 3) + ctr[:, :, None]).reshape(F, L * P, 3)
        assert torch.equal(d_src, ops.nn_dist(r, tgt)) and torch.equal(d_tgt, ops.nn_dist(tgt, r))
        assert int(i_src.max()) < m - 1 or m == 1       # the duplicate of point 0 is never chosen
        rc, tc = r.cpu(), tgt.cpu()
        bi = torch.arange(F)[:, None]
        d = rc - tc[bi, i_src.cpu().long()]
        assert torch.equal((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], d_src.cpu())
        d = tc - rc[bi, i_tgt.cpu().long()]
        assert torch.equal((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], d_tgt.cpu())
        off_req = off.clone().requires_grad_(True)
        loss = V._ChamferFn.apply(off_req, ctr, tgt)
        (2.0 * loss).backward()
        r64 = rc.double().requires_grad_(True)
        want = (((r64 - tc.double()[bi, i_src.cpu().long()]) ** 2).sum(-1).sum(1) +
                ((tc.double() - r64[bi, i_tgt.cpu().long()]) ** 2).sum(-1).sum(1)).mean()
        (2.0 * want).backward()
        assert abs(loss.item() - want.item()) <= 1e-6 * want.item()
        gw = r64.grad
        assert (off_req.grad.cpu().double() - gw).abs().max().item() <= 1e-6 * gw.abs().max().item()


def test_vq_train_op_matches_float64(dev):
    from pfpp_hip import ops
    from pfpp_hip import vqvae_train as V

    g = torch.Generator().manual_seed(1)
    K, D, R = 1024, 16, 2200
    cb = ((torch.rand(K, D, generator=g) * 2 - 1) / K).to(dev)
    z = (torch.randn(R, D, generator=g) * 2e-3).to(dev)
    slot = torch.arange(R // 4, dtype=torch.int32, device=dev)
    _, codes = ops.vq_encode(z.view(R // 4, 1, 4 * D), cb, slot, R // 4, return_codes=True)
    codes = codes.reshape(-1)
    gemb = torch.tensor([1.5], device=dev)
    vals, dz, dcb = V.vq_train(z, cb, codes, BETA, g_emb=gemb, grads=True)
    z64 = z.cpu().double().requires_grad_(True)
    cb64 = cb.cpu().double().requires_grad_(True)
    e = cb64[codes.cpu().long()]
    loss = torch.mean((e.detach() - z64) ** 2) + BETA * torch.mean((e - z64.detach()) ** 2)
    (1.5 * loss).backward()
    p = torch.bincount(codes.cpu().long(), minlength=K).double() / R
    perp = torch.exp(-torch.sum(p * torch.log(p + 1e-10)))
    assert abs(vals[0].item() - loss.item()) <= 1e-6 * loss.item()
    assert abs(vals[1].item() - perp.item()) <= 1e-6 * perp.item()
    for got, want in ((dz, z64.grad), (dcb, cb64.grad)):
        assert (got.cpu().double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()


def _codes_near_ties(sd, z_e64, codes):
    from oracle import pfpp_oracle as O

    cb = sd["vector_quantization.embedding.weight"].double()
    z = z_e64.reshape(-1, cb.shape[1]).double()
    d = (z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * z @ cb.t()
    own = d.argmin(1)
    c = codes.cpu().long().reshape(-1)
    diff = own != c
    gap = (d[torch.arange(len(c)), c] - d[torch.arange(len(c)), own])[diff]
    assert gap.numel() <= 3 and (gap.numel() == 0 or gap.max().item() < 1e-4), gap


def test_vqvae_step_matches_float64_autograd(dev, weights_sd):
    """whole VQVAE step on 8 puzzles (48 fragments): losses, perplexity, every parameter gradient, the running statistics after
    the step and num_batches_tracked; every discrete choice of the GPU is a near-tie where it differs from float64's"""
    from pfpp_hip import vqvae_train as V

    sd = {k: v.clone() for k, v in weights_sd("vqvae").items()}
    pcs, _ = _fragments(n_puzzles=8)
    model = _model("VQVAE", dev, sd)
    pd = pcs.to(dev)
    out, losses = _gpu_step(model, pd)
    torch.cuda.synchronize()
    eng = model.train_engine()
    # the GPU's discrete choices, from a second module with the same weights (same forward)
    o2, routes, codes = _gpu_routes(_model("VQVAE", dev, sd).train_engine(), pd)
    with torch.no_grad():
        r = (o2["pc_offset"] + o2["xyz"][:, :, None]).reshape(pd.shape[0], 1000, 3)
        _, i_src, _, i_tgt = V.chamfer_fwd(r.contiguous(), None, pd)
    gaps = {}
    cd64, emb64, perp64, grads64, sd64, z_e64 = _f64_step(sd, pcs, codes, i_src.cpu(), i_tgt.cpu(), routes=routes, gaps=gaps)
    _codes_near_ties(sd, z_e64, codes)
    _assert_near_ties(gaps)
    assert abs(losses["cd_loss"].item() - cd64.item()) <= 1e-4 * cd64.item()
    assert abs(losses["embedding_loss"].item() - emb64.item()) <= 1e-4 * emb64.item()
    assert abs(out["perplexity"].item() - perp64.item()) <= 1e-5 * perp64.item()
    worst = _check_grads({n: p.grad for n, p in model.named_parameters()}, grads64)
    print(f"worst gradient deviation {worst:.2e} of the tensor max; choices {gaps}")
    for name, buf in model.named_buffers():
        want = sd64[name]
        if "running_" in name:
            assert (buf.cpu().double() - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item()), name
        elif name.endswith("num_batches_tracked"):
            assert int(buf) == int(sd[name]) + 1, name
    assert eng.step_count == 0


def test_pn2_autoencoder_step_matches_float64_autograd(dev, weights_sd):
    from pfpp_hip import vqvae_train as V

    sd = {k: v.clone() for k, v in weights_sd("vqvae").items()}
    pcs, _ = _fragments(first=3)
    model = _model("PN2", dev, sd)
    pd = pcs.to(dev)
    out = model({"part_pcs": pd})
    loss = model.loss({"part_pcs": pd}, out)
    assert set(loss) == {"cd_loss"} and set(out) == {"pc_offset", "global_feat", "xyz"}
    loss["cd_loss"].backward()
    _, routes, _ = _gpu_routes(_model("PN2", dev, sd).train_engine(), pd)
    with torch.no_grad():
        r = (out["pc_offset"] + out["xyz"][:, :, None]).reshape(pd.shape[0], 1000, 3)
        _, i_src, _, i_tgt = V.chamfer_fwd(r.contiguous(), None, pd)
    gaps = {}
    cd64, _, _, grads64, _, _ = _f64_step(sd, pcs, None, i_src.cpu(), i_tgt.cpu(), vq=False, routes=routes, gaps=gaps)
    _assert_near_ties(gaps)
    assert abs(loss["cd_loss"].item() - cd64.item()) <= 1e-4 * cd64.item()
    worst = _check_grads({n: p.grad for n, p in model.named_parameters()}, grads64, prefix="pn2.")
    print(f"worst gradient deviation {worst:.2e} of the tensor max; choices {gaps}")


@pytest.mark.parametrize("level", [0, 1, 2])
def test_set_abstraction_level_backward_matches_float64(dev, weights_sd, level):
    """one set-abstraction level on its own (12 fragments; levels 2 and 3 with random input features on the sampled coordinates of
    the levels before): gradients of the conv weights, BatchNorm gamma / beta and the input features (pfpp_group_gather_bwd, the
    first layer's column order) against float64 autograd with the GPU's max rows and ReLU masks"""
    from oracle import pfpp_oracle as O
    from pfpp_hip import ops

    sd = {k: v.clone() for k, v in weights_sd("vqvae").items()}
    model = _model("PN2", dev, sd)
    eng = model.train_engine()
    pcs = _fragments(first=11)[0]
    F = pcs.shape[0]
    xyz = pcs.to(dev)
    for k in range(level):
        _, xyz = ops.fps(xyz.contiguous(), O.SA_CFG[k][1])
    g = torch.Generator().manual_seed(20 + level)
    feats = None
    if level:
        feats = torch.rand(F, xyz.shape[1], (128, 256)[level - 1], generator=g).to(dev)
    name, npoint, radius, nsample = O.SA_CFG[level]
    S = npoint or 25
    lv = eng.level_forward(name, S, radius, nsample, xyz.contiguous(), feats)
    C3 = lv["out"].shape[2]
    dout = (torch.randn(F * S, C3, generator=g) * 1e-3).to(dev)
    eng.flat.zero_grad()
    eng.flat.attach_grads()
    dfeats = eng.level_backward(lv, dout)
    torch.cuda.synchronize()
    sd64 = _sd64(sd)
    feats64 = feats.cpu().double().requires_grad_(True) if feats is not None else None
    gaps = {}
    _, out64 = _sa64(sd64, f"pn2.{name}", S, radius, nsample, xyz.cpu().double(), feats64, _lv_choices(lv), gaps)
    (out64 * dout.cpu().double().view(F, S, C3)).sum().backward()
    _assert_near_ties(gaps)
    assert (lv["out"].cpu().double() - out64.detach()).abs().max().item() <= 1e-4 * out64.detach().abs().max().item()
    grads64 = {k: v.grad for k, v in sd64.items() if k.startswith(f"pn2.{name}.") and isinstance(v, torch.Tensor) and v.grad is not None}
    mine = {n: p.grad for n, p in model.named_parameters() if n.startswith(f"{name}.")}
    assert len(mine) == len(grads64) == 12
    worst = _check_grads(mine, grads64, prefix="pn2.")
    if feats is None:
        assert dfeats is None
    else:
        want = feats64.grad
        rel = (dfeats.cpu().double() - want).abs().max().item() / want.abs().max().item()
        assert rel < GRAD_BAR, rel
        worst = max(worst, rel)
    print(f"level {level + 1}: worst gradient deviation {worst:.2e} of the tensor max; choices {gaps}")


def _fae(dev, sd, kind="VQVAE"):
    from pfpp_hip import config
    from puzzlefusion_plusplus.vqvae.model.fracture_ae import FractureAE

    fae = FractureAE(config.vqvae_train_config(kind))
    fae.ae.load_state_dict(sd)
    return fae.to(dev).train()


def _batch(dev, n=2, first=0):
    _, b = _fragments(n, first=first)
    return {"part_pcs": b["part_pcs"].to(dev), "num_parts": b["part_valids"].sum(1).to(dev)}


def test_adamw_and_scheduler_follow_torch(dev, weights_sd):
    """three FractureAE steps through configure_optimizers' FusedAdamW against torch.optim.AdamW in float64 fed with the engine's
    gradients (the BN-fed conv biases left out: Adam turns their noise-level gradients into +-lr steps); MultiStepLR halves the rate"""
    sd = {k: v.clone() for k, v in weights_sd("vqvae").items()}
    fae = _fae(dev, sd)
    conf = fae.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]
    names = [n for n, _ in fae.named_parameters()]
    ref = [p.detach().cpu().double().clone().requires_grad_(True) for p in fae.parameters()]
    ropt = torch.optim.AdamW(ref, lr=5e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6)
    batch = _batch(dev)
    for _ in range(3):
        loss = fae.training_step({k: v for k, v in batch.items()}, 0)
        loss.backward()
        for r, p in zip(ref, fae.parameters()):
            r.grad = p.grad.detach().cpu().double().clone()
        opt.step()
        ropt.step()
        opt.zero_grad()
        assert math.isfinite(loss.item())
    for n, r, p in zip(names, ref, fae.parameters()):
        if ".mlp_convs." in n and n.endswith(".bias"):
            continue
        d = (p.detach().cpu().double() - r.detach()).abs().max().item()
        assert d <= 1e-6 * max(1.0, r.abs().max().item()), (n, d)
    assert opt.engine.overflow_steps == 0
    assert fae.logged["train_loss/total_loss"] is not None and "train_perplexity" in fae.logged
    for _ in range(800):
        sched.step()
    assert abs(opt.param_groups[0]["lr"] - 2.5e-4) < 1e-12


# Bar of the 30-step loss curve against float64, calibrated on an MI355X: worst relative deviation of total_loss 1.8e-2 .. 2.5e-2
# in four runs, 1.9e-3 after the first update, 7e-8 before any update.  AdamW normalises every element: where a true gradient is
# below the fp32 rounding of its contraction (the BatchNorm-fed sums cancel heavily) the two runs step +-lr in different
# directions, so the curves part by O(lr) from the first update on.
CURVE_BAR = 5e-2


def test_module_loop_follows_float64(dev, weights_sd):
    """training_step -> backward -> step -> zero_grad for 30 steps on one fixed batch (2 puzzles, 12 fragments): finite throughout,
    cd_loss falls, and the total_loss curve stays within CURVE_BAR (relative) of a float64 torch run of the same 30 steps
    (torch.optim.AdamW, float64's own discrete choices).  This carries the state that lives between steps — the per-site gradient
    scales, the split planes AdamW refreshes and the forward reads, the running statistics — against an independent reference.
    Measured worst deviation on an MI355X: 2.5e-2 (CURVE_BAR 5e-2); the loss before the first update agrees to 1e-6, and the split
    planes the forward reads equal the fp32 parameters after the last update."""
    from puzzlefusion_plusplus.vqvae.model.fracture_ae import FractureAE

    sd = {k: v.clone() for k, v in weights_sd("vqvae").items()}
    fae = _fae(dev, sd)
    opt = fae.configure_optimizers()["optimizer"]
    batch = _batch(dev, n=2, first=5)
    pcs = _fragments(2, first=5)[0]
    gpu = []
    for _ in range(30):
        loss = fae.training_step(dict(batch), 0)
        loss.backward()
        opt.step()
        opt.zero_grad()
        gpu.append((float(loss.detach()), float(fae.logged["train_loss/cd_loss"].detach())))
    assert all(math.isfinite(t) and math.isfinite(c) for t, c in gpu)
    assert all(torch.isfinite(p).all() for p in fae.parameters())
    assert gpu[-1][1] < 0.9 * gpu[0][1], gpu
    assert opt.engine.overflow_steps == 0
    sd64 = _sd64(sd)
    params = [v for v in sd64.values() if isinstance(v, torch.Tensor) and v.requires_grad]
    opt64 = torch.optim.AdamW(params, **FractureAE.OPTIM)
    pcs64 = pcs.double()
    ref = []
    for _ in range(30):
        total, cd, _, _, _ = _f64_loss(sd64, pcs64)
        total.backward()
        opt64.step()
        opt64.zero_grad()
        ref.append((total.item(), cd.item()))
    dev_curve = [abs(a[0] - b[0]) / b[0] for a, b in zip(gpu, ref)]
    print(f"30-step total_loss curve: worst relative deviation {max(dev_curve):.2e} (step {dev_curve.index(max(dev_curve))}); "
          f"first {dev_curve[0]:.1e}, last {dev_curve[-1]:.1e}")
    assert dev_curve[0] < 1e-6 and max(dev_curve) < CURVE_BAR, dev_curve
    f = opt.engine.flat
    with torch.no_grad():
        assert (f.hi.float() + f.lo.float() - f.params).abs().max().item() <= 2.0 ** -20 * f.params.abs().max().item()
    fae.eval()
    fae.validation_step(dict(batch), 0)
    assert math.isfinite(float(fae.logged["val_loss/total_loss"]))


def test_run_to_run(dev, weights_sd):
    sd = {k: v.clone() for k, v in weights_sd("vqvae").items()}
    pd = _fragments()[0].to(dev)
    res = []
    for _ in range(2):
        m = _model("VQVAE", dev, sd)
        _, losses = _gpu_step(m, pd)
        res.append((losses["cd_loss"].item(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    assert abs(res[0][0] - res[1][0]) <= 1e-6 * res[0][0]
    for n, g in res[0][1].items():
        if ".mlp_convs." in n and n.endswith(".bias"):
            continue                 # zero in exact arithmetic (a train-mode BatchNorm follows): noise, bounded in the step tests
        h = res[1][1][n]
        assert (g - h).abs().max().item() <= 1e-6 * g.abs().max().item() + 1e-30, n


def test_hand_off_to_the_denoiser(dev, weights_sd):
    """the trained FractureAE's state (ae. stripped) loads strictly into Denoiser.encoder, its eval encode matches the oracle; a
    reference-layout optimizer state loads by position; F > 2048 and N != 25 x 40 raise ValueError"""
    from oracle import pfpp_oracle as O
    from pfpp_hip import config
    from puzzlefusion_plusplus.denoiser.model.denoiser import Denoiser

    sd = {k: v.clone() for k, v in weights_sd("vqvae").items()}
    fae = _fae(dev, sd)
    opt = fae.configure_optimizers()["optimizer"]
    batch = _batch(dev)
    fae.training_step(dict(batch), 0).backward()
    opt.step()
    opt.zero_grad()
    trained = {k[3:]: v.detach().cpu().clone() for k, v in fae.state_dict().items() if k.startswith("ae.")}
    assert len(trained) == 72
    den = Denoiser(config.denoiser_config())
    den.encoder.load_state_dict(trained, strict=True)
    den = den.to(dev)
    pcs = _fragments(first=7)[0]
    enc = den.encoder.eval()
    with torch.no_grad():
        got = enc.encode(pcs.to(dev))
        got_fae = fae.ae.eval().encode(pcs.to(dev))
    want = O.vqvae_encode(trained, pcs)
    dev_rows = (got["z_q"].cpu() - want["z_q"]).abs().amax(-1)
    assert int((dev_rows > 1e-3).sum()) <= 3
    assert torch.equal(got["xyz"].cpu(), want["xyz"])
    assert (got_fae["z_q"] - got["z_q"]).abs().max().item() <= 1e-5        # the live module sees the new weights and statistics
    # a reference-layout optimizer state (torch.optim.AdamW over FractureAE.parameters()) loads by position
    params = list(fae.parameters())
    state = {i: {"step": torch.tensor(4.0), "exp_avg": torch.full(p.shape, 0.01 * (i + 1)), "exp_avg_sq": torch.full(p.shape, 1e-4)}
             for i, p in enumerate(params)}
    groups = [dict(lr=5e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6, amsgrad=False, foreach=None, maximize=False,
                   capturable=False, differentiable=False, fused=None, params=list(range(len(params))))]
    opt.load_state_dict({"state": state, "param_groups": groups})
    flat = opt.engine.flat
    for i, (n, p) in enumerate(fae.named_parameters()):
        v = flat.view(flat.exp_avg, n[3:])
        assert torch.allclose(v.cpu(), torch.full(p.shape, 0.01 * (i + 1))), n
    assert opt.engine.step_count == 4
    fae.train()
    eng = fae.ae.train_engine()
    with pytest.raises(ValueError):
        eng.forward(torch.zeros((2049, 1000, 3), device=dev))
    with pytest.raises(ValueError):
        eng.forward(torch.zeros((2, 999, 3), device=dev))
