"""Verifier training on the HIP kernels (pfpp_hip.verifier_train, csrc/verifier_train.hip) against float64 torch restatements of
Verifier._loss / VerifierTransformer.forward in train mode (verifier/model/verifier.py:20-69, verifier_transformer.py:45-58).

Bars follow tests/test_gpu_train.py: rel(got, want) = max |got - want| / max |want|.  torchmetrics' binary metrics (the reference's)
are written down here: pred = fp32 sigmoid(logit) > 0.5; acc = (tp + tn) / n, precision = tp / (tp + fp), recall = tp / (tp + fn),
f1 = 2 tp / (2 tp + fp + fn), a zero denominator giving 0."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

H, DH, C = 8, 32, 256


def rel(got, want):
    return float((got.double().cpu() - want.double().cpu()).abs().max() / (want.double().cpu().abs().max() + 1e-30))


def _cfg(layers=6):
    from pfpp_hip import config

    return config.verifier_config(model=dict(num_layers=layers))


def _batch(B, seed=0, dev="cuda"):
    from pfpp_hip import synthetic

    b = synthetic.make_edges(B, seed=seed)
    # a learnable label: an edge matches when it has many matched points (count feature, column 6)
    b["cls_gt"] = ((b["edge_features"][..., 6] > 150) & (b["edge_valids"] > 0)).float()
    return {k: v.to(dev) for k, v in b.items()}


# ------------------------------------------------------------------------------------------------------------ attention kernel
def _attn_inputs(dev, B=4, E=190, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * E, 3 * C, generator=g)
    valid = (torch.rand(B, E, generator=g) < 0.6)
    valid[0] = False
    valid[0, 17] = True                          # one valid key
    valid[1] = False                             # no valid key
    return qkv, valid


def _attn_ref(qkv, valid, keep, p):
    """float64 restatement of MultiheadAttention's probability path with an explicit keep mask [B, H, E, E]"""
    B, E = valid.shape
    qkv = qkv.double().clone().requires_grad_(True)
    q, k, v = qkv.view(B, E, 3, H, DH).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(DH)
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    P = torch.softmax(s, -1)
    P = torch.nan_to_num(P, nan=0.0)             # the kernel's convention for a sequence without a valid key
    if keep is not None:
        P = P * keep.double() / (1 - p)
    out = (P @ v).permute(0, 2, 1, 3).reshape(B * E, C)
    return qkv, out


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_kernel_vs_float64(dev, p):
    from pfpp_hip import train_ops as T

    B, E = 4, 190
    qkv, valid = _attn_inputs(dev, B, E)
    seed, site = 1234, 7
    keep = T.verifier_attn_dropout_mask(B, H, E, p, seed, site, dev).cpu() if p > 0 else None
    kv = valid.to(torch.uint8).to(dev)
    out, lse = T.verifier_attn_fwd(qkv.to(dev), kv, B, E, H, DH, 1 / math.sqrt(DH), p, seed, site)
    q64, ref = _attn_ref(qkv, valid, keep, p)
    dout = torch.randn(B * E, C, generator=torch.Generator().manual_seed(3))
    ref.backward(dout.double())
    assert torch.isfinite(out).all() and rel(out, ref.detach()) < 1e-5
    dqkv = T.verifier_attn_bwd(qkv.to(dev), out, dout.to(dev), lse, kv, B, E, H, DH, 1 / math.sqrt(DH), p, seed, site)
    torch.cuda.synchronize()
    want = q64.grad
    for part in range(3):
        sl = slice(part * C, (part + 1) * C)
        assert rel(dqkv[:, sl], want[:, sl]) < 1e-5, part
    d = dqkv.cpu().view(B, E, 3 * C)
    assert (d[:, :, C:][~valid] == 0).all()                     # masked keys: exactly zero dk / dv
    assert (d[1] == 0).all() and (out.cpu().view(B, E, C)[1] == 0).all()     # no valid key: zeros, not NaN


def test_attention_dropout_mask_statistics_and_determinism(dev):
    from pfpp_hip import train_ops as T

    m = T.verifier_attn_dropout_mask(8, H, 190, 0.1, 99, 3, dev)
    n = m.numel()
    assert n >= 10 ** 6
    frac = m.double().mean().item()
    assert abs(frac - 0.9) < 5 * math.sqrt(0.9 * 0.1 / n)
    assert torch.equal(m, T.verifier_attn_dropout_mask(8, H, 190, 0.1, 99, 3, dev))
    assert not torch.equal(m, T.verifier_attn_dropout_mask(8, H, 190, 0.1, 99, 4, dev))


def test_attention_refuses_long_sequences(dev):
    from pfpp_hip import _lib
    from pfpp_hip import train_ops as T

    E = 257
    qkv = torch.zeros(E, 3 * C, device=dev)
    with pytest.raises(_lib.PfppError, match="code -2"):
        T.verifier_attn_fwd(qkv, torch.ones(1, E, dtype=torch.uint8, device=dev), 1, E, H, DH, 0.1, 0.1, 0, 0)


# ------------------------------------------------------------------------------------------------------------ head + BCE kernel
def _head_case(M, dev, seed=0, n_valid=None):
    g = torch.Generator().manual_seed(seed)
    h6 = torch.randn(M, C, generator=g)
    w = torch.randn(C, generator=g) * 0.05
    b = torch.randn(1, generator=g) * 0.1
    y = (torch.rand(M, generator=g) < 0.3).float()
    valid = torch.rand(M, generator=g) < 0.7
    if n_valid == 0:
        valid[:] = False
    return h6, w, b, y, valid


def _counts(logits, y, valid):
    pred = (torch.sigmoid(logits) > 0.5)[valid]
    pos = (y > 0.5)[valid]
    return [int((pred & pos).sum()), int((pred & ~pos).sum()), int((~pred & ~pos).sum()), int((~pred & pos).sum())]


def test_head_bce_kernel_vs_float64(dev):
    from pfpp_hip import train_ops as T

    M = 64 * 190
    h6, w, b, y, valid = _head_case(M, dev)
    # logits within +-1e-7 of zero: the fp32 sigmoid decides (a tiny positive logit can round to 0.5 and count as 0)
    tiny = torch.tensor([1e-7, -1e-7, 1e-8, -1e-8, 3e-8, 0.0])
    for j, t in enumerate(tiny):
        h6[j] = 0
        h6[j, 0] = (t - b[0]) / w[0]                 # logit ~ t (up to fp32 rounding: compared against torch on the same logits)
        valid[j] = True
    ws = T.verifier_head_workspace(dev)
    dw = torch.zeros(C, device=dev)
    db = torch.zeros(1, device=dev)
    logits, loss, dlogit, dh6, stats = T.verifier_head_bce(h6.to(dev), w.to(dev), b.to(dev), y.to(dev), valid.to(torch.uint8).to(dev),
                                                           dw, db, ws)
    h64 = h6.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    lg = h64 @ w64 + b64
    yv = y.double()[valid]
    ref = F.binary_cross_entropy_with_logits(lg[valid], yv, weight=torch.where(yv == 0, 0.2, 1.0).double())
    ref.backward()
    assert rel(logits, lg.detach()) < 1e-6
    assert rel(loss, ref.detach().reshape(1)) < 1e-6
    assert rel(dh6, h64.grad) < 1e-6 and rel(dw, w64.grad) < 1e-6 and rel(db, b64.grad) < 1e-6
    lg_ = lg.detach().double()
    want_dlogit = torch.zeros(M, dtype=torch.float64)
    want_dlogit[valid] = (torch.where(yv == 0, 0.2, 1.0) * (torch.sigmoid(lg_[valid]) - yv) / int(valid.sum())).double()
    assert rel(dlogit, want_dlogit) < 1e-6
    # confusion counts: exactly torch's fp32 sigmoid(x) > 0.5 on the kernel's logits (on the GPU, like the kernel)
    lk = logits.clone()
    assert stats.cpu().tolist() == _counts(lk, y.to(dev), valid.to(dev))
    assert ws.abs().sum().item() == 0                   # the workspace is left zeroed
    # a second call gives the same loss (the workspace really was reset)
    _, loss2, _, _, stats2 = T.verifier_head_bce(h6.to(dev), w.to(dev), b.to(dev), y.to(dev), valid.to(torch.uint8).to(dev),
                                                 torch.zeros(C, device=dev), torch.zeros(1, device=dev), ws)
    assert torch.equal(loss, loss2) and torch.equal(stats, stats2)


def test_head_bce_kernel_without_valid_edges(dev):
    from pfpp_hip import train_ops as T

    M = 190
    h6, w, b, y, valid = _head_case(M, dev, n_valid=0)
    ws = T.verifier_head_workspace(dev)
    dw = torch.zeros(C, device=dev)
    db = torch.zeros(1, device=dev)
    logits, loss, dlogit, dh6, stats = T.verifier_head_bce(h6.to(dev), w.to(dev), b.to(dev), y.to(dev), valid.to(torch.uint8).to(dev),
                                                           dw, db, ws)
    assert loss.item() == 0.0 and (dlogit == 0).all() and (dh6 == 0).all() and (dw == 0).all() and (db == 0).all()
    assert stats.cpu().tolist() == [0, 0, 0, 0]
    assert rel(logits, h6.double() @ w.double() + b.double()) < 1e-6


# ------------------------------------------------------------------------------------------------------------ whole step
def _module(layers, dev, seed=0):
    from puzzlefusion_plusplus.verifier.model.modules.verifier_transformer import VerifierTransformer

    torch.manual_seed(seed)
    return VerifierTransformer(_cfg(layers)).to(dev)


def _masks(B, E, layers, p, seed, dev):
    from pfpp_hip import train_ops as T
    from pfpp_hip.verifier_train import site

    M = B * E
    out = []
    for i in range(layers):
        out.append((T.verifier_attn_dropout_mask(B, H, E, p, seed, site(i, 0), dev).cpu(),
                    T.dropout_mask(M * C, p, seed, site(i, 1), dev).cpu().view(B, E, C),
                    T.dropout_mask(M * 2048, p, seed, site(i, 2), dev).cpu().view(B, E, 2048),
                    T.dropout_mask(M * C, p, seed, site(i, 3), dev).cpu().view(B, E, C)))
    return out


def _ref_step(module, batch, p, masks):
    """float64 autograd through a CPU deep copy of the module's own nn.TransformerEncoder layers (dropout p = 0 there), with the
    kernels' masks applied at the four sites when given"""
    m = copy.deepcopy(module).cpu().double()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0                      # the probability dropout is a float attribute, not a Dropout module
    ef = batch["edge_features"].cpu().double()
    ei = batch["edge_indices"].cpu()
    valid = batch["edge_valids"].cpu().bool()
    y = batch["cls_gt"].cpu().double()
    B, E, _ = ef.shape
    pe = m.edge_indices_pe.pe[0]
    h = m.edge_feature_emb(ef) + pe[ei].reshape(B, E, -1)
    for i, layer in enumerate(m.transformer_encoder.layers):
        if masks is None:
            h = layer(h, src_key_padding_mask=~valid)
            continue
        ka, k1, k2, k3 = (t.double() / (1 - p) for t in masks[i])
        at = layer.self_attn
        qkv = F.linear(h, at.in_proj_weight, at.in_proj_bias)
        q, k, v = qkv.view(B, E, 3, H, DH).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(DH)
        P = torch.softmax(s.masked_fill(~valid[:, None, None, :], float("-inf")), -1) * ka
        att = (P @ v).permute(0, 2, 1, 3).reshape(B, E, C)
        x1 = layer.norm1(h + at.out_proj(att) * k1)
        u = F.gelu(layer.linear1(x1)) * k2
        h = layer.norm2(x1 + layer.linear2(u) * k3)
    logits = m.mlp_out(h)[..., 0]
    yv = y[valid]
    loss = F.binary_cross_entropy_with_logits(logits[valid], yv, weight=torch.where(yv == 0, 0.2, 1.0).double())
    loss.backward()
    return loss.detach(), {n: q.grad for n, q in m.named_parameters()}


@pytest.mark.parametrize("B,layers,p", [(4, 2, 0.0), (4, 2, 0.1), (64, 1, 0.0), (64, 1, 0.1)])
def test_training_step_vs_float64_autograd(dev, B, layers, p):
    from pfpp_hip.verifier_train import VerifierTrainEngine

    module = _module(layers, dev)
    batch = _batch(B, seed=1, dev=dev)
    ref_module = copy.deepcopy(module)
    eng = VerifierTrainEngine(module, dropout=p)
    seed = 4242
    loss, stats, logits = eng.loss_and_grads(batch["edge_features"], batch["edge_indices"], batch["edge_valids"], batch["cls_gt"], seed=seed)
    torch.cuda.synchronize()
    masks = _masks(B, 190, layers, p, seed, dev) if p > 0 else None
    want_loss, want_g = _ref_step(ref_module, batch, p, masks)
    assert rel(loss, want_loss.reshape(1)) < 2e-5
    for n, q in module.named_parameters():
        assert q.grad is not None
        assert rel(q.grad, want_g[n]) < 2e-4, n


# ------------------------------------------------------------------------------------------------------------ optimizer
def test_two_adamw_steps_vs_torch_and_reference_state_dict(dev):
    from puzzlefusion_plusplus.verifier.model.verifier import Verifier

    torch.manual_seed(0)
    model = Verifier(_cfg(2)).to(dev)
    opt = model.configure_optimizers()
    names = [n for n, _ in model.named_parameters()]
    ref = {n: q.detach().cpu().double().clone().requires_grad_(True) for n, q in model.named_parameters()}
    ropt = torch.optim.AdamW(list(ref.values()), lr=2e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    # a torch AdamW over Verifier.parameters() on the GPU (the reference's optimizer), for the state_dict hand-over
    twin = copy.deepcopy(model)
    topt = torch.optim.AdamW(twin.parameters(), lr=2e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    for it in range(2):
        batch = _batch(8, seed=10 + it, dev=dev)
        model.train()
        loss = model.training_step(batch, it)
        loss.backward()
        for (n, q), r, t in zip(model.named_parameters(), ref.values(), twin.parameters()):
            r.grad = q.grad.detach().cpu().double().clone()
            t.grad = q.grad.detach().clone()
        opt.step()
        opt.zero_grad()
        ropt.step()
        topt.step()
        for n, q in model.named_parameters():
            assert (q.detach().cpu().double() - ref[n].detach()).abs().max().item() < 1e-6, (it, n)
    # the reference-style optimizer state loads by position into the fused optimizer and continues identically
    model2 = Verifier(_cfg(2)).to(dev)
    model2.load_state_dict(twin.state_dict())
    opt2 = model2.configure_optimizers()
    opt2.load_state_dict(topt.state_dict())
    batch = _batch(8, seed=20, dev=dev)
    model2.train()
    torch.manual_seed(7)
    model2.training_step(batch, 0).backward()
    for q, t in zip(model2.parameters(), twin.parameters()):
        t.grad = q.grad.detach().clone()
    opt2.step()
    topt.step()
    for (n, q), t in zip(model2.named_parameters(), twin.parameters()):
        assert (q.detach() - t.detach()).abs().max().item() < 1e-6, n
    assert names == [n for n, _ in model2.named_parameters()]


# ------------------------------------------------------------------------------------------------------------ module surface
def test_module_surface_matches_engine_and_eval_sees_new_weights(dev):
    from pfpp_hip.verifier_train import VerifierTrainEngine
    from puzzlefusion_plusplus.verifier.model.verifier import Verifier

    torch.manual_seed(0)
    model = Verifier(_cfg(2)).to(dev)
    keys = list(model.state_dict().keys())
    shapes = {k: v.shape for k, v in model.state_dict().items()}
    twin = copy.deepcopy(model.verifier)
    eng = VerifierTrainEngine(twin)
    opt = model.configure_optimizers()
    batch = _batch(8, seed=3, dev=dev)
    model.train()
    torch.manual_seed(11)
    loss = model.training_step(batch, 0)
    loss.backward()
    assert all(q.grad is not None for q in model.parameters())
    opt.step()
    opt.zero_grad()
    torch.manual_seed(11)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    loss2, _, _ = eng.loss_and_grads(batch["edge_features"], batch["edge_indices"], batch["edge_valids"], batch["cls_gt"], seed=seed)
    eng.optimizer_step()
    assert rel(loss.detach().reshape(1), loss2) < 1e-6
    for (n, q), t in zip(model.verifier.named_parameters(), twin.parameters()):
        assert (q.detach() - t.detach()).abs().max().item() < 1e-6, n
    assert list(model.state_dict().keys()) == keys and {k: v.shape for k, v in model.state_dict().items()} == shapes
    assert set(model.logged) >= {"training/loss", "training/cls_precision", "training/cls_recall", "training/cls_f1_score",
                                 "training/cls_acc"}
    # the next .eval() forward sees the updated weights
    model.eval()
    fresh = Verifier(_cfg(2)).to(dev).eval()
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        a = model(batch)["logits"]
        b = fresh(batch)["logits"]
    assert torch.equal(a, b)
    out = model._loss(batch, {"logits": a})
    assert set(out) == {"bce_loss", "cls_loss", "cls_acc", "cls_precision", "cls_recall", "cls_f1_score"}


def test_train_mode_forward_is_an_autograd_node(dev):
    """VerifierTransformer.forward in .train(): logits whose backward is the engine's (a loss written in torch on the logits)"""
    module = _module(2, dev)
    ref_module = copy.deepcopy(module)
    eng = module.train_engine()
    eng.p = 0.0
    batch = _batch(4, seed=5, dev=dev)
    module.train()
    logits = module(batch["edge_features"], batch["edge_indices"], batch["edge_valids"])
    valid = batch["edge_valids"].bool()
    yv = batch["cls_gt"][valid]
    loss = F.binary_cross_entropy_with_logits(logits[..., 0][valid], yv, weight=torch.where(yv == 0, 0.2, 1.0))
    loss.backward()
    want_loss, want_g = _ref_step(ref_module, batch, 0.0, None)
    assert rel(loss.detach().reshape(1), want_loss.reshape(1)) < 2e-5
    for n, q in module.named_parameters():
        assert rel(q.grad, want_g[n]) < 2e-4, n


# ------------------------------------------------------------------------------------------------------------ convergence
def test_training_loop_converges_on_a_learnable_rule(dev):
    """300 steps of the plain module loop on make_edges data labelled by the count feature: the loss falls and the accuracy over the
    valid edges of held-out batches reaches 0.9"""
    from puzzlefusion_plusplus.verifier.model.verifier import Verifier

    torch.manual_seed(0)
    model = Verifier(_cfg(2)).to(dev)
    opt = model.configure_optimizers()
    model.train()
    losses = []
    for i in range(300):
        batch = _batch(16, seed=100 + i % 20, dev=dev)
        loss = model.training_step(batch, i)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(x) for x in losses)
    assert sum(losses[-20:]) / 20 < 0.5 * sum(losses[:20]) / 20
    model.eval()
    accs = []
    with torch.no_grad():
        for s in range(3):
            batch = _batch(16, seed=500 + s, dev=dev)
            accs.append(float(model._loss(batch, model(batch))["cls_acc"]))
    assert min(accs) >= 0.9, accs
