"""Verifier training step on the MI355X: HIP engine vs the module-surface loop vs PyTorch-ROCm eager fp32 (the module's own
nn.TransformerEncoder with torch's kernels) at the reference's configuration (batch 64 x 190 edges, make_edges validity, six
layers).  Prints one JSON line.

    python tools/verifier_train_bench.py [--batch 64] [--layers 6] [--steps 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import copy
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "puzzlefusion-plusplus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def eager_loss(m, batch):
    """the reference's VerifierTransformer.forward + Verifier._loss with torch's kernels"""
    ef, ei, valid, y = batch["edge_features"], batch["edge_indices"], batch["edge_valids"].bool(), batch["cls_gt"]
    B, E, _ = ei.shape
    h = m.edge_feature_emb(ef) + m.edge_indices_pe.pe[0][ei].reshape(B, E, -1)
    h = m.transformer_encoder(h, src_key_padding_mask=~valid)
    logits = m.mlp_out(h)[..., 0][valid]
    yv = y[valid]
    return F.binary_cross_entropy_with_logits(logits, yv, weight=torch.where(yv == 0, 0.2, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from pfpp_hip import config, synthetic
    from pfpp_hip.verifier_train import VerifierTrainEngine
    from puzzlefusion_plusplus.verifier.model.verifier import Verifier

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = config.verifier_config(model=dict(num_layers=a.layers))
    b = synthetic.make_edges(a.batch, seed=0)
    b["cls_gt"] = ((b["edge_features"][..., 6] > 150) & (b["edge_valids"] > 0)).float()
    batch = {k: v.to(dev) for k, v in b.items()}
    model = Verifier(cfg).to(dev)
    eager = copy.deepcopy(model.verifier)                    # same weights, torch's kernels
    eng_mod = copy.deepcopy(model.verifier)
    eng = VerifierTrainEngine(eng_mod)
    opt = model.configure_optimizers()
    model.train()
    args = (batch["edge_features"], batch["edge_indices"], batch["edge_valids"], batch["cls_gt"])

    def engine_step():
        eng.loss_and_grads(*args, seed=int(torch.randint(0, 2 ** 62, (1,)).item()))
        eng.optimizer_step(zero_grad=True)

    def module_step():
        loss = model.training_step(batch, 0)
        loss.backward()
        opt.step()
        opt.zero_grad()

    eopt = torch.optim.AdamW(eager.parameters(), lr=2e-4, betas=(0.95, 0.999), weight_decay=1e-6, eps=1e-8)
    eager.train()

    def eager_step():
        eager_loss(eager, batch).backward()
        eopt.step()
        eopt.zero_grad()

    # loss difference with dropout 0 (same weights, before any step)
    ref = copy.deepcopy(model.verifier)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    chk = VerifierTrainEngine(copy.deepcopy(model.verifier), dropout=0.0)
    with torch.no_grad():
        l_eager = float(eager_loss(ref, batch))
    logits, ctx = chk.forward(*args[:3], seed=0, train=True, cls_gt=args[3])
    l_hip = float(ctx.t["loss"])
    del chk, ctx, ref

    ms_engine = timed(engine_step, a.steps, a.warmup)
    ms_module = timed(module_step, a.steps, a.warmup)
    ms_eager = timed(eager_step, a.steps, a.warmup)
    n_edges = int(batch["edge_valids"].numel())
    print(json.dumps({"metric": "verifier_train_step", "batch": a.batch, "edges": n_edges, "layers": a.layers,
                      "ms_per_step": round(ms_engine, 3), "module_loop_ms": round(ms_module, 3), "edges_per_s": round(n_edges / ms_engine * 1e3),
                      "torch_eager_fp32_ms": round(ms_eager, 3), "speedup_vs_eager": round(ms_eager / ms_engine, 2),
                      "loss_hip_p0": l_hip, "loss_eager_p0": l_eager, "loss_rel_diff_p0": abs(l_hip - l_eager) / abs(l_eager)}))


if __name__ == "__main__":
    main()
