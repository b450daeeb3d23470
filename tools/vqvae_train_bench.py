"""Milliseconds per VQ-VAE pre-training step (FractureAE, vqvae/model/fracture_ae.py) at the reference batch: --puzzles synthetic
puzzles (config/ae/data.yaml: batch 45 of <= 20 parts x 1000 points; the synthetic part-count distribution).

Three timings on one GPU, each the median over --steps steps after --warmup:
  engine   VQVAETrainEngine forward + Chamfer + backward + FusedAdamW step (HIP kernels, no autograd)
  module   FractureAE.training_step -> loss.backward() -> opt.step() -> opt.zero_grad() (the same engine behind the module surface)
  eager    the same network and losses in PyTorch eager fp32 autograd on the same GPU (torch.optim.AdamW); FPS and ball-query
           indices come from the HIP kernels (bit-exact with the reference's sampling)

    python tools/vqvae_train_bench.py [--puzzles 45] [--steps 5] [--warmup 2] [--skip-eager]
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "puzzlefusion-plusplus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch                        # noqa: E402
import torch.nn.functional as Fnn   # noqa: E402


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def eager_step_fn(sd, pcs):
    """PyTorch eager fp32 autograd of total_loss (set abstraction in .train(), quantizer, decoder, Chamfer) + AdamW"""
    from pfpp_hip import ops

    levels = (("sa1", 256, 0.2, 32), ("sa2", 128, 0.4, 64), ("sa3", 25, 0.8, 64))
    params = [v for v in sd.values() if v.requires_grad]
    opt = torch.optim.AdamW(params, lr=5e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6)
    F_ = pcs.shape[0]
    bi = torch.arange(F_, device=pcs.device)[:, None, None]

    def step():
        xyz, feats = pcs, None
        for name, S, radius, ns in levels:
            _, new_xyz = ops.fps(xyz.contiguous(), S)
            ball = ops.ball_query(xyz.contiguous(), new_xyz, radius, ns).long()
            g = xyz[bi, ball] - new_xyz[:, :, None]
            if feats is not None:
                g = torch.cat([g, feats[bi, ball]], -1)
            h = g.permute(0, 3, 2, 1)
            for i in range(3):
                p = f"pn2.{name}"
                h = Fnn.conv2d(h, sd[f"{p}.mlp_convs.{i}.weight"], sd[f"{p}.mlp_convs.{i}.bias"])
                h = Fnn.relu(Fnn.batch_norm(h, sd[f"{p}.mlp_bns.{i}.running_mean"], sd[f"{p}.mlp_bns.{i}.running_var"],
                                            sd[f"{p}.mlp_bns.{i}.weight"], sd[f"{p}.mlp_bns.{i}.bias"], True, 0.1, 1e-5))
            feats = torch.max(h, 2)[0].permute(0, 2, 1)
            xyz = new_xyz
        z_e = Fnn.linear(feats, sd["pn2.conv6.weight"].reshape(64, -1), sd["pn2.conv6.bias"])
        cb = sd["vector_quantization.embedding.weight"]
        z = z_e.reshape(-1, cb.shape[1])
        d = (z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * z @ cb.t()
        e = cb[d.argmin(1)]
        emb = torch.mean((e.detach() - z) ** 2) + 0.25 * torch.mean((e - z.detach()) ** 2)
        zq = (z + (e - z).detach()).reshape(F_, 25, -1)
        x = Fnn.relu(Fnn.linear(zq, sd["pn2.fc1.weight"], sd["pn2.fc1.bias"]))
        x = Fnn.relu(Fnn.linear(x, sd["pn2.fc2.weight"], sd["pn2.fc2.bias"]))
        off = Fnn.linear(x, sd["pn2.fc3.weight"], sd["pn2.fc3.bias"]).reshape(F_, 25, 40, 3)
        r = (off + xyz[:, :, None]).reshape(F_, 1000, 3)
        dd = torch.cdist(r, pcs) ** 2
        cd = (dd.min(2)[0].sum(1) + dd.min(1)[0].sum(1)).mean()
        (cd + emb).backward()
        opt.step()
        opt.zero_grad()

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=45)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true")
    a = ap.parse_args()
    from oracle import weights
    from pfpp_hip import config, synthetic
    from pfpp_hip import vqvae_train as V
    from puzzlefusion_plusplus.vqvae.model.fracture_ae import FractureAE

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    b = synthetic.make_batch(0, a.puzzles, num_points=1000)
    valid = b["part_valids"].bool()
    batch = {"part_pcs": b["part_pcs"].to(dev), "num_parts": valid.sum(1).to(dev)}
    pcs = b["part_pcs"][valid].contiguous().to(dev)
    F_ = pcs.shape[0]
    sd0 = weights.vqvae_state_dict()
    res = {"workload": "vqvae_train_step", "puzzles": a.puzzles, "fragments": F_}

    fae = FractureAE(config.vqvae_train_config())
    fae.ae.load_state_dict(sd0)
    fae = fae.to(dev).train()
    opt = fae.configure_optimizers()["optimizer"]
    eng = fae.ae.train_engine()
    one = torch.ones(1, device=dev)

    def engine_step():
        out, ctx = eng.forward(pcs)
        off = out["pc_offset"].view(F_, 1000, 3)
        d_src, i_src, d_tgt, i_tgt = V.chamfer_fwd(off, out["xyz"], pcs)
        V.chamfer_reduce(d_src, d_tgt, 1.0 / F_)
        g = V.chamfer_bwd(off, out["xyz"], pcs, i_src, i_tgt, 1.0 / F_)
        eng.backward(ctx, g_emb=one, g_off=g.view_as(out["pc_offset"]))
        opt.step()
        opt.zero_grad()

    with torch.no_grad():
        res["engine_ms"] = round(_time(engine_step, a.steps, a.warmup), 2)

    def module_step():
        loss = fae.training_step(dict(batch), 0)
        loss.backward()
        opt.step()
        opt.zero_grad()

    res["module_ms"] = round(_time(module_step, a.steps, a.warmup), 2)
    res["cd_loss"] = float(fae.logged["train_loss/cd_loss"].detach())
    res["peak_gb_hip"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    if not a.skip_eager:
        del fae, opt, eng
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        sd = {k: (v.to(dev).clone().requires_grad_("running_" not in k) if v.is_floating_point() else v.to(dev).clone())
              for k, v in sd0.items()}
        res["eager_ms"] = round(_time(eager_step_fn(sd, pcs), a.steps, a.warmup), 2)
        res["speedup_vs_eager"] = round(res["eager_ms"] / res["module_ms"], 2)
        res["peak_gb_eager"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
