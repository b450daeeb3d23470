"""Measure one training step of the matcher's head (pfpp_hip.matching_train.MatchingHeadTrainEngine) on one GPU; print one JSON line.

    python tools/matching_train_bench.py [--puzzles 2] [--reps 3] [--skip-eager] [--profile] [--out profiles/matching_train_bench_line.json]

Workload: the matcher bench's synthetic puzzles (tools/matching_bench.py): `--puzzles` puzzles of 8 pieces x 625 = 5,000 points, N' =
2,492 critical points each, labels given.  A step is loss_and_grads (both losses) + optimizer_step.  The comparison is the same step in
PyTorch-ROCm eager fp32 on the same GPU, restated the way the reference runs it: the three modules in .train() under autograd, the
zero-padded critical_feats, the Sinkhorn that rewrites log_s 20 times, F.binary_cross_entropy against a dense gt_perm, torch.optim.Adam.
The two alternate; reported are the medians of `--reps` wall times after one warm-up each, the engine's Sinkhorn backward alone by
device events against the bytes its 21 passes must move (3 N'^2 4 B per update pass: s and G read, G written), and the peak device memory
of both.  --profile runs only the engine's steps (for rocprofv3 --kernel-trace --stats).

--rigid: the same puzzles with weights (1, 1, 1) (pfpp_hip.matching_rigid.MatchingHeadRigidTrainEngine; part_pcs = every piece's
gt_pcs recentred and turned by a seeded rotation).  The eager step's rigid term is the reference's own procedure: a Python loop over
the piece pairs that slices ds_mat, copies the block to the host, solves Horn's 4 x 4 eigenproblem in numpy and copies the pose back
(tests/matching_rigid_cases.horn restates horn_87).  Also timed in the same run: the engine's step without the term, so that the
term's added cost is visible.  The default mode is unchanged."""
from __future__ import annotations

import argparse
import importlib.util
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "puzzlefusion-plusplus_amd"))

PIECES, PER_PIECE, MATCHES = 8, 625, 178
TAU, ITERS = 0.05, 20


def load_cases(stem: str = "matching_cases"):
    spec = importlib.util.spec_from_file_location(stem, ROOT / "tests" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def eager_rigid_loss(mats, part_pcs, label, piece, n_pieces, horn):
    """utils/loss.py:59-142 the way the reference runs it: per pair, the block to the host, Horn in numpy (float32 inputs), the pose back"""
    dev = mats[0].device
    loss, n_sum = torch.zeros((), device=dev), 0
    for b, mat in enumerate(mats):
        pts, pc = part_pcs[b, label[b]], piece[b, label[b]].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(np.bincount(pc, minlength=n_pieces))])
        mat_d = mat.detach().cpu().numpy()
        total = torch.sum(mat)
        for p in range(n_pieces):
            for q in range(p + 1, n_pieces):
                i0, i1, j0, j1 = off[p], off[p + 1], off[q], off[q + 1]
                if i1 == i0 or j1 == j0:
                    continue
                w = mat[i0:i1, j0:j1] + mat[j0:j1, i0:i1].transpose(1, 0)
                mat_s = torch.sum(w)
                if n_pieces > 2 and mat_s == 0 and total > 0:
                    continue
                src, tgt = pts[i0:i1], pts[j0:j1]
                R, t, _, _ = horn(src.cpu().numpy(), tgt.cpu().numpy(), mat_d[i0:i1, j0:j1] + mat_d[j0:j1, i0:i1].T)
                rot = torch.tensor(R.astype(np.float32), device=dev)
                trans = torch.tensor(t.astype(np.float32), device=dev)
                a = (torch.matmul(rot, src.transpose(1, 0)).transpose(1, 0) + trans) * torch.sum(w, dim=-1).reshape(-1, 1)
                c = torch.matmul(w, tgt)
                n_sum += int(i1 - i0)
                loss = loss + torch.sum(a ** 2 + c ** 2 - 2 * a * c) * mat_s
    return loss / n_sum


class EagerHead(torch.nn.Module):
    """the reference's training step behind part_feats in plain PyTorch"""

    def __init__(self, sd):
        super().__init__()
        nn = torch.nn
        self.pc_classifier = nn.Sequential(nn.BatchNorm1d(128), nn.ReLU(inplace=True), nn.Conv1d(128, 1, 1))
        self.affinity_extractor = nn.Sequential(nn.BatchNorm1d(128), nn.ReLU(inplace=True), nn.Conv1d(128, 512, 1))
        self.A = nn.Parameter(sd["affinity_layer.A"].clone())
        self.pc_classifier.load_state_dict({k[len("pc_classifier."):]: v for k, v in sd.items() if k.startswith("pc_classifier.")})
        self.affinity_extractor.load_state_dict({k[len("affinity_extractor."):]: v for k, v in sd.items() if k.startswith("affinity_extractor.")})
        self.train()

    def loss(self, feats, gt_pcs, label, piece, rigid=None):
        """feats [B, N, 128], gt_pcs [B, N, 3], label bool [B, N], piece int64 [B, N]; rigid = (part_pcs, n_pieces, horn) adds the
        rigid term"""
        F = torch.nn.functional
        B, N, _ = feats.shape
        logits = self.pc_classifier(feats.transpose(1, 2)).transpose(1, 2).reshape(-1)
        cls_loss = F.binary_cross_entropy_with_logits(logits, label.reshape(-1).float())
        n_sum = label.sum(1)
        n_max = int(n_sum.max())
        cf = torch.zeros(B, n_max, 128, device=feats.device)
        gp = torch.zeros(B, n_max, 3, device=feats.device)
        pc = torch.full((B, n_max), -1, dtype=torch.int64, device=feats.device)
        for b in range(B):
            cf[b, :n_sum[b]] = feats[b, label[b]]
            gp[b, :n_sum[b]] = gt_pcs[b, label[b]]
            pc[b, :n_sum[b]] = piece[b, label[b]]
        af = self.affinity_extractor(cf.permute(0, 2, 1)).permute(0, 2, 1)
        af = torch.cat([F.normalize(af[:, :, :256], p=2, dim=-1), F.normalize(af[:, :, 256:], p=2, dim=-1)], -1)
        s = torch.matmul(torch.matmul(af[:, :, :256], self.A), af[:, :, 256:].transpose(1, 2))
        with torch.no_grad():
            d = -2 * torch.matmul(gp, gp.transpose(1, 2))
            d += (gp ** 2).sum(-1)[:, :, None]
            d += (gp ** 2).sum(-1)[:, None, :]
            d = d.clamp_min(1e-12)
            same = pc[:, :, None] == pc[:, None, :]
            d = d + same * 1e6
            gt_perm = torch.zeros(B, n_max, n_max, device=feats.device).scatter_(2, d.argmin(-1, keepdim=True), 1) * (~same)
        total = torch.zeros((), device=feats.device)
        mats = []
        for b in range(B):
            n = int(n_sum[b])
            log_s = s[b, :n, :n] / TAU
            for i in range(ITERS):
                log_s = log_s - torch.logsumexp(log_s, 1 if i % 2 == 0 else 0, keepdim=True)
            mats.append(torch.exp(log_s))
            total = total + F.binary_cross_entropy(mats[b], gt_perm[b, :n, :n], reduction="sum")
        if rigid is None:
            return cls_loss + total / n_sum.sum()
        return cls_loss + total / n_sum.sum() + eager_rigid_loss(mats, rigid[0], label, piece, rigid[1], rigid[2])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--puzzles", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--profile", action="store_true", help="only the engine's steps (kernel trace)")
    ap.add_argument("--rigid", action="store_true", help="weights (1, 1, 1): the step with the rigid term")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("matching_train_bench: no GPU: nothing is measured without one", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    from pfpp_hip.matching import MatchingHead
    from pfpp_hip.matching_train import MatchingHeadTrainEngine, sinkhorn_train_bwd, sinkhorn_train_fwd

    cases = load_cases()
    sd_np = cases.head_state_dict()
    sd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd_np.items()}
    head = MatchingHead()
    head.load_state_dict(sd, strict=True)
    head.to(dev)
    eng = MatchingHeadTrainEngine(head, w_cls_loss=1.0, w_mat_loss=1.0)
    if args.rigid:
        from pfpp_hip.matching_rigid import MatchingHeadRigidTrainEngine

        plain_eng = eng
        eng = MatchingHeadRigidTrainEngine(head, w_cls_loss=1.0, w_mat_loss=1.0, w_rig_loss=1.0)
    sym = [(p, p + 1, MATCHES) for p in range(PIECES - 1)]
    pzs = [cases.build_puzzle([PER_PIECE] * PIECES, sym, [], 100 + k) for k in range(args.puzzles)]
    feats = torch.from_numpy(np.stack([p["part_feats"] for p in pzs])).to(dev)
    gt_pcs = torch.from_numpy(np.stack([p["gt_pcs"] for p in pzs])).to(dev)
    label = torch.from_numpy(np.stack([p["critical"] for p in pzs])).to(dev)
    n_pcs = np.stack([p["n_pcs"] for p in pzs])
    valids = np.stack([p["part_valids"] for p in pzs])
    piece = torch.from_numpy(np.stack([np.repeat(np.arange(n_pcs.shape[1]), n) for n in n_pcs])).to(dev)
    n_prime = [int(x) for x in label.sum(1).tolist()]
    extra, rigid = {}, None
    if args.rigid:
        rcases = load_cases("matching_rigid_cases")
        part_pcs = torch.from_numpy(rcases.make_part_pcs({"gt_pcs": gt_pcs.cpu().numpy(), "n_pcs": n_pcs})).to(dev)
        extra, rigid = {"part_pcs": part_pcs}, (part_pcs, PIECES, rcases.horn)

    def hip_step():
        loss_dict, _ = eng.loss_and_grads(feats, gt_pcs, n_pcs, valids, critical_label=label, **extra)
        eng.optimizer_step()
        return loss_dict["loss"]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    if args.profile:
        for _ in range(1 + args.reps):
            hip_step()
        torch.cuda.synchronize()
        return 0

    eager = opt = None
    if not args.skip_eager:
        eager = EagerHead(sd).to(dev)
        opt = torch.optim.Adam(eager.parameters(), lr=1e-3)

    def eager_step():
        opt.zero_grad(set_to_none=True)
        loss = eager.loss(feats, gt_pcs, label, piece, rigid)
        loss.backward()
        opt.step()
        return loss

    peak = {}
    for name, fn in (("hip", hip_step), ("eager", eager_step)):                # warm-up of every shape, and the peak memory of one step each
        if name == "eager" and eager is None:
            continue
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        first = fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        peak[name + "_loss"] = float(first.detach())
    times = {"hip": [], "eager": []}
    for _ in range(args.reps):                                                  # alternating
        times["hip"].append(wall(hip_step)[1])
        if eager is not None:
            times["eager"].append(wall(eager_step)[1])
    if args.rigid:
        def plain_step():
            loss_dict, _ = plain_eng.loss_and_grads(feats, gt_pcs, n_pcs, valids, critical_label=label)
            plain_eng.optimizer_step()
            return loss_dict["loss"]

        plain_step()
        plain = [wall(plain_step)[1] for _ in range(args.reps)]
        saved = eng.saved
        line = {"bench": "matching_head_train_rigid", "puzzles": args.puzzles, "points": PIECES * PER_PIECE, "n_critical": n_prime,
                "pairs": int(saved["kept"].numel()), "pairs_kept": int(saved["kept"].sum()), "hip_step_ms": statistics.median(times["hip"]),
                "hip_step_ms_without_rigid": statistics.median(plain), "rigid_added_ms": statistics.median(times["hip"]) - statistics.median(plain),
                "hip_loss_after_warmup": peak["hip_loss"], "hip_peak_step_mem_mb": peak["hip"],
                "extra_passes_must_move_mb_per_puzzle": 3 * n_prime[0] * n_prime[0] * 4 / 1e6}
        if eager is not None:
            line.update({"eager_step_ms": statistics.median(times["eager"]), "eager_loss_after_warmup": peak["eager_loss"],
                         "eager_peak_step_mem_mb": peak["eager"], "speedup_vs_eager": statistics.median(times["eager"]) / statistics.median(times["hip"])})
        text = json.dumps(line)
        print(text)
        if args.out:
            Path(args.out).write_text(text + "\n")
        return 0
    # the Sinkhorn of one puzzle on its own, by device events
    n = n_prime[0]
    s = (0.3 * torch.randn(n, n, device=dev)).contiguous()
    tgt = torch.randperm(n, device=dev).to(torch.int32)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    fwd_ms, bwd_ms = [], []
    for _ in range(1 + args.reps):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        ds_mat, _, pots = sinkhorn_train_fwd(s, tgt, tau=TAU, max_iter=ITERS)
        e1.record()
        sinkhorn_train_bwd(s, tgt, pots, ds_mat, g=1.0 / n, tau=TAU, max_iter=ITERS)
        e2.record()
        e2.synchronize()
        fwd_ms.append(e0.elapsed_time(e1)); bwd_ms.append(e1.elapsed_time(e2))
    fwd, bwd = statistics.median(fwd_ms[1:]), statistics.median(bwd_ms[1:])
    must = ITERS * 3 * n * n * 4
    line = {"bench": "matching_head_train", "puzzles": args.puzzles, "points": PIECES * PER_PIECE, "n_critical": n_prime,
            "hip_step_ms": statistics.median(times["hip"]), "hip_loss_after_warmup": peak["hip_loss"], "hip_peak_step_mem_mb": peak["hip"],
            "sinkhorn_fwd_ms_per_puzzle": fwd, "sinkhorn_bwd_ms_per_puzzle": bwd, "sinkhorn_bwd_must_move_mb": must / 1e6,
            "sinkhorn_bwd_gb_per_s": must / 1e9 / (bwd / 1e3), "autograd_would_keep_mb_per_puzzle": ITERS * n * n * 4 / 2 ** 20}
    if eager is not None:
        line.update({"eager_step_ms": statistics.median(times["eager"]), "eager_loss_after_warmup": peak["eager_loss"],
                     "eager_peak_step_mem_mb": peak["eager"], "speedup_vs_eager": statistics.median(times["eager"]) / statistics.median(times["hip"])})
    text = json.dumps(line)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
