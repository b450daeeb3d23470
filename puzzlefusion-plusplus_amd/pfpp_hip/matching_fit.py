"""Fitting the matcher end to end (the reference's Jigsaw_matching/train_matching.py and model/modules/matching_base_model.py around
the step the engines already run): the learning-rate schedule, Adam over all 175 parameter tensors in a handful of launches
(pfpp_adam_multi, csrc/train_ops.hip) and the validation metrics of one puzzle in one launch (pfpp_match_val_metrics,
csrc/matching_train.hip).

* cosine_warmup_lr: the rate in force during an epoch under configure_optimizers (:499-535) and Lightning's per-epoch scheduler.step().
* plan_adam_multi / adam_multi: the C entry's chunking restated on the host, and the entry itself.
* val_metrics: permutation loss of a masked doubly-stochastic matrix and (tp, fp, fn) of an assignment.
* MatcherOptimizer: torch.optim.Adam / AdamW over the parameters of a DescriptorTrainEngine and a head engine; it reads and writes
  the engines' own `state` dicts, so an engine's optimizer_step can continue from it and the reverse; state_dict() has
  torch.optim.Adam.state_dict()'s layout with the parameters indexed in the reference model's order.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._lib import check
from .matching import _gpu, _p

# ------------------------------------------------------------------------------------------------------------------ learning rate
def cosine_warmup_lr(epoch: int, total_epochs: int, max_lr: float, lr_decay: float, warmup_ratio: float, scheduler: str = "cosine") -> float:
    """the learning rate during `epoch` (0-based): CosineAnnealingWarmupRestarts (utils/lr.py:26-153) with first_cycle_steps =
    total_epochs, min_lr = max_lr / lr_decay, warmup_steps = int(total_epochs * warmup_ratio), cycle_mult = gamma = 1, stepped once at
    the end of every epoch.  Epoch 0 runs at min_lr: the class's init_lr() overwrites the rate its constructor's first step set.  The
    expressions keep the class's operand order, so the Python floats are its floats.  scheduler "" (LR_SCHEDULER empty): constant
    max_lr; anything but "cosine" is refused, as matching_base_model.py:518 asserts."""
    if not scheduler:
        return max_lr
    if scheduler.lower() != "cosine":
        raise ValueError(f"LR_SCHEDULER {scheduler!r}: only 'cosine' (or empty) is known")
    total, warmup = int(total_epochs), int(total_epochs * warmup_ratio)
    if not warmup < total:
        raise ValueError("the warm-up must be shorter than the cycle")
    min_lr = max_lr / lr_decay
    if epoch <= 0:
        return min_lr
    k = epoch % total
    if k < warmup:
        return (max_lr - min_lr) * k / warmup + min_lr
    return min_lr + (max_lr - min_lr) * (1 + math.cos(math.pi * (k - warmup) / (total - warmup))) / 2


# ------------------------------------------------------------------------------------------------------------------ multi-tensor Adam
MAX_TENSORS, MAX_BLOCKS, CHUNK = 36, 384, 8192          # PFPP_ADAM_MULTI_MAX_TENSORS / _MAX_BLOCKS / _CHUNK of include/pfpp.h


def plan_adam_multi(sizes: Sequence[int]) -> List[Tuple[int, int, int]]:
    """the launches pfpp_adam_multi issues for tensors of these element counts: (first_tensor, first_chunk, n_blocks) each.  A launch
    starts at chunk first_chunk of tensor first_tensor and takes the following chunks in order, tensor after tensor (empty tensors are
    skipped and take no slot), until it holds MAX_TENSORS tensors or MAX_BLOCKS chunks of CHUNK elements; a tensor that the block
    capacity cuts goes on in the next launch, where it takes a slot again."""
    launches: List[Tuple[int, int, int]] = []
    first, nt, nb = None, 0, 0
    for t, n in enumerate(sizes):
        if n < 0:
            raise ValueError("plan_adam_multi: negative element count")
        chunks, c = -(-int(n) // CHUNK), 0
        while c < chunks:
            if nt == MAX_TENSORS or nb == MAX_BLOCKS:
                launches.append((*first, nb))
                first, nt, nb = None, 0, 0
            if first is None:
                first = (t, c)
            take = min(chunks - c, MAX_BLOCKS - nb)
            nb, c, nt = nb + take, c + take, nt + 1
    if nb:
        launches.append((*first, nb))
    return launches


def adam_multi(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor], exp_avg_sqs: Sequence[torch.Tensor],
               steps: Sequence[int], *, lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
               g_scale: float = 1.0) -> None:
    """one Adam / AdamW step (pfpp_adamw's arithmetic, bit for bit) over a list of float32 tensors on the GPU; steps: every tensor's
    own step count AFTER this step (>= 1).  The tensors may be views (any 4-byte aligned address) but must be dense."""
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(steps) == n):
        raise ValueError("adam_multi: one gradient, two moments and one step count per parameter")
    for i in range(n):
        for t, what in ((params[i], "parameter"), (grads[i], "gradient"), (exp_avgs[i], "exp_avg"), (exp_avg_sqs[i], "exp_avg_sq")):
            _gpu(t, torch.float32, what)
            if t.numel() != params[i].numel() or not t.is_contiguous():
                raise ValueError(f"adam_multi: {what} {i} must be dense and of the parameter's size")
        if steps[i] < 1:
            raise ValueError("adam_multi: step counts start at 1")
    ptrs = lambda ts: [t.data_ptr() if t.numel() else None for t in ts]
    _adam_multi_launch(ptrs(params), ptrs(grads), ptrs(exp_avgs), ptrs(exp_avg_sqs), [t.numel() for t in params], steps, lr, betas, eps, weight_decay,
                       g_scale)


def _adam_multi_launch(p, g, m, v, sizes, steps, lr, betas, eps, weight_decay, g_scale) -> None:
    """pfpp_adam_multi on lists of device addresses (None for an empty tensor) that the caller has checked"""
    n = len(sizes)
    arr = C.c_void_p * n
    bc1 = (C.c_float * n)(*[1.0 - betas[0] ** s for s in steps])
    bc2 = (C.c_float * n)(*[1.0 - betas[1] ** s for s in steps])
    check(_lib.load().pfpp_adam_multi(n, arr(*p), arr(*g), arr(*m), arr(*v), (C.c_int64 * n)(*sizes), bc1, bc2, float(lr), float(betas[0]),
                                      float(betas[1]), float(eps), float(weight_decay), float(g_scale), ops._stream()), "pfpp_adam_multi")


# ------------------------------------------------------------------------------------------------------------------ validation metrics
def val_metrics(ds_mat: torch.Tensor, tgt: torch.Tensor, col: torch.Tensor, loss_out: Optional[torch.Tensor] = None,
                counts_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ds_mat float32 [n, n] (the masked Sinkhorn output), tgt int32 [n] (-1 = no target), col int64 [n] (the assignment's column per
    row) -> (loss float64 [1] = sum_ij BCE(ds_mat_ij, [j == tgt_i]) with both logs clamped at -100, counts int64 [3] = (tp, fp, fn))"""
    _gpu(ds_mat, torch.float32, "ds_mat"); _gpu(tgt, torch.int32, "tgt"); _gpu(col, torch.int64, "col")
    n = ds_mat.shape[0]
    if ds_mat.dim() != 2 or ds_mat.shape[1] != n or not ds_mat.is_contiguous() or n < 1:
        raise ValueError(f"val_metrics: ds_mat must be a contiguous square matrix, got {tuple(ds_mat.shape)}")
    if tgt.shape != (n,) or col.shape != (n,) or not tgt.is_contiguous() or not col.is_contiguous():
        raise ValueError("val_metrics: one target and one assigned column per row")
    loss = torch.empty(1, dtype=torch.float64, device=ds_mat.device) if loss_out is None else loss_out
    counts = torch.empty(3, dtype=torch.int64, device=ds_mat.device) if counts_out is None else counts_out
    ops._chk(loss, torch.float64, "loss"); ops._chk(counts, torch.int64, "counts")
    if loss.numel() != 1 or counts.numel() != 3:
        raise ValueError("val_metrics: loss [1] and counts [3]")
    check(_lib.load().pfpp_match_val_metrics(_p(ds_mat), n, _p(tgt), _p(col), _p(loss), _p(counts), ops._stream()), "pfpp_match_val_metrics")
    return loss, counts


# ------------------------------------------------------------------------------------------------------------------ the optimizer
# the order in which JointSegmentationAlignmentModel.__init__ registers its modules (joint_seg_align_model.py:38-49), hence of
# self.parameters() and of the indices in the optimizer's state_dict; it is not this tree's module order
REFERENCE_MODULE_ORDER = ("encoder", "affinity_layer", "pc_classifier", "affinity_extractor", "tf_self1", "tf_cross1")
_NORMS = (torch.nn.LayerNorm, torch.nn.GroupNorm, torch.nn.modules.batchnorm._BatchNorm, torch.nn.modules.instancenorm._InstanceNorm)


def reference_parameter_names(net: torch.nn.Module, head: torch.nn.Module) -> List[str]:
    """the names of the reference model's named_parameters(), in its order, from a DescriptorNetwork and a MatchingHead"""
    names = []
    for prefix in REFERENCE_MODULE_ORDER:
        owner = net if hasattr(net, prefix) else head
        names += [f"{prefix}.{k}" for k, _ in getattr(owner, prefix).named_parameters()]
    return names


def weight_decay_split(net: torch.nn.Module, head: torch.nn.Module) -> Tuple[List[str], List[str]]:
    """filter_wd_parameters (utils/utils.py:91-128) by name -> (no_decay, decay), each in the order the reference hands its list to AdamW:
    no_decay = the weights of the normalisation layers in sorted module order, then the biases of every module that has one in
    sorted module order; decay = the other parameters, sorted by name.  (The reference tells parameters apart by VALUE: a decayed
    tensor that happened to equal a non-decayed one element for element would leave its list; initialised weights never do.)"""
    w_name, b_name = [], []
    for prefix in REFERENCE_MODULE_ORDER:
        owner = net if hasattr(net, prefix) else head
        for name, m in getattr(owner, prefix).named_modules(prefix=prefix):
            if isinstance(m, _NORMS):
                w_name.append(name)
            if isinstance(getattr(m, "bias", None), torch.Tensor):
                b_name.append(name)
    no_decay = [f"{m}.weight" for m in sorted(w_name)] + [f"{m}.bias" for m in sorted(b_name)]
    seen = set(no_decay)
    decay = sorted(k for k in reference_parameter_names(net, head) if k not in seen)
    return no_decay, decay


class MatcherOptimizer:
    """configure_optimizers' optimizer (matching_base_model.py:499-515) over a DescriptorTrainEngine and a head engine: Adam when
    weight_decay is 0, else AdamW over the two groups of filter_wd_parameters.  step(lr) updates every parameter that has a .grad
    through pfpp_adam_multi; a parameter without one keeps its step count, as in torch.  The moments and step counts are the
    engines' own `state` entries (m, v, step)."""

    def __init__(self, descriptor_engine, head_engine, *, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, clip_grad=None):
        if clip_grad is not None:
            raise NotImplementedError("TRAIN.CLIP_GRAD is not None: gradient clipping needs a global-norm kernel that is not built "
                                      "(no experiment file of the reference sets it)")
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        engines = {"encoder": descriptor_engine.encoder, "tf_self1": descriptor_engine.tf_self1, "tf_cross1": descriptor_engine.tf_cross1}
        head_prefixes = ("affinity_layer", "pc_classifier", "affinity_extractor")
        self.entries: Dict[str, tuple] = {}             # reference name -> (engine, the engine's key)
        for prefix in REFERENCE_MODULE_ORDER:
            if prefix in head_prefixes:
                keys = [k for k in head_engine.params if k.startswith(prefix + ".")]
                self.entries.update({k: (head_engine, k) for k in keys})
            else:
                self.entries.update({f"{prefix}.{k}": (engines[prefix], k) for k in engines[prefix].params})
        self.names = list(self.entries)
        if self.names != reference_parameter_names(descriptor_engine.net, head_engine.head):
            raise ValueError("MatcherOptimizer: the engines' parameters are not the networks' named_parameters()")
        if self.weight_decay > 0:
            no_decay, decay = weight_decay_split(descriptor_engine.net, head_engine.head)
            if sorted(no_decay + decay) != sorted(self.names):
                raise ValueError("MatcherOptimizer: the decay split does not cover the parameters once each")
            self.groups = [(no_decay, 0.0), (decay, self.weight_decay)]
        else:
            self.groups = [(self.names, 0.0)]
        self._last_sizes: List[List[int]] = []

    @property
    def last_launches(self) -> int:
        """the kernel launches of the last step()"""
        return sum(len(plan_adam_multi(sizes)) for sizes in self._last_sizes)

    def _param(self, name: str) -> torch.nn.Parameter:
        eng, k = self.entries[name]
        return eng.params[k]

    def step(self, lr: float) -> None:
        """one optimizer step.  The host side is one pass over the parameters: what a tensor must satisfy is checked when its moments
        are created, and per step only what can change, the gradient (the engines hand out new tensors every step)"""
        self._last_sizes = []
        f32 = torch.float32
        for names, wd in self.groups:
            p_, g_, m_, v_, sizes, steps, keep = [], [], [], [], [], [], []
            for name in names:
                eng, k = self.entries[name]
                p = eng.params[k]
                g = p.grad
                if g is None:
                    continue
                st = eng.state.get(k)
                if st is None:
                    ops._chk(p.data, f32, name)
                    st = (torch.zeros_like(p.data), torch.zeros_like(p.data), 0)
                m, v, step = st
                if g.dtype is not f32 or g.device != p.device or g.shape != p.shape:
                    raise ValueError(f"{name}: the gradient is not a float32 tensor of the parameter's shape on its device")
                if not g.is_contiguous():
                    g = g.contiguous()
                eng.state[k] = (m, v, step + 1)
                n = p.numel()
                p_.append(p.data_ptr() if n else None); g_.append(g.data_ptr() if n else None)
                m_.append(m.data_ptr() if n else None); v_.append(v.data_ptr() if n else None)
                sizes.append(n); steps.append(step + 1); keep.append((p, g))
            _adam_multi_launch(p_, g_, m_, v_, sizes, steps, lr, self.betas, self.eps, wd, 1.0)
            self._last_sizes.append(sizes)
            for p, _ in keep:
                torch.autograd.graph.increment_version(p)      # the kernel wrote through raw pointers: the layers' pack caches watch _version

    # ---- torch.optim.Adam.state_dict()'s layout
    def _index_order(self) -> List[str]:
        return [name for names, _ in self.groups for name in names]

    def state_dict(self, lr: float = 1e-3) -> dict:
        """as torch.optim.Adam(model.parameters()).state_dict() (AdamW over the two groups when weight_decay > 0) would give it for
        the reference model: integer parameter indices in the reference's order, `step` a float32 0-dim tensor, moments on the CPU"""
        order = self._index_order()
        state = {}
        for i, name in enumerate(order):
            eng, k = self.entries[name]
            if k in eng.state:
                m, v, step = eng.state[k]
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": m.detach().cpu().clone(), "exp_avg_sq": v.detach().cpu().clone()}
        groups, at = [], 0
        for names, wd in self.groups:
            groups.append({"lr": float(lr), "betas": self.betas, "eps": self.eps, "weight_decay": wd, "amsgrad": False, "maximize": False,
                           "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                           "params": list(range(at, at + len(names)))})
            at += len(names)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd: dict) -> None:
        order = self._index_order()
        if sum(len(g["params"]) for g in sd["param_groups"]) != len(order) or len(sd["param_groups"]) != len(self.groups):
            raise ValueError("load_state_dict: the optimizer state is not one of this model and weight-decay setting")
        for name in order:
            eng, k = self.entries[name]
            eng.state.pop(k, None)
        for i, st in sd["state"].items():
            eng, k = self.entries[order[int(i)]]
            p = eng.params[k]
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"load_state_dict: {order[int(i)]}: moments of shape {tuple(st['exp_avg'].shape)} for a parameter {tuple(p.shape)}")
            to = lambda t: t.to(device=p.device, dtype=torch.float32).contiguous().clone()
            eng.state[k] = (to(st["exp_avg"]), to(st["exp_avg_sq"]), int(round(float(st["step"]))))


# ------------------------------------------------------------------------------------------------------------------ validation
LOSS_DICT_KEYS = ("cls_loss", "cls_acc", "cls_precision", "cls_recall", "cls_f1", "mat_loss", "loss", "mat_f1", "mat_precision", "mat_recall")


class MatcherValidator:
    """the reference's validation_step (matching_base_model.py:61-63: forward in eval mode with trainer.testing False, then
    _loss_function) behind the dataset's data_dict: eval-mode BatchNorms, the critical points of the GROUND-TRUTH labels, masked
    affinity, Sinkhorn, the assignment solved by scipy on the host while the device works on the next puzzle, loss = cls_loss +
    mat_loss, and mat_f1 / mat_precision / mat_recall from pfpp_match_val_metrics' counts.  rig_loss is added to the dict when
    w_rig_loss > 0, as the reference computes it then.

    A puzzle whose critical points lie on fewer than two pieces is the reference's masked-everything case: s is -1e6 everywhere, the
    Sinkhorn output the uniform matrix 1 / n, every target masked away.  It adds n^2 BCE(1 / n, 0) to the loss sum, n to fp and n to
    the row count (tools/make_matching_fit_goldens.py prints the reference's figures); no assignment is solved for it."""

    def __init__(self, net, head, *, w_rig_loss: float = 0.0, solver: str = "host", max_steps=None):
        """solver: "host" (scipy) or "device" (pfpp_hip.matching_assign.assign_batch: one launch over the puzzles of the batch, whose
        columns go straight into the metrics kernel; a puzzle whose step budget max_steps runs out is solved on the host)"""
        if solver not in ("host", "device"):
            raise ValueError(f"solver: expected 'host' or 'device', got {solver!r}")
        self.net, self.head, self.w_rig_loss = net, head, float(w_rig_loss)
        self.solver, self.max_steps = solver, max_steps
        self.saved: dict = {}
        self.timings: dict = {}

    @torch.no_grad()
    def step(self, data_dict, seed: Optional[int] = None) -> dict:
        feats = self.net(data_dict["part_pcs"], data_dict["n_pcs"], data_dict["part_valids"], seed=seed)
        return self.step_from_feats(feats, data_dict)

    @torch.no_grad()
    def step_from_feats(self, part_feats, data_dict, critical_label=None) -> dict:
        """part_feats float32 [B, N, 128] / flat; data_dict: gt_pcs, part_pcs, n_pcs, part_valids and critical_label_thresholds (or the
        labels themselves through critical_label, non-zero = critical)"""
        import time

        import numpy as np
        from scipy.optimize import linear_sum_assignment

        from .matching import PC_FEAT_DIM, _flatten, critical_points, fracture_labels, make_layout, sinkhorn
        from .matching_train import cls_bce, gt_targets

        head = self.head
        first = part_feats[0] if isinstance(part_feats, (list, tuple)) else part_feats
        _gpu(first, torch.float32, "part_feats")
        dev = first.device
        n_pcs, part_valids, gt_pcs = data_dict["n_pcs"], data_dict["part_valids"], data_dict["gt_pcs"]
        layout = make_layout(n_pcs, dev)
        feats = _flatten(part_feats, layout, PC_FEAT_DIM, "part_feats")
        pts = _flatten(gt_pcs, layout, 3, "gt_pcs")
        B, P = layout.n_pcs.shape
        pv = np.asarray(part_valids.detach().cpu().numpy() if torch.is_tensor(part_valids) else part_valids)
        n_valid = pv.reshape(B, P).sum(1).astype(np.int64)
        if critical_label is None:
            labels = fracture_labels(gt_pcs, n_pcs, data_dict["critical_label_thresholds"]).reshape(-1).to(torch.uint8)
        else:
            labels = (critical_label.reshape(-1) != 0).to(torch.uint8)
        t0 = time.perf_counter()
        logits, _, _, _ = head.classify(feats, layout)
        cls_loss, _, c4 = cls_bce(logits, labels, need_grad=False)
        crit, n_crit = critical_points(labels, layout)                    # of the ground truth: trainer.testing is False in validation
        crit_off = torch.zeros(B * P + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n_crit, 0, out=crit_off[1:])
        nc = n_crit.cpu().numpy().reshape(B, P)                           # the one read-back: the matrices are allocated from it
        rows = np.concatenate([[0], np.cumsum(nc.sum(1))]).astype(np.int64)
        R, n_max = int(rows[-1]), int(nc.sum(1).max(initial=0))
        losses = torch.zeros(B, dtype=torch.float64, device=dev)
        counts = torch.zeros((B, 3), dtype=torch.int64, device=dev)
        ds_list: List[torch.Tensor] = [torch.empty((0, 0), dtype=torch.float32, device=dev) for _ in range(B)]
        cols: List[Optional[torch.Tensor]] = [None] * B
        host_s = device_s = 0.0
        fallback: List[int] = []
        if R:
            f, row_piece = head.affinity_features(feats, layout, crit, crit_off, R)
            pa = head.primal_times_a(f)
            src = torch.nonzero(labels).reshape(-1)                       # global point index of every critical row: puzzle, piece, point order
            piece_of_row = torch.bucketize(src, layout.piece_off[1:], right=True).to(torch.int32)
            tgt = gt_targets(pts, src, piece_of_row, torch.from_numpy(rows).to(dev), n_max)
            solved = [b for b in range(B) if (nc[b] > 0).sum() >= 2]
            n_big = max((int(rows[b + 1] - rows[b]) for b in solved), default=0) if self.solver == "host" else 0
            # two pinned buffers taken in turn by the solved puzzles: at most one job is pending and job k is solved before job k + 1
            # becomes pending, so when job k + 2 takes job k's buffer that assignment has been read out of it (MatchingHead.forward)
            pinned = [torch.empty(n_big * n_big, dtype=torch.float32, pin_memory=True) for _ in range(2 if n_big else 0)]
            copy_stream = torch.cuda.Stream(dev) if self.solver == "host" else None
            pending, n_jobs = None, 0

            def solve(job):
                nonlocal host_s
                b, buf, ev = job
                ev.synchronize()
                t = time.perf_counter()
                _, col = linear_sum_assignment(-buf.numpy())
                host_s += time.perf_counter() - t
                cols[b] = torch.from_numpy(col.astype(np.int64)).to(dev)
                val_metrics(ds_list[b], tgt[rows[b]:rows[b + 1]], cols[b], losses[b:b + 1], counts[b])

            for b in range(B):
                r0, r1 = int(rows[b]), int(rows[b + 1])
                n = r1 - r0
                if n == 0:
                    continue
                if b not in solved:                                       # the masked-everything case
                    ds_list[b] = torch.full((n, n), 1.0 / n, dtype=torch.float32, device=dev)
                    val_metrics(ds_list[b], torch.full((n,), -1, dtype=torch.int32, device=dev), torch.arange(n, device=dev), losses[b:b + 1], counts[b])
                    continue
                s = head.affinity(f, r0, r1, pa)
                ds_list[b] = sinkhorn(s, row_piece[r0:r1], tau=head.tau, max_iter=head.max_iter, check_pieces=False)
                if self.solver == "device":
                    continue
                buf = pinned[n_jobs % 2][:n * n].view(n, n)
                n_jobs += 1
                copy_stream.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(copy_stream):
                    buf.copy_(ds_list[b], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(copy_stream)
                ds_list[b].record_stream(copy_stream)
                if pending is not None:
                    solve(pending)
                pending = (b, buf, ev)
            if pending is not None:
                solve(pending)
            if self.solver == "device" and solved:
                import warnings

                from .matching_assign import assign_batch

                t = time.perf_counter()
                res = assign_batch([ds_list[b] for b in solved], max_steps=self.max_steps)
                status = res.status.cpu().numpy()                         # B words: the one wait for the launch
                device_s = time.perf_counter() - t
                for k, b in enumerate(solved):
                    cols[b] = res.col[k]
                    if status[k] != 0:
                        fallback.append(b)
                        t = time.perf_counter()
                        _, col = linear_sum_assignment(-ds_list[b].cpu().numpy())
                        host_s += time.perf_counter() - t
                        cols[b] = torch.from_numpy(col.astype(np.int64)).to(dev)
                    val_metrics(ds_list[b], tgt[rows[b]:rows[b + 1]], cols[b], losses[b:b + 1], counts[b])
                if fallback:
                    warnings.warn(f"device assignment: the step budget (max_steps = {'the default' if self.max_steps is None else self.max_steps}) "
                                  f"ran out for puzzle(s) {fallback} of the batch; solved on the host instead")
        mat_loss = losses.sum() / R if R else torch.zeros((), dtype=torch.float64, device=dev)
        out = {"batch_size": B, "cls_loss": cls_loss[0].clone(), "mat_loss": mat_loss, "N_": torch.tensor(n_max)}
        if self.w_rig_loss > 0 and R:
            from .matching_rigid import rigid_pairs

            part = _flatten(data_dict["part_pcs"], layout, 3, "part_pcs").index_select(0, src)
            local = (piece_of_row.cpu().numpy().astype(np.int64) - np.repeat(np.arange(B) * P, np.diff(rows)))
            keep = [b for b in range(B) if rows[b + 1] > rows[b]]
            rp = rigid_pairs([ds_list[b] for b in keep], [part[rows[b]:rows[b + 1]] for b in keep], [local[rows[b]:rows[b + 1]] for b in keep],
                             [int(n_valid[b]) for b in keep], need_grad=False)
            out["rig_loss"] = rp["rig_loss"].clone()
        elif self.w_rig_loss > 0:                      # no critical point in the batch: no pair; the key stays so that epoch_end finds it in every batch
            out["rig_loss"] = torch.zeros((), dtype=torch.float64, device=dev)
        host = torch.cat([out["cls_loss"].reshape(1), out["mat_loss"].reshape(1), c4.double(), counts.sum(0).double()]).cpu()
        torch.cuda.current_stream(dev).synchronize()
        self.timings = {"wall_s": time.perf_counter() - t0, "host_assignment_s": host_s, "device_assignment_s": device_s,
                        "fallback_puzzles": len(fallback)}
        tp4, fp4, tn4, fn4 = (host[2 + i].to(torch.float32) for i in range(4))
        ratio = lambda a, b: a / b if float(b) > 0 else torch.zeros((), dtype=torch.float32)
        out.update(cls_loss=host[0], mat_loss=host[1], loss=host[0] + host[1], cls_acc=ratio(tp4 + tn4, tp4 + fp4 + tn4 + fn4), cls_precision=ratio(tp4, tp4 + fp4),
                   cls_recall=ratio(tp4, tp4 + fn4), cls_f1=ratio(2 * tp4, 2 * tp4 + fp4 + fn4))
        if "rig_loss" in out:
            out["rig_loss"] = out["rig_loss"].cpu()
        # joint_seg_align_model.py:405-415, in float32 like the reference's `.float()` sums
        tp, fp, fn = (host[6 + i].to(torch.float32) for i in range(3))
        const = torch.tensor(1e-7)
        precision, recall = tp / (tp + fp + const), tp / (tp + fn + const)
        out.update(mat_f1=2 * precision * recall / (precision + recall + const), mat_precision=precision, mat_recall=recall)
        self.saved = {"n_critical_pcs": n_crit.reshape(B, P), "cols": cols, "counts": counts.sum(0).cpu(), "ds_mat": ds_list, "row_off": rows}
        return out

    @staticmethod
    def epoch_end(outputs: Sequence[dict]) -> dict:
        """validation_epoch_end (matching_base_model.py:65-81): the batch-size-weighted mean of every entry, keyed val/<name>"""
        sizes = torch.tensor([float(o["batch_size"]) for o in outputs], dtype=torch.float64)
        return {f"val/{k}": float((torch.stack([torch.as_tensor(o[k]).double().reshape(()) for o in outputs]) * sizes).sum() / sizes.sum())
                for k in outputs[0] if k != "batch_size"}


# ------------------------------------------------------------------------------------------------------------------ configuration
def default_config() -> dict:
    """the defaults of the reference's utils/config.py with DATA = dataset_config.py's BREAKING_BAD and MODEL = model_config.py's JIGSAW,
    restated as data (the colour table and the category list, which nothing here reads, are left out)"""
    return {
        "MODEL_NAME": "", "MODULE": "", "BATCH_SIZE": 32, "NUM_WORKERS": 8, "LOG_FILE_NAME": "", "MODEL_SAVE_PATH": "", "DATASET": "", "PROJECT": "",
        "TRAIN": {"NUM_EPOCHS": 200, "OPTIMIZER": "SGD", "LR": 0.001, "LR_SCHEDULER": "cosine", "LR_DECAY": 100.0, "LR_STEP": [10, 20],
                  "WARMUP_RATIO": 0.0, "CLIP_GRAD": None, "beta1": 0, "beta2": 0.9, "WEIGHT_DECAY": 0.0, "MOMENTUM": 0.9, "VAL_EVERY": 5, "VIS": True,
                  "VAL_SAMPLE_VIS": 5, "LOSS": ""},
        "CALLBACK": {"MATCHING_TASK": ["trans"], "CHECKPOINT_MONITOR": "val/loss", "CHECKPOINT_MODE": "min"},
        "LOSS": {}, "EVAL": {}, "GPUS": [0], "PARALLEL_STRATEGY": "ddp", "FP16": False, "CUDNN": False, "WEIGHT_FILE": "", "OUTPUT_PATH": "",
        "STATISTIC_STEP": 100, "RANDOM_SEED": 42, "STATS": "",
        "VAL_ASSIGNMENT": "host",      # not a key of the reference: the validator's assignment solver, "host" (scipy) or "device"
        "DATA": {"DATA_DIR": "../Breaking-Bad-Dataset.github.io/data/", "DATA_FN": "everyday.{}.txt", "DATA_KEYS": ("part_ids",), "SUBSET": "",
                 "CATEGORY": "", "ROT_RANGE": -1.0, "NUM_PC_POINTS": 5000, "MIN_PART_POINT": 30, "MIN_NUM_PART": 2, "MAX_NUM_PART": 20,
                 "SHUFFLE_PARTS": False, "SAMPLE_BY": "area", "LENGTH": -1, "TEST_LENGTH": -1, "OVERFIT": -1, "FRACTURE_LABEL_THRESHOLD": 0.025},
        "MODEL": {"ROT_TYPE": "rmat", "PC_FEAT_DIM": 128, "AFF_FEAT_DIM": 512, "AFFINITY": "aff_dual", "ENCODER": "pointnet2_pt.msg.dynamic",
                  "TEST_S_MASK": True, "PC_CLS_METHOD": "binary", "PC_NUM_CLS": 2, "SINKHORN_MAXITER": 20, "SINKHORN_TAU": 0.05, "TF_NUM_HEADS": 8,
                  "TF_NUM_SAMPLE": 16, "LOSS": {"w_cls_loss": 1.0, "w_mat_loss": 0.0, "mat_epoch": 9, "w_rig_loss": 0.0, "rig_epoch": 199}},
    }


def _merge(a: dict, b: dict, where: str = "") -> None:
    """_merge_a_into_b (utils/config.py:126-160): every key of a must exist in b with the same type (an int for a float is converted)"""
    for k, v in a.items():
        if k not in b:
            raise KeyError(f"{where}{k} is not a valid config key")
        if isinstance(b[k], dict) and isinstance(v, dict):
            _merge(v, b[k], f"{where}{k}.")
            continue
        if b[k] is not None and v is not None and type(b[k]) is not type(v):
            if type(b[k]) is float and type(v) is int:
                v = float(v)
            elif isinstance(b[k], (tuple, list)) and isinstance(v, (tuple, list)):
                v = type(b[k])(v)
            else:
                raise ValueError(f"Type mismatch ({type(b[k])} vs. {type(v)}) for config key: {where}{k}")
        b[k] = v


def load_config(path=None, overrides: Sequence[str] = ()) -> dict:
    """parse_args + cfg_from_file + cfg_from_list: the reference's experiment yaml over default_config(), then KEY VALUE pairs
    (dotted keys, values through ast.literal_eval, types as the defaults'), then OUTPUT_PATH / MODEL_SAVE_PATH from MODEL_NAME
    (results/<name>, results/<name>/model_save) where an override does not set them"""
    from ast import literal_eval

    cfg = default_config()
    for one in ([] if path is None else [path] if isinstance(path, str) else list(path)):          # several files merge in order
        import yaml

        with open(one, "r") as f:
            _merge(yaml.safe_load(f) or {}, cfg)
    if len(overrides) % 2:
        raise ValueError("overrides come as KEY VALUE pairs")
    given = set()
    for k, v in zip(overrides[0::2], overrides[1::2]):
        *parents, leaf = k.split(".")
        d = cfg
        for p_ in parents:
            if not isinstance(d.get(p_), dict):
                raise KeyError(f"{k}: no config section {p_}")
            d = d[p_]
        try:
            value = literal_eval(v)
        except (ValueError, SyntaxError):
            value = v
        _merge({leaf: value}, d, ".".join(parents) + "." if parents else "")
        given.add(k)
    if cfg["MODEL_NAME"]:
        import os

        if "OUTPUT_PATH" not in given:
            cfg["OUTPUT_PATH"] = os.path.join("results", cfg["MODEL_NAME"])
        if "MODEL_SAVE_PATH" not in given:
            cfg["MODEL_SAVE_PATH"] = os.path.join("results", cfg["MODEL_NAME"], "model_save")
    return cfg


def _plain(x):
    """a config as containers torch.load(weights_only=True) accepts"""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


# ------------------------------------------------------------------------------------------------------------------ checkpoints
def model_state_dict(net: torch.nn.Module, head: torch.nn.Module) -> dict:
    """the reference model's state_dict from a DescriptorNetwork and a MatchingHead: its keys, in its module order, on the CPU"""
    sd = {}
    for prefix in REFERENCE_MODULE_ORDER:
        owner = net if hasattr(net, prefix) else head
        sd.update({f"{prefix}.{k}": v.detach().cpu().clone() for k, v in getattr(owner, prefix).state_dict().items()})
    return sd


def scheduler_state(epoch: int, cfg: dict) -> dict:
    """what CosineAnnealingWarmupRestarts.state_dict() holds after the step() that closes `epoch` (the fields the class reads back)"""
    T = cfg["TRAIN"]
    total, lr = int(T["NUM_EPOCHS"]), float(T["LR"])
    done = epoch + 1
    nxt = cosine_warmup_lr(done, total, lr, T["LR_DECAY"], T["WARMUP_RATIO"], T["LR_SCHEDULER"])
    return {"first_cycle_steps": total, "cycle_mult": 1.0, "base_max_lr": lr, "max_lr": lr, "min_lr": lr / T["LR_DECAY"],
            "warmup_steps": int(total * T["WARMUP_RATIO"]), "gamma": 1.0, "cur_cycle_steps": total, "cycle": done // total,
            "step_in_cycle": done % total, "base_lrs": [lr / T["LR_DECAY"]], "last_epoch": done, "_step_count": done + 1, "_last_lr": [nxt]}


def checkpoint_dict(state_dict: dict, optimizer_state: dict, epoch: int, global_step: int, cfg: dict, callbacks: Optional[dict] = None) -> dict:
    """a Lightning checkpoint's layout: state_dict, epoch (the epoch that ended), global_step, optimizer_states, lr_schedulers,
    hyper_parameters (the cfg as plain containers: the file loads with weights_only=True), callbacks (the top-k bookkeeping)"""
    return {"epoch": int(epoch), "global_step": int(global_step), "pytorch-lightning_version": "pfpp_hip", "state_dict": state_dict,
            "optimizer_states": [optimizer_state], "lr_schedulers": [scheduler_state(epoch, cfg)] if cfg["TRAIN"]["LR_SCHEDULER"] else [],
            "hyper_parameters": {"cfg": _plain(cfg)}, "callbacks": _plain(callbacks or {})}


def load_training_checkpoint(path: str) -> dict:
    """a checkpoint file read once -> its dict (a bare state_dict stays one).  A file of tensors and plain containers loads with
    weights_only=True; a real Lightning checkpoint of the reference, whose hyper_parameters hold an EasyDict, is unpickled in full with
    the classes that are not installed replaced by a placeholder (matching.load_checkpoint_state_dict's rule), so that its optimizer
    state, epoch and global_step are resumed as train_matching.py resumes them"""
    import pickle

    from .matching import _tolerant_pickle

    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        try:
            ckpt = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_tolerant_pickle)
        except Exception as e:
            raise RuntimeError(f"{path}: not a checkpoint this loader can read ({type(e).__name__}: {e})") from e
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    if not isinstance(sd, dict) or not sd or not all(torch.is_tensor(v) for v in sd.values()):
        raise RuntimeError(f"{path}: no state_dict of tensors found")
    return ckpt


class TopK:
    """ModelCheckpoint(monitor, mode, save_top_k=10) of train_matching.py:40-49: a validation epoch's file is kept while its score is
    among the k best seen; the worst is deleted when an eleventh arrives"""

    def __init__(self, monitor: str, mode: str, k: int = 10, best: Optional[dict] = None):
        if mode not in ("min", "max"):
            raise ValueError("CHECKPOINT_MODE is 'min' or 'max'")
        self.monitor, self.mode, self.k, self.best = monitor, mode, int(k), dict(best or {})

    def offer(self, path: str, score: float) -> Tuple[bool, Optional[str]]:
        """-> (write this file?, a file to delete)"""
        worse = (lambda a, b: a > b) if self.mode == "min" else (lambda a, b: a < b)
        if math.isnan(score):
            score = math.inf if self.mode == "min" else -math.inf
        if len(self.best) < self.k:
            self.best[path] = score
            return True, None
        worst = max(self.best, key=lambda p: self.best[p]) if self.mode == "min" else min(self.best, key=lambda p: self.best[p])
        if not worse(self.best[worst], score):
            return False, None
        del self.best[worst]
        self.best[path] = score
        return True, worst


# ------------------------------------------------------------------------------------------------------------------ the loop
def _mix_seed(*words: int) -> int:
    """a 31-bit seed from (cfg seed, epoch, step, purpose): nothing process-global, so a resumed run draws what the unbroken one drew"""
    import numpy as np

    return int(np.random.SeedSequence([int(w) for w in words]).generate_state(1)[0] & 0x7FFFFFFF)


class MatcherTrainer:
    """train_matching.py's trainer.fit for one GPU: the epoch loop over build_all_piece_matching_dataloader(cfg), the three loss phases of
    training_epoch_end, validation every VAL_EVERY epochs, JSON-lines logging under OUTPUT_PATH, Lightning-layout checkpoints in
    MODEL_SAVE_PATH (model_epoch=XXX.ckpt by the top-10 rule on CALLBACK.CHECKPOINT_MONITOR, last.ckpt every epoch) and resume."""

    def __init__(self, cfg: dict, *, device="cuda", train_store=None, val_store=None, net=None, head=None):
        import os

        from .matching import DescriptorNetwork, MatchingHead
        from .matching_dataset import build_all_piece_matching_dataloader
        from .matching_encoder_train import DescriptorTrainEngine
        from .matching_rigid import MatchingHeadRigidTrainEngine

        if len(cfg["GPUS"]) != 1:
            raise NotImplementedError(f"GPUS {cfg['GPUS']}: the matcher's fit loop runs on one GPU")
        T, M = cfg["TRAIN"], cfg["MODEL"]
        if "dgcnn" in str(M["ENCODER"]).lower().split("."):
            raise NotImplementedError(f"MODEL.ENCODER {M['ENCODER']!r}: the DGCNN encoder's forward in eval mode exists (generate_matching_data / "
                                      "evaluate_matching read such a checkpoint), its training step does not")
        if M["ENCODER"] != "pointnet2_pt.msg.dynamic" or M["PC_CLS_METHOD"].lower() != "binary" or M["AFFINITY"].lower() != "aff_dual":
            raise NotImplementedError("only the reference's released configuration (PointNet++ encoder, binary classifier, dual affinity) is built")
        cosine_warmup_lr(0, T["NUM_EPOCHS"], T["LR"], T["LR_DECAY"], T["WARMUP_RATIO"], T["LR_SCHEDULER"])       # refuses an unknown scheduler now
        self.cfg, self.device, self.seed = cfg, torch.device(device), int(cfg["RANDOM_SEED"])
        self.train_loader, self.val_loader = build_all_piece_matching_dataloader(cfg, seed=self.seed, device=device, train_store=train_store,
                                                                                 val_store=val_store)
        with torch.random.fork_rng(devices=[]):         # the initial weights are a function of RANDOM_SEED, the global generator is left alone
            torch.manual_seed(self.seed)
            net = net if net is not None else DescriptorNetwork()
            head = head if head is not None else MatchingHead(tau=M["SINKHORN_TAU"], max_iter=M["SINKHORN_MAXITER"])
        self.net, self.head = net.to(self.device), head.to(self.device)
        L = M["LOSS"]
        self.descriptor_engine = DescriptorTrainEngine(self.net)
        self.head_engine = MatchingHeadRigidTrainEngine(self.head, w_cls_loss=L["w_cls_loss"], w_mat_loss=L["w_mat_loss"], w_rig_loss=L["w_rig_loss"])
        self.optimizer = MatcherOptimizer(self.descriptor_engine, self.head_engine, weight_decay=T["WEIGHT_DECAY"], clip_grad=T["CLIP_GRAD"])
        self.topk = TopK(cfg["CALLBACK"]["CHECKPOINT_MONITOR"], cfg["CALLBACK"]["CHECKPOINT_MODE"])
        self.epoch, self.global_step = 0, 0            # the next epoch to run
        self.last_val: Optional[dict] = None
        self.out_dir, self.save_dir = cfg["OUTPUT_PATH"] or ".", cfg["MODEL_SAVE_PATH"] or "."
        os.makedirs(self.out_dir, exist_ok=True)
        os.makedirs(self.save_dir, exist_ok=True)
        self.log_path = os.path.join(self.out_dir, "train_log.jsonl")

    # ---- pieces
    def lr(self, epoch: int) -> float:
        T = self.cfg["TRAIN"]
        return cosine_warmup_lr(epoch, T["NUM_EPOCHS"], T["LR"], T["LR_DECAY"], T["WARMUP_RATIO"], T["LR_SCHEDULER"])

    def _log(self, record: dict) -> None:
        import json

        with open(self.log_path, "a") as f:
            f.write(json.dumps(record) + "\n")

    def train_step(self, d: dict, lr: float, seed: int) -> dict:
        from .matching_train import MatchingHeadLoss

        feats = self.descriptor_engine.forward(d["part_pcs"], d["n_pcs"], d["part_valids"], seed=seed)
        loss = MatchingHeadLoss.apply(feats, self.head_engine, d["gt_pcs"], d["n_pcs"], d["part_valids"], d["critical_label_thresholds"], None,
                                      d["part_pcs"])
        loss.backward()
        self.optimizer.step(lr)
        return {k: (float(v) if torch.is_tensor(v) else v) for k, v in self.head_engine.last_loss_dict.items()}

    def validate(self, epoch: int) -> dict:
        validator = MatcherValidator(self.net, self.head, w_rig_loss=self.head_engine.w_rig_loss, solver=self.cfg["VAL_ASSIGNMENT"])
        self.val_loader.set_epoch(0)                   # the same validation samples every time: the figures of two epochs compare
        outs = [validator.step(d, seed=_mix_seed(self.seed, 0, i, 2)) for i, d in enumerate(self.val_loader)]
        return MatcherValidator.epoch_end(outs)

    def checkpoint(self, epoch: int) -> dict:
        return checkpoint_dict(model_state_dict(self.net, self.head), self.optimizer.state_dict(self.lr(epoch + 1)), epoch, self.global_step, self.cfg,
                               {"ModelCheckpoint": {"monitor": self.topk.monitor, "best_k_models": self.topk.best}})

    # ---- resume (train_matching.py:78-101)
    def resume(self) -> Optional[str]:
        """WEIGHT_FILE when set (a full checkpoint is resumed, bare weights are loaded), else the newest model_* / last* file of
        MODEL_SAVE_PATH; -> the file used"""
        import os

        path = self.cfg["WEIGHT_FILE"]
        if not path:
            files = [f for f in os.listdir(self.save_dir) if "model_" in f or "last" in f]
            if not files:
                return None
            path = os.path.join(self.save_dir, max(files, key=lambda f: os.path.getmtime(os.path.join(self.save_dir, f))))
        from .matching import DESCRIPTOR_PREFIXES

        ckpt = load_training_checkpoint(path)
        sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
        self.net.load_state_dict({k: v for k, v in sd.items() if k.startswith(DESCRIPTOR_PREFIXES)}, strict=True)
        self.head.load_state_dict({k: v for k, v in sd.items() if not k.startswith(DESCRIPTOR_PREFIXES)}, strict=True)
        if isinstance(ckpt, dict) and "optimizer_states" in ckpt:
            self.optimizer.load_state_dict(ckpt["optimizer_states"][0])
            self.epoch, self.global_step = int(ckpt["epoch"]) + 1, int(ckpt["global_step"])
            best = (ckpt.get("callbacks") or {}).get("ModelCheckpoint")          # this tree's files; Lightning's own callback keys are not read
            self.topk.best = {k: float(v) for k, v in (best or {}).get("best_k_models", {}).items()}
            L = self.cfg["MODEL"]["LOSS"]
            for e in range(self.epoch):                # the loss weights are a function of the epochs that ended
                self.head_engine.on_epoch_end(e, L["mat_epoch"], L["rig_epoch"])
        return path

    # ---- the loop
    def fit(self, max_epochs: Optional[int] = None) -> None:
        import os

        T, L = self.cfg["TRAIN"], self.cfg["MODEL"]["LOSS"]
        end = int(T["NUM_EPOCHS"]) if max_epochs is None else min(int(T["NUM_EPOCHS"]), int(max_epochs))
        while self.epoch < end:
            epoch, lr = self.epoch, self.lr(self.epoch)
            self.train_loader.set_epoch(epoch)
            sums, n = {}, 0
            for i, d in enumerate(self.train_loader):
                rec = self.train_step(d, lr, _mix_seed(self.seed, epoch, i, 1))
                self.global_step += 1
                self._log({"kind": "step", "epoch": epoch, "step": self.global_step, "lr": lr, **{f"train/{k}": v for k, v in rec.items()}})
                for k, v in rec.items():
                    sums[k] = sums.get(k, 0.0) + float(v)
                n += 1
            # Lightning runs the validation loop before training_epoch_end: the validation of epoch == rig_epoch still has no rig_loss
            val = self.validate(epoch) if (epoch + 1) % int(T["VAL_EVERY"]) == 0 else None
            self.head_engine.on_epoch_end(epoch, L["mat_epoch"], L["rig_epoch"])
            record = {"kind": "epoch", "epoch": epoch, "lr": lr, "steps": n, **{f"train/{k}": v / max(n, 1) for k, v in sums.items()},
                      "w_mat_loss": self.head_engine.w_mat_loss, "w_rig_loss": self.head_engine.w_rig_loss}
            ckpt = None
            if val is not None:
                self.last_val = val
                record.update(self.last_val)
                name = os.path.join(self.save_dir, f"model_epoch={epoch:03d}.ckpt")
                monitor = self.topk.monitor
                if monitor not in self.last_val:
                    raise KeyError(f"CALLBACK.CHECKPOINT_MONITOR {monitor!r} is not a validation figure ({sorted(self.last_val)})")
                write, drop = self.topk.offer(name, self.last_val[monitor])
                if drop is not None and os.path.exists(drop):
                    os.remove(drop)
                ckpt = self.checkpoint(epoch)
                if write:
                    torch.save(ckpt, name)
            torch.save(ckpt if ckpt is not None else self.checkpoint(epoch), os.path.join(self.save_dir, "last.ckpt"))
            self._log(record)
            self.epoch = epoch + 1


def fit(cfg: dict, *, resume: bool = True, max_epochs: Optional[int] = None, **kw) -> MatcherTrainer:
    """train the matcher as train_matching.py does: build, resume from WEIGHT_FILE or the newest checkpoint, run the epochs"""
    trainer = MatcherTrainer(cfg, **kw)
    if resume:
        trainer.resume()
    trainer.fit(max_epochs)
    return trainer
