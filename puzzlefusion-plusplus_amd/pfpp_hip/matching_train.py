"""Training of the matcher's head behind part_feats (csrc/matching_train.hip, include/pfpp.h "matcher head, training").

The training-time forward of the reference's Jigsaw_matching/model/jigsaw/joint_seg_align_model.py:164-268 behind the descriptor
network, its _loss_function (:280-426), the backward of both and Adam (model/modules/matching_base_model.py:499-515):

* sinkhorn_train / gt_targets / normalize_halves_bwd / cls_bce / gather_raw / scatter_raw / colsum_ordered: the kernels on their own.
* MatchingHeadTrainEngine: one step over a ragged batch.  Both BatchNorms run on batch statistics (the affinity extractor's over the
  B N'_max rows of the zero-padded critical_feats, as in the reference), the critical points come from the ground-truth labels, s is
  not masked, no assignment is solved.  The Sinkhorn backward keeps max_iter potential vectors and one N' x N' matrix per puzzle
  where autograd keeps max_iter matrices.
* MatchingHeadLoss: the engine as a torch.autograd.Function of part_feats.

The rigid term of the loss (w_rig_loss, the reference's last 50 epochs) is matching_rigid.MatchingHeadRigidTrainEngine's: _step below
takes that class's factory of a RigidBatch and then runs the per-puzzle loop in three stages.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from . import train_ops as T
from ._lib import check
from .matching import AFF_FEAT_DIM, PC_FEAT_DIM, MatchingHead, _flatten, _gpu, _p, critical_points, fracture_labels, make_layout
from .vqvae_train import bn_relu_bwd

HALF = AFF_FEAT_DIM // 2


def _mm(A, W, out, *, M, N, K, lda, ldw, ldc, w_kmajor=False, w_off=0, c_off=0):
    """out[M, N] = A[M, K] . W^T (W [N, K], or [K, N] with w_kmajor) on the exact-fp32 matrix instructions: the head's arithmetic"""
    return ops.gemm(A, W, M=M, N=N, K=K, lda=lda, ldw=ldw, out=out, ldc=ldc, w_kmajor=w_kmajor, w_off=w_off, c_off=c_off, mode="f32")


def _tpad(x: torch.Tensor) -> torch.Tensor:
    """x [r, c] (any strides) -> its transpose [c, r rounded up to 4] with zero padding: the A operand of a product that contracts over rows"""
    r, c = x.shape
    out = torch.zeros((c, (r + 3) & ~3), dtype=x.dtype, device=x.device)
    out[:, :r] = x.t()
    return out


# ------------------------------------------------------------------------------------------------------------------ kernels
def _sinkhorn_ws(n: int, device) -> torch.Tensor:
    nbytes = _lib.load().pfpp_sinkhorn_train_workspace(n)
    if nbytes < 0:
        raise ValueError(f"sinkhorn_train: n = {n} is outside what the kernels are built for")
    return torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.float64, device=device)


def _check_s(s: torch.Tensor, tgt: torch.Tensor) -> int:
    _gpu(s, torch.float32, "s")
    _gpu(tgt, torch.int32, "tgt")
    if s.dim() != 2 or s.shape[0] != s.shape[1] or s.stride(1) != 1 or s.shape[0] < 1:
        raise ValueError(f"s: expected a square matrix with contiguous rows, got {tuple(s.shape)}")
    if tgt.shape != (s.shape[0],) or not tgt.is_contiguous():
        raise ValueError("tgt: one target column per row")
    return s.shape[0]


def sinkhorn_train_fwd(s: torch.Tensor, tgt: torch.Tensor, *, tau: float = 0.05, max_iter: int = 20, loss_out: Optional[torch.Tensor] = None,
                       row_loss: Optional[torch.Tensor] = None):
    """unmasked log-domain Sinkhorn of one puzzle and its permutation loss: s float32 [n, n] (rows may be strided), tgt int32 [n]
    (-1 = no target) -> (ds_mat float32 [n, n], loss float64 [1] = sum_ij BCE(ds_mat_ij, [j == tgt_i]), pots float64 [max_iter, n]);
    row_loss (float64 [n], optional) receives the rows' shares of the loss"""
    n = _check_s(s, tgt)
    dev = s.device
    if row_loss is not None:
        ops._chk(row_loss, torch.float64, "row_loss")
        if row_loss.shape != (n,):
            raise ValueError("row_loss: one number per row")
    pots = torch.empty((max(int(max_iter), 1), n), dtype=torch.float64, device=dev)
    ds_mat = torch.empty((n, n), dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev) if loss_out is None else loss_out
    ws = _sinkhorn_ws(n, dev)
    check(_lib.load().pfpp_sinkhorn_train_fwd(_p(s), s.stride(0), n, float(tau), int(max_iter), _p(tgt), _p(pots), _p(ds_mat), _p(loss), _p(row_loss),
                                              _p(ws), ws.numel() * 8, ops._stream()), "pfpp_sinkhorn_train_fwd")
    return ds_mat, loss, pots


def sinkhorn_train_bwd(s: torch.Tensor, tgt: torch.Tensor, pots: torch.Tensor, ds_mat: torch.Tensor, *, g: float = 1.0, tau: float = 0.05,
                       max_iter: int = 20, padded: bool = False, seed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g dLoss / ds of sinkhorn_train_fwd from the potentials it kept -> float32 [n, n]: a view of a buffer whose rows are padded to 4
    floats with zeros, the layout the GEMMs read (padded=True returns that buffer, [n, (n + 3) & ~3]).  seed (float32 [n, (n + 3) & ~3],
    zero padding columns): dLoss' / d ds_mat of a further term; the result is the gradient of both and is written over seed"""
    n = _check_s(s, tgt)
    _gpu(pots, torch.float64, "pots")
    _gpu(ds_mat, torch.float32, "ds_mat")
    if pots.shape != (max(int(max_iter), 1), n) or not pots.is_contiguous() or ds_mat.shape != (n, n) or not ds_mat.is_contiguous():
        raise ValueError("pots / ds_mat: not what sinkhorn_train_fwd returned for this s and max_iter")
    ldg = (n + 3) & ~3
    ws = _sinkhorn_ws(n, s.device)
    if seed is not None:
        _gpu(seed, torch.float32, "seed")
        if seed.shape != (n, ldg) or not seed.is_contiguous():
            raise ValueError(f"seed: expected the padded buffer [{n}, {ldg}], got {tuple(seed.shape)}")
        G = seed
        check(_lib.load().pfpp_sinkhorn_train_bwd_seeded(_p(s), s.stride(0), n, float(tau), int(max_iter), _p(tgt), _p(pots), _p(ds_mat), float(g),
                                                         _p(G), ldg, _p(ws), ws.numel() * 8, ops._stream()), "pfpp_sinkhorn_train_bwd_seeded")
        return G if padded else G[:, :n]
    G = torch.empty((n, ldg), dtype=torch.float32, device=s.device)
    if ldg > n:
        G[:, n:].zero_()
    check(_lib.load().pfpp_sinkhorn_train_bwd(_p(s), s.stride(0), n, float(tau), int(max_iter), _p(tgt), _p(pots), _p(ds_mat), float(g), _p(G), ldg,
                                              _p(ws), ws.numel() * 8, ops._stream()), "pfpp_sinkhorn_train_bwd")
    return G if padded else G[:, :n]


def gt_targets(gt_pcs: torch.Tensor, src: torch.Tensor, row_piece: torch.Tensor, puz_row_off: torch.Tensor, max_rows: int) -> torch.Tensor:
    """gt_pcs float32 [N, 3]; src int64 [R] = the global point index of every critical row (puzzle by puzzle), row_piece int32 [R] its
    piece, puz_row_off int64 [B + 1] -> tgt int32 [R]: the puzzle-local column of the nearest critical point of another piece, or -1"""
    _gpu(gt_pcs, torch.float32, "gt_pcs"); _gpu(src, torch.int64, "src"); _gpu(row_piece, torch.int32, "row_piece")
    _gpu(puz_row_off, torch.int64, "puz_row_off")
    if gt_pcs.dim() != 2 or gt_pcs.shape[1] != 3 or not gt_pcs.is_contiguous() or row_piece.shape != src.shape:
        raise ValueError("gt_targets: gt_pcs [N, 3] contiguous, one piece per row")
    tgt = torch.empty(src.numel(), dtype=torch.int32, device=gt_pcs.device)
    check(_lib.load().pfpp_match_gt_targets(_p(gt_pcs), gt_pcs.shape[0], _p(src.contiguous()), _p(row_piece.contiguous()), _p(puz_row_off.contiguous()),
                                            puz_row_off.numel() - 1, int(max_rows), _p(tgt), ops._stream()), "pfpp_match_gt_targets")
    return tgt


def normalize_halves_bwd(x: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """backward of F.normalize(p=2, eps=1e-12) on both 256-wide halves from the rows x [R, 512] before the normalisation"""
    ops._chk(x, torch.float32, "x"); ops._chk(dy, torch.float32, "dy")
    if x.shape != dy.shape or x.dim() != 2:
        raise ValueError("normalize_halves_bwd: x and dy [R, 512]")
    dx = torch.empty_like(dy) if out is None else out
    check(_lib.load().pfpp_match_normalize_halves_bwd(_p(x), _p(dy), _p(dx), x.shape[0], x.shape[1], ops._stream()), "pfpp_match_normalize_halves_bwd")
    return dx


def cls_bce(logits: torch.Tensor, labels: torch.Tensor, *, g: float = 1.0, need_grad: bool = True, dlogit: Optional[torch.Tensor] = None):
    """logits float32 [N] or a column [N, ld][:, 0], labels uint8 [N] -> (mean BCE-with-logits float64 [1], dlogit = g dLoss / dlogit
    (same strides as given, or [N]), counts int64 [4] = (tp, fp, tn, fn) of sigmoid(logit) > 0.5)"""
    _gpu(logits, torch.float32, "logits"); ops._chk(labels, torch.uint8, "labels")
    N = labels.numel()
    if logits.dim() != 1 or logits.numel() != N or N < 1:
        raise ValueError("cls_bce: one logit per label")
    dev = logits.device
    if need_grad and dlogit is None:
        dlogit = torch.empty(N, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.pfpp_match_cls_bce_workspace() // 8, dtype=torch.float64, device=dev)
    check(lib.pfpp_match_cls_bce(_p(logits), logits.stride(0), _p(labels), N, float(g), _p(loss), _p(dlogit if need_grad else None),
                                 dlogit.stride(0) if need_grad else 0, _p(counts), _p(ws), ws.numel() * 8, ops._stream()), "pfpp_match_cls_bce")
    return loss, dlogit, counts


def gather_raw(feats: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out [R, 128] = feats[idx[r]] without BatchNorm or ReLU; a zero row where idx[r] < 0"""
    ops._chk(feats, torch.float32, "feats"); ops._chk(idx, torch.int64, "idx")
    out = torch.empty((idx.numel(), feats.shape[1]), dtype=torch.float32, device=feats.device)
    check(_lib.load().pfpp_match_gather_raw(_p(feats), _p(idx), feats.shape[0], idx.numel(), feats.shape[1], _p(out), ops._stream()),
          "pfpp_match_gather_raw")
    return out


def scatter_raw(rows: torch.Tensor, idx: torch.Tensor, out: torch.Tensor, *, accumulate: bool = False) -> torch.Tensor:
    """out[idx[r]] = (or +=) rows[r] for idx[r] >= 0; every point at most once"""
    ops._chk(rows, torch.float32, "rows"); ops._chk(idx, torch.int64, "idx"); ops._chk(out, torch.float32, "out")
    if rows.shape != (idx.numel(), out.shape[1]):
        raise ValueError("scatter_raw: one row per index")
    check(_lib.load().pfpp_match_scatter_raw(_p(rows), _p(idx), out.shape[0], idx.numel(), out.shape[1], int(accumulate), _p(out), ops._stream()),
          "pfpp_match_scatter_raw")
    return out


def colsum_ordered(x: torch.Tensor) -> torch.Tensor:
    """out[c] = sum_r x[r, c] of x float32 [rows, cols] in a fixed order (fp64 partials per 64 rows, folded in order): the bias
    gradients, which two runs of a step then give bit for bit (train_ops.colsum ends in float atomics)"""
    _gpu(x, torch.float32, "x")
    if x.dim() != 2 or (x.numel() and x.stride(1) != 1):
        raise ValueError("colsum_ordered: x [rows, cols] with contiguous rows")
    rows, cols = x.shape
    if rows == 0:
        return torch.zeros(cols, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    out = torch.empty(cols, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(lib.pfpp_match_colsum_ordered_workspace(rows, cols) // 8, 1), dtype=torch.float64, device=x.device)
    check(lib.pfpp_match_colsum_ordered(_p(x), x.stride(0), rows, cols, _p(out), _p(ws), ws.numel() * 8, ops._stream()), "pfpp_match_colsum_ordered")
    return out


# ------------------------------------------------------------------------------------------------------------------ the engine
PARAM_NAMES = ("pc_classifier.0.weight", "pc_classifier.0.bias", "pc_classifier.2.weight", "pc_classifier.2.bias",
               "affinity_extractor.0.weight", "affinity_extractor.0.bias", "affinity_extractor.2.weight", "affinity_extractor.2.bias",
               "affinity_layer.A")


class MatchingHeadTrainEngine:
    """one training step of a MatchingHead: loss_and_grads() leaves the gradients in the .grad of the head's own parameters and
    returns d loss / d part_feats; optimizer_step() is torch.optim.Adam (weight decay 0) through pfpp_adamw.  The head's arithmetic
    (head.gemm_mode, "f32" by default), tau and max_iter are the head's.  `saved` keeps the last step's intermediate tensors (the two
    ReLU outputs among them: the tests feed their sign pattern to the float64 reference)."""

    _RIGID = False        # MatchingHeadRigidTrainEngine (matching_rigid.py) has the rigid term; this class refuses it

    def __init__(self, head: MatchingHead, *, w_cls_loss: float = 1.0, w_mat_loss: float = 0.0, w_rig_loss: float = 0.0):
        if w_rig_loss > 0 and not self._RIGID:
            raise NotImplementedError("w_rig_loss > 0: rigid_loss (utils/loss.py:59) needs part_pcs, which this engine's loss_and_grads does not "
                                      "take: use pfpp_hip.matching_rigid.MatchingHeadRigidTrainEngine")
        if head.gemm_mode != "f32":
            raise NotImplementedError("the head's training runs in the exact-fp32 GEMM mode only")
        self.head = head
        self.w_cls_loss, self.w_mat_loss, self.w_rig_loss = float(w_cls_loss), float(w_mat_loss), float(w_rig_loss)
        self.params: Dict[str, torch.nn.Parameter] = dict(head.named_parameters())
        if tuple(self.params) != PARAM_NAMES:
            raise ValueError(f"not a MatchingHead: parameters {list(self.params)}")
        self.state: Dict[str, Tuple[torch.Tensor, torch.Tensor, int]] = {}
        self.saved: dict = {}

    # ---- forward + backward
    def loss_and_grads(self, part_feats, gt_pcs, n_pcs, part_valids, *, critical_label_thresholds=None, critical_label=None):
        """part_feats float32 [B, N, 128] (or a list / flat), gt_pcs float32 [..., 3] likewise, n_pcs int [B, P], part_valids [B, P];
        critical_label ([B, N] or flat, non-zero = critical) or the thresholds compute_label takes -> (loss_dict, d_part_feats [sum N, 128]).
        loss_dict has the reference's keys; its three losses are 0-dim fp64 tensors on the device (the sums they come from are fp64)"""
        return self._step(part_feats, gt_pcs, n_pcs, part_valids, critical_label_thresholds, critical_label, None)

    def _step(self, part_feats, gt_pcs, n_pcs, part_valids, critical_label_thresholds, critical_label, make_rigid):
        """loss_and_grads; make_rigid (None, or a subclass's factory (counts, n_valid, row_off, src, device) -> an object with
        pair_sums(b, ds_mat), pose_and_fold(w), grad(b), fold and records(): matching_rigid.RigidBatch) switches the rigid term on: the
        per-puzzle loop then runs in three stages (forwards and pair sums, poses and fold, backwards) because the term's scale 1 / n_sum
        is batch-global"""
        first = part_feats[0] if isinstance(part_feats, (list, tuple)) else part_feats
        _gpu(first, torch.float32, "part_feats")
        dev = first.device
        layout = make_layout(n_pcs, dev)
        feats = _flatten(part_feats, layout, PC_FEAT_DIM, "part_feats")
        gfirst = gt_pcs[0] if isinstance(gt_pcs, (list, tuple)) else gt_pcs
        _gpu(gfirst, torch.float32, "gt_pcs")
        pts = _flatten(gt_pcs, layout, 3, "gt_pcs")
        B, P = layout.n_pcs.shape
        pv = np.asarray(part_valids.detach().cpu().numpy() if torch.is_tensor(part_valids) else part_valids)
        n_valid = pv.reshape(B, P).sum(1).astype(np.int64)
        for b in range(B):
            if layout.n_pcs[b, n_valid[b]:].any():
                raise ValueError(f"puzzle {b}: points in a slot behind its {n_valid[b]} valid pieces")
        N = feats.shape[0]
        if N < 2:
            raise ValueError("a training batch needs at least two points (BatchNorm on batch statistics)")
        if critical_label is None:
            if critical_label_thresholds is None:
                raise ValueError("either critical_label or critical_label_thresholds is needed")
            labels = fracture_labels(gt_pcs, n_pcs, critical_label_thresholds).reshape(-1).to(torch.uint8)
        else:
            lab = torch.cat([t.reshape(-1) for t in critical_label]) if isinstance(critical_label, (list, tuple)) else critical_label
            if not torch.is_tensor(lab) or not lab.is_cuda or lab.numel() != N:
                raise ValueError("critical_label: one label per point, on the GPU")
            labels = (lab.reshape(-1) != 0).to(torch.uint8)
        head, lib = self.head, _lib.load()
        matching = self.w_mat_loss != 0                       # joint_seg_align_model.py:221-223, :325-327: the classifier phase otherwise
        g_cls = self.w_cls_loss if matching else 1.0
        grads: Dict[str, Optional[torch.Tensor]] = {k: None for k in PARAM_NAMES}
        f32 = dict(dtype=torch.float32, device=dev)

        # ---- classifier over all points: BatchNorm (batch statistics) + ReLU + Conv1d(128, 1, 1), BCE with logits
        bn, conv = head.pc_classifier[0], head.pc_classifier[2]
        gam, bet = bn.weight.detach(), bn.bias.detach()
        mean_c, var_c = T.bn_stats(feats, bn.running_mean, bn.running_var, momentum=bn.momentum)
        bn.num_batches_tracked += 1
        h_c = T.bn_apply(feats, mean_c, var_c, gam, bet, eps=bn.eps)
        w4 = torch.zeros((4, PC_FEAT_DIM), **f32)             # the 1-wide convolution as a 4-wide GEMM (rows 1 - 3 zero): 16-byte rows
        w4[0] = conv.weight.detach().reshape(-1)
        b4 = torch.zeros(4, **f32)
        b4[0] = conv.bias.detach().reshape(())
        logits4 = ops.linear(h_c, w4, b4, mode=head.gemm_mode)
        dlog4 = torch.zeros((N, 4), **f32)
        cls_loss, _, counts = cls_bce(logits4[:, 0], labels, g=g_cls, dlogit=dlog4[:, 0])
        d_hc = _mm(dlog4, w4, torch.empty((N, PC_FEAT_DIM), **f32), M=N, N=PC_FEAT_DIM, K=4, lda=4, ldw=PC_FEAT_DIM, ldc=PC_FEAT_DIM, w_kmajor=True)
        dlog_t = _tpad(dlog4)
        dw4 = _mm(dlog_t, h_c, torch.empty((4, PC_FEAT_DIM), **f32), M=4, N=PC_FEAT_DIM, K=N, lda=dlog_t.shape[1], ldw=PC_FEAT_DIM, ldc=PC_FEAT_DIM,
                  w_kmajor=True)
        db4 = colsum_ordered(dlog4)
        dgam, dbet = torch.zeros(PC_FEAT_DIM, **f32), torch.zeros(PC_FEAT_DIM, **f32)
        d_feats = bn_relu_bwd(feats, d_hc, mean_c, var_c, gam, bet, dgam, dbet, eps=bn.eps)
        grads.update({"pc_classifier.0.weight": dgam, "pc_classifier.0.bias": dbet, "pc_classifier.2.weight": dw4[0].reshape(1, PC_FEAT_DIM, 1),
                      "pc_classifier.2.bias": db4[:1]})
        self.saved = {"h_cls": h_c, "logits": logits4[:, 0], "labels": labels}

        tp, fp, tn, fn = (counts[i].to(torch.float32) for i in range(4))
        ratio = lambda a, b: torch.where(b > 0, a / b.clamp_min(1), torch.zeros_like(a))
        loss_dict = {"batch_size": B, "cls_loss": cls_loss[0].clone(), "cls_acc": ratio(tp + tn, tp + fp + tn + fn), "cls_precision": ratio(tp, tp + fp),
                     "cls_recall": ratio(tp, tp + fn), "cls_f1": ratio(2 * tp, 2 * tp + fp + fn)}
        if not matching:
            loss_dict["loss"] = loss_dict["cls_loss"]
            self._store(grads)
            return loss_dict, d_feats

        # ---- critical points of the ground-truth labels, in piece order
        _, n_crit = critical_points(labels, layout)
        nc = n_crit.cpu().numpy().reshape(B, P)                # the one read-back: the matrices are allocated from it
        n_b = nc.sum(1).astype(np.int64)
        row_off = np.concatenate([[0], np.cumsum(n_b)]).astype(np.int64)
        R, n_max = int(row_off[-1]), int(n_b.max(initial=0))
        zero_like = lambda k: torch.zeros_like(self.params[k])
        if R == 0:                                             # the reference divides 0 by 0 here: no matching term, zero gradients
            for k in PARAM_NAMES[4:]:
                grads[k] = zero_like(k)
            mat_loss = torch.zeros((), dtype=torch.float64, device=dev)
            loss_dict.update(mat_loss=mat_loss, N_=torch.tensor(0), loss=self.w_cls_loss * cls_loss[0])
            if make_rigid is not None:                         # no pair at all: 0 / 0 in the reference's rigid term too
                loss_dict["rig_loss"] = torch.zeros((), dtype=torch.float64, device=dev)
            self._store(grads)
            return loss_dict, d_feats
        src = torch.nonzero(labels).reshape(-1)                # global point index of every critical row: puzzle, piece, point order
        row_piece = torch.bucketize(src, layout.piece_off[1:], right=True).to(torch.int32)
        Rp = B * n_max                                         # critical_feats is zero-padded to the largest N' (:113-116) ...
        pad_src = torch.full((Rp,), -1, dtype=torch.int64, device=dev)
        for b in range(B):
            pad_src[b * n_max:b * n_max + int(n_b[b])] = src[row_off[b]:row_off[b + 1]]
        tgt = gt_targets(pts, src, row_piece, torch.from_numpy(row_off).to(dev), n_max)

        # ---- affinity extractor over the padded rows: ... so its BatchNorm statistics count the zero rows too
        bna, conva = head.affinity_extractor[0], head.affinity_extractor[2]
        gam_a, bet_a = bna.weight.detach(), bna.bias.detach()
        xg = gather_raw(feats, pad_src)
        mean_a, var_a = T.bn_stats(xg, bna.running_mean, bna.running_var, momentum=bna.momentum)
        bna.num_batches_tracked += 1
        h_a = T.bn_apply(xg, mean_a, var_a, gam_a, bet_a, eps=bna.eps)
        w_a = conva.weight.detach().reshape(AFF_FEAT_DIM, PC_FEAT_DIM)
        f_pre = ops.linear(h_a, w_a, conva.bias.detach(), mode=head.gemm_mode)
        f = f_pre.clone()
        check(lib.pfpp_match_normalize_halves(_p(f), Rp, AFF_FEAT_DIM, ops._stream()), "pfpp_match_normalize_halves")
        pa = head.primal_times_a(f)

        # ---- per puzzle: affinity, Sinkhorn + loss, and straight on to its backward and the affinity's
        A = head.affinity_layer.A.detach()
        losses = torch.zeros(B, dtype=torch.float64, device=dev)
        dpa = torch.zeros((Rp, HALF), **f32)
        df = torch.zeros((Rp, AFF_FEAT_DIM), **f32)
        g_mat = self.w_mat_loss / R
        ds_mats = []

        def forward(b, n):
            r0 = b * n_max
            t_b = tgt[row_off[b]:row_off[b + 1]]
            s = head.affinity(f, r0, r0 + n, pa)
            ds_mat, _, pots = sinkhorn_train_fwd(s, t_b, tau=head.tau, max_iter=head.max_iter, loss_out=losses[b:b + 1])
            return s, t_b, pots, ds_mat

        def affinity_backward(b, n, G):
            r0, ldg = b * n_max, G.shape[1]
            # dM = ds X2, into its rows of dpa; dX2^T = (X1 A)^T ds, which reads ds as it lies ([K, N]) and transposes [n, 256] matrices only
            _mm(G, f, dpa, M=n, N=HALF, K=n, lda=ldg, ldw=AFF_FEAT_DIM, ldc=HALF, w_kmajor=True, w_off=r0 * AFF_FEAT_DIM + HALF, c_off=r0 * HALF)
            pa_t = _tpad(pa[r0:r0 + n])
            dx2_t = _mm(pa_t, G, torch.empty((HALF, ldg), **f32), M=HALF, N=n, K=n, lda=ldg, ldw=ldg, ldc=ldg, w_kmajor=True)
            df[r0:r0 + n, HALF:] = dx2_t[:, :n].t()

        rigid = None
        if make_rigid is None:
            for b in range(B):
                n = int(n_b[b])
                if n == 0:                                     # a puzzle without critical points contributes nothing
                    ds_mats.append(torch.empty((0, 0), **f32))
                    continue
                s, t_b, pots, ds_mat = forward(b, n)
                G = sinkhorn_train_bwd(s, t_b, pots, ds_mat, g=g_mat, tau=head.tau, max_iter=head.max_iter, padded=True)
                affinity_backward(b, n, G)
                ds_mats.append(ds_mat)
        else:
            # the rigid term: its scale w_rig_loss / n_sum is a sum over the whole batch and stays on the device, so every puzzle's
            # forward and pair sums come first, then the poses and the fold, then the backwards; s, pots and ds_mat are kept meanwhile
            rigid = make_rigid(nc, n_valid, row_off, src, dev)
            kept = []
            for b in range(B):
                n = int(n_b[b])
                if n == 0:
                    ds_mats.append(torch.empty((0, 0), **f32))
                    kept.append(None)
                    continue
                kept.append(forward(b, n))
                rigid.pair_sums(b, kept[b][3])
                ds_mats.append(kept[b][3])
            rigid.pose_and_fold(self.w_rig_loss)
            for b in range(B):
                if kept[b] is None:
                    continue
                s, t_b, pots, ds_mat = kept[b]
                G = sinkhorn_train_bwd(s, t_b, pots, ds_mat, g=g_mat, tau=head.tau, max_iter=head.max_iter, padded=True, seed=rigid.grad(b))
                affinity_backward(b, int(n_b[b]), G)
                kept[b] = None
        mat_loss = losses.sum() / R
        # dX1 = dM A^T for all rows; dA = X1^T dM
        _mm(dpa, A.contiguous(), df, M=Rp, N=HALF, K=HALF, lda=HALF, ldw=HALF, ldc=AFF_FEAT_DIM)
        x1_t = _tpad(f[:, :HALF])
        d_a = _mm(x1_t, dpa, torch.empty((HALF, HALF), **f32), M=HALF, N=HALF, K=Rp, lda=x1_t.shape[1], ldw=HALF, ldc=HALF, w_kmajor=True)
        normalize_halves_bwd(f_pre, df, out=df)
        d_ha = _mm(df, w_a, torch.empty((Rp, PC_FEAT_DIM), **f32), M=Rp, N=PC_FEAT_DIM, K=AFF_FEAT_DIM, lda=AFF_FEAT_DIM, ldw=PC_FEAT_DIM,
                   ldc=PC_FEAT_DIM, w_kmajor=True)
        df_t = _tpad(df)
        dw_a = _mm(df_t, h_a, torch.empty((AFF_FEAT_DIM, PC_FEAT_DIM), **f32), M=AFF_FEAT_DIM, N=PC_FEAT_DIM, K=Rp, lda=df_t.shape[1], ldw=PC_FEAT_DIM,
                   ldc=PC_FEAT_DIM, w_kmajor=True)
        db_a = colsum_ordered(df)
        dgam_a, dbet_a = torch.zeros(PC_FEAT_DIM, **f32), torch.zeros(PC_FEAT_DIM, **f32)
        d_xg = bn_relu_bwd(xg, d_ha, mean_a, var_a, gam_a, bet_a, dgam_a, dbet_a, eps=bna.eps)
        scatter_raw(d_xg, pad_src, d_feats, accumulate=True)
        grads.update({"affinity_extractor.0.weight": dgam_a, "affinity_extractor.0.bias": dbet_a,
                      "affinity_extractor.2.weight": dw_a.reshape(AFF_FEAT_DIM, PC_FEAT_DIM, 1), "affinity_extractor.2.bias": db_a, "affinity_layer.A": d_a})
        self.saved.update(h_aff=h_a, ds_mat=ds_mats, targets=tgt, row_off=row_off, pad_src=pad_src, n_critical_pcs=n_crit.reshape(B, P))
        loss_dict.update(mat_loss=mat_loss, N_=torch.tensor(n_max), loss=self.w_cls_loss * cls_loss[0] + self.w_mat_loss * mat_loss)
        if rigid is not None:
            rig_loss = rigid.fold[0].clone()
            loss_dict.update(rig_loss=rig_loss, loss=loss_dict["loss"] + self.w_rig_loss * rig_loss)
            self.saved.update(rigid.records())
        self._store(grads)
        return loss_dict, d_feats

    def _store(self, grads: Dict[str, Optional[torch.Tensor]]) -> None:
        for k, p in self.params.items():
            p.grad = None if grads[k] is None else grads[k].reshape(p.shape).contiguous()

    # ---- Adam
    def optimizer_step(self, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
        """torch.optim.Adam (the reference's optimizer when WEIGHT_DECAY is 0) over the parameters that have a gradient"""
        lib = _lib.load()
        for k, p in self.params.items():
            if p.grad is None:
                continue
            ops._chk(p.data, torch.float32, k)
            m, v, step = self.state.get(k) or (torch.zeros_like(p.data), torch.zeros_like(p.data), 0)
            step += 1
            check(lib.pfpp_adamw(_p(p.data), _p(p.grad), _p(m), _p(v), None, None, p.numel(), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                 0.0, 1.0 - betas[0] ** step, 1.0 - betas[1] ** step, 1.0, ops._stream()), "pfpp_adamw")
            self.state[k] = (m, v, step)


class MatchingHeadLoss(torch.autograd.Function):
    """loss = MatchingHeadLoss.apply(part_feats, engine, gt_pcs, n_pcs, part_valids, critical_label_thresholds, critical_label[,
    part_pcs]): the engine's loss as a function of part_feats [B, N, 128] or [sum N, 128]; the trailing part_pcs is handed to a
    MatchingHeadRigidTrainEngine's loss_and_grads (its rigid term).  loss.backward() hands engine's d_part_feats to whatever
    produced part_feats and sets the head's parameters' .grad to this application's gradients times the incoming gradient (from copies
    kept at the forward, so a second backward over a retained graph sets the same values again).  Like loss_and_grads it OVERWRITES
    the .grad of the head's parameters, in forward and in backward: one application per optimizer step; two applications before a
    backward, or gradient accumulation over several, are not what it does.  The loss is returned in part_feats' dtype;
    engine.last_loss_dict holds the step's loss_dict (losses in fp64)."""

    @staticmethod
    def forward(ctx, part_feats, engine, gt_pcs, n_pcs, part_valids, critical_label_thresholds=None, critical_label=None, part_pcs=None):
        extra = {} if part_pcs is None else {"part_pcs": part_pcs}     # a MatchingHeadRigidTrainEngine's rigid term (matching_rigid.py)
        loss_dict, d_feats = engine.loss_and_grads(part_feats.detach(), gt_pcs, n_pcs, part_valids,
                                                   critical_label_thresholds=critical_label_thresholds, critical_label=critical_label, **extra)
        engine.last_loss_dict = loss_dict
        ctx.engine, ctx.shape = engine, part_feats.shape
        ctx.grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in engine.params.items()}
        ctx.save_for_backward(d_feats)
        return loss_dict["loss"].to(part_feats.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        (d_feats,) = ctx.saved_tensors
        for k, p in ctx.engine.params.items():
            p.grad = None if ctx.grads[k] is None else ctx.grads[k] * grad_out.to(ctx.grads[k].dtype)
        return (d_feats * grad_out.to(d_feats.dtype)).reshape(ctx.shape), None, None, None, None, None, None, None
