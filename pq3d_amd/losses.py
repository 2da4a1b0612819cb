"""Instance-segmentation set criterion on the decoder's outputs: drop-in counterparts of
``HungarianMatcher`` (modules/third_party/mask3d/matcher.py:67-215), ``SetCriterion`` (criterion.py:95-270) and
``InstSegLoss`` (optim/loss/instseg_loss.py:9-52) for the shipped configuration (criterion_type 'set',
num_points = -1, class_weights = -1).

Where the reference loops over scenes and layers with a dozen torch ops each ((L n_b + 1) x B cost matrices per step,
each followed by a device->host copy), this runs three launches for the cost matrices of ALL layers and scenes
(include/pq3d_hip.h: prep, one grouped + batched fp32 MFMA GEMM, cost), ONE device->host copy, the assignments on
the host (scipy, as the reference), then the losses as gathers of the already computed cost entries plus one
gradient launch and two cross-entropy launches.  No CPU fallback for the device part.

``SetCriterion(..., matching="device")`` runs the assignments on the device instead (pq3d_amd/lsap.py: one launch for all
layers and scenes, exactly scipy's result): the forward then makes no device-to-host transfer, and with padded targets
(``SetCriterion.pad_targets``) decoder + criterion + backward can be captured into one graph.

Stage 2 (configs/unified_tasks_sceneverse.yaml, ``loss_list: [ground_loss, generation_loss]``): ``bce_with_logits_mean`` (csrc/ground.hip,
one launch each way), ``ground_loss``, ``generation_loss``, ``mask_loss`` and ``Query3DLoss``, the counterpart of optim/loss/loss.py's
``Loss`` for those terms."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
from scipy.optimize import linear_sum_assignment
from torch.autograd import Function

from . import _lib as L
from .lsap import check_errors, linear_sum_assignment_batched


class HungarianMatcher(nn.Module):
    """matcher.py:67-103 (parameter holder; the cost matrix is built by SetCriterion's fused path)."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0,
                 ignore_label: int = -100):
        super().__init__()
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"
        if num_points != -1:
            raise NotImplementedError("random point sub-sampling (num_points != -1) is not used by the shipped config")
        self.cost_class, self.cost_mask, self.cost_dice = cost_class, cost_mask, cost_dice
        self.num_points, self.ignore_label = num_points, ignore_label


def _targets_to_device(instance_labels: Sequence[torch.Tensor], segment_masks: Sequence[torch.Tensor], Ns: int, device):
    """list of [n_b] labels / [n_b, S_b] masks -> padded T [B,Nt,Ns] fp32, labels [B,Nt], seg_len, n_inst (int32)."""
    B = len(segment_masks)
    n_inst = [int(m.shape[0]) for m in segment_masks]
    seg_len = [int(m.shape[1]) for m in segment_masks]
    assert max(seg_len) <= Ns, "target masks have more segments than the prediction"
    Nt = max(max(n_inst), 1)
    T = torch.zeros(B, Nt, Ns, dtype=torch.float32)
    lab = torch.zeros(B, Nt, dtype=torch.int64)
    for b in range(B):
        T[b, :n_inst[b], :seg_len[b]] = segment_masks[b].float().cpu()
        lab[b, :n_inst[b]] = instance_labels[b].cpu()
    T = T.to(device)
    return T, lab.to(device), torch.tensor(seg_len, dtype=torch.int32, device=device), \
        torch.tensor(n_inst, dtype=torch.int32, device=device), n_inst, T.sum(-1)


class PaddedTargets:
    """Targets of one batch at a fixed ``max_instances`` (Nt), all device tensors: T [B, Nt, Ns] fp32 0/1 masks,
    labels [B, Nt] int64 (0 past n_inst), seg_len [B] int32, n_inst_dev [B] int32, t_sum [B, Nt] fp32 (= T.sum(-1)).
    ``copy_`` fills a static instance (the buffers a captured graph reads) from another batch of the same shapes."""
    __slots__ = ("T", "labels", "seg_len", "n_inst_dev", "t_sum")

    def __init__(self, T, labels, seg_len, n_inst_dev, t_sum):
        self.T, self.labels, self.seg_len, self.n_inst_dev, self.t_sum = T, labels, seg_len, n_inst_dev, t_sum

    def copy_(self, other: "PaddedTargets") -> "PaddedTargets":
        for k in self.__slots__:
            getattr(self, k).copy_(getattr(other, k))
        return self


def _costs(masks, logits, T, labels, seg_len, n_inst_dev, t_sum, w, ignore_label):
    """Cost matrices of ALL prediction layers and scenes in three launches: cost[l] = (total, mask term, dice term)
    [layers, 3, B, Nq, Nt].  Also returns what the gradient stage needs: (sigma(-X) ; sigma(X)), (mask product | dice
    numerator product), sum_s sigma.  Both terms are sums of non-negative terms over a doubled contraction,
    [T | 1 - T] [relu(-X) ; relu(X)] + sum_s log1p(exp(-|x|)) and [T | 1 - T] [sigma(-X) ; sigma(X)] / D (see csrc/loss.hip): their
    matched entries are the reported loss_mask / loss_dice, which are small exactly when the model is good."""
    n_layers = len(masks)
    B, Ns, Nq = masks[0].shape
    Nt, Ccls = T.shape[1], logits[0].shape[-1]
    dev = T.device
    assert n_layers <= L.MAXG // 2, "too many prediction layers for one grouped launch"
    nsplit = L.lib().pq3d_mask_cost_nsplit(Ns)
    sig = torch.empty(n_layers, B, 2 * Ns, Nq, dtype=torch.float32, device=dev)
    rel = torch.empty(n_layers, B, 2 * Ns, Nq, dtype=torch.float32, device=dev)
    part = torch.empty(2, n_layers, B, nsplit, Nq, dtype=torch.float32, device=dev)
    p = L.MaskPrepDesc()
    p.layers, p.B, p.Ns, p.Nq, p.nsplit = n_layers, B, Ns, Nq, nsplit
    for l in range(n_layers):
        p.X[l] = L.ptr(masks[l])
    p.seg_len, p.sig, p.sp_part, p.sg_part, p.rel = map(L.ptr, (seg_len, sig, part[0], part[1], rel))
    L.call("pq3d_mask_cost_prep", p)
    # ONE grouped + batched exact-f32 MFMA GEMM over K = 2 Ns: groups = (layer, relu planes | sigma planes), batch = scenes
    TXS = torch.empty(n_layers, 2, B, Nt, Nq, dtype=torch.float32, device=dev)
    T2 = torch.cat((T, 1.0 - T), 2)
    Bops = [t for l in range(n_layers) for t in (rel[l], sig[l])]
    Cs = [TXS[l, k] for l in range(n_layers) for k in (0, 1)]
    L.gemm(M=Nt, N=Nq, K=2 * Ns, A=[T2] * (2 * n_layers), B=Bops, Cs=Cs, ct=L.F32, lda=2 * Ns, ldb=Nq, ldc=Nq, transB=True,
           batch=B, strideA=Nt * 2 * Ns, strideB=2 * Ns * Nq, strideC=Nt * Nq)
    cost = torch.empty(n_layers, 3, B, Nq, Nt, dtype=torch.float32, device=dev)
    d = L.MatchCostDesc()
    d.layers, d.B, d.Nq, d.Nt, d.Ns, d.C, d.nsplit = n_layers, B, Nq, Nt, Ns, Ccls, nsplit
    d.w_class, d.w_mask, d.w_dice, d.ignore_label = w[0], w[1], w[2], ignore_label
    d.TXS, d.sp_part, d.sg_part, d.t_sum = map(L.ptr, (TXS, part[0], part[1], t_sum))
    d.seg_len, d.n_inst, d.labels, d.cost = map(L.ptr, (seg_len, n_inst_dev, labels, cost))
    for l in range(n_layers):
        d.cls_logits[l] = L.ptr(logits[l])
    L.call("pq3d_match_cost", d)
    return cost, (sig, TXS, part[1].sum(2))


class _SetCriterionFn(Function):
    """(mask logits of every layer, class logits of every layer) -> losses [n_layers, 3] = (ce, mask, dice).
    Six kernel launches per step (prep, GEMM, cost, CE forward | mask gradient, CE backward) + a handful of small
    index ops vectorised over layers."""

    @staticmethod
    def forward(ctx, crit, T, labels, seg_len, n_inst_dev, n_inst, t_sum, n_layers, *preds):
        masks = [p.contiguous().float() for p in preds[:n_layers]]
        logits = [p.contiguous().float() for p in preds[n_layers:]]
        B, Ns, Nq = masks[0].shape
        dev, Ccls = T.device, logits[0].shape[-1]
        m = crit.matcher
        w = (float(m.cost_class), float(m.cost_mask), float(m.cost_dice))
        cost_all, keep = _costs(masks, logits, T, labels, seg_len, n_inst_dev, t_sum, w, m.ignore_label)
        if crit.matching == "device":
            return _SetCriterionFn._device_tail(ctx, crit, cost_all, keep, masks, logits, T, labels, seg_len, n_inst_dev,
                                                n_inst, t_sum, n_layers, preds)
        host = cost_all[:, 0].cpu().numpy()            # the ONE device->host copy of the step: [layers, B, Nq, Nt]
        Nm = max(min(Nq, max(n_inst)), 1)
        q_idx = np.zeros((n_layers, B, Nm), dtype=np.int32)
        t_idx = np.zeros((n_layers, B, Nm), dtype=np.int32)
        n_match = np.zeros((n_layers, B), dtype=np.int32)
        indices: List[List[Tuple[torch.Tensor, torch.Tensor]]] = []
        for l in range(n_layers):
            per = []
            for b in range(B):
                i, j = linear_sum_assignment(host[l, b, :, :n_inst[b]])    # scipy, as matcher.py:184
                q_idx[l, b, :len(i)], t_idx[l, b, :len(j)], n_match[l, b] = i, j, len(i)
                per.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
            indices.append(per)
        packed = torch.from_numpy(np.concatenate([q_idx.reshape(-1), t_idx.reshape(-1), n_match.reshape(-1)])).to(dev)
        nqt = n_layers * B * Nm
        q_idx_d, t_idx_d = packed[:nqt].view(n_layers, B, Nm), packed[nqt:2 * nqt].view(n_layers, B, Nm)
        n_match_d = packed[2 * nqt:].view(n_layers, B)
        valid = torch.arange(Nm, device=dev)[None, None, :] < n_match_d[:, :, None]             # [layers, B, Nm]
        lidx = torch.arange(n_layers, device=dev)[:, None, None].expand(n_layers, B, Nm)
        bidx = torch.arange(B, device=dev)[None, :, None].expand(n_layers, B, Nm)
        qi, ti = q_idx_d.long(), t_idx_d.long()
        nmf = n_match_d.float().clamp(min=1.0)
        # matched-pair losses ARE the matched entries of the cost matrices (criterion.py:27-70 with num_points = -1)
        pair = cost_all[:, 1:3][lidx, :, bidx, qi, ti] * valid[..., None]                        # [layers, B, Nm, 2]
        losses = torch.zeros(n_layers, 3, dtype=torch.float32, device=dev)
        losses[:, 1:3] = (pair.sum(2) / nmf[..., None]).mean(1)
        # classification (criterion.py:136-163): unmatched queries -> the no-object class (= num_classes)
        tgt = torch.full((n_layers, B, Nq), crit.num_classes, dtype=torch.int64, device=dev)
        tgt[lidx[valid], bidx[valid], qi[valid]] = labels[bidx[valid], ti[valid]]
        row_loss = torch.empty(n_layers, B * Nq, dtype=torch.float32, device=dev)
        lse = torch.empty_like(row_loss)
        ce = L.CeDesc()
        ce.layers, ce.C, ce.R, ce.ignore_index = n_layers, Ccls, B * Nq, crit.ignore_label
        for l in range(n_layers):
            ce.logits[l] = L.ptr(logits[l])
        ce.target, ce.row_loss, ce.lse = L.ptr(tgt), L.ptr(row_loss), L.ptr(lse)
        L.call("pq3d_cross_entropy_fwd", ce)
        cnt = (tgt != crit.ignore_label).sum((1, 2)).clamp(min=1).float()
        losses[:, 0] = row_loss.sum(1) / cnt
        ctx.crit, ctx.n_layers, ctx.keep = crit, n_layers, keep
        ctx.masks, ctx.logits, ctx.tgt, ctx.lse, ctx.cnt = masks, logits, tgt, lse, cnt
        ctx.targets = (T, seg_len, t_sum, q_idx_d.contiguous(), t_idx_d.contiguous(), n_match_d.contiguous(), nmf, Nm)
        ctx.in_dtypes = [p.dtype for p in preds]
        crit._last_indices = indices
        return losses

    @staticmethod
    def _device_tail(ctx, crit, cost_all, keep, masks, logits, T, labels, seg_len, n_inst_dev, n_inst, t_sum, n_layers,
                     preds):
        """matching="device": the assignments of every (layer, scene) in one launch and the CE targets by a scatter, with
        no device-to-host transfer.  Same gathers and kernels as the host mode on the same indices."""
        B, Ns, Nq = masks[0].shape
        Nt, dev, Ccls = T.shape[1], T.device, logits[0].shape[-1]
        Nm = min(Nq, Nt)
        cmat = cost_all[:, 0].reshape(n_layers * B, Nq, Nt)                    # matrix g = (layer g // B, scene g % B)
        row, col, nmd, err = linear_sum_assignment_batched(cmat, None, n_inst_dev.repeat(n_layers))
        q_idx_d, t_idx_d = row.view(n_layers, B, Nm), col.view(n_layers, B, Nm)
        n_match_d = nmd.view(n_layers, B)
        bad = err.view(n_layers, B) != 0
        valid = torch.arange(Nm, device=dev)[None, None, :] < n_match_d[:, :, None]             # [layers, B, Nm]
        lidx = torch.arange(n_layers, device=dev)[:, None, None].expand(n_layers, B, Nm)
        bidx = torch.arange(B, device=dev)[None, :, None].expand(n_layers, B, Nm)
        qi, ti = q_idx_d.long(), t_idx_d.long()
        nmf = n_match_d.float().clamp(min=1.0)
        pair = cost_all[:, 1:3][lidx, :, bidx, qi, ti] * valid[..., None]                        # [layers, B, Nm, 2]
        per = pair.sum(2) / nmf[..., None]                                                      # [layers, B, 2]
        nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        losses = torch.zeros(n_layers, 3, dtype=torch.float32, device=dev)
        losses[:, 1:3] = torch.where(bad[..., None], nan, per).mean(1)      # a failed matrix: NaN losses of its layer
        # classification targets: matched queries take their target's label, the rest the no-object class; unmatched
        # slots scatter into a spare column Nq that is dropped (no boolean-mask indexing, no sync)
        tgt = torch.full((n_layers, B, Nq + 1), crit.num_classes, dtype=torch.int64, device=dev)
        tgt.scatter_(2, torch.where(valid, qi, torch.full_like(qi, Nq)), labels[bidx, ti])
        tgt = tgt[..., :Nq].contiguous()
        row_loss = torch.empty(n_layers, B * Nq, dtype=torch.float32, device=dev)
        lse = torch.empty_like(row_loss)
        ce = L.CeDesc()
        ce.layers, ce.C, ce.R, ce.ignore_index = n_layers, Ccls, B * Nq, crit.ignore_label
        for l in range(n_layers):
            ce.logits[l] = L.ptr(logits[l])
        ce.target, ce.row_loss, ce.lse = L.ptr(tgt), L.ptr(row_loss), L.ptr(lse)
        L.call("pq3d_cross_entropy_fwd", ce)
        cnt = (tgt != crit.ignore_label).sum((1, 2)).clamp(min=1).float()
        losses[:, 0] = torch.where(bad.any(1), nan, row_loss.sum(1) / cnt)
        ctx.crit, ctx.n_layers, ctx.keep = crit, n_layers, keep
        ctx.masks, ctx.logits, ctx.tgt, ctx.lse, ctx.cnt = masks, logits, tgt, lse, cnt
        ctx.targets = (T, seg_len, t_sum, q_idx_d, t_idx_d, n_match_d, nmf, Nm)
        ctx.in_dtypes = [p.dtype for p in preds]
        crit._last_err = err
        if n_inst is None:      # padded targets: the per-scene counts stay on the device
            crit._last_indices = [(qi[l], ti[l], n_match_d[l]) for l in range(n_layers)]
        else:
            crit._last_indices = [[(qi[l, b, :min(Nq, n_inst[b])], ti[l, b, :min(Nq, n_inst[b])]) for b in range(B)]
                                  for l in range(n_layers)]
        return losses

    @staticmethod
    def backward(ctx, g):
        T, seg_len, t_sum, q_idx_d, t_idx_d, n_match_d, nmf, Nm = ctx.targets
        n_layers = ctx.n_layers
        B, Ns, Nq = ctx.masks[0].shape
        Nt = T.shape[1]
        sig, TXS, sig_sum = ctx.keep
        g = g.contiguous().float()
        gmd = (g[:, 1:3, None] / (nmf[:, None, :] * B)).contiguous()    # [layers, 2, B]; the 1/S_b is applied in-kernel
        scale = (g[:, 0] / ctx.cnt).contiguous()                        # [layers]
        dmasks = [torch.empty_like(m) for m in ctx.masks]
        dlogits = [torch.empty_like(t) for t in ctx.logits]
        d = L.MaskGradDesc()
        d.layers, d.B, d.Ns, d.Nq, d.Nt, d.Nm = n_layers, B, Ns, Nq, Nt, Nm
        d.sig, d.T, d.TXS, d.sig_sum, d.t_sum, d.seg_len = map(L.ptr, (sig, T, TXS, sig_sum.contiguous(), t_sum, seg_len))
        d.q_idx, d.t_idx, d.n_match, d.g = map(L.ptr, (q_idx_d, t_idx_d, n_match_d, gmd))
        for l in range(n_layers):
            d.dX[l] = L.ptr(dmasks[l])
        L.call("pq3d_matched_mask_grad", d)
        ce = L.CeDesc()
        ce.layers, ce.C, ce.R, ce.ignore_index = n_layers, dlogits[0].shape[-1], B * Nq, ctx.crit.ignore_label
        for l in range(n_layers):
            ce.logits[l], ce.dlogits[l] = L.ptr(ctx.logits[l]), L.ptr(dlogits[l])
        ce.target, ce.lse, ce.scale = L.ptr(ctx.tgt), L.ptr(ctx.lse), L.ptr(scale)
        L.call("pq3d_cross_entropy_bwd", ce)
        grads = [t.to(dt) for t, dt in zip(dmasks + dlogits, ctx.in_dtypes)]
        return (None,) * 8 + tuple(grads)


class SetCriterion(nn.Module):
    """criterion.py:95-270: forward(predictions_mask, predictions_class, instance_labels, segment_masks) ->
    (losses dict with 'loss_ce', 'loss_mask', 'loss_dice' and the '_i' auxiliary copies, indices of the last layer).

    ``matching``: "host" (scipy per (layer, scene), the reference's path) or "device" (pq3d_amd/lsap.py, the same
    assignments with no device-to-host transfer; the last layer's indices are then int64 device tensors, and a failed
    assignment makes its layer's losses NaN -- ``check()`` raises scipy's error).  Device mode also takes
    ``targets=SetCriterion.pad_targets(...)`` instead of the two lists, which makes the step capturable; the indices are
    then (q_idx [B, Nm], t_idx [B, Nm], n_match [B]) device tensors with pairs k < n_match[b] valid."""

    def __init__(self, num_classes, matcher, weight_dict, losses, num_points, class_weights, ignore_label,
                 matching: str = "host"):
        super().__init__()
        if num_points != -1 or class_weights != -1:
            raise NotImplementedError("only num_points = -1, class_weights = -1 (configs/instseg_sceneverse.yaml:163-168)")
        if matching not in ("host", "device"):
            raise ValueError(f"matching must be 'host' or 'device', got {matching!r}")
        self.num_classes, self.matcher, self.weight_dict, self.losses = num_classes, matcher, weight_dict, list(losses)
        self.num_points, self.class_weights, self.ignore_label = num_points, class_weights, ignore_label
        self.matching = matching
        self._last_indices = None
        self._last_err = None

    @staticmethod
    def pad_targets(instance_labels: Sequence[torch.Tensor], segment_masks: Sequence[torch.Tensor], Ns: int,
                    max_instances: int, device=None) -> PaddedTargets:
        """The targets of one batch as device tensors at a fixed ``max_instances`` (host loop; call it outside a capture
        and ``copy_`` the result into the static targets a captured step reads).  Scenes may have 0 instances."""
        B = len(segment_masks)
        if B < 1 or len(instance_labels) != B:
            raise ValueError("one instance_labels and one segment_masks entry per scene")
        n_inst = [int(m.shape[0]) for m in segment_masks]
        if max_instances < 1 or max(n_inst) > max_instances:
            raise ValueError(f"max_instances = {max_instances} must be >= 1 and >= the largest instance count {max(n_inst)}")
        if max(int(m.shape[1]) for m in segment_masks) > Ns:
            raise ValueError("target masks have more segments than Ns")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        T = torch.zeros(B, max_instances, Ns, dtype=torch.float32)
        lab = torch.zeros(B, max_instances, dtype=torch.int64)
        for b in range(B):
            T[b, :n_inst[b], :segment_masks[b].shape[1]] = segment_masks[b].float().cpu()
            lab[b, :n_inst[b]] = instance_labels[b].cpu()
        T = T.to(dev)
        seg_len = torch.tensor([int(m.shape[1]) for m in segment_masks], dtype=torch.int32, device=dev)
        return PaddedTargets(T, lab.to(dev), seg_len, torch.tensor(n_inst, dtype=torch.int32, device=dev), T.sum(-1))

    def check(self) -> None:
        """Raise scipy's ValueError if an assignment of the last device-mode forward failed (reads the error codes)."""
        if self._last_err is not None:
            check_errors(self._last_err)

    def forward(self, predictions_mask, predictions_class, instance_labels=None, segment_masks=None, targets=None):
        n = len(predictions_mask)
        # reference order: the LAST prediction is the main output, the others are the auxiliary '_i' losses
        order = [n - 1] + list(range(n - 1))
        masks = [predictions_mask[i] for i in order]
        logits = [predictions_class[i] for i in order]
        dev = masks[0].device
        if targets is not None:
            if self.matching != "device":
                raise ValueError("padded targets need SetCriterion(..., matching='device')")
            if not isinstance(targets, PaddedTargets):
                raise ValueError("targets must come from SetCriterion.pad_targets")
            B, Ns = masks[0].shape[:2]
            if targets.T.shape[0] != B or targets.T.shape[2] != Ns or targets.T.device != dev:
                raise ValueError(f"padded targets {tuple(targets.T.shape)} on {targets.T.device} do not match predictions "
                                 f"[B = {B}, Ns = {Ns}] on {dev}")
            T, labels, seg_len, n_inst_dev, t_sum = (targets.T, targets.labels, targets.seg_len, targets.n_inst_dev,
                                                     targets.t_sum)
            n_inst = None
        else:
            T, labels, seg_len, n_inst_dev, n_inst, t_sum = _targets_to_device(instance_labels, segment_masks,
                                                                             masks[0].shape[1], dev)
        out = _SetCriterionFn.apply(self, T, labels, seg_len, n_inst_dev, n_inst, t_sum, n, *masks, *logits)
        names = {"labels": [(0, "loss_ce")], "masks": [(1, "loss_mask"), (2, "loss_dice")]}
        losses: Dict[str, torch.Tensor] = {}
        for l in range(n):
            suffix = "" if l == 0 else f"_{l - 1}"
            for kind in self.losses:
                for col, name in names[kind]:
                    losses[name + suffix] = out[l, col]
        return losses, self._last_indices[0]


class InstSegLoss(nn.Module):
    """optim/loss/instseg_loss.py:9-52: criterion_type 'set' (Hungarian matching, stage 1) or 'direct' (ground-truth
    masks, query i <-> instance i, configs/instseg_sceneverse_gt.yaml:160)."""

    def __init__(self, cfg, matching: str = "host"):
        super().__init__()
        self.cfg = cfg
        loss_cfg = cfg.model.get(self.__class__.__name__)
        self.criterion_type = loss_cfg.get("criterion_type", "set")
        assert self.criterion_type in ["set", "direct"]
        matcher = HungarianMatcher(**dict(loss_cfg.matcher))
        self.weight_dict = {"loss_ce": matcher.cost_class, "loss_mask": matcher.cost_mask, "loss_dice": matcher.cost_dice}
        if self.criterion_type == "set":
            self.set_criterion = SetCriterion(matcher=matcher, weight_dict=self.weight_dict, matching=matching,
                                              **dict(loss_cfg.criterion))
        else:   # instseg_loss.py:34-35: DirectCriterion(**loss_cfg.criterion) swallows the set criterion's other keys
            self.direct_criterion = DirectCriterion(**dict(loss_cfg.criterion))

    def forward(self, data_dict):
        if self.criterion_type == "direct":   # instseg_loss.py:41-43
            losses = self.direct_criterion(data_dict["predictions_mask"], data_dict["predictions_class"],
                                           data_dict["target_masks"], data_dict["target_masks_pad_masks"],
                                           data_dict["target_labels"])
        else:
            losses, indices = self.set_criterion(data_dict["predictions_mask"], data_dict["predictions_class"],
                                                 data_dict["instance_labels"], data_dict["segment_masks"])
            data_dict["indices"] = indices
        for k in list(losses.keys()):
            losses[k] = losses[k] * self.weight_dict[k.split("_")[0] + "_" + k.split("_")[1]]
        return [sum(losses.values()), losses]


# ------------------------------------------------------------------------------------------------ padded (direct) losses
class _PaddedMaskLoss(Function):
    """(X [B,S,N] mask logits, T [B,N,S], P [B,N,S] bool) -> (batch_mask_loss, batch_dice_loss)
    (optim/loss/instseg_loss.py:54-85): two launches forward (tile sums + tiny finalize ops), one backward."""

    @staticmethod
    def forward(ctx, X, T, P):
        X = X.contiguous().float()
        T = T.contiguous().float()
        P = P.contiguous()
        if P.dtype != torch.bool:
            P = P != 0
        B, S, N = X.shape
        nt = (S + 63) // 64
        part = torch.empty(B, nt, N, 4, dtype=torch.float32, device=X.device)
        L.call("pq3d_padded_mask_sums", X, T, P, part, B, S, N)
        sums = part.sum(1)                                   # [B, N, 4]
        sb, sp, si, su = sums.unbind(-1)
        valid = sp > 0
        cnt = valid.sum().float()
        lm = torch.where(valid, sb / (sp + 1e-6), torch.zeros_like(sb)).sum() / cnt
        dice = 1.0 - (2.0 * si + 1e-6) / (su + 1e-6)
        ld = torch.where(valid, dice, torch.zeros_like(dice)).sum() / cnt
        ctx.save_for_backward(X, T, P, sums.contiguous(), valid, cnt)
        return lm, ld

    @staticmethod
    def backward(ctx, gm_, gd_):
        X, T, P, sums, valid, cnt = ctx.saved_tensors
        B, S, N = X.shape
        sp = sums[..., 1]
        gm = (torch.where(valid, gm_ / (cnt * (sp + 1e-6)), torch.zeros_like(sp))).contiguous()
        gd = (torch.where(valid, gd_ / cnt, torch.zeros_like(sp))).contiguous()
        dX = torch.empty_like(X)
        L.call("pq3d_padded_mask_grad", X, T, P, sums, gm, gd, dX, B, S, N)
        return dX, None, None


def padded_mask_losses(pred_masks: torch.Tensor, targets: torch.Tensor, padding_mask: torch.Tensor):
    """(batch_mask_loss, batch_dice_loss) for pred_masks in the model's own layout [B, S, N] (segments first)."""
    return _PaddedMaskLoss.apply(pred_masks, targets, padding_mask)


def _segments_first(logits: torch.Tensor) -> torch.Tensor:
    """The reference passes pred_masks.permute(0, 2, 1) ([B, N, S]); undo the view (no copy when it is one)."""
    return logits.permute(0, 2, 1)


def batch_mask_loss(logits, targets, padding_mask):
    """optim/loss/instseg_loss.py:77-85; logits [B, N, S] as in the reference."""
    return padded_mask_losses(_segments_first(logits), targets, padding_mask)[0]


def batch_dice_loss(logits, targets, padding_mask):
    """optim/loss/instseg_loss.py:54-75; logits [B, N, S] as in the reference."""
    return padded_mask_losses(_segments_first(logits), targets, padding_mask)[1]


def cross_entropy_rows(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100,
                       add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.cross_entropy(logits.view(-1, C), labels.view(-1), ignore_index) through the CE kernels (mean over kept rows).
    ``add``: a 0-dim fp32 device tensor (the other terms of a total loss) added inside the mean launch -- "total = other + ce"
    without an elementwise launch; its gradient is the upstream gradient."""
    return _RowCE.apply(logits, labels, ignore_index, add)


class _RowCE(Function):
    """Forward: per-row loss + log-sum-exp (one launch), then the mean over the kept rows and 1 / kept (one launch).  Backward:
    one launch; the upstream gradient and 1 / kept stay on the device (scale, scale_mul).  No framework kernels."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, add=None):
        assert add is None or (add.numel() == 1 and add.dtype == torch.float32 and add.is_cuda)
        x = logits.contiguous().float().view(-1, logits.shape[-1])
        t = labels.contiguous().view(-1).long()
        R, Ccls = x.shape
        buf = torch.empty(2 * R + 1, dtype=torch.float32, device=x.device)      # row_loss | lse | 1 / kept
        row_loss, lse, inv = buf[:R], buf[R:2 * R], buf[2 * R:]
        # the RETURNED scalar lives in a tensor of its own: sharing the saved tensors' buffer (and version counter) made a caller's
        # in-place `loss /= accum_steps` / `total += aux` fail the backward with "modified by an inplace operation" 
        loss = torch.empty((), dtype=torch.float32, device=x.device)   # 0-dim, not a view: in-place ops on it are legal
        ce = L.CeDesc()
        ce.layers, ce.C, ce.R, ce.ignore_index = 1, Ccls, R, ignore_index
        ce.logits[0], ce.target, ce.row_loss, ce.lse = L.ptr(x), L.ptr(t), L.ptr(row_loss), L.ptr(lse)
        L.call("pq3d_cross_entropy_fwd", ce)
        L.call("pq3d_cross_entropy_mean", ce, loss, inv, add)
        ctx.has_add = add is not None
        ctx.save_for_backward(x, t, lse, inv)
        ctx.ignore_index, ctx.shape, ctx.dtype = ignore_index, logits.shape, logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        x, t, lse, inv = ctx.saved_tensors
        dl = torch.empty_like(x)
        scale = g.reshape(1)
        if scale.dtype != torch.float32 or not scale.is_contiguous():
            scale = scale.float().contiguous()
        ce = L.CeDesc()
        ce.layers, ce.C, ce.R, ce.ignore_index = 1, x.shape[1], x.shape[0], ctx.ignore_index
        ce.logits[0], ce.dlogits[0], ce.target, ce.lse, ce.scale = L.ptr(x), L.ptr(dl), L.ptr(t), L.ptr(lse), L.ptr(scale)
        ce.scale_mul = L.ptr(inv)
        L.call("pq3d_cross_entropy_bwd", ce)
        dl = dl.view(ctx.shape)
        return (dl if ctx.dtype == torch.float32 else dl.to(ctx.dtype)), None, None, (g if ctx.has_add else None)


def bce_with_logits_mean(logits: torch.Tensor, labels: torch.Tensor, weight: float = 1.0,
                         add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """weight * F.binary_cross_entropy_with_logits(torch.clamp(logits, min=-100), labels) [+ add] over all elements (the BCE
    branch of the reference's cross_entropy, optim/loss/query3d_loss.py:10-16): one launch forward, one backward.  ``add`` as
    in ``cross_entropy_rows``.  A logit below -100 (a padded slot's -inf) takes no gradient."""
    return _BceMean.apply(logits, labels, float(weight), add)


class _BceMean(Function):
    """Like _RowCE: the loss in a 0-dim tensor of its own; weight, 1 / N and the upstream gradient meet inside the kernels."""

    @staticmethod
    def forward(ctx, logits, labels, weight, add=None):
        assert add is None or (add.numel() == 1 and add.dtype == torch.float32 and add.is_cuda)
        if logits.shape != labels.shape:
            raise ValueError(f"logits {tuple(logits.shape)} and labels {tuple(labels.shape)} differ in shape")
        x = logits.contiguous().float().view(-1)
        y = labels.contiguous().float().view(-1)
        loss = torch.empty((), dtype=torch.float32, device=x.device)   # of its own: see _RowCE
        L.call("pq3d_bce_logits_fwd", x, y, x.numel(), weight, add, loss)
        ctx.save_for_backward(x, y)
        ctx.weight, ctx.has_add, ctx.shape, ctx.dtype = weight, add is not None, logits.shape, logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        scale = g.reshape(1)
        if scale.dtype != torch.float32 or not scale.is_contiguous():
            scale = scale.float().contiguous()
        dx = torch.empty_like(x)
        L.call("pq3d_bce_logits_bwd", x, y, x.numel(), ctx.weight, scale, dx)
        dx = dx.view(ctx.shape)
        return (dx if ctx.dtype == torch.float32 else dx.to(ctx.dtype)), None, None, (g if ctx.has_add else None)


def _head_loss(data_dict, head: str, fallback=None, weight: float = 1.0, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """query3d_loss.py:10-24: cross_entropy(data_dict[head + '_logits'], data_dict[head + '_label'])."""
    names = (head + "_logits", head + "_label")
    if names[0] not in data_dict and fallback is not None:
        names = fallback
    logits, label = data_dict[names[0]], data_dict[names[1]]
    if label is None:
        raise KeyError(f"{names[1]} is missing: {head}_loss needs the labels of {names[0]}")
    if label.shape == logits.shape:        # a 0-1 row per item: BCE over every slot, the padded ones included
        return bce_with_logits_mean(logits, label, weight, add)
    # index labels.  (The reference clamps here too; a row's log-sum-exp does not see a -inf turned into -100 unless the whole row
    # is below -100 + log(eps), so the CE kernels take the logits as they are.)
    ce = cross_entropy_rows(logits, label, -100, add if weight == 1.0 else None)
    if weight == 1.0:
        return ce
    return ce * weight if add is None else ce * weight + add


def ground_loss(data_dict, weight: float = 1.0, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The registry's 'ground_loss' (configs/unified_tasks_sceneverse.yaml: loss_list [ground_loss, generation_loss], weight 10):
    ground_logits / ground_label, else og3d_logits / tgt_object_id."""
    return _head_loss(data_dict, "ground", ("og3d_logits", "tgt_object_id"), weight, add)


def generation_loss(data_dict, weight: float = 1.0, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The registry's 'generation_loss': token cross-entropy of the teacher-forced logits (ignore_index -100)."""
    return _head_loss(data_dict, "generation", None, weight, add)


class Query3DLoss(nn.Module):
    """optim/loss/loss.py:113-152 (Loss) for the stage-2 terms ground_loss, generation_loss and mask_loss:
    forward(data_dict) -> (total_loss, all_losses), every term times loss_weights.get(name, 1.0), total_loss = the sum over
    loss_list (also all_losses['total_loss']).
    ``total(data_dict)`` returns the same total alone and is what a training step wants (``TrainStep(model, crit.total)``): there
    the terms are chained through the kernels' ``add`` operand, so the running total costs no elementwise launch where a term
    has one (BCE with any weight, CE with weight 1); the sum is then rounded once per term from fp64 instead of added in fp32."""
    TERMS = ("ground_loss", "generation_loss", "mask_loss")

    def __init__(self, loss_list: Sequence[str], loss_weights: Optional[Dict[str, float]] = None, vis_loss_list: Sequence[str] = ()):
        super().__init__()
        self.selected_keys = list(loss_list)
        self.all_keys = self.selected_keys + [k for k in vis_loss_list if k not in self.selected_keys]
        unknown = [k for k in self.all_keys if k not in self.TERMS]
        if unknown or not self.selected_keys:
            raise NotImplementedError(f"loss terms {unknown or '(none)'}: Query3DLoss covers {', '.join(self.TERMS)}")
        self.loss_weights = {k: float(v) for k, v in dict(loss_weights or {}).items()}

    def _term(self, k, data_dict, add=None):
        w = self.loss_weights.get(k, 1.0)
        if k == "mask_loss":
            cur = mask_loss(data_dict) * w
            return cur if add is None else add + cur
        return (ground_loss if k == "ground_loss" else generation_loss)(data_dict, w, add)

    def forward(self, data_dict):
        all_losses = {k: self._term(k, data_dict) for k in self.all_keys}
        total = sum(all_losses[k] for k in self.selected_keys)
        all_losses["total_loss"] = total
        return total, all_losses

    def total(self, data_dict) -> torch.Tensor:
        total = None
        for k in self.selected_keys:
            total = self._term(k, data_dict, total)
        return total


class DirectCriterion(nn.Module):
    """optim/loss/instseg_loss.py:88-133: ground-truth masks, no Hungarian matching (query i <-> instance i)."""

    def __init__(self, losses, ignore_label, **kwargs):
        super().__init__()
        self.losses, self.ignore_label = list(losses), ignore_label

    def loss_labels(self, logits, labels):
        if self.ignore_label != -100:
            labels = torch.where(labels == self.ignore_label, torch.full_like(labels, -100), labels)
        return {"loss_ce": cross_entropy_rows(logits, labels, -100)}

    def loss_masks(self, pred_masks, gt_masks, padding_mask):
        lm, ld = padded_mask_losses(pred_masks, gt_masks, padding_mask)     # pred_masks [B, S, N] as the model emits them
        return {"loss_mask": lm, "loss_dice": ld}

    def get_loss(self, loss, outputs, targets):
        if loss == "labels":
            return self.loss_labels(outputs["pred_logits"], targets["labels"])
        if loss == "masks":
            return self.loss_masks(outputs["pred_masks"], targets["masks"], targets["padding_mask"])
        raise AssertionError(loss)

    def forward(self, predictions_mask, predictions_class, target_masks, target_masks_pad_masks, target_labels):
        losses = {}
        targets = {"labels": target_labels, "masks": target_masks, "padding_mask": target_masks_pad_masks}
        for loss in self.losses:
            losses.update(self.get_loss(loss, {"pred_logits": predictions_class[-1], "pred_masks": predictions_mask[-1]},
                                        targets))
        for i in range(len(predictions_mask) - 1):
            for loss in self.losses:
                l_dict = self.get_loss(loss, {"pred_logits": predictions_class[i], "pred_masks": predictions_mask[i]},
                                       targets)
                losses.update({k + f"_{i}": v for k, v in l_dict.items()})
        return losses


def mask_loss(data_dict):
    """optim/loss/query3d_loss.py:28-39 (stage-2 'mask_loss': 5 x BCE + 2 x dice + 2 x object-masked class CE per layer)."""
    mask_gt = data_dict["gt_attn_mask"].logical_not().float()
    labels = torch.where(data_dict["obj_masks"].bool(), data_dict["instance_labels"],
                         torch.full_like(data_dict["instance_labels"], -100))
    total = 0
    for mask_pred, mask_cls in zip(data_dict["predictions_mask"], data_dict["predictions_class"]):
        lm, ld = padded_mask_losses(mask_pred, mask_gt, data_dict["padding_mask"])
        total = total + lm * 5 + ld * 2
        # (CE(none) * obj_masks).sum() / (obj_masks.sum() + 1e-6): rows outside obj_masks are ignored rows of the CE kernel
        n = data_dict["obj_masks"].sum().float()
        total = total + cross_entropy_rows(mask_cls, labels, -100) * (n / (n + 1e-6)) * 2
    return total
