"""Stage-2 grounding evaluators on the device (include/pq3d_hip.h: pq3d_refer_counts, pq3d_ground_f1_cost / _count;
csrc/ground.hip): drop-in counterparts of ``ScanReferEval`` (evaluator/scanrefer_eval.py), ``ReferIt3DEval``
(evaluator/referit3d_eval.py) and ``Multi3DReferEval`` (evaluator/multi3drefer_eval.py).

``refer_counts`` is one launch, ``multi3drefer_counts`` three (cost matrices, the batched assignment of pq3d_amd/lsap.py, the
counts); neither reads device memory on the host, so both can be captured.  The evaluators' ``update`` only launches and keeps
device tables; ``record`` makes the one device-to-host copy and forms the reference's (value, count) pairs and ratios on the
host in float64.

Not covered, and raised rather than skipped where a caller could ask for it: gathering across ranks (one process records its
own items), the ``save`` JSON, ``txt_acc``, and the per-object ``*_acc`` of ReferIt3DEval (needs use_cls_head; no shipped
config sets it)."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .lsap import MAX_DIM, linear_sum_assignment_batched

GROUPS = ("all", "multiple", "unique", "hard", "easy", "view_dep", "view_indep")      # rows of the count table
assert len(GROUPS) == L.H.PQ3D_REFER_GROUPS, "the kernels count another number of groups than the host names"
COLUMNS = ("items", "correct", "iou25", "iou50")
HIT_CORRECT, HIT_IOU25, HIT_IOU50, HIT_COUNTED = 1, 2, 4, 8
ERR_N_TGT, ERR_LSAP, ERR_INDEX = 1, 2, 4
EVAL_TYPES = ("zt_w_d", "zt_wo_d", "st_w_d", "st_wo_d", "mt")


class ReferCounts(NamedTuple):
    pred: torch.Tensor       # [B] int32
    hits: torch.Tensor       # [B] uint8, HIT_* bits
    counts: torch.Tensor     # [len(GROUPS), len(COLUMNS)] int32


class F1Counts(NamedTuple):
    out: torch.Tensor        # [B, 4] int32: tp25, tp50, P, G
    cost: torch.Tensor       # [B, n, n] fp32, written inside each item's n_b x n_b block only
    sizes: torch.Tensor      # [4, B] int32: P, G, n_b, error bits
    selected: torch.Tensor   # [B, O] int32: the selected slots in slot order, -1 past them
    col: torch.Tensor        # [B, n] int32: the assignment's column of every row < n_b


def _logits(logits, who):
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2 \
            or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"{who}: logits must be a float32 device tensor [B, O] with B, O >= 1")
    return logits.contiguous()


def _bytes(t, B, dev, who, name):
    """An optional per-item flag row: bool or uint8 [B] on the logits' device -> uint8 (a view for bool)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8) or t.device != dev or t.shape != (B,):
        raise ValueError(f"{who}: {name} must be a bool or uint8 tensor [{B}] on {dev}")
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def refer_counts(logits: torch.Tensor, labels: Optional[torch.Tensor] = None, tgt: Optional[torch.Tensor] = None, *,
                 is_multiple: Optional[torch.Tensor] = None, is_hard: Optional[torch.Tensor] = None,
                 is_view_dependent: Optional[torch.Tensor] = None, item_mask: Optional[torch.Tensor] = None) -> ReferCounts:
    """Predictions (argmax as torch's), hit bits and the count table of one batch in one launch.

    ``labels``: the 0-1 rows [3, B, O] float32 ``objects.ground_labels`` writes (tgt_object_id | _iou25 | _iou50); ``tgt``: int64
    target indices [B] (or [B, 1]), which then decide 'correct' instead of row 0.  At least one of the two; without ``labels``
    the iou25 / iou50 hits are 0.  The flag rows and ``item_mask`` are bool / uint8 [B]; only items of the mask are counted."""
    who = "refer_counts"
    logits = _logits(logits, who)
    B, O = logits.shape
    dev = logits.device
    if labels is None and tgt is None:
        raise ValueError(f"{who}: pass labels [3, B, O] or tgt [B]")
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.float32 or labels.device != dev or labels.shape != (3, B, O):
            raise ValueError(f"{who}: labels must be a float32 tensor [3, {B}, {O}] on {dev}")
        labels = labels.contiguous()
    if tgt is not None:
        if not isinstance(tgt, torch.Tensor) or tgt.dtype != torch.int64 or tgt.device != dev or tgt.numel() != B or tgt.dim() > 2:
            raise ValueError(f"{who}: tgt must be an int64 tensor [{B}] or [{B}, 1] on {dev}")
        tgt = tgt.reshape(B).contiguous()
    if 3 * B * O >= 2 ** 31:
        raise ValueError(f"{who}: 3 * B * O must stay below 2^31")
    flags = [_bytes(t, B, dev, who, n) for t, n in ((is_multiple, "is_multiple"), (is_hard, "is_hard"),
                                                    (is_view_dependent, "is_view_dependent"), (item_mask, "item_mask"))]
    pred = torch.empty(B, dtype=torch.int32, device=dev)
    hits = torch.empty(B, dtype=torch.uint8, device=dev)
    counts = torch.empty(len(GROUPS), len(COLUMNS), dtype=torch.int32, device=dev)
    L.call("pq3d_refer_counts", logits, labels, tgt, *flags, B, O, pred, hits, counts)
    return ReferCounts(pred, hits, counts)


def multi3drefer_counts(logits: torch.Tensor, obj_boxes: torch.Tensor, tgt_boxes: torch.Tensor, n_tgt: torch.Tensor) -> F1Counts:
    """``Multi3DReferEval.evaluate_one_query`` of every item in three launches: per item (tp25, tp50, P, G) with P the slots
    sigmoid(logit) > 0.5 selects and G = n_tgt.  ``obj_boxes`` float32 [B, O, 6], ``tgt_boxes`` FLOAT64 [B, T_max, 6] (the
    reference holds the targets as Python floats), ``n_tgt`` int32 [B].  The padded square matrix is solved, as the reference
    does.  An item's error bits (``sizes[3]``) are read by ``check_f1_errors`` or the evaluator's ``record``."""
    who = "multi3drefer_counts"
    logits = _logits(logits, who)
    B, O = logits.shape
    dev = logits.device
    if not isinstance(obj_boxes, torch.Tensor) or obj_boxes.dtype != torch.float32 or obj_boxes.device != dev \
            or obj_boxes.shape != (B, O, 6):
        raise ValueError(f"{who}: obj_boxes must be a float32 tensor [{B}, {O}, 6] on {dev}")
    if not isinstance(tgt_boxes, torch.Tensor) or tgt_boxes.dtype != torch.float64 or tgt_boxes.device != dev \
            or tgt_boxes.dim() != 3 or tgt_boxes.shape[0] != B or tgt_boxes.shape[1] < 1 or tgt_boxes.shape[2] != 6:
        raise ValueError(f"{who}: tgt_boxes must be a float64 tensor [{B}, T_max >= 1, 6] on {dev}")
    if not isinstance(n_tgt, torch.Tensor) or n_tgt.dtype != torch.int32 or n_tgt.device != dev or n_tgt.shape != (B,):
        raise ValueError(f"{who}: n_tgt must be an int32 tensor [{B}] on {dev}")
    T = int(tgt_boxes.shape[1])
    n = max(O, T)
    if n > MAX_DIM:
        raise ValueError(f"{who}: max(O, T_max) = {n} exceeds the assignment kernel's {MAX_DIM}")
    if B * n * n >= 2 ** 31:
        raise ValueError(f"{who}: B * n * n must stay below 2^31")
    cost = torch.empty(B, n, n, dtype=torch.float32, device=dev)
    sizes = torch.empty(4, B, dtype=torch.int32, device=dev)
    sel = torch.empty(B, O, dtype=torch.int32, device=dev)
    out = torch.empty(B, 4, dtype=torch.int32, device=dev)
    L.call("pq3d_ground_f1_cost", logits, obj_boxes.contiguous(), tgt_boxes.contiguous(), n_tgt.contiguous(), B, O, T, cost, sizes, sel)
    row, col, n_match, err = linear_sum_assignment_batched(cost, sizes[2], sizes[2])
    L.call("pq3d_ground_f1_count", cost, row, col, n_match, err, B, n, sizes, out)
    return F1Counts(out, cost, sizes, sel, col)


_F1_MESSAGES = {ERR_N_TGT: "n_tgt outside [0, T_max]", ERR_LSAP: "the assignment failed (a NaN box?)",
                ERR_INDEX: "an assignment index out of range"}


def _raise_f1(bits: Sequence[int]) -> None:
    for b, e in enumerate(bits):
        if e:
            what = "; ".join(m for k, m in _F1_MESSAGES.items() if e & k) or f"error bits {e}"
            raise ValueError(f"multi3drefer_counts: {what} (item {b})")


def check_f1_errors(counts: F1Counts) -> None:
    """Read the error bits of one ``multi3drefer_counts`` (a device-to-host copy) and raise ValueError for the first bad item."""
    _raise_f1(counts.sizes[3].cpu().tolist())


def f1_pair(tp25: int, tp50: int, P: int, G: int):
    """evaluate_one_query's return values from the counts: (1, 1) when both sides are empty, (0, 0) when one is."""
    if P == 0 and G == 0:
        return 1, 1
    if P == 0 or G == 0:
        return 0, 0
    return 2 * tp25 / (P + G), 2 * tp50 / (P + G)


class _Evaluator:
    """evaluator/build.py:13-56 (BaseEvaluator) without an accelerator: reset / update(data_dict) / record() -> (is_best,
    eval_dict with the metric ratios, 'target_metric' and 'best_result')."""
    target_metric = "og_acc"

    def __init__(self, save: bool = False):
        if save:
            raise NotImplementedError(f"{type(self).__name__}: the save JSON of the reference is not written")
        self.best_result = -np.inf
        self.reset()

    def reset(self):
        self.eval_dict: Dict[str, object] = {}
        self._kept: List[torch.Tensor] = []

    def _pairs(self, host: np.ndarray) -> List[Dict[str, tuple]]:
        raise NotImplementedError

    def record(self):
        if not self._kept:
            raise ValueError(f"{type(self).__name__}.record: no batch was added by update")
        sizes = [t.numel() for t in self._kept]
        host = torch.cat([t.reshape(-1) for t in self._kept]).cpu().numpy()       # the one device-to-host copy
        parts = np.split(host, np.cumsum(sizes)[:-1])
        per_batch = self._pairs(parts)
        self.eval_dict = {}
        for k in per_batch[0]:          # (value, count) per batch, summed in update order as BaseEvaluator.record does
            total_value = sum(m[k][0] for m in per_batch)
            total_count = sum(m[k][1] for m in per_batch)
            self.eval_dict[k] = total_value / max(total_count, 1)
        self._kept = []
        self.eval_dict["target_metric"] = self.eval_dict[self.target_metric]
        is_best = self.eval_dict["target_metric"] > self.best_result
        if is_best:
            self.best_result = self.eval_dict["target_metric"]
        self.eval_dict["best_result"] = self.best_result
        return is_best, self.eval_dict


def _refer_update(ev, data_dict, *flag_names):
    if "txt_cls_logits" in data_dict:
        raise NotImplementedError(f"{type(ev).__name__}: txt_acc (txt_cls_logits) is not covered")
    flags = {k: data_dict[k] for k in flag_names}
    logits = data_dict["og3d_logits"]
    t0 = data_dict["tgt_object_id"]
    rows = [data_dict.get("tgt_object_id_iou25"), data_dict.get("tgt_object_id_iou50")]
    index_form = t0.dtype == torch.int64 and t0.numel() == logits.shape[0]
    if index_form and rows[0] is None:
        labels = None
    else:           # row form (the unified wrapper's 0-1 rows): og_acc = "the row holds 1 at the prediction"
        first = torch.zeros_like(logits) if index_form else t0.float()
        labels = torch.stack([first] + [first if r is None else r.float() for r in rows])
    ev._kept.append(refer_counts(logits, labels, t0 if index_form else None, **flags).counts)


def _table(flat: np.ndarray):
    t = flat.reshape(len(GROUPS), len(COLUMNS)).astype(np.int64)
    return {g: {c: int(t[i, j]) for j, c in enumerate(COLUMNS)} for i, g in enumerate(GROUPS)}


class ScanReferEval(_Evaluator):
    """evaluator/scanrefer_eval.py: og_acc_iou25 / _iou50, their unique / multiple splits, og_acc."""
    target_metric = "og_acc"

    def update(self, data_dict):
        _refer_update(self, data_dict, "is_multiple")

    def _pairs(self, parts):
        res = []
        for flat in parts:
            t = _table(flat)
            m = {}
            for thr in ("iou25", "iou50"):
                m[f"og_acc_{thr}"] = (t["all"][thr], t["all"]["items"])
            for thr in ("iou25", "iou50"):
                m[f"og_acc_{thr}_unique"] = (t["unique"][thr], t["unique"]["items"])
            for thr in ("iou25", "iou50"):
                m[f"og_acc_{thr}_multiple"] = (t["multiple"][thr], t["multiple"]["items"])
            m["og_acc"] = (t["all"]["correct"], t["all"]["items"])
            res.append(m)
        return res


class ReferIt3DEval(_Evaluator):
    """evaluator/referit3d_eval.py: og_acc_easy / _hard / _view_dep / _view_indep, og_acc (the per-object *_acc keys need
    use_cls_head and are not covered)."""
    target_metric = "og_acc"

    def update(self, data_dict):
        _refer_update(self, data_dict, "is_hard", "is_view_dependent")

    def _pairs(self, parts):
        res = []
        for flat in parts:
            t = _table(flat)
            m = {f"og_acc_{g}": (t[g]["correct"], t[g]["items"]) for g in ("easy", "hard", "view_dep", "view_indep")}
            m["og_acc"] = (t["all"]["correct"], t["all"]["items"])
            res.append(m)
        return res


class Multi3DReferEval(_Evaluator):
    """evaluator/multi3drefer_eval.py: the F1 at IoU 0.25 / 0.5 per eval_type sub-group and overall.  data_dict: og3d_logits,
    obj_boxes, eval_type (a list of strings), and the targets either padded (tgt_obj_boxes float64 [B, T_max, 6] + n_tgt int32
    [B], device tensors) or as the reference's list of lists of boxes, padded here on the host."""
    target_metric = "iou50_overall"

    def reset(self):
        super().reset()
        self._types: List[List[str]] = []

    @staticmethod
    def pad_targets(gts: Sequence[Sequence[Sequence[float]]], device, T_max: Optional[int] = None):
        n = [len(g) for g in gts]
        T = max(max(n), 1) if T_max is None else int(T_max)
        if max(n) > T:
            raise ValueError(f"T_max = {T} is below the largest target count {max(n)}")
        boxes = np.zeros((len(gts), T, 6), dtype=np.float64)
        for b, g in enumerate(gts):
            if n[b]:
                boxes[b, :n[b]] = np.asarray(g, dtype=np.float64).reshape(n[b], 6)
        return torch.from_numpy(boxes).to(device), torch.tensor(n, dtype=torch.int32, device=device)

    def update(self, data_dict):
        logits = data_dict["og3d_logits"]
        gts = data_dict["tgt_obj_boxes"]
        if isinstance(gts, torch.Tensor):
            boxes, n_tgt = gts, data_dict["n_tgt"]
        else:
            boxes, n_tgt = self.pad_targets(gts, logits.device)
        types = list(data_dict["eval_type"])
        if len(types) != logits.shape[0]:
            raise ValueError("Multi3DReferEval.update: one eval_type per item")
        c = multi3drefer_counts(logits, data_dict["obj_boxes"], boxes, n_tgt)
        self._kept.append(torch.cat((c.out, c.sizes[3][:, None]), 1))
        self._types.append(types)

    def _pairs(self, parts):
        res = []
        for flat, types in zip(parts, self._types):
            t = flat.reshape(-1, 5).astype(np.int64)
            _raise_f1(t[:, 4].tolist())
            f1 = [f1_pair(*map(int, r[:4])) for r in t]
            s25, s50 = np.array([f[0] for f in f1]), np.array([f[1] for f in f1])
            m = {}
            for g in EVAL_TYPES:       # multi3drefer_eval.py:36-41, the sums item by item
                on = np.array([e == g for e in types])
                m["iou25_" + g] = (sum(s25[on]), sum(on)) if np.any(on) else (0, 0)
                m["iou50_" + g] = (sum(s50[on]), sum(on)) if np.any(on) else (0, 0)
            m["iou25_overall"] = (sum(s25), len(s25))
            m["iou50_overall"] = (sum(s50), len(s50))
            res.append(m)
        self._types = []
        return res
