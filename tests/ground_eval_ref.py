"""numpy restatement of csrc/ground.hip: the specification the GPU tests compare against, itself held against the
reference's own results in tests/test_ground_eval_ref.py (tests/golden/F28_ground_eval.npz).

  bce_logits_mean / bce_logits_grad   cross_entropy's BCE branch (optim/loss/query3d_loss.py:10-16) and its gradient, float64
  refer_counts                        argmax as torch's, hit bits, the [7, 4] count table
  scanrefer_pairs / referit3d_pairs   the evaluators' (value, count) pairs from a count table
  iou_matrix / select / f1_counts     Multi3DReferEval.evaluate_one_query: selection, the -IoU matrix with its fp32 / fp64
                                      split, scipy's assignment of the padded square, the counts; f1_pair, multi3drefer_pairs
  accumulate                          BaseEvaluator.record: sums of the pairs over batches, then the ratios
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

GROUPS = ("all", "multiple", "unique", "hard", "easy", "view_dep", "view_indep")
COLUMNS = ("items", "correct", "iou25", "iou50")
EVAL_TYPES = ("zt_w_d", "zt_wo_d", "st_w_d", "st_wo_d", "mt")
ERR_N_TGT = 1


# ------------------------------------------------------------------------------------------------------------------ loss
def bce_logits_mean(x, y, weight=1.0, add=None):
    """weight * mean(max(c, 0) - c y + log1p(exp(-|c|))) + add with c = clamp(x, min=-100), in float64 (NaN stays)."""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    c = np.where(x < -100.0, -100.0, x)
    with np.errstate(invalid="ignore"):
        per = np.where(c > 0, c, 0.0) - c * y + np.log1p(np.exp(-np.abs(c)))
    r = float(weight) * (per.sum() / x.size)
    return r + float(add) if add is not None else r


def bce_logits_grad(x, y, weight=1.0, g=1.0):
    """d loss / d x: g * weight / N * (sigmoid(x) - y) where x >= -100 (the clamp passes the gradient AT -100), 0 below."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    return np.where(x < -100.0, 0.0, float(g) * float(weight) / x.size * (s - y))


# ----------------------------------------------------------------------------------------------------------------- refer
def argmax_rows(logits):
    """torch.argmax(dim=1): the first NaN if the row has one, else the first largest entry."""
    logits = np.asarray(logits, dtype=np.float32)
    out = np.zeros(len(logits), dtype=np.int32)
    for b, row in enumerate(logits):
        nan = np.flatnonzero(np.isnan(row))
        out[b] = nan[0] if len(nan) else int(np.argmax(row))
    return out


def refer_counts(logits, labels=None, tgt=None, is_multiple=None, is_hard=None, is_view_dependent=None, item_mask=None):
    """-> pred [B] int32, hits [B] uint8 (1 correct, 2 iou25, 4 iou50, 8 counted), counts [7, 4] int32 (GROUPS x COLUMNS)."""
    pred = argmax_rows(logits)
    B = len(pred)
    ar = np.arange(B)
    h0 = (np.asarray(tgt).reshape(B) == pred) if tgt is not None else (np.asarray(labels)[0][ar, pred] != 0)
    h25 = np.asarray(labels)[1][ar, pred] != 0 if labels is not None else np.zeros(B, dtype=bool)
    h50 = np.asarray(labels)[2][ar, pred] != 0 if labels is not None else np.zeros(B, dtype=bool)
    on = np.ones(B, dtype=bool) if item_mask is None else np.asarray(item_mask) != 0
    hits = (h0 * 1 + h25 * 2 + h50 * 4 + on * 8).astype(np.uint8)
    counts = np.zeros((len(GROUPS), len(COLUMNS)), dtype=np.int32)
    cols = np.stack([np.ones(B, dtype=bool), h0, h25, h50], 1)

    def put(g, sel):
        counts[g] = cols[sel & on].sum(0)

    put(0, np.ones(B, dtype=bool))
    for k, fl in enumerate((is_multiple, is_hard, is_view_dependent)):
        if fl is not None:
            fl = np.asarray(fl) != 0
            put(1 + 2 * k, fl)
            put(2 + 2 * k, ~fl)
    return pred, hits, counts


def _t(counts):
    return {g: {c: int(counts[i, j]) for j, c in enumerate(COLUMNS)} for i, g in enumerate(GROUPS)}


def scanrefer_pairs(counts):
    """ScanReferEval.batch_metrics(include_count=True) without txt_acc, in its key order."""
    t = _t(counts)
    m = {}
    for thr in ("iou25", "iou50"):
        m[f"og_acc_{thr}"] = (t["all"][thr], t["all"]["items"])
    for thr in ("iou25", "iou50"):
        m[f"og_acc_{thr}_unique"] = (t["unique"][thr], t["unique"]["items"])
    for thr in ("iou25", "iou50"):
        m[f"og_acc_{thr}_multiple"] = (t["multiple"][thr], t["multiple"]["items"])
    m["og_acc"] = (t["all"]["correct"], t["all"]["items"])
    return m


def referit3d_pairs(counts):
    """ReferIt3DEval.batch_metrics(include_count=True) without txt_acc and the per-object *_acc."""
    t = _t(counts)
    m = {f"og_acc_{g}": (t[g]["correct"], t[g]["items"]) for g in ("easy", "hard", "view_dep", "view_indep")}
    m["og_acc"] = (t["all"]["correct"], t["all"]["items"])
    return m


# -------------------------------------------------------------------------------------------------------------------- f1
def select(logits_row):
    """Slots with 1 / (1 + expf(-x)) > 0.5f in slot order (fp32 arithmetic: -inf and 0 are out, +inf is in)."""
    x = np.asarray(logits_row, dtype=np.float32)
    with np.errstate(over="ignore"):
        s = np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))
    return np.flatnonzero(s > np.float32(0.5)).astype(np.int32)


def iou_matrix(pred, gt):
    """[P, G] float32: box3d_iou of the corners c -+ s / 2, pred fp32 [P, 6] (corners and volume in fp32), gt float64 [G, 6]
    (corners and volume in float64); intersection, union, + 1e-8 and the quotient in float64, rounded to fp32."""
    pred = np.asarray(pred, dtype=np.float32).reshape(-1, 6)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 6)
    ph, th = pred[:, 3:] / np.float32(2), gt[:, 3:] / 2.0
    pa, pb = ph + pred[:, :3], -ph + pred[:, :3]
    ta, tb = th + gt[:, :3], -th + gt[:, :3]
    pmin, pmax = np.minimum(pa, pb), np.maximum(pa, pb)                  # fp32
    tmin, tmax = np.minimum(ta, tb), np.maximum(ta, tb)
    dp, dt = pmax - pmin, tmax - tmin
    v1 = ((dp[:, 0] * dp[:, 1]) * dp[:, 2]).astype(np.float32)
    v2 = (dt[:, 0] * dt[:, 1]) * dt[:, 2]
    lo = np.maximum(pmin.astype(np.float64)[:, None, :], tmin[None, :, :])
    hi = np.minimum(pmax.astype(np.float64)[:, None, :], tmax[None, :, :])
    d = np.maximum(hi - lo, 0.0)
    inter = (d[..., 0] * d[..., 1]) * d[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (((v1.astype(np.float64)[:, None] + v2[None, :]) - inter) + 1e-8)
    return iou.astype(np.float32)


def padded_cost(pred, gt):
    """The n_b x n_b float32 matrix evaluate_one_query solves: -IoU in the leading P x G block, 0 elsewhere (n_b = max(P, G))."""
    P, G = len(pred), len(gt)
    nb = max(P, G)
    cost = np.zeros((nb, nb), dtype=np.float32)
    if P and G:
        cost[:P, :G] = -iou_matrix(pred, gt)
    return cost


def f1_counts(pred, gt):
    """-> (tp25, tp50, P, G) and the assignment's columns: pairs of the rows < P with IoU >= 0.25 / 0.5 (fp32 comparison)."""
    P, G = len(pred), len(gt)
    cost = padded_cost(pred, gt)
    if max(P, G) == 0:
        return (0, 0, 0, 0), np.zeros(0, dtype=np.int64)
    row, col = linear_sum_assignment(cost)
    iou = -cost[row[:P], col[:P]]
    return (int((iou >= np.float32(0.25)).sum()), int((iou >= np.float32(0.5)).sum()), P, G), col


def f1_pair(tp25, tp50, P, G):
    if P == 0 and G == 0:
        return 1, 1
    if P == 0 or G == 0:
        return 0, 0
    return 2 * tp25 / (P + G), 2 * tp50 / (P + G)


def multi3drefer_batch(logits, obj_boxes, tgt_boxes, n_tgt):
    """The device pipeline on one batch: out [B, 4] int32, err [B], the per-item selections and cost matrices."""
    logits, obj_boxes = np.asarray(logits, dtype=np.float32), np.asarray(obj_boxes, dtype=np.float32)
    tgt_boxes = np.asarray(tgt_boxes, dtype=np.float64)
    B, T = len(logits), tgt_boxes.shape[1]
    out, err = np.zeros((B, 4), dtype=np.int32), np.zeros(B, dtype=np.int32)
    sels, costs = [], []
    for b in range(B):
        if not 0 <= n_tgt[b] <= T:
            err[b] = ERR_N_TGT
            sels.append(np.zeros(0, dtype=np.int32))
            costs.append(np.zeros((0, 0), dtype=np.float32))
            continue
        sel = select(logits[b])
        pred, gt = obj_boxes[b][sel], tgt_boxes[b][:n_tgt[b]]
        out[b] = f1_counts(pred, gt)[0]
        sels.append(sel)
        costs.append(padded_cost(pred, gt))
    return out, err, sels, costs


def multi3drefer_pairs(out, eval_types):
    """Multi3DReferEval.batch_metrics' (value, count) pairs from the per-item counts (multi3drefer_eval.py:33-41)."""
    f1 = [f1_pair(*map(int, r)) for r in out]
    s25, s50 = np.array([f[0] for f in f1]), np.array([f[1] for f in f1])
    m = {}
    for g in EVAL_TYPES:
        on = np.array([e == g for e in eval_types])
        m["iou25_" + g] = (sum(s25[on]), sum(on)) if np.any(on) else (0, 0)
        m["iou50_" + g] = (sum(s50[on]), sum(on)) if np.any(on) else (0, 0)
    m["iou25_overall"] = (sum(s25), len(s25))
    m["iou50_overall"] = (sum(s50), len(s50))
    return m


def accumulate(per_batch, target_metric):
    """BaseEvaluator.record over the batches' pairs: total value / max(total count, 1) per key, plus 'target_metric'."""
    res = {}
    for k in per_batch[0]:
        res[k] = sum(m[k][0] for m in per_batch) / max(sum(m[k][1] for m in per_batch), 1)
    res["target_metric"] = res[target_metric]
    return res
