"""Restatement of the reference's box AP (common/eval_det.py: calc_iou, eval_det_cls, eval_det, voc_ap) and of the averages
InstSegEval.record (evaluator/instseg_eval.py:151-243) adds on top of eval_instseg, written loop by loop from their
definition in numpy.  Besides the APs it returns, per detection, ovmax, jmax and the TP flag -- what pq3d_box_match computes.

Records: ``preds[scene]`` is a list of (class, box [6] fp32, score) in column order, ``gts[scene]`` a list of (label, box [6]
fp32); both dicts in the order the scenes were recorded.  Equal scores inside a class are walked in a stable order (scene
order, then column): the reference's np.argsort(-confidence) leaves that order open."""
import math

import numpy as np


def calc_iou(a, b):
    """a, b: [6] float64 (centre | extent)."""
    lo, hi = [0.0] * 3, [0.0] * 3
    for k in range(3):
        max_a, max_b = a[k] + a[3 + k] / 2, b[k] + b[3 + k] / 2
        min_a, min_b = a[k] - a[3 + k] / 2, b[k] - b[3 + k] / 2
        hi[k] = max_a if max_a < max_b else max_b
        lo[k] = min_a if min_a > min_b else min_b
    if not all(hi[k] > lo[k] for k in range(3)):
        return 0.0
    inter = ((hi[0] - lo[0]) * (hi[1] - lo[1])) * (hi[2] - lo[2])
    vol_a = (a[3] * a[4]) * a[5]
    vol_b = (b[3] * b[4]) * b[5]
    return 1.0 * inter / (vol_a + vol_b - inter)


def voc_ap(rec, prec):
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def class_order(preds, gts):
    """The insertion order of eval_det's gt dict: every prediction class as met, scene by scene, then the other GT classes."""
    order = {}
    for sid in preds:
        for c, _b, _s in preds[sid]:
            order.setdefault(c)
    for sid in gts:
        for c, _b in gts[sid]:
            order.setdefault(c)
    return list(order)


def eval_det(preds, gts, ovthresh):
    """-> (ap {class: float64} in eval_det's key order, per scene a list over its detections of (ovmax, jmax, tp)); jmax is
    the index into gts[scene] (all classes), -1 without a same-class GT box."""
    ap = {}
    info = {sid: [None] * len(p) for sid, p in preds.items()}
    for c in class_order(preds, gts):
        dets = [(sid, k) for sid in preds for k, d in enumerate(preds[sid]) if d[0] == c]
        conf = np.array([preds[sid][k][2] for sid, k in dets], dtype=np.float64)
        srt = np.argsort(-conf, kind="stable")
        rows = {sid: [j for j, g in enumerate(gts.get(sid, [])) if g[0] == c] for sid in set(preds) | set(gts)}
        npos = sum(len(r) for r in rows.values())
        taken = {sid: [False] * len(r) for sid, r in rows.items()}
        tp, fp = np.zeros(len(dets)), np.zeros(len(dets))
        for d, i in enumerate(srt):
            sid, k = dets[i]
            bb = preds[sid][k][1].astype(float)
            ovmax, jmax = -np.inf, -1
            for jj, j in enumerate(rows[sid]):
                iou = calc_iou(bb, gts[sid][j][1].astype(float))
                if iou > ovmax:
                    ovmax, jmax = iou, jj
            hit = False
            if ovmax > ovthresh:
                if not taken[sid][jmax]:
                    hit = taken[sid][jmax] = True
            tp[d], fp[d] = float(hit), float(not hit)
            info[sid][k] = (ovmax, rows[sid][jmax] if jmax >= 0 else -1, hit)
        fp, tp = np.cumsum(fp), np.cumsum(tp)
        with np.errstate(invalid="ignore", divide="ignore"):
            rec = tp / float(npos)
            prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            ap[c] = voc_ap(rec, prec)
    return ap, info


def mean_ap(ap):
    vals = [v for v in ap.values() if not math.isnan(v)]
    return sum(vals) / len(vals) if vals else float("nan")


def box_results(preds, gts, name_of=str):
    """The box keys of InstSegEval.record."""
    ap50, ap25 = eval_det(preds, gts, 0.5)[0], eval_det(preds, gts, 0.25)[0]
    res = {"mean_box_ap_25": mean_ap(ap25), "mean_box_ap_50": mean_ap(ap50)}
    for c, v in ap50.items():
        res[f"{name_of(c)}_val_box_ap_50"] = v
    for c, v in ap25.items():
        res[f"{name_of(c)}_val_box_ap_25"] = v
    return res


def group_results(classes, group_order, head, common, tail):
    """The nine group means and mean_ap / mean_ap_50 / mean_ap_25 from eval_instseg's per-class dict."""
    import warnings
    rows = {"head": [], "common": [], "tail": []}
    for name in group_order:
        if name not in classes:
            continue
        row = np.array((float(classes[name]["ap"]), float(classes[name]["ap50%"]), float(classes[name]["ap25%"])))
        if name in head:
            rows["head"].append(row)
        elif name in common:
            rows["common"].append(row)
        elif name in tail:
            rows["tail"].append(row)
    arr = {g: np.stack(v) for g, v in rows.items()}
    res = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        means = {g: np.nanmean(arr[g], axis=0) for g in ("tail", "common", "head")}
        for i, suffix in enumerate(("ap", "ap_50", "ap_25")):
            for g in ("tail", "common", "head"):
                res[f"mean_{g}_{suffix}"] = means[g][i]
        o = np.nanmean(np.vstack((arr["head"], arr["common"], arr["tail"])), axis=0)
    res["mean_ap"], res["mean_ap_50"], res["mean_ap_25"] = o[0], o[1], o[2]
    return res


def match_arrays(preds, gts, thresholds):
    """Per scene (ovmax [K] float64, jmax [K] int32, flags [K] uint8) of record lists, for comparison with box_match."""
    infos = [eval_det(preds, gts, t)[1] for t in thresholds]
    out = {}
    for sid, p in preds.items():
        ov = np.array([infos[0][sid][k][0] for k in range(len(p))], dtype=np.float64)
        jm = np.array([infos[0][sid][k][1] for k in range(len(p))], dtype=np.int32)
        fl = np.zeros(len(p), dtype=np.uint8)
        for t, inf in enumerate(infos):
            assert all(inf[sid][k][0] == ov[k] and inf[sid][k][1] == jm[k] for k in range(len(p)))
            fl |= (np.array([inf[sid][k][2] for k in range(len(p))], dtype=bool).reshape(-1).astype(np.uint8) << t).astype(np.uint8)
        out[sid] = (ov.reshape(-1), jm.reshape(-1), fl.reshape(-1))
    return out
