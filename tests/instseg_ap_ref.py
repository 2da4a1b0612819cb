"""CPU restatement of instance-segmentation mask AP (common/eval_instseg.py: assign_instances_for_scan, evaluate_matches,
compute_averages) and of the evaluator's GT boxes (InstSegEval.record_preds), written loop by loop from their definition --
the checker of pq3d_amd.instseg_ap.  Not imported by the product."""
from __future__ import annotations

import numpy as np

INST = 1000


def overlaps_default():
    return np.append(np.arange(0.5, 0.95, 0.05), 0.25)


def point_tables(masks, ids, valid_class_ids):
    """Tables of one scene from its points: masks [P, K] bool, ids [P] int64 (label * 1000 + instance, 0 = unlabeled)."""
    masks = np.asarray(masks, dtype=bool)
    ids = np.asarray(ids, dtype=np.int64)
    valid = set(int(v) for v in valid_class_ids)
    labelled = np.isin(ids // INST, list(valid))
    gt = [int(i) for i in np.unique(ids) if i != 0 and int(i) // INST in valid]
    K = masks.shape[1]
    inter = np.zeros((K, len(gt)), dtype=np.int64)
    verts = np.zeros(len(gt), dtype=np.int64)
    for g, gid in enumerate(gt):
        rows = masks[ids == gid]
        verts[g] = rows.shape[0]
        inter[:, g] = rows.sum(0)
    void = masks[~labelled].sum(0).astype(np.int64)
    return dict(gt_ids=np.array(gt, dtype=np.int64), gt_verts=verts, inter=inter, void=void,
                pred_verts=masks.sum(0).astype(np.int64))


def _pr_area(y_true, y_score, hard_fn):
    """Precision-recall area of one class and threshold: the curve at every unique score threshold plus the artificial
    first point (precision 1, recall 0), integrated with step widths (r[i-1] - r[i+1]) / 2 (np.convolve with [-0.5, 0, 0.5])."""
    y_true = np.asarray(y_true, dtype=np.float64)
    y_score = np.asarray(y_score, dtype=np.float64)
    o = np.argsort(y_score)
    s, t = y_score[o], y_true[o]
    c = np.cumsum(t)
    n = len(s)
    total = c[-1] if n else 0
    thr_first = [i for i in range(n) if i == 0 or s[i] != s[i - 1]]
    prec, rec = [], []
    for i in thr_first:
        below = c[i - 1] if i > 0 else 0.0
        tp = total - below
        fp = (n - i) - tp
        fn = below + hard_fn
        prec.append(float(tp) / (tp + fp))
        rec.append(float(tp) / (tp + fn))
    prec = np.array(prec + [1.0])
    rec = np.array(rec + [0.0])
    padded = np.concatenate([[rec[0]], rec, [0.0]])
    steps = np.convolve(padded, [-0.5, 0, 0.5], "valid")
    return np.dot(prec, steps)


def ap_from_tables(scenes, valid_class_ids, min_region_size=100, overlaps=None):
    """scenes: list of (table, scores [K], classes [K] raw ids).  Returns ap [n_classes, n_overlaps] (class order of
    valid_class_ids)."""
    overlaps = overlaps_default() if overlaps is None else np.asarray(overlaps, dtype=np.float64)
    valid = [int(v) for v in valid_class_ids]
    ap = np.zeros((len(valid), len(overlaps)))
    for oi, th in enumerate(overlaps):
        for li, lab in enumerate(valid):
            y_true, y_score = [], []
            hard_fn = 0
            has_gt = has_pred = False
            for tab, scores, classes in scenes:
                gts = [g for g in range(len(tab["gt_ids"])) if int(tab["gt_ids"][g]) // INST == lab]
                preds = [k for k in range(len(classes)) if int(classes[k]) == lab and tab["pred_verts"][k] >= min_region_size]
                used = [g for g in gts if tab["gt_ids"][g] >= INST and tab["gt_verts"][g] >= min_region_size]
                has_gt = has_gt or bool(used)
                has_pred = has_pred or bool(preds)
                taken = set()
                for g in used:
                    score = None
                    for k in preds:
                        it = int(tab["inter"][k, g])
                        if it == 0 or k in taken:
                            continue
                        iou = float(it) / (tab["gt_verts"][g] + tab["pred_verts"][k] - it)
                        if iou <= th:
                            continue
                        conf = float(scores[k])
                        if score is None:
                            score = conf
                            taken.add(k)
                        else:
                            y_true.append(0.0)
                            y_score.append(min(score, conf))
                            score = max(score, conf)
                    if score is None:
                        hard_fn += 1
                    else:
                        y_true.append(1.0)
                        y_score.append(score)
                for k in preds:
                    pv = int(tab["pred_verts"][k])
                    hit = False
                    ignore = int(tab["void"][k])
                    for g in gts:
                        it = int(tab["inter"][k, g])
                        if it == 0:
                            continue
                        if float(it) / (tab["gt_verts"][g] + pv - it) > th:
                            hit = True
                        if tab["gt_ids"][g] < INST:
                            ignore += it
                        if tab["gt_verts"][g] < min_region_size:
                            ignore += it
                    if not hit and float(ignore) / pv <= th:
                        y_true.append(0.0)
                        y_score.append(float(scores[k]))
            if has_gt and has_pred:
                ap[li, oi] = _pr_area(y_true, y_score, hard_fn)
            elif has_gt:
                ap[li, oi] = 0.0
            else:
                ap[li, oi] = np.nan
    return ap


def averages(ap, class_labels, overlaps=None):
    """all_ap over classes x thresholds without 0.25 (NaN ignored), all_ap_50% / _25%, and per class ap / ap50% / ap25%.
    The reductions run over contiguous threshold-major copies, the element order of the reference's indexing."""
    overlaps = overlaps_default() if overlaps is None else np.asarray(overlaps, dtype=np.float64)
    rest = [i for i in range(len(overlaps)) if not np.isclose(overlaps[i], 0.25)]
    i50 = [i for i in range(len(overlaps)) if np.isclose(overlaps[i], 0.5)]
    i25 = [i for i in range(len(overlaps)) if np.isclose(overlaps[i], 0.25)]
    out = {"all_ap": np.nanmean(np.ascontiguousarray(ap[:, rest].T)),
           "all_ap_50%": np.nanmean(np.ascontiguousarray(ap[:, i50].T)),
           "all_ap_25%": np.nanmean(np.ascontiguousarray(ap[:, i25].T)), "classes": {}}
    for li, name in enumerate(class_labels):
        out["classes"][name] = {"ap": np.mean(ap[li, rest]), "ap50%": np.mean(ap[li, i50]), "ap25%": np.mean(ap[li, i25])}
    return out


def gt_boxes_f64(full_masks, xyz):
    """Boxes of the rows of full_masks [G', P] over xyz [P, 3]: float64 mean center, max - min extent; valid = row not
    empty."""
    full_masks = np.asarray(full_masks).astype(bool)
    xyz = np.asarray(xyz)
    boxes = np.zeros((full_masks.shape[0], 6))
    valid = np.zeros(full_masks.shape[0], dtype=bool)
    for r in range(full_masks.shape[0]):
        pts = xyz[full_masks[r]]
        if len(pts):
            boxes[r, :3] = pts.astype(np.float64).mean(0)
            boxes[r, 3:] = pts.max(0) - pts.min(0)
            valid[r] = True
    return boxes, valid
