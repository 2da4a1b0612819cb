"""Instance-segmentation mask AP from GPU overlap tables (csrc/instseg_ap.hip) and the ground-truth boxes of the evaluator.

The reference evaluates in InstSegEval.record (evaluator/instseg_eval.py) through common/eval_instseg.py: every scene's
full-resolution masks are kept on the host, assign_instances_for_scan recounts every (prediction, GT instance) intersection
with numpy passes over all points, and evaluate_matches runs the greedy matching as nested Python loops.  Here:

  ``overlap_tables``  one batched device pass over the [P_b, K] mask bytes of B scenes and their per-point GT ids
                      (label * 1000 + instance, 0 = unlabeled) -> per scene a few small integer arrays (two device-to-host
                      reads per call: the table sizes, then one packed buffer):
                        gt_ids [G]      the distinct nonzero ids whose label id // 1000 is valid, ascending;
                        gt_verts [G]    points of each id;
                        inter [K, G]    points shared by mask column k and instance g;
                        void [K]        points of column k whose label is not valid (unlabeled points included);
                        pred_verts [K]  points of column k.
  ``gt_boxes``        the GT boxes of InstSegEval.record_preds from full_masks [G', P] and raw_coordinates on the device.
  ``InstSegAP``       the matching and AP of evaluate_matches / compute_averages on those tables, in float64 on the host,
                      bit for bit the reference's numbers (tests/test_instseg_ap_ref.py, F23).

Semantics of ``InstSegAP.compute`` (common/eval_instseg.py, distance thresholds inf / -inf, one minimum region size):
  * a prediction counts when its class is a valid id and it has >= min_region_size points;
  * GT instances used for matching have id >= 1000 and >= min_region_size points; every same-label instance (also the
    small ones and groups) decides whether an unmatched prediction overlaps something, and the group / small ones add
    their intersections to its ignored points (a small group twice);
  * greedy matching per threshold: instances in ascending id order, their overlapping predictions in column order,
    predictions already taken skipped; the first match above the threshold takes the prediction, each further one adds a
    false positive at the lower score and keeps the higher score for the instance;
  * a prediction without a same-label overlap above the threshold is a false positive unless (void + ignored) / points
    > threshold;
  * AP per class and threshold from the unique score thresholds and the [-0.5, 0, 0.5] step widths; 0 for a class with
    GT but no predictions, NaN without GT; averages by nanmean over classes x thresholds without 0.25, np.average per class.
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .ops import SegmentPlan

INST = L.H.PQ3D_AP_INST                       # id = label * INST + instance
MAX_K, MAX_LABELS = L.H.PQ3D_AP_MAX_K, L.H.PQ3D_AP_MAX_LABELS       # valid label ids lie in [1, MAX_LABELS)
GT_CHUNK, BOX_PART_BYTES = L.H.PQ3D_INSTSEG_GT_CHUNK, L.H.PQ3D_INSTSEG_BOX_PART_BYTES


def default_overlaps() -> np.ndarray:
    """The reference's thresholds, built by the same expression (so the float64 values are identical)."""
    return np.append(np.arange(0.5, 0.95, 0.05), 0.25)


def _label_table(valid_class_ids) -> Tuple[np.ndarray, np.ndarray]:
    v = np.asarray(valid_class_ids).reshape(-1)
    if v.size == 0 or not np.issubdtype(v.dtype, np.integer):
        raise ValueError("valid_class_ids must be a non-empty sequence of integer label ids")
    labels = np.unique(v.astype(np.int64))
    if labels.size != v.size:
        raise ValueError("valid_class_ids holds duplicates")
    if labels[0] < 1 or labels[-1] >= MAX_LABELS:
        raise ValueError(f"valid label ids must lie in [1, {MAX_LABELS}) (label 0 marks unlabeled points)")
    rank = np.full(int(labels[-1]) + 1, -1, dtype=np.int32)
    rank[labels] = np.arange(labels.size, dtype=np.int32)
    return labels.astype(np.int32), rank


def _one_buffer(ts: Sequence[torch.Tensor]) -> torch.Tensor:
    """The per-scene tensors as one [sum of rows, ...] buffer: a view when they already lie back to back in one storage (the
    ``masks`` of instance_predictions' records), else a copy."""
    nz = [t for t in ts if t.numel()]
    ok = bool(nz) and all(t.is_contiguous() for t in nz)
    for a, b in zip(nz[:-1], nz[1:]):
        ok = ok and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()
    if ok and nz[0].untyped_storage().data_ptr() == nz[-1].untyped_storage().data_ptr():
        n = sum(int(t.shape[0]) for t in ts)
        return nz[0].as_strided((n,) + tuple(nz[0].shape[1:]), nz[0].stride())
    return torch.cat(list(ts)).contiguous()


def overlap_tables(masks: Sequence[torch.Tensor], gt_ids: Sequence[torch.Tensor], valid_class_ids) -> List[Dict[str, np.ndarray]]:
    """Per-scene overlap tables of ``masks[b]`` [P_b, K] bool and ``gt_ids[b]`` [P_b] int64 (device tensors, one K for the
    batch, 1 <= K <= 1024) for the label ids ``valid_class_ids``.  Returns one dict of host numpy arrays per scene:
    gt_ids [G] int64, gt_verts [G] int64, inter [K, G] int32, void [K] int64, pred_verts [K] int64.  Negative ids, shape,
    dtype and device mismatches raise ValueError."""
    B = len(masks)
    if B < 1 or len(gt_ids) != B:
        raise ValueError("one masks and one gt_ids tensor per scene, at least one scene")
    dev = masks[0].device
    if dev.type != "cuda":
        raise ValueError("overlap_tables needs device tensors (no CPU fallback)")
    for b in range(B):
        m, g = masks[b], gt_ids[b]
        if m.dtype != torch.bool or m.dim() != 2 or m.device != dev:
            raise ValueError(f"scene {b}: masks must be [P, K] bool on {dev}, got {tuple(m.shape)} {m.dtype} on {m.device}")
        if g.dtype != torch.int64 or g.dim() != 1 or g.device != dev:
            raise ValueError(f"scene {b}: gt_ids must be [P] int64 on {dev}, got {tuple(g.shape)} {g.dtype} on {g.device}")
        if g.shape[0] != m.shape[0]:
            raise ValueError(f"scene {b}: {m.shape[0]} mask rows but {g.shape[0]} GT ids")
    K = int(masks[0].shape[1])
    if not 1 <= K <= MAX_K or any(int(m.shape[1]) != K for m in masks):
        raise ValueError(f"every scene needs the same number of mask columns K in [1, {MAX_K}]")
    labels, rank = _label_table(valid_class_ids)
    P = [int(m.shape[0]) for m in masks]
    NP = sum(P)
    if NP >= (1 << 31) - 65536:
        raise ValueError(f"too many points for one call ({NP})")
    poff_h = np.concatenate([[0], np.cumsum(P)]).astype(np.int64)
    W = (labels.size * INST + 31) // 32
    mbuf = _one_buffer(masks)
    ids = _one_buffer(gt_ids)
    i32 = dict(dtype=torch.int32, device=dev)
    consts = torch.from_numpy(np.concatenate([rank, labels])).to(dev)
    lab_rank, labs = consts[:rank.size], consts[rank.size:]
    poff = torch.from_numpy(poff_h).to(dev)
    lkey = torch.empty(NP, **i32)
    bits = torch.empty(B * W, **i32)
    wpre = torch.empty(B * W, **i32)
    sizes = torch.empty(B + 1, dtype=torch.int64, device=dev)
    L.call("pq3d_ap_ids", ids, poff, B, NP, lab_rank, int(rank.size), W, lkey, bits, wpre, sizes,
           work=(f"B{B}P{NP}", 0.0, NP * 12.0 + B * W * 12.0))
    sz = sizes.cpu().numpy()                                # device-to-host read 1: table sizes + error bits
    if sz[B] & 1:
        raise ValueError("overlap_tables: gt_ids holds negative ids")
    G = sz[:B].astype(np.int64)
    goff_h = np.concatenate([[0], np.cumsum(G + 1)]).astype(np.int64)
    NG = int(goff_h[-1])
    tsz = G + G + K * G + 2 * K
    toff_h = np.concatenate([[0], np.cumsum(tsz)]).astype(np.int64)
    if NG >= (1 << 31) - 65536 or NG * K >= (1 << 40) or int(toff_h[-1]) >= (1 << 40):
        raise ValueError("overlap tables too large for one call")
    offs = torch.from_numpy(np.concatenate([goff_h, toff_h])).to(dev)
    goff, toff = offs[:B + 1], offs[B + 1:]
    key = torch.empty(NP, dtype=torch.int64, device=dev)
    L.call("pq3d_ap_keys", lkey, bits, wpre, poff, goff, B, NP, W, key, work=(f"B{B}P{NP}", 0.0, NP * 20.0))
    plan = SegmentPlan(key, NG)
    out = torch.empty(NG, K, **i32)
    L.call("pq3d_ap_count", mbuf, K, plan.buf, NP, NG, out, work=(f"B{B}P{NP}K{K}", 0.0, NP * (K + 4.0) + NG * K * 4.0))
    packed = torch.empty(int(toff_h[-1]), **i32)
    max_entries = int((G + K * G + K).max())
    L.call("pq3d_ap_pack", out, plan.buf, NP, NG, bits, wpre, labs, goff, toff, B, K, W, max_entries, packed,
           work=(f"B{B}NG{NG}K{K}", 0.0, NG * K * 4.0 + toff_h[-1] * 4.0))
    host = packed.cpu().numpy()                             # device-to-host read 2: every table of the batch
    res = []
    for b in range(B):
        g, t = int(G[b]), host[toff_h[b]:toff_h[b + 1]]
        res.append(dict(gt_ids=t[:g].astype(np.int64), gt_verts=t[g:2 * g].astype(np.int64),
                        inter=t[2 * g:2 * g + K * g].reshape(K, g).copy(), void=t[2 * g + K * g:2 * g + K * g + K].astype(np.int64),
                        pred_verts=t[2 * g + K * g + K:].astype(np.int64)))
    return res


def gt_boxes(full_masks: Sequence[torch.Tensor], raw_coordinates: Sequence[torch.Tensor]) -> List[Dict[str, torch.Tensor]]:
    """Boxes of the rows of ``full_masks[b]`` [G'_b, P_b] (bool or 0/1 uint8) over ``raw_coordinates[b]`` [P_b, 3] fp32, all
    device tensors: one dict per scene with ``boxes`` [G'_b, 6] fp32 (mean center xyz, max - min extent xyz; zeros for an
    empty row) and ``valid`` [G'_b] bool (row not empty) -- InstSegEval.record_preds' GT boxes before its ignore-label
    filter.  Sums in fp64 in a fixed order: bit-identical run to run."""
    B = len(full_masks)
    if B < 1 or len(raw_coordinates) != B:
        raise ValueError("one full_masks and one raw_coordinates tensor per scene, at least one scene")
    dev = full_masks[0].device
    if dev.type != "cuda":
        raise ValueError("gt_boxes needs device tensors (no CPU fallback)")
    rows, flat = [], []
    npts_first = 0
    for b in range(B):
        m, x = full_masks[b], raw_coordinates[b]
        if m.dtype not in (torch.bool, torch.uint8) or m.dim() != 2 or m.device != dev:
            raise ValueError(f"scene {b}: full_masks must be [G', P] bool / uint8 on {dev}")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3 or x.device != dev or x.shape[0] != m.shape[1]:
            raise ValueError(f"scene {b}: raw_coordinates must be [P, 3] fp32 on {dev} with P = {m.shape[1]}")
        rows.append((int(m.shape[0]), int(m.shape[1]), npts_first))
        npts_first += int(m.shape[1])
        flat.append(m.contiguous().view(torch.uint8).reshape(-1))
    R = sum(r[0] for r in rows)
    out = []
    if R == 0:
        return [dict(boxes=torch.zeros(0, 6, dtype=torch.float32, device=dev), valid=torch.zeros(0, dtype=torch.bool, device=dev))
                for _ in range(B)]
    if R >= 65536:
        raise ValueError(f"gt_boxes takes fewer than 65536 mask rows per call, got {R}")
    moff, pfirst, npts, chunks = [], [], [], []
    mb = 0
    for g, p, f in rows:
        for j in range(g):
            moff.append(mb + j * p)
            pfirst.append(f)
            npts.append(p)
            chunks.append((p + GT_CHUNK - 1) // GT_CHUNK)
        mb += g * p
    coff = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64)
    n_chunks = int(coff[-1])
    rinfo = torch.from_numpy(np.concatenate([moff, pfirst, npts, coff]).astype(np.int64)).to(dev)
    mbuf = torch.cat(flat) if len(flat) > 1 else flat[0]
    xyz = torch.cat([x.contiguous() for x in raw_coordinates]) if B > 1 else raw_coordinates[0].contiguous()
    ws = torch.empty(max(n_chunks, 1) * BOX_PART_BYTES, dtype=torch.uint8, device=dev)
    boxes = torch.empty(R, 6, dtype=torch.float32, device=dev)
    valid = torch.empty(R, dtype=torch.bool, device=dev)
    L.call("pq3d_instseg_gt_boxes", mbuf, xyz, rinfo, R, n_chunks, ws, ws.numel(), boxes, valid,
           work=(f"R{R}P{npts_first}", 0.0, mb + npts_first * 12.0 + R * 25.0))
    r0 = 0
    for g, _p, _f in rows:
        out.append(dict(boxes=boxes[r0:r0 + g], valid=valid[r0:r0 + g]))
        r0 += g
    return out


class InstSegAP:
    """Mask AP over overlap tables: ``add`` one scene at a time (a repeated key replaces the scene), ``records`` /
    ``extend`` move the per-scene data between processes (plain picklable tuples of numpy arrays), ``compute`` returns the
    raw ``ap`` [n_classes, n_overlaps] and a dict shaped like eval_instseg's return value.  ``valid_class_ids`` /
    ``class_labels``: the dataset's label ids and names, in the order of the result's classes."""

    def __init__(self, valid_class_ids, class_labels, min_region_size: int = 100, overlaps=None):
        self.valid_class_ids = np.asarray(valid_class_ids, dtype=np.int64).reshape(-1)
        self.class_labels = list(class_labels)
        if len(self.class_labels) != self.valid_class_ids.size:
            raise ValueError("one class label per valid class id")
        _label_table(self.valid_class_ids)
        self.min_region_size = int(min_region_size)
        self.overlaps = default_overlaps() if overlaps is None else np.asarray(overlaps, dtype=np.float64).reshape(-1)
        self._index = {int(c): i for i, c in enumerate(self.valid_class_ids)}
        self._scenes: Dict = {}

    def add(self, scene_key, table: Dict[str, np.ndarray], scores, classes) -> None:
        """One scene: ``table`` from overlap_tables, ``scores`` [K] and ``classes`` [K] (raw dataset label ids, after the
        evaluator's label mapping) of its mask columns."""
        scores = np.asarray(scores).reshape(-1)
        classes = np.asarray(classes).reshape(-1).astype(np.int64)
        K = table["pred_verts"].shape[0]
        if scores.shape[0] != K or classes.shape[0] != K or table["inter"].shape != (K, table["gt_ids"].shape[0]):
            raise ValueError(f"scene {scene_key!r}: scores / classes / tables disagree on K")
        self._scenes[scene_key] = (np.asarray(table["gt_ids"], np.int64), np.asarray(table["gt_verts"], np.int64),
                                   np.asarray(table["inter"]), np.asarray(table["void"], np.int64),
                                   np.asarray(table["pred_verts"], np.int64), scores, classes)

    def records(self) -> List[tuple]:
        return list(self._scenes.items())

    def extend(self, records) -> None:
        for k, v in records:
            self._scenes[k] = v

    def __len__(self) -> int:
        return len(self._scenes)

    # -- matching of one scene ------------------------------------------------------------------------------------------
    def _scene(self, rec, ys: List[List[list]], yt: List[List[list]], hard_fn: np.ndarray, has_gt: np.ndarray,
               has_pred: np.ndarray) -> None:
        gt_ids, gt_verts, inter, void, pred_verts, scores, classes = rec
        th = self.overlaps
        mrs = self.min_region_size
        pli = np.array([self._index.get(int(c), -1) for c in classes], dtype=np.int64)
        keep = (pli >= 0) & (pred_verts >= mrs)
        gli = np.array([self._index.get(int(i // INST), -1) for i in gt_ids], dtype=np.int64)
        for li in np.unique(np.concatenate([pli[keep], gli[gli >= 0]])):
            pc = np.nonzero(keep & (pli == li))[0]                # prediction columns of the class, column order
            gc = np.nonzero(gli == li)[0]                         # its GT instances, ascending id
            gv = gt_verts[gc]
            group = gt_ids[gc] < INST
            small = gv < mrs
            filt = ~group & ~small
            if filt.any():
                has_gt[li] = True
            if pc.size:
                has_pred[li] = True
            I = inter[pc][:, gc].astype(np.int64)                 # [np, ng]
            pv = pred_verts[pc]
            conf = scores[pc].astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                ov = np.where(I > 0, I.astype(np.float64) / (gv[None, :] + pv[:, None] - I), 0.0)
            # unmatched predictions: no same-label overlap above the threshold, ignored share <= threshold
            mo = ov.max(axis=1) if gc.size else np.zeros(pc.size)
            ign = void[pc] + (I * (group.astype(np.int64) + small.astype(np.int64))[None, :]).sum(axis=1)
            prop = ign.astype(np.float64) / pv if pc.size else np.zeros(0)
            fp_un = (mo[None, :] <= th[:, None]) & (prop[None, :] <= th[:, None])      # [n_th, np]
            # greedy matching, all thresholds at once
            fi = np.nonzero(filt)[0]
            nth = th.size
            visited = np.zeros((nth, pc.size), dtype=bool)
            matched = np.zeros((nth, fi.size), dtype=bool)
            best = np.full((nth, fi.size), -np.inf)
            extra_t: List[np.ndarray] = []
            extra_s: List[np.ndarray] = []
            for a, g in enumerate(fi):
                for p in np.nonzero(I[:, g] > 0)[0]:
                    hit = ~visited[:, p] & (ov[p, g] > th)
                    if not hit.any():
                        continue
                    again = hit & matched[:, a]
                    if again.any():
                        extra_t.append(np.nonzero(again)[0])
                        extra_s.append(np.minimum(best[again, a], conf[p]))
                        best[again, a] = np.maximum(best[again, a], conf[p])
                    first = hit & ~matched[:, a]
                    if first.any():
                        matched[first, a] = True
                        best[first, a] = conf[p]
                        visited[first, p] = True
            hard_fn[li] += fi.size - matched.sum(axis=1)
            for oi in range(nth):
                s_parts = [best[oi, matched[oi]], conf[fp_un[oi]]]
                t_parts = [np.ones(int(matched[oi].sum())), np.zeros(int(fp_un[oi].sum()))]
                for ti, sv in zip(extra_t, extra_s):
                    sel = ti == oi
                    if sel.any():
                        s_parts.append(sv[sel])
                        t_parts.append(np.zeros(int(sel.sum())))
                ys[li][oi].extend(s_parts)
                yt[li][oi].extend(t_parts)

    def compute(self) -> Tuple[np.ndarray, dict]:
        n_cls, nth = self.valid_class_ids.size, self.overlaps.size
        ys = [[[] for _ in range(nth)] for _ in range(n_cls)]
        yt = [[[] for _ in range(nth)] for _ in range(n_cls)]
        hard_fn = np.zeros((n_cls, nth), dtype=np.int64)
        has_gt = np.zeros(n_cls, dtype=bool)
        has_pred = np.zeros(n_cls, dtype=bool)
        for rec in self._scenes.values():
            self._scene(rec, ys, yt, hard_fn, has_gt, has_pred)
        ap = np.zeros((n_cls, nth), dtype=np.float64)
        for li in range(n_cls):
            for oi in range(nth):
                if has_gt[li] and has_pred[li]:
                    ap[li, oi] = _average_precision(np.concatenate([np.empty(0)] + ys[li][oi]),
                                                    np.concatenate([np.empty(0)] + yt[li][oi]), int(hard_fn[li, oi]))
                elif has_gt[li]:
                    ap[li, oi] = 0.0
                else:
                    ap[li, oi] = np.nan
        return ap, self._averages(ap)

    def _averages(self, ap: np.ndarray) -> dict:
        aps = ap[None]                                      # [distance thresholds = 1, classes, overlaps]
        o50 = np.where(np.isclose(self.overlaps, 0.5))
        o25 = np.where(np.isclose(self.overlaps, 0.25))
        rest = np.where(np.logical_not(np.isclose(self.overlaps, 0.25)))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            res = {"all_ap": np.nanmean(aps[0, :, rest]), "all_ap_50%": np.nanmean(aps[0, :, o50]),
                   "all_ap_25%": np.nanmean(aps[0, :, o25]), "classes": {}}
            for li, name in enumerate(self.class_labels):
                res["classes"][name] = {"ap": np.average(aps[0, li, rest]), "ap50%": np.average(aps[0, li, o50]),
                                        "ap25%": np.average(aps[0, li, o25])}
        return res


def _average_precision(y_score: np.ndarray, y_true: np.ndarray, hard_fn: int) -> float:
    """Area under the precision-recall curve of one class and threshold, as evaluate_matches integrates it."""
    order = np.argsort(y_score)
    srt = y_score[order]
    csum = np.cumsum(y_true[order])
    _, first = np.unique(srt, return_index=True)
    n = len(srt)
    n_true = csum[-1] if len(csum) > 0 else 0
    csum = np.append(csum, 0)
    prec = np.zeros(len(first) + 1)
    rec = np.zeros(len(first) + 1)
    below = csum[first - 1]                                 # true examples scored below each threshold (index -1 -> 0)
    tp = n_true - below
    fp = (n - first) - tp
    fn = below + hard_fn
    prec[:-1] = tp / (tp + fp)
    rec[:-1] = tp / (tp + fn)
    prec[-1], rec[-1] = 1.0, 0.0
    r = np.append(np.append(rec[0], rec), 0.0)
    steps = np.convolve(r, [-0.5, 0, 0.5], "valid")
    return float(np.dot(prec, steps))
