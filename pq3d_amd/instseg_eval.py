"""Stage-1 evaluation on the device: box AP (include/pq3d_hip.h: pq3d_box_match; csrc/instseg_box.hip) and one
``InstSegEval`` with the reference's ``update`` / ``record`` (evaluator/instseg_eval.py) around instance_predictions,
overlap_tables / InstSegAP, gt_boxes and the box matching.

  ``box_match``    the matching of eval_det_cls (common/eval_det.py) for a batch of scenes in one launch: per detection the best
                   same-class GT box of its scene (ovmax, jmax) and one TP bit per IoU threshold.  Device tensors in, device
                   tensors out, no host read: it can be captured (the small offset / threshold tensors of a batch shape are
                   made once and kept).
  ``BoxAP``        per detection (class, score, flags), per scene the GT labels; ``compute`` does the global per-class stable
                   sort, the cumulative sums, voc_ap and the mean in float64 numpy on the host, in eval_det's key order.
  ``InstSegEval``  ``update(data_dict)`` launches everything and keeps the box records on the device; ``record()`` makes one
                   device-to-host copy of them and returns ``(is_best, results)`` with every key of the reference's record().

Rules of the matching: a detection looks at the GT boxes of its own scene with its own class; ovmax / jmax are the
first maximum of calc_iou under a strict >; it is a TP at threshold t iff ovmax > t and no detection of the scene with the same
jmax and ovmax > t comes before it in score order.  np.argsort(-confidence) of the reference is not stable, so the order of
equal scores is not pinned there; here it is the order of ``update`` (of ``add``), then the column.

Not covered, and raised rather than skipped where a caller could ask for it: gathering across ranks (``records`` / ``extend``
move the state between processes), the ``save`` JSON and the heatmaps."""
from __future__ import annotations

import functools
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .instseg import instance_predictions
from .instseg_ap import MAX_K, InstSegAP, gt_boxes, overlap_tables

MAX_G, MAX_T = L.H.PQ3D_BOX_MAX_G, L.H.PQ3D_BOX_MAX_T
ERR_NAN_SCORE, ERR_PRED_BOX, ERR_GT_BOX, ERR_OFFSETS = 1, 2, 4, 8
_ERRORS = {ERR_NAN_SCORE: "a NaN score", ERR_PRED_BOX: "a non-finite prediction box", ERR_GT_BOX: "a non-finite GT box",
           ERR_OFFSETS: "scene offsets out of range"}


@functools.lru_cache(maxsize=64)
def _consts(dev: torch.device, K: Tuple[int, ...], G: Tuple[int, ...], thresholds: Tuple[float, ...]):
    """The offset and threshold tensors of one batch shape, made once per (device, shape): a later call with the same shape
    copies nothing from the host, so it can be captured."""
    off = np.concatenate([[0], np.cumsum(K), [0], np.cumsum(G)]).astype(np.int64)
    off = torch.from_numpy(off).to(dev)
    return off[:len(K) + 1], off[len(K) + 1:], torch.tensor(thresholds, dtype=torch.float64).to(dev)


def _flat(ts: Sequence[torch.Tensor], dtype, tail: Tuple[int, ...], dev, who: str, name: str) -> torch.Tensor:
    out = []
    for b, t in enumerate(ts):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
            raise ValueError(f"{who}: scene {b}: {name} must be a device tensor [n{''.join(', %d' % x for x in tail)}] on {dev}")
        if t.dtype == torch.bool and dtype == torch.uint8:
            t = t.contiguous().view(torch.uint8)
        if t.dtype != dtype:
            raise ValueError(f"{who}: scene {b}: {name} must be {dtype}, got {t.dtype}")
        out.append(t)
    return (torch.cat(out) if len(out) > 1 else out[0]).contiguous()


def box_match(pred_records: Sequence[Dict[str, torch.Tensor]], gt_records: Sequence[Dict[str, torch.Tensor]],
              thresholds: Sequence[float] = (0.25, 0.5)) -> Dict[str, object]:
    """The box matching of one batch.  ``pred_records[b]``: ``boxes`` [K_b, 6] fp32, ``classes`` [K_b] int64, ``scores``
    [K_b] fp32, ``box_valid`` [K_b] bool / uint8 (the records of instance_predictions, classes after the label mapping);
    ``gt_records[b]``: ``boxes`` [G_b, 6] fp32, ``labels`` [G_b] int64, ``valid`` [G_b] bool / uint8.  K_b <= 1024, G_b <= 4096,
    1 <= len(thresholds) <= 4 (ValueError before any launch).

    Returns device tensors over the concatenated detections: ``ovmax`` [NK] fp64, ``jmax`` [NK] int32 (scene-local GT row),
    ``flags`` [NK] uint8 (bit t: TP at thresholds[t]), ``err`` [1] int32 (ERR_* bits; ``check_errors`` reads it), and
    ``koff`` / ``goff``, the host offsets of the scenes (``consts``: the device offsets and thresholds the launch read)."""
    who = "box_match"
    B = len(pred_records)
    if B < 1 or len(gt_records) != B:
        raise ValueError(f"{who}: one prediction and one GT record per scene, at least one scene")
    thr = tuple(float(t) for t in thresholds)
    if not 1 <= len(thr) <= MAX_T:
        raise ValueError(f"{who}: 1 to {MAX_T} thresholds, got {len(thr)}")
    dev = pred_records[0]["boxes"].device
    if dev.type != "cuda":
        raise ValueError(f"{who} needs device tensors (no CPU fallback)")
    pb = _flat([r["boxes"] for r in pred_records], torch.float32, (6,), dev, who, "boxes")
    pc = _flat([r["classes"] for r in pred_records], torch.int64, (), dev, who, "classes")
    ps = _flat([r["scores"] for r in pred_records], torch.float32, (), dev, who, "scores")
    pv = _flat([r["box_valid"] for r in pred_records], torch.uint8, (), dev, who, "box_valid")
    gb = _flat([r["boxes"] for r in gt_records], torch.float32, (6,), dev, who, "GT boxes")
    gl = _flat([r["labels"] for r in gt_records], torch.int64, (), dev, who, "GT labels")
    gv = _flat([r["valid"] for r in gt_records], torch.uint8, (), dev, who, "GT valid")
    K = tuple(int(r["boxes"].shape[0]) for r in pred_records)
    G = tuple(int(r["boxes"].shape[0]) for r in gt_records)
    for b in range(B):
        if not (pred_records[b]["classes"].shape[0] == pred_records[b]["scores"].shape[0] == pred_records[b]["box_valid"].shape[0] == K[b]):
            raise ValueError(f"{who}: scene {b}: boxes / classes / scores / box_valid disagree on K")
        if not (gt_records[b]["labels"].shape[0] == gt_records[b]["valid"].shape[0] == G[b]):
            raise ValueError(f"{who}: scene {b}: GT boxes / labels / valid disagree on G")
        if K[b] > MAX_K:
            raise ValueError(f"{who}: scene {b}: {K[b]} detections, at most {MAX_K} per scene")
        if G[b] > MAX_G:
            raise ValueError(f"{who}: scene {b}: {G[b]} GT boxes, at most {MAX_G} per scene")
    koff, goff, thr_d = _consts(dev, K, G, thr)
    NK, NG = sum(K), sum(G)
    ovmax = torch.empty(NK, dtype=torch.float64, device=dev)
    jmax = torch.empty(NK, dtype=torch.int32, device=dev)
    flags = torch.empty(NK, dtype=torch.uint8, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    L.call("pq3d_box_match", pb, pc, ps, pv, koff, NK, gb, gl, gv, goff, NG, thr_d, len(thr), B, max(G), ovmax, jmax, flags, err,
           work=(f"B{B}K{NK}G{NG}T{len(thr)}", 0.0, NK * 50.0 + NG * 33.0))
    return dict(ovmax=ovmax, jmax=jmax, flags=flags, err=err, koff=np.concatenate([[0], np.cumsum(K)]).astype(np.int64),
                goff=np.concatenate([[0], np.cumsum(G)]).astype(np.int64),
                consts=(koff, goff, thr_d))                   # (whoever replays a captured call keeps them alive with the result)


def check_errors(err: int, who: str = "box_match") -> None:
    L.raise_error_word(who, err, _ERRORS)


def voc_ap(rec: np.ndarray, prec: np.ndarray) -> np.float64:
    """Area under the precision envelope over the recall steps (VOC, the all-points form)."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


class BoxAP:
    """Box AP over matched detections: ``add`` one scene at a time (a repeated key replaces the scene and keeps its place),
    ``records`` / ``extend`` move the per-scene data between processes (plain picklable tuples of numpy arrays), ``compute``
    returns per threshold ``{class_id: ap}`` (in eval_det's key order: the prediction classes as met, scene by scene, then the
    remaining GT classes) and the mean over the classes that are not NaN (NaN when there is none)."""

    def __init__(self, thresholds: Sequence[float] = (0.25, 0.5)):
        self.thresholds = tuple(float(t) for t in thresholds)
        if not 1 <= len(self.thresholds) <= MAX_T:
            raise ValueError(f"1 to {MAX_T} thresholds")
        self._scenes: Dict = {}

    def add(self, scene_key, classes, scores, flags, gt_labels) -> None:
        """One scene: ``classes`` / ``scores`` / ``flags`` [n] of its detections in column order (valid boxes only), and
        ``gt_labels`` [g], the labels of its GT boxes."""
        classes = np.asarray(classes).reshape(-1).astype(np.int64)
        scores = np.asarray(scores).reshape(-1)
        flags = np.asarray(flags).reshape(-1).astype(np.uint8)
        if not classes.shape == scores.shape == flags.shape:
            raise ValueError(f"scene {scene_key!r}: classes / scores / flags disagree on the number of detections")
        if np.isnan(scores).any():
            raise ValueError(f"scene {scene_key!r}: a NaN score")
        self._scenes[scene_key] = (classes, scores, flags, np.asarray(gt_labels).reshape(-1).astype(np.int64))

    def records(self) -> List[tuple]:
        return list(self._scenes.items())

    def extend(self, records) -> None:
        for k, v in records:
            self._scenes[k] = v

    def __len__(self) -> int:
        return len(self._scenes)

    def compute(self) -> Tuple[List[Dict[int, np.float64]], List[float]]:
        order: Dict[int, None] = {}
        for classes, _s, _f, _g in self._scenes.values():
            for c in classes.tolist():
                order.setdefault(c)
        for _c, _s, _f, gl in self._scenes.values():
            for c in gl.tolist():
                order.setdefault(c)
        cls_all = np.concatenate([np.empty(0, np.int64)] + [v[0] for v in self._scenes.values()])
        sc_all = np.concatenate([np.empty(0)] + [v[1].astype(np.float64) for v in self._scenes.values()])
        fl_all = np.concatenate([np.empty(0, np.uint8)] + [v[2] for v in self._scenes.values()])
        gl_all = np.concatenate([np.empty(0, np.int64)] + [v[3] for v in self._scenes.values()])
        aps: List[Dict[int, np.float64]] = [{} for _ in self.thresholds]
        for c in order:
            sel = cls_all == c
            conf, fl = sc_all[sel], fl_all[sel]
            srt = np.argsort(-conf, kind="stable")            # order of add, then column, among equal scores
            npos = int((gl_all == c).sum())
            for t in range(len(self.thresholds)):
                hit = ((fl[srt] >> t) & 1).astype(np.float64)
                tp, fp = np.cumsum(hit), np.cumsum(1.0 - hit)
                with np.errstate(invalid="ignore", divide="ignore"):
                    rec = tp / float(npos)
                    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
                    aps[t][c] = voc_ap(rec, prec)
        means = []
        for t in range(len(self.thresholds)):
            vals = [v for v in aps[t].values() if not np.isnan(v)]
            means.append(sum(vals) / len(vals) if vals else float("nan"))
        return aps, means


def _label_lut(id_map: Optional[Dict[int, int]]) -> Optional[np.ndarray]:
    if not id_map:
        return None
    keys = np.array([int(k) for k in id_map], dtype=np.int64)
    if keys.min() < 0 or keys.max() >= (1 << 20):
        raise ValueError("id_map keys must lie in [0, 2^20)")
    lut = np.arange(int(keys.max()) + 1, dtype=np.int64)
    lut[keys] = np.array([int(v) for v in id_map.values()], dtype=np.int64)
    return lut


class InstSegEval:
    """The reference's stage-1 evaluator (evaluator/instseg_eval.py) on the device.

    ``valid_class_ids`` / ``class_labels``: the dataset's raw label ids and names (InstSegAP).  ``id_map``: the
    scannet200_id_to_scannet_raw_id dict, applied to the predicted classes and to instance_labels on the device through a
    lookup table; ids not in it (``ignore_label`` too) pass unchanged.  ``class_names``: raw id -> name for the
    ``<name>_val_box_ap_25/50`` keys (str(id) without it).  ``groups`` = {"head": [...], "common": [...], "tail": [...]} and
    ``group_order``: the dataset's class-name lists (the reference's HEAD_ / COMMON_ / TAIL_CATS_SCANNET_200 and
    VALID_CLASS_IDS_200_VALIDATION); without them the ``mean_*`` group keys are left out.

    ``update(data_dict)`` reads predictions_class, predictions_mask, voxel2segment, voxel_to_full_maps, segment_to_full_maps,
    raw_coordinates, instance_labels, full_masks, scan_id (voxel_features with DBSCAN) as device tensors or per-scene lists,
    and ``gt_ids``: per scene [P_b] int64, label * 1000 + instance (the reference reads them from inst_ids_mask3d/<scan>.txt
    at record time).  A repeated scan_id replaces the scene.  ``record()`` returns ``(is_best, results)`` and clears the
    per-scene state."""

    def __init__(self, valid_class_ids, class_labels, *, id_map: Optional[Dict[int, int]] = None,
                 class_names: Optional[Dict[int, str]] = None, groups: Optional[Dict[str, Sequence[str]]] = None,
                 group_order: Optional[Sequence[str]] = None, topk_per_scene: int = 100, use_dbscan: bool = False,
                 filter_out_no_object_queries: bool = False, dbscan_eps: float = 0.95, ignore_label: int = -100,
                 min_region_size: int = 100, target_metric: str = "all_ap", save: bool = False):
        if save:
            raise NotImplementedError("InstSegEval: the save JSON is not covered")
        if (groups is None) != (group_order is None):
            raise ValueError("pass groups and group_order together")
        if groups is not None and sorted(groups) != ["common", "head", "tail"]:
            raise ValueError('groups needs exactly the keys "head", "common" and "tail"')
        self.mask_ap = InstSegAP(valid_class_ids, class_labels, min_region_size=min_region_size)
        self.box_ap = BoxAP((0.25, 0.5))
        self.valid_class_ids = self.mask_ap.valid_class_ids
        self._lut_h = _label_lut(id_map)
        self._lut: Dict[torch.device, torch.Tensor] = {}
        self.class_names = dict(class_names) if class_names is not None else None
        self.groups = {k: set(v) for k, v in groups.items()} if groups is not None else None
        self.group_order = list(group_order) if group_order is not None else None
        self.topk_per_scene = int(topk_per_scene)
        self.use_dbscan, self.filter_out_no_object_queries = bool(use_dbscan), bool(filter_out_no_object_queries)
        self.dbscan_eps = float(dbscan_eps)
        self.ignore_label = int(ignore_label)
        self.target_metric = target_metric
        self.best_result = -np.inf
        self.total_count = 0
        self._pending: Dict = {}                              # scan_id -> device box record, until record() / records()

    # -- label mapping ------------------------------------------------------------------------------------------------------
    def _map(self, x: torch.Tensor) -> torch.Tensor:
        if self._lut_h is None:
            return x
        lut = self._lut.get(x.device)
        if lut is None:
            lut = self._lut[x.device] = torch.from_numpy(self._lut_h).to(x.device)
        inside = (x >= 0) & (x < lut.numel())
        return torch.where(inside, lut[x.clamp(0, lut.numel() - 1)], x)

    # -- update -----------------------------------------------------------------------------------------------------------------
    def update(self, data_dict) -> None:
        d = data_dict
        logits, masks = d["predictions_class"], d["predictions_mask"]
        logits = logits[-1] if isinstance(logits, (list, tuple)) else logits
        masks = masks[-1] if isinstance(masks, (list, tuple)) else masks
        if isinstance(masks, (list, tuple)):
            masks = torch.stack(list(masks))
        scan_ids = list(d["scan_id"])
        B = len(scan_ids)
        if logits.dim() != 3 or logits.shape[0] != B:
            raise ValueError("predictions_class[-1] must be [B, Q, C+1] with one scan_id per scene")
        raw = list(d["raw_coordinates"])
        vox = None
        if self.use_dbscan:
            vf = d["voxel_features"]
            if isinstance(vf, torch.Tensor):                 # the batch's voxels back to back, coordinates in the last 3 columns
                vox = [t.contiguous() for t in vf[:, -3:].split([int(v.numel()) for v in d["voxel2segment"]])]
            else:
                vox = [t[:, -3:].contiguous() for t in vf]
        recs = instance_predictions(logits, masks, list(d["voxel2segment"]), list(d["voxel_to_full_maps"]),
                                    list(d["segment_to_full_maps"]), raw, topk_per_scene=self.topk_per_scene,
                                    filter_out_no_object_queries=self.filter_out_no_object_queries, use_dbscan=self.use_dbscan,
                                    voxel_coordinates=vox, dbscan_eps=self.dbscan_eps)
        classes = [self._map(r["classes"]) for r in recs]
        gt_ids = list(d["gt_ids"])
        full_masks, inst = list(d["full_masks"]), list(d["instance_labels"])
        if not (len(gt_ids) == len(full_masks) == len(inst) == B):
            raise ValueError("one gt_ids / full_masks / instance_labels entry per scene")
        # mask AP: overlap tables (scenes of one K per call), scores and classes to the host
        tables: List[Optional[dict]] = [None] * B
        by_k: Dict[int, List[int]] = {}
        for b, r in enumerate(recs):
            by_k.setdefault(int(r["masks"].shape[1]), []).append(b)
        for K, bs in by_k.items():
            if K == 0:                                        # (DBSCAN / the filter can leave a scene without columns)
                ms = [torch.zeros(recs[b]["masks"].shape[0], 1, dtype=torch.bool, device=logits.device) for b in bs]
            else:
                ms = [recs[b]["masks"] for b in bs]
            for b, t in zip(bs, overlap_tables(ms, [gt_ids[b] for b in bs], self.valid_class_ids)):
                if K == 0:
                    t = dict(t, inter=t["inter"][:0], void=t["void"][:0], pred_verts=t["pred_verts"][:0])
                tables[b] = t
        sc_h = torch.cat([r["scores"] for r in recs]).cpu().numpy()
        cl_h = torch.cat(classes).cpu().numpy()
        k0 = 0
        for b, r in enumerate(recs):
            K = int(r["scores"].shape[0])
            self.mask_ap.add(scan_ids[b], tables[b], sc_h[k0:k0 + K], cl_h[k0:k0 + K])
            k0 += K
        # box AP: GT boxes, matching; everything stays on the device
        gtb = gt_boxes(full_masks, raw)
        gt_recs = []
        for b in range(B):
            lab = self._map(inst[b].to(torch.int64).reshape(-1))
            if lab.shape[0] != gtb[b]["boxes"].shape[0]:
                raise ValueError(f"scene {b}: {lab.shape[0]} instance_labels but {gtb[b]['boxes'].shape[0]} full_masks rows")
            gt_recs.append(dict(boxes=gtb[b]["boxes"], labels=lab, valid=gtb[b]["valid"] & (lab != self.ignore_label)))
        pred_recs = [dict(boxes=r["boxes"], classes=c, scores=r["scores"], box_valid=r["box_valid"]) for r, c in zip(recs, classes)]
        m = box_match(pred_recs, gt_recs)
        for b in range(B):
            a, e = int(m["koff"][b]), int(m["koff"][b + 1])
            self._pending[scan_ids[b]] = (classes[b], recs[b]["scores"], pred_recs[b]["box_valid"], m["flags"][a:e],
                                          gt_recs[b]["labels"], gt_recs[b]["valid"], m["err"])
        self.total_count += int(logits.shape[1])

    # -- device records -> host ---------------------------------------------------------------------------------------------
    def _flush(self) -> None:
        """The one device-to-host copy of the box records kept since the last flush."""
        if not self._pending:
            return
        parts, layout = [], []
        for key, rec in self._pending.items():
            sizes = []
            for t in rec:
                t = t.contiguous()
                t = t.view(torch.uint8) if t.dtype != torch.uint8 else t
                parts.append(t.reshape(-1))
                sizes.append(int(t.numel()))
            layout.append((key, sizes))
        host = torch.cat(parts).cpu().numpy()
        o = 0
        for key, sizes in layout:
            f = []
            for n, dt in zip(sizes, (np.int64, np.float32, np.uint8, np.uint8, np.int64, np.uint8, np.int32)):
                f.append(host[o:o + n].copy().view(dt))
                o += n
            classes, scores, valid, flags, glab, gvalid, err = f
            check_errors(int(err[0]), f"InstSegEval: scene {key!r}")
            v = valid != 0
            self.box_ap.add(key, classes[v], scores[v], flags[v], glab[gvalid != 0])
        self._pending = {}

    def records(self) -> Tuple[List[tuple], List[tuple]]:
        """(mask AP records, box AP records): plain picklable tuples of numpy arrays, for ``extend`` in another process."""
        self._flush()
        return self.mask_ap.records(), self.box_ap.records()

    def extend(self, records) -> None:
        self._flush()
        mask_records, box_records = records
        self.mask_ap.extend(mask_records)
        self.box_ap.extend(box_records)

    def gather(self, *_a, **_k):
        raise NotImplementedError("InstSegEval: gathering across ranks is not covered; move records() with extend()")

    def reset(self) -> None:
        self.total_count = 0

    # -- record -------------------------------------------------------------------------------------------------------------------
    def _name(self, class_id: int) -> str:
        return str(class_id) if self.class_names is None else self.class_names[class_id]

    def record(self):
        self._flush()
        (ap25, ap50), (mean25, mean50) = self.box_ap.compute()
        res: Dict[str, object] = {"mean_box_ap_25": mean25, "mean_box_ap_50": mean50}
        for c, v in ap50.items():
            res[f"{self._name(c)}_val_box_ap_50"] = v
        for c, v in ap25.items():
            res[f"{self._name(c)}_val_box_ap_25"] = v
        _ap, avgs = self.mask_ap.compute()
        res.update(avgs)
        if self.groups is not None:
            rows = {"head": [], "common": [], "tail": []}
            for name in self.group_order:
                if name not in res["classes"]:
                    continue
                c = res["classes"][name]
                row = np.array((float(c["ap"]), float(c["ap50%"]), float(c["ap25%"])))
                for g in ("head", "common", "tail"):
                    if name in self.groups[g]:
                        rows[g].append(row)
                        break
            arr = {g: np.stack(v) if v else np.full((0, 3), np.nan) for g, v in rows.items()}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                means = {g: np.nanmean(arr[g], axis=0) for g in ("tail", "common", "head")}
                for i, suffix in enumerate(("ap", "ap_50", "ap_25")):      # the reference's key order
                    for g in ("tail", "common", "head"):
                        res[f"mean_{g}_{suffix}"] = means[g][i]
                o = np.nanmean(np.vstack((arr["head"], arr["common"], arr["tail"])), axis=0)
            res["mean_ap"], res["mean_ap_50"], res["mean_ap_25"] = o[0], o[1], o[2]
        if self.target_metric not in res:
            raise KeyError(f"target_metric {self.target_metric!r} is not among the results")
        is_best = bool(res[self.target_metric] > self.best_result)
        if is_best:
            self.best_result = res[self.target_metric]
        self.mask_ap._scenes = {}
        self.box_ap._scenes = {}
        res["target_metric"] = res[self.target_metric]
        res["best_result"] = self.best_result
        return is_best, res
