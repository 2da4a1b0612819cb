"""Grounding (stage-2) batches prepared on the GPU (csrc/object_prep.hip): from scans held in device memory to the
dict ``Query3DUnified`` reads with ``memories: [mv, pc, voxel, prompt]`` and ``heads: [ground, generation]``.

The reference builds this per sample on the host (data/datasets/sceneverse_base.py): ``_load_one_scan`` makes the per-object
point lists, ``convert_pc_to_box`` and ``match_gt_to_pred``; ``get_scene`` draws ``np.random.choice`` of 1024 points per
object and runs ``_obj_processing_post``; the dataset wrapper makes the 0-1 label rows and pads.  At the shipped batch
(128 samples x 80 objects x 1024 points x 6 fp32) ``obj_fts`` alone is about 250 MB per step, a gather from scans that fit
in HBM many times over.  Here:

  build_object_bank        once per scan set (may synchronise): per-object CSR of point indices, boxes
  match_boxes              match_gt_to_pred of one scan's GT and predicted boxes
  sample_objects           the hot path: one launch, no device-to-host read, capturable, a new draw per replay
  ground_labels            the 0-1 rows tgt_object_id, tgt_object_id_iou25, tgt_object_id_iou50
  prepare_grounding_batch  the whole dict

The rules are restated in tests/object_prep_ref.py, which is the specification; the kernels equal it bit for bit.  Which
objects an item shows (``keep_obj``, the ``max_obj_len`` crop, the language filter) stays with the caller: ``selected`` holds
the chosen objects as indices local to the item's scan in the bank (0 .. ``bank.num_objects[scan]`` - 1), -1 = padded slot.
numpy's random stream is not reproduced: the draws follow a counter-based rule keyed by (seed, item, slot)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

MAX_POINTS, MAX_ROWS = L.H.PQ3D_OBJECT_MAX_POINTS, L.H.PQ3D_OBJECT_MAX_ROWS       # points / object rows per scan
CHUNK, MAX_SAMPLE = L.H.PQ3D_OBJECT_CHUNK, L.H.PQ3D_OBJECT_MAX_SAMPLE
_ERRORS = {1: "scene_of_item holds a scan index outside the bank",
           2: "selected holds an object index outside [-1, objects of the item's scan)",
           4: "a sampling cycle walk hit its iteration cap",
           8: "targets holds an object index outside [-1, GT objects of the item's scan)",
           16: "the object bank's tables are inconsistent"}


def _dev(who: str, *ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise L.Pq3dError(f"{who}: needs device tensors (no CPU fallback)")


def _i64(vals, dev) -> torch.Tensor:
    return torch.tensor(np.asarray(vals, dtype=np.int64), dtype=torch.int64, device=dev)


@dataclass
class ObjectBank:
    """The objects of S scans: ``order[entry_offsets[o] : entry_offsets[o + 1]]`` are the points of object o (indices local
    to its scan, ascending); the objects of scan s are ``object_offsets[s] : object_offsets[s + 1]``.  ``source_row[o]``: the
    row of the scan's ``instance_ids`` / ``masks`` object o came from (rows that select no point are dropped)."""
    points: torch.Tensor             # [P, 6] fp32
    point_offsets: torch.Tensor      # [S + 1] int64
    object_offsets: torch.Tensor     # [S + 1] int32
    entry_offsets: torch.Tensor      # [O + 1] int64
    order: torch.Tensor              # [E] int32
    source_row: torch.Tensor         # [O] int32
    object_scan: torch.Tensor        # [O] int32
    box_center: torch.Tensor         # [O, 3] fp32
    box_size: torch.Tensor           # [O, 3] fp32
    num_points: List[int]            # per scan (host)
    num_objects: List[int]           # per scan (host)

    @property
    def num_scans(self) -> int:
        return len(self.num_points)

    def scan_objects(self, s: int) -> slice:
        o0 = sum(self.num_objects[:s])
        return slice(o0, o0 + self.num_objects[s])


def build_object_bank(points: Sequence[torch.Tensor], *, point2instance: Optional[Sequence[torch.Tensor]] = None,
                      instance_ids: Optional[Sequence[torch.Tensor]] = None,
                      masks: Optional[Sequence[torch.Tensor]] = None) -> ObjectBank:
    """Per-scan lists of device tensors: ``points`` [P_s, 6] fp32 (xyz | rgb) and either ``point2instance`` [P_s] int64 with
    ``instance_ids`` [O_s] int64 (object o = the points with ``id == instance_ids[o]``) or ``masks`` [K_s, P_s] bool (rows may
    overlap).  Any number of scans; at most 2^20 points and 1024 object rows per scan.  Runs once per scan set and reads
    the row sizes back (two host synchronisations)."""
    who = "build_object_bank"
    ids_form = masks is None
    if ids_form == (point2instance is None) or ids_form != (instance_ids is not None) or len(points) < 1:
        raise ValueError(f"{who}: pass at least one scan and either point2instance with instance_ids, or masks")
    sel = [point2instance, instance_ids] if ids_form else [masks]
    if any(len(x) != len(points) for x in sel):
        raise ValueError(f"{who}: one entry per scan in every list")
    _dev(who, *points, *[t for x in sel for t in x])
    S, dev = len(points), points[0].device
    P, rows = [int(p.shape[0]) for p in points], []
    for s in range(S):
        if points[s].dtype != torch.float32 or points[s].dim() != 2 or points[s].shape[1] != 6 or P[s] < 1:
            raise ValueError(f"{who}: points[{s}] must be a non-empty [P, 6] fp32 tensor")
        if P[s] > MAX_POINTS:
            raise ValueError(f"{who}: at most {MAX_POINTS} points per scan, scan {s} has {P[s]}")
        if ids_form:
            ok = point2instance[s].dtype == torch.int64 and tuple(point2instance[s].shape) == (P[s],) and \
                instance_ids[s].dtype == torch.int64 and instance_ids[s].dim() == 1
            rows.append(int(instance_ids[s].shape[0]) if ok else -1)
        else:
            ok = masks[s].dtype == torch.bool and masks[s].dim() == 2 and masks[s].shape[1] == P[s]
            rows.append(int(masks[s].shape[0]) if ok else -1)
        if not ok:
            raise ValueError(f"{who}: scan {s} needs point2instance [P] int64 with instance_ids [O] int64, or masks [K, P] bool")
        if rows[s] > MAX_ROWS:
            raise ValueError(f"{who}: at most {MAX_ROWS} object rows per scan, scan {s} has {rows[s]}")
    pts = torch.cat([p.contiguous() for p in points], 0) if S > 1 else points[0].contiguous()
    pt_off, row_off = np.cumsum([0] + P), np.cumsum([0] + rows)
    R = int(row_off[-1])
    chunks = [(p + CHUNK - 1) // CHUNK for p in P]
    cell_off = np.cumsum([0] + [chunks[s] for s in range(S) for _ in range(rows[s])])
    row_scan = torch.tensor(np.repeat(np.arange(S), rows), dtype=torch.int64, device=dev)
    d_pt, d_row, d_cell = _i64(pt_off, dev), _i64(row_off, dev), _i64(cell_off, dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    if R == 0:
        kept = torch.empty(0, dtype=torch.int64, device=dev)
        order, entry = i32(0), torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        if ids_form:
            form = (torch.cat(list(point2instance)).contiguous(), torch.cat(list(instance_ids)).contiguous(), None, None)
        else:
            flat = torch.cat([m.contiguous().view(torch.uint8).reshape(-1) for m in masks])
            form = (None, None, flat, _i64(np.cumsum([0] + [r * p for r, p in zip(rows, P)]), dev))
        cells = int(cell_off[-1])
        cnt, cbase, total = i32(cells), i32(cells), i32(R)
        L.call("pq3d_object_count", d_pt, d_row, d_cell, *form, S, R, cells, cnt, cbase, total)
        row_entry = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(total.long(), 0)])
        E = int(row_entry[-1])                                         # (host sync: outside any graph)
        order = i32(E)
        if E:
            L.call("pq3d_object_emit", d_pt, d_row, d_cell, *form, S, R, cells, cbase, row_entry, E, order)
        kept = torch.nonzero(total > 0)[:, 0]
        entry = torch.cat([row_entry[kept], row_entry[-1:]])
    scan = row_scan[kept]
    n_obj = torch.bincount(scan, minlength=S)
    obj_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(n_obj, 0)]).int()
    O = int(kept.shape[0])
    center, size = torch.empty(O, 3, dtype=torch.float32, device=dev), torch.empty(O, 3, dtype=torch.float32, device=dev)
    scan32 = scan.int()
    if O:
        L.call("pq3d_object_boxes", pts, d_pt, obj_off, entry, order, S, scan32, O, center, size)
    return ObjectBank(pts, d_pt, obj_off, entry, order, (kept - d_row[scan]).int(), scan32, center, size, P, n_obj.tolist())


def match_boxes(gt_center: torch.Tensor, gt_size: torch.Tensor, pred_center: torch.Tensor, pred_size: torch.Tensor):
    """``match_gt_to_pred`` of one scan: [G, 3] fp32 GT and [K, 3] fp32 predicted boxes (centre, size).  Returns ``matched``
    [G] int32 (the first index of the strictly largest IoU, -1 when K = 0) and ``iou25`` / ``iou50`` [G, K] uint8.  The IoU
    is box3d_iou's formula with its ``+ 1e-8``, in fp64."""
    who = "match_boxes"
    _dev(who, gt_center, gt_size, pred_center, pred_size)
    for a, b in ((gt_center, gt_size), (pred_center, pred_size)):
        if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3 or a.shape != b.shape:
            raise ValueError(f"{who}: centres and sizes are [N, 3] fp32 tensors of equal shape")
    G, K, dev = int(gt_center.shape[0]), int(pred_center.shape[0]), gt_center.device
    matched = torch.full((G,), -1, dtype=torch.int32, device=dev)
    i25, i50 = torch.zeros(G, K, dtype=torch.uint8, device=dev), torch.zeros(G, K, dtype=torch.uint8, device=dev)
    if G and K:
        L.call("pq3d_match_boxes", gt_center.contiguous(), gt_size.contiguous(), pred_center.contiguous(), pred_size.contiguous(),
               G, K, matched, i25, i50)
    return matched, i25, i50


@dataclass
class MatchTables:
    """``match_boxes`` of every scan of a GT bank against the same scan of a predicted bank, concatenated for
    ``ground_labels``: ``gt_offsets`` [S + 1] int32 into ``matched``, ``table_offsets`` [S + 1] int64 into the flat tables."""
    matched: torch.Tensor
    iou25: torch.Tensor
    iou50: torch.Tensor
    gt_offsets: torch.Tensor
    table_offsets: torch.Tensor
    num_gt: List[int]
    num_pred: List[int]


def match_banks(gt: ObjectBank, pred: ObjectBank) -> MatchTables:
    """The match tables of two banks over the same scans (``_load_one_scan``'s ``match_gt_to_pred`` per scan)."""
    if gt.num_scans != pred.num_scans:
        raise ValueError("match_banks: the banks hold different numbers of scans")
    dev, ms, a, b = gt.points.device, [], [], []
    for s in range(gt.num_scans):
        g, p = gt.scan_objects(s), pred.scan_objects(s)
        m, x, y = match_boxes(gt.box_center[g], gt.box_size[g], pred.box_center[p], pred.box_size[p])
        ms.append(m); a.append(x.reshape(-1)); b.append(y.reshape(-1))
    tab = np.cumsum([0] + [g * k for g, k in zip(gt.num_objects, pred.num_objects)])
    pad = torch.zeros(1, dtype=torch.uint8, device=dev)               # (never read: keeps the pointers non-null)
    return MatchTables(torch.cat(ms + [torch.full((1,), -1, dtype=torch.int32, device=dev)]), torch.cat(a + [pad]), torch.cat(b + [pad]),
                       gt.object_offsets, _i64(tab, dev), list(gt.num_objects), list(pred.num_objects))


def _batch_args(who: str, bank: ObjectBank, scene_of_item: torch.Tensor, selected: torch.Tensor) -> Tuple[int, int]:
    _dev(who, scene_of_item, selected)
    if selected.dtype != torch.int32 or selected.dim() != 2 or not selected.is_contiguous() or selected.shape[1] < 1:
        raise ValueError(f"{who}: selected must be a contiguous [B, O_max] int32 tensor")
    B = int(selected.shape[0])
    if scene_of_item.dtype != torch.int32 or tuple(scene_of_item.shape) != (B,) or B < 1 or not scene_of_item.is_contiguous():
        raise ValueError(f"{who}: scene_of_item must be a contiguous [B] int32 tensor, B >= 1")
    if bank.order.numel() < 1:
        raise ValueError(f"{who}: the bank holds no object")
    return B, int(selected.shape[1])


def sample_objects(bank: ObjectBank, scene_of_item: torch.Tensor, selected: torch.Tensor, *, num_points: int = 1024,
                   seed: torch.Tensor, rotation: Optional[torch.Tensor] = None):
    """``get_scene``'s point subsampling and ``_obj_processing_post`` for a batch, one launch of one workgroup per
    (item, slot).  ``scene_of_item`` [B] int32: the item's scan in the bank; ``selected`` [B, O_max] int32: its objects
    (scan-local indices, -1 = padded); ``seed``: 1-element int64 device tensor, read by the kernel (bump it between
    replays of a captured graph for a new draw); ``rotation``: optional [B, 3, 3] fp32, xyz' = xyz (row vector) x rotation.

    Returns ``(dict(obj_fts [B, O_max, num_points, 6], obj_locs, obj_boxes [B, O_max, 6], obj_pad_masks [B, O_max] bool), err)``;
    ``err`` is a device int32 word for ``check_objects``.  An object of n >= num_points points is sampled without
    replacement, a smaller one with replacement.  No device-to-host read."""
    who = "sample_objects"
    B, O = _batch_args(who, bank, scene_of_item, selected)
    _dev(who, seed, rotation)
    num_points = int(num_points)
    if not 1 <= num_points <= MAX_SAMPLE:
        raise ValueError(f"{who}: need 1 <= num_points <= {MAX_SAMPLE}, got {num_points}")
    if seed.dtype != torch.int64 or seed.numel() != 1:
        raise ValueError(f"{who}: seed must be a 1-element int64 device tensor")
    if rotation is not None and (rotation.dtype != torch.float32 or tuple(rotation.shape) != (B, 3, 3) or not rotation.is_contiguous()):
        raise ValueError(f"{who}: rotation must be a contiguous [B, 3, 3] fp32 tensor")
    dev = selected.device
    fts = torch.empty(B, O, num_points, 6, dtype=torch.float32, device=dev)
    locs = torch.empty(2, B, O, 6, dtype=torch.float32, device=dev)
    pad = torch.empty(B, O, dtype=torch.bool, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    L.call("pq3d_object_sample", bank.points, bank.point_offsets, bank.object_offsets, bank.entry_offsets, bank.order, bank.num_scans,
           scene_of_item, selected, B, O, num_points, seed, rotation, fts, locs[0], locs[1], pad, err)
    return dict(obj_fts=fts, obj_locs=locs[0], obj_boxes=locs[1], obj_pad_masks=pad), err


def check_objects(err: torch.Tensor, who: str = "sample_objects") -> None:
    """Read the error word(s) of ``sample_objects`` / ``ground_labels`` / ``prepare_grounding_batch`` (a host sync) and raise
    ValueError with the text of the bits, prefixed with the entry point's name ``who``."""
    word = 0
    for w in err.reshape(-1).tolist():
        word |= int(w)
    L.raise_error_word(who, word, _ERRORS)


def ground_labels(bank: ObjectBank, scene_of_item: torch.Tensor, selected: torch.Tensor, targets: torch.Tensor, *,
                  match: Optional[MatchTables] = None):
    """The 0-1 rows ``tgt_object_id``, ``tgt_object_id_iou25``, ``tgt_object_id_iou50`` [B, O_max] fp32 (``make_bce_label``
    of get_scene's target lists) and the error word.  ``targets`` [B, T_max] int32: the item's target objects, -1 padded.

    ``pc_type='gt'`` (``match`` None): ``bank`` is the GT bank, ``selected`` and ``targets`` index it; all three rows mark the
    slots that hold a target.  ``pc_type='pred'``: ``bank`` is the predicted bank ``selected`` indexes, ``targets`` index the
    GT objects of ``match`` (``match_banks(gt_bank, bank)``): ``tgt_object_id`` marks the slots holding ``matched[t]``, the
    other two the slots whose prediction has IoU >= 0.25 / 0.5 with a target.  A target whose matched prediction is not among
    ``selected`` marks no slot (the reference's ``list.index`` would raise; the selection is the caller's here)."""
    who = "ground_labels"
    B, O = _batch_args(who, bank, scene_of_item, selected)
    _dev(who, targets)
    if targets.dtype != torch.int32 or targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] < 1 or not targets.is_contiguous():
        raise ValueError(f"{who}: targets must be a contiguous [B, T_max] int32 tensor")
    if match is not None and match.num_pred != list(bank.num_objects):
        raise ValueError(f"{who}: match was not built against this bank (match_banks(gt_bank, bank))")
    dev = selected.device
    out = torch.empty(3, B, O, dtype=torch.float32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    m = (None,) * 5 if match is None else (match.matched, match.iou25, match.iou50, match.gt_offsets, match.table_offsets)
    L.call("pq3d_ground_labels", bank.object_offsets, bank.num_scans, scene_of_item, selected, targets, B, O, int(targets.shape[1]), *m,
           out, err)
    return out[0], out[1], out[2], err


def gather_object_rows(bank: ObjectBank, table: torch.Tensor, scene_of_item: torch.Tensor, selected: torch.Tensor) -> torch.Tensor:
    """[B, O_max, D] rows of an offline per-object feature ``table`` [objects of the bank, D] fp32 (in the bank's object
    order: ``bank.source_row`` tells which input rows were kept), zeros for padded slots."""
    who = "gather_object_rows"
    B, O = _batch_args(who, bank, scene_of_item, selected)
    _dev(who, table)
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] != sum(bank.num_objects) or table.shape[1] < 1:
        raise ValueError(f"{who}: table must be [objects of the bank, D] fp32")
    out = torch.empty(B, O, table.shape[1], dtype=torch.float32, device=selected.device)
    L.call("pq3d_object_rows", table.contiguous(), int(table.shape[1]), bank.object_offsets, bank.num_scans, scene_of_item, selected, B, O,
           out)
    return out


def prepare_grounding_batch(bank: ObjectBank, scene_of_item: torch.Tensor, selected: torch.Tensor, targets: torch.Tensor, *,
                            num_points: int = 1024, seed: torch.Tensor, rotation: Optional[torch.Tensor] = None,
                            match: Optional[MatchTables] = None, mv_table: Optional[torch.Tensor] = None,
                            voxel_table: Optional[torch.Tensor] = None) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """The scene side of a stage-2 batch as ``Query3DUnified`` reads it (get_scene's data_dict after the wrapper's label rows
    and padding): ``obj_fts`` = ``pc_seg_fts``, ``obj_locs`` = ``query_locs`` = ``seg_center``, ``obj_boxes``, the pad masks of
    every memory (one tensor: every slot is an object in all of them), ``coord_min`` / ``coord_max`` [B, 3] over the valid
    slots, the three label rows and, when the offline tables are given, ``mv_seg_fts`` / ``voxel_seg_fts``.  Returns
    ``(dict, err)``; ``err`` [2] int32 for ``check_objects``.  No device-to-host read; the prompt side (tokens, response) is
    the caller's."""
    d, e0 = sample_objects(bank, scene_of_item, selected, num_points=num_points, seed=seed, rotation=rotation)
    t0, t25, t50, e1 = ground_labels(bank, scene_of_item, selected, targets, match=match)
    B, O = selected.shape
    rng = torch.empty(2, B, 3, dtype=torch.float32, device=selected.device)
    L.call("pq3d_object_range", d["obj_locs"], d["obj_pad_masks"], B, O, rng[0], rng[1])
    pad = d["obj_pad_masks"]
    d.update(pc_seg_fts=d["obj_fts"], pc_seg_pad_masks=pad, mv_seg_pad_masks=pad, voxel_seg_pad_masks=pad, seg_pad_masks=pad,
             query_pad_masks=pad, query_locs=d["obj_locs"], seg_center=d["obj_locs"], coord_min=rng[0], coord_max=rng[1],
             tgt_object_id=t0, tgt_object_id_iou25=t25, tgt_object_id_iou50=t50)
    if mv_table is not None:
        d["mv_seg_fts"] = gather_object_rows(bank, mv_table, scene_of_item, selected)
    if voxel_table is not None:
        d["voxel_seg_fts"] = gather_object_rows(bank, voxel_table, scene_of_item, selected)
    return d, torch.cat([e0, e1])
