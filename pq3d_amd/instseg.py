"""Instance-segmentation predictions from the mask head's outputs, on the GPU (csrc/instseg.hip).

The reference builds them in InstSegEval.eval_instance_step (evaluator/instseg_eval.py:85-149) on the host, one scene and one
query at a time.  ``instance_predictions`` computes the same per-scene records for a whole batch of ragged scenes in a fixed
number of launches (independent of the batch size), with one device-to-host read (the range check of the index maps).

Semantics (use_dbscan = False, filter_out_no_object_queries = False), per scene b with K = topk_per_scene (Q when -1):
  1. prob = softmax(pred_logits[b]) over the C+1 classes in fp32, last column (no object) dropped: [Q, C].
  2. The K largest entries of prob.flatten(), descending; ties go to the LOWER flat index (torch.topk leaves this
     unspecified).  query = idx // C, class = idx % C; a query can be selected with several classes.
  3. score = prob * sum_v sigmoid(m) [m > 0] / (sum_v [m > 0] + 1e-6) over the scene's voxels v, m = pred_masks[b][s(v), query]
     (summed over segments, weighted by their voxel counts).
  4. mask[p] = 2 * sum > count of [m > 0] at s1 = voxel2segment[voxel_to_full_maps[p]] over the points of p's full-resolution
     segment segment_to_full_maps[p]: the reference's scatter_mean(...) > 0.5 without a division.
  5. Columns sorted by score, descending; ties by top-k rank.
  6. Boxes over the points of each mask: center = mean, extent = max - min of raw_coordinates; box_valid = mask not empty
     (the reference leaves such boxes out of bbox_preds but keeps the mask in preds).
Classes are the C-class ids, before any dataset label mapping.  Results are bit-identical run to run.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch

from . import _lib as L
from .ops import SegmentPlan
from .profiler import timed

SEG_CHUNK = 64           # PQ3D_INSTSEG_SEG_CHUNK
PT_CHUNK = 256           # PQ3D_INSTSEG_PT_CHUNK
MAX_K = 1024             # PQ3D_INSTSEG_MAX_K
BOX_PART_BYTES = 64      # PQ3D_INSTSEG_BOX_PART_BYTES
_ERRORS = {1: "voxel2segment holds ids outside [0, S)",
           2: "voxel_to_full_maps holds ids outside [0, number of voxels of the scene)",
           4: "segment_to_full_maps holds negative ids"}


def _cat(ts: Sequence[torch.Tensor], dtype, what: str, dev) -> torch.Tensor:
    for t in ts:
        if t.dtype != dtype or t.device != dev:
            raise ValueError(f"{what}: expected {dtype} tensors on {dev}, got {t.dtype} on {t.device}")
    return torch.cat([t.reshape(-1) if t.dim() == 1 else t for t in ts]).contiguous()


def instance_predictions(pred_logits: torch.Tensor, pred_masks: torch.Tensor, voxel2segment: Sequence[torch.Tensor],
                         voxel_to_full_maps: Sequence[torch.Tensor], segment_to_full_maps: Sequence[torch.Tensor],
                         raw_coordinates: Sequence[torch.Tensor], topk_per_scene: int = 100) -> List[Dict[str, torch.Tensor]]:
    """Per-scene instance predictions of ``pred_logits`` [B, Q, C+1] (predictions_class[-1]) and ``pred_masks`` [B, S, Q]
    (predictions_mask[-1]), both fp32 on the device.  The index maps and coordinates are per-scene lists of device tensors:
    ``voxel2segment[b]`` [V_b] int64 (segment of each voxel), ``voxel_to_full_maps[b]`` [P_b] int64 (voxel of each point),
    ``segment_to_full_maps[b]`` [P_b] int64 (full-resolution segment of each point), ``raw_coordinates[b]`` [P_b, 3] fp32.

    Returns one dict per scene: ``masks`` [P_b, K] bool (views into one buffer), ``scores`` [K] fp32, ``classes`` [K] int64,
    ``boxes`` [K, 6] fp32 (center xyz, extent xyz; zeros where the mask is empty) and ``box_valid`` [K] bool, all sorted by
    score.  Index values outside their tables raise ValueError."""
    if pred_logits.dim() != 3 or pred_masks.dim() != 3:
        raise ValueError("pred_logits must be [B, Q, C+1] and pred_masks [B, S, Q]")
    assert pred_logits.dtype == torch.float32 and pred_masks.dtype == torch.float32, \
        "the mask head returns fp32 class and mask logits in every compute mode"
    dev = pred_logits.device
    if not pred_logits.is_cuda or pred_masks.device != dev:
        raise L.Pq3dError("instance_predictions needs device tensors on one device (no CPU fallback)")
    B, Q, C1 = pred_logits.shape
    S = pred_masks.shape[1]
    if pred_masks.shape[0] != B or pred_masks.shape[2] != Q:
        raise ValueError(f"pred_masks {tuple(pred_masks.shape)} does not match pred_logits {tuple(pred_logits.shape)}")
    if not (len(voxel2segment) == len(voxel_to_full_maps) == len(segment_to_full_maps) == len(raw_coordinates) == B):
        raise ValueError("one voxel2segment / voxel_to_full_maps / segment_to_full_maps / raw_coordinates entry per scene")
    if B < 1 or S < 1 or C1 < 2:
        raise ValueError("need B >= 1, S >= 1 and C+1 >= 2")
    C_ = C1 - 1
    K = Q if int(topk_per_scene) == -1 else int(topk_per_scene)
    if not 1 <= K <= min(MAX_K, Q * C_):
        raise ValueError(f"topk_per_scene must be -1 or in [1, min({MAX_K}, Q*C = {Q * C_})], got {topk_per_scene}")
    V = [int(t.numel()) for t in voxel2segment]
    P = [int(t.numel()) for t in voxel_to_full_maps]
    for b in range(B):
        if int(segment_to_full_maps[b].numel()) != P[b] or tuple(raw_coordinates[b].shape) != (P[b], 3):
            raise ValueError(f"scene {b}: segment_to_full_maps [P] and raw_coordinates [P, 3] must match "
                             f"voxel_to_full_maps (P = {P[b]})")
    v2s = _cat(voxel2segment, torch.int64, "voxel2segment", dev)
    v2f = _cat(voxel_to_full_maps, torch.int64, "voxel_to_full_maps", dev)
    s2f = _cat(segment_to_full_maps, torch.int64, "segment_to_full_maps", dev)
    xyz = _cat(raw_coordinates, torch.float32, "raw_coordinates", dev)
    NV, NP = sum(V), sum(P)
    chunks = [(p + PT_CHUNK - 1) // PT_CHUNK for p in P]
    offs_h = [0]
    for v in V:
        offs_h.append(offs_h[-1] + v)
    offs_h.append(0)
    for p in P:
        offs_h.append(offs_h[-1] + p)
    offs_h.append(0)
    for c in chunks:
        offs_h.append(offs_h[-1] + c)
    n_chunks = offs_h[-1]
    offs = torch.tensor(offs_h, dtype=torch.int64).to(dev)
    logits, masks_in = pred_logits.contiguous(), pred_masks.contiguous()
    lib, st = L.lib(), L.stream()
    i32 = dict(dtype=torch.int32, device=dev)

    # 1. range checks + voxels per segment (read back below, after the launches that do not depend on it)
    nvox = torch.empty(B * S, **i32)
    stats = torch.empty(2, dtype=torch.int64, device=dev)
    L.check(timed("pq3d_instseg_check", f"B{B}V{NV}P{NP}", 0.0, NV * 8.0 + NP * 16.0 + B * S * 4.0,
                  lib.pq3d_instseg_check, L.ptr(v2s), L.ptr(v2f), L.ptr(s2f), L.ptr(offs), B, S, NV, NP, L.ptr(nvox),
                  L.ptr(stats), st), "pq3d_instseg_check")
    # 2. softmax + top-K
    prob = torch.empty(B, Q * C_, dtype=torch.float32, device=dev)
    sel_prob = torch.empty(B, K, dtype=torch.float32, device=dev)
    sel_query, sel_class = torch.empty(B, K, **i32), torch.empty(B, K, **i32)
    L.check(timed("pq3d_instseg_topk", f"B{B}Q{Q}C{C1}K{K}", 0.0, B * Q * C1 * 4.0 + B * K * 12.0,
                  lib.pq3d_instseg_topk, L.ptr(logits), B, Q, C1, K, L.ptr(prob), L.ptr(sel_prob), L.ptr(sel_query),
                  L.ptr(sel_class), st), "pq3d_instseg_topk")
    # 3. bit table [B*S, K] (top-k order) + mask scores, sorted by score
    nsc = (S + SEG_CHUNK - 1) // SEG_CHUNK
    table = torch.empty(B * S, K, dtype=torch.float32, device=dev)
    ws = torch.empty(B * nsc * K * 16, dtype=torch.uint8, device=dev)
    scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    classes = torch.empty(B, K, dtype=torch.int64, device=dev)
    order = torch.empty(B, K, **i32)
    L.check(timed("pq3d_instseg_scores", f"B{B}S{S}Q{Q}K{K}", 0.0, B * S * (K * 8.0 + 4.0) + B * K * 24.0,
                  lib.pq3d_instseg_scores, L.ptr(masks_in), L.ptr(nvox), L.ptr(sel_prob), L.ptr(sel_query),
                  L.ptr(sel_class), B, S, Q, K, L.ptr(table), L.ptr(ws), ws.numel(), L.ptr(scores), L.ptr(classes),
                  L.ptr(order), st), "pq3d_instseg_scores")

    err, sf = (int(x) for x in stats.cpu().tolist())        # the one device-to-host read of the call
    if err:
        raise ValueError("instance_predictions: " + "; ".join(m for bit, m in _ERRORS.items() if err & bit))
    Sf = max(sf, 1)
    if B * Sf >= (1 << 31) - 65536:
        raise ValueError(f"segment_to_full_maps ids too large for a batched grouping (B * (max id + 1) = {B * Sf})")

    # 4. vote per full-resolution segment: rows voxel2segment[voxel_to_full_maps[p]] of the table, grouped by segment_to_full_maps
    gather = torch.empty(NP, dtype=torch.int64, device=dev)
    key = torch.empty(NP, dtype=torch.int64, device=dev)
    L.check(timed("pq3d_instseg_compose", f"B{B}P{NP}", 0.0, NP * 40.0, lib.pq3d_instseg_compose, L.ptr(v2s), L.ptr(v2f),
                  L.ptr(s2f), L.ptr(offs), B, S, Sf, NP, L.ptr(gather), L.ptr(key), st), "pq3d_instseg_compose")
    out = torch.empty(NP, K, dtype=torch.bool, device=dev)
    if NP > 0:
        plan = SegmentPlan(key, B * Sf)
        vsum, vcount = plan.reduce(table, gather, None, K, False)
        bws = torch.empty(n_chunks * K * BOX_PART_BYTES, dtype=torch.uint8, device=dev)
    else:
        vsum = vcount = bws = None
    # 5. masks in sorted column order + boxes
    boxes = torch.empty(B, K, 6, dtype=torch.float32, device=dev)
    valid = torch.empty(B, K, dtype=torch.bool, device=dev)
    L.check(timed("pq3d_instseg_expand", f"B{B}P{NP}K{K}", 0.0, NP * (K * 5.0 + 20.0) + n_chunks * K * BOX_PART_BYTES,
                  lib.pq3d_instseg_expand, L.ptr(vsum), L.ptr(vcount), L.ptr(key), L.ptr(xyz), L.ptr(offs), L.ptr(order), B,
                  NP, n_chunks, K, L.ptr(out), L.ptr(bws), 0 if bws is None else bws.numel(), L.ptr(boxes), L.ptr(valid), st),
            "pq3d_instseg_expand")
    res = []
    p0 = offs_h[B + 1]
    for b in range(B):
        res.append(dict(masks=out[p0:p0 + P[b]], scores=scores[b], classes=classes[b], boxes=boxes[b], box_valid=valid[b]))
        p0 += P[b]
    return res
