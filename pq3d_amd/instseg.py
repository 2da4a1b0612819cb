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

filter_out_no_object_queries / use_dbscan (instseg_eval.py:104-116, 245-270; csrc/instseg_dbscan.hip), per scene:
  F. Filter: keep the queries whose argmax over the C+1 probabilities (ties: lower index, as torch.argmax) is not C, in
     query order, with their C class probabilities (the no-object column dropped).  The reference compares with the literal
     200, which is "not C" for the shipped C = 200.
  D. DBSCAN (min_samples = 1 only, so every point is a core point): kept query q's voxels M_q = {v : m(v, q) > 0} split into
     the connected components of "((dx*dx + dy*dy) + dz*dz) <= eps*eps", evaluated in fp64 on the fp32 voxel coordinates in
     exactly this order without contraction.  Each component is one column with q's class probabilities; its mask is q's
     logits inside the component and 0 elsewhere.  Columns are ordered by q, then by the component's smallest voxel index
     (sklearn's label order); a query with an empty M_q gives no column.  The partition is unique, so the columns are
     deterministic whatever order the kernels join them in.
  Top-k then runs over the Q'_b columns: K_b = min(K, Q'_b * C) (topk_per_scene = -1: K_b = Q'_b), flat index = column * C
  + class, ties to the lower flat index.  The reference raises on K > Q'_b * C and on a scene without columns; here those
  give a short record or an empty one (masks [P_b, 0]), so K_b may differ from scene to scene.  With DBSCAN the mask score
  is a voxel-level sum (a component can cut a segment in two) and the vote rows are voxel-level: voxel_to_full_maps[p]
  instead of voxel2segment[voxel_to_full_maps[p]].  The cell grid of a DBSCAN call (cells of side eps / sqrt(3) per scene)
  is limited to 2^24 cells over the batch.  A DBSCAN call makes two device-to-host reads (index checks + coordinate bounds,
  then the column counts); the filter alone keeps the one read.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .ops import SegmentPlan

SEG_CHUNK, PT_CHUNK, MAX_K = L.H.PQ3D_INSTSEG_SEG_CHUNK, L.H.PQ3D_INSTSEG_PT_CHUNK, L.H.PQ3D_INSTSEG_MAX_K
BOX_PART_BYTES, GRID_WORDS = L.H.PQ3D_INSTSEG_BOX_PART_BYTES, L.H.PQ3D_DBSCAN_GRID_WORDS
MAX_CELLS = L.H.PQ3D_DBSCAN_MAX_CELLS      # cells of a DBSCAN call's grid over the batch (24-bit cell keys)
_ERRORS = {1: "voxel2segment holds ids outside [0, S)",
           2: "voxel_to_full_maps holds ids outside [0, number of voxels of the scene)",
           4: "segment_to_full_maps holds negative ids",
           8: "voxel_coordinates holds non-finite values"}


def _cat(ts: Sequence[torch.Tensor], dtype, what: str, dev) -> torch.Tensor:
    for t in ts:
        if t.dtype != dtype or t.device != dev:
            raise ValueError(f"{what}: expected {dtype} tensors on {dev}, got {t.dtype} on {t.device}")
    return torch.cat([t.reshape(-1) if t.dim() == 1 else t for t in ts]).contiguous()


def instance_predictions(pred_logits: torch.Tensor, pred_masks: torch.Tensor, voxel2segment: Sequence[torch.Tensor],
                         voxel_to_full_maps: Sequence[torch.Tensor], segment_to_full_maps: Sequence[torch.Tensor],
                         raw_coordinates: Sequence[torch.Tensor], topk_per_scene: int = 100,
                         filter_out_no_object_queries: bool = False, use_dbscan: bool = False,
                         voxel_coordinates: Optional[Sequence[torch.Tensor]] = None,
                         dbscan_eps: float = 0.95) -> List[Dict[str, torch.Tensor]]:
    """Per-scene instance predictions of ``pred_logits`` [B, Q, C+1] (predictions_class[-1]) and ``pred_masks`` [B, S, Q]
    (predictions_mask[-1]), both fp32 on the device.  The index maps and coordinates are per-scene lists of device tensors:
    ``voxel2segment[b]`` [V_b] int64 (segment of each voxel), ``voxel_to_full_maps[b]`` [P_b] int64 (voxel of each point),
    ``segment_to_full_maps[b]`` [P_b] int64 (full-resolution segment of each point), ``raw_coordinates[b]`` [P_b, 3] fp32.

    Returns one dict per scene: ``masks`` [P_b, K] bool (views into one buffer), ``scores`` [K] fp32, ``classes`` [K] int64,
    ``boxes`` [K, 6] fp32 (center xyz, extent xyz; zeros where the mask is empty) and ``box_valid`` [K] bool, all sorted by
    score.  Index values outside their tables raise ValueError.

    ``filter_out_no_object_queries`` / ``use_dbscan``: the reference's eval options (module docstring); ``voxel_coordinates``
    (required with ``use_dbscan``) is a per-scene list of [V_b, 3] fp32 device tensors in voxel2segment[b] order (the
    reference's voxel_features[:, -3:] split by scene), ``dbscan_eps`` the neighbourhood radius (the reference hard-codes
    0.95).  With either option the record length K_b may differ from scene to scene."""
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
    kall = int(topk_per_scene) == -1
    K = Q if kall else int(topk_per_scene)
    ragged = bool(filter_out_no_object_queries) or bool(use_dbscan)
    if not ragged and not 1 <= K <= min(MAX_K, Q * C_):
        raise ValueError(f"topk_per_scene must be -1 or in [1, min({MAX_K}, Q*C = {Q * C_})], got {topk_per_scene}")
    if ragged and not (1 <= K <= MAX_K or (kall and use_dbscan)):
        raise ValueError(f"topk_per_scene must be -1 or in [1, {MAX_K}], got {topk_per_scene}")
    if use_dbscan:
        eps = float(dbscan_eps)
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError(f"dbscan_eps must be a finite number > 0, got {dbscan_eps}")
        if voxel_coordinates is None or len(voxel_coordinates) != B:
            raise ValueError("use_dbscan needs voxel_coordinates: one [V_b, 3] fp32 device tensor per scene")
    V = [int(t.numel()) for t in voxel2segment]
    P = [int(t.numel()) for t in voxel_to_full_maps]
    for b in range(B):
        if int(segment_to_full_maps[b].numel()) != P[b] or tuple(raw_coordinates[b].shape) != (P[b], 3):
            raise ValueError(f"scene {b}: segment_to_full_maps [P] and raw_coordinates [P, 3] must match "
                             f"voxel_to_full_maps (P = {P[b]})")
        if use_dbscan and tuple(voxel_coordinates[b].shape) != (V[b], 3):
            raise ValueError(f"scene {b}: voxel_coordinates must be [V, 3] with V = {V[b]} (voxel2segment), "
                             f"got {tuple(voxel_coordinates[b].shape)}")
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
    i32 = dict(dtype=torch.int32, device=dev)

    # 1. range checks + voxels per segment (read back below, after the launches that do not depend on it)
    nvox = torch.empty(B * S, **i32)
    stats = torch.empty(2, dtype=torch.int64, device=dev)
    L.call("pq3d_instseg_check", v2s, v2f, s2f, offs, B, S, NV, NP, nvox, stats,
           work=(f"B{B}V{NV}P{NP}", 0.0, NV * 8.0 + NP * 16.0 + B * S * 4.0))
    if use_dbscan:
        xyzv = _cat(voxel_coordinates, torch.float32, "voxel_coordinates", dev)
        return _dbscan_predictions(logits, masks_in, v2s, v2f, s2f, xyz, xyzv, offs, offs_h, stats, B, S, Q, C1, K, kall,
                                   bool(filter_out_no_object_queries), eps, V, P, n_chunks)
    # 2. softmax + top-K
    prob = torch.empty(B, Q * C_, dtype=torch.float32, device=dev)
    sel_prob = torch.empty(B, K, dtype=torch.float32, device=dev)
    sel_query, sel_class = torch.empty(B, K, **i32), torch.empty(B, K, **i32)
    if ragged:      # the filter alone: dropped queries' candidates left out of the select (query order kept: no compaction)
        qvalid, kout = torch.empty(B * Q, **i32), torch.empty(B, **i32)
        seg = torch.arange(0, (B + 1) * Q * C_, Q * C_, dtype=torch.int64).to(dev)
        L.call("pq3d_instseg_prob", logits, B, Q, C1, prob, qvalid, work=(f"B{B}Q{Q}C{C1}f", 0.0, B * Q * C1 * 8.0))
        L.call("pq3d_instseg_topk_ragged", prob, seg, qvalid, B, C_, K, int(kall), Q * C_, sel_prob, sel_query, sel_class, kout,
               work=(f"B{B}Q{Q}C{C1}K{K}", 0.0, B * Q * C_ * 4.0 + B * K * 12.0))
    else:
        L.call("pq3d_instseg_topk", logits, B, Q, C1, K, prob, sel_prob, sel_query, sel_class,
               work=(f"B{B}Q{Q}C{C1}K{K}", 0.0, B * Q * C1 * 4.0 + B * K * 12.0))
    # 3. bit table [B*S, K] (top-k order) + mask scores, sorted by score
    nsc = (S + SEG_CHUNK - 1) // SEG_CHUNK
    table = torch.empty(B * S, K, dtype=torch.float32, device=dev)
    ws = torch.empty(B * nsc * K * 16, dtype=torch.uint8, device=dev)
    scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    classes = torch.empty(B, K, dtype=torch.int64, device=dev)
    order = torch.empty(B, K, **i32)
    L.call("pq3d_instseg_scores", masks_in, nvox, sel_prob, sel_query, sel_class, B, S, Q, K, table, ws, ws.numel(), scores, classes, order,
           work=(f"B{B}S{S}Q{Q}K{K}", 0.0, B * S * (K * 8.0 + 4.0) + B * K * 24.0))

    if ragged:
        host = torch.cat((stats, kout.to(torch.int64))).cpu().tolist()     # the one device-to-host read of the call
        err, sf, Kb = int(host[0]), int(host[1]), [int(x) for x in host[2:]]
    else:
        err, sf = (int(x) for x in stats.cpu().tolist())        # the one device-to-host read of the call
        Kb = [K] * B
    Sf = _check_stats(err, sf, B)

    return _vote_and_boxes(v2s, v2f, s2f, xyz, offs, offs_h, table, order, scores, classes, B, S, Sf, K, Kb, P, n_chunks)


def _check_stats(err: int, sf: int, B: int) -> int:
    L.raise_error_word("instance_predictions", err, _ERRORS)
    Sf = max(sf, 1)
    if B * Sf >= (1 << 31) - 65536:
        raise ValueError(f"segment_to_full_maps ids too large for a batched grouping (B * (max id + 1) = {B * Sf})")
    return Sf


def _vote_and_boxes(v2s, v2f, s2f, xyz, offs, offs_h, table, order, scores, classes, B, S, Sf, K, Kb, P, n_chunks):
    """Steps 4-5 on the 0/1 table [B*S, K] whose row of point p is b*S + v2s[voff[b] + voxel_to_full_maps[p]]; scene b's
    record keeps its first Kb[b] sorted columns."""
    dev = table.device
    NP = sum(P)
    # 4. vote per full-resolution segment: rows voxel2segment[voxel_to_full_maps[p]] of the table, grouped by segment_to_full_maps
    gather = torch.empty(NP, dtype=torch.int64, device=dev)
    key = torch.empty(NP, dtype=torch.int64, device=dev)
    L.call("pq3d_instseg_compose", v2s, v2f, s2f, offs, B, S, Sf, NP, gather, key, work=(f"B{B}P{NP}", 0.0, NP * 40.0))
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
    L.call("pq3d_instseg_expand", vsum, vcount, key, xyz, offs, order, B, NP, n_chunks, K, out, bws, 0 if bws is None else bws.numel(),
           boxes, valid, work=(f"B{B}P{NP}K{K}", 0.0, NP * (K * 5.0 + 20.0) + n_chunks * K * BOX_PART_BYTES))
    res = []
    p0 = offs_h[B + 1]
    for b in range(B):
        k = Kb[b]
        if k == K:
            res.append(dict(masks=out[p0:p0 + P[b]], scores=scores[b], classes=classes[b], boxes=boxes[b], box_valid=valid[b]))
        else:
            res.append(dict(masks=out[p0:p0 + P[b], :k], scores=scores[b, :k], classes=classes[b, :k], boxes=boxes[b, :k],
                            box_valid=valid[b, :k]))
        p0 += P[b]
    return res


def _empty_records(P, dev):
    return [dict(masks=torch.zeros(p, 0, dtype=torch.bool, device=dev), scores=torch.zeros(0, dtype=torch.float32, device=dev),
                 classes=torch.zeros(0, dtype=torch.int64, device=dev), boxes=torch.zeros(0, 6, dtype=torch.float32, device=dev),
                 box_valid=torch.zeros(0, dtype=torch.bool, device=dev)) for p in P]


def _fdec(code: int) -> float:
    """Inverse of the kernels' order-preserving float code."""
    u = (code & 0x7FFFFFFF) if code & 0x80000000 else (~code & 0xFFFFFFFF)
    return float(np.array([u], dtype=np.uint32).view(np.float32)[0])


def _dbscan_predictions(logits, masks_in, v2s, v2f, s2f, xyz, xyzv, offs, offs_h, stats, B, S, Q, C1, K, kall, filt, eps, V, P,
                        n_chunks):
    dev = logits.device
    i32 = dict(dtype=torch.int32, device=dev)
    C_ = C1 - 1
    NV = sum(V)
    # D1. coordinate bounds + non-finite flag, class probabilities (+ filter flags); read 1: flags, Sf, bounds
    bounds = torch.empty(B * 6, **i32)
    L.call("pq3d_dbscan_bounds", xyzv, offs, B, NV, bounds, stats, work=(f"B{B}V{NV}", 0.0, NV * 12.0))
    prob = torch.empty(B, Q * C_, dtype=torch.float32, device=dev)
    qvalid = torch.empty(B * Q, **i32) if filt else None
    L.call("pq3d_instseg_prob", logits, B, Q, C1, prob, qvalid, work=(f"B{B}Q{Q}C{C1}{'f' if filt else ''}", 0.0, B * Q * C1 * 8.0))
    host = torch.cat((stats, bounds.to(torch.int64) & 0xFFFFFFFF)).cpu().tolist()
    Sf = _check_stats(int(host[0]), int(host[1]), B)
    if NV == 0:
        return _empty_records(P, dev)
    # D2. grid per scene: cells of side eps / sqrt(3) * (1 - 1e-6) from the scene's minimum
    cell = eps / math.sqrt(3.0) * (1.0 - 1e-6)
    gtab, ndense = [], 0
    for b in range(B):
        if V[b] == 0:
            lo, n = [0.0] * 3, [1, 1, 1]
        else:
            code = [int(x) for x in host[2 + 6 * b:8 + 6 * b]]
            lo = [_fdec(~c & 0xFFFFFFFF) for c in code[:3]]
            hi = [_fdec(c) for c in code[3:]]
            n = [int(math.floor((hi[d] - lo[d]) / cell)) + 1 for d in range(3)]
        cells = n[0] * n[1] * n[2]
        if ndense + cells > MAX_CELLS:
            raise ValueError(f"use_dbscan: the cell grid (side {cell:.4g}) of the batch needs more than 2^24 cells "
                             f"(scene {b}: {n[0]} x {n[1]} x {n[2]}); use a larger dbscan_eps or fewer scenes per call")
        gtab.append([ndense, n[0], n[1], n[2]] + [int(np.array([x], np.float32).view(np.uint32)[0]) for x in lo] + [0])
        ndense += cells
    gtab = torch.tensor(gtab, dtype=torch.int64).reshape(-1).to(dev)
    key = torch.empty(NV, dtype=torch.int64, device=dev)
    L.call("pq3d_dbscan_keys", xyzv, offs, gtab, B, NV, cell, key, work=(f"B{B}V{NV}", 0.0, NV * 20.0))
    plan = SegmentPlan(key, ndense)
    ncap = min(NV, ndense)
    if Q * ncap >= (1 << 31) - 1 or Q * (NV // 64 + 1) >= (1 << 31):
        raise ValueError(f"use_dbscan: Q * cells ({Q} * {ncap}) must fit 31 bits")
    wsb = int(L.lib().pq3d_dbscan_ws_bytes(NV, Q, ncap, B))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    colseg = torch.empty(B + 1, dtype=torch.int64, device=dev)
    L.call("pq3d_dbscan_components", masks_in, v2s, offs, qvalid, xyzv, key, gtab, plan.buf, ndense, B, S, Q, NV, ncap, eps, ws, wsb,
           colseg, work=(f"B{B}V{NV}Q{Q}", 0.0, NV * (Q * 4.0 + 40.0)))
    cs = [int(x) for x in colseg.cpu().tolist()]                   # read 2: the columns per scene
    Qp = [cs[b + 1] - cs[b] for b in range(B)]
    Kb = [q if kall else min(K, q * C_) for q in Qp]
    Kmax, ncol = max(Kb), cs[B]
    if kall and Kmax > MAX_K:
        raise ValueError(f"topk_per_scene = -1 selects one entry per column: {Kmax} columns > {MAX_K}")
    if Kmax == 0:
        return _empty_records(P, dev)
    # D3. columns in (query, smallest voxel) order, their probabilities, top-K over each scene's Q'_b * C candidates
    col = torch.empty(ncol * 4, **i32)
    colprob = torch.empty(ncol * C_, dtype=torch.float32, device=dev)
    L.call("pq3d_dbscan_columns", prob, offs, B, Q, C_, NV, ncap, ncol, ws, col, colprob, work=(f"B{B}N{ncol}C{C_}", 0.0, ncol * C_ * 8.0))
    seg = colseg * C_
    sel_prob = torch.empty(B, Kmax, dtype=torch.float32, device=dev)
    sel_query, sel_class, kout = torch.empty(B, Kmax, **i32), torch.empty(B, Kmax, **i32), torch.empty(B, **i32)
    L.call("pq3d_instseg_topk_ragged", colprob, seg, None, B, C_, Kmax, int(kall), max(Qp) * C_, sel_prob, sel_query, sel_class, kout,
           work=(f"B{B}N{ncol}C{C_}K{Kmax}", 0.0, ncol * C_ * 4.0 + B * Kmax * 12.0))
    # D4. voxel-level table [B * Vmax, K] + scores, ranked
    Vmax = max(V)
    nch = (Vmax + SEG_CHUNK - 1) // SEG_CHUNK
    table = torch.empty(B * Vmax, Kmax, dtype=torch.float32, device=dev)
    part = torch.empty(B * nch * Kmax * 16, dtype=torch.uint8, device=dev)
    L.call("pq3d_dbscan_table", masks_in, v2s, offs, ws, col, colseg, sel_query, kout, B, S, Q, Kmax, NV, ncap, Vmax, table, part,
           part.numel(), work=(f"B{B}V{NV}K{Kmax}", 0.0, NV * (Kmax * 12.0 + 8.0)))
    scores = torch.empty(B, Kmax, dtype=torch.float32, device=dev)
    classes = torch.empty(B, Kmax, dtype=torch.int64, device=dev)
    order = torch.empty(B, Kmax, **i32)
    L.call("pq3d_instseg_rank", part, nch, sel_prob, sel_class, B, Kmax, scores, classes, order,
           work=(f"B{B}K{Kmax}", 0.0, B * nch * Kmax * 16.0))
    # D5. vote on voxel-level rows: the table row of point p is b * Vmax + voxel_to_full_maps[p]
    local = torch.cat([torch.arange(v, dtype=torch.int64, device=dev) for v in V])
    return _vote_and_boxes(local, v2f, s2f, xyz, offs, offs_h, table, order, scores, classes, B, Vmax, Sf, Kmax, Kb, P,
                           n_chunks)
