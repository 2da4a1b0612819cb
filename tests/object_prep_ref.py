"""numpy restatement of pq3d_amd/objects.py + csrc/object_prep.hip: the specification of the stage-2 (grounding)
batch preparation.  Plain loops and the exact rule; the kernels equal it bit for bit.

What it restates from the reference (data/datasets/sceneverse_base.py, data/data_utils.py):
  bank      _load_one_scan's per-object point lists (``pcds[instance_labels == inst_id]`` / ``pcds[mask]``: ascending point
            index, rows without a point dropped) and convert_pc_to_box in fp32
  match     match_gt_to_pred with box3d_iou's formula (the ``+ 1e-8``) in float64
  sample    get_scene's ``np.random.choice(n, num_points, replace=n < num_points)`` with a counter-based rule of our own
            (numpy's stream is not pinned) and _obj_processing_post in float64, rounded to fp32 once
  labels    get_scene lines 304-316 / 358-360 and make_bce_label
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
CHUNK = 1024            # PQ3D_OBJECT_CHUNK: points per (row, chunk) cell of the bank build
ROUNDS = 4              # Feistel rounds
WALK_CAP = 256          # PQ3D_OBJECT_WALK_CAP: cycle-walk iterations before the error bit
MAX_SAMPLE = 4096       # PQ3D_OBJECT_MAX_SAMPLE
NT = 256                # threads of a sample_objects workgroup (the reduction tree's width)
ERR_SCENE, ERR_SELECTED, ERR_WALK, ERR_TARGET = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------------ hash, key, permutation
def fin(h):
    """32-bit finaliser (the dropout hash's): works on ints and on uint64 arrays holding 32-bit values."""
    h = np.asarray(h, dtype=np.uint64) & M32
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & M32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def object_key(seed: int, item: int, slot: int):
    """(k0, k1) of one (item, slot) draw from the 64-bit seed word."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0 = int(fin((s & M32) ^ ((item * 0x9E3779B1) & M32)))
    k1 = int(fin((k0 + (s >> 32) + ((slot * 0x85EBCA6B) & M32) + 0x27D4EB2F) & M32))
    return k0, k1


def hash_j(k0: int, k1: int, j):
    """The 32-bit word of draw j (sampling with replacement)."""
    h = (np.asarray(j, dtype=np.uint64) & M32) ^ k0
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & M32
    h = h ^ (h >> 15)
    h = (h + k1) & M32
    h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def feistel_bits(n: int) -> int:
    """Smallest even width w >= 2 with 2^w >= n: for n >= 2 the domain 2^w is below 4 n."""
    w = 2
    while (1 << w) < n:
        w += 2
    return w


def round_keys(k0: int, k1: int):
    return [int(fin((k1 + r * 0x9E3779B1) & M32)) ^ k0 for r in range(ROUNDS)]


def feistel(x, half: int, rk):
    """One pass of the balanced Feistel network over 2 * half bits: a bijection of [0, 4^half)."""
    x = np.asarray(x, dtype=np.uint64)
    mask = (1 << half) - 1
    L, R = x >> half, x & mask
    for r in range(ROUNDS):
        L, R = R, L ^ (fin(R ^ rk[r]) & mask)
    return (L << half) | R


def perm(n: int, k0: int, k1: int, j):
    """perm(j) for every j of the array (all < n): the keyed bijection of [0, n) by cycle-walking.  Returns (values int64,
    most Feistel passes any j needed, capped): a j still out of range after WALK_CAP passes yields 0 and capped = True."""
    j = np.asarray(j, dtype=np.uint64)
    if n == 1:
        return np.zeros(j.shape, dtype=np.int64), 0, False
    half, rk = feistel_bits(n) // 2, round_keys(k0, k1)
    x, out = j.copy(), np.zeros(j.shape, dtype=np.int64)
    live = np.ones(j.shape, dtype=bool)
    steps = 0
    for _ in range(WALK_CAP):
        if not live.any():
            break
        steps += 1
        x[live] = feistel(x[live], half, rk)
        done = live & (x < n)
        out[done] = x[done].astype(np.int64)
        live &= ~done
    return out, steps, bool(live.any())


def sample_indices(n: int, num_points: int, seed: int, item: int, slot: int):
    """The num_points draws (positions in the object's ascending point list) of one slot and the 'walk capped' flag."""
    k0, k1 = object_key(seed, item, slot)
    j = np.arange(num_points, dtype=np.uint64)
    if n >= num_points:
        idx, _, capped = perm(n, k0, k1, j)
        return idx, capped
    return ((hash_j(k0, k1, j) * np.uint64(n)) >> np.uint64(32)).astype(np.int64), False


# ------------------------------------------------------------------------------------------------ bank
def convert_pc_to_box_f32(xyz: np.ndarray):
    """convert_pc_to_box in fp32: (min + max) / 2 and max - min, each one fp32 operation."""
    xyz = np.asarray(xyz, dtype=np.float32)
    mn, mx = xyz.min(0), xyz.max(0)
    return ((mn + mx) / np.float32(2)).astype(np.float32), (mx - mn).astype(np.float32)


def build_object_bank(points, *, point2instance=None, instance_ids=None, masks=None):
    """Per-scan lists as in pq3d_amd.objects.build_object_bank, numpy arrays.  Returns a dict: points (concatenated),
    point_offsets [S+1], object_offsets [S+1], entry_offsets [O+1], order (scan-local point indices, ascending within each
    object), source_row [O] (row of the scan's input), box_center / box_size [O, 3] fp32."""
    S = len(points)
    order, entry, obj_off, src, bc, bs = [], [0], [0], [], [], []
    for s in range(S):
        P = points[s].shape[0]
        if masks is not None:
            rows = [np.asarray(masks[s][k], dtype=bool) for k in range(masks[s].shape[0])]
        else:
            rows = [np.asarray(point2instance[s]) == i for i in np.asarray(instance_ids[s])]
        for k, row in enumerate(rows):
            sel = [p for p in range(P) if row[p]]
            if not sel:
                continue
            order.extend(sel)
            entry.append(entry[-1] + len(sel))
            src.append(k)
            c, z = convert_pc_to_box_f32(points[s][sel, :3])
            bc.append(c)
            bs.append(z)
        obj_off.append(len(src))
    return dict(points=np.concatenate(points, 0).astype(np.float32), point_offsets=np.cumsum([0] + [p.shape[0] for p in points]),
                object_offsets=np.array(obj_off, dtype=np.int64), entry_offsets=np.array(entry, dtype=np.int64),
                order=np.array(order, dtype=np.int32), source_row=np.array(src, dtype=np.int32),
                box_center=np.array(bc, dtype=np.float32).reshape(-1, 3), box_size=np.array(bs, dtype=np.float32).reshape(-1, 3))


# ------------------------------------------------------------------------------------------------ match_gt_to_pred
def box_iou(gc, gs, pc, ps) -> np.float64:
    """box3d_iou of two centre | size boxes through construct_bbox_corners' min / max corners (c -+ s / 2), float64."""
    g0, g1 = [np.float64(-gs[k]) / 2 + np.float64(gc[k]) for k in range(3)], [np.float64(gs[k]) / 2 + np.float64(gc[k]) for k in range(3)]
    p0, p1 = [np.float64(-ps[k]) / 2 + np.float64(pc[k]) for k in range(3)], [np.float64(ps[k]) / 2 + np.float64(pc[k]) for k in range(3)]
    # (a box of negative size would swap its corners, as the reference's min / max over the eight corners does)
    g0, g1 = [min(a, b) for a, b in zip(g0, g1)], [max(a, b) for a, b in zip(g0, g1)]
    p0, p1 = [min(a, b) for a, b in zip(p0, p1)], [max(a, b) for a, b in zip(p0, p1)]
    d = [max(min(g1[k], p1[k]) - max(g0[k], p0[k]), np.float64(0)) for k in range(3)]
    inter = d[0] * d[1] * d[2]
    v1 = (g1[0] - g0[0]) * (g1[1] - g0[1]) * (g1[2] - g0[2])
    v2 = (p1[0] - p0[0]) * (p1[1] - p0[1]) * (p1[2] - p0[2])
    return np.float64(inter) / (v1 + v2 - inter + np.float64(1e-8))


def match_boxes(gt_center, gt_size, pred_center, pred_size):
    """matched [G] int32 (first index of the strictly largest IoU, -1 without predictions), iou25 / iou50 [G, K] uint8."""
    G, K = len(gt_center), len(pred_center)
    matched = np.full(G, -1, dtype=np.int32)
    i25, i50 = np.zeros((G, K), dtype=np.uint8), np.zeros((G, K), dtype=np.uint8)
    for g in range(G):
        best = np.float64(-1)
        for k in range(K):
            iou = box_iou(gt_center[g], gt_size[g], pred_center[k], pred_size[k])
            if iou > best:
                best, matched[g] = iou, k
            i25[g, k] = iou >= 0.25
            i50[g, k] = iou >= 0.5
    return matched, i25, i50


# ------------------------------------------------------------------------------------------------ sample_objects
def _tree(v: np.ndarray, op, identity):
    """The workgroup's fixed reduction tree over the values v[0 .. n) (float64): thread t owns the pairs (2 p, 2 p + 1),
    p = t, t + 256, ..., and folds v[2 t], v[2 t + 1], v[2 t + 512], v[2 t + 513], ... in that order starting from the
    identity; a butterfly over the 64 lanes of each wave (offsets 32 .. 1, lane = op(lane, partner)); the four wave results
    (lane 0) combine as op(op(w0, w1), op(w2, w3))."""
    n = v.shape[0]
    k = (n + 2 * NT - 1) // (2 * NT)
    pad = np.full(k * 2 * NT, identity, dtype=np.float64)
    pad[:n] = v
    acc = np.full(NT, identity, dtype=np.float64)
    for r in pad.reshape(k, NT, 2):
        for h in range(2):
            acc = op(acc, r[:, h])
    lane = np.arange(NT)
    for o in (32, 16, 8, 4, 2, 1):
        acc = op(acc, acc[lane ^ o])
    w = acc[::64]
    return op(op(w[0:1], w[1:2]), op(w[2:3], w[3:4]))[0]


_add = lambda a, b: a + b
_min = lambda a, b: np.where(b < a, b, a)
_max = lambda a, b: np.where(b > a, b, a)


def object_values(rows: np.ndarray, rotation=None):
    """_obj_processing_post of ONE object's sampled rows [n, 6] fp32 in float64, rounded to fp32 at the end: (fts [n, 6],
    locs [6] = mean | size, boxes [6] = (min + max) / 2 | size).  rotation: [3, 3] fp32, xyz' = xyz (row vector) x rotation,
    each coordinate (x R0k + y R1k) + z R2k."""
    r = np.asarray(rows, dtype=np.float32).astype(np.float64)
    n = r.shape[0]
    xyz = r[:, :3]
    if rotation is not None:
        R = np.asarray(rotation, dtype=np.float32).astype(np.float64)
        xyz = np.stack([(xyz[:, 0] * R[0, k] + xyz[:, 1] * R[1, k]) + xyz[:, 2] * R[2, k] for k in range(3)], 1)
    mean = np.array([_tree(xyz[:, k], _add, 0.0) / np.float64(n) for k in range(3)])
    mn = np.array([_tree(xyz[:, k], _min, np.inf) for k in range(3)])
    mx = np.array([_tree(xyz[:, k], _max, -np.inf) for k in range(3)])
    size = mx - mn
    locs = np.concatenate([mean, size]).astype(np.float32)
    boxes = np.concatenate([(mn + mx) / 2, size]).astype(np.float32)
    c = xyz - mean[None]
    d2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    dist = max(np.sqrt(_tree(d2, _max, -np.inf)), np.float64(1e-6))      # sqrt is monotone: the max of the roots
    fts = np.concatenate([c / dist, r[:, 3:]], 1).astype(np.float32)
    return fts, locs, boxes


def sample_objects(bank: dict, scene_of_item, selected, *, num_points: int, seed: int, rotation=None, return_indices=False):
    """obj_fts [B, O, n, 6], obj_locs / obj_boxes [B, O, 6] fp32, obj_pad_masks [B, O] bool and the error word.  A slot
    whose scene or object index is out of range (or whose walk hit the cap) sets its bit and is written as a padded slot."""
    scene_of_item, selected = np.asarray(scene_of_item), np.asarray(selected)
    B, O = selected.shape
    S = len(bank["object_offsets"]) - 1
    fts = np.zeros((B, O, num_points, 6), dtype=np.float32)
    locs, boxes = np.zeros((B, O, 6), dtype=np.float32), np.zeros((B, O, 6), dtype=np.float32)
    pad = np.zeros((B, O), dtype=bool)
    indices = np.full((B, O, num_points), -1, dtype=np.int64)
    err = 0
    for b in range(B):
        s = int(scene_of_item[b])
        if not 0 <= s < S:
            err |= ERR_SCENE
            continue
        o0, n_obj = int(bank["object_offsets"][s]), int(bank["object_offsets"][s + 1] - bank["object_offsets"][s])
        for q in range(O):
            o = int(selected[b, q])
            if o == -1:
                continue
            if not 0 <= o < n_obj:
                err |= ERR_SELECTED
                continue
            e0, e1 = int(bank["entry_offsets"][o0 + o]), int(bank["entry_offsets"][o0 + o + 1])
            idx, capped = sample_indices(e1 - e0, num_points, seed, b, q)
            if capped:
                err |= ERR_WALK
                continue
            pts = bank["order"][e0 + idx].astype(np.int64)
            indices[b, q] = pts
            rows = bank["points"][int(bank["point_offsets"][s]) + pts]
            fts[b, q], locs[b, q], boxes[b, q] = object_values(rows, None if rotation is None else rotation[b])
            pad[b, q] = True
    out = (fts, locs, boxes, pad, err)
    return out + (indices,) if return_indices else out


# ------------------------------------------------------------------------------------------------ ground_labels
def ground_labels(object_offsets, scene_of_item, selected, targets, match=None):
    """The 0-1 rows tgt_object_id, tgt_object_id_iou25, tgt_object_id_iou50 [B, O] fp32 and the error word.

    gt form (match None): slot q is 1 in all three rows iff selected[b, q] is one of the item's targets (scan-local object
    indices of the bank ``selected`` indexes, whose per-scan object offsets are ``object_offsets``).
    pred form: ``match`` = per-scan list of (matched, iou25, iou50) from match_boxes(gt boxes, pred boxes); targets index
    the GT objects of the scan, ``selected`` the predicted ones.  tgt_object_id: slot q is 1 iff matched[t] == selected[b, q]
    for a target t; iou25 / iou50: iff some target's row has the bit of prediction selected[b, q] set.

    A target whose matched (or overlapping) prediction is not among ``selected`` marks no slot: the row may stay all zero.
    (The reference's ``selected_obj_idxs.index(id)`` would raise there; its crop keeps the targets first, so it only meets
    the case when the caller's own selection drops one.  That is the caller's choice here, not an error.)  matched = -1
    (a scan without predictions) marks nothing either."""
    scene_of_item, selected, targets = np.asarray(scene_of_item), np.asarray(selected), np.asarray(targets)
    B, O = selected.shape
    S = len(object_offsets) - 1
    out = np.zeros((3, B, O), dtype=np.float32)
    err = 0
    for b in range(B):
        s = int(scene_of_item[b])
        if not 0 <= s < S:
            err |= ERR_SCENE
            continue
        n_sel = int(object_offsets[s + 1] - object_offsets[s])
        n_tgt = n_sel if match is None else len(match[s][0])
        tg = []
        for t in targets[b]:
            if t == -1:
                continue
            if not 0 <= t < n_tgt:
                err |= ERR_TARGET
                continue
            tg.append(int(t))
        for q in range(O):
            o = int(selected[b, q])
            if o == -1:
                continue
            if not 0 <= o < n_sel:
                err |= ERR_SELECTED
                continue
            for t in tg:
                if match is None:
                    if t == o:
                        out[:, b, q] = 1
                else:
                    matched, i25, i50 = match[s]
                    if matched[t] == o:
                        out[0, b, q] = 1
                    if i25[t, o]:
                        out[1, b, q] = 1
                    if i50[t, o]:
                        out[2, b, q] = 1
    return out[0], out[1], out[2], err
