"""CPU restatement of the instance-prediction step with filter_out_no_object_queries and use_dbscan (InstSegEval
eval_instance_step :104-116 and dbscan :245-270 with min_samples = 1), written from the definition in pq3d_amd/instseg.py --
the checker of the GPU path.  DBSCAN with min_samples = 1 is the connected components of the graph
"((dx*dx + dy*dy) + dz*dz) <= eps*eps" in fp64 on the fp32 coordinates: a scipy cKDTree proposes candidate pairs (a radius a
little above eps), each pair is re-tested with that exact expression, and scipy.sparse.csgraph.connected_components labels
the graph.  Not imported by the product."""
from __future__ import annotations

import numpy as np
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def adjacent(a: np.ndarray, b: np.ndarray, eps: float) -> np.ndarray:
    """The exact adjacency test of rows of a and b ([n, 3] fp32), fp64, no contraction (numpy rounds every operation)."""
    d = a.astype(np.float64) - b.astype(np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= np.float64(eps) * np.float64(eps)


def components(xyz: np.ndarray, eps: float) -> np.ndarray:
    """Labels [n] of the components of n fp32 points, numbered in the order of their smallest point index."""
    n = xyz.shape[0]
    if n == 0:
        return np.zeros(0, np.int64)
    pairs = cKDTree(xyz.astype(np.float64)).query_pairs(eps * (1.0 + 1e-9), output_type="ndarray")
    if len(pairs):
        pairs = pairs[adjacent(xyz[pairs[:, 0]], xyz[pairs[:, 1]], eps)]
    g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])) if len(pairs) else ([], ([], [])), shape=(n, n))
    _, lab = connected_components(g.tocsr(), directed=False)
    first = np.full(lab.max() + 1, n)
    np.minimum.at(first, lab, np.arange(n))
    rank = np.empty_like(first)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[lab]


def columns(logits, masks, v2s, xyzv, filt: bool, dbscan: bool, eps: float = 0.95):
    """Columns of one scene before the top-k: prob [Q', C] and voxel-level mask logits [V, Q'] (filter, then DBSCAN)."""
    p = torch.softmax(logits.float(), dim=-1)
    C = p.shape[1] - 1
    keep = torch.argmax(p, dim=-1) != C if filt else torch.ones(p.shape[0], dtype=torch.bool)
    prob, mv = p[keep][:, :C], masks[v2s][:, keep]
    if not dbscan:
        return prob, mv
    xyz = xyzv.numpy().astype(np.float32)
    probs, cols = [], []
    for q in range(mv.shape[1]):
        on = (mv[:, q] > 0).numpy()
        idx = np.nonzero(on)[0]
        if len(idx) == 0:
            continue
        lab = components(xyz[idx], eps)
        for c in range(lab.max() + 1):
            sel = torch.zeros(mv.shape[0], dtype=torch.bool)
            sel[torch.from_numpy(idx[lab == c])] = True
            cols.append(torch.where(sel, mv[:, q], torch.zeros(())))
            probs.append(prob[q])
    if not cols:
        return torch.zeros(0, C), torch.zeros(mv.shape[0], 0)
    return torch.stack(probs), torch.stack(cols, 1)


def scene_predictions(logits, masks, v2s, v2f, s2f, xyz, xyzv=None, topk=100, filt=False, dbscan=False, eps=0.95):
    """One scene (CPU tensors; xyzv [V, 3] the voxel coordinates): the record of pq3d_amd.instseg.instance_predictions --
    masks [P, K_b] bool, scores, classes, boxes, box_valid sorted by score (ties by top-k rank).  The tail is
    tests/instseg_ref.scene_predictions on voxel-level columns."""
    prob, mv = columns(logits, masks, v2s, xyzv, filt, dbscan, eps)
    Qc, C = prob.shape
    K = Qc if topk == -1 else min(topk, Qc * C)
    flat = prob.flatten()
    sel = torch.sort(flat, descending=True, stable=True).indices[:K]       # ties: lower flat index first
    p_sel, query, cls = flat[sel], sel // C, sel % C
    m = mv[:, query]                                                         # [V, K] voxel logits of the selections
    on = (m > 0).float()
    score = p_sel * ((torch.sigmoid(m) * on).sum(0) / (on.sum(0) + 1e-6))
    bits = (mv[v2f][:, query] > 0).long()                                    # [P, K] at the point's voxel
    nf = int(s2f.max()) + 1 if s2f.numel() else 1
    vote = torch.zeros(nf, K, dtype=torch.long).index_add_(0, s2f, bits)
    count = torch.zeros(nf, dtype=torch.long).index_add_(0, s2f, torch.ones_like(s2f))
    full = (2 * vote > count[:, None])[s2f]
    srt = torch.sort(score, descending=True, stable=True).indices
    full, score, cls = full[:, srt], score[srt], cls[srt]
    boxes = torch.zeros(K, 6)
    valid = torch.zeros(K, dtype=torch.bool)
    for k in range(K):
        pts = xyz[full[:, k]]
        if pts.shape[0]:
            boxes[k, :3] = pts.double().mean(0).float()
            boxes[k, 3:] = pts.max(0).values - pts.min(0).values
            valid[k] = True
    return dict(masks=full, scores=score, classes=cls, boxes=boxes, box_valid=valid)


def eps_ulp_pairs(eps: float):
    """Pairs of fp32 points whose distance along one axis is the fp32 value next to float32(eps) (one ulp below, at, one ulp
    above), plus a fp32-rounded diagonal: [n, 2, 3] fp32."""
    e32 = np.float32(eps)
    ds = [np.nextafter(e32, np.float32(0)), e32, np.nextafter(e32, np.float32(np.inf))]
    out = []
    for axis in range(3):
        for d in ds:
            a = np.array([1.5, -2.25, 0.75], np.float32)
            b = a.copy()
            b[axis] = np.float32(a[axis] + d)
            out.append((a, b))
    for d in ds:
        a = np.array([0.0, 0.0, 0.0], np.float32)
        out.append((a, np.full(3, np.float32(d / np.float32(np.sqrt(3.0))), np.float32)))
    return np.array(out, np.float32)
