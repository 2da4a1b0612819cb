"""CPU restatement of the instance-prediction step (InstSegEval.eval_instance_step with use_dbscan = False and
filter_out_no_object_queries = False), written from its definition at voxel level -- the checker of
pq3d_amd.instseg.instance_predictions -- plus the tie-aware comparison of two prediction records.  Not imported by the
product."""
from __future__ import annotations

import numpy as np
import torch


def scene_predictions(logits, masks, v2s, v2f, s2f, xyz, topk=100):
    """One scene: logits [Q, C+1], masks [S, Q], voxel2segment [V], voxel_to_full_maps [P], segment_to_full_maps [P],
    raw_coordinates [P, 3] (CPU).  Returns masks [P, K] bool, scores [K], classes [K], boxes [K, 6], box_valid [K], sorted
    by score (ties by top-k rank)."""
    prob = torch.softmax(logits.float(), dim=-1)[:, :-1]
    Q, C = prob.shape
    K = Q if topk == -1 else topk
    flat = prob.flatten()
    sel = torch.sort(flat, descending=True, stable=True).indices[:K]       # ties: lower flat index first
    p_sel, query, cls = flat[sel], sel // C, sel % C
    mv = masks[v2s][:, query]                                               # [V, K] voxel logits of the selections
    on = (mv > 0).float()
    mask_score = (torch.sigmoid(mv) * on).sum(0) / (on.sum(0) + 1e-6)
    score = p_sel * mask_score
    bits = (masks[v2s[v2f]][:, query] > 0).long()                            # [P, K] at the point's voxel's segment
    nf = int(s2f.max()) + 1 if s2f.numel() else 1
    vote = torch.zeros(nf, K, dtype=torch.long).index_add_(0, s2f, bits)
    count = torch.zeros(nf, dtype=torch.long).index_add_(0, s2f, torch.ones_like(s2f))
    full = (2 * vote > count[:, None])[s2f]                                 # mean > 0.5, exactly
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


def predictions(inp, topk=100):
    """All scenes of a synth.instseg_inputs-style dict."""
    return [scene_predictions(inp["pred_logits"][b], inp["pred_masks"][b], inp["voxel2segment"][b],
                              inp["voxel_to_full_maps"][b], inp["segment_to_full_maps"][b], inp["raw_coordinates"][b], topk)
            for b in range(inp["pred_logits"].shape[0])]


def topk_gap(logits, K):
    """Relative gap between the K-th and (K+1)-th largest class probability of a scene (0 when K = Q*C)."""
    p = torch.sort(torch.softmax(logits.float(), -1)[:, :-1].flatten(), descending=True).values
    if K >= p.numel():
        return float("inf")
    return float((p[K - 1] - p[K]) / p[K - 1])


def assert_match(got, ref, rtol=1e-5, atol=1e-6, what=""):
    """Classes, masks and box extents exactly equal column for column, scores and centers within rtol; columns whose
    reference scores tie (within rtol) are compared as a set, since the order among ties is not defined."""
    g = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in got.items()}
    r = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in ref.items()}
    K = r["scores"].shape[0]
    assert g["scores"].shape == (K,) and g["masks"].shape == r["masks"].shape, (what, g["masks"].shape, r["masks"].shape)
    np.testing.assert_allclose(g["scores"], r["scores"], rtol=rtol, atol=atol, err_msg=what)
    i = 0
    while i < K:                                       # groups of (near-)tied reference scores
        j = i + 1
        while j < K and abs(r["scores"][j] - r["scores"][i]) <= rtol * abs(r["scores"][i]) + atol:
            j += 1
        cols = list(range(i, j))

        def keyed(d):
            return sorted(cols, key=lambda c: (int(d["classes"][c]), np.packbits(d["masks"][:, c].astype(bool)).tobytes()))
        for cg, cr in zip(keyed(g), keyed(r)):
            tag = f"{what} column {cr} (tie group {i}..{j - 1})"
            assert int(g["classes"][cg]) == int(r["classes"][cr]), tag
            assert np.array_equal(g["masks"][:, cg].astype(bool), r["masks"][:, cr].astype(bool)), tag
            assert bool(g["box_valid"][cg]) == bool(r["box_valid"][cr]), tag
            if r["box_valid"][cr]:
                assert np.array_equal(g["boxes"][cg, 3:], r["boxes"][cr, 3:]), (tag, g["boxes"][cg], r["boxes"][cr])
                np.testing.assert_allclose(g["boxes"][cg, :3], r["boxes"][cr, :3], rtol=rtol, atol=atol, err_msg=tag)
        i = j
