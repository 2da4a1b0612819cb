#!/usr/bin/env python3
"""Generate F24_instseg_dbscan.npz by running the reference's own InstSegEval.eval_instance_step with
filter_out_no_object_queries and / or use_dbscan (evaluator/instseg_eval.py:104-116, 245-270; sklearn DBSCAN with eps 0.95,
min_samples 1) on seeded scenes (runs where the reference is present; never imported by a test).

    python tests/golden/make_golden_instseg_dbscan.py

Same import recipe as make_golden_instseg.py.  One scene per reference call: with use_dbscan the reference re-slices
coordinates_per_voxel in place (instseg_eval.py:114), so a second scene of one call would index an empty tensor.  Voxel
coordinates come from synth.instseg_voxel_coordinates (one representative point per voxel on a 0.1 lattice, two segments
cut in two).  The boundary rule: sklearn's adjacency at exactly eps depends on its neighbour algorithm, so every fixture
scene is asserted to hold no voxel pair within a relative 1e-4 of eps.

Stored per case name / scene b: the inputs (pred_logits [1, Q, C+1], pred_masks [1, S, Q], the index maps as int32,
raw_coordinates, voxel_coordinates) and the reference's preds / bbox_preds as in F22 (masks np.packbits-ed over [P, K_b]).
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pq3d_amd import synth  # noqa: E402
from tests import instseg_dbscan_ref, instseg_ref  # noqa: E402

OUT = os.path.join(HERE, "F24_instseg_dbscan.npz")
EPS = 0.95
C = 200       # the reference's filter compares with the literal 200
# name: (seed, points per scene, S, Q, filter, dbscan, topk_per_scene)
CASES = {"filt_k100": (31, (1500, 1100), 64, 20, True, False, 100),
         "filt_kall": (32, (1300, 900), 64, 20, True, False, -1),
         "dbscan_k100": (33, (1600,), 64, 20, False, True, 100),
         "dbscan_kall": (34, (1400,), 64, 20, False, True, -1),
         "both_k100": (35, (1500,), 64, 20, True, True, 100),
         "both_kall": (36, (1200,), 64, 20, True, True, -1)}
KEYS = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps")


def load_instseg_eval():
    spec = importlib.util.spec_from_file_location("make_golden_instseg", os.path.join(HERE, "make_golden_instseg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_instseg_eval()


def make_evaluator(InstSegEval, topk, filt, dbscan):
    ev = InstSegEval.__new__(InstSegEval)
    ev.config = types.SimpleNamespace(eval=types.SimpleNamespace(topk_per_scene=topk))
    ev.preds, ev.bbox_preds, ev.bbox_gt = {}, {}, {}
    ev.ignore_label = -100
    ev.use_dbscan = dbscan
    ev.filter_out_no_object_queries = filt
    ev.label_converter = types.SimpleNamespace(scannet200_id_to_scannet_raw_id={})   # identity mapping
    return ev


def min_boundary_gap(xyz):
    d = np.sqrt(((xyz[:, None, :].astype(np.float64) - xyz[None, :, :].astype(np.float64)) ** 2).sum(-1))
    return float(np.abs(d - EPS).min() / EPS)


def boundary_gap(logits, masks, v2s, xyzv, filt, dbscan, topk):
    """Relative gap between the K-th and (K+1)-th candidate probability over the columns (the components of one query tie,
    and torch.topk's order among ties is unspecified)."""
    prob, _ = instseg_dbscan_ref.columns(logits, masks, v2s, xyzv, filt, dbscan, EPS)
    p = torch.sort(prob.flatten(), descending=True).values
    K = prob.shape[0] if topk == -1 else topk
    if K >= p.numel():
        return float("inf")
    return float((p[K - 1] - p[K]) / p[K - 1])


def scenes(seed, P, S, Q, filt, dbscan, topk):
    """The first seed from `seed` on whose scenes have a clear top-k boundary (with DBSCAN the components of a query tie,
    so most seeds cut a tie group at K: the DBSCAN cases hold one scene each)."""
    for s in range(seed, seed + 6000, 100):
        inp = synth.instseg_inputs(s, P=P, S=S, Q=Q, C=C)
        logits = inp["pred_logits"].clone()
        for b in range(len(P)):
            logits[b, 3, C] = 12.0           # queries dropped by the filter (no-object argmax)
            logits[b, 7, C] = 11.0
        inp["pred_logits"] = logits
        xyzv = synth.instseg_voxel_coordinates(inp)
        if all(boundary_gap(logits[b], inp["pred_masks"][b], inp["voxel2segment"][b], xyzv[b], filt, dbscan, topk) > 1e-5
               for b in range(len(P))):
            return s, inp, xyzv
    raise AssertionError("no seed with a clear top-k boundary")


def run_case(InstSegEval, name, seed, P, S, Q, filt, dbscan, topk):
    seed, inp, xyzv = scenes(seed, P, S, Q, filt, dbscan, topk)
    B = len(P)
    logits = inp["pred_logits"]
    out = {f"{name}/topk": np.int64(topk), f"{name}/B": np.int64(B), f"{name}/filter": np.int64(filt),
           f"{name}/dbscan": np.int64(dbscan), f"{name}/eps": np.float64(EPS)}
    stats = dict(split_queries=0, cut_segments=0, dropped=0, empty_queries=0)
    for b in range(B):
        gap = min_boundary_gap(xyzv[b].numpy())
        assert gap > 1e-4, f"{name}/{b}: a voxel pair lies within {gap:.2e} (relative) of eps"
        ev = make_evaluator(InstSegEval, topk, filt, dbscan)
        sid = f"{name}_{b}"
        v2s, v2f, s2f = (inp[k][b] for k in KEYS)
        ev.eval_instance_step([logits[b:b + 1]], [inp["pred_masks"][b:b + 1]], [v2f], [v2s], [s2f],
                              [torch.zeros(0, dtype=torch.int64)], [inp["raw_coordinates"][b].numpy()],
                              [torch.zeros(0, P[b])], [sid], xyzv[b])
        pr = ev.preds[sid]
        masks = np.asarray(pr["pred_masks"]) != 0
        K = masks.shape[1]
        out[f"{name}/{b}/pred_logits"] = logits[b:b + 1].numpy()
        out[f"{name}/{b}/pred_masks"] = inp["pred_masks"][b:b + 1].numpy()
        for key in KEYS:
            out[f"{name}/{b}/{key}"] = inp[key][b].numpy().astype(np.int32)
        out[f"{name}/{b}/raw_coordinates"] = inp["raw_coordinates"][b].numpy()
        out[f"{name}/{b}/voxel_coordinates"] = xyzv[b].numpy()
        out[f"{name}/{b}/masks_packed"] = np.packbits(masks.reshape(-1))
        out[f"{name}/{b}/scores"] = np.asarray(pr["pred_scores"], np.float32)
        out[f"{name}/{b}/classes"] = np.asarray(pr["pred_classes"], np.int64)
        boxes, valid = np.zeros((K, 6), np.float32), np.zeros(K, bool)
        it = iter(ev.bbox_preds[sid])
        for k in range(K):
            if masks[:, k].any():
                cls, box, score = next(it)
                boxes[k], valid[k] = box, True
        assert next(it, None) is None
        out[f"{name}/{b}/boxes"], out[f"{name}/{b}/box_valid"] = boxes, valid
        ref = dict(masks=masks, scores=out[f"{name}/{b}/scores"], classes=out[f"{name}/{b}/classes"], boxes=boxes,
                   box_valid=valid)
        got = instseg_dbscan_ref.scene_predictions(logits[b], inp["pred_masks"][b], v2s, v2f, s2f, inp["raw_coordinates"][b],
                                                   xyzv[b], topk, filt, dbscan, EPS)
        instseg_ref.assert_match(got, ref, what=f"{name}/{b} restatement vs reference")
        # coverage
        p = torch.softmax(logits[b], -1)
        keep = torch.argmax(p, -1) != C if filt else torch.ones(Q, dtype=torch.bool)
        stats["dropped"] += int((~keep).sum())
        mv = inp["pred_masks"][b][v2s]
        stats["empty_queries"] += int((~(mv[:, keep] > 0).any(0)).sum())
        if dbscan:
            x = xyzv[b].numpy()
            for q in np.nonzero(keep.numpy())[0]:
                idx = np.nonzero((mv[:, q] > 0).numpy())[0]
                if len(idx) == 0:
                    continue
                lab = instseg_dbscan_ref.components(x[idx], EPS)
                stats["split_queries"] += int(lab.max() > 0)
                segs = v2s.numpy()[idx]
                for s in np.unique(segs):
                    stats["cut_segments"] += int(len(np.unique(lab[segs == s])) > 1)
    need = ("dropped",) if filt else ()
    need += ("split_queries", "cut_segments", "empty_queries") if dbscan else ()
    assert all(stats[k] > 0 for k in need), (name, stats)
    print(name, "seed", seed, stats)
    return out


def main():
    torch.manual_seed(0)
    InstSegEval = load_instseg_eval()
    out = {}
    for name, args in CASES.items():
        out.update(run_case(InstSegEval, name, *args))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
