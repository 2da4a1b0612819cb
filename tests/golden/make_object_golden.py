#!/usr/bin/env python3
"""Generate F27_object_prep.npz by running the reference's own grounding-batch code on a tiny synthetic scan (runs where the
reference is present; never imported by the product):

    python tests/golden/make_object_golden.py [--out PATH]

  data/data_utils.py                     convert_pc_to_box
  data/datasets/sceneverse_base.py       SceneVerseBase.match_gt_to_pred, SceneVerseBase._obj_processing_post

Import recipe (as make_golden_instseg.py): `data` / `data.datasets` are bare packages, so only the modules named above and
data/datasets/constant.py run; `common.misc`, `torch_scatter` and `jsonlines` are stand-ins (nothing on this path calls
them).  The dataset object is made with SceneVerseBase.__new__; `build_rotate_mat` of the module is replaced by a function
returning the matrix the case fixes (the reference draws it at random).

Stored: the scan (points [P, 6] fp32, point ids, the GT instance ids, overlapping predicted masks), the boxes of every GT and
predicted object (convert_pc_to_box on fp32 points: fp32 results), the match tables of match_gt_to_pred on those boxes given
as Python floats (float64 arithmetic, the reference's own number type there), and _obj_processing_post of given index lists:
in float64 without rotation, in fp32 with a rotation, and in float64 with the same rotation (the yardstick of the fp32 case).
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "F27_object_prep.npz")
P, N_IDS, K_PRED, N_SAMPLE = 400, 7, 6, 64


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference():
    sys.path.insert(0, REF)
    for pkg in ("data", "data.datasets"):
        _stub(pkg).__path__ = [os.path.join(REF, *pkg.split("."))]
    _stub("common.misc", rgetattr=lambda *a, **k: None)
    _stub("torch_scatter", scatter_mean=None, scatter_add=None)
    _stub("jsonlines")
    du = importlib.import_module("data.data_utils")
    sb = importlib.import_module("data.datasets.sceneverse_base")
    return du, sb


def make_scan(rng):
    xyz = (rng.random((P, 3)) * np.array([6.0, 5.0, 2.5]) - np.array([3.0, 2.5, 0.0])).astype(np.float32)
    rgb = (rng.random((P, 3)) * 2 - 1).astype(np.float32)
    points = np.concatenate([xyz, rgb], 1)
    # instances: slabs along x, so that boxes overlap little; id 5 carries no point, id -1 is background
    p2i = np.clip(np.floor((xyz[:, 0] + 3.0) / 6.0 * 5), 0, 4).astype(np.int64)
    p2i[rng.random(P) < 0.1] = -1
    inst_ids = np.array([3, 0, 5, 1, 4, 2, 6], dtype=np.int64)          # 5 and 6: no point
    # predictions: shifted slabs (partial overlaps), one copy of instance 1, one empty row, one row over everything
    masks = np.zeros((K_PRED, P), dtype=bool)
    masks[0] = (xyz[:, 0] > -3.0) & (xyz[:, 0] < -1.2)
    masks[1] = p2i == 1
    masks[2] = (xyz[:, 0] > -0.9) & (xyz[:, 0] < 1.0) & (xyz[:, 1] < 1.0)
    masks[4] = True
    masks[5] = (xyz[:, 0] > 1.1) & (xyz[:, 2] > 0.4)
    return points, p2i, inst_ids, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    du, sb = load_reference()
    rng = np.random.default_rng(27)
    points, p2i, inst_ids, masks = make_scan(rng)
    out = dict(points=points, point2instance=p2i, instance_ids=inst_ids, masks=masks)

    def boxes(pcd_list):
        cs = [du.convert_pc_to_box(pc) for pc in pcd_list]
        assert all(isinstance(v, np.float32) for c, b in cs for v in c + b)
        return [c for c, _ in cs], [b for _, b in cs]

    gt_pcds = [points[p2i == i] for i in inst_ids if (p2i == i).any()]
    pred_pcds = [points[m] for m in masks if m.any()]
    gt_c, gt_b = boxes(gt_pcds)
    pr_c, pr_b = boxes(pred_pcds)
    out.update(gt_center=np.array(gt_c, dtype=np.float32), gt_size=np.array(gt_b, dtype=np.float32),
               pred_center=np.array(pr_c, dtype=np.float32), pred_size=np.array(pr_b, dtype=np.float32))
    ds = sb.SceneVerseBase.__new__(sb.SceneVerseBase)
    ds.split = "train"
    as_float = lambda rows: [[float(v) for v in r] for r in rows]
    scan = dict(obj_loc=as_float(gt_c), obj_box=as_float(gt_b), obj_loc_pred=as_float(pr_c), obj_box_pred=as_float(pr_b))
    ds.match_gt_to_pred(scan)
    G, K = len(gt_c), len(pr_c)
    i25, i50 = np.zeros((G, K), dtype=np.uint8), np.zeros((G, K), dtype=np.uint8)
    for g in range(G):
        i25[g, scan["iou25_list"][g]] = 1
        i50[g, scan["iou50_list"][g]] = 1
    out.update(matched=np.array(scan["matched_list"], dtype=np.int32), iou25=i25, iou50=i50)
    assert i25.sum() > i50.sum() > 0 and (i25 == 0).any()

    # _obj_processing_post of three objects' given draws (with repeats for the small one)
    sizes = [len(pc) for pc in gt_pcds]
    objs = [int(np.argmax(sizes)), int(np.argmin(sizes)), 2]
    idx = np.stack([rng.integers(0, sizes[o], N_SAMPLE) for o in objs])
    pcds = np.stack([gt_pcds[o][idx[k]] for k, o in enumerate(objs)])                      # [3, n, 6] fp32
    theta = 0.7
    rot = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]], dtype=np.float32)
    out.update(sample_objects=np.array(objs, dtype=np.int64), sample_idx=idx, sample_rows=pcds, rotation=np.ascontiguousarray(rot.T))

    def post(arr, matrix):
        sb.build_rotate_mat = lambda split, rot_aug: matrix
        fts, locs, bxs, _ = ds._obj_processing_post(arr.copy(), rot_aug=True)
        return fts.numpy(), locs.numpy(), bxs.numpy()

    for tag, arr, matrix in (("f64", pcds.astype(np.float64), None), ("f32rot", pcds, rot), ("f64rot", pcds.astype(np.float64), rot.astype(np.float64))):
        fts, locs, bxs = post(arr, matrix)
        assert fts.dtype == arr.dtype
        out.update({f"{tag}_fts": fts, f"{tag}_locs": locs, f"{tag}_boxes": bxs})
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes); G {G} K {K} matched {scan['matched_list']}")


if __name__ == "__main__":
    main()
