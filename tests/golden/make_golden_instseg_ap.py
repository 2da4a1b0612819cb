#!/usr/bin/env python3
"""Generate F23_instseg_ap.npz by running the reference's own mask-AP code (common/eval_instseg.py: eval_instseg, plus
assign_instances_for_scan and evaluate_matches for the raw ap array) and the GT-box loop of InstSegEval.record_preds
(evaluator/instseg_eval.py) on seeded scenes (runs where the reference is present; never imported by the product).

    python tests/golden/make_golden_instseg_ap.py [--out PATH]

common/eval_instseg.py is loaded by file path; the GT id files it reads are written into a temporary directory laid out as
eval_instseg expects.  InstSegEval is loaded with make_golden_instseg.py's import stand-ins.  CLASS_LABELS /
VALID_CLASS_IDS are captured from the module after eval_instseg ran (it sets them).

Stored: per scene b the inputs (masks np.packbits-ed over the flattened [P, K] array, scores, raw classes, GT ids,
full_masks packbits-ed over [G', P], instance labels, coordinates) and bbox_gt (rows of full_masks that gave a box, their
labels and boxes); for the set: ap [n_classes, n_overlaps], all_ap / all_ap_50% / all_ap_25%, per-class [ap, ap50%, ap25%],
the captured label lists.
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pq3d_amd import synth  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "F23_instseg_ap.npz")
DATASET = "ScanNet"
IGNORE = -100
# name: (seed, P, K, G, labels of the instances)
SCENES = [("s0", 31, 1500, 20, 9, (2, 4, 5, 6)),
          ("s1", 32, 1300, 16, 8, (2, 4, 7)),
          ("s2", 33, 900, 10, 0, (2,)),          # no valid GT
          ("s3", 34, 1100, 14, 6, (4, 8))]       # label 8: GT without predictions


def load_eval_module():
    spec = importlib.util.spec_from_file_location("pq3d_ref_eval_instseg", os.path.join(REF, "common", "eval_instseg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_instseg_eval():
    spec = importlib.util.spec_from_file_location("make_golden_instseg", os.path.join(HERE, "make_golden_instseg.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg.load_instseg_eval(), mg


def build_scenes():
    scenes = []
    for name, seed, P, K, G, labels in SCENES:
        masks, ids, scores, classes = synth.instseg_ap_scene(seed, P=P, K=K, G=G, labels=labels, invalid_labels=(1, 3))
        scenes.append(dict(name=name, masks=masks, ids=ids, scores=scores, classes=classes))
    s0, s1, s3 = scenes[0], scenes[1], scenes[3]
    # s0: split its largest instance in two halves; column 0 covers both (IoU 0.5 with each, same label)
    gids, cnt = np.unique(s0["ids"][s0["ids"] >= 2000], return_counts=True)
    big = gids[np.argmax(cnt)]
    pts = np.nonzero(s0["ids"] == big)[0]
    lab = big // 1000
    s0["ids"][pts[: len(pts) // 2]] = lab * 1000 + 998
    s0["ids"][pts[len(pts) // 2:]] = lab * 1000 + 999
    s0["masks"][:, 0] = False
    s0["masks"][pts, 0] = True
    s0["classes"][0] = lab
    # s0: columns 1, 2 both cover most of the second instance (several predictions on one GT instance)
    g2 = gids[np.argsort(cnt)[-2]]
    p2 = np.nonzero(s0["ids"] == g2)[0]
    for k, frac in ((1, 0.9), (2, 0.8)):
        s0["masks"][:, k] = False
        s0["masks"][p2[: int(len(p2) * frac)], k] = True
        s0["classes"][k] = g2 // 1000
    s0["classes"][3] = 9                                       # a class with predictions and no GT anywhere
    s0["classes"][4] = 1                                       # an invalid class
    s1["scores"][0] = s0["scores"][5]                          # equal scores across scenes
    s1["scores"][1] = s0["scores"][1]
    s3["classes"][s3["classes"] == 8] = 4                      # label 8 has GT but no predictions
    for b, s in enumerate(scenes):
        s["coords"] = synth._rng(100 + b, "coords").standard_normal((len(s["ids"]), 3)).astype(np.float32) * 3
        u = [int(i) for i in np.unique(s["ids"]) if i != 0]
        fm = np.zeros((len(u) + 1, len(s["ids"])), dtype=bool)
        for r, i in enumerate(u):
            fm[r] = s["ids"] == i
        s["full_masks"] = fm                                   # last row empty
        il = np.array([i // 1000 for i in u] + [5], dtype=np.int64)
        if len(u) > 1:
            il[1] = IGNORE
        s["instance_labels"] = il
    return scenes


def check_coverage(scenes, valid):
    valid = set(int(v) for v in valid)
    pv = np.concatenate([s["masks"].sum(0) for s in scenes])
    cls = np.concatenate([s["classes"] for s in scenes])
    ids = np.concatenate([s["ids"] for s in scenes])
    gt_lab = {int(i) // 1000 for i in ids if i and int(i) // 1000 in valid}
    pred_lab = {int(c) for c, v in zip(cls, pv) if int(c) in valid and v >= 100}
    sizes = [int((ids == i).sum()) for i in np.unique(ids) if i and int(i) // 1000 in valid]
    stats = dict(small_preds=int((pv < 100).sum()), invalid_class=int(sum(int(c) not in valid for c in cls)),
                 small_gt=int(sum(n < 100 for n in sizes)), invalid_label_pts=int(sum(i and int(i) // 1000 not in valid for i in ids)),
                 unlabeled_pts=int((ids == 0).sum()), gt_only_classes=len(gt_lab - pred_lab), pred_only_classes=len(pred_lab - gt_lab),
                 scene_without_gt=int(any(not any(i and int(i) // 1000 in valid for i in s["ids"]) for s in scenes)),
                 equal_scores=int(scenes[0]["scores"][5] == scenes[1]["scores"][0]))
    assert all(v > 0 for v in stats.values()), stats
    print(stats)


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=OUT)
    a = ap_.parse_args()
    torch.manual_seed(0)
    ev_mod = load_eval_module()
    scenes = build_scenes()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gdir = os.path.join(tmp, DATASET, "meta", "inst_ids_mask3d")
        os.makedirs(gdir)
        preds = {}
        for s in scenes:
            with open(os.path.join(gdir, s["name"] + ".txt"), "w") as f:
                f.write("\n".join(str(int(i)) for i in s["ids"]) + "\n")
            preds[s["name"]] = {"pred_masks": s["masks"], "pred_scores": s["scores"], "pred_classes": s["classes"]}
        cfg = types.SimpleNamespace(data=types.SimpleNamespace(scene_verse_aux=tmp))
        with contextlib.redirect_stdout(io.StringIO()):
            avgs = ev_mod.eval_instseg(preds, DATASET, cfg)
        labels, valid = list(ev_mod.CLASS_LABELS), np.asarray(ev_mod.VALID_CLASS_IDS, dtype=np.int64)
        check_coverage(scenes, valid)
        matches = {}
        for s in scenes:
            gt2pred, pred2gt = ev_mod.assign_instances_for_scan(preds[s["name"]], os.path.join(gdir, s["name"] + ".txt"))
            matches[s["name"]] = {"gt": gt2pred, "pred": pred2gt}
        ap = ev_mod.evaluate_matches(matches)[0]
    out["ap"] = ap
    out["all_ap"] = np.float64(avgs["all_ap"])
    out["all_ap_50"] = np.float64(avgs["all_ap_50%"])
    out["all_ap_25"] = np.float64(avgs["all_ap_25%"])
    out["class_ap"] = np.array([[avgs["classes"][n]["ap"], avgs["classes"][n]["ap50%"], avgs["classes"][n]["ap25%"]]
                                for n in labels], dtype=np.float64)
    out["class_labels"] = np.array(labels)
    out["valid_class_ids"] = valid
    out["scenes"] = np.array([s["name"] for s in scenes])
    # GT boxes by InstSegEval.record_preds
    InstSegEval, mg = load_instseg_eval()
    ev = mg.make_evaluator(InstSegEval, 100)
    ev.record_preds([s["scores"] for s in scenes], [s["masks"].astype(np.float32) for s in scenes],
                    [s["classes"].copy() for s in scenes], [torch.from_numpy(s["full_masks"]) for s in scenes],
                    [s["coords"] for s in scenes], [torch.from_numpy(s["instance_labels"]) for s in scenes],
                    [s["name"] for s in scenes])
    for b, s in enumerate(scenes):
        P, K = s["masks"].shape
        pre = f"{b}/"
        out[pre + "masks_packed"] = np.packbits(s["masks"].reshape(-1))
        out[pre + "shape"] = np.array([P, K], dtype=np.int64)
        out[pre + "scores"] = s["scores"]
        out[pre + "classes"] = s["classes"]
        out[pre + "ids"] = s["ids"]
        out[pre + "full_masks_packed"] = np.packbits(s["full_masks"].reshape(-1))
        out[pre + "n_full"] = np.int64(s["full_masks"].shape[0])
        out[pre + "instance_labels"] = s["instance_labels"]
        out[pre + "coords"] = s["coords"]
        gt = ev.bbox_gt[s["name"]]
        rows = [r for r in range(s["full_masks"].shape[0]) if s["instance_labels"][r] != IGNORE and s["full_masks"][r].any()]
        assert len(rows) == len(gt) and all(int(lbl) == int(s["instance_labels"][r]) for r, (lbl, _) in zip(rows, gt))
        out[pre + "bbox_rows"] = np.array(rows, dtype=np.int64)
        out[pre + "bbox_gt"] = np.array([box for _, box in gt], dtype=np.float32).reshape(-1, 6)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes); all_ap {out['all_ap']:.6f}")


if __name__ == "__main__":
    main()
