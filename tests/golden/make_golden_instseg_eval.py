#!/usr/bin/env python3
"""Generate F29_instseg_eval.npz by running the reference's own box AP (common/eval_det.py: eval_det) on seeded box records and
its own InstSegEval (evaluator/instseg_eval.py: eval_instance_step, record_preds, record) on a few small seeded scenes (runs
where the reference is present; never imported by the product).

    python tests/golden/make_golden_instseg_eval.py [--out PATH]

common/eval_det.py is loaded by file path; InstSegEval with make_golden_instseg.py's import stand-ins; the GT id files
eval_instseg reads are written into a temporary directory, as make_golden_instseg_ap.py does.  Small synthetic head / common /
tail lists and a validation order are patched into the evaluator's module for the run and stored.

Stored:
  box/...   per scene b the records (pboxes [K, 6], pclasses, pscores, pvalid: 0 = empty mask column, left out of the
            reference's records; gboxes [G, 6], glabels, grow_valid: 0 = empty GT row; label -100 = ignored row), eval_det's
            classes in its key order with their AP at 0.25 and 0.5, and the two means of InstSegEval.record.
  full/...  the inputs of InstSegEval.update for B scenes (as F22 stores them, plus gt_ids, full_masks, instance_labels, the
            label map and name lists) and the whole record() dict: scalar keys and values in order, and the per-class rows.
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import math
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pq3d_amd import synth  # noqa: E402
from tests import instseg_eval_ref, instseg_ref  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "F29_instseg_eval.npz")
DATASET = "ScanNet"
IGNORE = -100
MARGIN = 1e-3            # every IoU stays this far from 0.25 / 0.5; scores of one class this far (relative) from each other
FULL = dict(seed=41, P=(900, 700, 800), S=40, Q=16, C=20, topk=24)


def load_by_path(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_make_golden_instseg():
    spec = importlib.util.spec_from_file_location("make_golden_instseg", os.path.join(HERE, "make_golden_instseg.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


# ---------------------------------------------------------------------------------------------------------------- box cases
def _box(rng, scale=2.0):
    return np.concatenate([rng.normal(size=3) * scale, rng.random(3) + 0.2]).astype(np.float32)


def box_scene(rng, K, G, ncls):
    gt = [(int(rng.integers(2, ncls + 2)), _box(rng)) for _ in range(G)]
    pr = []
    for _ in range(K):
        if G and rng.random() < 0.7:
            lab, b = gt[rng.integers(G)]
            b = b.copy()
            b[:3] += (rng.normal(size=3) * 0.08).astype(np.float32)
            b[3:] *= np.float32(1 + rng.normal() * 0.1)
            if rng.random() < 0.15:
                lab = int(rng.integers(2, ncls + 3))
        else:
            lab, b = int(rng.integers(2, ncls + 3)), _box(rng)
        pr.append((lab, b.astype(np.float32), np.float32(rng.random())))
    return pr, gt


def build_box_cases():
    """-> list of dict(name, preds [(class, box, score, valid)], gts [(label, box, row_valid)])."""
    rng = np.random.default_rng(2929)
    ncls = 5                                                 # labels 2 .. 6 in GT, 2 .. 7 in predictions
    scenes = []
    for s, (K, G) in enumerate([(40, 9), (33, 7), (20, 0), (25, 5), (1, 1), (65, 12)]):
        pr, gt = box_scene(rng, K, G, ncls)
        scenes.append(dict(name=f"b{s}", preds=[(c, b, sc, True) for c, b, sc in pr], gts=[(c, b, True) for c, b in gt]))
    s0, s1, s3, s5 = scenes[0], scenes[1], scenes[3], scenes[5]
    s0["gts"].append(s0["gts"][0])                           # duplicate GT boxes
    c, b, sc, _ = s0["preds"][1]
    s0["preds"][1] = (c, np.concatenate([b[:3], np.zeros(3, np.float32)]), sc, True)       # a zero-extent box
    s0["preds"][2] = (3000, s0["preds"][2][1], s0["preds"][2][2], True)                    # a class outside the valid ids
    s0["preds"].insert(5, (2, np.zeros(6, np.float32), np.float32(0.5), False))            # an empty mask column
    s3["gts"] = [(9, g[1], True) for g in s3["gts"][:2]] + s3["gts"][2:]                   # class 9: GT only
    s1["gts"].insert(1, (IGNORE, _box(rng), True))                                         # an ignored GT row
    s1["gts"].insert(3, (4, np.zeros(6, np.float32), False))                               # an empty GT row
    # two boxes that only touch on a face: class 11 has this one GT box and this one detection
    s5["gts"].append((11, np.array([0, 0, 0, 1, 1, 1], np.float32), True))
    s5["preds"].append((11, np.array([1, 0, 0, 1, 1, 1], np.float32), np.float32(0.875), True))
    # a detection inside a GT box with a quarter..half of its volume: TP at 0.25 only
    s5["gts"].append((12, np.array([5, 5, 5, 2, 2, 2], np.float32), True))
    s5["preds"].append((12, np.array([5, 5, 5, 2, 2, 0.75], np.float32), np.float32(0.8125), True))
    return scenes


def box_records(scenes):
    preds = {s["name"]: [(c, b, sc) for c, b, sc, v in s["preds"] if v] for s in scenes}
    gts = {s["name"]: [(c, b) for c, b, v in s["gts"] if v and c != IGNORE] for s in scenes}
    return preds, gts


def check_box_coverage(scenes, preds, gts, ap25, ap50):
    info25, info50 = instseg_eval_ref.eval_det(preds, gts, 0.25)[1], instseg_eval_ref.eval_det(preds, gts, 0.5)[1]
    pc = {c for p in preds.values() for c, _b, _s in p}
    gc = {c for g in gts.values() for c, _b in g}
    same_best = tp25_only = touch = 0
    for sid in preds:
        js = [i[1] for i in info25[sid] if i[1] >= 0 and i[0] > 0.25]
        same_best += len(js) - len(set(js))
        tp25_only += sum(a[2] and not b[2] for a, b in zip(info25[sid], info50[sid]))
    t = info25["b5"][-2]                                     # the class-11 detection: its only GT box shares a face with it
    touch = int(t[0] == 0.0 and t[1] == len(gts["b5"]) - 2 and not t[2])
    for c in pc:                                            # (the records are stored bit for bit: distinct is enough)
        sc = np.sort(np.array([s for p in preds.values() for cc, _b, s in p if cc == c], dtype=np.float64))
        assert sc.size < 2 or (np.diff(sc) > 0).all(), f"class {c}: equal scores"
    dup = any(any(np.array_equal(a[1], b[1]) and a[0] == b[0] for i, a in enumerate(g) for b in g[i + 1:]) for g in gts.values())
    stats = dict(scene_without_gt=int(any(len(g) == 0 for g in gts.values())), gt_only_class=len(gc - pc),
                 pred_only_class=sum(math.isnan(v) for v in ap25.values()), invalid_pred_class=int(3000 in pc),
                 duplicate_gt=int(dup), same_best_gt=same_best, tp25_not_tp50=tp25_only,
                 zero_extent=sum(int((b[3:] == 0).all()) for p in preds.values() for _c, b, _s in p), touching=touch,
                 empty_column=sum(not v for s in scenes for *_x, v in s["preds"]),
                 ignored_gt=sum(c == IGNORE for s in scenes for c, _b, _v in s["gts"]),
                 empty_gt=sum(not v for s in scenes for _c, _b, v in s["gts"]))
    assert all(v > 0 for v in stats.values()), stats
    assert any(0 < v < 1 for v in ap25.values()) and any(v == 0 for v in ap50.values())
    print("box", stats)


def run_box_cases(eval_det_mod, out):
    scenes = build_box_cases()
    preds, gts = box_records(scenes)
    aps = {}
    for thr in (0.25, 0.5):
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            aps[thr] = eval_det_mod.eval_det(preds, gts, ovthresh=thr, use_07_metric=False)[-1]
        mine = instseg_eval_ref.eval_det(preds, gts, thr)[0]
        assert list(mine) == list(aps[thr]) and all(np.array_equal(mine[c], aps[thr][c], equal_nan=True) for c in mine), thr
    check_box_coverage(scenes, preds, gts, aps[0.25], aps[0.5])
    out["box/scenes"] = np.array([s["name"] for s in scenes])
    for b, s in enumerate(scenes):
        out[f"box/{b}/pboxes"] = np.array([p[1] for p in s["preds"]], np.float32).reshape(-1, 6)
        out[f"box/{b}/pclasses"] = np.array([p[0] for p in s["preds"]], np.int64)
        out[f"box/{b}/pscores"] = np.array([p[2] for p in s["preds"]], np.float32)
        out[f"box/{b}/pvalid"] = np.array([p[3] for p in s["preds"]], bool)
        out[f"box/{b}/gboxes"] = np.array([g[1] for g in s["gts"]], np.float32).reshape(-1, 6)
        out[f"box/{b}/glabels"] = np.array([g[0] for g in s["gts"]], np.int64)
        out[f"box/{b}/grow_valid"] = np.array([g[2] for g in s["gts"]], bool)
    assert list(aps[0.25]) == list(aps[0.5])
    out["box/classes"] = np.array(list(aps[0.25]), np.int64)
    out["box/ap25"] = np.array(list(aps[0.25].values()), np.float64)
    out["box/ap50"] = np.array(list(aps[0.5].values()), np.float64)
    for thr, key in ((0.25, "box/mean25"), (0.5, "box/mean50")):      # as InstSegEval.record forms them
        vals = [v for v in aps[thr].values() if not math.isnan(v)]
        out[key] = np.float64(sum(vals) / len(vals))


# ---------------------------------------------------------------------------------------------------------------- full record()
def build_full_case(valid, labels):
    """Seeded scenes whose GT is cut from the restated predictions, so that masks and boxes match some instances well, some
    partly and some not at all."""
    f = FULL
    inp = synth.instseg_inputs(f["seed"], P=f["P"], S=f["S"], Q=f["Q"], C=f["C"])
    B = len(f["P"])
    # model class c -> raw id: the first C valid ids, class 5 -> 1 (a raw id that is not valid)
    id_map = {c: int(valid[c]) for c in range(f["C"])}
    id_map[5] = 1
    names = {int(i): str(n) for i, n in zip(valid, labels)}
    names[1] = "wall"
    inv = {v: k for k, v in id_map.items()}
    scenes = []
    for b in range(B):
        assert instseg_ref.topk_gap(inp["pred_logits"][b], f["topk"]) > 1e-5
        ref = instseg_ref.scene_predictions(inp["pred_logits"][b], inp["pred_masks"][b], inp["voxel2segment"][b],
                                            inp["voxel_to_full_maps"][b], inp["segment_to_full_maps"][b],
                                            inp["raw_coordinates"][b], f["topk"])
        masks, classes = ref["masks"].numpy().astype(bool), ref["classes"].numpy()
        P = masks.shape[0]
        ids = np.zeros(P, np.int64)
        n_inst = 0
        for k in range(masks.shape[1]):
            raw = id_map[int(classes[k])]
            free = masks[:, k] & (ids == 0)
            if raw == 1 or free.sum() < 60 or n_inst >= 5:
                continue
            n_inst += 1
            if n_inst == 4:                                  # one instance of another class than its prediction
                raw = int(valid[(list(valid).index(raw) + 7) % f["C"]])
            ids[free] = raw * 1000 + n_inst
        if b == 1:
            ids[:] = np.where(ids > 0, 0, ids)              # a scene without GT
        u = [int(i) for i in np.unique(ids) if i]
        fm = np.zeros((len(u) + 2, P), bool)
        for r, i in enumerate(u):
            fm[r] = ids == i
        fm[len(u) + 1] = masks[:, 0]                         # an ignored row; row len(u) stays empty
        il = np.array([inv.get(i // 1000, 3) for i in u] + [3, IGNORE], np.int64)
        scenes.append(dict(name=f"scan{b}", ids=ids, full_masks=fm, instance_labels=il))
    return inp, scenes, id_map, names


def run_full_case(mg, out, tmp):
    InstSegEval = mg.load_instseg_eval()
    mod = sys.modules["evaluator.instseg_eval"]
    z23 = np.load(os.path.join(HERE, "F23_instseg_ap.npz"))   # the 200-class lists eval_instseg sets (checked below)
    valid, labels = z23["valid_class_ids"].astype(np.int64), [str(x) for x in z23["class_labels"]]
    inp, scenes, id_map, names = build_full_case(valid, labels)
    f = FULL
    B = len(scenes)
    gdir = os.path.join(tmp, DATASET, "meta", "inst_ids_mask3d")
    os.makedirs(gdir, exist_ok=True)
    for s in scenes:
        with open(os.path.join(gdir, s["name"] + ".txt"), "w") as fh:
            fh.write("\n".join(str(int(i)) for i in s["ids"]) + "\n")
    used = [names[id_map[c]] for c in range(f["C"]) if id_map[c] != 1]
    head, common, tail = used[:6] + ["wall"], used[6:12] + [labels[150]], used[12:18] + [labels[160], labels[161]]
    order = list(reversed(used)) + ["wall", labels[150], labels[160], labels[161], labels[170]]
    mod.HEAD_CATS_SCANNET_200, mod.COMMON_CATS_SCANNET_200, mod.TAIL_CATS_SCANNET_200 = head, common, tail
    mod.VALID_CLASS_IDS_200_VALIDATION = tuple(order)
    ev = mg.make_evaluator(InstSegEval, f["topk"])
    ev.label_converter = types.SimpleNamespace(scannet200_id_to_scannet_raw_id=id_map, scannet_raw_id_to_raw_name=names)
    ev.config.data = types.SimpleNamespace(scene_verse_aux=tmp)
    ev.dataset_name, ev.save, ev.accelerator = DATASET, False, None
    ev.target_metric, ev.best_result = "all_ap", -np.inf
    ev.eval_instance_step([inp["pred_logits"]], [inp["pred_masks"]], inp["voxel_to_full_maps"], inp["voxel2segment"],
                          inp["segment_to_full_maps"], [torch.from_numpy(s["instance_labels"].copy()) for s in scenes],
                          [x.numpy() for x in inp["raw_coordinates"]], [torch.from_numpy(s["full_masks"]) for s in scenes],
                          [s["name"] for s in scenes], None)
    preds = {k: [(c, np.asarray(b, np.float32), np.float32(s)) for c, b, s in v] for k, v in ev.bbox_preds.items()}
    gts = {k: [(c, np.asarray(b, np.float32)) for c, b in v] for k, v in ev.bbox_gt.items()}
    kept = {k: dict(v) for k, v in ev.preds.items()}
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        is_best, res = ev.record()
    assert is_best and res["best_result"] == res["all_ap"]
    ev_mod = sys.modules["common.eval_instseg"]
    assert np.array_equal(np.asarray(ev_mod.VALID_CLASS_IDS), valid) and [str(x) for x in ev_mod.CLASS_LABELS] == labels
    # margins: device scores and box centres differ from the host's in the last bits; no order or threshold may hinge on them
    info = instseg_eval_ref.eval_det(preds, gts, 0.25)[1]
    for sid, rows in info.items():
        for ov, _j, _t in rows:
            assert ov == -np.inf or (abs(ov - 0.25) > MARGIN and abs(ov - 0.5) > MARGIN), (sid, ov)
    by_class = {}
    for v in kept.values():
        for c, s in zip(v["pred_classes"], v["pred_scores"]):
            by_class.setdefault(int(c), []).append(float(s))
    for c, sc in by_class.items():
        sc = np.sort(np.array(sc))
        assert (np.diff(sc) > 1e-4 * sc[1:]).all(), f"class {c}: scores too close"
    mine = instseg_eval_ref.box_results(preds, gts, lambda c: names[c])
    for k, v in mine.items():
        assert np.array_equal(np.float64(v), np.float64(res[k]), equal_nan=True), k
    grp = instseg_eval_ref.group_results(res["classes"], order, head, common, tail)
    for k, v in grp.items():
        assert np.array_equal(np.float64(v), np.float64(res[k]), equal_nan=True), k
    tp25 = sum(t for rows in info.values() for _o, _j, t in rows)
    stats = dict(box_tp25=int(tp25), box_classes=len([k for k in res if k.endswith("_val_box_ap_25")]),
                 nonzero_group_means=sum(bool(res[k] > 0) for k in grp), all_ap_positive=int(res["all_ap"] > 0),
                 nan_box_class=sum(math.isnan(res[k]) for k in res if k.endswith("_val_box_ap_25")),
                 invalid_pred_class=int("wall_val_box_ap_25" in res))
    assert all(v > 0 for v in stats.values()), stats
    print("full", stats, {k: float(res[k]) for k in ("mean_box_ap_25", "mean_box_ap_50", "all_ap", "mean_ap", "mean_head_ap")})
    pre = "full/"
    out[pre + "topk"], out[pre + "B"] = np.int64(f["topk"]), np.int64(B)
    out[pre + "pred_logits"], out[pre + "pred_masks"] = inp["pred_logits"].numpy(), inp["pred_masks"].numpy()
    for b, s in enumerate(scenes):
        for key in ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps"):
            out[f"{pre}{b}/{key}"] = inp[key][b].numpy().astype(np.int32)
        out[f"{pre}{b}/raw_coordinates"] = inp["raw_coordinates"][b].numpy()
        out[f"{pre}{b}/gt_ids"] = s["ids"]
        out[f"{pre}{b}/full_masks_packed"] = np.packbits(s["full_masks"].reshape(-1))
        out[f"{pre}{b}/n_full"] = np.int64(s["full_masks"].shape[0])
        out[f"{pre}{b}/instance_labels"] = s["instance_labels"]
    out[pre + "scenes"] = np.array([s["name"] for s in scenes])
    out[pre + "id_map"] = np.array(sorted(id_map.items()), np.int64)
    out[pre + "valid_class_ids"], out[pre + "class_labels"] = valid, np.array(labels)
    out[pre + "name_ids"] = np.array(sorted(names), np.int64)
    out[pre + "names"] = np.array([names[i] for i in sorted(names)])
    out[pre + "head"], out[pre + "common"], out[pre + "tail"] = np.array(head), np.array(common), np.array(tail)
    out[pre + "group_order"] = np.array(order)
    keys = [k for k in res if k != "classes"]
    out[pre + "result_keys"] = np.array(keys)
    out[pre + "result_values"] = np.array([res[k] for k in keys], np.float64)
    out[pre + "class_ap"] = np.array([[res["classes"][n]["ap"], res["classes"][n]["ap50%"], res["classes"][n]["ap25%"]]
                                      for n in labels], np.float64)


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--out", default=OUT)
    a = ap_.parse_args()
    torch.manual_seed(0)
    mg = load_make_golden_instseg()
    sys.path.insert(0, REF)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        run_full_case(mg, out, tmp)                          # (loads the reference's packages, eval_det among them)
    run_box_cases(sys.modules["common.eval_det"], out)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
