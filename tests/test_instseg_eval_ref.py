"""CPU: the box-AP restatement (tests/instseg_eval_ref.py) reproduces, bit for bit (NaN equal to NaN), the reference's own
eval_det and InstSegEval.record outputs stored in tests/golden/F29_instseg_eval.npz (tests/golden/
make_golden_instseg_eval.py); pq3d_amd.instseg_eval.BoxAP does the same from the restatement's TP flags."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from pq3d_amd.instseg_eval import BoxAP
from tests import instseg_eval_ref, util

F29 = os.path.join(util.GOLDEN, "F29_instseg_eval.npz")
REF = "/root/reference"
IGNORE = -100
THRESHOLDS = (0.25, 0.5)


def load_box_cases():
    """-> (z, scenes): per scene the stored rows (pboxes, pclasses, pscores, pvalid, gboxes, glabels, gvalid = row not empty
    and label not ignored)."""
    z = np.load(F29)
    scenes = []
    for b, name in enumerate(z["box/scenes"]):
        s = {k: z[f"box/{b}/{k}"] for k in ("pboxes", "pclasses", "pscores", "pvalid", "gboxes", "glabels", "grow_valid")}
        s["name"] = str(name)
        s["gvalid"] = s["grow_valid"] & (s["glabels"] != IGNORE)
        scenes.append(s)
    return z, scenes


def record_lists(scenes):
    """The reference's record dicts: valid rows only."""
    preds = {s["name"]: [(int(c), b, sc) for c, b, sc, v in zip(s["pclasses"], s["pboxes"], s["pscores"], s["pvalid"]) if v]
             for s in scenes}
    gts = {s["name"]: [(int(c), b) for c, b, v in zip(s["glabels"], s["gboxes"], s["gvalid"]) if v] for s in scenes}
    return preds, gts


def full_rows(matched, s):
    """The restatement's per-detection arrays over valid rows and valid GT rows -> over all stored rows (invalid: -inf, -1, 0)."""
    ov, jm, fl = matched
    K = s["pvalid"].shape[0]
    grow = np.nonzero(s["gvalid"])[0]
    ov_f, jm_f, fl_f = np.full(K, -np.inf), np.full(K, -1, np.int32), np.zeros(K, np.uint8)
    v = np.nonzero(s["pvalid"])[0]
    ov_f[v], fl_f[v] = ov, fl
    jm_f[v] = np.where(jm >= 0, grow[np.maximum(jm, 0)] if grow.size else -1, -1)
    return ov_f, jm_f, fl_f


def assert_box_aps(aps, means, z):
    for t, key in enumerate(("ap25", "ap50")):
        assert list(aps[t]) == [int(c) for c in z["box/classes"]], "class key order"
        assert np.array_equal(np.array(list(aps[t].values()), np.float64), z[f"box/{key}"], equal_nan=True), key
    assert np.float64(means[0]) == z["box/mean25"] and np.float64(means[1]) == z["box/mean50"]


def full_results(z):
    keys = [str(k) for k in z["full/result_keys"]]
    return dict(zip(keys, z["full/result_values"])), keys


def assert_full_results(res, z):
    want, keys = full_results(z)
    assert [k for k in res if k != "classes"] == keys, "result keys and their order"
    for k in keys:
        assert np.array_equal(np.float64(res[k]), want[k], equal_nan=True), (k, res[k], want[k])
    labels = [str(x) for x in z["full/class_labels"]]
    cls = np.array([[res["classes"][n]["ap"], res["classes"][n]["ap50%"], res["classes"][n]["ap25%"]] for n in labels])
    assert np.array_equal(cls, z["full/class_ap"], equal_nan=True)


def test_restatement_matches_reference_box_ap():
    z, scenes = load_box_cases()
    preds, gts = record_lists(scenes)
    aps = [instseg_eval_ref.eval_det(preds, gts, t)[0] for t in THRESHOLDS]
    assert_box_aps(aps, [instseg_eval_ref.mean_ap(a) for a in aps], z)
    a25 = np.array(list(aps[0].values()))
    assert np.isnan(a25).any() and (a25 == 0).any() and ((a25 > 0) & (a25 < 1)).any()


def test_restatement_matches_reference_record_averages():
    z = np.load(F29)
    want, _keys = full_results(z)
    labels = [str(x) for x in z["full/class_labels"]]
    classes = {n: {"ap": r[0], "ap50%": r[1], "ap25%": r[2]} for n, r in zip(labels, z["full/class_ap"])}
    got = instseg_eval_ref.group_results(classes, [str(x) for x in z["full/group_order"]], [str(x) for x in z["full/head"]],
                                         [str(x) for x in z["full/common"]], [str(x) for x in z["full/tail"]])
    assert len(got) == 12
    for k, v in got.items():
        assert np.array_equal(np.float64(v), want[k], equal_nan=True), k


def _box_ap_of(order, scenes, matched, via_records=False):
    m = BoxAP(THRESHOLDS)
    for b in order:
        s = scenes[b]
        v = s["pvalid"]
        m.add(s["name"], s["pclasses"][v], s["pscores"][v], matched[s["name"]][2], s["glabels"][s["gvalid"]])
    if via_records:
        other = BoxAP(THRESHOLDS)
        other.extend(pickle.loads(pickle.dumps(m.records())))
        m = other
    return m.compute()


def test_box_ap_on_restated_flags_matches_reference_fixture():
    z, scenes = load_box_cases()
    preds, gts = record_lists(scenes)
    matched = instseg_eval_ref.match_arrays(preds, gts, THRESHOLDS)
    aps, means = _box_ap_of(range(len(scenes)), scenes, matched)
    assert_box_aps(aps, means, z)
    aps, means = _box_ap_of(range(len(scenes)), scenes, matched, via_records=True)
    assert_box_aps(aps, means, z)


def test_parallel_rule_equals_the_sequential_walk():
    """The rule pq3d_box_match implements -- first in (-score, column) order among the scene's detections with the same jmax
    and ovmax > t -- gives the flags of the reference's walk with its taken marks."""
    _z, scenes = load_box_cases()
    preds, gts = record_lists(scenes)
    matched = instseg_eval_ref.match_arrays(preds, gts, THRESHOLDS)
    for sid, p in preds.items():
        ov, jm, fl = matched[sid]
        sc = np.array([d[2] for d in p], np.float32)
        order = sorted(range(len(p)), key=lambda k: (-float(sc[k]), k))
        for t, thr in enumerate(THRESHOLDS):
            seen, want = set(), np.zeros(len(p), bool)
            for k in order:
                if ov[k] > thr and jm[k] not in seen:
                    seen.add(jm[k])
                    want[k] = True
            assert np.array_equal(want, (fl >> t) & 1 == 1), (sid, thr)


def test_record_on_restated_scene_records_matches_reference_record():
    """InstSegEval.record() -- the host half: box AP, mask AP, group means, key order, is_best -- on per-scene records restated
    on the CPU (tests/instseg_ref.py predictions, point-level overlap tables, float64 GT boxes, the restatement's flags)."""
    import torch
    from pq3d_amd.instseg_eval import InstSegEval
    from tests import instseg_ap_ref, instseg_ref
    z = np.load(F29)
    s = lambda k: [str(x) for x in z[k]]
    id_map = {int(k): int(v) for k, v in z["full/id_map"]}
    names = dict(zip((int(i) for i in z["full/name_ids"]), s("full/names")))
    ev = InstSegEval(z["full/valid_class_ids"], s("full/class_labels"), id_map=id_map, class_names=names,
                     groups=dict(head=s("full/head"), common=s("full/common"), tail=s("full/tail")),
                     group_order=s("full/group_order"), topk_per_scene=int(z["full/topk"]))
    remap = lambda a: np.array([id_map.get(int(x), int(x)) for x in a], np.int64)
    preds, gts, scenes = {}, {}, []
    for b, name in enumerate(s("full/scenes")):
        t = lambda k, dt: torch.from_numpy(z[f"full/{b}/{k}"].astype(dt))
        xyz = z[f"full/{b}/raw_coordinates"]
        r = instseg_ref.scene_predictions(torch.from_numpy(z["full/pred_logits"][b]), torch.from_numpy(z["full/pred_masks"][b]),
                                          t("voxel2segment", np.int64), t("voxel_to_full_maps", np.int64),
                                          t("segment_to_full_maps", np.int64), torch.from_numpy(xyz), int(z["full/topk"]))
        r = {k: v.numpy() for k, v in r.items()}
        classes = remap(r["classes"])
        ids = z[f"full/{b}/gt_ids"]
        ev.mask_ap.add(name, instseg_ap_ref.point_tables(r["masks"].astype(bool), ids, z["full/valid_class_ids"]), r["scores"], classes)
        n = int(z[f"full/{b}/n_full"])
        fm = np.unpackbits(z[f"full/{b}/full_masks_packed"], count=n * ids.shape[0]).reshape(n, -1).astype(bool)
        gbox, grow = instseg_ap_ref.gt_boxes_f64(fm, xyz)
        glab = remap(z[f"full/{b}/instance_labels"])
        gv = grow & (glab != IGNORE)
        pv = r["box_valid"].astype(bool)
        preds[name] = [(int(c), bx.astype(np.float32), sc) for c, bx, sc, v in zip(classes, r["boxes"], r["scores"], pv) if v]
        gts[name] = [(int(c), bx.astype(np.float32)) for c, bx, v in zip(glab, gbox, gv) if v]
        scenes.append((name, classes[pv], r["scores"][pv], glab[gv]))
    matched = instseg_eval_ref.match_arrays(preds, gts, THRESHOLDS)
    for name, classes, scores, glab in scenes:
        ev.box_ap.add(name, classes, scores, matched[name][2], glab)
    is_best, res = ev.record()
    assert is_best and res["target_metric"] == res["all_ap"] == res["best_result"] and len(ev.box_ap) == 0
    assert_full_results(res, z)


def test_box_ap_without_scenes_and_argument_errors():
    aps, means = BoxAP().compute()
    assert aps == [{}, {}] and all(np.isnan(m) for m in means)
    m = BoxAP()
    with pytest.raises(ValueError):
        m.add("s", [1, 2], [0.5], [0, 0], [])
    with pytest.raises(ValueError):
        m.add("s", [1], [np.nan], [0], [])
    with pytest.raises(ValueError):
        BoxAP(())


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_regenerated_fixture_matches(tmp_path):
    out = tmp_path / "F29.npz"
    subprocess.run([sys.executable, os.path.join(util.GOLDEN, "make_golden_instseg_eval.py"), "--out", str(out)], check=True,
                   capture_output=True)
    a, b = np.load(F29), np.load(out)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
