"""CPU: the mask-AP restatement (tests/instseg_ap_ref.py) and pq3d_amd.instseg_ap.InstSegAP reproduce the reference's own
evaluate_matches / eval_instseg outputs and record_preds' GT boxes stored in tests/golden/F23_instseg_ap.npz
(tests/golden/make_golden_instseg_ap.py) exactly; the scene order does not matter."""
import ast
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from pq3d_amd.instseg_ap import InstSegAP, default_overlaps
from tests import instseg_ap_ref, util

F23 = os.path.join(util.GOLDEN, "F23_instseg_ap.npz")
REF = "/root/reference"


def load_f23():
    z = np.load(F23)
    scenes = []
    for b, name in enumerate(z["scenes"]):
        P, K = (int(x) for x in z[f"{b}/shape"])
        n_full = int(z[f"{b}/n_full"])
        scenes.append(dict(name=str(name), masks=np.unpackbits(z[f"{b}/masks_packed"], count=P * K).reshape(P, K).astype(bool),
                           scores=z[f"{b}/scores"], classes=z[f"{b}/classes"], ids=z[f"{b}/ids"],
                           full_masks=np.unpackbits(z[f"{b}/full_masks_packed"], count=n_full * P).reshape(n_full, P).astype(bool),
                           instance_labels=z[f"{b}/instance_labels"], coords=z[f"{b}/coords"], bbox_rows=z[f"{b}/bbox_rows"],
                           bbox_gt=z[f"{b}/bbox_gt"]))
    return z, scenes


def assert_averages(got, z, labels):
    for key, zk in (("all_ap", "all_ap"), ("all_ap_50%", "all_ap_50"), ("all_ap_25%", "all_ap_25")):
        assert np.array_equal(np.float64(got[key]), z[zk], equal_nan=True), (key, got[key], z[zk])
    cls = np.array([[got["classes"][n]["ap"], got["classes"][n]["ap50%"], got["classes"][n]["ap25%"]] for n in labels])
    assert np.array_equal(cls, z["class_ap"], equal_nan=True)


def test_restatement_matches_reference_fixture():
    z, scenes = load_f23()
    valid, labels = z["valid_class_ids"], [str(x) for x in z["class_labels"]]
    tabs = [(instseg_ap_ref.point_tables(s["masks"], s["ids"], valid), s["scores"], s["classes"]) for s in scenes]
    ap = instseg_ap_ref.ap_from_tables(tabs, valid)
    assert np.array_equal(ap, z["ap"], equal_nan=True)
    assert np.isnan(ap).any() and (ap == 0).any() and ((ap > 0) & (ap < 1)).any()
    assert_averages(instseg_ap_ref.averages(ap, labels), z, labels)
    for s in scenes:
        boxes, valid_rows = instseg_ap_ref.gt_boxes_f64(s["full_masks"], s["coords"])
        rows = [r for r in range(len(valid_rows)) if valid_rows[r] and s["instance_labels"][r] != -100]
        assert rows == list(s["bbox_rows"])
        assert np.array_equal(boxes[rows, 3:].astype(np.float32), s["bbox_gt"][:, 3:])
        np.testing.assert_allclose(boxes[rows, :3], s["bbox_gt"][:, :3], rtol=1e-5, atol=1e-6)


def _ap_of(order, z, scenes, via_records=False):
    valid, labels = z["valid_class_ids"], [str(x) for x in z["class_labels"]]
    m = InstSegAP(valid, labels)
    for b in order:
        s = scenes[b]
        m.add(s["name"], instseg_ap_ref.point_tables(s["masks"], s["ids"], valid), s["scores"], s["classes"])
    if via_records:
        other = InstSegAP(valid, labels)
        other.extend(pickle.loads(pickle.dumps(m.records())))
        m = other
    return m.compute()


def test_instseg_ap_on_restated_tables_matches_reference_fixture():
    z, scenes = load_f23()
    ap, avgs = _ap_of(range(len(scenes)), z, scenes)
    assert np.array_equal(ap, z["ap"], equal_nan=True)
    assert_averages(avgs, z, [str(x) for x in z["class_labels"]])


@pytest.mark.parametrize("order", [(3, 1, 0, 2), (2, 3, 1, 0)])
def test_scene_order_and_records_round_trip_change_nothing(order):
    z, scenes = load_f23()
    ap, avgs = _ap_of(order, z, scenes, via_records=True)
    assert np.array_equal(ap, z["ap"], equal_nan=True)
    assert_averages(avgs, z, [str(x) for x in z["class_labels"]])


def test_repeated_key_replaces_scene():
    z, scenes = load_f23()
    valid, labels = z["valid_class_ids"], [str(x) for x in z["class_labels"]]
    m = InstSegAP(valid, labels)
    s0, s1 = scenes[0], scenes[1]
    m.add("x", instseg_ap_ref.point_tables(s1["masks"], s1["ids"], valid), s1["scores"], s1["classes"])
    m.add("x", instseg_ap_ref.point_tables(s0["masks"], s0["ids"], valid), s0["scores"], s0["classes"])
    ref = instseg_ap_ref.ap_from_tables([(instseg_ap_ref.point_tables(s0["masks"], s0["ids"], valid), s0["scores"],
                                          s0["classes"])], valid)
    assert len(m) == 1
    assert np.array_equal(m.compute()[0], ref, equal_nan=True)


def test_group_and_small_instances_follow_the_restatement():
    """Label 0 valid in a hand-made table: ids below 1000 are groups (never matched, their overlap ignored -- twice when
    also small); overlap_tables refuses label 0, InstSegAP takes such tables as given."""
    K, ids = 3, np.array([5, 1003, 1004, 2001], dtype=np.int64)
    tab = dict(gt_ids=ids, gt_verts=np.array([300, 50, 400, 500]),
               inter=np.array([[150, 0, 0, 0], [40, 30, 0, 0], [0, 0, 390, 0]], dtype=np.int32),
               void=np.array([10, 60, 0]), pred_verts=np.array([160, 130, 400]))
    scores, classes = np.array([0.9, 0.8, 0.7], np.float32), np.array([0, 1, 1])
    m = InstSegAP.__new__(InstSegAP)
    m.valid_class_ids, m.class_labels = np.array([0, 1, 2]), ["g", "a", "b"]
    m.min_region_size, m.overlaps, m._index, m._scenes = 100, default_overlaps(), {0: 0, 1: 1, 2: 2}, {}
    m.add("s", tab, scores, classes)
    ref = instseg_ap_ref.ap_from_tables([(tab, scores, classes)], [0, 1, 2])
    assert np.array_equal(m.compute()[0], ref, equal_nan=True)


def test_argument_errors():
    with pytest.raises(ValueError):
        InstSegAP([2, 4], ["a"])
    with pytest.raises(ValueError):
        InstSegAP([0, 4], ["a", "b"])
    with pytest.raises(ValueError):
        InstSegAP([4, 4], ["a", "b"])


def _constant_labels():
    tree = ast.parse(open(os.path.join(REF, "data", "datasets", "constant.py")).read())
    vals = {}
    for n in tree.body:
        if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id in ("VALID_CLASS_IDS_200",
                                                                                                    "CLASS_LABELS_200"):
            vals[n.targets[0].id] = ast.literal_eval(n.value)
    return vals["VALID_CLASS_IDS_200"], vals["CLASS_LABELS_200"]


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_integration_label_lists_equal_the_captured_ones():
    """INTEGRATION.md derives the evaluator's lists from data/datasets/constant.py: the 200-class lists without wall and floor."""
    ids, names = _constant_labels()
    pairs = [(i, n) for i, n in zip(ids, names) if n not in ("wall", "floor")]
    z = np.load(F23)
    assert len(pairs) == 198
    assert [p[0] for p in pairs] == [int(x) for x in z["valid_class_ids"]]
    assert [p[1] for p in pairs] == [str(x) for x in z["class_labels"]]


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_regenerated_fixture_matches(tmp_path):
    out = tmp_path / "F23.npz"
    subprocess.run([sys.executable, os.path.join(util.GOLDEN, "make_golden_instseg_ap.py"), "--out", str(out)], check=True,
                   capture_output=True)
    a, b = np.load(F23), np.load(out)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
