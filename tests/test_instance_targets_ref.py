"""CPU: the numpy restatement of the instance-target rules (tests/instance_targets_ref.py) on hand-written tiny scenes, so
that the specification the GPU kernels are compared with is itself pinned."""
import numpy as np

from tests import instance_targets_ref as R


def _eq(got, want, dtype):
    want = np.asarray(want, dtype=dtype)
    return got.dtype == dtype and got.shape == want.shape and np.array_equal(got, want)


def test_first_occurrence_decides_the_label():
    # instance 3: first point (index 1) carries 7, a later one 9; instance 5: first point carries 4 although most carry 8
    ids, lab, seg, full = R.instance_targets([5, 3, 3, 5, 5], [4, 7, 9, 8, 8], [0, 1, 1, 0, 2])
    assert _eq(ids, [3, 5], np.int64) and _eq(lab, [7, 4], np.int64)
    assert _eq(seg, [[0, 1, 0], [1, 0, 1]], bool)
    assert _eq(full, [[0, 1, 1, 0, 0], [1, 0, 0, 1, 1]], bool)


def test_first_occurrence_inside_the_filter_drops_the_instance():
    # instance 1's first point has class 2 (filtered) although the others have 6; instance 0's first point has 6, a later one 2
    ids, lab, seg, full = R.instance_targets([1, 0, 1, 0], [2, 6, 6, 2], [0, 0, 1, 1])
    assert _eq(ids, [0], np.int64) and _eq(lab, [6], np.int64)
    assert _eq(seg, [[1, 1]], bool) and _eq(full, [[0, 1, 0, 1]], bool)


def test_gap_in_the_ids_keeps_ascending_rows():
    ids, lab, seg, full = R.instance_targets([40, 2, 40, 7], [5, 5, 5, 9], [3, 0, 0, 3])
    assert _eq(ids, [2, 7, 40], np.int64) and _eq(lab, [5, 9, 5], np.int64)
    assert seg.shape == (3, 4) and _eq(seg, [[1, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1]], bool)
    assert _eq(full, [[0, 1, 0, 0], [0, 0, 0, 1], [1, 0, 1, 0]], bool)


def test_minus_one_present_and_absent():
    ids, lab, seg, full = R.instance_targets([-1, 0, -1, 1], [-100, 3, 3, 4], [0, 0, 1, 1])
    assert _eq(ids, [0, 1], np.int64) and _eq(lab, [3, 4], np.int64)
    assert _eq(seg, [[1, 0], [0, 1]], bool) and _eq(full, [[0, 1, 0, 0], [0, 0, 0, 1]], bool)
    ids, lab, seg, full = R.instance_targets([0, 1], [3, 4], [0, 0])
    assert _eq(ids, [0, 1], np.int64) and _eq(seg, [[1], [1]], bool) and _eq(full, [[1, 0], [0, 1]], bool)
    # only -1: no instance, the shapes keep S and P
    ids, lab, seg, full = R.instance_targets([-1, -1, -1], [5, 5, 5], [0, 4, 1])
    assert ids.shape == (0,) and ids.dtype == np.int64 and lab.shape == (0,) and seg.shape == (0, 5) and full.shape == (0, 3)


def test_filtered_class_and_custom_filter():
    args = ([0, 1, 2, 3], [0, 2, 1, -100], [0, 1, 2, 3])
    ids, lab, seg, full = R.instance_targets(*args)
    assert _eq(ids, [2, 3], np.int64) and _eq(lab, [1, -100], np.int64)
    assert _eq(seg, [[0, 0, 1, 0], [0, 0, 0, 1]], bool) and _eq(full, [[0, 0, 1, 0], [0, 0, 0, 1]], bool)
    ids, lab, _seg, _full = R.instance_targets(*args, filter_out_classes=(-100, 1))
    assert _eq(ids, [0, 1], np.int64) and _eq(lab, [0, 2], np.int64)
    ids, _lab, _seg, _full = R.instance_targets(*args, filter_out_classes=())
    assert _eq(ids, [0, 1, 2, 3], np.int64)


def test_segment_shared_by_two_instances():
    ids, lab, seg, full = R.instance_targets([0, 1, 0, 1, -1], [3, 4, 3, 4, 3], [1, 1, 0, 2, 1])
    assert _eq(ids, [0, 1], np.int64)
    assert _eq(seg, [[1, 1, 0], [0, 1, 1]], bool), "segment 1 belongs to both instances (and to the unlabelled point)"
    assert seg.sum(1).tolist() == [2, 2] and full.sum(1).tolist() == [2, 2]


def test_collate_gt_keys():
    t = R.batch_targets([[0, 1, 1], [-1, 4]], [[3, 4, 4], [5, 6]], [[0, 1, 2], [0, 0]])
    assert [len(i) for i in t["instance_ids"]] == [2, 1] and [m.shape for m in t["segment_masks"]] == [(2, 3), (1, 1)]
    gt = R.collate_gt(t["instance_labels"], t["segment_masks"])
    assert _eq(gt["target_labels"], [[3, 4], [6, -100]], np.int64)
    assert _eq(gt["target_masks"], [[[1, 0, 0], [0, 1, 1]], [[1, 0, 0], [0, 0, 0]]], np.float32)
    assert _eq(gt["offline_attn_mask"], [[[0, 1, 1], [1, 0, 0]], [[0, 1, 1], [1, 1, 1]]], bool)
    assert _eq(gt["target_masks_pad_masks"], [[[1, 1, 1], [1, 1, 1]], [[1, 0, 0], [0, 0, 0]]], bool)
