"""The numpy restatement of the grounding-batch preparation (tests/object_prep_ref.py, the specification of
pq3d_amd/objects.py): its sampling rule by its own properties, and its boxes, match tables and _obj_processing_post against
fixture F27 (the reference's own functions on a tiny scan, tests/golden/make_object_golden.py)."""
import os

import numpy as np
import pytest

from tests import object_prep_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F27_object_prep.npz")
KEYS = [(0, 0, 0), (1234567890123, 3, 7), (-5, 127, 79)]          # (seed, item, slot)


@pytest.fixture(scope="module")
def z():
    return dict(np.load(GOLDEN))


def test_feistel_is_a_bijection_for_every_small_n():
    for n in range(1, 301):
        assert 4 ** (R.feistel_bits(n) // 2) >= n and (n < 2 or 4 ** (R.feistel_bits(n) // 2) < 4 * n)
        for seed, item, slot in KEYS:
            k0, k1 = R.object_key(seed, item, slot)
            v, steps, capped = R.perm(n, k0, k1, np.arange(n))
            assert not capped and steps < R.WALK_CAP
            assert np.array_equal(np.sort(v), np.arange(n)), (n, seed)


def test_first_draws_distinct_at_power_of_two_edges():
    num_points = 1024
    for k in range(1, 21):
        for n in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            for seed, item, slot in KEYS:
                k0, k1 = R.object_key(seed, item, slot)
                m = min(n, num_points)
                v, steps, capped = R.perm(n, k0, k1, np.arange(m))
                assert not capped and steps < R.WALK_CAP
                assert v.min() >= 0 and v.max() < n and len(np.unique(v)) == m, (n, seed)


def test_sample_indices_with_and_without_replacement_and_keys_differ():
    a, _ = R.sample_indices(5000, 64, 11, 0, 0)
    assert len(np.unique(a)) == 64 and a.max() < 5000
    b, _ = R.sample_indices(10, 64, 11, 0, 0)                   # fewer points than draws: with replacement
    assert b.min() >= 0 and b.max() < 10 and len(np.unique(b)) > 5
    assert np.array_equal(a, R.sample_indices(5000, 64, 11, 0, 0)[0])
    for other in ((12, 0, 0), (11, 1, 0), (11, 0, 1), (11 + (1 << 32), 0, 0)):
        assert not np.array_equal(a, R.sample_indices(5000, 64, *other)[0])
    assert np.array_equal(R.sample_indices(1, 8, 3, 0, 0)[0], np.zeros(8))
    assert np.array_equal(np.sort(R.sample_indices(64, 64, 3, 0, 0)[0]), np.arange(64))


def test_bank_and_boxes_equal_the_reference(z):
    ids = R.build_object_bank([z["points"]], point2instance=[z["point2instance"]], instance_ids=[z["instance_ids"]])
    keep = [k for k, i in enumerate(z["instance_ids"]) if (z["point2instance"] == i).any()]
    assert ids["source_row"].tolist() == keep and len(keep) < len(z["instance_ids"])
    assert np.array_equal(ids["box_center"], z["gt_center"]) and np.array_equal(ids["box_size"], z["gt_size"])
    for o, k in enumerate(keep):
        pts = ids["order"][ids["entry_offsets"][o]:ids["entry_offsets"][o + 1]]
        assert np.array_equal(pts, np.nonzero(z["point2instance"] == z["instance_ids"][k])[0])
    ms = R.build_object_bank([z["points"]], masks=[z["masks"]])
    assert ms["source_row"].tolist() == [k for k in range(len(z["masks"])) if z["masks"][k].any()]
    assert np.array_equal(ms["box_center"], z["pred_center"]) and np.array_equal(ms["box_size"], z["pred_size"])


def test_match_tables_equal_the_reference(z):
    matched, i25, i50 = R.match_boxes(z["gt_center"], z["gt_size"], z["pred_center"], z["pred_size"])
    assert np.array_equal(matched, z["matched"]) and np.array_equal(i25, z["iou25"]) and np.array_equal(i50, z["iou50"])
    m0, a0, b0 = R.match_boxes(z["gt_center"], z["gt_size"], z["pred_center"][:0], z["pred_size"][:0])
    assert (m0 == -1).all() and a0.shape == (len(matched), 0) == b0.shape


def _ulp_f32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def test_values_within_one_ulp_of_the_float64_reference(z):
    """The restatement rounds the float64 result to fp32 once; the reference's float64 sum order is not pinned, so each
    element may differ from fp32(reference) by the one final rounding: 1 fp32 ulp."""
    for k in range(z["sample_rows"].shape[0]):
        fts, locs, boxes = R.object_values(z["sample_rows"][k])
        for got, want in ((fts, z["f64_fts"][k]), (locs, z["f64_locs"][k]), (boxes, z["f64_boxes"][k])):
            assert got.dtype == np.float32
            assert (np.abs(got.astype(np.float64) - want) <= _ulp_f32(want)).all()


def test_rotated_values_no_worse_than_the_fp32_reference(z):
    """With a rotation the reference computes in fp32; against its own float64 evaluation the restatement's largest error
    must not exceed the fp32 reference's."""
    for name in ("fts", "locs", "boxes"):
        mine = np.stack([dict(zip(("fts", "locs", "boxes"), R.object_values(z["sample_rows"][k], z["rotation"])))[name]
                         for k in range(z["sample_rows"].shape[0])])
        yard = z["f64rot_" + name]
        e_mine = np.abs(mine.astype(np.float64) - yard).max()
        e_ref = np.abs(z["f32rot_" + name].astype(np.float64) - yard).max()
        assert e_mine <= e_ref, (name, e_mine, e_ref)
        assert (np.abs(mine.astype(np.float64) - yard) <= _ulp_f32(yard)).all()


def test_degenerate_object_keeps_the_clamp():
    rows = np.tile(np.array([[1.5, -2.0, 0.25, 0.1, 0.2, 0.3]], dtype=np.float32), (16, 1))
    fts, locs, boxes = R.object_values(rows)
    assert np.isfinite(fts).all() and (fts[:, :3] == 0).all() and (locs[3:] == 0).all()
    assert np.array_equal(locs[:3], rows[0, :3]) and np.array_equal(boxes[:3], rows[0, :3])


def test_ground_labels_forms():
    off = np.array([0, 4, 9])
    soi = np.array([1, 0])
    sel = np.array([[4, 0, 2, -1], [3, 1, -1, -1]])
    tg = np.array([[2, 4, -1], [0, -1, -1]])
    a, b, c, err = R.ground_labels(off, soi, sel, tg)
    assert err == 0 and a.tolist() == [[1, 0, 1, 0], [0, 0, 0, 0]] and np.array_equal(a, b) and np.array_equal(a, c)
    # pred form: scan 0 has 2 GT objects and 4 predictions, scan 1 has 3 GT objects and 5 predictions
    m0 = (np.array([1, 3]), np.eye(2, 4, dtype=np.uint8), np.zeros((2, 4), dtype=np.uint8))
    i25 = np.zeros((3, 5), dtype=np.uint8); i25[0, [0, 2]] = 1; i25[2, 3] = 1
    i50 = np.zeros((3, 5), dtype=np.uint8); i50[0, 2] = 1
    m1 = (np.array([2, 1, 3]), i25, i50)
    a, b, c, err = R.ground_labels(off, soi, sel, np.array([[0, 2, -1], [1, -1, -1]]), match=[m0, m1])
    # item 0 (scan 1): matched 2 -> slot 2; matched 3 is not selected: no slot.  item 1 (scan 0): matched 3 -> slot 0
    assert err == 0 and a.tolist() == [[0, 0, 1, 0], [1, 0, 0, 0]]
    assert b.tolist() == [[0, 1, 1, 0], [0, 1, 0, 0]] and c.tolist() == [[0, 0, 1, 0], [0, 0, 0, 0]]
    assert R.ground_labels(off, np.array([2, 0]), sel, tg)[3] == R.ERR_SCENE
    assert R.ground_labels(off, soi, np.array([[5, 0, 2, -1], [3, 1, -1, -1]]), tg)[3] == R.ERR_SELECTED
    assert R.ground_labels(off, soi, sel, np.array([[2, 5, -1], [0, -1, -1]]))[3] == R.ERR_TARGET
