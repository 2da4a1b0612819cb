"""GPU: overlap tables (pq3d_amd.instseg_ap.overlap_tables, csrc/instseg_ap.hip) equal the point-level restatement
tests/instseg_ap_ref.py exactly; F23 (the reference's own mask AP, tests/golden/make_golden_instseg_ap.py) is reproduced
bit for bit through the GPU tables and InstSegAP; GT boxes (gt_boxes, csrc/instseg.hip) have exact extents and centers
within rtol 1e-5."""
import os

import numpy as np
import pytest
import torch

from pq3d_amd import synth
from pq3d_amd.instseg_ap import InstSegAP, gt_boxes, overlap_tables
from tests import instseg_ap_ref, util
from tests.test_instseg_ap_ref import assert_averages, load_f23

pytestmark = pytest.mark.gpu
DEV = "cuda"
F22 = os.path.join(util.GOLDEN, "F22_instseg_predict.npz")
VALID = (2, 3, 5, 7, 9, 14, 1191)


def _tables(masks, ids, valid):
    return overlap_tables([torch.from_numpy(m).to(DEV) for m in masks], [torch.from_numpy(i).to(DEV) for i in ids], valid)


def _assert_tables(got, ref, what=""):
    for k in ("gt_ids", "gt_verts", "inter", "void", "pred_verts"):
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k].astype(np.int64), ref[k].astype(np.int64)), (what, k)


def _scene(seed, P, K, G, labels=(2, 5, 7, 1191), invalid=(1, 4)):
    m, i, _s, _c = synth.instseg_ap_scene(seed, P=P, K=K, G=G, labels=labels, invalid_labels=invalid,
                                           min_inst=1 if P < 2000 else 20)
    return m, i


def test_f23_tables_and_ap_end_to_end():
    z, scenes = load_f23()
    valid, labels = z["valid_class_ids"], [str(x) for x in z["class_labels"]]
    tabs = [_tables([s["masks"]], [s["ids"]], valid)[0] for s in scenes]    # the F23 scenes differ in K: one call each
    m = InstSegAP(valid, labels)
    for s, t in zip(scenes, tabs):
        _assert_tables(t, instseg_ap_ref.point_tables(s["masks"], s["ids"], valid), s["name"])
        m.add(s["name"], t, s["scores"], s["classes"])
    ap, avgs = m.compute()
    assert np.array_equal(ap, z["ap"], equal_nan=True)
    assert_averages(avgs, z, labels)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_ragged_batches_match_restatement(B):
    rng = np.random.default_rng(B)
    P = [int(x) for x in rng.integers(1, 3000, B)]
    P[0] = 1 if B > 1 else 257                              # one point; chunk-unaligned sizes elsewhere
    K = [1, 37, 100][B % 3]
    sc = [_scene(10 * B + b, P[b], K, max(1, min(12, P[b] // 40))) for b in range(B)]
    got = _tables([s[0] for s in sc], [s[1] for s in sc], VALID)
    for b, (m, i) in enumerate(sc):
        _assert_tables(got[b], instseg_ap_ref.point_tables(m, i, VALID), f"B={B} scene {b}")


@pytest.mark.parametrize("K", [1, 1024, 1023])
def test_k_extremes(K):
    sc = [_scene(70 + K % 7, 1500, K, 10), _scene(71, 700, K, 5)]
    got = _tables([s[0] for s in sc], [s[1] for s in sc], VALID)
    for b, (m, i) in enumerate(sc):
        _assert_tables(got[b], instseg_ap_ref.point_tables(m, i, VALID), f"K={K} scene {b}")


def test_void_only_and_gt_less_scenes():
    rng = np.random.default_rng(5)
    m0 = rng.random((600, 20)) < 0.3
    i0 = np.where(rng.random(600) < 0.5, 0, 4001).astype(np.int64)        # unlabeled + invalid label only
    m1, i1 = _scene(6, 900, 20, 0)
    m2, i2 = _scene(7, 1100, 20, 8)
    got = _tables([m0, m1, m2], [i0, i1, i2], VALID)
    for b, (m, i) in enumerate(((m0, i0), (m1, i1), (m2, i2))):
        _assert_tables(got[b], instseg_ap_ref.point_tables(m, i, VALID), f"scene {b}")
    assert got[0]["gt_ids"].size == 0 and np.array_equal(got[0]["void"], m0.sum(0))


def test_4096_instances_in_one_scene():
    rng = np.random.default_rng(8)
    P, K = 60_000, 40
    labs = np.array(VALID)
    inst = labs[rng.integers(0, len(labs), 4096)] * 1000 + rng.integers(1, 1000, 4096)
    inst = np.unique(inst)
    while inst.size < 4096:
        inst = np.unique(np.concatenate([inst, labs[rng.integers(0, len(labs), 64)] * 1000 + rng.integers(1, 1000, 64)]))
    inst = inst[:4096]
    ids = np.concatenate([inst, inst[rng.integers(0, 4096, P - 4096)]])
    ids[rng.random(P) < 0.1] = 0
    ids[:4096] = inst
    masks = rng.random((P, K)) < 0.2
    got = _tables([masks], [ids], VALID)[0]
    assert got["gt_ids"].size == 4096
    _assert_tables(got, instseg_ap_ref.point_tables(masks, ids, VALID), "4096 instances")


def test_batch_equals_single_calls_and_reruns_are_bit_identical():
    sc = [_scene(90 + b, 800 + 313 * b, 64, 9) for b in range(4)]
    a = _tables([s[0] for s in sc], [s[1] for s in sc], VALID)
    again = _tables([s[0] for s in sc], [s[1] for s in sc], VALID)
    for b in range(4):
        one = _tables([sc[b][0]], [sc[b][1]], VALID)[0]
        for k in a[b]:
            assert np.array_equal(a[b][k], one[k]) and np.array_equal(a[b][k], again[b][k]), (b, k)


def test_tables_from_instance_prediction_masks():
    """The device masks of instance_predictions (F22 inputs, views into one buffer) give the same tables as their host copy."""
    from pq3d_amd.instseg import instance_predictions
    z = np.load(F22)
    name = "k100"
    B = int(z[f"{name}/B"])
    keys = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps", "raw_coordinates")
    maps = {k: [torch.from_numpy(z[f"{name}/{b}/{k}"]).to(torch.float32 if k == "raw_coordinates" else torch.int64).to(DEV)
                for b in range(B)] for k in keys}
    recs = instance_predictions(torch.from_numpy(z[f"{name}/pred_logits"]).to(DEV),
                                torch.from_numpy(z[f"{name}/pred_masks"]).to(DEV), *[maps[k] for k in keys], topk_per_scene=100)
    rng = np.random.default_rng(3)
    ids = [torch.from_numpy(np.where(rng.random(r["masks"].shape[0]) < 0.2, 0,
                                     rng.choice([2001, 2002, 5003, 1191004, 4005], r["masks"].shape[0]))).to(DEV) for r in recs]
    dev_t = overlap_tables([r["masks"] for r in recs], ids, VALID)
    host = [r["masks"].cpu() for r in recs]
    host_t = overlap_tables([h.to(DEV) for h in host], ids, VALID)
    for b in range(B):
        for k in dev_t[b]:
            assert np.array_equal(dev_t[b][k], host_t[b][k]), (b, k)
        _assert_tables(dev_t[b], instseg_ap_ref.point_tables(host[b].numpy(), ids[b].cpu().numpy(), VALID), f"F22 scene {b}")


def test_gt_boxes_match_reference_and_float64():
    z, scenes = load_f23()
    got = gt_boxes([torch.from_numpy(s["full_masks"]).to(DEV) for s in scenes],
                   [torch.from_numpy(s["coords"]).to(DEV) for s in scenes])
    again = gt_boxes([torch.from_numpy(s["full_masks"]).to(DEV) for s in scenes],
                     [torch.from_numpy(s["coords"]).to(DEV) for s in scenes])
    for b, (s, g) in enumerate(zip(scenes, got)):
        boxes, valid = g["boxes"].cpu().numpy(), g["valid"].cpu().numpy()
        assert torch.equal(g["boxes"], again[b]["boxes"]) and torch.equal(g["valid"], again[b]["valid"])
        ref, ref_valid = instseg_ap_ref.gt_boxes_f64(s["full_masks"], s["coords"])
        assert np.array_equal(valid, ref_valid) and not valid[-1], "the last row is empty"
        assert (boxes[~valid] == 0).all()
        assert np.array_equal(boxes[valid, 3:], ref[valid, 3:].astype(np.float32))
        np.testing.assert_allclose(boxes[valid, :3], ref[valid, :3], rtol=1e-5, atol=1e-6)
        rows = s["bbox_rows"]
        assert np.array_equal(boxes[rows, 3:], s["bbox_gt"][:, 3:])
        np.testing.assert_allclose(boxes[rows, :3], s["bbox_gt"][:, :3], rtol=1e-5, atol=1e-6)


def test_gt_boxes_large_rows():
    rng = np.random.default_rng(4)
    P = 20_000                                              # several 4096-point chunks per row, last one partial
    fm = rng.random((5, P)) < np.array([0.5, 0.01, 0.0, 1.0, 0.0001])[:, None]
    xyz = (rng.standard_normal((P, 3)) * 4).astype(np.float32)
    g = gt_boxes([torch.from_numpy(fm).to(DEV)], [torch.from_numpy(xyz).to(DEV)])[0]
    ref, ref_valid = instseg_ap_ref.gt_boxes_f64(fm, xyz)
    boxes = g["boxes"].cpu().numpy()
    assert np.array_equal(g["valid"].cpu().numpy(), ref_valid)
    assert np.array_equal(boxes[ref_valid, 3:], ref[ref_valid, 3:].astype(np.float32))
    np.testing.assert_allclose(boxes[ref_valid, :3], ref[ref_valid, :3], rtol=1e-5, atol=1e-6)


def test_argument_errors():
    m = torch.zeros(10, 4, dtype=torch.bool, device=DEV)
    i = torch.zeros(10, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        overlap_tables([m], [torch.full((10,), -1, dtype=torch.int64, device=DEV)], VALID)    # negative id
    with pytest.raises(ValueError):
        overlap_tables([m], [i[:9]], VALID)                                                    # P mismatch
    with pytest.raises(ValueError):
        overlap_tables([m.to(torch.uint8)], [i], VALID)                                        # dtype
    with pytest.raises(ValueError):
        overlap_tables([m], [i.int()], VALID)
    with pytest.raises(ValueError):
        overlap_tables([m.cpu()], [i.cpu()], VALID)                                            # device
    with pytest.raises(ValueError):
        overlap_tables([torch.zeros(10, 1025, dtype=torch.bool, device=DEV)], [i], VALID)      # K > 1024
    with pytest.raises(ValueError):
        overlap_tables([torch.zeros(10, 0, dtype=torch.bool, device=DEV)], [i], VALID)         # K = 0
    with pytest.raises(ValueError):
        overlap_tables([m, torch.zeros(5, 3, dtype=torch.bool, device=DEV)], [i, i[:5]], VALID)  # K differs
    with pytest.raises(ValueError):
        overlap_tables([m], [i], (0, 2))                                                       # label 0
    with pytest.raises(ValueError):
        gt_boxes([m.T.contiguous()], [torch.zeros(9, 3, device=DEV)])                           # P mismatch
