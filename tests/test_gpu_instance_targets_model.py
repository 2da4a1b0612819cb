"""GPU: the derived training targets where they are consumed: prepare_instseg_batch(point2instance=, point2semantic=), the
device set criterion on padded_instance_targets, InstSegLoss 'direct' on the 'gt' collate keys and instseg_ap.gt_boxes on the
new full masks, each against the numpy restatement tests/instance_targets_ref.py (exact comparisons)."""
import functools

import numpy as np
import pytest
import torch

from tests import instance_targets_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = 0.02
NQ, NCLS = 12, 20
W = dict(cost_class=2.0, cost_mask=5.0, cost_dice=2.0)
WD = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _scenes():
    """Two scenes of about 3000 points on a floor and a wall, 40 patch segments (every id present), about 8 instances that
    cut across the patches, unlabelled (-1) points, one instance of a filtered class, labels mixed inside an instance."""
    out = []
    for b, P in enumerate((3100, 2900)):
        r = np.random.default_rng([b, 77])
        u, w = r.random(P), r.random(P)
        wall = r.random(P) < 0.3
        xyz = np.where(wall[:, None], np.stack([u * 1.6, np.zeros(P), w * 0.6], 1), np.stack([u * 1.6, w * 1.0, np.zeros(P)], 1))
        xyz = (xyz + r.normal(0, 0.004, (P, 3))).astype(np.float32)
        seg = (np.minimum((u * 8).astype(np.int64), 7) * 5 + np.minimum((w * 5).astype(np.int64), 4)).astype(np.int64)
        seg[:40] = np.arange(40)
        inst = np.minimum((u * 9 + w * 0.7).astype(np.int64), 9) * (2 if b else 1)        # scene 1: ids with gaps
        inst[r.random(P) < 0.1] = -1
        own = np.array([5, 2, 7, 1, 19, 3, 3, 11, 4, 6])[inst // (2 if b else 1)]          # the second instance is filtered
        sem = np.where(r.random(P) < 0.2, r.integers(0, NCLS, P), own).astype(np.int64)
        sem[inst == -1] = -100
        first = {int(i): int(np.flatnonzero(inst == i)[0]) for i in np.unique(inst)}
        for i, p in first.items():                                                         # labels inside [0, NCLS) decide
            if i >= 0:
                sem[p] = own[p]
        out.append(dict(xyz=xyz, feat=np.concatenate([r.random((P, 3)).astype(np.float32), xyz], 1), seg=seg, inst=inst, sem=sem))
    return out


@functools.lru_cache(maxsize=None)
def _want():
    sc = _scenes()
    return R.batch_targets([s["inst"] for s in sc], [s["sem"] for s in sc], [s["seg"] for s in sc])


def _d(k):
    return [_dev(s[k]) for s in _scenes()]


def _eq(t, a):
    return t.dtype == torch.from_numpy(np.asarray(a)).dtype and tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), a)


def test_the_scenes_are_what_the_tests_assume():
    want = _want()
    assert [len(i) for i in want["instance_ids"]] == [9, 9] and want["instance_ids"][1].max() == 18
    assert all(m.shape[1] == 40 for m in want["segment_masks"]) and all((l >= 0).all() and (l < NCLS).all() for l in want["instance_labels"])


def test_prepare_instseg_batch_derives_the_targets():
    from pq3d_amd import scene
    want = _want()
    old = scene.prepare_instseg_batch(_d("xyz"), _d("feat"), _d("seg"), VS, NQ, point2instance=_d("inst"),
                                      instance_ids=[_dev(i) for i in want["instance_ids"]])
    new = scene.prepare_instseg_batch(_d("xyz"), _d("feat"), _d("seg"), VS, NQ, point2instance=_d("inst"), point2semantic=_d("sem"))
    assert sorted(set(new) - set(old)) == ["full_masks", "instance_ids", "instance_labels", "segment_masks"]
    for k in old:
        a, b = old[k], new[k]
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else all(torch.equal(x, y) for x, y in zip(a, b)), k
    for k in ("instance_ids", "instance_labels", "segment_masks", "full_masks"):
        assert all(_eq(new[k][b], want[k][b]) for b in range(2)), k
    gtq = scene.prepare_instseg_batch(_d("xyz"), _d("feat"), _d("seg"), VS, NQ, point2instance=_d("inst"), point2semantic=_d("sem"),
                                      query_sample_strategy="gt", offline_mask_source="gt")
    assert torch.equal(gtq["query_locs"], old["obj_center"]) and torch.equal(gtq["obj_center"], old["obj_center"])
    ref = R.collate_gt(want["instance_labels"], want["segment_masks"])
    assert sorted(set(gtq) - set(new)) == sorted(ref)
    for k, v in ref.items():
        assert _eq(gtq[k], v), k
    with pytest.raises(NotImplementedError, match="pred"):
        scene.prepare_instseg_batch(_d("xyz"), _d("feat"), _d("seg"), VS, NQ, point2instance=_d("inst"), point2semantic=_d("sem"),
                                    offline_mask_source="pred")
    with pytest.raises(ValueError):
        scene.prepare_instseg_batch(_d("xyz"), _d("feat"), _d("seg"), VS, NQ, offline_mask_source="gt")
    # a filter that keeps everything changes the derived instances (and their centres)
    every = scene.prepare_instseg_batch(_d("xyz"), _d("feat"), _d("seg"), VS, NQ, point2instance=_d("inst"), point2semantic=_d("sem"),
                                        filter_out_classes=())
    assert [len(i) for i in every["instance_ids"]] == [10, 10] and tuple(every["obj_center"].shape) == (2, 10, 3)


def _predictions(Nq, n_layers=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    masks = [torch.randn(2, 40, Nq, generator=g).to(DEV) for _ in range(n_layers)]
    logits = [torch.randn(2, Nq, NCLS + 1, generator=g).to(DEV) for _ in range(n_layers)]
    return masks, logits


def test_device_set_criterion_on_padded_instance_targets():
    from pq3d_amd import scene
    from pq3d_amd.losses import HungarianMatcher, SetCriterion
    want = _want()
    crit = SetCriterion(num_classes=NCLS, matcher=HungarianMatcher(num_points=-1, ignore_label=-100, **W), weight_dict=WD,
                        losses=["labels", "masks"], num_points=-1, class_weights=-1, ignore_label=-100, matching="device")
    masks, logits = _predictions(NQ)
    ours, err = scene.padded_instance_targets(_d("inst"), _d("sem"), _d("seg"), 40, 11)
    scene.check_instance_targets(err)
    host = SetCriterion.pad_targets([torch.from_numpy(l) for l in want["instance_labels"]],
                                    [torch.from_numpy(m) for m in want["segment_masks"]], 40, 11)
    la, ia = crit(masks, logits, targets=ours)
    ia = [t.clone() for t in ia]
    lb, ib = crit(masks, logits, targets=host)
    crit.check()
    assert sorted(la) == sorted(lb) and len(la) == 6
    for k in la:
        assert torch.isfinite(la[k]) and torch.equal(la[k], lb[k]), k
    assert all(torch.equal(x, y) for x, y in zip(ia, ib))


def test_instseg_loss_direct_on_the_gt_keys():
    from pq3d_amd import scene
    from pq3d_amd.losses import InstSegLoss
    from pq3d_amd.model import Cfg
    want = _want()
    cfg = Cfg({"model": {"InstSegLoss": {
        "criterion_type": "direct", "matcher": dict(num_points=-1, ignore_label=-100, **W),
        "criterion": dict(num_classes=NCLS, losses=["labels", "masks"], num_points=-1, class_weights=-1, ignore_label=-100)}}})
    batch = scene.prepare_instseg_batch(_d("xyz"), _d("feat"), _d("seg"), VS, NQ, point2instance=_d("inst"), point2semantic=_d("sem"),
                                        query_sample_strategy="gt", offline_mask_source="gt")
    masks, logits = _predictions(9)                      # 'gt' queries: query i <-> instance i
    assert tuple(batch["query_locs"].shape) == (2, 9, 3)
    dd = dict(batch, predictions_mask=masks, predictions_class=logits)
    total, losses = InstSegLoss(cfg)(dd)
    ref = {k: _dev(v) for k, v in R.collate_gt(want["instance_labels"], want["segment_masks"]).items()}
    total_ref, losses_ref = InstSegLoss(cfg)(dict(ref, predictions_mask=masks, predictions_class=logits))
    assert torch.isfinite(total) and torch.equal(total, total_ref) and sorted(losses) == sorted(losses_ref)
    assert all(torch.equal(losses[k], losses_ref[k]) for k in losses)


def test_gt_boxes_accepts_the_new_full_masks():
    from pq3d_amd import instseg_ap, scene
    want = _want()
    t = scene.instance_targets(_d("inst"), _d("sem"), _d("seg"))
    ours = instseg_ap.gt_boxes(t["full_masks"], _d("xyz"))
    ref = instseg_ap.gt_boxes([_dev(m) for m in want["full_masks"]], _d("xyz"))
    for a, b in zip(ours, ref):
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
        assert bool(a["valid"].all())
