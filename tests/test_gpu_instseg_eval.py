"""GPU: pq3d_box_match (pq3d_amd.instseg_eval.box_match, csrc/instseg_box.hip) equals the loop-by-loop restatement
tests/instseg_eval_ref.py exactly -- flags and jmax equal, ovmax bit for bit -- on the F29 scenes and on seeded scenes at the
sizes where the kernel takes another path; BoxAP.compute and InstSegEval.record() reproduce F29 (the reference's own eval_det
and InstSegEval.record, tests/golden/make_golden_instseg_eval.py) bit for bit.  No tolerance anywhere: every output is an
integer or a float64 of a fixed operation order."""
import pickle

import numpy as np
import pytest
import torch

from pq3d_amd import _lib
from pq3d_amd import instseg_eval as IE
from pq3d_amd.instseg_eval import BoxAP, InstSegEval, box_match
from tests import instseg_eval_ref
from tests.test_instseg_eval_ref import (F29, IGNORE, assert_box_aps, assert_full_results, full_rows, load_box_cases,
                                         record_lists)

pytestmark = pytest.mark.gpu
DEV = "cuda"
THRESHOLDS = (0.25, 0.5)
T4 = (0.1, 0.25, 0.5, 0.75)


def _dev(scenes):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    preds = [dict(boxes=t(s["pboxes"]), classes=t(s["pclasses"]), scores=t(s["pscores"]), box_valid=t(s["pvalid"])) for s in scenes]
    gts = [dict(boxes=t(s["gboxes"]), labels=t(s["glabels"]), valid=t(s["gvalid"])) for s in scenes]
    return preds, gts


def _seeded(name, seed, K, G, ncls=5):
    """One scene in the stored layout: detections jittered around GT boxes (some with another class, some free), a few
    invalid rows on both sides; scores distinct inside the scene."""
    rng = np.random.default_rng([seed, K, G])
    box = lambda n: np.concatenate([rng.normal(size=(n, 3)) * 2, rng.random((n, 3)) + 0.2], 1).astype(np.float32)
    gb, gl = box(G), rng.integers(2, ncls + 2, G).astype(np.int64)
    pb, pc = box(K), rng.integers(2, ncls + 3, K).astype(np.int64)
    if G:
        src = rng.integers(0, G, K)
        near = rng.random(K) < 0.7
        jit = gb[src].copy()
        jit[:, :3] += (rng.normal(size=(K, 3)) * 0.08).astype(np.float32)
        jit[:, 3:] *= (1 + rng.normal(size=(K, 1)) * 0.1).astype(np.float32)
        pb[near] = jit[near]
        same = near & (rng.random(K) < 0.85)
        pc[same] = gl[src[same]]
    ps = rng.permutation(K).astype(np.float32) / np.float32(max(K, 1))
    pv, gv = rng.random(K) > 0.05, rng.random(G) > 0.05
    if K == 1:
        pv[:] = True
    return dict(name=name, pboxes=pb, pclasses=pc, pscores=ps, pvalid=pv, gboxes=gb, glabels=gl, grow_valid=gv, gvalid=gv)


def _check(scenes, thresholds):
    """box_match of the scenes in one call against the restatement."""
    preds, gts = _dev(scenes)
    m = box_match(preds, gts, thresholds)
    assert int(m["err"].item()) == 0
    ref = instseg_eval_ref.match_arrays(*record_lists(scenes), thresholds)
    ov, jm, fl = m["ovmax"].cpu().numpy(), m["jmax"].cpu().numpy(), m["flags"].cpu().numpy()
    for b, s in enumerate(scenes):
        a, e = int(m["koff"][b]), int(m["koff"][b + 1])
        rov, rjm, rfl = full_rows(ref[s["name"]], s)
        assert np.array_equal(fl[a:e], rfl), (s["name"], "flags")
        assert np.array_equal(jm[a:e], rjm), (s["name"], "jmax")
        assert np.array_equal(ov[a:e].view(np.int64), rov.view(np.int64)), (s["name"], "ovmax bits")
    return m


def test_f29_scenes_and_box_ap():
    z, scenes = load_box_cases()
    m = _check(scenes, THRESHOLDS)
    again = box_match(*_dev(scenes), THRESHOLDS)
    for k in ("ovmax", "jmax", "flags"):
        assert torch.equal(m[k].view(torch.uint8), again[k].view(torch.uint8)), k
    fl = m["flags"].cpu().numpy()
    ap = BoxAP(THRESHOLDS)
    for b, s in enumerate(scenes):
        f = fl[int(m["koff"][b]):int(m["koff"][b + 1])]
        ap.add(s["name"], s["pclasses"][s["pvalid"]], s["pscores"][s["pvalid"]], f[s["pvalid"]], s["glabels"][s["gvalid"]])
    assert_box_aps(*ap.compute(), z)


@pytest.mark.parametrize("K,G", [(1, 0), (1, 1), (63, 5), (64, 5), (65, 5), (257, 70), (1024, 300)])
def test_sizes_match_restatement(K, G):
    _check([_seeded("s", 7, K, G)], THRESHOLDS)


def test_more_gt_rows_than_one_tile_and_the_large_winner_table():
    """G = 4096 with 4 thresholds: eight staged tiles and the 64 KB winner table (the launch with more than 64 KB of LDS)."""
    _check([_seeded("s", 9, 6, 4096, ncls=40)], T4)
    _check([_seeded("s", 10, 40, 513, ncls=3)], THRESHOLDS)


@pytest.mark.parametrize("thresholds", [(0.25,), THRESHOLDS, T4])
def test_ragged_batch_with_an_empty_scene(thresholds):
    scenes = [_seeded("a", 11, 63, 5), _seeded("b", 12, 0, 0), _seeded("c", 13, 65, 7)]
    m = _check(scenes, thresholds)
    one = box_match(*_dev(scenes[2:]), thresholds)
    assert torch.equal(m["flags"][63:], one["flags"]) and torch.equal(m["jmax"][63:], one["jmax"])
    assert torch.equal(m["ovmax"][63:].view(torch.int64), one["ovmax"].view(torch.int64))


def test_equal_scores_go_to_the_lower_column():
    g = np.array([[0, 0, 0, 1, 1, 1]], np.float32)
    p = np.array([[0.05, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1], [0, 0.02, 0, 1, 1, 1]], np.float32)
    s = dict(name="t", pboxes=p, pclasses=np.full(3, 4, np.int64), pscores=np.full(3, 0.5, np.float32), pvalid=np.ones(3, bool),
             gboxes=g, glabels=np.array([4], np.int64), grow_valid=np.ones(1, bool), gvalid=np.ones(1, bool))
    m = _check([s], THRESHOLDS)
    assert m["flags"].cpu().tolist() == [3, 0, 0] and m["jmax"].cpu().tolist() == [0, 0, 0]
    s["pscores"] = np.array([0.5, 0.75, 0.5], np.float32)      # a higher score wins whatever the column
    assert _check([s], THRESHOLDS)["flags"].cpu().tolist() == [0, 3, 0]


def test_error_word_and_the_other_scenes():
    scenes = [_seeded("a", 21, 40, 6), _seeded("b", 22, 30, 5), _seeded("c", 23, 20, 4)]
    clean = box_match(*_dev(scenes), THRESHOLDS)
    assert int(clean["err"].item()) == 0
    k_nan = int(np.nonzero(scenes[1]["pvalid"])[0][0])
    for field, value, bit in (("pscores", np.nan, IE.ERR_NAN_SCORE), ("pboxes", np.inf, IE.ERR_PRED_BOX)):
        bad = [dict(s) for s in scenes]
        arr = bad[1][field].copy()
        if field == "pboxes":
            arr[k_nan, 4] = value
        else:
            arr[k_nan] = value
        bad[1][field] = arr
        m = box_match(*_dev(bad), THRESHOLDS)
        assert int(m["err"].item()) == bit
        k = 40 + k_nan
        assert m["flags"][k].item() == 0 and m["jmax"][k].item() == -1 and m["ovmax"][k].item() == -np.inf
        for rng_ in (slice(0, 40), slice(70, 90)):              # the other scenes are unchanged
            assert torch.equal(m["flags"][rng_], clean["flags"][rng_]) and torch.equal(m["jmax"][rng_], clean["jmax"][rng_])
            assert torch.equal(m["ovmax"][rng_].view(torch.int64), clean["ovmax"][rng_].view(torch.int64))
        with pytest.raises(ValueError):
            IE.check_errors(int(m["err"].item()))
    bad = [dict(s) for s in scenes]
    g = int(np.nonzero(bad[2]["gvalid"])[0][0])
    arr = bad[2]["gboxes"].copy()
    arr[g, 0] = -np.inf
    bad[2]["gboxes"] = arr
    m = box_match(*_dev(bad), THRESHOLDS)
    assert int(m["err"].item()) == IE.ERR_GT_BOX and not (m["jmax"][70:] == g).any()
    assert torch.equal(m["flags"][:70], clean["flags"][:70])


def test_limits_raise_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a launch was made")
    monkeypatch.setattr(_lib, "call", no_launch)
    ok = _seeded("a", 31, 4, 3)
    for K, G in ((1025, 3), (4, 4097)):
        big = _seeded("b", 32, K, G)
        with pytest.raises(ValueError):
            box_match(*_dev([ok, big]), THRESHOLDS)
    with pytest.raises(ValueError):
        box_match(*_dev([ok]), (0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError):
        box_match(*_dev([ok]), ())
    p, g = _dev([ok])
    with pytest.raises(ValueError):
        box_match([{k: v.cpu() for k, v in p[0].items()}], [{k: v.cpu() for k, v in g[0].items()}])
    p[0]["classes"] = p[0]["classes"].int()
    with pytest.raises(ValueError):
        box_match(p, g)


def test_capture_and_replay_on_static_buffers():
    batches = [[_seeded("a", 40 + i, 70, 9), _seeded("b", 50 + i, 33, 4)] for i in range(3)]
    preds, gts = _dev(batches[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        box_match(preds, gts, THRESHOLDS)                       # warm-up: the offset / threshold tensors of this shape
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m = box_match(preds, gts, THRESHOLDS)
    for scenes in batches[1:]:
        new_p, new_g = _dev(scenes)
        for dst, src in zip(preds + gts, new_p + new_g):
            for k in dst:
                dst[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        eager = box_match(new_p, new_g, THRESHOLDS)
        assert int(m["err"].item()) == 0
        assert torch.equal(m["flags"], eager["flags"]) and torch.equal(m["jmax"], eager["jmax"])
        assert torch.equal(m["ovmax"].view(torch.int64), eager["ovmax"].view(torch.int64))


# ---- InstSegEval.record() against the reference's whole record() dict ---------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    z = np.load(F29)
    B = int(z["full/B"])
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dt if dt is not None else torch.from_numpy(a).dtype).to(DEV)
    d = dict(predictions_class=[t(z["full/pred_logits"])], predictions_mask=[t(z["full/pred_masks"])],
             scan_id=[str(x) for x in z["full/scenes"]])
    for key in ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps"):
        d[key] = [t(z[f"full/{b}/{key}"], torch.int64) for b in range(B)]
    d["raw_coordinates"] = [t(z[f"full/{b}/raw_coordinates"]) for b in range(B)]
    d["gt_ids"] = [t(z[f"full/{b}/gt_ids"]) for b in range(B)]
    d["instance_labels"] = [t(z[f"full/{b}/instance_labels"]) for b in range(B)]
    d["full_masks"] = []
    for b in range(B):
        n, P = int(z[f"full/{b}/n_full"]), z[f"full/{b}/gt_ids"].shape[0]
        d["full_masks"].append(t(np.unpackbits(z[f"full/{b}/full_masks_packed"], count=n * P).reshape(n, P).astype(bool)))
    return z, d


def _evaluator(z):
    s = lambda k: [str(x) for x in z[k]]
    return InstSegEval(z["full/valid_class_ids"], s("full/class_labels"), id_map={int(k): int(v) for k, v in z["full/id_map"]},
                       class_names=dict(zip((int(i) for i in z["full/name_ids"]), s("full/names"))),
                       groups=dict(head=s("full/head"), common=s("full/common"), tail=s("full/tail")),
                       group_order=s("full/group_order"), topk_per_scene=int(z["full/topk"]))


def _part(d, sel):
    out = {}
    for k, v in d.items():
        if k in ("predictions_class", "predictions_mask"):
            out[k] = [v[0][sel]]
        else:
            out[k] = [v[b] for b in sel]
    return out


def test_record_reproduces_the_reference_record(full):
    z, d = full
    ev = _evaluator(z)
    ev.update(d)
    is_best, res = ev.record()
    assert is_best and res["best_result"] == res["all_ap"] == res["target_metric"]
    assert_full_results(res, z)
    assert len(ev.mask_ap) == 0 and len(ev.box_ap) == 0         # record() clears the per-scene state
    ev.update(d)                                                # a second run: the same bits, and no longer the best
    is_best2, res2 = ev.record()
    assert not is_best2
    assert_full_results(res2, z)


def test_two_updates_equal_one_and_records_round_trip(full):
    z, d = full
    ev = _evaluator(z)
    ev.update(_part(d, [0, 1]))
    ev.update(_part(d, [2]))
    ev.update(_part(d, [2]))                                    # a repeated scan_id replaces the scene
    other = _evaluator(z)
    other.extend(pickle.loads(pickle.dumps(ev.records())))
    assert_full_results(other.record()[1], z)
    assert_full_results(ev.record()[1], z)


def test_update_keeps_the_box_records_on_the_device(full, monkeypatch):
    z, d = full
    ev = _evaluator(z)
    ev.update(d)
    assert len(ev._pending) == 3 and len(ev.box_ap) == 0
    assert all(t.is_cuda for rec in ev._pending.values() for t in rec)
    with pytest.raises(NotImplementedError):
        ev.gather()
    with pytest.raises(NotImplementedError):
        InstSegEval(z["full/valid_class_ids"], [str(x) for x in z["full/class_labels"]], save=True)
    assert IGNORE == ev.ignore_label
