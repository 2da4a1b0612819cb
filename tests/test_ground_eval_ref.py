"""CPU: the numpy restatement tests/ground_eval_ref.py (what the GPU tests of csrc/ground.hip compare against) held against
the reference's own results in tests/golden/F28_ground_eval.npz (made by tests/golden/make_ground_eval_golden.py): IoU
matrices bit for bit, every count, pair and F1 equal, the loss and its gradient to float64 / float32 rounding."""
import os

import numpy as np
import pytest

from tests import ground_eval_ref as R

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F28_ground_eval.npz"))
EPS32 = float(np.finfo(np.float32).eps)


def test_bce_loss_and_gradient():
    x, y = Z["bce_x"], Z["bce_y"]
    assert np.isneginf(x).sum() >= 5 and (x == -100).any() and (x == -100.5).any() and (x == -1e4).any() and (x == 88).any()
    want = R.bce_logits_mean(x, y)
    # the reference returns float32 from both runs (its label.float()); the float64-logits run is float64 arithmetic rounded once
    assert abs(float(Z["bce_loss_f64"]) - want) <= 0.5 * EPS32 * want
    assert abs(float(Z["bce_loss_f32"]) - want) <= 4 * EPS32 * want
    g = R.bce_logits_grad(x, y)
    g64 = Z["bce_grad_f64"]
    assert g64.dtype == np.float64
    assert np.abs(g - g64).max() <= 1e-15
    assert np.array_equal(g == 0, g64 == 0) and (g[x < -100] == 0).all() and (g[x == -100] != 0).all()
    assert np.abs(g - Z["bce_grad_f32"]).max() <= 4 * EPS32 / x.size
    assert (Z["bce_grad_f32"][x < -100] == 0).all()      # (sigmoid(-100) / N underflows in fp32: more zeros than these)
    # weight and add fold in
    assert R.bce_logits_mean(x, y, 10.0, 0.25) == pytest.approx(10 * want + 0.25, rel=1e-15)
    assert np.isnan(R.bce_logits_mean([0.5, np.nan], [0, 0]))


def test_refer_counts_against_both_evaluators():
    x, tgt = Z["refer_logits"], Z["refer_tgt"]
    labels = np.stack([np.zeros_like(x), Z["refer_iou25"].astype(np.float32), Z["refer_iou50"].astype(np.float32)])
    flags = dict(is_multiple=Z["refer_is_multiple"], is_hard=Z["refer_is_hard"], is_view_dependent=Z["refer_is_view_dependent"])
    pred, hits, counts = R.refer_counts(x, labels, tgt, **flags)
    assert np.array_equal(pred, Z["refer_pred"])
    assert pred[1] == 0 and pred[2] == 3 and pred[3] == 4 and pred[4] == 2            # all -inf, a tie, one NaN, two NaNs
    for name, pairs in (("scanrefer", R.scanrefer_pairs(counts)), ("referit3d", R.referit3d_pairs(counts))):
        keys = [str(k) for k in Z[name + "_keys"]]
        assert list(pairs) == keys                                                    # the reference's keys in its order
        assert np.array_equal(np.array([pairs[k] for k in keys], dtype=np.float64), Z[name + "_pairs"])
    # the row form of tgt_object_id gives the same counts when every item has one target
    one_hot = np.zeros_like(x)
    one_hot[np.arange(len(x)), tgt[:, 0]] = 1
    labels[0] = one_hot
    p2, h2, c2 = R.refer_counts(x, labels, None, **flags)
    assert np.array_equal(c2, counts) and np.array_equal(h2, hits)
    # an item mask counts its items only
    mask = np.arange(len(x)) % 2 == 0
    _, hm, cm = R.refer_counts(x, labels, tgt, item_mask=mask, **flags)
    _, _, cs = R.refer_counts(x[mask], labels[:, mask], tgt[mask], **{k: v[mask] for k, v in flags.items()})
    assert np.array_equal(cm, cs) and np.array_equal((hm & 8) != 0, mask)


def test_iou_matrices_counts_and_f1():
    n_pred, n_gt = Z["f1_n_pred"], Z["f1_n_gt"]
    C = len(n_pred)
    assert C >= 35
    on25 = on50 = 0
    for c in range(C):
        P, G = int(n_pred[c]), int(n_gt[c])
        pred, gt = Z["f1_pred"][c, :P], Z["f1_gt"][c, :G]
        iou = R.iou_matrix(pred, gt)
        assert np.array_equal(iou.view(np.int32), Z["f1_iou"][c, :P, :G].view(np.int32)), f"case {c}"
        (tp25, tp50, p, g), _col = R.f1_counts(pred, gt)
        assert (p, g) == (P, G)
        f1 = R.f1_pair(tp25, tp50, P, G)
        assert np.array_equal(np.array(f1, dtype=np.float64), Z["f1_scores"][c]), f"case {c}"
        on25 += tp25
        on50 += tp50
    assert on25 > on50 > 0
    # the cases of the issue are there: empty sides, P < G, P > G, P = G, a zero-volume box, IoUs at the thresholds
    assert ((n_pred == 0) & (n_gt == 0)).any() and ((n_pred == 0) & (n_gt > 0)).any() and ((n_pred > 0) & (n_gt == 0)).any()
    assert (n_pred < n_gt).any() and (n_pred > n_gt).any() and ((n_pred == n_gt) & (n_pred > 1)).any()
    live_p = np.arange(Z["f1_pred"].shape[1])[None] < n_pred[:, None]
    live_g = np.arange(Z["f1_gt"].shape[1])[None] < n_gt[:, None]
    assert (Z["f1_pred"][..., 3:].prod(-1)[live_p] == 0).any() and (Z["f1_gt"][..., 3:].prod(-1)[live_g] == 0).any()
    vals = Z["f1_iou"][(n_pred == 1) & (n_gt == 1), 0, 0]
    for thr in (np.float32(0.25), np.float32(0.5)):
        assert (vals == thr).any() and (vals == np.nextafter(thr, np.float32(0))).any()


def test_selection_rule_and_batch_pipeline():
    x = np.array([-np.inf, 0.0, np.inf, 1e-3, -1e-3, 5.0, -5.0, 88.0], dtype=np.float32)
    assert R.select(x).tolist() == [2, 3, 5, 7]
    # a fixture case through the batch form, an item with a bad target count beside it
    c = int(np.flatnonzero((Z["f1_n_pred"] > 2) & (Z["f1_n_gt"] > 1))[0])
    P, G = int(Z["f1_n_pred"][c]), int(Z["f1_n_gt"][c])
    O = P + 2
    logits = np.full((2, O), -3.0, dtype=np.float32)
    logits[:, 1:1 + P] = 2.0
    boxes = np.zeros((2, O, 6), dtype=np.float32)
    boxes[:, 1:1 + P] = Z["f1_pred"][c, :P]
    tb = np.stack([Z["f1_gt"][c], Z["f1_gt"][c]])
    out, err, sels, costs = R.multi3drefer_batch(logits, boxes, tb, np.array([G, tb.shape[1] + 1], dtype=np.int32))
    assert err.tolist() == [0, R.ERR_N_TGT] and out[1].tolist() == [0, 0, 0, 0] and sels[0].tolist() == list(range(1, 1 + P))
    assert np.array_equal(np.array(R.f1_pair(*out[0]), dtype=np.float64), Z["f1_scores"][c])
    assert np.array_equal(-costs[0][:P, :G], Z["f1_iou"][c, :P, :G])
    m = R.multi3drefer_pairs(out[:1], ["mt"])
    assert m["iou25_mt"] == (Z["f1_scores"][c, 0], 1) and m["iou50_zt_w_d"] == (0, 0) and m["iou50_overall"][1] == 1
    assert R.accumulate([m, m], "iou50_overall")["target_metric"] == Z["f1_scores"][c, 1]
