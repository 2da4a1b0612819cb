"""pq3d_amd/ground_eval.py + csrc/ground.hip against the numpy restatement tests/ground_eval_ref.py, exactly: refer_counts
(predictions, hit bits, count table), the Multi3DRefer pipeline (cost matrices bit for bit against the reference's own IoU
matrices of fixture F28, counts on random batches), the three evaluators' metric dicts, the error paths and a captured graph.

Logits are 0, +-inf or at least 1e-3 in magnitude: inside 0 < |x| < 1e-6 the device expf and another sigmoid may disagree on
which side of 0.5 a slot falls (DESIGN 7g leaves that band unpinned)."""
import os

import numpy as np
import pytest
import torch

from tests import ground_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS, OS, TS = (1, 5, 64, 65), (1, 3, 64, 65, 130), (1, 4, 9)
Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F28_ground_eval.npz"))


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# ----------------------------------------------------------------------------------------------------------------- refer
def refer_case(B, O, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, O)).astype(np.float32)
    x[rng.random((B, O)) < 0.2] = -np.inf
    plant = [lambda r: r.__setitem__(slice(None), -np.inf),                       # a fully padded row
             lambda r: r.__setitem__([0, O - 1, O // 2], 9.0),                    # a tie
             lambda r: r.__setitem__(O // 2, np.nan),                             # a NaN
             lambda r: r.__setitem__([O - 1, O // 3], np.nan),                    # two NaNs, beside a +inf
             lambda r: r.__setitem__(O - 1, np.inf)]
    for k, f in enumerate(plant):
        f(x[(3 * k + 1) % B])
    labels = (rng.random((3, B, O)) < 0.3).astype(np.float32)
    tgt = rng.integers(0, O, B).astype(np.int64)
    flags = [(rng.random(B) < p).astype(np.uint8) for p in (0.6, 0.4, 0.3)]
    mask = (rng.random(B) < 0.7).astype(np.uint8)
    return x, labels, tgt, flags, mask


@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("B", BS)
def test_refer_counts(B, O):
    from pq3d_amd.ground_eval import refer_counts
    x, labels, tgt, (mu, ha, vd), mask = refer_case(B, O, 100 * B + O)
    forms = [dict(labels=labels), dict(labels=labels, tgt=tgt), dict(tgt=tgt),
             dict(labels=labels, is_multiple=mu), dict(tgt=tgt, is_hard=ha, is_view_dependent=vd),
             dict(labels=labels, tgt=tgt, is_multiple=mu, is_hard=ha, is_view_dependent=vd, item_mask=mask)]
    for kw in forms:
        got = refer_counts(_t(x), **{k: (_t(v) if k in ("labels", "tgt") else _t(v).bool() if k == "is_hard" else _t(v))
                                     for k, v in kw.items()})
        pred, hits, counts = R.refer_counts(x, **kw)
        assert np.array_equal(got.pred.cpu().numpy(), pred), kw.keys()
        assert np.array_equal(got.hits.cpu().numpy(), hits), kw.keys()
        assert np.array_equal(got.counts.cpu().numpy(), counts), kw.keys()
    assert counts[0, 0] == int(mask.sum()) and counts[1, 0] + counts[2, 0] == counts[0, 0]


def test_refer_counts_argument_checks():
    from pq3d_amd.ground_eval import refer_counts
    x = _t(np.zeros((4, 3), dtype=np.float32))
    tgt = _t(np.zeros(4, dtype=np.int64))
    for bad in (dict(), dict(tgt=tgt.int()), dict(tgt=tgt[:3]), dict(labels=x), dict(tgt=tgt, is_hard=tgt),
                dict(tgt=tgt.cpu()), dict(tgt=tgt, item_mask=torch.ones(5, dtype=torch.bool, device=DEV))):
        with pytest.raises(ValueError):
            refer_counts(x, **bad)
    with pytest.raises(ValueError):
        refer_counts(x.double(), tgt=tgt)
    with pytest.raises(ValueError):
        refer_counts(x.cpu(), tgt=tgt.cpu())


# -------------------------------------------------------------------------------------------------------------------- f1
P_NEAR, NEAR, FAR = 0.45, (0.12, 0.12), (0.65, 0.3)     # share of near copies; (centre shift / size, size change) of near and far ones


def f1_case(B, O, T, seed):
    """Targets: 0 .. T random boxes per item.  Predictions: jittered copies of the targets in random slots (near copies and
    far ones, so that matched IoUs spread over (0, 1)), a few strays; the other slots are not selected (negative, 0 or -inf)."""
    rng = np.random.default_rng(seed)
    tb = np.concatenate([rng.random((B, T, 3)) * 6 - 3, rng.random((B, T, 3)) * 1.2 + 0.3], 2)
    n_tgt = rng.integers(0, T + 1, B).astype(np.int32)
    boxes = np.concatenate([rng.random((B, O, 3)) * 6 - 3, rng.random((B, O, 3)) * 1.2 + 0.3], 2).astype(np.float32)
    neg = -(rng.random((B, O)) * 6 + 1e-3).astype(np.float32)
    neg[rng.random((B, O)) < 0.15] = 0.0
    neg[rng.random((B, O)) < 0.15] = -np.inf
    logits = neg
    for b in range(B):
        P = min(O, max(0, int(n_tgt[b]) + int(rng.integers(-2, 3))))
        slots = rng.permutation(O)[:P]
        for k, q in enumerate(slots):
            logits[b, q] = np.inf if rng.random() < 0.1 else np.float32(rng.random() * 6 + 1e-3)
            if k < n_tgt[b]:
                g = tb[b, k]
                shift, scale = (NEAR if rng.random() < P_NEAR else FAR)
                c = g[:3] + (rng.random(3) * 2 - 1) * shift * g[3:]
                s = g[3:] * (1 + (rng.random(3) * 2 - 1) * scale)
                boxes[b, q] = np.concatenate([c, s]).astype(np.float32)
    return logits, boxes, tb, n_tgt


@pytest.fixture(scope="module")
def f1_cases():
    """Every (B, O, T_max) batch with its restatement, computed once."""
    cases = {}
    for B in BS:
        for O in OS:
            for T in TS:
                inp = f1_case(B, O, T, 7 + 1000 * B + 10 * O + T)
                cases[B, O, T] = (inp, R.multi3drefer_batch(*inp))
    return cases


def test_matched_ious_fall_on_both_sides_of_both_thresholds(f1_cases):
    """(CPU side) of the restatement's matched pairs at least a third lies below and a third at or above each threshold."""
    ious = []
    for (logits, boxes, tb, n_tgt), (out, err, sels, costs) in f1_cases.values():
        for b in range(len(logits)):
            P, G = int(out[b, 2]), int(out[b, 3])
            if P and G:
                _, col = R.f1_counts(boxes[b][sels[b]], tb[b][:G])
                ious += [-costs[b][i, col[i]] for i in range(P) if col[i] < G]
    ious = np.array(ious)
    assert len(ious) > 2000
    for thr in (0.25, 0.5):
        assert (ious < thr).mean() >= 1 / 3 and (ious >= thr).mean() >= 1 / 3, (thr, (ious < thr).mean())


def _check_batch(got, inp, want):
    logits, boxes, tb, n_tgt = inp
    out, err, sels, costs = want
    B, O = logits.shape
    assert np.array_equal(got.out.cpu().numpy(), out)
    sizes, sel, cost = got.sizes.cpu().numpy(), got.selected.cpu().numpy(), got.cost.cpu().numpy()
    assert np.array_equal(sizes[3], err)
    for b in range(B):
        nb = costs[b].shape[0]
        assert sizes[0, b] == out[b, 2] and sizes[1, b] == out[b, 3] and sizes[2, b] == nb
        assert np.array_equal(sel[b], np.concatenate([sels[b], np.full(O - len(sels[b]), -1, dtype=np.int32)]))
        assert np.array_equal(cost[b, :nb, :nb].view(np.int32), costs[b].view(np.int32)), b


@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("B", BS)
def test_multi3drefer_counts_random_batches(f1_cases, B, O):
    from pq3d_amd.ground_eval import multi3drefer_counts
    for T in TS:
        inp, want = f1_cases[B, O, T]
        logits, boxes, tb, n_tgt = inp
        _check_batch(multi3drefer_counts(_t(logits), _t(boxes), _t(tb), _t(n_tgt)), inp, want)


def fixture_batch():
    """The box sets of F28 as one batch: case c's predictions sit in slots 1 .. P_c of item c."""
    n_pred, n_gt = Z["f1_n_pred"], Z["f1_n_gt"]
    C, Pm = len(n_pred), Z["f1_pred"].shape[1]
    O = Pm + 3
    rng = np.random.default_rng(4)
    logits = np.full((C, O), -2.5, dtype=np.float32)
    logits[:, 0] = -np.inf
    logits[:, -1] = 0.0
    boxes = (rng.random((C, O, 6)) + 0.5).astype(np.float32)
    for c in range(C):
        logits[c, 1:1 + n_pred[c]] = 1.0 + c
        boxes[c, 1:1 + n_pred[c]] = Z["f1_pred"][c, :n_pred[c]]
    return logits, boxes, Z["f1_gt"].copy(), n_gt.astype(np.int32)


def test_fixture_box_sets_through_the_kernels():
    """Cost matrices bit for bit against the IoU matrices the reference's own box3d_iou gave, F1 equal to evaluate_one_query's."""
    from pq3d_amd.ground_eval import check_f1_errors, f1_pair, multi3drefer_counts
    logits, boxes, tb, n_tgt = fixture_batch()
    got = multi3drefer_counts(_t(logits), _t(boxes), _t(tb), _t(n_tgt))
    check_f1_errors(got)
    out, cost = got.out.cpu().numpy(), got.cost.cpu().numpy()
    for c in range(len(n_tgt)):
        P, G = int(Z["f1_n_pred"][c]), int(n_tgt[c])
        nb = max(P, G)
        assert out[c, 2] == P and out[c, 3] == G
        assert np.array_equal((-cost[c, :P, :G]).view(np.int32), Z["f1_iou"][c, :P, :G].view(np.int32)), c
        block = cost[c, :nb, :nb].copy()
        block[:P, :G] = 0
        assert not block.any()
        assert np.array_equal(np.array(f1_pair(*map(int, out[c])), dtype=np.float64), Z["f1_scores"][c]), c
    _check_batch(got, (logits, boxes, tb, n_tgt), R.multi3drefer_batch(logits, boxes, tb, n_tgt))


def test_bad_target_count_and_size_limit(f1_cases):
    from pq3d_amd.ground_eval import ERR_N_TGT, Multi3DReferEval, check_f1_errors, multi3drefer_counts
    inp, _ = f1_cases[5, 65, 4]
    logits, boxes, tb, n_tgt = inp
    bad = n_tgt.copy()
    bad[1], bad[3] = 5, -1
    want = R.multi3drefer_batch(logits, boxes, tb, bad)
    got = multi3drefer_counts(_t(logits), _t(boxes), _t(tb), _t(bad))
    _check_batch(got, (logits, boxes, tb, bad), want)                 # the other items' results are intact
    assert got.sizes[3].cpu().tolist() == [0, ERR_N_TGT, 0, ERR_N_TGT, 0] and got.out[1].cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="item 1"):
        check_f1_errors(got)
    ev = Multi3DReferEval()
    ev.update(dict(og3d_logits=_t(logits), obj_boxes=_t(boxes), tgt_obj_boxes=_t(tb), n_tgt=_t(bad), eval_type=["mt"] * 5))
    with pytest.raises(ValueError, match="n_tgt"):
        ev.record()
    big = torch.zeros(1, 1025, device=DEV)
    with pytest.raises(ValueError, match="1024"):                     # before any launch
        multi3drefer_counts(big, torch.zeros(1, 1025, 6, device=DEV), _t(tb[:1]), _t(n_tgt[:1]))
    for args in ((_t(logits).double(), _t(boxes), _t(tb), _t(n_tgt)), (_t(logits), _t(boxes), _t(tb).float(), _t(n_tgt)),
                 (_t(logits), _t(boxes), _t(tb), _t(n_tgt).long()), (_t(logits), _t(boxes)[:, :3], _t(tb), _t(n_tgt)),
                 (_t(logits), _t(boxes), _t(tb), _t(n_tgt).cpu())):
        with pytest.raises(ValueError):
            multi3drefer_counts(*args)


# ------------------------------------------------------------------------------------------------------------ evaluators
def test_evaluators_accumulate_like_the_reference(f1_cases):
    from pq3d_amd.ground_eval import Multi3DReferEval, ReferIt3DEval, ScanReferEval
    scan, refit, m3d = ScanReferEval(), ReferIt3DEval(), Multi3DReferEval()
    want_scan, want_refit, want_m3d = [], [], []
    rng = np.random.default_rng(9)
    for k, (B, O, T) in enumerate(((64, 65, 4), (5, 3, 9), (65, 130, 1))):
        x, labels, tgt, (mu, ha, vd), _ = refer_case(B, O, 50 + k)
        row_form = k == 1              # the unified wrapper's 0-1 rows for this batch, index targets for the others
        dd = dict(og3d_logits=_t(x), tgt_object_id=_t(labels[0]) if row_form else _t(tgt)[:, None],
                  tgt_object_id_iou25=_t(labels[1]), tgt_object_id_iou50=_t(labels[2]),
                  is_multiple=_t(mu).bool(), is_hard=_t(ha).bool(), is_view_dependent=_t(vd).bool())
        scan.update(dd)
        refit.update(dd)
        kw = dict(labels=labels) if row_form else dict(labels=np.stack([np.zeros_like(x), labels[1], labels[2]]), tgt=tgt)
        want_scan.append(R.scanrefer_pairs(R.refer_counts(x, is_multiple=mu, **kw)[2]))
        want_refit.append(R.referit3d_pairs(R.refer_counts(x, is_hard=ha, is_view_dependent=vd, **kw)[2]))
        (logits, boxes, tb, n_tgt), (out, _err, _s, _c) = f1_cases[B, O, T]
        types = [R.EVAL_TYPES[i] for i in rng.integers(0, 4 if k else 5, B)]        # ('mt' only in the first batch)
        if k == 1:                      # the reference's own form: lists of boxes
            m3d.update(dict(og3d_logits=_t(logits), obj_boxes=_t(boxes), eval_type=types,
                            tgt_obj_boxes=[tb[b, :n_tgt[b]].tolist() for b in range(B)]))
        else:
            m3d.update(dict(og3d_logits=_t(logits), obj_boxes=_t(boxes), eval_type=types, tgt_obj_boxes=_t(tb), n_tgt=_t(n_tgt)))
        want_m3d.append(R.multi3drefer_pairs(out, types))
    for ev, want in ((scan, want_scan), (refit, want_refit), (m3d, want_m3d)):
        is_best, got = ev.record()
        ref = R.accumulate(want, ev.target_metric)
        assert is_best and got["best_result"] == ref["target_metric"]
        assert [k for k in got if k != "best_result"] == list(ref)
        for k, v in ref.items():
            assert got[k] == v, k
    assert scan.target_metric == refit.target_metric == "og_acc" and m3d.target_metric == "iou50_overall"
    with pytest.raises(NotImplementedError):
        ScanReferEval(save=True)
    with pytest.raises(NotImplementedError):
        scan.update(dict(txt_cls_logits=None))


def test_f1_pipeline_in_a_captured_graph(f1_cases):
    from pq3d_amd.ground_eval import multi3drefer_counts
    a, wa = f1_cases[64, 65, 4]
    b = f1_case(64, 65, 4, 12345)
    wb = R.multi3drefer_batch(*b)
    static = [_t(v) for v in a]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        multi3drefer_counts(*static)                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = multi3drefer_counts(*static)
    for inp, want in ((b, wb), (a, wa)):
        for st, v in zip(static, inp):
            st.copy_(_t(v))
        graph.replay()
        torch.cuda.synchronize()
        _check_batch(res, inp, want)
        eager = multi3drefer_counts(*static)
        assert torch.equal(eager.out, res.out) and torch.equal(eager.sizes, res.sizes) and torch.equal(eager.col, res.col)
