"""GPU: the batched linear sum assignment (pq3d_amd/lsap.py, csrc/lsap.hip) is exactly scipy's linear_sum_assignment, and
SetCriterion(matching="device") gives the host mode's indices, losses and gradients -- also replayed from a captured graph
with padded targets (the host mode's device-to-host copy cannot be captured)."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from pq3d_amd import losses as HL
from pq3d_amd import synth
from pq3d_amd.losses import HungarianMatcher, SetCriterion
from pq3d_amd.lsap import BAD_SIZE, INFEASIBLE, INVALID, MAX_DIM, check_errors, linear_sum_assignment_batched

pytestmark = pytest.mark.gpu
DEV = "cuda"
W = dict(cost_class=2.0, cost_mask=5.0, cost_dice=2.0)
WD = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0}


def _solve(blocks, R=None, Cm=None):
    """Pack the host matrices into one padded [G, R, Cmax] launch (padding filled with NaN: it must never be read)."""
    R = R or max(b.shape[0] for b in blocks)
    Cm = Cm or max(b.shape[1] for b in blocks)
    cost = np.full((len(blocks), R, Cm), np.nan, np.float32)
    for g, b in enumerate(blocks):
        cost[g, :b.shape[0], :b.shape[1]] = b
    nr = torch.tensor([b.shape[0] for b in blocks], dtype=torch.int32, device=DEV)
    nc = torch.tensor([b.shape[1] for b in blocks], dtype=torch.int32, device=DEV)
    out = linear_sum_assignment_batched(torch.from_numpy(cost).to(DEV), nr, nc)
    return [t.cpu().numpy() for t in out]


def _assert_scipy(blocks, R=None, Cm=None):
    rows, cols, nm, err = _solve(blocks, R, Cm)
    for g, b in enumerate(blocks):
        i, j = linear_sum_assignment(b)
        assert err[g] == 0 and nm[g] == len(i), (g, b.shape, err[g], nm[g])
        np.testing.assert_array_equal(rows[g, :nm[g]], i, err_msg=f"matrix {g} {b.shape}")
        np.testing.assert_array_equal(cols[g, :nm[g]], j, err_msg=f"matrix {g} {b.shape}")
        assert not rows[g, nm[g]:].any() and not cols[g, nm[g]:].any()


def _kind(r, kind, nr, nc):
    if kind == "uniform":
        return r.random((nr, nc)).astype(np.float32)
    if kind == "quantized":
        return (np.round(r.random((nr, nc)) * 10) / 10).astype(np.float32)
    if kind == "integer":
        return r.integers(0, 4, (nr, nc)).astype(np.float32)
    return np.full((nr, nc), 0.25, np.float32)


@pytest.mark.parametrize("kind", ["uniform", "quantized", "integer", "constant"])
def test_small_mixed_sizes_in_one_launch(kind):
    r = np.random.default_rng(3)
    blocks = [_kind(r, kind, int(a), int(b)) for a, b in r.integers(1, 14, (300, 2))]
    _assert_scipy(blocks, 13, 13)


@pytest.mark.parametrize("shape", [(200, 60), (60, 200), (100, 130), (64, 64), (200, 1), (1, 200), (1, 1)])
@pytest.mark.parametrize("kind", ["uniform", "quantized", "constant"])
def test_criterion_shaped_matrices(shape, kind):
    r = np.random.default_rng(shape[0] * 7 + shape[1])
    blocks = [_kind(r, kind, *shape) for _ in range(6)]
    _assert_scipy(blocks)
    if kind == "constant":
        rows, cols, nm, _ = _solve(blocks)
        assert (rows[:, :nm[0]] == np.arange(min(shape))).all() and (cols[:, :nm[0]] == np.arange(min(shape))).all()


def test_zero_and_one_columns_and_full_size_defaults():
    r = np.random.default_rng(5)
    c = torch.from_numpy(r.random((4, 50, 8)).astype(np.float32)).to(DEV)
    rows, cols, nm, err = linear_sum_assignment_batched(c, None, torch.tensor([0, 1, 8, 0], dtype=torch.int32, device=DEV))
    assert err.tolist() == [0, 0, 0, 0] and nm.tolist() == [0, 1, 8, 0]
    for g, n in ((1, 1), (2, 8)):
        i, j = linear_sum_assignment(c[g, :, :n].cpu().numpy())
        assert rows[g, :n].tolist() == i.tolist() and cols[g, :n].tolist() == j.tolist()
    assert not rows[0].any() and not cols[3].any()
    rows, cols, nm, err = linear_sum_assignment_batched(c)          # n_rows / n_cols default to R / Cmax
    for g in range(4):
        i, j = linear_sum_assignment(c[g].cpu().numpy())
        assert rows[g].tolist() == i.tolist() and cols[g].tolist() == j.tolist() and nm[g] == 8


def test_stated_maximum_sizes():
    r = np.random.default_rng(9)
    # 1024 x 1024 is past the LDS staging budget (global-memory path); the others fit it or not per launch
    _assert_scipy([r.random((MAX_DIM, MAX_DIM)).astype(np.float32),
                   (np.round(r.random((MAX_DIM, 1000)) * 20) / 20).astype(np.float32),
                   r.random((60, MAX_DIM)).astype(np.float32)], MAX_DIM, MAX_DIM)
    _assert_scipy([r.random((MAX_DIM, 60)).astype(np.float32) for _ in range(3)])
    _assert_scipy([r.random((60, MAX_DIM)).astype(np.float32) for _ in range(3)])


def test_real_cost_matrices_of_the_criterion():
    """The matrices of _costs at the bench's sizes: B = 4, Ns = 4096, Nq = 200, 13 layers, up to 60 instances."""
    B, Ns, Nq, nl = 4, 4096, 200, 13
    r = np.random.default_rng(0)
    seg_len = [Ns] + [int(x) for x in r.integers(Ns // 2, Ns, B - 1)]
    n_inst = [int(x) for x in r.integers(30, 61, B)]
    masks, logits, labels, seg = synth.criterion_inputs(seed=1, B=B, Ns=Ns, Nq=Nq, C=201, n_layers=nl, seg_len=seg_len,
                                                        n_inst=n_inst)
    T, lab, sl, nid, n_inst, t_sum = HL._targets_to_device(labels, seg, Ns, DEV)
    cost, _ = HL._costs([m.to(DEV) for m in masks], [l.to(DEV) for l in logits], T, lab, sl, nid, t_sum, (2.0, 5.0, 2.0), -100)
    Nt = T.shape[1]
    cm = cost[:, 0].reshape(nl * B, Nq, Nt)
    rows, cols, nm, err = (t.cpu().numpy() for t in linear_sum_assignment_batched(cm, None, nid.repeat(nl)))
    host = cm.cpu().numpy()
    for g in range(nl * B):
        i, j = linear_sum_assignment(host[g, :, :n_inst[g % B]])
        assert err[g] == 0 and nm[g] == len(i)
        assert np.array_equal(rows[g, :len(i)], i) and np.array_equal(cols[g, :len(j)], j), g


def test_error_codes_leave_the_other_matrices_correct():
    r = np.random.default_rng(13)
    good = [r.random((7, 5)).astype(np.float32) for _ in range(3)]
    nan = r.random((6, 6)).astype(np.float32); nan[2, 3] = np.nan
    ninf = r.random((4, 9)).astype(np.float32); ninf[3, 8] = -np.inf
    inf_rows = r.random((5, 4)).astype(np.float32); inf_rows[:, 1:] = np.inf       # tall: 5 rows share one finite column
    inf_cols = inf_rows.T.copy()
    blocks = [good[0], nan, good[1], ninf, inf_rows, inf_cols, good[2]]
    rows, cols, nm, err = _solve(blocks)
    assert err.tolist() == [0, INVALID, 0, INVALID, INFEASIBLE, INFEASIBLE, 0]
    assert nm.tolist() == [5, 0, 5, 0, 0, 0, 5]
    for g in (0, 2, 6):
        i, j = linear_sum_assignment(blocks[g])
        assert np.array_equal(rows[g, :5], i) and np.array_equal(cols[g, :5], j)
    for g in (1, 3, 4, 5):
        assert not rows[g].any() and not cols[g].any()
    for g, msg in ((1, "invalid numeric entries"), (4, "infeasible")):
        with pytest.raises(ValueError, match=msg):
            linear_sum_assignment(blocks[g])
        with pytest.raises(ValueError, match=msg):
            check_errors(torch.tensor([0] * g + [int(err[g])], dtype=torch.int32, device=DEV))
    ok = linear_sum_assignment_batched(torch.zeros(2, 3, 3, device=DEV),
                                       torch.tensor([4, 3], dtype=torch.int32, device=DEV), None)[3]
    assert ok.tolist() == [BAD_SIZE, 0]
    check_errors(torch.zeros(3, dtype=torch.int32, device=DEV))


def test_bad_inputs_raise():
    c = torch.zeros(2, 3, 4, device=DEV)
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(c.double())
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(c.cpu())
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(c[0])
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(torch.zeros(1, MAX_DIM + 1, 4, device=DEV))
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(torch.zeros(1, 4, MAX_DIM + 1, device=DEV))
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(c, None, torch.ones(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(c, torch.ones(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        linear_sum_assignment_batched(c, torch.ones(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        make_criterion(matching="gpu")
    masks, logits, labels, seg = synth.criterion_inputs()
    dm = [m.to(DEV) for m in masks]
    dl = [l.to(DEV) for l in logits]
    host = make_criterion()
    tg = host.pad_targets(labels, seg, 70, 12)
    with pytest.raises(ValueError, match="matching='device'"):
        host(dm, dl, targets=tg)
    with pytest.raises(ValueError):
        host.pad_targets(labels, seg, 70, 8)           # a scene has 9 instances
    with pytest.raises(ValueError):
        host.pad_targets(labels, seg, 60, 12)          # a scene has 70 segments
    with pytest.raises(ValueError):
        make_criterion(matching="device")(dm, dl, targets=make_criterion().pad_targets(labels[:2], seg[:2], 70, 12))


# ------------------------------------------------------------------------------------------------ the criterion
def make_criterion(num_classes=20, matching="host"):
    matcher = HungarianMatcher(num_points=-1, ignore_label=-100, **W)
    return SetCriterion(num_classes=num_classes, matcher=matcher, weight_dict=WD, losses=["labels", "masks"], num_points=-1,
                        class_weights=-1, ignore_label=-100, matching=matching)


def _total(losses):
    return sum(v * WD["_".join(k.split("_")[:2])] for k, v in losses.items())


def _run(crit, masks, logits, *args, **kw):
    dm = [m.to(DEV).requires_grad_(True) for m in masks]
    dl = [l.to(DEV).requires_grad_(True) for l in logits]
    losses, idx = crit(dm, dl, *args, **kw)
    _total(losses).backward()
    return losses, idx, [t.grad for t in dm + dl]


def _exact(a, b):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def _same_as_host(masks, logits, labels, seg, C):
    hl, hidx, hg = _run(make_criterion(C - 1), masks, logits, labels, seg)
    dl, didx, dg = _run(make_criterion(C - 1, "device"), masks, logits, labels, seg)
    assert sorted(hl) == sorted(dl)
    for k in hl:
        _exact(dl[k], hl[k])
    assert len(didx) == len(hidx)
    for (qi, ti), (hq, ht) in zip(didx, hidx):
        assert qi.is_cuda and qi.dtype == torch.int64
        assert torch.equal(qi.cpu(), hq) and torch.equal(ti.cpu(), ht)
    for a, b in zip(dg, hg):
        _exact(a, b)


def test_device_matching_equals_host_on_reference_inputs():
    masks, logits, labels, seg = synth.criterion_inputs()
    _same_as_host(masks, logits, labels, seg, 21)


@pytest.mark.parametrize("B,Ns,Nq,C,nl", [(2, 300, 100, 201, 2), (4, 1024, 200, 201, 3)])
def test_device_matching_equals_host_at_larger_sizes(B, Ns, Nq, C, nl):
    r = np.random.default_rng(B * 1000 + Ns)
    seg_len = [Ns] + [int(x) for x in r.integers(Ns // 2, Ns, B - 1)]
    n_inst = [int(x) for x in r.integers(3, min(Nq, 90), B)]
    masks, logits, labels, seg = synth.criterion_inputs(seed=B + Ns, B=B, Ns=Ns, Nq=Nq, C=C, n_layers=nl, seg_len=seg_len,
                                                        n_inst=n_inst)
    _same_as_host(masks, logits, labels, seg, C)


def test_invalid_costs_give_nan_losses_and_check_raises():
    masks, logits, labels, seg = synth.criterion_inputs()
    masks[0][0, 3, 2] = float("nan")                 # first auxiliary layer ('_0'), scene 0, a valid segment
    crit = make_criterion(matching="device")
    losses, _, _ = _run(crit, masks, logits, labels, seg)
    assert torch.isnan(losses["loss_mask_0"]) and torch.isnan(losses["loss_ce_0"])
    assert torch.isfinite(losses["loss_mask"]) and torch.isfinite(losses["loss_dice_1"])
    with pytest.raises(ValueError, match="invalid numeric entries"):
        crit.check()


def test_captured_criterion_replays_batches_of_different_targets():
    """forward + backward of the device-mode criterion on padded targets in one CUDA graph, replayed on batches with
    different contents and instance counts (0 included); each replay equals an eager device-mode run on the same padded
    targets bit for bit, and the eager host-mode run on the ragged targets in indices and (to rounding) in losses and
    gradients."""
    B, Ns, Nq, C, nl, NT = 3, 300, 100, 21, 3, 12
    counts = [(5, 9, 3), (0, 12, 4), (7, 4, 0)]
    batches = [synth.criterion_inputs(seed=50 + k, B=B, Ns=Ns, Nq=Nq, C=C, n_layers=nl, seg_len=(300, 211, 260),
                                      n_inst=n) for k, n in enumerate(counts)]
    crit = make_criterion(C - 1, "device")
    masks0, logits0, labels0, seg0 = batches[0]
    dm = [m.to(DEV).requires_grad_(True) for m in masks0]
    dl = [l.to(DEV).requires_grad_(True) for l in logits0]
    static = crit.pad_targets(labels0, seg0, Ns, NT)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            for t in dm + dl:
                t.grad = None
            _total(crit(dm, dl, targets=static)[0]).backward()
    torch.cuda.current_stream().wait_stream(side)
    for t in dm + dl:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses, idx = crit(dm, dl, targets=static)
        _total(losses).backward()
    for k, (masks, logits, labels, seg) in enumerate(batches):
        with torch.no_grad():
            for t, s in zip(dm + dl, masks + logits):
                t.copy_(s)
        static.copy_(crit.pad_targets(labels, seg, Ns, NT))
        graph.replay()
        torch.cuda.synchronize()
        eager = make_criterion(C - 1, "device")
        el, eidx, eg = _run(eager, masks, logits, targets=eager.pad_targets(labels, seg, Ns, NT))
        for key in el:
            _exact(losses[key], el[key])
        for a, b in zip(idx, eidx):
            assert torch.equal(a, b)
        for t, b in zip(dm + dl, eg):
            _exact(t.grad, b)
        hl, hidx, hg = _run(make_criterion(C - 1), masks, logits, labels, seg)
        q, t_, nm = idx
        assert nm.tolist() == [min(Nq, n) for n in counts[k]]
        for b, (hq, ht) in enumerate(hidx):
            assert torch.equal(q[b, :nm[b]].cpu(), hq) and torch.equal(t_[b, :nm[b]].cpu(), ht)
        for key in hl:
            torch.testing.assert_close(losses[key], hl[key], rtol=1e-6, atol=1e-7)
        for t, b in zip(dm + dl, hg):
            torch.testing.assert_close(torch.nan_to_num(t.grad), torch.nan_to_num(b), rtol=1e-5, atol=1e-7)

