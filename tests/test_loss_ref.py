"""CPU: the float64 restatement of the segmentation losses (tests/loss_ref.py) against fixtures F9 / F10 (the reference's own
classes) and the fp32 oracle, the stability of the assignments the GPU tests compare, and the fp32 arithmetic fact behind
the termwise matched mask loss."""
import numpy as np
import pytest
import torch

from oracle import loss_oracle as LO
from pq3d_amd import synth
from tests import loss_ref as R
from tests import util

W = R.W


def test_restatement_reproduces_set_criterion_fixture():
    z, _ = util.load_fixture("F9_set_criterion")
    masks, logits, labels, seg = synth.criterion_inputs()
    ref = R.set_criterion(masks, logits, labels, seg, num_classes=20, **W)
    assert abs(float(ref["total"]) - float(z["total"])) <= 1e-5 * abs(float(z["total"]))
    assert sorted(ref["losses"]) == sorted(k[5:] for k in z.files if k.startswith("loss/"))
    for k, v in ref["losses"].items():
        assert abs(float(v) - float(z["loss/" + k])) <= 2e-6 * max(1.0, abs(float(z["loss/" + k]))), k
    for b, (i, j) in enumerate(ref["indices"][-1]):
        assert np.array_equal(i.numpy(), z[f"indices/{b}/q"]) and np.array_equal(j.numpy(), z[f"indices/{b}/t"])
    for l in range(len(masks)):
        util.check_against(z, f"grad/mask/{l}", ref["grad_mask"][l], atol=1e-7, rtol=1e-4)
        util.check_against(z, f"grad/logits/{l}", ref["grad_logits"][l], atol=1e-7, rtol=1e-4, cap=util.MAX_GRAD)


def test_restatement_reproduces_direct_losses_fixture():
    z, _ = util.load_fixture("F10_direct_losses")
    masks, logits, tgt, pad, labels, obj_masks, lab2 = synth.direct_loss_inputs()
    masks = [m.double().requires_grad_(True) for m in masks]
    logits = [l.double().requires_grad_(True) for l in logits]
    losses = R.direct_criterion(masks, logits, tgt, pad, labels)
    total = LO.instseg_loss(losses, **W)[0]
    ml = R.mask_loss({"gt_attn_mask": tgt.logical_not(), "instance_labels": lab2, "obj_masks": obj_masks,
                      "padding_mask": pad, "predictions_mask": masks, "predictions_class": logits})
    (total + ml).backward()
    assert total.dtype == ml.dtype == torch.float64
    assert abs(total.item() - float(z["total"])) <= 1e-5 * abs(float(z["total"]))
    assert abs(ml.item() - float(z["mask_loss"])) <= 1e-5 * abs(float(z["mask_loss"]))
    for k, v in losses.items():
        assert abs(v.item() - float(z["loss/" + k])) <= 2e-6 * max(1.0, abs(float(z["loss/" + k]))), k
    for l in range(len(masks)):
        util.check_against(z, f"grad/mask/{l}", masks[l].grad, atol=1e-7, rtol=1e-4)
        util.check_against(z, f"grad/logits/{l}", logits[l].grad, atol=1e-7, rtol=1e-4, cap=util.MAX_GRAD)


def _close32(a, b, what):
    """fp32 rounding of sums of a few thousand terms: 2e-6 relative to max(1, |.|), the bound the oracle's fixture test uses."""
    a, b = float(a.detach()), float(b.detach())
    assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), what


def test_restatement_agrees_with_fp32_oracle_on_synthetic_inputs():
    masks, logits, labels, seg = synth.criterion_inputs()
    ref = R.set_criterion(masks, logits, labels, seg, num_classes=20, **W)
    om = [m.clone().requires_grad_(True) for m in masks]
    ol = [l.clone().requires_grad_(True) for l in logits]
    olosses, oidx = LO.set_criterion(om, ol, labels, seg, num_classes=20, **W)
    LO.instseg_loss(olosses, **W)[0].backward()
    assert sorted(olosses) == sorted(ref["losses"])
    for k in olosses:
        _close32(olosses[k], ref["losses"][k], k)
    for (i, j), (oi, oj) in zip(ref["indices"][-1], oidx):
        assert torch.equal(i, oi) and torch.equal(j, oj)
    for b in range(3):
        want = ref["planes"][-1][b][0]
        got = LO.cost_matrix(logits[-1][b], masks[-1][b], labels[b], seg[b], **W)
        assert float((got.double() - want).abs().max()) <= 2e-6 * float(want.abs().max())
    for a, g in zip(om + ol, ref["grad_mask"] + ref["grad_logits"]):
        fin = torch.isfinite(g)
        assert torch.equal(fin, torch.isfinite(a.grad))
        assert float((a.grad.double() - g)[fin].abs().max()) <= 1e-7 + 1e-4 * float(g[fin].abs().max())
    # the padded losses and the row cross-entropy
    masks, logits, tgt, pad, labels, _om, _l2 = synth.direct_loss_inputs()
    for x in masks:
        xo = x.clone().requires_grad_(True)
        lm, ld = LO.batch_mask_loss(xo.permute(0, 2, 1), tgt, pad), LO.batch_dice_loss(xo.permute(0, 2, 1), tgt, pad)
        (3 * lm + 7 * ld).backward()
        rm, rd, rg = R.padded_losses(x, tgt, pad, 3.0, 7.0)
        _close32(lm, rm, "batch_mask_loss")
        _close32(ld, rd, "batch_dice_loss")
        assert float((xo.grad.double() - rg).abs().max()) <= 1e-7 + 1e-4 * float(rg.abs().max())
    for lg in logits:
        got = torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), labels.reshape(-1))
        _close32(got, R.cross_entropy_rows(lg, labels), "cross_entropy_rows")


def test_empty_scene_switch_and_label_check():
    """A scene without instances: NaN as the reference computes it (criterion.py:186 divides by num_masks = 0), 0 under the
    project's rule; the other scenes' terms are the same either way.  A label outside [0, C) raises."""
    masks, logits, labels, seg, _p, ref = R.case("c")
    idx = ref["indices"][-1]
    kw = dict(num_classes=20)
    nan = R.layer_losses(logits[-1].double(), masks[-1].double(), labels, seg, idx, empty="nan", **kw)
    zero = R.layer_losses(logits[-1].double(), masks[-1].double(), labels, seg, idx, empty="zero", **kw)
    assert torch.isnan(nan["loss_mask"]) and torch.isnan(nan["loss_dice"]) and torch.isfinite(nan["loss_ce"])
    keep = [0, 2]
    sub = R.layer_losses(logits[-1][keep].double(), masks[-1][keep].double(), [labels[b] for b in keep],
                         [seg[b] for b in keep], [idx[b] for b in keep], **kw)
    for k in ("loss_mask", "loss_dice"):
        assert float(zero[k]) == pytest.approx(float(sub[k]) * 2 / 3, rel=1e-14) and float(zero[k]) > 0
        assert float(zero[k]) == float(ref["losses"][k])
    for bad in (21, -3, 1 << 40):
        lab = labels[0].clone()
        lab[1] = bad
        with pytest.raises(ValueError):
            R.cost_planes(logits[-1][0], masks[-1][0], lab, seg[0], **W)


@pytest.mark.parametrize("cid", sorted(R.CASES))
def test_assignments_of_the_gpu_cases_are_stable(cid):
    """What the GPU tests rely on when they ask for the float64 assignment: the optimum does not move under 50 random
    perturbations of the total cost, uniform in +-5 x the tolerance the device cost is held to (2e-5 max|cost|).  Where no
    scene has more instances than queries, the optimum is the planted injection."""
    masks, logits, labels, seg, planted, ref = R.case(cid)
    cfg = R.CASES[cid]
    r = np.random.default_rng(7)
    for l in range(cfg["n_layers"]):
        for b in range(cfg["B"]):
            cost = ref["planes"][l][b][0].numpy()
            i0, j0 = ref["indices"][l][b]
            assert len(i0) == min(cfg["Nq"], cfg["n_inst"][b])
            if cost.size == 0:
                continue
            assert np.isfinite(cost).all()
            amp = 5 * 2e-5 * np.abs(cost).max()
            for _ in range(50):
                i, j = R.assign(torch.from_numpy(cost + r.uniform(-amp, amp, cost.shape)))
                assert torch.equal(i, i0) and torch.equal(j, j0), (cid, l, b)
            if cfg["n_inst"][b] <= cfg["Nq"]:
                q, inst = planted[l][b]
                o = np.argsort(q)
                assert np.array_equal(i0.numpy(), q[o]) and np.array_equal(j0.numpy(), inst[o]), (cid, l, b)


def test_fp32_termwise_mask_loss_keeps_its_digits_and_the_cancelling_form_does_not():
    """The arithmetic fact behind the mask cost's formulation (csrc/loss.hip), on the CPU in fp32 numpy against float64, at
    (Ns 1030, Nq 100, 37 instances, k = 12): the matched loss_mask as the reference forms it (separate pos / neg BCE planes
    contracted with t and 1 - t, every term non-negative) and as the shortcut pos - neg = -x forms it,
    cost_mask = (sum_s softplus(x) - (T X)) / S, a difference of two O(k S) sums.
    Measured here: true loss_mask 1.0147e-05; termwise relative error 8.9e-08, cancelling form 4.0e-02.  (torch's own fp32
    binary_cross_entropy_with_logits, which the fp32 oracle's layer_losses uses, is off by 1.2e-04: it forms
    (1 - t) x - logsigmoid(x), which cancels at a confident negative.)"""
    cfg = dict(R.CASES["e"], k=12, n_layers=1)
    masks, logits, labels, seg, _planted = R.planted_inputs(R.SEEDS["e"], **cfg)
    ref = R.set_criterion(masks, logits, labels, seg, num_classes=200, empty="zero", **W)
    want = float(ref["losses"]["loss_mask"])
    i, j = (v.numpy() for v in ref["indices"][0][0])
    f32 = np.float32
    x = masks[0][0].numpy()                                                 # [Ns, Nq] fp32
    t = seg[0].numpy().astype(f32)                                          # [Nt, Ns]
    softplus = lambda v: (np.maximum(v, f32(0)) + np.log1p(np.exp(-np.abs(v)))).astype(f32)
    pos, neg = softplus(-x), softplus(x)                                    # BCE against all-ones / all-zeros targets
    tw = (np.einsum("sq,ts->qt", pos, t) + np.einsum("sq,ts->qt", neg, f32(1) - t)) / f32(x.shape[0])
    cm = (neg.sum(0, dtype=f32)[:, None] - (t @ x).T) / f32(x.shape[0])     # pos - neg = -x: the one-GEMM shortcut
    assert tw.dtype == cm.dtype == f32
    termwise = float(tw[i, j].sum(dtype=f32) / f32(len(i)))
    cancelling = float(cm[i, j].sum(dtype=f32) / f32(len(i)))
    # for the record: the error E of oracle.loss_oracle.layer_losses, which the GPU tests measure their bound with
    oracle = float(LO.layer_losses(logits[0], masks[0], labels, seg, ref["indices"][0], num_classes=200)["loss_mask"])
    print(f"fp32 oracle (torch BCE) rel. error {abs(oracle - want) / want:.2e}")
    e_term, e_canc = abs(termwise - want) / want, abs(cancelling - want) / want
    print(f"loss_mask {want:.4e}: termwise fp32 rel. error {e_term:.2e}, cancelling fp32 form {e_canc:.2e}")
    assert e_term <= 1e-5
    assert e_canc > 1e-3
