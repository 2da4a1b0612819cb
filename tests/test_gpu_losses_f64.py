"""GPU: the segmentation losses (pq3d_amd/losses.py, csrc/loss.hip) against the float64 restatement tests/loss_ref.py on
confident predictions aligned with their targets (loss_ref.planted_inputs), at the sizes where the kernels change path.

Set criterion cases (loss_ref.CASES; B, Ns, Nq, C | seg_len | n_inst | k):
  a  3, 300, 70, 21 | 300, 257, 1 | 40, 7, 1 | 12   two prep splits (256 boundary), gradient-tile tail (300 = 18 x 16 + 12),
                                                    second 64-query block, a one-segment scene
  b  2, 520, 65, 21 | 520, 333 | 90, 3 | 12         more targets than queries (Nm = Nq), second trip of the 64-stride target loop
  c  3, 300, 70, 21 | 300, 200, 123 | 5, 0, 9 | 12  an empty scene between full ones
  d  2, 64, 12, 21 | 64, 40 | 0, 0 | 12             every scene empty (Nt, Nm padded to 1): all queries no-object, mask / dice 0
  e  1, 1030, 100, 201 | 1030 | 37 | 100            saturated logits (exp(-x) overflows), class loop of 3 x 64 + 9
  f  1, 1, 1, 5 | 1 | 1 | 12                        degenerate sizes
  g  1, 40, 512, 21 | 40 | 3 | 12                   LDS tile above 64 KiB in pq3d_matched_mask_grad (one layer)
  h  case a, every label of scene 1 = ignore_label  class cost -1 throughout, CE kept-row count

loss_mask is held to a RELATIVE bound (it is a sum of non-negative terms): 8 x max(E, 2^-23) x |ref|, E = the relative error
of the fp32 oracle (oracle.loss_oracle.layer_losses, CPU, same inputs and indices) against float64; loss_dice to
8 x max(E_abs, 2^-23) absolutely (1 - ratio cancels in the reference too).  E is not small at these inputs: torch's fp32
binary_cross_entropy_with_logits forms (1 - t) x - logsigmoid(x), which cancels at a confident negative.

Measured on an MI355X (main prediction layer; the tests print these figures).  `before` = with cost_mask formed as
(sum_s softplus(x) - T X) / S and cost_dice as 1 - (2 I + 1) / D, whose matched entries the losses were and are:
  case  loss_mask (float64)  E (fp32 oracle)  device rel. err  before    | loss_dice   E_abs    device abs err  before
  a     1.3574e-05           1.9e-05          5.1e-08          4.4e-03   | 1.6353e-04  7.0e-09  2.2e-11         3.5e-09
  b     1.0427e-05           2.0e-04          2.6e-08          4.0e-03   | 4.1053e-04  1.2e-08  7.6e-12         1.2e-09
  e     6.1087e-44           9.8e-01          9.3e-03          6e+35 (3.7e-08 reported; -2.7e-08 in the auxiliary layer)
        (case e's loss is an fp32 denormal: 9.3e-03 is its grid)        | 0           0        0               0
At the one-element sizes (case f, padded case B) a whole tensor is one small number, and the bounds relative to a tensor's
maximum become relative to that number: there the old forms missed the dice cost plane (3.5e-08 on 1.9e-06: 1 - ratio
cancels) and the mask gradients (2.6e-07 on 3.3e-05: sigma(x) - t from the rounded sigma(12) = 1 - 6e-06); the kernels now form
both from sigma(x) and sigma(-x).
"""
import numpy as np
import pytest
import torch

from oracle import loss_oracle as LO
from pq3d_amd import _lib as L
from pq3d_amd import losses as HL
from pq3d_amd import synth
from pq3d_amd.losses import DirectCriterion, HungarianMatcher, SetCriterion, padded_mask_losses
from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
W = R.W
WD = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 2.0}
EPS = 2.0 ** -23


def make_criterion(num_classes, matching="host"):
    matcher = HungarianMatcher(num_points=-1, ignore_label=-100, **W)
    return SetCriterion(num_classes=num_classes, matcher=matcher, weight_dict=WD, losses=["labels", "masks"], num_points=-1,
                        class_weights=-1, ignore_label=-100, matching=matching)


def _total(losses):
    return sum(v * WD["_".join(k.split("_")[:2])] for k, v in losses.items())


def _run(masks, logits, labels, seg, C, matching="host", dtype=torch.float32):
    """One criterion forward + backward -> (losses, indices[l][b] in the order of ``masks``, mask grads, class-logit grads)."""
    crit = make_criterion(C - 1, matching)
    dm = [m.to(DEV, dtype).requires_grad_(True) for m in masks]
    dl = [l.to(DEV, dtype).requires_grad_(True) for l in logits]
    losses, _ = crit(dm, dl, labels, seg)
    _total(losses).backward()
    n = len(masks)
    idx = [None] * n
    for pos, l in enumerate([n - 1] + list(range(n - 1))):      # the criterion puts the main (last) prediction first
        idx[l] = [(i.cpu(), j.cpu()) for i, j in crit._last_indices[pos]]
    return losses, idx, [t.grad for t in dm], [t.grad for t in dl]


def _oracle_errors(cid, l):
    """(E, E_abs) of the fp32 oracle's loss_mask / loss_dice of layer l against float64, on the float64 indices.  Scenes
    without instances are left out of the oracle's call and put back as zeros of the mean (the project's rule)."""
    masks, logits, labels, seg, _p, ref = R.case(cid)
    B = masks[l].shape[0]
    ne = [b for b in range(B) if len(labels[b]) > 0]
    name = "" if l == len(masks) - 1 else f"_{l}"
    rm, rd = float(ref["losses"]["loss_mask" + name]), float(ref["losses"]["loss_dice" + name])
    if not ne:
        return 0.0, 0.0
    o = LO.layer_losses(logits[l][ne], masks[l][ne], [labels[b] for b in ne], [seg[b] for b in ne],
                        [ref["indices"][l][b] for b in ne], num_classes=R.CASES[cid]["C"] - 1)
    om, od = float(o["loss_mask"]) * len(ne) / B, float(o["loss_dice"]) * len(ne) / B
    return abs(om - rm) / abs(rm), abs(od - rd)


def _check_grad(got, ref, what):
    got = got.double().cpu()
    fin = torch.isfinite(ref)
    assert bool(torch.isfinite(got[fin]).all()), f"{what}: non-finite where the float64 gradient is finite"
    if bool(fin.any()):
        err, scale = float((got - ref)[fin].abs().max()), float(ref[fin].abs().max())
        assert err <= 1e-7 + 2e-4 * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("cid", sorted(R.CASES))
def test_cost_planes_match_float64(cid):
    masks, logits, labels, seg, _p, ref = R.case(cid)
    cfg = R.CASES[cid]
    T, lab, seg_len, n_inst_dev, n_inst, t_sum = HL._targets_to_device(labels, seg, cfg["Ns"], DEV)
    cost, _ = HL._costs([m.to(DEV) for m in masks], [l.to(DEV) for l in logits], T, lab, seg_len, n_inst_dev, t_sum,
                        (W["cost_class"], W["cost_mask"], W["cost_dice"]), -100)
    cost = cost.cpu()
    assert cost.shape == (cfg["n_layers"], 3, cfg["B"], cfg["Nq"], max(max(cfg["n_inst"]), 1))
    for l in range(cfg["n_layers"]):
        for b in range(cfg["B"]):
            n = n_inst[b]
            if n < cost.shape[-1]:
                assert float(cost[l, :, b, :, n:].abs().max()) == 0.0
            for p, name in enumerate(("total", "mask", "dice")):
                want = ref["planes"][l][b][p]
                if n == 0:
                    continue
                err = float((cost[l, p, b, :, :n].double() - want).abs().max())
                assert err <= 2e-5 * float(want.abs().max()), (name, l, b, err)


@pytest.mark.parametrize("cid", sorted(R.CASES))
def test_set_criterion_matches_float64(cid):
    """Indices, the three losses of every layer and both kinds of gradients (host matching)."""
    masks, logits, labels, seg, _p, ref = R.case(cid)
    cfg = R.CASES[cid]
    losses, idx, gm, gl = _run(masks, logits, labels, seg, cfg["C"])
    n = cfg["n_layers"]
    assert sorted(losses) == sorted(ref["losses"])
    for l in range(n):
        name = "" if l == n - 1 else f"_{l}"
        for b in range(cfg["B"]):
            assert torch.equal(idx[l][b][0], ref["indices"][l][b][0]) and torch.equal(idx[l][b][1], ref["indices"][l][b][1])
        got = {k: float(losses[k + name]) for k in ("loss_ce", "loss_mask", "loss_dice")}
        want = {k: float(ref["losses"][k + name]) for k in got}
        E, E_abs = _oracle_errors(cid, l)
        rel = abs(got["loss_mask"] - want["loss_mask"]) / abs(want["loss_mask"]) if want["loss_mask"] else 0.0
        print(f"case {cid} layer {l}: loss_mask {want['loss_mask']:.4e} E {E:.2e} device rel. err {rel:.2e} | "
              f"loss_dice {want['loss_dice']:.4e} E_abs {E_abs:.2e} device abs err {abs(got['loss_dice'] - want['loss_dice']):.2e} | "
              f"loss_ce {want['loss_ce']:.4e} device abs err {abs(got['loss_ce'] - want['loss_ce']):.2e}")
        assert abs(got["loss_ce"] - want["loss_ce"]) <= 2e-6 * max(1.0, abs(want["loss_ce"]))
        if max(cfg["n_inst"]) == 0:
            assert got["loss_mask"] == 0.0 and got["loss_dice"] == 0.0 and want["loss_mask"] == 0.0
        else:
            assert abs(got["loss_mask"] - want["loss_mask"]) <= 8 * max(E, EPS) * abs(want["loss_mask"])
            assert abs(got["loss_dice"] - want["loss_dice"]) <= 8 * max(E_abs, EPS)
        _check_grad(gm[l], ref["grad_mask"][l], f"mask gradient {l}")
        _check_grad(gl[l], ref["grad_logits"][l], f"class-logit gradient {l}")
        for b in range(cfg["B"]):
            unmatched = torch.ones(cfg["Nq"], dtype=torch.bool)
            unmatched[idx[l][b][0]] = False
            g = gm[l][b].cpu()
            if bool(unmatched.any()):
                assert float(g[:, unmatched].abs().max()) == 0.0
            if cfg["seg_len"][b] < cfg["Ns"]:
                assert float(g[cfg["seg_len"][b]:].abs().max()) == 0.0
            if cfg["n_inst"][b] == 0:
                assert float(g.abs().max()) == 0.0


@pytest.mark.parametrize("cid", ["a", "b", "c"])
def test_device_matching_is_bit_identical_to_host_and_runs_repeat(cid):
    masks, logits, labels, seg, _p, ref = R.case(cid)
    C = R.CASES[cid]["C"]
    host = _run(masks, logits, labels, seg, C)
    again = _run(masks, logits, labels, seg, C)
    dev = _run(masks, logits, labels, seg, C, "device")
    for other in (again, dev):
        for k in host[0]:
            torch.testing.assert_close(other[0][k], host[0][k], rtol=0, atol=0)
        for l in range(len(masks)):
            for (i, j), (hi, hj), (ri, rj) in zip(other[1][l], host[1][l], ref["indices"][l]):
                assert torch.equal(i, hi) and torch.equal(j, hj) and torch.equal(i, ri) and torch.equal(j, rj)
        for a, b in zip(other[2] + other[3], host[2] + host[3]):
            torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_bf16_predictions_give_the_bf16_rounding_of_the_fp32_gradients():
    masks, logits, labels, seg, _p, _ref = R.case("a")
    bm, bl = [m.bfloat16() for m in masks], [l.bfloat16() for l in logits]
    lo16, idx16, gm16, gl16 = _run(bm, bl, labels, seg, 21, dtype=torch.bfloat16)
    lo32, idx32, gm32, gl32 = _run([m.float() for m in bm], [l.float() for l in bl], labels, seg, 21)
    for k in lo32:
        torch.testing.assert_close(lo16[k], lo32[k], rtol=0, atol=0)
    for a, b in zip(gm16 + gl16, gm32 + gl32):
        assert a.dtype == torch.bfloat16 and b.dtype == torch.float32
        torch.testing.assert_close(a, b.bfloat16(), rtol=0, atol=0)


@pytest.mark.parametrize("bad", [21, -3, 1 << 40])
def test_label_outside_the_classes_poisons_its_cost_entries(bad):
    """A label that is neither ignore_label nor in [0, C): the cost kernel must not read the class logits out of bounds.  Its
    column of the total cost is NaN (the CE kernels' convention), every other entry is what the clean labels give; host
    matching raises scipy's error, device matching gives NaN losses (the targets are shared by all layers) and check() raises."""
    masks, logits, labels, seg = synth.criterion_inputs()
    T, lab, seg_len, n_inst_dev, n_inst, t_sum = HL._targets_to_device(labels, seg, 70, DEV)
    dm, dl = [m.to(DEV) for m in masks], [l.to(DEV) for l in logits]
    clean, _ = HL._costs(dm, dl, T, lab, seg_len, n_inst_dev, t_sum, (2.0, 5.0, 2.0), -100)
    labels = [l.clone() for l in labels]
    labels[0][1] = bad
    T, lab, seg_len, n_inst_dev, n_inst, t_sum = HL._targets_to_device(labels, seg, 70, DEV)
    cost, _ = HL._costs(dm, dl, T, lab, seg_len, n_inst_dev, t_sum, (2.0, 5.0, 2.0), -100)
    assert bool(torch.isnan(cost[:, 0, 0, :, 1]).all())
    poisoned = torch.zeros_like(cost, dtype=torch.bool)
    poisoned[:, 0, 0, :, 1] = True
    assert torch.equal(cost[~poisoned], clean[~poisoned])
    with pytest.raises(ValueError, match="invalid numeric entries"):
        make_criterion(20)(dm, dl, labels, seg)
    crit = make_criterion(20, "device")
    losses, _ = crit(dm, dl, labels, seg)
    for k, v in losses.items():
        assert bool(torch.isnan(v)), k
    with pytest.raises(ValueError, match="invalid numeric entries"):
        crit.check()


# ------------------------------------------------------------------------------------------------ padded (direct) losses
PADDED = {
    "A": dict(B=3, S=65, N=67, invalid=((1, 0), (1, 30), (1, 66)), n_valid=(67, 67, 1)),   # 64 + 1 segment tile; N not a
    # multiple of 4 or 16; padding instances inside the batch; a scene with one valid instance
    "B": dict(B=1, S=1, N=1),                                                              # degenerate
    "C": dict(B=1, S=130, N=260),                                                          # sums kernel's LDS tile above 64 KiB
}


def _padded_oracle_errors(x, T, P, rm, rd):
    om = float(LO.batch_mask_loss(x.permute(0, 2, 1), T, P))
    od = float(LO.batch_dice_loss(x.permute(0, 2, 1), T, P))
    return abs(om - rm) / abs(rm), abs(od - rd)


@pytest.mark.parametrize("k", [12, 100])
@pytest.mark.parametrize("pid", sorted(PADDED))
def test_padded_mask_losses_match_float64(pid, k):
    x, T, P = R.planted_padded_inputs(11, k=k, **PADDED[pid])
    rm, rd, rg = R.padded_losses(x, T, P, 3.0, 7.0)
    rm, rd = float(rm), float(rd)
    E, E_abs = _padded_oracle_errors(x, T, P, rm, rd)
    xd = x.to(DEV).requires_grad_(True)
    lm, ld = padded_mask_losses(xd, T.to(DEV), P.to(DEV))
    (3 * lm + 7 * ld).backward()
    print(f"padded {pid} k {k}: lm {rm:.4e} E {E:.2e} device rel. err {abs(float(lm) - rm) / abs(rm):.2e} | "
          f"ld {rd:.4e} E_abs {E_abs:.2e} device abs err {abs(float(ld) - rd):.2e}")
    assert abs(float(lm) - rm) <= 8 * max(E, EPS) * abs(rm)
    assert abs(float(ld) - rd) <= 8 * max(E_abs, EPS)
    _check_grad(xd.grad, rg, "dX")
    outside = ~P.permute(0, 2, 1)
    if bool(outside.any()):
        assert float(xd.grad.cpu()[outside].abs().max()) == 0.0


def test_direct_criterion_matches_float64_on_confident_inputs():
    cfg, C = PADDED["A"], 21
    r = np.random.default_rng(5)
    x0, T, P = R.planted_padded_inputs(11, k=12, **cfg)
    masks = [x0 + 0.25 * l for l in range(2)]                                              # two layers on the same targets
    logits = [torch.from_numpy(r.standard_normal((cfg["B"], cfg["N"], C)).astype(np.float32)) for _ in range(2)]
    labels = torch.from_numpy(r.integers(0, C, (cfg["B"], cfg["N"])))
    labels[~P.any(-1)] = -100
    rm = [m.double().requires_grad_(True) for m in masks]
    rl = [l.double().requires_grad_(True) for l in logits]
    ref = R.direct_criterion(rm, rl, T, P, labels)
    LO.instseg_loss(ref, **W)[0].backward()
    dm = [m.to(DEV).requires_grad_(True) for m in masks]
    dl = [l.to(DEV).requires_grad_(True) for l in logits]
    got = DirectCriterion(losses=["labels", "masks"], ignore_label=-100)(dm, dl, T.to(DEV), P.to(DEV), labels.to(DEV))
    _total(got).backward()
    assert sorted(got) == sorted(ref)
    for l, name in ((1, ""), (0, "_0")):
        want = {k: float(ref[k + name]) for k in ("loss_ce", "loss_mask", "loss_dice")}
        E, E_abs = _padded_oracle_errors(masks[l], T, P, want["loss_mask"], want["loss_dice"])
        assert abs(float(got["loss_ce" + name]) - want["loss_ce"]) <= 2e-6 * max(1.0, abs(want["loss_ce"]))
        assert abs(float(got["loss_mask" + name]) - want["loss_mask"]) <= 8 * max(E, EPS) * abs(want["loss_mask"])
        assert abs(float(got["loss_dice" + name]) - want["loss_dice"]) <= 8 * max(E_abs, EPS)
        _check_grad(dm[l].grad, rm[l].grad, f"mask gradient {l}")
        _check_grad(dl[l].grad, rl[l].grad, f"class-logit gradient {l}")
        assert float(dm[l].grad.cpu()[~P.permute(0, 2, 1)].abs().max()) == 0.0
        assert float(dl[l].grad.cpu()[labels == -100].abs().max()) == 0.0


def test_padded_losses_refuse_tiles_that_do_not_fit_the_lds():
    """N >= 640 (sums kernel, 64-row tile above 160 KiB) and N >= 1024 (gradient kernel, 16-row tile above 64 KiB) are
    argument errors of the library, returned before anything is launched: the output buffers keep their contents."""
    for N in (640, 1024):
        x, T, P = torch.zeros(1, 16, N, device=DEV), torch.zeros(1, N, 16, device=DEV), torch.ones(1, N, 16, dtype=torch.bool,
                                                                                                 device=DEV)
        with pytest.raises(L.Pq3dError, match=r"pq3d_padded_mask_sums failed \(rc=-1\): .*N too large"):
            padded_mask_losses(x, T, P)
        part = torch.full((1, 1, N, 4), 7.0, device=DEV)
        with pytest.raises(L.Pq3dError, match=r"rc=-1"):
            L.call("pq3d_padded_mask_sums", x, T, P, part, 1, 16, N)
        torch.cuda.synchronize()
        assert float(part.min()) == float(part.max()) == 7.0
    part = torch.full((1, 1, 639, 4), 7.0, device=DEV)                     # the largest N the sums kernel takes
    L.call("pq3d_padded_mask_sums", x[:, :, :639].contiguous(), T[:, :639].contiguous(), P[:, :639].contiguous(), part, 1, 16, 639)
    assert float(part[..., 1].min()) == float(part[..., 1].max()) == 16.0
    sums, g, dX = torch.ones(1, N, 4, device=DEV), torch.ones(1, N, device=DEV), torch.full((1, 16, N), 7.0, device=DEV)
    with pytest.raises(L.Pq3dError, match=r"pq3d_padded_mask_grad failed \(rc=-1\): .*N too large"):
        L.call("pq3d_padded_mask_grad", x, T, P, sums, g, g, dX, 1, 16, N)
    torch.cuda.synchronize()
    assert float(dX.min()) == float(dX.max()) == 7.0
