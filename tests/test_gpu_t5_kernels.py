"""GPU: the caption head's T5 kernels (pq3d_rmsnorm_fwd / _bwd_res_drop, pq3d_embedding_* with and without dropout,
pq3d_t5_prep, pq3d_t5_bias_bwd, pq3d_sum_n behind ops.fanout) against the float64 restatements of tests/t5_ref.py (kept
honest by tests/test_t5_ref.py), every element, through the ops wrappers; and the gradients of every T5-body parameter of
pq3d_amd.t5.decoder_logits against HF T5ForConditionalGeneration in float64.

Tolerances of the single-launch kernels: K * u * abs-bound, u = 2^-24, abs-bound = the restated expression with every term
replaced by its absolute value (t5_ref.*_abs).
  y, rstd   K = 32   the sum of squares is a positive-term sum of depth <= PL + 6 <= 38 (PL values per lane, six wave_sum
                     levels), the rsqrt halves its relative error to ~19u; division, eps, sqrt, reciprocal, two products
  dx        K = 64   the same depth for mean(g xh), relative to mean(|g xh|), and the products / the residual add around it.
                     The float64 backward reads the rstd the forward KERNEL stored (as the backward kernel does), so the
                     forward's error is not counted twice
  gathers   equality (embedding forward, t5_prep's ids / bias / kpm: copies)
  dw, dtable, drel   K = n + 8, n = the number of addends of that entry (rows; occurrences of the id; scenes x causal pairs
                     of the bucket): n - 1 additions in any order (atomics, trees) and at most two roundings per addend
An entry whose sum is empty has abs-bound 0: it must be exactly 0.

RMSNorm instantiations reached, by d: 48, 64 -> PL 1; 100, 128 -> 2; 192, 256 -> 4; 512 -> 8; 768, 1024 -> 16;
1152, 2048 -> 32.  R = 4101 at d = 64: 1026 row blocks > the backward's 1024-block cap, so waves 0..4 take two rows.

Body gradients: HIP fp32 against the same HF module in float64 on the host (relative L2 error per tensor), bounded by 8 x
E32, the error of the stock HF module in float32 on the host against the same float64 run, measured in the test itself.
The float64 copy's T5LayerNorm forwards are replaced by t5_ref.rmsnorm: HF's own forms the variance in float32 whatever
the module's dtype (``hidden_states.to(torch.float32).pow(2).mean(-1)``), which would leave fp32-sized errors, correlated
with the float32 run's, in the "float64" reference.
Measured on an MI355X, relative L2 error against float64 (B 3, N 7 ragged, fixture F8's architecture, random weights;
T = 33 and tie_word_embeddings=False take the fused pq3d_t5_prep branch of decoder_logits, T = 115 the separate ops;
the largest HIP / E32 ratio is 1.66, the bound 8):
  tensor (decoder., .weight dropped)        T = 33              tie_word_embeddings=False   T = 115 (separate prep ops)
                                            E32      HIP        E32      HIP                E32      HIP
  logits                                    3.43e-07 3.51e-07   3.43e-07 3.51e-07           3.46e-07 3.45e-07
  d_enc                                     4.33e-07 4.92e-07   4.13e-07 5.08e-07           4.22e-07 5.74e-07
  shared                                    4.04e-07 4.37e-07   4.06e-07 4.54e-07           4.30e-07 4.53e-07
  block.0.layer.0.SelfAttention.q           5.44e-07 5.59e-07   5.17e-07 5.79e-07           5.77e-07 6.20e-07
  block.0.layer.0.SelfAttention.k           5.59e-07 5.73e-07   5.30e-07 6.05e-07           5.99e-07 6.78e-07
  block.0.layer.0.SelfAttention.v           4.47e-07 4.68e-07   4.60e-07 5.01e-07           5.39e-07 5.65e-07
  block.0.layer.0.SelfAttention.o           4.94e-07 4.75e-07   4.75e-07 4.98e-07           5.30e-07 5.06e-07
  block.0.layer.0.SelfAttention.rel_bias    4.90e-07 5.74e-07   5.51e-07 6.53e-07           6.69e-07 6.94e-07
  block.0.layer.0.layer_norm                5.69e-07 5.45e-07   5.35e-07 6.18e-07           3.76e-07 6.23e-07
  block.0.layer.1.EncDecAttention.q         4.78e-07 4.64e-07   4.77e-07 5.65e-07           5.45e-07 5.75e-07
  block.0.layer.1.EncDecAttention.k         5.13e-07 4.86e-07   4.98e-07 6.16e-07           4.65e-07 5.51e-07
  block.0.layer.1.EncDecAttention.v         3.99e-07 4.03e-07   3.89e-07 4.28e-07           3.80e-07 4.41e-07
  block.0.layer.1.EncDecAttention.o         4.34e-07 4.49e-07   4.12e-07 4.34e-07           4.26e-07 4.19e-07
  block.0.layer.1.layer_norm                5.99e-07 5.34e-07   5.53e-07 6.92e-07           5.46e-07 6.18e-07
  block.0.layer.2.DenseReluDense.wi         4.16e-07 4.28e-07   4.18e-07 4.29e-07           4.55e-07 4.68e-07
  block.0.layer.2.DenseReluDense.wo         3.69e-07 3.85e-07   3.80e-07 3.95e-07           4.59e-07 4.98e-07
  block.0.layer.2.layer_norm                4.27e-07 4.67e-07   4.44e-07 5.07e-07           4.11e-07 4.67e-07
  block.1.layer.0.SelfAttention.q           8.83e-07 9.05e-07   9.03e-07 9.78e-07           8.00e-07 8.05e-07
  block.1.layer.0.SelfAttention.k           8.96e-07 9.10e-07   8.98e-07 9.47e-07           8.02e-07 8.68e-07
  block.1.layer.0.SelfAttention.v           4.02e-07 3.93e-07   4.05e-07 3.96e-07           4.70e-07 5.22e-07
  block.1.layer.0.SelfAttention.o           3.71e-07 3.91e-07   3.95e-07 4.03e-07           4.19e-07 4.32e-07
  block.1.layer.0.layer_norm                4.61e-07 4.79e-07   4.55e-07 5.09e-07           4.06e-07 4.73e-07
  block.1.layer.1.EncDecAttention.q         5.82e-07 6.40e-07   5.62e-07 5.83e-07           5.22e-07 5.39e-07
  block.1.layer.1.EncDecAttention.k         6.66e-07 6.21e-07   5.54e-07 6.19e-07           3.96e-07 4.75e-07
  block.1.layer.1.EncDecAttention.v         3.36e-07 3.62e-07   3.29e-07 3.48e-07           4.09e-07 4.91e-07
  block.1.layer.1.EncDecAttention.o         3.87e-07 3.90e-07   3.92e-07 3.97e-07           4.46e-07 4.30e-07
  block.1.layer.1.layer_norm                4.41e-07 4.97e-07   4.76e-07 4.97e-07           6.17e-07 7.12e-07
  block.1.layer.2.DenseReluDense.wi         4.35e-07 4.41e-07   4.44e-07 4.38e-07           4.54e-07 4.51e-07
  block.1.layer.2.DenseReluDense.wo         4.16e-07 4.31e-07   4.18e-07 4.26e-07           4.55e-07 4.73e-07
  block.1.layer.2.layer_norm                4.60e-07 4.84e-07   4.94e-07 5.46e-07           5.06e-07 5.60e-07
  final_layer_norm                          3.86e-07 3.78e-07   3.40e-07 3.70e-07           2.81e-07 4.13e-07"""
import copy
import functools
import types

import pytest
import torch

from pq3d_amd import _lib as L
from pq3d_amd import ops, synth, t5
from tests import t5_ref as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
EPS = 1e-6
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def within(got, want, tol, what=""):
    """|got - want| <= tol for EVERY element (float64 on the host); the message names the worst one."""
    got, want = got.detach().to("cpu", F64), want.to(F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite"
    err = (got - want).abs()
    bad = err > tol
    if bool(bad.any()):
        i = int((err - tol).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} outside; worst at flat {i}: got {got.flatten()[i]:.9g} "
                             f"want {want.flatten()[i]:.9g} err {err.flatten()[i]:.3g} tol {tol.expand_as(err).flatten()[i]:.3g}")


# ------------------------------------------------------------------------------------------------ RMSNorm
RMS_D = [48, 64, 100, 128, 192, 256, 512, 768, 1024, 1152, 2048]
RMS_SHAPES = [(r, d) for d in RMS_D for r in (1, 5, 37)] + [(4101, 64)]


@functools.lru_cache(maxsize=None)
def rms_case(Rr, d):
    """x (a row x 1e3, a row x 1e-4 and an all-zero row when there are >= 5 rows), w around 1 with negative entries, the two
    upstream gradients, and the float64 forward: computed once per shape, shared by the routes, never written to."""
    g = gen(1000 * d + Rr)
    x = torch.randn(Rr, d, generator=g)
    if Rr >= 5:
        x[1] *= 1e3
        x[2] *= 1e-4
        x[3] = 0
    w = 1 + 0.3 * torch.randn(d, generator=g)
    w[::5] *= -1
    dy, dres = torch.randn(Rr, d, generator=g), torch.randn(Rr, d, generator=g)
    y64, r64 = R.rmsnorm(x, w, EPS)
    return x, w, dy, dres, y64, r64


def check_rms_backward(x, w, rstd_dev, dy, dres, dx, dw, extra_dw=None):
    want_dx, want_dw = R.rmsnorm_bwd(x, w, rstd_dev, dy, dres)
    ax, aw = R.rmsnorm_bwd_abs(x, w, rstd_dev, dy, dres)
    n = x.shape[0]
    within(dx, want_dx, 64 * U * ax, "dx")
    if extra_dw is not None:      # accumulate = 1: one more addend
        want_dw, aw, n = want_dw + extra_dw.to(F64), aw + extra_dw.to(F64).abs(), n + 1
    assert float(aw.min()) > 0
    within(dw, want_dw, (n + 8) * U * aw, "dw")


@pytest.mark.parametrize("route", ["rmsnorm", "res_both", "res_y_only", "res_passthrough_only"])
@pytest.mark.parametrize("Rr,d", RMS_SHAPES)
def test_rmsnorm_forward_and_backward(Rr, d, route):
    x, w, dy, dres, y64, r64 = rms_case(Rr, d)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    if route == "rmsnorm":
        y, x2 = ops.rmsnorm(xg, wg, EPS), None
    else:
        y, x2 = ops.rmsnorm_res(xg, wg, EPS)
        assert torch.equal(x2, xg)
    rstd = y.grad_fn.saved_tensors[2]
    within(y, y64, 32 * U * y64.abs(), "y")
    within(rstd, r64, 32 * U * r64, "rstd")
    if Rr >= 5:
        assert bool((y[3] == 0).all()) and abs(float(rstd[3]) - 1e3) <= 32 * U * 1e3
    if route == "res_passthrough_only":
        # the norm's output unused: autograd materialises its gradient as zeros (the Function does not switch that off), so the
        # backward kernel DOES launch, with dy = 0: dx = 0 + dres bit for bit, dw = 0
        x2.backward(dres.to(DEV))
        assert torch.equal(xg.grad.cpu(), dres)
        assert wg.grad is not None and wg.grad.shape == (d,) and not bool(wg.grad.any())
        return
    if route == "res_both":                   # both gradients arrive in ONE backward launch, summed in the kernel
        torch.autograd.backward([y, x2], [dy.to(DEV), dres.to(DEV)])
    else:
        y.backward(dy.to(DEV))
    check_rms_backward(x, w, rstd, dy, dres if route == "res_both" else None, xg.grad, wg.grad)
    if Rr >= 5:                               # zero row: dx = r g (+ dres), to the last bit of the float64 value's rounding
        extra = dres[3].double() if route == "res_both" else torch.zeros(d, dtype=F64)
        within(xg.grad[3], 1e3 * dy[3].double() * w.double() + extra, 64 * U * (1e3 * (dy[3] * w).abs().double() + extra.abs()),
               "dx of the zero row")


def test_rmsnorm_backward_without_a_gradient_for_y_launches_nothing():
    """_RMSNorm.backward's `dy is None` branch returns the residual's gradient as it is.  autograd never passes None here (see
    the pass-through route above), so the branch is entered the only way it can be: called on the saved context."""
    x, w, _dy, dres, _y64, _r64 = rms_case(5, 100)
    y, _x2 = ops.rmsnorm_res(x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True), EPS)
    dres_d = dres.to(DEV)
    out = ops._RMSNorm.backward(y.grad_fn, None, dres_d)
    assert len(out) == 5 and out[0] is dres_d and all(o is None for o in out[1:])


@pytest.mark.parametrize("Rr,d", [(5, 100), (37, 512), (5, 2048), (4101, 64)])
def test_rmsnorm_backward_accumulates_onto_a_prefilled_dw(Rr, d):
    x, w, dy, dres, _y64, _r64 = rms_case(Rr, d)
    xd, wd, dyd, dresd = (t.to(DEV) for t in (x, w, dy, dres))
    y, rstd, dx = torch.empty_like(xd), torch.empty(Rr, device=DEV), torch.full_like(xd, float("nan"))
    L.call("pq3d_rmsnorm_fwd", xd, wd, y, rstd, Rr, d, EPS)
    prefill = torch.randn(d, generator=gen(d)) * 3
    dw = prefill.to(DEV)
    L.call("pq3d_rmsnorm_bwd_res_drop", xd, wd, rstd, dyd, dresd, dx, dw, Rr, d, 1, None, None)
    check_rms_backward(x, w, rstd, dy, dres, dx, dw, extra_dw=prefill)
    dw0 = torch.full((d,), float("nan"), device=DEV)          # accumulate = 0 overwrites whatever was there
    L.call("pq3d_rmsnorm_bwd_res_drop", xd, wd, rstd, dyd, dresd, dx, dw0, Rr, d, 0, None, None)
    check_rms_backward(x, w, rstd, dy, dres, dx, dw0)


def ulps_apart(a, b):
    """Distance in fp32 units in the last place (both finite, same sign or zero)."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return (ia - ib).abs()


@pytest.mark.parametrize("d", [100, 512])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_rmsnorm_backward_writes_the_dropout_masked_copy(p, d):
    Rr = 37
    x, w, dy, dres, _y64, _r64 = rms_case(Rr, d)
    drop = ops.make_drop(p, (9 << 20) + d, torch.device(DEV))
    keep = ops.dropout_mask(Rr, d, drop).cpu()
    assert 0 < int(keep.sum()) < keep.numel()
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    slot = {}
    y, x2 = ops.rmsnorm_res(xg, wg, EPS, grad_drop=(drop, slot))
    rstd = y.grad_fn.saved_tensors[2]
    torch.autograd.backward([y, x2], [dy.to(DEV), dres.to(DEV)])
    check_rms_backward(x, w, rstd, dy, dres, xg.grad, wg.grad)
    assert set(slot) == {"g", "of"} and torch.equal(slot["of"], xg.grad)
    dx, gm = xg.grad.cpu(), slot["g"].cpu()
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))          # fp32, as the kernels form it
    assert abs(float(scale) - 1 / (1 - p)) <= 4 * U / (1 - p)
    assert bool((gm[~keep] == 0).all())
    assert bool(torch.isfinite(gm).all()) and int(ulps_apart(gm[keep], (dx * scale)[keep]).max()) <= 1


def test_rmsnorm_rejects_rows_wider_than_2048():
    x, w = torch.zeros(2, 2049, device=DEV), torch.ones(2049, device=DEV)
    with pytest.raises(L.Pq3dError, match="pq3d_rmsnorm_fwd"):
        ops.rmsnorm(x, w, EPS)
    r, dx, dw = torch.ones(2, device=DEV), torch.zeros_like(x), torch.full((2049,), 7.0, device=DEV)
    with pytest.raises(L.Pq3dError, match="pq3d_rmsnorm_bwd"):
        L.call("pq3d_rmsnorm_bwd_res_drop", x, w, r, x, None, dx, dw, 2, 2049, 0, None, None)
    assert bool((dw == 7).all())          # the check precedes the zero-fill of dw: nothing launched


# ------------------------------------------------------------------------------------------------ embedding
EMB_ROWS = 50


def emb_ids(layout, g):
    """[3, 17] int64.  'spread': 51 ids cannot all differ in a 50-row table -- every row once, one of them twice."""
    if layout == "equal":
        return torch.full((3, 17), 23, dtype=torch.int64)
    if layout == "spread":
        return torch.randperm(EMB_ROWS, generator=g)[torch.arange(51) % EMB_ROWS].view(3, 17)
    if layout == "random":
        return torch.randint(0, EMB_ROWS, (3, 17), generator=g)
    return torch.randint(0, EMB_ROWS, (2100,), generator=g)      # 'long': R d = 2100 x 512 > 4096 blocks x 256 threads


def check_embedding(layout, d, p):
    g = gen(31 * d + len(layout))
    ids = emb_ids(layout, g)
    table = torch.randn(EMB_ROWS, d, generator=g)
    dout = torch.randn(*ids.shape, d, generator=g)
    drop = ops.make_drop(p, (10 << 20) + d, torch.device(DEV)) if p else None
    keep = ops.dropout_mask(ids.numel(), d, drop).cpu() if p else None
    tg = table.to(DEV).requires_grad_(True)
    out = ops.embedding(tg, ids.to(DEV), drop=drop)
    assert out.shape == (*ids.shape, d) and out.dtype == torch.float32
    if p:
        want = R.embedding(table, ids, keep, p)
        within(out, want, 4 * U * want.abs(), "embedding with dropout")    # the fp32 1 / (1 - p) and one product
        assert bool((out.cpu()[~keep.view_as(out)] == 0).all())
    else:
        assert torch.equal(out.cpu(), table[ids])
    out.backward(dout.to(DEV))
    want = R.embedding_bwd(dout, ids, EMB_ROWS, keep, p)
    ab = R.embedding_bwd_abs(dout, ids, EMB_ROWS, keep, p)
    n = R.embedding_bwd_terms(ids, EMB_ROWS)
    if not p:
        assert bool((ab[n > 0] > 0).all())
    within(tg.grad, want, (n[:, None] + 8) * U * ab, "dtable")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", ["equal", "spread", "random"])
@pytest.mark.parametrize("d", [1, 7, 64, 512])
def test_embedding_forward_and_table_gradient(d, layout, p):
    check_embedding(layout, d, p)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embedding_grid_stride_loop(p):
    check_embedding("long", 512, p)


# ------------------------------------------------------------------------------------------------ t5_prep forward
def prep_labels(B, T, g):
    """Random labels in [6, 900); -100 at position 0, in the middle and in the last place (of scenes 0, 1 % B, 2 % B); every
    other last label is 999, which occurs nowhere else: the last label is never a decoder input."""
    lab = torch.randint(6, 900, (B, T), generator=g)
    lab[:, T - 1] = 999
    lab[0, 0] = -100
    lab[1 % B, T // 2] = -100
    lab[2 % B, T - 1] = -100
    if T == 1 and B == 1:
        lab[0, 0] = 999
    return lab


@pytest.mark.parametrize("B,T,H,N", [(1, 1, 1, 1), (3, 33, 4, 7), (11, 114, 8, 100), (2, 5, 6, None)])
def test_t5_prep_forward(B, T, H, N):
    g = gen(B * 1000 + T)
    NB, start, pad = 32, 3, 5
    lab = prep_labels(B, T, g)
    rel = torch.randn(NB, H, generator=g)
    buckets = t5.relative_buckets(T, NB, 128, "cpu")
    ev = (torch.rand(B, N, generator=g) < 0.6) if N is not None else None
    ids, bias, kpm = ops.t5_prep(rel.to(DEV), lab.to(DEV), buckets.to(DEV), ev.to(DEV) if ev is not None else None, start, pad, H)
    wi, wb, wk = R.t5_prep(rel, lab, buckets, ev, start, pad, H)
    assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), wi)
    assert not bool((ids == 999).any()) and not bool((ids == -100).any()) and bool((ids[:, 0] == start).all())
    if T >= 3:
        assert int(ids[1 % B, T // 2 + 1]) == pad
    assert bias.dtype == torch.float32 and bias.shape == (B, H, T, T)
    assert torch.equal(bias.cpu(), wb)                          # a gather plus -inf: bit-equal (torch.equal: -inf == -inf)
    if N is None:
        assert kpm is None
    else:
        assert kpm.dtype == torch.bool and torch.equal(kpm.cpu(), wk)


# ------------------------------------------------------------------------------------------------ t5_bias_bwd
BUCKET_CFG = {32: 128, 8: 16, 40: 128, 256: 512}      # num_buckets -> max_distance


# every B x T x (NB, H) whose dbias stays within 4 MB: at T = 114 that leaves H = 12 to B = 1 (B = 8, 9, 17 meet H = 12 at T = 33)
BIAS_CASES = [(B, T, NB, H) for B in (1, 8, 9, 17) for T in (1, 2, 33, 114) for NB, H in ((32, 4), (8, 1), (40, 12), (256, 2))
              if B * H * T * T * 4 <= 4 << 20]


@pytest.mark.parametrize("B,T,NB,H", BIAS_CASES)
def test_t5_bias_bwd(B, T, NB, H):
    check_bias_bwd(B, T, NB, H, t5.relative_buckets(T, NB, BUCKET_CFG[NB], "cpu"))


def test_t5_bias_bwd_bucket_ids_up_to_255():
    """The kernel keeps the bucket ids in LDS as bytes.  relative_buckets gives none above 113 at T <= 114, so this table is
    made by hand: every id of 0..255 but a few, with 127, 128 and 255 (where a signed byte would turn) among the causal pairs."""
    T, NB = 33, 256
    buckets = torch.randint(0, NB, (T, T), generator=gen(255))
    buckets[buckets == 200] = 201                      # one id certainly empty
    buckets[5, 2], buckets[6, 3], buckets[7, 7], buckets[32, 0] = 127, 128, 255, 255
    n = R.t5_bias_bwd_terms(buckets, NB, 1)
    assert int(n[200]) == 0 and int((n[128:] > 0).sum()) > 100 and int(n[255]) >= 2
    check_bias_bwd(3, T, NB, 2, buckets)


def check_bias_bwd(B, T, NB, H, buckets):
    g = gen(B * 100000 + T * 300 + NB)
    dbias = torch.randn(B, H, T, T, generator=g)
    dbias.masked_fill_(torch.ones(T, T, dtype=torch.bool).triu(1), 1e30)          # above the diagonal: ignored by contract
    want, ab, n = R.t5_bias_bwd(dbias, buckets, NB), R.t5_bias_bwd_abs(dbias, buckets, NB), R.t5_bias_bwd_terms(buckets, NB, B)
    assert bool((ab[n > 0] > 0).all()) and float(ab.max()) < 1e6
    tol = (n[:, None] + 8) * U * ab
    lab = torch.zeros(B, T, dtype=torch.int64, device=DEV)
    bd, dbd = buckets.to(DEV), dbias.to(DEV)

    def through_the_wrapper():
        rel = torch.randn(NB, H, generator=gen(1)).to(DEV).requires_grad_(True)
        _ids, bias, _ = ops.t5_prep(rel, lab, bd, None, 0, 0, H)
        bias.backward(dbd)
        return rel.grad
    drel = through_the_wrapper()
    within(drel, want, tol, "drel")
    assert bool((drel.cpu()[n == 0] == 0).all())                 # a bucket no causal pair falls in: exactly 0
    assert torch.equal(through_the_wrapper(), drel)              # fixed summation order: bit-identical
    prefill = torch.randn(NB, H, generator=g) * 3
    acc = prefill.to(DEV)
    L.call("pq3d_t5_bias_bwd", dbd, bd, acc, B, T, H, NB, 1)
    within(acc, want + prefill.double(), (n[:, None] + 9) * U * (ab + prefill.double().abs()), "drel, accumulate = 1")
    assert torch.equal(acc.cpu()[n == 0], prefill[n == 0])       # ... and unchanged there with accumulate = 1


def test_t5_bias_bwd_rejects_T_115():
    T = 115
    assert T * T > 114 * 114 and T * T * 5 + 16 > 64 * 1024 >= 114 * 114 * 5 + 16
    dbias, buckets = torch.zeros(1, 1, T, T, device=DEV), torch.zeros(T, T, dtype=torch.int64, device=DEV)
    drel = torch.full((32, 1), 7.0, device=DEV)
    with pytest.raises(L.Pq3dError, match="pq3d_t5_bias_bwd"):
        L.call("pq3d_t5_bias_bwd", dbias, buckets, drel, 1, T, 1, 32, 0)
    assert bool((drel == 7).all())


# ------------------------------------------------------------------------------------------------ fanout
@pytest.mark.parametrize("n", [2, 3, 6])
def test_fanout_sums_the_consumers_gradients(n):
    g = gen(n)
    x = torch.randn(3, 4, 33, 33, generator=g)
    gs = [torch.randn(3, 4, 33, 33, generator=g) for _ in range(n)]
    ws = [0.5 + 0.75 * i for i in range(n)]
    xg = x.to(DEV).requires_grad_(True)
    outs = ops.fanout(xg, n)
    assert len(outs) == n and all(torch.equal(o, xg) for o in outs)
    sum(wi * (o * gi.to(DEV)).sum() for wi, o, gi in zip(ws, outs, gs)).backward()
    want = sum(wi * gi.double() for wi, gi in zip(ws, gs))
    ab = sum(wi * gi.double().abs() for wi, gi in zip(ws, gs))
    within(xg.grad, want, (n + 8) * U * ab, "fanout gradient")


def test_fanout_fallback_with_a_bf16_gradient():
    """autograd casts a consumer's gradient to the output's dtype before the node sees it, so the mixed-dtype branch is
    entered the only way it can be: _Fanout.backward called with the gradients."""
    g = gen(4)
    gs = [torch.randn(2, 36, generator=g).to(DEV) for _ in range(3)]
    gs[1] = gs[1].to(torch.bfloat16)
    got, none = ops._Fanout.backward(None, *gs)
    assert none is None and got.dtype == torch.float32
    want = sum(t.double().cpu() for t in gs)
    within(got, want, (3 + 8) * U * sum(t.double().cpu().abs() for t in gs), "fallback sum")
    same = ops._Fanout.backward(None, *[t.float() for t in gs])[0]       # the one-launch route on the same values
    within(same, want, (3 + 8) * U * sum(t.double().cpu().abs() for t in gs), "pq3d_sum_n")


# ------------------------------------------------------------------------------------------------ body gradients
def rel_l2(a, ref):
    a, ref = a.detach().to("cpu", F64), ref.detach().to(F64)
    return float((a - ref).norm() / ref.norm())


def hf_run(model, enc, enc_valid, labels):
    """logits, d enc and the gradient of every parameter HF's backward reaches; loss = cross-entropy on the logits."""
    from transformers.modeling_outputs import BaseModelOutput
    model.zero_grad(set_to_none=True)
    e = enc.detach().clone().to(next(model.parameters()).dtype).requires_grad_(True)
    logits = model(encoder_outputs=BaseModelOutput(last_hidden_state=e), attention_mask=enc_valid, labels=labels).logits
    torch.nn.functional.cross_entropy(logits.flatten(0, 1), labels.flatten(), ignore_index=-100).backward()
    out = {"logits": logits.detach(), "d_enc": e.grad}
    out.update({k: p.grad for k, p in model.named_parameters() if p.grad is not None})
    return out


def float64_copy(model):
    """The module in float64 with the variance of its T5LayerNorms in float64 too (module docstring)."""
    from transformers.models.t5.modeling_t5 import T5LayerNorm
    m = copy.deepcopy(model).double()

    def forward(self, hidden_states):
        return R.rmsnorm(hidden_states, self.weight, self.variance_epsilon)[0]
    for mod in m.modules():
        if isinstance(mod, T5LayerNorm):
            mod.forward = types.MethodType(forward, mod)
    return m


@pytest.mark.parametrize("variant,T,tie", [("fused prep", 33, True), ("tie_word_embeddings = False", 33, False), ("T = 115: separate prep ops", 115, True)])
def test_body_gradients_against_hf_float64(variant, T, tie):
    from transformers import T5Config, T5ForConditionalGeneration
    _z, a = util.load_fixture("F8_t5_head")
    cfg = T5Config(**dict(a["hf_config"]), tie_word_embeddings=tie)
    m32 = T5ForConditionalGeneration(cfg)
    # transformers 5 keeps the weights tied whatever the configuration says and reads tie_word_embeddings = False as "do not
    # scale the decoder output by d_model^-0.5"; earlier versions also untie lm_head.  Either way the variant differs.
    untied = m32.lm_head.weight is not m32.shared.weight
    assert t5.scales_decoder_output(cfg) == tie and (not untied or not tie)
    synth.fill_module(m32, 21)
    m32.eval()
    B, N, d = 3, 7, cfg.d_model
    g = gen(T)
    enc = torch.randn(B, N, d, generator=g)
    enc_valid = torch.arange(N)[None] < torch.tensor([N, 3, 5])[:, None]
    labels = torch.randint(2, cfg.vocab_size, (B, T), generator=g)
    labels[1, T - 8:] = -100
    ref = hf_run(float64_copy(m32), enc, enc_valid, labels)
    cpu32 = hf_run(m32, enc, enc_valid, labels)

    mg = copy.deepcopy(m32).to(DEV)
    mg.zero_grad(set_to_none=True)
    eg, lg = enc.to(DEV).requires_grad_(True), labels.to(DEV)
    fused = T * T <= 114 * 114
    logits = t5.decoder_logits(mg, eg, enc_valid.to(DEV), lg, L.F32, training=False)
    torch.nn.functional.cross_entropy(logits.flatten(0, 1), lg.flatten(), ignore_index=-100).backward()
    got = {"logits": logits.detach(), "d_enc": eg.grad}
    got.update({k: p.grad for k, p in mg.named_parameters() if p.grad is not None})

    names = list(ref)
    need = ["shared.weight", "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", "decoder.final_layer_norm.weight"]
    need += [f"decoder.block.{i}.layer.{j}.layer_norm.weight" for i in range(cfg.num_decoder_layers) for j in range(3)]
    need += [f"decoder.block.{i}.layer.{j}.{att}.{w}.weight" for i in range(cfg.num_decoder_layers)
             for j, att in ((0, "SelfAttention"), (1, "EncDecAttention")) for w in "qkvo"]
    need += [f"decoder.block.{i}.layer.2.DenseReluDense.{w}.weight" for i in range(cfg.num_decoder_layers) for w in ("wi", "wo")]
    need += ["lm_head.weight"] if untied else []
    assert set(need) <= set(names), sorted(set(need) - set(names))
    assert not any(k.startswith("encoder.") for k in names) and set(got) == set(names), sorted(set(got) ^ set(names))
    failures = []
    print(f"\nbody gradients, {variant} (fused t5_prep branch: {fused}): relative L2 error against float64")
    for k in names:
        assert k in got, f"{k}: HF gives a gradient, the HIP body none"
        if not bool(ref[k].any()):
            assert not bool(got[k].any()), f"{k}: identically zero in float64, not on the HIP body"
            continue
        e32, ehip = rel_l2(cpu32[k], ref[k]), rel_l2(got[k], ref[k])
        print(f"  {k:75s} E32 {e32:.3e}   HIP {ehip:.3e}   ratio {ehip / e32 if e32 else float('inf'):.2f}")
        if not ehip <= 8 * e32:
            failures.append((k, e32, ehip))
    assert not failures, failures
