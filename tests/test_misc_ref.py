"""CPU: the float64 restatements of tests/misc_ref.py against the oracle, and a plain float32 walk of every formula against
its bound, for every case tests/test_gpu_misc_f64.py runs:
  (a) pairwise locations and Fourier features in float64 equal oracle.pq3d_oracle.calc_pairwise_locs / fourier_embed in
      float64 (to 1e-12: the oracle sums through torch's reductions and a matmul, the restatement term by term);
  (b) the float32 restatement of each formula stays under misc_ref.SHARE = 0.6 of its bound;
  (c) the band |v| < 1e-3 holds at most 1 % of the elements of every spatial-bias case, and every case has the one-hot
      positions (v >= 0.1) the backward test needs, at which the float32 one-hot terms stay under 0.6 of 8 u |term|."""

import numpy as np
import pytest
import torch

from oracle import pq3d_oracle as O
from tests import misc_ref as R

U = R.U


def _share(got, want, tol):
    return float((np.abs(np.asarray(got, np.float64) - want) / tol).max()) if np.size(want) else 0.0


# ------------------------------------------------------------------------------------------------ pairwise locations
@pytest.mark.parametrize("L,B", R.PL_CASES)
def test_pairwise_locs_restatement(L, B):
    c = R.pl_centres(L, B)
    ref = R.pairwise_locs(c)
    want = O.calc_pairwise_locs(torch.from_numpy(c).double()).numpy()
    assert ref.shape == (B, L, L, 5) and np.abs(ref - want).max() <= 1e-12
    assert np.abs(ref).max() <= 1 + 1e-12
    f32 = R.pairwise_locs(c, dtype=np.float32)
    assert f32.dtype == np.float32
    share = _share(f32, ref, R.PL_TOL)
    print(f"pairwise_locs L={L} B={B}: float32 error {share * 8:.2f} u")
    assert share <= R.SHARE
    if L == 1:
        assert (f32[..., 0] == 1).all() and (f32[..., 2] == 1).all() and (ref[..., 0] == 1).all() and (ref[..., 2] == 1).all()
    if L >= 6:     # the planted pairs are what they claim to be
        assert (c[0, 0] == c[0, 1]).all() and (c[0, 2, :2] == c[0, 3, :2]).all() and c[0, 2, 2] != c[0, 3, 2]
        assert 5e-7 < abs(float(c[0, 5, 0]) - float(c[0, 4, 0])) < 2e-6
        assert ref[0, 2, 3, 2] < 1e-4 and abs(abs(ref[0, 2, 3, 1]) - 1) < 1e-8      # stacked: d2 / dist ~ 0, dz / dist = -+1


# ------------------------------------------------------------------------------------------------ Fourier features
@pytest.mark.parametrize("half,Na,Nb", R.FOURIER_CASES)
def test_fourier_restatement(half, Na, Nb):
    xa6, xb, cmin, cmax, G = R.fourier_inputs(half, Na, Nb)
    worst = 0.0
    for x in (xa6[..., :3], xb):
        ref, mag = R.fourier(x, cmin, cmax, G)
        want = O.fourier_embed(*(torch.from_numpy(np.ascontiguousarray(a)).double() for a in (x, G, cmin, cmax))).numpy()
        assert ref.shape == (R.FOURIER_B, x.shape[1], 2 * half)
        if x.shape[1]:
            assert np.abs(ref - want).max() <= 1e-12
            t = (x.astype(np.float64) - cmin[:, None]) / (cmax - cmin)[:, None]
            assert t.min() < 0 or t.max() > 1 or x.shape[1] < 5      # some points lie outside the box
        f32, _ = R.fourier(x, cmin, cmax, G, dtype=np.float32)
        assert f32.dtype == np.float32
        worst = max(worst, _share(f32, ref, R.fourier_tol(mag)))
    print(f"fourier half={half} Na={Na} Nb={Nb}: float32 share of the bound {worst:.3f}")
    assert worst <= R.SHARE


# ------------------------------------------------------------------------------------------------ spatial bias
def _sb_case(B, L, H):
    c, W, bw = R.sb_inputs(B, L, H)
    pl = R.pairwise_locs(c, dtype=np.float32)
    v, mag = R.sb_pre(pl, W, bw)
    return pl, W, bw, v, mag


@pytest.mark.parametrize("B,L,H", R.SB_CASES)
def test_spatial_bias_case_conditions_and_forward(B, L, H):
    pl, W, bw, v, mag = _sb_case(B, L, H)
    band = float(R.sb_band(v).mean())
    pos = R.sb_onehot_positions(v, mag)
    print(f"spatial bias B={B} L={L} H={H}: band share {band:.4%}, {len(pos)} one-hot positions")
    assert band <= R.BAND_CAP                                  # (c)
    assert pos and all(v[e // (L * L), h, e % (L * L)] >= R.ONEHOT_MIN_V for e, h in pos)
    for g in range(1, R.sb_groups(B, L, H)):                   # the other groups' weights keep the band condition too
        _, Wg, bg = R.sb_inputs(B, L, H, group=g)
        assert float(R.sb_band(R.sb_pre(pl, Wg, bg)[0]).mean()) <= R.BAND_CAP, g
    out32 = R.sb_fwd(pl, W, bw, dtype=np.float32)
    assert out32.dtype == np.float32
    R.sb_assert_fwd(out32, v, mag, share=R.SHARE, what="float32 restatement")     # (b)


@pytest.mark.parametrize("B,L,H", R.SB_CASES)
def test_spatial_bias_backward_float32_within_share(B, L, H):
    pl, W, bw, v, mag = _sb_case(B, L, H)
    db = R.sb_upstream(B, L, H, v)
    assert (db[R.sb_band(v)] == 0).all()
    dW, dbw = R.sb_bwd(pl, W, bw, db)
    tW, tb = R.sb_bwd_tol(pl, v, mag, db)
    dW32, dbw32 = R.sb_bwd(pl, W, bw, db, dtype=np.float32)
    assert dW32.dtype == np.float32 and dW.shape == (H, 5) and dbw.shape == (H,)
    live = tW > 0
    share = max(_share(dW32[live], dW[live], tW[live]), _share(dbw32[tb > 0], dbw[tb > 0], tb[tb > 0]))
    print(f"spatial bias backward B={B} L={L} H={H}: float32 share of the bound {share:.3f}")
    assert share <= R.SHARE
    assert (dW32[~live] == 0).all() and (dW[~live] == 0).all()
    worst = R.sb_onehot_share32(pl, W, bw, v, R.sb_onehot_positions(v, mag))
    print(f"  one-hot terms: float32 share of 8 u |term| {worst:.3f}")
    assert worst <= R.SHARE


def test_case_seeds_are_the_first_that_meet_the_stated_conditions():
    """Every case misses none of misc_ref.sb_case_misses' conditions at its seed; a case listed in SB_SEED misses one at every
    smaller seed (the seeds answer to these CPU conditions and to nothing else)."""
    assert set(R.SB_SEED) <= set(R.SB_CASES)
    for case in R.SB_CASES:
        seed = R.SB_SEED.get(case, 0)
        assert R.sb_case_misses(*case, seed) == [], case
        for lower in range(seed):
            assert R.sb_case_misses(*case, lower), (case, lower)


def test_spatial_bias_backward_matches_autograd_in_float64():
    B, L, H = 3, 23, 4
    pl, W, bw, v, mag = _sb_case(B, L, H)
    db = R.sb_upstream(B, L, H, v)
    Wt, bt = torch.from_numpy(W).double().requires_grad_(True), torch.from_numpy(bw).double().requires_grad_(True)
    pre = torch.from_numpy(pl).double().reshape(B, L * L, 5) @ Wt.t() + bt
    out = torch.log(torch.clamp(torch.relu(pre), min=float(R.CLAMP32))).permute(0, 2, 1)
    assert np.abs(out.detach().numpy() - R.sb_fwd(pl, W, bw)).max() <= 1e-12
    out.backward(torch.from_numpy(db).double())
    dW, dbw = R.sb_bwd(pl, W, bw, db)
    assert np.abs(Wt.grad.numpy() - dW).max() <= 1e-9 and np.abs(bt.grad.numpy() - dbw).max() <= 1e-9


@pytest.mark.parametrize("n,want", [(1, [0]), (256, [0, 255]), (1024, [0, 255, 256, 511, 512, 767, 768, 1023]),
                                    (1089, [0, 255, 256, 511, 512, 767, 768, 1023, 1024, 1088])])
def test_onehot_elements_small(n, want):
    assert R.sb_onehot_elements(n) == want


def test_onehot_elements_grid_capped_case():
    B, L, _ = R.SB_BIG
    n = B * L * L
    st = 512 * 256
    assert n > 4 * st                   # the kernel's walk needs a second iteration
    el = R.sb_onehot_elements(n)
    for e in (0, n - 1, 255, 256, st - 1, st, 2 * st, 3 * st, 4 * st - 1, 4 * st, (n - 1) // 256 * 256):
        assert e in el
    assert all(e - 1 in el and e in el for e in range(256, n, 256))      # both sides of every one of the 2064 block boundaries
    assert len(el) == 2 + 2 * ((n - 1) // 256) == 4130


# ------------------------------------------------------------------------------------------------ gate mix, gelu backward
@pytest.mark.parametrize("n", R.GATE_N)
def test_gate_mix_float32_within_share(n):
    for k in (range(5) if n < 5 else (0,)):
        q, u, g, dy = R.gate_inputs(n, k)
        ref = R.gate_mix(q, u, g, dy)
        f32 = R.gate_mix(q, u, g, dy, dtype=np.float32)
        for name, a, r, t in zip(("y", "dq", "du", "dg"), f32, ref, R.gate_tols(q, u, dy)):
            assert a.dtype == np.float32
            nz = t > 0
            assert _share(a[nz], r[nz], t[nz]) <= R.SHARE, (name, n, k)
        hi, lo = g == 100, g == -100
        assert (f32[0][hi] == u[hi]).all() and (f32[0][lo] == q[lo]).all()
    if n >= 5:
        assert set(R.GATE_SPECIAL) <= set(g.tolist())


@pytest.mark.parametrize("n", R.ACT_N)
def test_gelu_backward_float32_within_share(n):
    for k in (range(8) if n < 8 else (0,)):
        dy, sv = (torch.from_numpy(a) for a in R.act_inputs(n, k))
        for saved in (sv, sv.bfloat16().float()):
            ref = R.act_bwd(dy, saved, "gelu")
            f32 = R.act_bwd(dy, saved, "gelu", dtype=torch.float32)
            assert f32.dtype == torch.float32
            assert float(((f32.double() - ref).abs() / R.gelu_bwd_tol(dy)).max()) <= R.SHARE
    x = torch.tensor([0.0, 1e-30, 6.0, -6.0], dtype=torch.float64)
    want = [0.5, 0.5, 1.0, 0.0]
    assert all(abs(float(a) - b) < 1e-7 for a, b in zip(R.gelu_grad(x), want))
    xg = torch.linspace(-4, 4, 33, dtype=torch.float64, requires_grad=True)      # the closed form is gelu's derivative
    torch.nn.functional.gelu(xg).sum().backward()
    assert float((xg.grad - R.gelu_grad(xg.detach())).abs().max()) < 1e-12


def test_sum_left_to_right_is_sequential_fp32():
    parts = [np.float32([1.0, 2.0 ** 24]), np.float32([2.0 ** -24, 1.0]), np.float32([2.0 ** -24, 1.0])]
    assert R.sum_left_to_right(parts).tolist() == [1.0, 2.0 ** 24]      # each addend is rounded away on its own
    assert R.sum_left_to_right(parts[::-1]).tolist() == [np.float32(1.0 + 2.0 ** -23), 2.0 ** 24 + 2.0]
