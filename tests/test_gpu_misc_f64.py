"""GPU: the small kernels of pq3d_amd/csrc/misc.hip against the float64 restatements of tests/misc_ref.py on the same fp32
inputs, or -- where the fp32 arithmetic is reproducible on the CPU -- against the exact fp32 / bf16 bits.  The bounds are
derived in tests/misc_ref.py (u = 2^-24) and shown on the CPU to leave room by tests/test_misc_ref.py; the case lists are the
ones that file walks.  Shapes are the smallest at which each kernel changes path: block and stride edges, the grid caps, the
chunking of the wrappers at 32 tensors, odd lengths, views that start inside a 16-byte piece."""
import functools
import itertools

import numpy as np
import pytest
import torch

from pq3d_amd import _lib as L
from pq3d_amd import ops
from tests import misc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
F32, BF16 = torch.float32, torch.bfloat16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy() if t.dtype == BF16 else t.detach().cpu().numpy()


def within(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    if want.size == 0:
        return
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    share = float(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0)).max())
    print(f"{what}: worst error {err.max():.3e}, {share:.3f} of its bound")
    assert share <= 1.0, (what, share)


def same_bits(got: torch.Tensor, want: torch.Tensor, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int32 if got.dtype == F32 else torch.int16
    a, b = got.detach().cpu().contiguous().view(it), want.detach().cpu().contiguous().view(it)
    bad = int((a != b).sum())
    assert bad == 0, (what, f"{bad} of {a.numel()} elements differ")


# ------------------------------------------------------------------------------------------------ pairwise locations
@pytest.mark.parametrize("L_,B", R.PL_CASES)
def test_pairwise_locs(L_, B):
    c = R.pl_centres(L_, B)
    ref = R.pairwise_locs(c)
    ct = dev(c)
    six = torch.randn(B, L_, 6, device=DEV)
    six[..., :3] = ct
    wide = torch.randn(B, L_ + 2, 3, device=DEV)
    wide[:, :L_] = ct
    layouts = {"contiguous": ct, "stride 6": six[..., :3], "batch-strided": wide[:, :L_]}
    assert layouts["stride 6"].stride(1) == 6 and layouts["batch-strided"].stride(0) != L_ * 3
    for name, x in layouts.items():
        out = host(ops.pairwise_locs(x))
        within(out, ref, R.PL_TOL, f"pairwise_locs L={L_} B={B} {name}")
        if L_ == 1:
            assert (out[..., 0] == 1).all() and (out[..., 2] == 1).all()


# ------------------------------------------------------------------------------------------------ Fourier features
@pytest.mark.parametrize("half,Na,Nb", R.FOURIER_CASES)
def test_fourier_and_fourier_pair(half, Na, Nb):
    xa6, xb, cmin, cmax, G = R.fourier_inputs(half, Na, Nb)
    (refa, maga), (refb, magb) = R.fourier(xa6[..., :3], cmin, cmax, G), R.fourier(xb, cmin, cmax, G)
    A, Bt, cm, cx, Gd = dev(xa6)[..., :3], dev(xb), dev(cmin), dev(cmax), dev(G)
    assert Na == 0 or A.stride(1) == 6
    within(host(ops.fourier(A, cm, cx, Gd)), refa, R.fourier_tol(maga), f"fourier half={half} set a ({Na})")
    within(host(ops.fourier(Bt, cm, cx, Gd)), refb, R.fourier_tol(magb), f"fourier half={half} set b ({Nb})")
    pair = host(ops.fourier_pair(A, Bt, cm, cx, Gd))
    assert pair.shape == (R.FOURIER_B * (Na + Nb), 2 * half)
    within(pair[:R.FOURIER_B * Na], refa.reshape(-1, 2 * half), R.fourier_tol(maga).reshape(-1, 2 * half), f"fourier_pair half={half} set a ({Na})")
    within(pair[R.FOURIER_B * Na:], refb.reshape(-1, 2 * half), R.fourier_tol(magb).reshape(-1, 2 * half), f"fourier_pair half={half} set b ({Nb})")


# ------------------------------------------------------------------------------------------------ spatial bias
@functools.lru_cache(maxsize=None)
def _sb_case(B, L_, H):
    """The case's pairwise locations (from the device kernel, as the model feeds them) and, per group of weights on demand, the
    float64 pre-activation; computed once per case and shared by the tests below (never modified)."""
    c, _, _ = R.sb_inputs(B, L_, H)
    pl_t = ops.pairwise_locs(dev(c))
    return {"pl_t": pl_t, "pl": host(pl_t), "groups": {}}


def _sb_group(B, L_, H, g=0):
    case = _sb_case(B, L_, H)
    if g not in case["groups"]:
        _, W, bw = R.sb_inputs(B, L_, H, group=g)
        v, mag = R.sb_pre(case["pl"], W, bw)
        assert float(R.sb_band(v).mean()) <= R.BAND_CAP, (B, L_, H, g)
        case["groups"][g] = (W, bw, v, mag)
    return case["groups"][g]


@pytest.mark.parametrize("B,L_,H", R.SB_CASES)
def test_spatial_bias_forward(B, L_, H):
    pl_t = _sb_case(B, L_, H)["pl_t"]
    W, bw, v, mag = _sb_group(B, L_, H)
    out = ops.spatial_bias(pl_t, dev(W), dev(bw))
    assert out.shape == (B, H, L_, L_)
    R.sb_assert_fwd(host(out), v, mag, what=f"B={B} L={L_} H={H} ops.spatial_bias")


@pytest.mark.parametrize("groups", [3, 32])
@pytest.mark.parametrize("B,L_,H", R.SB_CASES)
def test_spatial_bias_forward_grouped(B, L_, H, groups):
    pl_t = _sb_case(B, L_, H)["pl_t"]
    distinct = min(groups, R.sb_groups(B, L_, H))      # the grid-capped case repeats 3 weight sets over its 32 groups
    Ws = [dev(_sb_group(B, L_, H, g % distinct)[0]) for g in range(groups)]
    bws = [dev(_sb_group(B, L_, H, g % distinct)[1]) for g in range(groups)]
    outs = [torch.full((B, H, L_, L_), float("nan"), device=DEV) for _ in range(groups)]
    L.call("pq3d_spatial_bias_fwd_grouped", pl_t, L.parr(Ws), L.parr(bws), L.parr(outs), groups, B, H, L_)
    for g in range(groups):
        if g < distinct:
            _, _, v, mag = _sb_group(B, L_, H, g)
            R.sb_assert_fwd(host(outs[g]), v, mag, what=f"B={B} L={L_} H={H} group {g} of {groups}")
        else:
            assert torch.equal(outs[g], outs[g % distinct]), g      # same inputs, same kernel: the same bits


def _sb_dense(B, L_, H, g=0):
    W, bw, v, mag = _sb_group(B, L_, H, g)
    pl = _sb_case(B, L_, H)["pl"]
    db = R.sb_upstream(B, L_, H, v, seed=g)
    return W, bw, db, R.sb_bwd(pl, W, bw, db), R.sb_bwd_tol(pl, v, mag, db)


@pytest.mark.parametrize("B,L_,H", R.SB_CASES)
def test_spatial_bias_backward_dense(B, L_, H):
    """A dense random upstream gradient through autograd, through the overwriting entry (into garbage) and through the
    accumulating entry (into pre-filled dW / dbw, which it must add to)."""
    pl_t = _sb_case(B, L_, H)["pl_t"]
    W, bw, db, (dW, dbw), (tW, tb) = _sb_dense(B, L_, H)
    what = f"B={B} L={L_} H={H}"
    Wt, bt, dbt = dev(W).requires_grad_(True), dev(bw).requires_grad_(True), dev(db).view(B, H, L_, L_)
    ops.spatial_bias(pl_t, Wt, bt).backward(dbt)
    within(host(Wt.grad), dW, tW, f"spatial bias dW {what} autograd")
    within(host(bt.grad), dbw, tb, f"spatial bias dbw {what} autograd")
    gW, gb = torch.full((H, 5), float("nan"), device=DEV), torch.full((H,), 1e30, device=DEV)
    L.call("pq3d_spatial_bias_bwd", pl_t, Wt.detach(), bt.detach(), dbt, gW, gb, B, H, L_)
    within(host(gW), dW, tW, f"spatial bias dW {what} overwrite")
    within(host(gb), dbw, tb, f"spatial bias dbw {what} overwrite")
    # accumulate: the pre-filled value is one more term of the sum, touched by at most one atomic add per block
    r = np.random.default_rng([8, B, L_, H])
    pW, pb = (r.standard_normal((H, 5)) * 10).astype(np.float32), (r.standard_normal(H) * 10).astype(np.float32)
    aW, ab = dev(pW), dev(pb)
    L.call("pq3d_spatial_bias_bwd_acc", pl_t, Wt.detach(), bt.detach(), dbt, aW, ab, B, H, L_)
    nb = R.sb_blocks(B * L_ * L_) + 1
    within(host(aW), dW + pW, tW + nb * U * (np.abs(pW) + np.abs(dW)), f"spatial bias dW {what} accumulate")
    within(host(ab), dbw + pb, tb + nb * U * (np.abs(pb) + np.abs(dbw)), f"spatial bias dbw {what} accumulate")


@pytest.mark.parametrize("B,L_,H", R.SB_CASES)
def test_spatial_bias_backward_grouped(B, L_, H):
    """pq3d_spatial_bias_bwd_grouped (what the fused step calls), 3 groups of different weights and upstream gradients; it
    accumulates, here into zeros."""
    pl_t = _sb_case(B, L_, H)["pl_t"]
    cases = [_sb_dense(B, L_, H, g) for g in range(3)]
    Ws, bws, dbs = ([dev(c[k]) for c in cases] for k in range(3))
    dWs, dbws = [torch.zeros(H, 5, device=DEV) for _ in cases], [torch.zeros(H, device=DEV) for _ in cases]
    L.call("pq3d_spatial_bias_bwd_grouped", pl_t, L.parr(Ws), L.parr(bws), L.parr(dbs), L.parr(dWs), L.parr(dbws), 3, B, H, L_)
    for g, c in enumerate(cases):
        within(host(dWs[g]), c[3][0], c[4][0], f"spatial bias dW B={B} L={L_} H={H} group {g}")
        within(host(dbws[g]), c[3][1], c[4][1], f"spatial bias dbw B={B} L={L_} H={H} group {g}")


@pytest.mark.parametrize("B,L_,H", R.SB_CASES)
def test_spatial_bias_backward_one_hot(B, L_, H):
    """One non-zero upstream element at a time, at the first and the last element and on either side of every block / stride
    edge of the kernel's walk: dW[h] and dbw[h] are then that single term (8 u |term|) and every other head's sums exactly
    zero -- a dropped or mis-indexed element cannot hide in a sum."""
    case = _sb_case(B, L_, H)
    W, bw, v, mag = _sb_group(B, L_, H)
    LL = L_ * L_
    pos = R.sb_onehot_positions(v, mag)
    assert pos
    Wt, bt = dev(W), dev(bw)
    dbias = torch.zeros(B * H * LL, device=DEV)
    res = torch.full((len(pos), 6 * H), float("nan"), device=DEV)
    gval = 1.375
    for k, (e, h) in enumerate(pos):
        b, ij = divmod(e, LL)
        idx = (b * H + h) * LL + ij
        dbias[idx:idx + 1].fill_(gval)
        L.call("pq3d_spatial_bias_bwd", case["pl_t"], Wt, bt, dbias, res[k, :5 * H], res[k, 5 * H:], B, H, L_)
        dbias[idx:idx + 1].zero_()
    got = host(res)
    f = case["pl"].reshape(B, LL, 5).astype(np.float64)
    worst = 0.0
    for k, (e, h) in enumerate(pos):
        b, ij = divmod(e, LL)
        want = R.sb_onehot_terms(gval, v[b, h, ij], f[b, ij])
        dW, dbw = got[k, :5 * H].reshape(H, 5), got[k, 5 * H:]
        mine = np.append(dW[h], dbw[h]).astype(np.float64)
        err = np.abs(mine - want)
        assert (err <= 8 * U * np.abs(want)).all(), (e, h, mine, want)
        worst = max(worst, float((err[want != 0] / (8 * U * np.abs(want[want != 0]))).max()))
        others = np.arange(H) != h
        assert (dW[others] == 0).all() and (dbw[others] == 0).all(), (e, h)
    print(f"spatial bias one-hot B={B} L={L_} H={H}: {len(pos)} positions, worst {worst:.3f} of 8 u |term|")


# ------------------------------------------------------------------------------------------------ gate mix
@pytest.mark.parametrize("n", R.GATE_N)
def test_gate_mix(n):
    for k in (range(5) if n < 5 else (0,)):
        q, u, g, dy = R.gate_inputs(n, k)
        ref, tols = R.gate_mix(q, u, g, dy), R.gate_tols(q, u, dy)
        qt, ut, gt = (dev(a).requires_grad_(True) for a in (q, u, g))
        y = ops.gate_mix(qt, ut, gt)
        y.backward(dev(dy))
        got = [host(t) for t in (y, qt.grad, ut.grad, gt.grad)]
        for name, a, r, t in zip(("y", "dq", "du", "dg"), got, ref, tols):
            within(a, r, t, f"gate_mix n={n} {name}")
        hi, lo = g == 100, g == -100
        assert (got[0][hi] == u[hi]).all() and (got[0][lo] == q[lo]).all()


# ------------------------------------------------------------------------------------------------ fill_cols
@pytest.mark.parametrize("R_,C_,cols", [(5, 1, []), (5, 1, [0]), (5, 1, [0, 0]), (9, 21, []), (9, 21, [0, 20]),
                                        (9, 21, [3, 3, 7]), (9, 21, [0, 2, 20, 2])])
def test_fill_cols(R_, C_, cols):
    g = torch.Generator().manual_seed(R_ * C_ + len(cols))
    x, dy = torch.randn(R_, C_, generator=g), torch.randn(R_, C_, generator=g)
    ct = torch.tensor(cols, dtype=torch.int32, device=DEV)
    xt = x.to(DEV).requires_grad_(True)
    y = ops.fill_cols(xt, ct, float("-inf"))
    want = x.clone()
    want[:, cols] = float("-inf")
    same_bits(y, want, "fill_cols forward")
    y.backward(dy.to(DEV))
    wd = dy.clone()
    wd[:, cols] = 0.0
    same_bits(xt.grad, wd, "fill_cols backward")


# ------------------------------------------------------------------------------------------------ mask denominators
@pytest.mark.parametrize("M", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 257])
def test_mask_inv_den(M, n):
    g = torch.Generator().manual_seed(M * 1000 + n)
    for all_masked_at0 in (True, False):
        masks = torch.rand(M, n, generator=g) < 0.5
        masks[:, 0] = all_masked_at0
        if n > 1:
            masks[:, 1] = False
            masks[:, 2] = True
        out = host(ops.mask_inv_den([m.to(DEV) for m in masks]))
        den = (~masks).sum(0).double().numpy()
        dead = den == 0
        assert dead[0] == all_masked_at0
        big = np.float32(1) / np.float32(1e-8)
        assert (R.ulps32(out[dead], np.full(int(dead.sum()), big)) <= 1).all()
        want = 1.0 / (den[~dead] + 1e-8)
        within(out[~dead], want, 2 * U * want, f"mask_inv_den M={M} n={n}")


# ------------------------------------------------------------------------------------------------ activation backward
@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
@pytest.mark.parametrize("n", R.ACT_N)
def test_act_bwd(act, n):
    for k in (range(8) if n < 8 else (0,)):
        dy32, sv32 = (torch.from_numpy(a) for a in R.act_inputs(n, k))
        for dt_dy, dt_s, dt_o in itertools.product((F32, BF16), repeat=3):
            dy, sv = dy32.to(dt_dy), sv32.to(dt_s)
            out = ops.act_bwd(dy.to(DEV), sv.to(DEV), act, dt_o)
            assert out.dtype == dt_o and out.shape == dy.shape
            exact = R.act_bwd(dy, sv, act)                      # float64 of the values the kernel was given
            what = f"act_bwd {act} n={n} dy {dt_dy} saved {dt_s} out {dt_o}"
            if act != "gelu":                                   # a copy or a zero: no arithmetic
                same_bits(out, exact.float().to(dt_o), what)
            elif dt_o == F32:
                within(host(out), exact.numpy(), R.gelu_bwd_tol(dy).numpy(), what)
            else:                                               # one bf16 grid step around the rounded float64 value
                want = exact.to(BF16)
                d = (R.bf16_ordered(out.cpu()) - R.bf16_ordered(want)).abs()
                assert int(d.max()) <= 1, (what, int(d.max()))


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_inputs(R_, N, ld, dtype, groups, seed):
    """Small integers (|x| <= 8): every order of addition is exact in fp32, so the sums are known exactly.  The columns
    beyond N of a padded row hold 2^40: a kernel that read them would show it."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randint(-8, 9, (R_, ld), generator=g).float() for _ in range(groups)]
    for x in xs:
        x[:, N:] = 2.0 ** 40
    return [x.to(dtype).to(DEV) for x in xs], [x[:, :N].double().sum(0) for x in xs]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("R_", R.COLSUM_R)
def test_colsum_exact_on_integer_inputs(R_, dtype):
    for N, pad, acc in itertools.product(R.COLSUM_N, (0, 5), (0, 1, 2)):
        ld = N + pad
        xs, sums = _colsum_inputs(R_, N, ld, dtype, 3, R_ * 1000 + N)
        prior = torch.arange(N, dtype=F32) - 3.0
        outs = [prior.clone().to(DEV) if acc else torch.full((N,), float("nan"), device=DEV) for _ in xs]
        L.call("pq3d_colsum_grouped", L.parr(xs), L.parr(outs), 3, L.dt_of(xs[0]), R_, N, ld, acc)
        for o, s in zip(outs, sums):
            want = s + (prior.double() if acc else 0)
            assert torch.equal(o.cpu().double(), want), ("colsum_grouped", R_, N, ld, acc)
        one = torch.full((N,), float("nan"), device=DEV)
        L.call("pq3d_colsum", xs[1], L.dt_of(xs[1]), R_, N, ld, one)
        assert torch.equal(one.cpu().double(), sums[1]), ("colsum", R_, N, ld)
        if pad == 0 and acc == 0:
            assert torch.equal(ops.colsum(xs[2]).cpu().double(), sums[2]), ("ops.colsum", R_, N)


def test_colsum_random_values_against_float64():
    R_, N = 1000, 130
    x = torch.randn(R_, N, generator=torch.Generator().manual_seed(3))
    want = x.double().sum(0)
    within(host(ops.colsum(x.to(DEV))), want.numpy(), (R_ * U * x.double().abs().sum(0)).numpy(), "colsum random fp32")
    xb = x.bfloat16()
    within(host(ops.colsum(xb.to(DEV))), xb.double().sum(0).numpy(), (R_ * U * xb.double().abs().sum(0)).numpy(), "colsum random bf16")


# ------------------------------------------------------------------------------------------------ row scaling
@pytest.mark.parametrize("C_", R.SCALE_ROWS_C)
@pytest.mark.parametrize("in_dtype", [F32, BF16])
def test_scale_rows(C_, in_dtype):
    """C = 7 and bf16 input take the scalar path, fp32 with C % 8 == 0 the 8-wide one.  Dropped rows hold inf / NaN and come out
    exactly 0; kept rows are the fp32 product, bit for bit."""
    R_ = 37
    g = torch.Generator().manual_seed(C_)
    x = torch.randn(R_, C_, generator=g).to(in_dtype)
    scale = torch.randn(R_, generator=g)
    zero_flag = (torch.rand(R_, generator=g) < 0.3).to(torch.uint8)
    keep_mask = (torch.rand(R_, generator=g) < 0.7).to(torch.uint8)
    assert 0 < int(zero_flag.sum()) < R_ and 0 < int(keep_mask.sum()) < R_
    for use_s, use_z, use_k, out_dtype in itertools.product((False, True), (False, True), (False, True), (F32, BF16)):
        keep = torch.ones(R_, dtype=torch.bool)
        if use_z:
            keep &= zero_flag == 0
        if use_k:
            keep &= keep_mask != 0
        xin = x.clone()
        xin[~keep] = torch.tensor([float("inf"), float("nan")]).repeat(C_)[:C_].to(in_dtype)
        want = xin.float() * (scale[:, None] if use_s else 1.0)
        want[~keep] = 0.0
        out = ops.scale_rows(xin.to(DEV), R_, out_dtype, scale=scale.to(DEV) if use_s else None,
                             zero_flag=zero_flag.to(DEV) if use_z else None, keep_mask=keep_mask.to(DEV) if use_k else None)
        same_bits(out, want.to(out_dtype), f"scale_rows C={C_} in {in_dtype} out {out_dtype} scale={use_s} zero_flag={use_z} keep_mask={use_k}")


# ------------------------------------------------------------------------------------------------ casts
def _tie_inputs(n, seed):
    """fp32 values with exact bf16 ties up front (round to even decides: 1 + 2^-8 -> 1, 1 + 3 x 2^-8 -> 1 + 2^-6) and their
    negatives; b makes a + b hit the same ties from 1 + 2^-7 x k."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 5 * 2.0 ** -8, 2.0 ** -8 + 2.0 ** -16])
    a[:6] = ties
    b[:4] = 0.0
    a[6], b[6] = 1.0, 2.0 ** -8                    # the sum is a tie
    a[7], b[7] = 1 + 2.0 ** -7, 2.0 ** -8          # a tie that rounds up to even
    return a, b


@pytest.mark.parametrize("n", [8, 2056])
def test_add_cast_and_cast_bf16(n):
    groups = 3
    ab = [_tie_inputs(n, 10 * n + g) for g in range(groups)]
    a_t, b_t = [a.to(DEV) for a, _ in ab], [b.to(DEV) for _, b in ab]
    for with_b, out_dtype in itertools.product((False, True), (BF16, F32)):
        outs = [torch.zeros(n, dtype=out_dtype, device=DEV) for _ in ab]
        L.call("pq3d_add_cast", L.parr(a_t), L.parr(b_t) if with_b else None, L.parr(outs), groups, L.dt_of(outs[0]), n)
        for (a, b), o in zip(ab, outs):
            same_bits(o, ((a + b) if with_b else a).to(out_dtype), f"pq3d_add_cast n={n} b={with_b} out {out_dtype}")
    for (a, _), o in zip(ab, ops.cast_bf16(a_t)):
        same_bits(o, a.bfloat16(), f"cast_bf16 n={n}")
    assert float(torch.tensor(1 + 2.0 ** -8).bfloat16()) == 1.0 and float(torch.tensor(1 + 3 * 2.0 ** -8).bfloat16()) == 1 + 2.0 ** -6


@pytest.mark.parametrize("cols", [32, 64, 96])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("groups", [1, 2])
def test_cast_transpose(cols, T, groups):
    rows = T * cols
    g = torch.Generator().manual_seed(cols + T)
    srcs = [torch.randn(rows, cols, generator=g) for _ in range(groups)]
    for s in srcs:
        s[0, :4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)])
    st = [s.to(DEV) for s in srcs]
    outs = [torch.zeros(rows, cols, dtype=BF16, device=DEV) for _ in srcs]
    outTs = [torch.zeros(T, cols, cols, dtype=BF16, device=DEV) for _ in srcs]
    L.call("pq3d_cast_transpose", L.parr(st), L.parr(outs), L.parr(outTs), groups, rows, cols)
    for s, o, oT in zip(srcs, outs, outTs):
        same_bits(o, s.bfloat16(), "cast_transpose out")
        for t in range(T):
            same_bits(oT[t], s[t * cols:(t + 1) * cols].t().contiguous().bfloat16(), f"cast_transpose outT[{t}]")


# ------------------------------------------------------------------------------------------------ fixed-order sums
def _parts(count, shape, seed, integer=False, offset=None):
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    parts = []
    for i in range(count):
        flat = torch.randint(-8, 9, (n + 1,), generator=g).float() if integer else torch.randn(n + 1, generator=g) * 10.0 ** (i % 5 - 2)
        parts.append((flat, 1 if offset == i else 0))
    return [f[o:o + n].reshape(shape) for f, o in parts], [f.to(DEV)[o:o + n].view(shape) for f, o in parts]


@pytest.mark.parametrize("count", R.SUM_PARTS)
@pytest.mark.parametrize("shape", R.SUM_SHAPES)
def test_sum_n_is_the_left_to_right_fp32_sum(count, shape):
    """Parts of mixed magnitudes, so that the order of the additions shows in the bits; any element count (15 = 3 x 5 is no
    multiple of 4: the parent commit raised Pq3dError); one part a contiguous view from element 1 of its storage."""
    for offset in (None, min(1, count - 1)):
        cpu, gpu = _parts(count, shape, 100 * count + len(shape), offset=offset)
        if offset is not None:
            assert gpu[offset].data_ptr() % 16 == 4 and gpu[offset].is_contiguous()
        out = ops.sum_n(gpu)
        same_bits(out, torch.from_numpy(R.sum_left_to_right([p.numpy() for p in cpu])), f"sum_n {count} parts {shape} offset {offset}")
    cpu, gpu = _parts(count, shape, 7, integer=True)
    assert torch.equal(ops.sum_n(gpu).cpu().double(), sum(p.double() for p in cpu))


@pytest.mark.parametrize("shape_a,shape_b", [((15,), (1028,)), ((1028,), (3, 5)), ((15,), (3, 5)), ((4,), (1028,))])
def test_sum_pair_equals_two_sum_n(shape_a, shape_b):
    _, a = _parts(3, shape_a, 21)
    _, b = _parts(32, shape_b, 22)
    oa, ob = ops.sum_pair(a, b)
    same_bits(oa, ops.sum_n(a), f"sum_pair a {shape_a}")
    same_bits(ob, ops.sum_n(b), f"sum_pair b {shape_b}")
    cpu_a, _ = _parts(3, shape_a, 21)
    same_bits(oa, torch.from_numpy(R.sum_left_to_right([p.numpy() for p in cpu_a])), "sum_pair a against the CPU")


# ------------------------------------------------------------------------------------------------ means
def _mean_ws(device):
    (ws,) = [w for k, w in ops._MEAN_WS.items() if isinstance(k, torch.device) and k == device]
    return ws


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("n", R.MEAN_ALL_N)
def test_mean_all(n, view):
    """Integer inputs (the sum is exact in any order): the result is float32(S) / float32(n).  Two calls in a row on different
    data: the arrival counter in the workspace is zero again after the first.  view: x[1:] of a 1-D tensor, which starts inside
    a 16-byte piece (the parent commit raised Pq3dError)."""
    g = torch.Generator().manual_seed(n)
    for call in range(2):
        base = torch.randint(-8, 9, (n + 1,), generator=g).float()
        x = base.to(DEV)[1:] if view else base[1:].to(DEV)
        assert x.is_contiguous() and x.data_ptr() % 16 == (4 if view else 0)
        x.requires_grad_(True)
        m = ops.mean_all(x)
        want = np.float32(float(base[1:].double().sum())) / np.float32(n)
        assert float(m.detach()) == float(want), (n, call, float(m.detach()), float(want))
        assert int(_mean_ws(x.device)[:1].view(torch.int32)) == 0, "arrival counter not reset"
        (m * 3.0).backward()
        fill = np.float32(3.0) * np.float32(1.0 / n)              # pq3d_fill_scaled: g x float32(1 / n)
        assert R.ulps32(fill, np.float32(3.0 / n)) <= 1
        assert x.grad.shape == x.shape and bool((x.grad == float(fill)).all()), (n, call)


def test_mean_many_edges():
    """Elements exactly at clamp_min (the gradient passes, as torch.clamp's does), a view that starts inside a 16-byte piece
    (scalar path), 33 tensors (two launches), tensors of 1, 3 and 5 elements."""
    g = torch.Generator().manual_seed(9)
    cm = -50.0
    xs = [torch.randn(c, generator=g) * 40 for c in (1, 3, 5, 1023, 4096)] + [torch.randn(7, 3, generator=g) * 40 for _ in range(28)]
    modes = ["clamp_min", "plain", "finite", "clamp_min", "clamp_min"] + ["clamp_min", "plain", "finite", "plain"] * 7
    assert len(xs) == 33 and len(modes) == 33
    xs[0][0] = cm
    xs[3][:9] = torch.tensor([cm, cm - 1e-3, cm + 1e-3, cm, -51.0, -49.0, cm, 0.0, cm])
    xs[7][0, :2] = float("-inf")
    xs[2][1] = float("nan")
    wide = torch.randn(4098, generator=g) * 40
    wide[1:5] = torch.tensor([cm, -60.0, cm, 7.0])
    xs[4] = wide[1:4097]
    gpu = [x.to(DEV).requires_grad_(True) for x in xs]
    gpu[4] = wide.to(DEV)[1:4097].requires_grad_(True)
    assert gpu[4].data_ptr() % 16 == 4 and gpu[4].is_contiguous()
    f = {"plain": lambda t: t, "clamp_min": lambda t: t.clamp(min=cm), "finite": lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))}
    ref = [x.double().requires_grad_(True) for x in xs]
    means = [f[m](t).mean() for m, t in zip(modes, ref)]
    total = sum(means)
    out = ops.mean_many(gpu, modes, clamp_min=cm)
    # any-order fp32 sum of n terms, the division, then the sum over the tensors
    tol = sum((t.numel() + 1) * U * float(f[m](t.detach()).abs().mean()) for m, t in zip(modes, ref)) + 33 * U * sum(abs(float(v.detach())) for v in means)
    within(float(out.detach()), float(total.detach()), tol, "mean_many forward")
    (out * 3.0).backward()
    (total * 3.0).backward()
    for i, (a, r, m) in enumerate(zip(gpu, ref, modes)):
        want = np.where(r.grad.numpy() != 0, np.float32(3.0) / np.float32(r.numel()), np.float32(0)).astype(np.float32)
        same_bits(a.grad, torch.from_numpy(want), f"mean_many gradient of tensor {i} ({m})")
    assert float(gpu[0].grad[0]) != 0 and float(gpu[3].grad[0]) != 0 and float(gpu[3].grad[1]) == 0 and float(gpu[4].grad[0]) != 0


# ------------------------------------------------------------------------------------------------ mask_not
@pytest.mark.parametrize("count", [1, 33])
def test_mask_not(count):
    g = torch.Generator().manual_seed(count)
    masks = [torch.rand(n, generator=g) < 0.5 for n in ([1, 257] * 17)[:count]]
    if count > 1:
        masks += [torch.rand(3, 5, generator=g) < 0.5, torch.rand(3, 5, generator=g) < 0.5]
    outs = ops.mask_not([m.to(DEV) for m in masks])
    assert len(outs) == len(masks)
    off = 0
    for m, o in zip(masks, outs):
        assert o.dtype == torch.bool and o.shape == m.shape and torch.equal(o.cpu(), ~m)
        assert o.untyped_storage().data_ptr() == outs[0].untyped_storage().data_ptr() and o.storage_offset() == off
        off += m.numel()


# ------------------------------------------------------------------------------------------------ refused arguments
def test_arguments_outside_an_entrys_domain_are_refused_before_any_launch():
    z = torch.zeros(17 * 5 + 64 * 48, device=DEV)
    zb = torch.zeros(64 * 48, dtype=BF16, device=DEV)
    with pytest.raises(L.Pq3dError, match="cols % 32"):
        L.call("pq3d_cast_transpose", L.parr([z]), L.parr([zb]), L.parr([zb]), 1, 48, 48)
    with pytest.raises(L.Pq3dError, match="multiple of 8"):
        L.call("pq3d_add_cast", L.parr([z]), None, L.parr([zb]), 1, L.BF16, 12)
    pl = torch.zeros(1, 2, 2, 5, device=DEV)
    with pytest.raises(L.Pq3dError, match="at most 16 heads"):
        L.call("pq3d_spatial_bias_bwd_grouped", pl, L.parr([z]), L.parr([z]), L.parr([z]), L.parr([z]), L.parr([z]), 1, 1, 17, 2)
    with pytest.raises(L.Pq3dError, match="bad args"):
        L.call("pq3d_colsum", z, L.F32, 4, 8, 7, z)          # ld < N
