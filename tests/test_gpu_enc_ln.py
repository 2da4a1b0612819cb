"""GPU: the encoders' one-launch Linear+LayerNorm forward (csrc/enc_ln.hip) and the bf16 hand-over of dlin in their backward,
bit for bit against the two-launch / fp32 path they replace (ops._ENC_LN / ops._ENC_DLIN_BF16 switched off)."""
import pytest
import torch

from pq3d_amd import _lib as L
from pq3d_amd import ops
from pq3d_amd._lib import BF16, BF16X3, F32
from tests.enc_common import DEV, N, _bits_equal, _count_calls, _order_bound, _params, rnd

pytestmark = pytest.mark.gpu


class _Tape:
    """Stand-in for the autograd context of _LinearLNGroup.forward: keeps what the op saves (mean, rstd, then lin of every group first)."""

    def save_for_backward(self, *ts):
        self.saved = ts


def _inputs(G, R, K):
    xs = []
    for g in range(G):
        x = rnd(R, K, seed=40 + g)
        flat = x.view(-1)
        flat[::7] = 0.0          # exact zeros and negative zeros among the operands
        flat[3::11] = -0.0
        flat[0], flat[-1] = 0.0, -0.0
        xs.append(x.to(DEV))
    return xs


def _forward(xs, Ws, bs, gs, be, ct=BF16X3):
    tape = _Tape()
    ys = ops._LinearLNGroup.forward(tape, ct, 1e-5, len(xs), False, *xs, *Ws, *bs, *gs, *be)
    G, R = len(xs), xs[0].shape[0]
    mean, rstd = tape.saved[:2]   # flat, group after group; then one lin [R, N] per group
    return ys, torch.stack(tape.saved[2:2 + G]), mean.view(G, R), rstd.view(G, R)


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("R", [1, 31, 32, 33, 97, 2049])
def test_one_launch_forward_keeps_the_bits(R, G, K, monkeypatch):
    """y, lin, mean, rstd of pq3d_linear_ln_fwd against pq3d_gemm (BF16X3) + pq3d_add_ln_fwd: the tile edges, one row past the
    gemm_wk / gemm_fast dispatch boundary (2049), one and three groups.  At most 65 x 3 = 195 tiles: below the CU count, so every
    workgroup has ONE tile here; the persistent loop is test_one_launch_forward_many_tiles_per_workgroup's."""
    _check_forward_bits(R, G, K, monkeypatch)


def _tile_ranges(R, G):
    """Tile ranges [t0, t1) of the launch's workgroups, as csrc/enc_ln.hip deals them: one workgroup per CU (at most one per tile)
    over the G x ceil(R / 32) tiles laid end to end.  Returns (tiles per group, ranges)."""
    T = (R + 31) // 32
    total = T * G
    grid = min(total, torch.cuda.get_device_properties(0).multi_processor_count)
    return T, [(total * b // grid, total * (b + 1) // grid) for b in range(grid)]


def _rows_for_loop(G):
    """Smallest R = 32 j + 1 (a partial last tile) from 2 tiles per CU on at which every workgroup has at least 2 tiles and, for
    G > 1, every group boundary lies strictly inside some workgroup's range: that workgroup reloads W, bias, gamma and beta in
    mid-loop.  (Ranges are floor(total b / grid): with few tiles per workgroup the boundaries tend to fall on range ends.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for j in range(2 * cus // G, 2 * cus // G + 512):
        R = 32 * j + 1
        T, rng = _tile_ranges(R, G)
        if min(t1 - t0 for t0, t1 in rng) >= 2 and all(any(t0 < g * T < t1 for t0, t1 in rng) for g in range(1, G)):
            return R
    raise AssertionError("no row count puts the group boundaries inside workgroups' tile ranges")


@pytest.mark.parametrize("G,K", [(1, 256), (3, 256), (3, 64)])
def test_one_launch_forward_many_tiles_per_workgroup(G, K, monkeypatch):
    """The persistent loop past its first tile: the prefetch of the next tile's rows during the current tile's products, the reuse
    of the x planes and the output tile in LDS behind the two barriers, and (G = 3) the reload of W / bias / gamma / beta where a
    workgroup's range crosses into the next group.  On 256 CUs: G = 1 has 16385 rows (513 tiles, 2-3 per workgroup); G = 3 has
    8161 rows (3 x 256 tiles, 3 per workgroup; workgroups 85 and 170 cross a group).  K = 64: a row tile has fewer chunks than
    the workgroup has threads."""
    R = _rows_for_loop(G)
    T, rng = _tile_ranges(R, G)
    cross = [i for i, (a, b) in enumerate(rng) if any(a < g * T < b for g in range(1, G))]
    print(f"R={R}: {T} tiles per group, {len(rng)} workgroups of {min(b - a for a, b in rng)}-{max(b - a for a, b in rng)} tiles, "
          f"crossing a group: {cross}")
    assert min(b - a for a, b in rng) >= 2 and (G == 1 or len(cross) >= G - 1)
    _check_forward_bits(R, G, K, monkeypatch)


def _check_forward_bits(R, G, K, monkeypatch):
    xs = _inputs(G, R, K)
    par = _params(G, K)
    seen = _count_calls(monkeypatch)
    monkeypatch.setattr(ops, "_ENC_LN", True)
    new = _forward(xs, *par)
    assert seen == ["pq3d_linear_ln_fwd"]
    del seen[:]
    monkeypatch.setattr(ops, "_ENC_LN", False)
    old = _forward(xs, *par)
    assert seen == ["pq3d_gemm", "pq3d_add_ln_fwd"]
    for g in range(G):
        assert _bits_equal(new[0][g], old[0][g]), f"y[{g}]"
    for name, a, b in zip(("lin", "mean", "rstd"), new[1:], old[1:]):
        assert _bits_equal(a, b), name
    assert torch.isfinite(new[1]).all() and torch.isfinite(new[0][0]).all()


def _two_launches(xs, Ws, bs, gs, be, ct):
    """The grouped GEMM and the independent-branch LayerNorm launch, issued here directly (not through ops.linear_ln_group)."""
    G, (R, K), n = len(xs), xs[0].shape, Ws[0].shape[0]
    lin = torch.empty(G, R, n, device=DEV)
    ys = torch.empty(G, R, n, device=DEV)
    mean = torch.empty(G, R, device=DEV)
    rstd = torch.empty(G, R, device=DEV)
    L.gemm(M=R, N=n, K=K, A=[x.contiguous() for x in xs], B=list(Ws), bias=list(bs), Cs=[lin[g] for g in range(G)], ct=ct, lda=K,
           ldb=K, ldc=n)
    d = ops._ln_desc(None, [lin[g] for g in range(G)], gs, be, None, 1e-5, R, None, mean, rstd)
    d.independent, d.dt_y = 1, F32
    for g in range(G):
        d.ys[g] = L.ptr(ys[g])
    L.call("pq3d_add_ln_fwd", d)
    return ys


def test_fallback_keeps_two_launches(monkeypatch):
    """N = 768 and a non-contiguous x stay on the two launches: the results of those two launches issued directly, and the new
    entry point is not entered."""
    monkeypatch.setattr(ops, "_ENC_LN", True)
    seen = _count_calls(monkeypatch)
    R, K = 40, 256
    cases = [(_inputs(2, R, K), _params(2, K, 768)),
             ([rnd(R, 2 * K, seed=5).to(DEV)[:, :K], rnd(R, 2 * K, seed=6).to(DEV)[:, K:]], _params(2, K))]
    assert not cases[1][0][0].is_contiguous()
    for xs, (Ws, bs, gs, be) in cases:
        del seen[:]
        ys = ops.linear_ln_group(xs, Ws, bs, gs, be, ct=BF16X3)
        assert "pq3d_linear_ln_fwd" not in seen and seen.count("pq3d_add_ln_fwd") == 1
        ref = _two_launches(xs, Ws, bs, gs, be, BF16X3)
        for g in range(2):
            assert _bits_equal(ys[g], ref[g])
    # other compute types keep the two launches as well
    xs, (Ws, bs, gs, be) = _inputs(1, R, K), _params(1, K)
    for ct in (F32, BF16):
        del seen[:]
        ops.linear_ln_group(xs, Ws, bs, gs, be, ct=ct)
        assert "pq3d_linear_ln_fwd" not in seen


def _ln_bwd(lin, mean, rstd, gs, be, dys, dtype):
    """One pq3d_add_ln_bwd launch as _LinearLNGroup.backward issues it; returns (dlin, dgamma, dbeta)."""
    G, R = lin.shape[0], lin.shape[1]
    dlin = torch.empty(lin.shape, dtype=dtype, device=DEV)
    dg = torch.zeros(G, N, device=DEV)
    db = torch.zeros(G, N, device=DEV)
    d = ops._ln_desc(None, [lin[g] for g in range(G)], gs, be, None, 1e-5, R, None, mean, rstd)
    d.independent, d.accumulate, d.dt_d_o = 1, 1, L.dt_of(dlin)
    for g in range(G):
        d.dys[g], d.d_o[g], d.dgamma[g], d.dbeta[g] = L.ptr(dys[g]), L.ptr(dlin[g]), L.ptr(dg[g]), L.ptr(db[g])
    L.call("pq3d_add_ln_bwd", d)
    return dlin, dg, db


@pytest.mark.parametrize("R", [1, 33, 300])
def test_ln_backward_stores_dlin_in_bf16(R):
    """d_o requested in bf16 is the fp32 d_o rounded to nearest even, bit for bit; dgamma / dbeta do not depend on it: equal bits
    where one workgroup forms them (R = 1), else within the reordering bound of their per-workgroup atomics."""
    G = 2
    _, _, gs, be = _params(G, 64)
    lin = torch.stack([rnd(R, N, seed=3 + g) for g in range(G)]).to(DEV)
    dys = [rnd(R, N, seed=9 + g).to(DEV) for g in range(G)]
    mean = lin.mean(-1)
    rstd = 1.0 / torch.sqrt(lin.var(-1, unbiased=False) + 1e-5)
    d32, dg32, db32 = _ln_bwd(lin, mean, rstd, gs, be, dys, torch.float32)
    d16, dg16, db16 = _ln_bwd(lin, mean, rstd, gs, be, dys, torch.bfloat16)
    assert d16.dtype == torch.bfloat16
    assert torch.equal(d16.view(torch.int16), d32.to(torch.bfloat16).view(torch.int16))
    if R == 1:
        assert _bits_equal(dg16, dg32) and _bits_equal(db16, db32)
    else:
        dy = torch.stack(dys).double()
        xh = (lin.double() - mean.double()[..., None]) * rstd.double()[..., None]
        for a, b, c in ((dg16, dg32, (dy * xh).abs().sum(1)), (db16, db32, dy.abs().sum(1))):
            assert bool(((a.double() - b.double()).abs() <= _order_bound(c, R)).all())


def _grads(xs, par, gy, monkeypatch, bf16):
    monkeypatch.setattr(ops, "_ENC_DLIN_BF16", bf16)
    leaves = [[t.clone().requires_grad_(True) for t in ts] for ts in (*par, xs)]
    ys = ops.linear_ln_group(leaves[4], *leaves[:4], ct=BF16X3)
    torch.autograd.backward(list(ys), gy)
    return [[t.grad for t in ts] for ts in leaves]   # dW, db, dgamma, dbeta, dx


def _maxdiff(a, b):
    return max(float((s.double() - t.double()).abs().max()) for s, t in zip(a, b))


@pytest.mark.parametrize("R", [97, 2049])
def test_backward_handover_keeps_the_gradients(R, monkeypatch):
    """All four parameter gradients of _LinearLNGroup with dlin handed over in bf16 against the fp32 hand-over.  The operand values
    the weight-gradient MFMAs see are the same, so dW / db differ by the order of their fp32 atomics only: equal bits at R = 97
    (one reduction chunk, one writer per element: the fp32 path is checked to repeat itself first), within twice the fp32 path's
    own call-to-call difference at R = 2049 (split-K).  dgamma / dbeta: within the reordering bound of the LayerNorm backward's
    per-workgroup atomics.  dx = dlin W (x requires a gradient here) has one writer per element and no split-K; every kernel
    pq3d_gemm sends it to (gemm_wk at R = 97, the 64 x 64 / 128 x 128 tile kernels at R = 2049) rounds an fp32 A to bf16 as it
    stages it and sums k ascending into one accumulator, so a bf16 A gives the same bits at both sizes."""
    G, K = 3, 256
    xs = _inputs(G, R, K)
    par = _params(G, K)
    gy = [rnd(R, N, seed=90 + g).to(DEV) for g in range(G)]
    p1 = _grads(xs, par, gy, monkeypatch, False)
    p2 = _grads(xs, par, gy, monkeypatch, False)
    new = _grads(xs, par, gy, monkeypatch, True)
    for k, name in ((0, "dW"), (1, "db")):
        own = _maxdiff(p1[k], p2[k])
        d1, d2 = _maxdiff(new[k], p1[k]), _maxdiff(new[k], p2[k])
        print(f"R={R} {name}: fp32 path call-to-call {own:.3e}, bf16 hand-over vs the two fp32 runs {d1:.3e} {d2:.3e}")
        if R == 97:
            assert own == 0.0, f"{name}: the fp32 path does not repeat itself at R = {R}"
            assert all(_bits_equal(a, b) for a, b in zip(new[k], p1[k])), name
        else:
            assert d1 <= 2.0 * own and d2 <= 2.0 * own, name
    for g in range(G):
        assert new[4][g].dtype == torch.float32 and _bits_equal(p1[4][g], p2[4][g]), f"dx[{g}]: the fp32 path does not repeat itself"
        assert _bits_equal(new[4][g], p1[4][g]), f"dx[{g}]"
    # LayerNorm parameter gradients: the forward tape in float64 gives the size of the addends
    monkeypatch.setattr(ops, "_ENC_LN", False)
    _, lin, mean, rstd = _forward(xs, *par)
    dy = torch.stack(gy).double()
    xh = (lin.double() - mean.double()[..., None]) * rstd.double()[..., None]
    for k, c in ((2, (dy * xh).abs().sum(1)), (3, dy.abs().sum(1))):
        for g in range(G):
            assert bool(((new[k][g].double() - p1[k][g].double()).abs() <= _order_bound(c[g], R)).all())
