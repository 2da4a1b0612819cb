"""GPU: batch-statistics BatchNorm over the rows of a level (pq3d_amd/sparse.py: bn_stats / bn_apply / bn_bwd_reduce /
bn_bwd_apply on csrc/sparse_conv_bwd.hip) against float64 ``F.batch_norm(training=True)`` + autograd of
y = relu(bn(z) + residual): the forward output, dz, dweight, dbias, the residual branch's gradient and the updated running
buffers.  Inputs and outputs are column views of wider buffers (the concatenation buffers of the network).

The bar of every tensor is 8 x the relative L2 error of the SAME computation run in float32 on the host (8: the project's factor
for "our fp32 against a float32 host run"); the residual branch's gradient is dy under the ReLU mask and is compared for
equality.  Measured on an MI355X, worst ratio error / (float32 host error) over the cases (N, C, with / without
ReLU + residual):
    y 1.42   dz 1.30   dweight 1.68   dbias 2.00   running_mean 1.04   running_var 1.06
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
T = 64
EPS, MOM = 1e-5, 0.1


def _host(z, res, w, b, rm, rv, up, relu, dtype):
    """(y, dz, dw, db, dres, running_mean, running_var) of y = [relu](batch_norm(z) + res) in ``dtype`` on the host"""
    z, w, b = (t.to(dtype).clone().requires_grad_(True) for t in (z, w, b))
    res = res.to(dtype).clone().requires_grad_(True) if res is not None else None
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = F.batch_norm(z, rm, rv, w, b, True, MOM, EPS)
    if res is not None:
        y = y + res
    if relu:
        y = y.clamp_min(0)
    gs = torch.autograd.grad(y, [z, w, b] + ([res] if res is not None else []), up.to(dtype))
    return [y.detach(), gs[0], gs[1], gs[2], gs[3] if res is not None else None, rm, rv]


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _ours(sp, z, res, w, b, rm, rv, up, relu):
    """the same through the kernels, every row tensor a column view of a wider buffer"""
    N, C = z.shape
    wide = lambda t, off, pad: torch.cat([torch.full((N, off), float("nan")), t, torch.full((N, pad), float("nan"))], 1).cuda()[:, off:off + C]
    zg, upg = wide(z, 8, 4), wide(up, 4, 12)
    resg = wide(res, 16, 0) if res is not None else None
    rm, rv, nbt = rm.clone().cuda(), rv.clone().cuda(), torch.tensor(7).cuda()
    mean, rstd = sp.bn_stats(zg, EPS, MOM, rm, rv, nbt)
    buf = torch.full((N, C + 40), 7.25, device="cuda")
    y = sp.bn_apply(zg, mean, rstd, w.cuda(), b.cuda(), residual=resg, act="relu" if relu else None, out=buf, col_off=24)
    assert bool((buf[:, :24] == 7.25).all()) and bool((buf[:, 24 + C:] == 7.25).all()) and y.data_ptr() == buf[:, 24:].data_ptr()
    dw, db = sp.bn_bwd_reduce(upg, zg, mean, rstd, y=y if relu else None)
    dresbuf = torch.full((N, C + 8), 1.5, device="cuda")
    dres = dresbuf[:, 8:]
    dz = sp.bn_bwd_apply(upg, zg, mean, rstd, w.cuda(), dw, db, y=y if relu else None, dres=dres if res is not None else None)
    assert bool((dresbuf[:, :8] == 1.5).all())
    if res is not None:      # the accumulating form adds the same g onto what the buffer holds
        acc = torch.full((N, C), 2.0, device="cuda")
        sp.bn_bwd_apply(upg, zg, mean, rstd, w.cuda(), dw, db, y=y if relu else None, dres=acc, dres_add=True)
        assert torch.equal(acc, dres + 2.0)
    assert int(nbt) == 8
    return [y, dz, dw, db, dres if res is not None else None, rm, rv], (mean, rstd)


NAMES = ("y", "dz", "dweight", "dbias", "dres", "running_mean", "running_var")


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("N", [2, T + 1, 600])
def test_batchnorm_forward_backward_against_float64(N, C):
    from pq3d_amd import sparse as sp
    g = torch.Generator().manual_seed(N * 100 + C)
    z = torch.randn(N, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g)
    res, up = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    rm, rv = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    for relu, r in ((True, res), (False, None)):
        want = _host(z, r, w, b, rm, rv, up, relu, torch.float64)
        host = _host(z, r, w, b, rm, rv, up, relu, torch.float32)
        got, _ = _ours(sp, z, r, w, b, rm, rv, up, relu)
        for name, a, h, ref in zip(NAMES, got, host, want):
            if ref is None:
                continue
            assert bool(torch.isfinite(a).all())
            if name == "dres":      # dy under the ReLU mask: no arithmetic, so the same numbers
                assert torch.equal(a.cpu().double(), ref), f"dres (N={N}, C={C})"
                continue
            e, e32 = _rel(a.cpu(), ref), _rel(h, ref)
            print(f"N={N} C={C} relu={relu} {name}: {e:.3e} ({e / max(e32, 1e-300):.2f} x host float32 {e32:.3e})")
            assert e <= 8 * e32, f"{name} (N={N}, C={C}, relu={relu}): {e:.3e} > 8 x {e32:.3e}"
    # two calls: the same bits, and the counter advances by one per call
    a1, _ = _ours(sp, z, res, w, b, rm, rv, up, True)
    a2, _ = _ours(sp, z, res, w, b, rm, rv, up, True)
    assert all(torch.equal(p, q) for p, q in zip(a1, a2))


def test_one_row_gives_beta_and_no_nan():
    """N = 1: variance 0, xhat = 0, the output is beta (+ residual); torch refuses this shape in training mode, so the
    statement is checked directly.  The unbiased factor N / (N - 1) is taken as 1 here: the running variance stays finite."""
    from pq3d_amd import sparse as sp
    C = 32
    g = torch.Generator().manual_seed(0)
    z, w, b = torch.randn(1, C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda(), torch.randn(C, generator=g).cuda()
    rm, rv, nbt = torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.tensor(0).cuda()
    mean, rstd = sp.bn_stats(z, EPS, MOM, rm, rv, nbt)
    y = sp.bn_apply(z, mean, rstd, w, b)
    assert torch.equal(y, b[None, :]) and torch.equal(mean, z[0]) and bool(torch.isfinite(rstd).all())
    assert torch.allclose(rv.cpu(), torch.full((C,), 1 - MOM), rtol=1e-6, atol=0) and bool(torch.isfinite(rm).all()) and int(nbt) == 1
    up = torch.randn(1, C, generator=g).cuda()
    dw, db = sp.bn_bwd_reduce(up, z, mean, rstd)
    dz = sp.bn_bwd_apply(up, z, mean, rstd, w, dw, db)
    assert torch.equal(db, up[0]) and bool((dw == 0).all()) and bool((dz == 0).all())


def test_unbiased_factor_at_two_rows_is_exactly_two():
    from pq3d_amd import sparse as sp
    C = 96
    lo = torch.arange(C, dtype=torch.float32)
    z = torch.stack([lo, lo + 2.0]).cuda()              # per channel: mean lo + 1, biased variance 1, unbiased 2 -- all exact
    rv = torch.full((C,), 123.0).cuda()
    mean, rstd = sp.bn_stats(z, 0.0, 1.0, None, rv, None)        # momentum 1: the buffer becomes the new value itself
    assert torch.equal(mean.cpu(), lo + 1.0) and torch.equal(rstd, torch.ones(C).cuda())     # biased variance exactly 1
    assert torch.equal(rv, torch.full((C,), 2.0).cuda())


def test_large_mean_does_not_cancel_the_variance():
    """A channel whose mean is 1000 x its standard deviation: a two-pass fp32 variance sits near N 2^-24 ~ 4e-5 of relative error
    at N = 600, the E[x^2] - mean^2 form near 6e-2.  The bar 1e-3 separates them with room on both sides."""
    from pq3d_amd import sparse as sp
    N, C = 600, 32
    g = torch.Generator().manual_seed(5)
    z = torch.randn(N, C, generator=g)
    z[:, 3] += 1000.0
    z[:, 17] = z[:, 17] * 0.01 - 10.0
    mean, rstd = sp.bn_stats(z.cuda(), EPS)
    var = 1.0 / rstd.cpu().double() ** 2 - EPS
    want = z.double().var(0, unbiased=False)
    rel = ((var - want).abs() / want)
    print(f"relative error of the batch variance: large-mean channels {float(rel[3]):.2e} {float(rel[17]):.2e}, worst {float(rel.max()):.2e}")
    assert float(rel.max()) <= 1e-3
    assert float(((mean.cpu().double() - z.double().mean(0)).abs() / z.double().std(0)).max()) <= 1e-3
