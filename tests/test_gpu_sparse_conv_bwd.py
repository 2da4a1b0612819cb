"""GPU: the sparse convolution's backward operators (pq3d_amd/sparse.py: sparse_conv_bwd_input = pq3d_sparse_conv_fwd on the
transposed map with the weight read transposed; sparse_conv_bwd_weight = pq3d_sparse_conv_wgrad) against float64 autograd
through tests/sparse_ref.py::conv_table under a fixed random upstream gradient (tests/sparse_train_ref.py::conv_grads).  The
kernel maps that serve as ``conv_table``'s tables are the pyramid's own, which tests/test_gpu_sparse_conv.py pins to the
restatement.  EVERY element is held to the forward test's bound, u = 2^-24:
    input gradient   |err| <= ((n + 8) u [+ 1.01 * 2^-8 in bf16]) * A,  A = sum |dY| |W| (+ |residual|), n = Cout * (pairs that
                     use the input row)
    weight gradient  |err| <= ((n_k + 8) u [+ 1.01 * 2^-8]) * sum |x| |dY|,  n_k = present pairs of offset k (any summation
                     order of n_k terms is within (n_k - 1) u: the row split and its chunk-order sum do not change the bound)
Coordinates: those of tests/test_gpu_sparse_conv.py (two overlapping scenes, a solid block, a thin plane, an isolated voxel,
negative and odd coordinates, more than 4 T + 1 rows; the 24 x 24 plane for the stride-2 convolution)."""
import pytest
import torch

from tests import sparse_train_ref as TR
from tests.test_gpu_sparse_conv import _setup

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F32, BF16 = 0, 1
CASES_DX = [(32, 32, 27, "same"), (64, 128, 27, "same"), (384, 256, 27, "same"), (128, 96, 27, "same"), (32, 32, 8, "down"),
            (256, 256, 8, "up")]
CASES_DW = CASES_DX + [(3, 32, 125, "same")]


@pytest.fixture(scope="module")
def S():
    return _setup(10)


@pytest.fixture(scope="module")
def S2():
    return _setup(24)


_REF = {}


def _case(S, S2, Cin, Cout, K, kind):
    """The forward map, its transpose, fp32 operands and (once per case, shared by the tests) the float64 gradients."""
    key = (Cin, Cout, K, kind)
    if key in _REF:
        return _REF[key]
    S = S2 if kind == "down" else S
    pyr = S["pyr"]
    if kind == "same":
        kmap = pyr.nbr5 if K == 125 else pyr.nbr3[0]
        kmap_t = kmap
    elif kind == "down":
        kmap, kmap_t = pyr.down[0], pyr.up[0]
    else:
        kmap, kmap_t = pyr.up[0], pyr.down[0]
    g = torch.Generator().manual_seed(7 + Cin * 1000 + Cout + K)
    x, dy = torch.randn(kmap.n_in, Cin, generator=g), torch.randn(kmap.n_out, Cout, generator=g)
    W = torch.randn(K, Cin, Cout, generator=g) * (K * Cin) ** -0.5
    tab = kmap.nbr.cpu().long()
    dX, dW, A_x, A_w = TR.conv_grads(x, tab, W, dy)
    n_in, n_k = TR.pair_counts(tab, kmap.n_in)
    _REF[key] = dict(sp=S["sparse"], T=S["T"], kmap=kmap, kmap_t=kmap_t, x=x, dy=dy, W=W, tab=tab, dX=dX, dW=dW, A_x=A_x, A_w=A_w,
                     n_in=n_in, n_k=n_k, g=g)
    return _REF[key]


def _tol(n, A, ct):
    return ((n + 8) * U + (2.0 ** -8 * 1.01 if ct == BF16 else 0.0)) * A


@pytest.mark.parametrize("Cin,Cout,K,kind", CASES_DX)
def test_input_gradient_every_element(S, S2, Cin, Cout, K, kind):
    c = _case(S, S2, Cin, Cout, K, kind)
    sp, kt = c["sp"], c["kmap_t"]
    assert kt.n_out == c["kmap"].n_in >= 4 * c["T"] + 1 or kind == "up"
    rev = kind == "same"
    dy, W = c["dy"].cuda(), c["W"].cuda()
    res = torch.randn(kt.n_out, Cin, generator=c["g"])
    n = (Cout * c["n_in"]).double()[:, None]
    unused = c["n_in"] == 0
    worst = {}
    for ct in (F32, BF16):
        # plain, accumulate epilogue, and accumulate at a column offset of a wider buffer with dY a column view of another
        plain = sp.sparse_conv_bwd_input(dy, kt, W, rev, ct=ct)
        acc = sp.sparse_conv_bwd_input(dy, kt, W, rev, ct=ct, residual=res.cuda())
        wide_dy = torch.full((dy.shape[0], Cout + 24), float("nan"), device="cuda")
        wide_dy[:, 16:16 + Cout] = dy
        buf = torch.full((kt.n_out, Cin + 40), 7.25, device="cuda")
        sp.sparse_conv_bwd_input(wide_dy[:, 16:16 + Cout], kt, W, rev, ct=ct, residual=res.cuda(), out=buf, col_off=24)
        assert bool((buf[:, :24] == 7.25).all()) and bool((buf[:, 24 + Cin:] == 7.25).all())
        assert torch.equal(buf[:, 24:24 + Cin], acc)
        for name, got, want, A in (("plain", plain, c["dX"], c["A_x"]), ("acc", acc, c["dX"] + res.double(), c["A_x"] + res.double().abs())):
            err, tol = (got.cpu().double() - want).abs(), _tol(n, A, ct)
            worst[(name, ct)] = float((err / tol.clamp_min(1e-300)).max())
            bad = err > tol
            assert not bool(bad.any()), f"{name} ct={ct}: {int(bad.sum())} elements over their bound, worst ratio {worst[(name, ct)]:.3g}"
        assert bool((plain.cpu()[unused] == 0).all())
        for ntl in (2, 4, 6, 8):
            assert torch.equal(sp.sparse_conv_bwd_input(dy, kt, W, rev, ct=ct, residual=res.cuda(), ntl=ntl), acc), f"ntl={ntl}: bits differ"
        assert torch.equal(sp.sparse_conv_bwd_input(dy, kt, W.bfloat16(), rev, ct=BF16), sp.sparse_conv_bwd_input(dy, kt, W, rev, ct=BF16))
    print(f"\nsparse_conv dX Cin={Cin} Cout={Cout} K={K} {kind}: worst err/tol " + ", ".join(f"{e}/ct{t}={v:.3f}" for (e, t), v in worst.items()))


def test_unused_input_rows_get_exact_zeros(S, S2):
    """An input row no output row uses (its row of the transposed map is empty) gets exact zeros; the other rows are unchanged."""
    c = _case(S, S2, 32, 32, 27, "same")
    sp, kt, T = c["sp"], c["kmap_t"], c["T"]
    nbr = kt.nbr.clone()
    gone = torch.zeros(kt.n_out, dtype=torch.bool, device="cuda")
    gone[3] = gone[-1] = True
    gone[T:2 * T] = True
    nbr[gone] = -1
    cut = sp.KernelMap(nbr, kt.n_in)
    dy, W = c["dy"].cuda(), c["W"].cuda()
    for ct in (F32, BF16):
        a, b = sp.sparse_conv_bwd_input(dy, cut, W, True, ct=ct), sp.sparse_conv_bwd_input(dy, kt, W, True, ct=ct)
        assert bool((a[gone] == 0).all()) and torch.equal(a[~gone], b[~gone])
    from pq3d_amd import _lib
    with pytest.raises(_lib.Pq3dError, match="wmode"):      # no packed (Cin < 16) form of the input gradient
        sp.sparse_conv_bwd_input(torch.zeros(kt.n_in, 3, device="cuda"), kt, torch.zeros(27, 32, 3, device="cuda"), True)


@pytest.mark.parametrize("Cin,Cout,K,kind", CASES_DW)
def test_weight_gradient_every_element(S, S2, Cin, Cout, K, kind):
    c = _case(S, S2, Cin, Cout, K, kind)
    sp, full, T = c["sp"], c["kmap"], c["T"]
    Nf = full.n_out
    assert Nf >= 4 * T + 1
    x, dy = c["x"].cuda(), c["dy"].cuda()
    wide_x = torch.full((x.shape[0], Cin + 24), float("nan"), device="cuda")      # x as a column view of a concatenation buffer
    wide_x[:, 8:8 + Cin] = x
    wide_dy = torch.full((dy.shape[0], Cout + 8), float("nan"), device="cuda")
    wide_dy[:, 4:4 + Cout] = dy
    worst = {}
    for rows in sorted({1, T - 1, T, T + 1, 4 * T + 1, Nf}):
        if rows == Nf:
            kmap, dW, A, n_k = full, c["dW"], c["A_w"], c["n_k"]
        else:
            kmap = sp.KernelMap(full.nbr[:rows].contiguous(), full.n_in)
            _dX, dW, _Ax, A = TR.conv_grads(c["x"], c["tab"][:rows], c["W"], c["dy"][:rows])
            n_k = TR.pair_counts(c["tab"][:rows], full.n_in)[1]
        tiles = (rows + T - 1) // T
        for ct in (F32, BF16):
            tol = _tol(n_k.double()[:, None, None], A, ct)
            for splits in (0, 1, 2, 3, tiles + 3):        # the library's choice; forced; more chunks than row tiles
                got = sp.sparse_conv_bwd_weight(x, kmap, dy[:rows], ct=ct, splits=splits)
                err = (got.cpu().double() - dW).abs()
                worst[ct] = max(worst.get(ct, 0.0), float((err / tol.clamp_min(1e-300)).max()))
                bad = err > tol
                assert not bool(bad.any()), f"rows={rows} ct={ct} splits={splits}: {int(bad.sum())} elements over their bound"
                assert bool((got.cpu()[n_k == 0] == 0).all()), "an offset without a present pair must give an exact-zero slab"
                assert torch.equal(got, sp.sparse_conv_bwd_weight(x, kmap, dy[:rows], ct=ct, splits=splits)), "same split, other bits"
            strided = sp.sparse_conv_bwd_weight(wide_x[:, 8:8 + Cin], kmap, wide_dy[:rows, 4:4 + Cout], ct=ct, splits=2)
            assert torch.equal(strided, sp.sparse_conv_bwd_weight(x, kmap, dy[:rows], ct=ct, splits=2))
    print(f"\nsparse_conv dW Cin={Cin} Cout={Cout} K={K} {kind}: worst err/tol " + ", ".join(f"ct{t}={v:.3f}" for t, v in worst.items()))


def test_weight_gradient_workspace_and_arguments(S, S2):
    from pq3d_amd import _lib
    c = _case(S, S2, 32, 32, 27, "same")
    sp, kmap = c["sp"], c["kmap"]
    x, dy = c["x"].cuda(), c["dy"].cuda()
    need = _lib.lib().pq3d_sparse_conv_wgrad_ws_bytes(kmap.n_out, 32, 32, 27, 3)
    assert need == 3 * 27 * 32 * 32 * 4 and _lib.lib().pq3d_sparse_conv_wgrad_ws_bytes(kmap.n_out, 32, 32, 27, 1) == 0
    assert _lib.lib().pq3d_sparse_conv_wgrad_ws_bytes(kmap.n_out, 32, 32, 27, 5000) == -1
    auto = sp.wgrad_splits(kmap.n_out, 32, 32, 27)
    assert 1 <= auto <= (kmap.n_out + c["T"] - 1) // c["T"] and sp.wgrad_splits(kmap.n_out, 32, 32, 27, 7) == 7
    out = torch.full((27, 32, 32), 3.5, device="cuda")
    small = torch.empty(need // 4 - 1, device="cuda")
    with pytest.raises(_lib.Pq3dError, match="workspace too small"):
        sp.sparse_conv_bwd_weight(x, kmap, dy, splits=3, out=out, ws=small)
    torch.cuda.synchronize()
    assert bool((out == 3.5).all()), "a refused call must launch nothing"
    ok = sp.sparse_conv_bwd_weight(x, kmap, dy, splits=3, out=out, ws=torch.empty(need // 4, device="cuda"))
    assert ok is out and torch.equal(out, sp.sparse_conv_bwd_weight(x, kmap, dy, splits=3))
    with pytest.raises(_lib.Pq3dError, match="splits"):
        sp.sparse_conv_bwd_weight(x, kmap, dy, splits=5000)
    with pytest.raises(_lib.Pq3dError):
        sp.sparse_conv_bwd_weight(x.cpu(), kmap, dy)
