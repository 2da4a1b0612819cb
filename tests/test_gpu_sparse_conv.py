"""GPU: the sparse 3-D convolution kernel (csrc/sparse_conv.hip: pq3d_sparse_conv_fwd, pq3d_sparse_nbr) and the coordinate
pyramid (pq3d_amd/sparse.py) against the float64 dense restatement tests/sparse_ref.py.  EVERY output element is checked
against a bound derived for it: tol = c * A with A = |scale| * sum |x| |W| + |shift| + |bias| + |residual| (the restatement's
``absolute`` form), u = 2^-24, n = Cin * (offsets present for that row), and
    ct = F32  : c = (n + 8) u                       (exact products, fp32 accumulation of n terms, a few epilogue roundings)
    ct = BF16 : c = 2^-8 * 1.01 + (n + 8) u         (both operands rounded to bf16, 2^-9 relative each; fp32 accumulation)
Coordinates: two scenes with overlapping xyz (a shared 10 x 10 plane), negative and odd coordinates, a solid 4 x 4 x 4 block,
an isolated voxel and the thin plane; output row counts 1, T - 1, T, T + 1 and 4 T + 1 around the kernel's row tile T."""
import pytest
import torch

from tests import sparse_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F32, BF16 = 0, 1


def _coords(p=10):
    g = torch.Generator().manual_seed(11)
    r4, r10 = torch.arange(-5, -1), torch.arange(-3, -3 + p)
    block = torch.cartesian_prod(r4, r4, r4)                                                   # all 27 neighbours inside
    plane = torch.cat([torch.cartesian_prod(r10, r10), torch.full((p * p, 1), 3)], 1)          # thin plane z = 3
    lone = torch.tensor([[5, 5, -3]])                                                          # centre offset only (k = 3 and 5)
    rnd = torch.unique(torch.stack([torch.randint(-5, 7, (60,), generator=g), torch.randint(-5, 7, (60,), generator=g),
                                    torch.randint(-5, 1, (60,), generator=g)], 1), dim=0)[:40]
    s0, s1 = torch.cat([block, plane, lone]), torch.cat([plane, rnd])
    c = torch.cat([torch.cat([torch.zeros(len(s0), 1, dtype=torch.long), s0], 1),
                   torch.cat([torch.ones(len(s1), 1, dtype=torch.long), s1], 1)])
    return c[torch.randperm(len(c), generator=g)].int()


def _match(a, b):
    """for every row of a (integer [n, 4]) its row in b"""
    rows = {tuple(r): i for i, r in enumerate(b.tolist())}
    return torch.tensor([rows[tuple(r)] for r in a.tolist()])


def _setup(p):
    from pq3d_amd import sparse
    coords = _coords(p)
    pyr = sparse.CoordPyramid(coords.cuda())
    return dict(sparse=sparse, coords=coords, pyr=pyr, perm=pyr.perm.cpu(), T=sparse.ROW_TILE, N=len(coords))


@pytest.fixture(scope="module")
def S():
    return _setup(10)


@pytest.fixture(scope="module")
def S2():
    """the same shapes with a 24 x 24 plane: the stride-2 case then has more than 4 T + 1 OUTPUT (coarse) rows"""
    return _setup(24)


def test_coordinate_sets_cover_the_named_shapes(S):
    c, T = S["coords"].long(), S["T"]
    assert len(c) >= 4 * T + 1 and int(c[:, 1:].min()) < 0
    tab = R.table(c, 1, c, R.offsets(3))
    present = (tab >= 0).sum(1)
    assert int((present == 27).sum()) >= 8 and int((present == 1).sum()) >= 1        # block interior; the isolated voxel
    a, b = c[c[:, 0] == 0][:, 1:], c[c[:, 0] == 1][:, 1:]
    assert len({tuple(r) for r in a.tolist()} & {tuple(r) for r in b.tolist()}) >= 100   # the scenes overlap in xyz


def test_maps_match_the_restatement(S):
    """Level coordinates as sets, every kernel map after undoing the internal permutation, parents against ops.parents_from_coords."""
    from pq3d_amd import ops
    pyr, c = S["pyr"], S["coords"]
    ours = [pyr.level_coords(l).cpu().long() for l in range(5)]
    ref = [R.level_coords(c, 1 << l) for l in range(5)]
    to_ref, to_int = [], []
    for l in range(5):
        assert sorted(map(tuple, ours[l].tolist())) == list(map(tuple, ref[l].tolist())), f"level {l} coordinate set"
        assert pyr.n[l] == len(ref[l])
        m = _match(ours[l], ref[l])                       # internal row -> restatement row
        to_ref.append(m)
        to_int.append(torch.cat([torch.empty(len(m), dtype=torch.long).scatter_(0, m, torch.arange(len(m))), torch.tensor([-1])]))
    def same(kmap, tab_ref, l_out, l_in):
        want = to_int[l_in][tab_ref[to_ref[l_out]]]       # restatement rows -> internal rows (-1 stays -1)
        assert torch.equal(kmap.nbr.cpu().long(), want)
        T = S["T"]
        occ = kmap.occ.cpu().view(-1, 4)
        for t in range(occ.shape[0]):
            bits = (want[t * T:(t + 1) * T] >= 0).any(0)
            for k in range(want.shape[1]):
                assert bool((int(occ[t, k >> 5]) >> (k & 31)) & 1) == bool(bits[k]), "occupancy word"
    for l in range(5):
        same(pyr.nbr3[l], R.table(ref[l], 1 << l, ref[l], R.offsets(3)), l, l)
    same(pyr.nbr5, R.table(ref[0], 1, ref[0], R.offsets(5)), 0, 0)
    for l in range(4):
        same(pyr.down[l], R.table(ref[l], 1 << l, ref[l + 1], R.offsets(2)), l + 1, l)
        same(pyr.up[l], R.up_table(ref[l + 1], ref[l], 1 << l), l, l + 1)
    for h in range(5):
        l = 4 - h
        want = ops.parents_from_coords(c.cuda(), pyr.level_coords(l) if l else c.cuda(), 1 << l)
        assert torch.equal(pyr.parents[h], want), f"parents of output level {h}"
    assert torch.equal(pyr.level_coords(0)[pyr.inv].cpu(), c)


CASES = [(3, 32, 125, "same"), (32, 32, 27, "same"), (64, 128, 27, "same"), (384, 256, 27, "same"), (128, 96, 27, "same"),
         (96, 96, 27, "same"), (32, 32, 8, "down"), (256, 256, 8, "up")]
EPILOGUES = ["none", "bn_relu", "bn_res_relu", "bias"]


def _reference(S, Cin, Cout, K, kind):
    """x (internal order, fp32), W, and in float64: the accumulation, its |x| |W| form and the present-offset count per output row."""
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + K)
    pyr, c, perm = S["pyr"], S["coords"], S["perm"]
    W = torch.randn(K, Cin, Cout, generator=g) * (K * Cin) ** -0.5
    one, oneW = torch.ones(S["N"], 1, dtype=torch.float64), torch.ones(K, 1, 1, dtype=torch.float64)
    if kind == "same":
        k = round(K ** (1 / 3))
        kmap = pyr.nbr5 if K == 125 else pyr.nbr3[0]
        x = torch.randn(S["N"], Cin, generator=g)
        f = lambda a, w, ab=False: R.conv(c, a, w, k, 1, ab)[perm]
        x_int = x[perm]
    elif kind == "down":
        kmap = pyr.down[0]
        x = torch.randn(S["N"], Cin, generator=g)
        cc = R.level_coords(c, 2)
        idx = _match(pyr.level_coords(1).cpu().long(), cc)
        f = lambda a, w, ab=False: R.conv_down(c, a, w, 1, ab)[1][idx]
        x_int = x[perm]
    else:
        kmap = pyr.up[0]
        cc = R.level_coords(c, 2)
        idx = _match(pyr.level_coords(1).cpu().long(), cc)
        x_int = torch.randn(len(cc), Cin, generator=g)
        x = torch.empty_like(x_int)
        x[idx] = x_int                                       # the same features in the restatement's coarse row order
        one = torch.ones(len(cc), 1, dtype=torch.float64)
        f = lambda a, w, ab=False: R.conv_up(cc, a, w, c, 1, ab)[perm]
    return dict(kmap=kmap, x=x_int.contiguous(), W=W, acc=f(x.double(), W.double()), A=f(x.double(), W.double(), True),
                present=f(one, oneW)[:, 0].round(), g=g)


@pytest.mark.parametrize("Cin,Cout,K,kind", CASES)
def test_sparse_conv_every_element(S, S2, Cin, Cout, K, kind):
    S = S2 if kind == "down" else S
    sp, T = S["sparse"], S["T"]
    ref = _reference(S, Cin, Cout, K, kind)
    full, g = ref["kmap"], ref["g"]
    Nf = full.n_out
    assert Nf >= 4 * T + 1
    scale = torch.randn(Cout, generator=g)
    shift, bias, res = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g), torch.randn(Nf, Cout, generator=g)
    res_gpu = res.cuda()
    if (Cin, Cout) == (64, 128):        # the block's 1 x 1 downsample (K = 1: a row GEMM on pq3d_gemm) is the residual
        Wd = torch.randn(Cin, Cout, generator=g) * Cin ** -0.5
        res_gpu = sp.row_gemm(ref["x"].cuda(), Wd.t().contiguous().cuda(), None, F32)
        want, bound = ref["x"].double() @ Wd.double(), ref["x"].double().abs() @ Wd.double().abs()
        assert bool(((res_gpu.cpu().double() - want).abs() <= (Cin + 8) * U * bound).all()), "1x1 downsample (row GEMM)"
        res = res_gpu.cpu()
    x, W = ref["x"].cuda(), ref["W"].cuda()
    Wb = W.bfloat16()
    n = Cin * ref["present"]
    worst = {}
    sizes = sorted({1, T - 1, T, T + 1, 4 * T + 1, Nf})
    for rows in sizes:
        kmap = full if rows == Nf else sp.KernelMap(full.nbr[:rows].contiguous(), full.n_in)
        for ep in EPILOGUES:
            kw, acc, A = {}, ref["acc"][:rows], ref["A"][:rows]
            if ep in ("bn_relu", "bn_res_relu"):
                kw.update(scale=scale.cuda(), shift=shift.cuda(), act="relu")
                acc, A = acc * scale.double() + shift.double(), A * scale.double().abs() + shift.double().abs()
            if ep == "bn_res_relu":
                kw.update(residual=res_gpu[:rows])
                acc, A = acc + res[:rows].double(), A + res[:rows].double().abs()
            if ep == "bias":
                kw.update(bias=bias.cuda())
                acc, A = acc + bias.double(), A + bias.double().abs()
            if "act" in kw:
                acc = acc.clamp_min(0)
            for ct in (F32, BF16):
                if kind == "up":        # written at a column offset into a wider buffer: the other columns stay untouched
                    buf = torch.full((rows, Cout + 40), 7.25, device="cuda")
                    sp.sparse_conv(x, kmap, Wb if ct == BF16 else W, ct=ct, out=buf, col_off=24, **kw)
                    assert bool((buf[:, :24] == 7.25).all()) and bool((buf[:, 24 + Cout:] == 7.25).all())
                    y = buf[:, 24:24 + Cout]
                else:
                    y = sp.sparse_conv(x, kmap, Wb if ct == BF16 else W, ct=ct, **kw)
                c = (n[:rows, None] + 8) * U + (2.0 ** -8 * 1.01 if ct == BF16 else 0.0)
                err = (y.cpu().double() - acc).abs()
                tol = c * A
                ratio = float((err / tol.clamp_min(1e-300)).max())
                worst[(ep, ct)] = max(worst.get((ep, ct), 0.0), ratio)
                bad = err > tol
                assert not bool(bad.any()), f"rows={rows} {ep} ct={ct}: {int(bad.sum())} elements over their bound, worst ratio {ratio:.3g}"
                if ep == "none":
                    assert bool((y.cpu()[ref["present"][:rows] == 0] == 0).all())
                if rows == Nf and ep == "bn_res_relu":
                    y2 = sp.sparse_conv(x, kmap, W, ct=ct, **kw)       # fp32 weights converted in the kernel: the same bits, twice
                    y3 = sp.sparse_conv(x, kmap, W, ct=ct, **kw)
                    assert torch.equal(y2, y3)
                    if kind != "up":
                        assert torch.equal(y, y2)
    print(f"\nsparse_conv Cin={Cin} Cout={Cout} K={K} {kind}: worst err/tol " + ", ".join(f"{e}/ct{c}={v:.3f}" for (e, c), v in worst.items()))


@pytest.mark.parametrize("Cin,Cout,K,kind", CASES)
def test_every_channel_tiling_meets_the_bound_with_the_same_bits(S, S2, Cin, Cout, K, kind):
    """The kernel is instantiated for 32, 64, 96 and 128 output channels per workgroup and the library picks by size (the wide
    tiles only from tens of thousands of rows on).  Each instantiation is forced here (descriptor field ``ntl``), checked
    element by element against the same bound (full epilogue), and must give the bits of the library's own choice."""
    S = S2 if kind == "down" else S
    sp = S["sparse"]
    ref = _reference(S, Cin, Cout, K, kind)
    kmap, g = ref["kmap"], ref["g"]
    scale, shift, res = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g), torch.randn(kmap.n_out, Cout, generator=g)
    acc = (ref["acc"] * scale.double() + shift.double() + res.double()).clamp_min(0)
    A = ref["A"] * scale.double().abs() + shift.double().abs() + res.double().abs()
    x, W = ref["x"].cuda(), ref["W"].cuda()
    kw = dict(scale=scale.cuda(), shift=shift.cuda(), residual=res.cuda(), act="relu")
    n = Cin * ref["present"]
    for ct in (F32, BF16):
        auto = sp.sparse_conv(x, kmap, W, ct=ct, **kw)
        tol = ((n[:, None] + 8) * U + (2.0 ** -8 * 1.01 if ct == BF16 else 0.0)) * A
        for ntl in (2, 4, 6, 8):
            y = sp.sparse_conv(x, kmap, W, ct=ct, ntl=ntl, **kw)
            bad = (y.cpu().double() - acc).abs() > tol
            assert not bool(bad.any()), f"ntl={ntl} ct={ct}: {int(bad.sum())} elements over their bound"
            assert torch.equal(y, auto), f"ntl={ntl} ct={ct}: bits differ from the library's own tiling"
    from pq3d_amd import _lib
    with pytest.raises(_lib.Pq3dError, match="ntl"):
        sp.sparse_conv(x, kmap, W, ntl=3)


def test_absent_rows_are_exactly_zero(S):
    """Rows with no present offset (and whole tiles of them: an all-zero occupancy word) give exact zeros; the rest is unchanged."""
    sp, T, pyr = S["sparse"], S["T"], S["pyr"]
    nbr = pyr.nbr3[0].nbr.clone()
    nbr[5] = -1
    nbr[T:2 * T] = -1
    nbr[-1] = -1
    kmap = sp.KernelMap(nbr, pyr.n[0])
    assert int(kmap.occ.cpu()[1].abs().sum()) == 0
    g = torch.Generator().manual_seed(2)
    x, W = torch.randn(pyr.n[0], 32, generator=g).cuda(), (torch.randn(27, 32, 32, generator=g) / 30).cuda()
    for ct in (F32, BF16):
        y, y0 = sp.sparse_conv(x, kmap, W, ct=ct), sp.sparse_conv(x, pyr.nbr3[0], W, ct=ct)
        gone = torch.zeros(pyr.n[0], dtype=torch.bool, device="cuda")
        gone[5] = gone[-1] = True
        gone[T:2 * T] = True
        assert bool((y[gone] == 0).all()) and torch.equal(y[~gone], y0[~gone])
        assert torch.equal(y, sp.sparse_conv(x, kmap, W, ct=ct, use_occ=False))


def test_bad_arguments_are_refused(S):
    from pq3d_amd import _lib
    sp, pyr = S["sparse"], S["pyr"]
    x, W = torch.zeros(pyr.n[0], 32, device="cuda"), torch.zeros(27, 32, 32, device="cuda")
    with pytest.raises(_lib.Pq3dError, match="leading dimensions"):
        d_out = torch.zeros(pyr.n[0], 32, device="cuda")
        d = _lib.SparseConvDesc()
        d.N_out, d.N_in, d.Cin, d.Cout, d.K, d.ldx, d.ldo, d.col_off = pyr.n[0], pyr.n[0], 32, 32, 27, 32, 32, 8
        d.x, d.nbr, d.W, d.out = x.data_ptr(), pyr.nbr3[0].nbr.data_ptr(), W.data_ptr(), d_out.data_ptr()
        _lib.call("pq3d_sparse_conv_fwd", d)
    with pytest.raises(_lib.Pq3dError):
        sp.sparse_conv(x.cpu(), pyr.nbr3[0], W)
