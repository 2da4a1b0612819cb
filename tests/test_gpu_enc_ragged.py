"""GPU: grouped Linear+LayerNorm encoders whose groups differ in row count -- pq3d_linear_ln_fwd's tile list over unequal groups
(csrc/enc_ln.hip), the per-branch rows of the independent-branch LayerNorm backward (csrc/norm.hip), the op on its per-group tape
(ops._LinearLNGroup) and the model's one call for the position pair and the scene memories (PQ3D_ENC_MERGE).  Everything is
compared with the per-group launches of the same kernels: bit for bit where a value has one writer, within the reordering bound
of its fp32 addends where atomics form it."""
import pytest
import torch

from pq3d_amd import _lib as L
from pq3d_amd import ops
from pq3d_amd._lib import BF16X3
from pq3d_amd.modules import set_compute
from tests import util
from tests.enc_common import DEV, N, _bits_equal, _count_calls, _order_bound, _params, rnd

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _inputs(rows, K):
    xs = []
    for g, R in enumerate(rows):
        x = rnd(R, K, seed=40 + g)
        flat = x.view(-1)
        flat[::7] = 0.0          # exact zeros and negative zeros among the operands
        flat[3::11] = -0.0
        xs.append(x.to(DEV))
    return xs


# ------------------------------------------------------------------------------------------------ forward launch
def _fwd_launch(xs, par, rows, R=0):
    """One pq3d_linear_ln_fwd launch issued directly.  rows: the descriptor's per-group counts (None: all zero, R rows per group).
    Returns per-group (lin, mean, rstd, y); mean / rstd packed group after group in one buffer, as the header says."""
    Ws, bs, gs, be = par
    G, K = len(xs), xs[0].shape[1]
    cnt = list(rows) if rows is not None else [R] * G
    lin = [torch.empty(r, N, device=DEV) for r in cnt]
    y = [torch.empty(r, N, device=DEV) for r in cnt]
    mean = torch.empty(sum(cnt), device=DEV)
    rstd = torch.empty(sum(cnt), device=DEV)
    d = L.LinearLnDesc()
    d.R, d.K, d.N, d.groups, d.eps = R, K, N, G, EPS
    d.mean, d.rstd = L.ptr(mean), L.ptr(rstd)
    for g in range(G):
        d.x[g], d.W[g], d.bias[g], d.gamma[g], d.beta[g] = L.ptr(xs[g]), L.ptr(Ws[g]), L.ptr(bs[g]), L.ptr(gs[g]), L.ptr(be[g])
        d.lin[g], d.y[g] = L.ptr(lin[g]), L.ptr(y[g])
        if rows is not None:
            d.rows[g] = rows[g]
    L.call("pq3d_linear_ln_fwd", d)
    off = [sum(cnt[:g]) for g in range(G)]
    return [(lin[g], mean[off[g]:off[g] + cnt[g]], rstd[off[g]:off[g] + cnt[g]], y[g]) for g in range(G)]


def _check_ragged_forward(rows, K):
    xs = _inputs(rows, K)
    par = _params(len(rows), K)
    new = _fwd_launch(xs, par, rows)
    for g, R in enumerate(rows):
        one = _fwd_launch([xs[g]], [p[g:g + 1] for p in par], None, R)[0]
        for name, a, b in zip(("lin", "mean", "rstd", "y"), new[g], one):
            assert _bits_equal(a, b), f"{name}[{g}] of rows {rows}"
        assert all(bool(torch.isfinite(t).all()) for t in new[g])


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("rows", [(1, 33), (32, 31, 97), (64, 1, 32, 65), (2049, 5)], ids=lambda r: "+".join(map(str, r)))
def test_ragged_forward_keeps_the_bits(rows, K):
    """lin, mean, rstd and y of one launch over groups of different row counts against one single-group launch of the same kernel
    per group: one-row groups, groups that end on and next to a tile edge, a group of many tiles in front of a short one."""
    _check_ragged_forward(rows, K)


@pytest.mark.parametrize("K", [64, 256])
def test_zero_rows_mean_uniform(K):
    """All-zero rows with R set (every caller from before per-group rows) against the same counts written out."""
    xs = _inputs((97, 97, 97), K)
    par = _params(3, K)
    old = _fwd_launch(xs, par, None, 97)
    new = _fwd_launch(xs, par, (97, 97, 97))
    for g in range(3):
        for name, a, b in zip(("lin", "mean", "rstd", "y"), new[g], old[g]):
            assert _bits_equal(a, b), f"{name}[{g}]"


def _tile_ranges(rows):
    """Tile ranges [t0, t1) of the launch's workgroups as csrc/enc_ln.hip deals them: one workgroup per CU (at most one per tile)
    over the groups' ceil(rows / 32) tiles laid end to end.  Returns (first tile of every group after the first, ranges)."""
    tiles = [(r + 31) // 32 for r in rows]
    total = sum(tiles)
    grid = min(total, torch.cuda.get_device_properties(0).multi_processor_count)
    return [sum(tiles[:g]) for g in range(1, len(rows))], [(total * b // grid, total * (b + 1) // grid) for b in range(grid)]


def _rows_for_loop():
    """Chosen as tests/test_gpu_enc_ln.py::_rows_for_loop chooses: the smallest R = 32 j + 1 from 2 tiles per CU on at which the
    groups (R, R - 800, 33) give every workgroup at least 2 tiles and put both group boundaries strictly inside a workgroup's
    range -- that workgroup reloads W, bias, gamma and beta in mid-loop and switches to another row count."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for j in range(max(cus, 27), cus + 512):
        R = 32 * j + 1
        rows = (R, R - 800, 33)
        bnd, rng = _tile_ranges(rows)
        if min(t1 - t0 for t0, t1 in rng) >= 2 and all(any(t0 < b < t1 for t0, t1 in rng) for b in bnd):
            return rows
    raise AssertionError("no row count puts the group boundaries inside workgroups' tile ranges")


@pytest.mark.parametrize("K", [64, 256])
def test_ragged_forward_many_tiles_per_workgroup(K):
    """The persistent loop across unequal groups: every workgroup has at least 2 tiles, and each group boundary lies strictly
    inside some workgroup's range (asserted on the ranges before any bits are compared)."""
    rows = _rows_for_loop()
    bnd, rng = _tile_ranges(rows)
    cross = [i for i, (a, b) in enumerate(rng) if any(a < t < b for t in bnd)]
    print(f"rows={rows}: boundaries at tiles {bnd}, {len(rng)} workgroups of {min(b - a for a, b in rng)}-{max(b - a for a, b in rng)} "
          f"tiles, crossing a group: {cross}")
    assert min(b - a for a, b in rng) >= 2
    assert all(any(a < t < b for a, b in rng) for t in bnd) and len(set(rows)) == len(rows)
    _check_ragged_forward(rows, K)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
SENT = 12345.0
TAIL = 5   # sentinel rows behind every group


def _ln_bwd(lin, mean, rstd, gs, be, dys, dtype, rows):
    """One pq3d_add_ln_bwd launch over len(lin) independent branches.  rows None: the uniform form (R rows each).  d_o buffers carry
    TAIL sentinel rows.  Returns ([dlin with tail], dgamma, dbeta)."""
    G = len(lin)
    dlin = [torch.full((t.shape[0] + TAIL, N), SENT, dtype=dtype, device=DEV) for t in lin]
    dg = torch.zeros(G, N, device=DEV)
    db = torch.zeros(G, N, device=DEV)
    d = ops._ln_desc(None, list(lin), gs, be, None, EPS, 1, None, mean, rstd)
    d.independent, d.accumulate, d.dt_d_o = 1, 1, L.dt_of(dlin[0])
    for g in range(G):
        d.dys[g], d.d_o[g], d.dgamma[g], d.dbeta[g] = L.ptr(dys[g]), L.ptr(dlin[g]), L.ptr(dg[g]), L.ptr(db[g])
        if rows is not None:
            d.rows[g] = rows[g]
    L.call("pq3d_add_ln_bwd", d)
    return dlin, dg, db


def _ln_case(rows):
    """Tape of a forward over `rows` (lin, packed mean / rstd) and upstream gradients.  The buffers the kernel reads are followed
    by NaN rows: a read past a group's count would show in dlin, dgamma or dbeta."""
    G = len(rows)
    _, _, gs, be = _params(G, 64)
    nan = float("nan")

    def padded(t):   # the group's rows as a view of a buffer with a NaN tail
        buf = torch.full((t.shape[0] + TAIL, *t.shape[1:]), nan, device=DEV)
        buf[:t.shape[0]] = t.to(DEV)
        return buf[:t.shape[0]]
    lin = [padded(rnd(R, N, seed=3 + g)) for g, R in enumerate(rows)]
    dys = [padded(rnd(R, N, seed=9 + g)) for g, R in enumerate(rows)]
    tot = sum(rows)
    mean = torch.full((tot + TAIL,), nan, device=DEV)
    rstd = torch.full((tot + TAIL,), nan, device=DEV)
    mean[:tot] = torch.cat([t.mean(-1) for t in lin])
    rstd[:tot] = torch.cat([1.0 / torch.sqrt(t.var(-1, unbiased=False) + EPS) for t in lin])
    return lin, dys, mean, rstd, gs, be


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [(1, 33), (300, 97, 32)], ids=lambda r: "+".join(map(str, r)))
def test_ln_backward_per_group_rows(rows, dtype):
    """One launch with per-branch rows against one single-branch launch per group: dlin bit for bit, dgamma / dbeta within the
    reordering bound of their addends (sizes from the tape in float64), nothing read or written past a group's rows."""
    lin, dys, mean, rstd, gs, be = _ln_case(rows)
    tot = sum(rows)
    m0, r0 = mean.clone(), rstd.clone()
    dl, dg, db = _ln_bwd(lin, mean, rstd, gs, be, dys, dtype, rows)
    assert _bits_equal(mean[tot:], m0[tot:]) and _bits_equal(rstd[tot:], r0[tot:])   # (inputs: NaN tails untouched)
    off = 0
    for g, R in enumerate(rows):
        one, dg1, db1 = _ln_bwd([lin[g]], mean[off:off + R].clone(), rstd[off:off + R].clone(), gs[g:g + 1], be[g:g + 1], [dys[g]],
                                dtype, None)
        bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert dl[g].dtype == dtype and torch.equal(dl[g][:R].view(bits), one[0][:R].view(bits)), f"dlin[{g}]"
        assert bool((dl[g][R:] == SENT).all()), f"dlin[{g}]: rows past the group's count were written"
        assert bool(torch.isfinite(dl[g][:R].float()).all()) and bool(torch.isfinite(dg[g]).all()) and bool(torch.isfinite(db[g]).all())
        dy = dys[g].double()
        xh = (lin[g].double() - mean[off:off + R].double()[:, None]) * rstd[off:off + R].double()[:, None]
        for name, a, b, c in (("dgamma", dg[g], dg1[0], (dy * xh).abs().sum(0)), ("dbeta", db[g], db1[0], dy.abs().sum(0))):
            err = (a.double() - b.double()).abs()
            print(f"rows={rows} {name}[{g}]: max diff {float(err.max()):.3e}, smallest bound {float(_order_bound(c, R).min()):.3e}")
            if R == 1:
                assert _bits_equal(a, b), f"{name}[{g}]: one addend per column"
            assert bool((err <= _order_bound(c, R)).all()), f"{name}[{g}]"
        off += R


# ------------------------------------------------------------------------------------------------ the op through autograd
def _op_grads(xs, par):
    leaves = [[t.clone().requires_grad_(True) for t in ts] for ts in par]
    ys = ops.linear_ln_group(xs, *leaves, ct=BF16X3, eps=EPS)
    return ys, leaves


@pytest.mark.parametrize("rows", [(97, 2049, 33), (2049, 2305, 4097)], ids=lambda r: "+".join(map(str, r)))
def test_op_unequal_rows_gradients(rows, monkeypatch):
    """ops.linear_ln_group over unequal rows, K = 256: one forward and one LayerNorm-backward launch; dW / db against the
    float64 product of the operands the MFMAs see (dlin as stored in bf16, x rounded to bf16).  Products of two bf16 values are
    exact in fp32, so a gradient element is an fp32 sum of R addends in some order (split-K chunks, atomics): at most R - 1
    roundings of partial sums no larger than sum|addend|, i.e. within R 2^-24 sum|addend| of the exact sum.
    (97, 2049, 33): one weight-gradient launch per row count.  (2049, 2305, 4097), a row past a 256-row chunk each: long
    reductions, ONE grouped launch with a reduction length per group (pq3d_gemm_desc.Kg)."""
    K = 256
    xs = _inputs(rows, K)
    par = _params(len(rows), K)
    gy = [rnd(R, N, seed=90 + g).to(DEV) for g, R in enumerate(rows)]
    seen = _count_calls(monkeypatch)
    ys, leaves = _op_grads(xs, par)
    assert seen == ["pq3d_linear_ln_fwd"]
    del seen[:]
    torch.autograd.backward(list(ys), gy)
    assert seen.count("pq3d_add_ln_bwd:i") == 1 and "pq3d_add_ln_bwd" not in seen
    if min(rows) >= 2048:
        assert seen.count("pq3d_gemm") == 1 and "pq3d_gemm_tt_multi" not in seen
    # the tape and dlin again, from the launches themselves (both bit-reproducible)
    fw = _fwd_launch(xs, par, rows)
    u = 2.0 ** -24
    for g, R in enumerate(rows):
        lin, mean, rstd, y = fw[g]
        assert _bits_equal(ys[g].detach(), y), f"y[{g}]"
        dl, dg1, db1 = _ln_bwd([lin], mean.clone(), rstd.clone(), par[2][g:g + 1], par[3][g:g + 1], [gy[g]], torch.bfloat16, None)
        a = dl[0][:R].double()
        b = xs[g].to(torch.bfloat16).double()
        for name, got, ref, mag in (("dW", leaves[0][g].grad, a.t() @ b, a.abs().t() @ b.abs()),
                                    ("db", leaves[1][g].grad, a.sum(0), a.abs().sum(0))):
            err = (got.double() - ref).abs()
            print(f"R={R} {name}[{g}]: max error {float(err.max()):.3e}, smallest bound {float((R * u * mag).min()):.3e}, "
                  f"largest error / bound {float((err / (R * u * mag).clamp_min(1e-300)).max()):.3e}")
            assert bool((err <= R * u * mag).all()), f"{name}[{g}]"
        dy = gy[g].double()
        xh = (lin.double() - mean.double()[:, None]) * rstd.double()[:, None]
        for name, got, ref, c in (("dgamma", leaves[2][g].grad, dg1[0], (dy * xh).abs().sum(0)),
                                  ("dbeta", leaves[3][g].grad, db1[0], dy.abs().sum(0))):
            assert bool(((got.double() - ref.double()).abs() <= _order_bound(c, R)).all()), f"{name}[{g}]"


def _tt_multi_slices(R, problems, n=N, k=256):
    """k-slices pq3d_gemm_tt_multi gives a [n, k] weight gradient over R rows in a launch of `problems` such products, as
    csrc/gemm_ttmulti.hip's tt_multi_launch decides for its 256 x 128 tile: 64-row chunks, as many slices as keep the launch within
    one round of 256 workgroups, never more than there are chunks."""
    tiles = problems * (n // 256) * (k // 128)
    return max(1, min(256 // tiles, (R + 63) // 64))


def test_op_unequal_rows_sole_writer_bits():
    """Where a weight-gradient element has ONE writer (one k-slice) or two whose sums commute on the zeroed slot (0 + a + b =
    0 + b + a in fp32), dW and db of the ragged op equal the per-group calls' bit for bit.  The issue names rows <= 256 for this;
    which of the candidate row counts up to 256 qualify is derived from pq3d_gemm_tt_multi's slice rule (_tt_multi_slices), in
    the per-group launch (one problem) AND in the ragged op's launch of the row count's class (97 rows: two groups, one launch of
    two problems).  The per-group call is checked to repeat itself first.  The candidates that do not qualify (3-4 slices: the
    per-group call does not repeat its own bits, seen at R = 200) are asserted to be exactly those above 128 rows and are covered
    by test_op_unequal_rows_gradients' bound."""
    K = 256
    cand = (97, 33, 64, 97, 128, 200, 256)
    ok = [R for R in cand if max(_tt_multi_slices(R, 1), _tt_multi_slices(R, cand.count(R))) <= 2]
    assert sorted(set(cand) - set(ok)) == [200, 256], "the slice rule restated here no longer gives 1-2 slices up to 128 rows"
    rows = tuple(ok)
    assert rows.count(97) == 2 and len(rows) == 5
    xs = _inputs(rows, K)
    par = _params(len(rows), K)
    gy = [rnd(R, N, seed=90 + g).to(DEV) for g, R in enumerate(rows)]
    ys, leaves = _op_grads(xs, par)
    torch.autograd.backward(list(ys), gy)
    for g in range(len(rows)):
        runs = []
        for _ in range(2):
            y1, l1 = _op_grads(xs[g:g + 1], [p[g:g + 1] for p in par])
            torch.autograd.backward(list(y1), [gy[g]])
            runs.append(l1)
            assert _bits_equal(y1[0].detach(), ys[g].detach()), f"y[{g}]"
        for k, name in ((0, "dW"), (1, "db")):
            assert _bits_equal(runs[0][k][0].grad, runs[1][k][0].grad), f"{name}[{g}]: the per-group call does not repeat itself"
            assert _bits_equal(leaves[k][g].grad, runs[0][k][0].grad), f"{name}[{g}]"


def test_op_unequal_rows_fallback(monkeypatch):
    """Shapes the one-launch forward does not take (N = 768; an input that wants its gradient) fall back to one grouped call per
    class of equal row count -- the launches of before -- and give those calls' results."""
    seen = _count_calls(monkeypatch)
    rows, K = (40, 24, 40), 256
    xs = _inputs(rows, K)
    par = _params(3, K, 768)
    ys = ops.linear_ln_group(xs, *par, ct=BF16X3, eps=EPS)
    assert "pq3d_linear_ln_fwd" not in seen and seen.count("pq3d_add_ln_fwd") == 2 and seen.count("pq3d_gemm") == 2
    ref = ops.linear_ln_group([xs[0], xs[2]], *[[p[0], p[2]] for p in par], ct=BF16X3, eps=EPS)
    assert _bits_equal(ys[0], ref[0]) and _bits_equal(ys[2], ref[1]) and ys[1].shape == (24, 768)
    del seen[:]
    par = _params(3, K)
    xg = [x.clone().requires_grad_(True) for x in xs]
    ys = ops.linear_ln_group(xg, *par, ct=BF16X3, eps=EPS)
    assert seen.count("pq3d_linear_ln_fwd") == 2
    torch.autograd.backward(list(ys), [torch.ones_like(y) for y in ys])
    assert all(x.grad is not None and x.grad.shape == x.shape for x in xg)


# ------------------------------------------------------------------------------------------------ the model
def _model_args(d, H=8):
    return dict(B=2, Ns=64, Nq=8, d=d, H=H, L=4, memories=["voxel", "mv", "pc"], heads=[], spatial=True, structure="parallel",
                seed=0, data_seed=1234)


def _run_model(model, args, dd, seen):
    del seen[:]
    model.zero_grad()
    out = model({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in dd.items()})
    nf = list(seen)
    del seen[:]
    loss = util.synthetic_loss(out, args["heads"], out["query_embeds"])
    loss.backward()
    return out["query_embeds"].detach().clone(), loss.detach().clone(), nf, list(seen)


def test_model_merges_the_encoders(monkeypatch):
    """config-2-shaped Query3DUnified (bf16 mode) at B = 2, Ns = 64, Nq = 8: with PQ3D_ENC_MERGE on, the position pair and the three
    scene memories are one pq3d_linear_ln_fwd and one pq3d_add_ln_bwd launch (two of each when off), and the outputs are bit for
    bit the same."""
    args = _model_args(256)
    _cfg, model, _sd, dd = util.model_case(args)
    set_compute(model, "bf16")
    model.to(DEV)
    seen = _count_calls(monkeypatch)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "_ENC_MERGE", on)
        res[on] = _run_model(model, args, dd, seen)
        q, loss, fwd, bwd = res[on]
        print(f"merge={on}: forward pq3d_linear_ln_fwd x{fwd.count('pq3d_linear_ln_fwd')}, "
              f"backward pq3d_add_ln_bwd (independent branches) x{bwd.count('pq3d_add_ln_bwd:i')}")
        assert fwd.count("pq3d_linear_ln_fwd") == (1 if on else 2) and bwd.count("pq3d_add_ln_bwd:i") == (1 if on else 2)
    assert _bits_equal(res[True][0], res[False][0]) and _bits_equal(res[True][1], res[False][1])


def test_model_d768_keeps_its_calls(monkeypatch):
    """d = 768 is not the one-launch forward's: the switch changes nothing, launch for launch."""
    args = _model_args(768, H=12)
    _cfg, model, _sd, dd = util.model_case(args)
    set_compute(model, "bf16")
    model.to(DEV)
    seen = _count_calls(monkeypatch)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "_ENC_MERGE", on)
        res[on] = _run_model(model, args, dd, seen)
        assert "pq3d_linear_ln_fwd" not in res[on][2]
    assert res[True][2] == res[False][2] and res[True][3] == res[False][3]
    assert _bits_equal(res[True][0], res[False][0]) and _bits_equal(res[True][1], res[False][1])
