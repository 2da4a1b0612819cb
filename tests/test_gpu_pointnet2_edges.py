"""GPU: the PointNet++ point-set kernels (pq3d_amd/csrc/pointnet2.hip) against the restatements of tests/pointnet2_ref.py
(kept honest by tests/test_pointnet2_ref.py) at the sizes where the kernels take another path, on ties, at the radius and
with degenerate clouds.

What is compared how:
  indices (furthest point sampling, ball query, three_nn)     equal
  gather / group forward, three_nn d2, three_interpolate      the same bits as the fp32 restatement (the file is built with
                                                              -ffp-contract=off: fixed-order fp32 expressions)
  three_nn's dist through the wrapper                         the same bits as np.sqrt of the restated d2
  the two scatter-add gradients                               every element against float64: an element that is the fp32
      sum, in any order, of k terms t_1..t_k differs from the exact sum by at most (k - 1) u sum|t_i| (u = 2^-24, first
      order); the tests allow  k u sum|t_i|  for gather and  (k + 1) u sum|t_i|  for interpolate, whose terms g * w are
      themselves fp32 products (one more rounding each).  k = 0: exactly 0.  Gather with k = 1: the same bits.
      The bound is first order in u: the rigorous worst case is gamma_(k-1) = (k - 1) u / (1 - (k - 1) u), which stays
      below k u only while k (k - 1) u <= 1, i.e. k <= 4096.  The one-address cases (k = 16389 and 2 x 16391) are past
      that: there the second-order part, about (k u)^2 = 1e-6 relative, exceeds the one-u slack, so k u sum|t| is not a
      worst-case bound for them.  It is kept as the stated bound all the same: reaching the worst case needs every
      rounding error at its maximum with one sign, while the terms here have random signs and magnitudes, and the
      measured error of those cases is below 1e-3 of the bound.
Outputs whose every element must be written (furthest point sampling, ball query incl. empty balls, three_nn, and the
gather / interpolate forwards at sizes past one grid pass) go through _lib.call into buffers pre-filled with -7 / NaN; the
rest goes through the autograd wrappers.  Every case has B >= 2 with a different cloud per batch entry, and no input or
term is subnormal (gradient values have magnitudes in [0.5, 2): the build uses unsafe fp32 atomics).

Paths by size.  fps_kernel<NT,PT>: N <= 256 <64,4> (one wave: no cross-wave exchange), <= 1024 <256,4>, <= 2048 <256,8>,
<= 4096 <512,8>, <= 8192 <1024,8>.  ball_query_kernel: 64 points per step, pre-fill of nsample slots 64 at a time.
gather_kernel: 16 channels per block, one grid pass covers 65536 elements; gather_grad / three_interpolate(_grad): 16384.
three_nn_kernel: 256 known points per LDS tile, 256 unknown points per block."""
import numpy as np
import pytest
import torch

from pq3d_amd import _lib as L
from pq3d_amd import pointnet2 as P
from tests import pointnet2_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
F32 = np.float32


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def ints(*shape):
    return torch.full(shape, -7, dtype=torch.int32, device=DEV)


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def same(got, want, what=""):
    """Equal as bit patterns, every element (so NaN never passes as 'close' and -0 is not +0)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at flat index {bad[0]}: got " \
                          f"{got.ravel()[bad[0]]!r}, want {want.ravel()[bad[0]]!r}"


def grad_within(got, ref, ref_abs, terms, extra, what=""):
    """|got - ref| <= (k + extra) u sum|t| for EVERY element; k = 0: exactly 0; extra = 0 and k = 1: the same bits."""
    got = got.detach().cpu().numpy()
    assert got.dtype == F32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert np.isfinite(got).all(), what + ": non-finite"
    k = np.broadcast_to(terms[:, None, :], ref.shape)
    tol = (k + extra) * U * ref_abs
    err = np.abs(got.astype(np.float64) - ref)
    w = int(np.argmax(err - tol))
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} of {got.size} out of bound (k {k.min()}..{k.max()}), the " \
                               f"worst at flat index {w}: got {got.ravel()[w]!r}, want {ref.ravel()[w]!r}, k " \
                               f"{k.ravel()[w]}, allowed {tol.ravel()[w]:.3e}"
    assert (got[k == 0] == 0).all(), what + ": an element nothing scatters into is not 0"
    if extra == 0:
        same(got[k == 1], ref[k == 1].astype(F32), what + " (single-term elements)")


def signed(r, *shape):
    """fp32 values with magnitude in [0.5, 2) and a random sign: no zeros, no subnormal terms or partial sums."""
    return (r.uniform(0.5, 2.0, shape) * r.choice([-1.0, 1.0], shape)).astype(F32)


# ------------------------------------------------------------------------------------------------ furthest point sampling
def fps(xyz, M):
    B, N, _ = xyz.shape
    out = ints(B, M)
    L.call("pq3d_furthest_point_sampling", dev(xyz, F32), out, B, N, M)
    return out.cpu().numpy()


def check_fps(xyz, M, what):
    xyz = np.asarray(xyz, dtype=F32)
    B, N, _ = xyz.shape
    got, want = fps(xyz, M), R.furthest_point_sampling(xyz, B, N, M)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: first difference at (batch, step) {tuple(bad[0])}: got {got[tuple(bad[0])]}, want " \
                          f"{want[tuple(bad[0])]}"
    return got


def fps_clouds(N, seed):
    """Two clouds: one on a 0.125 grid (exact arithmetic, duplicated points and equal distances at every step, the origin
    dead), one continuous with a tenth of its points zeroed (dead) at random places."""
    r = np.random.default_rng(seed)
    p = r.uniform(-1, 1, (2, N, 3)).astype(F32)
    p[0] = np.round(p[0] * 8) / 8
    p[1, r.permutation(N)[:N // 10]] = 0.0
    return p


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191,
                               8192])
def test_fps_every_instantiation_and_both_sides_of_every_switch(N):
    check_fps(fps_clouds(N, 1000 + N), min(N, 40), f"N {N}")


def test_fps_single_sample():
    got = check_fps(fps_clouds(300, 5), 1, "M 1")
    assert got.tolist() == [[0], [0]]


def test_fps_lattice_every_step_a_tie():
    g = (np.arange(6) + 1) * 0.25
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(216, 3)
    centred = (lat - 0.875)[np.random.default_rng(3).permutation(216)]        # another cloud: centred, shuffled order
    got = check_fps(np.stack([lat, centred]), 216, "6x6x6 lattice")
    assert sorted(got[0].tolist()) == list(range(216)) and sorted(got[1].tolist()) == list(range(216))


def test_fps_identical_live_points():
    p = np.empty((2, 100, 3), dtype=F32)
    p[0], p[1] = (0.5, 0.25, -1.0), (-0.3, 0.7, 0.2)
    got = check_fps(p, 10, "identical points")
    assert (got == 0).all()                     # every distance is 0 from the first step on: the smallest index, 0


def test_fps_more_samples_than_live_points():
    r = np.random.default_rng(8)
    p = np.zeros((2, 40, 3), dtype=F32)
    live = [np.sort(r.permutation(np.arange(1, 40))[:10]), np.concatenate([[0], np.sort(r.permutation(np.arange(1, 40))[:9])])]
    for b in range(2):
        p[b, live[b]] = r.uniform(0.2, 1, (10, 3))
    got = check_fps(p, 20, "40 points, 10 live, M 20")
    for b in range(2):
        head = got[b, 1:11] if b == 0 else got[b, :10]          # cloud 0 starts on its dead point 0
        assert sorted(head.tolist()) == live[b].tolist()
        assert (got[b, 11:] == live[b][0]).all()                # exhausted: all minima 0 -> the first live point


def test_fps_all_zero_cloud():
    got = check_fps(np.zeros((2, 70, 3), dtype=F32), 5, "all-zero cloud")
    assert (got == 0).all()


def test_fps_dead_first_point():
    p = fps_clouds(300, 6)
    p[:, 0] = 0.0
    got = check_fps(p, 40, "point 0 dead")
    assert (got[:, 0] == 0).all() and (got[:, 1:] != 0).all()


def test_fps_rejects_more_than_8192_points():
    out = ints(2, 4)
    with pytest.raises(L.Pq3dError, match="at most 8192"):
        L.call("pq3d_furthest_point_sampling", dev(fps_clouds(8193, 7)), out, 2, 8193, 4)
    assert (out == -7).all()                    # the check precedes any launch


# ------------------------------------------------------------------------------------------------ ball query
def ball(centers, pts, radius, nsample):
    B, N, _ = pts.shape
    M = centers.shape[1]
    out = ints(B, M, nsample)
    L.call("pq3d_ball_query", dev(centers, F32), dev(pts, F32), out, B, N, M, float(radius), int(nsample))
    return out.cpu().numpy()


def check_ball(centers, pts, radius, nsample, what):
    centers, pts = np.asarray(centers, dtype=F32), np.asarray(pts, dtype=F32)
    B, N, _ = pts.shape
    got = ball(centers, pts, radius, nsample)
    want = R.ball_query(centers, pts, B, N, centers.shape[1], radius, nsample)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: first difference at (batch, centre, slot) {tuple(bad[0])}: got " \
                          f"{got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    return got


@pytest.mark.parametrize("N,M,nsample", [(1, 1, 1), (1, 3, 200), (63, 5, 63), (63, 1, 200), (64, 1, 64), (64, 3, 65),
                                         (65, 5, 1), (65, 3, 64), (130, 5, 200), (130, 1, 63), (130, 3, 65), (130, 5, 64)])
def test_ball_query_sizes(N, M, nsample):
    r = np.random.default_rng(N * 1000 + M * 10 + nsample)
    pts = r.uniform(-1, 1, (2, N, 3)).astype(F32)
    centers = r.uniform(-0.5, 0.5, (2, M, 3)).astype(F32)
    centers[:, 0] = pts[:, N // 2]                        # a centre on a point of the cloud: d2 = 0 is a hit
    for radius in (0.5, 0.8, 3.9):                        # a few hits; about a quarter of the cloud; every point
        check_ball(centers, pts, radius, nsample, f"N {N} M {M} nsample {nsample} radius {radius}")


def test_ball_query_radius_boundary():
    q = np.nextafter(F32(0.25), F32(0))
    pts = np.array([[[0.25, 0, 0], [q, 0, 0], [0, 0.25, 0], [0.1, 0.1, 0]],
                    [[0.1, 0.1, 0], [0, 0.25, 0], [0, 0, -q], [-0.25, 0, 0]]], dtype=F32)
    got = check_ball(np.zeros((2, 1, 3), dtype=F32), pts, 0.25, 4, "radius boundary")
    assert got.tolist() == [[[1, 3, 1, 1]], [[0, 2, 0, 0]]]       # d2 == r2 is outside the ball ('<' is strict)


def _planted(hits_per_centre, N, seed):
    """A cloud whose centre j = (3 j, 0, 0) has exactly the points hits_per_centre[j] within 0.1 of it (radius 0.25); every
    other point lies far from all centres."""
    r = np.random.default_rng(seed)
    pts = (r.uniform(-1, 1, (N, 3)) + (0, 40, 0)).astype(F32)
    centers = np.array([[3.0 * j, 0, 0] for j in range(len(hits_per_centre))], dtype=F32)
    for j, hits in enumerate(hits_per_centre):
        if not hits:
            continue
        v = r.standard_normal((len(hits), 3))
        pts[hits] = centers[j] + 0.1 * r.uniform(0.1, 1, (len(hits), 1)) * v / np.linalg.norm(v, axis=1, keepdims=True)
    return pts, centers


@pytest.mark.parametrize("nsample", [8, 200])
def test_ball_query_planted_hit_patterns(nsample):
    """Per cloud four centres: more than 8 hits within the first 64 points; the 8th hit inside the second 64-point step; a
    first hit at index >= 64 (the pre-fill happens in a later step than the first); an empty ball."""
    ev, od = lambda lo, hi: list(range(lo, hi, 2)), lambda lo, hi: list(range(lo + 1, hi, 2))
    plans = [[ev(0, 40) + [66, 90, 120], od(0, 10) + od(64, 84) + [127], [70, 100, 129], []],      # 20 + 3;  5 + 10 + 1
             [[64, 65, 126, 128], ev(2, 16) + ev(100, 114), [], [1, 5, 11, 21, 33, 41, 51, 61, 63]]]    # 7 + 7;  9
    for plan in plans:                                    # no point serves two centres
        flat = sum(plan, [])
        assert len(set(flat)) == len(flat)
    built = [_planted(plan, 130, 30 + b) for b, plan in enumerate(plans)]
    pts, centers = np.stack([x[0] for x in built]), np.stack([x[1] for x in built])
    got = check_ball(centers, pts, 0.25, nsample, f"planted hits, nsample {nsample}")
    for b, plan in enumerate(plans):
        for j, hits in enumerate(plan):
            want = (hits[:nsample] + hits[:1] * nsample)[:nsample] if hits else [0] * nsample
            assert got[b, j].tolist() == want, (b, j)


def test_ball_query_empty_balls_are_written_as_zeros():
    r = np.random.default_rng(4)
    pts = r.uniform(-1, 1, (2, 130, 3)).astype(F32)
    centers = (r.uniform(-1, 1, (2, 5, 3)) + (0, 0, 30)).astype(F32)
    got = check_ball(centers, pts, 0.5, 65, "empty balls")
    assert (got == 0).all()


# ------------------------------------------------------------------------------------------------ gather / group
@pytest.mark.parametrize("C,Lx,N", [(1, 1, 5), (16, 65535, 300), (17, 65536, 300), (33, 65539, 300), (16, 65539, 41),
                                    (1, 65536, 300)])
def test_gather_forward(C, Lx, N):
    r = np.random.default_rng(C * 100000 + Lx)
    pts = r.standard_normal((2, C, N)).astype(F32)
    idx = r.integers(0, N, (2, Lx)).astype(np.int32)
    idx[:, -1] = N - 1
    out = nans(2, C, Lx)
    L.call("pq3d_gather_points", dev(pts), dev(idx), out, 2, C, N, Lx)
    want = R.gather_points(pts, idx, 2, C, N, Lx)
    same(out.cpu().numpy(), want, f"gather C {C} L {Lx}")
    same(P.gather_operation(dev(pts), dev(idx)).cpu().numpy(), want, f"gather_operation C {C} L {Lx}")


def test_group_forward_257_by_257():
    r = np.random.default_rng(12)
    pts = r.standard_normal((2, 17, 300)).astype(F32)
    idx = r.integers(0, 300, (2, 257, 257)).astype(np.int32)
    got = P.grouping_operation(dev(pts), dev(idx)).cpu().numpy()
    same(got, R.gather_points(pts, idx, 2, 17, 300, 257 * 257).reshape(2, 17, 257, 257), "group 257 x 257")


def check_gather_grad(idx, C, N, seed, what, group=None):
    r = np.random.default_rng(seed)
    B, Lx = idx.shape
    g = signed(r, B, C, Lx)
    feats = torch.zeros(B, C, N, device=DEV, requires_grad=True)
    if group is None:
        P.gather_operation(feats, dev(idx)).backward(dev(g))
    else:
        P.grouping_operation(feats, dev(idx.reshape(B, *group))).backward(dev(g.reshape(B, C, *group)))
    terms = R.gather_points_grad_terms(idx, B, N, Lx)
    grad_within(feats.grad, R.gather_points_grad(g, idx, B, C, N, Lx), R.gather_points_grad_abs(g, idx, B, C, N, Lx), terms,
                0, what)
    return terms


@pytest.mark.parametrize("Lx", [16383, 16384, 16389])
def test_gather_grad_around_one_grid_pass(Lx):
    idx = np.random.default_rng(Lx).integers(0, 500, (2, Lx)).astype(np.int32)
    check_gather_grad(idx, 3, 500, Lx + 1, f"gather grad L {Lx}")


def test_group_grad_set_abstraction_size():
    idx = np.random.default_rng(77).integers(0, 1024, (2, 512 * 32)).astype(np.int32)
    check_gather_grad(idx, 3, 1024, 78, "group grad 512 x 32", group=(512, 32))


def test_gather_grad_all_terms_on_one_address():
    idx = np.empty((2, 16389), dtype=np.int32)
    idx[0], idx[1] = 3, 5
    terms = check_gather_grad(idx, 2, 7, 31, "gather grad, one address")
    assert terms.tolist() == [[0, 0, 0, 16389, 0, 0, 0], [0, 0, 0, 0, 0, 16389, 0]]


def test_gather_grad_permutation_is_bit_equal():
    r = np.random.default_rng(32)
    idx = np.stack([r.permutation(16389), r.permutation(16389)]).astype(np.int32)
    terms = check_gather_grad(idx, 2, 16389, 33, "gather grad, permutation")
    assert (terms == 1).all()


def test_gather_grad_untouched_points_are_zero():
    idx = (2 * np.random.default_rng(34).integers(0, 500, (2, 16384))).astype(np.int32)
    idx[1] += 1                                           # cloud 0 leaves the odd points alone, cloud 1 the even ones
    terms = check_gather_grad(idx, 3, 1000, 35, "gather grad, untouched points")
    assert (terms[0, 1::2] == 0).all() and (terms[1, 0::2] == 0).all()


# ------------------------------------------------------------------------------------------------ three_nn
def check_three_nn(unknown, known, what):
    unknown, known = np.asarray(unknown, dtype=F32), np.asarray(known, dtype=F32)
    B, n, _ = unknown.shape
    m = known.shape[1]
    d2, idx = nans(B, n, 3), ints(B, n, 3)
    tu, tk = dev(unknown), dev(known)
    L.call("pq3d_three_nn", tu, tk, d2, idx, B, n, m)
    rd2, ridx = R.three_nn(unknown, known, B, n, m)
    got = idx.cpu().numpy()
    bad = np.argwhere(got != ridx)
    assert bad.size == 0, f"{what}: first index difference at {tuple(bad[0])}: got {got[tuple(bad[0])]}, want " \
                          f"{ridx[tuple(bad[0])]}"
    same(d2.cpu().numpy(), rd2, what + " d2")
    dist, widx = P.three_nn(tu, tk)
    assert np.array_equal(widx.cpu().numpy(), ridx), what
    same(dist.cpu().numpy(), np.sqrt(rd2), what + " dist")
    return rd2, ridx


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("m", [1, 2, 3, 255, 256, 257, 513])
def test_three_nn_sizes(m, n):
    r = np.random.default_rng(m * 1000 + n)
    d2, idx = check_three_nn(r.uniform(-1, 1, (2, n, 3)), r.uniform(-1, 1, (2, m, 3)), f"three_nn m {m} n {n}")
    if m < 3:                                             # the missing neighbours: +inf and index 0
        assert np.isposinf(d2[:, :, m:]).all() and (idx[:, :, m:] == 0).all() and np.isfinite(d2[:, :, :m]).all()


def test_three_nn_duplicated_known_and_coincident_unknown_points():
    r = np.random.default_rng(9)
    pool = np.round(r.uniform(-1, 1, (2, 24, 3)) * 4) / 4                     # few distinct places, on a 0.25 grid
    known = np.stack([pool[b][r.integers(0, 24, 300)] for b in range(2)])     # duplicates on both sides of the 256 tile
    unknown = np.round(r.uniform(-1, 1, (2, 300, 3)) * 4) / 4                 # equal distances to distinct places too
    unknown[:, :150] = known[:, 299:149:-1]                                   # on top of known points
    d2, idx = check_three_nn(unknown, known, "three_nn duplicates")
    assert (d2[:, :150, 0] == 0).all() and (idx[:, :, 0] < idx[:, :, 1])[d2[:, :, 0] == d2[:, :, 1]].all()


# ------------------------------------------------------------------------------------------------ three_interpolate
def interp_inputs(n, C, m, seed):
    r = np.random.default_rng(seed)
    pts = r.standard_normal((2, C, m)).astype(F32)
    idx = r.integers(0, m, (2, n, 3)).astype(np.int32)
    idx[:, ::7, 1] = idx[:, ::7, 0]                        # a repeated index within a row
    idx[:, ::11, :] = idx[:, ::11, :1]                     # all three the same (what fewer than three known points gives)
    w = r.uniform(0.05, 1.0, (2, n, 3)).astype(F32)
    return pts, idx, w, signed(r, 2, C, n)


def check_interp(pts, idx, w, g, what):
    B, C, m = pts.shape
    n = idx.shape[1]
    out = nans(B, C, n)
    L.call("pq3d_three_interpolate", dev(pts), dev(idx), dev(w), out, B, C, m, n)
    want = R.three_interpolate(pts, idx, w, B, C, m, n)
    same(out.cpu().numpy(), want, what + " forward")
    feats = dev(pts).requires_grad_(True)
    res = P.three_interpolate(feats, dev(idx), dev(w))
    same(res.detach().cpu().numpy(), want, what + " forward (wrapper)")
    res.backward(dev(g))
    terms = R.three_interpolate_grad_terms(idx, B, m, n)
    grad_within(feats.grad, R.three_interpolate_grad(g, idx, w, B, C, m, n),
                R.three_interpolate_grad_abs(g, idx, w, B, C, m, n), terms, 1, what + " grad")
    return terms


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", [1, 16384, 16391])
def test_three_interpolate_and_grad_around_one_grid_pass(n, C):
    terms = check_interp(*interp_inputs(n, C, 50, n + C), f"three_interpolate n {n} C {C}")
    assert n > 1 or (terms == 0).sum() >= 2 * 47          # n = 1: nearly every known point gets no term: exactly 0


def test_three_interpolate_grad_all_rows_on_the_same_three_points():
    pts, idx, w, g = interp_inputs(16391, 3, 10, 55)
    idx[0], idx[1] = (2, 5, 7), (1, 1, 4)
    terms = check_interp(pts, idx, w, g, "three_interpolate, same three points")
    assert terms[0].tolist() == [0, 0, 16391, 0, 0, 16391, 0, 16391, 0, 0]
    assert terms[1].tolist() == [0, 2 * 16391, 0, 0, 16391, 0, 0, 0, 0, 0]
