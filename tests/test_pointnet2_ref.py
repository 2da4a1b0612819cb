"""The restatements of tests/pointnet2_ref.py, held to (1) oracle/pointnet2_oracle.py bit for bit on the inputs of every case
of oracle/run_ref_pointnet2.py::cases(), (2) the outputs of the reference's own kernels (fixture F18) wherever
tests/test_pointnet2.py holds the oracle to them, at its tolerances, and (3) hand-made cases whose answers are written
out: the radius boundary, ties, fewer than three known points, exhausted and dead clouds -- the places no fixture reaches."""
import os

import numpy as np
import pytest

from oracle import pointnet2_oracle as PO
from oracle import run_ref_pointnet2 as RC
from tests import pointnet2_ref as R

F32 = np.float32
INF = np.inf


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero(got.view(u).ravel() != want.view(u).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} != " \
                          f"{want.ravel()[bad[0]]!r}"


def _weights(d2):
    dist = np.sqrt(d2)
    w = (F32(1.0) / (dist + F32(1e-8))).astype(F32)
    return (w / w.sum(2, keepdims=True)).astype(F32)


@pytest.mark.parametrize("name,kind,p", RC.cases(), ids=[c[0] for c in RC.cases()])
def test_restatements_match_the_oracle_bit_for_bit(name, kind, p):
    B = p["B"]
    if kind == "fps":
        pts = RC.cloud(B, p["N"], p["seed"], p["pad_zero"])
        same_bits(R.furthest_point_sampling(pts, B, p["N"], p["M"]), PO.furthest_point_sampling(pts, p["M"]), name)
    elif kind == "ball":
        pts, centers, feats, gout = RC.ball_inputs(p)
        M, ns, C, N = centers.shape[1], p["nsample"], p["C"], p["N"]
        idx = R.ball_query(centers, pts, B, N, M, p["radius"], ns)
        same_bits(idx, PO.ball_query(centers, pts, p["radius"], ns), name)
        same_bits(R.gather_points(feats, idx, B, C, N, M * ns).reshape(B, C, M, ns), PO.group_points(feats, idx), name)
        g = R.gather_points_grad(gout, idx, B, C, N, M * ns)       # the oracle accumulates in float64 too, then rounds
        same_bits(g.astype(F32), PO.gather_points_grad(gout.reshape(B, C, -1), idx.reshape(B, -1), N), name)
    else:
        known, unknown, feats, gout, ggat = RC.interp_inputs(p)
        n, m, C = p["Nu"], p["Nk"], p["C"]
        d2, idx = R.three_nn(unknown, known, B, n, m)
        od2, oidx = PO.three_nn(unknown, known)
        same_bits(idx, oidx, name)
        same_bits(d2, od2, name)
        w = _weights(d2)
        same_bits(R.three_interpolate(feats, idx, w, B, C, m, n), PO.three_interpolate(feats, oidx, w), name)
        fidx = R.furthest_point_sampling(known, B, m, p["M"])
        same_bits(fidx, PO.furthest_point_sampling(known, p["M"]), name)
        same_bits(R.gather_points(feats, fidx, B, C, m, p["M"]), PO.gather_points(feats, fidx), name)
        same_bits(R.gather_points_grad(ggat, fidx, B, C, m, p["M"]).astype(F32), PO.gather_points_grad(ggat, fidx, m), name)


def test_restatements_match_the_reference_kernels_fixture():
    """The comparisons of test_pointnet2.py::test_oracle_matches_the_reference_kernels_fixture, at its tolerances, plus the
    two scatter-add gradients at the tolerances test_hip_kernels_match_the_reference_kernels_fixture gives the kernels."""
    path = os.path.join(os.path.dirname(__file__), "golden", "F18_pointnet2_ref.npz")
    z = np.load(path)        # the fixture is committed: a missing file is an error here, not a skip
    for name, kind, p in RC.cases():
        B = p["B"]
        if kind == "fps":
            pts = RC.cloud(B, p["N"], p["seed"], p["pad_zero"])
            assert np.array_equal(R.furthest_point_sampling(pts, B, p["N"], p["M"]), z[name + "/idx"]), name
        elif kind == "ball":
            pts, centers, feats, gout = RC.ball_inputs(p)
            M, ns, C, N = centers.shape[1], p["nsample"], p["C"], p["N"]
            idx = R.ball_query(centers, pts, B, N, M, p["radius"], ns)
            assert np.array_equal(idx, z[name + "/idx"]), name
            assert np.array_equal(R.gather_points(feats, idx, B, C, N, M * ns).reshape(B, C, M, ns), z[name + "/grouped"]), name
            rg = R.gather_points_grad(gout, idx, B, C, N, M * ns)
            assert np.abs(rg - z[name + "/grouped_grad"]).max() <= 1e-4 * max(1.0, np.abs(rg).max()), name
        else:
            known, unknown, feats, gout, ggat = RC.interp_inputs(p)
            n, m, C = p["Nu"], p["Nk"], p["C"]
            d2, idx = R.three_nn(unknown, known, B, n, m)
            assert np.array_equal(idx, z[name + "/idx"]), name
            assert np.abs(d2 - z[name + "/dist2"]).max() <= 1e-6
            w = z[name + "/weight"]
            assert np.abs(R.three_interpolate(feats, idx, w, B, C, m, n) - z[name + "/interp"]).max() <= 1e-5
            ig = R.three_interpolate_grad(gout, idx, w, B, C, m, n)
            assert np.abs(ig - z[name + "/interp_grad"]).max() <= 1e-4 * max(1.0, np.abs(ig).max())
            fidx = R.furthest_point_sampling(known, B, m, p["M"])
            assert np.array_equal(fidx, z[name + "/fps_idx"]), name
            assert np.array_equal(R.gather_points(feats, fidx, B, C, m, p["M"]), z[name + "/gathered"]), name
            gg = R.gather_points_grad(ggat, fidx, B, C, m, p["M"])
            assert np.abs(gg - z[name + "/gathered_grad"]).max() <= 1e-5 * max(1.0, np.abs(gg).max())


# ---------------------------------------------------------------------------------------------------- written-out cases
def test_fps_ties_take_the_smallest_index():
    #         0          1           2          3           4 (= point 0)
    p = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 0, 0]]
    # from 0: d2 = 0 4 2 2 0 -> 1;  minima 0 0 2 2 0 -> tie, 2;  point 3 keeps min(2, 4) = 2 -> 3;  all 0 -> 0
    assert R.furthest_point_sampling(p, 1, 5, 5).tolist() == [[0, 1, 2, 3, 0]]
    assert PO.furthest_point_sampling(np.array([p], dtype=F32), 5).tolist() == [[0, 1, 2, 3, 0]]
    assert R.furthest_point_sampling(p, 1, 5, 1).tolist() == [[0]]
    assert R.furthest_point_sampling([[3, 4, 5]], 1, 1, 1).tolist() == [[0]]
    assert R.furthest_point_sampling([[3, 4, 5]] * 4, 2, 2, 2).tolist() == [[0, 0], [0, 0]]       # identical live points


def test_fps_dead_points_and_exhausted_clouds():
    # point 0 and point 2 are dead (|p|^2 = 0 and 1e-4 <= 1e-3); slot 0 is index 0 all the same
    p = [[0, 0, 0], [1, 0, 0], [0.01, 0, 0], [-1, 0, 0]]
    # from 0: live minima 1 (pt 1), 1 (pt 3) -> tie, 1;  then 0, min(1, 4) = 1 -> 3;  then 0, 0 -> the first live point, 1
    assert R.furthest_point_sampling(p, 1, 4, 6).tolist() == [[0, 1, 3, 1, 1, 1]]
    assert PO.furthest_point_sampling(np.array([p], dtype=F32), 6).tolist() == [[0, 1, 3, 1, 1, 1]]
    assert R.furthest_point_sampling(np.zeros((2, 5, 3)), 2, 5, 4).tolist() == [[0, 0, 0, 0]] * 2     # nothing live
    # |p|^2 exactly at the threshold is dead ('>' is strict): fp32(1e-3) itself as a squared norm cannot be hit with one
    # coordinate, so take the two sides of it
    lo, hi = F32(0.031622), F32(0.031623)          # lo^2 < 1e-3 < hi^2
    assert F32(lo * lo) <= F32(1e-3) < F32(hi * hi)
    assert R.furthest_point_sampling([[1, 0, 0], [lo, 0, 0], [hi, 0, 0]], 1, 3, 3).tolist() == [[0, 2, 0]]


def test_ball_query_boundary_prefill_and_empty():
    q = float(np.nextafter(F32(0.25), F32(0)))
    pts = [[0.25, 0, 0], [q, 0, 0], [0, 0.25, 0], [0.1, 0.1, 0]]
    for f in (lambda c, p, r, ns: R.ball_query(c, p, 1, 4, 1, r, ns),
              lambda c, p, r, ns: PO.ball_query(np.array([c], dtype=F32), np.array([p], dtype=F32), r, ns)):
        assert f([[0, 0, 0]], pts, 0.25, 4).tolist() == [[[1, 3, 1, 1]]]       # d2 == r2 is outside
        assert f([[0, 0, 0]], pts, 0.25, 1).tolist() == [[[1]]]
        assert f([[0, 0, 0]], pts, 1.0, 3).tolist() == [[[0, 1, 2]]]           # more hits than slots: the first three
        assert f([[0, 0, 0]], pts, 1.0, 6).tolist() == [[[0, 1, 2, 3, 0, 0]]]  # the rest repeats the first hit
        assert f([[9, 9, 9]], pts, 0.25, 3).tolist() == [[[0, 0, 0]]]          # empty ball
    two = R.ball_query([[0, 0, 0], [0, 0.25, 0], [9, 9, 9], [0, 0, 0]], pts + [[9, 9, 9]] * 4, 2, 4, 2, 0.25, 2)
    assert two.tolist() == [[[1, 3], [2, 3]], [[0, 1], [0, 0]]]                # batch 1 has its own cloud and centres


def test_gather_and_its_gradient():
    pts = np.arange(2 * 3 * 4, dtype=F32).reshape(2, 3, 4)          # points[b, c, k] = 12 b + 4 c + k
    idx = [[0, 0, 2], [3, 1, 3]]
    out = R.gather_points(pts, idx, 2, 3, 4, 3)
    assert out.dtype == F32 and out[0].tolist() == [[0, 0, 2], [4, 4, 6], [8, 8, 10]]
    assert out[1].tolist() == [[15, 13, 15], [19, 17, 19], [23, 21, 23]]
    g = [[[1, -2, 4]], [[8, 16, -32]]]
    grad = R.gather_points_grad(g, idx, 2, 1, 4, 3)
    assert grad.dtype == np.float64 and grad.tolist() == [[[-1, 0, 4, 0]], [[0, 16, 0, -24]]]
    assert R.gather_points_grad_abs(g, idx, 2, 1, 4, 3).tolist() == [[[3, 0, 4, 0]], [[0, 16, 0, 40]]]
    assert R.gather_points_grad_terms(idx, 2, 4, 3).tolist() == [[2, 0, 1, 0], [0, 1, 0, 2]]


def test_three_nn_fewer_than_three_known_points():
    for f in (lambda u, k: R.three_nn(u, k, 1, len(u), len(k)),
              lambda u, k: PO.three_nn(np.array([u], dtype=F32), np.array([k], dtype=F32))):
        d2, idx = f([[1, 0, 0], [0, 2, 0]], [[0, 0, 0]])
        assert d2.dtype == F32 and idx.dtype == np.int32 and d2.shape == idx.shape == (1, 2, 3)
        assert d2.tolist() == [[[1, INF, INF], [4, INF, INF]]] and idx.tolist() == [[[0, 0, 0], [0, 0, 0]]]
        d2, idx = f([[0, 0, 0], [3, 0, 0]], [[2, 0, 0], [0, 0, 0]])
        assert d2.tolist() == [[[0, 4, INF], [1, 9, INF]]] and idx.tolist() == [[[1, 0, 0], [0, 1, 0]]]
        d2, idx = f([[0, 0, 0]], [[2, 0, 0], [0, 0, 0], [1, 0, 0]])
        assert d2.tolist() == [[[0, 1, 4]]] and idx.tolist() == [[[1, 2, 0]]]


def test_three_nn_equal_distances_keep_the_earliest_index():
    a, b = [1, 2, 3], [1, 2, 4]
    for f in (lambda u, k: R.three_nn(u, k, 1, len(u), len(k)),
              lambda u, k: PO.three_nn(np.array([u], dtype=F32), np.array([k], dtype=F32))):
        d2, idx = f([a, b], [a, a, b, a, b])          # duplicated known points, unknown points on top of them
        assert idx.tolist() == [[[0, 1, 3], [2, 4, 0]]] and d2.tolist() == [[[0, 0, 0], [0, 0, 1]]]
        d2, idx = f([[0, 0, 0]], [[0, 0, 2], [0, 1, 0], [0, 0, -2], [-1, 0, 0], [1, 0, 0]])     # 4 1 4 1 1
        assert idx.tolist() == [[[1, 3, 4]]] and d2.tolist() == [[[1, 1, 1]]]
        d2, idx = f([[0, 0, 0]], [[0, 0, 2], [0, 0, -2], [0, 1, 0], [2, 0, 0]])                 # 4 4 1 4
        assert idx.tolist() == [[[2, 0, 1]]] and d2.tolist() == [[[1, 4, 4]]]


def test_three_interpolate_and_its_gradient():
    pts = [[[1, 2, 3], [10, 20, 30]], [[-1, -2, -3], [0.5, 0.25, 0.125]]]
    idx = [[[0, 1, 1], [2, 2, 2]], [[0, 0, 1], [2, 1, 0]]]
    w = [[[0.5, 0.25, 0.25], [1, 2, 4]], [[0.5, 0.5, 1], [8, 4, 2]]]
    out = R.three_interpolate(pts, idx, w, 2, 2, 3, 2)
    assert out.dtype == F32 and out.tolist() == [[[1.5, 21], [15, 210]], [[-3, -34], [0.75, 3]]]
    same_bits(out, PO.three_interpolate(np.array(pts, dtype=F32), np.array(idx), np.array(w, dtype=F32)))
    g = [[[1, -1]], [[2, 4]]]
    grad = R.three_interpolate_grad(g, idx, w, 2, 1, 3, 2)
    assert grad.dtype == np.float64 and grad.tolist() == [[[0.5, 0.5, -7]], [[10, 18, 32]]]
    assert R.three_interpolate_grad_abs(g, idx, w, 2, 1, 3, 2).tolist() == [[[0.5, 0.5, 7]], [[10, 18, 32]]]
    assert R.three_interpolate_grad_terms(idx, 2, 3, 2).tolist() == [[1, 2, 3], [3, 2, 1]]
    # the forward's rounding order: ((p0 w0) + (p1 w1)) + p2 w2 in fp32, not a float64 sum rounded once
    e = 2.0 ** -24
    one = R.three_interpolate([[[1, e, e]]], [[[0, 1, 2]]], [[[1, 1, 1]]], 1, 1, 3, 1)
    assert one.tolist() == [[[1.0]]]                  # 1 + e rounds to 1 twice; the exact sum 1 + 2e would round to 1 + 2e
    other = R.three_interpolate([[[1, e, e]]], [[[1, 2, 0]]], [[[1, 1, 1]]], 1, 1, 3, 1)
    assert other.tolist() == [[[1.0 + 2 * e]]]
