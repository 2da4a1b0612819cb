"""Plain numpy restatements of the PointNet++ point-set entry points (pq3d_amd/csrc/pointnet2.hip), one function per C entry
point, taking the entry point's arguments in its order (inputs as arrays of any shape with the right element count, outputs
returned instead of written, no stream).  Written from the contract the kernels document, loops over the sequential axis
and all, with no project import; tests/test_pointnet2_ref.py keeps them honest against oracle/pointnet2_oracle.py, the F18
fixture and hand-written cases, tests/test_gpu_pointnet2_edges.py compares the kernels with them.

Arithmetic: whatever the GPU tests compare bit for bit is fp32 in the kernels' operation order (the file is built with
-ffp-contract=off, so every product and sum rounds on its own):
  d2(a, b)            ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2
  |p|^2               ((px px) + (py py)) + (pz pz)              (furthest point sampling: a point is live when > 1e-3)
  r2                  fp32(radius) * fp32(radius)                (ball query: a hit is d2 < r2, strictly)
  three_interpolate   ((p0 w0) + (p1 w1)) + (p2 w2)
The two scatter-add gradients are float64, and each has two companions in the style of tests/t5_ref.py's
embedding_bwd_abs / embedding_bwd_terms: the sum of |term| and the number of terms of every output element.

Degenerate cases:
  furthest point sampling   slot 0 is index 0, dead or not; the arg-max takes the SMALLEST index among equal distances; when
                            no live point exists the result is index 0
  ball query                slots past the last hit repeat the first hit; an empty ball is all zeros
  three_nn                  strict '<' insertion in index order, so the earliest index wins among equal distances; with fewer
                            than three known points the missing neighbours have d2 = +inf and index 0"""
import numpy as np

F32 = np.float32


def _a(x, dtype, *shape):
    return np.ascontiguousarray(np.asarray(x, dtype=dtype)).reshape(shape)


def _d2(ax, ay, az, bx, by, bz):
    dx, dy, dz = (ax - bx).astype(F32), (ay - by).astype(F32), (az - bz).astype(F32)
    return ((dx * dx + dy * dy).astype(F32) + dz * dz).astype(F32)


# ------------------------------------------------------------------------------------------------ furthest point sampling
def furthest_point_sampling(xyz, B, N, M):
    """xyz [B,N,3] -> idx [B,M] int32.  Every live point keeps the minimum of its d2 to the points chosen so far (from
    1e10); each step takes the live point with the largest minimum."""
    xyz = _a(xyz, F32, B, N, 3)
    out = np.zeros((B, M), dtype=np.int32)
    for b in range(B):
        x, y, z = xyz[b, :, 0], xyz[b, :, 1], xyz[b, :, 2]
        live = ((x * x + y * y).astype(F32) + z * z).astype(F32) > F32(1e-3)
        mind = np.full(N, 1e10, dtype=F32)
        last = 0
        for s in range(1, M):
            d = _d2(x, y, z, x[last], y[last], z[last])
            mind[live] = np.minimum(d[live], mind[live])
            if live.any():
                best = mind[live].max()
                last = int(np.flatnonzero(live & (mind == best))[0])
            else:
                last = 0
            out[b, s] = last
    return out


# ------------------------------------------------------------------------------------------------ ball query
def ball_query(new_xyz, xyz, B, N, M, radius, nsample):
    """new_xyz [B,M,3] centres, xyz [B,N,3] -> idx [B,M,nsample] int32: the first nsample hits in index order."""
    new_xyz, xyz = _a(new_xyz, F32, B, M, 3), _a(xyz, F32, B, N, 3)
    r2 = F32(F32(radius) * F32(radius))
    out = np.zeros((B, M, nsample), dtype=np.int32)
    for b in range(B):
        for j in range(M):
            c = new_xyz[b, j]
            hits = np.flatnonzero(_d2(c[0], c[1], c[2], xyz[b, :, 0], xyz[b, :, 1], xyz[b, :, 2]) < r2)[:nsample]
            if hits.size:
                out[b, j, :] = hits[0]
                out[b, j, :hits.size] = hits
    return out


# ------------------------------------------------------------------------------------------------ gather / group
def gather_points(points, idx, B, C, N, L):
    """points [B,C,N], idx [B,L] -> out [B,C,L], out[b,c,i] = points[b,c,idx[b,i]] (group_points: L = npoint * nsample)."""
    points, idx = _a(points, F32, B, C, N), _a(idx, np.int64, B, L)
    out = np.empty((B, C, L), dtype=F32)
    for b in range(B):
        out[b] = points[b][:, idx[b]]
    return out


def _scatter(terms, idx, B, C, N):
    """out[b,c,k] = sum of terms[b,c,i] over the i with idx[b,i] == k (float64)."""
    out = np.zeros((B, C, N), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            out[b, c] = np.bincount(idx[b], weights=terms[b, c], minlength=N)
    return out


def gather_points_grad(grad_out, idx, B, C, N, L):
    """grad_out [B,C,L], idx [B,L] -> grad_points [B,C,N] float64."""
    return _scatter(_a(grad_out, np.float64, B, C, L), _a(idx, np.int64, B, L), B, C, N)


def gather_points_grad_abs(grad_out, idx, B, C, N, L):
    return _scatter(np.abs(_a(grad_out, np.float64, B, C, L)), _a(idx, np.int64, B, L), B, C, N)


def gather_points_grad_terms(idx, B, N, L):
    """Number of addends of grad_points[b, :, k] (the same for every channel): [B,N]."""
    idx = _a(idx, np.int64, B, L)
    return np.stack([np.bincount(idx[b], minlength=N) for b in range(B)]) if B else np.zeros((0, N), dtype=np.int64)


# ------------------------------------------------------------------------------------------------ three_nn
def three_nn(unknown, known, B, N, M):
    """unknown [B,N,3], known [B,M,3] -> (dist2 [B,N,3] fp32, idx [B,N,3] int32): the three smallest SQUARED distances in
    ascending order with their indices."""
    unknown, known = _a(unknown, F32, B, N, 3), _a(known, F32, B, M, 3)
    d2 = np.full((B, N, 3), np.inf, dtype=F32)
    idx = np.zeros((B, N, 3), dtype=np.int32)
    for b in range(B):
        ux, uy, uz = unknown[b, :, 0], unknown[b, :, 1], unknown[b, :, 2]
        b1, b2, b3 = (np.full(N, np.inf, dtype=F32) for _ in range(3))
        i1, i2, i3 = (np.zeros(N, dtype=np.int32) for _ in range(3))
        for k in range(M):
            d = _d2(ux, uy, uz, known[b, k, 0], known[b, k, 1], known[b, k, 2])
            first = d < b1
            second = ~first & (d < b2)
            third = ~first & ~second & (d < b3)
            shift3 = first | second                      # the old second best moves to the third place
            b3, i3 = np.where(shift3, b2, np.where(third, d, b3)), np.where(shift3, i2, np.where(third, k, i3))
            b2, i2 = np.where(first, b1, np.where(second, d, b2)), np.where(first, i1, np.where(second, k, i2))
            b1, i1 = np.where(first, d, b1), np.where(first, k, i1)
        d2[b] = np.stack([b1, b2, b3], 1)
        idx[b] = np.stack([i1, i2, i3], 1)
    return d2, idx


# ------------------------------------------------------------------------------------------------ three_interpolate
def three_interpolate(points, idx, weight, B, C, M, N):
    """points [B,C,M], idx / weight [B,N,3] -> out [B,C,N] fp32 = ((p0 w0) + (p1 w1)) + (p2 w2)."""
    points, idx, weight = _a(points, F32, B, C, M), _a(idx, np.int64, B, N, 3), _a(weight, F32, B, N, 3)
    out = np.empty((B, C, N), dtype=F32)
    for b in range(B):
        t = [(points[b][:, idx[b, :, k]] * weight[b, None, :, k]).astype(F32) for k in range(3)]
        out[b] = ((t[0] + t[1]).astype(F32) + t[2]).astype(F32)
    return out


def _interp_scatter(g, idx, w, B, C, M, N):
    out = np.zeros((B, C, M), dtype=np.float64)
    for k in range(3):
        out += _scatter(g * w[:, None, :, k], idx[:, :, k], B, C, M)
    return out


def three_interpolate_grad(grad_out, idx, weight, B, C, M, N):
    """grad_out [B,C,N], idx / weight [B,N,3] -> grad_points [B,C,M] float64: every (i, k) adds grad_out[b,c,i] *
    weight[b,i,k] to grad_points[b,c,idx[b,i,k]]."""
    return _interp_scatter(_a(grad_out, np.float64, B, C, N), _a(idx, np.int64, B, N, 3), _a(weight, np.float64, B, N, 3),
                           B, C, M, N)


def three_interpolate_grad_abs(grad_out, idx, weight, B, C, M, N):
    return _interp_scatter(np.abs(_a(grad_out, np.float64, B, C, N)), _a(idx, np.int64, B, N, 3),
                           np.abs(_a(weight, np.float64, B, N, 3)), B, C, M, N)


def three_interpolate_grad_terms(idx, B, M, N):
    """Number of addends of grad_points[b, :, k]: [B,M] (an index repeated within a row counts every time)."""
    idx = _a(idx, np.int64, B, N * 3)
    return np.stack([np.bincount(idx[b], minlength=M) for b in range(B)]) if B else np.zeros((0, M), dtype=np.int64)
