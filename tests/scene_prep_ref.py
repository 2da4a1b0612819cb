"""Plain numpy restatement of the scene-preparation rules (pq3d_amd/scene.py): the specification the GPU kernels
are tested against.  float32 arithmetic exactly as specified, loops, nothing clever.  (MinkowskiEngine and fpsample, which
the reference's dataloader calls, are not available, so the expected values cannot come from them.)"""
import numpy as np

F32 = np.float32


def quantize(x: np.ndarray, voxel_size: float) -> np.ndarray:
    """q = floor(x / fp32(voxel_size)) with the correctly rounded fp32 division."""
    x = np.asarray(x, dtype=F32)
    return np.floor(x / F32(voxel_size)).astype(np.int64)


def quantize_reciprocal(x: np.ndarray, voxel_size: float) -> np.ndarray:
    """The WRONG rule (multiplying by the rounded reciprocal); kept so that a test can show that it differs."""
    x = np.asarray(x, dtype=F32)
    return np.floor(x * (F32(1.0) / F32(voxel_size))).astype(np.int64)


def voxelize(coordinates, voxel_size: float):
    """coordinates: list of [P_b, 3].  Returns voxel_coordinates [V, 4] int32 (scene, qx, qy, qz; scene after scene),
    unique_map (per scene: first occurrence of every voxel, ascending) and inverse_map (per scene: voxel of every point)."""
    rows, umaps, invs = [], [], []
    for b, c in enumerate(coordinates):
        q = quantize(c, voxel_size)
        seen, um, inv = {}, [], np.empty(len(q), dtype=np.int64)
        for i in range(len(q)):
            k = (int(q[i, 0]), int(q[i, 1]), int(q[i, 2]))
            if k not in seen:
                seen[k] = len(um)
                um.append(i)
            inv[i] = seen[k]
        um = np.asarray(um, dtype=np.int64)
        rows.append(np.concatenate([np.full((len(um), 1), b, dtype=np.int64), q[um]], 1))
        umaps.append(um)
        invs.append(inv)
    return np.concatenate(rows).astype(np.int32), umaps, invs


def fps(points: np.ndarray, m: int, start_idx: int = 0) -> np.ndarray:
    """Exact farthest point sampling: dist = +inf; d = (dx*dx + dy*dy) + dz*dz in fp32 (every operation rounded on its own);
    dist = min(dist, d); next = arg-max of dist, ties to the smallest index (np.argmax returns the first maximum)."""
    p = np.asarray(points, dtype=F32)
    assert 1 <= m <= len(p) and 0 <= start_idx < len(p)
    dist = np.full(len(p), np.inf, dtype=F32)
    out = np.empty(m, dtype=np.int64)
    out[0] = start_idx
    for s in range(1, m):
        c = p[out[s - 1]]
        dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F32
        dist = np.minimum(dist, d)
        out[s] = int(np.argmax(dist))
    return out


def centers(coordinates: np.ndarray, ids: np.ndarray, size: int) -> np.ndarray:
    """float64 scatter_mean(coordinates, ids, dim_size = size); an id without points gives a zero row."""
    tot = np.zeros((size, 3), dtype=np.float64)
    cnt = np.zeros(size, dtype=np.float64)
    for i in range(len(ids)):
        tot[ids[i]] += coordinates[i].astype(np.float64)
        cnt[ids[i]] += 1
    return tot / np.maximum(cnt, 1)[:, None]
