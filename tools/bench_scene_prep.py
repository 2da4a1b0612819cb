#!/usr/bin/env python3
"""Timing of scene preparation (pq3d_amd.scene, csrc/scene_prep.hip) on synthetic room surfaces (the surfaces of
synth.instseg_room, raw points not snapped to the lattice): --P points per scene at 2 cm voxels, B = 1 and B = 4, M = 120
queries.  Per call, [min, median, max] ms of --iters calls after 3 warm-up calls:
  voxelize_ms   scene.voxelize (host clock around the call: it ends in its one device-to-host read)
  fps_ms        scene.farthest_point_sample on the float voxel lattice coordinates (device-event pairs; key kernels, the
                sort of the Morton keys, staging and the sampling loop)
  prepare_ms    the whole scene.prepare_instseg_batch (host clock; two device-to-host reads)
  torch_fps_ms  the same sampling as a stock-torch loop on the same GPU: the scenes padded to [B, N, 3], M - 1 steps of
                gather / subtract / square / minimum / argmax (device-event pairs).  torch.argmax does not fix the order of
                ties, so on a lattice its sequence may differ: torch_same_sequence reports whether it did not
  rescan_share  tiles re-scanned per step / tiles, mean over the M - 1 steps and the scenes (1.0 = no pruning)
Prints one JSON line.    python tools/bench_scene_prep.py [--P 100000 --M 120 --iters 20 --torch-iters 5]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd import scene

VOXEL = 0.02


def room_points(seed, n, room=(8.0, 6.0, 3.0), seg=0.3):
    """n points on the floor and the four walls of a room with 4 mm noise, `seg`-sized patches as segments, colour | xyz."""
    r = np.random.default_rng([seed, 4711])
    X, Y, Z = room
    areas = np.array([X * Y, X * Z, X * Z, Y * Z, Y * Z])
    face = r.choice(5, n, p=areas / areas.sum())
    u, w, z = r.random(n), r.random(n), np.zeros(n)
    faces = [np.stack([u * X, w * Y, z], 1), np.stack([u * X, z, w * Z], 1), np.stack([u * X, z + Y, w * Z], 1),
             np.stack([z, u * Y, w * Z], 1), np.stack([z + X, u * Y, w * Z], 1)]
    xyz = np.zeros((n, 3))
    for f in range(5):
        xyz[face == f] = faces[f][face == f]
    cell = np.floor(xyz / seg).astype(np.int64)
    _, p2s = np.unique((face * 1000 + cell[:, 0]) * 1000000 + cell[:, 1] * 1000 + cell[:, 2], return_inverse=True)
    xyz = (xyz + r.normal(0, 0.004, (n, 3))).astype(np.float32)
    return xyz, np.concatenate([r.random((n, 3)).astype(np.float32), xyz], 1), p2s.astype(np.int64)


def host_ms(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return [round(ts[0], 3), round(statistics.median(ts), 3), round(ts[-1], 3)]


def event_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return [round(t[0], 3), round(statistics.median(t), 3), round(t[-1], 3)]


def torch_fps(pts, valid, m):
    """pts [B, N, 3] padded, valid [B, N]: the M-step loop in stock torch ops, first sample row 0."""
    B = pts.shape[0]
    rows = torch.arange(B, device=pts.device)
    dist = torch.where(valid, torch.inf, -1.0).float()
    idx = torch.zeros(B, dtype=torch.long, device=pts.device)
    out = torch.empty(B, m, dtype=torch.long, device=pts.device)
    out[:, 0] = idx
    for s in range(1, m):
        d = pts - pts[rows, idx][:, None, :]
        d = d * d
        dist = torch.minimum(dist, (d[..., 0] + d[..., 1]) + d[..., 2])
        idx = dist.argmax(1)
        out[:, s] = idx
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000); ap.add_argument("--M", type=int, default=120)
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--torch-iters", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scene_prep.py needs a GPU"
    out = dict(metric="scene_prep", P=a.P, M=a.M, voxel_size=VOXEL)
    for B in (1, 4):
        raw = [room_points(100 + b, a.P) for b in range(B)]
        xyz, feat, p2s = ([torch.from_numpy(r[k]).cuda() for r in raw] for k in range(3))
        vc, um, _inv = scene.voxelize(xyz, VOXEL)
        V = [int(u.shape[0]) for u in um]
        lattice = list(torch.split(vc[:, 1:].float(), V))
        idx, scanned, tiles = scene.farthest_point_sample(lattice, a.M, return_scanned=True)
        share = float(np.mean([int(s) / ((a.M - 1) * t) for s, t in zip(scanned.tolist(), tiles)]))
        N = max(V)
        pad = torch.zeros(B, N, 3, device="cuda")
        valid = torch.zeros(B, N, dtype=torch.bool, device="cuda")
        for b in range(B):
            pad[b, :V[b]], valid[b, :V[b]] = lattice[b], True
        res = dict(points=B * a.P, voxels=V, tiles=tiles, rescan_share=round(share, 4),
                   voxelize_ms=host_ms(lambda: scene.voxelize(xyz, VOXEL), a.iters),
                   fps_ms=event_ms(lambda: scene.farthest_point_sample(lattice, a.M), a.iters),
                   prepare_ms=host_ms(lambda: scene.prepare_instseg_batch(xyz, feat, p2s, VOXEL, a.M), a.iters),
                   torch_fps_ms=event_ms(lambda: torch_fps(pad, valid, a.M), a.torch_iters),
                   torch_same_sequence=bool(torch.equal(torch_fps(pad, valid, a.M), idx)))
        res["fps_speedup"] = round(res["torch_fps_ms"][1] / res["fps_ms"][1], 2)
        out[f"B{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
