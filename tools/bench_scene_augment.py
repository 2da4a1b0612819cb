#!/usr/bin/env python3
"""Timing of the train-time scene augmentation (pq3d_amd.scene.augment_scenes, csrc/scene_augment.hip) on synthetic room
surfaces snapped to the test grid (multiples of 2^-10: every fp64 sum is exact, so the three legs must agree bit for bit):
--P points per scene, B = 1 and B = 4, all stages on.  Per call, [min, median, max] ms of --iters calls after 3 warm-up calls:
  augment_ms   scene.augment_scenes (device-event pairs; B > 1 includes the concatenation of the scenes)
  torch_ms     the same rule written with stock torch operations on the same GPU, one scene after the other (device-event pairs)
  host_ms      what a caller without the kernels pays: the scenes copied to the host, the numpy restatement
               (tests/scene_augment_ref.py) with its point-wise part on --threads threads, the results copied back
               (host clock around work that ends in a device synchronise)
Before timing the three legs must give equal tables.  Prints one JSON line.
    python tools/bench_scene_augment.py [--P 100000 --iters 20 --threads 16]"""
import argparse, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd import scene
from tests import scene_augment_ref as R


def room_points(seed, n, room=(8.0, 6.0, 3.0)):
    """n points on the floor and the four walls of a room with 4 mm noise, snapped to multiples of 2^-10; colours in [0, 256)."""
    r = np.random.default_rng([seed, 4712])
    X, Y, Z = room
    areas = np.array([X * Y, X * Z, X * Z, Y * Z, Y * Z])
    face = r.choice(5, n, p=areas / areas.sum())
    u, w, z = r.random(n), r.random(n), np.zeros(n)
    faces = [np.stack([u * X, w * Y, z], 1), np.stack([u * X, z, w * Z], 1), np.stack([u * X, z + Y, w * Z], 1),
             np.stack([z, u * Y, w * Z], 1), np.stack([z + X, u * Y, w * Z], 1)]
    xyz = np.zeros((n, 3))
    for f in range(5):
        xyz[face == f] = faces[f][face == f]
    xyz = np.round((xyz + r.normal(0, 0.004, (n, 3))) * 1024) / 1024
    return xyz.astype(np.float32), r.uniform(0, 255.99, (n, 3)).astype(np.float32)


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


def torch_augment(xs, cs, rows, consts):
    """The rule with every stage on in stock torch operations (one rounded fp32 operation per torch call, no host read):
    rows [B, AUG_K] and consts [6] on the device."""
    f = lambda row, name: row[scene.AUG_FIELDS[name][0]:sum(scene.AUG_FIELDS[name])]
    clip = lambda v: torch.where(v < 0, 0.0, torch.where(v > 255, 255.0, v))
    xo, fo = [], []
    for b, (x, c) in enumerate(zip(xs, cs)):
        row = rows[b]
        mean = (x.double().sum(0) / float(x.shape[0])).float()
        lo, hi = x.min(0).values - mean, x.max(0).values - mean
        off = ((hi - lo) * f(row, "u") + lo) * 0.5
        x = (x - mean) + off
        flip = torch.cat([f(row, "flip"), torch.zeros(1, device=x.device)]) != 0
        x = torch.where(flip, (hi + off) - x, x) * f(row, "scale")
        for Rm in f(row, "rot").view(3, 3, 3):
            x = torch.stack([(Rm[i, 0] * x[:, 0] + Rm[i, 1] * x[:, 1]) + Rm[i, 2] * x[:, 2] for i in range(3)], 1)
        t = torch.trunc(c)
        t = torch.where((t >= 0) & (t <= 255), t, torch.where(t > 255, 255.0, 0.0))
        v = t * f(row, "alpha")
        t = torch.trunc(clip(v + f(row, "beta255")))
        t = torch.trunc(clip(t + f(row, "shift")))
        xo.append(x)
        fo.append(torch.cat([(t - consts[:3]) * consts[3:], x], 1))
    return xo, fo


def host_augment(xs, cs, rows, pool, threads):
    """Today's caller: device -> host, the numpy restatement (point-wise part in `threads` chunks), host -> device."""
    cc = R.color_constants()
    xo, fo = [], []
    for b, (x, c) in enumerate(zip(xs, cs)):
        x, c, p = x.cpu().numpy(), c.cpu().numpy(), R.unpack(rows[b])
        k = R.constants(x, p)
        cuts = np.linspace(0, len(x), threads + 1).astype(int)
        parts = list(pool.map(lambda i: R.apply(x[cuts[i]:cuts[i + 1]], c[cuts[i]:cuts[i + 1]], p, k, cc), range(threads)))
        xo.append(torch.from_numpy(np.concatenate([q[0] for q in parts])).cuda())
        fo.append(torch.from_numpy(np.concatenate([q[1] for q in parts])).cuda())
    return xo, fo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000); ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scene_augment.py needs a GPU"
    out = dict(metric="scene_augment", P=a.P, iters=a.iters, host_threads=a.threads)
    consts = torch.from_numpy(scene.color_constants()).cuda()
    with ThreadPoolExecutor(a.threads) as pool:
        for B in (1, 4):
            raw = [room_points(200 + b, a.P) for b in range(B)]
            xs, cs = ([torch.from_numpy(r[k]).cuda() for r in raw] for k in range(2))
            rows_host = scene.draw_scene_augment(B, scene.SceneAugmentConfig(), np.random.default_rng(B))
            rows, rows_np = rows_host.cuda(), rows_host.numpy()
            ours = scene.augment_scenes(xs, cs, rows)
            scene.check_scene_augment(ours[2])
            for name, other in (("torch", torch_augment(xs, cs, rows, consts)), ("host", host_augment(xs, cs, rows_np, pool, a.threads))):
                for b in range(B):
                    assert torch.equal(ours[0][b], other[0][b]) and torch.equal(ours[1][b], other[1][b]), f"{name} leg differs in scene {b}"
            res = dict(points=B * a.P, legs_equal=True,
                       augment_ms=event_ms(lambda: scene.augment_scenes(xs, cs, rows), a.iters),
                       torch_ms=event_ms(lambda: torch_augment(xs, cs, rows, consts), a.iters),
                       host_ms=host_ms(lambda: host_augment(xs, cs, rows_np, pool, a.threads), a.iters))
            res["torch_over_augment"] = round(res["torch_ms"][1] / res["augment_ms"][1], 2)
            res["host_over_augment"] = round(res["host_ms"][1] / res["augment_ms"][1], 2)
            out[f"B{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
