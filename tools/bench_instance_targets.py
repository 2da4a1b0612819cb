#!/usr/bin/env python3
"""Timing of the instance-segmentation training targets (pq3d_amd.scene instance_targets / padded_instance_targets,
csrc/instance_targets.hip) on synthetic room surfaces: --P points per scene, patch segments (about 1.5k per scene), about
60 instances per scene (some unlabelled points, some instances of a filtered class), B = 1 and B = 4.  Per call,
[min, median, max] ms of --iters calls after 3 warm-up calls:
  instance_targets_ms   scene.instance_targets with full masks (host clock around the call: it ends in its one device-to-host read)
  no_full_masks_ms      the same without full_masks (host clock)
  padded_ms             scene.padded_instance_targets at Ns = the largest segment count, max_instances = 100 (device-event
                        pairs; no device-to-host read)
  host_ms               what a caller does today: the id arrays copied to the host, the per-scene tables built there with
                        np.unique (the reference's extract_inst_info, bool masks, without full_masks), then
                        SetCriterion.pad_targets (host clock; --host-iters calls)
  torch_list_ms         stock torch on the same GPU, list form: torch.unique(return_inverse=True), first occurrence by
                        scatter_reduce(amin), index-put masks, per-scene .tolist() for the shapes (host clock)
  torch_padded_ms       stock torch on the same GPU, padded form from the list form: zeros + slice copies (host clock: the
                        list form's reads are part of it)
`equal` reports that the three formulations gave the same tables.  Prints one JSON line.
    python tools/bench_instance_targets.py [--P 100000 --iters 20 --host-iters 5]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd import scene
from pq3d_amd.losses import PaddedTargets, SetCriterion

FILTER = (0, 2)
NT = 100


def room_ids(seed, n, room=(8.0, 6.0, 3.0), seg=0.3, n_inst=60):
    """n points on the floor and the four walls of a room; `seg`-sized patches as segments; instances = the segments nearest to
    n_inst random seeds inside a radius (the rest: -1); one class per instance, 5 % of the points carry another class."""
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
    seeds = xyz[r.integers(0, n, n_inst)]
    d = np.stack([((xyz - s) ** 2).sum(-1) for s in seeds], 1)
    p2i = np.where(d.min(1) < 1.0, d.argmin(1) * 3, -1).astype(np.int64)          # ids with gaps
    own = r.integers(0, 20, n_inst)
    sem = np.where(r.random(n) < 0.05, r.integers(0, 20, n), own[np.maximum(p2i, 0) // 3]).astype(np.int64)
    return p2i, sem, p2s.astype(np.int64)


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


def host_targets(p2i, sem, seg, Ns):
    """The caller's path today: ids to the host, extract_inst_info's tables in numpy, SetCriterion.pad_targets."""
    labels, masks = [], []
    for i, l, s in zip(p2i, sem, seg):
        i, l, s = i.cpu().numpy(), l.cpu().numpy(), s.cpu().numpy()
        ids, first, inv = np.unique(i, return_index=True, return_inverse=True)
        lab = l[first]
        m = np.zeros((len(ids), int(s.max()) + 1), dtype=bool)
        m[inv, s] = True
        keep = (ids != -1) & ~np.isin(lab, FILTER)
        labels.append(torch.from_numpy(lab[keep])); masks.append(torch.from_numpy(m[keep]))
    return SetCriterion.pad_targets(labels, masks, Ns, NT)


def torch_list(p2i, sem, seg, with_full=True):
    """Stock torch ops on the device, one scene at a time."""
    flt = torch.tensor(FILTER, device=p2i[0].device)
    out = dict(instance_ids=[], instance_labels=[], segment_masks=[], full_masks=[])
    for i, l, s in zip(p2i, sem, seg):
        ids, inv = torch.unique(i, return_inverse=True)
        n, P = int(ids.shape[0]), int(i.shape[0])                          # (host sync)
        first = torch.full((n,), P, dtype=torch.int64, device=i.device).scatter_reduce(0, inv, torch.arange(P, device=i.device), "amin")
        lab = l[first]
        m = torch.zeros(n, int(s.max()) + 1, dtype=torch.bool, device=i.device)          # (host sync)
        m[inv, s] = True
        keep = (ids != -1) & ~torch.isin(lab, flt)
        out["instance_ids"].append(ids[keep]); out["instance_labels"].append(lab[keep]); out["segment_masks"].append(m[keep])
        if with_full:
            out["full_masks"].append((torch.arange(n, device=i.device)[:, None] == inv[None, :])[keep])
    return out


def torch_padded(p2i, sem, seg, Ns):
    t = torch_list(p2i, sem, seg, with_full=False)
    B, dev = len(p2i), p2i[0].device
    T = torch.zeros(B, NT, Ns, device=dev)
    lab = torch.zeros(B, NT, dtype=torch.int64, device=dev)
    for b in range(B):
        g, s = t["segment_masks"][b].shape
        T[b, :g, :s] = t["segment_masks"][b].float()
        lab[b, :g] = t["instance_labels"][b]
    return PaddedTargets(T, lab, torch.tensor([m.shape[1] for m in t["segment_masks"]], dtype=torch.int32, device=dev),
                         torch.tensor([m.shape[0] for m in t["segment_masks"]], dtype=torch.int32, device=dev), T.sum(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000); ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_instance_targets.py needs a GPU"
    out = dict(metric="instance_targets", P=a.P, max_instances=NT)
    for B in (1, 4):
        raw = [room_ids(200 + b, a.P) for b in range(B)]
        p2i, sem, seg = ([torch.from_numpy(r[k]).cuda() for r in raw] for k in range(3))
        ours = scene.instance_targets(p2i, sem, seg)
        Ns = max(int(m.shape[1]) for m in ours["segment_masks"])
        stock = torch_list(p2i, sem, seg)
        padded, err = scene.padded_instance_targets(p2i, sem, seg, Ns, NT)
        scene.check_instance_targets(err)
        host, stock_padded = host_targets(p2i, sem, seg, Ns), torch_padded(p2i, sem, seg, Ns)
        equal = all(torch.equal(x, y) for k in ours for x, y in zip(ours[k], stock[k])) and \
            all(torch.equal(getattr(padded, k), getattr(host, k)) and torch.equal(getattr(padded, k), getattr(stock_padded, k))
                for k in PaddedTargets.__slots__)
        res = dict(points=B * a.P, segments=[int(m.shape[1]) for m in ours["segment_masks"]],
                   instances=[int(m.shape[0]) for m in ours["segment_masks"]], equal=bool(equal),
                   full_mask_bytes=sum(int(m.numel()) for m in ours["full_masks"]),
                   instance_targets_ms=host_ms(lambda: scene.instance_targets(p2i, sem, seg), a.iters),
                   no_full_masks_ms=host_ms(lambda: scene.instance_targets(p2i, sem, seg, with_full_masks=False), a.iters),
                   padded_ms=event_ms(lambda: scene.padded_instance_targets(p2i, sem, seg, Ns, NT), a.iters),
                   host_ms=host_ms(lambda: host_targets(p2i, sem, seg, Ns), a.host_iters),
                   torch_list_ms=host_ms(lambda: torch_list(p2i, sem, seg), a.iters),
                   torch_padded_ms=host_ms(lambda: torch_padded(p2i, sem, seg, Ns), a.iters))
        res["padded_speedup_vs_host"] = round(res["host_ms"][1] / res["padded_ms"][1], 2)
        res["padded_speedup_vs_torch"] = round(res["torch_padded_ms"][1] / res["padded_ms"][1], 2)
        res["list_speedup_vs_torch"] = round(res["torch_list_ms"][1] / res["instance_targets_ms"][1], 2)
        out[f"B{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
