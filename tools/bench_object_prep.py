#!/usr/bin/env python3
"""Timing of the grounding-batch point sampling (pq3d_amd.objects.sample_objects, csrc/object_prep.hip) at the shipped stage-2
shape: --B 128 items x --O 80 objects x --points 1024 points, on --scans synthetic room scans of --P points cut into
--objects objects each (nearest of random centres, so object sizes straddle 1024: both sampling modes run).  Coordinates are
multiples of 2^-10 and the per-item rotations are quarter turns (entries 0 / +-1): every fp64 sum is exact, so the three legs
must agree bit for bit whatever their summation order.  Per call, [min, median, max] ms of --iters calls after 3 warm-ups:
  sample_ms   objects.sample_objects (device-event pairs)
  torch_ms    the same rule -- the keyed Feistel draw with its cycle walk, the gather, _obj_processing_post in fp64 -- written
              with stock torch operations on the same GPU (device-event pairs; the walk's loop reads one flag per pass)
  host_ms     today's host path: per item, np.random.choice per object as get_scene draws it, the gather from the per-object
              float64 point lists, _obj_processing_post in numpy float64, stacked, cast, copied to the device (--threads
              threads over the items; host clock around work that ends in a device synchronise).  numpy's stream is not
              the rule's: the draw is made for its cost and the gather uses the rule's indices, so that the tables are equal.
Before timing the three legs must give equal tables.  Prints one JSON line: the times, the bytes sample_objects writes and the
fraction of the HBM roof (8.0 TB/s specified, 6.3 TB/s measured by a float4 copy) that is.
    python tools/bench_object_prep.py [--B 128 --O 80 --points 1024 --scans 16 --P 100000 --objects 96 --iters 20 --threads 16]"""
import argparse, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd import objects as OB
from tests import object_prep_ref as R

M32 = 0xFFFFFFFF


def room_scan(seed, n, n_obj, room=(8.0, 6.0, 3.0)):
    """n points in a room, snapped to multiples of 2^-10, colours in [-1, 1]; the instance of a point is its nearest of n_obj
    random centres."""
    r = np.random.default_rng([seed, 4713])
    xyz = np.round(r.random((n, 3)) * np.array(room) * 1024) / 1024
    centres = r.random((n_obj, 3)) * np.array(room)
    ids = np.empty(n, dtype=np.int64)
    for a in range(0, n, 8192):
        ids[a:a + 8192] = ((xyz[a:a + 8192, None] - centres[None]) ** 2).sum(2).argmin(1)
    return np.concatenate([xyz, r.random((n, 3)) * 2 - 1], 1).astype(np.float32), ids


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


def host_ms(fn, iters):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return [round(ts[0], 3), round(statistics.median(ts), 3), round(ts[-1], 3)]


# ------------------------------------------------------------------------------------------- the rule in stock torch
def _fin(h):
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & M32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def torch_indices(n, num_points, seed, O):
    """Positions [N, num_points] int64 of every slot's draws; n [N] int64 points per slot (0 = padded).  int64 tensors hold
    the 32-bit words."""
    dev, N = n.device, n.shape[0]
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    slot = torch.arange(N, device=dev)
    item, q = slot // O, slot % O
    k0 = _fin((s & M32) ^ ((item * 0x9E3779B1) & M32))
    k1 = _fin((k0 + (s >> 32) + ((q * 0x85EBCA6B) & M32) + 0x27D4EB2F) & M32)
    rk = [(_fin((k1 + r * 0x9E3779B1) & M32) ^ k0)[:, None] for r in range(R.ROUNDS)]
    j = torch.arange(num_points, device=dev)[None].expand(N, -1)
    h = j ^ k0[:, None]
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & M32
    h = h ^ (h >> 15)
    h = (h + k1[:, None]) & M32
    h = (h * 0x846CA68B) & M32
    with_repl = ((h ^ (h >> 16)) * n[:, None]) >> 32
    half = torch.ones_like(n)
    for _ in range(10):
        half = torch.where((torch.ones_like(n) << (2 * half)) < n, half + 1, half)
    half, mask, nn = half[:, None], ((torch.ones_like(n) << half) - 1)[:, None], n[:, None]
    walk = (n >= num_points) & (n >= 2)
    x, live = j.clone(), walk[:, None].expand(N, num_points).clone()
    for _ in range(R.WALK_CAP):
        if not bool(live.any()):
            break
        Lh, Rh = x >> half, x & mask
        for r in range(R.ROUNDS):
            Lh, Rh = Rh, Lh ^ (_fin(Rh ^ rk[r]) & mask)
        x = torch.where(live, (Lh << half) | Rh, x)
        live = live & (x >= nn)
    return torch.where(walk[:, None], x, torch.where(nn >= num_points, torch.zeros_like(x), with_repl))


def torch_sample(bank, soi, sel, num_points, seed, rot, return_idx=False):
    B, O = sel.shape
    s = soi.long()[:, None].expand(B, O).reshape(-1)
    o = sel.long().reshape(-1)
    valid = o >= 0
    g = bank.object_offsets.long()[s] + o.clamp(min=0)
    e0 = bank.entry_offsets[g]
    n = torch.where(valid, bank.entry_offsets[g + 1] - e0, torch.zeros_like(e0))
    idx = torch_indices(n, num_points, seed, O)
    if return_idx:
        return idx.view(B, O, num_points)
    pts = bank.order.long()[(e0[:, None] + idx).clamp(max=bank.order.numel() - 1)] + bank.point_offsets[s][:, None]
    rows = bank.points[pts]                                                    # [N, n, 6]
    xyz = rows[:, :, :3].double()
    Rm = rot.double()[:, None].expand(B, O, 3, 3).reshape(-1, 3, 3)
    xyz = torch.stack([(xyz[:, :, 0] * Rm[:, 0, k, None] + xyz[:, :, 1] * Rm[:, 1, k, None]) + xyz[:, :, 2] * Rm[:, 2, k, None]
                       for k in range(3)], 2)
    mean = xyz.sum(1) / float(num_points)
    mn, mx = xyz.amin(1), xyz.amax(1)
    size = mx - mn
    c = xyz - mean[:, None]
    d2 = (c[:, :, 0] * c[:, :, 0] + c[:, :, 1] * c[:, :, 1]) + c[:, :, 2] * c[:, :, 2]
    dist = torch.sqrt(d2.amax(1)).clamp(min=1e-6)
    fts = torch.cat([(c / dist[:, None, None]).float(), rows[:, :, 3:]], 2)
    keep = valid[:, None]
    locs = torch.where(keep, torch.cat([mean, size], 1).float(), 0.0)
    boxes = torch.where(keep, torch.cat([(mn + mx) / 2, size], 1).float(), 0.0)
    fts = torch.where(keep[:, :, None], fts, 0.0)
    return dict(obj_fts=fts.view(B, O, num_points, 6), obj_locs=locs.view(B, O, 6), obj_boxes=boxes.view(B, O, 6),
                obj_pad_masks=valid.view(B, O))


# ------------------------------------------------------------------------------------------- today's host path
def host_item(obj_pcds, sel_b, idx_b, rot_b, num_points):
    """get_scene + _obj_processing_post of one item in numpy float64 (obj_pcds: the scan's per-object float64 point lists)."""
    chosen = [o for o in sel_b if o >= 0]
    for o in chosen:                                                          # the reference's draw (cost only, see the docstring)
        np.random.choice(len(obj_pcds[o]), size=num_points, replace=len(obj_pcds[o]) < num_points)
    pc = np.array([obj_pcds[o][idx_b[q]] for q, o in enumerate(chosen)])      # [n_obj, n, 6] float64
    pc[:, :, :3] = pc[:, :, :3] @ rot_b
    xyz = pc[:, :, :3]
    center, mn, mx = xyz.mean(1), xyz.min(1), xyz.max(1)
    locs = np.concatenate([center, mx - mn], 1)
    boxes = np.concatenate([(mn + mx) / 2, mx - mn], 1)
    xyz -= center[:, None]
    dist = np.maximum(np.sqrt((xyz ** 2).sum(2)).max(1), 1e-6)
    xyz /= dist[:, None, None]
    return pc.astype(np.float32), locs.astype(np.float32), boxes.astype(np.float32)


def host_sample(scan_pcds, soi, sel, idx, rot, num_points, pool):
    B, O = sel.shape
    fts = np.zeros((B, O, num_points, 6), dtype=np.float32)
    locs, boxes = np.zeros((B, O, 6), dtype=np.float32), np.zeros((B, O, 6), dtype=np.float32)
    pad = sel >= 0

    def one(b):
        f, l, x = host_item(scan_pcds[soi[b]], sel[b], idx[b], rot[b], num_points)
        fts[b, :len(f)], locs[b, :len(f)], boxes[b, :len(f)] = f, l, x
    list(pool.map(one, range(B)))
    return dict(obj_fts=torch.from_numpy(fts).cuda(), obj_locs=torch.from_numpy(locs).cuda(), obj_boxes=torch.from_numpy(boxes).cuda(),
                obj_pad_masks=torch.from_numpy(pad).cuda())


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("B", 128), ("O", 80), ("points", 1024), ("scans", 16), ("P", 100_000), ("objects", 96), ("iters", 20),
                          ("threads", 16)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_object_prep.py needs a GPU"
    rng = np.random.default_rng(1)
    scans = [room_scan(300 + s, a.P, a.objects) for s in range(a.scans)]
    t0 = time.perf_counter()
    bank = OB.build_object_bank([torch.from_numpy(p).cuda() for p, _ in scans], point2instance=[torch.from_numpy(i).cuda() for _, i in scans],
                                instance_ids=[torch.arange(a.objects).cuda() for _ in scans])
    torch.cuda.synchronize()
    bank_ms = (time.perf_counter() - t0) * 1e3
    soi = (np.arange(a.B) % a.scans).astype(np.int32)
    sel = np.full((a.B, a.O), -1, dtype=np.int32)
    for b in range(a.B):
        k = min(a.O, bank.num_objects[soi[b]])
        sel[b, :k] = rng.permutation(bank.num_objects[soi[b]])[:k]
    sel[1, a.O // 2:] = -1                                                     # one item with padded slots
    quarter = [np.array(m, dtype=np.float32) for m in ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]],
                                                        [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[0, 1, 0], [-1, 0, 0], [0, 0, 1]])]
    rot = np.stack([quarter[i] for i in rng.integers(0, 4, a.B)])
    seed = 20260
    d_soi, d_sel, d_rot = torch.from_numpy(soi).cuda(), torch.from_numpy(sel).cuda(), torch.from_numpy(rot).cuda()
    d_seed = torch.tensor([seed], dtype=torch.int64, device="cuda")
    ours = lambda: OB.sample_objects(bank, d_soi, d_sel, num_points=a.points, seed=d_seed, rotation=d_rot)
    got, err = ours()
    OB.check_objects(err)
    # the host's per-object float64 lists, and the rule's indices for its gather
    order, entry, ooff = bank.order.cpu().numpy(), bank.entry_offsets.cpu().numpy(), bank.object_offsets.cpu().numpy()
    scan_pcds = [[scans[s][0][order[entry[o]:entry[o + 1]]].astype(np.float64) for o in range(ooff[s], ooff[s + 1])] for s in range(a.scans)]
    idx = torch_sample(bank, d_soi, d_sel, a.points, seed, d_rot, return_idx=True).cpu().numpy()      # (checked through the tables below)
    assert np.array_equal(idx[0, 0], R.sample_indices(len(scan_pcds[soi[0]][sel[0, 0]]), a.points, seed, 0, 0)[0])
    rot64 = rot.astype(np.float64)
    with ThreadPoolExecutor(a.threads) as pool:
        host = lambda: host_sample(scan_pcds, soi, sel, idx, rot64, a.points, pool)
        tch = lambda: torch_sample(bank, d_soi, d_sel, a.points, seed, d_rot)
        for name, other in (("torch", tch()), ("host", host())):
            for k, v in got.items():
                assert torch.equal(v, other[k]), f"{name} leg differs in {k}"
        nbytes = got["obj_fts"].numel() * 4 + 2 * got["obj_locs"].numel() * 4 + got["obj_pad_masks"].numel()
        out = dict(metric="object_prep", B=a.B, O=a.O, points=a.points, scans=a.scans, scan_points=a.P, objects_per_scan=a.objects,
                   valid_slots=int((sel >= 0).sum()), slots_with_replacement=int(sum(len(scan_pcds[soi[b]][o]) < a.points
                                                                                     for b in range(a.B) for o in sel[b] if o >= 0)),
                   iters=a.iters, host_threads=a.threads, legs_equal=True, bank_build_ms=round(bank_ms, 2), bytes_written=nbytes,
                   sample_ms=event_ms(ours, a.iters), torch_ms=event_ms(tch, a.iters), host_ms=host_ms(host, max(3, a.iters // 4)))
    sec = out["sample_ms"][1] * 1e-3
    out["write_TBps"] = round(nbytes / sec / 1e12, 3)
    out["hbm_roof_fraction"] = dict(spec_8p0=round(nbytes / sec / 8.0e12, 3), measured_6p3=round(nbytes / sec / 6.3e12, 3))
    out["torch_over_sample"] = round(out["torch_ms"][1] / out["sample_ms"][1], 2)
    out["host_over_sample"] = round(out["host_ms"][1] / out["sample_ms"][1], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
