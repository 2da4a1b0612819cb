#!/usr/bin/env python3
"""Timing of the box matching of box AP (pq3d_amd.instseg_eval.box_match, csrc/instseg_box.hip) on a validation-sized set:
--scenes scenes x --K detections, --G GT boxes per scene over 20 classes, thresholds 0.25 and 0.5, all scenes in one call.
Median ms of --iters runs by device events after warm-up, against two baselines:
  host   the restatement's loops (tests/instseg_eval_ref.py, the reference's host path), timed on --ref-scenes scenes, scaled;
  torch  the same rule in stock torch operations on the same GPU (padded [B, K, G] float64 IoU, first maximum, stable rank,
         scatter-min winner table), from inputs that are already stacked.
kernel_ms is the launch on inputs flattened once (what torch_ms compares with); box_match_lists_ms is box_match on the per-scene
lists of all scenes (it concatenates them on every call: host-bound), box_match_4_scenes_ms / torch_4_scenes_ms the batch one
InstSegEval.update call sees.  All legs must give equal flags before anything is timed.  Prints one JSON line.
    python tools/bench_instseg_eval.py [--scenes 312 --K 100 --G 50 --iters 20 --ref-scenes 8]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd.instseg_eval import box_match

LABELS = (2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 21, 22, 23, 24)
THRESHOLDS = (0.25, 0.5)


def scene(seed, K, G):
    rng = np.random.default_rng([seed, K, G])
    box = lambda n: np.concatenate([rng.normal(size=(n, 3)) * 2, rng.random((n, 3)) + 0.2], 1).astype(np.float32)
    labels = np.asarray(LABELS, np.int64)
    gb, gl = box(G), labels[rng.integers(0, len(labels), G)]
    src, near = rng.integers(0, G, K), rng.random(K) < 0.7
    pb, pc = box(K), labels[rng.integers(0, len(labels), K)]
    jit = gb[src].copy()
    jit[:, :3] += (rng.normal(size=(K, 3)) * 0.08).astype(np.float32)
    jit[:, 3:] *= (1 + rng.normal(size=(K, 1)) * 0.1).astype(np.float32)
    pb[near] = jit[near]
    same = near & (rng.random(K) < 0.85)
    pc[same] = gl[src[same]]
    ps = (rng.permutation(K).astype(np.float32) + np.float32(rng.random())) / np.float32(K)
    return dict(pboxes=pb, pclasses=pc, pscores=ps, gboxes=gb, glabels=gl)


def median_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def torch_match(pb, pc, ps, gb, gl, thr):
    """The rule of pq3d_box_match on padded [B, K, ...] / [B, G, ...] tensors (every row valid) in stock torch operations."""
    B, K, G = pb.shape[0], pb.shape[1], gb.shape[1]
    a, g = pb.double(), gb.double()
    amax, amin = a[..., :3] + a[..., 3:] / 2, a[..., :3] - a[..., 3:] / 2
    gmax, gmin = g[..., :3] + g[..., 3:] / 2, g[..., :3] - g[..., 3:] / 2
    hi = torch.minimum(amax[:, :, None], gmax[:, None])
    lo = torch.maximum(amin[:, :, None], gmin[:, None])
    d = hi - lo
    inter = (d[..., 0] * d[..., 1]) * d[..., 2]
    va, vg = (a[..., 3] * a[..., 4]) * a[..., 5], (g[..., 3] * g[..., 4]) * g[..., 5]
    iou = torch.where((hi > lo).all(-1), inter / ((va[:, :, None] + vg[:, None]) - inter), torch.zeros_like(inter))
    iou = torch.where(pc[:, :, None] == gl[:, None], iou, torch.full_like(iou, -float("inf")))
    ov = iou.max(-1).values
    idx = torch.arange(G, device=pb.device).expand(B, K, G)
    jm = torch.where(iou == ov[..., None], idx, G).min(-1).values                 # the first maximum
    jm = torch.where(ov > -float("inf"), jm, -1)
    order = torch.sort(ps, dim=1, descending=True, stable=True).indices
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(K, device=pb.device).expand(B, K))
    flags = torch.zeros(B, K, dtype=torch.uint8, device=pb.device)
    for t, th in enumerate(thr):
        hit = ov > th
        key = torch.where(hit, rank, K)
        win = torch.full((B, G + 1), K, dtype=rank.dtype, device=pb.device)
        win.scatter_reduce_(1, jm.clamp(min=0), key, "amin")
        flags |= ((hit & (win.gather(1, jm.clamp(min=0)) == rank)).to(torch.uint8) << t)
    return ov, jm, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=312); ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--G", type=int, default=50); ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ref-scenes", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_instseg_eval.py needs a GPU"
    from tests import instseg_eval_ref
    sc = [scene(3000 + b, a.K, a.G) for b in range(a.scenes)]
    t = lambda x: torch.from_numpy(x).cuda()
    preds = [dict(boxes=t(s["pboxes"]), classes=t(s["pclasses"]), scores=t(s["pscores"]),
                  box_valid=torch.ones(a.K, dtype=torch.bool, device="cuda")) for s in sc]
    gts = [dict(boxes=t(s["gboxes"]), labels=t(s["glabels"]), valid=torch.ones(a.G, dtype=torch.bool, device="cuda")) for s in sc]
    pb, pc, ps = (torch.stack([p[k] for p in preds]) for k in ("boxes", "classes", "scores"))
    gb, gl = (torch.stack([g[k] for g in gts]) for k in ("boxes", "labels"))
    thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device="cuda")
    # every leg gives the same flags
    m = box_match(preds, gts, THRESHOLDS)
    assert int(m["err"].item()) == 0
    ov_t, jm_t, fl_t = torch_match(pb, pc, ps, gb, gl, thr)
    assert torch.equal(m["flags"], fl_t.reshape(-1)) and torch.equal(m["jmax"].long(), jm_t.reshape(-1))
    ovmax_equal = bool(torch.equal(m["ovmax"], ov_t.reshape(-1)))
    n_ref = max(1, min(a.ref_scenes, a.scenes))
    rp = {f"s{b}": [(int(c), bx, s_) for c, bx, s_ in zip(sc[b]["pclasses"], sc[b]["pboxes"], sc[b]["pscores"])] for b in range(n_ref)}
    rg = {f"s{b}": [(int(c), bx) for c, bx in zip(sc[b]["glabels"], sc[b]["gboxes"])] for b in range(n_ref)}
    t0 = time.perf_counter()
    ref = instseg_eval_ref.match_arrays(rp, rg, THRESHOLDS)
    host_ms = (time.perf_counter() - t0) * 1e3 * a.scenes / n_ref
    fl = m["flags"].cpu().numpy()
    for b in range(n_ref):
        assert np.array_equal(ref[f"s{b}"][2], fl[b * a.K:(b + 1) * a.K]), f"scene {b}: host flags differ"
    kernel_ms = median_ms(lambda: box_match(preds, gts, THRESHOLDS), a.iters)
    # the launch alone, on inputs flattened once (box_match concatenates the per-scene tensors on every call)
    from pq3d_amd import _lib as L
    from pq3d_amd.instseg_eval import _consts
    koff, goff, thr_d = _consts(pb.device, (a.K,) * a.scenes, (a.G,) * a.scenes, THRESHOLDS)
    NK, NG = a.scenes * a.K, a.scenes * a.G
    pv, gv = torch.ones(NK, dtype=torch.uint8, device="cuda"), torch.ones(NG, dtype=torch.uint8, device="cuda")
    ov2, jm2, fl2, err2 = torch.empty_like(m["ovmax"]), torch.empty_like(m["jmax"]), torch.empty_like(m["flags"]), torch.empty_like(m["err"])
    launch = lambda: L.call("pq3d_box_match", pb, pc, ps, pv, koff, NK, gb, gl, gv, goff, NG, thr_d, len(THRESHOLDS), a.scenes, a.G,
                            ov2, jm2, fl2, err2)
    launch_ms = median_ms(launch, a.iters)
    assert torch.equal(fl2, m["flags"])
    torch_ms = median_ms(lambda: torch_match(pb, pc, ps, gb, gl, thr), a.iters)
    b4_ms = median_ms(lambda: box_match(preds[:4], gts[:4], THRESHOLDS), a.iters)     # the batch an update() call sees
    torch_b4_ms = median_ms(lambda: torch_match(pb[:4], pc[:4], ps[:4], gb[:4], gl[:4], thr), a.iters)
    # kernel_ms and torch_ms both start from stacked inputs; box_match_lists_ms adds the concatenation of the per-scene lists
    out = dict(metric="instseg_box_match", scenes=a.scenes, K=a.K, G=a.G, thresholds=list(THRESHOLDS), iters=a.iters,
               kernel_ms=round(launch_ms, 4), torch_ms=round(torch_ms, 4), box_match_lists_ms=round(kernel_ms, 4),
               box_match_4_scenes_ms=round(b4_ms, 4), torch_4_scenes_ms=round(torch_b4_ms, 4),
               host_restatement_ms_scaled=round(host_ms, 1), host_scenes_timed=n_ref,
               speedup_vs_torch=round(torch_ms / launch_ms, 2), speedup_vs_host=round(host_ms / launch_ms, 1),
               ovmax_bits_equal_torch=ovmax_equal, tp25=int((m["flags"] & 1).sum().item()),
               tp50=int(((m["flags"] >> 1) & 1).sum().item()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
