#!/usr/bin/env python3
"""Timing of mask AP (pq3d_amd.instseg_ap): the GPU overlap tables at P = 200k points, K = 100 columns, G = 60 instances for
B = 1 and B = 4 (ms per scene by device events after warm-up, algorithmic bytes, GB/s), gt_boxes on the same scenes' GT rows,
and on the CPU InstSegAP.compute() over 312 synthetic scenes against the restatement tests/instseg_ap_ref.py (timed on
--ref-scenes of them and scaled).  Also the host bytes kept per scene: tables against the [P, K] masks.  Prints one JSON line.
    python tools/bench_instseg_ap.py [--P 200000 --K 100 --G 60 --iters 20 --scenes 312 --ref-scenes 8]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd import synth
from pq3d_amd.instseg_ap import InstSegAP, gt_boxes, overlap_tables
from pq3d_amd.profiler import KernelTimer

LABELS = (2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 21, 22, 23, 24)


def events(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200_000); ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--G", type=int, default=60); ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scenes", type=int, default=312); ap.add_argument("--scene-P", type=int, default=20_000)
    ap.add_argument("--ref-scenes", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_instseg_ap.py needs a GPU"
    valid = np.array(LABELS)
    out = dict(metric="instseg_ap", P=a.P, K=a.K, G=a.G)
    sc = [synth.instseg_ap_scene(200 + b, P=a.P, K=a.K, G=a.G, labels=LABELS, invalid_labels=(1, 3)) for b in range(4)]
    dev = [(torch.from_numpy(m).cuda(), torch.from_numpy(i).cuda()) for m, i, _s, _c in sc]
    for B in (1, 4):
        buf = torch.cat([d[0] for d in dev[:B]])              # one [sum P, K] buffer, as instance_predictions returns
        masks = list(buf.split(a.P))
        ids = [d[1] for d in dev[:B]]
        ms = events(lambda: overlap_tables(masks, ids, valid), a.iters)
        with KernelTimer() as kt:
            overlap_tables(masks, ids, valid)
        nb = B * a.P * (a.K + 8)                               # mask bytes + ids, read once; the tables are small
        out[f"tables_B{B}"] = dict(ms_per_call=round(ms, 4), ms_per_scene=round(ms / B, 4), bytes=int(nb),
                                   GBps=round(nb / (ms * 1e-3) / 1e9, 1),
                                   kernel_us={f"{n}:{k}": round(v["ms"] * 1e3, 1) for (n, k), v in kt.summary().items()})
    # GT boxes of the 4 scenes: one row per instance
    fms = []
    for m, i, _s, _c in sc:
        u = np.unique(i[i > 0])
        fms.append(torch.from_numpy(i[None, :] == u[:, None]).cuda())
    xyz = [torch.randn(a.P, 3, device="cuda") for _ in range(4)]
    ms = events(lambda: gt_boxes(fms, xyz), a.iters)
    out["gt_boxes_B4"] = dict(rows=int(sum(f.shape[0] for f in fms)), ms_per_call=round(ms, 4), ms_per_scene=round(ms / 4, 4),
                              bytes=int(sum(f.numel() for f in fms)))
    # CPU: compute() over the synthetic set (tables from the GPU), against the restatement
    from tests import instseg_ap_ref
    names = [f"L{x}" for x in LABELS]
    m = InstSegAP(valid, names)
    recs = []
    for b in range(a.scenes):
        mk, i, s, c = synth.instseg_ap_scene(1000 + b, P=a.scene_P, K=a.K, G=50, labels=LABELS, invalid_labels=(1, 3))
        t = overlap_tables([torch.from_numpy(mk).cuda()], [torch.from_numpy(i).cuda()], valid)[0]
        m.add(f"scene{b}", t, s, c)
        recs.append((t, s, c))
    t0 = time.perf_counter()
    m.compute()
    t_ours = time.perf_counter() - t0
    t0 = time.perf_counter()
    instseg_ap_ref.ap_from_tables(recs[:a.ref_scenes], valid)
    t_ref = (time.perf_counter() - t0) * a.scenes / max(a.ref_scenes, 1)
    kept = np.mean([sum(v.nbytes for v in t.values()) + s.nbytes + c.nbytes for t, s, c in recs])
    out.update(compute_s=round(t_ours, 3), scenes=a.scenes, restatement_s_scaled=round(t_ref, 2),
               speedup_vs_restatement=round(t_ref / t_ours, 1), host_bytes_per_scene_tables=int(kept),
               host_bytes_per_scene_masks=int(a.P * a.K))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
