#!/usr/bin/env python3
"""Timing of instance predictions with the filter and DBSCAN on (pq3d_amd.instseg.instance_predictions, csrc/instseg_dbscan.hip):
synthetic room surfaces at 2 cm voxels (synth.instseg_room: V voxels, Q queries, C classes, K = 100), ms per scene by device
events after warm-up at B = 1 and B = 4 with the per-entry-point breakdown, against the same work on the CPU: the
reference's per-query sklearn.cluster.DBSCAN(eps, min_samples=1) (or the restatement tests/instseg_dbscan_ref.py when
sklearn is missing) timed on --cpu-queries queries of the scene and scaled to Q.  Prints one JSON line.
    python tools/bench_instseg_dbscan.py [--V 100000 --Q 200 --C 200 --K 100 --iters 10 --cpu-queries 4]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd import synth
from pq3d_amd.instseg import instance_predictions
from pq3d_amd.profiler import KernelTimer

KEYS = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps", "raw_coordinates")


def events(fn, iters):
    for _ in range(2):
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
    ap.add_argument("--V", type=int, default=100_000); ap.add_argument("--Q", type=int, default=200)
    ap.add_argument("--C", type=int, default=200); ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--eps", type=float, default=0.95); ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cpu-queries", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_instseg_dbscan.py needs a GPU"
    rooms = [synth.instseg_room(100 + b, V=a.V, Q=a.Q, C=a.C) for b in range(4)]
    out = dict(metric="instseg_dbscan", V=a.V, Q=a.Q, C=a.C, K=a.K, eps=a.eps)
    for B in (1, 4):
        logits = torch.cat([r["pred_logits"] for r in rooms[:B]]).cuda()
        S = max(r["pred_masks"].shape[1] for r in rooms[:B])
        masks = torch.full((B, S, a.Q), -1.0)
        for b, r in enumerate(rooms[:B]):
            masks[b, :r["pred_masks"].shape[1]] = r["pred_masks"][0]
        masks = masks.cuda()
        maps = {k: [r[k][0].cuda() for r in rooms[:B]] for k in KEYS + ("voxel_coordinates",)}

        def run():
            return instance_predictions(logits, masks, *[maps[k] for k in KEYS], topk_per_scene=a.K,
                                        filter_out_no_object_queries=True, use_dbscan=True,
                                        voxel_coordinates=maps["voxel_coordinates"], dbscan_eps=a.eps)
        ms = events(run, a.iters)
        plain = events(lambda: instance_predictions(logits, masks, *[maps[k] for k in KEYS], topk_per_scene=a.K), a.iters)
        with KernelTimer() as kt:
            recs = run()
        stages = {f"{n}:{k}": round(v["ms"] * 1e3, 1) for (n, k), v in kt.summary().items()}
        out[f"B{B}"] = dict(ms_per_call=round(ms, 3), ms_per_scene=round(ms / B, 3), plain_ms_per_scene=round(plain / B, 3),
                            K_b=[int(r["scores"].shape[0]) for r in recs], stage_us=stages)
    # CPU: the reference's per-query DBSCAN on the first scene's kept queries, scaled to all queries
    r = rooms[0]
    mv = r["pred_masks"][0][r["voxel2segment"][0]]
    xyz = r["voxel_coordinates"][0].numpy()
    qs = [q for q in range(a.Q) if bool((mv[:, q] > 0).any())][:a.cpu_queries]
    try:
        from sklearn.cluster import DBSCAN
        how = "sklearn DBSCAN(n_jobs=-1)"
        fit = lambda x: DBSCAN(eps=a.eps, min_samples=1, n_jobs=-1).fit(x).labels_
    except ImportError:
        from tests import instseg_dbscan_ref
        how = "restatement (cKDTree + connected_components)"
        fit = lambda x: instseg_dbscan_ref.components(x, a.eps)
    t0 = time.perf_counter()
    nvox = []
    for q in qs:
        sel = xyz[(mv[:, q] > 0).numpy()]
        nvox.append(int(sel.shape[0]))
        fit(sel)
    per_q = (time.perf_counter() - t0) / max(len(qs), 1)
    out.update(cpu=how, cpu_s_per_query=round(per_q, 4), cpu_query_voxels=nvox, cpu_s_per_scene_scaled=round(per_q * a.Q, 2),
               speedup_vs_cpu_B4=round(per_q * a.Q * 1e3 / out["B4"]["ms_per_scene"], 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
