#!/usr/bin/env python3
"""Timing of the instance-prediction step (pq3d_amd.instseg.instance_predictions; the reference's
InstSegEval.eval_instance_step without DBSCAN) at the full-size scene (P = 200k points, V ~ 100k voxels, S = 4096 segments,
Q = 200 queries, C = 200 classes, top-100) for B = 1 and B = 4 (c4-like), against the CPU restatement tests/instseg_ref.py.
Prints one JSON line: ms per scene by device events after warm-up, the algorithmic bytes and the achieved GB/s, the time per
entry point (profiler.KernelTimer, a separate pass) and the CPU time per scene.
    python tools/bench_instseg_post.py [--P 200000 --S 4096 --Q 200 --C 200 --K 100 --iters 20]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pq3d_amd import synth
from pq3d_amd.instseg import instance_predictions
from pq3d_amd.profiler import KernelTimer

KEYS = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps", "raw_coordinates")


def algorithmic_bytes(inp, K):
    """What the step must read and write once: logits, mask logits, the index maps, the coordinates, the bool masks and the
    per-selection outputs (the [S, K] bit table and the vote stay in cache and are not counted)."""
    B, Q, C1 = inp["pred_logits"].shape
    S = inp["pred_masks"].shape[1]
    V = sum(t.numel() for t in inp["voxel2segment"])
    P = sum(t.numel() for t in inp["voxel_to_full_maps"])
    return B * Q * C1 * 4 + B * S * Q * 4 + V * 8 + P * (8 + 8 + 12) + P * K + B * K * (4 + 8 + 24 + 1)


def run(a, B):
    inp = synth.instseg_inputs(1, P=(a.P,) * B, S=a.S, Q=a.Q, C=a.C, mean_seg=60)
    d = {"pred_logits": inp["pred_logits"].cuda(), "pred_masks": inp["pred_masks"].cuda()}
    d.update({k: [t.cuda() for t in inp[k]] for k in KEYS})
    args = (d["pred_logits"], d["pred_masks"]) + tuple(d[k] for k in KEYS)
    for _ in range(3):
        instance_predictions(*args, topk_per_scene=a.K)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        instance_predictions(*args, topk_per_scene=a.K)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    with KernelTimer() as kt:
        instance_predictions(*args, topk_per_scene=a.K)
    kern = {f"{n}:{k}": round(v["ms"] * 1e3, 1) for (n, k), v in kt.summary().items()}
    nb = algorithmic_bytes(inp, a.K)
    return inp, dict(B=B, ms_per_call=round(ms, 4), ms_per_scene=round(ms / B, 4), bytes=int(nb),
                     GBps=round(nb / (ms * 1e-3) / 1e9, 1), kernel_us=kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200_000); ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--Q", type=int, default=200); ap.add_argument("--C", type=int, default=200)
    ap.add_argument("--K", type=int, default=100); ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-iters", type=int, default=2); ap.add_argument("--batches", default="1,4")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_instseg_post.py needs a GPU"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    res = {}
    inp1 = None
    for B in (int(x) for x in a.batches.split(",")):
        inp, res[B] = run(a, B)
        inp1 = inp1 if B != 1 else inp
    out = dict(metric="instseg_predictions", P=a.P, S=a.S, Q=a.Q, C=a.C, K=a.K, full_size=res.get(1), c4_like=res.get(4))
    if a.cpu_iters > 0 and inp1 is not None:
        from tests import instseg_ref
        t = time.perf_counter()
        for _ in range(a.cpu_iters):
            instseg_ref.predictions(inp1, a.K)
        cpu_ms = (time.perf_counter() - t) * 1e3 / a.cpu_iters
        out.update(cpu_restatement_ms_per_scene=round(cpu_ms, 2), torch_threads=torch.get_num_threads(),
                   speedup_vs_cpu=round(cpu_ms / res[1]["ms_per_scene"], 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
