#!/usr/bin/env python3
"""Timing of the set criterion's matching on the device (pq3d_amd/lsap.py) at bench_criterion.py's sizes.  Prints one
JSON line with
  - the batched device LSA alone on the real cost matrices of _costs, and scipy on the same matrices (results compared);
  - the criterion forward + backward, eager, with matching="host" and matching="device";
  - the device-mode step (padded targets) replayed from a captured graph.
    python tools/bench_lsap.py [--B 4 --Ns 4096 --Nq 200 --layers 13 --inst 60 --steps 20]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment
from pq3d_amd import losses as HL
from pq3d_amd import synth
from pq3d_amd.losses import HungarianMatcher, SetCriterion
from pq3d_amd.lsap import linear_sum_assignment_batched


def _events_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4); ap.add_argument("--Ns", type=int, default=4096)
    ap.add_argument("--Nq", type=int, default=200); ap.add_argument("--layers", type=int, default=13)
    ap.add_argument("--inst", type=int, default=60); ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lsap.py needs a GPU"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = "cuda"
    r = np.random.default_rng(0)
    seg_len = [a.Ns] + [int(x) for x in r.integers(a.Ns // 2, a.Ns, a.B - 1)]
    n_inst = [int(x) for x in r.integers(a.inst // 2, a.inst + 1, a.B)]
    masks, logits, labels, seg = synth.criterion_inputs(seed=1, B=a.B, Ns=a.Ns, Nq=a.Nq, C=201, n_layers=a.layers,
                                                        seg_len=seg_len, n_inst=n_inst)
    W = dict(cost_class=2.0, cost_mask=5.0, cost_dice=2.0)

    def make(matching):
        return SetCriterion(num_classes=200, matcher=HungarianMatcher(num_points=-1, **W), weight_dict={},
                            losses=["labels", "masks"], num_points=-1, class_weights=-1, ignore_label=-100, matching=matching)

    dm = [m.to(dev).requires_grad_(True) for m in masks]
    dl = [l.to(dev).requires_grad_(True) for l in logits]
    res = {"workload": f"set criterion matching, {a.layers} prediction layers x B={a.B} scenes, Ns={a.Ns}, Nq={a.Nq}, "
                       f"C=201, targets/scene {n_inst}", "device": torch.cuda.get_device_name(0)}

    # 1. the LSA alone on the real cost matrices
    with torch.no_grad():
        T, lab, sl, nid, n_inst_h, t_sum = HL._targets_to_device(labels, seg, a.Ns, dev)
        cost, _ = HL._costs(dm, dl, T, lab, sl, nid, t_sum, (2.0, 5.0, 2.0), -100)
    G, Nt = a.layers * a.B, T.shape[1]
    cm = cost[:, 0].reshape(G, a.Nq, Nt).contiguous()
    ncol = nid.repeat(a.layers)
    out = linear_sum_assignment_batched(cm, None, ncol)
    res["device_lsa_ms"] = _events_ms(lambda: linear_sum_assignment_batched(cm, None, ncol), a.steps)
    host = cm.cpu().numpy()
    blocks = [host[g, :, :n_inst_h[g % a.B]] for g in range(G)]
    t0 = time.perf_counter()
    ref = [linear_sum_assignment(b) for b in blocks]
    res["scipy_lsa_ms_same_matrices"] = (time.perf_counter() - t0) * 1e3
    rows, cols, nm, err = (t.cpu().numpy() for t in out)
    res["device_lsa_equals_scipy"] = bool(all(err[g] == 0 and np.array_equal(rows[g, :nm[g]], i) and
                                              np.array_equal(cols[g, :nm[g]], j) for g, (i, j) in enumerate(ref)))
    res["matrices"] = G

    # 2. the criterion forward + backward, eager
    def stepper(crit, **kw):
        def step():
            for t in dm + dl:
                t.grad = None
            losses, _ = crit(dm, dl, **kw)
            sum(losses.values()).backward()
        return step

    for mode in ("host", "device"):
        step = stepper(make(mode), instance_labels=labels, segment_masks=seg)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        res[f"criterion_fwd_bwd_eager_{mode}_ms"] = (time.perf_counter() - t0) / a.steps * 1e3

    # 3. the device-mode step with padded targets, replayed from a captured graph
    crit = make("device")
    static = crit.pad_targets(labels, seg, a.Ns, max(n_inst))
    step = stepper(crit, targets=static)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for t in dm + dl:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses, _ = crit(dm, dl, targets=static)
        sum(losses.values()).backward()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        graph.replay()
    torch.cuda.synchronize()
    res["criterion_fwd_bwd_graph_device_ms"] = (time.perf_counter() - t0) / a.steps * 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
