#!/usr/bin/env python3
"""Timing of the stage-2 grounding loss and evaluator kernels (csrc/ground.hip) at the shipped shape: --B 128 items x --O 80
objects, 1 to --T 8 targets per item, about --sel 4 selected slots per item.  Per call, [min, median, max] ms of --iters calls
after 3 warm-ups (device-event pairs; host clock around work that ends in a device synchronise for the host legs):
  loss_ms / loss_torch_ms        ground_loss forward + backward (weight 10): bce_with_logits_mean against
                                 F.binary_cross_entropy_with_logits(torch.clamp(x, min=-100), y) * 10 with autograd, eager;
  refer_ms / refer_torch_ms      refer_counts (labels + every flag) against argmax / gather / masked sums in stock torch
  f1_ms / f1_graph_ms            multi3drefer_counts: cost matrices, batched assignment, counts; nothing leaves the device (eager, and
                                 per replay of the three launches captured into a graph)
  f1_torch_ms                    the IoU of every (slot, target) pair in stock torch on the GPU (fp32 / fp64 split as the rule has
                                 it), one device-to-host copy, then the padded square and scipy per item on the host
  f1_host_ms                     the reference's host formulation as restated in tests/ground_eval_ref.py: device-to-host copy of
                                 logits and boxes, per item numpy IoU matrix + scipy.optimize.linear_sum_assignment
The loss legs are eager only: autograd is not captured in a process whose eager legs have already created the leaf's gradient
accumulator on the default stream (torch warns that this can break a capture); tests/test_gpu_ground_loss.py captures
Query3DLoss forward + backward from a fresh leaf and replays it bit for bit.
Before timing, every leg must give the same tables (the losses agree to fp32 rounding).  Prints one JSON line.
    python tools/bench_ground_eval.py [--B 128 --O 80 --T 8 --sel 4 --iters 20]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment
from pq3d_amd import ground_eval as GE
from pq3d_amd.losses import bce_with_logits_mean
from tests import ground_eval_ref as R


def event_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return [round(t[0], 4), round(statistics.median(t), 4), round(t[-1], 4)]


def host_ms(fn, iters):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return [round(ts[0], 4), round(statistics.median(ts), 4), round(ts[-1], 4)]


def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def make_batch(B, O, T, n_sel, seed=1):
    rng = np.random.default_rng(seed)
    tb = np.concatenate([rng.random((B, T, 3)) * 6 - 3, rng.random((B, T, 3)) * 1.2 + 0.3], 2)
    n_tgt = rng.integers(1, T + 1, B).astype(np.int32)
    boxes = np.concatenate([rng.random((B, O, 3)) * 6 - 3, rng.random((B, O, 3)) * 1.2 + 0.3], 2).astype(np.float32)
    logits = -(rng.random((B, O)) * 8 + 0.5).astype(np.float32)
    logits[:, O - O // 8:] = -np.inf                                         # padded slots, as GroundHead fills them
    labels = np.zeros((3, B, O), dtype=np.float32)
    for b in range(B):
        P = int(np.clip(n_sel + rng.integers(-2, 3), 0, O - O // 8))
        for k, q in enumerate(rng.permutation(O - O // 8)[:P]):
            logits[b, q] = rng.random() * 6 + 0.5
            if k < n_tgt[b]:
                g = tb[b, k]
                boxes[b, q] = np.concatenate([g[:3] + (rng.random(3) - 0.5) * 0.5 * g[3:], g[3:] * (0.8 + 0.4 * rng.random(3))])
                labels[:, b, q] = (1, 1, rng.random() < 0.6)
    return logits, boxes, tb, n_tgt, labels


def torch_iou(logits, boxes, tb):
    """[B, O, T] fp32 IoU of every slot with every target, and the selection mask: the rule's fp32 / fp64 split in stock torch."""
    ph = boxes[..., 3:] / 2
    pa, pb = ph + boxes[..., :3], -ph + boxes[..., :3]
    pmin, pmax = torch.minimum(pa, pb), torch.maximum(pa, pb)
    th = tb[..., 3:] / 2
    ta, tbb = th + tb[..., :3], -th + tb[..., :3]
    tmin, tmax = torch.minimum(ta, tbb), torch.maximum(ta, tbb)
    dp, dt = pmax - pmin, tmax - tmin
    v1, v2 = ((dp[..., 0] * dp[..., 1]) * dp[..., 2]).double(), (dt[..., 0] * dt[..., 1]) * dt[..., 2]
    d = (torch.minimum(pmax.double()[:, :, None], tmax[:, None]) - torch.maximum(pmin.double()[:, :, None], tmin[:, None])).clamp(min=0)
    inter = (d[..., 0] * d[..., 1]) * d[..., 2]
    iou = (inter / (((v1[:, :, None] + v2[:, None]) - inter) + 1e-8)).float()
    return iou, torch.sigmoid(logits) > 0.5


def f1_torch_leg(logits, boxes, tb, n_tgt_host):
    iou, sel = torch_iou(logits, boxes, tb)
    iou, sel = iou.cpu().numpy(), sel.cpu().numpy()
    out = np.zeros((len(iou), 4), dtype=np.int32)
    for b in range(len(iou)):
        m = iou[b][sel[b], :n_tgt_host[b]]
        P, G = m.shape
        nb = max(P, G)
        if P and G:
            sq = np.zeros((nb, nb), dtype=np.float32)
            sq[:P, :G] = -m
            row, col = linear_sum_assignment(sq)
            v = -sq[row[:P], col[:P]]
            out[b, :2] = (v >= np.float32(0.25)).sum(), (v >= np.float32(0.5)).sum()
        out[b, 2:] = P, G
    return out


def refer_torch_leg(logits, labels, flags):
    B = logits.shape[0]
    pred = torch.argmax(logits, 1)
    hit = labels[:, torch.arange(B, device=logits.device), pred] != 0                       # [3, B]
    cols = torch.cat([torch.ones(1, B, dtype=torch.bool, device=logits.device), hit]).int()   # [4, B]
    groups = [torch.ones(B, dtype=torch.bool, device=logits.device)]
    for f in flags:
        groups += [f, ~f]
    return pred.int(), (torch.stack(groups).int()[:, None, :] * cols[None]).sum(2).int()


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("B", 128), ("O", 80), ("T", 8), ("sel", 4), ("iters", 20)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ground_eval.py needs a GPU"
    logits, boxes, tb, n_tgt, labels = make_batch(a.B, a.O, a.T, a.sel)
    d_logits, d_boxes, d_tb, d_ntgt, d_labels = (torch.from_numpy(v).cuda() for v in (logits, boxes, tb, n_tgt, labels))
    rng = np.random.default_rng(2)
    flags = [torch.from_numpy(rng.random(a.B) < p).cuda() for p in (0.6, 0.4, 0.3)]
    out = dict(metric="ground_eval", B=a.B, O=a.O, T_max=a.T, iters=a.iters)

    # ---- ground_loss forward + backward
    x = d_logits.clone().requires_grad_(True)
    y = d_labels[0]

    def ours_loss():
        loss = bce_with_logits_mean(x, y, 10.0)
        return loss, torch.autograd.grad(loss, x)[0]

    def torch_loss():
        loss = F.binary_cross_entropy_with_logits(torch.clamp(x, min=-100), y) * 10.0
        return loss, torch.autograd.grad(loss, x)[0]

    (l0, g0), (l1, g1) = ours_loss(), torch_loss()
    want = R.bce_logits_mean(logits, labels[0], 10.0)
    assert abs(l0.item() - want) <= 8 * np.spacing(np.float32(want)) and abs(l1.item() - want) <= 1e-5 * want
    assert float((g0 - g1).abs().max()) <= 1e-3 / x.numel()
    del l0, g0, l1, g1
    out.update(loss_ms=event_ms(ours_loss, a.iters), loss_torch_ms=event_ms(torch_loss, a.iters))
    out["loss_torch_over_ours"] = round(out["loss_torch_ms"][1] / out["loss_ms"][1], 2)

    # ---- refer_counts
    ours_refer = lambda: GE.refer_counts(d_logits, d_labels, None, is_multiple=flags[0], is_hard=flags[1], is_view_dependent=flags[2])
    tch_refer = lambda: refer_torch_leg(d_logits, d_labels, flags)
    got, (tp, tc) = ours_refer(), tch_refer()
    assert torch.equal(got.pred, tp) and torch.equal(got.counts, tc), "refer legs differ"
    out.update(refer_ms=event_ms(ours_refer, a.iters), refer_torch_ms=event_ms(tch_refer, a.iters))
    out["refer_torch_over_ours"] = round(out["refer_torch_ms"][1] / out["refer_ms"][1], 2)

    # ---- the Multi3DRefer pipeline
    ours_f1 = lambda: GE.multi3drefer_counts(d_logits, d_boxes, d_tb, d_ntgt)
    tch_f1 = lambda: f1_torch_leg(d_logits, d_boxes, d_tb, n_tgt)
    host_f1 = lambda: R.multi3drefer_batch(d_logits.cpu().numpy(), d_boxes.cpu().numpy(), tb, n_tgt)[0]
    got = ours_f1()
    GE.check_f1_errors(got)
    table = got.out.cpu().numpy()
    assert np.array_equal(table, tch_f1()) and np.array_equal(table, host_f1()), "f1 legs differ"
    out.update(selected_per_item=round(float(table[:, 2].mean()), 2), targets_per_item=round(float(table[:, 3].mean()), 2),
               f1_ms=event_ms(ours_f1, a.iters), f1_torch_ms=host_ms(tch_f1, a.iters), f1_host_ms=host_ms(host_f1, a.iters))
    g, _ = captured(ours_f1)
    out["f1_graph_ms"] = event_ms(g.replay, a.iters)
    out["f1_torch_over_ours"] = round(out["f1_torch_ms"][1] / out["f1_ms"][1], 2)
    out["f1_host_over_ours"] = round(out["f1_host_ms"][1] / out["f1_ms"][1], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
