#!/usr/bin/env python3
"""Timing of the frozen voxel backbone (pq3d_amd.sparse.Res16UNet34C, csrc/sparse_conv.hip) on synthetic room surfaces at 2 cm
voxels (synth.instseg_room: V voxels per scene), B = 1 and B = 4, compute 'fp32' and 'bf16':
  map_ms      building the coordinate pyramid and every kernel map (host clock around work that ends in a synchronise; it
              contains the one host synchronisation per batch), median of --map-iters
  total_ms    all convolutions of one forward: every one of --iters forwards after 3 warm-up forwards is timed with its own
              device-event pair; [min, median, max] (the torch loop: --torch-iters forwards)
  max_rel_diff  the largest relative L2 difference between a feature map of ours and the torch loop's, at the size timed
  classes     per convolution class (level = tensor stride of the OUTPUT rows x kind): calls, ms (device event pairs around the
              launches of one forward: they include launch gaps, so their sum exceeds what a trace would give), and the
              achieved algorithmic TFLOP/s and GB/s (2 P Cin Cout operations, P = present (row, offset) pairs of the map -- on
              surfaces about a third of N_out K; input rows, map, output and weights counted once)
  torch_*     baseline: the textbook gather -> matmul -> index_add_ loop over the kernel offsets in stock torch on the same
              GPU, same inputs, same maps (index lists prepared outside the timed window), BatchNorm / residual / ReLU as
              separate torch ops -- there is no MinkowskiEngine for this GPU to compare with
--train times forward + backward of the TRAINABLE network instead (batch-statistics BatchNorm, sparse-convolution backward):
  fwd_bwd_ms / torch_fwd_bwd_ms  one training forward + backward, ours and the same torch loop under torch autograd with
              batch_norm in training mode; [min, median, max] by the same device-event method
  classes     (B = 4) calls and ms of ours per class of launch (forward convolution, input gradient, weight gradient, BatchNorm,
              1 x 1 GEMM) and torch_ms: the torch loop's time for the same class of work on the same tensors
Prints one JSON line.    python tools/bench_voxel_backbone.py [--train] [--V 100000 --iters 30 --torch-iters 8]"""
import argparse, json, os, re, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pq3d_amd import sparse, synth
from pq3d_amd.profiler import KernelTimer


def room_coords(B, V):
    rows = []
    for b in range(B):
        xyz = synth.instseg_room(100 + b, V=V, Q=1, C=1)["voxel_coordinates"][0].numpy()
        q = np.unique(np.round(xyz / 0.02).astype(np.int64), axis=0)
        rows.append(np.concatenate([np.full((len(q), 1), b), q], 1))
    return torch.from_numpy(np.concatenate(rows)).int()


def events(fn, iters):
    """[min, median, max] ms of `iters` calls, each between its own pair of device events, after 3 warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return [round(t[0], 3), round(statistics.median(t), 3), round(t[-1], 3)]


class TorchLoop:
    """sparse.sparse_conv / sparse.row_gemm with the same signatures in stock torch ops, timed per call with event pairs."""

    def __init__(self):
        self.pairs, self.records = {}, []

    def _timed(self, key, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); y = fn(); e1.record()
        self.records.append((key, e0, e1))
        return y

    def conv(self, x, kmap, W, *, ct=0, scale=None, shift=None, bias=None, residual=None, act=None, out=None, col_off=0, use_occ=True):
        if id(kmap) not in self.pairs:      # index lists per offset: part of the map, prepared outside the timed window (warm-up)
            self.pairs[id(kmap)] = [((kmap.nbr[:, k] >= 0).nonzero()[:, 0], kmap.nbr[:, k][kmap.nbr[:, k] >= 0].long()) for k in range(kmap.K)]
        pairs, dt = self.pairs[id(kmap)], (torch.bfloat16 if ct == 1 else torch.float32)
        K, Cin, Cout = W.shape
        if out is None:
            out = torch.empty(kmap.n_out, col_off + Cout, device=x.device)

        def run():
            acc = torch.zeros(kmap.n_out, Cout, device=x.device)
            xs = x.to(dt)
            for k, (o, i) in enumerate(pairs):
                if o.numel():
                    acc.index_add_(0, o, (xs[i] @ W[k].to(dt)).float())
            y = acc
            if scale is not None:
                y = y * scale + shift
            if bias is not None:
                y = y + bias
            if residual is not None:
                y = y + residual
            out[:, col_off:col_off + Cout] = torch.relu(y) if act == "relu" else y
            return out
        return self._timed(("conv", kmap.n_out, kmap.n_in, K), run)

    def gemm(self, x, Wt, bias, ct, act=None):
        dt = torch.bfloat16 if ct == 1 else torch.float32
        def run():
            y = (x.to(dt) @ Wt.t().to(dt)).float()
            return y + bias if bias is not None else y
        return self._timed(("gemm", x.shape[0], x.shape[0], 1), run)


def torch_train_step(model, pyr, feats, tl, Rs):
    """Forward + backward of the TRAINING network in stock torch under autograd: the gather -> matmul -> index_add loop per
    offset, nn.functional.batch_norm in training mode (on copies of the running buffers), ReLU, torch.cat.  Returns the
    parameter gradients."""
    import torch.nn.functional as F
    ct = model.ct
    dt = torch.bfloat16 if ct == 1 else torch.float32
    params = []

    def pairs_of(kmap):
        if id(kmap) not in tl.pairs:
            tl.pairs[id(kmap)] = [((kmap.nbr[:, k] >= 0).nonzero()[:, 0], kmap.nbr[:, k][kmap.nbr[:, k] >= 0].long()) for k in range(kmap.K)]
        return tl.pairs[id(kmap)]

    def cbr(conv, norm, x, kmap, residual=None, act=True):
        W, bn = conv.kernel, norm.bn
        params.extend([W, bn.weight, bn.bias])
        if conv.K == 1:
            z = (x.to(dt) @ W.to(dt)).float()
        else:
            z, xs = torch.zeros(kmap.n_out, conv.cout, device=x.device), x.to(dt)
            for k, (o, i) in enumerate(pairs_of(kmap)):
                if o.numel():
                    z.index_add_(0, o, (xs[i] @ W[k].to(dt)).float())
        y = F.batch_norm(z, bn.running_mean.clone(), bn.running_var.clone(), bn.weight, bn.bias, True, bn.momentum, bn.eps)
        if residual is not None:
            y = y + residual
        return torch.relu(y) if act else y

    def block(bi, x, l):
        for blk in getattr(model, f"block{bi}"):
            y = cbr(blk.conv1, blk.norm1, x, pyr.nbr3[l])
            res = cbr(blk.downsample[0], blk.downsample[1], x, None, act=False) if blk.downsample is not None else x
            x = cbr(blk.conv2, blk.norm2, y, pyr.nbr3[l], residual=res)
        return x

    x = cbr(model.conv0p1s1, model.bn0, feats.index_select(0, pyr.perm), pyr.nbr5 if model.conv0p1s1.K == 125 else pyr.nbr3[0])
    skip = [x]
    for i, name in enumerate(("conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2")):
        x = block(i + 1, cbr(getattr(model, name), getattr(model, f"bn{i + 1}"), x, pyr.down[i]), i + 1)
        skip.append(x)
    maps = [x]
    for i, name in enumerate(("convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2")):
        l = 3 - i
        x = cbr(getattr(model, name), getattr(model, f"bntr{4 + i}"), x, pyr.up[l])
        x = block(5 + i, torch.cat([x, skip[l]], 1), l)
        maps.append(x)
    maps[4] = maps[4].index_select(0, pyr.inv)
    return torch.autograd.grad(sum((m * r).sum() for m, r in zip(maps, Rs)), params)


def train_leg(a, out):
    """--train: forward + backward ms of Res16UNet34C(trainable=True).train() against the stock-torch loop under autograd, B = 1
    and 4, both compute modes; at B = 4 a per-class split of ours (KernelTimer around one step) next to the torch loop's time
    for the same class of work, measured operator by operator on the tensors of our tape (the median of --torch-iters event pairs after 3 warm-up calls around: the gather ->
    matmul -> index_add input gradient, the per-offset x^T dy weight gradient, batch_norm forward + backward through autograd)."""
    import torch.nn.functional as F
    model = sparse.Res16UNet34C(3, a.out_channels, {"bn_momentum": 0.02, "conv1_kernel_size": 5}, trainable=True)
    synth.fill_module(model, 0)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_var.copy_(m.running_var.abs() + 0.5)
    model.cuda().train()
    params = [p for n, p in model.named_parameters() if not n.startswith("final")]
    for B in (1, 4):
        coords = room_coords(B, a.V).cuda()
        feats = torch.rand(coords.shape[0], 3, device="cuda")
        pyr = sparse.CoordPyramid(coords)
        g = torch.Generator(device="cuda").manual_seed(3)
        Rs = [torch.randn(pyr.n[4 - h], c, device="cuda", generator=g) for h, c in enumerate((256, 256, 128, 96, 96))]
        res = dict(voxels=int(coords.shape[0]), level_rows=pyr.n)

        def ours():
            _o, maps = model.run(pyr, feats)
            return torch.autograd.grad(sum((m * r).sum() for m, r in zip(maps, Rs)), params)

        for compute in ("fp32", "bf16"):
            model.compute = compute
            total = events(ours, a.iters)
            tl = TorchLoop()
            torch_total = events(lambda: torch_train_step(model, pyr, feats, tl, Rs), a.torch_iters)
            go, gt = ours(), torch_train_step(model, pyr, feats, tl, Rs)
            grad_norm = float(torch.cat([x.flatten() for x in go]).norm())      # (the two steps list their parameters in different orders)
            r = dict(fwd_bwd_ms=total, torch_fwd_bwd_ms=torch_total, speedup=round(torch_total[1] / total[1], 2), grad_norm=float(f"{grad_norm:.4g}"),
                     torch_grad_norm=float(f"{float(torch.cat([x.flatten() for x in gt]).norm()):.4g}"))
            if B == 4:
                with KernelTimer() as kt:
                    ours()
                cls = {}
                for (name, key), v in kt.summary().items():
                    c = ("input_gradient" if re.search(r"w[12]$", key) else "forward_conv") if name == "pq3d_sparse_conv_fwd" else \
                        "weight_gradient" if name == "pq3d_sparse_conv_wgrad" else "batchnorm" if name.startswith("pq3d_bn_") else \
                        "1x1_gemm" if name == "pq3d_gemm" else name
                    e = cls.setdefault(c, dict(calls=0, ms=0.0))
                    e["calls"] += v["calls"]; e["ms"] += v["ms"]
                dt = torch.bfloat16 if compute == "bf16" else torch.float32
                tms = dict(input_gradient=0.0, weight_gradient=0.0, batchnorm=0.0)

                def timed(key, fn):      # the tool's method per operator: 3 warm-up calls, then the median of --torch-iters
                    tms[key] += events(fn, a.torch_iters)[1]
                for lname, (conv, norm, t) in model.training_tape(pyr, feats).items():
                    z, bn = t["z"], norm.bn
                    dy = torch.randn_like(z)

                    def bn_fb():
                        zz = z.detach().requires_grad_(True)
                        y = torch.relu(F.batch_norm(zz, bn.running_mean.clone(), bn.running_var.clone(), bn.weight, bn.bias, True, bn.momentum, bn.eps))
                        torch.autograd.grad(y, (zz, bn.weight, bn.bias), dy)
                    timed("batchnorm", bn_fb)
                    if conv.K == 1:
                        continue
                    x, W, prs = t["x"], conv.kernel.detach(), [(o, i) for o, i in tl.pairs[id(t["kmap"])] if o.numel()]
                    ks = [k for k, (o, i) in enumerate(tl.pairs[id(t["kmap"])]) if o.numel()]

                    def dx():
                        acc, d = torch.zeros(x.shape[0], x.shape[1], device="cuda"), dy.to(dt)
                        for k, (o, i) in zip(ks, prs):
                            acc.index_add_(0, i, (d[o] @ W[k].to(dt).t()).float())

                    def dw():
                        xs, d, gw = x.to(dt), dy.to(dt), torch.zeros_like(W)
                        for k, (o, i) in zip(ks, prs):
                            gw[k] = (xs[i].t() @ d[o]).float()
                    if lname != "conv0p1s1":
                        timed("input_gradient", dx)
                    timed("weight_gradient", dw)
                r["classes"] = {k: dict(calls=v["calls"], ms=round(v["ms"], 3), torch_ms=round(tms[k], 3) if k in tms else None)
                                for k, v in sorted(cls.items())}
            res[compute] = r
        out[f"train_B{B}"] = res


def class_of(n, n_out, n_in, K):
    lvl = f"s{1 << n.index(n_out)}" if n_out in n else f"n{n_out}"
    kind = {125: "stem5", 27: "conv3", 1: "1x1"}.get(K) or ("down2" if n_out < n_in else "up2")
    return f"{lvl}/{kind}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=100_000); ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--torch-iters", type=int, default=8)
    ap.add_argument("--map-iters", type=int, default=5); ap.add_argument("--out-channels", type=int, default=200)
    ap.add_argument("--train", action="store_true", help="time forward + backward of the trainable network instead")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxel_backbone.py needs a GPU"
    if a.train:
        out = dict(metric="voxel_backbone_train", V=a.V, out_channels=a.out_channels)
        train_leg(a, out)
        print(json.dumps(out))
        return
    model = sparse.Res16UNet34C(3, a.out_channels, {"bn_momentum": 0.02, "conv1_kernel_size": 5})
    synth.fill_module(model, 0)
    model.cuda()
    out = dict(metric="voxel_backbone", V=a.V, out_channels=a.out_channels)
    for B in (1, 4):
        coords = room_coords(B, a.V).cuda()
        feats = torch.rand(coords.shape[0], 3, device="cuda")
        sparse.CoordPyramid(coords)
        ts = []
        for _ in range(a.map_iters):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            pyr = sparse.CoordPyramid(coords)
            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        kmaps = pyr.nbr3 + [pyr.nbr5] + pyr.down + pyr.up
        pairs = {(km.n_out, km.n_in, km.K): int((km.nbr >= 0).sum()) for km in kmaps}      # present (row, offset) pairs per map
        res = dict(voxels=int(coords.shape[0]), level_rows=pyr.n, present_k3=[round(pairs[(km.n_out, km.n_in, 27)] / km.n_out, 1) for km in pyr.nbr3], map_ms=round(statistics.median(ts), 3))
        for compute in ("fp32", "bf16"):
            model.compute = compute
            total = events(lambda: model.run(pyr, feats), a.iters)
            with KernelTimer() as kt:
                _o, ours = model.run(pyr, feats)
            cls = {}
            for (name, key), v in kt.summary().items():
                if name == "pq3d_sparse_conv_fwd":
                    n_out, n_in, Ci, Co, K = (int(t) for t in re.match(r"No(\d+)Ni(\d+)Ci(\d+)Co(\d+)K(\d+)", key).groups())
                    v = dict(v, flops=v["calls"] * 2.0 * pairs[(n_out, n_in, K)] * Ci * Co)     # present pairs, not N_out K
                else:
                    n_out = n_in = int(re.match(r"M(\d+)", key).group(1)); K = 1
                c = cls.setdefault(class_of(pyr.n, n_out, n_in, K), dict(calls=0, ms=0.0, flops=0.0, bytes=0.0))
                for f in c:
                    c[f] += v[f]
            # baseline: the same network through stock torch ops
            tl = TorchLoop()
            real = sparse.sparse_conv, sparse.row_gemm
            sparse.sparse_conv, sparse.row_gemm = tl.conv, tl.gemm
            try:
                with torch.no_grad():
                    run_t = lambda: model._run(pyr, feats)
                    torch_total = events(run_t, a.torch_iters)
                    tl.records.clear()
                    _o, theirs = run_t()
                    torch.cuda.synchronize()
            finally:
                sparse.sparse_conv, sparse.row_gemm = real
            tcls = {}
            for (kind, n_out, n_in, K), e0, e1 in tl.records:
                k = class_of(pyr.n, n_out, n_in, K)
                tcls[k] = tcls.get(k, 0.0) + e0.elapsed_time(e1)
            diff = max(float((x - y).norm() / y.norm()) for x, y in zip(ours, theirs))
            res[compute] = dict(total_ms=total, torch_total_ms=torch_total, speedup=round(torch_total[1] / total[1], 2),
                                map_share=round(res["map_ms"] / total[1], 3), max_rel_diff=float(f"{diff:.3g}"),
                                classes={k: dict(calls=v["calls"], ms=round(v["ms"], 3), torch_ms=round(tcls.get(k, 0.0), 3),
                                                 tflops=round(v["flops"] / v["ms"] / 1e9, 2), gbs=round(v["bytes"] / v["ms"] / 1e6, 1))
                                         for k, v in sorted(cls.items())})
        out[f"B{B}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
