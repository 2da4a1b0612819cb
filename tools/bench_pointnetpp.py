"""Frozen PointNet++ tokenizer (object_encoder.py:22-28) on M object clouds of P points: the row-GEMM HIP path
(pq3d_amd/pointnetpp.py) vs the reference's channel-first layout (1x1 Conv2d + BatchNorm2d + max_pool2d on stock
PyTorch-ROCm, fed by the same HIP point-set operators).  Usage: python tools/bench_pointnetpp.py [--clouds 640] [--points 1024]

--train: one TRAINING step (forward + backward, batch-statistics BatchNorm) of PointNetPP(trainable=True) against the same
network in stock torch on the same GPU -- gather + nn.Conv2d + nn.BatchNorm2d + max_pool2d on this package's FPS and ball-query
indices, with torch autograd.  Median ms of 20 steps per leg, the peak memory of a step, and how far the gradients are apart."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pq3d_amd import pointnet2 as P2, synth  # noqa: E402
from pq3d_amd.pointnetpp import POINTNETPP_TOKENIZER, PointNetPP  # noqa: E402


def channel_first_forward(net, pc):
    """pointnet2_modules.py:23-70 verbatim in structure, torch layers on [B, C, npoint, nsample]."""
    xyz, feats = pc[..., :3].contiguous(), pc[..., 3:].transpose(1, 2).contiguous()
    for sa in net.encoder:
        if sa.npoint is not None:
            new_xyz = P2.gather_operation(xyz.transpose(1, 2).contiguous(), P2.furthest_point_sample(xyz, sa.npoint)).transpose(1, 2).contiguous()
            x = P2.QueryAndGroup(sa.radius, sa.nsample)(xyz, new_xyz, feats)
        else:
            new_xyz = None
            x = P2.GroupAll()(xyz, None, feats)
        for layer in sa.mlps[0]:
            bn = layer.bn.bn
            x = F.relu(F.batch_norm(F.conv2d(x, layer.conv.weight), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))
        feats = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)
        xyz = new_xyz
    return net.fc(feats.view(feats.size(0), -1))


def stock_modules(net):
    """The SharedMLPs and fc as stock torch modules (nn.Conv2d 1x1 without bias, nn.BatchNorm2d, nn.Linear) holding copies of
    ``net``'s parameters and buffers."""
    import copy
    stages = torch.nn.ModuleList()
    for sa in net.encoder:
        seq = []
        for layer in sa.mlps[0]:
            seq += [copy.deepcopy(layer.conv), copy.deepcopy(layer.bn.bn), torch.nn.ReLU(inplace=True)]
        stages.append(torch.nn.Sequential(*seq))
    return stages, copy.deepcopy(net.fc)


def stock_train_forward(net, stages, fc, pc):
    """pointnet2_modules.py:23-70 in structure: torch gathers on this package's indices, channel-first torch layers, autograd."""
    xyz, feats = pc[..., :3].contiguous(), pc[..., 3:].transpose(1, 2).contiguous()
    M = pc.shape[0]
    for sa, mlp in zip(net.encoder, stages):
        if sa.npoint is not None:
            fps = P2.furthest_point_sample(xyz, sa.npoint)
            new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
            li = P2.ball_query(sa.radius, sa.nsample, xyz, new_xyz).long().view(M, 1, -1)
            gx = torch.gather(xyz.transpose(1, 2), 2, li.expand(-1, 3, -1)).view(M, 3, sa.npoint, sa.nsample)
            gx = gx - new_xyz.transpose(1, 2).unsqueeze(-1)
            gf = torch.gather(feats, 2, li.expand(-1, feats.shape[1], -1)).view(M, feats.shape[1], sa.npoint, sa.nsample)
            x = torch.cat([gx, gf], 1)
        else:
            new_xyz = None
            x = torch.cat([xyz.transpose(1, 2), feats], 1).unsqueeze(2)
        x = mlp(x)
        feats = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)
        xyz = new_xyz
    return fc(feats.view(M, -1))


def median_ms(fn, iters):
    fn(); fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(sorted(ts)[len(ts) // 2], 3)


def train_bench(a):
    spec = {k: [list(x) if isinstance(x, list) else x for x in v] for k, v in POINTNETPP_TOKENIZER.items()}
    net = PointNetPP(**spec, trainable=True)
    synth.fill_module(net, 0)
    net.cuda().train()
    stages, fc = stock_modules(net)
    stages.cuda().train(); fc.cuda()
    pc = synth.pointcloud_inputs(a.clouds, a.points).cuda()
    R = torch.randn(a.clouds, spec["sa_mlps"][-1][-1], generator=torch.Generator().manual_seed(3)).cuda()
    ours, theirs = list(net.parameters()), list(stages.parameters()) + list(fc.parameters())
    out = {"workload": f"PointNet++ tokenizer TRAINING step (forward + backward), {a.clouds} clouds x {a.points} points x 6",
           "data": "synthetic", "timing": f"median of {a.iters} steps, ms"}

    def step(fwd, params):
        return torch.autograd.grad((fwd() * R).sum(), params)

    ref = step(lambda: stock_train_forward(net, stages, fc, pc), theirs)
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out["stock_torch_fp32_ms"] = median_ms(lambda: step(lambda: stock_train_forward(net, stages, fc, pc), theirs), a.iters)
    out["stock_torch_fp32_peak_step_GB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)
    cat = lambda gs: torch.cat([g.flatten() for g in gs])
    for compute in ("fp32", "bf16"):
        net.compute = compute
        got = step(lambda: net(pc), ours)
        out[f"hip_rows_{compute}_grad_rel_l2_vs_stock"] = float((cat(got) - cat(ref)).norm() / cat(ref).norm())
        del got
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out[f"hip_rows_{compute}_ms"] = median_ms(lambda: step(lambda: net(pc), ours), a.iters)
        out[f"hip_rows_{compute}_peak_step_GB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)
        out[f"hip_rows_{compute}_forward_only_ms"] = median_ms(lambda: net(pc), a.iters)
    print(json.dumps(out))


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / iters * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=640)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=None, help="default 10; 20 with --train")
    ap.add_argument("--train", action="store_true", help="time one training step against stock torch with autograd")
    a = ap.parse_args()
    a.iters = a.iters or (20 if a.train else 10)
    if a.train:
        return train_bench(a)
    net = PointNetPP(**{k: [list(x) if isinstance(x, list) else x for x in v] for k, v in POINTNETPP_TOKENIZER.items()})
    synth.fill_module(net, 0)
    net.cuda().eval().requires_grad_(False)
    pc = synth.pointcloud_inputs(a.clouds, a.points).cuda()
    out = {"workload": f"PointNet++ tokenizer, {a.clouds} clouds x {a.points} points x 6", "data": "synthetic"}
    with torch.no_grad():
        ref = channel_first_forward(net, pc)
        out["channel_first_torch_fp32_ms"] = timeit(lambda: channel_first_forward(net, pc), a.iters)
        for compute in ("fp32", "bf16"):
            net.compute = compute
            got = net(pc)
            out[f"hip_rows_{compute}_ms"] = timeit(lambda: net(pc), a.iters)
            out[f"hip_rows_{compute}_max_rel_err_vs_channel_first"] = float((got - ref).abs().max() / ref.abs().max())
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            net(pc); s.synchronize()
            with torch.cuda.graph(g, stream=s):
                net(pc)
        out["hip_rows_bf16_graph_ms"] = timeit(g.replay, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
