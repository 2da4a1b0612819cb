#!/usr/bin/env python3
"""Generate F30_pointnetpp_train.npz: ONE TRAINING STEP of the reference's PointNet++ tokenizer (runs where the reference is
present; never imported by the product).

    python tests/golden/make_golden_pointnetpp_train.py [--out PATH]

The module tree, the SharedMLP stacks (Conv2d 1x1 -> BatchNorm2d -> ReLU), F.max_pool2d and fc ARE the reference's own
objects (modules/layers/pointnet.py:22-63, imported with make_golden.py's recipe), in train mode, float64, torch autograd on
the CPU.  The CUDA-only point-set operators in between (furthest_point_sample, ball_query, grouping_operation) cannot run
there and are supplied by oracle/pointnet2_oracle.py, as make_golden.run_pointnetpp_case does; their index outputs are stored
under ``oracle/`` to say so.  A small spec keeps the file small; weights are NOT stored (regenerated from ``pq3d_amd.synth``,
a checksum detects RNG drift).

Stored: pc [6, 64, 6] fp32, R [6, 80] (loss = sum(out * R)), out, grad/<parameter> for every parameter,
buf/<buffer> for every running_mean / running_var / num_batches_tracked after the step (all float64 / int64),
oracle/fps/<i>, oracle/ball/<i>, meta/{args, keys, weights_checksum}.
"""
from __future__ import annotations

import argparse
import builtins
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pq3d_amd import synth  # noqa: E402

OUT = os.path.join(HERE, "F30_pointnetpp_train.npz")
SPEC = dict(sa_n_points=[8, 4, None], sa_n_samples=[8, 8, None], sa_radii=[0.2, 0.4, None],
            sa_mlps=[[3, 16, 16, 32], [32, 32, 32, 64], [64, 64, 96, 80]])
SEED, DATA_SEED, CLOUDS, POINTS = 13, 33, 6, 64


def load_make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


def inputs():
    """synth.pointcloud_inputs' data with two clouds squeezed (a slab and a rod), so that radius-0.2 balls over 64 points are
    both short of nsample and full."""
    pc = synth.pointcloud_inputs(CLOUDS, POINTS, 3, DATA_SEED)
    pc[1, :, 1:3] *= 0.1
    R = torch.from_numpy(np.random.default_rng(DATA_SEED + 1).standard_normal((CLOUDS, SPEC["sa_mlps"][-1][-1])))
    return pc, R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    load_make_golden().import_reference()
    builtins.__POINTNET2_SETUP__ = True
    pn = importlib.import_module("modules.layers.pointnet")
    from oracle import pointnet2_oracle as po
    torch.manual_seed(0)
    net = pn.PointNetPP(**{k: [list(x) if isinstance(x, list) else x for x in v] for k, v in SPEC.items()})
    sd = synth.fill_module(net, SEED)
    net.double().train()
    pc, R = inputs()
    out = {"meta/weights_checksum": np.float64(synth.state_checksum(sd)),
           "meta/args": np.array(repr(dict(seed=SEED, data_seed=DATA_SEED, spec=SPEC))),
           "meta/keys": np.array(repr([(k, tuple(v.shape)) for k, v in net.state_dict().items()])),
           "pc": pc.numpy(), "R": R.numpy()}
    xyz32, feats = pn.break_up_pc(pc)
    feats = feats.double()
    for i, sa in enumerate(net.encoder):
        xyz = xyz32.double()
        if sa.npoint is not None:
            fps = po.furthest_point_sampling(xyz32.numpy(), sa.npoint)
            new_xyz32 = torch.gather(xyz32, 1, torch.from_numpy(fps).long().unsqueeze(-1).expand(-1, -1, 3))
            idx = po.ball_query(new_xyz32.numpy(), xyz32.numpy(), SPEC["sa_radii"][i], SPEC["sa_n_samples"][i])
            out[f"oracle/fps/{i}"], out[f"oracle/ball/{i}"] = fps, idx
            B_, np_, ns_ = idx.shape
            li = torch.from_numpy(idx).long().view(B_, 1, -1)
            gx = torch.gather(xyz.transpose(1, 2), 2, li.expand(-1, 3, -1)).view(B_, 3, np_, ns_)
            gx = gx - new_xyz32.double().transpose(1, 2).unsqueeze(-1)               # pointnet2_utils.py:345-347
            gf = torch.gather(feats, 2, li.expand(-1, feats.shape[1], -1)).view(B_, feats.shape[1], np_, ns_)
            new_features = torch.cat([gx, gf], dim=1)                                # pointnet2_utils.py:353-356
        else:
            new_xyz32 = None
            new_features = sa.groupers[0](xyz, None, feats)                          # the reference's GroupAll (pure torch)
        new_features = sa.mlps[0](new_features)                                       # the reference's SharedMLP, train mode
        feats = torch.nn.functional.max_pool2d(new_features, kernel_size=[1, new_features.size(3)]).squeeze(-1)
        xyz32 = new_xyz32
    y = net.fc(feats.view(feats.size(0), -1))
    (y * R).sum().backward()
    out["out"] = y.detach().numpy()
    for k, p in net.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    for k, b in net.named_buffers():
        out["buf/" + k] = b.numpy()
    ball = out["oracle/ball/0"]
    assert (ball[:, :, -1] == ball[:, :, 0]).any() and (ball[:, :, -1] != ball[:, :, 0]).any(), "want short and full balls"
    np.savez_compressed(args.out, **out)
    print(f"{os.path.basename(args.out)}: {os.path.getsize(args.out) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
