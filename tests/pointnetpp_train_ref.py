"""Reference for TRAINING the PointNet++ tokenizer (pq3d_amd/pointnetpp.py: PointNetPP(trainable=True)): one training step
restated in plain torch, any dtype, with torch autograd; shares no code with the package.  Built on the oracle's furthest
point sampling and ball query (oracle/pointnet2_oracle.py; integer outputs, computed from the fp32 coordinates whatever the
dtype).  tests/test_pointnetpp_train_ref.py holds it to fixture F30, which the reference's own module tree produced.

    RoundOperands / RoundGrad   bf16 emulation of a product's forward operands and of the gradient entering both backward products
    train_step                  the training-mode forward (batch-statistics BatchNorm2d, momentum 0.1, eps 1e-5, the running
                                buffers of nn.BatchNorm2d), loss = sum(out * R), every parameter gradient
"""
import numpy as np
import torch

from oracle import pointnet2_oracle as po

EPS, MOMENTUM = 1e-5, 0.1


def _bf(t):
    return t.bfloat16().to(t.dtype)


class RoundOperands(torch.autograd.Function):
    """forward: the operand rounded to bf16; backward: the gradient unchanged (the product's own gradient is what is wanted)"""
    @staticmethod
    def forward(ctx, t):
        return _bf(t)

    @staticmethod
    def backward(ctx, g):
        return g


class RoundGrad(torch.autograd.Function):
    """forward: identity; backward: the gradient rounded to bf16 -- it is an operand of both backward products"""
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def train_step(sd, pc, sa_n_points, sa_n_samples, sa_radii, R, dtype=torch.float64, bf16=False, trace=None):
    """One training step of the tokenizer on the clouds ``pc`` [M, P, 3 + C] (fp32) from the state ``sd`` ({name: tensor}, the
    module's state_dict).  Returns {name: tensor}: 'out' [M, Cout], 'grad/<parameter>' for every parameter, 'buf/<buffer>' for
    every running_mean / running_var / num_batches_tracked after the step.  ``bf16``: the operands of every product (the 1x1
    convolutions and fc; forward, input-gradient and weight-gradient products) rounded to bf16, everything else in ``dtype``.
    ``trace`` (a dict) receives the oracle's indices 'fps/<i>', 'ball/<i>' and the arg-max 'arg/<i>' [M, np, C] of every stage."""
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()
              if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var"))}
    rnd = (lambda t: RoundOperands.apply(t)) if bf16 else (lambda t: t)
    gr = (lambda t: RoundGrad.apply(t)) if bf16 else (lambda t: t)
    new = {}
    pc = pc.float()
    xyz = pc[..., :3]
    feats = pc[..., 3:].to(dtype) if pc.shape[-1] > 3 else None               # [M, N, C], channels last throughout
    M = pc.shape[0]
    for i, (npoint, nsample, radius) in enumerate(zip(sa_n_points, sa_n_samples, sa_radii)):
        if npoint is not None:
            fps = po.furthest_point_sampling(xyz.numpy(), npoint)
            new_xyz = torch.gather(xyz, 1, torch.from_numpy(fps).long().unsqueeze(-1).expand(-1, -1, 3))
            idx = po.ball_query(new_xyz.numpy(), xyz.numpy(), radius, nsample)
            if trace is not None:
                trace[f"fps/{i}"], trace[f"ball/{i}"] = fps, idx
            li = torch.from_numpy(idx).long().view(M, -1)                    # [M, np * ns]
            take = lambda t: torch.gather(t, 1, li.unsqueeze(-1).expand(-1, -1, t.shape[-1])).view(M, npoint, nsample, -1)
            x = take(xyz.to(dtype)) - new_xyz.to(dtype)[:, :, None, :]       # pointnet2_utils.py:345-347
            if feats is not None:
                x = torch.cat([x, take(feats)], -1)                          # pointnet2_utils.py:353-356
        else:
            new_xyz = None
            x = xyz.to(dtype) if feats is None else torch.cat([xyz.to(dtype), feats], -1)
            x = x[:, None]                                                   # GroupAll: [M, 1, N, 3 + C], no centring
        j = 0
        while f"encoder.{i}.mlps.0.layer{j}.conv.weight" in params:
            k = f"encoder.{i}.mlps.0.layer{j}."
            z = gr(rnd(x) @ rnd(params[k + "conv.weight"][:, :, 0, 0]).t())
            n = z.shape[0] * z.shape[1] * z.shape[2]
            mean, var = z.mean((0, 1, 2)), z.var((0, 1, 2), unbiased=False)
            with torch.no_grad():
                unb = var * (n / (n - 1)) if n > 1 else var
                new[k + "bn.bn.running_mean"] = (1 - MOMENTUM) * sd[k + "bn.bn.running_mean"].to(dtype) + MOMENTUM * mean
                new[k + "bn.bn.running_var"] = (1 - MOMENTUM) * sd[k + "bn.bn.running_var"].to(dtype) + MOMENTUM * unb
                new[k + "bn.bn.num_batches_tracked"] = sd[k + "bn.bn.num_batches_tracked"] + 1
            x = torch.relu((z - mean) / torch.sqrt(var + EPS) * params[k + "bn.bn.weight"] + params[k + "bn.bn.bias"])
            j += 1
        feats = x.max(2).values                                              # [M, np, C]: pointnet2_modules.py:62-65
        if trace is not None:                                                # the FIRST maximum, as F.max_pool2d takes it
            trace[f"arg/{i}"] = np.argmax(x.detach().numpy() == feats.detach().numpy()[:, :, None, :], axis=2)
        xyz = new_xyz
    flat = feats.transpose(1, 2).reshape(M, -1)                              # (C, npoint) order: pointnet.py:63
    out = gr(rnd(flat) @ rnd(params["fc.weight"]).t()) + params["fc.bias"]
    names = sorted(params)
    grads = torch.autograd.grad((out * R.to(dtype)).sum(), [params[k] for k in names])
    res = {"out": out.detach()}
    res.update({f"grad/{k}": g for k, g in zip(names, grads)})
    res.update({f"buf/{k}": v for k, v in new.items()})
    return res
