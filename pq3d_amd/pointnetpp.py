"""The frozen PointNet++ point-cloud tokenizer: ``PointNetPP`` of modules/layers/pointnet.py:22-63 as
``ObjectEncoder(backbone='pointnet++', freeze_backbone=True)`` runs it (modules/vision/object_encoder.py:22-28,63-69;
configs/unified_tasks_sceneverse.yaml:144-152) -- three set-abstraction stages (pointnet2_modules.py:23-70) and a Linear.

MI355X design (not the reference's channel-first conv stack): every (cloud, centre, sample) is one channels-last ROW.
Per stage: furthest-point sampling and ball query (pq3d_amd/pointnet2.py kernels), ``pq3d_group_rows`` writes the
centred-xyz + feature rows straight from the ball-query indices, the SharedMLP's 1x1 Conv2d + BatchNorm2d(eval) + ReLU
layers run as row GEMMs with the frozen BatchNorm folded into weight and bias (bias + ReLU in the GEMM epilogue, bf16 or
exact-fp32 MFMA), and ``pq3d_group_maxpool`` takes the max over the samples, which IS the next stage's feature-row
layout -- no transposes anywhere.  By default inference only: batch-statistics BatchNorm / training the backbone raises.

``PointNetPP(trainable=True)`` in training mode runs the same stage walk with fp32 rows and, per layer, a raw-weight
row GEMM -> ``pq3d_bn_stats`` (which also moves the running buffers) -> ``pq3d_bn_apply`` with ReLU; a stage's last layer is
``pq3d_bn_relu_maxpool`` instead (max and arg-max over the samples, the normalised rows never written).  The whole network is
ONE autograd node: the forward fills a tape per layer (input rows, raw z, mean, rstd, the activation of the non-pooled layers),
the backward walks it in reverse -- ``pq3d_bn_pool_bwd_*`` / ``pq3d_bn_bwd_*``, the two gradient GEMMs per layer (weight
gradients over row chunks summed in chunk order: no atomics), ``pq3d_group_rows_bwd`` between stages.  Statistics are over all
rows of the call, so a training forward is one pass (no ``CHUNK``); xyz takes no gradient.

Parameter names and shapes are the reference's (``encoder.{i}.mlps.0.layer{j}.conv.weight`` [Cout,Cin,1,1],
``...layer{j}.bn.bn.{weight,bias,running_mean,running_var}``, ``fc.*``), so ``pointnet_tokenizer.pth`` loads unchanged.
No CPU fallback."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from . import pointnet2 as P2
from . import sparse as S


def group_rows(xyz, new_xyz, feats, feat_channels: int, idx, np_: int, ns: int, out_dtype) -> torch.Tensor:
    """rows [B*np*ns, Kp] (Kp = 3 + C rounded up to 8): see pq3d_group_rows.  ``feats`` may be a strided row view
    [B, N, >=C] (e.g. the colour columns of an xyz+rgb cloud)."""
    B, N, _ = xyz.shape
    Kp = (3 + feat_channels + 7) // 8 * 8
    out = torch.empty(B * np_ * ns, Kp, dtype=out_dtype, device=xyz.device)
    fs = 0
    if feat_channels:
        assert feats.stride(-1) == 1 and feats.stride(0) == N * feats.stride(1)
        fs = feats.stride(1)
    L.call("pq3d_group_rows", xyz, new_xyz, feats if feat_channels else None, L.dt_of(feats) if feat_channels else 0, fs, idx, out,
           L.dt_of(out), B, N, feat_channels, np_, ns, Kp)
    return out


def group_maxpool(rows, G: int, ns: int) -> torch.Tensor:
    C = rows.shape[-1]
    out = torch.empty(G, C, dtype=rows.dtype, device=rows.device)
    L.call("pq3d_group_maxpool", rows, out, L.dt_of(rows), G, ns, C)
    return out


def bn_relu_maxpool(z, G: int, ns: int, mean, rstd, weight, bias):
    """(pooled [G, C] fp32, arg [G, C] int32) of the raw rows ``z`` [G * ns, C] (rows may be strided): max over the samples of
    relu(batch norm) and the first sample attaining it (pq3d_bn_relu_maxpool)."""
    C = z.shape[1]
    assert z.dtype == torch.float32 and z.dim() == 2 and z.shape[0] == G * ns and z.stride(1) == 1
    pooled = torch.empty(G, C, dtype=torch.float32, device=z.device)
    arg = torch.empty(G, C, dtype=torch.int32, device=z.device)
    L.call("pq3d_bn_relu_maxpool", z, z.stride(0), G, ns, C, mean, rstd, weight, bias, pooled, arg,
           work=(f"G{G}ns{ns}C{C}", 5.0 * G * ns * C, 4.0 * G * ns * C))
    return pooled, arg


def bn_pool_bwd(gp, pooled, arg, z, G: int, ns: int, mean, rstd, weight):
    """(dz [G * ns, C], dweight [C], dbias [C]): BatchNorm backward of the pooled layer from the pooled gradient ``gp`` [G, C];
    the row gradient (gp at the arg-max row of a positive maximum, 0 elsewhere) is never formed."""
    C = z.shape[1]
    assert gp.dtype == torch.float32 and gp.shape == (G, C) and gp.is_contiguous() and pooled.shape == (G, C) and arg.shape == (G, C)
    assert z.dtype == torch.float32 and z.shape[0] == G * ns and z.stride(1) == 1
    dg, db = torch.empty(C, dtype=torch.float32, device=z.device), torch.empty(C, dtype=torch.float32, device=z.device)
    L.call("pq3d_bn_pool_bwd_reduce", gp, pooled, arg, z, z.stride(0), G, ns, C, mean, rstd, dg, db, S._bn_part(G * ns, C, z.device),
           work=(f"G{G}ns{ns}C{C}", 5.0 * G * ns * C, 4.0 * G * ns * C))
    dz = torch.empty(G * ns, C, dtype=torch.float32, device=z.device)
    L.call("pq3d_bn_pool_bwd_apply", gp, pooled, arg, z, z.stride(0), G, ns, C, mean, rstd, weight, dg, db, dz, C,
           work=(f"G{G}ns{ns}C{C}", 8.0 * G * ns * C, 8.0 * G * ns * C))
    return dz, dg, db


GROUP_BWD_MAX_POINTS, GROUP_BWD_MAX_ENTRIES = L.H.PQ3D_GROUP_BWD_MAX_POINTS, L.H.PQ3D_GROUP_BWD_MAX_ENTRIES


def group_rows_bwd(drows, C: int, idx, B: int, N: int, np_: int, ns: int, col_off: int = 3) -> torch.Tensor:
    """dfeats [B, N, C]: the gradient of ``group_rows`` with respect to the point features from the row gradient ``drows``
    [B * np * ns, >= col_off + C] -- every point's entries added in increasing (centre, sample) order (pq3d_group_rows_bwd).
    ``idx`` None: GroupAll."""
    assert drows.dtype == torch.float32 and drows.dim() == 2 and drows.shape[0] == B * np_ * ns and drows.stride(1) == 1
    assert idx is None or (idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == B * np_ * ns)
    out = torch.empty(B, N, C, dtype=torch.float32, device=drows.device)
    L.call("pq3d_group_rows_bwd", drows, drows.stride(0), col_off, idx, out, C, B, N, C, np_, ns)
    return out


def _row_wgrad(dz, x, ct: int) -> torch.Tensor:
    """dz.T @ x, [Cout, K] fp32, of two row matrices: the rows are cut into S equal chunks (one batched GEMM, one writer per
    element) whose slabs are added in chunk order -- no split-K atomics, the same bits run to run.  S depends on the row count
    only."""
    R, Co = dz.shape
    K = x.shape[1]
    S_ = 1
    while S_ < 64 and R % (2 * S_) == 0 and R // (2 * S_) >= 2048:
        S_ *= 2
    rows = R // S_
    ws = torch.empty(S_, Co, K, dtype=torch.float32, device=dz.device)
    L.gemm(M=Co, N=K, K=rows, A=[dz], B=[x], Cs=[ws], ct=ct, lda=dz.stride(0), ldb=x.stride(0), ldc=K, transA=True, transB=True,
           batch=S_, strideA=rows * dz.stride(0), strideB=rows * x.stride(0), strideC=Co * K)
    return ws[0] if S_ == 1 else ops.sum_n(list(ws.unbind(0)))


class _PointNetTrain(torch.autograd.Function):
    """PointNetPP's training forward and backward as ONE autograd node: inputs are every conv.weight / bn.weight / bn.bias in
    stage and layer order, then fc.weight and fc.bias; the output is the token.  The tape holds no output of the node."""

    @staticmethod
    def forward(ctx, net, pc, *params):
        ctx.net, ctx.tape = net, []
        return net._train_forward(pc, ctx.tape)

    @staticmethod
    def backward(ctx, g):
        return (None, None, *ctx.net._train_backward(ctx.tape, g.float().contiguous()))


# ------------------------------------------------------------------------------------------------ parameter containers
class _BN(nn.Sequential):
    """pytorch_utils.py:39-63 (_BNBase / BatchNorm2d): child ``bn``."""

    def __init__(self, c):
        super().__init__()
        self.add_module("bn", nn.BatchNorm2d(c))


class _ConvBN(nn.Sequential):
    """pytorch_utils.py:67-190 (Conv2d = 1x1 conv [+ BatchNorm2d] + ReLU, post-activation order)."""

    def __init__(self, cin, cout, bn):
        super().__init__()
        conv = nn.Conv2d(cin, cout, kernel_size=1, bias=not bn)
        nn.init.kaiming_normal_(conv.weight)
        if conv.bias is not None:
            nn.init.constant_(conv.bias, 0)
        self.add_module("conv", conv)
        if bn:
            self.add_module("bn", _BN(cout))


class SharedMLP(nn.Sequential):
    """pytorch_utils.py:11-36."""

    def __init__(self, spec: List[int], bn: bool = True):
        super().__init__()
        for i in range(len(spec) - 1):
            self.add_module(f"layer{i}", _ConvBN(spec[i], spec[i + 1], bn))


class PointnetSAModule(nn.Module):
    """pointnet2_modules.py:125-158 (single-scale set abstraction; npoint=None groups all points)."""

    def __init__(self, *, mlp: List[int], npoint: Optional[int] = None, radius: Optional[float] = None,
                 nsample: Optional[int] = None, bn: bool = True, use_xyz: bool = True):
        super().__init__()
        if not use_xyz:
            raise NotImplementedError("use_xyz=False is not used by the reference's point encoder")
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        spec = list(mlp)
        spec[0] += 3                         # pointnet2_modules.py:119-120
        self.groupers = nn.ModuleList()      # parameter-free in the reference; kept for module-tree parity
        self.mlps = nn.ModuleList([SharedMLP(spec, bn=bn)])


class PointNetPP(nn.Module):
    """modules/layers/pointnet.py:22-63.  forward(features [M, P, 3 + C]) -> [M, sa_mlps[-1][-1]]."""

    CHUNK = 2048   # clouds per pass (bounds the row buffers: ~0.4 MB of bf16 rows per cloud at the shipped sizes)

    def __init__(self, sa_n_points: list, sa_n_samples: list, sa_radii: list, sa_mlps: list, bn=True, use_xyz=True,
                 trainable: bool = False):
        super().__init__()
        if trainable and not bn:
            raise NotImplementedError("PointNetPP(trainable=True) trains the BatchNorm network only (bn=True)")
        self.trainable = bool(trainable)
        n_sa = len(sa_n_points)
        if not (n_sa == len(sa_n_samples) == len(sa_radii) == len(sa_mlps)):
            raise ValueError("Lens of given hyper-params are not compatible")
        self.encoder = nn.ModuleList(PointnetSAModule(npoint=sa_n_points[i], nsample=sa_n_samples[i], radius=sa_radii[i],
                                                      mlp=sa_mlps[i], bn=bn, use_xyz=use_xyz) for i in range(n_sa))
        out_n_points = sa_n_points[-1] if sa_n_points[-1] is not None else 1
        self.fc = nn.Linear(out_n_points * sa_mlps[-1][-1], sa_mlps[-1][-1])
        self.compute = "bf16"
        self._folded = {}

    @property
    def ct(self) -> int:
        return ops.BF16 if self.compute == "bf16" else ops.F32

    def _fold(self, layer: _ConvBN):
        """Frozen BatchNorm folded into the 1x1 conv: W' = W * g/sqrt(var+eps) (K zero-padded to 8), b' = beta - mean*s
        (+ s*conv.bias).  Cached against the tensors' version counters, so load_state_dict / in-place edits refold.  A trainable
        network folds afresh every time: an optimizer that writes the parameters' storage (TrainStep's flat AdamW) bumps no
        version counter."""
        conv = layer.conv
        bn = layer.bn.bn if hasattr(layer, "bn") else None
        src = [conv.weight] + ([conv.bias] if conv.bias is not None else []) + \
              ([bn.weight, bn.bias, bn.running_mean, bn.running_var] if bn is not None else [])
        key = tuple((t.data_ptr(), t._version) for t in src) + (self.ct,)
        hit = self._folded.get(id(layer))
        if hit is not None and hit[0] == key and not self.trainable:
            return hit[1], hit[2]
        W = conv.weight.detach()[:, :, 0, 0].float()
        b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(W.shape[0], device=W.device)
        if bn is not None:
            s = bn.weight.detach().float() * torch.rsqrt(bn.running_var.float() + bn.eps)
            W, b = W * s[:, None], bn.bias.detach().float() + (b - bn.running_mean.float()) * s
        Kp = (W.shape[1] + 7) // 8 * 8
        Wp = torch.zeros(W.shape[0], Kp, device=W.device)
        Wp[:, :W.shape[1]] = W
        Wp = Wp.contiguous()
        if self.ct == ops.BF16:   # rounded once here instead of by every row tile (and eligible for the 128x128-tile GEMM)
            Wp = Wp.to(torch.bfloat16)
        if not self.trainable:
            self._folded[id(layer)] = (key, Wp, b.contiguous())
        return Wp, b.contiguous()

    def _mlp(self, rows, mlp: SharedMLP):
        ct, ad = self.ct, ops.act_dtype(self.ct)
        for layer in mlp:
            W, b = self._fold(layer)
            rows = ops.linear(rows, W, b, ct=ct, act="relu", out_dtype=ad)
        return rows

    def _walk(self, pc, rows_dtype, stage):
        """The network's graph, for both modes: the flattened [M, C * npoint] input of ``fc``.
        ``stage(sa, rows, G, ns, grouping)`` runs one stage's SharedMLP and pooling on its grouped rows [G * ns, Kp] and returns the
        pooled features [G, Cout]; ``grouping``: what the rows were built from (idx, N, C, np, ns)."""
        M, N, D = pc.shape
        xyz = pc[..., 0:3].contiguous()
        feats, C = (pc[..., 3:], D - 3) if D > 3 else (None, 0)          # a strided view: rows are read in place
        for sa in self.encoder:
            if sa.npoint is not None:
                fps = P2.furthest_point_sample(xyz, sa.npoint)                                   # [M, np] int32
                new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
                idx = P2.ball_query(sa.radius, sa.nsample, xyz, new_xyz)                        # [M, np, ns]
                np_, ns = sa.npoint, sa.nsample
                rows = group_rows(xyz, new_xyz, feats, C, idx, np_, ns, rows_dtype)
            else:                                                                              # GroupAll: no centring
                np_, ns, new_xyz, idx = 1, N, None, None
                rows = group_rows(xyz, None, feats, C, None, 1, N, rows_dtype)
            pooled = stage(sa, rows, M * np_, ns, dict(idx=idx, N=N, C=C, np=np_, ns=ns))
            C = pooled.shape[-1]
            feats = pooled.view(M, np_, C)
            xyz, N = new_xyz, np_
        return feats.transpose(1, 2).reshape(M, -1) if feats.shape[1] > 1 else feats.reshape(M, -1)   # (C, npoint) order

    def _forward_chunk(self, pc):
        flat = self._walk(pc, ops.act_dtype(self.ct), lambda sa, rows, G, ns, _grouping: group_maxpool(self._mlp(rows, sa.mlps[0]), G, ns))
        return ops.linear(flat, self.fc.weight, self.fc.bias, ct=self.ct)

    # ---- training: batch-statistics BatchNorm, one autograd node for the whole network
    def _train_params(self):
        """Every trained parameter in the order of the training node's inputs and gradients."""
        ps = [p for sa in self.encoder for layer in sa.mlps[0] for p in (layer.conv.weight, layer.bn.bn.weight, layer.bn.bn.bias)]
        return ps + [self.fc.weight, self.fc.bias]

    def _train_forward(self, pc, tape):
        """Per layer: raw-weight row GEMM -> batch statistics (running buffers updated on the device) -> normalise + ReLU, the last
        layer of a stage pooled instead; then fc.  ``tape`` receives one record per stage (its grouping, per layer the input rows,
        the zero-padded weight, z, mean, rstd and the activation of the non-pooled layers, the pooled maximum and its arg-max)
        and one for fc."""
        ct = self.ct

        def stage(sa, rows, G, ns, grouping):
            layers, x, recs = list(sa.mlps[0]), rows, []
            for j, layer in enumerate(layers):
                bn = layer.bn.bn
                assert bn.momentum is not None and bn.affine and bn.track_running_stats
                W = layer.conv.weight.detach()
                Cout, Cin = W.shape[0], W.shape[1]
                W, Kp = W.view(Cout, Cin), x.shape[1]
                if Kp != Cin:                       # a stage's first layer: K = 3 + C, zero-padded to 8 as group_rows pads the rows
                    W = torch.cat([W, W.new_zeros(Cout, Kp - Cin)], 1)
                z = torch.empty(x.shape[0], Cout, dtype=torch.float32, device=x.device)
                L.gemm(M=x.shape[0], N=Cout, K=Kp, A=[x], B=[W], Cs=[z], ct=ct, lda=x.stride(0), ldb=Kp, ldc=Cout)
                mean, rstd = S.bn_stats(z, bn.eps, bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked)
                rec = dict(x=x, W=W, cin=Cin, z=z, mean=mean, rstd=rstd, y=None)
                recs.append(rec)
                if j == len(layers) - 1:
                    pooled, arg = bn_relu_maxpool(z, G, ns, mean, rstd, bn.weight.detach(), bn.bias.detach())
                else:
                    x = rec["y"] = S.bn_apply(z, mean, rstd, bn.weight.detach(), bn.bias.detach(), act="relu")
            tape.append(dict(grouping, sa=sa, G=G, layers=recs, pooled=pooled, arg=arg))
            return pooled

        flat = self._walk(pc, torch.float32, stage).contiguous()
        M, Kf = flat.shape
        Co = self.fc.weight.shape[0]
        out = torch.empty(M, Co, dtype=torch.float32, device=flat.device)
        L.gemm(M=M, N=Co, K=Kf, A=[flat], B=[self.fc.weight.detach()], bias=[self.fc.bias.detach()], Cs=[out], ct=ct, lda=Kf, ldb=Kf,
               ldc=Co)
        tape.append(dict(flat=flat, M=M))
        return out

    def _train_backward(self, tape, g):
        """The tape walked in reverse; returns the gradients in ``_train_params`` order."""
        ct = self.ct
        fc, stages = tape[-1], tape[:-1]
        flat, M = fc["flat"], fc["M"]
        W = self.fc.weight.detach()
        Co, Kf = W.shape
        d = torch.empty(M, Kf, dtype=torch.float32, device=g.device)
        L.gemm(M=M, N=Kf, K=Co, A=[g], B=[W], Cs=[d], ct=ct, lda=Co, ldb=Kf, ldc=Kf, transB=True)
        tail = [_row_wgrad(g, flat, ct), ops.colsum(g)]
        last = stages[-1]
        if last["np"] > 1:                          # fc read the pooled features in (C, npoint) order
            d = d.view(M, -1, last["np"]).transpose(1, 2).contiguous()
        gp = d.view(last["G"], -1)
        grads = []
        for i in range(len(stages) - 1, -1, -1):
            st = stages[i]
            recs, per = st["layers"], []
            for j in range(len(recs) - 1, -1, -1):
                t, bn = recs[j], st["sa"].mlps[0][j].bn.bn
                if j == len(recs) - 1:
                    dz, dg, db = bn_pool_bwd(gp, st["pooled"], st["arg"], t["z"], st["G"], st["ns"], t["mean"], t["rstd"], bn.weight.detach())
                else:
                    dg, db = S.bn_bwd_reduce(d, t["z"], t["mean"], t["rstd"], y=t["y"])
                    dz = S.bn_bwd_apply(d, t["z"], t["mean"], t["rstd"], bn.weight.detach(), dg, db, y=t["y"])
                dW = _row_wgrad(dz, t["x"], ct)[:, :t["cin"]].reshape(dz.shape[1], t["cin"], 1, 1)     # the padded columns are dropped
                per.append([dW, dg, db])
                if j > 0 or i > 0:                  # the first stage's rows are data
                    Cout, Kp = t["W"].shape
                    d = torch.empty(dz.shape[0], Kp, dtype=torch.float32, device=g.device)
                    L.gemm(M=dz.shape[0], N=Kp, K=Cout, A=[dz], B=[t["W"]], Cs=[d], ct=ct, lda=Cout, ldb=Kp, ldc=Kp, transB=True)
            grads = [x for layer in reversed(per) for x in layer] + grads
            if i > 0:
                gp = group_rows_bwd(d, st["C"], st["idx"], M, st["N"], st["np"], st["ns"]).view(M * st["N"], st["C"])
        return grads + tail

    def forward(self, features):
        bn_training = [m.training for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        if self.trainable and self.training:
            if not all(bn_training):
                raise NotImplementedError("a training-mode PointNetPP(trainable=True) runs every BatchNorm on batch statistics: "
                                          "a BatchNorm left in eval mode inside it is not provided")
            if not features.is_cuda:
                raise RuntimeError("pq3d_amd PointNetPP needs a HIP device tensor (no CPU fallback)")
            # one pass over all clouds: the statistics are over every row of the call (no CHUNK)
            return _PointNetTrain.apply(self, features.detach().contiguous().float(), *self._train_params())
        if any(bn_training):
            raise NotImplementedError("PointNetPP on the HIP kernels is the FROZEN tokenizer (BatchNorm in eval mode, "
                                      "ObjectEncoder(freeze_backbone=True)); batch-statistics BatchNorm is not provided")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("training the PointNet++ backbone is not provided: call under torch.no_grad() "
                                      "(freeze_backbone=True) or set requires_grad_(False)")
        if not features.is_cuda:
            raise RuntimeError("pq3d_amd PointNetPP needs a HIP device tensor (no CPU fallback)")
        pc = features.detach().contiguous().float()
        with torch.no_grad():
            outs = [self._forward_chunk(pc[i:i + self.CHUNK]) for i in range(0, pc.shape[0], self.CHUNK)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


POINTNETPP_TOKENIZER = dict(sa_n_points=[32, 16, None], sa_n_samples=[32, 32, None], sa_radii=[0.2, 0.4, None],
                            sa_mlps=[[3, 64, 64, 128], [128, 128, 128, 256], [256, 256, 512, 768]])   # object_encoder.py:23-28
