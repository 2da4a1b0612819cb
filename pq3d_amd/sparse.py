"""Sparse-convolution voxel backbone on the HIP kernels: coordinate pyramid, kernel maps and Res16UNet34C (frozen, forward only).

Reference: ``PCDMask3DSegLevelEncoder.backbone`` = ``Res16UNet34C`` on MinkowskiEngine (modules/vision/pcd_mask3d_encoder.py:121,
modules/third_party/mask3d/res16unet.py:28-314,390-391, resnet.py:99-152, resnet_block.py:7-68).  MinkowskiEngine cannot be run
where this was written, so the coordinate rules below are MinkowskiEngine 0.5's *as far as they can be known without running it*;
what the tests pin is the mathematical definition, against a float64 dense restatement (tests/sparse_ref.py).

Coordinate rules (``coords`` [N, 1+3] int32: batch, x, y, z, distinct rows, as ``ME.utils.sparse_collate`` lays them out)
  * level coordinates at tensor stride s: the distinct ``(b, floor(xyz / s) * s)`` -- floor, not truncation, for negative
    coordinates (the rule of ``ops.parents_from_coords``);
  * offsets of an odd kernel size k at tensor stride s: ``{-(k // 2) .. k // 2} * s`` per axis; of the even size 2 (the stride-2
    convolutions, input stride s_in): ``{0, 1} * s_in``;
  * the offset INDEX (first dimension of a ``kernel`` parameter) runs with x fastest, then y, then z: ``kernel_offsets`` is the
    one place that says so (a fixture from a machine with MinkowskiEngine corrects the order there);
  * transposed convolution (kernel 2, stride 2) onto the cached finer level: every fine voxel has exactly one parent and
    uses the kernel slice of offset ``(fine - parent) / s_fine``.

Rows of every level are kept in an internal order (sorted by batch, then z, y, x: the rows of one 64-row tile of the
convolution kernel are then neighbours in space and share most of their gathered input rows).  Only ``parents`` and what
``Res16UNet34C.forward`` returns at full resolution are in the caller's row order.

Building a ``CoordPyramid`` needs the level sizes on the host (``torch.unique``): one synchronisation per batch, outside any
graph.  Everything ``Res16UNet34C.run`` launches afterwards is capturable.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import BF16, F32

ROW_TILE = 64        # PQ3D_SPARSE_TILE (include/pq3d_hip.h): output rows per workgroup = rows per occupancy word
_BIAS = 1 << 19      # coordinates (in units of the level's stride) are packed as 20-bit fields
_ACT = {None: 0, "none": 0, "relu": 1}


# ------------------------------------------------------------------------------------------------ coordinates and kernel maps
def kernel_offsets(kernel_size: int) -> torch.Tensor:
    """[K, 3] int32 (dx, dy, dz) of every kernel offset, in units of the input level's tensor stride, in the order of the
    first dimension of a ``kernel`` parameter: x fastest, then y, then z.  Odd sizes are centred, the even size 2 is {0, 1}."""
    r = range(-(kernel_size // 2), kernel_size // 2 + 1) if kernel_size % 2 else range(kernel_size)
    return torch.tensor([(dx, dy, dz) for dz in r for dy in r for dx in r], dtype=torch.int32)


def _pack(b: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """int64 sort key of voxels (b, q = xyz in stride units): batch, then z, y, x (x fastest = the internal row order)."""
    q = q + _BIAS
    return (b << 60) | (q[:, 2] << 40) | (q[:, 1] << 20) | q[:, 0]


def _unpack(key: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    m = (1 << 20) - 1
    return key >> 60, torch.stack([key & m, (key >> 20) & m, (key >> 40) & m], 1) - _BIAS


class KernelMap:
    """``nbr`` [N_out, K] int32 (row of the input level under each offset, -1 = absent) and the per-tile occupancy words."""
    __slots__ = ("nbr", "occ", "n_out", "n_in", "K")

    def __init__(self, nbr: torch.Tensor, n_in: int):
        self.nbr, self.n_out, self.n_in, self.K = nbr, nbr.shape[0], int(n_in), nbr.shape[1]
        self.occ = torch.empty((self.n_out + ROW_TILE - 1) // ROW_TILE, 4, dtype=torch.int32, device=nbr.device)
        L.call("pq3d_sparse_nbr", None, n_in, None, self.n_out, None, self.K, nbr, self.occ)


class CoordPyramid:
    """The five coordinate levels (tensor strides 1, 2, 4, 8, 16) of one batch and every kernel map the backbone uses.

    ``level_coords(l)``  [N_l, 1+3] int32 coordinates of internal level l (stride 2^l), in the internal row order
    ``perm`` / ``inv``   caller row -> level-0 row is ``inv``; ``perm`` is its inverse (``x_internal = x_caller[perm]``)
    ``nbr3[l]``, ``nbr5`` the k = 3 map of every level, the k = 5 map of level 0
    ``down[l]``, ``up[l]`` the kernel-2 stride-2 map level l -> l + 1 (rows: coarse) and its transpose (rows: fine), l = 0..3
    ``parents[h]``       [N] int64 row of every caller-order voxel in OUTPUT level h (h = 0..4 <-> strides 16, 8, 4, 2, 1: the
                         order of the backbone's feature maps); level 4 is returned in caller order, so ``parents[4]`` = arange
    """

    def __init__(self, coords: torch.Tensor):
        if not coords.is_cuda:
            raise L.Pq3dError("pq3d_amd kernels need device tensors (no CPU fallback)")
        assert coords.dim() == 2 and coords.shape[1] == 4, "voxel_coordinates is [N, 1+3] (batch, x, y, z)"
        c = coords.long()
        N = c.shape[0]
        assert N > 0, "empty batch"
        lo, hi, bmax = int(c[:, 1:].min()), int(c[:, 1:].max()), int(c[:, 0].max())      # (host sync: outside any graph)
        assert -_BIAS + 8 <= lo and hi < _BIAS - 8 and 0 <= int(c[:, 0].min()) and bmax < 8, \
            "coordinates must lie in (-2^19, 2^19) and the batch index in [0, 8)"
        dev = coords.device
        keys, inv = torch.unique(_pack(c[:, 0], c[:, 1:]), return_inverse=True)
        assert keys.numel() == N, "voxel_coordinates must be distinct (quantise before collating, as sparse_collate's callers do)"
        self.N, self.device, self.batch_size = N, dev, bmax + 1
        self.inv = inv
        self.perm = torch.empty_like(inv).scatter_(0, inv, torch.arange(N, device=dev))
        self.keys, self.q, self.child, self.kidx = [keys], [], [], []
        for l in range(5):
            b, q = _unpack(self.keys[l])
            self.q.append(torch.cat([b[:, None], q], 1).int().contiguous())
            if l == 4:
                break
            qc = torch.div(q, 2, rounding_mode="floor")
            ck, up = torch.unique(_pack(b, qc), return_inverse=True)
            d = q - 2 * qc
            self.keys.append(ck)
            self.child.append(up)                                   # fine row -> coarse row
            self.kidx.append(d[:, 0] + 2 * d[:, 1] + 4 * d[:, 2])   # offset index of (fine - parent) / s_fine: x fastest
        self.n = [int(k.numel()) for k in self.keys]
        o3, o5 = kernel_offsets(3).to(dev), kernel_offsets(5).to(dev)
        self.nbr3 = [self._lookup(l, o3) for l in range(5)]
        self.nbr5 = self._lookup(0, o5)
        self.down, self.up = [], []
        for l in range(4):
            nf, nc = self.n[l], self.n[l + 1]
            rows = torch.arange(nf, device=dev, dtype=torch.int32)
            dn = torch.full((nc, 8), -1, dtype=torch.int32, device=dev)
            dn[self.child[l], self.kidx[l]] = rows
            tr = torch.full((nf, 8), -1, dtype=torch.int32, device=dev)
            tr[rows.long(), self.kidx[l]] = self.child[l].int()
            self.down.append(KernelMap(dn, nf))
            self.up.append(KernelMap(tr, nc))
        par = [inv]
        for l in range(4):
            par.append(self.child[l][par[-1]])
        self.parents = [par[4], par[3], par[2], par[1], torch.arange(N, device=dev)]

    def _lookup(self, l: int, offs: torch.Tensor) -> KernelMap:
        nbr = torch.empty(self.n[l], offs.shape[0], dtype=torch.int32, device=self.device)
        L.call("pq3d_sparse_nbr", self.keys[l], self.n[l], self.q[l], self.n[l], offs, offs.shape[0], nbr, None)
        return KernelMap(nbr, self.n[l])

    def level_coords(self, l: int) -> torch.Tensor:
        q = self.q[l].clone()
        q[:, 1:] *= 1 << l
        return q


# ------------------------------------------------------------------------------------------------ the operator
def sparse_conv(x: torch.Tensor, kmap: KernelMap, W: torch.Tensor, *, ct: int = F32, scale=None, shift=None, bias=None,
                residual=None, act: Optional[str] = None, out: Optional[torch.Tensor] = None, col_off: int = 0,
                use_occ: bool = True, ntl: int = 0) -> torch.Tensor:
    """out[:, col_off : col_off + Cout] = act((sum_k x[nbr[:, k]] @ W[k]) * scale + shift + bias + residual), one launch
    (pq3d_sparse_conv_fwd).  ``x`` [N_in, Cin] and ``residual`` [N_out, Cout] fp32, rows may be strided (column views of a
    wider buffer); ``W`` [K, Cin, Cout] fp32 or bf16; ``out`` [N_out, >= col_off + Cout] fp32 (allocated when None).
    ``ntl``: output channels per workgroup / 16 (2, 4, 6 or 8; 0 = the library's choice) -- no output bit depends on it."""
    K, Cin, Cout = W.shape
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape == (kmap.n_in, Cin) and x.stride(1) == 1, "x is [N_in, Cin] fp32"
    assert kmap.K == K and W.is_contiguous() and kmap.nbr.is_contiguous()
    if out is None:
        out = torch.empty(kmap.n_out, col_off + Cout, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == kmap.n_out and out.stride(1) == 1
    assert out.shape[1] >= col_off + Cout
    d = L.SparseConvDesc()
    d.N_out, d.N_in, d.Cin, d.Cout, d.K = kmap.n_out, kmap.n_in, Cin, Cout, K
    d.ct, d.dtW, d.act, d.col_off, d.ntl = ct, L.dt_of(W), _ACT[act], col_off, ntl
    d.ldx, d.ldo = x.stride(0), out.stride(0)
    d.x, d.nbr, d.W, d.out = L.ptr(x), L.ptr(kmap.nbr), L.ptr(W), L.ptr(out)
    for name, t in (("scale", scale), ("shift", shift), ("bias", bias)):
        if t is not None:
            assert t.dtype == torch.float32 and t.numel() == Cout and t.is_contiguous()
            setattr(d, name, L.ptr(t))
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.shape == (kmap.n_out, Cout) and residual.stride(1) == 1
        d.residual, d.ldr = L.ptr(residual), residual.stride(0)
    if use_occ:
        d.occ = L.ptr(kmap.occ)
    esz = 2 if W.dtype == torch.bfloat16 else 4
    L.call("pq3d_sparse_conv_fwd", d, work=(f"No{kmap.n_out}Ni{kmap.n_in}Ci{Cin}Co{Cout}K{K}ct{ct}", 2.0 * kmap.n_out * K * Cin * Cout,
                                            4.0 * kmap.n_in * Cin + 4.0 * kmap.n_out * (K + Cout) + esz * K * Cin * Cout))
    return out


def row_gemm(x: torch.Tensor, Wt: torch.Tensor, bias: Optional[torch.Tensor], ct: int, act: Optional[str] = None) -> torch.Tensor:
    """A K = 1 convolution is a plain row GEMM: y = act(x @ Wt.T + bias) on pq3d_gemm.  ``Wt`` [Cout, Cin] fp32 or bf16; ``x`` rows
    may be strided."""
    Cout, Cin = Wt.shape
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == Cin and x.stride(1) == 1
    y = torch.empty(x.shape[0], Cout, dtype=torch.float32, device=x.device)
    if x.shape[0]:
        L.gemm(M=x.shape[0], N=Cout, K=Cin, A=[x], B=[Wt], bias=[bias], Cs=[y], ct=ct, lda=x.stride(0), ldb=Cin, ldc=Cout, act=act)
    return y


# ------------------------------------------------------------------------------------------------ modules
class SparseConv(nn.Module):
    """Parameter holder with MinkowskiConvolution(/Transpose)'s names and shapes: ``kernel`` [K, Cin, Cout] ([Cin, Cout] when
    K = 1), ``bias`` [1, Cout] when asked for."""

    def __init__(self, cin: int, cout: int, kernel_size: int, bias: bool = False):
        super().__init__()
        K = kernel_size ** 3
        self.cin, self.cout, self.K = cin, cout, K
        self.kernel = nn.Parameter(torch.empty((K, cin, cout) if K > 1 else (cin, cout)).normal_(0.0, (K * cin) ** -0.5))
        if bias:
            self.bias = nn.Parameter(torch.zeros(1, cout))


class SparseBatchNorm(nn.Module):
    """MinkowskiBatchNorm's layout: the statistics live in ``.bn`` (an nn.BatchNorm1d).  Eval mode only."""

    def __init__(self, c: int, momentum: float = 0.1):
        super().__init__()
        self.bn = nn.BatchNorm1d(c, momentum=momentum)


class BasicBlock(nn.Module):
    """resnet_block.py:7-68 (parameters only; the arithmetic is Res16UNet34C.run's)."""

    def __init__(self, inplanes: int, planes: int, downsample: Optional[nn.Module], bn_momentum: float = 0.1):
        super().__init__()
        self.conv1 = SparseConv(inplanes, planes, 3)
        self.norm1 = SparseBatchNorm(planes, bn_momentum)
        self.conv2 = SparseConv(planes, planes, 3)
        self.norm2 = SparseBatchNorm(planes, bn_momentum)
        self.downsample = downsample


class Res16UNet34C(nn.Module):
    """res16unet.py:28-314 with BLOCK = BasicBlock, LAYERS = (2, 3, 4, 6, 2, 2, 2, 2), PLANES = (32, 64, 128, 256, 256, 128, 96,
    96): the reference's parameter and buffer names, so a checkpoint's ``voxel_encoder.backbone.*`` entries load.  FROZEN and
    forward only: BatchNorm is eval-mode, folded to a per-channel scale and shift once in ``prepare()`` (which also converts
    the kernels to the compute type), and every convolution -> BatchNorm -> (+ residual) -> ReLU is one launch.

    ``forward(coords, feats)`` -> ``(out, [five feature maps, strides 16, 8, 4, 2, 1])`` as the reference's forward
    (res16unet.py:241-314): ``out`` IS the last block's output ([N, 96], the same tensor as the stride-1 map) -- the reference
    never applies ``final`` in its forward, so ``final.{kernel,bias}`` exist as state_dict entries only and ``out_channels``
    shapes nothing but them.  ``out`` and the stride-1 map are in the caller's row order, the coarser maps in the pyramid's
    internal order (``CoordPyramid.parents`` index them).  ``pyramid(coords, feats, hlevels)`` -> what
    ``data_dict['voxel_pyramid']`` expects (batched form).  A batch holds at most 8 scenes and coordinates lie in
    (-2^19, 2^19) voxels (the packing of the sort keys; ``CoordPyramid`` refuses anything else).

    ``prepare()`` runs at the first forward and again after ``load_state_dict`` / ``.to()`` / a change of ``compute``; after
    editing a parameter or buffer IN PLACE call ``prepare(force=True)``."""

    PLANES = (32, 64, 128, 256, 256, 128, 96, 96)
    LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)
    INIT_DIM = 32

    def __init__(self, in_channels: int, out_channels: int, config, out_fpn: bool = True, D: int = 3, compute: str = "fp32"):
        super().__init__()
        assert D == 3, "the 3-D network only"
        self.out_fpn, self.compute = out_fpn, compute
        mom = float(config["bn_momentum"])
        P = self.PLANES
        self.inplanes = self.INIT_DIM
        self.conv0p1s1 = SparseConv(in_channels, self.inplanes, int(config["conv1_kernel_size"]))
        assert self.conv0p1s1.K in (27, 125), "conv1_kernel_size 3 or 5"
        self.bn0 = SparseBatchNorm(self.inplanes, mom)
        for i, name in enumerate(("conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2")):
            setattr(self, name, SparseConv(self.inplanes, self.inplanes, 2))
            setattr(self, f"bn{i + 1}", SparseBatchNorm(self.inplanes, mom))
            setattr(self, f"block{i + 1}", self._make_layer(P[i], self.LAYERS[i], mom))
        skips = (P[2], P[1], P[0], self.INIT_DIM)
        for i, name in enumerate(("convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2")):
            setattr(self, name, SparseConv(self.inplanes, P[4 + i], 2))
            setattr(self, f"bntr{4 + i}", SparseBatchNorm(P[4 + i], mom))
            self.inplanes = P[4 + i] + skips[i]
            setattr(self, f"block{5 + i}", self._make_layer(P[4 + i], self.LAYERS[4 + i], mom))
        self.final = SparseConv(P[7], out_channels, 1, bias=True)
        del self.inplanes
        self._prep = None
        self.requires_grad_(False)
        self.eval()

    def _make_layer(self, planes: int, blocks: int, mom: float) -> nn.Sequential:
        downsample = None
        if self.inplanes != planes:
            downsample = nn.Sequential(SparseConv(self.inplanes, planes, 1), SparseBatchNorm(planes, mom))
        layers = [BasicBlock(self.inplanes, planes, downsample, mom)]
        self.inplanes = planes
        layers += [BasicBlock(planes, planes, None, mom) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    # ---- frozen-only contract
    def train(self, mode: bool = True):
        if mode and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("Res16UNet34C on the HIP kernels is the FROZEN backbone (BatchNorm in eval mode, "
                                      "PCDMask3DSegLevelEncoder(freeze_backbone=True)); batch-statistics BatchNorm and the "
                                      "sparse-convolution backward are the next step and are not provided")
        return super().train(False)     # a parent's .train() leaves the frozen backbone in eval mode

    def _apply(self, fn, *a, **k):
        self._prep = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):     # reached by this module's own and by any parent's load_state_dict
        self._prep = None
        return super()._load_from_state_dict(*a, **k)

    @property
    def ct(self) -> int:
        return {"fp32": F32, "bf16": BF16, "bf16x3": BF16}[self.compute]

    def prepare(self, force: bool = False):
        """Fold every BatchNorm (eval) into scale / shift and convert every kernel (K = 1 included) to the compute type, once."""
        key = (self.ct, self.conv0p1s1.kernel.device)
        if not force and self._prep is not None and self._prep["key"] == key:
            return self._prep
        wdt = torch.bfloat16 if self.ct == BF16 else torch.float32
        P = {"key": key}

        def fold(norm):
            bn = norm.bn
            s = (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps))
            return s.float().contiguous(), (bn.bias.detach().double() - bn.running_mean.double() * s).float().contiguous()

        def add(name, conv, norm):
            scale, shift = fold(norm) if norm is not None else (None, None)
            w = conv.kernel.detach()
            if conv.K == 1:     # row GEMM: the scale goes into the weight (fp32, before the conversion), the shift is the bias
                P[name] = ((w * scale[None, :]).t().to(wdt).contiguous(), shift)
            else:
                P[name] = (w.to(wdt).contiguous(), scale, shift)
        for i, name in enumerate(("conv0p1s1", "conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2")):
            add(name, getattr(self, name), getattr(self, f"bn{i}"))
        for i, name in enumerate(("convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2")):
            add(name, getattr(self, name), getattr(self, f"bntr{4 + i}"))
        for bi in range(1, 9):
            for j, blk in enumerate(getattr(self, f"block{bi}")):
                add(f"block{bi}.{j}.conv1", blk.conv1, blk.norm1)
                add(f"block{bi}.{j}.conv2", blk.conv2, blk.norm2)
                if blk.downsample is not None:
                    add(f"block{bi}.{j}.downsample", blk.downsample[0], blk.downsample[1])
        self._prep = P
        return P

    # ---- the launches (capturable)
    def run(self, pyr: CoordPyramid, feats: torch.Tensor):
        """All convolutions for a built pyramid: no host synchronisation, no allocation outside torch's caching allocator."""
        if self.training or any(m.training for m in self.modules()):
            raise NotImplementedError("Res16UNet34C on the HIP kernels runs in eval mode only (frozen backbone)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("training the voxel backbone is not provided: call under torch.no_grad() "
                                      "(freeze_backbone=True) or set requires_grad_(False)")
        if not feats.is_cuda:
            raise L.Pq3dError("pq3d_amd kernels need device tensors (no CPU fallback)")
        assert feats.shape == (pyr.N, self.conv0p1s1.cin), "feats is [N, in_channels] in the row order of the coordinates"
        with torch.no_grad():
            return self._run(pyr, feats.detach().float())

    def _run(self, pyr, feats):
        P, ct, n, dev = self.prepare(), self.ct, pyr.n, feats.device
        PL, I = self.PLANES, self.INIT_DIM
        new = lambda rows, c: torch.empty(rows, c, dtype=torch.float32, device=dev)

        def conv(name, x, kmap, residual=None, out=None, col_off=0):
            W, scale, shift = P[name]
            return sparse_conv(x, kmap, W, ct=ct, scale=scale, shift=shift, residual=residual, act="relu", out=out, col_off=col_off)

        def block(bi, x, l, out=None, col_off=0):
            blocks = getattr(self, f"block{bi}")
            for j, blk in enumerate(blocks):
                name = f"block{bi}.{j}"
                last = j == len(blocks) - 1
                y = conv(name + ".conv1", x, pyr.nbr3[l])
                res = row_gemm(x, *P[name + ".downsample"], ct) if blk.downsample is not None else x
                x = conv(name + ".conv2", y, pyr.nbr3[l], residual=res, out=out if last else None, col_off=col_off if last else 0)
                if last and out is not None:
                    x = out[:, col_off:col_off + blk.conv2.cout]
            return x

        # the four concatenation buffers [transposed-convolution output | skip]: both halves are written where they are produced
        cat8, cat7 = new(n[0], PL[7] + I), new(n[1], PL[6] + PL[0])
        cat6, cat5 = new(n[2], PL[5] + PL[1]), new(n[3], PL[4] + PL[2])
        x0 = feats.index_select(0, pyr.perm)
        conv("conv0p1s1", x0, pyr.nbr5 if self.conv0p1s1.K == 125 else pyr.nbr3[0], out=cat8, col_off=PL[7])
        out_p1 = cat8[:, PL[7]:]
        b1 = block(1, conv("conv1p1s2", out_p1, pyr.down[0]), 1, out=cat7, col_off=PL[6])
        b2 = block(2, conv("conv2p2s2", b1, pyr.down[1]), 2, out=cat6, col_off=PL[5])
        b3 = block(3, conv("conv3p4s2", b2, pyr.down[2]), 3, out=cat5, col_off=PL[4])
        f16 = block(4, conv("conv4p8s2", b3, pyr.down[3]), 4)
        conv("convtr4p16s2", f16, pyr.up[3], out=cat5)
        f8 = block(5, cat5, 3)
        conv("convtr5p8s2", f8, pyr.up[2], out=cat6)
        f4 = block(6, cat6, 2)
        conv("convtr6p4s2", f4, pyr.up[1], out=cat7)
        f2 = block(7, cat7, 1)
        conv("convtr7p2s2", f2, pyr.up[0], out=cat8)
        f1 = block(8, cat8, 0)
        out = f1.index_select(0, pyr.inv)      # res16unet.py:307-314: the forward returns block8's output; `final` is never applied
        return out, [f16, f8, f4, f2, out]

    def forward(self, coords: torch.Tensor, feats: torch.Tensor):
        out, maps = self.run(CoordPyramid(coords), feats)
        return (out, maps) if self.out_fpn else out

    def pyramid(self, coords: torch.Tensor, feats: torch.Tensor, hlevels: Sequence[int] = (0, 1, 2, 3)) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """``[(features [N_level, C_level], parents [N] int64)]`` for every level in ``hlevels + [4]``: the batched form of
        ``PCDMask3DSegLevelEncoder.forward`` (rows of all scenes concatenated; ``parents`` in the caller's voxel order)."""
        pyr = CoordPyramid(coords)
        _out, maps = self.run(pyr, feats)
        return [(maps[h], pyr.parents[h]) for h in list(hlevels) + [4]]
