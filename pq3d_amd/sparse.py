"""Sparse-convolution voxel backbone on the HIP kernels: coordinate pyramid, kernel maps, the convolution's forward and backward
operators, batch-statistics BatchNorm, and Res16UNet34C (frozen and forward only by default; ``trainable=True`` trains it).

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
graph.  Everything ``Res16UNet34C.run`` launches afterwards -- the training forward and its backward included -- is capturable.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import BF16, F32

ROW_TILE = L.H.PQ3D_SPARSE_TILE        # output rows per workgroup = rows per occupancy word
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
def _conv_launch(x, kmap, W, Cin, Cout, wmode, ct, scale, shift, bias, residual, act, out, col_off, use_occ, ntl):
    K = W.shape[0]
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape == (kmap.n_in, Cin) and x.stride(1) == 1, "x is [N_in, Cin] fp32"
    assert kmap.K == K and W.is_contiguous() and kmap.nbr.is_contiguous()
    if out is None:
        out = torch.empty(kmap.n_out, col_off + Cout, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == kmap.n_out and out.stride(1) == 1
    assert out.shape[1] >= col_off + Cout
    d = L.SparseConvDesc()
    d.N_out, d.N_in, d.Cin, d.Cout, d.K = kmap.n_out, kmap.n_in, Cin, Cout, K
    d.ct, d.dtW, d.act, d.col_off, d.ntl, d.wmode = ct, L.dt_of(W), _ACT[act], col_off, ntl, wmode
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
    L.call("pq3d_sparse_conv_fwd", d, work=(f"No{kmap.n_out}Ni{kmap.n_in}Ci{Cin}Co{Cout}K{K}ct{ct}" + (f"w{wmode}" if wmode else ""),
                                            2.0 * kmap.n_out * K * Cin * Cout,
                                            4.0 * kmap.n_in * Cin + 4.0 * kmap.n_out * (K + Cout) + esz * K * Cin * Cout))
    return out


def sparse_conv(x: torch.Tensor, kmap: KernelMap, W: torch.Tensor, *, ct: int = F32, scale=None, shift=None, bias=None,
                residual=None, act: Optional[str] = None, out: Optional[torch.Tensor] = None, col_off: int = 0,
                use_occ: bool = True, ntl: int = 0) -> torch.Tensor:
    """out[:, col_off : col_off + Cout] = act((sum_k x[nbr[:, k]] @ W[k]) * scale + shift + bias + residual), one launch
    (pq3d_sparse_conv_fwd).  ``x`` [N_in, Cin] and ``residual`` [N_out, Cout] fp32, rows may be strided (column views of a
    wider buffer); ``W`` [K, Cin, Cout] fp32 or bf16; ``out`` [N_out, >= col_off + Cout] fp32 (allocated when None).
    ``ntl``: output channels per workgroup / 16 (2, 4, 6 or 8; 0 = the library's choice) -- no output bit depends on it."""
    K, Cin, Cout = W.shape
    return _conv_launch(x, kmap, W, Cin, Cout, 0, ct, scale, shift, bias, residual, act, out, col_off, use_occ, ntl)


def sparse_conv_bwd_input(dy: torch.Tensor, kmap_t: KernelMap, W: torch.Tensor, reverse_k: bool = False, *, ct: int = F32,
                          residual=None, out: Optional[torch.Tensor] = None, col_off: int = 0, use_occ: bool = True,
                          ntl: int = 0) -> torch.Tensor:
    """Input gradient of ``sparse_conv``: out[:, col_off : col_off + Cin] = sum_k dy[kmap_t.nbr[:, k]] @ W[k'].T + residual with
    ``W`` the FORWARD weight [K, Cin, Cout] as it is stored (the kernel reads it transposed: no copy).  ``kmap_t`` is the
    transpose of the forward's map: ``up[l]`` for a ``down[l]`` convolution and the reverse with k' = k; for the centred
    kernels the same ``nbr3`` / ``nbr5`` map with ``reverse_k=True`` (k' = K - 1 - k).  ``dy`` [kmap_t.n_in, Cout] fp32, rows may
    be strided; ``residual`` [kmap_t.n_out, Cin] is added in the epilogue -- the gradient accumulate of a tensor with a second
    consumer.  An input row no output row uses gets exact zeros (+ residual)."""
    K, Cin, Cout = W.shape
    return _conv_launch(dy, kmap_t, W, Cout, Cin, 2 if reverse_k else 1, ct, None, None, None, residual, None, out, col_off,
                        use_occ, ntl)


def wgrad_splits(n_out: int, Cin: int, Cout: int, K: int, splits: int = 0) -> int:
    """The number of row chunks ``sparse_conv_bwd_weight`` uses (``splits`` = 0: the library's choice from the sizes)."""
    S = int(L.lib().pq3d_sparse_conv_wgrad_splits(n_out, Cin, Cout, K, splits))
    if S < 1:
        raise L.Pq3dError("pq3d_sparse_conv_wgrad_splits: splits must be 0 (chosen from the sizes) or 1 .. 4096")
    return S


def sparse_conv_bwd_weight(x: torch.Tensor, kmap: KernelMap, dy: torch.Tensor, *, ct: int = F32, splits: int = 0,
                           out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, use_occ: bool = True) -> torch.Tensor:
    """Weight gradient of ``sparse_conv``: dW[k] = x[kmap.nbr[:, k]].T @ dy, [K, Cin, Cout] fp32, every element written
    (pq3d_sparse_conv_wgrad).  ``x`` [N_in, Cin], ``dy`` [N_out, Cout] fp32, rows may be strided.  The rows are cut into
    ``splits`` chunks (0 = chosen from the sizes) whose partial slabs are summed in chunk order: no atomics, the same bits run
    to run for a given ``splits``.  ``ws``: fp32 workspace (allocated when None; a given one that is too small is refused)."""
    Cin, Cout, K = x.shape[1], dy.shape[1], kmap.K
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] == kmap.n_in and x.stride(1) == 1, "x is [N_in, Cin] fp32"
    assert dy.dtype == torch.float32 and dy.dim() == 2 and dy.shape[0] == kmap.n_out and dy.stride(1) == 1, "dy is [N_out, Cout] fp32"
    assert kmap.nbr.is_contiguous()
    if out is None:
        out = torch.empty(K, Cin, Cout, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape == (K, Cin, Cout) and out.is_contiguous()
    need = int(L.lib().pq3d_sparse_conv_wgrad_ws_bytes(kmap.n_out, Cin, Cout, K, splits))
    if need < 0:
        raise L.Pq3dError("pq3d_sparse_conv_wgrad_ws_bytes: splits must be 0 (chosen from the sizes) or 1 .. 4096")
    if ws is None and need:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    d = L.SparseWgradDesc()
    d.N_out, d.N_in, d.Cin, d.Cout, d.K, d.ct, d.splits = kmap.n_out, kmap.n_in, Cin, Cout, K, ct, splits
    d.ldx, d.ldy = x.stride(0), dy.stride(0)
    d.x, d.nbr, d.dy, d.dW = L.ptr(x), L.ptr(kmap.nbr), L.ptr(dy), L.ptr(out)
    if ws is not None:
        assert ws.dtype == torch.float32 and ws.is_contiguous()
        d.ws, d.ws_bytes = L.ptr(ws), ws.numel() * 4
    if use_occ:
        d.occ = L.ptr(kmap.occ)
    L.call("pq3d_sparse_conv_wgrad", d, work=(f"No{kmap.n_out}Ni{kmap.n_in}Ci{Cin}Co{Cout}K{K}ct{ct}", 2.0 * kmap.n_out * K * Cin * Cout,
                                              4.0 * kmap.n_in * Cin + 4.0 * kmap.n_out * (K + Cout) + 4.0 * K * Cin * Cout + 2.0 * need))
    return out


# ------------------------------------------------------------------------------------------------ batch-statistics BatchNorm
def _rows(t, C, name):
    assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == C and t.stride(1) == 1, f"{name} is [N, C] fp32 (rows may be strided)"
    return t


def _bn_part(N: int, C: int, dev) -> torch.Tensor:
    return torch.empty(int(L.lib().pq3d_bn_ws_floats(N, C)), dtype=torch.float32, device=dev)


def bn_stats(z: torch.Tensor, eps: float, momentum: float = 0.0, running_mean=None, running_var=None, num_batches_tracked=None):
    """(mean, rstd) [C] of the rows of ``z`` [N, C] (biased variance, rstd = 1 / sqrt(var + eps)), summed in a fixed order without
    ever forming E[x^2] - mean^2.  The running buffers (optional) are updated in place on the device as nn.BatchNorm1d does in
    training mode: (1 - momentum) old + momentum new with the unbiased variance, ``num_batches_tracked`` += 1."""
    N, C = z.shape
    _rows(z, C, "z")
    mean, rstd = torch.empty(C, dtype=torch.float32, device=z.device), torch.empty(C, dtype=torch.float32, device=z.device)
    for t in (running_mean, running_var):
        assert t is None or (t.dtype == torch.float32 and t.shape == (C,) and t.is_contiguous())
    assert num_batches_tracked is None or (num_batches_tracked.dtype == torch.int64 and num_batches_tracked.numel() == 1)
    L.call("pq3d_bn_stats", z, z.stride(0), N, C, float(eps), float(momentum), mean, rstd, running_mean, running_var,
           num_batches_tracked, _bn_part(N, C, z.device), work=(f"N{N}C{C}", 4.0 * N * C, 4.0 * N * C))
    return mean, rstd


def bn_apply(z: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, residual=None,
             act: Optional[str] = None, out: Optional[torch.Tensor] = None, col_off: int = 0) -> torch.Tensor:
    """out[:, col_off : col_off + C] = act((z - mean) * rstd * weight + bias + residual); returns that column view."""
    N, C = z.shape
    _rows(z, C, "z")
    if out is None:
        out = torch.empty(N, col_off + C, dtype=torch.float32, device=z.device)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == N and out.stride(1) == 1 and out.shape[1] >= col_off + C
    if residual is not None:
        _rows(residual, C, "residual")
        assert residual.shape[0] == N
    L.call("pq3d_bn_apply", z, z.stride(0), N, C, mean, rstd, weight, bias, residual, residual.stride(0) if residual is not None else 0,
           _ACT[act], out, out.stride(0), col_off, work=(f"N{N}C{C}", 4.0 * N * C, (12.0 if residual is not None else 8.0) * N * C))
    return out[:, col_off:col_off + C]


def bn_bwd_reduce(dy: torch.Tensor, z: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, y: Optional[torch.Tensor] = None):
    """(dweight, dbias) [C]: sum_r g xhat and sum_r g with g = dy * [y > 0] (``y``: the ReLU output) or g = dy; fixed order."""
    N, C = z.shape
    _rows(z, C, "z"); _rows(dy, C, "dy")
    assert dy.shape[0] == N and (y is None or (_rows(y, C, "y").shape[0] == N))
    dg, db = torch.empty(C, dtype=torch.float32, device=z.device), torch.empty(C, dtype=torch.float32, device=z.device)
    L.call("pq3d_bn_bwd_reduce", dy, dy.stride(0), y, y.stride(0) if y is not None else 0, z, z.stride(0), N, C, mean, rstd, dg, db,
           _bn_part(N, C, z.device), work=(f"N{N}C{C}", 5.0 * N * C, (12.0 if y is not None else 8.0) * N * C))
    return dg, db


def bn_bwd_apply(dy: torch.Tensor, z: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, weight: torch.Tensor, dweight: torch.Tensor,
                 dbias: torch.Tensor, *, y: Optional[torch.Tensor] = None, dres: Optional[torch.Tensor] = None, dres_add: bool = False,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dz = weight rstd (g - dbias / N - xhat dweight / N) with (dweight, dbias) of ``bn_bwd_reduce``; ``dres`` [N, C] (optional,
    rows may be strided) receives g, the gradient of the residual branch: written, or added with ``dres_add``."""
    N, C = z.shape
    _rows(z, C, "z"); _rows(dy, C, "dy")
    assert dy.shape[0] == N and (y is None or (_rows(y, C, "y").shape[0] == N))
    if out is None:
        out = torch.empty(N, C, dtype=torch.float32, device=z.device)
    _rows(out, C, "out")
    assert out.shape[0] == N and (dres is None or _rows(dres, C, "dres").shape[0] == N)
    L.call("pq3d_bn_bwd_apply", dy, dy.stride(0), y, y.stride(0) if y is not None else 0, z, z.stride(0), N, C, mean, rstd, weight,
           dweight, dbias, out, out.stride(0), dres, dres.stride(0) if dres is not None else 0, int(dres_add),
           work=(f"N{N}C{C}", 8.0 * N * C, 16.0 * N * C))
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


def _gemm_raw(x: torch.Tensor, W: torch.Tensor, ct: int) -> torch.Tensor:
    """x @ W with the K = 1 convolution's kernel as it is stored ([Cin, Cout] fp32): the training forward of a ``downsample``."""
    Cin, Cout = W.shape
    y = torch.empty(x.shape[0], Cout, dtype=torch.float32, device=x.device)
    L.gemm(M=x.shape[0], N=Cout, K=Cin, A=[x], B=[W], Cs=[y], ct=ct, lda=x.stride(0), ldb=Cout, ldc=Cout, transB=True)
    return y


def _gemm_raw_bwd(x: torch.Tensor, W: torch.Tensor, dz: torch.Tensor, ct: int):
    """(dx, dW) of ``_gemm_raw``: dz @ W.T and x.T @ dz (one writer per element: no split-K atomics)."""
    Cin, Cout = W.shape
    R = x.shape[0]
    dx = torch.empty(R, Cin, dtype=torch.float32, device=x.device)
    dW = torch.empty(Cin, Cout, dtype=torch.float32, device=x.device)
    L.gemm(M=R, N=Cin, K=Cout, A=[dz], B=[W], Cs=[dx], ct=ct, lda=dz.stride(0), ldb=Cout, ldc=Cin)
    L.gemm(M=Cin, N=Cout, K=R, A=[x], B=[dz], Cs=[dW], ct=ct, lda=x.stride(0), ldb=dz.stride(0), ldc=Cout, transA=True, transB=True)
    return dx, dW


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
    """MinkowskiBatchNorm's layout: the statistics live in ``.bn`` (an nn.BatchNorm1d).  Parameters and buffers only: the
    arithmetic (folded in eval mode, batch statistics in training mode) is Res16UNet34C.run's."""

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


class _BackboneTrain(torch.autograd.Function):
    """Res16UNet34C's training forward and backward as ONE autograd node: inputs are every kernel / bn.weight / bn.bias in
    the order of the network's layer table, outputs the five feature maps."""

    @staticmethod
    def forward(ctx, net, pyr, feats, *params):
        tape = {}
        outs = net._train_forward(pyr, feats, tape)
        # the coarse maps are outputs AND tape entries (the ReLU mask of their own layer, the input of the next transposed
        # convolution): those go through save_for_backward.  An output kept as a plain attribute ties the node to its own
        # result -- the graph, with the parameters' AccumulateGrad nodes of the stream it ran on, would outlive the step.
        pos = {id(o): i for i, o in enumerate(outs[:4])}
        for t in tape.values():
            for key in ("x", "y"):
                if id(t[key]) in pos:
                    t[key] = pos[id(t[key])]
        assert sum(isinstance(t[key], int) for t in tape.values() for key in ("x", "y")) == 8
        ctx.save_for_backward(*outs[:4])
        ctx.net, ctx.pyr, ctx.tape = net, pyr, tape
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, g16, g8, g4, g2, gout):
        tape = {k: dict(v) for k, v in ctx.tape.items()}
        saved = ctx.saved_tensors
        for t in tape.values():
            for key in ("x", "y"):
                if isinstance(t[key], int):
                    t[key] = saved[t[key]]
        cg = lambda g: None if g is None else g.float().contiguous()
        grads = ctx.net._train_backward(ctx.pyr, tape, cg(g16), cg(g8), cg(g4), cg(g2), gout)
        flat = [g for name, _c, _n in ctx.net._layers for g in grads[name]]
        return (None, None, None, *flat)


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
    editing a parameter or buffer IN PLACE call ``prepare(force=True)``.

    ``trainable=True``: parameters require grad and ``train()`` / ``eval()`` behave as on any module.  In training mode ``run``
    executes convolution (raw fp32 weights, converted in the kernel) -> batch statistics -> normalise for every layer, updates the
    running buffers on the device, and returns the five maps from ONE autograd node whose backward walks the recorded tape in
    reverse (input gradient = the forward kernel on the transposed map, weight gradient over row chunks without atomics,
    BatchNorm backward; ``'bf16'`` and ``'bf16x3'`` both mean bf16 operands there).  Batch statistics are per process (no
    SyncBatchNorm).  ``final.*`` never gets a gradient: ``unused_parameters()`` lists it.  In eval mode a trainable module runs
    the folded path above under ``no_grad``, folding afresh at every forward (its weights change under the optimizer);
    with grad enabled it raises."""

    PLANES = (32, 64, 128, 256, 256, 128, 96, 96)
    LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)
    INIT_DIM = 32
    # The U-Net's graph below the stem.  Down stage i takes level i to level i + 1 (tensor stride 2^(i+1)): (stride-2 convolution,
    # its BatchNorm, the block group that follows; planes PLANES[i]).  Up stage i takes level 4 - i to level 3 - i: (transposed
    # convolution, its BatchNorm, the block group that runs on [its output | skip]; planes PLANES[4 + i], width of that skip).
    _DOWN = (("conv1p1s2", "bn1", "block1"), ("conv2p2s2", "bn2", "block2"),
             ("conv3p4s2", "bn3", "block3"), ("conv4p8s2", "bn4", "block4"))
    _UP = (("convtr4p16s2", "bntr4", "block5", PLANES[2]), ("convtr5p8s2", "bntr5", "block6", PLANES[1]),
           ("convtr6p4s2", "bntr6", "block7", PLANES[0]), ("convtr7p2s2", "bntr7", "block8", INIT_DIM))
    # (left, skip) widths of the concatenation buffer of level l = 0..3, the one up stage 3 - l fills: the forward writes the
    # skip at column `left`, the backward splits the buffer's gradient there
    _CAT = tuple(zip(PLANES[4:], (stage[3] for stage in _UP)))[::-1]

    def __init__(self, in_channels: int, out_channels: int, config, out_fpn: bool = True, D: int = 3, compute: str = "fp32",
                 trainable: bool = False):
        super().__init__()
        assert D == 3, "the 3-D network only"
        self.out_fpn, self.compute, self.trainable = out_fpn, compute, bool(trainable)
        mom = float(config["bn_momentum"])
        P = self.PLANES
        self.inplanes = self.INIT_DIM
        self.conv0p1s1 = SparseConv(in_channels, self.inplanes, int(config["conv1_kernel_size"]))
        assert self.conv0p1s1.K in (27, 125), "conv1_kernel_size 3 or 5"
        self.bn0 = SparseBatchNorm(self.inplanes, mom)
        for i, (conv, bn, group) in enumerate(self._DOWN):
            setattr(self, conv, SparseConv(self.inplanes, self.inplanes, 2))
            setattr(self, bn, SparseBatchNorm(self.inplanes, mom))
            setattr(self, group, self._make_layer(P[i], self.LAYERS[i], mom))
        for i, (conv, bn, group, skip) in enumerate(self._UP):
            setattr(self, conv, SparseConv(self.inplanes, P[4 + i], 2))
            setattr(self, bn, SparseBatchNorm(P[4 + i], mom))
            self.inplanes = P[4 + i] + skip
            setattr(self, group, self._make_layer(P[4 + i], self.LAYERS[4 + i], mom))
        self.final = SparseConv(P[7], out_channels, 1, bias=True)
        del self.inplanes
        self._prep = None
        # every (name, convolution, BatchNorm) the forward runs, in the order of the training node's inputs and gradients
        # (``final`` is not one of them), and the names of each group's blocks.  Plain containers of MODULES: nn.Module does not
        # register them a second time, and whatever replaces a parameter or its data leaves them valid.
        stages = self._DOWN + self._UP
        self._layers = [(conv, getattr(self, conv), getattr(self, bn)) for conv, bn, *_ in (("conv0p1s1", "bn0"),) + stages]
        self._blocks = {}
        for group in (s[2] for s in stages):
            self._blocks[group] = [f"{group}.{j}" for j in range(len(getattr(self, group)))]
            for name, blk in zip(self._blocks[group], getattr(self, group)):
                self._layers += [(name + ".conv1", blk.conv1, blk.norm1), (name + ".conv2", blk.conv2, blk.norm2)]
                if blk.downsample is not None:
                    self._layers.append((name + ".downsample", blk.downsample[0], blk.downsample[1]))
        self._by_name = {name: (conv, norm) for name, conv, norm in self._layers}
        if self.trainable:
            return                      # parameters require grad, training mode: as any freshly built module
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
        if self.trainable:
            return super().train(mode)
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
        # a trainable network's weights move under an optimizer that updates them in place (TrainStep's flat AdamW leaves no
        # trace on the module): its eval-mode forward folds afresh every time instead of trusting a cache
        if not force and not self.trainable and self._prep is not None and self._prep["key"] == key:
            return self._prep
        wdt = torch.bfloat16 if self.ct == BF16 else torch.float32
        P = {"key": key}

        def fold(norm):
            bn = norm.bn
            s = (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps))
            return s.float().contiguous(), (bn.bias.detach().double() - bn.running_mean.double() * s).float().contiguous()

        for name, conv, norm in self._layers:
            scale, shift = fold(norm)
            w = conv.kernel.detach()
            if conv.K == 1:     # row GEMM: the scale goes into the weight (fp32, before the conversion), the shift is the bias
                P[name] = ((w * scale[None, :]).t().to(wdt).contiguous(), shift)
            else:
                P[name] = (w.to(wdt).contiguous(), scale, shift)
        self._prep = P
        return P

    # ---- the launches (capturable)
    def run(self, pyr: CoordPyramid, feats: torch.Tensor):
        """All convolutions for a built pyramid: no host synchronisation, no allocation outside torch's caching allocator."""
        train = self.trainable and self.training
        if not train:
            if self.training or any(m.training for m in self.modules()):
                raise NotImplementedError("Res16UNet34C on the HIP kernels runs in eval mode only (frozen backbone)")
            if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                raise NotImplementedError("training the voxel backbone is not provided: call under torch.no_grad() "
                                          "(freeze_backbone=True) or set requires_grad_(False)")
        if not feats.is_cuda:
            raise L.Pq3dError("pq3d_amd kernels need device tensors (no CPU fallback)")
        assert feats.shape == (pyr.N, self.conv0p1s1.cin), "feats is [N, in_channels] in the row order of the coordinates"
        feats = feats.detach().float()
        if train:
            params = [p for _name, conv, norm in self._layers for p in (conv.kernel, norm.bn.weight, norm.bn.bias)]
            maps = list(_BackboneTrain.apply(self, pyr, feats, *params))
            return maps[4], maps
        with torch.no_grad():
            return self._run(pyr, feats)

    def _walk(self, pyr, feats, layer):
        """The network's graph, for both modes: the five feature maps (strides 16, 8, 4, 2, 1; the last in the caller's row order).
        ``layer(name, x, kmap, residual=None, act="relu", out=None, col_off=0)`` executes one named layer (``kmap`` None: the
        1 x 1 ``downsample``) and returns its activation, the [rows, Cout] column view of ``out`` at ``col_off``."""
        # (concatenation buffer [transposed-convolution output | skip], column of the skip) of levels 0..3.  Both halves are
        # written where they are produced: the skip by the way down's last layer at that level.
        cat = [(torch.empty(pyr.n[l], left + skip, dtype=torch.float32, device=feats.device), left)
               for l, (left, skip) in enumerate(self._CAT)]

        def blocks(group, x, l, out=None, col_off=0):
            names = self._blocks[group]
            for j, name in enumerate(names):
                last = j == len(names) - 1
                y = layer(name + ".conv1", x, pyr.nbr3[l])
                res = layer(name + ".downsample", x, None, act=None) if name + ".downsample" in self._by_name else x
                x = layer(name + ".conv2", y, pyr.nbr3[l], residual=res, out=out if last else None, col_off=col_off if last else 0)
            return x

        out, col_off = cat[0]
        x = layer("conv0p1s1", feats.index_select(0, pyr.perm), pyr.nbr5 if self.conv0p1s1.K == 125 else pyr.nbr3[0], out=out, col_off=col_off)
        for l, (conv, _bn, group) in enumerate(self._DOWN, 1):
            out, col_off = cat[l] if l < 4 else (None, 0)      # the coarsest level feeds no skip
            x = blocks(group, layer(conv, x, pyr.down[l - 1]), l, out, col_off)
        maps = [x]
        for l, (conv, _bn, group, _skip) in zip((3, 2, 1, 0), self._UP):
            layer(conv, x, pyr.up[l], out=cat[l][0])
            x = blocks(group, cat[l][0], l)
            maps.append(x)
        maps[4] = x.index_select(0, pyr.inv)   # res16unet.py:307-314: the forward returns block8's output; `final` is never applied
        return maps

    def _run(self, pyr, feats):
        P, ct = self.prepare(), self.ct

        def layer(name, x, kmap, residual=None, act="relu", out=None, col_off=0):
            if kmap is None:
                return row_gemm(x, *P[name], ct, act)
            W, scale, shift = P[name]
            y = sparse_conv(x, kmap, W, ct=ct, scale=scale, shift=shift, residual=residual, act=act, out=out, col_off=col_off)
            return y if out is None else y[:, col_off:col_off + W.shape[2]]      # sparse_conv returns the whole buffer
        maps = self._walk(pyr, feats, layer)
        return maps[4], maps

    # ---- training: batch-statistics BatchNorm, one autograd node for the whole network
    def unused_parameters(self):
        """``final.*`` when trainable: the forward never applies ``final`` (as the reference's), so it never gets a gradient."""
        return list(self.final.parameters()) if self.trainable else []

    def training_tape(self, pyr: CoordPyramid, feats: torch.Tensor):
        """One training-mode forward outside autograd (the running buffers ARE updated): ``{layer name: (conv, norm, record)}``
        with the record the backward works from -- ``x`` the layer's input, ``kmap`` its kernel map (None for the 1 x 1
        ``downsample``), ``z`` the raw convolution output, ``y`` the activation, ``mean`` / ``rstd`` the batch statistics.
        For tools that time or inspect single layers."""
        tape = {}
        with torch.no_grad():
            self._train_forward(pyr, feats.detach().float(), tape)
        return {name: (conv, norm, tape[name]) for name, conv, norm in self._layers}

    def _train_forward(self, pyr, feats, tape):
        """Convolution (raw fp32 weights, converted in the kernel) -> batch statistics -> normalise for every layer; ``tape``
        receives, per layer name, what the backward needs: the input, the raw output z, the activation y, mean and rstd."""
        ct, mods = self.ct, self._by_name

        def layer(name, x, kmap, residual=None, act="relu", out=None, col_off=0):
            conv, norm = mods[name]
            bn = norm.bn
            z = sparse_conv(x, kmap, conv.kernel.detach(), ct=ct) if conv.K > 1 else _gemm_raw(x, conv.kernel.detach(), ct)
            mean, rstd = bn_stats(z, bn.eps, bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked)
            y = bn_apply(z, mean, rstd, bn.weight.detach(), bn.bias.detach(), residual=residual, act=act, out=out, col_off=col_off)
            tape[name] = dict(x=x, kmap=kmap, z=z, y=y, mean=mean, rstd=rstd, act=act)
            return y
        return tuple(self._walk(pyr, feats, layer))

    def _train_backward(self, pyr, tape, g16, g8, g4, g2, gout):
        """The tape walked in reverse.  Returns {layer name: (dkernel, dbn.weight, dbn.bias)}.  The gradient of a concatenation is
        one buffer whose halves are read as strided views; a tensor with two consumers (block input and skip connection, a
        feature map that is also an output) gets the second gradient through the input-gradient kernel's ``residual``."""
        ct, mods = self.ct, self._by_name
        grads = {}

        def bn_back(name, dy, dres=None):
            """dz of layer ``name`` from the gradient of its activation; records the BatchNorm parameter gradients."""
            (_conv, norm), t = mods[name], tape[name]
            y = t["y"] if t["act"] else None
            dg, db = bn_bwd_reduce(dy, t["z"], t["mean"], t["rstd"], y=y)
            dz = bn_bwd_apply(dy, t["z"], t["mean"], t["rstd"], norm.bn.weight.detach(), dg, db, y=y, dres=dres)
            grads[name] = [None, dg, db]
            return dz

        def conv_back(name, dz, kmap_t, reverse_k, residual=None, need_dx=True):
            """Weight gradient of layer ``name`` (recorded) and the gradient of its input (+ residual)."""
            (conv, _norm), t = mods[name], tape[name]
            grads[name][0] = sparse_conv_bwd_weight(t["x"], t["kmap"], dz, ct=ct)
            return sparse_conv_bwd_input(dz, kmap_t, conv.kernel.detach(), reverse_k, ct=ct, residual=residual) if need_dx else None

        def block_back(group, l, d):
            """``d``: gradient of block group ``group``'s output -> gradient of its input."""
            for name in reversed(self._blocks[group]):
                g = torch.empty(d.shape[0], d.shape[1], dtype=torch.float32, device=d.device)   # the residual branch's gradient
                dz2 = bn_back(name + ".conv2", d, dres=g)
                dy1 = conv_back(name + ".conv2", dz2, pyr.nbr3[l], True)
                dz1 = bn_back(name + ".conv1", dy1)
                dn = name + ".downsample"
                if dn in mods:
                    dzd = bn_back(dn, g)
                    g, grads[dn][0] = _gemm_raw_bwd(tape[dn]["x"], mods[dn][0].kernel.detach(), dzd, ct)
                d = conv_back(name + ".conv1", dz1, pyr.nbr3[l], True, residual=g)
            return d

        def up_back(name, dcat, left, l, g_ext):
            """transposed convolution level l + 1 -> l whose output is the ``left`` columns of ``dcat``'s buffer"""
            return conv_back(name, bn_back(name, dcat[:, :left]), pyr.down[l], False, residual=g_ext)

        def down_back(name, d, l, dskip):
            """stride-2 convolution level l -> l + 1 whose input is also the skip connection with gradient ``dskip``"""
            return conv_back(name, bn_back(name, d), pyr.up[l], False, residual=dskip)

        if gout is None:
            d = torch.zeros(pyr.N, self.PLANES[7], dtype=torch.float32, device=pyr.device)
        else:
            d = gout.float().index_select(0, pyr.perm)            # out = f1[inv]  =>  df1 = dout[perm]
        dskip = []              # by level: the skip half of the concatenation buffer's gradient
        for l, g_ext in enumerate((g2, g4, g8, g16)):
            (conv, _bn, group, _skip), (left, _s) = self._UP[3 - l], self._CAT[l]
            dcat = block_back(group, l, d)
            dskip.append(dcat[:, left:])
            d = up_back(conv, dcat, left, l, g_ext)
        for l in (3, 2, 1, 0):
            conv, _bn, group = self._DOWN[l]
            d = down_back(conv, block_back(group, l + 1, d), l, dskip[l])
        conv_back("conv0p1s1", bn_back("conv0p1s1", d), None, False, need_dx=False)   # feats never requires grad
        return grads

    def forward(self, coords: torch.Tensor, feats: torch.Tensor):
        out, maps = self.run(CoordPyramid(coords), feats)
        return (out, maps) if self.out_fpn else out

    def pyramid(self, coords: torch.Tensor, feats: torch.Tensor, hlevels: Sequence[int] = (0, 1, 2, 3)) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """``[(features [N_level, C_level], parents [N] int64)]`` for every level in ``hlevels + [4]``: the batched form of
        ``PCDMask3DSegLevelEncoder.forward`` (rows of all scenes concatenated; ``parents`` in the caller's voxel order)."""
        pyr = CoordPyramid(coords)
        _out, maps = self.run(pyr, feats)
        return [(maps[h], pyr.parents[h]) for h in list(hlevels) + [4]]
