"""Attention launch policy: every pq3d_attn_fwd / pq3d_attn_bwd call of the package is planned and launched here -- the key-split
factor and its workspace (key_splits, ws_elems: pure, pinned on the CPU by tests/test_attn_plan.py), whether the self-attention
backward may form dO itself (sa_fold_ok), the descriptor (desc) and the two launchers (fwd, bwd) with their work and timer key."""
import math

import torch

from . import _lib as L
from ._lib import BF16, BF16X3


def key_splits(B, H, Lq, Lk, dh, ct, q_dtype, *, bwd, bias, mask, planes=False) -> int:
    """Key-split factor of one call (bias, mask, planes: whether it has them); each rule restates a test of the C++ dispatcher it names.
    INVARIANT: every forward factor depends on the key length ONLY, never on the batch -- a scene's result must not change with how
    scenes are batched or sharded over ranks (tests/test_gpu_fullsize.py).  The backward's may: gradients are summed with atomics anyway."""
    nkb = (Lk + 63) // 64
    if planes:   # pq3d_attn_fwd_x3 (attn_x3.hip): at most 1024 keys per workgroup at d_h = 32, 512 at d_h = 64
        return max(1, -(-nkb // (16 if dh == 32 else 8)))
    # not with dbias.  Measured (tools/probes/attn_bench.py + bench.py): c2 (16 key blocks) and c5 (32) are fastest with 2 splits,
    # c4 (64) with 4 (forward 70 -> 57 us, step 5.56 -> 5.43 ms); 8 only adds combine traffic.
    ks = (1 if nkb < 8 else 2 if nkb < 64 else 4) if not bias else 1
    if not bwd and ct == BF16 and q_dtype == torch.bfloat16 and not bias and not mask and Lq <= 128 <= Lk and dh == 32 and nkb <= 16:
        # pq3d_attn_fwd_resident_try (attn_resident.hip): the all-keys-resident forward holds up to 1024 keys per workgroup: config 2
        # needs no split (and no combine launch).  Longer scenes keep the streaming kernel and its split (measured at config 5,
        # 2048 keys: resident with 2 splits 63-76 us vs streaming 58 us)
        ks = 1
    if bwd and ks > 1 and ct == BF16 and not bias and Lq <= 128 and dh in (32, 64) and \
            (B * H >= 320 or (B * H <= 256 and Lk >= 512 and dh == 32)):
        # pq3d_attn_bwd_resident_try: the all-queries-resident backward runs one workgroup per (scene, head, slice): once the stacked
        # batch alone fills the chip (config 5: 48 x 8) a second slice only adds dQ partials (85 -> 75 us).  At most one workgroup per
        # CU (config 2: 24 x 8): its 8-wave variant (launch_res) takes all keys of a (scene, head) -- no dQ partials, no combine launch.
        ks = 1
    if bwd and ks > 2 and ct == BF16 and not bias and 128 < Lq <= 256 and dh == 32 and B * H * (ks // 2) <= 256 and Lk // (ks // 2) >= 512:
        ks //= 2      # launch_res, the 8-wave resident backward (two query halves, config 4): half the key slices, one workgroup per CU
    if bwd and ct == BF16 and not bias and Lq <= 128 and dh == 64 and nkb >= 16 and B * H * ks < 512:
        # launch_res_dh<64>: d_h = 64 resident backward (4 waves per workgroup, the shipped stage-1 decoder: 12 x 12 (scene, head)
        # pairs, 2048 keys): at least two workgroups per CU -- measured 2 / 4 / 8 / 16 slices: 15.12 / 14.82 / 14.97 / 15.45 ms
        ks = min(8, -(-512 // (B * H)))
    return ks


def ws_elems(ks, B, H, Lq, dh) -> int:
    """fp32 elements of the key-split workspace: per slice and query the partial output row, its running maximum and its sum."""
    return ks * B * H * Lq * (dh + 2) if ks > 1 else 0


def sa_fold_ok(ct, B, H, L_, dm, drop, df, W) -> bool:
    """The split-bf16 self-attention backward kernel (the decoder's in 'bf16' mode) can form dO = df W itself (attn_sa.hip)."""
    if ct != BF16 or dm != 32 * H or dm % 32 or drop is not None or df.dtype != torch.float32 or W.dtype != torch.float32 or \
            not df.is_contiguous() or not W.is_contiguous() or (df.data_ptr() | W.data_ptr()) & 15:
        return False
    # sa32::sa_lds_bytes(Lq, Lk, bwd = true, dm_fold = dm) of attn_sa_body.h restated: (4 LPq + 4 LPk + dm) rows of LDH = 40 bf16,
    # LPk + 2 LPq floats, 16 bytes; both lengths rounded up to 32 here (the kernel rounds LPq to 16): never less than its count
    lp = (L_ + 31) & ~31
    return L_ <= 240 and (4 * lp + 4 * lp + dm) * 40 * 2 + (lp + 2 * lp) * 4 + 16 <= 160 * 1024


def desc(q, k, v, o, lse, H, ct, zero_attn, *, scale=None, kpm=None, mask=None, row_open=None, bias=None, mask_bmod=0, drop=None,
         drop_bmod=0, mask_bits=None, planes=None, grads=None, proj_dout=None):
    """(AttnDesc, workspace or None) of one call on head-packed [B, L, H dh] operands; the caller holds the workspace until the call
    has been enqueued.  grads = (dout, dq, dk, dv, delta, dbias): a backward call; with proj_dout = (g, W) the kernel forms dO = g W
    itself (pq3d_attn_proj, DOUT) and grads[0] is ignored -- the caller checks sa_fold_ok() first.  planes = (k_lo, v_lo, q_bf,
    o_bf): forward only, compute mode 'bf16x3' -- q / o fp32, k / v the hi planes (csrc/attn_x3.hip)."""
    B, Lq, dm = q.shape
    Lk, dh = k.shape[1], dm // H
    d = L.AttnDesc(B=B, H=H, Lq=Lq, Lk=Lk, dh=dh, ct=ct, dt=L.dt_of(q), zero_attn=int(zero_attn), mask_bmod=mask_bmod, drop_bmod=drop_bmod)
    d.scale = 1.0 / math.sqrt(dh) if scale is None else scale
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        assert t.stride(-1) == 1
        setattr(d, name + "_sb", t.stride(0)); setattr(d, name + "_sl", t.stride(1)); setattr(d, name + "_sh", dh)
    d.q, d.k, d.v, d.o, d.lse = map(L.ptr, (q, k, v, o, lse))
    d.kpm, d.mask, d.row_open, d.bias, d.mask_bits = map(L.ptr, (kpm, mask, row_open, bias, mask_bits if mask is not None else None))
    L.set_drop(d.drop, drop)
    if planes is not None:
        assert grads is None and ct == BF16X3 and q.dtype == torch.float32 and k.dtype == torch.bfloat16
        d.k_lo, d.v_lo, d.q_bf, d.o_bf = map(L.ptr, planes)
    if grads is not None:
        d.dout, d.dq, d.dk, d.dv, d.delta, d.dbias = map(L.ptr, grads)
    if proj_dout is not None:
        d.proj.mode, d.proj.dm, d.proj.x, d.proj.w[0] = L.H.PQ3D_ATTN_PROJ_DOUT, dm, L.ptr(proj_dout[0]), L.ptr(proj_dout[1])
    ks = key_splits(B, H, Lq, Lk, dh, ct, q.dtype, bwd=grads is not None, bias=bias is not None, mask=mask is not None,
                    planes=planes is not None)
    ws = torch.empty(ws_elems(ks, B, H, Lq, dh), dtype=torch.float32, device=q.device) if ks > 1 else None
    d.ksplit, d.ws = ks if ks > 1 else 0, L.ptr(ws)
    return d, ws


def _key(d, key_m3) -> str:
    # bench.py's kernel_for parses this key to name the kernel behind a timer entry and checks that against the trace's launch counts
    # (mapping_verified).  The fused decoder pass marks 3-D-mask calls "m3" (key_m3=True: they miss the resident forward);
    # ops.attention's key never carried the mark and stays byte for byte as it was.
    return f"B{d.B}H{d.H}Lq{d.Lq}Lk{d.Lk}dh{d.dh}ct{d.ct}" + ("m3" if key_m3 and d.mask else "")


def fwd(q, k, v, o, lse, H, ct, zero_attn, *, key_m3=False, **kw) -> None:
    """o, lse of one pq3d_attn_fwd call; keywords: desc()."""
    d, ws = desc(q, k, v, o, lse, H, ct, zero_attn, **kw)   # ws: held until the call has been enqueued
    L.call("pq3d_attn_fwd", d, work=(_key(d, key_m3), 4.0 * q.numel() * d.Lk, (q.numel() * 2 + k.numel() * 2) * q.element_size()))


def bwd(q, k, v, o, lse, H, ct, zero_attn, *, key_m3=False, **kw) -> None:
    """dq, dk, dv, delta [, dbias] of one pq3d_attn_bwd call; keywords: desc(), grads among them."""
    d, ws = desc(q, k, v, o, lse, H, ct, zero_attn, **kw)   # ws: as in fwd
    # ALGORITHMIC flops (backward = 2 x forward = 8 B Lq Lk d); the two recompute kernels EXECUTE 14:
    # dQ kernel S, dP, dQ (6) + dK/dV kernel S, dP, dK, dV (8)
    L.call("pq3d_attn_bwd", d, work=(_key(d, key_m3), 8.0 * q.numel() * d.Lk, (q.numel() * 3 + k.numel() * 4) * q.element_size()))
