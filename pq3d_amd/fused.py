"""Fused forward/backward executor for the parallel-structure query decoder (QueryMaskEncoder, query_encoder.py:52-181,
+ MaskHeadSegLevel, mask_head.py:11-57) -- the production fast path.

The modular path (modules.py + ops.py: one autograd Function per kernel) is launch-bound: ~900 dependent dispatches
per config-2 step.  This executor runs the same arithmetic with a hand-written backward so that
  * the M scene memories of a layer are ONE launch each for Q-projection, attention, out-projection, LayerNorm
    (grouped GEMM / memories stacked along the attention batch);
  * K/V projections of every (layer, memory) are hoisted out of the layer loop into ONE grouped GEMM (their inputs
    are layer-invariant), and their backward is one K-concatenated GEMM per gradient;
  * input gradients that sum over consumers are produced by K-concatenated GEMMs / the "+ aux" epilogue instead
    of separate add kernels;
  * every parameter gradient is accumulated (split-K atomics / accumulating column sums) into one flat fp32 arena
    that is zeroed once per backward -- no per-GEMM memsets, no autograd slice/zero/add kernels for the packed
    in_proj weights, and weight sharing across num_blocks accumulates for free.
It is numerically the same computation as the modular path (same kernels, same rounding points).

Both directions of the autograd node (`_FusedDecoder`) are a class holding the state its steps share, with one method per
sublayer step: `_DecoderForward.run` hoists the layer-invariant work and walks the layer applications in order,
`_DecoderBackward.run` walks the tape in reverse; what both derive from the FusedSpec and the inputs is in `_DecoderPass`.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from typing import Dict, List, Optional

import torch
from torch.autograd import Function

from . import _lib as L
from . import arena, attn, ops, wgrad
from .attn import sa_fold_ok
from .ops import ln_bwd as _ln_bwd, ln_fwd as _ln_fwd   # (tests reach them as fused._ln_fwd / fused._ln_bwd)
from .wgrad import _colsum_acc  # noqa: F401  (importable from fused as before: tests/test_gpu_ops.py)
from ._lib import BF16

MAXG = L.MAXG


# one-launch row-local chain (csrc/chain_ffn.hip) for the forward's out-projection + LayerNorm + FFN + LayerNorm; PQ3D_CHAIN=0 or
# fused.set_chain(False) keeps the five launches (same bits: A/B measurements, tests)
_CHAIN = os.environ.get("PQ3D_CHAIN", "1") != "0"


def set_chain(on: bool) -> None:
    global _CHAIN
    _CHAIN = bool(on)


def _chain_on(dev) -> bool:
    """Chains requested AND valid on this device (ops.chain_device_ok: MI355X in SPX mode, round-robin workgroup -> XCD placement measured)."""
    return _CHAIN and ops.chain_device_ok(dev)


def _chain_flag_buf(owner, name, rows, dev):
    """Hand-off words of one chain call site, kept on its owner as attribute `name` (ops.chain_check and the tests read it):
    allocated on first use, again on another device or when too small for `rows` rows."""
    flags = getattr(owner, name, None)
    if flags is None or flags.device != dev or flags.numel() < ((rows + 31) // 32) * 128:
        flags = ops.chain_flags(max(rows, 2048), dev)
        setattr(owner, name, flags)
    return flags


def _gemm_chunks(lists, **kw):
    """L.gemm(**lists, **kw) for list-valued operands of any length: at most MAXG groups per launch."""
    for s in range(0, len(lists["A"]), MAXG):
        L.gemm(**{k: v[s:s + MAXG] for k, v in lists.items()}, **kw)


# one attention sublayer's parameters: W / b = [q, k, v] weights / biases, Wo / bo = out-projection, Wkv = the packed K and V rows
_Proj = namedtuple("_Proj", "W b Wo bo Wkv")
_det = torch.Tensor.detach


def _mha_views(mha, of=lambda p: p):
    """_Proj of a MultiheadAttention-style module: views of of(parameter), never copies -- the parameters' own (not detached)
    by default, the kernels' operands with of=_det, the matching views of the gradient arena with of=_DecoderBackward.G."""
    w, b = of(mha.in_proj_weight), of(mha.in_proj_bias)
    d = w.shape[1]
    return _Proj([w[:d], w[d:2 * d], w[2 * d:]], [b[:d], b[d:2 * d], b[2 * d:]], of(mha.out_proj.weight), of(mha.out_proj.bias),
                 w[d:])


def _sa_views(sa, spatial, of=lambda p: p):
    """_Proj of a self-attention sublayer: MultiHeadAttentionSpatial keeps q / k / v as the Linears w_qs / w_ks / w_vs and the
    out-projection as fc; the plain sublayer is a MultiheadAttention."""
    msa = sa.self_attn
    if not spatial:
        return _mha_views(msa, of)
    return _Proj([of(msa.w_qs.weight), of(msa.w_ks.weight), of(msa.w_vs.weight)],
                 [of(msa.w_qs.bias), of(msa.w_ks.bias), of(msa.w_vs.bias)], of(msa.fc.weight), of(msa.fc.bias), None)


class FusedSpec:
    """Static description of one fused decoder invocation (non-tensor state handed to the Function)."""

    def __init__(self, enc, mh, mems, ct, act, use_self_mask, num_blocks, spatial, mh_count, offline, skip_pred,
                 drop_base=None, mh_drop=False):
        self.enc, self.mh, self.mems, self.ct, self.act = enc, mh, list(mems), ct, act
        self.use_self_mask, self.num_blocks, self.spatial = use_self_mask, num_blocks, spatial
        self.mh_count, self.offline, self.skip_pred = mh_count, offline, skip_pred
        self.stacked_kpm = None      # optional [M, B, Ns] key-padding masks of the memories, stacked (set by fused_decoder)
        # memory inputs are passed as U unique source tensors: src[i][j] = source of memory j in layer i (a multi-scale
        # voxel memory has one source per layer, query_encoder.py:90-91), mh_src[k] = source of mask-head memory k
        # (the LAST scale of a multi-scale memory, query3d_unified.py:163-165)
        self.src, self.mh_src, self.n_src = None, None, len(self.mems)
        self.prompt = False          # structure 'mixed': a sequential prompt cross-attention follows the parallel scene memories
        self.kv3 = False             # compute mode 'bf16x3': split-bf16 key/value side (set by fused_decoder)
        self.drop_base = drop_base   # dropout-site base of the encoder when train-mode dropout is active, else None
        self.mh_drop = mh_drop       # mask head's cls_head dropout active

    def drop(self, module, app, kind, device, m=0):
        """Dropout site of `module` (its own p) at layer application `app`, or None when dropout is off."""
        if self.drop_base is None or not (module.dropout_p > 0.0):
            return None
        return ops.make_drop(module.dropout_p, ops.drop_site(self.drop_base, app, kind, m), device)


def _mh_forward(spec, x, keys, inv_den, seg_pad, rec, call):
    """One MaskHeadSegLevel call (number `call` of this forward) on the fused path; returns (cls, mlog, amask)."""
    mh = spec.mh
    ct = ops.small_ct(spec.ct)     # query-side GEMMs: split-bf16 in 'bf16' mode (fp32 operands and outputs)
    ad = ops.act_dtype(ct)
    B, Nq, d = x.shape
    R = B * Nq
    c0, c2, c4 = mh.cls_head[0], mh.cls_head[2], mh.cls_head[4]
    Mm = len(keys)
    mps = list(mh.mask_pred_list)[:Mm]
    Ns = keys[0].shape[1]
    hdrop = None
    if _chain_on(x.device) and ct == L.BF16X3 and not spec.mh_drop and x.dtype == torch.float32 and x.is_contiguous() and \
            ops.chain_mh_ok(d, c0.out_features, c4.out_features, Mm, R) and c4.bias is not None:
        # the row-local part (class MLP + the mask predictions' query projections) in one launch (csrc/chain_mh.hip)
        flags = _chain_flag_buf(mh, "_chain_flags", 2048, x.device)
        colfill = mh._foc_flags if mh._foc_cols.numel() else None
        h1, h2, mean, rstd, cls, qm = ops.chain_mh_fwd(
            x, c0.weight.detach(), c0.bias.detach(), c2.weight.detach(), c2.bias.detach(), c2.eps, c4.weight.detach(),
            c4.bias.detach(), colfill, float("-inf"), [mp.q_proj.weight.detach() for mp in mps],
            [mp.q_proj.bias.detach() for mp in mps], flags)
    else:
        h1 = torch.empty(B, Nq, c0.out_features, dtype=torch.float32, device=x.device)
        L.gemm(M=R, N=c0.out_features, K=d, A=[x], B=[c0.weight.detach()], bias=[c0.bias.detach()], Cs=[h1], ct=ct,
               lda=d, ldb=d, ldc=c0.out_features, act="relu")
        h2, mean, rstd = _ln_fwd(None, [h1], [c2.weight.detach()], [c2.bias.detach()], c2.eps, None, Nq)
        if spec.mh_drop:   # nn.Dropout between LayerNorm and the classifier (utils.py:23), site (mask-head base, call)
            hdrop = ops.make_drop(mh.dropout_p, ops.drop_site(mh._drop_base, call, ops.DROP_MLP_HEAD), x.device)
            h2 = ops._dropout_apply(h2, hdrop)
        C_ = c4.out_features
        cls_raw = torch.empty(B, Nq, C_, dtype=torch.float32, device=x.device)
        L.gemm(M=R, N=C_, K=c0.out_features, A=[h2], B=[c4.weight.detach()], bias=[c4.bias.detach()], Cs=[cls_raw], ct=ct,
               lda=c0.out_features, ldb=c0.out_features, ldc=C_)
        cls = cls_raw
        if mh._foc_cols.numel():
            cls = torch.empty_like(cls_raw)
            L.call("pq3d_fill_cols", cls_raw, cls, R, C_, mh._foc_cols, mh._foc_cols.numel(), float("-inf"))
        qm = torch.empty(Mm, B, Nq, d, dtype=ad, device=x.device)
        L.gemm(M=R, N=d, K=d, A=[x] * Mm, B=[mp.q_proj.weight.detach() for mp in mps],
               bias=[mp.q_proj.bias.detach() for mp in mps], Cs=[qm[m] for m in range(Mm)], ct=ct, lda=d, ldb=d, ldc=d)
    mlog = torch.empty(B, Ns, Nq, dtype=torch.float32, device=x.device)
    amask = torch.empty(B, Nq, Ns, dtype=torch.bool, device=x.device)
    L.gemm(M=Ns, N=Nq, K=d, A=list(keys), B=[qm[m] for m in range(Mm)], Cs=[mlog] + [None] * (Mm - 1), ct=ct, lda=d,
           ldb=d, ldc=Nq, batch=B, strideA=Ns * d, strideB=Nq * d, strideC=Ns * Nq, kconcat=Mm, row_scale=inv_den,
           row_fill_flag=seg_pad, row_fill=-1e6, mask_out=amask)
    rec.update(mh_x=x.detach(), mh_h1=h1, mh_h2=h2, mh_mean=mean, mh_rstd=rstd, mh_qm=qm, mh_drop=hdrop)
    return cls, mlog, amask


def _attn(q, k, v, o, lse, H, ct, zero_attn, bwd=None, **kw):
    """One attention launch of the fused pass: forward, or backward with bwd = (dout, dq, dk, dv, delta, dbias); keywords: attn.desc."""
    (attn.fwd if bwd is None else attn.bwd)(q, k, v, o, lse, H, ct, zero_attn, key_m3=True, grads=bwd, **kw)


class _PendingDx:
    """Upstream gradient of a layer application that the NEXT backward chain launch forms itself (csrc/chain_ffn_bwd.hip, step 0):
    sum_m dq_m Wq_m + dxr."""
    __slots__ = ("dq_all", "Wqs", "dxr", "gq")

    def __init__(self, dq_all, Wqs, dxr, gq):
        self.dq_all, self.Wqs, self.dxr, self.gq = dq_all, Wqs, dxr, gq


class _DecoderPass:
    """What both directions of one fused decoder invocation derive from its FusedSpec and inputs: compute types, sizes, the
    memories' source maps (src[i][j], mh_src[k]: see FusedSpec), the cross-attention modules cas[i][j] of the M scene memories
    (pcas[i]: the prompt memory's) per layer and detached views of the attention weights (caw / pcw / saw, _Proj each)."""

    def __init__(self, spec, qpos, Ns):
        self.spec = spec
        self.enc, self.ct = enc, ct = spec.enc, spec.ct
        self.ad = ops.act_dtype(ct)
        self.layers = layers = list(enc.unified_encoder)
        self.Ln, self.H = Ln, _ = len(layers), enc.num_heads
        self.B, self.Nq, self.d = B, Nq, _ = qpos.shape
        self.Ns = Ns
        self.R, self.Rk, self.dev = B * Nq, B * Ns, qpos.device
        self.M, self.U = M, _ = len(spec.mems), spec.n_src
        self.src = spec.src if spec.src is not None else [list(range(M)) for _ in range(Ln)]
        self.mh_src = spec.mh_src if spec.mh_src is not None else list(range(M))
        mem_idx = [layers[0].memories.index(m) for m in spec.mems]
        self.cas = [[layer.cross_attn_list[j] for j in mem_idx] for layer in layers]
        self.pcas = [layer.memory2ca["prompt"] for layer in layers] if spec.prompt else None
        self.caw = [[_mha_views(ca.multihead_attn, _det) for ca in cl] for cl in self.cas]
        self.pcw = [_mha_views(pc.multihead_attn, _det) for pc in self.pcas] if spec.prompt else None
        self.saw = [_sa_views(layer.self_attn, spec.spatial, _det) for layer in layers]

    def ca_mask_kw(self, rec):
        """Mask keywords of a layer application's cross-attention launch (forward and backward): the per-query attention mask
        of that application (shared by the M memories stacked along the batch: mask_bmod) or the memories' key-padding masks."""
        if self.spec.use_self_mask:
            return dict(mask=rec["attn_mask"], row_open=rec["row_open"], mask_bmod=self.B, mask_bits=rec["mask_bits"])
        return dict(kpm=self.kpm_all)


class _DecoderBackward(_DecoderPass):
    """One backward pass of the fused decoder: the state every sublayer step shares (saved tensors, sizes, the gradient
    arena, the deferred weight-gradient queue, the K/V gradient buffers) and one method per step, run in reverse order of the
    forward: mask head -> FFN -> self-attention -> (prompt cross-attention) -> cross-attention over the scene memories, per
    layer application; then the hoisted K/V projections' backward.  `_FusedDecoder.backward` is `_DecoderBackward(...).run()`."""

    def __init__(self, ctx, dxf, dheads):
        self.ctx, self.dxf, self.tape = ctx, dxf, ctx.tape
        spec = ctx.spec
        U, M = spec.n_src, len(spec.mems)
        sv = ctx.saved_tensors
        self.x0, self.qpos, self.qmask, self.pos, self.pl, self.seg_pad, self.coef = sv[:7]
        self.feats, self.masks = list(sv[7:7 + U]), list(sv[7 + U:7 + U + M])
        super().__init__(spec, self.qpos, self.feats[0].shape[1])
        B, d, Ns, dev = self.B, self.d, self.Ns, self.dev
        self.params = ctx.params
        self.KV, self.kpm_all = ctx.KV, ctx.kpm_all
        self.n_mh = n_mh = ctx.n_mh
        self.dcls, self.dmlog = list(dheads[:n_mh]), list(dheads[n_mh:2 * n_mh])
        self.n_app = n_app = len(self.tape)
        self._open_arena()   # self.gv (parameter -> gradient view), self.accumulate, self.in_place, self.dxr_zero
        G = self.G           # views of the gradient arena that match caw / pcw / saw
        self.cag = [[_mha_views(ca.multihead_attn, G) for ca in cl] for cl in self.cas]
        self.pcg = [_mha_views(pc.multihead_attn, G) for pc in self.pcas] if spec.prompt else None
        self.sag = [_sa_views(layer.self_attn, spec.spatial, G) for layer in self.layers]
        self.dwq = wgrad.Queue(split_x2=False)
        self.sb_queue = []   # (W, b, d bias, dW, db) of every spatial self-attention application
        self.dqpos_parts: List[torch.Tensor] = []
        self.dKV = torch.empty(n_app, 2, M, B, Ns, d, dtype=self.ad, device=dev)
        self.dPKV = torch.empty(n_app, 2, B, ctx.prompt.shape[1], d, dtype=self.ad, device=dev) if spec.prompt else None
        self._mh_calls, self._mh_pre, self._mh_dcl = 0, None, None   # mask_head_chain(): per-pass buffers shared by its calls
        self.dkeys = None    # accumulated gradient of the mask-head key projections [Mm,B,Ns,d] fp32->ad
        self.dk_terms = []   # queued (g, q_m) terms of it (one K-concatenated launch at the end)
        ready_cb = getattr(self.enc, "grads_ready", None) if self.in_place else None   # only when the owner's buffers were written
        self.per_layer = bool(getattr(self.enc, "grad_bucket_per_layer", False)) and ready_cb is not None
        if ready_cb is not None:
            def ready(tag):
                # weight gradients queued by ops.linear layers that ran backward BEFORE the decoder (heads)
                # must be in their slots before an owner is told that a bucket is final
                arena.dw_deferred_flush()
                ready_cb(tag)
        else:
            ready = lambda tag: None
        self.ready = ready
        # the output heads consume the decoder's outputs, so their backward has run when this one starts (the reference:
        # query3d_unified.py:193-218): whatever they wrote into their arena slots is final now -- an owner may start that
        # bucket's all-reduce under the whole decoder backward (config 5: the caption body's 240 MB)
        ready("heads")

    def _open_arena(self):
        """Gradient arena: every parameter gradient of the decoder is a view of a flat zeroed fp32 buffer (the data-parallel
        reducer's / optimizer's, or one of this pass); arena.open_decoder decides fresh vs accumulating pass."""
        enc, M = self.enc, self.M
        # input gradients of the M-branch cross-attention LayerNorms are accumulated with atomics by the M branch blocks; that
        # buffer and the gradient arena are zeroed by ONE launch for the whole backward
        self.dxr_zero = torch.empty(self.n_app, self.B, self.Nq, self.d, dtype=torch.float32, device=self.dev) if M > 1 else None
        self.gv, self.accumulate, self.in_place = arena.open_decoder(
            getattr(enc, "grad_arena", None), getattr(enc, "grad_arena_buffers", ()), self.params, self.dxr_zero)

    def G(self, p):
        return self.gv[id(p)]

    def mask_head(self, rec, dc, dm, dx_in):
        """Backprop one mask-head call; returns dx_in + its contribution to d(query)."""
        cur = dx_in
        if self.mask_head_chain_ok(rec, dc, dm, cur):
            return self.mask_head_chain(rec, dc, dm, cur)
        ctx, spec, ct, ad, B, Nq, d, Ns = self.ctx, self.spec, self.ct, self.ad, self.B, self.Nq, self.d, self.Ns
        R, dev, G, dwq, seg_pad = self.R, self.dev, self.G, self.dwq, self.seg_pad
        mh = spec.mh
        c0, c2, c4 = mh.cls_head[0], mh.cls_head[2], mh.cls_head[4]
        x_in = rec["mh_x"]
        Hd, C_ = c0.out_features, c4.out_features
        assert not isinstance(cur, _PendingDx)
        if dc is not None:
            dcl = dc.contiguous()
            if mh._foc_cols.numel():
                t = torch.empty_like(dcl)
                L.call("pq3d_fill_cols", dcl, t, R, C_, mh._foc_cols, mh._foc_cols.numel(), 0.0)
                dcl = t
            dh2 = torch.empty(B, Nq, Hd, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=Hd, K=C_, A=[dcl], B=[c4.weight.detach()], Cs=[dh2], ct=ct, lda=C_, ldb=Hd, ldc=Hd, transB=True)
            dwq.add([dcl], [rec["mh_h2"]], None, [G(c4.weight)], ct, [G(c4.bias)])
            if rec.get("mh_drop") is not None:
                dh2 = ops._dropout_apply(dh2, rec["mh_drop"])
            _, dh1 = _ln_bwd(None, [rec["mh_h1"]], [c2.weight.detach()], [c2.bias.detach()], c2.eps, None, Nq,
                             rec["mh_mean"], rec["mh_rstd"], dh2, [G(c2.weight)], [G(c2.bias)])
            dpre = ops.act_bwd(dh1[0], rec["mh_h1"], "relu", ad)
            nxt = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=d, K=Hd, A=[dpre], B=[c0.weight.detach()], Cs=[nxt], aux=[cur], act_grad="add", ct=ct,
                   lda=Hd, ldb=d, ldc=d, transB=True)
            dwq.add([dpre], [x_in], None, [G(c0.weight)], ct, [G(c0.bias)])
            cur = nxt
        if dm is not None:
            Mm = spec.mh_count
            mps = list(mh.mask_pred_list)[:Mm]
            qm = rec["mh_qm"]
            g = ops.scale_rows(dm.contiguous(), B * Ns, ad, scale=ctx.inv_den, zero_flag=seg_pad)
            self.add_dkeys(g, qm)
            dqm = self.mh_dqm(g)
            nxt = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=d, K=d, A=[dqm[m] for m in range(Mm)], B=[mp.q_proj.weight.detach() for mp in mps],
                   Cs=[nxt] + [None] * (Mm - 1), aux=[cur] + [None] * (Mm - 1), act_grad="add", ct=ct, lda=d, ldb=d,
                   ldc=d, transB=True, kconcat=Mm)
            dwq.add([dqm[m] for m in range(Mm)], [x_in] * Mm, None, [G(mp.q_proj.weight) for mp in mps], ct,
                    [G(mp.q_proj.bias) for mp in mps])
            cur = nxt
        return cur

    def add_dkeys(self, g, qm):
        """d keys = sum over the mask-head calls of g_c @ q_m,c: nothing consumes it before the end of the backward, so the
        terms are queued and formed by ONE K-concatenated launch there (each call used to re-read and re-write the
        [Mm, B, Ns, d] fp32 sum through the "+ aux" epilogue: 100 MB per call at config 4)."""
        B, Nq, d, Ns, Mm = self.B, self.Nq, self.d, self.Ns, self.spec.mh_count
        if Mm * (len(self.dk_terms) + 1) <= MAXG:
            self.dk_terms.append((g, qm))
            return
        newk = torch.empty(Mm, B, Ns, d, dtype=torch.float32, device=self.dev)
        L.gemm(M=Ns, N=d, K=Nq, A=[g] * Mm, B=[qm[m] for m in range(Mm)], Cs=[newk[m] for m in range(Mm)],
               aux=[self.dkeys[m] for m in range(Mm)] if self.dkeys is not None else None,
               act_grad="add" if self.dkeys is not None else None, ct=self.ct, lda=Nq, ldb=d, ldc=d, transB=True, batch=B,
               strideA=Ns * Nq, strideB=Nq * d, strideC=Ns * d)
        self.dkeys = newk

    def mh_dqm(self, g):
        """Query-side gradient of one call's mask logits, g^T keys: [Nq x d] outputs per (memory, scene) over a reduction of Ns
        segments: few tiles, long K -> split-K into an fp32 buffer once Ns is large (c4: 192 workgroups x 64 k-tiles otherwise)."""
        B, Nq, d, Ns, Mm = self.B, self.Nq, self.d, self.Ns, self.spec.mh_count
        sk = min(8, Ns // 512) if Ns >= 1024 else 1
        dqm = torch.empty(Mm, B, Nq, d, dtype=torch.float32 if sk > 1 else self.ad, device=self.dev)
        L.gemm(M=Nq, N=d, K=Ns, A=[g] * Mm, B=list(self.ctx.keys), Cs=[dqm[m] for m in range(Mm)], ct=self.ct, lda=Nq, ldb=d, ldc=d,
               transA=True, transB=True, batch=B, strideA=Ns * Nq, strideB=Ns * d, strideC=Nq * d, splitk=sk)
        return dqm

    def mask_head_chain_ok(self, rec, dc, dm, cur) -> bool:
        mh = self.spec.mh
        c0, c4 = mh.cls_head[0], mh.cls_head[4]
        if isinstance(cur, _PendingDx):
            cur = cur.dxr
        return (dc is not None and dm is not None and _chain_on(self.dev) and self.ct == BF16 and self.ad == torch.bfloat16 and
                rec.get("mh_drop") is None and ops.chain_mh_ok(self.d, c0.out_features, c4.out_features, self.spec.mh_count, self.R)
                and rec["mh_h1"].dtype == torch.float32 and isinstance(cur, torch.Tensor) and cur.dtype == torch.float32
                and cur.is_contiguous())

    def _mh_logit_grads(self):
        """{id(rec): (g, dqm)} of every mask-head call of the pass: the query-side gradient of the mask logits, dqm_c =
        g_c^T keys, depends on the loss' gradient of that call's logits and on the keys only -- not on anything the backward
        pass computes -- so the products of ALL calls are formed by ONE launch when the first call runs backward (config 4: 5
        launches of 31-34 us -> one of ~105; their split-K outputs are one buffer zeroed by one launch)."""
        if self._mh_pre is not None:
            return self._mh_pre
        ctx, spec, ct, ad, B, Nq, d, Ns, dev = self.ctx, self.spec, self.ct, self.ad, self.B, self.Nq, self.d, self.Ns, self.dev
        Mm = spec.mh_count
        calls = []
        if ctx.final_rec is not None:
            calls.append((ctx.final_rec, self.dcls[-1], self.dmlog[-1]))
        if spec.mh is not None and not spec.skip_pred:
            calls += [(self.tape[a], self.dcls[a], self.dmlog[a]) for a in range(self.n_app - 1, -1, -1)]
        calls = [(r_, dm_) for r_, dc_, dm_ in calls if self.mask_head_chain_ok(r_, dc_, dm_, self.qpos)]   # (qpos: any fp32 rows)
        self._mh_pre = {}
        per = max(1, MAXG // max(Mm, 1))
        if not calls or Mm < 1:
            return self._mh_pre
        sk = min(8, Ns // 512) if Ns >= 1024 else 1
        buf = torch.empty(len(calls), Mm, B, Nq, d, dtype=torch.float32 if sk > 1 else ad, device=dev)
        if sk > 1:
            ops.zero_many([buf])   # split-K partial sums are added into the outputs
        gs = ops.scale_rows_many([dm_ for _r, dm_ in calls], B * Ns, ad, scale=ctx.inv_den, zero_flag=self.seg_pad)   # one launch
        for c0_ in range(0, len(calls), per):
            idx = range(c0_, min(c0_ + per, len(calls)))
            L.gemm(M=Nq, N=d, K=Ns, A=[gs[c_] for c_ in idx for _m in range(Mm)], B=list(ctx.keys) * len(idx),
                   Cs=[buf[c_, m] for c_ in idx for m in range(Mm)], ct=ct, lda=Nq, ldb=d, ldc=d, transA=True, transB=True, batch=B,
                   strideA=Ns * Nq, strideB=Ns * d, strideC=Nq * d, splitk=sk, accumulate=sk > 1)
        for c_, (r_, _dm) in enumerate(calls):
            self._mh_pre[id(r_)] = (gs[c_], buf[c_])
        return self._mh_pre

    def mask_head_chain(self, rec, dc, dm, cur):
        """mask_head() with the row-local steps in one launch (csrc/chain_mh.hip): the mask logits' query-side gradient first
        (not row-local: a reduction over the scene's segments), then class-MLP backward + both input-gradient products."""
        ctx, spec, ct, ad, seg_pad, B = self.ctx, self.spec, self.ct, self.ad, self.seg_pad, self.B
        Nq, Ns, dev, G, dwq = self.Nq, self.Ns, self.dev, self.G, self.dwq
        mh, Mm, x_in, qm = spec.mh, spec.mh_count, rec["mh_x"], rec["mh_qm"]
        c0, c2, c4 = mh.cls_head[0], mh.cls_head[2], mh.cls_head[4]
        mps = list(mh.mask_pred_list)[:Mm]
        pre = self._mh_logit_grads().get(id(rec))
        g = pre[0] if pre is not None else ops.scale_rows(dm.contiguous(), B * Ns, ad, scale=ctx.inv_den, zero_flag=seg_pad)
        self.add_dkeys(g, qm)
        call = self._mh_calls
        self._mh_calls += 1
        dqm = pre[1] if pre is not None else self.mh_dqm(g)
        if self._mh_dcl is None and mh._foc_cols.numel():   # adjacent rows call after call: their column sums (the bias
            self._mh_dcl = torch.empty(self.n_mh, B, Nq, c4.out_features, dtype=torch.float32, device=dev)   # gradient) in one launch
        flags = _chain_flag_buf(mh, "_chain_flags_bwd", 2048, dev)
        dcl, dpre, out = ops.chain_mh_bwd(
            dc.contiguous(), mh._foc_flags if mh._foc_cols.numel() else None, c4.weight.detach(), rec["mh_h1"], rec["mh_mean"],
            rec["mh_rstd"], c2.weight.detach(), G(c2.weight), G(c2.bias), c0.weight.detach(),
            None if isinstance(cur, _PendingDx) else cur,
            [dqm[m] for m in range(Mm)], [mp.q_proj.weight.detach() for mp in mps], flags,
            dcl_out=self._mh_dcl[call] if self._mh_dcl is not None else None,
            prev=(cur.dq_all, cur.Wqs, cur.dxr, cur.gq) if isinstance(cur, _PendingDx) else None)
        dwq.add([dcl], [rec["mh_h2"]], None, [G(c4.weight)], ct, [G(c4.bias)])
        dwq.add([dpre], [x_in], None, [G(c0.weight)], ct, [G(c0.bias)])
        dwq.add([dqm[m] for m in range(Mm)], [x_in] * Mm, None, [G(mp.q_proj.weight) for mp in mps], ct,
                [G(mp.q_proj.bias) for mp in mps])
        return out

    def kv_terms(self, apps, into_queue):
        """(dK|dV, W) operand lists of the hoisted K/V projections' backward for the applications `apps`; with
        into_queue their weight / bias gradient products are queued."""
        ctx, tape, ct, src, dwq, dKV, dPKV = self.ctx, self.tape, self.ct, self.src, self.dwq, self.dKV, self.dPKV
        A_, B_, Xf, X2, GWs, Gbs = [], [], [], [], [], []
        for a_ in apps:
            i_ = tape[a_]["i"]
            for j, (cw, cg) in enumerate(zip(self.caw[i_], self.cag[i_])):
                A_ += [dKV[a_, 0, j], dKV[a_, 1, j]]
                B_ += cw.W[1:]
                Xf += [ctx.kin[src[i_][j]], ctx.vin[src[i_][j]]]
                X2 += [ctx.kin2[src[i_][j]], None]
                GWs += cg.W[1:]
                Gbs += cg.b[1:]
        if into_queue:
            dwq.add(A_, Xf, X2, GWs, ct, Gbs)
            if self.spec.prompt:   # the prompt memory's K / V rows of its cross-attention's in_proj weights
                for a_ in apps:
                    pg = self.pcg[tape[a_]["i"]]
                    dwq.add([dPKV[a_, 0], dPKV[a_, 1]], [ctx.prompt, ctx.prompt], None, pg.W[1:], ct, pg.b[1:])
        return A_, B_

    def flush_spatial(self):
        pl, H, B, Nq, sb_queue = self.pl, self.H, self.B, self.Nq, self.sb_queue
        for i0 in range(0, len(sb_queue), MAXG):
            chunk = sb_queue[i0:i0 + MAXG]
            arrs = [L.parr([t[k] for t in chunk]) for k in range(5)]
            L.call("pq3d_spatial_bias_bwd_grouped", pl, *arrs, len(chunk), B, H, Nq)
        del sb_queue[:]

    def ffn(self, rec, layer, dx):
        """FFN sublayer: returns d(x2), the gradient of the sublayer's input (residual + linear1 path)."""
        spec, ct, ad, B, Nq, d, R, dev, G, dwq = self.spec, self.ct, self.ad, self.B, self.Nq, self.d, self.R, self.dev, self.G, self.dwq
        x2 = rec["x2"]
        # ---------------- FFN backward
        ffn = layer.ffn
        F_ = ffn.linear1.out_features
        # dx2r = residual-branch gradient, dy = (dropout-masked) gradient of the linear2 output (sum of the partials)
        dx2r, dy = _ln_bwd(x2, [rec["z"]], [ffn.norm.weight.detach()], [ffn.norm.bias.detach()], ffn.norm.eps, None, Nq,
                           rec["mean_f"][:1], rec["rstd_f"][:1], dx, [G(ffn.norm.weight)], [G(ffn.norm.bias)],
                           drop=rec["dr_fr"])
        dy = dy[0]
        dhp = torch.empty(B, Nq, F_, dtype=ad, device=dev)
        # inner dropout.  ReLU: the saved h is post-dropout, so [h > 0] already carries the keep-mask and only the
        # 1/(1-p) factor is left -> alpha.  GELU (round 3): the epilogue regenerates the forward's mask on the incoming
        # gradient (same site, same [R, F] indices) before multiplying by gelu'(pre) -- epi_row's order: dropout, then
        # the activation gradient
        relu = spec.act != "gelu"
        L.gemm(M=R, N=F_, K=d, A=[dy], B=[ffn.linear2.weight.detach()], Cs=[dhp],
               aux=[rec["h"] if relu else rec["pre"]], act_grad=spec.act, ct=ct, lda=d, ldb=F_, ldc=F_,
               transB=True, alpha=1.0 / (1.0 - rec["dr_fi"].p) if (rec["dr_fi"] is not None and relu) else 1.0,
               drop=rec["dr_fi"] if not relu else None)
        dwq.add([dy], [rec["h"]], None, [G(ffn.linear2.weight)], ct, [G(ffn.linear2.bias)])
        dx2 = dx2r   # dx2 = dx2r + dhp W1: split-K accumulated in place onto the residual-branch gradient
        L.gemm(M=R, N=d, K=F_, A=[dhp], B=[ffn.linear1.weight.detach()], Cs=[dx2], ct=ct, lda=F_, ldb=d, ldc=d,
               transB=True, splitk=4, accumulate=True)
        dwq.add([dhp], [x2], None, [G(ffn.linear1.weight)], ct, [G(ffn.linear1.bias)])
        return dx2

    def sa_chain_ok(self, rec) -> bool:
        """q / k / v input gradients + merged LayerNorm backward + cross-attention d O as one launch (csrc/chain_sa_bwd.hip)."""
        return (_chain_on(self.dev) and self.ct == BF16 and self.ad == torch.bfloat16 and not self.spec.prompt and rec["dr_cr"] is None
                and ops.chain_ca_ok(self.R, self.d, self.M) and rec["op_all"].dtype == torch.float32)

    def ffn_chain_ok(self, rec, layer, dx) -> bool:
        """The FFN backward + the self-attention post-norm backward can run as ONE launch (csrc/chain_ffn_bwd.hip)."""
        ffn = layer.ffn
        return (_chain_on(self.dev) and self.ct == BF16 and self.ad == torch.bfloat16 and self.spec.act == "relu" and isinstance(dx, (torch.Tensor, _PendingDx))
                and rec["dr_fr"] is None and rec["dr_fi"] is None and rec["dr_sr"] is None and rec["h"].dtype == torch.float32
                and ops.chain_ffn_ok(self.R, self.d, ffn.linear1.out_features))

    def ffn_chain(self, rec, layer, dx):
        """FFN sublayer + the self-attention post-norm in one launch: returns (dx1r, df), both the same gradient (no dropout);
        queues the two weight-gradient products of the FFN exactly as ffn() does."""
        ct, G, dwq = self.ct, self.G, self.dwq
        ffn, sa = layer.ffn, layer.self_attn
        flags = _chain_flag_buf(self.enc, "_chain_flags_bwd", 2048, self.dev)
        prev = (dx.dq_all, dx.Wqs, dx.dxr, dx.gq) if isinstance(dx, _PendingDx) else None
        dy, dhp, df = ops.chain_ffn_bwd(
            None if prev is not None else dx.contiguous(), rec["x2"], rec["z"], ffn.norm.weight.detach(), rec["mean_f"][:1], rec["rstd_f"][:1], G(ffn.norm.weight),
            G(ffn.norm.bias), ffn.linear2.weight.detach(), rec["h"], ffn.linear1.weight.detach(), rec["x1s"], rec["f"],
            sa.norm.weight.detach(), rec["mean_s"], rec["rstd_s"], G(sa.norm.weight), G(sa.norm.bias), flags, prev=prev)[:3]
        dwq.add([dy], [rec["h"]], None, [G(ffn.linear2.weight)], ct, [G(ffn.linear2.bias)])
        dwq.add([dhp], [rec["x2"]], None, [G(ffn.linear1.weight)], ct, [G(ffn.linear1.bias)])
        return df, df

    def self_attn(self, rec, layer, dx2, pre=None):
        """Self-attention sublayer: returns the three addends of d(x1s) (from q, from k, from v + residual)."""
        spec, ct, qpos, H, B, Nq, d = self.spec, self.ct, self.qpos, self.H, self.B, self.Nq, self.d
        R, dev, G, dwq = self.R, self.dev, self.G, self.dwq
        # ---------------- self-attention backward
        sa = layer.self_attn
        sw, sg = self.saw[rec["i"]], self.sag[rec["i"]]
        Wl, Wo = sw.W, sw.Wo
        x1s = rec["x1s"]    # the self-attention sublayer's input (x1, or the prompt cross-attention's output)
        if pre is not None:   # formed by the chain launch (ffn_chain)
            dx1r, df = pre
        else:
            dx1r, df = _ln_bwd(x1s, [rec["f"]], [sa.norm.weight.detach()], [sa.norm.bias.detach()], sa.norm.eps, None, Nq,
                               rec["mean_s"], rec["rstd_s"], dx2, [G(sa.norm.weight)], [G(sa.norm.bias)],
                               drop=rec["dr_sr"])
            df = df[0]
        fold = sa_fold_ok(ct, B, H, Nq, d, rec["dr_sa"], df, Wo)
        do_s = None
        if not fold:
            do_s = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=d, K=d, A=[df], B=[Wo], Cs=[do_s], ct=ct, lda=d, ldb=d, ldc=d, transB=True)
        dwq.add([df], [rec["o_s"]], None, [sg.Wo], ct, [sg.bo])
        qkv = rec["qkv"]
        dqkv = torch.empty(3, B, Nq, d, dtype=torch.float32, device=dev)
        delta = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)
        dsb = torch.empty_like(rec["sbias"]) if spec.spatial else None
        _attn(qkv[0], qkv[1], qkv[2], rec["o_s"], rec["lse_s"], H, ops.sa_ct(ct), False, kpm=self.qmask, bias=rec["sbias"],
              bwd=(do_s, dqkv[0], dqkv[1], dqkv[2], delta, dsb), drop=rec["dr_sa"],
              proj_dout=(df, Wo) if fold else None)
        if spec.spatial:   # deferred: one grouped launch for all layer applications at the end of the backward
            fc = sa.self_attn.pairwise_loc_fc
            self.sb_queue.append((fc.weight.detach(), fc.bias.detach(), dsb, G(fc.weight), G(fc.bias)))
        # d(x1 + qpos) from q and k, d(x1) from v (+ the residual-branch gradient): three independent products, ONE
        # launch; their sum is formed by the consumer (the next LayerNorm backward reads three addends) instead of
        # by a second, dependent "+ aux" launch
        self._sa_chain = None
        if self.sa_chain_ok(rec):
            # these products, the merged cross-attention post-norm backward and the cross-attention d O in ONE launch
            # (csrc/chain_sa_bwd.hip); cross_attn() picks the results up
            cl = self.cas[rec["i"]]
            flags = _chain_flag_buf(self.enc, "_chain_flags_sab", 2048, dev)
            a_ = self._cur_app
            g3, dop, dxr, do_all = ops.chain_sa_bwd(
                dqkv, [w_.contiguous() for w_ in Wl], dx1r, rec["x_in"], rec["op_all"], [ca.norm.weight.detach() for ca in cl],
                rec["mean_c"], rec["rstd_c"], self.coef[a_] if self.coef is not None else None, Nq, [G(ca.norm.weight) for ca in cl],
                [G(ca.norm.bias) for ca in cl], [cw.Wo for cw in self.caw[rec["i"]]], flags)
            self._sa_chain = (dxr, dop, do_all)
        else:
            g3 = torch.empty(3, B, Nq, d, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=d, K=d, A=[dqkv[0], dqkv[1], dqkv[2]], B=list(Wl), Cs=[g3[0], g3[1], g3[2]],
                   aux=[None, None, dx1r], act_grad="add", ct=ct, lda=d, ldb=d, ldc=d, transB=True)
        self.dqpos_parts += [g3[0], g3[1]]
        dwq.add([dqkv[0], dqkv[1], dqkv[2]], [x1s] * 3, [qpos, qpos, None], sg.W, ct, sg.b)
        return [g3[0], g3[1], g3[2]]

    def prompt_cross_attn(self, a, rec, dx1):
        """structure 'mixed': the prompt memory's sequential cross-attention; dx1 is d(x1s), returns d(x1)."""
        ctx, ct, ad, qpos, H, B, Nq, d = self.ctx, self.ct, self.ad, self.qpos, self.H, self.B, self.Nq, self.d
        R, dev, G, dwq, dPKV = self.R, self.dev, self.G, self.dwq, self.dPKV
        i, x1 = rec["i"], rec["x1"]
        # ---------------- prompt cross-attention backward (sequential, single memory): dx1 is d(x1s) here
        pc, pw, pg = self.pcas[i], self.pcw[i], self.pcg[i]
        dx1pr, dopp = _ln_bwd(x1, [rec["opp"]], [pc.norm.weight.detach()], [pc.norm.bias.detach()], pc.norm.eps, None,
                              Nq, rec["mean_p"], rec["rstd_p"], dx1, [G(pc.norm.weight)], [G(pc.norm.bias)],
                              drop=rec["dr_pr"])
        do_p = torch.empty(B, Nq, d, dtype=ad, device=dev)
        L.gemm(M=R, N=d, K=d, A=[dopp[0]], B=[pw.Wo], Cs=[do_p], ct=ct, lda=d, ldb=d, ldc=d, transB=True)
        dwq.add([dopp[0]], [rec["o_p"]], None, [pg.Wo], ct, [pg.bo])
        dq_p = torch.empty(B, Nq, d, dtype=ad, device=dev)
        delta_p = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)
        _attn(rec["qp"], ctx.PKV[i, 0], ctx.PKV[i, 1], rec["o_p"], rec["lse_p"], H, ct, True, kpm=ctx.pmask,
              bwd=(do_p, dq_p, dPKV[a, 0], dPKV[a, 1], delta_p, None), drop=rec["dr_pa"])
        gq_p = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
        dx1n = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
        L.gemm(M=R, N=d, K=d, A=[dq_p], B=[pw.W[0]], Cs=[dx1n], C2=[gq_p], aux=[dx1pr], act_grad="add", ct=ct, lda=d,
               ldb=d, ldc=d, transB=True)
        self.dqpos_parts.append(gq_p)
        dwq.add([dq_p], [x1], [qpos], [pg.W[0]], ct, [pg.b[0]])
        return dx1n

    def cross_attn(self, a, rec, dx1):
        """Cross-attention over the M scene memories (one launch each for out-projection, attention, query projection):
        returns d(x_in) of the layer application; dK / dV of the application go to self.dKV[a]."""
        spec, ct, ad, M, qpos, coef, H = self.spec, self.ct, self.ad, self.M, self.qpos, self.coef, self.H
        B, Nq, d, Ns, R, dev = self.B, self.Nq, self.d, self.Ns, self.R, self.dev
        KV, dxr_zero, G, dwq, dKV = self.KV, self.dxr_zero, self.G, self.dwq, self.dKV
        i, x_in = rec["i"], rec["x_in"]
        # ---------------- cross-attention backward (M memories per launch)
        cl, cw, cg = self.cas[i], self.caw[i], self.cag[i]
        pre = getattr(self, "_sa_chain", None)
        self._sa_chain = None
        if pre is not None:   # formed by self_attn()'s chain launch
            dxr, dop, do_all = pre
        else:
            dxr, dop = _ln_bwd(x_in, [rec["op_all"][m] for m in range(M)], [ca.norm.weight.detach() for ca in cl],
                               [ca.norm.bias.detach() for ca in cl], cl[0].norm.eps, coef[a] if coef is not None else None,
                               Nq, rec["mean_c"], rec["rstd_c"],
                               dx1, [G(ca.norm.weight) for ca in cl], [G(ca.norm.bias) for ca in cl], drop=rec["dr_cr"],
                               dx_zeroed=dxr_zero[a] if dxr_zero is not None else None)
            do_all = torch.empty(M, B, Nq, d, dtype=ad, device=dev)
            L.gemm(M=R, N=d, K=d, A=[dop[m] for m in range(M)], B=[w.Wo for w in cw], Cs=[do_all[m] for m in range(M)], ct=ct,
                   lda=d, ldb=d, ldc=d, transB=True)
        dwq.add([dop[m] for m in range(M)], [rec["o_all"][m] for m in range(M)], None, [g.Wo for g in cg], ct, [g.bo for g in cg])
        dq_all = torch.empty(M, B, Nq, d, dtype=ad, device=dev)
        delta_c = torch.empty(M * B, H, Nq, dtype=torch.float32, device=dev)
        _attn(rec["q_all"].view(M * B, Nq, d), KV[i, 0].view(M * B, Ns, d), KV[i, 1].view(M * B, Ns, d),
              rec["o_all"].view(M * B, Nq, d), rec["lse"], H, ct, True,
              bwd=(do_all.view(M * B, Nq, d), dq_all.view(M * B, Nq, d), dKV[a, 0].view(M * B, Ns, d),
                   dKV[a, 1].view(M * B, Ns, d), delta_c, None), drop=rec["dr_ca"], drop_bmod=B, **self.ca_mask_kw(rec))
        Wqs = [w.W[0] for w in cw]
        gq = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
        # the input gradient of the query projections feeds the FFN backward of the application in front of this one: when that
        # one runs as a chain launch (and no mask-head call sits in between) the launch forms it itself (step 0)
        if spec.mh is None or spec.skip_pred:
            fold = a > 0 and M <= 3 and dq_all.dtype == torch.bfloat16 and \
                self.ffn_chain_ok(self.tape[a - 1], self.layers[self.tape[a - 1]["i"]], dxr)
        else:   # a mask-head call sits in front of this application: its chain launch forms the sum (csrc/chain_mh.hip)
            fold = M <= 3 and dq_all.dtype == torch.bfloat16 and self.mask_head_chain_ok(rec, self.dcls[a], self.dmlog[a], dxr)
        if fold:
            dxn = _PendingDx(dq_all, Wqs, dxr, gq)
        else:
            dxn = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=d, K=d, A=[dq_all[m] for m in range(M)], B=Wqs, Cs=[dxn] + [None] * (M - 1),
                   C2=[gq] + [None] * (M - 1), aux=[dxr] + [None] * (M - 1), act_grad="add", ct=ct, lda=d, ldb=d, ldc=d,
                   transB=True, kconcat=M)
        self.dqpos_parts.append(gq)
        dwq.add([dq_all[m] for m in range(M)], [x_in] * M, [qpos] * M, [g.W[0] for g in cg], ct, [g.b[0] for g in cg])
        return dxn

    def layer(self, a, dx):
        """One layer application in reverse: FFN, self-attention, (prompt) cross-attention, the mask-head call in front of it."""
        spec = self.spec
        rec = self.tape[a]
        i = rec["i"]
        layer = self.layers[i]
        self._cur_app = a
        if self.ffn_chain_ok(rec, layer, dx):
            dx1 = self.self_attn(rec, layer, None, pre=self.ffn_chain(rec, layer, dx))
        else:
            dx2 = self.ffn(rec, layer, dx)
            dx1 = self.self_attn(rec, layer, dx2)
        if spec.prompt:
            dx1 = self.prompt_cross_attn(a, rec, dx1)
        dx = self.cross_attn(a, rec, dx1)
        # ---------------- mask-head call that preceded this layer
        if spec.mh is not None and not spec.skip_pred:
            dx = self.mask_head(rec, self.dcls[a], self.dmlog[a], dx)
        # ---------------- per-layer gradient buckets (data parallel, SURVEY 8e: "bucketed per decoder layer in reverse
        # execution order"): the first-block application of layer i is the LAST to run backward, so every gradient of
        # layer i's parameters -- its queued weight-gradient products, the K/V rows of its in_proj weights (from the
        # dK / dV of all its applications) and its spatial-bias projection -- is complete once they are flushed here;
        # ready(i) lets the owner start that bucket's all-reduce while the earlier layers still run backward
        if self.per_layer and a < self.Ln:
            self.kv_terms(range(i, self.n_app, self.Ln), into_queue=True)
            self.dwq.flush()
            self.flush_spatial()
            self.ready(i)
        return dx

    def run(self):
        ctx, dxf = self.ctx, self.dxf
        dx = dxf.contiguous().float() if dxf is not None else torch.zeros(self.B, self.Nq, self.d, device=self.dev)
        if ctx.final_rec is not None:
            dx = self.mask_head(ctx.final_rec, self.dcls[-1], self.dmlog[-1], dx)
        for a in range(self.n_app - 1, -1, -1):
            dx = self.layer(a, dx)
        return self.inputs(dx)

    def kconcat_sum(self, A, B, out, rows, transB):
        """out (or nothing) + sum_g A[g] B[g] as a [B, rows, d] fp32 tensor: K-concatenated launches of at most MAXG terms, each
        adding the one before it through the "+ aux" epilogue."""
        d = self.d
        for s in range(0, len(A), MAXG):
            nxt = torch.empty(self.B, rows, d, dtype=torch.float32, device=self.dev)
            n = len(A[s:s + MAXG])
            L.gemm(M=self.B * rows, N=d, K=d, A=A[s:s + MAXG], B=B[s:s + MAXG], Cs=[nxt] + [None] * (n - 1),
                   aux=([out] + [None] * (n - 1)) if out is not None else None, act_grad="add" if out is not None else None,
                   ct=self.ct, lda=d, ldb=d, ldc=d, transB=transB, kconcat=n)
            out = nxt
        return out

    def inputs(self, dx):
        """After the last layer: the deferred weight-gradient flush, then the input gradients -- the hoisted K/V projections'
        backward (sum over all layer applications per source tensor), d pos, d query_pos, d prompt."""
        ctx, spec, tape, ct, ad, M, U, src = self.ctx, self.spec, self.tape, self.ct, self.ad, self.M, self.U, self.src
        mh_src, pos, Ln, B, Nq, d, Ns, Rk = self.mh_src, self.pos, self.Ln, self.B, self.Nq, self.d, self.Ns, self.Rk
        dev, n_app, G, dwq, dqpos_parts, dKV, dPKV = self.dev, self.n_app, self.G, self.dwq, self.dqpos_parts, self.dKV, self.dPKV
        # ---- hoisted K/V projection backward (sum over all applications)
        need_feat = [ctx.needs_input_grad[11 + u] for u in range(U)]
        dfeats: List[Optional[torch.Tensor]] = [None] * U
        single = U == M and all(src[i][j] == j for i in range(Ln) for j in range(M)) and mh_src[:M] == list(range(M))[:len(mh_src)]
        Akv, Bkv = self.kv_terms(range(n_app), into_queue=not self.per_layer)
        # ---- every parameter gradient of the decoder (+ mask head) is complete after this flush: in a data-parallel step
        # its all-reduce starts HERE (enc.grads_ready, set by the step owner) and overlaps the key/value input-gradient
        # products below and the encoders' backward that autograd runs after this function returns
        dkm_list = {}
        if self.dk_terms:
            Mm_, nc = spec.mh_count, len(self.dk_terms)
            newk = torch.empty(Mm_, B, Ns, d, dtype=torch.float32, device=dev)
            L.gemm(M=Ns, N=d, K=Nq, A=[t_[0] for m in range(Mm_) for t_ in self.dk_terms],
                   B=[t_[1][m] for m in range(Mm_) for t_ in self.dk_terms],
                   Cs=[c_ for m in range(Mm_) for c_ in [newk[m]] + [None] * (nc - 1)],
                   aux=[c_ for m in range(Mm_) for c_ in [self.dkeys[m]] + [None] * (nc - 1)] if self.dkeys is not None else None,
                   act_grad="add" if self.dkeys is not None else None, ct=ct, lda=Nq, ldb=d, ldc=d, transB=True, batch=B,
                   strideA=Ns * Nq, strideB=Nq * d, strideC=Ns * d, kconcat=nc)
            self.dkeys, self.dk_terms = newk, []
        if self.dkeys is not None:
            for j in range(spec.mh_count):
                mp = list(spec.mh.mask_pred_list)[j]
                dkm_list[j] = ops.scale_rows(self.dkeys[j], Rk, ad, keep_mask=ctx.mh_valid[j])
                dwq.add([dkm_list[j]], [ctx.mh_feats[j]], None, [G(mp.k_proj.weight)], ct)
        dwq.flush()
        self.flush_spatial()
        self.ready("decoder")   # every parameter gradient of the decoder (+ mask head) is final
        # bf16 path: the input-gradient products read TRANSPOSED bf16 copies of the K/V weights (one copy launch from the
        # forward's pre-cast rows), which turns them into plain NT products -- the 128x128-tile kernel's layout -- and the
        # memories then share launches (K-concatenation per memory, several outputs per launch)
        tposed = ctx.wkv is not None and dKV.dtype == torch.bfloat16
        if tposed:
            wkvT = ctx.wkvT if ctx.wkvT is not None else \
                ctx.wkv.view(Ln, M, 2, d, d).transpose(-1, -2).contiguous()       # [l, m, t][k_in][n_out]
            Bkv = [wkvT[tape[a]["i"], j, t] for a in range(n_app) for j in range(M) for t in (0, 1)]
            kT = None
            if self.dkeys is not None:
                # transposed bf16 copies of the mask-head key projections: one launch (pq3d_cast_transpose; rows = cols = d)
                kws = [mp.k_proj.weight.detach() for mp in list(spec.mh.mask_pred_list)[:spec.mh_count]]
                if d % 32 == 0 and ad == torch.bfloat16 and len(kws) <= MAXG and all(w_.is_contiguous() and w_.shape == (d, d) for w_ in kws):
                    kT, kS = torch.empty(2, len(kws), d, d, dtype=ad, device=dev)
                    L.call("pq3d_cast_transpose", L.parr(kws), L.parr([kS[m_] for m_ in range(len(kws))]),
                           L.parr([kT[m_] for m_ in range(len(kws))]), len(kws), d, d)
                else:
                    kT = torch.stack(kws).transpose(1, 2).contiguous().to(ad)
        # d source_u = sum over the (application, memory) pairs that read it of (dK Wk + dV Wv) [+ mask-head key path]
        jobs = []
        for u in range(U):
            if not need_feat[u]:
                continue
            pairs = [(a, j) for a in range(n_app) for j in range(M) if src[tape[a]["i"]][j] == u]
            Aj = [Akv[2 * (a * M + j) + t] for a, j in pairs for t in (0, 1)]
            Bj = [Bkv[2 * (a * M + j) + t] for a, j in pairs for t in (0, 1)]
            for j in range(spec.mh_count if self.dkeys is not None else 0):
                if mh_src[j] != u:
                    continue
                mp = list(spec.mh.mask_pred_list)[j]
                Aj.append(dkm_list[j])
                Bj.append(kT[j] if tposed else mp.k_proj.weight.detach())
            jobs.append((u, Aj, Bj))
        per = len(jobs[0][1]) if jobs else 0
        want_dpos = pos is not None and ctx.needs_input_grad[4]
        dqpos_done = None
        dpos = None
        nk, nv = n_app, n_app + (1 if self.dkeys is not None else 0)
        if single and tposed and want_dpos and len(jobs) == M and nk * M <= MAXG and nv * M <= MAXG and \
                (self.dkeys is None or spec.mh_count == M):
            # the position embedding enters every memory's KEY input, so d pos = sum_m (K part of d feat_m): form the K
            # parts once (one launch, M outputs), add them into the V parts through the "+ aux" epilogue (second launch)
            # and sum them for d pos -- instead of a third product over all (layer, memory) key terms
            Kp = torch.empty(M, B, Ns, d, dtype=torch.float32, device=dev)
            L.gemm(M=Rk, N=d, K=d, A=[jb[1][2 * a] for jb in jobs for a in range(n_app)],
                   B=[jb[2][2 * a] for jb in jobs for a in range(n_app)],
                   Cs=[c_ for j in range(M) for c_ in [Kp[j]] + [None] * (nk - 1)], ct=ct, lda=d, ldb=d, ldc=d, kconcat=nk)
            outs = [torch.empty(B, Ns, d, dtype=torch.float32, device=dev) for _ in range(M)]
            vA = [[jb[1][2 * a + 1] for a in range(n_app)] + jb[1][2 * n_app:] for jb in jobs]
            vB = [[jb[2][2 * a + 1] for a in range(n_app)] + jb[2][2 * n_app:] for jb in jobs]
            L.gemm(M=Rk, N=d, K=d, A=[t_ for l_ in vA for t_ in l_], B=[t_ for l_ in vB for t_ in l_],
                   Cs=[c_ for o_ in outs for c_ in [o_] + [None] * (nv - 1)],
                   aux=[c_ for j in range(M) for c_ in [Kp[j]] + [None] * (nv - 1)], act_grad="add", ct=ct, lda=d, ldb=d,
                   ldc=d, kconcat=nv)
            for jb, o_ in zip(jobs, outs):
                dfeats[jb[0]] = o_
            if ctx.needs_input_grad[2] and len(dqpos_parts) > 1:   # d query_pos and d pos: one launch, adjacent outputs
                dqpos_done, dpos = ops.sum_pair(dqpos_parts, [Kp[j] for j in range(M)])
            else:
                dpos = ops.sum_n([Kp[j] for j in range(M)])
            want_dpos = False
        elif tposed and jobs and 0 < per <= MAXG and all(len(jb[1]) == per for jb in jobs):
            cap = max(1, MAXG // per)   # memories per launch
            for c0 in range(0, len(jobs), cap):
                chunk = jobs[c0:c0 + cap]
                outs = [torch.empty(B, Ns, d, dtype=torch.float32, device=dev) for _ in chunk]
                L.gemm(M=Rk, N=d, K=d, A=[t_ for jb in chunk for t_ in jb[1]], B=[t_ for jb in chunk for t_ in jb[2]],
                       Cs=[c_ for o_ in outs for c_ in [o_] + [None] * (per - 1)], ct=ct, lda=d, ldb=d, ldc=d,
                       kconcat=per)
                for jb, o_ in zip(chunk, outs):
                    dfeats[jb[0]] = o_
        else:
            for j, Aj, Bj in jobs:
                out = None
                if not Aj:   # a source no layer reads (e.g. a surplus scale): zero gradient
                    out = torch.zeros(B, Ns, d, dtype=torch.float32, device=dev)
                dfeats[j] = self.kconcat_sum(Aj, Bj, out, Ns, transB=not tposed)
        if want_dpos:
            dpos = self.kconcat_sum(Akv[0::2], Bkv[0::2], dpos, Ns, transB=not tposed)
        dqpos = dqpos_done
        if ctx.needs_input_grad[2] and dqpos is None:
            dqpos = ops.sum_n(dqpos_parts)
        dx0 = dx if ctx.needs_input_grad[1] else None
        dprompt = None
        if spec.prompt and ctx.needs_input_grad[9]:
            # d prompt = sum over layer applications of dK_p Wk + dV_p Wv: one K-concatenated launch
            Ap = [dPKV[a_, t] for a_ in range(n_app) for t in (0, 1)]
            Bp = [w_ for a_ in range(n_app) for w_ in self.pcw[tape[a_]["i"]].W[1:]]
            dprompt = self.kconcat_sum(Ap, Bp, None, ctx.prompt.shape[1], transB=True)
        pgrads = [G(p) if (p.requires_grad and not self.accumulate) else None for p in self.params]
        return (None, dx0, dqpos, None, dpos, None, None, None, None, dprompt, None, *dfeats, *([None] * M), *pgrads)


class _DecoderForward(_DecoderPass):
    """One forward pass of the fused decoder, the mirror of _DecoderBackward: the state every step shares and one method per
    step, run in forward order: the hoisted K/V projections, (the prompt memory's K/V), the mask-head keys, the spatial bias;
    then per layer application the mask-head call in front of it -> cross-attention over the scene memories -> (prompt
    cross-attention) -> self-attention -> FFN.  `_FusedDecoder.forward` is `_DecoderForward(...).run(ctx)`.  The object holds
    the returned query state and the tape, so nothing that lives on `ctx` may reference it (see run())."""

    def __init__(self, spec, needs_grad, x0, qpos, qmask, pos, pl, seg_pad, offline_mask, coef, prompt, prompt_kpm, rest):
        U, M = spec.n_src, len(spec.mems)
        super().__init__(spec, qpos, rest[0].shape[1])
        self.needs_grad = needs_grad
        self.params = rest[U + M:]
        self.cq = ops.small_ct(self.ct)   # query-side GEMMs (M = B*N_q rows): split-bf16 in 'bf16' mode, exact f32 otherwise
        self.kv3 = spec.kv3               # compute mode 'bf16x3': split-bf16 key/value side (hi + lo bf16 planes), see fused_decoder()
        self.x0, self.qpos, self.pos, self.qmask = ops._c(x0), ops._c(qpos), ops._c(pos), ops._c(qmask)
        self.feats = [ops._c(f) for f in rest[:U]]   # the U unique sources
        self.masks = [ops._c(m) for m in rest[U:U + M]]
        self.pl, self.seg_pad, self.offline_mask, self.coef = pl, seg_pad, offline_mask, coef
        self.prompt, self.pmask = (ops._c(prompt), ops._c(prompt_kpm)) if spec.prompt else (None, None)
        self.tape: List[dict] = []
        self.q_next = None   # the next application's cross-attention queries when the chain launch of this one formed them
        self.attn_mask = self.row_open = None

    def hoist_kv(self):
        """The layer-invariant key/value side: the MFMA operands kin_m = (feat_m + pos), vin_m = feat_m and the K/V rows of
        every in_proj_weight, rounded once, then KV[l, 0|1, m] = (feat_m [+ pos]) @ W{k,v}_{l,m}^T + b of every (layer,
        memory) as ONE grouped GEMM (KV_lo: the residual planes of compute mode 'bf16x3')."""
        ct, ad, dev, kv3, pos, feats, caw, src = self.ct, self.ad, self.dev, self.kv3, self.pos, self.feats, self.caw, self.src
        B, Ns, d, U, M, Ln = self.B, self.Ns, self.d, self.U, self.M, self.Ln
        # ---- operands in the activation dtype (bf16 path: the 2*L*M hoisted GEMMs and their weight-gradient GEMM then read
        # 2 B/element, not 8)
        kvin_lo = None
        if ct == BF16 and (B * Ns * d) % 8 == 0 and 2 * U <= MAXG:
            kvin = torch.empty(2, U, B, Ns, d, dtype=ad, device=dev)
            f_srcs, f_adds = feats * 2, [pos] * U + [None] * U
            f_outs = [kvin[0, u] for u in range(U)] + [kvin[1, u] for u in range(U)]
            if kv3:   # both planes of (feat + pos) and feat in one launch; the K / V weights' residual planes join it below
                kvin_lo = torch.empty(2, U, B, Ns, d, dtype=ad, device=dev)
            else:
                L.call("pq3d_add_cast", L.parr(f_srcs), L.parr(f_adds), L.parr(f_outs), 2 * U, L.BF16, B * Ns * d)
            kin, vin, kin2 = [kvin[0, u] for u in range(U)], [kvin[1, u] for u in range(U)], [None] * U
        else:
            kin, vin, kin2 = feats, feats, [pos] * U
        self.kin, self.vin, self.kin2 = kin, vin, kin2
        self.KV = KV = torch.empty(Ln, 2, M, B, Ns, d, dtype=ad, device=dev)
        # bf16 path: the K/V rows of every in_proj_weight are rounded ONCE (one launch) instead of by each of the M/64 row
        # tiles that read them; with both operands in bf16 the projection takes the 128x128-tile kernel (gemm128.hip),
        # whose output is bit-identical to converting in flight
        wkv = wkvT = None
        if kin2[0] is None and ct == BF16 and Ln * M <= MAXG and (2 * d * d) % 8 == 0:
            wkv = torch.empty(Ln, M, 2 * d, d, dtype=ad, device=dev)
            w_srcs = [cw.Wkv for cl in caw for cw in cl]
            w_outs = [wkv[i, j] for i in range(Ln) for j in range(M)]
            if d % 32 == 0 and self.needs_grad:
                # the same launch also leaves the transposed blocks [l, m, t][k_in][n_out] the backward's input-gradient
                # products read (plain NT products on W^T: the 128x128-tile kernel's layout)
                wkvT = torch.empty(Ln, M, 2, d, d, dtype=ad, device=dev)
                L.call("pq3d_cast_transpose", L.parr(w_srcs), L.parr(w_outs),
                       L.parr([wkvT[i, j] for i in range(Ln) for j in range(M)]), len(w_srcs), 2 * d, d)
            else:
                L.call("pq3d_add_cast", L.parr(w_srcs), L.parr([None] * len(w_srcs)), L.parr(w_outs), len(w_srcs), L.BF16,
                       2 * d * d)
        self.wkv, self.wkvT = wkv, wkvT
        self.KV_lo = KV_lo = None
        if kv3:
            # split-bf16 projection of pre-split operands (csrc/gemm_x3p.hip: the four planes of a k slice staged once, lo.hi + hi.lo
            # + hi.hi per term pair), its fp32-grade result leaving as hi / lo bf16 planes (PQ3D_ACT_PLANES): KV = exactly the
            # 'bf16'-mode tensor the backward reads, KV_lo the residual the forward's split-bf16 attention adds (csrc/attn_x3.hip)
            assert wkv is not None and kvin_lo is not None
            wkv_lo = torch.empty_like(wkv)
            # the big buffers here are allocated in this order and the residual planes held until the pass ends: another order
            # / freeing them early moves the allocator's blocks under everything that follows (0.2-0.3 % of the replayed c2 / c4 step)
            self.planes_lo = (kvin_lo, wkv_lo)
            ops.split_planes(f_srcs + w_srcs, f_adds + [None] * (Ln * M), f_outs + [None] * (Ln * M),
                             [kvin_lo[0, u] for u in range(U)] + [kvin_lo[1, u] for u in range(U)] +
                             [wkv_lo[i, j] for i in range(Ln) for j in range(M)])
            self.KV_lo = KV_lo = torch.empty_like(KV)
        terms = []   # one GEMM group per (layer, memory, K | V)
        for i in range(Ln):
            for j, cw in enumerate(caw[i]):
                u = src[i][j]
                for t in (0, 1):
                    term = dict(A=(kin, vin)[t][u], A2=(kin2[u], None)[t], B=cw.W[1 + t] if wkv is None else wkv[i, j, t * d:(t + 1) * d],
                                bias=cw.b[1 + t], Cs=KV[i, t, j])
                    if kv3:
                        term.update(A2=kvin_lo[t, u], B2=wkv_lo[i, j, t * d:(t + 1) * d], C2=KV_lo[i, t, j])
                    terms.append(term)
        _gemm_chunks({k: [term[k] for term in terms] for k in terms[0]}, M=self.Rk, N=d, K=d, ct=L.BF16X3 if kv3 else ct, lda=d,
                     ldb=d, ldc=d, **(dict(act_grad="planes") if kv3 else {}))

    def hoist_prompt_kv(self):
        """structure 'mixed' (query_encoder.py:162-165): the prompt memory's K / V of every layer, hoisted like the scene
        memories' (the prompt is layer-invariant, pos = None: query3d_unified.py:134-136): one grouped launch."""
        kv3, prompt, B, d, Ln, dev = self.kv3, self.prompt, self.B, self.d, self.Ln, self.dev
        T = prompt.shape[1]
        # compute mode 'bf16x3': the (short) prompt memory's cross-attention runs at fp32 grade on kernels that exist -- split-bf16
        # projections with fp32 K / V, the exact-f32 attention -- and leaves bf16 copies as the tape of the single-bf16 backward
        self.PKV_fwd = out = torch.empty(Ln, 2, B, T, d, dtype=torch.float32 if kv3 else self.ad, device=dev)
        _gemm_chunks(dict(A=[prompt] * (2 * Ln), B=[w for pw in self.pcw for w in pw.W[1:]], bias=[b for pw in self.pcw for b in pw.b[1:]],
                          Cs=[out[i, t] for i in range(Ln) for t in (0, 1)]),
                     M=B * T, N=d, K=d, ct=self.cq if kv3 else self.ct, lda=d, ldb=d, ldc=d)
        self.PKV = ops.cast_bf16([out])[0] if kv3 else out

    def mask_head_keys(self):
        """The stacked key-padding mask of the memories and the (layer-invariant) mask-head keys."""
        spec, masks, B, Ns, d, M = self.spec, self.masks, self.B, self.Ns, self.d, self.M
        self.kpm_all = None
        if not spec.use_self_mask:
            st = spec.stacked_kpm   # [M, B, Ns] already stacked by the model (same memory order): no copy
            self.kpm_all = st.reshape(M * B, Ns) if st is not None else torch.cat(masks, 0)
        self.mh_feats = [self.feats[u] for u in self.mh_src]
        self.keys = self.inv_den = self.mh_valid = None
        if spec.mh is not None:
            Mm = spec.mh_count
            mps = list(spec.mh.mask_pred_list)[:Mm]
            self.mh_valid = valid = ops.mask_not(masks[:Mm])   # one launch
            cq = self.cq   # fp32-grade keys (split-bf16): see MaskHeadSegLevel.project_keys
            keys_buf = torch.empty(Mm, B, Ns, d, dtype=ops.act_dtype(cq), device=self.dev)
            self.keys = [keys_buf[m] for m in range(Mm)]
            L.gemm(M=self.Rk, N=d, K=d, A=self.mh_feats[:Mm], B=[mp.k_proj.weight.detach() for mp in mps], Cs=self.keys,
                   row_mask=valid, ct=cq, lda=d, ldb=d, ldc=d)
            self.inv_den = ops.mask_inv_den(masks[:Mm])

    def spatial_bias(self):
        """Spatial attention bias log(clamp(relu(W_l . pairwise_locs))) of every layer: one grouped launch (depends on the
        layer's weights only, not on the query state, and is shared by the blocks that re-traverse the layers)."""
        Ln, B, H, Nq = self.Ln, self.B, self.H, self.Nq
        self.sbias_all = None
        if not self.spec.spatial:
            return
        self.sbias_all = sbias_all = torch.empty(Ln, B, H, Nq, Nq, dtype=torch.float32, device=self.dev)
        fcs = [layer.self_attn.self_attn.pairwise_loc_fc for layer in self.layers]
        for i0 in range(0, Ln, MAXG):
            n_ = min(MAXG, Ln - i0)
            L.call("pq3d_spatial_bias_fwd_grouped", self.pl, L.parr([fc.weight.detach() for fc in fcs[i0:i0 + n_]]),
                   L.parr([fc.bias.detach() for fc in fcs[i0:i0 + n_]]), L.parr([sbias_all[i0 + k] for k in range(n_)]), n_, B, H, Nq)

    def cross_attn(self, app, rec, x):
        """Cross-attention over the M scene memories, 4 launches: query projections (unless the previous application's chain
        launch formed them), attention with the memories stacked along the batch, out-projections, merged post-norm.  Returns
        (x1, qkv): qkv = the self-attention's projections when the chain launch (csrc/chain_ca.hip) formed them too."""
        spec, ct, ad, cq, kv3, qpos, coef = self.spec, self.ct, self.ad, self.cq, self.kv3, self.qpos, self.coef
        H, B, Nq, d, Ns, R, M, dev = self.H, self.B, self.Nq, self.d, self.Ns, self.R, self.M, self.dev
        i, dr_ca, dr_cr = rec["i"], rec["dr_ca"], rec["dr_cr"]
        cl, cw, KV = self.cas[i], self.caw[i], self.KV
        if self.q_next is not None:   # formed by the previous layer application's chain launch (csrc/chain_ffn.hip, step 6)
            q_all, self.q_next = self.q_next, None
        else:
            q_all = torch.empty(M, B, Nq, d, dtype=torch.float32 if kv3 else ad, device=dev)
            L.gemm(M=R, N=d, K=d, A=[x] * M, A2=[qpos] * M, B=[w.W[0] for w in cw], bias=[w.b[0] for w in cw],
                   Cs=[q_all[m] for m in range(M)], ct=cq, lda=d, ldb=d, ldc=d)
        o_all = torch.empty(M, B, Nq, d, dtype=ad, device=dev)
        lse = torch.empty(M * B, H, Nq, dtype=torch.float32, device=dev)
        q_in, o_out, planes = q_all, o_all, None
        if kv3:
            # split-bf16 cross-attention (csrc/attn_x3.hip): fp32 q in, fp32 o out (-> the split-bf16 out-projection); the
            # bf16 copies it leaves of q and o are what the (single-bf16) backward reads -- a 'bf16'-mode tape
            q_all = torch.empty(M, B, Nq, d, dtype=ad, device=dev)
            o_out = torch.empty(M, B, Nq, d, dtype=torch.float32, device=dev)
            planes = (self.KV_lo[i, 0], self.KV_lo[i, 1], q_all, o_all)
        _attn(q_in.view(M * B, Nq, d), KV[i, 0].view(M * B, Ns, d), KV[i, 1].view(M * B, Ns, d), o_out.view(M * B, Nq, d), lse, H,
              L.BF16X3 if kv3 else ct, True, drop=dr_ca, drop_bmod=B, planes=planes, **self.ca_mask_kw(rec))
        # out-projections + merged post-norm + the self-attention's q / k / v projections: ONE launch when the shapes allow
        # (csrc/chain_ca.hip: same bits as the three launches below)
        chain_ca = _chain_on(dev) and ct == BF16 and cq == L.BF16X3 and not spec.prompt and dr_cr is None and \
            ops.chain_ca_ok(R, d, M) and o_all.dtype == torch.bfloat16
        qkv = None
        gammas, betas = [ca.norm.weight.detach() for ca in cl], [ca.norm.bias.detach() for ca in cl]
        if chain_ca:
            sw = self.saw[i]
            flags = _chain_flag_buf(self.enc, "_chain_flags_ca", 2048, dev)
            op_all, x1, mean_c, rstd_c, qkv = ops.chain_ca_fwd(
                o_out, [w.Wo for w in cw], [w.bo for w in cw], x, gammas, betas, cl[0].norm.eps,
                coef[app] if coef is not None else None, Nq, qpos, [t_.contiguous() for t_ in sw.W],
                [t_.contiguous() for t_ in sw.b], flags)
        else:
            op_all = torch.empty(M, B, Nq, d, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=d, K=d, A=[o_out[m] for m in range(M)], B=[w.Wo for w in cw], bias=[w.bo for w in cw],
                   Cs=[op_all[m] for m in range(M)], ct=cq if kv3 else ct, lda=d, ldb=d, ldc=d)
            x1, mean_c, rstd_c = _ln_fwd(x, [op_all[m] for m in range(M)], gammas, betas, cl[0].norm.eps,
                                         coef[app] if coef is not None else None, Nq, drop=dr_cr)
        rec.update(q_all=q_all, o_all=o_all, lse=lse, op_all=op_all, mean_c=mean_c, rstd_c=rstd_c, x1=x1)
        return x1, qkv

    def prompt_cross_attn(self, app, rec, x1):
        """structure 'mixed': the sequential prompt cross-attention on the parallel block's output (CrossAttentionLayer.forward_post,
        query_encoder.py:288-307: q = x1 + query_pos, k = v = prompt, own LayerNorm), 4 launches.  Returns x1s."""
        spec, ct, cq, kv3, qpos, H, B, Nq, d, R, dev = self.spec, self.ct, self.cq, self.kv3, self.qpos, self.H, self.B, self.Nq, self.d, self.R, self.dev
        i = rec["i"]
        pc, pw, PKV = self.pcas[i], self.pcw[i], self.PKV_fwd   # what the forward's attention reads
        dr_pa = spec.drop(pc, app, ops.DROP_CA_ATTN, dev, m=4)   # sequential slot 4 + 0 (modules.QueryEncoderLayer)
        dr_pr = spec.drop(pc, app, ops.DROP_CA_RES, dev, m=4)
        adp = torch.float32 if kv3 else self.ad
        qp = torch.empty(B, Nq, d, dtype=adp, device=dev)
        L.gemm(M=R, N=d, K=d, A=[x1], A2=[qpos], B=[pw.W[0]], bias=[pw.b[0]], Cs=[qp], ct=cq, lda=d, ldb=d, ldc=d)
        o_p = torch.empty(B, Nq, d, dtype=adp, device=dev)
        lse_p = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)
        _attn(qp, PKV[i, 0], PKV[i, 1], o_p, lse_p, H, L.F32 if kv3 else ct, True, kpm=self.pmask, drop=dr_pa)
        opp = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
        L.gemm(M=R, N=d, K=d, A=[o_p], B=[pw.Wo], bias=[pw.bo], Cs=[opp], ct=cq if kv3 else ct, lda=d, ldb=d, ldc=d)
        if kv3:   # the backward's bf16 tape
            qp, o_p = ops.cast_bf16([qp, o_p])
        x1s, mean_p, rstd_p = _ln_fwd(x1, [opp], [pc.norm.weight.detach()], [pc.norm.bias.detach()], pc.norm.eps, None, Nq, drop=dr_pr)
        rec.update(qp=qp, o_p=o_p, lse_p=lse_p, opp=opp, mean_p=mean_p, rstd_p=rstd_p, dr_pa=dr_pa, dr_pr=dr_pr)
        return x1s

    def self_attn(self, app, rec, layer, x1s, qkv):
        """Self-attention (N_q x N_q scores per scene: projections at fp32 grade, attention core on the exact-f32 MFMA path) and
        the row-local tail of the layer: ffn_chain() when the chain launch applies, else out-projection + post-norm and ffn().
        Returns x3, the layer's output."""
        spec, ct, cq, qpos, qmask, H, B, Nq, d, R, dev = self.spec, self.ct, self.cq, self.qpos, self.qmask, self.H, self.B, self.Nq, self.d, self.R, self.dev
        i, dr_sa, dr_sr, dr_fi, dr_fr = rec["i"], rec["dr_sa"], rec["dr_sr"], rec["dr_fi"], rec["dr_fr"]
        sa, sw = layer.self_attn, self.saw[i]
        if qkv is None:
            qkv = torch.empty(3, B, Nq, d, dtype=torch.float32, device=dev)
            L.gemm(M=R, N=d, K=d, A=[x1s] * 3, A2=[qpos, qpos, None], B=sw.W, bias=sw.b, Cs=[qkv[0], qkv[1], qkv[2]], ct=cq,
                   lda=d, ldb=d, ldc=d)
        sbias = self.sbias_all[i] if spec.spatial else None   # layer-invariant across blocks: computed once (spatial_bias)
        o_s = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
        lse_s = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)
        F_ = layer.ffn.linear1.out_features
        chain = _chain_on(dev) and cq == L.BF16X3 and spec.act == "relu" and dr_sr is None and dr_fi is None and dr_fr is None and \
            ops.chain_ffn_ok(R, d, F_) and sa.norm.weight.shape[0] == d
        # the self-attention core as step 0 of that launch (one launch less per layer; same bits as pq3d_attn_fwd's kernel)
        sa_in = chain and dr_sa is None and ops.sa_ct(ct) == L.BF16X3 and ops.chain_sa_ok(Nq, H, d) and qkv.is_contiguous() and \
            (sbias is None or (sbias.is_contiguous() and sbias.dtype == torch.float32)) and \
            (qmask is None or (qmask.is_contiguous() and qmask.dtype == torch.bool))
        if not sa_in:
            _attn(qkv[0], qkv[1], qkv[2], o_s, lse_s, H, ops.sa_ct(ct), False, kpm=qmask, bias=sbias, drop=dr_sa)
        rec.update(qkv=qkv, sbias=sbias, o_s=o_s, lse_s=lse_s)
        if chain:
            return self.ffn_chain(app, rec, layer, x1s, sa_in)
        f = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)
        L.gemm(M=R, N=d, K=d, A=[o_s], B=[sw.Wo], bias=[sw.bo], Cs=[f], ct=cq, lda=d, ldb=d, ldc=d)
        x2, mean_s, rstd_s = _ln_fwd(x1s, [f], [sa.norm.weight.detach()], [sa.norm.bias.detach()], sa.norm.eps, None, Nq, drop=dr_sr)
        rec.update(f=f, mean_s=mean_s, rstd_s=rstd_s, x2=x2)
        return self.ffn(rec, layer, x2)

    def ffn_chain(self, app, rec, layer, x1s, sa_in):
        """The row-local tail of the layer in ONE launch (csrc/chain_ffn.hip: out-projection, post-norm, FFN, post-norm; 8
        workgroups per 32-row tile handing rows over inside one XCD) -- the five launches' bits; with sa_in the self-attention
        core is its step 0.  Returns x3."""
        kv3, qpos, H, d, M, Ln = self.kv3, self.qpos, self.H, self.d, self.M, self.Ln
        sa, ffn, sw, qkv = layer.self_attn, layer.ffn, self.saw[rec["i"]], rec["qkv"]
        flags = _chain_flag_buf(self.enc, "_chain_flags", self.R, self.dev)
        # ... and the NEXT application's cross-attention query projections (they read this application's output): the
        # mask head in front of the next layer reads x3, not the queries, so nothing else moves
        nextq = None
        if app + 1 < self.spec.num_blocks * Ln and M <= 3 and self.ad == torch.bfloat16:
            cn = self.caw[(rec["i"] + 1) % Ln]
            nextq = (qpos, [w.W[0] for w in cn], [w.b[0] for w in cn])
        outs = ops.chain_ffn_fwd(
            rec["o_s"], sw.Wo, sw.bo, x1s, sa.norm.weight.detach(), sa.norm.bias.detach(), sa.norm.eps,
            ffn.linear1.weight.detach(), ffn.linear1.bias.detach(), ffn.linear2.weight.detach(), ffn.linear2.bias.detach(),
            ffn.norm.weight.detach(), ffn.norm.bias.detach(), ffn.norm.eps, flags, nextq=nextq,
            q_dtype=torch.float32 if kv3 else torch.bfloat16,
            sa=(qkv[0], qkv[1], qkv[2], rec["sbias"], self.qmask, rec["lse_s"], 1.0 / math.sqrt(d // H)) if sa_in else None)
        f, x2, mean_s, rstd_s, h, _zp, z, x3, mean_f, rstd_f = outs[:10]
        self.q_next = outs[10] if nextq is not None else None
        rec.update(f=f, mean_s=mean_s, rstd_s=rstd_s, x2=x2, h=h, pre=None, z=z, mean_f=mean_f, rstd_f=rstd_f)
        return x3

    def ffn(self, rec, layer, x2):
        """FFN sublayer, 3 launches: linear1 + activation (+ inner dropout), linear2, residual + LayerNorm.  Returns x3."""
        spec, cq, B, Nq, d, R, dev = self.spec, self.cq, self.B, self.Nq, self.d, self.R, self.dev
        ffn = layer.ffn
        F_ = ffn.linear1.out_features
        h = torch.empty(B, Nq, F_, dtype=ops.act_dtype(cq), device=dev)
        pre = torch.empty_like(h) if spec.act == "gelu" else None
        L.gemm(M=R, N=F_, K=d, A=[x2], B=[ffn.linear1.weight.detach()], bias=[ffn.linear1.bias.detach()], Cs=[h],
               C2=[pre], ct=cq, lda=d, ldb=d, ldc=F_, act=spec.act, drop=rec["dr_fi"])
        # linear2 has K = F = 2048 on only M/64 x d/64 = 52 tiles: a long serial k-loop on a fifth of the chip.  Its K
        # range is split over KS groups of ONE grouped launch (no atomics: each group owns an output), and the
        # LayerNorm kernel adds the partial sums (+ residual, + dropout of the summed branch) in a fixed order --
        # deterministic, so the bit-exact padding-invariance / scene-independence properties hold.
        KS = 4 if F_ % (4 * 64) == 0 else 1
        zp = torch.empty(KS, B, Nq, d, dtype=torch.float32, device=dev)
        Fk = F_ // KS
        hv, w2 = h.view(R, F_), ffn.linear2.weight.detach()
        L.gemm(M=R, N=d, K=Fk, A=[hv[:, k * Fk:(k + 1) * Fk] for k in range(KS)],
               B=[w2[:, k * Fk:(k + 1) * Fk] for k in range(KS)],
               bias=[ffn.linear2.bias.detach()] + [None] * (KS - 1), Cs=[zp[k] for k in range(KS)], ct=cq, lda=F_,
               ldb=F_, ldc=d)
        z = torch.empty(B, Nq, d, dtype=torch.float32, device=dev)   # sum of the partials, kept for the backward
        x3, mean_f, rstd_f = _ln_fwd(x2, [zp[k] for k in range(KS)], [ffn.norm.weight.detach()], [ffn.norm.bias.detach()],
                                     ffn.norm.eps, None, Nq, drop=rec["dr_fr"], sum_branches=True, osum=z)
        rec.update(h=h, pre=pre, z=z, mean_f=mean_f, rstd_f=rstd_f)
        return x3

    def layer(self, app, i, x, pcls, pmask):
        """One layer application: its dropout sites, the mask-head call in front of it (-> the attention mask), then
        cross-attention, (prompt cross-attention), self-attention and FFN; appends the tape record.  Returns the new x."""
        spec, ct, dev = self.spec, self.ct, self.dev
        layer, ca0 = self.layers[i], self.cas[i][0]
        rec: Dict[str, object] = {"i": i, "x_in": x}
        # dropout sites of this layer application (None when dropout is off); memories are stacked along the
        # attention batch in groups of B -> drop_bmod=B gives memory j the site of slot j
        rec.update(dr_ca=spec.drop(ca0, app, ops.DROP_CA_ATTN, dev), dr_cr=spec.drop(ca0, app, ops.DROP_CA_RES, dev),
                   dr_sa=None if spec.spatial else spec.drop(layer.self_attn, app, ops.DROP_SA_ATTN, dev),
                   dr_sr=spec.drop(layer.self_attn, app, ops.DROP_SA_RES, dev),
                   dr_fi=spec.drop(layer.ffn, app, ops.DROP_FFN_INNER, dev), dr_fr=spec.drop(layer.ffn, app, ops.DROP_FFN_RES, dev))
        if spec.mh is not None and not spec.skip_pred:
            cls, mlog, amask = _mh_forward(spec, x, self.keys, self.inv_den, self.seg_pad, rec, app)
            pcls.append(cls)
            pmask.append(mlog)
            self.attn_mask = self.offline_mask if spec.offline else amask
        elif spec.offline:
            self.attn_mask = self.offline_mask
        mask_bits = None
        if spec.use_self_mask:
            # row-open flags AND the mask as bit words (open rows cleared) from one pass over the bytes: the
            # resident backward reads 1/8 of the mask and no byte tiles (attn_resident.hip MASK3 == 2)
            if ct == BF16:
                self.row_open, mask_bits = ops.mask_pack(self.attn_mask)
            else:
                self.row_open = ops.mask_row_all(self.attn_mask)
        rec["attn_mask"], rec["row_open"], rec["mask_bits"] = self.attn_mask, self.row_open, mask_bits
        x1, qkv = self.cross_attn(app, rec, x)
        rec["x1s"] = x1s = self.prompt_cross_attn(app, rec, x1) if spec.prompt else x1   # input of the self-attention sublayer
        x3 = self.self_attn(app, rec, layer, x1s, qkv)
        self.tape.append(rec)
        return x3

    def run(self, ctx):
        spec, Ln = self.spec, self.Ln
        self.hoist_kv()
        self.PKV = None
        if spec.prompt:
            self.hoist_prompt_kv()
        self.mask_head_keys()
        self.spatial_bias()
        pcls, pmask = [], []
        x = self.x0
        for blk in range(spec.num_blocks):
            for i in range(Ln):
                x = self.layer(blk * Ln + i, i, x, pcls, pmask)
        final_rec = None
        if spec.mh is not None:
            # detached aliases: x is also RETURNED, i.e. it becomes a tensor whose grad_fn is this ctx -- kept here as the same
            # object it would close a reference cycle (ctx -> rec -> x -> grad_fn = ctx) that only Python's cycle collector
            # frees: the saved activations of every step would outlive it, and under GraphedQuery3D the captured forward's
            # autograd graph did (round 4: its capture-stream AccumulateGrad nodes cost config 4's 'autograd' mode 2 ms per step).
            # For the same reason ctx gets plain tensors, lists and modules below, never this object or a bound method of it
            final_rec = {"x_in": x.detach()}
            cls, mlog, _ = _mh_forward(spec, x, self.keys, self.inv_den, self.seg_pad, final_rec, spec.num_blocks * Ln)
            if spec.skip_pred:
                pcls, pmask = [], []
            pcls.append(cls)
            pmask.append(mlog)
        ctx.kin, ctx.vin, ctx.kin2, ctx.wkv, ctx.wkvT = self.kin, self.vin, self.kin2, self.wkv, self.wkvT
        if spec.mh is not None:
            ctx.mh_valid = self.mh_valid
        ctx.spec, ctx.tape, ctx.final_rec = spec, self.tape, final_rec
        ctx.KV, ctx.keys, ctx.inv_den, ctx.kpm_all = self.KV, self.keys, self.inv_den, self.kpm_all
        ctx.PKV, ctx.pcas, ctx.prompt, ctx.pmask = self.PKV, self.pcas, self.prompt, self.pmask
        ctx.cas, ctx.n_mh = self.cas, len(pcls)
        ctx.params = self.params
        ctx.save_for_backward(self.x0, self.qpos, self.qmask, self.pos, self.pl, self.seg_pad, self.coef, *self.feats, *self.masks)
        ctx.M, ctx.U, ctx.src, ctx.mh_src, ctx.mh_feats = self.M, self.U, self.src, self.mh_src, self.mh_feats
        return (x, *pcls, *pmask)


class _FusedDecoder(Function):
    """inputs: spec, x0, qpos, qmask, pos, pairwise_locs, seg_pad, offline_mask, coef, prompt, prompt_kpm, U feats,
    M masks, *params."""

    @staticmethod
    def forward(ctx, spec: FusedSpec, x0, qpos, qmask, pos, pl, seg_pad, offline_mask, coef, prompt, prompt_kpm, *rest):
        return _DecoderForward(spec, any(ctx.needs_input_grad), x0, qpos, qmask, pos, pl, seg_pad, offline_mask, coef, prompt,
                               prompt_kpm, rest).run(ctx)

    @staticmethod
    def backward(ctx, dxf, *dheads):
        return _DecoderBackward(ctx, dxf, dheads).run()


def fused_decoder(enc, input_dict, pairwise_locs, mask_head=None, seg_fts_for_match=None, seg_masks=None,
                  offline_attn_masks=None, skip_prediction=False):
    """Run QueryMaskEncoder (+ MaskHeadSegLevel) through the fused executor.  Returns
    (query, predictions_class, predictions_mask) exactly like QueryMaskEncoder.forward followed by the final
    mask-head call.  Raises NotImplementedError for configurations it does not cover (callers fall back to the
    modular path)."""
    layer0 = enc.unified_encoder[0]
    if layer0.structure not in ("parallel", "mixed"):
        raise NotImplementedError("fused path covers structure='parallel' and 'mixed'")
    if any(getattr(m_, "normalize_before", False) or getattr(m_, "spatial_attn_fusion", "mul") != "mul" for m_ in enc.modules()):
        raise NotImplementedError("fused path: post-norm layers with spatial_attn_fusion='mul' (the shipped configurations)")
    training = enc.training
    mems = [m for m in layer0.memories if training or m not in layer0.drop_memories_test]
    prompt = pmask = None
    if layer0.structure == "mixed":
        # query_encoder.py:162-165: parallel over the scene memories, then sequential_ca(query, ['prompt']) -- the literal
        # list, so the prompt attends even when drop_memories_test names it
        mems = [m for m in mems if m != "prompt"]
        if "prompt" not in layer0.memory2ca or "prompt" not in input_dict:
            raise NotImplementedError("fused path: structure='mixed' needs a prompt memory")
        prompt, pmask, ppos = input_dict["prompt"][:3]
        if ppos is not None or pmask.ndim != 2 or isinstance(prompt, (list, tuple)):
            raise NotImplementedError("fused path: prompt memory with a position tensor / 3-D mask / multi-scale list")
    if not mems or any(m == "prompt" for m in mems):
        raise NotImplementedError("fused path needs scene memories (a prompt memory only under structure='mixed')")
    x0, qmask, qpos = input_dict["query"][:3]
    feats = [input_dict[m][0] for m in mems]
    masks = [input_dict[m][1] for m in mems]
    poss = [input_dict[m][2] for m in mems]
    if any(m.ndim != 2 for m in masks):
        raise NotImplementedError("fused path: pre-set 3-D masks")
    Ln_ = len(enc.unified_encoder)
    # unique source tensors: a multi-scale voxel memory (list: one [B, N_seg, d] tensor per layer, the last one for the
    # mask head -- pcd_mask3d_encoder.py:133-154, query_encoder.py:90-91) contributes one source per scale
    uniq, src = [], [[0] * len(mems) for _ in range(Ln_)]

    def uid(t):
        for k, q in enumerate(uniq):
            if q is t:
                return k
        uniq.append(t)
        return len(uniq) - 1
    for j, f in enumerate(feats):
        if isinstance(f, (list, tuple)):
            if len(f) < Ln_:
                raise NotImplementedError("fused path: a multi-scale memory needs one scale per layer")
            for i in range(Ln_):
                src[i][j] = uid(f[i])
        else:
            for i in range(Ln_):
                src[i][j] = uid(f)
    if any(p is not poss[0] for p in poss) or len({tuple(f.shape) for f in uniq}) != 1:
        raise NotImplementedError("fused path: memories must share one position tensor and one shape")
    if len(mems) * Ln_ * 2 > 4 * MAXG:
        raise NotImplementedError("fused path: too many (layer, memory) groups")
    mh_count, mh_src = 0, []
    if mask_head is not None:
        if seg_fts_for_match is None:
            raise NotImplementedError("fused path: mask head without seg_fts_for_match")
        mh_count = min(len(seg_fts_for_match), len(mask_head.mask_pred_list))   # mask_head.py:31: zip() truncates
        for k, sf in enumerate(seg_fts_for_match[:mh_count]):
            want = feats[k][-1] if (k < len(feats) and isinstance(feats[k], (list, tuple))) else (feats[k] if k < len(feats) else None)
            if sf[0] is not want:
                raise NotImplementedError("fused path: mask-head memories must be the leading scene memories")
            mh_src.append(uid(sf[0]))
    if enc.use_self_mask and mask_head is None:
        raise NotImplementedError("use_self_mask without a mask head")
    coef = None
    if training and layer0.memory_dropout > 0.0:
        # query_encoder.py:145-151: every layer application draws its own per-(scene, memory) keep mask -> [apps, M, B]
        from .modules import memory_keep_coef
        hook = getattr(enc, "memory_keep_hook", None)
        n_app = enc.num_blocks * len(enc.unified_encoder)
        B_ = x0.shape[0]
        coef = torch.stack([memory_keep_coef(B_, len(mems), layer0.memory_dropout, x0.device,
                                             hook(a, B_, len(mems), x0.device) if hook is not None else None)
                            for a in range(n_app)]).contiguous()
    ct = L.BF16 if layer0.compute in ("bf16", "bf16x3") else L.F32
    # compute mode 'bf16x3': the split-bf16 key/value side where its kernels cover the shape (128-row-tile plane GEMM: d % 128 == 0;
    # csrc/attn_x3.hip: d_h = 32 / 64, <= 256 queries), the exact-f32 kernels otherwise -- same accuracy contract
    kv3 = False
    if layer0.compute == "bf16x3":
        B_, Ns_, d_ = uniq[0].shape
        kv3 = (d_ % 128 == 0 and d_ in (32 * enc.num_heads, 64 * enc.num_heads) and x0.shape[1] <= 256 and B_ * Ns_ >= 128 and 2 * len(uniq) <= MAXG and
               len(mems) * Ln_ <= MAXG and all(f.dtype == torch.float32 for f in uniq) and
               (prompt is None or (prompt.dtype == torch.float32 and (prompt.shape[0] * prompt.shape[1] * d_) % 8 == 0 and
                                   (x0.shape[0] * x0.shape[1] * d_) % 8 == 0)))
        if not kv3:
            ct = L.F32
    drop_base, mh_drop = None, False
    if training:   # the caller (QueryMaskEncoder.forward) has opened the RNG epoch (modules.begin_dropout_step)
        layers_ = list(enc.unified_encoder)
        ps = [m.dropout_p for l_ in layers_ for m in (list(l_.cross_attn_list) + [l_.self_attn, l_.ffn])]
        if any(p_ > 0.0 for p_ in ps):
            if any(len({c.dropout_p for c in l_.cross_attn_list}) > 1 for l_ in layers_):
                raise NotImplementedError("fused path: one dropout probability per layer's cross-attention list")
            drop_base = enc._drop_base
        mh_drop = mask_head is not None and mask_head.dropout_p > 0.0
    spec = FusedSpec(enc, mask_head, mems, ct, layer0.ffn.activation, enc.use_self_mask, enc.num_blocks,
                     enc.spatial_selfattn, mh_count, offline_attn_masks is not None, skip_prediction, drop_base, mh_drop)
    st = input_dict.get("_stacked_scene_kpm")
    if st is not None and list(st[1]) == list(mems) and st[0].is_contiguous() and \
            all(masks[j].data_ptr() == st[0][j].data_ptr() for j in range(len(mems))):
        spec.stacked_kpm = st[0]
    spec.src, spec.mh_src, spec.n_src = src, mh_src, len(uniq)
    spec.kv3 = kv3
    spec.prompt = prompt is not None
    params = [p for p in enc.parameters()] + ([p for p in mask_head.parameters()] if mask_head is not None else [])
    outs = _FusedDecoder.apply(spec, x0, qpos, qmask, poss[0], pairwise_locs, seg_masks, offline_attn_masks, coef,
                               prompt, pmask, *uniq, *masks, *params)
    query = outs[0]
    n = (len(outs) - 1) // 2
    return query, list(outs[1:1 + n]), list(outs[1 + n:1 + 2 * n])
