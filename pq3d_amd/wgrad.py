"""Weight-gradient launch policy: every parameter gradient dW[N, K] += g^T (x [+ x2]) (and db[N] += column sums of g) of the
package is planned and launched here -- which kernel runs it (pq3d_gemm_tt_multi for short reductions, bf16 operands on
128 x 128 tiles for long ones, grouped split-K pq3d_gemm otherwise), the split-K depth, whether the bias gradient rides on
the same launch, and the queue that defers products to a few grouped launches.  Callers keep the differences that are
theirs: the split-K cap, the max(2, .) floor, and whether the one-launch flush must pay for itself (tt_multi_pays)."""
from __future__ import annotations

import os
from typing import Sequence

import torch

from . import _lib as L
from ._lib import BF16

MAXG = L.MAXG
# PQ3D_DETERMINISTIC=1: reductions that have an order-independent form take it (today: bias-gradient column sums of long
# accumulating calls, include/pq3d_hip.h pq3d_colsum_grouped accumulate == 2).  Split-K weight gradients and the LayerNorm
# parameter gradients still add with fp32 atomics.
DETERMINISTIC = os.environ.get("PQ3D_DETERMINISTIC", "0") == "1"

SPLITK_CAP_LAYER = 512   # products launched where they arise (ops layers' backward; also the LM head's dx split)
SPLITK_CAP_FLUSH = 768   # products of a queue flush


def splitk(tiles: int, R: int, ct: int, cap: int) -> int:
    """Split-K depth of a reduction over R rows whose launch has `tiles` 64 x 64 output tiles (all groups together)."""
    nkt = max(1, R // (64 if ct == BF16 else 32))
    return max(1, min(nkt // 2 if nkt >= 2 else 1, cap // max(tiles, 1), 64))


def colsum_fusable(gs, xs, x2s, N: int, K: int, ct: int) -> bool:
    """Can the bias gradients (column sums of gs) ride on the weight-gradient launch?  Only on pq3d_gemm's aligned fast path."""
    epl = 8 if ct == BF16 else 4
    x2s = x2s if x2s is not None else [None] * len(xs)
    return N % epl == 0 and K % epl == 0 and N >= epl and K >= epl and \
        all(t.data_ptr() % 16 == 0 for t in list(gs) + list(xs)) and \
        all(x2 is None or (x2.dtype == torch.float32 and x.dtype == torch.float32) for x, x2 in zip(xs, x2s))


def dw_long_path(N: int, K: int, R: int, count: int, ct: int) -> bool:
    """A LONG reduction with enough 128 x 128 output tiles to fill the chip: operands rounded to bf16 once (dw_operands), then
    the 128 x 128-tile bf16 kernel (gemm_tt128) -- config 2's input encoders (3 groups of [256, 256] over 8192 rows = 12 tiles)
    are not: 14 us of rounding + 33 us against 29 us on the 64 x 64 chunk kernel, measured; config s2's 16-24 groups of
    [768, 768] = 576+ tiles are.  Short reductions are pq3d_gemm_tt_multi's."""
    return ct == BF16 and R >= 2048 and R % 64 == 0 and N % 128 == 0 and K % 128 == 0 and (N // 128) * (K // 128) * count >= 64


def dw_operands(gs, xs, x2s, N: int, K: int, R: int, ct: int):
    """Operands of weight-gradient products dW[N, K] += g^T (x [+ x2]) over a LONG reduction (R >= 2048 rows: the encoders'
    B * N_seg rows, every projection of the stage-2 shipped shape with its 128 x 80 object rows): fp32 operands are rounded to
    bf16 ONCE by one launch per operand shape -- the rounding the GEMM staging applies anyway, (x + x2) summed in fp32 first
    -- so that the product takes the 128 x 128-tile bf16 kernel (gemm_tt128_kernel: half the operand re-reads of the 64 x 64
    tile, 2 B per element instead of 4; config s2: 155 -> ~490 TFLOP/s on these launches).  Returns (gs, xs, x2s)."""
    if not dw_long_path(N, K, R, len(gs), ct):
        return gs, xs, x2s
    x2s = list(x2s) if x2s is not None else [None] * len(xs)
    if all(t.dtype == torch.bfloat16 for t in list(gs) + list(xs)) and all(t is None for t in x2s):
        return gs, xs, None
    if any(t.dtype != torch.float32 for t in x2s if t is not None) or \
            any(t.dtype == torch.bfloat16 and t2 is not None for t, t2 in zip(xs, x2s)):
        return gs, xs, (x2s if any(t is not None for t in x2s) else None)
    cache, jobs = {}, {}

    def conv(t, t2):
        if t.dtype == torch.bfloat16:
            return t
        key = (t.data_ptr(), t2.data_ptr() if t2 is not None else 0, t.numel())
        o = cache.get(key)
        if o is None:
            if t.numel() % 8 or t.data_ptr() % 16 or (t2 is not None and t2.data_ptr() % 16) or not t.is_contiguous():
                return None
            o = cache[key] = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
            jobs.setdefault(t.numel(), []).append((t, t2, o))
        return o
    g2 = [conv(t, None) for t in gs]
    x2 = [conv(t, t2) for t, t2 in zip(xs, x2s)]
    if any(t is None for t in g2 + x2):
        return gs, xs, (x2s if any(t is not None for t in x2s) else None)
    for n, lst in jobs.items():
        for s0 in range(0, len(lst), MAXG):
            ch = lst[s0:s0 + MAXG]
            L.call("pq3d_add_cast", *(L.parr([j[k] for j in ch]) for k in range(3)), len(ch), L.BF16, n)
    return g2, x2, None


def _colsum_acc(xs: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], rows: int) -> None:
    """outs[g] += column sums of xs[g] viewed as [rows, N] (bias gradients into the arena)."""
    N = xs[0].numel() // rows
    # operands of one output that lie back to back in memory (the mask head's calls write slices of one buffer) are one taller
    # operand: (first tensor, output, number of row blocks)
    merged = []
    for xt, ot in zip(xs, outs):
        if merged and merged[-1][1].data_ptr() == ot.data_ptr() and xt.dtype == merged[-1][0].dtype and \
                xt.data_ptr() == merged[-1][0].data_ptr() + merged[-1][2] * rows * N * xt.element_size():
            merged[-1][2] += 1
        else:
            merged.append([xt, ot, 1])
    for nblk in sorted({m_[2] for m_ in merged}):
        # a launch adds with one (non-atomic) writer per output element: outputs must be unique within a launch
        # (shared weights across num_blocks put the same bias slice in several groups) -> greedy batching
        batches, cur, seen = [], ([], []), set()
        for xt, ot, nb_ in merged:
            if nb_ != nblk:
                continue
            if ot.data_ptr() in seen or len(cur[0]) == MAXG:
                batches.append(cur)
                cur, seen = ([], []), set()
            cur[0].append(xt); cur[1].append(ot); seen.add(ot.data_ptr())
        batches.append(cur)
        for xc, oc in batches:
            # accumulate = 2: the one-writer (bit-reproducible) form at every row count; 1 lets long columns add row slices atomically
            L.call("pq3d_colsum_grouped", L.parr(xc), L.parr(oc), len(xc), L.dt_of(xc[0]), rows * nblk, N, N, 2 if DETERMINISTIC else 1)


def launch(gs, xs, x2s, dws, dbs, ct: int, cap: int, *, min2: bool = True, accumulate: bool = True, alpha: float = 1.0) -> None:
    """dws[i][N, K] (+)= alpha gs[i]^T (xs[i] + x2s[i]) for same-shape problems: long reductions on bf16 operands (dw_operands),
    then grouped split-K pq3d_gemm launches of <= MAXG groups.  dbs[i][N] += column sums of gs[i] rides on the same launch
    where colsum_fusable holds, else grouped column sums follow.  min2: split-K of at least 2 (the accumulating callers)."""
    N, K = dws[0].shape
    R = gs[0].numel() // N
    fuse = dbs is not None and colsum_fusable(gs, xs, x2s, N, K, ct)
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    gs, xs, x2s = dw_operands(gs, xs, x2s, N, K, R, ct)
    for i in range(0, len(gs), MAXG):
        sl = slice(i, i + MAXG)
        sk = splitk(tiles * len(gs[sl]), R, ct, cap)
        L.gemm(M=N, N=K, K=R, A=gs[sl], B=xs[sl], B2=x2s[sl] if x2s is not None else None, Cs=dws[sl], ct=ct, lda=N, ldb=K,
               ldc=K, transA=True, transB=True, splitk=max(2, sk) if min2 else sk, accumulate=accumulate, alpha=alpha,
               colsum=dbs[sl] if fuse else None)
    if dbs is not None and not fuse:
        _colsum_acc(gs, dbs, R)


def ragged_fits(gs, xs, N: int, K: int, Rs, ct: int) -> bool:
    """Can dW_i[N, K] += g_i^T x_i over DIFFERENT long row counts Rs share one grouped launch (pq3d_gemm_desc.Kg: the whole-chunk
    kernel with a reduction length per group)?  Only products that the per-class launches would send to that kernel anyway: single-
    bf16 products of rows too many for pq3d_gemm_tt_multi (R >= 2048) and too few tiles for the 128 x 128-tile kernel."""
    if ct != BF16 or len(gs) > MAXG or N % 8 or K % 8 or min(Rs) < 2048 or len({t.dtype for t in gs}) > 1 or len({t.dtype for t in xs}) > 1:
        return False
    if any(dw_long_path(N, K, r, sum(1 for q in Rs if q == r), ct) for r in set(Rs)):
        return False
    if gs[0].dtype == torch.bfloat16 and xs[0].dtype == torch.bfloat16:   # the 128 x 128-tile kernel's operands
        return False
    return all(t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in list(gs) + list(xs))


def launch_ragged(gs, xs, dws, dbs, Rs) -> None:
    """dws[i][N, K] += gs[i]^T xs[i] over Rs[i] rows, dbs[i][N] += column sums of gs[i]: ONE split-K launch (see ragged_fits)."""
    N, K = dws[0].shape
    L.gemm(M=N, N=K, K=max(Rs), A=list(gs), B=list(xs), Cs=list(dws), ct=BF16, lda=N, ldb=K, ldc=K, transA=True, transB=True, splitk=2,
           accumulate=True, colsum=list(dbs), Kg=list(Rs))


def tt_multi_ok(g, x, x2, dw, db, N: int, K: int, R: int) -> bool:
    """Can dW[N, K] += g^T (x [+ x2]) (+ db[N] += colsum g) join the one-launch flush (pq3d_gemm_tt_multi)?  Not for long
    reductions (R >= 2048): config 2's 3 encoders of [256 x 256] over 8192 rows measured slower there (k-slices x 256 x 128
    tiles = 3x the atomics of the 64 x 64 split: c4 +1.0 %, c2 +0.2 .. 1.7 % on the same box)."""
    if R >= 2048 or R < 1 or N % 8 or K % 8 or N < 8 or K < 8 or R * max(N, K) >= (1 << 31):
        return False
    for t in (g, x):
        if t.dtype not in (torch.float32, torch.bfloat16) or not t.is_contiguous() or t.data_ptr() % 16:
            return False
    if x2 is not None and (x2.dtype != torch.float32 or x.dtype != torch.float32 or not x2.is_contiguous() or x2.data_ptr() % 16):
        return False
    if dw.dtype != torch.float32 or not dw.is_contiguous() or (db is not None and (db.dtype != torch.float32 or not db.is_contiguous())):
        return False
    return g.numel() == R * N and x.numel() == R * K


def tt_multi_fits(problems, N: int, K: int, R: int, ct: int) -> bool:
    """Can every problem (g, x, x2, dw, db) of one shape join pq3d_gemm_tt_multi?  Long reductions over many tiles
    (dw_long_path) stay on the 128 x 128-tile bf16 kernel."""
    return ct == BF16 and not dw_long_path(N, K, R, len(problems), ct) and all(tt_multi_ok(*p, N, K, R) for p in problems)


def tt_multi_pays(problems) -> bool:
    """The one-launch flush wins through its 256 x 128 tiles (2.5-3x fewer operand re-reads from L2) while those fit about one
    round of workgroups (<= 400 wide tiles: the decoder's flush at configs 2 / 4 / 5); a flush WITHOUT such a launch -- the
    caption body's ~660 wide tiles over 512 rows, which the library sends back to 64 x 64 tiles -- is faster as one
    gemm_wktt launch per (shape, dtype) bucket (config 5, same box: 6.21 vs 6.27 ms per step)."""
    wt = sum((dw.shape[-2] // 256) * (dw.shape[-1] // 128) for _g, _x, _x2, dw, _db in problems
             if dw.shape[-2] % 256 == 0 and dw.shape[-1] % 128 == 0)
    return 0 < wt <= 400


def tt_multi(problems) -> None:
    """problems: [(g [R,N], x [R,K], x2 or None, dw [N,K], db [N] or None)] -- every weight (and bias) gradient of a flush in
    ONE launch per 56 problems (csrc/gemm_ttmulti.hip) instead of one launch per (shape, dtype) bucket."""
    for s0 in range(0, len(problems), L.TT_MAX_PROBLEMS):
        ch = problems[s0:s0 + L.TT_MAX_PROBLEMS]
        arr = (L.TtProblem * len(ch))()
        fl = nb = 0.0
        for q, (g, x, x2, dw, db) in zip(arr, ch):
            N, K = dw.shape[-2], dw.shape[-1]
            R = g.numel() // N
            q.M, q.N, q.K, q.lda, q.ldb = N, K, R, N, K
            q.dtA, q.dtB = L.dt_of(g), L.dt_of(x)
            q.A, q.B, q.B2, q.C, q.colsum = L.ptr(g), L.ptr(x), L.ptr(x2), L.ptr(dw), L.ptr(db)
            fl += 2.0 * N * K * R
            nb += float(g.numel() * g.element_size() + x.numel() * x.element_size() + (x2.numel() * x2.element_size() if x2 is not None else 0)
                        + N * K * 4 + (N * 4 if db is not None else 0))   # compulsory: both operands once, the fp32 result (+ bias gradient)
        L.call("pq3d_gemm_tt_multi", arr, len(ch), work=(f"ttmulti{len(ch)}", fl, nb))


class Queue:
    """Deferred weight-gradient products.  A dW = g^T (x [+ x2]) that only feeds a gradient slot need not run when it arises:
    it is queued and flushed as a few launches -- one pq3d_gemm_tt_multi for every short reduction when that pays, grouped
    split-K launches per (shape, dtype) bucket for the rest -- instead of one launch per linear layer (c2's decoder: 41
    launches -> 6).  Buckets keep insertion order.  split_x2: products with and without an x2 addend go to separate buckets
    (the whole-pass queue); without it they share one (the decoder's queue: one launch takes a mixed x2 list)."""

    def __init__(self, split_x2: bool):
        self.split_x2 = split_x2
        self.buckets, self.nbytes = {}, 0   # nbytes: operand bytes the queue keeps alive

    def add(self, gs, xs, x2s, dws, ct: int, dbs=None) -> None:
        for i, (g, x, dw) in enumerate(zip(gs, xs, dws)):
            x2 = x2s[i] if x2s is not None else None
            db = dbs[i] if dbs is not None else None
            N, K = dw.shape
            key = (N, K, g.numel() // N, g.dtype, x.dtype, x2 is not None if self.split_x2 else None, db is not None, ct)
            self.buckets.setdefault(key, []).append((g, x, x2, dw, db))
            self.nbytes += g.numel() * g.element_size() + x.numel() * x.element_size() + \
                (x2.numel() * x2.element_size() if x2 is not None else 0)

    def flush(self, run: bool = True) -> None:
        """Launch (run=False: drop) the queued products."""
        # (forking the buckets over 3 / 5 streams -- parallel branches of the captured graph -- was measured at config 2:
        # 1.50 -> 1.80 / 2.17 ms; branch joins cost far more than the overlapped tails save)
        buckets, self.buckets, self.nbytes = self.buckets, {}, 0
        if not run:
            return
        multi, rest = [], {}
        for key, probs in buckets.items():
            if tt_multi_fits(probs, key[0], key[1], key[2], key[7]):
                multi += probs
            else:
                rest[key] = probs
        if multi and tt_multi_pays(multi):   # every short-reduction weight / bias gradient of the flush: ONE launch
            tt_multi(multi)
        else:
            rest = buckets
        for key, probs in rest.items():
            gs, xs, x2s, dws, dbs = (list(c) for c in zip(*probs))
            launch(gs, xs, x2s if any(t is not None for t in x2s) else None, dws, dbs if key[6] else None, key[7], SPLITK_CAP_FLUSH)
