"""Flat float64 restatement of the optimizer side of the training step -- the checker of pq3d_amd/csrc/optim.hip
(pq3d_sumsq_partials, pq3d_train_scalars, pq3d_adamw) and of pq3d_amd.trainer.TrainStep.optimizer_step.  Not imported
by the product.

oracle/train_oracle.py states the same step per parameter (``adamw_step``, pinned against the reference's optimizer and
scheduler by tests/test_train_oracle.py).  Here the step is written over ONE flat buffer cut into segments
``(end, lr_mul, weight_decay)``, as pq3d_opt_segments describes it: a segment's learning rate is ``lr * lr_mul``, a
segment with ``lr_mul < 0`` is a parameter without a gradient this step and stays untouched (torch.optim.AdamW skips a
``grad is None`` parameter), and the bias corrections use the one global step count.  tests/test_optim_ref.py checks
this restatement against torch.optim.AdamW, clip_grad_norm_ and LambdaLR in float64."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from oracle import train_oracle as T

Segment = Tuple[int, float, float]     # (exclusive end offset, lr_mul (< 0: skip), weight_decay)


# Segment values for the tables below, cycled over the non-empty live segments: neighbouring lr_mul differ by 2x or more,
# so an element updated with its neighbour's values moves by at least half an update away from where it should be.
LR_MULS = (1.0, 3.0, 0.5, 2.0)
WEIGHT_DECAYS = (0.01, 0.05, 0.0, 0.02)
EMPTY = (7.0, 0.3)          # values of empty segments: an element that picks these up is visibly wrong
SKIP = (-1.0, 0.0)          # what TrainStep._segments writes for a parameter without a gradient


def _assign(ends, live):
    """Segment table from ``ends`` (clipped, non-decreasing) and a live flag per segment; values cycle over the
    non-empty live segments, skip segments get SKIP, empty ones EMPTY."""
    out, k, start = [], 0, 0
    for e, is_live in zip(ends, live):
        if not is_live:
            out.append((e, *SKIP))
        elif e <= start:
            out.append((e, *EMPTY))
        else:
            out.append((e, LR_MULS[k % 4], WEIGHT_DECAYS[k % 4]))
            k += 1
        start = max(start, e)
    return out


def segment_tables(n: int):
    """The segment tables the tests run at every size n:
    one      -- a single segment ending exactly at n;
    sixteen  -- PQ3D_MAX_OPT_SEGMENTS segments, ends at offsets = 1, 2 and 3 (mod 4), three boundaries inside the second
                float4 (ends 5, 6, 7), boundaries inside the first float4 the grid-stride loop reaches on its second
                pass (2048 blocks x 256 threads x 4 = 2097152), inside the last float4 and the n % 4 tail, last end > n;
    skip     -- skip segments between live ones inside the first two float4s, a skipped last element, last end > n."""
    half = (n // 2) // 4 * 4 + 3
    ends = sorted(min(max(e, 0), n) for e in (5, 6, 7, 9, 14, 19, 30, half, 1021, 1022, 4094, 2097153, 2097158,
                                                 n - 2, n - 1)) + [n + 5]
    sk_ends = [min(e, n) for e in (1, 2, 3, 6, 7, 13, max(14, n - 1))] + [n + 2]
    return {"one": _assign([n], [True]),
            "sixteen": _assign(ends, [True] * 16),
            "skip": _assign(sk_ends, [True, False, True, False, True, False, True, False])}


def lr_factor(sched: str, done: int, warmup: int, total: int, gamma: float = 1.0, stride: int = 1) -> float:
    """LambdaLR factor of the optimizer step that follows ``done`` steps.  ``warmup`` is already scaled by the number of
    processes (optim/scheduler.py:20) and ``stride`` scheduler steps are taken per optimizer step (the accelerate-prepared
    LambdaLR), so the factor is lambda(done * stride): train_oracle.adamw_step's ``num_gpu`` schedule."""
    return T.lr_factor(sched, done * max(int(stride), 1), warmup, total, gamma)


def clip_coef(norm: float, max_norm: Optional[float]) -> float:
    """torch.nn.utils.clip_grad_norm_ in float64: clamp(max_norm / (norm + 1e-6), max=1); no clipping if max_norm is
    0 / None (train_oracle.clip_coef, without its rounding of the norm to fp32)."""
    return min(1.0, max_norm / (norm + 1e-6)) if max_norm and max_norm > 0 else 1.0


def scalars(*, lr: float, beta1: float, beta2: float, max_norm: Optional[float], sched: str, warmup: int, total: int,
            gamma: float, stride: int, done: int, norm: float):
    """pq3d_train_scalars' outputs for optimizer step ``done + 1``: (lr, lr / bc1, 1 / sqrt(bc2), clip coefficient,
    norm), with bc = 1 - beta^(done + 1)."""
    t = done + 1
    lr_t = lr * lr_factor(sched, done, warmup, total, gamma, stride)
    return lr_t, lr_t / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t), clip_coef(norm, max_norm), norm


def segment_slices(segs: Sequence[Segment], n: int):
    """(slice, lr_mul, weight_decay) per non-empty segment; ends are clipped to n, a segment starts where the last
    one ended."""
    out, start = [], 0
    for end, lm, wd in segs:
        e = min(int(end), n)
        if e > start:
            out.append((slice(start, e), float(lm), float(wd)))
        start = max(start, e)
    assert start == n, "the segment table must cover [0, n)"
    return out


def adamw_flat(p, g, m, v, segs: Sequence[Segment], *, lr: float, step_size: float, inv_bc2s: float, coef: float,
               beta1: float, beta2: float, eps: float) -> None:
    """One AdamW step IN PLACE on flat float64 tensors (torch.optim.AdamW's arithmetic, amsgrad=False): per segment
    g' = coef * g; p *= 1 - lr * lr_mul * wd; m = lerp(m, g', 1 - beta1); v = beta2 v + (1 - beta2) g'^2;
    p -= step_size * lr_mul * m / (sqrt(v) * inv_bc2s + eps).  Skip segments stay untouched."""
    for sl, lm, wd in segment_slices(segs, p.numel()):
        if lm < 0:
            continue
        gr = g[sl] * coef
        p[sl] *= 1.0 - lr * lm * wd
        m[sl] += (gr - m[sl]) * (1.0 - beta1)
        v[sl] = v[sl] * beta2 + (1.0 - beta2) * gr * gr
        p[sl] -= step_size * lm * m[sl] / (v[sl].sqrt() * inv_bc2s + eps)


class FlatAdamW:
    """The whole optimizer step on a flat float64 state: norm over the WHOLE flat gradient (TrainStep zeroes the
    gradient of skipped parameters, so they add nothing), schedule, clip, AdamW, global step count."""

    def __init__(self, p, *, lr: float, betas=(0.9, 0.98), eps: float = 1e-8, max_norm: Optional[float] = None,
                 sched: str = "warmup_cosine", warmup: int = 0, total: int = 1, gamma: float = 1.0, stride: int = 1):
        self.p = p.double().clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.lr, self.betas, self.eps, self.max_norm = lr, betas, eps, max_norm
        self.sched, self.warmup, self.total, self.gamma, self.stride = sched, warmup, total, gamma, stride
        self.done = 0

    def step(self, g, segs: Sequence[Segment]):
        g = g.double()
        norm = float(torch.linalg.vector_norm(g))
        sc = scalars(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], max_norm=self.max_norm, sched=self.sched,
                     warmup=self.warmup, total=self.total, gamma=self.gamma, stride=self.stride, done=self.done, norm=norm)
        adamw_flat(self.p, g, self.m, self.v, segs, lr=sc[0], step_size=sc[1], inv_bc2s=sc[2], coef=sc[3],
                   beta1=self.betas[0], beta2=self.betas[1], eps=self.eps)
        self.done += 1
        return sc
