"""Shared by the GPU tests of the grouped Linear+LayerNorm encoders (test_gpu_enc_ln.py, test_gpu_enc_ragged.py,
test_gpu_enc_launches.py): seeded operands, the bit comparison, the reordering bound and the launch spies."""
import torch

from pq3d_amd import _lib as L

DEV = "cuda"
N = 256


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).float()


def _params(G, K, n=N):
    Ws = [rnd(n, K, seed=50 + g, scale=0.06).to(DEV) for g in range(G)]
    bs = [rnd(n, seed=60 + g, scale=0.1).to(DEV) for g in range(G)]
    gs = [(1 + rnd(n, seed=70 + g, scale=0.1)).to(DEV) for g in range(G)]
    be = [rnd(n, seed=80 + g, scale=0.1).to(DEV) for g in range(G)]
    return Ws, bs, gs, be


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _order_bound(contrib_abs, terms):
    """Largest difference between two fp32 sums of the same `terms` addends taken in different orders: each order is within
    (terms - 1) 2^-24 sum|addend| of the exact sum (first-order bound of recursive summation), so two orders are within twice that."""
    return 2.0 * max(terms - 1, 1) * 2.0 ** -24 * contrib_abs


def _count_calls(monkeypatch):
    """Names of the launches that go through L.call; an independent-branch LayerNorm backward (only the grouped Linear+LN op
    issues one) is recorded as 'pq3d_add_ln_bwd:i'."""
    seen = []
    real = L.call

    def spy(name, *a, **kw):
        seen.append(name + ":i" if name == "pq3d_add_ln_bwd" and a[0].independent else name)
        return real(name, *a, **kw)
    monkeypatch.setattr(L, "call", spy)
    return seen


def _record_launches(monkeypatch):
    """(entry point, work key) of every launch that goes through L.call, in order; the key is what names the launch for the
    profiler (None where the caller gives none)."""
    seen = []
    real = L.call

    def spy(name, *a, **kw):
        seen.append((name, (kw.get("work") or (None,))[0]))
        return real(name, *a, **kw)
    monkeypatch.setattr(L, "call", spy)
    return seen
