"""float64 restatements, input builders, case lists and tolerance helpers for the small kernels of pq3d_amd/csrc/misc.hip
(pairwise locations, Fourier features, spatial attention bias, gate mix, gelu backward and the glue around them).

Every restatement takes a ``dtype``: numpy float64 is the reference the GPU tests compare with; numpy float32 walks the same
formula with plain fp32 operations in the kernels' order and is what tests/test_misc_ref.py holds to SHARE = 0.6 of each
bound on the CPU, so that a bound is known to have room before a kernel ever meets it.  The bounds are forward error bounds
of fp32 arithmetic without contraction (the library is built with -ffp-contract=off), u = 2^-24:

  pairwise_locs   8 u absolute on each of the five channels (outputs in [-1, 1], non-negative sums under the roots)
  fourier         6 u sum_c |t_c G[c, j]| + 4 u, t_c = 2 pi x the normalised coordinate, in float64
  spatial bias    v the float64 pre-activation, mag = |bw_h| + sum_c |W[h, c] f_c|, TAU = 1e-3:
                    v >= TAU   |out - log v| <= 7 u mag / v + 4 u max(1, |log v|)
                    v <= -TAU  out = float32(log(float32(1e-6))) within 2 fp32 ulp
                    |v| < TAU  (the band) out finite and in [log 1e-6 - 1e-5, log(2 TAU)]: log next to the relu / clamp corner
                               is unboundedly ill-conditioned, band elements are never compared numerically
  its backward    upstream gradient zero on band elements; g = dbias / v (v >= TAU), else 0;
                    tol dW[h, c] = sum_i |g_i f_ic| (7 u mag_i / v_i + 4 u) + n u sum_i |g_i f_ic|, n = B L L (the second
                    term bounds a sum in ANY order: it covers the atomics); dbw[h] the same with f = 1
                  accumulating entry: the value P found in dW / dbw is one more addend, touched by one atomic add per block
                    (blocks = min(ceil(ceil(n / 4) / 256), 512)), each rounding at most u (|P| + |dW|): + (blocks + 1) u (|P| + |dW|)
                  one-hot upstream gradient: the single term g f_c / v within 8 u |term|, every other head exactly 0
  gate mix        y within 16 u (|q| + |u|); dq, du within 16 u |dy|; dg within 16 u |dy| (|q| + |u|)
  gelu backward   16 u |dy| absolute (fp32 output)
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
TAU = 1e-3
SHARE = 0.6          # the float32 restatement's share of each bound (tests/test_misc_ref.py)
BAND_CAP = 0.01      # at most this share of a spatial-bias case's elements may lie in the band
ONEHOT_MIN_V = 0.1   # a one-hot upstream gradient sits where the pre-activation is at least this
CLAMP32 = np.float32(1e-6)
LOG_CLAMP32 = np.float32(math.log(float(CLAMP32)))
TWO_PI32 = np.float32(6.283185307179586)


def _rng(*key):
    return np.random.default_rng(list(key))


def ulps32(a, b):
    """Distance in fp32 grid steps between same-sign float32 arrays."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def bf16_ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 values as integers in value order (sign-magnitude bits folded: -0 and +0 both 0, neighbours differ by 1 across
    zero too), so that a difference counts bf16 grid steps."""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, 0x8000 - b, b)


# ------------------------------------------------------------------------------------------------ pairwise locations
PL_CASES = [(L, B) for L in (1, 7, 8, 9, 33, 65, 257) for B in (1, 3)]
PL_TOL = 8 * U


def pl_centres(L, B):
    """Centres uniform in [0, 4]^3; scene 0 holds a coincident pair (0, 1), a vertically stacked pair (2, 3: dx = dy = 0) and a
    pair 1e-6 apart (4, 5) as far as L allows."""
    c = (_rng(1, L, B).random((B, L, 3)) * 4).astype(np.float32)
    if L >= 2:
        c[0, 1] = c[0, 0]
    if L >= 4:
        c[0, 3] = c[0, 2]
        c[0, 3, 2] += np.float32(0.75)
    if L >= 6:
        c[0, 5] = c[0, 4]
        c[0, 5, 0] += np.float32(1e-6)
        assert c[0, 5, 0] != c[0, 4, 0]
    return c


def pairwise_locs(c, eps=1e-10, dtype=np.float64):
    """[B, L, 3] -> [B, L, L, 5]: (dist / max dist, dz / dist, d2 / dist, dy / d2, dx / d2), dist = sqrt(|d|^2 + eps),
    d2 = sqrt(dx^2 + dy^2 + eps), d = c_i - c_j."""
    c = np.asarray(c).astype(dtype)
    eps = dtype(eps)
    d = c[:, :, None, :] - c[:, None, :, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    dist = np.sqrt(dx * dx + dy * dy + dz * dz + eps)
    d2 = np.sqrt(dx * dx + dy * dy + eps)
    mx = dist.reshape(dist.shape[0], -1).max(1)[:, None, None]
    return np.stack([dist / mx, dz / dist, d2 / dist, dy / d2, dx / d2], -1)


# ------------------------------------------------------------------------------------------------ Fourier features
FOURIER_B = 3
FOURIER_CASES = [(half, na, nb) for half in (1, 32, 96, 128, 384) for na, nb in ((40, 77), (0, 5), (5, 0), (1, 1))]


def fourier_inputs(half, Na, Nb):
    """(xa6 [3, Na, 6] whose [..., :3] is point set a, xb [3, Nb, 3], cmin, cmax [3, 3], G [3, half]); a box of its own per scene,
    points up to a quarter of its extent outside it."""
    r = _rng(2, half, Na, Nb)
    cmin = np.array([[0, 0, 0], [-1, -1, 0], [0.5, -2, -0.25]], np.float32)
    cmax = np.array([[4, 4, 4], [5, 4, 3], [3.5, 2, 2.75]], np.float32)
    ext = (cmax - cmin)[:, None, :]

    def pts(n, w):
        x = r.random((FOURIER_B, n, w)).astype(np.float32)
        x[..., :3] = cmin[:, None, :] + (x[..., :3] * 1.5 - 0.25) * ext
        return x.astype(np.float32)
    return pts(Na, 6), pts(Nb, 3), cmin, cmax, r.standard_normal((3, half)).astype(np.float32)


def fourier(xyz, cmin, cmax, G, dtype=np.float64):
    """[B, N, 3] -> ([B, N, 2 half] = [sin | cos](proj), mag [B, N, half] = sum_c |t_c G[c, j]|)."""
    xyz, cmin, cmax, G = (np.asarray(a).astype(dtype) for a in (xyz, cmin, cmax, G))
    two_pi = TWO_PI32 if dtype is np.float32 else 2 * math.pi
    t = (xyz - cmin[:, None, :]) / (cmax[:, None, :] - cmin[:, None, :])
    t = t * two_pi
    proj = np.zeros(xyz.shape[:2] + (G.shape[1],), dtype)
    mag = np.zeros_like(proj)
    for c in range(3):
        term = t[..., c, None] * G[c]
        proj = proj + term
        mag = mag + np.abs(term)
    return np.concatenate([np.sin(proj), np.cos(proj)], -1), mag


def fourier_tol(mag64):
    tol = 6 * U * mag64 + 4 * U
    return np.concatenate([tol, tol], -1)


# ------------------------------------------------------------------------------------------------ spatial bias
SB_HEADS = (1, 4, 8, 9, 12, 16)          # 8 -> 9 switches the backward template
SB_BL = ((1, 1), (2, 7), (1, 16), (1, 32), (1, 33), (3, 23))   # B L L = 256, 1024 fill whole blocks, 1089 leaves a partial one
SB_BIG = (8, 257, 4)                     # more elements than 512 blocks x 256 threads x 4: grid cap, second stride iteration
SB_CASES = [(B, L, H) for B, L in SB_BL for H in SB_HEADS] + [SB_BIG]
# the first seed of a case that misses none of the conditions of sb_case_misses, where that is not seed 0
SB_SEED = {(1, 1, 4): 2, (2, 7, 1): 7, (2, 7, 8): 1, (1, 33, 1): 3, (3, 23, 1): 2, (8, 257, 4): 2}


def sb_groups(B, L, H):
    """Weight sets of the 32-group forward: 32 of their own, 3 (repeated) for the grid-capped case."""
    return 3 if (B, L, H) == SB_BIG else 32


def sb_inputs(B, L, H, group=0, seed=None):
    """(centres [B, L, 3] uniform in [0, 4]^3, W [H, 5], bw [H] ~ N(0, 0.5^2)); ``group`` draws other weights, same centres."""
    seed = SB_SEED.get((B, L, H), 0) if seed is None else seed
    c = (_rng(3, B, L, seed).random((B, L, 3)) * 4).astype(np.float32)
    r = _rng(4, B, L, H, seed, group)
    return c, (r.standard_normal((H, 5)) * 0.5).astype(np.float32), (r.standard_normal(H) * 0.5).astype(np.float32)


def sb_pre(pl, W, bw, dtype=np.float64):
    """Pre-activation v [B, H, LL] = bw_h + sum_c W[h, c] f_c (c ascending, as the kernels add) and mag of the same shape."""
    B = pl.shape[0]
    f = np.asarray(pl).reshape(B, -1, 5).astype(dtype)
    W, bw = np.asarray(W).astype(dtype), np.asarray(bw).astype(dtype)
    v = np.broadcast_to(bw[None, :, None], (B, W.shape[0], f.shape[1])).copy()
    mag = np.abs(v)
    for c in range(5):
        term = W[None, :, c, None] * f[:, None, :, c]
        v = v + term
        mag = mag + np.abs(term)
    return v, mag


def sb_fwd(pl, W, bw, dtype=np.float64):
    """log(max(max(v, 0), 1e-6)) as [B, H, LL]."""
    v, _ = sb_pre(pl, W, bw, dtype)
    return np.log(np.maximum(np.maximum(v, dtype(0)), dtype(CLAMP32)))


def sb_band(v64):
    return np.abs(v64) < TAU


def sb_fwd_report(out, v64, mag64):
    """Figures of a forward result [B, H, LL] against the float64 pre-activation: 'share' = worst error / bound over v >= TAU,
    'neg_ulps' = worst fp32 grid distance from log(1e-6) over v <= -TAU, 'band_ok', 'band_share'."""
    out = np.asarray(out, np.float32).reshape(v64.shape)
    pos, neg, band = v64 >= TAU, v64 <= -TAU, sb_band(v64)
    rep = {"share": 0.0, "neg_ulps": 0, "band_share": float(band.mean()), "band_ok": True}
    if pos.any():
        lv = np.log(v64[pos])
        tol = 7 * U * mag64[pos] / v64[pos] + 4 * U * np.maximum(1.0, np.abs(lv))
        rep["share"] = float((np.abs(out[pos].astype(np.float64) - lv) / tol).max())
    if neg.any():
        rep["neg_ulps"] = int(ulps32(out[neg], np.full(int(neg.sum()), LOG_CLAMP32)).max())
    if band.any():
        ob = out[band].astype(np.float64)
        rep["band_ok"] = bool(np.isfinite(ob).all() and (ob >= math.log(1e-6) - 1e-5).all() and (ob <= math.log(2 * TAU)).all())
    return rep


def sb_assert_fwd(out, v64, mag64, share=1.0, what=""):
    rep = sb_fwd_report(out, v64, mag64)
    print(f"spatial bias forward {what}: {rep}")
    assert np.isfinite(np.asarray(out)).all(), what
    assert rep["share"] <= share, (what, rep)
    assert rep["neg_ulps"] <= 2, (what, rep)
    assert rep["band_ok"], (what, rep)
    return rep


def sb_upstream(B, L, H, v64, seed=0):
    """Dense N(0, 1) upstream gradient [B, H, LL], zero on band elements (both sides then contribute exactly nothing there)."""
    g = _rng(5, B, L, H, seed).standard_normal(v64.shape).astype(np.float32)
    g[sb_band(v64)] = 0
    return g


def sb_bwd(pl, W, bw, dbias, dtype=np.float64):
    """(dW [H, 5], dbw [H]) of sum(dbias * out): g = dbias / v where the clamp passes, 0 elsewhere.  float64 takes v >= TAU as
    'passes' (the upstream gradient is zero in the band, v <= -TAU never passes); float32 the kernel's own v > 1e-6."""
    B = pl.shape[0]
    f = np.asarray(pl).reshape(B, -1, 5).astype(dtype)
    v, _ = sb_pre(pl, W, bw, dtype)
    db = np.asarray(dbias).reshape(v.shape).astype(dtype)
    ok = v > dtype(CLAMP32) if dtype is np.float32 else v >= TAU
    g = np.where(ok, db / np.where(ok, v, dtype(1)), dtype(0))
    dW = np.stack([(g * f[:, None, :, c]).sum((0, 2), dtype=dtype) for c in range(5)], -1)
    return dW, g.sum((0, 2), dtype=dtype)


def sb_bwd_tol(pl, v64, mag64, dbias):
    B = pl.shape[0]
    f = np.abs(np.asarray(pl).reshape(B, -1, 5).astype(np.float64))
    ok = v64 >= TAU
    vs = np.where(ok, v64, 1.0)
    g = np.where(ok, np.abs(np.asarray(dbias).reshape(v64.shape).astype(np.float64)) / vs, 0.0)
    rel = 7 * U * mag64 / vs + 4 * U
    n = v64.shape[0] * v64.shape[2]
    tW = np.stack([(g * f[:, None, :, c] * rel).sum((0, 2)) + n * U * (g * f[:, None, :, c]).sum((0, 2)) for c in range(5)], -1)
    return tW, (g * rel).sum((0, 2)) + n * U * g.sum((0, 2))


def sb_blocks(n):
    """Blocks of the backward launch over n = B L L elements: 256 threads x 4 elements each, at most 512 blocks."""
    return min(-(-(-(-n // 4)) // 256), 512)


def sb_onehot_elements(n):
    """Flat element indices (of B L L) for one-hot upstream gradients: the first and the last element and the elements on
    either side of every edge of the backward launch's walk, worked out from n alone: blocks of 256 threads, four elements
    per thread a stride st = 256 x blocks apart (+ 4 st per further iteration), blocks = min(ceil(ceil(n / 4) / 256), 512).
    The edges are all multiples of 256 (block boundaries) and of st (per-thread strides, iterations) below n."""
    st = 256 * sb_blocks(n)
    el = {0, n - 1}
    for e in set(range(256, n, 256)) | set(range(st, n, st)):
        el |= {e - 1, e}
    return sorted(el)


def sb_onehot_pick(v64, mag64, elem, h0=None):
    """(element, head) for a one-hot upstream gradient at flat element ``elem``: head h0 there if it is given and has
    v >= ONEHOT_MIN_V; otherwise, at the nearest element that has such a head (``elem`` itself first), the head whose v is the
    best conditioned (largest v / mag: the rounding of v spends mag / v of the 8 u the term is held to).  None when the case
    has no such position."""
    B, H, LL = v64.shape
    n = B * LL
    if h0 is not None and v64[elem // LL, h0, elem % LL] >= ONEHOT_MIN_V:
        return elem, h0
    for dist in range(n):
        for e in ((elem,) if dist == 0 else (elem + dist, elem - dist)):
            if 0 <= e < n:
                vv, mm = v64[e // LL, :, e % LL], mag64[e // LL, :, e % LL]
                if (vv >= ONEHOT_MIN_V).any():
                    return e, int(np.argmax(np.where(vv >= ONEHOT_MIN_V, vv / mm, -1.0)))
    return None


def sb_onehot_share32(pl, W, bw, v64, positions, g=1.375):
    """Worst share of 8 u |term| that the float32 restatement of the one-hot terms takes over ``positions``."""
    B = pl.shape[0]
    f = np.asarray(pl, np.float32).reshape(B, -1, 5)
    v32, _ = sb_pre(pl, W, bw, dtype=np.float32)
    LL, worst = f.shape[1], 0.0
    for e, h in positions:
        b, ij = divmod(e, LL)
        want = sb_onehot_terms(g, v64[b, h, ij], f[b, ij])
        got = sb_onehot_terms(np.float32(g), v32[b, h, ij], f[b, ij])
        nz = want != 0
        worst = max(worst, float((np.abs(got[nz].astype(np.float64) - want[nz]) / (8 * U * np.abs(want[nz]))).max()))
    return worst


def sb_case_misses(B, L, H, seed):
    """The conditions a seed of a spatial-bias case has to meet, as the list of those it misses (tests/test_misc_ref.py holds
    every case to an empty list, and every entry of SB_SEED to being the first seed with one): the band holds at most BAND_CAP
    of the elements for every group of weights; a one-hot position exists; the float32 restatement of the one-hot terms stays
    under SHARE of 8 u |term| at the positions chosen."""
    c, W, bw = sb_inputs(B, L, H, seed=seed)
    pl = pairwise_locs(c, dtype=np.float32)
    v, mag = sb_pre(pl, W, bw)
    miss = []
    for g in range(sb_groups(B, L, H)):
        vg = v if g == 0 else sb_pre(pl, *sb_inputs(B, L, H, group=g, seed=seed)[1:])[0]
        if float(sb_band(vg).mean()) > BAND_CAP:
            miss.append(f"band of group {g}")
    pos = sb_onehot_positions(v, mag)
    if not pos:
        miss.append("no one-hot position")
    elif sb_onehot_share32(pl, W, bw, v, pos) > SHARE:
        miss.append("one-hot float32 share")
    return miss


def sb_onehot_terms(g, v, f):
    """The six sums (dW[h, 0..4], dbw[h]) a single upstream element g leaves at pre-activation v, features f [5]; computed in
    the type of v (float64, or float32 in the kernel's order: g / v first, then the products)."""
    t = type(v)
    q = t(g) / v
    return np.append(q * f.astype(t), q).astype(t)


def sb_onehot_positions(v64, mag64):
    """[(element, head)] for the one-hot backward checks of a case: the first element (head 0), the last element (head H - 1)
    and the edge elements of sb_onehot_elements."""
    B, H, LL = v64.shape
    n = B * LL
    out = {}
    for e in sb_onehot_elements(n):
        p = sb_onehot_pick(v64, mag64, e, 0 if e == 0 else (H - 1 if e == n - 1 else None))
        if p is not None:
            out[p] = None
    return list(out)


# ------------------------------------------------------------------------------------------------ gate mix
GATE_N = (1, 255, 256, 257, 4096 * 256 + 3)     # the last: grid cap (4096 blocks) and the grid stride
GATE_SPECIAL = (0.0, 20.0, -20.0, 100.0, -100.0)   # at +-100 the fp32 sigmoid is exactly 1 / 0: y = u / q exactly


def gate_inputs(n, k=0):
    """q, u, g, dy [n]; g ~ N(0, 2^2) with GATE_SPECIAL (rotated by k) over the first and the last five elements."""
    r = _rng(6, n)
    q, u, dy = (r.standard_normal(n).astype(np.float32) for _ in range(3))
    g = (r.standard_normal(n) * 2).astype(np.float32)
    for i in range(min(n, 5)):
        g[i] = GATE_SPECIAL[(i + k) % 5]
        g[n - 1 - i] = GATE_SPECIAL[(i + k) % 5]
    return q, u, g, dy


def gate_mix(q, u, g, dy, dtype=np.float64):
    """(y, dq, du, dg) of y = (1 - s) q + s u, s = 1 / (1 + exp(-g))."""
    q, u, g, dy = (np.asarray(a).astype(dtype) for a in (q, u, g, dy))
    with np.errstate(over="ignore"):
        s = dtype(1) / (dtype(1) + np.exp(-g))
    return (dtype(1) - s) * q + s * u, (dtype(1) - s) * dy, s * dy, dy * (u - q) * s * (dtype(1) - s)


def gate_tols(q, u, dy):
    q, u, dy = (np.abs(np.asarray(a).astype(np.float64)) for a in (q, u, dy))
    return 16 * U * (q + u), 16 * U * dy, 16 * U * dy, 16 * U * dy * (q + u)


# ------------------------------------------------------------------------------------------------ activation backward
ACT_N = (1, 257)
ACT_SPECIAL = (0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 6.0, -6.0)


def act_inputs(n, k=0):
    """(dy, saved) [n] fp32; saved ~ N(0, 2^2) with ACT_SPECIAL (rotated by k) in front."""
    r = _rng(7, n)
    dy = r.standard_normal(n).astype(np.float32)
    sv = (r.standard_normal(n) * 2).astype(np.float32)
    for i in range(min(n, 8)):
        sv[i] = ACT_SPECIAL[(i + k) % 8]
    return dy, sv


def gelu_grad(x: torch.Tensor) -> torch.Tensor:
    """d gelu / dx = Phi(x) + x phi(x) in x's own precision (torch: numpy has no erf)."""
    one = torch.ones((), dtype=x.dtype)
    return 0.5 * (one + torch.erf(x * (0.70710678118654752 * one))) + x * (0.3989422804014327 * one) * torch.exp(-0.5 * one * x * x)


def act_bwd(dy: torch.Tensor, saved: torch.Tensor, act: str, dtype=torch.float64) -> torch.Tensor:
    dy, saved = dy.to(dtype), saved.to(dtype)
    if act == "relu":
        return torch.where(saved > 0, dy, torch.zeros_like(dy))
    if act == "gelu":
        return dy * gelu_grad(saved)
    return dy


def gelu_bwd_tol(dy: torch.Tensor) -> torch.Tensor:
    return 16 * U * dy.double().abs()


# ------------------------------------------------------------------------------------------------ glue: case lists
COLSUM_R = (0, 1, 15, 16, 17, 63, 64, 65, 1000)
COLSUM_N = (1, 63, 64, 65, 130)
SCALE_ROWS_C = (7, 8, 24)
SUM_PARTS = (1, 2, 31, 32, 33, 40)        # the wrapper chunks at MAXG - 1 = 31
SUM_SHAPES = ((4,), (1028,), (15,), (3, 5))
MEAN_ALL_N = (1, 3, 4, 5, 1023, 4 * 256 * 256 + 7)   # the last asks for more than PQ3D_MEAN_MAX_BLOCKS blocks


def sum_left_to_right(parts):
    """The fp32 sum of the parts in list order, one rounding per addition."""
    out = np.asarray(parts[0], np.float32).copy()
    for p in parts[1:]:
        out = (out + np.asarray(p, np.float32)).astype(np.float32)
    return out
