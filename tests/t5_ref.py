"""Float64 restatements of the caption head's T5 kernels (csrc/norm.hip RMSNorm, csrc/misc.hip + csrc/t5glue.hip embedding,
csrc/t5glue.hip pq3d_t5_prep / pq3d_t5_bias_bwd), written from the operations' definitions (T5LayerNorm, nn.Embedding,
T5's _shift_right and relative-position bias), plain torch on the host, no project import.  tests/test_t5_ref.py keeps them
honest against transformers and torch.autograd; tests/test_gpu_t5_kernels.py compares the kernels with them.

Every value function has an ``*_abs`` companion: the same expression with every term replaced by its absolute value.  A
rounding-error bound of a sum is a multiple of that quantity (never of the possibly cancelled value itself), so the GPU tests
state their tolerances as K * 2^-24 * abs-bound."""
import torch

F64 = torch.float64


def _d(t):
    return t.to("cpu", F64)      # (not detached: tests/test_t5_ref.py differentiates the forward restatements)


# ------------------------------------------------------------------------------------------------ RMSNorm (T5LayerNorm)
def rmsnorm(x, w, eps):
    """y = x * rsqrt(mean(x^2) + eps) * w over the last dim; returns (y, rstd [rows...]).  |y| is its own abs-bound."""
    x, w = _d(x), _d(w)
    r = ((x * x).mean(-1, keepdim=True) + float(eps)).rsqrt()
    return x * r * w, r.squeeze(-1)


def rmsnorm_bwd(x, w, rstd, dy, dres=None):
    """dx = r (g - xh mean(g xh)) + dres,  g = dy w,  xh = x r;  dw = sum_rows dy xh.  x, dy, dres [R, d]; rstd [R]."""
    x, w, dy, r = _d(x), _d(w), _d(dy), _d(rstd).unsqueeze(-1)
    xh, g = x * r, dy * w
    dx = r * (g - xh * (g * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + _d(dres)
    return dx, (dy * xh).flatten(0, -2).sum(0)


def rmsnorm_bwd_abs(x, w, rstd, dy, dres=None):
    x, w, dy, r = _d(x).abs(), _d(w).abs(), _d(dy).abs(), _d(rstd).abs().unsqueeze(-1)
    xh, g = x * r, dy * w
    dx = r * (g + xh * (g * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + _d(dres).abs()
    return dx, (dy * xh).flatten(0, -2).sum(0)


# ------------------------------------------------------------------------------------------------ embedding
def embedding(table, ids, keep=None, p=0.0):
    """table[ids]; with a keep mask [ids.numel(), d] (bool): keep ? row / (1 - p) : 0 (inverted dropout)."""
    out = _d(table)[ids.cpu().long()]
    if keep is not None:
        out = out * _d(keep).view_as(out) / (1.0 - p)
    return out


def embedding_bwd(dout, ids, rows, keep=None, p=0.0):
    """index_add of the (masked, scaled) output gradient into a zero table of ``rows`` rows."""
    g = _d(dout)
    d = g.shape[-1]
    if keep is not None:
        g = g * _d(keep).view_as(g) / (1.0 - p)
    return torch.zeros(rows, d, dtype=F64).index_add_(0, ids.cpu().long().flatten(), g.reshape(-1, d))


def embedding_bwd_abs(dout, ids, rows, keep=None, p=0.0):
    return embedding_bwd(_d(dout).abs(), ids, rows, keep, p)


def embedding_bwd_terms(ids, rows):
    """Number of addends of every table row's gradient."""
    return torch.bincount(ids.cpu().long().flatten(), minlength=rows)


# ------------------------------------------------------------------------------------------------ t5_prep
def t5_prep(rel, labels, buckets, enc_valid, start_id, pad_id, H):
    """ids [B, T] = [start, labels[:-1]] with -100 -> pad;  bias [B, H, T, T] = rel[buckets[q, k], h] for k <= q, -inf above
    the diagonal;  kpm [B, N] = not enc_valid (None without enc_valid).  ``bias`` keeps rel's dtype: it is a gather."""
    labels, buckets, rel = labels.cpu().long(), buckets.cpu().long(), rel.detach().cpu()
    B, T = labels.shape
    assert rel.shape[1] == H
    ids = torch.empty_like(labels)
    ids[:, 0] = start_id
    ids[:, 1:] = labels[:, :-1]
    ids[ids == -100] = pad_id
    bias = rel[buckets].permute(2, 0, 1).clone()                            # [H, T, T]
    q, k = torch.arange(T)[:, None], torch.arange(T)[None, :]
    bias[:, k > q] = float("-inf")
    kpm = None if enc_valid is None else enc_valid.cpu().bool().logical_not()
    return ids, bias.unsqueeze(0).expand(B, H, T, T).contiguous(), kpm


def t5_bias_bwd(dbias, buckets, NB):
    """d rel [NB, H] = sum over the scenes and over the causal pairs k <= q of bucket nb of dbias[b, h, q, k]; what dbias
    holds above the diagonal is ignored."""
    g, buckets = _d(dbias), buckets.cpu().long()
    B, H, T, _ = g.shape
    q, k = torch.arange(T)[:, None], torch.arange(T)[None, :]
    causal = (k <= q)
    s = g.sum(0)[:, causal]                                                 # [H, pairs]
    return torch.zeros(NB, H, dtype=F64).index_add_(0, buckets[causal], s.t().contiguous())


def t5_bias_bwd_abs(dbias, buckets, NB):
    return t5_bias_bwd(_d(dbias).abs(), buckets, NB)


def t5_bias_bwd_terms(buckets, NB, B):
    """Number of addends of every bucket's gradient (the same for all heads): B x its causal pairs."""
    buckets = buckets.cpu().long()
    T = buckets.shape[0]
    q, k = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return torch.bincount(buckets[k <= q], minlength=NB) * B
