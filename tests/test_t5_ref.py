"""CPU: the float64 restatements of tests/t5_ref.py against transformers' T5 (T5LayerNorm, _shift_right, compute_bias,
_relative_position_bucket) and torch.autograd, and pq3d_amd.t5.relative_buckets against HF's bucket function.  The GPU tests
(tests/test_gpu_t5_kernels.py) then compare the HIP kernels with the restatements.

T5LayerNorm and float64: HF forms the variance as ``hidden_states.to(torch.float32).pow(2).mean(-1)`` whatever the input's
dtype, so ``T5LayerNorm(...).double()`` still carries an fp32 variance.  The comparison therefore uses inputs on a grid where
that fp32 variance is nearly exact: x = 2^s * k / 8 with integers |k| <= 32 (one power of two per row).  Then x and x^2 are
fp32 numbers and every partial sum of the d <= 2048 squares fits 24 bits, so the sum is exact in any order; what remains
is the division by d (u = 2^-24), the addition of eps (eps itself rounded to fp32: 2u in all) and the fp32 rsqrt (2u):
relative error of HF's rstd <= 3u / 2 + 2u, and the products after it are float64.  The test allows 4u |y|."""
import pytest
import torch

from tests import t5_ref as R

U = 2.0 ** -24
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def grid_rows(Rr, d, g):
    """[Rr, d] on the grid of the module docstring: a plain row, then (Rr >= 4) one scaled by 2^10, one by 2^-13 (mean
    square ~ 1e-7: eps = 1e-6 dominates) and an all-zero row."""
    x = torch.randint(-32, 33, (Rr, d), generator=g).to(F64) / 8
    if Rr >= 4:
        x[1] *= 2.0 ** 10
        x[2] *= 2.0 ** -13
        x[3] = 0
    return x


def tiny_t5(**kw):
    from transformers import T5Config, T5ForConditionalGeneration
    cfg = dict(vocab_size=64, d_model=16, d_kv=4, d_ff=16, num_layers=1, num_decoder_layers=1, num_heads=3,
               decoder_start_token_id=3, pad_token_id=5, eos_token_id=1)
    cfg.update(kw)
    torch.manual_seed(0)
    return T5ForConditionalGeneration(T5Config(**cfg)).double().eval()


# ------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("d", [1, 48, 100, 512, 2048])
def test_rmsnorm_matches_hf_t5layernorm(d):
    from transformers.models.t5.modeling_t5 import T5LayerNorm
    g = gen(d)
    x = grid_rows(5, d, g)
    w = 1 + 0.5 * torch.randn(d, generator=g, dtype=F64)
    w[::3] *= -1
    ln = T5LayerNorm(d, eps=1e-6).double()
    with torch.no_grad():
        ln.weight.copy_(w)
        want = ln(x)
    y, rstd = R.rmsnorm(x, w, 1e-6)
    assert want.dtype == F64 and y.shape == x.shape and rstd.shape == (5,)
    assert bool(((y - want).abs() <= 4 * U * y.abs()).all()), float(((y - want).abs() / y.abs().clamp_min(1e-300)).max() / U)
    assert torch.equal(y[3], torch.zeros(d, dtype=F64)) and abs(float(rstd[3]) - 1e3) < 1e-9     # zero row: rstd = eps^-1/2
    assert abs(float(rstd[2]) * float((x[2] * x[2]).mean() + 1e-6) ** 0.5 - 1) < 1e-12


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("Rr,d", [(1, 1), (5, 48), (7, 100), (4, 513)])
def test_rmsnorm_bwd_matches_autograd(Rr, d, with_res):
    g = gen(100 * Rr + d)
    x = torch.randn(Rr, d, generator=g, dtype=F64)
    if Rr >= 4:
        x[1] *= 1e3
        x[2] *= 1e-4
        x[3] = 0
    w = 1 + 0.5 * torch.randn(d, generator=g, dtype=F64)
    dy = torch.randn(Rr, d, generator=g, dtype=F64)
    dres = torch.randn(Rr, d, generator=g, dtype=F64) if with_res else None
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y, rstd = R.rmsnorm(xa, wa, 1e-6)
    loss = (y * dy).sum()
    if with_res:
        loss = loss + (xa * dres).sum()
    loss.backward()
    dx, dw = R.rmsnorm_bwd(x, w, rstd.detach(), dy, dres)
    ax, aw = R.rmsnorm_bwd_abs(x, w, rstd.detach(), dy, dres)
    assert bool(((dx - xa.grad).abs() <= 1e-13 * ax + 1e-300).all())
    assert bool(((dw - wa.grad).abs() <= 1e-13 * aw + 1e-300).all())
    assert bool((ax >= dx.abs()).all()) and bool((aw >= dw.abs()).all())
    if Rr >= 4:      # zero row: dx = r g
        assert torch.allclose(dx[3], 1e3 * dy[3] * w + (dres[3] if with_res else 0), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", ["equal", "spread", "random"])
def test_embedding_bwd_matches_autograd(layout, p):
    g = gen(7)
    rows, d = 50, 7
    ids = {"equal": torch.full((3, 17), 11), "spread": (torch.randperm(rows, generator=g)[torch.arange(51) % rows]).view(3, 17),
           "random": torch.randint(0, rows, (3, 17), generator=g)}[layout]
    table = torch.randn(rows, d, generator=g, dtype=F64)
    keep = (torch.rand(51, d, generator=g) >= p) if p > 0 else None
    dout = torch.randn(3, 17, d, generator=g, dtype=F64)
    ta = table.clone().requires_grad_(True)
    out = R.embedding(ta, ids, keep, p)
    want = torch.nn.functional.embedding(ids, table)
    if keep is not None:
        want = want * keep.view(3, 17, d) / (1 - p)
        assert bool((out[~keep.view(3, 17, d)] == 0).all())
    assert torch.allclose(out.detach(), want, rtol=1e-15, atol=0)
    (out * dout).sum().backward()
    dt = R.embedding_bwd(dout, ids, rows, keep, p)
    ab = R.embedding_bwd_abs(dout, ids, rows, keep, p)
    assert bool(((dt - ta.grad).abs() <= 1e-13 * ab).all())
    n = R.embedding_bwd_terms(ids, rows)
    assert int(n.sum()) == 51 and bool((dt[n == 0] == 0).all()) and bool((ab[n == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ t5_prep
def hf_buckets(T, nb, md):
    from transformers.models.t5.modeling_t5 import T5Attention
    q, k = torch.arange(T)[:, None], torch.arange(T)[None, :]
    return T5Attention._relative_position_bucket(k - q, bidirectional=False, num_buckets=nb, max_distance=md)


def labels_with_ignored(B, T, g, vocab=64):
    """Random labels; -100 at position 0 (scene 0), in the middle (scene 1 % B) and in the last place (scene 2 % B)."""
    lab = torch.randint(6, vocab, (B, T), generator=g)
    lab[0, 0] = -100
    lab[1 % B, T // 2] = -100
    lab[2 % B, T - 1] = -100
    return lab


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (4, 17), (2, 33)])
def test_t5_prep_ids_match_hf_shift_right(B, T):
    m = tiny_t5()
    lab = labels_with_ignored(B, T, gen(T))
    rel = torch.zeros(32, 3, dtype=F64)
    ids, _bias, kpm = R.t5_prep(rel, lab, hf_buckets(T, 32, 128), None, 3, 5, 3)
    assert kpm is None and torch.equal(ids, m._shift_right(lab))
    assert bool((ids[:, 0] == 3).all()) and not bool((ids == -100).any())
    ev = torch.rand(B, 6, generator=gen(1)) < 0.6
    assert torch.equal(R.t5_prep(rel, lab, hf_buckets(T, 32, 128), ev, 3, 5, 3)[2], ~ev)


@pytest.mark.parametrize("T,nb,md", [(1, 32, 128), (2, 8, 16), (33, 32, 128), (114, 32, 128), (40, 12, 100)])
def test_t5_prep_bias_and_its_gradient_match_hf_compute_bias(T, nb, md):
    B = 3
    m = tiny_t5(relative_attention_num_buckets=nb, relative_attention_max_distance=md)
    att = m.decoder.block[0].layer[0].SelfAttention
    assert att.is_decoder and att.has_relative_attention_bias
    H = att.n_heads
    g = gen(T + nb)
    with torch.no_grad():
        att.relative_attention_bias.weight.copy_(torch.randn(nb, H, generator=g, dtype=F64))
    rel = att.relative_attention_bias.weight
    causal = torch.ones(T, T, dtype=torch.bool).triu(1)
    want = att.compute_bias(T, T).expand(B, H, T, T).masked_fill(causal, float("-inf"))
    buckets = hf_buckets(T, nb, md)
    _ids, bias, _ = R.t5_prep(rel, torch.zeros(B, T, dtype=torch.long), buckets, None, 0, 0, H)
    assert bias.dtype == F64 and torch.equal(bias, want.detach())
    dbias = torch.randn(B, H, T, T, generator=g, dtype=F64)
    dbias.masked_fill_(causal, 1e30)                     # above the diagonal: ignored by contract
    want.backward(dbias)
    drel = R.t5_bias_bwd(dbias, buckets, nb)
    ab = R.t5_bias_bwd_abs(dbias, buckets, nb)
    assert bool(((drel - rel.grad).abs() <= 1e-13 * ab).all()) and float(ab.max()) < 1e6
    n = R.t5_bias_bwd_terms(buckets, nb, B)
    assert int(n.sum()) == B * T * (T + 1) // 2
    assert bool((drel[n == 0] == 0).all()) and bool((rel.grad[n == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ relative_buckets
@pytest.mark.parametrize("nb,md", [(32, 128), (8, 16), (32, 64), (64, 128), (16, 128), (256, 512), (12, 100)])
def test_relative_buckets_match_hf_on_the_causal_pairs(nb, md):
    from pq3d_amd.t5 import relative_buckets
    for T in (1, 2, 17, 33, 114, 200, 512):
        got = relative_buckets(T, nb, md, "cpu")
        want = hf_buckets(T, nb, md)
        causal = torch.ones(T, T, dtype=torch.bool).tril()
        assert got.shape == (T, T) and got.dtype == torch.int64
        assert int((got[causal] != want[causal]).sum()) == 0, (T, nb, md)
        assert int(got.min()) >= 0 and int(got.max()) < nb          # also above the diagonal: the kernels index with it
