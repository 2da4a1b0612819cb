"""GPU: the CLIP text prompt encoder on the HIP kernels (pq3d_amd/clip_text.py, csrc/clip_text.hip) against fixture F25 (the
reference's own CLIPLanguageEncoder over the installed transformers, tiny random-init architecture) and against the float64
restatement tests/clip_text_ref.py.  Padded query positions are don't-care everywhere (the decoder masks them)."""
import numpy as np
import pytest
import torch

from pq3d_amd import _lib as L
from pq3d_amd import clip_text as CT
from pq3d_amd import ops, synth
from tests import clip_text_ref as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32 = dict(atol=2e-5, rtol=2e-5)    # tests/test_gpu_t5_head.py's bar for fp32 logits (util.check_against's formula)


def close(got, want, atol, rtol, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f"{what}: max abs err {err:.3e} (scale {scale:.3e}, bar {atol + rtol * scale:.3e})")
    assert err <= atol + rtol * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"
    return err


def fixture_case(case, compute):
    z, a = util.load_fixture("F25_clip_text")
    enc, sd = R.fixture_module(z, a, case, compute)
    enc.to(DEV).eval()
    return z, a, enc, sd, torch.from_numpy(z["ids"]).to(DEV), torch.from_numpy(z["masks"]).to(DEV)


@pytest.mark.parametrize("case", ["mlp", "attn"])
def test_fp32_parity_with_the_reference_module(case):
    """Backbone and final output at every valid position (the length-1 and length-2 prompts and the rows behind the masked key
    included); for 'mlp' the projection's gradients of the fixture's weighted-mean loss."""
    z, a, enc, _sd, ids, masks = fixture_case(case, "fp32")
    v = z["masks"]
    assert list(v.sum(1)) == [77, 12, 2, 1, 19]
    close(enc._tower(ids, masks).cpu().numpy()[v], z[f"{case}/backbone"][v], **FP32, what=f"{case} backbone")
    y = enc(ids, masks)
    close(y.detach().cpu().numpy()[v], z[f"{case}/out"][v], **FP32, what=f"{case} out")
    if case == "mlp":
        keep = masks[..., None].float()
        (y * util.loss_weight("clip_mlp", y.shape).to(DEV) * keep).mean().backward()
        for n, p in enc.projection.named_parameters():
            util.check_against(z, "grad/projection." + n, p.grad, atol=1e-7, rtol=1e-3, cap=util.MAX_GRAD)
        assert all(p.grad is None for p in enc.model.parameters())


@pytest.mark.parametrize("compute", ["bf16", "bf16x3"])
@pytest.mark.parametrize("case", ["mlp", "attn"])
def test_lower_precision_modes_within_twice_the_reference_autocast_error(case, compute):
    """Error at valid positions <= 2 x the error of the SAME reference module under CPU bf16 autocast against its own fp32 output
    (recorded in the fixture; the factor covers rounding at different sites than autocast).  Measured values: DESIGN.md section 7a."""
    z, a, enc, _sd, ids, masks = fixture_case(case, compute)
    v = z["masks"]
    with torch.no_grad():
        bb, y = enc._tower(ids, masks), enc(ids, masks)
    for name, got in (("backbone", bb), ("out", y)):
        bar = 2.0 * float(z[f"meta/bf16_err/{case}/{name}"])
        err = float(np.abs(got.float().cpu().numpy()[v] - z[f"{case}/{name}"][v]).max())
        print(f"{compute} {case} {name}: max abs err {err:.3e}, reference bf16 autocast {bar / 2:.3e}")
        assert err <= bar, f"{compute} {case} {name}: {err:.3e} > 2 x {bar / 2:.3e}"


def _attn_inputs(T, n=3, H=2, seed=0):
    g = torch.Generator().manual_seed(seed + T)
    qkv = torch.randn(n, T, 3 * H * 64, generator=g)
    valid = torch.rand(n, T, generator=g) < 0.7
    valid[:, 0] = True
    valid[n - 1, 0] = False            # one prompt without its first token: the rows before its first valid key see nothing
    if T > 2:
        valid[n - 1, 1] = False
    return qkv, valid


def _attn_ref(qkv, valid, H):
    n, T, _ = qkv.shape
    q, k, v = (t.view(n, T, H, 64).transpose(1, 2) for t in qkv.double().chunk(3, -1))
    return R.causal_attention(q, k, v, valid, 64 ** -0.5).transpose(1, 2).reshape(n, T, H * 64)


@pytest.mark.parametrize("T", [1, 33, 64, 77])
def test_attention_kernel_against_float64(T):
    """fp32 I/O: the fp32 bar (64-term dots, <= 77-term value sums and __expf are each a few 2^-24 relative).  bf16 I/O: the same
    inputs rounded to bf16 for both sides, plus one bf16 rounding of the output (8 significant bits: half a spacing is at most
    2^-8 of the value)."""
    qkv, valid = _attn_inputs(T)
    want = _attn_ref(qkv, valid, 2)
    got = CT.attn_causal(qkv.to(DEV), valid.to(DEV), 2)
    close(got.cpu().numpy(), want.numpy(), **FP32, what=f"T={T} fp32")
    blind = ~(valid.cumsum(1) > 0)     # query rows with no visible key
    assert blind[2, 0] and (T <= 2 or blind[2, 1])
    assert (got.cpu()[blind] == 0).all() and (want[blind] == 0).all()
    q16 = qkv.to(torch.bfloat16)
    got16 = CT.attn_causal(q16.to(DEV), valid.to(DEV), 2)
    assert got16.dtype == torch.bfloat16 and (got16.cpu()[blind] == 0).all()
    close(got16.float().cpu().numpy(), _attn_ref(q16.float(), valid, 2).numpy(), atol=2e-5, rtol=2e-5 + 2.0 ** -8, what=f"T={T} bf16")
    got_all = CT.attn_causal(qkv.to(DEV), None, 2)       # no mask: plain causal attention
    close(got_all.cpu().numpy(), _attn_ref(qkv, torch.ones_like(valid), 2).numpy(), **FP32, what=f"T={T} no mask")


def test_attention_kernel_refuses_more_than_77_tokens():
    qkv = torch.zeros(1, 78, 3 * 64, device=DEV)
    out = torch.full((1, 78, 64), 7.0, device=DEV)
    with pytest.raises(L.Pq3dError, match=r"pq3d_attn_causal_fwd failed \(rc=-1\): .*77"):
        L.call("pq3d_attn_causal_fwd", qkv, None, out, 1, 78, 1, L.F32, 0.125)
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "nothing may be launched"
    enc = CT.CLIPLanguageEncoder(None, hf_config=dict(util.load_fixture("F25_clip_text")[1]["hf_config"], max_position_embeddings=80))
    with pytest.raises(ValueError):
        enc.to(DEV)(torch.zeros(1, 78, dtype=torch.long, device=DEV), torch.ones(1, 78, dtype=torch.bool, device=DEV))
    small = CT.CLIPLanguageEncoder(None, hf_config=dict(util.load_fixture("F25_clip_text")[1]["hf_config"], max_position_embeddings=16))
    with pytest.raises(ValueError):
        small.to(DEV)(torch.zeros(1, 17, dtype=torch.long, device=DEV), torch.ones(1, 17, dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("d", [192, 96])
def test_embed_l2norm_and_quick_gelu_against_torch(d):
    g = torch.Generator().manual_seed(d)
    n, T, vocab = 3, 77, 50
    tok, pos = torch.randn(vocab, d, generator=g), torch.randn(T + 3, d, generator=g)
    ids = torch.randint(0, vocab, (n, T), generator=g)
    ids[0, 3], ids[1, 0], ids[2, 76] = -5, 10 ** 6, vocab      # out of vocabulary: clamped to rows 0 / vocab - 1
    want = tok[ids.clamp(0, vocab - 1)] + pos[:T]
    x = CT.clip_embed(tok.to(DEV), pos.to(DEV), ids.to(DEV))
    assert torch.equal(x.cpu(), want)
    assert torch.equal(CT.clip_embed(tok.to(DEV), pos.to(DEV), ids.to(DEV), out_dtype=torch.bfloat16).cpu(), want.to(torch.bfloat16))
    with pytest.raises(ValueError):
        CT.clip_embed(tok.to(DEV), pos[:T - 1].to(DEV), ids.to(DEV))
    # row normalisation, rows = 77 * 3: fp32 sum of d squares, worst case d * 2^-24 relative
    r = want.view(n * T, d).clone()
    r[5] = 0.0
    r[6] = 1e-20
    y = CT.l2norm_rows(r.to(DEV)).cpu()
    assert torch.isfinite(y).all() and (y[5] == 0).all()
    ref = torch.nn.functional.normalize(r.double(), p=2, dim=1)
    close(y[:6].numpy(), ref[:6].numpy(), atol=d * 2.0 ** -24, rtol=0, what=f"l2norm d={d}")
    close(y[7:].numpy(), ref[7:].numpy(), atol=d * 2.0 ** -24, rtol=0, what=f"l2norm d={d}")
    assert torch.allclose(y[6], torch.full_like(y[6], 1e-8), rtol=1e-5, atol=0)     # ||x|| < eps: x / eps, as F.normalize
    # quick-GELU epilogue of the GEMM, M = 231 rows, N / K = d / (288 - d): not multiples of the 64-wide tiles
    k = 288 - d
    a, w, b = torch.randn(n * T, k, generator=g), torch.randn(d, k, generator=g) * 0.2, torch.randn(d, generator=g)
    pre = torch.nn.functional.linear(a.double(), w.double(), b.double())
    out = ops.linear(a.to(DEV), w.to(DEV), b.to(DEV), ct=L.F32, act="quick_gelu")
    close(out.cpu().numpy(), (pre * torch.sigmoid(1.702 * pre)).numpy(), **FP32, what=f"quick_gelu d={d}")
    ar = a.to(DEV).requires_grad_(True)
    with pytest.raises(L.Pq3dError, match="forward only"):
        ops.linear(ar, w.to(DEV), b.to(DEV), ct=L.F32, act="quick_gelu").sum().backward()


def test_forward_is_graph_capturable_and_the_weight_pack_follows_load_state_dict():
    z, a, enc, sd, ids, masks = fixture_case("mlp", "bf16")
    s_ids, s_masks = ids.clone(), masks.clone()
    with torch.no_grad():
        eager0 = enc(ids, masks).clone()         # builds the frozen-weight pack
        pack = enc._packs[(str(ids.device), "bf16")][1]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(s_ids, s_masks)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s_out = enc(s_ids, s_masks)
        assert enc._packs[(str(ids.device), "bf16")][1] is pack, "the pack must not be rebuilt inside the capture"
        graph.replay()
        assert torch.equal(s_out, eager0)
        ids2 = ids.flip(0).contiguous()
        ids2[:, 0] = ids[:, 0]
        masks2 = masks.roll(1, 0).contiguous()
        s_ids.copy_(ids2); s_masks.copy_(masks2)
        graph.replay()
        eager2 = enc(ids2, masks2)
        assert torch.equal(s_out, eager2) and not torch.equal(eager2, eager0)
        del graph
        # one weight changed through load_state_dict: the pack is rebuilt and the output moves
        new = {k: t.clone() for k, t in sd.items()}
        new["model.text_model.encoder.layers.0.mlp.fc1.weight"][3, 5] += 0.5
        enc.load_state_dict(new)
        moved = enc(ids, masks)
        assert enc._packs[(str(ids.device), "bf16")][1] is not pack
        assert not torch.equal(moved, eager0) and torch.isfinite(moved).all()


def test_model_encodes_text_prompts_end_to_end():
    from pq3d_amd.model import Query3DUnified, make_cfg
    _z, a = util.load_fixture("F25_clip_text")
    mem, d, B, T = ["voxel", "mv", "prompt"], 64, 4, 12
    cfg = make_cfg(d=d, H=4, L=2, memories=mem, heads=["ground"], structure="mixed",
                   txt_encoder=dict(hf_config=a["hf_config"], output_dim=d, use_projection=True, projection_type="mlp"))
    model = Query3DUnified(cfg, compute="fp32")
    synth.fill_module(model, 0)
    model.to(DEV)
    dd = synth.synth_data_dict(B, 48, 10, {"voxel": d, "mv": d}, seed=5, memories=mem)
    dd.update(synth.prompt_loc_inputs(B, T, seed=3))
    g = torch.Generator().manual_seed(1)
    txt = torch.tensor([True, False, True, False])
    ids = torch.randint(3, a["hf_config"]["vocab_size"], (B, T), generator=g)
    ids[:, 0] = 0
    dd["prompt"][txt] = ids[txt].float()                     # token ids travel in the (float) prompt rows, as in the reference
    dd["prompt_type"][txt] = Query3DUnified.PROMPT_TYPE["txt"]
    dd["prompt_pad_masks"][0] = torch.arange(T) < 7
    dd["prompt_pad_masks"][2] = torch.arange(T) < T
    dev = lambda: {k: v.clone().to(DEV) for k, v in dd.items()}
    model.eval()
    with torch.no_grad():
        b = dev()
        feat, kpm = model.prompt_encoder(b)
        direct = model.txt_encoder(ids[txt].to(DEV), dd["prompt_pad_masks"][txt].to(DEV))
    assert torch.equal(feat[txt.to(DEV)], direct) and torch.equal(kpm, b["prompt_pad_masks"].logical_not())
    assert not kpm[1, 0] and kpm[1, 1:].all()               # 'loc' prompts keep token 0 only
    model.train()
    out = model(dev())
    gl = out["ground_logits"]
    loss = torch.where(torch.isfinite(gl), gl, torch.zeros_like(gl)).square().mean() + out["query_embeds"].square().mean()
    assert torch.isfinite(loss)
    loss.backward()
    proj = list(model.txt_encoder.projection.parameters())
    assert proj and all(p.grad is not None and torch.isfinite(p.grad).all() for p in proj)
    assert any(float(p.grad.abs().max()) > 0 for p in proj)
    assert all(p.grad is None for p in model.txt_encoder.model.parameters())
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())
