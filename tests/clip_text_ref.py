"""Plain float64 torch restatement of the CLIP text prompt encoder (modules/language/clip.py over HF
CLIPTextModelWithProjection), reading a state_dict with the reference's keys.  Test-side only: pins fixture F25 on the CPU
(tests/test_clip_text_ref.py) and is the reference of the kernel tests (tests/test_gpu_clip_text.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def causal_attention(q, k, v, valid, scale):
    """q, k, v [n, H, T, dh]; valid [n, T] bool.  Key j is visible to query i iff j <= i and valid[n, j]; softmax over the visible
    keys; a row with no visible key is zeros (the documented deviation from HF's uniform row)."""
    T = q.shape[2]
    vis = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()[None, None] & valid[:, None, None, :]
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.where(vis, (s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))).exp(), torch.zeros_like(s))
    den = e.sum(-1, keepdim=True)
    return (e / torch.where(den > 0, den, torch.ones_like(den))) @ v


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def tower(sd, cfg, ids, masks, prefix="model."):
    """last_hidden_state -> text_projection -> F.normalize(p=2, dim=2), float64 [n, T, projection_dim]."""
    g = lambda k: sd[prefix + k].double()
    d, H, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg.get("layer_norm_eps", 1e-5)
    n, T = ids.shape
    x = g("text_model.embeddings.token_embedding.weight")[ids] + g("text_model.embeddings.position_embedding.weight")[:T]
    heads = lambda t: t.view(n, T, H, d // H).transpose(1, 2)
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        lin = lambda t, name: F.linear(t, g(p + name + ".weight"), g(p + name + ".bias"))
        h = F.layer_norm(x, (d,), g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), eps)
        o = causal_attention(heads(lin(h, "self_attn.q_proj")), heads(lin(h, "self_attn.k_proj")), heads(lin(h, "self_attn.v_proj")),
                             masks, (d // H) ** -0.5)
        x = x + lin(o.transpose(1, 2).reshape(n, T, d), "self_attn.out_proj")
        h = F.layer_norm(x, (d,), g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"), eps)
        x = x + lin(quick_gelu(lin(h, "mlp.fc1")), "mlp.fc2")
    x = F.layer_norm(x, (d,), g("text_model.final_layer_norm.weight"), g("text_model.final_layer_norm.bias"), eps)
    return F.normalize(F.linear(x, g("text_projection.weight")), p=2, dim=2)


def projection(sd, case, txt, masks, nhead=12):
    """The module's trainable projection stage in eval mode (dropout off)."""
    g = lambda k: sd["projection." + k].double()
    if case["projection_type"] == "mlp":     # get_mlp_head: Linear, ReLU, LayerNorm(eps 1e-12), Dropout, Linear
        h = F.relu(F.linear(txt, g("0.weight"), g("0.bias")))
        h = F.layer_norm(h, h.shape[-1:], g("2.weight"), g("2.bias"), 1e-12)
        return F.linear(h, g("4.weight"), g("4.bias"))
    n, T, d = txt.shape
    for i in range(case.get("num_projection_layers", 1)):   # post-norm SelfAttentionLayer over the valid keys (no causal mask)
        q, k, v = F.linear(txt, g(f"{i}.self_attn.in_proj_weight"), g(f"{i}.self_attn.in_proj_bias")).chunk(3, -1)
        hd = lambda t: t.view(n, T, nhead, d // nhead).transpose(1, 2)
        s = (hd(q) @ hd(k).transpose(-1, -2)) * (d // nhead) ** -0.5
        s = s.masked_fill(~masks[:, None, None, :], float("-inf"))
        o = (s.softmax(-1) @ hd(v)).transpose(1, 2).reshape(n, T, d)
        o = F.linear(o, g(f"{i}.self_attn.out_proj.weight"), g(f"{i}.self_attn.out_proj.bias"))
        txt = F.layer_norm(txt + o, (d,), g(f"{i}.norm.weight"), g(f"{i}.norm.bias"), 1e-5)
    return txt


def encoder(sd, cfg, case, ids, masks):
    """(backbone, final output) of CLIPLanguageEncoder in eval mode, float64."""
    bb = tower(sd, cfg, ids, masks)
    return bb, (projection(sd, case, bb, masks) if case.get("use_projection") else bb)


def fixture_module(z, args, case, compute="fp32"):
    """Our CLIPLanguageEncoder for one case of fixture F25, filled with the fixture's synthetic weights (checksum checked)."""
    from pq3d_amd import synth
    from pq3d_amd.clip_text import CLIPLanguageEncoder
    enc = CLIPLanguageEncoder(None, weights="tiny", hf_config=args["hf_config"], **args["cases"][case])
    enc.compute = compute
    sd = synth.fill_module(enc, args["seed"])
    want = float(z[f"meta/weights_checksum/{case}"])
    assert abs(synth.state_checksum(sd) - want) < 1e-6 * want
    for m in enc.modules():
        if hasattr(m, "compute"):
            m.compute = compute
    return enc, sd
