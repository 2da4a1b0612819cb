"""The CLIP text prompt encoder on the HIP kernels (modules/language/clip.py:11-42, the stage-2 config's ``txt_encoder``).

Third-party arithmetic: the reference drives HF ``CLIPTextModelWithProjection`` (frozen, under ``torch.no_grad``), applies
``text_projection`` to EVERY token, L2-normalises and then runs its own trainable projection stage.  This restates the text
tower from its published architecture (token + position embedding; pre-LayerNorm residual blocks with causal self-attention
over the valid tokens and a quick-GELU MLP; final LayerNorm; bias-free projection) on this package's ops plus
csrc/clip_text.hip (embedding, causal attention for T <= 77, row L2 normalisation) and the GEMM's quick-GELU epilogue.
The parameter tree is plain ``nn.Module`` containers with HF's state_dict keys, so a reference checkpoint loads over it.
Nothing is ever fetched: without a checkpoint the tower has the ViT-L/14 text dimensions (or ``hf_config``) and random
weights.  Pinned by fixture F25 (reference module + the installed transformers) in tests/test_gpu_clip_text.py.

One deviation: a query token with NO visible key (token 0 masked) yields a zero attention row; HF's additive mask gives an
implementation-defined uniform row there.  It cannot occur when token 0 is valid, which CLIP's BOS always is."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .modules import SelfAttentionLayer, _PostNormBase, get_mlp_head, layer_repeat, mlp_head_forward

VIT_L14_TEXT = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                    max_position_embeddings=77, projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
DROP_BASE_TXT_ENC = 8 << 20
ATTN_CAUSAL_MAX_T = L.H.PQ3D_ATTN_CAUSAL_MAX_T
# module compute mode -> (GEMM compute type, dtype of the frozen weight copies and of the MFMA-operand activations).  'bf16x3'
# forms every product of the tower split-bf16 from fp32 operands (fp32-grade); the residual stream, LayerNorm, softmax and the
# normalisation are fp32 in every mode.
_MODE = {"fp32": (L.F32, torch.float32), "bf16": (L.BF16, torch.bfloat16), "bf16x3": (L.BF16X3, torch.float32)}


def clip_embed(tok: torch.Tensor, pos: torch.Tensor, ids: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """x[n, t] = tok[ids[n, t]] + pos[t]; ids outside the vocabulary are clamped (include/pq3d_hip.h)."""
    n, T = ids.shape
    if T > pos.shape[0]:
        raise ValueError(f"{T} tokens but the position table has {pos.shape[0]} rows")
    assert ids.dtype == torch.int64 and tok.dtype == pos.dtype and tok.shape[1] == pos.shape[1]
    x = torch.empty(n, T, tok.shape[1], dtype=out_dtype, device=ids.device)
    L.call("pq3d_clip_embed", tok.contiguous(), pos.contiguous(), ids.contiguous(), x, n, T, tok.shape[1], tok.shape[0],
           L.dt_of(tok), L.dt_of(x))
    return x


def attn_causal(qkv: torch.Tensor, valid: Optional[torch.Tensor], H: int, scale: Optional[float] = None) -> torch.Tensor:
    """Causal self-attention over the packed [n, T, 3 H 64] output of one q|k|v projection; ``valid`` [n, T] bool (True = the
    key may be attended), any pattern.  Rows without a visible key are zeros."""
    n, T, w = qkv.shape
    assert w == 3 * H * 64, "pq3d_attn_causal_fwd: d_h is fixed at 64"
    assert valid is None or (valid.dtype == torch.bool and tuple(valid.shape) == (n, T))
    out = torch.empty(n, T, H * 64, dtype=qkv.dtype, device=qkv.device)
    L.call("pq3d_attn_causal_fwd", qkv.contiguous(), None if valid is None else valid.contiguous(), out, n, T, H, L.dt_of(qkv),
           float(64 ** -0.5 if scale is None else scale))
    return out


def l2norm_rows(x: torch.Tensor, eps: float = 1e-12, out_dtype=torch.float32) -> torch.Tensor:
    """F.normalize(x, p=2, dim=-1): x / max(||x||, eps); a zero row stays zero."""
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    d = x.shape[-1]
    L.call("pq3d_l2norm_rows", x.contiguous(), y, x.numel() // d, d, L.dt_of(x), L.dt_of(y), float(eps))
    return y


# ------------------------------------------------------------------------------------------------ parameter containers
class _Attn(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(d, d) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, d, f):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(d, f), nn.Linear(f, d)


class _Layer(nn.Module):
    def __init__(self, d, f, eps):
        super().__init__()
        self.self_attn = _Attn(d)
        self.layer_norm1 = nn.LayerNorm(d, eps=eps)
        self.mlp = _MLP(d, f)
        self.layer_norm2 = nn.LayerNorm(d, eps=eps)


class _Embeddings(nn.Module):
    def __init__(self, vocab, positions, d):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, d)
        self.position_embedding = nn.Embedding(positions, d)


class _Encoder(nn.Module):
    def __init__(self, n, d, f, eps):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(d, f, eps) for _ in range(n)])


class _TextTransformer(nn.Module):
    def __init__(self, c):
        super().__init__()
        d, eps = c["hidden_size"], c["layer_norm_eps"]
        self.embeddings = _Embeddings(c["vocab_size"], c["max_position_embeddings"], d)
        self.encoder = _Encoder(c["num_hidden_layers"], d, c["intermediate_size"], eps)
        self.final_layer_norm = nn.LayerNorm(d, eps=eps)


class _Config(dict):
    """The CLIPTextConfig fields the tower reads, as attributes (``model.config.hidden_size`` as on the HF object)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class CLIPTextTower(nn.Module):
    """Parameter tree of HF ``CLIPTextModelWithProjection`` (state_dict keys ``text_model.*``, ``text_projection.weight``).  The
    modules are containers only: the arithmetic is CLIPLanguageEncoder._tower."""

    def __init__(self, hf_config: Optional[dict] = None):
        super().__init__()
        c = {**VIT_L14_TEXT, **dict(hf_config or {})}
        if c["hidden_act"] != "quick_gelu":
            raise NotImplementedError(f"CLIP text tower: hidden_act {c['hidden_act']!r} (only 'quick_gelu' has a kernel)")
        if c["hidden_size"] != 64 * c["num_attention_heads"]:
            raise NotImplementedError("CLIP text tower: the attention kernel needs d_h = 64")
        self.config = _Config(c)
        self.text_model = _TextTransformer(c)
        self.text_projection = nn.Linear(c["hidden_size"], c["projection_dim"], bias=False)


class CLIPLanguageEncoder(_PostNormBase):
    """modules/language/clip.py:11-42.  ``forward(txt_ids, txt_masks)`` ([n, T] int64, [n, T] bool with True = valid) returns
    [n, T, output_dim] ('mlp' projection) or [n, T, projection_dim].  The tower is frozen (``requires_grad=False``, forward under
    ``no_grad``); the projection stage trains.  ``hf_config`` (a dict of ``CLIPTextConfig`` fields over the ViT-L/14 text defaults)
    sets the architecture; ``weights`` is kept for signature parity and is never fetched -- load a checkpoint with
    ``load_state_dict``.  No host synchronisation in forward: capturable in a HIP graph once the weight pack is built (first call)."""

    def __init__(self, cfg, weights="openai/clip-vit-large-patch14", output_dim=768, freeze_backbone=True, use_projection=False,
                 projection_type="mlp", num_projection_layers=1, dropout=0.1, hf_config=None):
        super().__init__()
        if not freeze_backbone:
            raise NotImplementedError("CLIPLanguageEncoder: freeze_backbone=False (a backward through the text tower) is out of scope")
        self.weights = weights
        self.model = CLIPTextTower(hf_config)
        self.model.requires_grad_(False)
        self.use_projection, self.projection_type = use_projection, projection_type
        self.dropout_p, self._drop_base = float(dropout), DROP_BASE_TXT_ENC
        hidden = self.model.config.hidden_size
        if use_projection:
            if projection_type == "mlp":
                self.projection = get_mlp_head(hidden, output_dim, output_dim, dropout=dropout)
            elif projection_type == "attention":
                self.projection = layer_repeat(SelfAttentionLayer(hidden, nhead=12, dropout=dropout, normalize_before=False,
                                                                  batch_first=True), num_projection_layers)
                for i, layer in enumerate(self.projection):   # one dropout-site range per layer
                    layer._drop_base = DROP_BASE_TXT_ENC + ((i + 1) << 12)
            else:
                raise NotImplementedError(projection_type)
        self._packs: Dict = {}

    # -- frozen weights, packed once per (device, compute mode): q|k|v as one [3 d, d] operand, copies in the operand dtype
    def _pack(self, device):
        ps = list(self.model.parameters())
        stamp = (sum(p._version for p in ps), ps[0].data_ptr())
        key = (str(device), self.compute)
        hit = self._packs.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
        wdt = _MODE[self.compute][1]
        w = lambda t: t.detach().to(wdt).contiguous()
        layers = []
        for lyr in self.model.text_model.encoder.layers:
            a = lyr.self_attn
            layers.append(dict(
                wqkv=torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach().to(wdt).contiguous(),
                bqkv=torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0).detach().contiguous(),
                wo=w(a.out_proj.weight), bo=a.out_proj.bias.detach(), w1=w(lyr.mlp.fc1.weight), b1=lyr.mlp.fc1.bias.detach(),
                w2=w(lyr.mlp.fc2.weight), b2=lyr.mlp.fc2.bias.detach()))
        pack = dict(layers=layers, wproj=w(self.model.text_projection.weight))
        self._packs[key] = (stamp, pack)
        return pack

    @torch.no_grad()
    def _tower(self, txt_ids: torch.Tensor, txt_masks: torch.Tensor) -> torch.Tensor:
        """CLIPTextModelWithProjection(...).last_hidden_state -> text_projection -> F.normalize(p=2, dim=2), fp32 [n, T, proj]."""
        tm, c = self.model.text_model, self.model.config
        n, T = txt_ids.shape
        if T > c.max_position_embeddings or T > ATTN_CAUSAL_MAX_T:
            raise ValueError(f"CLIPLanguageEncoder: {T} tokens; the position table has {c.max_position_embeddings} rows and the "
                             f"attention kernel covers {ATTN_CAUSAL_MAX_T}")
        ct, ad = _MODE[self.compute]
        pk = self._pack(txt_ids.device)
        valid = txt_masks if txt_masks.dtype == torch.bool else txt_masks != 0
        H, eps = c.num_attention_heads, c.layer_norm_eps
        ln = lambda x_, m: ops.add_layernorm(None, [x_], [m.weight], [m.bias], eps=eps, out_dtype=ad)
        x = clip_embed(tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight, txt_ids)   # fp32 residual stream
        for lyr, p in zip(tm.encoder.layers, pk["layers"]):
            qkv = ops.linear(ln(x, lyr.layer_norm1), p["wqkv"], p["bqkv"], ct=ct, out_dtype=ad)
            x = ops.linear(attn_causal(qkv, valid, H), p["wo"], p["bo"], ct=ct, residual=x)
            h = ops.linear(ln(x, lyr.layer_norm2), p["w1"], p["b1"], ct=ct, act="quick_gelu", out_dtype=ad)
            x = ops.linear(h, p["w2"], p["b2"], ct=ct, residual=x)
        y = ops.linear(ln(x, tm.final_layer_norm), pk["wproj"], None, ct=ct)
        return l2norm_rows(y)

    def forward(self, txt_ids: torch.Tensor, txt_masks: torch.Tensor) -> torch.Tensor:
        txt = self._tower(txt_ids, txt_masks)
        if not self.use_projection:
            return txt
        if self.projection_type == "mlp":
            dev = txt.device
            return mlp_head_forward(self.projection, txt, self.ct, drop=self._drop(self._head_ctx(dev), ops.DROP_MLP_HEAD, dev))
        kpm = txt_masks.logical_not()
        for layer in self.projection:
            txt = layer(txt, tgt_key_padding_mask=kpm)
        return txt
