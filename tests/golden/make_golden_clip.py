#!/usr/bin/env python3
"""Generate F25_clip_text.npz by running the reference's own text prompt encoder class (modules/language/clip.py:
CLIPLanguageEncoder) on seeded token ids (runs where the reference is present; never imported by the product).

    python tests/golden/make_golden_clip.py [--out PATH]

The reference is imported with make_golden.py's stand-in recipe.  The pretrained checkpoint cannot be fetched, so
``CLIPTextModelWithProjection.from_pretrained`` is pointed at a random-init model of the TINY architecture for the duration of
the construction (as run_t5_case does for T5); the third-party body stays whatever the installed transformers computes.
Weights are NOT stored: they are regenerated from ``pq3d_amd.synth`` (name + seed keyed); a checksum detects RNG drift.

Stored per case ('mlp': use_projection, projection_type 'mlp', output_dim 96; 'attn': projection_type 'attention', one layer):
  backbone   the frozen tower's output after text_projection and F.normalize, [n, T, 192] fp32
  out        the module's output in eval mode, [n, T, 96 or 192] fp32
  (both with the rows of masked query positions zeroed: those are don't-care, the decoder masks them)
  grad/projection.*  ('mlp' only) gradients of the projection stage for loss = mean(out * loss_weight * valid), sampled
  meta/bf16_err/<case>/{backbone,out}  max |bf16 - fp32| at valid positions of the SAME reference module run under CPU bf16 autocast
  meta/keys/<case>  the module's state_dict keys and shapes
Inputs: ids [5, 77], masks [5, 77] (True = valid): valid lengths 77, 12, 2, 1 and one prompt of length 20 with a masked key in
the middle of its valid span.
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from pq3d_amd import synth  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "F25_clip_text.npz")
TINY = dict(vocab_size=512, hidden_size=192, intermediate_size=768, num_hidden_layers=2, num_attention_heads=3,
            max_position_embeddings=77, projection_dim=192, hidden_act="quick_gelu", bos_token_id=0, pad_token_id=1, eos_token_id=2)
CASES = {"mlp": dict(use_projection=True, projection_type="mlp", output_dim=96),
         "attn": dict(use_projection=True, projection_type="attention", num_projection_layers=1)}
SEED, T = 17, 77
LENGTHS, HOLE = (77, 12, 2, 1, 20), (4, 9)     # prompt 4: key 9 of its 20 valid tokens is masked


def load_make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


def inputs():
    r = np.random.default_rng(SEED)
    ids = r.integers(3, TINY["vocab_size"], (len(LENGTHS), T))
    masks = np.arange(T)[None, :] < np.array(LENGTHS)[:, None]
    for b, n in enumerate(LENGTHS):
        ids[b, 0] = TINY["bos_token_id"]
        if n > 1:
            ids[b, n - 1] = TINY["eos_token_id"]
        ids[b, n:] = TINY["pad_token_id"]
    masks[HOLE] = False
    return torch.from_numpy(ids), torch.from_numpy(masks)


def build_head(case):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    if "modules.language" not in sys.modules:      # a bare package: modules/language/__init__.py would import the BERT encoder too
        m = types.ModuleType("modules.language")
        m.__path__ = [os.path.join(REF, "modules", "language")]
        sys.modules["modules.language"] = m
    orig = CLIPTextModelWithProjection.from_pretrained
    CLIPTextModelWithProjection.from_pretrained = classmethod(lambda cls, weights, **kw: cls(CLIPTextConfig(**TINY)))
    try:
        clip = importlib.import_module("modules.language.clip")
        torch.manual_seed(0)
        head = clip.CLIPLanguageEncoder(None, weights="tiny", **CASES[case])
    finally:
        CLIPTextModelWithProjection.from_pretrained = orig
    return head


def backbone(head, ids, masks):
    with torch.no_grad():
        txt = head.model(ids, masks).last_hidden_state
        return torch.nn.functional.normalize(head.model.text_projection(txt), p=2, dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    out_path = ap.parse_args().out
    if not os.path.isdir(REF):
        print("reference not present: nothing generated")
        return
    mg = load_make_golden()
    mg.import_reference()
    ids, masks = inputs()
    out = {"meta/args": np.array(repr(dict(seed=SEED, hf_config=TINY, cases=CASES, lengths=LENGTHS, hole=HOLE))),
           "ids": ids.numpy(), "masks": masks.numpy()}
    keep = masks[..., None].float()
    for case in CASES:
        head = build_head(case)
        sd = synth.fill_module(head, SEED)
        head.eval()
        out[f"meta/weights_checksum/{case}"] = np.float64(synth.state_checksum(sd))
        out[f"meta/keys/{case}"] = np.array(repr([(k, tuple(v.shape)) for k, v in head.state_dict().items()]))
        bb = backbone(head, ids, masks)
        y = head(ids, masks)
        out[f"{case}/backbone"] = (bb * keep).numpy()
        out[f"{case}/out"] = (y.detach() * keep).numpy()
        if case == "mlp":
            loss = (y * mg.loss_weight("clip_mlp", y.shape) * keep).mean()
            loss.backward()
            out["mlp/loss"] = np.float64(loss.item())
            for n, p in head.projection.named_parameters():
                mg.put(out, "grad/projection." + n, p.grad, mg.MAX_GRAD)
            assert all(p.grad is None for p in head.model.parameters())
        with torch.autocast("cpu", dtype=torch.bfloat16):
            bb16, y16 = backbone(head, ids, masks), head(ids, masks)
        out[f"meta/bf16_err/{case}/backbone"] = np.float64(((bb16.float() - bb).abs() * keep).max())
        out[f"meta/bf16_err/{case}/out"] = np.float64(((y16.detach().float() - y.detach()).abs() * keep).max())
        print(case, "bf16 autocast err: backbone", float(out[f"meta/bf16_err/{case}/backbone"]), "out", float(out[f"meta/bf16_err/{case}/out"]),
              "| max|out|", float((y.detach() * keep).abs().max()))
    np.savez_compressed(out_path, **out)
    print(f"{out_path}: {os.path.getsize(out_path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
