"""CPU: the float64 restatement of the CLIP text prompt encoder (tests/clip_text_ref.py) against fixture F25 (the reference's own
CLIPLanguageEncoder over the installed transformers), the state_dict contract of pq3d_amd.clip_text.CLIPLanguageEncoder, and
make_cfg / Query3DUnified with and without a configured text encoder."""
import ast

import numpy as np
import pytest
import torch

from pq3d_amd.model import Query3DUnified, make_cfg
from tests import clip_text_ref as R
from tests import util

TOL = dict(atol=1e-5, rtol=1e-5)   # tests/test_oracle_golden.py's bar for fp32 fixtures
CASES = ("mlp", "attn")


def close(got, want, atol, rtol):
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= atol + rtol * scale, f"max abs err {err:.3e} (scale {scale:.3e})"
    return err


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture(case):
    z, a = util.load_fixture("F25_clip_text")
    _enc, sd = R.fixture_module(z, a, case)
    ids, masks = torch.from_numpy(z["ids"]), torch.from_numpy(z["masks"])
    assert masks[:, 0].all() and not masks[a["hole"]] and masks[a["hole"][0], a["hole"][1] + 1]
    bb, out = R.encoder(sd, a["hf_config"], a["cases"][case], ids, masks)
    v = masks.numpy()
    close(bb.numpy()[v], z[f"{case}/backbone"][v], **TOL)
    close(out.numpy()[v], z[f"{case}/out"][v], **TOL)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_keys_match_the_reference_module(case):
    z, a = util.load_fixture("F25_clip_text")
    enc, _sd = R.fixture_module(z, a, case)
    ref = ast.literal_eval(str(z[f"meta/keys/{case}"]))
    assert [(k, tuple(v.shape)) for k, v in sorted(enc.state_dict().items())] == sorted(ref)
    assert all(not p.requires_grad for p in enc.model.parameters()) and all(p.requires_grad for p in enc.projection.parameters())


def test_default_architecture_is_vit_l14_text_and_nothing_is_fetched():
    from pq3d_amd import CLIPLanguageEncoder
    with torch.device("meta"):
        enc = CLIPLanguageEncoder(None)
    sd = enc.state_dict()
    assert sd["model.text_model.embeddings.token_embedding.weight"].shape == (49408, 768)
    assert sd["model.text_model.embeddings.position_embedding.weight"].shape == (77, 768)
    assert sd["model.text_model.encoder.layers.11.mlp.fc1.weight"].shape == (3072, 768)
    assert sd["model.text_projection.weight"].shape == (768, 768) and not hasattr(enc, "projection")
    with pytest.raises(NotImplementedError):
        CLIPLanguageEncoder(None, freeze_backbone=False)


def test_make_cfg_without_a_text_encoder_is_unchanged():
    kw = dict(d=64, H=4, L=1, memories=["voxel", "prompt"], heads=["ground"], structure="mixed")
    z, a = util.load_fixture("F25_clip_text")
    plain, none = Query3DUnified(make_cfg(**kw)), Query3DUnified(make_cfg(**kw, txt_encoder=None))
    assert "txt_encoder" not in make_cfg(**kw).model
    assert list(plain.state_dict()) == list(none.state_dict()) and not hasattr(plain, "txt_encoder")
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in none.named_modules()]
    dd = {"prompt": torch.zeros(2, 5), "prompt_pad_masks": torch.ones(2, 5, dtype=torch.bool), "prompt_type": torch.tensor([1, 1])}
    with pytest.raises(NotImplementedError):
        plain.prompt_encoder(dd)
    with_txt = Query3DUnified(make_cfg(**kw, txt_encoder=dict(hf_config=a["hf_config"], output_dim=64, use_projection=True)))
    extra = [k for k in with_txt.state_dict() if k not in plain.state_dict()]
    assert extra and all(k.startswith("txt_encoder.") for k in extra) and len(with_txt.state_dict()) == len(plain.state_dict()) + len(extra)
    groups = with_txt.get_opt_params()      # frozen tower skipped, every trainable parameter covered
    got = {id(p) for g in groups for p in g["params"]}
    assert got == {id(p) for p in with_txt.parameters() if p.requires_grad}
    assert not got & {id(p) for p in with_txt.txt_encoder.model.parameters()}
    assert {id(p) for p in with_txt.txt_encoder.projection.parameters()} <= got
