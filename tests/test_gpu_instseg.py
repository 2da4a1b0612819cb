"""GPU: instance-segmentation predictions (pq3d_amd.instseg.instance_predictions, csrc/instseg.hip) against the reference's own
InstSegEval.eval_instance_step outputs (tests/golden/F22_instseg_predict.npz, tests/golden/make_golden_instseg.py) and the
CPU restatement tests/instseg_ref.py: classes, masks and box extents exactly equal column for column in sorted order, scores
and box centers within rtol 1e-5, tied scores compared as a set."""
import os

import numpy as np
import pytest
import torch

from pq3d_amd import synth
from pq3d_amd.instseg import instance_predictions
from tests import instseg_ref, util

pytestmark = pytest.mark.gpu
DEV = "cuda"
F22 = os.path.join(util.GOLDEN, "F22_instseg_predict.npz")
KEYS = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps", "raw_coordinates")


def _f22_cases():
    z = np.load(F22)
    return z, sorted({k.split("/")[0] for k in z.files})


def _to_dev(inp):
    out = {"pred_logits": inp["pred_logits"].to(DEV), "pred_masks": inp["pred_masks"].to(DEV)}
    for k in KEYS:
        out[k] = [t.to(DEV) for t in inp[k]]
    return out


def _call(inp, topk):
    d = _to_dev(inp)
    return instance_predictions(d["pred_logits"], d["pred_masks"], d["voxel2segment"], d["voxel_to_full_maps"],
                                d["segment_to_full_maps"], d["raw_coordinates"], topk_per_scene=topk)


def _f22_case(z, name):
    B = int(z[f"{name}/B"])
    inp = {"pred_logits": torch.from_numpy(z[f"{name}/pred_logits"]), "pred_masks": torch.from_numpy(z[f"{name}/pred_masks"])}
    for k in KEYS:
        inp[k] = [torch.from_numpy(z[f"{name}/{b}/{k}"]).to(torch.float32 if k == "raw_coordinates" else torch.int64)
                  for b in range(B)]
    refs = []
    for b in range(B):
        P, K = inp["voxel_to_full_maps"][b].numel(), z[f"{name}/{b}/scores"].shape[0]
        masks = np.unpackbits(z[f"{name}/{b}/masks_packed"], count=P * K).reshape(P, K).astype(bool)
        refs.append(dict(masks=masks, scores=z[f"{name}/{b}/scores"], classes=z[f"{name}/{b}/classes"],
                         boxes=z[f"{name}/{b}/boxes"], box_valid=z[f"{name}/{b}/box_valid"]))
    return inp, int(z[f"{name}/topk"]), refs


def _check_record(r, P, K):
    assert r["masks"].shape == (P, K) and r["masks"].dtype == torch.bool and r["masks"].is_cuda
    assert r["scores"].shape == (K,) and r["scores"].dtype == torch.float32
    assert r["classes"].shape == (K,) and r["classes"].dtype == torch.int64
    assert r["boxes"].shape == (K, 6) and r["boxes"].dtype == torch.float32
    assert r["box_valid"].shape == (K,) and r["box_valid"].dtype == torch.bool


@pytest.mark.parametrize("name", ["k100", "kall"])
def test_f22_matches_reference_eval_instance_step(name):
    """Every scene of a case in ONE batched call against the reference's preds / bbox_preds."""
    z, names = _f22_cases()
    assert name in names
    inp, topk, refs = _f22_case(z, name)
    got = _call(inp, topk)
    assert len(got) == len(refs)
    for b, (g, r) in enumerate(zip(got, refs)):
        _check_record(g, inp["voxel_to_full_maps"][b].numel(), r["scores"].shape[0])
        instseg_ref.assert_match(g, r, what=f"F22 {name} scene {b}")


def test_full_size_scene_matches_restatement():
    """P = 200k points, V ~ 100k voxels, S = 4096, Q = 200, C = 200, K = 100: masks exact."""
    inp = synth.instseg_inputs(1, P=(200_000,), S=4096, Q=200, C=200, mean_seg=60)
    assert instseg_ref.topk_gap(inp["pred_logits"][0], 100) > 1e-5
    got = _call(inp, 100)[0]
    ref = instseg_ref.predictions(inp, 100)[0]
    _check_record(got, 200_000, 100)
    instseg_ref.assert_match(got, ref, what="full size")


def test_batched_equals_per_scene_and_runs_are_bit_identical():
    inp = synth.instseg_inputs(7, P=(3000, 1200, 4100, 10), S=128, Q=32, C=30)
    got = _call(inp, 60)
    again = _call(inp, 60)
    for b in range(4):
        one = {"pred_logits": inp["pred_logits"][b:b + 1], "pred_masks": inp["pred_masks"][b:b + 1]}
        one.update({k: inp[k][b:b + 1] for k in KEYS})
        single = _call(one, 60)[0]
        for k in ("masks", "scores", "classes", "boxes", "box_valid"):
            assert torch.equal(got[b][k], single[k]), (b, k)
            assert torch.equal(got[b][k], again[b][k]), (b, k)


@pytest.mark.parametrize("K", [1, 1024])
def test_k_extremes(K):
    inp = synth.instseg_inputs(3, P=(2500, 1700), S=80, Q=64, C=40)
    for b in range(2):
        assert instseg_ref.topk_gap(inp["pred_logits"][b], K) > 1e-5
    got = _call(inp, K)
    for b, ref in enumerate(instseg_ref.predictions(inp, K)):
        _check_record(got[b], inp["voxel_to_full_maps"][b].numel(), K)
        instseg_ref.assert_match(got[b], ref, what=f"K={K} scene {b}")


@pytest.mark.parametrize("which", ["v2s_high", "v2s_neg", "v2f_high", "v2f_neg", "s2f_neg"])
def test_out_of_range_ids_raise_value_error(which):
    inp = synth.instseg_inputs(4, P=(900, 700), S=48, Q=16, C=12)
    S = inp["pred_masks"].shape[1]
    key, val = {"v2s_high": ("voxel2segment", S), "v2s_neg": ("voxel2segment", -1),
                "v2f_high": ("voxel_to_full_maps", inp["voxel2segment"][1].numel()), "v2f_neg": ("voxel_to_full_maps", -3),
                "s2f_neg": ("segment_to_full_maps", -1)}[which]
    inp[key][1] = inp[key][1].clone()
    inp[key][1][5] = val
    with pytest.raises(ValueError):
        _call(inp, 20)
    with pytest.raises(ValueError):         # more selections than (query, class) pairs, as torch.topk would refuse
        _call(synth.instseg_inputs(4, P=(50,), S=48, Q=4, C=3, ninf_cols=(), double_class=False), 13)


@pytest.mark.parametrize("compute", ["fp32", "bf16", "bf16x3"])
def test_end_to_end_from_mask_head(compute):
    """A c4-slice Query3DUnified with the mask head (F4b's configuration) runs a forward; its last-layer outputs are fp32 in
    every compute mode and their instance predictions match the CPU restatement on the same outputs."""
    from pq3d_amd.modules import set_compute
    z, args = util.load_fixture("F4b_c4_slice")
    _cfg, model, _sd, dd = util.model_case(args)
    set_compute(model, compute)
    model.to(DEV)
    with torch.no_grad():
        out = model({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in dd.items()})
    logits, masks = out["predictions_class"][-1], out["predictions_mask"][-1]
    assert logits.dtype == torch.float32 and masks.dtype == torch.float32, (logits.dtype, masks.dtype)
    B, Q, C1 = logits.shape
    S = masks.shape[1]
    maps = synth.instseg_inputs(5, P=(4000, 2500), S=S, Q=Q, C=C1 - 1, mean_seg=30)
    inp = {"pred_logits": logits.cpu(), "pred_masks": masks.cpu(), **{k: maps[k] for k in KEYS}}
    for b in range(B):
        assert instseg_ref.topk_gap(inp["pred_logits"][b], 100) > 1e-6
    got = instance_predictions(logits, masks, *[[t.to(DEV) for t in maps[k]] for k in KEYS], topk_per_scene=100)
    for b, ref in enumerate(instseg_ref.predictions(inp, 100)):
        instseg_ref.assert_match(got[b], ref, what=f"{compute} scene {b}")


def test_large_candidate_set_streams_from_the_probability_array():
    """Q*C = 60 000 candidates: above the register-resident capacity of the top-k workgroup (49 152)."""
    inp = synth.instseg_inputs(6, P=(1500, 900), S=64, Q=300, C=200)
    for b in range(2):
        assert instseg_ref.topk_gap(inp["pred_logits"][b], 200) > 1e-5
    got = _call(inp, 200)
    for b, ref in enumerate(instseg_ref.predictions(inp, 200)):
        instseg_ref.assert_match(got[b], ref, what=f"Q*C=60000 scene {b}")
