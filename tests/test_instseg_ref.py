"""CPU: the restatement of the instance-prediction step (tests/instseg_ref.py) reproduces the reference's own
InstSegEval.eval_instance_step outputs stored in tests/golden/F22_instseg_predict.npz (tests/golden/make_golden_instseg.py),
and the product entry point refuses host tensors (no CPU fallback)."""
import os

import numpy as np
import pytest
import torch

from pq3d_amd import synth
from tests import instseg_ref, util

F22 = os.path.join(util.GOLDEN, "F22_instseg_predict.npz")
KEYS = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps", "raw_coordinates")


@pytest.mark.parametrize("name", ["k100", "kall"])
def test_restatement_matches_reference_fixture(name):
    z = np.load(F22)
    B, topk = int(z[f"{name}/B"]), int(z[f"{name}/topk"])
    logits, masks = torch.from_numpy(z[f"{name}/pred_logits"]), torch.from_numpy(z[f"{name}/pred_masks"])
    assert torch.isinf(logits).any(), "the fixture holds -inf logit columns"
    for b in range(B):
        idx = [torch.from_numpy(z[f"{name}/{b}/{k}"]).long() for k in KEYS[:3]]
        xyz = torch.from_numpy(z[f"{name}/{b}/raw_coordinates"])
        got = instseg_ref.scene_predictions(logits[b], masks[b], *idx, xyz, topk)
        P, K = idx[1].numel(), z[f"{name}/{b}/scores"].shape[0]
        assert K == (logits.shape[1] if topk == -1 else topk)
        ref = dict(masks=np.unpackbits(z[f"{name}/{b}/masks_packed"], count=P * K).reshape(P, K).astype(bool),
                   scores=z[f"{name}/{b}/scores"], classes=z[f"{name}/{b}/classes"], boxes=z[f"{name}/{b}/boxes"],
                   box_valid=z[f"{name}/{b}/box_valid"])
        assert not ref["box_valid"].all(), "the fixture holds empty masks"
        instseg_ref.assert_match(got, ref, what=f"{name} scene {b}")


def test_synthetic_scenes_are_seeded_and_have_straddling_voxels():
    a = synth.instseg_inputs(9, P=(3000, 800), S=100)
    b = synth.instseg_inputs(9, P=(3000, 800), S=100)
    assert torch.equal(a["pred_masks"], b["pred_masks"])
    for k in KEYS:
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k]))
    s1 = a["voxel2segment"][0][a["voxel_to_full_maps"][0]]
    assert (s1 != a["segment_to_full_maps"][0]).any()


def test_instance_predictions_refuses_host_tensors():
    from pq3d_amd._lib import Pq3dError
    from pq3d_amd.instseg import instance_predictions
    inp = synth.instseg_inputs(2, P=(100,), S=20, Q=8, C=6)
    with pytest.raises(Pq3dError):
        instance_predictions(inp["pred_logits"], inp["pred_masks"], *[inp[k] for k in KEYS], topk_per_scene=10)
