"""CPU: the restatement of the filter / DBSCAN options of the instance-prediction step (tests/instseg_dbscan_ref.py) reproduces
the reference's own InstSegEval.eval_instance_step outputs in tests/golden/F24_instseg_dbscan.npz
(tests/golden/make_golden_instseg_dbscan.py), and its exact fp64 adjacency rule joins pairs at eps +- 1 ulp exactly as
sklearn's DBSCAN(algorithm='kd_tree') does."""
import os

import numpy as np
import pytest
import torch

from tests import instseg_dbscan_ref, instseg_ref, util

F24 = os.path.join(util.GOLDEN, "F24_instseg_dbscan.npz")
CASES = ["filt_k100", "filt_kall", "dbscan_k100", "dbscan_kall", "both_k100", "both_kall"]
KEYS = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps")


def f24_scene(z, name, b):
    """(inputs of scene b of case `name` as CPU tensors, the reference's record)."""
    inp = {k: torch.from_numpy(z[f"{name}/{b}/{k}"]).long() for k in KEYS}
    for k in ("pred_logits", "pred_masks", "raw_coordinates", "voxel_coordinates"):
        inp[k] = torch.from_numpy(z[f"{name}/{b}/{k}"])
    P, K = inp["voxel_to_full_maps"].numel(), z[f"{name}/{b}/scores"].shape[0]
    ref = dict(masks=np.unpackbits(z[f"{name}/{b}/masks_packed"], count=P * K).reshape(P, K).astype(bool),
               scores=z[f"{name}/{b}/scores"], classes=z[f"{name}/{b}/classes"], boxes=z[f"{name}/{b}/boxes"],
               box_valid=z[f"{name}/{b}/box_valid"])
    return inp, ref


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_fixture(name):
    z = np.load(F24)
    B, topk = int(z[f"{name}/B"]), int(z[f"{name}/topk"])
    filt, dbscan, eps = bool(z[f"{name}/filter"]), bool(z[f"{name}/dbscan"]), float(z[f"{name}/eps"])
    for b in range(B):
        inp, ref = f24_scene(z, name, b)
        got = instseg_dbscan_ref.scene_predictions(inp["pred_logits"][0], inp["pred_masks"][0], inp["voxel2segment"],
                                                   inp["voxel_to_full_maps"], inp["segment_to_full_maps"],
                                                   inp["raw_coordinates"], inp["voxel_coordinates"], topk, filt, dbscan, eps)
        instseg_ref.assert_match(got, ref, what=f"{name} scene {b}")


@pytest.mark.parametrize("eps", [0.95, 0.5, 1.25, 0.05])
def test_exact_rule_matches_kd_tree_dbscan_at_eps_ulps(eps):
    from sklearn.cluster import DBSCAN
    pairs = instseg_dbscan_ref.eps_ulp_pairs(eps)
    joined = [int(instseg_dbscan_ref.components(p, eps).max() == 0) for p in pairs]
    sk = [int(DBSCAN(eps=eps, min_samples=1, algorithm="kd_tree").fit(p.astype(np.float64)).labels_.max() == 0) for p in pairs]
    assert joined == sk
    assert 0 < sum(joined) < len(joined), "the pairs straddle the boundary"


def test_components_are_numbered_by_smallest_index():
    x = np.array([[5, 0, 0], [0, 0, 0], [5.5, 0, 0], [0.5, 0, 0], [20, 0, 0]], np.float32)
    assert instseg_dbscan_ref.components(x, 0.95).tolist() == [0, 1, 0, 1, 2]


def test_dbscan_option_needs_voxel_coordinates_before_any_launch():
    from pq3d_amd import synth
    from pq3d_amd.instseg import instance_predictions
    inp = synth.instseg_inputs(2, P=(100,), S=20, Q=8, C=6)
    args = [inp["pred_logits"], inp["pred_masks"]] + [inp[k] for k in KEYS + ("raw_coordinates",)]
    with pytest.raises(Exception):      # host tensors or a missing coordinate list: refused, never computed on the host
        instance_predictions(*args, topk_per_scene=10, use_dbscan=True)
