"""GPU: instance predictions with filter_out_no_object_queries / use_dbscan (pq3d_amd.instseg.instance_predictions,
csrc/instseg_dbscan.hip, the ragged top-k of csrc/instseg.hip) against the reference's own outputs
(tests/golden/F24_instseg_dbscan.npz) and the CPU restatement tests/instseg_dbscan_ref.py, with the bars of
test_gpu_instseg.py: classes, masks and box extents exact column for column, scores and box centers within rtol 1e-5, tied
scores compared as a set."""
import os

import numpy as np
import pytest
import torch

from pq3d_amd import synth
from pq3d_amd.instseg import instance_predictions
from tests import instseg_dbscan_ref, instseg_ref, util
from tests.test_instseg_dbscan_ref import CASES, f24_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
F24 = os.path.join(util.GOLDEN, "F24_instseg_dbscan.npz")
KEYS = ("voxel2segment", "voxel_to_full_maps", "segment_to_full_maps", "raw_coordinates")


def _call(inp, topk, filt=False, dbscan=False, eps=0.95, xyzv=None):
    return instance_predictions(inp["pred_logits"].to(DEV), inp["pred_masks"].to(DEV),
                                *[[t.to(DEV) for t in inp[k]] for k in KEYS], topk_per_scene=topk,
                                filter_out_no_object_queries=filt, use_dbscan=dbscan,
                                voxel_coordinates=None if xyzv is None else [t.to(DEV) for t in xyzv], dbscan_eps=eps)


def _ref(inp, b, topk, filt, dbscan, eps, xyzv):
    return instseg_dbscan_ref.scene_predictions(inp["pred_logits"][b], inp["pred_masks"][b],
                                                *[inp[k][b] for k in KEYS], None if xyzv is None else xyzv[b], topk,
                                                filt, dbscan, eps)


def _check_record(r, P):
    K = r["scores"].shape[0]
    assert r["masks"].shape == (P, K) and r["masks"].dtype == torch.bool and r["masks"].is_cuda
    assert r["classes"].shape == (K,) and r["classes"].dtype == torch.int64
    assert r["boxes"].shape == (K, 6) and r["box_valid"].shape == (K,)


@pytest.mark.parametrize("name", CASES)
def test_f24_matches_reference_eval_instance_step(name):
    z = np.load(F24)
    B, topk = int(z[f"{name}/B"]), int(z[f"{name}/topk"])
    filt, dbscan, eps = bool(z[f"{name}/filter"]), bool(z[f"{name}/dbscan"]), float(z[f"{name}/eps"])
    for b in range(B):
        one, ref = f24_scene(z, name, b)
        inp = {"pred_logits": one["pred_logits"], "pred_masks": one["pred_masks"]}
        inp.update({k: [one[k]] for k in KEYS})
        got = _call(inp, topk, filt, dbscan, eps, [one["voxel_coordinates"]] if dbscan else None)[0]
        _check_record(got, one["voxel_to_full_maps"].numel())
        instseg_ref.assert_match(got, ref, what=f"F24 {name} scene {b}")


def _scenes(seed, P=(1500, 900, 1200), S=64, Q=20, C=30):
    inp = synth.instseg_inputs(seed, P=P, S=S, Q=Q, C=C)
    inp["pred_logits"][:, 3, C] = 12.0          # dropped by the filter
    return inp, synth.instseg_voxel_coordinates(inp)


@pytest.mark.parametrize("filt,dbscan", [(True, False), (False, True), (True, True)])
def test_batched_equals_per_scene_and_restatement_and_runs_are_bit_identical(filt, dbscan):
    inp, xyzv = _scenes(41)
    got = _call(inp, 60, filt, dbscan, 0.95, xyzv)
    again = _call(inp, 60, filt, dbscan, 0.95, xyzv)
    for b in range(3):
        one = {"pred_logits": inp["pred_logits"][b:b + 1], "pred_masks": inp["pred_masks"][b:b + 1]}
        one.update({k: inp[k][b:b + 1] for k in KEYS})
        single = _call(one, 60, filt, dbscan, 0.95, xyzv[b:b + 1])[0]
        for k in ("masks", "scores", "classes", "boxes", "box_valid"):
            assert torch.equal(got[b][k], single[k]), (b, k)
            assert torch.equal(got[b][k], again[b][k]), (b, k)
        instseg_ref.assert_match(got[b], _ref(inp, b, 60, filt, dbscan, 0.95, xyzv), what=f"scene {b}")


def test_large_room_matches_restatement():
    """~50k voxels on room surfaces, Q = 100, C = 200, K = 100, filter + DBSCAN."""
    inp = synth.instseg_room(3, V=50_000, Q=100, C=200)
    xyzv = inp.pop("voxel_coordinates")
    got = _call(inp, 100, True, True, 0.95, xyzv)[0]
    ref = _ref(inp, 0, 100, True, True, 0.95, xyzv)
    _check_record(got, 50_000)
    instseg_ref.assert_match(got, ref, what="room 50k")


def test_many_components_stream_the_top_k_from_memory():
    """eps below the 0.1 lattice of the coordinates: every lattice point its own component, Q' * C > 49 152 candidates (the
    R = 0 top-k path)."""
    inp = synth.instseg_inputs(42, P=(2000,), S=64, Q=8, C=200)
    xyzv = synth.instseg_voxel_coordinates(inp, cut_segments=0)
    got = _call(inp, 100, False, True, 0.09, xyzv)[0]
    prob, _ = instseg_dbscan_ref.columns(inp["pred_logits"][0], inp["pred_masks"][0], inp["voxel2segment"][0], xyzv[0],
                                         False, True, 0.09)
    assert prob.numel() > 49_152
    ref = _ref(inp, 0, 100, False, True, 0.09, xyzv)
    instseg_ref.assert_match(got, ref, what="many components")


@pytest.mark.parametrize("eps", [0.95, 0.05])      # shifted pairs that still straddle the boundary
def test_eps_ulp_pairs_match_restatement(eps):
    pairs = instseg_dbscan_ref.eps_ulp_pairs(eps)
    n = pairs.shape[0]
    # one scene: the pairs 3 eps + 3 apart along x, one segment and one query covering all voxels
    xyz = pairs.copy()
    xyz[:, :, 0] += (np.arange(n, dtype=np.float32) * np.float32(3 * eps + 3))[:, None]
    xyz = xyz.reshape(-1, 3)
    V = xyz.shape[0]
    inp = {"pred_logits": torch.zeros(1, 1, 3), "pred_masks": torch.ones(1, 1, 1),
           "voxel2segment": [torch.zeros(V, dtype=torch.int64)], "voxel_to_full_maps": [torch.arange(V)],
           "segment_to_full_maps": [torch.arange(V)], "raw_coordinates": [torch.from_numpy(xyz)]}
    xyzv = [torch.from_numpy(xyz)]
    got = _call(inp, -1, False, True, eps, xyzv)[0]
    joined = [int(instseg_dbscan_ref.components(p, eps).max() == 0) for p in xyz.reshape(n, 2, 3)]   # after the shift
    assert 0 < sum(joined) < n
    assert got["scores"].shape[0] == sum(2 - j for j in joined)
    ref = _ref(inp, 0, -1, False, True, eps, xyzv)
    instseg_ref.assert_match(got, ref, what=f"eps {eps} pairs")


def test_every_query_filtered_gives_an_empty_record():
    inp, xyzv = _scenes(43, P=(800, 700), Q=10, C=12)
    inp["pred_logits"][0, :, 12] = 50.0                    # scene 0: every query's argmax is no-object
    for dbscan in (False, True):
        got = _call(inp, 20, True, dbscan, 0.95, xyzv)
        assert got[0]["masks"].shape == (800, 0) and got[0]["scores"].shape == (0,)
        assert got[1]["scores"].shape[0] == 20


def test_eps_beyond_the_scene_gives_the_plain_path():
    inp = synth.instseg_inputs(44, P=(1500, 1000), S=64, Q=20, C=30, empty_queries=0)
    xyzv = synth.instseg_voxel_coordinates(inp, cut_segments=0)
    plain = _call(inp, 50)
    big = _call(inp, 50, False, True, 1000.0, xyzv)
    for b in range(2):
        assert big[b]["scores"].shape == plain[b]["scores"].shape
        instseg_ref.assert_match(big[b], {k: v.cpu() for k, v in plain[b].items()}, what=f"scene {b}")


def test_bad_inputs_raise_value_error():
    inp, xyzv = _scenes(45, P=(600,), Q=6, C=8)
    with pytest.raises(ValueError):
        _call(inp, 10, False, True, 0.95, None)                      # missing voxel_coordinates
    with pytest.raises(ValueError):
        _call(inp, 10, False, True, 0.95, [xyzv[0][:-1]])             # mis-shaped
    with pytest.raises(ValueError):
        _call(inp, 10, False, True, 0.0, xyzv)                        # eps <= 0
    bad = xyzv[0].clone()
    bad[5, 1] = float("nan")
    with pytest.raises(ValueError):
        _call(inp, 10, False, True, 0.95, [bad])                      # non-finite, through the flag word
    far = xyzv[0].clone()
    far[0, 0] = 1e6
    with pytest.raises(ValueError):
        _call(inp, 10, False, True, 0.95, [far])                      # grid beyond 2^24 cells
