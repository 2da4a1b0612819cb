"""CPU: the numpy restatement of the scene-preparation rules (tests/scene_prep_ref.py) is itself right where that can be
known without the reference's libraries: the quantisation rule is torch-CPU's, voxelize is a consistent first-occurrence
grouping, and farthest point sampling gives a sequence that can be checked by hand."""
import numpy as np
import torch

from tests import scene_prep_ref as R

VS = 0.02


def _neighbours(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))])


def quantisation_data() -> np.ndarray:
    """Random values plus every lattice multiple k * fp32(0.02), |k| <= 20000 (+-400 m), and its two fp32 neighbours."""
    r = np.random.default_rng(11)
    k = np.arange(-20000, 20001, dtype=np.float32)
    return np.concatenate([r.uniform(-60, 60, 2_000_000).astype(np.float32), _neighbours(k * np.float32(VS))])


def test_quantisation_rule_is_torch_cpu_division_and_not_the_reciprocal():
    x = quantisation_data()
    want = torch.floor(torch.from_numpy(x) / VS).long().numpy()      # the reference: np.floor(coordinates / voxel_size) on a tensor
    assert np.array_equal(R.quantize(x, VS), want)
    assert np.array_equal(R.quantize(x.astype(np.float64), VS), want)
    wrong = int((R.quantize_reciprocal(x, VS) != want).sum())
    assert wrong > 0, "the multiply-by-reciprocal form must differ on this data: the case has gone blunt"


def test_restated_voxelize_is_a_first_occurrence_grouping():
    r = np.random.default_rng(5)
    scenes = [r.uniform(-0.3, 0.3, (700, 3)).astype(np.float32), r.uniform(0, 0.1, (1, 3)).astype(np.float32),
              np.repeat(r.uniform(-1, 1, (30, 3)), 20, 0).astype(np.float32)[r.permutation(600)]]
    vc, umaps, invs = R.voxelize(scenes, VS)
    assert vc.dtype == np.int32 and vc.shape == (sum(len(u) for u in umaps), 4)
    at = 0
    for b, c in enumerate(scenes):
        q, um, inv = R.quantize(c, VS), umaps[b], invs[b]
        assert np.array_equal(q[um][inv], q), "q[unique_map][inverse_map] != q"
        assert np.all(np.diff(um) > 0), "representatives must ascend"
        assert len(np.unique(q[um], axis=0)) == len(um), "a voxel appears twice"
        for v, i in enumerate(um):                                  # the representative is the voxel's first point
            assert i == np.flatnonzero(inv == v)[0]
        assert np.array_equal(vc[at:at + len(um), 0], np.full(len(um), b)) and np.array_equal(vc[at:at + len(um), 1:], q[um])
        at += len(um)
    assert len(umaps[1]) == 1 and len(umaps[2]) <= 30


def test_restated_fps_on_a_5x5_lattice():
    """Points (x, y, 0), index = 5 y + x.  From (0,0): the far corner 24 (d = 32); then the corners 4 and 20 tie at 16 (lower
    index first); the centre 12 (8); then the four edge midpoints tie at 4 and come in index order."""
    pts = np.array([(x, y, 0) for y in range(5) for x in range(5)], dtype=np.float32)
    assert R.fps(pts, 9).tolist() == [0, 24, 4, 20, 12, 2, 10, 14, 22]
    assert R.fps(pts, 3, start_idx=12).tolist() == [12, 0, 4]
    same = np.ones((7, 3), dtype=np.float32)
    assert R.fps(same, 4).tolist() == [0, 0, 0, 0]
