"""GPU: scene preparation (pq3d_amd/scene.py, csrc/scene_prep.hip) against the numpy restatement tests/scene_prep_ref.py:
voxelize and farthest point sampling are compared EXACTLY (integers and index sequences), centres against a float64 mean,
and the prepared batch drives Query3DUnified with its backbone and instance_predictions."""
import functools

import numpy as np
import pytest
import torch

from tests import scene_prep_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = 0.02
TILE = 256           # rows per tile of the FPS kernel for scenes of at most 2^18 points


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _surface(seed: int, n: int, room=(8.0, 6.0, 3.0)) -> np.ndarray:
    """n raw points on the floor and the four walls of a room (synth.instseg_room's surfaces, not snapped to the lattice)."""
    r = np.random.default_rng([seed, 99])
    X, Y, Z = room
    areas = np.array([X * Y, X * Z, X * Z, Y * Z, Y * Z])
    face = r.choice(5, n, p=areas / areas.sum())
    u, w, z = r.random(n), r.random(n), np.zeros(n)
    faces = [np.stack([u * X, w * Y, z], 1), np.stack([u * X, z, w * Z], 1), np.stack([u * X, z + Y, w * Z], 1),
             np.stack([z, u * Y, w * Z], 1), np.stack([z + X, u * Y, w * Z], 1)]
    xyz = np.zeros((n, 3))
    for f in range(5):
        xyz[face == f] = faces[f][face == f]
    return (xyz + r.normal(0, 0.004, (n, 3)) - np.array([X / 2, Y / 2, 0.5])).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ voxelize
def _check_voxelize(scenes, vs=VS):
    from pq3d_amd import scene
    dev = [_dev(s) for s in scenes]
    vc, um, inv = scene.voxelize(dev, vs)
    vc2, um2, inv2 = scene.voxelize(dev, vs)
    assert torch.equal(vc, vc2) and all(torch.equal(a, b) for a, b in zip(um + inv, um2 + inv2)), "two runs differ"
    rvc, rum, rinv = R.voxelize(scenes, vs)
    assert vc.dtype == torch.int32 and tuple(vc.shape) == rvc.shape
    assert np.array_equal(vc.cpu().numpy(), rvc), "voxel_coordinates differ"
    for b in range(len(scenes)):
        assert um[b].dtype == torch.int64 and inv[b].dtype == torch.int64
        assert np.array_equal(um[b].cpu().numpy(), rum[b]), f"unique_map of scene {b} differs"
        assert np.array_equal(inv[b].cpu().numpy(), rinv[b]), f"inverse_map of scene {b} differs"


@pytest.mark.parametrize("P", [1, 63, 64, 65, 5000])
def test_voxelize_one_scene(P):
    r = np.random.default_rng(P)
    _check_voxelize([r.uniform(-0.4, 0.4, (P, 3)).astype(np.float32)])


def test_voxelize_ragged_batch_with_a_one_point_scene():
    r = np.random.default_rng(3)
    _check_voxelize([r.uniform(-0.5, 0.3, (2049, 3)).astype(np.float32), r.uniform(-1, 1, (1, 3)).astype(np.float32),
                     r.uniform(0.0, 0.4, (777, 3)).astype(np.float32)])
    # the same cloud in two scenes: equal coordinates of different scenes are different voxels
    c = r.uniform(-0.2, 0.2, (300, 3)).astype(np.float32)
    _check_voxelize([c, c])


@pytest.mark.parametrize("P", [2047, 2048, 2049])
def test_voxelize_around_one_scan_block(P):
    """One block of the count / emit kernels' scan is PQ3D_VOXELIZE_BLOCK = 2048 points."""
    r = np.random.default_rng(P)
    _check_voxelize([r.uniform(-0.4, 0.4, (P, 3)).astype(np.float32)])


def test_voxelize_eight_scenes_with_boundaries_inside_a_block():
    """The scene table's maximum: one-point scenes, boundaries inside a 2048-point block (rows 1, 701, 702, 2049, 4098,
    4101) and one on a block's first row (2048)."""
    r = np.random.default_rng(14)
    lens = [1, 700, 1, 1346, 1, 2049, 3, 500]
    assert np.cumsum(lens).tolist()[:5] == [1, 701, 702, 2048, 2049]
    _check_voxelize([r.uniform(-0.3, 0.3, (n, 3)).astype(np.float32) for n in lens])


def test_voxelize_more_block_sums_than_scan_threads():
    """Above 2048 * 1024 points every thread of the one-workgroup scan of the block sums takes more than one of them.  The
    points come from 300 voxels, so that the restatement's table stays small."""
    r = np.random.default_rng(15)
    P = 2048 * 1024 + 3
    centres = (r.integers(-40, 40, (300, 3)) + 0.5) * VS
    pts = (centres[r.integers(0, 300, P)] + r.uniform(-0.4, 0.4, (P, 3)) * VS).astype(np.float32)
    _check_voxelize([pts])


def test_voxelize_many_duplicates():
    """5000 points in about 40 voxels: long runs on one table slot, atomicMin contention on the representative."""
    r = np.random.default_rng(8)
    centres = (r.integers(-30, 30, (40, 3)) + 0.5) * VS
    pts = (centres[r.integers(0, 40, 5000)] + r.uniform(-0.4, 0.4, (5000, 3)) * VS).astype(np.float32)
    assert len(R.voxelize([pts], VS)[1][0]) <= 40
    _check_voxelize([pts])
    _check_voxelize([np.zeros((700, 3), dtype=np.float32)])


def test_voxelize_negative_coordinates_and_voxel_boundaries():
    """Lattice multiples of fp32(0.02), negative ones included, and their fp32 neighbours: the points where the division
    rule decides the voxel (the reciprocal form differs on this data)."""
    r = np.random.default_rng(2)
    k = np.concatenate([np.arange(-3000, 3001), r.integers(-500000, 500000, 3000)]).astype(np.float32)
    x = k * np.float32(VS)
    x = np.concatenate([x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))])
    assert (R.quantize_reciprocal(x, VS) != R.quantize(x, VS)).any()
    pts = np.stack([x, x[r.permutation(len(x))], x[r.permutation(len(x))]], 1)
    _check_voxelize([pts, -pts[:5001]])
    _check_voxelize([r.uniform(-900, -100, (3000, 3)).astype(np.float32)], vs=0.05)


def test_voxelize_room_of_100k_points():
    _check_voxelize([_surface(0, 100_000)])


def test_voxelize_refuses_bad_input():
    from pq3d_amd import _lib, scene
    r = np.random.default_rng(4)
    good = r.uniform(-1, 1, (500, 3)).astype(np.float32)
    for bad in (float("nan"), float("inf"), -float("inf"), 0.02 * (1 << 19), -0.02 * ((1 << 19) + 3), 3.0e38):
        pts = good.copy()
        pts[321, 1] = bad
        with pytest.raises(ValueError, match="voxelize"):
            scene.voxelize([_dev(good), _dev(pts)], VS)
    scene.voxelize([_dev(np.full((3, 3), VS * ((1 << 19) - 9), dtype=np.float32))], VS)     # the last voxel inside the range
    with pytest.raises(ValueError):
        scene.voxelize([_dev(good)], 0.0)
    with pytest.raises(ValueError):
        scene.voxelize([_dev(good)] * 9, VS)
    with pytest.raises(_lib.Pq3dError):
        scene.voxelize([torch.from_numpy(good)], VS)


# ----------------------------------------------------------------------------------------------------------------- FPS
def _check_fps(clouds, m, start_idx=0):
    from pq3d_amd import scene
    got = scene.farthest_point_sample([_dev(c) for c in clouds], m, start_idx)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(clouds), m)
    got = got.cpu().numpy()
    for b, c in enumerate(clouds):
        want = R.fps(c, m, start_idx)
        bad = np.flatnonzero(got[b] != want)
        assert bad.size == 0, f"scene {b}: first difference at step {bad[0]}: got {got[b][bad[0]]}, want {want[bad[0]]}"
    return got


def _lattice(shape, seed, shuffle=True):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return g[np.random.default_rng(seed).permutation(len(g))] if shuffle else g


@pytest.mark.parametrize("N", [63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 1023, 1025])
def test_fps_sizes_around_wave_workgroup_and_tile(N):
    r = np.random.default_rng(N)
    _check_fps([r.uniform(-2, 2, (N, 3)).astype(np.float32)], min(N, 40))


def test_fps_degenerate_sizes():
    r = np.random.default_rng(1)
    _check_fps([r.uniform(-1, 1, (1, 3)).astype(np.float32)], 1)
    for N in (2, 65, 300):                  # m = N: every point is taken exactly once
        c = r.uniform(-1, 1, (N, 3)).astype(np.float32)
        assert sorted(_check_fps([c], N)[0].tolist()) == list(range(N))


def test_fps_lattice_ties_follow_caller_indices():
    """Integer lattices: every distance is an exact small integer, most steps are ties.  The rows are shuffled, so the internal
    (Morton) order and the caller order disagree everywhere."""
    _check_fps([_lattice((5, 5, 1), 0, shuffle=False)], 25)
    _check_fps([_lattice((5, 5, 1), 1)], 25)
    _check_fps([_lattice((17, 13, 5), 2)], 300)
    _check_fps([_lattice((40, 33, 2), 3)], 200)


def test_fps_identical_points():
    got = _check_fps([np.full((700, 3), 0.25, dtype=np.float32)], 9)
    assert got[0].tolist() == [0] * 9
    assert _check_fps([np.full((700, 3), 0.25, dtype=np.float32)], 5, start_idx=33)[0].tolist() == [33, 0, 0, 0, 0]


def test_fps_float_cloud_and_start_index():
    c = np.random.default_rng(6).standard_normal((4000, 3)).astype(np.float32)
    _check_fps([c], 150)
    _check_fps([c], 64, start_idx=3999)
    _check_fps([c[:777]], 64, start_idx=123)


def test_fps_two_far_clusters_prune_nearly_everything():
    from pq3d_amd import scene
    r = np.random.default_rng(7)
    c = np.concatenate([r.uniform(0, 1, (3000, 3)), r.uniform(0, 1, (3000, 3)) + 1000.0]).astype(np.float32)
    c = c[r.permutation(len(c))]
    _check_fps([c], 100)
    _idx, scanned, tiles = scene.farthest_point_sample([_dev(c)], 100, return_scanned=True)
    assert tiles == [(6000 + TILE - 1) // TILE] and 0 < int(scanned[0]) <= 99 * tiles[0]


def test_fps_ragged_batch_equals_single_calls():
    from pq3d_amd import scene
    r = np.random.default_rng(9)
    clouds = [r.uniform(-3, 3, (1500, 3)).astype(np.float32), _lattice((9, 9, 3), 4), r.uniform(0, 1, (64, 3)).astype(np.float32)]
    got = _check_fps(clouds, 50, start_idx=7)
    for b, c in enumerate(clouds):
        assert np.array_equal(scene.farthest_point_sample([_dev(c)], 50, 7).cpu().numpy()[0], got[b])


def test_fps_sixty_four_small_scenes():
    """The scene table's maximum, PQ3D_FPS_MAX_SCENES = 64: scenes of 1 to 70 points at m = 1, which is also the smallest
    scene; then 64 scenes of 5 to 70 points at m = 5, their smallest."""
    r = np.random.default_rng(16)
    lens = (1 + np.arange(64) * 37 % 70).tolist()
    assert len(lens) == 64 and min(lens) == 1 and max(lens) == 70
    _check_fps([r.uniform(-2, 2, (n, 3)).astype(np.float32) for n in lens], 1)
    lens = [max(n, 5) for n in lens]
    _check_fps([r.uniform(-2, 2, (n, 3)).astype(np.float32) for n in lens], 5, start_idx=4)


@functools.lru_cache(maxsize=None)
def _room_voxels():
    q = np.unique(R.quantize(_surface(1, 130_000), VS), axis=0)
    return q[np.random.default_rng(12).permutation(len(q))].astype(np.float32)


def test_fps_room_of_100k_voxels():
    v = _room_voxels()
    assert len(v) >= 100_000
    _check_fps([v], 120)


def test_fps_above_the_small_tile_limit():
    """N > 2^18 switches to 1024-row tiles (N up to 2^20 = 1024 tiles of one workgroup)."""
    r = np.random.default_rng(13)
    _check_fps([r.uniform(-5, 5, ((1 << 18) + 5, 3)).astype(np.float32)], 12)
    _check_fps([r.uniform(-5, 5, (1 << 20, 3)).astype(np.float32)], 6)


def test_fps_refuses_bad_arguments():
    from pq3d_amd import _lib, scene
    c = np.random.default_rng(0).uniform(-1, 1, (50, 3)).astype(np.float32)
    for m in (51, 0, -1):
        with pytest.raises(ValueError):
            scene.farthest_point_sample([_dev(c)], m)
    with pytest.raises(ValueError):
        scene.farthest_point_sample([_dev(c), _dev(c[:10])], 11)
    with pytest.raises(ValueError):
        scene.farthest_point_sample([_dev(c)], 5, start_idx=50)
    with pytest.raises(_lib.Pq3dError):
        scene.farthest_point_sample([torch.from_numpy(c)], 5)


# ---------------------------------------------------------------------------------------------- prepare_instseg_batch
S_MODEL = 40


def _scenes(seed=21, P=(1700, 1300)):
    """Raw scenes in a 1.2 x 1.0 x 0.12 m slab: colour | xyz features, S_MODEL segments (every id present), instances with
    unlabelled (-1) points and an instance id without points."""
    r = np.random.default_rng(seed)
    out = []
    for b, p in enumerate(P):
        xyz = (r.uniform(0, 1, (p, 3)) * [1.2, 1.0, 0.12] - [0.5, 0.4, 0.04]).astype(np.float32)
        seg = np.concatenate([np.arange(S_MODEL), r.integers(0, S_MODEL, p - S_MODEL)])[r.permutation(p)].astype(np.int64)
        inst = r.integers(-1, 6, p).astype(np.int64)
        inst[inst == 4] = 5
        ids = np.array([0, 1, 2, 3, 5, 4][:6 - b], dtype=np.int64)         # (4 has no points: a zero centre)
        out.append(dict(xyz=xyz, feat=np.concatenate([r.random((p, 3)).astype(np.float32), xyz], 1), seg=seg, inst=inst, ids=ids))
    return out


def _prepare(sc, **kw):
    from pq3d_amd import scene
    return scene.prepare_instseg_batch([_dev(s["xyz"]) for s in sc], [_dev(s["feat"]) for s in sc], [_dev(s["seg"]) for s in sc],
                                       VS, 9, point2instance=[_dev(s["inst"]) for s in sc], instance_ids=[_dev(s["ids"]) for s in sc],
                                       **kw)


def _pad(rows, width):
    out = np.zeros((len(rows), max(len(r) for r in rows), width), dtype=np.float64)
    mask = np.zeros(out.shape[:2], dtype=bool)
    for b, r in enumerate(rows):
        out[b, :len(r)], mask[b, :len(r)] = r, True
    return out, mask


def _close(got: torch.Tensor, want: np.ndarray):
    """The segment-pooling test's bound (tests/test_gpu_segment.py): 2e-6 * max(1, |reference|) against the float64 mean."""
    err = float(np.abs(got.cpu().double().numpy() - want).max())
    assert tuple(got.shape) == want.shape and err <= 2e-6 * max(1.0, float(np.abs(want).max())), err


@pytest.mark.parametrize("query_from", ["points", "voxels"])
def test_prepare_instseg_batch_every_key(query_from):
    sc = _scenes()
    out = _prepare(sc, query_from=query_from)
    vc, um, inv = R.voxelize([s["xyz"] for s in sc], VS)
    B, V = len(sc), [len(u) for u in um]
    eq = lambda t, a: t.dtype == torch.from_numpy(a).dtype and np.array_equal(t.cpu().numpy(), a)
    assert eq(out["voxel_coordinates"], vc)
    assert eq(out["voxel_features"], np.concatenate([s["feat"][u] for s, u in zip(sc, um)]))
    locs = []
    for b, s in enumerate(sc):
        assert eq(out["voxel2segment"][b], s["seg"][um[b]]) and eq(out["coordinates"][b], s["feat"][um[b]][:, -3:])
        assert eq(out["voxel_to_full_maps"][b], inv[b]) and eq(out["segment_to_full_maps"][b], s["seg"])
        assert eq(out["raw_coordinates"][b], s["xyz"])
        lattice = vc[sum(V[:b]):sum(V[:b + 1]), 1:].astype(np.float32)
        f = R.fps(lattice, 9)
        locs.append(s["xyz"][f] if query_from == "points" else s["xyz"][um[b][f]])
    assert eq(out["query_locs"], np.stack(locs)) and eq(out["query_pad_masks"], np.ones((B, 9), dtype=bool))
    assert eq(out["coord_min"], np.stack([s["xyz"].min(0) for s in sc])) and eq(out["coord_max"], np.stack([s["xyz"].max(0) for s in sc]))
    seg, seg_mask = _pad([R.centers(s["xyz"], s["seg"], int(s["seg"].max()) + 1) for s in sc], 3)
    _close(out["seg_center"], seg)
    assert eq(out["seg_pad_masks"], seg_mask)
    objs = []
    for s in sc:
        p2i = np.where(s["inst"] == -1, s["ids"].max() + 1, s["inst"])
        objs.append(R.centers(s["xyz"], p2i, int(p2i.max()) + 1)[s["ids"]])
    obj, obj_mask = _pad(objs, 3)
    assert np.all(objs[0][5] == 0.0), "an instance id without points has a zero centre"
    _close(out["obj_center"], obj)
    assert eq(out["obj_pad_masks"], obj_mask)


def test_prepare_instseg_batch_gt_queries_and_errors():
    from pq3d_amd import _lib, scene
    sc = _scenes()
    out = _prepare(sc, query_sample_strategy="gt")
    assert torch.equal(out["query_locs"], out["obj_center"]) and torch.equal(out["query_pad_masks"], out["obj_pad_masks"])
    assert tuple(out["query_locs"].shape) == (2, 6, 3) and out["obj_pad_masks"].sum(1).tolist() == [6, 5]
    dev = lambda k: [_dev(s[k]) for s in sc]
    with pytest.raises(ValueError, match="num_queries"):
        scene.prepare_instseg_batch(dev("xyz"), dev("feat"), dev("seg"), VS, 10 ** 6)
    with pytest.raises(ValueError, match="gt"):
        scene.prepare_instseg_batch(dev("xyz"), dev("feat"), dev("seg"), VS, 9, query_sample_strategy="gt")
    with pytest.raises(NotImplementedError):
        scene.prepare_instseg_batch(dev("xyz"), dev("feat"), dev("seg"), VS, 9, query_sample_strategy="random")
    with pytest.raises(_lib.Pq3dError):
        scene.prepare_instseg_batch([torch.from_numpy(s["xyz"]) for s in sc], dev("feat"), dev("seg"), VS, 9)
    import pq3d_amd
    assert pq3d_amd.prepare_instseg_batch is scene.prepare_instseg_batch and pq3d_amd.voxelize is scene.voxelize


def test_prepared_batch_drives_the_model_and_the_predictions():
    """Raw points -> prepare_instseg_batch -> Query3DUnified with its voxel backbone -> instance_predictions."""
    from pq3d_amd import synth
    from pq3d_amd.instseg import instance_predictions
    from tests.test_gpu_voxel_model import S, _model
    assert S == S_MODEL
    sc = _scenes()
    batch = _prepare(sc)
    assert tuple(batch["seg_center"].shape) == (2, S, 3) and bool(batch["seg_pad_masks"].all())
    dd = synth.synth_data_dict(2, S, 9, {"mv": 64, "voxel": 64}, seed=5, memories=["mv"], full_valid=True)
    dd = {k: v.cuda() for k, v in dd.items()}
    dd.update({k: batch[k] for k in ("voxel_coordinates", "voxel_features", "voxel2segment", "seg_center", "seg_pad_masks", "query_locs",
                                     "query_pad_masks", "coord_min", "coord_max")})
    with torch.no_grad():
        out = _model(True)(dd)
    logits, masks = out["predictions_class"][-1], out["predictions_mask"][-1]
    assert tuple(masks.shape) == (2, S, 9) and tuple(logits.shape) == (2, 9, 21)
    assert not bool(torch.isnan(logits).any()) and not bool(torch.isnan(masks).any())     # (-inf: the model's filled class columns)
    preds = instance_predictions(logits, masks, batch["voxel2segment"], batch["voxel_to_full_maps"], batch["segment_to_full_maps"],
                                 batch["raw_coordinates"], topk_per_scene=20)
    for b, p in enumerate(preds):
        assert tuple(p["masks"].shape) == (len(sc[b]["xyz"]), 20) and bool(torch.isfinite(p["scores"]).all())
