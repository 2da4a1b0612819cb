"""CPU: the numpy restatement of the train-time scene augmentation (tests/scene_augment_ref.py) pinned by hand-written cases,
and the host side of pq3d_amd.scene that carries the library conventions: SceneAugmentConfig, its reader of the two
serialised Compose files, and draw_scene_augment."""
import ctypes
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

from pq3d_amd import scene
from tests import scene_augment_ref as R

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instseg_aug")
VOLUME, IMAGE = os.path.join(GOLDEN, "volumentations_aug.yaml"), os.path.join(GOLDEN, "albumentations_aug.yaml")
# three points whose sums, means and products below are exact in fp32
X3 = np.array([[1.0, 2.0, -3.0], [3.0, -2.0, 5.0], [5.0, 6.0, 1.0]], dtype=F32)      # mean (3, 2, 1), min (1, -2, -3), max (5, 6, 5)
C3 = np.array([[0.0, 255.0, 254.9], [10.5, 100.0, 200.0], [17.0, 128.0, 64.0]], dtype=F32)
MEAN255, RSTD255 = R.color_constants()


def _normalized(c_int):
    return (np.asarray(c_int, dtype=F32) - MEAN255) * RSTD255


# ------------------------------------------------------------------------------------------------- each stage alone
def test_evaluation_path_keeps_coordinates_and_normalizes_colour():
    x, f, err = R.augment(X3, C3, None)
    assert err == 0 and x.tobytes() == X3.tobytes()
    assert np.array_equal(f[:, 3:], X3)
    assert np.array_equal(f[:, :3], _normalized([[0, 255, 254], [10, 100, 200], [17, 128, 64]]))
    # the constants: fp32(mean * 255) and the fp32 reciprocal of fp32(std * 255)
    assert MEAN255.dtype == F32 and RSTD255.dtype == F32
    assert MEAN255[0] == F32(0.47793125906962 * 255) and RSTD255[2] == F32(1) / F32(0.27018971370874995 * 255)
    # all stages off in training = the evaluation path
    x2, f2, _ = R.augment(X3, C3, R.params())
    assert x2.tobytes() == X3.tobytes() and f2.tobytes() == f.tobytes()


def test_centre_alone():
    x, f, _ = R.augment(X3, C3, R.params(on_centre=1))
    assert np.array_equal(x, [[-2, 0, -4], [0, -4, 4], [2, 4, 0]]) and np.array_equal(f[:, 3:], x)


def test_offset_alone_and_after_centre():
    # offset alone: lo = min, hi = max of the raw points; off = ((hi - lo) * u + lo) * 0.5
    u = [0.5, 0.25, 0.0]
    x, _, _ = R.augment(X3, C3, R.params(on_offset=1, u=u))
    off = np.array([(4 * 0.5 + 1) * 0.5, (8 * 0.25 - 2) * 0.5, (8 * 0.0 - 3) * 0.5], dtype=F32)       # (1.5, 0, -1.5)
    assert np.array_equal(x, X3 + off)
    # after the centre stage: lo = (-2, -4, -4), hi = (2, 4, 4)
    x, _, _ = R.augment(X3, C3, R.params(on_centre=1, on_offset=1, u=u))
    off = np.array([(4 * 0.5 - 2) * 0.5, (8 * 0.25 - 4) * 0.5, (8 * 0.0 - 4) * 0.5], dtype=F32)       # (0, -1, -2)
    assert np.array_equal(x, (X3 - np.array([3, 2, 1], dtype=F32)) + off)


def test_flip_alone_and_with_the_earlier_stages():
    x, _, _ = R.augment(X3, C3, R.params(on_flip=1, flip=[1, 0]))
    assert np.array_equal(x, [[4, 2, -3], [2, -2, 5], [0, 6, 1]])                   # 5 - x on axis 0 only
    x, _, _ = R.augment(X3, C3, R.params(on_flip=1, flip=[1, 1]))
    assert np.array_equal(x, [[4, 4, -3], [2, 8, 5], [0, 0, 1]])                    # the z axis never flips
    x, _, _ = R.augment(X3, C3, R.params(on_flip=0, flip=[1, 1]))
    assert np.array_equal(x, X3)                                                    # the stage flag gates the draw
    # centre + offset + flip: cmax = (max - mean) + off = (2, 4) + (0, -1) = (2, 3); x2 = centred + (0, -1, -2)
    x, _, _ = R.augment(X3, C3, R.params(on_centre=1, on_offset=1, on_flip=1, flip=[1, 1], u=[0.5, 0.25, 0.0]))
    assert np.array_equal(x, [[4, 4, -6], [2, 8, 2], [0, 0, -2]])


def test_scale_alone():
    x, _, _ = R.augment(X3, C3, R.params(on_scale=1, scale=[1.5, 0.5, 2.0]))
    assert np.array_equal(x, X3 * np.array([1.5, 0.5, 2.0], dtype=F32))
    assert np.array_equal(x[0], [1.5, 1.0, -6.0])


def test_rotate_alone_applies_three_matrices_in_turn():
    Rz = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]          # +90 degrees about z: (1, 0, 0) -> (0, 1, 0)
    Rx = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]          # +90 degrees about x: (0, 1, 0) -> (0, 0, 1)
    I = np.eye(3)
    x, _, _ = R.augment(X3, C3, R.params(on_rotate=1, rot=[Rz, I, I]))
    assert np.array_equal(x, [[-2, 1, -3], [2, 3, 5], [-6, 5, 1]])
    x, _, _ = R.augment(X3, C3, R.params(on_rotate=1, rot=[Rz, I, Rx]))            # Rx (Rz x), not Rz (Rx x)
    assert np.array_equal(x, [[-2, 3, 1], [2, -5, 3], [-6, -1, 5]])
    # y_i = (R_i0 * x_0 + R_i1 * x_1) + R_i2 * x_2 with every operation rounded on its own
    M = np.array([[0.1, 0.2, 0.3], [0.7, -0.3, 0.9], [1e-3, 3.0, -0.7]], dtype=F32)
    x, _, _ = R.augment(X3, C3, R.params(on_rotate=1, rot=[M, I, I]))
    for p in range(3):
        for i in range(3):
            assert x[p, i] == F32(F32(F32(M[i, 0] * X3[p, 0]) + F32(M[i, 1] * X3[p, 1])) + F32(M[i, 2] * X3[p, 2]))


def test_colour_alone_truncates_and_clips():
    # brightness / contrast: trunc(clip(c0 * alpha + beta255)); c0 = (0, 255, 254 | 10, 100, 200 | 17, 128, 64)
    _, f, err = R.augment(X3, C3, R.params(on_colour=1, alpha=1.5, beta255=-20.0))
    assert err == 0
    assert np.array_equal(f[:, :3], _normalized([[0, 255, 255], [0, 130, 255], [5, 172, 76]]))     # 25.5 - 20 = 5.5 -> 5
    # the shift: trunc(clip(c1 + shift)), per channel
    _, f, _ = R.augment(X3, C3, R.params(on_colour=1, shift=[-10.5, 0.75, 1.0]))
    assert np.array_equal(f[:, :3], _normalized([[0, 255, 255], [0, 100, 201], [6, 128, 65]]))     # 10 - 10.5 -> clip 0; 17 - 10.5 = 6.5 -> 6
    # the clip edges: v just inside and just outside [0, 255]
    c = np.array([[1.0, 1.0, 1.0]], dtype=F32)
    for beta, want in ((-1.0, 0), (-1.5, 0), (254.0, 255), (254.5, 255), (253.99, 254), (-0.5, 0)):
        _, f, _ = R.augment(X3[:1], c, R.params(on_colour=1, beta255=beta))
        assert np.array_equal(f[:, :3], _normalized([[want] * 3])), beta
    # both steps truncate: 100 * 1.004 = 100.4 -> 100, + 0.7 -> 100.7 -> 100 (one truncation at the end would give 101)
    _, f, _ = R.augment(X3[:1], np.full((1, 3), 100.0, dtype=F32), R.params(on_colour=1, alpha=1.004, shift=[0.7] * 3))
    assert np.array_equal(f[:, :3], _normalized([[100] * 3]))


def test_uint8_conversion_saturates_and_reports():
    cases = [(0.0, 0, 0), (255.0, 255, 0), (254.9, 254, 0), (255.9, 255, 0), (-0.9, 0, 0), (-1.0, 0, 2), (256.0, 255, 2),
             (float("nan"), 0, 2), (float("inf"), 255, 2), (-float("inf"), 0, 2), (1e9, 255, 2)]
    for value, want, bit in cases:
        c = np.array([[value, 7.0, 7.0]], dtype=F32)
        for p in (None, R.params()):
            _, f, err = R.augment(X3[:1], c, p)
            assert err == bit and np.array_equal(f[:, :3], _normalized([[want, 7, 7]])), value
    x = X3.copy()
    x[1, 2] = np.inf
    assert R.augment(x, C3, None)[2] == 1 and R.augment(x, C3, R.params(on_centre=1))[2] == 1


# ------------------------------------------------------------------------------- the one-pass shortcut and the fp64 sum
@pytest.mark.parametrize("seed", range(4))
def test_one_pass_constants_equal_brute_force_extrema(seed):
    """lo, hi and cmax come from the raw minimum / maximum; they must be the extrema of the transformed points exactly."""
    r = np.random.default_rng(seed)
    x = (r.normal(0, 3, (5000, 3)) + r.uniform(-50, 50, 3)).astype(F32)
    u = r.random(3, dtype=F32)
    p = R.params(on_centre=1, on_offset=1, on_flip=1, flip=[1, 1], u=u)
    k = R.constants(x, p)
    x1 = x - k["mean"]
    lo, hi = x1.min(0), x1.max(0)
    assert np.array_equal(k["off"], ((hi - lo) * u + lo) * F32(0.5))
    x2 = x1 + k["off"]
    assert np.array_equal(k["cmax"], x2.max(0))
    got, _, _ = R.augment(x, np.zeros_like(x), p)
    want = x2.copy()
    want[:, :2] = x2.max(0)[:2] - x2[:, :2]
    assert np.array_equal(got, want)
    # with the centre stage off the pivot is formed from the raw extrema, with the offset stage off without the offset
    p = R.params(on_offset=1, on_flip=1, flip=[1, 1], u=u)
    k = R.constants(x, p)
    off = ((x.max(0) - x.min(0)) * u + x.min(0)) * F32(0.5)
    assert np.array_equal(k["off"], off) and np.array_equal(k["cmax"], (x + off).max(0))
    k = R.constants(x, R.params(on_centre=1, on_flip=1, flip=[1, 1]))
    assert np.array_equal(k["cmax"], x1.max(0))


def test_grid_sums_are_exact_in_any_order():
    """The GPU tests' coordinates (multiples of 2^-10, |x| < 64): the fp64 sum does not depend on the order, so the mean's
    bits are fixed by the restatement alone."""
    r = np.random.default_rng(5)
    x = R.grid_points(r, 100_000)
    assert np.abs(x).max() < 64 and np.array_equal(x * 1024, np.round(x * 1024))
    s = R.stats(x)[0]
    for a in range(3):
        col = x[:, a].astype(np.float64)
        assert s[a] == math.fsum(col) == float(np.sum(col[::-1])) == float(np.sum(np.sort(col))) == sum(col[r.permutation(len(col))].tolist())
        assert float(s[a]) * 1024 == round(float(s[a]) * 1024)


# ------------------------------------------------------------------------------------------------- draw_scene_augment
def _fields(rows):
    rows = rows.numpy()
    return {n: rows[:, at:at + k] for n, (at, k) in scene.AUG_FIELDS.items()}


def test_draw_fields_lie_inside_their_ranges():
    cfg = scene.SceneAugmentConfig()
    rows = scene.draw_scene_augment(1000, cfg, np.random.default_rng(0))
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (1000, scene.AUG_K) and not rows.is_cuda
    f = _fields(rows)
    inside = lambda v, lo, hi: bool(((v >= F32(lo)) & (v <= F32(hi))).all())          # (the bounds rounded to fp32 as the fields are)
    assert inside(f["u"], 0, 1) and bool((f["u"] < 1).all())
    assert set(np.unique(f["flip"]).tolist()) == {0.0, 1.0} and 0.4 < f["flip"].mean() < 0.6
    assert inside(f["scale"], 0.9, 1.1) and f["scale"].std() > 0.03
    assert inside(f["alpha"], 0.8, 1.2) and inside(f["beta255"], -0.2 * 255, 0.2 * 255) and inside(f["shift"], -20, 20)
    assert f["beta255"].min() < -40 and f["beta255"].max() > 40 and f["shift"].min() < -18 and f["shift"].max() > 18
    for s in scene.AUG_STAGES:
        assert bool((f["on_" + s] == 1).all())
    assert bool((f["reserved"] == 0).all())
    rot = f["rot"].reshape(1000, 3, 3, 3).astype(np.float64)
    eye = np.eye(3)
    assert np.abs(rot @ rot.transpose(0, 1, 3, 2) - eye).max() < 1e-6 and np.allclose(np.linalg.det(rot), 1, atol=1e-6)
    # the configured axes and angle limits: rotation j keeps its axis, its angle lies inside the limit
    for j, (axis, (lo, hi)) in enumerate(cfg.rotations):
        assert np.abs(rot[:, j] @ np.array(axis) - np.array(axis)).max() < 1e-6
        angle = np.arccos(np.clip((np.trace(rot[:, j], axis1=1, axis2=2) - 1) / 2, -1, 1))
        assert angle.max() <= hi + 1e-3 and (j == 0 or angle.max() > 0.9 * hi)
    assert np.arccos(np.clip((np.trace(rot[:, 0], axis1=1, axis2=2) - 1) / 2, -1, 1)).max() > 3.0
    # a subset of stages sets only those flags
    f = _fields(scene.draw_scene_augment(3, cfg, np.random.default_rng(1), stages=("scale", "colour")))
    assert [float(f["on_" + s][0, 0]) for s in scene.AUG_STAGES] == [0, 0, 0, 1, 0, 1]
    with pytest.raises(ValueError):
        scene.draw_scene_augment(1, cfg, np.random.default_rng(1), stages=("elastic",))


def test_draw_rotation_sense_and_seed():
    quarter = dataclasses.replace(scene.SceneAugmentConfig(), rotations=(((0.0, 0.0, 1.0), (math.pi / 2, math.pi / 2)),
                                                                           ((0.0, 1.0, 0.0), (0.0, 0.0)), ((1.0, 0.0, 0.0), (0.0, 0.0))))
    p = R.unpack(scene.draw_scene_augment(1, quarter, np.random.default_rng(3))[0].numpy())
    assert np.abs(p["rot"][0] @ np.array([1, 0, 0]) - np.array([0, 1, 0])).max() < 1e-7      # right-handed, applied as R x
    assert np.array_equal(p["rot"][1], np.eye(3)) and np.array_equal(p["rot"][2], np.eye(3))
    assert np.abs(scene._rotation((0, 1, 0), math.pi / 2) @ np.array([0, 0, 1]) - np.array([1, 0, 0])).max() < 1e-15
    assert np.abs(scene._rotation((2, 0, 0), math.pi / 2) @ np.array([0, 1, 0]) - np.array([0, 0, 1])).max() < 1e-15
    a = scene.draw_scene_augment(4, scene.SceneAugmentConfig(), np.random.default_rng(11))
    b = scene.draw_scene_augment(4, scene.SceneAugmentConfig(), np.random.default_rng(11))
    c = scene.draw_scene_augment(4, scene.SceneAugmentConfig(), np.random.default_rng(12))
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_row_layout_is_the_bound_struct():
    from pq3d_amd import _lib
    assert scene.AUG_K == 48 and scene.AUG_K * 4 == ctypes.sizeof(_lib.SceneAugmentParams)
    spans = sorted(scene.AUG_FIELDS.values())
    assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])) and sum(spans[-1]) == scene.AUG_K
    p = R.unpack(np.arange(48, dtype=F32))
    assert p["rot"].shape == (3, 3, 3) and p["rot"][1, 0, 0] == 8 + 9 and p["alpha"] == 35 and p["on_colour"] == 45


# ---------------------------------------------------------------------------------------------- SceneAugmentConfig.from_files
def test_from_files_gives_the_defaults_on_the_shipped_files():
    assert scene.SceneAugmentConfig.from_files(VOLUME, IMAGE) == scene.SceneAugmentConfig()


def test_from_files_refuses_what_it_does_not_implement(tmp_path):
    text = open(VOLUME).read()
    bad = tmp_path / "volume.yaml"
    bad.write_text(text.replace("transforms.Scale3d", "transforms.ElasticTransform3d"))
    with pytest.raises(NotImplementedError, match="volumentations.augmentations.transforms.ElasticTransform3d"):
        scene.SceneAugmentConfig.from_files(str(bad), IMAGE)
    bad.write_text(text.replace("always_apply: true", "always_apply: false", 1))
    with pytest.raises(NotImplementedError, match="always_apply"):
        scene.SceneAugmentConfig.from_files(str(bad), IMAGE)
    img = tmp_path / "image.yaml"
    img.write_text(open(IMAGE).read().replace("transforms.RGBShift", "transforms.HueSaturationValue"))
    with pytest.raises(NotImplementedError, match="HueSaturationValue"):
        scene.SceneAugmentConfig.from_files(VOLUME, str(img))
    img.write_text(open(IMAGE).read().replace("brightness_by_max: true", "brightness_by_max: false"))
    with pytest.raises(NotImplementedError, match="brightness_by_max"):
        scene.SceneAugmentConfig.from_files(VOLUME, str(img))
