"""Plain numpy restatement of the train-time augmentation of instance-segmentation scenes (pq3d_amd/scene.py augment_scenes,
csrc/scene_augment.hip): the specification the GPU kernels are tested against, bit for bit.  Every arithmetic step
is ONE fp32 operation in the order written (numpy rounds every operation on float32 arrays on its own; nothing is fused); the
only fp64 is the sum behind the mean.  (volumentations and albumentations, which the reference's get_scene calls, are not
available, so the expected values cannot come from them.)

A parameter set is a dict: u [3], flip [2], scale [3], rot [3, 3, 3], alpha, beta255, shift [3] and the stage flags on_centre,
on_offset, on_flip, on_scale, on_rotate, on_colour; ``unpack`` builds it from a row of ``draw_scene_augment``."""
import numpy as np

F32 = np.float32
COLOR_MEAN = (0.47793125906962, 0.4303257521323044, 0.3749598901421883)
COLOR_STD = (0.2834475483823543, 0.27566157565723015, 0.27018971370874995)
STAGES = ("centre", "offset", "flip", "scale", "rotate", "colour")


def unpack(row) -> dict:
    """A [K] fp32 row of pq3d_scene_augment_params as the dict the functions below take."""
    from pq3d_amd.scene import AUG_FIELDS
    row = np.asarray(row, dtype=F32)
    p = {n: row[at:at + k].copy() for n, (at, k) in AUG_FIELDS.items() if n != "reserved"}
    p["rot"] = p["rot"].reshape(3, 3, 3)
    for n in list(p):
        if p[n].shape == (1,):
            p[n] = p[n][0]
    return p


def params(**kw) -> dict:
    """A parameter set with every stage off and neutral values, updated by ``kw`` (for hand-written cases)."""
    p = dict(u=np.zeros(3, F32), flip=np.zeros(2, F32), scale=np.ones(3, F32), rot=np.stack([np.eye(3, dtype=F32)] * 3),
             alpha=F32(1), beta255=F32(0), shift=np.zeros(3, F32), **{"on_" + s: F32(0) for s in STAGES})
    for k, v in kw.items():
        assert k in p, k
        p[k] = np.asarray(v, dtype=F32).reshape(np.shape(p[k]))
    return p


def color_constants(color_mean=COLOR_MEAN, color_std=COLOR_STD):
    """mean255 = fp32(mean * 255), rstd255 = fp32(1) / fp32(std * 255): computed once on the host."""
    mean = np.asarray(color_mean, dtype=np.float64)
    std = np.asarray(color_std, dtype=np.float64)
    return (mean * 255.0).astype(F32), F32(1) / (std * 255.0).astype(F32)


def stats(x):
    """fp64 sums, fp32 minima and maxima of the three axes."""
    x = np.asarray(x, dtype=F32)
    return x.astype(np.float64).sum(0), x.min(0), x.max(0)


def constants(x, p) -> dict:
    """mean, off and cmax [3] fp32 from ONE pass over the raw points (fp32 rounding is monotone, so mn - mean and mx - mean
    are the exact minimum and maximum of the centred points, and (mx - mean) + off the exact maximum of the shifted ones).
    A stage that is off leaves its term out."""
    x = np.asarray(x, dtype=F32)
    s, mn, mx = stats(x)
    mean = (s / np.float64(len(x))).astype(F32)
    lo, hi = (mn - mean, mx - mean) if p["on_centre"] else (mn, mx)
    off = ((hi - lo) * p["u"] + lo) * F32(0.5)
    cmax = hi + off if p["on_offset"] else hi
    for v in (mean, lo, hi, off, cmax):
        assert v.dtype == F32
    return dict(mean=mean, off=off, cmax=cmax)


def clip(v):
    return np.where(v < 0, F32(0), np.where(v > 255, F32(255), v)).astype(F32)


def to_uint8(c):
    """trunc(c) saturated to [0, 255], NaN -> 0; and whether any value had to be saturated (error bit 2)."""
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.asarray(c, dtype=F32))
        ok = (t >= 0) & (t <= 255)
        return np.where(ok, t, np.where(t > 255, F32(255), F32(0))).astype(F32), bool((~ok).any())


def apply(x, c, p, k, cc):
    """The point-wise part for points x, c [n, 3] of one scene: p the parameter set or None (evaluation), k = constants(...)
    of the WHOLE scene, cc = color_constants(...).  Returns (coordinates_out [n, 3], features_out [n, 6], error bits)."""
    x = np.array(x, dtype=F32)
    err = 0 if np.isfinite(x).all() else 1
    if p is not None:
        if p["on_centre"]:
            x = x - k["mean"]
        if p["on_offset"]:
            x = x + k["off"]
        if p["on_flip"]:
            for a in (0, 1):
                if p["flip"][a]:
                    x[:, a] = k["cmax"][a] - x[:, a]
        if p["on_scale"]:
            x = x * p["scale"]
        if p["on_rotate"]:
            for R in p["rot"]:
                x = np.stack([(R[i, 0] * x[:, 0] + R[i, 1] * x[:, 1]) + R[i, 2] * x[:, 2] for i in range(3)], 1)
    c, bad = to_uint8(c)
    err |= 2 if bad else 0
    if p is not None and p["on_colour"]:
        v = c * p["alpha"]
        v = v + p["beta255"]
        c = np.trunc(clip(v))
        c = np.trunc(clip(c + p["shift"]))
    f = (c - cc[0]) * cc[1]
    assert x.dtype == F32 and f.dtype == F32
    return x, np.concatenate([f, x], 1), err


def augment(x, c, p, color_mean=COLOR_MEAN, color_std=COLOR_STD):
    """One scene: x, c [P, 3]; p a parameter set (train) or None (evaluation)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return apply(x, c, p, constants(x, p) if p is not None else None, color_constants(color_mean, color_std))


def grid_points(rng, n, span=64.0):
    """n points whose coordinates are multiples of 2^-10 with |x| < span <= 64: at most 17 significant bits each, so every
    fp64 sum of up to 2^24 of them is exact in ANY order and the restatement alone fixes the bits of the mean."""
    q = rng.integers(-int(span * 1024) + 1, int(span * 1024), (n, 3))
    return (q / 1024.0).astype(F32)
