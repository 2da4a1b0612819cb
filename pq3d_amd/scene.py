"""Instance-segmentation scenes prepared on the GPU (csrc/scene_prep.hip): from raw points to the batch that
``Query3DUnified`` (stage 1), ``instance_predictions`` and ``InstSegAP`` read.

The reference does this on the host, one scene at a time, with MinkowskiEngine, torch_scatter and fpsample
(data/datasets/sceneverse_instseg.py get_scene / sample_query, data/datasets/instseg_wrapper.py collate_fn):

    voxel_coordinates = np.floor(coordinates / voxel_size)
    _, unique_map, inverse_map = ME.utils.sparse_quantize(voxel_coordinates, return_index=True, return_inverse=True)
    fps_idx = fpsample.bucket_fps_kdline_sampling(voxel_coordinates[unique_map], num_queries, h=3)
    query_locs = coordinates[fps_idx]
    ME.utils.sparse_collate(...), pad_sequence(...)

Rules (the restatement in tests/scene_prep_ref.py is the specification):
  voxelize   q = floor(x / fp32(voxel_size)), correctly rounded fp32 division; a voxel's representative is its lowest point
             index, a scene's voxels are ordered by ascending representative; ``inverse_map`` is local to the scene.
             MinkowskiEngine 0.5's own representative and order are not pinned by execution (the library is not
             available); nothing downstream depends on them (``CoordPyramid`` re-sorts).
  FPS        exact: dist = +inf, first sample ``start_idx``, d = (dx*dx + dy*dy) + dz*dz in fp32, dist = min(dist, d), next
             = arg-max, ties to the smallest caller index.  fpsample's start index and tie order are not pinned either.
One device-to-host read per ``voxelize`` (the voxel counts and the error word); ``farthest_point_sample`` has none.

``augment_scenes`` (csrc/scene_augment.hip) is get_scene's step before all this: the train-time augmentation of the
points and colours, the colour normalisation and ``features = colour | xyz``, by the rule restated in
tests/scene_augment_ref.py; its random parameters are drawn on the host by ``draw_scene_augment``."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import collate, ops

MAX_SCENES = L.H.PQ3D_VOXELIZE_MAX_SCENES            # (the packed key of sparse._pack has 3 scene bits)
MAX_POINTS, BLOCK = L.H.PQ3D_VOXELIZE_MAX_POINTS, L.H.PQ3D_VOXELIZE_BLOCK
FPS_MAX_SCENES, FPS_MAX_POINTS = L.H.PQ3D_FPS_MAX_SCENES, L.H.PQ3D_FPS_MAX_POINTS
_ERRORS = {1: "coordinates hold non-finite values",
           2: "floor(coordinates / voxel_size) leaves [-2^19 + 8, 2^19 - 8)",
           4: "voxel hash table overflow"}
INSTANCE_MAX_SCENES, INSTANCE_MAX_IDS = L.H.PQ3D_INSTANCE_MAX_SCENES, L.H.PQ3D_INSTANCE_MAX_IDS
INSTANCE_MAX_FILTER, INSTANCE_MAX_SEGMENTS = L.H.PQ3D_INSTANCE_MAX_FILTER, L.H.PQ3D_INSTANCE_MAX_SEGMENTS
_INSTANCE_ERRORS = {1: f"point2instance holds values outside [-1, {INSTANCE_MAX_IDS})",
                    2: "point2segment holds negative values or values beyond the segment limit (Ns in the padded form)",
                    4: "a scene has more kept instances than max_instances"}


def _need_device(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise L.Pq3dError("pq3d_amd kernels need device tensors (no CPU fallback)")


def _ragged(lists: Sequence[Sequence[torch.Tensor]], what: str, dtype, tail: tuple, text: str, max_points=None):
    """Per-scene lists whose scene b holds non-empty [N_b, *tail] device tensors (the same N_b in every list): the
    concatenation of each list, then the one host offsets array and the lengths."""
    for ts in lists:
        for t, t0 in zip(ts, lists[0]):
            _need_device(t)
            shape = (t0.shape[0] if t0.dim() else 0, *tail)
            if t.dtype != dtype or tuple(t.shape) != shape or shape[0] < 1 or t.device != lists[0][0].device:
                raise ValueError(f"{what}: {text}")
    lens = [int(t.shape[0]) for t in lists[0]]
    if max_points is not None and sum(lens) > max_points:
        raise ValueError(f"{what}: at most {max_points} points per call, got {sum(lens)}")
    off = (C.c_int64 * (len(lens) + 1))(0, *np.cumsum(lens).tolist())
    return (*((ts[0] if len(ts) == 1 else torch.cat(list(ts), 0)).contiguous() for ts in lists), off, lens)


def _scenes(ts: Sequence[torch.Tensor], what: str, max_scenes: int, max_points=None) -> Tuple[torch.Tensor, C.Array, List[int]]:
    """Concatenated fp32 [N, 3] device tensor, the host offsets array and the per-scene lengths."""
    if len(ts) < 1 or len(ts) > max_scenes:
        raise ValueError(f"{what}: between 1 and {max_scenes} scenes, got {len(ts)}")
    return _ragged([ts], what, torch.float32, (3,), "every scene is a non-empty [N, 3] fp32 tensor on one device", max_points)


def voxelize(coordinates: Sequence[torch.Tensor], voxel_size: float):
    """``coordinates``: per-scene [P_b, 3] fp32 device tensors (at most 8 scenes).  Returns ``voxel_coordinates`` [V, 1+3]
    int32 (scene, qx, qy, qz; scene after scene: sparse_collate's layout), ``unique_map`` (per scene [V_b] int64: the
    representative point of every voxel) and ``inverse_map`` (per scene [P_b] int64: the voxel of every point, local to the
    scene: ``voxel_to_full_maps``).  Non-finite or out-of-range coordinates raise ValueError."""
    pts, off, lens = _scenes(coordinates, "voxelize", MAX_SCENES, MAX_POINTS)
    vs = float(np.float32(voxel_size))
    if not (np.isfinite(vs) and vs > 0.0):
        raise ValueError(f"voxel_size must be a finite number > 0, got {voxel_size}")
    B, P, dev = len(lens), sum(lens), pts.device
    cap = 1 << max(1, (2 * P - 1).bit_length())
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    i32 = torch.empty(cap + 2 * P + (P + BLOCK - 1) // BLOCK, dtype=torch.int32, device=dev)
    rep, slot, pv, bsum = i32[:cap], i32[cap:cap + P], i32[cap + P:cap + 2 * P], i32[cap + 2 * P:]
    unique_map = torch.empty(P, dtype=torch.int64, device=dev)
    inverse_map = torch.empty(P, dtype=torch.int64, device=dev)
    vcoord = torch.empty(P, 4, dtype=torch.int32, device=dev)
    meta = torch.empty(B + 2, dtype=torch.int64, device=dev)
    L.call("pq3d_voxelize", pts, C.cast(off, C.c_void_p), B, vs, cap, keys, rep, slot, pv, bsum, unique_map, inverse_map, vcoord, meta)
    m = meta.tolist()                                             # (host sync: outside any graph)
    L.raise_error_word("voxelize", m[B + 1], _ERRORS)
    vofs = m[:B + 1]
    return (vcoord[:vofs[B]], [unique_map[vofs[b]:vofs[b + 1]] for b in range(B)],
            list(torch.split(inverse_map, lens)))


def farthest_point_sample(points: Sequence[torch.Tensor], m: int, start_idx: int = 0, *, return_scanned: bool = False):
    """Exact farthest point sampling of ``m`` of the points of every scene (per-scene [N_b, 3] fp32 device tensors with finite
    values, N_b up to 2^20): [B, m] int64 rows of each scene, the first one ``start_idx``; ties go to the smallest row.
    ``return_scanned``: also the per-scene count [B] int64 of tiles the pruning re-scanned over the m - 1 steps and the
    number of tiles per scene (a list).  No host synchronisation."""
    pts, off, lens = _scenes(points, "farthest_point_sample", FPS_MAX_SCENES)
    m, start_idx = int(m), int(start_idx)
    if m < 1 or m > min(lens):
        raise ValueError(f"farthest_point_sample: need 1 <= m <= the smallest scene ({min(lens)} points), got m = {m}")
    if max(lens) > FPS_MAX_POINTS:
        raise ValueError(f"farthest_point_sample: at most {FPS_MAX_POINTS} points per scene, got {max(lens)}")
    if not 0 <= start_idx < min(lens):
        raise ValueError(f"farthest_point_sample: start_idx {start_idx} outside the smallest scene ({min(lens)} points)")
    B, N, dev = len(lens), sum(lens), pts.device
    offp = C.cast(off, C.c_void_p)
    rows = int(L.lib().pq3d_fps_scene_rows(offp, B))
    L.check(0 if rows >= 0 else -1, "pq3d_fps_scene_rows")
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    f32 = torch.empty(B * 6 + rows * 4 + rows // 256 * 6 + 4, dtype=torch.float32, device=dev)
    ws_at = (B * 6 + 3) // 4 * 4                                   # 16-byte rows
    bbox, ws, tilebox = f32[:B * 6], f32[ws_at:ws_at + rows * 4], f32[ws_at + rows * 4:]
    L.call("pq3d_fps_scene_keys", pts, offp, B, bbox, keys)
    perm = torch.sort(keys, stable=True).indices
    cidx = torch.empty(rows, dtype=torch.int32, device=dev)
    idx = torch.empty(B, m, dtype=torch.int32, device=dev)
    scanned = torch.zeros(B, dtype=torch.int64, device=dev) if return_scanned else None
    L.call("pq3d_fps_scene", pts, offp, B, perm, m, start_idx, ws, rows, cidx, tilebox, idx, scanned)
    if return_scanned:
        T = 256 if max(lens) <= 1 << 18 else 1024
        return idx.long(), scanned, [(n + T - 1) // T for n in lens]
    return idx.long()


def _centers(coordinates: Sequence[torch.Tensor], ids: Sequence[torch.Tensor], sizes: Sequence[int]) -> List[torch.Tensor]:
    """torch_scatter.scatter_mean(coordinates[b], ids[b], dim=0) per scene with dim_size = sizes[b], as ONE segment reduction of
    the batch (ids offset by b * max size); an id no point carries gives a zero row."""
    S = max(sizes)
    flat = torch.cat([i + b * S for b, i in enumerate(ids)])
    table = ops.scatter_mean(torch.cat(list(coordinates), 0).contiguous(), flat, len(ids) * S)
    return [table[b * S:b * S + sizes[b]] for b in range(len(ids))]


# ------------------------------------------------------------------------------------------ training targets
def _id_scenes(p2i, sem, seg, what: str):
    """The three per-point id arrays of a batch, concatenated: int64 [P] device tensors, the host offsets array, the lengths."""
    B = len(p2i)
    if B < 1 or B > INSTANCE_MAX_SCENES or len(sem) != B or len(seg) != B:
        raise ValueError(f"{what}: between 1 and {INSTANCE_MAX_SCENES} scenes, one point2instance / point2semantic / point2segment each")
    return _ragged([p2i, sem, seg], what, torch.int64, (), "every scene has three non-empty [P_b] int64 tensors on one device", MAX_POINTS)


def _filter(filter_out_classes) -> Tuple[C.c_void_p, int]:
    """The host array of the filtered classes (as the pointer the entry point takes) and its length."""
    f = [int(c) for c in filter_out_classes]
    if len(f) > INSTANCE_MAX_FILTER:
        raise ValueError(f"at most {INSTANCE_MAX_FILTER} filter_out_classes, got {len(f)}")
    return C.cast((C.c_int64 * max(len(f), 1))(*f), C.c_void_p), len(f)


class _InstanceTables:
    """First half of ``instance_targets`` (the kernels before the host read): the id tables of a batch and ``meta`` [2 B + 1]
    int32 = kept instances per scene, segments per scene, the error word.  ``masks(meta as a list)`` is the second half."""

    def __init__(self, point2instance, point2semantic, point2segment, filter_out_classes):
        self.p2i, sem, self.seg, self.off, self.lens = _id_scenes(point2instance, point2semantic, point2segment, "instance_targets")
        B, dev = len(self.lens), self.p2i.device
        flt, n_flt = _filter(filter_out_classes)
        ws = torch.empty(2, B, INSTANCE_MAX_IDS + 1, dtype=torch.int32, device=dev)
        self.rank = ws[1]
        self.table = torch.empty(2, B, INSTANCE_MAX_IDS, dtype=torch.int64, device=dev)          # instance ids | labels
        self.meta = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
        L.call("pq3d_instance_tables", self.p2i, sem, self.seg, C.cast(self.off, C.c_void_p), B, flt, n_flt, INSTANCE_MAX_SEGMENTS,
               INSTANCE_MAX_IDS, ws[0], self.rank, self.table[0], self.table[1],
               self.meta[:B], self.meta[B:2 * B], self.meta[2 * B:])

    def last_ids(self) -> torch.Tensor:
        """[B] int64: the largest kept instance id of every scene, -1 for a scene without instances (no host read)."""
        n = self.meta[:len(self.lens)].long()
        return torch.where(n > 0, self.table[0].gather(1, (n - 1).clamp(min=0)[:, None])[:, 0], -1)

    def masks(self, meta: Sequence[int], with_full_masks: bool) -> Dict[str, list]:
        B, dev = len(self.lens), self.p2i.device
        L.raise_error_word("instance_targets", meta[2 * B], _INSTANCE_ERRORS)
        G, S = meta[:B], meta[B:2 * B]
        seg_masks = torch.zeros(sum(g * s for g, s in zip(G, S)), dtype=torch.uint8, device=dev)
        full = torch.empty(sum(g * p for g, p in zip(G, self.lens)) if with_full_masks else 0, dtype=torch.uint8, device=dev)
        prank = torch.empty(sum((p + 15) // 16 * 16 for p in self.lens), dtype=torch.int16, device=dev) if full.numel() else None
        rows, cols = (C.c_int64 * B)(*G), (C.c_int64 * B)(*S)
        L.call("pq3d_instance_masks", self.p2i, self.seg, C.cast(self.off, C.c_void_p), B, self.rank, C.cast(rows, C.c_void_p),
               C.cast(cols, C.c_void_p), seg_masks if seg_masks.numel() else None, prank, full if full.numel() else None)
        split = lambda flat, widths: [m.view(torch.bool).view(g, w) for m, g, w in
                                      zip(torch.split(flat, [g * w for g, w in zip(G, widths)]), G, widths)]
        return dict(instance_ids=[self.table[0, b, :G[b]] for b in range(B)], instance_labels=[self.table[1, b, :G[b]] for b in range(B)],
                    segment_masks=split(seg_masks, S), full_masks=split(full, self.lens) if with_full_masks else None)


def instance_targets(point2instance: Sequence[torch.Tensor], point2semantic: Sequence[torch.Tensor],
                     point2segment: Sequence[torch.Tensor], *, filter_out_classes: Sequence[int] = (0, 2),
                     with_full_masks: bool = True) -> Dict[str, Optional[list]]:
    """The training targets of a batch of scenes (at most 8) from their per-point ids, on the device: what the reference's
    extract_inst_info builds per scene on the host.  Per scene b three [P_b] int64 device tensors: ``point2instance`` (values
    in [-1, 4096), -1 = no object, gaps allowed), ``point2semantic`` (any value) and ``point2segment`` (>= 0).

    The distinct instance ids in ascending order are the candidates; an instance's label is ``point2semantic`` at its LOWEST
    point index; it is kept iff its id is not -1 and its label is not in ``filter_out_classes``.  Returns per-scene lists:
    ``instance_ids`` [G_b] int64, ``instance_labels`` [G_b] int64, ``segment_masks`` [G_b, S_b] bool (S_b = largest segment
    id + 1; true iff some point carries (instance, segment)) and ``full_masks`` [G_b, P_b] bool (None when
    ``with_full_masks`` is false).  G_b = 0 is legal.

    The masks are ``torch.bool``, one byte per cell, where the reference's ``full_masks`` is an int64 tensor: every consumer
    (``instseg_ap.gt_boxes``, the criterion's ``.float()``) only tests or converts the cells, and eight bytes per cell are
    80 MB for 100 instances x 100k points.  One device-to-host read (the counts and the error word); ids outside their
    range raise ValueError."""
    t = _InstanceTables(point2instance, point2semantic, point2segment, filter_out_classes)
    return t.masks(t.meta.tolist(), with_full_masks)                # (host sync: outside any graph)


def padded_instance_targets(point2instance: Sequence[torch.Tensor], point2semantic: Sequence[torch.Tensor],
                            point2segment: Sequence[torch.Tensor], Ns: int, max_instances: int, *,
                            filter_out_classes: Sequence[int] = (0, 2), out=None):
    """The same targets written straight into the padded layout the device criterion reads (``losses.PaddedTargets`` at
    ``Nt = max_instances``, what ``SetCriterion.pad_targets`` builds in a host loop) with NO device-to-host read.  Returns
    ``(targets, err)``: ``err`` is a device int32 word (``check_instance_targets(err)`` reads it and raises): bit 1 an
    instance id outside [-1, 4096), bit 2 a segment id outside [0, Ns), bit 4 more than ``max_instances`` kept instances
    in a scene; the offending points (rows) are skipped.  ``out``: an existing PaddedTargets of these shapes to fill (the
    static buffers a captured step reads); everything in it is overwritten."""
    from .losses import PaddedTargets
    p2i, sem, seg, off, lens = _id_scenes(point2instance, point2semantic, point2segment, "padded_instance_targets")
    B, dev, Ns, Nt = len(lens), p2i.device, int(Ns), int(max_instances)
    if not (1 <= Ns <= INSTANCE_MAX_SEGMENTS and 1 <= Nt <= INSTANCE_MAX_IDS):
        raise ValueError(f"padded_instance_targets: need 1 <= Ns <= {INSTANCE_MAX_SEGMENTS} and 1 <= max_instances <= {INSTANCE_MAX_IDS}")
    flt, n_flt = _filter(filter_out_classes)
    if out is None:
        out = PaddedTargets(torch.empty(B, Nt, Ns, dtype=torch.float32, device=dev), torch.empty(B, Nt, dtype=torch.int64, device=dev),
                            torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                            torch.empty(B, Nt, dtype=torch.float32, device=dev))
    else:
        want = dict(T=((B, Nt, Ns), torch.float32), labels=((B, Nt), torch.int64), seg_len=((B,), torch.int32),
                    n_inst_dev=((B,), torch.int32), t_sum=((B, Nt), torch.float32))
        for k, (shape, dt) in want.items():
            t = getattr(out, k)
            if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError(f"padded_instance_targets: out.{k} must be a contiguous {dt} tensor of shape {shape} on {dev}")
    ws = torch.empty(2 * B * (INSTANCE_MAX_IDS + 1) + B * Nt + 1, dtype=torch.int32, device=dev)
    n = B * (INSTANCE_MAX_IDS + 1)
    first, rank, cnt, err = ws[:n], ws[n:2 * n], ws[2 * n:2 * n + B * Nt], ws[2 * n + B * Nt:]
    offp = C.cast(off, C.c_void_p)
    L.call("pq3d_instance_tables", p2i, sem, seg, offp, B, flt, n_flt, Ns, Nt, first, rank,
           None, out.labels, out.n_inst_dev, out.seg_len, err)
    L.call("pq3d_instance_masks_padded", p2i, seg, offp, B, rank, Ns, Nt, out.T, cnt, out.t_sum)
    return out, err


def check_instance_targets(err: torch.Tensor) -> None:
    """Read the error word of ``padded_instance_targets`` (a host sync) and raise ValueError with the text of its bits."""
    L.raise_error_word("padded_instance_targets", int(err.reshape(-1)[0]), _INSTANCE_ERRORS)


# ----------------------------------------------------------------------------- train-time augmentation
# One row of ``params``: the fields of pq3d_scene_augment_params (include/pq3d_hip.h, bound as _lib.SceneAugmentParams) as
# {name: (first float, floats)}; this is the only place the Python side spells the layout.
AUG_FIELDS: Dict[str, Tuple[int, int]] = {n: (getattr(L.SceneAugmentParams, n).offset // 4, getattr(L.SceneAugmentParams, n).size // 4)
                                          for n, *_ in L.SceneAugmentParams._fields_}
AUG_K = L.H.PQ3D_SCENE_AUGMENT_K
AUG_STAGES = ("centre", "offset", "flip", "scale", "rotate", "colour")
COLOR_MEAN = (0.47793125906962, 0.4303257521323044, 0.3749598901421883)      # the reference's A.Normalize constants
COLOR_STD = (0.2834475483823543, 0.27566157565723015, 0.27018971370874995)
_AUGMENT_ERRORS = {1: "coordinates hold non-finite values",
                   2: "colors hold non-finite values or values whose integer part leaves [0, 255] (saturated)"}


@dataclass(frozen=True)
class SceneAugmentConfig:
    """Limits of the train-time augmentation; the defaults are the two augmentation files the stage-1 configs ship
    (volumentations: Scale3d, three RotateAroundAxis3d; albumentations: RandomBrightnessContrast, RGBShift; all
    ``always_apply``) and get_scene's own flip probability."""
    scale_limit: Tuple[Tuple[float, float], ...] = ((-0.1, 0.1), (-0.1, 0.1), (-0.1, 0.1))     # factor = 1 + U(lo, hi) per axis
    rotations: Tuple[Tuple[Tuple[float, float, float], Tuple[float, float]], ...] = (           # (axis, (lo, hi) radians), in turn
        ((0.0, 0.0, 1.0), (-3.141592653589793, 3.141592653589793)),
        ((0.0, 1.0, 0.0), (-0.13089969389957, 0.13089969389957)),
        ((1.0, 0.0, 0.0), (-0.13089969389957, 0.13089969389957)))
    contrast_limit: Tuple[float, float] = (-0.2, 0.2)         # alpha = 1 + U(lo, hi)
    brightness_limit: Tuple[float, float] = (-0.2, 0.2)       # beta = U(lo, hi), times 255 (brightness_by_max)
    rgb_shift_limit: Tuple[Tuple[float, float], ...] = ((-20.0, 20.0), (-20.0, 20.0), (-20.0, 20.0))   # r, g, b
    flip_p: float = 0.5

    @staticmethod
    def from_files(volume_yaml: str, image_yaml: str) -> "SceneAugmentConfig":
        """Read the two serialised ``Compose`` files: Scale3d followed by three RotateAroundAxis3d, and
        RandomBrightnessContrast followed by RGBShift, every one ``always_apply``.  Anything else is not implemented."""
        import yaml

        def transforms(path, want):
            with open(path) as f:
                ts = yaml.safe_load(f)["transform"]["transforms"]
            names = [t["__class_fullname__"].rsplit(".", 1)[-1] for t in ts]
            for n, t in zip(names, ts):
                if n not in want:
                    raise NotImplementedError(f"{path}: transform {t['__class_fullname__']} is not implemented")
                if not t.get("always_apply", False):
                    raise NotImplementedError(f"{path}: {n} without always_apply is not implemented")
            if names != want:
                raise NotImplementedError(f"{path}: expected the transforms {want} in this order, got {names}")
            return ts

        pair = lambda v: (float(v[0]), float(v[1]))
        scale, *rots = transforms(volume_yaml, ["Scale3d"] + ["RotateAroundAxis3d"] * 3)
        bc, shift = transforms(image_yaml, ["RandomBrightnessContrast", "RGBShift"])
        if not bc.get("brightness_by_max", True):
            raise NotImplementedError(f"{image_yaml}: RandomBrightnessContrast without brightness_by_max is not implemented")
        return SceneAugmentConfig(
            scale_limit=tuple(pair(v) for v in scale["scale_limit"]),
            rotations=tuple((tuple(float(a) for a in r["axis"]), pair(r["rotation_limit"])) for r in rots),
            contrast_limit=pair(bc["contrast_limit"]), brightness_limit=pair(bc["brightness_limit"]),
            rgb_shift_limit=tuple(pair(shift[k]) for k in ("r_shift_limit", "g_shift_limit", "b_shift_limit")))


def _rotation(axis: Sequence[float], angle: float) -> np.ndarray:
    """Rodrigues' formula in fp64: the right-handed rotation by ``angle`` about ``axis`` through the origin, applied as R x."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) * np.cos(angle) + np.sin(angle) * K + (1.0 - np.cos(angle)) * np.outer(a, a)


def draw_scene_augment(B: int, cfg: SceneAugmentConfig, rng: np.random.Generator, *,
                       stages: Sequence[str] = AUG_STAGES) -> torch.Tensor:
    """The random parameters of ``B`` scenes: a CPU fp32 tensor [B, AUG_K] of pq3d_scene_augment_params rows (``AUG_FIELDS``),
    drawn on the host from ``rng`` (no device read); the caller copies it to the device.  ``stages``: the stages whose flag
    is set (all by default).  Everything that depends on the conventions of volumentations / albumentations (factor
    = 1 + U, the rotation centre and sense, alpha / beta, which channel a shift belongs to) is decided HERE and nowhere else:
    the kernels only apply the rows."""
    unknown = sorted(set(stages) - set(AUG_STAGES))
    if unknown:
        raise ValueError(f"draw_scene_augment: unknown stages {unknown} (known: {AUG_STAGES})")
    if len(cfg.rotations) != 3 or len(cfg.scale_limit) != 3 or len(cfg.rgb_shift_limit) != 3:
        raise ValueError("draw_scene_augment: the config needs 3 scale limits, 3 rotations and 3 shift limits")
    rows = np.zeros((int(B), AUG_K), dtype=np.float32)

    def put(row, name, value):
        at, n = AUG_FIELDS[name]
        row[at:at + n] = np.asarray(value, dtype=np.float64).reshape(n)

    for row in rows:
        put(row, "u", rng.random(3, dtype=np.float32))           # (drawn in fp32: a rounded fp64 draw could reach 1)
        put(row, "flip", rng.random(2) < cfg.flip_p)
        put(row, "scale", [1.0 + rng.uniform(lo, hi) for lo, hi in cfg.scale_limit])
        put(row, "rot", np.stack([_rotation(axis, rng.uniform(lo, hi)) for axis, (lo, hi) in cfg.rotations]))
        put(row, "alpha", 1.0 + rng.uniform(*cfg.contrast_limit))
        put(row, "beta255", rng.uniform(*cfg.brightness_limit) * 255.0)
        put(row, "shift", [rng.uniform(lo, hi) for lo, hi in cfg.rgb_shift_limit])
        for s in AUG_STAGES:
            put(row, "on_" + s, float(s in stages))
    return torch.from_numpy(rows)


def color_constants(color_mean: Sequence[float] = COLOR_MEAN, color_std: Sequence[float] = COLOR_STD) -> np.ndarray:
    """The six fp32 constants of the Normalize stage: fp32(mean * 255) and the fp32 reciprocal of fp32(std * 255)."""
    mean = np.asarray(color_mean, dtype=np.float64).reshape(3)
    std = np.asarray(color_std, dtype=np.float64).reshape(3)
    return np.concatenate([(mean * 255.0).astype(np.float32), np.float32(1.0) / (std * 255.0).astype(np.float32)])


def augment_scenes(coordinates: Sequence[torch.Tensor], colors: Sequence[torch.Tensor], params: Optional[torch.Tensor], *,
                   train: bool = True, color_mean: Sequence[float] = COLOR_MEAN, color_std: Sequence[float] = COLOR_STD,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """get_scene's point-wise part for a batch of scenes (at most 8), on the device: per scene ``coordinates[b]`` [P_b, 3] and
    ``colors[b]`` [P_b, 3] fp32 (raw colours in [0, 256)), ``params`` [B, AUG_K] fp32 device rows from ``draw_scene_augment``.
    ``train=True``: centre, random offset, axis flips, scale, three rotations, brightness / contrast and RGB shift, each
    under its flag; always: colour -> integer -> Normalize, ``features = colour | xyz``.  ``train=False`` (``params`` may be
    None): the coordinates come back bit for bit.  Returns ``(coordinates_out, features_out, err)``: per-scene views of one
    [P, 3] and one [P, 6] tensor and the device error word [1] int32 (``check_scene_augment(err)`` reads it).  Two launches,
    no device-to-host read; the same inputs give the same bits.  ``out=(xyz [P, 3], features [P, 6])``: contiguous fp32
    buffers to write into (the static buffers of a captured step)."""
    pts, off, lens = _scenes(coordinates, "augment_scenes", MAX_SCENES, MAX_POINTS)
    col, _off, clens = _scenes(colors, "augment_scenes", MAX_SCENES)
    if clens != lens or col.device != pts.device:
        raise ValueError("augment_scenes: one [P_b, 3] colors tensor per scene, matching coordinates")
    B, P, dev = len(lens), sum(lens), pts.device
    if train:
        if params is None:
            raise ValueError("augment_scenes: train=True needs params (draw_scene_augment)")
        _need_device(params)
        if params.dtype != torch.float32 or tuple(params.shape) != (B, AUG_K) or not params.is_contiguous() or params.device != dev:
            raise ValueError(f"augment_scenes: params must be a contiguous fp32 [{B}, {AUG_K}] tensor on {dev}")
    if out is None:
        xyz_out, feat_out = torch.empty(P, 3, dtype=torch.float32, device=dev), torch.empty(P, 6, dtype=torch.float32, device=dev)
    else:
        xyz_out, feat_out = out
        for t, w in ((xyz_out, 3), (feat_out, 6)):
            _need_device(t)
            if t.dtype != torch.float32 or tuple(t.shape) != (P, w) or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"augment_scenes: out must be contiguous fp32 tensors [{P}, 3] and [{P}, 6] on {dev}")
    offp = C.cast(off, C.c_void_p)
    ws_bytes = int(L.lib().pq3d_scene_augment_ws_bytes(offp, B))
    L.check(0 if ws_bytes >= 0 else -1, "pq3d_scene_augment_ws_bytes")
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev) if train else None
    err = torch.empty(1, dtype=torch.int32, device=dev)
    consts = (C.c_float * 6)(*color_constants(color_mean, color_std).tolist())
    L.call("pq3d_scene_augment_stats", pts, offp, B, int(bool(train)), ws, ws_bytes, err)
    L.call("pq3d_scene_augment_apply", pts, col, offp, B, params if train else None, ws, ws_bytes, C.cast(consts, C.c_void_p),
           xyz_out, feat_out, err)
    return list(torch.split(xyz_out, lens)), list(torch.split(feat_out, lens)), err


def check_scene_augment(err: torch.Tensor) -> None:
    """Read the error word of ``augment_scenes`` (a host sync) and raise ValueError with the text of its bits."""
    L.raise_error_word("augment_scenes", int(err.reshape(-1)[0]), _AUGMENT_ERRORS)


def prepare_instseg_batch(coordinates: Sequence[torch.Tensor], features: Optional[Sequence[torch.Tensor]],
                          point2segment: Sequence[torch.Tensor], voxel_size: float, num_queries: int, *,
                          query_sample_strategy: str = "fps", point2instance: Optional[Sequence[torch.Tensor]] = None,
                          instance_ids: Optional[Sequence[torch.Tensor]] = None, query_from: str = "points",
                          point2semantic: Optional[Sequence[torch.Tensor]] = None, filter_out_classes: Sequence[int] = (0, 2),
                          offline_mask_source: Optional[str] = None, colors: Optional[Sequence[torch.Tensor]] = None,
                          augment: Optional[torch.Tensor] = None) -> Dict[str, object]:
    """get_scene + collate_fn of the reference for a batch of scenes, on the device.  Per scene b: ``coordinates[b]`` [P_b, 3]
    fp32, ``features[b]`` [P_b, F] fp32 (the reference: colour | xyz, so that ``voxel_features[:, -3:]`` are coordinates),
    ``point2segment[b]`` [P_b] int64; optional ``point2instance[b]`` [P_b] int64 (-1 = no instance) with
    ``instance_ids[b]`` [I_b] int64 for the object centres.

    Returns the keys the model and the evaluators read: ``voxel_coordinates`` [V, 4] int32 and ``voxel_features`` [V, F]
    (``features[unique_map]``), the per-scene lists ``voxel2segment`` (``point2segment[unique_map]``), ``coordinates``
    (``voxel_features[:, -3:]``), ``voxel_to_full_maps``, ``segment_to_full_maps``, ``raw_coordinates``, and, padded with
    collate.pad_sequence, ``seg_center`` / ``seg_pad_masks``, ``obj_center`` / ``obj_pad_masks`` (when instances are given),
    ``query_locs`` / ``query_pad_masks``, ``coord_min`` / ``coord_max`` [B, 3].

    Centres are scatter_mean over the points: dim_size = largest id + 1, an id without points gives a zero row, instance -1
    counts as ``instance_ids.max() + 1`` (as the reference does) and ``obj_center`` is the table at ``instance_ids``.

    ``query_sample_strategy="fps"``: farthest point sampling of ``num_queries`` voxels on the float voxel lattice
    coordinates.  ``query_from="points"`` reproduces the reference, quirk included: ``query_locs = coordinates[fps_idx]``
    indexes the RAW POINTS with VOXEL indices (sample_query is handed the unquantised cloud), so the locations are those of
    the first V_b points of the file, not of the sampled voxels.  ``query_from="voxels"`` gives
    ``coordinates[unique_map[fps_idx]]``, the sampled voxels' representative points.  ``"gt"`` returns ``obj_center``.

    With ``point2instance`` and ``point2semantic`` ([P_b] int64 each) and no ``instance_ids`` the training targets are
    derived from the point ids (``instance_targets`` with ``filter_out_classes``): the list keys ``instance_ids``,
    ``instance_labels``, ``segment_masks`` and ``full_masks`` are added, and the derived ``instance_ids`` give ``obj_center``.
    ``offline_mask_source='gt'`` then adds collate_fn's padded keys ``offline_attn_mask`` (True as masked), ``target_labels``
    (padded with -100), ``target_masks`` (fp32) and ``target_masks_pad_masks``; any other value is not implemented.
    Host reads: one in ``voxelize``, one for the largest segment / instance ids (and the derived targets' counts).

    ``colors`` (per scene [P_b, 3] fp32 raw colours, ``features`` then None): the batch is built from
    ``augment_scenes(coordinates, colors, augment, train=augment is not None)``: ``augment`` [B, AUG_K] device rows of
    ``draw_scene_augment`` give the train-time augmentation, None the evaluation path (colour normalisation and the
    feature rows only).  ``raw_coordinates`` are then the augmented coordinates, as in get_scene; the error word of
    ``augment_scenes`` rides in the second host read."""
    B = len(coordinates)
    if colors is not None and features is not None:
        raise ValueError("pass features or colors, not both")
    if colors is None and augment is not None:
        raise ValueError("augment needs colors")
    if colors is None and features is None:
        raise ValueError("one of features and colors is needed")
    if not (len(features if colors is None else colors) == len(point2segment) == B):
        raise ValueError("one features / point2segment entry per scene")
    if query_sample_strategy not in ("fps", "gt"):
        raise NotImplementedError(f"{query_sample_strategy} is not implemented")
    if query_from not in ("points", "voxels"):
        raise ValueError(f"query_from must be 'points' or 'voxels', got {query_from!r}")
    if offline_mask_source not in (None, "gt"):
        raise NotImplementedError(f"{offline_mask_source} is not implemented")
    with_obj = point2instance is not None
    derive = with_obj and instance_ids is None and point2semantic is not None     # the targets come from the point ids
    if derive and (len(point2instance) != B or len(point2semantic) != B):
        raise ValueError("one point2instance / point2semantic entry per scene")
    if with_obj and not derive and (instance_ids is None or len(point2instance) != B or len(instance_ids) != B):
        raise ValueError("point2instance needs instance_ids, one entry per scene each")
    if query_sample_strategy == "gt" and not with_obj:
        raise ValueError("query_sample_strategy='gt' needs point2instance and instance_ids")
    if offline_mask_source == "gt" and not derive:
        raise ValueError("offline_mask_source='gt' needs point2instance and point2semantic (and no instance_ids)")
    aug_err = None
    if colors is not None:
        coordinates, features, aug_err = augment_scenes(coordinates, colors, augment, train=augment is not None)
    voxel_coordinates, unique_map, inverse_map = voxelize(coordinates, voxel_size)
    for b in range(B):
        if features[b].shape[0] != coordinates[b].shape[0] or point2segment[b].shape != coordinates[b].shape[:1]:
            raise ValueError(f"scene {b}: features [P, F] and point2segment [P] must match coordinates [P, 3]")
        if point2segment[b].dtype != torch.int64 or features[b].dtype != torch.float32:
            raise ValueError("features are fp32, point2segment int64")
    vfeat = [features[b][unique_map[b]] for b in range(B)]
    out: Dict[str, object] = dict(
        voxel_coordinates=voxel_coordinates, voxel_features=torch.cat(vfeat, 0),
        voxel2segment=[point2segment[b][unique_map[b]] for b in range(B)], coordinates=[f[:, -3:] for f in vfeat],
        voxel_to_full_maps=inverse_map, segment_to_full_maps=list(point2segment), raw_coordinates=list(coordinates))
    # table sizes of the scatter_means (largest id + 1): one read for the whole batch
    # (derived targets: their counts and error word ride in the same read; a scene without instances counts as largest id -1)
    tops = [point2segment[b].max() for b in range(B)]
    if derive:
        tables = _InstanceTables(point2instance, point2semantic, point2segment, filter_out_classes)
        last_id = tables.last_ids()
        tops = torch.cat([torch.stack(tops), last_id, torch.stack([point2instance[b].max() for b in range(B)]), tables.meta.long()])
    else:
        if with_obj:
            tops += [instance_ids[b].max() for b in range(B)] + [point2instance[b].max() for b in range(B)]
            last_id = tops[B:2 * B]
        tops = torch.stack(tops)
    if aug_err is not None:                                      # (the augmentation's error word rides in the same read)
        tops = torch.cat([tops, aug_err.long()])
    tops = tops.tolist()                                         # (host sync)
    if aug_err is not None:
        L.raise_error_word("prepare_instseg_batch", tops.pop(), _AUGMENT_ERRORS)
    if derive:
        targets = tables.masks(tops[3 * B:], True)
        instance_ids = targets["instance_ids"]
        out.update(targets)
        if offline_mask_source == "gt":                          # collate_fn: True as masked
            padded, padding = collate.pad_sequence_2d(targets["segment_masks"], return_mask=True)
            out["offline_attn_mask"], out["target_masks"] = padded.logical_not(), padded.float()
            out["target_labels"] = collate.pad_sequence(targets["instance_labels"], pad=-100)
            out["target_masks_pad_masks"] = padding.logical_not()
    seg_center = _centers(coordinates, point2segment, [t + 1 for t in tops[:B]])
    ones = lambda ts: [torch.ones(t.shape[0], dtype=torch.bool, device=t.device) for t in ts]
    out["seg_center"], out["seg_pad_masks"] = collate.pad_sequence(seg_center), collate.pad_sequence(ones(seg_center))
    if with_obj:
        p2i = [torch.where(point2instance[b] == -1, last_id[b] + 1, point2instance[b]) for b in range(B)]
        sizes = [max(tops[2 * B + b], tops[B + b] + 1) + 1 for b in range(B)]     # (covers the row that -1 maps to)
        table = _centers(coordinates, p2i, sizes)
        obj_center = [table[b][instance_ids[b]] for b in range(B)]
        out["obj_center"], out["obj_pad_masks"] = collate.pad_sequence(obj_center), collate.pad_sequence(ones(obj_center))
    if query_sample_strategy == "fps":
        V = [int(u.shape[0]) for u in unique_map]
        if int(num_queries) < 1 or int(num_queries) > min(V):
            raise ValueError(f"num_queries = {num_queries} needs 1 <= num_queries <= the voxels of the smallest scene ({min(V)})")
        lattice = list(torch.split(voxel_coordinates[:, 1:].float(), V))
        fps_idx = farthest_point_sample(lattice, int(num_queries))
        if query_from == "points":
            locs = [coordinates[b][fps_idx[b]] for b in range(B)]
        else:
            locs = [coordinates[b][unique_map[b][fps_idx[b]]] for b in range(B)]
        out["query_locs"], out["query_pad_masks"] = collate.pad_sequence(locs), collate.pad_sequence(ones(locs))
    else:
        out["query_locs"], out["query_pad_masks"] = out["obj_center"], out["obj_pad_masks"]
    out["coord_min"] = collate.pad_sequence([c.min(0)[0] for c in coordinates])
    out["coord_max"] = collate.pad_sequence([c.max(0)[0] for c in coordinates])
    return out
