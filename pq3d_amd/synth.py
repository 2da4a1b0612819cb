"""Deterministic synthetic weights and inputs (SURVEY §8c fixture plan, §8d synthetic inputs).

Used by the golden-fixture generator, the tests and ``bench.py``.  Everything is drawn from
``numpy.random.default_rng`` keyed by (seed, crc32(name)) so a tensor's values depend only on
its *name and shape*, never on module construction order: the same call fills the reference
modules (golden generation), the oracle's flat dict and the HIP modules.
"""
from __future__ import annotations

import zlib
from typing import Dict, Mapping, Sequence

import numpy as np
import torch


def _rng(seed: int, name: str) -> np.random.Generator:
    return np.random.default_rng([seed, zlib.crc32(name.encode())])


def synth_tensor(name: str, shape: Sequence[int], seed: int = 0) -> torch.Tensor:
    """matrices ~ N(0,0.05) (so attention is not degenerate), biases ~ N(0,0.02),
    LayerNorm / BatchNorm gamma ~ U(0.5,1.5), Fourier ``gauss_B`` ~ N(0,1), BatchNorm running_var ~ U(0.5,1.5),
    running_mean ~ N(0,0.1)."""
    r = _rng(seed, name)
    shape = tuple(int(s) for s in shape)
    if name.endswith("num_batches_tracked"):
        return torch.zeros(shape, dtype=torch.int64)
    if name.endswith("gauss_B"):
        a = r.standard_normal(shape)
    elif name.endswith("running_var"):
        a = r.uniform(0.5, 1.5, shape)
    elif name.endswith("running_mean"):
        a = 0.1 * r.standard_normal(shape)
    elif len(shape) >= 2:
        a = 0.05 * r.standard_normal(shape)
    elif name.endswith("weight"):
        a = r.uniform(0.5, 1.5, shape)
    else:
        a = 0.02 * r.standard_normal(shape)
    return torch.from_numpy(a.astype(np.float32))


def synth_state_dict(shapes: Mapping[str, Sequence[int]], seed: int = 0) -> Dict[str, torch.Tensor]:
    return {k: synth_tensor(k, tuple(v), seed) for k, v in shapes.items()}


def fill_module(module: torch.nn.Module, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Overwrite every parameter/buffer of ``module`` with its synthetic value; returns the dict."""
    sd = module.state_dict()
    new = synth_state_dict({k: v.shape for k, v in sd.items()}, seed)
    module.load_state_dict(new, strict=True)
    return new


def state_checksum(sd: Mapping[str, torch.Tensor]) -> float:
    """Order-independent fingerprint stored in fixtures to detect RNG drift."""
    return float(sum(float(v.double().abs().sum()) for v in sd.values()))


def synth_data_dict(B: int, n_seg: int, n_q: int, d_in: Mapping[str, int], seed: int = 1234,
                    memories: Sequence[str] = ("voxel", "mv", "pc"), prompt_len: int = 0, d_model: int = 0,
                    full_valid: bool = False, query_valid_min: int | None = None,
                    loc_dim: int = 3) -> Dict[str, torch.Tensor]:
    """SURVEY §8d synthetic inputs.  Pad masks here are the data_dict convention: True = valid."""
    r = np.random.default_rng(seed)
    valid_len = r.integers(n_seg // 2, n_seg + 1, size=B)
    valid_len[0] = n_seg
    if full_valid:
        valid_len[:] = n_seg
    seg_valid = np.arange(n_seg)[None, :] < valid_len[:, None]
    dd: Dict[str, torch.Tensor] = {}
    for m in memories:
        if m == "prompt":
            continue
        f = r.standard_normal((B, n_seg, d_in[m])).astype(np.float32)
        f[~seg_valid] = 0.0
        dd[f"{m}_seg_fts"] = torch.from_numpy(f)
        dd[f"{m}_seg_pad_masks"] = torch.from_numpy(seg_valid.copy())
    dd["seg_pad_masks"] = torch.from_numpy(seg_valid.copy())
    dd["seg_center"] = torch.from_numpy(r.uniform(0, 4, (B, n_seg, loc_dim)).astype(np.float32))
    dd["query_locs"] = torch.from_numpy(r.uniform(0, 4, (B, n_q, loc_dim)).astype(np.float32))
    dd["coord_min"] = torch.zeros(B, 3)
    dd["coord_max"] = torch.full((B, 3), 4.0)
    if query_valid_min is None:
        qv = np.ones((B, n_q), dtype=bool)
    else:
        ql = r.integers(query_valid_min, n_q + 1, size=B)
        qv = np.arange(n_q)[None, :] < ql[:, None]
    dd["query_pad_masks"] = torch.from_numpy(qv)
    if prompt_len:
        pl = r.integers(max(1, prompt_len // 4), prompt_len + 1, size=B)
        pv = np.arange(prompt_len)[None, :] < pl[:, None]
        pf = r.standard_normal((B, prompt_len, d_model)).astype(np.float32)
        pf[~pv] = 0.0
        dd["prompt_feat"] = torch.from_numpy(pf)
        dd["prompt_pad_masks"] = torch.from_numpy(pv)
    return dd


def prompt_loc_inputs(B: int, T: int, seed: int = 77) -> Dict[str, torch.Tensor]:
    """Location prompts of query3d_unified.py:80-108 (PromptType.LOC = 3): prompt [B, T] whose first entries are a point in the
    scene's coordinate range, ragged pad masks (True = valid), one prompt type per scene.  Shared by tests/golden/make_golden.py
    (fixture F20) and the tests."""
    r = np.random.default_rng(seed)
    pl = r.integers(1, T + 1, size=B)
    return {"prompt": torch.from_numpy(r.uniform(0, 4, (B, T)).astype(np.float32)),
            "prompt_pad_masks": torch.from_numpy(np.arange(T)[None, :] < pl[:, None]),
            "prompt_type": torch.full((B,), 3, dtype=torch.long)}


def variant_inputs(B=2, Ns=50, Nq=12, d=64, seed=31):
    """Inputs of fixture F21 (pre-norm layers, 'bias' spatial fusion, GroundHeadV1), shared by make_golden.py and the tests:
    a query state, two scene memories with ragged padding, position embeddings, query centres."""
    r = np.random.default_rng(seed)
    t = lambda *sh: torch.from_numpy(r.standard_normal(sh).astype(np.float32))
    vl = r.integers(Ns // 2, Ns + 1, size=B); vl[0] = Ns
    pad = torch.from_numpy(np.arange(Ns)[None, :] >= vl[:, None])          # True = padded
    ql = r.integers(Nq // 2, Nq + 1, size=B); ql[0] = Nq
    qpad = torch.from_numpy(np.arange(Nq)[None, :] >= ql[:, None])
    feats = {}
    for m in ("voxel", "mv"):
        f = t(B, Ns, d); f[pad] = 0.0
        feats[m] = f
    return dict(query=t(B, Nq, d), qpos=t(B, Nq, d), fpos=t(B, Ns, d), feats=feats, pad=pad, qpad=qpad,
                centers=torch.from_numpy(r.uniform(0, 4, (B, Nq, 3)).astype(np.float32)),
                txt=t(B, 5, d), pre=t(B, Nq, d))


def criterion_inputs(seed=21, B=3, Ns=70, Nq=12, C=21, n_layers=3, seg_len=(70, 55, 61), n_inst=(5, 9, 3)):
    """Synthetic predictions / targets of the F9 criterion fixture (also rebuilt by the tests)."""
    r = np.random.default_rng(seed)
    masks, logits = [], []
    for _ in range(n_layers):
        m = (r.standard_normal((B, Ns, Nq)) * 2.0).astype(np.float32)
        for b in range(B):
            m[b, seg_len[b]:] = -1e6          # what the mask head writes for padded segments (mask_head.py:38)
        lg = r.standard_normal((B, Nq, C)).astype(np.float32)
        lg[..., [0, 2]] = -np.inf              # filter_out_classes (mask_head.py:28)
        masks.append(torch.from_numpy(m)); logits.append(torch.from_numpy(lg))
    labels = [torch.from_numpy(r.integers(3, C - 1, n_inst[b])) for b in range(B)]
    labels[1][2] = -100                        # one ignored target
    seg = [torch.from_numpy((r.random((n_inst[b], seg_len[b])) < 0.2).astype(np.int64)) for b in range(B)]
    return masks, logits, labels, seg


def direct_loss_inputs(seed=31, B=3, S=70, N=12, C=21, n_layers=2, seg_len=(70, 55, 61), n_inst=(5, 12, 3)):
    """Synthetic predictions / padded targets of the F10 fixture (DirectCriterion and the stage-2 mask_loss)."""
    r = np.random.default_rng(seed)
    masks, logits = [], []
    for _ in range(n_layers):
        masks.append(torch.from_numpy((r.standard_normal((B, S, N)) * 2.0).astype(np.float32)))
        logits.append(torch.from_numpy(r.standard_normal((B, N, C)).astype(np.float32)))
    tgt = torch.zeros(B, N, S)
    pad = torch.zeros(B, N, S, dtype=torch.bool)          # False for padding pixels and padding instances
    labels = torch.full((B, N), -100, dtype=torch.int64)
    for b in range(B):
        tgt[b, :n_inst[b], :seg_len[b]] = torch.from_numpy((r.random((n_inst[b], seg_len[b])) < 0.25).astype(np.float32))
        pad[b, :n_inst[b], :seg_len[b]] = True
        labels[b, :n_inst[b]] = torch.from_numpy(r.integers(0, C, n_inst[b]))
    obj_masks = labels >= 0
    lab2 = labels.clamp(min=0)
    return masks, logits, tgt, pad, labels, obj_masks, lab2


def collate_inputs(seed=41):
    """Ragged per-sample tensors of the F11 collate fixture: segment features, centres, labels (int64), pad masks (bool),
    instance x segment target masks (int64, 2-D ragged)."""
    r = np.random.default_rng(seed)
    lens = [37, 5, 64, 1]
    feats = [torch.from_numpy(r.standard_normal((n, 24)).astype(np.float32)) for n in lens]
    centers = [torch.from_numpy(r.uniform(0, 4, (n, 3)).astype(np.float32)) for n in lens]
    labels = [torch.from_numpy(r.integers(0, 200, n)) for n in lens]
    valid = [torch.ones(n, dtype=torch.bool) for n in lens]
    ninst = [4, 9, 2, 1]
    seg_masks = [torch.from_numpy((r.random((k, n)) < 0.3).astype(np.int64)) for k, n in zip(ninst, lens)]
    return feats, centers, labels, valid, seg_masks


def pointcloud_inputs(M: int = 4, P: int = 300, C: int = 3, seed: int = 21) -> torch.Tensor:
    """Object point clouds [M, P, 3 + C] for the PointNet++ tokenizer: xyz uniform in a unit cube (so radius-0.2 balls
    hold fewer than nsample points and the fill rule is exercised), one cloud squeezed to a thin slab, colours in [0,1]."""
    r = np.random.default_rng(seed)
    xyz = r.uniform(-0.5, 0.5, (M, P, 3))
    xyz[M - 1, :, 2] *= 0.05
    rgb = r.uniform(0.0, 1.0, (M, P, C))
    return torch.from_numpy(np.concatenate([xyz, rgb], -1).astype(np.float32))


def _cut_runs(lengths: np.ndarray, n: int) -> np.ndarray:
    """The leading run lengths (each >= 1) that cover n items, the last one shortened to fit."""
    end = np.cumsum(lengths)
    k = int(np.searchsorted(end, n)) + 1
    out = lengths[:k].astype(np.int64)
    out[-1] -= int(end[k - 1]) - n
    return out


def instseg_inputs(seed: int = 5, P=(2000,), S: int = 64, Q: int = 24, C: int = 20, ninf_cols=(0, 2), mean_voxel: float = 2.0,
                   mean_seg: float = 40.0, empty_queries: int = 2, double_class: bool = True):
    """Seeded inputs of the instance-prediction step (InstSegEval.eval_instance_step, evaluator/instseg_eval.py:85-149) for
    len(P) ragged scenes of P[b] points.  Returns CPU tensors: pred_logits [B, Q, C+1] (columns `ninf_cols` -inf, as the mask
    head fills them), pred_masks [B, S, Q], and per scene voxel2segment [V_b], voxel_to_full_maps [P_b], segment_to_full_maps
    [P_b] (int64) and raw_coordinates [P_b, 3] (fp32).

    Scene layout: full-resolution segments with geometric sizes (mean `mean_seg` points) laid out along a walk; voxels are runs
    of 1..2*mean_voxel-1 consecutive points of that walk, so some voxels straddle a segment boundary; a voxel's segment is the
    segment of its representative (first) point, so s1 = voxel2segment[voxel_to_full_maps[p]] differs from
    segment_to_full_maps[p] for some points, and small segments can end up without a voxel.  Points and voxels are then
    shuffled.  The first `empty_queries` queries have all-negative mask logits and a confident class (selected, empty masks);
    with `double_class` query Q-1 is confident in two classes (selected twice)."""
    r = np.random.default_rng([seed, 90210])
    B = len(P)
    logits = r.standard_normal((B, Q, C + 1)).astype(np.float32) * 2.0
    masks = (r.standard_normal((B, S, Q)) * 3.0).astype(np.float32)
    v2s_l, v2f_l, s2f_l, xyz_l = [], [], [], []
    for b in range(B):
        n = int(P[b])
        sizes = _cut_runs(r.geometric(1.0 / mean_seg, n), n)
        nseg = len(sizes)
        assert nseg <= S, f"scene {b}: {nseg} segments > S = {S}"
        ids = r.permutation(S)[:nseg]                       # segment ids scattered over [0, S): unused ids have no voxel
        seg_of_walk = np.repeat(ids, sizes)
        centers = r.uniform(0.0, 8.0, (nseg, 3))
        xyz_walk = np.repeat(centers, sizes, axis=0) + r.normal(0.0, 0.3, (n, 3))
        vs = _cut_runs(r.integers(1, int(2 * mean_voxel), n), n)
        nvox = len(vs)
        vox_walk = np.repeat(np.arange(nvox), vs)
        first = np.concatenate([[0], np.cumsum(vs)[:-1]])
        vperm = r.permutation(nvox)                         # voxel id order shuffled
        vnew = np.empty(nvox, np.int64)
        vnew[vperm] = np.arange(nvox)                       # voxel vperm[i] gets id i
        v2s = seg_of_walk[first][vperm]
        pperm = r.permutation(n)
        v2f = vnew[vox_walk][pperm]
        s2f = seg_of_walk[pperm]
        v2s_l.append(torch.from_numpy(v2s.astype(np.int64)))
        v2f_l.append(torch.from_numpy(v2f.astype(np.int64)))
        s2f_l.append(torch.from_numpy(s2f.astype(np.int64)))
        xyz_l.append(torch.from_numpy(xyz_walk[pperm].astype(np.float32)))
        for q in range(min(empty_queries, Q)):
            masks[b, :, q] = -np.abs(masks[b, :, q]) - 0.1
            logits[b, q, int(r.integers(0, C))] = 9.0 + q
        if double_class and Q > empty_queries:
            c1, c2 = r.choice([c for c in range(C) if c not in ninf_cols], 2, replace=False)
            logits[b, Q - 1, c1], logits[b, Q - 1, c2] = 7.5, 7.0
    for c in ninf_cols:
        logits[:, :, c] = -np.inf
    return dict(pred_logits=torch.from_numpy(logits), pred_masks=torch.from_numpy(masks), voxel2segment=v2s_l,
                voxel_to_full_maps=v2f_l, segment_to_full_maps=s2f_l, raw_coordinates=xyz_l)


def instseg_voxel_coordinates(inp, lattice: float = 0.1, cut_segments: int = 2, shift: float = 4.0):
    """Voxel coordinates for the DBSCAN option of the instance-prediction step from an instseg_inputs dict: one
    representative point per voxel (its lowest point index, as features[unique_map] keeps one row per voxel), snapped to a
    `lattice` grid (squared distances are then multiples of lattice^2, away from the boundary eps^2 = 0.9025 for lattice
    0.1).  In each scene the voxels of the first `cut_segments` segments with >= 4 voxels are cut in two: every second one is
    moved by `shift` along x, so a component boundary splits those segments.  Returns a list of [V_b, 3] fp32 CPU tensors."""
    out = []
    for b in range(len(inp["voxel2segment"])):
        v2s, v2f = inp["voxel2segment"][b].numpy(), inp["voxel_to_full_maps"][b].numpy()
        V = v2s.shape[0]
        rep = np.full(V, v2f.shape[0], np.int64)
        np.minimum.at(rep, v2f, np.arange(v2f.shape[0]))
        xyz = inp["raw_coordinates"][b].numpy().astype(np.float64)[rep]
        ids, cnt = np.unique(v2s, return_counts=True)
        for s in ids[cnt >= 4][:cut_segments]:
            vs = np.nonzero(v2s == s)[0]
            xyz[vs[1::2], 0] += shift
        out.append(torch.from_numpy((np.round(xyz / lattice) * lattice).astype(np.float32)))
    return out


def instseg_room(seed: int = 0, V: int = 100_000, Q: int = 200, C: int = 200, voxel: float = 0.02, seg: float = 0.3,
                 room=(8.0, 6.0, 3.0)):
    """One synthetic room scene for the DBSCAN option at `voxel` resolution: V voxels on the floor and the four walls of a
    room, one point per voxel, segments = `seg`-sized patches of a surface; query q's mask logits are positive on the
    segments within 0.4-1.2 m of one or two random surface centres (two blobs: split by DBSCAN); class logits as
    instseg_inputs.  Returns an instseg_inputs-style dict with B = 1 plus voxel_coordinates."""
    r = np.random.default_rng([seed, 4711])
    X, Y, Z = room
    areas = np.array([X * Y, X * Z, X * Z, Y * Z, Y * Z])
    face = r.choice(5, V, p=areas / areas.sum())
    u, w = r.random(V), r.random(V)
    xyz = np.zeros((V, 3))
    xyz[face == 0] = np.stack([u * X, w * Y, 0 * u], 1)[face == 0]
    xyz[face == 1] = np.stack([u * X, 0 * u, w * Z], 1)[face == 1]
    xyz[face == 2] = np.stack([u * X, 0 * u + Y, w * Z], 1)[face == 2]
    xyz[face == 3] = np.stack([0 * u, u * Y, w * Z], 1)[face == 3]
    xyz[face == 4] = np.stack([0 * u + X, u * Y, w * Z], 1)[face == 4]
    xyz = np.round(xyz / voxel) * voxel
    cellk = np.floor(xyz / seg).astype(np.int64)
    key = (face * 1000 + cellk[:, 0]) * 1000000 + cellk[:, 1] * 1000 + cellk[:, 2]
    _, v2s = np.unique(key, return_inverse=True)
    S = int(v2s.max()) + 1
    cen = np.zeros((S, 3))
    np.add.at(cen, v2s, xyz)
    cen /= np.bincount(v2s, minlength=S)[:, None]
    masks = np.full((S, Q), -3.0, np.float32)
    for q in range(Q):
        for k in range(1 + int(r.random() < 0.5)):
            c = xyz[r.integers(0, V)]
            rad = r.uniform(0.4, 1.2)
            near = np.linalg.norm(cen - c, axis=1) < rad
            masks[near, q] = r.uniform(0.5, 4.0, int(near.sum())).astype(np.float32)
    logits = r.standard_normal((1, Q, C + 1)).astype(np.float32) * 2.0
    t = lambda a: [torch.from_numpy(a)]
    return dict(pred_logits=torch.from_numpy(logits), pred_masks=torch.from_numpy(masks[None]),
                voxel2segment=t(v2s.astype(np.int64)), voxel_to_full_maps=t(np.arange(V, dtype=np.int64)),
                segment_to_full_maps=t(v2s.astype(np.int64)), raw_coordinates=t(xyz.astype(np.float32)),
                voxel_coordinates=t(xyz.astype(np.float32)))


def instseg_ap_scene(seed: int, P: int = 3000, K: int = 24, G: int = 12, labels=(3, 5, 7, 9, 14), invalid_labels=(1, 2),
                     void_frac: float = 0.15, min_inst: int = 20):
    """One synthetic scene for mask AP: per-point GT ids (label * 1000 + instance, 0 = unlabeled; a share of the void
    points carries an invalid label), K predicted masks that mostly cover one instance (a random 60-100 % of it plus
    scattered points; some cover two instances, some are pure noise), float32 scores and raw class ids (mostly the covered
    instance's label, some another valid one, a few an invalid one).  Returns numpy masks [P, K] bool, ids [P] int64,
    scores [K] float32, classes [K] int64."""
    rng = _rng(seed, f"instseg_ap/{P}/{K}/{G}")
    labels = np.asarray(labels, dtype=np.int64)
    n_void = int(P * void_frac)
    sizes = rng.dirichlet(np.full(G, 0.8)) * (P - n_void - G * min_inst)
    sizes = (np.floor(sizes).astype(np.int64) + min_inst) if G else np.zeros(0, np.int64)
    inst_ids = labels[rng.integers(0, len(labels), G)] * 1000 + rng.permutation(np.arange(1, 1000))[:G]
    ids = np.zeros(P, dtype=np.int64)
    pos = rng.permutation(P)
    o = 0
    for g in range(G):
        ids[pos[o:o + sizes[g]]] = inst_ids[g]
        o += int(sizes[g])
    rest = pos[o:]
    if len(invalid_labels) and len(rest):
        bad = rest[rng.random(len(rest)) < 0.4]
        ids[bad] = np.asarray(invalid_labels)[rng.integers(0, len(invalid_labels), len(bad))] * 1000 + rng.integers(1, 50, len(bad))
    masks = np.zeros((P, K), dtype=bool)
    classes = np.zeros(K, dtype=np.int64)
    for k in range(K):
        kind = rng.random()
        if G and kind < 0.85:
            tg = [rng.integers(0, G)] + ([rng.integers(0, G)] if kind > 0.75 else [])
            for g in tg:
                pts = np.nonzero(ids == inst_ids[g])[0]
                masks[pts[rng.random(len(pts)) < rng.uniform(0.6, 1.0)], k] = True
            masks[rng.integers(0, P, int(rng.integers(0, max(2, P // 50)))), k] = True
            lab = inst_ids[tg[0]] // 1000
            u = rng.random()
            classes[k] = lab if u < 0.75 else (labels[rng.integers(0, len(labels))] if u < 0.93 or not len(invalid_labels)
                                               else invalid_labels[0])
        else:
            masks[rng.integers(0, P, int(rng.integers(1, max(2, P // 10)))), k] = True
            classes[k] = labels[rng.integers(0, len(labels))]
    scores = rng.random(K).astype(np.float32)
    return masks, ids, scores, classes
