"""GPU: the train-time scene augmentation (pq3d_amd/scene.py augment_scenes, csrc/scene_augment.hip) against the numpy
restatement tests/scene_augment_ref.py.  Every comparison is BITWISE (torch.equal on the fp32 outputs) and every case runs
twice with identical results.  The coordinates are multiples of 2^-10 with |x| < 64, so every fp64 sum is exact in any order
(tests/test_scene_augment_ref.py checks that on the CPU) and the restatement alone fixes the bits; the colours are arbitrary
floats in [0, 256)."""
import functools

import numpy as np
import pytest
import torch

from tests import scene_augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _host(a):
    return torch.from_numpy(np.array(a))


@functools.lru_cache(maxsize=None)
def _scene(seed: int, n: int, span: float = 64.0):
    """(coordinates, colours) of a scene of n points: grid coordinates, colours anywhere in [0, 256)."""
    r = np.random.default_rng([seed, n])
    c = np.minimum(r.uniform(0, 256, (n, 3)).astype(F32), np.nextafter(F32(256), F32(0)))
    x, c = R.grid_points(r, n, span), c
    x.setflags(write=False); c.setflags(write=False)
    return x, c


def _rows(B, seed, stages=None):
    from pq3d_amd import scene
    kw = {} if stages is None else dict(stages=stages)
    return scene.draw_scene_augment(B, scene.SceneAugmentConfig(), np.random.default_rng(seed), **kw)


def _set(rows, b, name, value):
    from pq3d_amd import scene
    at, n = scene.AUG_FIELDS[name]
    rows[b, at:at + n] = torch.as_tensor(np.asarray(value, dtype=F32).reshape(n))


def _reference(scenes, rows, train=True):
    return [R.augment(x, c, R.unpack(rows[b].numpy()) if train else None) for b, (x, c) in enumerate(scenes)]


def _run(scenes, rows, train=True, skip=(), **kw):
    """augment_scenes twice (the runs must agree bit for bit, but for the scenes in ``skip``, whose outputs are unspecified);
    the outputs on the host and the error word."""
    from pq3d_amd import scene
    xs, cs = [_dev(x) for x, _ in scenes], [_dev(c) for _, c in scenes]
    prm = rows.to(DEV) if rows is not None else None
    runs = []
    for _ in range(2):
        xo, fo, err = scene.augment_scenes(xs, cs, prm, train=train, **kw)
        assert err.dtype == torch.int32 and tuple(err.shape) == (1,) and err.is_cuda
        assert len(xo) == len(fo) == len(scenes)
        runs.append((xo, fo, int(err)))
    for k, (a, b) in enumerate(zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1])):
        assert k % len(scenes) in skip or torch.equal(a, b), "two runs differ"
    assert runs[0][2] == runs[1][2]
    for b, (x, _) in enumerate(scenes):
        assert xo[b].dtype == fo[b].dtype == torch.float32 and tuple(xo[b].shape) == (len(x), 3) and tuple(fo[b].shape) == (len(x), 6)
    return [t.cpu() for t in xo], [t.cpu() for t in fo], runs[0][2]


def _check(scenes, rows, train=True, want_err=0, skip=()):
    xo, fo, err = _run(scenes, rows, train, skip)
    ref = _reference(scenes, rows, train)
    assert err == want_err == functools.reduce(lambda a, b: a | b, (r[2] for r in ref))
    for b, (rx, rf, _) in enumerate(ref):
        if b in skip:
            continue
        assert torch.equal(xo[b], torch.from_numpy(rx)), f"coordinates of scene {b} differ from the restatement"
        assert torch.equal(fo[b], torch.from_numpy(rf)), f"features of scene {b} differ from the restatement"
        assert torch.equal(fo[b][:, 3:], xo[b])
    return xo, fo


# sizes around the 4-point group, the wave and the 2048-point reduction block
@pytest.mark.parametrize("P", [1, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_one_scene_all_stages(P):
    _check([_scene(1, P)], _rows(1, P))


@pytest.mark.parametrize("stage", R.STAGES)
def test_each_stage_alone(stage):
    scenes = [_scene(2, 2049), _scene(3, 77)]
    rows = _rows(2, 5, stages=(stage,))
    for b in range(2):
        _set(rows, b, "flip", [1, b])
    xo, fo = _check(scenes, rows)
    if stage == "colour":
        assert all(torch.equal(xo[b], _host(scenes[b][0])) for b in range(2))
    else:                  # the colour columns are those of the evaluation path
        assert all(torch.equal(fo[b][:, :3], torch.from_numpy(R.augment(*scenes[b], None)[1][:, :3])) for b in range(2))
        assert not torch.equal(xo[0], _host(scenes[0][0]))


def test_evaluation_path_keeps_the_coordinates():
    scenes = [_scene(4, 2049), _scene(5, 3)]
    for rows in (None, _rows(2, 6)):                 # (params are ignored when train is false)
        xo, fo = _check(scenes, rows, train=False)
        for b in range(2):
            assert xo[b].numpy().tobytes() == scenes[b][0].tobytes()
    # other Normalize constants reach the kernel
    from pq3d_amd import scene
    mean, std = (0.5, 0.25, 0.125), (0.2, 0.3, 0.4)
    _, fo, _ = _run(scenes, None, train=False, color_mean=mean, color_std=std)
    for b in range(2):
        assert torch.equal(fo[b], torch.from_numpy(R.augment(*scenes[b], None, mean, std)[1]))
    assert scene.color_constants(mean, std).tobytes() == np.concatenate(R.color_constants(mean, std)).tobytes()


RAGGED = (1, 5, 4099, 61, 2049, 6, 130, 1002)       # every scene boundary off a multiple of 4; a tail of 1 point


def test_ragged_batch_equals_the_single_scene_calls():
    bounds = np.cumsum(RAGGED)
    assert all(b % 4 for b in bounds) and RAGGED[0] == 1 and max(RAGGED) > 2 * 2048
    scenes = [_scene(10 + b, n) for b, n in enumerate(RAGGED)]
    rows = _rows(8, 7)
    xo, fo = _check(scenes, rows)
    for b in range(8):
        x1, f1, err = _run([scenes[b]], rows[b:b + 1])
        assert err == 0 and torch.equal(x1[0], xo[b]) and torch.equal(f1[0], fo[b])


def test_unaligned_views_take_the_point_by_point_path():
    """Scenes handed over as views that start 12 bytes into a buffer (one scene: no concatenation realigns them)."""
    from pq3d_amd import scene
    x, c = _scene(6, 1030)
    bx, bc = _dev(np.concatenate([np.zeros((1, 3), F32), x])), _dev(np.concatenate([np.zeros((1, 3), F32), c]))
    assert bx[1:].data_ptr() % 16 != 0
    rows = _rows(1, 8)
    xo, fo, err = scene.augment_scenes([bx[1:]], [bc[1:]], rows.to(DEV))
    rx, rf, _ = R.augment(x, c, R.unpack(rows[0].numpy()))
    assert int(err) == 0 and torch.equal(xo[0].cpu(), torch.from_numpy(rx)) and torch.equal(fo[0].cpu(), torch.from_numpy(rf))


def test_room_of_100k_points():
    r = np.random.default_rng(12)
    room = np.array([8.0, 6.0, 3.0])
    x = r.random((100_000, 3)) * room
    face = r.integers(0, 5, 100_000)                                   # floor and four walls
    x[face == 0, 2] = 0; x[face == 1, 1] = 0; x[face == 2, 1] = room[1]; x[face == 3, 0] = 0; x[face == 4, 0] = room[0]
    x = (np.round((x + r.normal(0, 0.004, x.shape)) * 1024) / 1024).astype(F32)
    c = r.uniform(0, 255.99, x.shape).astype(F32)
    _check([(x, c)], _rows(1, 13))


def test_limits_flips_and_heavy_clipping():
    """Both flips, scale and rotations at their limits; one scene brightened until many colours clip at 255, one darkened
    until many clip at 0."""
    from pq3d_amd import scene
    cfg = scene.SceneAugmentConfig()
    scenes = [_scene(20, 3001), _scene(21, 2050)]
    rows = _rows(2, 9)
    for b, sgn in enumerate((1.0, -1.0)):
        _set(rows, b, "flip", [1, 1])
        _set(rows, b, "scale", [1 + cfg.scale_limit[0][b], 1 + cfg.scale_limit[1][1 - b], 1 + cfg.scale_limit[2][b]])
        _set(rows, b, "rot", np.stack([scene._rotation(axis, lim[b]) for axis, lim in cfg.rotations]))
        _set(rows, b, "alpha", 1 + sgn * 0.2)
        _set(rows, b, "beta255", sgn * 0.2 * 255)
        _set(rows, b, "shift", [sgn * 20, sgn * 20, -sgn * 20])
    _, fo = _check(scenes, rows)
    mean255, rstd255 = R.color_constants()
    top, bottom = torch.from_numpy((F32(255) - mean255) * rstd255), torch.from_numpy((F32(0) - mean255) * rstd255)
    assert int((fo[0][:, :2] == top[:2]).sum()) > 1000 and int((fo[1][:, :2] == bottom[:2]).sum()) > 1000


def test_error_word_coordinates():
    from pq3d_amd import scene
    for bad in (float("nan"), float("inf"), -float("inf")):
        scenes = [_scene(30, 500), tuple(a.copy() for a in _scene(31, 2100)), _scene(32, 9)]
        scenes[1][0][1234, 1] = bad
        for train in (True, False):
            _check(scenes, _rows(3, 14), train=train, want_err=1, skip=(1,))
    err = scene.augment_scenes([_dev(scenes[1][0])], [_dev(scenes[1][1])], None, train=False)[2]
    with pytest.raises(ValueError, match="augment_scenes: coordinates hold non-finite values"):
        scene.check_scene_augment(err)
    scene.check_scene_augment(scene.augment_scenes([_dev(scenes[0][0])], [_dev(scenes[0][1])], None, train=False)[2])


def test_error_word_colours_saturate():
    from pq3d_amd import scene
    for bad, sat in ((-1.0, 0), (256.0, 255), (float("nan"), 0), (float("inf"), 255), (-3e38, 0)):
        scenes = [_scene(33, 40), tuple(a.copy() for a in _scene(34, 2100))]
        scenes[1][1][2050, 2] = bad
        for train in (True, False):
            _check(scenes, _rows(2, 15, stages=("centre", "scale")), train=train, want_err=2)       # (saturated as the restatement says)
        fo = _run(scenes, None, train=False)[1]
        mean255, rstd255 = R.color_constants()
        assert fo[1][2050, 2] == torch.tensor((F32(sat) - mean255[2]) * rstd255[2])
    both = tuple(a.copy() for a in _scene(35, 70))
    both[0][3, 0], both[1][69, 1] = np.nan, 300.0
    err = scene.augment_scenes([_dev(both[0])], [_dev(both[1])], None, train=False)[2]
    assert int(err) == 3
    with pytest.raises(ValueError, match="coordinates hold non-finite values; colors hold"):
        scene.check_scene_augment(err)


def test_argument_errors():
    from pq3d_amd import _lib, scene
    x, c = _scene(40, 100)
    dx, dc, rows = _dev(x), _dev(c), _rows(1, 16).to(DEV)
    with pytest.raises(_lib.Pq3dError):
        scene.augment_scenes([_host(x)], [dc], rows)
    with pytest.raises(_lib.Pq3dError):
        scene.augment_scenes([dx], [_host(c)], rows)
    with pytest.raises(_lib.Pq3dError):
        scene.augment_scenes([dx], [dc], rows.cpu())
    with pytest.raises(_lib.Pq3dError):
        scene.augment_scenes([dx], [dc], rows, out=(torch.empty(100, 3), torch.empty(100, 6)))
    bad_calls = [
        lambda: scene.augment_scenes([dx.double()], [dc], rows),                        # dtype
        lambda: scene.augment_scenes([dx], [dc[:, :2]], rows),                          # shape
        lambda: scene.augment_scenes([dx], [dc[:50]], rows),                            # lengths differ
        lambda: scene.augment_scenes([dx], [dc, dc], rows),                             # one colours entry per scene
        lambda: scene.augment_scenes([dx[:0]], [dc[:0]], rows),                         # empty scene
        lambda: scene.augment_scenes([dx] * 9, [dc] * 9, _rows(9, 1).to(DEV)),          # more than 8 scenes
        lambda: scene.augment_scenes([dx], [dc], rows[:, :-1].contiguous()),            # params of the wrong width
        lambda: scene.augment_scenes([dx, dx], [dc, dc], rows),                         # one row per scene
        lambda: scene.augment_scenes([dx], [dc], rows.double()),
        lambda: scene.augment_scenes([dx], [dc], None, train=True),                     # training needs params
        lambda: scene.augment_scenes([dx], [dc], rows, out=(torch.empty(99, 3, device=DEV), torch.empty(100, 6, device=DEV))),
        lambda: scene.augment_scenes([dx], [dc], rows, out=(torch.empty(100, 3, device=DEV), torch.empty(100, 12, device=DEV)[:, ::2])),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    scene.augment_scenes([dx], [dc], None, train=False)                                 # (params may be None in evaluation)


def _graph_nodes_and_edges(graph):
    """(number of nodes, [(from, to)]) of the captured graph behind a torch.cuda.CUDAGraph(keep_graph=True), asked of the HIP
    runtime the process has loaded (hipGraphGetNodes / hipGraphGetEdges)."""
    import ctypes
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    g, n = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = n.value
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(n)) == 0
    src, dst = (ctypes.c_void_p * max(n.value, 1))(), (ctypes.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(n)) == 0
    return nodes, [(src[k], dst[k]) for k in range(n.value)]


def test_capture_replays_with_new_parameters():
    """augment_scenes(out=) under torch.cuda.graph: replayed with two parameter blocks copied into the static params, it
    equals the eager call each time; the captured graph is a plain chain (no node with two successors or predecessors)."""
    from pq3d_amd import scene
    scenes = [_scene(50, 2500), _scene(51, 333)]
    xs, cs = [_dev(x) for x, _ in scenes], [_dev(c) for _, c in scenes]
    P = sum(len(x) for x, _ in scenes)
    static_rows = _rows(2, 17).to(DEV)
    out = (torch.zeros(P, 3, device=DEV), torch.zeros(P, 6, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scene.augment_scenes(xs, cs, static_rows, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        xo, fo, err = scene.augment_scenes(xs, cs, static_rows, out=out)
    assert xo[0].data_ptr() == out[0].data_ptr() and fo[0].data_ptr() == out[1].data_ptr()
    nodes, edges = _graph_nodes_and_edges(graph)
    sources, targets = [a for a, _ in edges], [b for _, b in edges]
    assert nodes >= 2 and len(edges) == nodes - 1, f"{nodes} nodes and {len(edges)} edges are not a chain"
    assert len(set(sources)) == len(sources) and len(set(targets)) == len(targets), "the captured graph has parallel branches"
    graph.instantiate()
    for seed in (18, 19):
        rows = _rows(2, seed)
        static_rows.copy_(rows)
        for t in out:
            t.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        ex, ef, eerr = scene.augment_scenes(xs, cs, rows.to(DEV))
        assert int(err) == int(eerr) == 0
        for b, (rx, rf, _) in enumerate(_reference(scenes, rows)):
            assert torch.equal(xo[b], ex[b]) and torch.equal(fo[b], ef[b])
            assert torch.equal(xo[b].cpu(), torch.from_numpy(rx)) and torch.equal(fo[b].cpu(), torch.from_numpy(rf))


def _same(a, b, key):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            _same(x, y, key)
    elif a is None:
        assert b is None, key
    else:
        assert a.dtype == b.dtype and torch.equal(a, b), key


def test_prepare_instseg_batch_from_colours():
    from pq3d_amd import scene
    r = np.random.default_rng(60)
    scenes = [_scene(61, 3000, 2.0), _scene(62, 1501, 2.0)]
    xs, cs = [_dev(x) for x, _ in scenes], [_dev(c) for _, c in scenes]
    p2s = [_dev(r.integers(0, 40, len(x))) for x, _ in scenes]
    p2i = [_dev(r.integers(-1, 6, len(x))) for x, _ in scenes]
    sem = [_dev(r.integers(0, 9, len(x))) for x, _ in scenes]
    kw = dict(point2instance=p2i, point2semantic=sem, offline_mask_source="gt")
    rows = _rows(2, 20)
    for train in (True, False):
        ref = _reference(scenes, rows, train)
        want = scene.prepare_instseg_batch([_dev(rx) for rx, _, _ in ref], [_dev(rf) for _, rf, _ in ref], p2s, 0.02, 16, **kw)
        got = scene.prepare_instseg_batch(xs, None, p2s, 0.02, 16, colors=cs, augment=rows.to(DEV) if train else None, **kw)
        assert sorted(got) == sorted(want)
        for key in want:
            _same(got[key], want[key], key)
        assert train or all(torch.equal(a, b) for a, b in zip(got["raw_coordinates"], xs))
    # with neither new argument: what the call without them returns
    feats = [_dev(rf) for _, rf, _ in ref]
    a = scene.prepare_instseg_batch(xs, feats, p2s, 0.02, 16, **kw)
    b = scene.prepare_instseg_batch(xs, feats, p2s, 0.02, 16, colors=None, augment=None, **kw)
    for key in a:
        _same(a[key], b[key], key)
    # the error word arrives through the read of the table sizes
    bad = [cs[0], cs[1].clone()]
    bad[1][7, 0] = -1.0
    with pytest.raises(ValueError, match="prepare_instseg_batch: colors hold"):
        scene.prepare_instseg_batch(xs, None, p2s, 0.02, 16, colors=bad, augment=rows.to(DEV))
    with pytest.raises(ValueError, match="not both"):
        scene.prepare_instseg_batch(xs, feats, p2s, 0.02, 16, colors=cs)
    with pytest.raises(ValueError, match="augment needs colors"):
        scene.prepare_instseg_batch(xs, feats, p2s, 0.02, 16, augment=rows.to(DEV))
