"""GPU: instance-segmentation training targets from point ids (pq3d_amd/scene.py instance_targets / padded_instance_targets,
csrc/instance_targets.hip) against the numpy restatement tests/instance_targets_ref.py.  Every output is an integer or 0/1,
so every comparison is exact, and every case runs twice and must give identical bits."""
import numpy as np
import pytest
import torch

from pq3d_amd.scene import INSTANCE_MAX_IDS as CAP
from tests import instance_targets_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("instance_ids", "instance_labels", "segment_masks", "full_masks")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).to(DEV)


def _scene(seed, P, S, ids, classes=(0, 1, 2, 3, 7, -100), mixed=0.3):
    """P points over the instance ids `ids` (-1 may be among them) and S segments (the largest one present); an instance's
    points mostly carry its own class, a share `mixed` of them another one, so the first occurrence matters."""
    r = np.random.default_rng([seed, P, S])
    ids = np.asarray(ids, dtype=np.int64)
    which = r.integers(0, len(ids), P)
    p2i = ids[which]
    own = r.choice(classes, len(ids))
    sem = np.where(r.random(P) < mixed, r.choice(classes, P), own[which]).astype(np.int64)
    seg = r.integers(0, S, P).astype(np.int64)
    seg[r.integers(0, P)] = S - 1
    return p2i, sem, seg


def _run(scenes, **kw):
    from pq3d_amd import scene
    return scene.instance_targets(*[[_dev(s[k]) for s in scenes] for k in range(3)], **kw)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or all(torch.equal(x, y) for x, y in zip(a[k], b[k])) for k in KEYS)


def _check(scenes, filter_out_classes=(0, 2)):
    """List form against the restatement, twice.  Returns the restatement."""
    got = _run(scenes, filter_out_classes=filter_out_classes)
    assert _same(got, _run(scenes, filter_out_classes=filter_out_classes)), "two runs differ"
    want = R.batch_targets(*[[s[k] for s in scenes] for k in range(3)], filter_out_classes)
    for b in range(len(scenes)):
        for k in KEYS:
            g, w = got[k][b], want[k][b]
            assert g.dtype == (torch.int64 if k in KEYS[:2] else torch.bool) and tuple(g.shape) == w.shape, (k, b, g.shape, w.shape)
            assert np.array_equal(g.cpu().numpy(), w), f"{k} of scene {b} differs"
    return want


def _pad_ref(want, Ns, Nt):
    from pq3d_amd.losses import SetCriterion
    return SetCriterion.pad_targets([torch.from_numpy(l) for l in want["instance_labels"]],
                                    [torch.from_numpy(m) for m in want["segment_masks"]], Ns, Nt)


def _padded(scenes, Ns, Nt, **kw):
    from pq3d_amd import scene
    return scene.padded_instance_targets(*[[_dev(s[k]) for s in scenes] for k in range(3)], Ns, Nt, **kw)


def _check_padded(scenes, Ns, Nt, want=None, out=None):
    from pq3d_amd.losses import PaddedTargets
    want = want or R.batch_targets(*[[s[k] for s in scenes] for k in range(3)])
    ref = _pad_ref(want, Ns, Nt)
    got, err = _padded(scenes, Ns, Nt, out=out)
    assert out is None or got is out
    assert err.dtype == torch.int32 and int(err) == 0
    for k in PaddedTargets.__slots__:
        g, w = getattr(got, k), getattr(ref, k)
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"{k} differs from SetCriterion.pad_targets"
    again, _ = _padded(scenes, Ns, Nt)
    assert all(torch.equal(getattr(got, k), getattr(again, k)) for k in PaddedTargets.__slots__), "two runs differ"
    return got


# ------------------------------------------------------------------------------------------------------------ list form
@pytest.mark.parametrize("P,S", [(1, 1), (255, 3), (256, 65), (257, 130), (5000, 130)])
def test_one_scene_sizes(P, S):
    want = _check([_scene(1, P, S, [-1, 0, 1, 2, 5, 9, 11])])
    _check_padded([_scene(1, P, S, [-1, 0, 1, 2, 5, 9, 11])], S + 3, 9, want)


def test_ragged_batch_with_a_one_point_scene():
    scenes = [_scene(2, 5000, 65, [-1, 0, 3, 4, 8]), _scene(3, 1, 1, [6], classes=(5,)), _scene(4, 257, 3, [0, 1, 2, 3])]
    want = _check(scenes)
    assert [len(i) for i in want["instance_ids"]][1] == 1
    _check_padded(scenes, 65, 6, want)


def test_eight_scenes():
    scenes = [_scene(10 + b, [255, 256, 257, 1, 700, 64, 65, 1300][b], [1, 3, 65, 1, 130, 3, 3, 65][b], list(range(-1, 3 + 2 * b)))
              for b in range(8)]
    want = _check(scenes)
    _check_padded(scenes, 130, 20, want)


@pytest.mark.parametrize("G", [63, 65, 300])
def test_instance_counts_across_wave_and_workgroup_boundaries(G):
    s = _scene(G, 5000, 65, np.arange(-1, G), classes=(1, 3, 7, 9), mixed=0.0)
    want = _check([s])
    assert len(want["instance_ids"][0]) == G
    _check_padded([s], 65, G, want)                      # max_instances exactly G, Ns exactly S


def test_ids_with_gaps_up_to_the_cap():
    ids = [0, 5, 63, 64, 65, 1000, 1023, 1024, 1025, CAP - 2, CAP - 1]
    want = _check([_scene(5, 3000, 65, ids, classes=(1, 3)), _scene(6, 300, 3, [-1, CAP - 1], classes=(4,))])
    assert want["instance_ids"][0].tolist() == ids and want["instance_ids"][1].tolist() == [CAP - 1]


def test_only_unlabelled_none_unlabelled_and_everything_filtered():
    only = _scene(7, 700, 3, [-1])
    none = _scene(8, 700, 3, [0, 1, 2], classes=(1, 3), mixed=0.0)
    filtered = _scene(9, 700, 65, [-1, 0, 1, 2, 3], classes=(0, 2), mixed=0.0)
    want = _check([only, filtered, none])
    assert [len(i) for i in want["instance_ids"]] == [0, 0, 3]
    assert want["segment_masks"][1].shape == (0, 65) and want["full_masks"][0].shape == (0, 700)
    _check_padded([only, filtered, none], 65, 4, want)
    _check([only])
    _check([filtered], filter_out_classes=())            # nothing filtered: the four instances appear
    _check([none], filter_out_classes=(1, 3))


def test_first_occurrence_decides_label_and_filter():
    """Instances whose points carry mixed labels: the first point's label inside / outside filter_out_classes."""
    P = 1200
    r = np.random.default_rng(11)
    p2i = r.integers(0, 4, P).astype(np.int64)
    seg = r.integers(0, 9, P).astype(np.int64)
    sem = np.full(P, 5, dtype=np.int64)
    first = [int(np.flatnonzero(p2i == i)[0]) for i in range(4)]
    sem[first[0]] = 2                                    # instance 0: first label filtered, every other point 5 -> dropped
    sem[p2i == 1] = 0
    sem[first[1]] = 6                                    # instance 1: first label 6, every other point filtered -> kept, label 6
    sem[np.flatnonzero(p2i == 2)[1:]] = r.choice([0, 2, 5, 8], (p2i == 2).sum() - 1)     # instance 2: first label 5 -> kept
    want = _check([(p2i, sem, seg)])
    assert want["instance_ids"][0].tolist() == [1, 2, 3] and want["instance_labels"][0].tolist() == [6, 5, 5]
    _check_padded([(p2i, sem, seg)], 9, 3, want)


def test_contention_counts_each_cell_once():
    """5000 points in 3 instances x 2 segments: every mask cell has hundreds of writers."""
    r = np.random.default_rng(12)
    p2i, seg = r.integers(0, 3, 5000).astype(np.int64), r.integers(0, 2, 5000).astype(np.int64)
    s = (p2i, np.full(5000, 4, dtype=np.int64), seg)
    want = _check([s])
    assert want["segment_masks"][0].all()
    got = _check_padded([s], 2, 3, want)
    assert got.t_sum.tolist() == [[2.0, 2.0, 2.0]] and got.T.sum().item() == 6.0


def test_shared_segments_and_an_instance_spanning_every_segment():
    r = np.random.default_rng(13)
    P, S = 4000, 130
    p2i = r.integers(-1, 6, P).astype(np.int64)
    seg = r.integers(0, S, P).astype(np.int64)
    seg[p2i == 3] = 7                                    # instance 3 lives in one segment, which 0, 1, 2 and 4 share
    for i in (0, 1, 2, 4):
        seg[np.flatnonzero(p2i == i)[0]] = 7
    span = np.flatnonzero(p2i == 5)
    seg[span[:S]] = np.arange(S)                         # instance 5 spans every segment
    want = _check([(p2i, np.full(P, 1, dtype=np.int64), seg)])
    m = want["segment_masks"][0]
    assert m[5].all() and m[3].sum() == 1 and m[:, 7].all()
    _check_padded([(p2i, np.full(P, 1, dtype=np.int64), seg)], S, 6, want)


def test_without_full_masks():
    s = _scene(14, 900, 65, [-1, 0, 1, 2])
    got = _run([s], with_full_masks=False)
    want = R.batch_targets([s[0]], [s[1]], [s[2]])
    assert got["full_masks"] is None and np.array_equal(got["segment_masks"][0].cpu().numpy(), want["segment_masks"][0])


# ---------------------------------------------------------------------------------------------------------- padded form
def test_padded_out_overwrites_garbage():
    from pq3d_amd.losses import PaddedTargets
    scenes = [_scene(15, 2000, 65, [-1, 0, 1, 4, 6, 7]), _scene(16, 300, 3, [0, 2])]
    B, Ns, Nt = 2, 70, 8
    out = PaddedTargets(torch.full((B, Nt, Ns), 7.5, device=DEV), torch.full((B, Nt), -3, dtype=torch.int64, device=DEV),
                        torch.full((B,), 99, dtype=torch.int32, device=DEV), torch.full((B,), 99, dtype=torch.int32, device=DEV),
                        torch.full((B, Nt), float("nan"), device=DEV))
    _check_padded(scenes, Ns, Nt, out=out)
    _check_padded(scenes[::-1], Ns, Nt, out=out)         # and again over the previous batch's values


def test_padded_wrong_out_shapes_raise():
    from pq3d_amd.losses import PaddedTargets
    s = _scene(17, 100, 3, [0, 1])
    out = PaddedTargets(torch.zeros(1, 4, 5, device=DEV), torch.zeros(1, 4, dtype=torch.int64, device=DEV),
                        torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                        torch.zeros(1, 4, device=DEV))
    with pytest.raises(ValueError, match="out.T"):
        _padded([s], 6, 4, out=out)


# --------------------------------------------------------------------------------------------------------------- errors
def _with(s, k, at, value):
    a = [x.copy() for x in s]
    a[k][at] = value
    return tuple(a)


def _others_intact(scenes, bad, Ns, Nt, bit):
    """Padded form on a batch whose scene `bad` holds an illegal value: the error word has `bit`, the other scenes' rows equal
    the restatement."""
    from pq3d_amd import scene
    from pq3d_amd.losses import PaddedTargets
    got, err = _padded(scenes, Ns, Nt)
    assert int(err) & bit, int(err)
    with pytest.raises(ValueError):
        scene.check_instance_targets(err)
    good = [b for b in range(len(scenes)) if b != bad]
    ref = _pad_ref(R.batch_targets(*[[scenes[b][k] for b in good] for k in range(3)]), Ns, Nt)
    for k in PaddedTargets.__slots__:
        assert torch.equal(getattr(got, k)[good], getattr(ref, k)), f"{k} of the other scenes is corrupted"
    return got, int(err)


def test_bad_instance_ids_raise_and_leave_the_batch_intact():
    scenes = [_scene(20, 900, 9, [-1, 0, 1, 2]), _scene(21, 700, 9, [-1, 0, 1, 4, 5]), _scene(22, 300, 3, [0, 3])]
    for bad in (-2, CAP, 2 ** 62, -2 ** 62):
        broken = [scenes[0], _with(scenes[1], 0, 350, bad), scenes[2]]
        with pytest.raises(ValueError, match="point2instance"):
            _run(broken)
        got, err = _others_intact(broken, 1, 9, 6, 1)
        assert err == 1
        # the offending point is skipped: the scene equals the restatement without it
        rest = tuple(np.delete(a, 350) for a in scenes[1])
        ref = _pad_ref(R.batch_targets([rest[0]], [rest[1]], [rest[2]]), 9, 6)
        assert torch.equal(got.T[1], ref.T[0]) and torch.equal(got.labels[1], ref.labels[0]) and torch.equal(got.t_sum[1], ref.t_sum[0])
    _check([_with(scenes[1], 0, 350, CAP - 1)])          # the largest legal id


def test_bad_segments_raise_and_leave_the_batch_intact():
    scenes = [_scene(23, 900, 9, [-1, 0, 1, 2]), _scene(24, 700, 9, [-1, 0, 1, 4, 5]), _scene(25, 300, 3, [0, 3])]
    for bad in (-1, -2 ** 62, 2 ** 62):
        broken = [scenes[0], scenes[1], _with(scenes[2], 2, 17, bad)]
        with pytest.raises(ValueError, match="point2segment"):
            _run(broken)
        assert _others_intact(broken, 2, 9, 6, 2)[1] == 2


def test_extreme_semantic_labels_are_legal():
    s = _scene(26, 500, 3, [0, 1, 2], classes=(1,), mixed=0.0)
    first = [int(np.flatnonzero(s[0] == i)[0]) for i in range(3)]
    s = _with(_with(s, 1, first[0], 2 ** 62), 1, first[2], -2 ** 62)
    want = _check([s])
    assert want["instance_labels"][0].tolist() == [2 ** 62, 1, -2 ** 62]
    _check_padded([s], 3, 3, want)


def test_padded_more_segments_than_ns_and_more_instances_than_max():
    scenes = [_scene(27, 900, 8, [-1, 0, 1, 2]), _scene(28, 700, 10, [-1, 0, 1, 4, 5, 6], classes=(1, 3, 7)), _scene(29, 300, 3, [0, 3])]
    got, err = _others_intact(scenes, 1, 8, 6, 2)                       # S = 10 > Ns = 8
    assert err == 2 and int(got.seg_len[1]) == 8
    got, err = _others_intact(scenes, 1, 10, 3, 4)                      # G = 5 > max_instances = 3
    assert err == 4 and int(got.n_inst_dev[1]) == 3
    want = R.batch_targets(*[[scenes[1][k]] for k in range(3)])
    assert torch.equal(got.labels[1].cpu(), torch.from_numpy(want["instance_labels"][0][:3]))
    assert np.array_equal(got.T[1].cpu().numpy(), want["segment_masks"][0][:3].astype(np.float32))
    _check_padded(scenes, 10, 5)                                       # exactly enough of both: no error


def test_argument_errors_and_cpu_tensors():
    from pq3d_amd import _lib, scene
    s = _scene(30, 50, 3, [0, 1])
    d = [[_dev(s[k])] for k in range(3)]
    c = [[torch.from_numpy(s[k])] for k in range(3)]
    with pytest.raises(_lib.Pq3dError):
        scene.instance_targets(*c)
    with pytest.raises(_lib.Pq3dError):
        scene.padded_instance_targets(*c, 3, 2)
    with pytest.raises(_lib.Pq3dError):
        scene.instance_targets(d[0], c[1], d[2])
    with pytest.raises(ValueError):
        scene.instance_targets(d[0] * 9, d[1] * 9, d[2] * 9)
    with pytest.raises(ValueError):
        scene.instance_targets(d[0], d[1], [d[2][0][:10]])
    with pytest.raises(ValueError):
        scene.instance_targets(d[0], d[1], [d[2][0].int()])
    with pytest.raises(ValueError):
        scene.padded_instance_targets(*d, 0, 2)
    with pytest.raises(ValueError):
        scene.padded_instance_targets(*d, 3, CAP + 1)
    with pytest.raises(ValueError):
        scene.instance_targets(*d, filter_out_classes=tuple(range(17)))
    import pq3d_amd
    assert pq3d_amd.instance_targets is scene.instance_targets and pq3d_amd.padded_instance_targets is scene.padded_instance_targets
