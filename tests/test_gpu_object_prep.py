"""pq3d_amd/objects.py + csrc/object_prep.hip against the numpy restatement tests/object_prep_ref.py, bit for bit: the object
bank (ids and masks forms), match_boxes, sample_objects (eager and under a captured graph), ground_labels, and a
prepare_grounding_batch output through a tiny stage-2 Query3DUnified."""
import numpy as np
import pytest
import torch

from pq3d_amd.objects import CHUNK      # points per (row, chunk) cell of the bank build
from tests import object_prep_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    want = np.asarray(want)
    g = _bits(got)
    assert g.shape == want.shape, (g.shape, want.shape)
    assert np.array_equal(g, want.view(np.int32) if want.dtype == np.float32 else want)


def _points(rng, P):
    """[P, 6] fp32 rows; the red channel carries the point's index, so a feature row names the point it was gathered from."""
    xyz = (rng.random((P, 3)) * np.array([6.0, 5.0, 2.5]) - np.array([3.0, 2.5, 0.0])).astype(np.float32)
    return np.concatenate([xyz, np.arange(P, dtype=np.float32)[:, None], rng.random((P, 2)).astype(np.float32)], 1)


def _scan(rng, sizes, background, degenerate=None):
    """A scan whose instance k has sizes[k] points scattered over the scan (ids 10 * k + 3), `background` points of id -1."""
    P = sum(sizes) + background
    ids = np.concatenate([np.full(n, 10 * k + 3) for k, n in enumerate(sizes)] + [np.full(background, -1)]).astype(np.int64)
    ids = ids[rng.permutation(P)]
    pts = _points(rng, P)
    if degenerate is not None:
        pts[ids == 10 * degenerate + 3, :3] = np.array([1.5, -2.0, 0.25], dtype=np.float32)
    return pts, ids, np.array([10 * k + 3 for k in range(len(sizes))], dtype=np.int64)


SIZES0 = [1, 63, 64, 65, 127, 129, 1023, 1024, 1025, 40]        # object 9: all points equal
SIZES1 = [200, 70]


@pytest.fixture(scope="module")
def banks():
    from pq3d_amd import objects as OB
    rng = np.random.default_rng(5)
    s0, s1 = _scan(rng, SIZES0, 150, degenerate=9), _scan(rng, SIZES1, 30)
    pts, p2i, ids = [s0[0], s1[0]], [s0[1], s1[1]], [s0[2], s1[2]]
    ref = R.build_object_bank(pts, point2instance=p2i, instance_ids=ids)
    bank = OB.build_object_bank([_t(p) for p in pts], point2instance=[_t(p) for p in p2i], instance_ids=[_t(i) for i in ids])
    return bank, ref


def _check_bank(bank, ref):
    _same(bank.order, ref["order"])
    _same(bank.entry_offsets, ref["entry_offsets"])
    _same(bank.object_offsets, ref["object_offsets"].astype(np.int32))
    _same(bank.source_row, ref["source_row"])
    _same(bank.box_center, ref["box_center"])
    _same(bank.box_size, ref["box_size"])
    assert bank.num_objects == np.diff(ref["object_offsets"]).tolist()
    for o in range(len(ref["source_row"])):
        seg = ref["order"][ref["entry_offsets"][o]:ref["entry_offsets"][o + 1]]
        assert (np.diff(seg) > 0).all()


def test_bank_ids_form_chunk_edges_dropped_rows_two_scans(banks):
    from pq3d_amd import objects as OB
    _check_bank(*banks)                                          # scattered objects of 1 .. 1025 points, two scans
    # contiguous runs that straddle the CHUNK boundaries: objects of CHUNK - 1, CHUNK, CHUNK + 1 and 1 points starting
    # at point 700; id 77 has no point (dropped), the second scan is smaller than one chunk
    rng = np.random.default_rng(6)
    runs = [(5, 700), (11, CHUNK - 1), (12, CHUNK), (13, CHUNK + 1), (14, 1), (5, 9)]
    p2i0 = np.concatenate([np.full(n, i) for i, n in runs]).astype(np.int64)
    ids0 = np.array([14, 77, 13, 11, 5, 12], dtype=np.int64)
    p2i1 = rng.integers(-1, 4, 333).astype(np.int64)
    ids1 = np.array([2, 9, 0], dtype=np.int64)
    pts = [_points(rng, len(p2i0)), _points(rng, 333)]
    ref = R.build_object_bank(pts, point2instance=[p2i0, p2i1], instance_ids=[ids0, ids1])
    bank = OB.build_object_bank([_t(p) for p in pts], point2instance=[_t(p2i0), _t(p2i1)], instance_ids=[_t(ids0), _t(ids1)])
    _check_bank(bank, ref)
    assert ref["source_row"].tolist() == [0, 2, 3, 4, 5, 0, 2] and bank.num_objects == [5, 2]
    again = OB.build_object_bank([_t(p) for p in pts], point2instance=[_t(p2i0), _t(p2i1)], instance_ids=[_t(ids0), _t(ids1)])
    assert torch.equal(again.order, bank.order) and torch.equal(again.box_center, bank.box_center)


def test_bank_masks_form_overlap_empty_and_full_rows():
    from pq3d_amd import objects as OB
    rng = np.random.default_rng(7)
    P0, P1 = 2 * CHUNK + 37, 90
    m0 = rng.random((5, P0)) < 0.3
    m0[1] = False
    m0[3] = True
    m0[4] = m0[0] | (rng.random(P0) < 0.1)                       # overlaps row 0
    m1 = rng.random((2, P1)) < 0.5
    pts = [_points(rng, P0), _points(rng, P1)]
    ref = R.build_object_bank(pts, masks=[m0, m1])
    bank = OB.build_object_bank([_t(p) for p in pts], masks=[_t(m0), _t(m1)])
    _check_bank(bank, ref)
    assert ref["source_row"].tolist() == [0, 2, 3, 4, 0, 1]
    full = ref["order"][ref["entry_offsets"][2]:ref["entry_offsets"][3]]
    assert np.array_equal(full, np.arange(P0))


def test_match_boxes_lattice_ties_epsilon_and_no_predictions():
    from pq3d_amd import objects as OB
    f = lambda rows: np.array(rows, dtype=np.float32)
    gc = f([[0, 0, 0], [4, 4, 4], [0.125, 0.25, -0.375], [10, 10, 10]])
    gs = f([[1, 1, 1], [2, 2, 2], [0.75, 1.5, 0.25], [1, 1, 1]])
    pc = f([[0, 0, 0.25], [0, 0, 0], [0, 0, 0], [4, 4, 4], [4, 4, 4], [0.25, 0.25, -0.25], [-20, 0, 0], [0, 0, 0.125]])
    ps = f([[1, 1, 0.5], [1, 1, 1], [1, 1, 1], [1, 1, 1], [4, 4, 4], [1, 1.5, 0.5], [1, 1, 1], [1, 1, 0.75]])
    want = R.match_boxes(gc, gs, pc, ps)
    got = OB.match_boxes(_t(gc), _t(gs), _t(pc), _t(ps))
    for g, w in zip(got, want):
        _same(g, w)
    matched, i25, i50 = want
    # GT 0 against prediction 0: intersection 0.5, union 1: exactly 0.5 without the epsilon, so it reads False
    assert i25[0, 0] == 1 and i50[0, 0] == 0
    assert matched[0] == 1 and i50[0, 1] == 1 and i50[0, 2] == 1          # identical boxes 1 and 2: the first wins
    # nested both ways, 1/8 each before the epsilon: 1 / (8 + 1e-8) for the inner box, 8 / (64 + 1e-8) for the outer, which is larger
    assert matched[1] == 4 and i25[1, 3] == 0 and i25[1, 4] == 0
    assert matched[3] == 0 and not i25[3].any()                           # disjoint from everything: IoU 0 > -1 at index 0
    m0, a0, b0 = OB.match_boxes(_t(gc), _t(gs), _t(pc[:0]), _t(ps[:0]))
    assert m0.tolist() == [-1] * 4 and tuple(a0.shape) == (4, 0) == tuple(b0.shape)


SOI = np.array([0, 1, 0, 0], dtype=np.int32)
SEL64 = np.array([[0, 1, 2], [1, -1, 0], [3, 4, 5], [9, 8, -1]], dtype=np.int32)      # n = 1, 63, 64 | 70, pad, 200 | 65, 127, 129 | equal, 1025


def _rotation(rng, B):
    out = []
    for _ in range(B):
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        out.append(q)
    return np.array(out, dtype=np.float32)


def _check_sample(bank, ref, soi, sel, n, seed, rot):
    from pq3d_amd import objects as OB
    d, err = OB.sample_objects(bank, _t(soi), _t(sel), num_points=n, seed=torch.tensor([seed], dtype=torch.int64, device=DEV),
                               rotation=None if rot is None else _t(rot))
    fts, locs, boxes, pad, e, idx = R.sample_objects(ref, soi, sel, num_points=n, seed=seed, rotation=rot, return_indices=True)
    assert int(err) == e == 0
    OB.check_objects(err)
    _same(d["obj_pad_masks"], pad)
    _same(d["obj_locs"], locs)
    _same(d["obj_boxes"], boxes)
    _same(d["obj_fts"], fts)
    got = d["obj_fts"].cpu().numpy()
    assert np.isfinite(got).all() and (got[~pad] == 0).all()
    for b in range(sel.shape[0]):
        for q in range(sel.shape[1]):
            if not pad[b, q]:
                continue
            o = ref["object_offsets"][soi[b]] + sel[b, q]
            members = ref["order"][ref["entry_offsets"][o]:ref["entry_offsets"][o + 1]]
            drawn = got[b, q, :, 3].astype(np.int64)                         # the point index rides in the red channel
            assert np.array_equal(drawn, idx[b, q]) and np.isin(drawn, members).all()
            if len(members) >= n:
                assert len(np.unique(drawn)) == n
    return got


@pytest.mark.parametrize("rotated", [False, True])
def test_sample_objects_equals_restatement(banks, rotated):
    bank, ref = banks
    rot = _rotation(np.random.default_rng(8), 4) if rotated else None
    a = _check_sample(bank, ref, SOI, SEL64, 64, 2024, rot)
    assert (a[3, 0, :, :3] == 0).all()                           # the degenerate object: the 1e-6 clamp, no NaN
    b = _check_sample(bank, ref, SOI, SEL64, 64, 2024, rot)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))    # the same seed: the same bits
    c = _check_sample(bank, ref, SOI, SEL64, 64, 2025, rot)
    assert not np.array_equal(a[3, 1, :, 3], c[3, 1, :, 3]) and not np.array_equal(a[1, 2, :, 3], c[1, 2, :, 3])


def test_sample_objects_1024_points_and_odd_count(banks):
    bank, ref = banks
    sel = np.array([[6, 7, 8], [0, 1, -1]], dtype=np.int32)      # n = 1023, 1024, 1025 | 200, 70
    soi = np.array([0, 1], dtype=np.int32)
    _check_sample(bank, ref, soi, sel, 1024, 99, _rotation(np.random.default_rng(9), 2))
    _check_sample(bank, ref, soi, sel, 63, 99, None)             # an odd num_points takes the unvectorised stores


def test_errors_host_checks_and_error_word(banks):
    from pq3d_amd import objects as OB
    from pq3d_amd._lib import Pq3dError
    bank, ref = banks
    seed = torch.tensor([1], dtype=torch.int64, device=DEV)
    soi, sel = _t(SOI), _t(SEL64)
    with pytest.raises(Pq3dError, match="^sample_objects"):
        OB.sample_objects(bank, soi.cpu(), sel, num_points=64, seed=seed)
    with pytest.raises(Pq3dError, match="^build_object_bank"):
        OB.build_object_bank([torch.zeros(4, 6)], masks=[torch.ones(1, 4, dtype=torch.bool)])
    with pytest.raises(Pq3dError, match="^match_boxes"):
        OB.match_boxes(torch.zeros(1, 3), torch.zeros(1, 3), torch.zeros(1, 3), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="^sample_objects: need 1 <= num_points"):
        OB.sample_objects(bank, soi, sel, num_points=OB.MAX_SAMPLE + 1, seed=seed)
    with pytest.raises(ValueError, match="^sample_objects: seed"):
        OB.sample_objects(bank, soi, sel, num_points=64, seed=seed.int())
    with pytest.raises(ValueError, match="^build_object_bank: at most 1024 object rows"):
        OB.build_object_bank([torch.zeros(4, 6, device=DEV)], masks=[torch.ones(OB.MAX_ROWS + 1, 4, dtype=torch.bool, device=DEV)])
    with pytest.raises(ValueError, match="^build_object_bank: at most 1048576 points"):
        big = torch.zeros(OB.MAX_POINTS + 1, 6, device=DEV)
        OB.build_object_bank([big], masks=[torch.ones(1, OB.MAX_POINTS + 1, dtype=torch.bool, device=DEV)])
    # out-of-range entries only fail the range check: they are never used as an index
    for bad_soi, bad_sel, bit in ((np.array([0, 2, 0, -1], dtype=np.int32), SEL64, R.ERR_SCENE),
                                  (SOI, np.where(SEL64 == 4, 10, np.where(SEL64 == 1, -2, SEL64)).astype(np.int32), R.ERR_SELECTED)):
        d, err = OB.sample_objects(bank, _t(bad_soi), _t(bad_sel), num_points=64, seed=seed)
        fts, locs, boxes, pad, e = R.sample_objects(ref, bad_soi, bad_sel, num_points=64, seed=1)
        assert int(err) == e == bit
        _same(d["obj_fts"], fts)
        _same(d["obj_pad_masks"], pad)
        with pytest.raises(ValueError, match="^sample_objects: "):
            OB.check_objects(err)


def test_sample_objects_replays_with_a_new_seed_under_a_captured_graph(banks):
    from pq3d_amd import objects as OB
    bank, ref = banks
    soi, sel = _t(SOI), _t(SEL64)
    seed = torch.tensor([40], dtype=torch.int64, device=DEV)
    OB.sample_objects(bank, soi, sel, num_points=64, seed=seed)                 # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d, err = OB.sample_objects(bank, soi, sel, num_points=64, seed=seed)
    draws = []
    for s in (41, 42):
        seed.fill_(s)
        g.replay()
        torch.cuda.synchronize()
        fts, locs, boxes, pad, e = R.sample_objects(ref, SOI, SEL64, num_points=64, seed=s)
        assert int(err) == 0
        _same(d["obj_fts"], fts)
        _same(d["obj_locs"], locs)
        _same(d["obj_pad_masks"], pad)
        draws.append(d["obj_fts"].cpu().numpy().copy())
    assert not np.array_equal(draws[0][2, 2, :, 3], draws[1][2, 2, :, 3])


def test_ground_labels_gt_and_pred_forms(banks):
    from pq3d_amd import objects as OB
    bank, ref = banks
    tg = np.array([[2, 0, -1], [0, -1, -1], [5, 5, 3], [7, -1, -1]], dtype=np.int32)       # item 3: its target is not selected
    got = OB.ground_labels(bank, _t(SOI), _t(SEL64), _t(tg))
    want = R.ground_labels(ref["object_offsets"], SOI, SEL64, tg)
    for g, w in zip(got[:3], want[:3]):
        _same(g, w)
    assert int(got[3]) == want[3] == 0 and want[0].tolist() == [[1, 0, 1], [0, 0, 1], [1, 0, 1], [0, 0, 0]]
    # pred form: predictions = masks over the same two scans; targets index the GT bank
    rng = np.random.default_rng(10)
    pts = [ref["points"][ref["point_offsets"][s]:ref["point_offsets"][s + 1]] for s in range(2)]
    masks = []
    for s, K in ((0, 6), (1, 3)):
        x = pts[s][:, 0]
        lo = np.linspace(-3, 3, K + 1)
        m = np.stack([(x >= lo[k] - 0.5) & (x < lo[k + 1] + 0.5) for k in range(K)])
        masks.append(m)
    # two predictions that reproduce GT objects of scan 0: IoU 1 rows besides the weak slab overlaps
    g7 = ref["order"][ref["entry_offsets"][7]:ref["entry_offsets"][8]]
    masks[0][2] = False
    masks[0][2, g7] = True
    pred = OB.build_object_bank([_t(p) for p in pts], masks=[_t(m) for m in masks])
    pref = R.build_object_bank(pts, masks=masks)
    mt = OB.match_banks(bank, pred)
    mref = [R.match_boxes(ref["box_center"][a:b], ref["box_size"][a:b], pref["box_center"][c:d], pref["box_size"][c:d])
            for (a, b), (c, d) in zip(zip(ref["object_offsets"][:-1], ref["object_offsets"][1:]),
                                      zip(pref["object_offsets"][:-1], pref["object_offsets"][1:]))]
    assert mref[0][0][7] == 2 and mref[0][2][7, 2] == 1
    sel = np.array([[0, 2, 5], [2, -1, 0], [1, 3, 4], [0, 1, -1]], dtype=np.int32)
    tgp = np.array([[7, 8, -1], [1, 0, -1], [7, -1, -1], [6, 9, 0]], dtype=np.int32)       # item 2: matched 2 is not selected
    got = OB.ground_labels(pred, _t(SOI), _t(sel), _t(tgp), match=mt)
    want = R.ground_labels(pref["object_offsets"], SOI, sel, tgp, match=mref)
    for g, w in zip(got[:3], want[:3]):
        _same(g, w)
    assert int(got[3]) == want[3] == 0 and want[0][0, 1] == 1 and want[0][2].sum() == 0 and want[1].sum() > want[2].sum() > 0
    bad = tgp.copy()
    bad[0, 0] = 10                                               # scan 0 has 10 GT objects
    got = OB.ground_labels(pred, _t(SOI), _t(sel), _t(bad), match=mt)
    want = R.ground_labels(pref["object_offsets"], SOI, sel, bad, match=mref)
    assert int(got[3]) == want[3] == R.ERR_TARGET
    _same(got[0], want[0])
    with pytest.raises(ValueError, match="^sample_objects: targets"):
        OB.check_objects(got[3])


def test_prepare_grounding_batch_drives_a_stage2_model(banks):
    from pq3d_amd import objects as OB, synth
    from pq3d_amd.model import Query3DUnified, make_cfg
    from pq3d_amd.modules import ObjectEncoder, set_compute
    bank, ref = banks
    d, T, n = 64, 6, 64
    mem = ["mv", "pc", "voxel", "prompt"]
    model = Query3DUnified(make_cfg(d=d, H=4, L=2, memories=mem, heads=["ground"], structure="mixed", d_in={"mv": 32, "pc": 768, "voxel": 48}),
                           compute="fp32")
    model.pc_encoder = ObjectEncoder(None, backbone="pointnet++", freeze_backbone=True, input_feat_size=768, hidden_size=d,
                                     use_projection=True, use_cls_head=False, dropout=0.0)
    set_compute(model, "fp32")
    synth.fill_module(model, 0)
    model.to(DEV).eval()
    rng = np.random.default_rng(11)
    O = sum(bank.num_objects)
    mv, vx = _t(rng.standard_normal((O, 32)).astype(np.float32)), _t(rng.standard_normal((O, 48)).astype(np.float32))
    tg = np.array([[2, -1], [0, 1], [5, -1], [8, -1]], dtype=np.int32)
    seed = torch.tensor([3], dtype=torch.int64, device=DEV)
    for sel in (np.array([[0, 1, 2], [1, 0, 1], [3, 4, 5], [9, 8, 7]], dtype=np.int32), SEL64):
        batch, err = OB.prepare_grounding_batch(bank, _t(SOI), _t(sel), _t(tg), num_points=n, seed=seed,
                                                rotation=_t(_rotation(rng, 4)), mv_table=mv, voxel_table=vx)
        OB.check_objects(err)
        pad = batch["obj_pad_masks"]
        assert batch["pc_seg_fts"] is batch["obj_fts"] and tuple(batch["obj_fts"].shape) == (4, 3, n, 6)
        locs = batch["obj_locs"].cpu().numpy()
        for b in range(4):
            v = pad[b].cpu().numpy()
            assert np.array_equal(batch["coord_min"][b].cpu().numpy(), locs[b, v, :3].min(0))
            assert np.array_equal(batch["coord_max"][b].cpu().numpy(), locs[b, v, :3].max(0))
        o_glob = ref["object_offsets"][SOI][:, None] + sel
        want_mv = np.where((sel >= 0)[:, :, None], mv.cpu().numpy()[np.clip(o_glob, 0, O - 1)], 0)
        assert np.array_equal(batch["mv_seg_fts"].cpu().numpy(), want_mv) and tuple(batch["voxel_seg_fts"].shape) == (4, 3, 48)
        _same(batch["tgt_object_id"], R.ground_labels(ref["object_offsets"], SOI, sel, tg)[0])
        g = torch.Generator().manual_seed(2)
        batch["prompt_feat"] = torch.randn(4, T, d, generator=g).to(DEV)
        batch["prompt_pad_masks"] = (torch.arange(T)[None] < torch.tensor([T, 3, 1, 4])[:, None]).to(DEV)
        with torch.no_grad():
            out = model(batch)
        logits = out["og3d_logits"]
        assert tuple(logits.shape) == (4, 3)
        assert torch.isfinite(logits[pad]).all() and (logits[~pad] == float("-inf")).all()
        if bool(pad.all()):
            assert torch.isfinite(logits).all()
