"""GPU: TRAINING the PointNet++ tokenizer -- PointNetPP(trainable=True).train() (pq3d_amd/pointnetpp.py: batch-statistics
BatchNorm, the fused pooled layer and its backward, the grouping gradient, one autograd node).

Kernels, each against the existing kernels or the host at the smallest shapes that can go wrong:
    pq3d_bn_relu_maxpool            torch.equal to the max over samples of pq3d_bn_apply(act='relu'); arg = numpy's first arg-max
    pq3d_bn_pool_bwd_reduce/_apply  torch.equal to pq3d_bn_bwd_reduce / _apply fed the dense gradient scattered at arg
    pq3d_group_rows_bwd             integer-valued gradients (exact sums) equal a host index_add; real-valued ones are bit-identical
                                    run to run and equal the host sum taken in increasing entry order in float32

Network: one step on fixture F12's 4 clouds with the shipped spec against tests/pointnetpp_train_ref.py::train_step in float64
(kept honest by fixture F30, tests/test_pointnetpp_train_ref.py).  Compared as relative L2: the output, the gradient of every
parameter, the running buffers after the step.  Bars, by tests/test_gpu_voxel_backbone_train.py's scheme:
E32 = the reference run in float32 on the host, E16 = the reference with the operands of every product rounded to bf16;
    compute 'fp32': error <= 8 * max(E32 of that tensor, E32 of all gradients concatenated)
    compute 'bf16': error <= 2 * max(E16 of that tensor, E16 of all gradients concatenated)

Measured on an MI355X, worst ratio of error to the bar's base over the tensors of each kind:
    pointnet++ training fp32: bn gradients 0.70 x (grad/encoder.0.mlps.0.layer2.bn.bn.bias)   conv gradients 1.03 x (grad/encoder.1.mlps.0.layer0.conv.weight)   fc gradients 0.29 x (grad/fc.weight)   output 0.30 x (out)   running buffers 0.04 x (buf/encoder.2.mlps.0.layer0.bn.bn.running_mean)   [E of the output 1.4e-06, of all gradients 5.2e-06]
    pointnet++ training bf16: bn gradients 1.03 x (grad/encoder.1.mlps.0.layer2.bn.bn.bias)   conv gradients 0.98 x (grad/encoder.0.mlps.0.layer2.conv.weight)   fc gradients 0.06 x (grad/fc.weight)   output 0.06 x (out)   running buffers 0.01 x (buf/encoder.2.mlps.0.layer0.bn.bn.running_mean)   [E of the output 2.1e-02, of all gradients 3.7e-01]
(the bars are 8 x and 2 x these bases.  The gradients' own E is far above the output's -- nine BatchNorm backward passes over as
few as 64 rows amplify rounding -- so the 'fp32' leg is the one that pins the structure; the 'bf16' leg is loose by nature.)

Then behaviour (accumulation, no stale fold, the graph is freed, capture) and the model: Query3DUnified with
ObjectEncoder(backbone='pointnet++', freeze_backbone=False, trainable_backbone=True) takes one TrainStep."""
import weakref

import numpy as np
import pytest
import torch

from tests import pointnetpp_train_ref as TR
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------ the kernels
# (G, ns, C): one row; odd sizes; exactly one 64-row block per 2 groups and two 32-column blocks; a ragged column block and
# ns no multiple of the 8 row lanes; 5024 rows = 79 row blocks of 64, the last one ragged (32 rows)
POOL_SHAPES = [(1, 1, 1), (3, 5, 5), (7, 32, 64), (5, 33, 130), (157, 32, 40)]


def _pool_case(G, ns, C, seed=0):
    from pq3d_amd import sparse as S
    g = torch.Generator().manual_seed(seed + 1000 * C + G)
    N = G * ns
    buf = torch.randn(N, C + 3, generator=g)
    z = buf[:, :C]                                                   # strided rows: ldz = C + 3
    if ns >= 3:
        z.view(G, ns, C)[:, 2] = z.view(G, ns, C)[:, 0]              # duplicated rows inside every group: ties
    if G >= 3:
        z.view(G, ns, C)[1] = -50.0 - torch.rand(ns, C, generator=g)  # a group far below the mean: every activation <= 0
    gamma, beta = torch.rand(C, generator=g) + 0.5, 0.1 * torch.randn(C, generator=g)
    gp = torch.randn(G, C, generator=g)
    z, gamma, beta, gp = buf.to(DEV)[:, :C], gamma.to(DEV), beta.to(DEV), gp.to(DEV)
    mean, rstd = S.bn_stats(z, 1e-5)
    y = S.bn_apply(z, mean, rstd, gamma, beta, act="relu")
    return S, z, gamma, beta, gp, mean, rstd, y


@pytest.mark.parametrize("G,ns,C", POOL_SHAPES)
def test_bn_relu_maxpool_equals_bn_apply_then_max(G, ns, C):
    from pq3d_amd import pointnetpp as PP
    S, z, gamma, beta, gp, mean, rstd, y = _pool_case(G, ns, C)
    pooled, arg = PP.bn_relu_maxpool(z, G, ns, mean, rstd, gamma, beta)
    yv = y.view(G, ns, C)
    assert pooled.shape == (G, C) and arg.shape == (G, C) and arg.dtype == torch.int32
    assert torch.equal(pooled, yv.max(1).values)
    assert np.array_equal(arg.cpu().numpy(), np.argmax(yv.cpu().numpy(), axis=1))      # numpy: the first occurrence
    if G >= 3:
        assert float(pooled[1].abs().max()) == 0.0 and int(arg[1].abs().max()) == 0    # all <= 0: pooled 0, arg 0
    if ns >= 3:
        assert not bool((arg == 2).any())                                                # a copy never beats its original


@pytest.mark.parametrize("G,ns,C", POOL_SHAPES)
def test_pooled_backward_equals_the_dense_pair(G, ns, C):
    from pq3d_amd import pointnetpp as PP
    S, z, gamma, beta, gp, mean, rstd, y = _pool_case(G, ns, C)
    pooled, arg = PP.bn_relu_maxpool(z, G, ns, mean, rstd, gamma, beta)
    dy = torch.zeros(G, ns, C, device=DEV)
    dy.scatter_(1, arg.long()[:, None, :], gp[:, None, :])
    dy = dy.view(G * ns, C)
    dg, db = S.bn_bwd_reduce(dy, z, mean, rstd, y=y)
    dz = S.bn_bwd_apply(dy, z, mean, rstd, gamma, dg, db, y=y)
    fz, fg, fb = PP.bn_pool_bwd(gp, pooled, arg, z, G, ns, mean, rstd, gamma)
    assert torch.equal(fg, dg) and torch.equal(fb, db)
    assert torch.equal(fz, dz)


def _host_group_bwd(drows, idx, B, N, C, np_, ns, dtype):
    """sum over the entries of every point in increasing entry order, in ``dtype`` on the host"""
    d = drows.cpu().view(B, np_ * ns, -1)[:, :, 3:3 + C].to(dtype)
    ref = torch.zeros(B, N, C, dtype=dtype)
    ix = idx.cpu().long().view(B, -1)
    rows = torch.arange(B)
    for e in range(np_ * ns):
        ref[rows, ix[:, e]] += d[:, e]
    return ref


def _int_rows(B, np_, ns, C, g):
    Kp = (3 + C + 7) // 8 * 8
    return torch.randint(-8, 9, (B * np_ * ns, Kp), generator=g).float().to(DEV)


@pytest.mark.parametrize("B,N,np_,ns,C", [(2, 1, 3, 4, 5), (3, 40, 7, 1, 1), (2, 50, 6, 9, 5), (2, 300, 16, 32, 128),
                                          (2, 8192, 128, 256, 1)])
def test_group_rows_bwd_integer_sums(B, N, np_, ns, C):
    """N = 1; ns = 1; C in {1, 5, 128}; more entries than one 64-wide placement step; both caps at once (97 KB of LDS)."""
    from pq3d_amd import pointnetpp as PP
    g = torch.Generator().manual_seed(N + C)
    idx = torch.randint(0, N, (B, np_, ns), generator=g).int()
    if N > 2:
        idx[idx == 1] = 0                            # point 1: referenced by no entry
        idx[-1] = 2                                  # the last cloud: point 2 is referenced by EVERY entry
    idx = idx.to(DEV)
    drows = _int_rows(B, np_, ns, C, g)
    got = PP.group_rows_bwd(drows, C, idx, B, N, np_, ns)
    ref = torch.zeros(B, N, C, dtype=torch.float64)
    for b in range(B):
        ref[b].index_add_(0, idx[b].flatten().cpu().long(), drows.cpu().view(B, np_ * ns, -1)[b, :, 3:3 + C].double())
    assert got.shape == (B, N, C) and torch.equal(got.cpu().double(), ref)
    if N > 2:
        assert float(got[:, 1].abs().max()) == 0.0 and float(got[-1, 3:].abs().max()) == 0.0


def test_group_rows_bwd_ball_query_fills_group_all_and_caps():
    from pq3d_amd import _lib as L, pointnet2 as P2, pointnetpp as PP
    g = torch.Generator().manual_seed(5)
    B, N, np_, ns, C = 3, 200, 16, 32, 5
    xyz = torch.rand(B, N, 3, generator=g) - 0.5
    xyz[0, :, 1:] *= 0.05                                            # a rod: its radius-0.25 balls are full, the cube's are short
    xyz = xyz.to(DEV)
    fps = P2.furthest_point_sample(xyz, np_)
    new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    idx = P2.ball_query(0.25, ns, xyz, new_xyz)
    assert bool((idx[:, :, -1] == idx[:, :, 0]).any()) and bool((idx[:, :, -1] != idx[:, :, 0]).any())   # short balls and full ones
    drows = _int_rows(B, np_, ns, C, g)
    got = PP.group_rows_bwd(drows, C, idx, B, N, np_, ns)
    assert torch.equal(got.cpu(), _host_group_bwd(drows, idx, B, N, C, np_, ns, torch.float64).float())
    # real-valued gradients: the same bits every run, and the host's sum in increasing entry order
    real = torch.randn(B * np_ * ns, 8, generator=g).to(DEV)
    a, b = PP.group_rows_bwd(real, C, idx, B, N, np_, ns), PP.group_rows_bwd(real, C, idx, B, N, np_, ns)
    assert torch.equal(a, b) and torch.equal(a.cpu(), _host_group_bwd(real, idx, B, N, C, np_, ns, torch.float32))
    # GroupAll: a strided column copy
    allrows = torch.randn(B * N, 8, generator=g).to(DEV)
    assert torch.equal(PP.group_rows_bwd(allrows, C, None, B, N, 1, N), allrows[:, 3:3 + C].reshape(B, N, C))
    # over a cap: refused with text, nothing launched
    one = torch.zeros(PP.GROUP_BWD_MAX_ENTRIES + 1, 8, device=DEV)
    with pytest.raises(L.Pq3dError, match="PQ3D_GROUP_BWD_MAX"):
        PP.group_rows_bwd(one, 1, torch.zeros(1, 1, PP.GROUP_BWD_MAX_ENTRIES + 1, dtype=torch.int32, device=DEV), 1, 4, 1,
                          PP.GROUP_BWD_MAX_ENTRIES + 1)
    with pytest.raises(L.Pq3dError, match="PQ3D_GROUP_BWD_MAX"):
        PP.group_rows_bwd(one[:8], 1, torch.zeros(1, 2, 4, dtype=torch.int32, device=DEV), 1, PP.GROUP_BWD_MAX_POINTS + 1, 2, 4)
    with pytest.raises(L.Pq3dError, match="np == 1, ns == N"):
        PP.group_rows_bwd(one[:8], 1, None, 1, 4, 2, 4)


# ------------------------------------------------------------------------------------------------------------ the network
def _spec():
    from pq3d_amd.pointnetpp import POINTNETPP_TOKENIZER
    return {k: [list(x) if isinstance(x, list) else x for x in v] for k, v in POINTNETPP_TOKENIZER.items()}


@pytest.fixture(scope="module")
def case():
    from pq3d_amd import synth
    from pq3d_amd.pointnetpp import PointNetPP
    z, a = util.load_fixture("F12_pointnetpp")
    spec = _spec()
    sd = synth.fill_module(PointNetPP(**spec), a["seed"])
    pc = torch.from_numpy(z["pc"])
    R = torch.randn(pc.shape[0], spec["sa_mlps"][-1][-1], generator=torch.Generator().manual_seed(21))
    step = lambda dtype, bf16=False, trace=None: TR.train_step(sd, pc, spec["sa_n_points"], spec["sa_n_samples"], spec["sa_radii"], R,
                                                               dtype, bf16=bf16, trace=trace)
    trace = {}
    ref = step(torch.float64, trace=trace)
    E = {}
    for tag, r in (("fp32", step(torch.float32)), ("bf16", step(torch.float32, bf16=True))):
        e = {k: _rel(r[k], ref[k]) for k in ref if not k.endswith("num_batches_tracked")}
        gk = [k for k in ref if k.startswith("grad/")]
        e["all_grads"] = _rel(torch.cat([r[k].flatten() for k in gk]), torch.cat([ref[k].flatten() for k in gk]))
        E[tag] = e
    return dict(spec=spec, sd=sd, pc=pc.to(DEV), R=R.to(DEV), ref=ref, E=E, trace=trace)


def _fresh(case, compute, **kw):
    from pq3d_amd.pointnetpp import PointNetPP
    m = PointNetPP(**case["spec"], trainable=True, **kw)
    m.load_state_dict(case["sd"])
    m.compute = compute
    return m.to(DEV)


def _step(case, model):
    out = model(case["pc"])
    (out * case["R"]).sum().backward()
    return out


def test_point_set_kernels_reproduce_the_oracles_indices(case):
    from pq3d_amd import pointnet2 as P2
    xyz = case["pc"][..., :3].contiguous()
    for i in range(2):
        npoint, ns, radius = (case["spec"][k][i] for k in ("sa_n_points", "sa_n_samples", "sa_radii"))
        fps = P2.furthest_point_sample(xyz, npoint)
        assert np.array_equal(fps.cpu().numpy(), case["trace"][f"fps/{i}"])
        new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        assert np.array_equal(P2.ball_query(radius, ns, xyz, new_xyz).cpu().numpy(), case["trace"][f"ball/{i}"])
        xyz = new_xyz


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_training_step_matches_float64_reference(case, compute):
    model = _fresh(case, compute)
    assert model.training and model.trainable and all(p.requires_grad for p in model.parameters())
    pc = case["pc"].clone().requires_grad_(True)
    out = model(pc)
    assert out.requires_grad and out.dtype == torch.float32
    (out * case["R"]).sum().backward()
    assert pc.grad is None                                          # the points are data
    got = {"out": out.detach().cpu()}
    for name, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
        got[f"grad/{name}"] = p.grad.cpu()
    sd = model.state_dict()
    ref, E = case["ref"], case["E"][compute]
    for k in ref:
        if k.startswith("buf/"):
            got[k] = sd[k[4:]].cpu()
    factor = 8.0 if compute == "fp32" else 2.0
    assert sorted(got) == sorted(ref)
    worst, over = {}, []
    for k in sorted(ref):
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(ref[k]) == 1, k
            continue
        assert got[k].shape == ref[k].shape, k
        e, base = _rel(got[k], ref[k]), max(E[k], E["all_grads"])
        kind = "output" if k == "out" else "running buffers" if k.startswith("buf/") else \
            "conv gradients" if k.endswith("conv.weight") else "fc gradients" if k.startswith("grad/fc.") else "bn gradients"
        if e / base > worst.get(kind, (0.0, ""))[0]:
            worst[kind] = (e / base, k)
        if e > factor * base:
            over.append(f"{k}: {e:.3e} > {factor} x {base:.3e}")
    print(f"\npointnet++ training {compute}: " + "   ".join(f"{kind} {r:.2f} x ({k})" for kind, (r, k) in sorted(worst.items())) +
          f"   [E of the output {E['out']:.1e}, of all gradients {E['all_grads']:.1e}]")
    assert not over, "\n".join(over)


def test_second_step_accumulates_and_no_fold_is_stale(case):
    model = _fresh(case, "fp32")
    with torch.no_grad():
        before = model.eval()(case["pc"])
        model.train()
    out = _step(case, model)
    # the step's graph dies with its output (no collector run): the tape must not hold an output of its own node
    r = weakref.ref(out)
    del out
    assert r() is None, "a training step's output is kept alive by its own autograd node"
    g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
    _step(case, model)
    for n, p in model.named_parameters():
        # the second gradient equals the first (batch statistics do not depend on the running buffers): .grad holds g + g
        assert torch.equal(p.grad, g1[n] + g1[n]), n
    assert all(int(m.num_batches_tracked) == 2 for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))
    model.eval()
    with pytest.raises(NotImplementedError, match="training the PointNet\\+\\+ backbone is not provided"):
        model(case["pc"])                                           # eval mode with grad enabled: as the frozen network
    w = model.encoder[0].mlps[0].layer0.conv.weight
    with torch.no_grad():
        moved = model(case["pc"])                                   # the running buffers moved: eval output changed
        w.mul_(0.5)                                                 # what an optimizer step does
        after = model(case["pc"])
        w.data.mul_(2.0)                                            # a step that leaves no trace on the module (TrainStep's flat
        again = model(case["pc"])                                   # AdamW writes the storage directly)
    assert not torch.equal(moved, before)
    assert not torch.equal(after, moved), "eval mode ran on a stale folded copy of the weights"
    assert not torch.equal(again, after), "eval mode kept the folded weights of the previous eval forward"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_forward_backward_is_graph_capturable(case, compute):
    model = _fresh(case, compute)
    params = list(model.parameters())

    def fb():
        return torch.autograd.grad((model(case["pc"]) * case["R"]).sum(), params)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):          # eager reference and warm-up on a side stream, as a capture's callers do
        eager = [g.clone() for g in fb()]
        fb()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = fb()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grads, eager))
    assert all(torch.equal(a, b) for a, b in zip(fb(), eager))


def test_defaults_still_refuse_and_the_frozen_keyword_changes_nothing(case):
    from pq3d_amd.modules import ObjectEncoder
    from pq3d_amd.pointnetpp import PointNetPP
    net = PointNetPP(**case["spec"]).to(DEV)
    assert not net.trainable
    with pytest.raises(NotImplementedError):             # BatchNorm in training mode
        net.train()(case["pc"])
    with pytest.raises(NotImplementedError):             # trainable parameters with grad enabled
        net.eval()(case["pc"])
    with pytest.raises(NotImplementedError, match="trainable_backbone"):
        ObjectEncoder(None, backbone="pointnet++", freeze_backbone=False)
    with pytest.raises(NotImplementedError):
        PointNetPP(**case["spec"], bn=False, trainable=True)
    kw = dict(backbone="pointnet++", input_feat_size=768, hidden_size=64, use_projection=True, use_cls_head=False, dropout=0.0)
    enc = ObjectEncoder(None, freeze_backbone=True, trainable_backbone=True, **kw)
    assert not enc.backbone.trainable
    enc.compute = "fp32"
    enc.backbone.load_state_dict(case["sd"])
    enc.to(DEV).train()
    emb = enc(case["pc"].view(2, 2, *case["pc"].shape[1:]))
    assert emb.shape == (2, 2, 64) and emb.requires_grad   # the projection trains, the tokenizer does not
    emb.sum().backward()
    assert all(p.grad is None for p in enc.backbone.parameters()) and enc.input_feat_proj[0].weight.grad is not None
    assert all(int(m.num_batches_tracked) == 0 for m in enc.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d))
    # the trainable encoder returns (embeds, class logits) with its cls_head, as the frozen one does
    enc2 = ObjectEncoder(None, freeze_backbone=False, trainable_backbone=True, **dict(kw, use_cls_head=True, tgt_cls_num=11))
    assert enc2.backbone.trainable
    enc2.compute = "fp32"
    enc2.to(DEV).train()
    emb2, logits = enc2(case["pc"].view(2, 2, *case["pc"].shape[1:]))
    assert emb2.shape == (2, 2, 64) and logits.shape == (2, 2, 11)
    (emb2.sum() + logits.sum()).backward()
    assert all(p.grad is not None for p in enc2.backbone.parameters())


# ---------------------------------------------------------------------------------------------------------------- the model
def test_model_trains_the_point_tokenizer():
    from pq3d_amd import synth
    from pq3d_amd.model import Query3DUnified, make_cfg
    from pq3d_amd.modules import ObjectEncoder, set_compute
    from pq3d_amd.trainer import TrainStep
    d, O, P = 64, 3, 64
    model = Query3DUnified(make_cfg(d=d, H=4, L=2, memories=["mv", "pc"], heads=["ground"], d_in={"mv": 32, "pc": 768}), compute="fp32")
    model.pc_encoder = ObjectEncoder(None, backbone="pointnet++", freeze_backbone=False, trainable_backbone=True, input_feat_size=768,
                                     hidden_size=d, use_projection=True, use_cls_head=False, dropout=0.1)
    set_compute(model, "fp32")
    synth.fill_module(model, 0)
    model.to(DEV).train()
    bb = model.pc_encoder.backbone
    assert bb.trainable and bb.training
    group = [g for g in model.get_opt_params() if any(id(p) == id(bb.fc.weight) for p in g["params"])]
    assert len(group) == 1 and group[0].get("name", "pc_encoder") == "pc_encoder"
    ids = {id(p) for g in model.get_opt_params() for p in g["params"]}
    assert all(id(p) in ids for p in bb.parameters())
    dd = synth.synth_data_dict(2, O, 7, {"mv": 32, "pc": 768}, seed=5, memories=["mv"], full_valid=True)
    dd["pc_seg_fts"] = synth.pointcloud_inputs(2 * O, P, 3, seed=9).view(2, O, P, 6)
    dd["pc_seg_pad_masks"] = dd["mv_seg_pad_masks"].clone()
    dd = {k: v.to(DEV) for k, v in dd.items()}

    def loss_fn(out):
        gl = out["ground_logits"]
        return out["query_embeds"].square().mean() + torch.where(torch.isfinite(gl), gl, torch.zeros_like(gl)).square().mean()

    ts = TrainStep(model, loss_fn, lr=1e-3, grad_norm=5.0, warmup_steps=0, total_steps=10)
    flat = {id(p) for p in ts.reducer.params}
    assert all(id(p) in flat for p in bb.parameters())
    before = {n: p.detach().clone() for n, p in bb.named_parameters()}
    bufs = {n: b.detach().clone() for n, b in bb.named_buffers()}
    loss = ts.step(dict(dd))
    assert bool(torch.isfinite(loss))
    for n, p in bb.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p, before[n]), n
    for n, b in bb.named_buffers():
        assert not torch.equal(b, bufs[n]), n
    # eval mode runs on the running statistics: a cloud's token does not depend on what else is in the batch (with batch
    # statistics it would move by O(1); no row's summation order depends on its tile-mates, the row GEMMs may tile
    # differently at another row count: 1e-5 of the largest value)
    model.eval()
    clouds = dd["pc_seg_fts"].flatten(0, 1)
    with torch.no_grad():
        both, alone = bb(clouds), bb(clouds[:1])
        out = model(dict(dd))
    assert float((both[:1] - alone).abs().max()) <= 1e-5 * float(both.abs().max()), "an eval-mode token changed with the batch composition"
    assert bool(torch.isfinite(out["query_embeds"]).all()) and not bb.training
