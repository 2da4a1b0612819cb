"""GPU: TRAINING the voxel backbone -- Res16UNet34C(trainable=True).train() (pq3d_amd/sparse.py: batch-statistics BatchNorm, the
sparse-convolution backward, one autograd node) against tests/sparse_train_ref.py::train_network in float64 with torch
autograd, on tests/test_gpu_voxel_backbone.py's voxels and state.  The loss is the sum over all five maps of map * R with fixed
random R, so every output's gradient path is exercised at once.  Compared as relative L2: the five maps, the gradient of every
kernel / bn.weight / bn.bias, the running buffers after the step.

Bars, by the forward test's scheme:  E32 = the reference run in float32 on the host, E16 = the reference with the operands of
every product rounded to bf16 (forward, input-gradient and weight-gradient products alike);
    compute 'fp32': error <= 8 * max(E32 of that tensor, E32 of all gradients concatenated)
    compute 'bf16': error <= 2 * max(E16 of that tensor, E16 of all gradients concatenated)
(the max keeps a tiny tensor's near-zero E from becoming its bar).

Measured on an MI355X, worst ratio of error to the bar's base over the tensors of each kind:
    fp32: maps 0.00   kernel gradients 1.49 (block3.1.conv1)   bn gradients 1.56 (block2.0.norm1 bias)   running buffers 0.00
    bf16: maps 0.06   kernel gradients 1.06 (block2.0.downsample)   bn gradients 1.35 (block1.1.norm1 bias)   running buffers 0.00
(The gradients' own E is far above the maps': median 8e-4 per tensor in float32 and 0.25 with bf16 operands, against 1e-6 / 1e-2
for the maps -- thirty-four BatchNorm backward passes amplify rounding -- so E of all gradients is the base of the maps' and
buffers' bars, which they meet with room.)

Then the model: Query3DUnified with PCDMask3DSegLevelEncoder(build_backbone="trainable", freeze_backbone=False) takes one
TrainStep from raw voxels."""
import weakref

import pytest
import torch

from tests import sparse_train_ref as TR
from tests.test_gpu_voxel_backbone import CIN, COUT, _match, make_state, make_voxels

pytestmark = pytest.mark.gpu
MOM = 0.02
CONFIG = {"bn_momentum": MOM, "conv1_kernel_size": 5, "dialations": [1, 1, 1, 1]}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _reference(sd, tabs, feats, Rs, dtype, bf16=False):
    """{name: tensor}: maps 'map0'..'map4', 'grad/<parameter>', 'buf/<buffer>' of one training step of the reference"""
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()
              if k.endswith(("kernel", "bn.weight", "bn.bias")) and not k.startswith("final")}
    buffers = {k: v for k, v in sd.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    maps, new = TR.train_network(params, buffers, tabs, feats, dtype, MOM, bf16=bf16)
    loss = sum((m * r.to(dtype)).sum() for m, r in zip(maps, Rs))
    names = sorted(params)
    grads = torch.autograd.grad(loss, [params[n] for n in names])
    out = {f"map{h}": m.detach() for h, m in enumerate(maps)}
    out.update({f"grad/{n}": g for n, g in zip(names, grads)})
    out.update({f"buf/{n}": v for n, v in new.items()})
    return out


@pytest.fixture(scope="module")
def case():
    from pq3d_amd import sparse
    coords, sd = make_voxels(), make_state()
    feats = torch.rand(len(coords), CIN, generator=torch.Generator().manual_seed(1))
    tabs = TR.tables(coords)
    g = torch.Generator().manual_seed(21)
    sizes = [len(tabs["C"][4 - h]) for h in range(5)]
    Rs = [torch.randn(n, c, generator=g) for n, c in zip(sizes, (256, 256, 128, 96, 96))]     # in the reference's row order
    ref = _reference(sd, tabs, feats, Rs, torch.float64)
    r32 = _reference(sd, tabs, feats, Rs, torch.float32)
    r16 = _reference(sd, tabs, feats, Rs, torch.float32, bf16=True)
    E = {}
    for tag, r in (("fp32", r32), ("bf16", r16)):
        e = {k: _rel(r[k], ref[k]) for k in ref if not k.endswith("num_batches_tracked")}
        gk = [k for k in ref if k.startswith("grad/")]
        e["all_grads"] = _rel(torch.cat([r[k].flatten() for k in gk]), torch.cat([ref[k].flatten() for k in gk]))
        E[tag] = e
    pyr = sparse.CoordPyramid(coords.cuda())
    idx = [_match(tabs["C"][4 - h], pyr.level_coords(4 - h).cpu().long()) for h in range(4)]    # reference row -> internal row
    R_ours = []
    for h in range(4):
        r = torch.empty_like(Rs[h])
        r[idx[h]] = Rs[h]
        R_ours.append(r.cuda())
    R_ours.append(Rs[4].cuda())
    return dict(sparse=sparse, coords=coords, feats=feats, sd=sd, ref=ref, E=E, pyr=pyr, idx=idx, R=R_ours)


def _fresh(case, compute):
    m = case["sparse"].Res16UNet34C(CIN, COUT, CONFIG, out_fpn=True, compute=compute, trainable=True)
    m.load_state_dict(case["sd"])
    return m.cuda()


def _step(case, model):
    out, maps = model.run(case["pyr"], case["feats"].cuda())
    loss = sum((m * r).sum() for m, r in zip(maps, case["R"]))
    loss.backward()
    return out, maps


def test_trainable_keyword_and_modes(case):
    sp = case["sparse"]
    m = _fresh(case, "fp32")
    assert m.training and all(p.requires_grad for p in m.parameters())
    assert m.eval() is m and not m.training and m.train() is m and m.training
    assert [id(p) for p in m.unused_parameters()] == [id(p) for p in m.final.parameters()]
    frozen = sp.Res16UNet34C(CIN, COUT, CONFIG)
    assert not frozen.training and not any(p.requires_grad for p in frozen.parameters()) and frozen.unused_parameters() == []
    m.eval()
    with pytest.raises(NotImplementedError, match="training the voxel backbone is not provided"):
        m.run(case["pyr"], case["feats"].cuda())            # eval mode with grad enabled: as the frozen network
    with torch.no_grad():
        out, maps = m.run(case["pyr"], case["feats"].cuda())
    assert out.shape == (len(case["coords"]), 96) and not out.requires_grad


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_training_step_matches_float64_reference(case, compute):
    model = _fresh(case, compute)
    feats = case["feats"].cuda().requires_grad_(True)
    out, maps = model.run(case["pyr"], feats)
    assert torch.equal(out, maps[4]) and out.requires_grad
    sum((m * r).sum() for m, r in zip(maps, case["R"])).backward()
    assert model.final.kernel.grad is None and model.final.bias.grad is None and feats.grad is None
    got = {f"map{h}": maps[h].detach().cpu()[case["idx"][h]] for h in range(4)}
    got["map4"] = maps[4].detach().cpu()
    sd = model.state_dict()
    for name, p in model.named_parameters():
        if not name.startswith("final"):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            got[f"grad/{name}"] = p.grad.cpu()
    for k in case["ref"]:
        if k.startswith("buf/"):
            got[k] = sd[k[4:]].cpu()
    ref, E = case["ref"], case["E"][compute]
    factor = 8.0 if compute == "fp32" else 2.0
    assert sorted(got) == sorted(ref)
    worst, over = {}, []
    for k in sorted(ref):
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(ref[k]) == 8
            continue
        assert got[k].shape == ref[k].shape, k
        e, base = _rel(got[k], ref[k]), max(E[k], E["all_grads"])
        kind = "maps" if k.startswith("map") else "running buffers" if k.startswith("buf/") else \
            "kernel gradients" if k.endswith("kernel") else "bn gradients"
        if e / base > worst.get(kind, (0.0, ""))[0]:
            worst[kind] = (e / base, k)
        if e > factor * base:
            over.append(f"{k}: {e:.3e} > {factor} x {base:.3e}")
    print(f"\nvoxel backbone training {compute}: " + "   ".join(f"{kind} {r:.2f} x ({k})" for kind, (r, k) in sorted(worst.items())))
    assert not over, "\n".join(over)


def test_second_step_accumulates_and_prepare_is_invalidated(case):
    model = _fresh(case, "fp32")
    with torch.no_grad():
        model.eval()
        before, _ = model.run(case["pyr"], case["feats"].cuda())
        model.train()
    out, maps = _step(case, model)
    # the step's graph dies with its outputs (no collector run): the tape must not hold an output of its own node
    refs = [weakref.ref(m) for m in maps]
    del out, maps
    assert all(r() is None for r in refs), "a training step's outputs are kept alive by its own autograd node"
    g1 = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    _step(case, model)
    for n, p in model.named_parameters():
        if n.startswith("final"):
            continue
        # the second gradient equals the first (batch statistics do not depend on the running buffers): .grad holds g + g
        assert torch.equal(p.grad, g1[n] + g1[n]), n
    assert int(model.bn0.bn.num_batches_tracked) == 7 + 2
    with torch.no_grad():
        model.conv0p1s1.kernel.mul_(0.5)                      # what an optimizer step does
        model.eval()
        after, _ = model.run(case["pyr"], case["feats"].cuda())
    assert not torch.equal(after, before), "eval mode ran on a stale folded copy of the weights"
    with torch.no_grad():                                     # eval -> a step that leaves no trace on the module -> eval
        model.conv0p1s1.kernel.data.mul_(2.0)                 # (TrainStep's flat AdamW writes the storage directly)
        again, _ = model.run(case["pyr"], case["feats"].cuda())
    assert not torch.equal(again, after), "eval mode kept the folded weights of the previous eval forward"


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_forward_backward_is_graph_capturable(case, compute):
    model = _fresh(case, compute)
    feats = case["feats"].cuda()
    params = [p for n, p in model.named_parameters() if not n.startswith("final")]

    def fb():
        out, maps = model.run(case["pyr"], feats)
        loss = sum((m * r).sum() for m, r in zip(maps, case["R"]))
        return torch.autograd.grad(loss, params)

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


# ---------------------------------------------------------------------------------------------------------------- the model
def _model():
    from pq3d_amd import synth
    from pq3d_amd.model import Cfg, Query3DUnified, make_cfg
    from tests.test_gpu_voxel_model import BACKBONE
    cfg = make_cfg(d=64, H=4, L=4, memories=["voxel", "mv"], heads=["mask"], use_self_mask=True, num_blocks=2, C=21, foc=(0, 2))
    cfg.model["use_offline_voxel_fts"] = False
    args = dict(backbone_kwargs=BACKBONE, hidden_size=64, hlevels=[0, 1, 2, 3], dropout=0.1, freeze_backbone=False,
                build_backbone="trainable")
    cfg.model["voxel_encoder"] = Cfg(name="PCDMask3DSegLevelEncoder", args=Cfg(args))
    model = Query3DUnified(cfg, compute="fp32")
    synth.fill_module(model, 0)
    for m in model.voxel_encoder.backbone.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_var.copy_(m.running_var.abs() + 0.5)
    return model.to("cuda")


def test_model_trains_from_raw_voxels():
    from pq3d_amd import synth
    from pq3d_amd.trainer import TrainStep
    from tests.test_gpu_voxel_model import S, _voxels
    model = _model().train()
    bb = model.voxel_encoder.backbone
    assert bb.trainable and bb.training
    ids = {id(p) for g in model.get_opt_params() for p in g["params"]}
    assert all(id(p) in ids for p in bb.parameters())
    group = [g for g in model.get_opt_params() if any(id(p) == id(bb.conv0p1s1.kernel) for p in g["params"])]
    assert len(group) == 1 and group[0].get("name", "voxel_encoder") == "voxel_encoder"
    coords, feats, v2s = _voxels()
    dd = synth.synth_data_dict(2, S, 9, {"mv": 64, "voxel": 64}, seed=5, memories=["mv"])
    dd = {k: v.cuda() for k, v in dd.items()}
    dd.update(voxel_coordinates=coords.cuda(), voxel_features=feats.cuda(), voxel2segment=[p.cuda() for p in v2s])

    def loss_fn(out):
        return out["query_embeds"].square().mean() + sum(m.clamp(min=-50.0).mean() for m in out["predictions_mask"])

    ts = TrainStep(model, loss_fn, lr=1e-3, grad_norm=5.0, warmup_steps=0, total_steps=10)
    flat = {id(p) for p in ts.reducer.params}
    assert not any(id(p) in flat for p in bb.final.parameters()) and id(bb.conv0p1s1.kernel) in flat
    before = {n: p.detach().clone() for n, p in bb.named_parameters()}
    loss = ts.step(dd)
    assert bool(torch.isfinite(loss))
    for n, p in bb.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        assert torch.equal(p, before[n]) == n.startswith("final"), n
    # eval mode runs on the running statistics: a scene's features do not depend on what else is in the batch (with batch
    # statistics they would move by O(1); no row's summation order depends on its tile-mates, the 1 x 1 row GEMMs may tile
    # differently at another row count: 1e-5 of the largest feature)
    model.eval()
    keep = coords[:, 0] == 0
    with torch.no_grad():
        both = model.voxel_encoder.voxel_pyramid(coords.cuda(), feats[:, :-3].cuda())
        alone = model.voxel_encoder.voxel_pyramid(coords[keep].cuda(), feats[keep][:, :-3].cuda())
        out = model(dict(dd))
    a, b = both[-1][0][keep.cuda()], alone[-1][0]
    assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()), "eval-mode features changed with the batch composition"
    assert bool(torch.isfinite(out["query_embeds"]).all()) and not bb.training
