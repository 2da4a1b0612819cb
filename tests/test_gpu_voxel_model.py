"""GPU: Query3DUnified with the voxel encoder built WITH its backbone (PCDMask3DSegLevelEncoder(build_backbone=True)): fed raw
voxels only (``voxel_coordinates`` + ``voxel_features``) it computes the pyramid itself and gives, bit for bit, what the same
model gives when handed ``voxel_pyramid = backbone.pyramid(...)``; without the keyword the encoder is today's."""
import pytest
import torch

pytestmark = pytest.mark.gpu
S = 40
BACKBONE = dict(config=dict(dialations=[1, 1, 1, 1], conv1_kernel_size=5, bn_momentum=0.02), in_channels=3, out_channels=8,
                out_fpn=True)          # the layout of configs/instseg_sceneverse.yaml:105-112 (out_channels shrunk)


def _voxels():
    g = torch.Generator().manual_seed(8)
    rows, v2s = [], []
    for b in range(2):
        xyz = torch.unique(torch.cat([torch.randint(-20, 28, (500 + 100 * b, 2), generator=g),
                                      torch.randint(-2, 2, (500 + 100 * b, 1), generator=g)], 1), dim=0)
        rows.append(torch.cat([torch.full((len(xyz), 1), b), xyz], 1))
        v2s.append(torch.randint(0, S - 3 * b, (len(xyz),), generator=g))
    coords = torch.cat(rows).int()
    feats = torch.cat([torch.rand(len(coords), 3, generator=g), coords[:, 1:].float() * 0.02], 1)    # colour | xyz
    return coords, feats, v2s


def _model(build_backbone):
    from pq3d_amd import synth
    from pq3d_amd.model import Cfg, Query3DUnified, make_cfg
    cfg = make_cfg(d=64, H=4, L=4, memories=["voxel", "mv"], heads=["mask"], use_self_mask=True, num_blocks=2, C=21, foc=(0, 2))
    cfg.model["use_offline_voxel_fts"] = False
    args = dict(backbone_kwargs=BACKBONE, hidden_size=64, hlevels=[0, 1, 2, 3], dropout=0.1)
    if build_backbone:
        args.update(freeze_backbone=True, build_backbone=True)
    cfg.model["voxel_encoder"] = Cfg(name="PCDMask3DSegLevelEncoder", args=Cfg(args))
    model = Query3DUnified(cfg, compute="fp32")
    synth.fill_module(model, 0)
    if build_backbone:      # running variances must be positive
        for m in model.voxel_encoder.backbone.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_var.copy_(m.running_var.abs() + 0.5)
    return model.to("cuda").eval()


def test_model_computes_the_pyramid_from_raw_voxels():
    from pq3d_amd import synth
    model = _model(True)
    enc = model.voxel_encoder
    assert any(k.startswith("voxel_encoder.backbone.conv0p1s1.kernel") for k in model.state_dict())
    assert all(not p.requires_grad for p in enc.backbone.parameters())
    coords, feats, v2s = _voxels()
    dd = synth.synth_data_dict(2, S, 9, {"mv": 64, "voxel": 64}, seed=5, memories=["mv"])
    dd = {k: v.cuda() for k, v in dd.items()}
    dd.update(voxel_coordinates=coords.cuda(), voxel_features=feats.cuda(), voxel2segment=[p.cuda() for p in v2s])
    with torch.no_grad():
        raw = model(dict(dd))
        given = dict(dd)
        given["voxel_pyramid"] = enc.backbone.pyramid(dd["voxel_coordinates"], dd["voxel_features"][:, :-3], [0, 1, 2, 3])
        sup = model(given)
        bogus = dict(given)         # a supplied pyramid wins: the raw voxels are not looked at
        bogus["voxel_features"] = torch.full_like(dd["voxel_features"], float("nan"))
        sup2 = model(bogus)
    assert len(raw["predictions_mask"]) == 4 * 2 + 1
    for a, b, c in zip(raw["predictions_mask"], sup["predictions_mask"], sup2["predictions_mask"]):
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a[a > -1e5]).all())
    assert torch.equal(raw["query_embeds"], sup["query_embeds"])
    # the voxel memory really depends on the raw voxels
    other = dict(dd)
    other["voxel_features"] = dd["voxel_features"] * 0.5
    with torch.no_grad():
        assert not torch.equal(model(other)["query_embeds"], raw["query_embeds"])
    shuffled = dict(dd)             # rows that are not scene after scene are refused, not silently mis-pooled
    perm = torch.randperm(len(coords), generator=torch.Generator().manual_seed(0)).cuda()
    shuffled["voxel_coordinates"], shuffled["voxel_features"] = dd["voxel_coordinates"][perm], dd["voxel_features"][perm]
    with pytest.raises(AssertionError, match="scene 0's voxels, then scene 1's"):
        model(shuffled)
    model.train()                   # the frozen backbone stays in eval mode under the model's train()
    assert not enc.backbone.training and all(not m.training for m in enc.backbone.modules())


def test_encoder_without_the_keyword_is_unchanged():
    from pq3d_amd import modules as M
    enc = M.PCDMask3DSegLevelEncoder(None, BACKBONE, hidden_size=64, hlevels=[0, 1, 2, 3], dropout=0.1)
    assert not hasattr(enc, "backbone")
    assert sorted(enc.state_dict()) == sorted(f"feat_proj_list.{i}.{j}.{w}" for i in range(5) for j in (0, 1) for w in ("weight", "bias"))
    with pytest.raises(NotImplementedError, match="build_backbone=True"):
        enc.voxel_pyramid(None, None)
    with pytest.raises(NotImplementedError, match="FROZEN"):
        M.PCDMask3DSegLevelEncoder(None, BACKBONE, hidden_size=64, build_backbone=True, freeze_backbone=False)
    model = _model(False)
    assert not any("backbone" in k for k in model.state_dict())
