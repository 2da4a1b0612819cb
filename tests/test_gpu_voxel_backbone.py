"""GPU: Res16UNet34C (pq3d_amd/sparse.py; frozen, forward only) against the same network composed from the float64 restatement
tests/sparse_ref.py: in_channels 3, out_channels 8, kernels ~ N(0, 1 / (K Cin)), random BatchNorm affine and running statistics
(variance in [0.5, 2]), two scenes of about 1 500 surface voxels (the stride-16 level holds more than one row tile in total).

Thirty-four chained convolutions make an a-priori bound meaningless, so every bar is measured here against the float64 run:
    E32  relative L2 error of the restatement run in float32 on the host
    E16  the same with every convolution's inputs and kernels rounded to bf16
    compute 'fp32': error <= 8 * E32 (the factor of the T5 body test for the same comparison)
    compute 'bf16': error <= 2 * E16 (kernel and emulation differ only in fp32 summation order)
for each of the five feature maps (strides 16, 8, 4, 2, 1) and ``out`` -- which, as in the reference's forward
(res16unet.py:307-314), is the last block's output: ``final`` is never applied and exists as state_dict entries only.

Measured on an MI355X (error, ratio to the bar's base), maps in the order 16, 8, 4, 2, 1, out:
    fp32: 5.07e-07 (3.26 x E32)  3.91e-07 (2.28 x)  1.68e-07 (1.46 x)  1.09e-07 (1.04 x)  8.76e-08 (0.97 x)  8.76e-08 (0.97 x)
    bf16: 1.79e-03 (1.00 x E16)  2.00e-03 (0.98 x)  1.39e-03 (0.99 x)  1.34e-03 (1.07 x)  1.20e-03 (1.10 x)  1.20e-03 (1.10 x)
(the bf16 stem keeps its 3-channel input exact, see csrc/sparse_conv.hip: one reason the kernel can sit below the emulation).
"""
import pytest
import torch

from tests import sparse_ref as R

pytestmark = pytest.mark.gpu

LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)                   # res16unet.py:329 (Res16UNet34)
PLANES = (32, 64, 128, 256, 256, 128, 96, 96)       # res16unet.py:391 (Res16UNet34C)
INIT, CIN, COUT = 32, 3, 8
DOWN = ("conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2")
UP = ("convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2")
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")   # MinkowskiBatchNorm.bn is an nn.BatchNorm1d


def expected_shapes():
    """{state_dict key: shape}, written out from the reference class definitions (res16unet.py:28-239, resnet.py:99-152,
    resnet_block.py:24-50; kernels [K, Cin, Cout], [Cin, Cout] when K = 1; bias [1, Cout])."""
    sd = {}

    def bn(p, c):
        for s in BN:
            sd[f"{p}.bn.{s}"] = () if s == "num_batches_tracked" else (c,)

    def layer(p, inplanes, planes, blocks):
        for j in range(blocks):
            cin = inplanes if j == 0 else planes
            sd[f"{p}.{j}.conv1.kernel"] = (27, cin, planes); bn(f"{p}.{j}.norm1", planes)
            sd[f"{p}.{j}.conv2.kernel"] = (27, planes, planes); bn(f"{p}.{j}.norm2", planes)
            if j == 0 and inplanes != planes:
                sd[f"{p}.0.downsample.0.kernel"] = (inplanes, planes); bn(f"{p}.0.downsample.1", planes)

    sd["conv0p1s1.kernel"] = (125, CIN, INIT); bn("bn0", INIT)
    inpl = INIT
    for i in range(4):
        sd[f"{DOWN[i]}.kernel"] = (8, inpl, inpl); bn(f"bn{i + 1}", inpl)
        layer(f"block{i + 1}", inpl, PLANES[i], LAYERS[i]); inpl = PLANES[i]
    skips = (PLANES[2], PLANES[1], PLANES[0], INIT)
    for i in range(4):
        sd[f"{UP[i]}.kernel"] = (8, inpl, PLANES[4 + i]); bn(f"bntr{4 + i}", PLANES[4 + i])
        layer(f"block{5 + i}", PLANES[4 + i] + skips[i], PLANES[4 + i], LAYERS[4 + i]); inpl = PLANES[4 + i]
    sd["final.kernel"] = (PLANES[7], COUT); sd["final.bias"] = (1, COUT)
    return sd


def make_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in expected_shapes().items():
        if k.endswith("kernel"):
            fan = shp[0] * shp[1] if len(shp) == 3 else shp[0]
            sd[k] = torch.randn(shp, generator=g) * fan ** -0.5
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(7)
        elif k.endswith("running_var"):
            sd[k] = torch.rand(shp, generator=g) * 1.5 + 0.5
        elif k.endswith("bn.weight"):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        else:                                    # bn.bias, running_mean, final.bias
            sd[k] = torch.randn(shp, generator=g) * 0.3
    return sd


def make_voxels(seed=4, per_scene=1500, extent=64):
    """surface voxels of a box of `extent` voxels per scene; scene 1 is shifted to negative, odd coordinates"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(2):
        face = torch.randint(0, 6, (3 * per_scene,), generator=g)
        uv = torch.randint(0, extent, (3 * per_scene, 2), generator=g)
        w = torch.where(face % 2 == 0, 0, extent - 1)
        ax = face // 2
        xyz = torch.stack([torch.where(ax == 0, w, uv[:, 0]), torch.where(ax == 1, w, torch.where(ax == 0, uv[:, 0], uv[:, 1])),
                           torch.where(ax == 2, w, uv[:, 1])], 1)
        xyz = torch.unique(xyz, dim=0)
        xyz = xyz[torch.randperm(len(xyz), generator=g)][:per_scene] - b * 37
        out.append(torch.cat([torch.full((len(xyz), 1), b), xyz], 1))
    return torch.cat(out).int()


def ref_network(sd, coords, feats, dtype, rnd=None):
    """res16unet.py:241-314 + resnet_block.py:52-68 composed from the restatement; level 0 in the caller's row order, the
    coarser levels in the restatement's (sorted) order.  Returns (out, [maps 16, 8, 4, 2, 1], level coordinates)."""
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    C = [coords.long()] + [R.level_coords(coords, 1 << l) for l in range(1, 5)]
    t3 = [R.table(C[l], 1 << l, C[l], R.offsets(3)) for l in range(5)]
    t5 = R.table(C[0], 1, C[0], R.offsets(5))
    dn = [R.table(C[l], 1 << l, C[l + 1], R.offsets(2)) for l in range(4)]
    up = [R.up_table(C[l + 1], C[l], 1 << l) for l in range(4)]
    conv = lambda x, tab, name: R.conv_table(x, tab, sd[name + ".kernel"], rnd=rnd)
    relu = lambda y: y.clamp_min(0)

    def bn(y, p):
        return (y - sd[p + ".bn.running_mean"]) / torch.sqrt(sd[p + ".bn.running_var"] + 1e-5) * sd[p + ".bn.weight"] + sd[p + ".bn.bias"]

    def lin(x, name):
        w = sd[name + ".kernel"]
        return (rnd(x) @ rnd(w)) if rnd is not None else x @ w

    def layer(x, p, l, blocks):
        for j in range(blocks):
            q = f"{p}.{j}"
            y = relu(bn(conv(x, t3[l], q + ".conv1"), q + ".norm1"))
            y = bn(conv(y, t3[l], q + ".conv2"), q + ".norm2")
            res = bn(lin(x, q + ".downsample.0"), q + ".downsample.1") if q + ".downsample.0.kernel" in sd else x
            x = relu(y + res)
        return x

    x = feats.to(dtype)
    skip = [relu(bn(conv(x, t5, "conv0p1s1"), "bn0"))]
    x = skip[0]
    for i in range(4):
        x = relu(bn(conv(x, dn[i], DOWN[i]), f"bn{i + 1}"))
        x = layer(x, f"block{i + 1}", i + 1, LAYERS[i])
        skip.append(x)
    maps = [x]
    for i in range(4):
        l = 3 - i
        x = relu(bn(conv(x, up[l], UP[i]), f"bntr{4 + i}"))
        x = layer(torch.cat([x, skip[l]], 1), f"block{5 + i}", l, LAYERS[4 + i])
        maps.append(x)
    return x, maps, C          # res16unet.py:311-314: the forward returns block8's output; `final` is not applied


def _match(a, b):
    rows = {tuple(r): i for i, r in enumerate(b.tolist())}
    return torch.tensor([rows[tuple(r)] for r in a.tolist()])


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.fixture(scope="module")
def case():
    from pq3d_amd import sparse
    coords, sd = make_voxels(), make_state()
    feats = torch.rand(len(coords), CIN, generator=torch.Generator().manual_seed(1))
    assert len(R.level_coords(coords, 16)) > sparse.ROW_TILE, "the stride-16 level must span more than one row tile"
    bf = lambda t: t.bfloat16().to(t.dtype)
    out64, maps64, C = ref_network(sd, coords, feats, torch.float64)
    out32, maps32, _ = ref_network(sd, coords, feats, torch.float32)
    out16, maps16, _ = ref_network(sd, coords, feats, torch.float32, rnd=bf)
    ref = maps64 + [out64]
    E32 = [_rel(a, b) for a, b in zip(maps32 + [out32], ref)]
    E16 = [_rel(a, b) for a, b in zip(maps16 + [out16], ref)]
    model = sparse.Res16UNet34C(CIN, COUT, {"bn_momentum": 0.02, "conv1_kernel_size": 5, "dialations": [1, 1, 1, 1]}, out_fpn=True)
    model.load_state_dict(sd)
    model.cuda()
    return dict(sparse=sparse, model=model, coords=coords, feats=feats, ref=ref, C=C, E32=E32, E16=E16, sd=sd)


def test_state_dict_is_the_reference_layout(case):
    want = expected_shapes()
    got = {k: tuple(v.shape) for k, v in case["model"].state_dict().items()}
    assert sorted(got) == sorted(want), "state_dict key set differs from the reference classes'"
    assert got == want
    fresh = case["sparse"].Res16UNet34C(CIN, COUT, {"bn_momentum": 0.02, "conv1_kernel_size": 5})
    res = fresh.load_state_dict(case["sd"])          # strict
    assert not res.missing_keys and not res.unexpected_keys
    assert all(not p.requires_grad for p in fresh.parameters()) and not fresh.training


def test_train_raises(case):
    m = case["sparse"].Res16UNet34C(CIN, COUT, {"bn_momentum": 0.02, "conv1_kernel_size": 5})
    assert m.train() is m and not m.training           # frozen: a parent's .train() leaves it in eval mode
    m.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="batch-statistics BatchNorm and the sparse-convolution backward"):
        m.train()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_backbone_matches_float64_restatement(case, compute):
    model, pyr_mod = case["model"], case["sparse"]
    model.compute = compute
    coords, feats = case["coords"].cuda(), case["feats"].cuda()
    out, maps = model(coords, feats)
    pyr = pyr_mod.CoordPyramid(coords)
    got = []
    for h in range(4):                                       # coarse maps: internal row order -> the restatement's
        l = 4 - h
        idx = _match(case["C"][l], pyr.level_coords(l).cpu().long())
        got.append(maps[h].cpu()[idx])
    got += [maps[4].cpu(), out.cpu()]
    assert out.shape == (len(coords), PLANES[7]) and torch.equal(out, maps[4])      # `final` (out_channels = 8) shapes no output
    base, factor = (case["E32"], 8.0) if compute == "fp32" else (case["E16"], 2.0)
    errs = [_rel(g, r) for g, r in zip(got, case["ref"])]
    print(f"\nvoxel backbone {compute}: " + "  ".join(f"{e:.3e} ({e / b:.2f}x of {b:.3e})" for e, b in zip(errs, base)))
    for name, e, b, g, r in zip(("16", "8", "4", "2", "1", "out"), errs, base, got, case["ref"]):
        assert g.shape == r.shape and bool(torch.isfinite(g).all())
        assert e <= factor * b, f"map {name} ({compute}): relative L2 error {e:.3e} > {factor} x {b:.3e}"
    # the pyramid form: same features, parents = ops.parents_from_coords
    pl = model.pyramid(coords, feats, [0, 1, 2, 3])
    assert len(pl) == 5 and all(torch.equal(f, m) for (f, _p), m in zip(pl, maps))
    assert all(p.dtype == torch.int64 and p.shape == (len(coords),) for _f, p in pl)
    assert all(int(p.max()) < f.shape[0] and int(p.min()) >= 0 for f, p in pl)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_convolutions_are_graph_capturable(case, compute):
    model = case["model"]
    model.compute = compute
    coords, feats = case["coords"].cuda(), case["feats"].cuda()
    pyr = case["sparse"].CoordPyramid(coords)                 # the one host synchronisation, outside the graph
    eager_out, eager_maps = model.run(pyr, feats)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.run(pyr, feats)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, maps = model.run(pyr, feats)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_out) and all(torch.equal(a, b) for a, b in zip(maps, eager_maps))
    again_out, _ = model.run(pyr, feats)
    assert torch.equal(again_out, eager_out)
