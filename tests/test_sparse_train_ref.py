"""CPU: tests/sparse_train_ref.py (the float64 reference of the voxel backbone's TRAINING step) against independent statements:
the convolution's gradients against a dictionary-of-coordinates double loop, BatchNorm against torch.nn.functional.batch_norm,
the bf16 emulation's two rounding points, and the whole network's autograd gradient against central differences."""
import torch
import torch.nn.functional as F

from tests import sparse_ref as R
from tests import sparse_train_ref as TR
from tests.test_gpu_voxel_backbone import make_state


def _small_coords(n=70, seed=3, lo=-6, hi=7):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(2):
        xyz = torch.unique(torch.randint(lo, hi, (n, 3), generator=g), dim=0) - 3 * b
        rows.append(torch.cat([torch.full((len(xyz), 1), b), xyz], 1))
    return torch.cat(rows)


def test_conv_grads_match_a_coordinate_dictionary_loop():
    c = _small_coords()
    g = torch.Generator().manual_seed(0)
    offs = R.offsets(3)
    tab = R.table(c, 1, c, offs)
    x, W, dy = torch.randn(len(c), 5, generator=g), torch.randn(27, 5, 4, generator=g), torch.randn(len(c), 4, generator=g)
    dX, dW, A_x, A_w = TR.conv_grads(x, tab, W, dy)
    row = {tuple(r): i for i, r in enumerate(c.tolist())}
    wX, wW, aX, aW = torch.zeros_like(dX), torch.zeros_like(dW), torch.zeros_like(dX), torch.zeros_like(dW)
    n_in, n_k = torch.zeros(len(c), dtype=torch.long), torch.zeros(27, dtype=torch.long)
    xd, Wd, dyd = x.double(), W.double(), dy.double()
    for o, (b, px, py, pz) in enumerate(c.tolist()):
        for k, (dx, dy_, dz) in enumerate(offs):
            i = row.get((b, px + dx, py + dy_, pz + dz))
            if i is None:
                continue
            wX[i] += Wd[k] @ dyd[o]
            aX[i] += Wd[k].abs() @ dyd[o].abs()
            wW[k] += torch.outer(xd[i], dyd[o])
            aW[k] += torch.outer(xd[i].abs(), dyd[o].abs())
            n_in[i] += 1
            n_k[k] += 1
    for got, want in ((dX, wX), (dW, wW), (A_x, aX), (A_w, aW)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    ci, ck = TR.pair_counts(tab, len(c))
    assert torch.equal(ci, n_in) and torch.equal(ck, n_k)


def test_rounding_points_of_the_bf16_emulation():
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(6, 8, generator=g, requires_grad=True), torch.randn(8, 3, generator=g, requires_grad=True)
    up = torch.randn(6, 3, generator=g)
    bf = lambda t: t.bfloat16().float()
    y = TR.RoundGrad.apply(TR.RoundOperands.apply(a) @ TR.RoundOperands.apply(b))
    da, db = torch.autograd.grad(y, (a, b), up)
    assert torch.equal(y.detach(), bf(a.detach()) @ bf(b.detach()))
    assert torch.equal(da, bf(up) @ bf(b.detach()).t()) and torch.equal(db, bf(a.detach()).t() @ bf(up))


def _tiny_case(dtype):
    c = _small_coords(160, seed=5, lo=-24, hi=24)      # ~40 voxels at stride 16: no BatchNorm over two or three rows
    sd = make_state()
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()
              if k.endswith(("kernel", "bn.weight", "bn.bias")) and not k.startswith("final")}
    buffers = {k: v for k, v in sd.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    feats = torch.rand(len(c), 3, generator=torch.Generator().manual_seed(2))
    return c, params, buffers, feats


def test_batch_statistics_follow_torch_batch_norm():
    """the stem's BatchNorm of train_network against F.batch_norm(training=True): output, both running buffers, the counter"""
    c, params, buffers, feats = _tiny_case(torch.float64)
    tabs = TR.tables(c)
    maps, new = TR.train_network(params, buffers, tabs, feats, torch.float64, 0.02)
    assert [m.shape[1] for m in maps] == [256, 256, 128, 96, 96] and maps[4].shape[0] == len(c)
    z = R.conv_table(feats.double(), tabs["t5"], params["conv0p1s1.kernel"].detach())
    rm, rv = buffers["bn0.bn.running_mean"].double().clone(), buffers["bn0.bn.running_var"].double().clone()
    F.batch_norm(z, rm, rv, params["bn0.bn.weight"].detach(), params["bn0.bn.bias"].detach(), True, 0.02, TR.EPS)
    assert torch.allclose(new["bn0.bn.running_mean"], rm, rtol=1e-12, atol=1e-14)
    assert torch.allclose(new["bn0.bn.running_var"], rv, rtol=1e-12, atol=1e-14)
    assert int(new["bn0.bn.num_batches_tracked"]) == int(buffers["bn0.bn.num_batches_tracked"]) + 1
    assert sorted(new) == sorted(buffers)


def test_network_gradient_matches_central_differences():
    c, params, buffers, feats = _tiny_case(torch.float64)
    tabs = TR.tables(c)
    g = torch.Generator().manual_seed(9)
    maps, _ = TR.train_network(params, buffers, tabs, feats, torch.float64, 0.02)
    Rs = [torch.randn(m.shape, generator=g, dtype=torch.float64) for m in maps]
    loss = lambda ms: sum((m * r).sum() for m, r in zip(ms, Rs))
    names = ["conv0p1s1.kernel", "block1.0.conv2.kernel", "block4.0.downsample.0.kernel", "convtr5p8s2.kernel", "bn2.bn.bias"]
    grads = dict(zip(names, torch.autograd.grad(loss(maps), [params[n] for n in names])))
    # ReLU kinks inside +-h bias a long step and double rounding a short one: the quotient must agree at ONE of two step sizes
    for n in names:
        p = params[n]
        idx = tuple(int(s) // 2 for s in p.shape)
        fds = []
        for h in (1e-6, 1e-8):
            with torch.no_grad():
                p[idx] += h
                up = loss(TR.train_network(params, buffers, tabs, feats, torch.float64, 0.02)[0])
                p[idx] -= 2 * h
                dn = loss(TR.train_network(params, buffers, tabs, feats, torch.float64, 0.02)[0])
                p[idx] += h
            fds.append(float((up - dn) / (2 * h)))
        want = float(grads[n][idx])
        assert min(abs(fd - want) for fd in fds) <= 1e-5 * max(1.0, abs(want)), (n, fds, want)
