"""CPU: tests/sparse_ref.py (the float64 dense restatement the GPU sparse-convolution tests compare against) agrees with a direct
dictionary-of-coordinates double loop written from the definition: about 40 voxels with negative and odd coordinates in two
scenes that share xyz; kernel sizes 3 and 5, kernel 2 with stride 2 and its transpose, at tensor strides 1 and 2; to 1e-12."""
import pytest
import torch

from tests import sparse_ref as R


def _voxels(seed=3, n=40, s=1):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randint(-5, 4, (3 * n, 3), generator=g)
    xyz = torch.unique(xyz, dim=0)[torch.randperm(torch.unique(xyz, dim=0).shape[0], generator=g)][:n // 2]
    a = torch.cat([torch.zeros(len(xyz), 1, dtype=torch.long), xyz], 1)
    b = torch.cat([torch.ones(len(xyz) - 3, 1, dtype=torch.long), xyz[3:]], 1)        # scene 1 shares xyz with scene 0
    c = torch.cat([a, b])
    c[:, 1:] *= s
    return c[torch.randperm(c.shape[0], generator=g)]


def _dict_conv(cin, x, W, offs, s, cout_coords, absolute=False):
    """out[o] = sum_k x[row of cout_coords[o] + offs[k] * s] @ W[k], by dictionary lookup."""
    rows = {tuple(int(v) for v in c): i for i, c in enumerate(cin)}
    out = torch.zeros(len(cout_coords), W.shape[2], dtype=torch.float64)
    for o, c in enumerate(cout_coords):
        b, xx, yy, zz = (int(v) for v in c)
        for k, (dx, dy, dz) in enumerate(offs):
            i = rows.get((b, xx + dx * s, yy + dy * s, zz + dz * s))
            if i is not None:
                out[o] += (x[i].abs() @ W[k].abs()) if absolute else (x[i] @ W[k])
    return out


def _close(a, b):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("k,s", [(3, 1), (5, 1), (3, 2)])
def test_odd_kernels(k, s, absolute):
    c = _voxels(s=s)
    assert int(c[:, 1:].min()) < 0 and len(c) >= 35
    g = torch.Generator().manual_seed(k)
    x = torch.randn(len(c), 3, generator=g, dtype=torch.float64)
    W = torch.randn(k ** 3, 3, 4, generator=g, dtype=torch.float64)
    want = _dict_conv(c, x, W, R.offsets(k), s, c, absolute)
    _close(R.conv(c, x, W, k, s, absolute), want)
    _close(R.conv_table(x, R.table(c, s, c, R.offsets(k)), W, absolute), want)
    assert R.offsets(3)[0] == (-1, -1, -1) and R.offsets(3)[1] == (0, -1, -1) and R.offsets(3)[3] == (-1, 0, -1)   # x fastest


@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("s", [1, 2])
def test_stride2_and_transpose(s, absolute):
    c = _voxels(seed=5, s=s)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(len(c), 3, generator=g, dtype=torch.float64)
    W = torch.randn(8, 3, 4, generator=g, dtype=torch.float64)
    cc, y = R.conv_down(c, x, W, s, absolute)
    # coarse coordinates: distinct (b, floor(xyz / 2s) * 2s), floor for negatives
    want_cc = sorted({(int(b), *(int(v) // (2 * s) * (2 * s) for v in xyz)) for b, *xyz in c.tolist()})
    assert [tuple(r) for r in cc.tolist()] == want_cc
    want = _dict_conv(c, x, W, R.offsets(2), s, cc, absolute)
    _close(y, want)
    _close(R.conv_table(x, R.table(c, s, cc, R.offsets(2)), W, absolute), want)
    # transposed: every fine voxel takes its parent's row times the kernel slice of (fine - parent) / s
    Wt = torch.randn(8, 4, 2, generator=g, dtype=torch.float64)
    rows = {tuple(r): i for i, r in enumerate(cc.tolist())}
    want_up = torch.zeros(len(c), 2, dtype=torch.float64)
    for f, (b, *xyz) in enumerate(c.tolist()):
        par = [v // (2 * s) * (2 * s) for v in xyz]
        d = [(v - p) // s for v, p in zip(xyz, par)]
        kk = d[0] + 2 * d[1] + 4 * d[2]
        yi, wk = y[rows[(b, *par)]], Wt[kk]
        want_up[f] = (yi.abs() @ wk.abs()) if absolute else (yi @ wk)
    _close(R.conv_up(cc, y, Wt, c, s, absolute), want_up)
    _close(R.conv_table(y, R.up_table(cc, c, s), Wt, absolute), want_up)


def test_scenes_do_not_see_each_other():
    c = _voxels()
    x = torch.randn(len(c), 2, dtype=torch.float64)
    W = torch.randn(27, 2, 2, dtype=torch.float64)
    both = R.conv(c, x, W, 3, 1)
    m = c[:, 0] == 0
    c0 = c[m]
    alone = R.conv(c0, x[m], W, 3, 1)
    _close(both[m], alone)
