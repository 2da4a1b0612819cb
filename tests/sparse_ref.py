"""Float64 restatement of the sparse 3-D convolutions of the voxel backbone (pq3d_amd/sparse.py, csrc/sparse_conv.hip), written
against the DEFINITION and sharing no code with the package: the features are scattered into a dense grid shifted by the
minimum coordinate, ``torch.nn.functional.conv3d`` / ``conv_transpose3d`` runs with the kernel re-indexed from the offset order
(x fastest, then y, then z), and the result is read back at the output coordinates.  tests/test_sparse_ref.py keeps this file
honest against a dictionary-of-coordinates double loop.

    coords        [N, 1+3] integer (batch, x, y, z), distinct rows; features [N, C] in the same row order
    level_coords  the distinct (b, floor(xyz / s) * s), lexicographically sorted (``unique`` on the host)
    conv          odd kernel k at tensor stride s (same coordinates in and out): offsets {-(k//2)..k//2} * s
    conv_down     kernel 2, stride 2: out at level 2s, offsets {0, 1} * s
    conv_up       transposed kernel 2, stride 2 onto given fine coordinates: offset (fine - parent) / s_fine
Every function takes ``absolute=True`` for the sum of |x| |W| (the per-element error bound's scale) and works in the dtype of
its inputs.  ``table`` / ``conv_table`` are the same definition through an index grid (row ids scattered into a dense integer
grid, neighbours read by shifting): what the whole-network restatement uses, where a dense grid per channel is too large.
"""
import torch
import torch.nn.functional as F


def offsets(k):
    """[(dx, dy, dz)] in kernel-index order: x fastest."""
    r = range(-(k // 2), k // 2 + 1) if k % 2 else range(k)
    return [(dx, dy, dz) for dz in r for dy in r for dx in r]


def level_coords(coords, s):
    c = coords.long().cpu()
    q = torch.cat([c[:, :1], torch.div(c[:, 1:], s, rounding_mode="floor") * s], 1)
    return torch.unique(q, dim=0)


def _grid(q, feats, origin, shape):
    """dense [B, C, X, Y, Z] with feats at q - origin"""
    B = int(q[:, 0].max()) + 1
    g = torch.zeros(B, feats.shape[1], *shape, dtype=feats.dtype)
    p = q[:, 1:] - origin
    g[q[:, 0], :, p[:, 0], p[:, 1], p[:, 2]] = feats
    return g


def _read(g, q, origin):
    p = q[:, 1:] - origin
    return g[q[:, 0], :, p[:, 0], p[:, 1], p[:, 2]]


def _w_conv(W, k):     # [K, Cin, Cout], K index = x + k y + k^2 z  ->  conv3d's [Cout, Cin, kx, ky, kz] on an (X, Y, Z) grid
    return W.reshape(k, k, k, W.shape[1], W.shape[2]).permute(4, 3, 2, 1, 0).contiguous()


def conv(coords, feats, W, k, s, absolute=False):
    """out[o] = sum_d feats[row of coords[o] + d s] W[index of d], d over the k^3 centred offsets."""
    c = coords.long().cpu()
    q = torch.cat([c[:, :1], torch.div(c[:, 1:], s, rounding_mode="floor")], 1)
    assert bool((q[:, 1:] * s == c[:, 1:]).all()), "coordinates are not at tensor stride s"
    x, W = (feats.abs(), W.abs()) if absolute else (feats, W)
    origin = q[:, 1:].min(0).values
    shape = (q[:, 1:].max(0).values - origin + 1).tolist()
    y = F.conv3d(_grid(q, x.cpu(), origin, shape), _w_conv(W.cpu(), k), padding=k // 2)
    return _read(y, q, origin)


def conv_down(coords, feats, W, s, absolute=False):
    """kernel 2, stride 2 from level s to level 2 s.  Returns (coarse coordinates, features)."""
    c = coords.long().cpu()
    q = torch.cat([c[:, :1], torch.div(c[:, 1:], s, rounding_mode="floor")], 1)
    x, W = (feats.abs(), W.abs()) if absolute else (feats, W)
    origin = torch.div(q[:, 1:].min(0).values, 2, rounding_mode="floor") * 2        # even: the 2-blocks line up with the grid
    shape = [int(v) + (int(v) & 1) for v in (q[:, 1:].max(0).values - origin + 1)]
    y = F.conv3d(_grid(q, x.cpu(), origin, shape), _w_conv(W.cpu(), 2), stride=2)
    cc = level_coords(c, 2 * s)
    qc = torch.cat([cc[:, :1], torch.div(cc[:, 1:], 2 * s, rounding_mode="floor")], 1)
    return cc, _read(y, qc, torch.div(origin, 2, rounding_mode="floor"))


def conv_up(coarse, feats, W, fine, s_fine, absolute=False):
    """transposed kernel 2, stride 2: out[f] = feats[parent(f)] W[index of (f - parent(f)) / s_fine] at the given fine coordinates."""
    cc, cf = coarse.long().cpu(), fine.long().cpu()
    qc = torch.cat([cc[:, :1], torch.div(cc[:, 1:], 2 * s_fine, rounding_mode="floor")], 1)
    qf = torch.cat([cf[:, :1], torch.div(cf[:, 1:], s_fine, rounding_mode="floor")], 1)
    x, W = (feats.abs(), W.abs()) if absolute else (feats, W)
    origin = qc[:, 1:].min(0).values
    shape = (qc[:, 1:].max(0).values - origin + 1).tolist()
    wt = W.cpu().reshape(2, 2, 2, W.shape[1], W.shape[2]).permute(3, 4, 2, 1, 0).contiguous()   # [Cin, Cout, kx, ky, kz]
    y = F.conv_transpose3d(_grid(qc, x.cpu(), origin, shape), wt, stride=2)
    return _read(y, qf, 2 * origin)


# ---- the same definition through an index grid ------------------------------------------------------------------------
def table(coords_in, s_in, coords_out, offs):
    """[N_out, K] long: row of ``coords_in`` (tensor stride s_in) at coords_out + offs[k] * s_in, -1 where there is none."""
    ci, co = coords_in.long().cpu(), coords_out.long().cpu()
    qi = torch.cat([ci[:, :1], torch.div(ci[:, 1:], s_in, rounding_mode="floor")], 1)
    qo = torch.cat([co[:, :1], torch.div(co[:, 1:], s_in, rounding_mode="floor")], 1)
    o = torch.tensor(offs)
    lo = torch.minimum(qi[:, 1:].min(0).values, qo[:, 1:].min(0).values + o.min(0).values)
    hi = torch.maximum(qi[:, 1:].max(0).values, qo[:, 1:].max(0).values + o.max(0).values)
    B = int(max(qi[:, 0].max(), qo[:, 0].max())) + 1
    g = torch.full((B, *(hi - lo + 1).tolist()), -1, dtype=torch.long)
    p = qi[:, 1:] - lo
    g[qi[:, 0], p[:, 0], p[:, 1], p[:, 2]] = torch.arange(ci.shape[0])
    cols = []
    for d in o:
        p = qo[:, 1:] + d - lo
        cols.append(g[qo[:, 0], p[:, 0], p[:, 1], p[:, 2]])
    return torch.stack(cols, 1)


def up_table(coarse, fine, s_fine):
    """[N_fine, 8] long: the parent's row in the column of offset (fine - parent) / s_fine, -1 elsewhere."""
    cf = fine.long().cpu()
    par = torch.cat([cf[:, :1], torch.div(cf[:, 1:], 2 * s_fine, rounding_mode="floor") * 2 * s_fine], 1)
    t = table(coarse, 2 * s_fine, par, [(0, 0, 0)])[:, 0]
    d = torch.div(cf[:, 1:] - par[:, 1:], s_fine, rounding_mode="floor")
    out = torch.full((cf.shape[0], 8), -1, dtype=torch.long)
    out[torch.arange(cf.shape[0]), d[:, 0] + 2 * d[:, 1] + 4 * d[:, 2]] = t
    return out


def conv_table(feats, tab, W, absolute=False, rnd=None):
    """sum_k feats[tab[:, k]] @ W[k] in the dtype of ``feats``; ``rnd`` (optional) rounds both operands first (bf16 emulation)."""
    x, W = (feats.abs(), W.abs()) if absolute else (feats, W)
    if rnd is not None:
        x, W = rnd(x), rnd(W)
    out = torch.zeros(tab.shape[0], W.shape[2], dtype=x.dtype)
    xz = torch.cat([x, torch.zeros(1, x.shape[1], dtype=x.dtype)])      # row -1 -> zeros
    for k in range(tab.shape[1]):
        if bool((tab[:, k] >= 0).any()):
            out += xz[tab[:, k]] @ W[k]
    return out
