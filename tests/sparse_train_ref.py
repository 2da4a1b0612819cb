"""Reference helpers for TRAINING the voxel backbone (pq3d_amd/sparse.py: Res16UNet34C(trainable=True)), built on the float64
restatement tests/sparse_ref.py and plain torch autograd; they share no code with the package.  tests/test_sparse_train_ref.py
keeps them honest on the CPU.

    conv_grads         (dX, dW) of sparse_ref.conv_table by autograd, and their |.| forms: the per-element error bounds' scale
    pair_counts        how many (output row, offset) pairs feed an input row / an offset: the bounds' term count
    RoundOperands / RoundGrad   bf16 emulation of a product's forward operands and of the gradient entering both backward products
    train_network      tests/test_gpu_voxel_backbone.py::ref_network with batch-statistics BatchNorm (training mode) and the
                       running-buffer update of nn.BatchNorm1d
"""
import torch

from tests import sparse_ref as R

LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)
DOWN = ("conv1p1s2", "conv2p2s2", "conv3p4s2", "conv4p8s2")
UP = ("convtr4p16s2", "convtr5p8s2", "convtr6p4s2", "convtr7p2s2")
EPS = 1e-5


def conv_grads(x, tab, W, dy):
    """float64 (dX, dW, A_x, A_w) of y = conv_table(x, tab, W) under the upstream gradient dy:
    A_x[i, c] = sum |dy| |W| over the pairs that use input row i, A_w[k, c, n] = sum |x| |dy| over the pairs of offset k."""
    x, W, dy = x.double(), W.double(), dy.double()
    xg, Wg = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    dX, dW = torch.autograd.grad(R.conv_table(xg, tab, Wg), (xg, Wg), dy)
    # the product is bilinear: the gradient with respect to one operand does not depend on its value, so ones stand in for it
    ox, oW = torch.ones_like(x).requires_grad_(True), torch.ones_like(W).requires_grad_(True)
    A_x, = torch.autograd.grad(R.conv_table(ox, tab, W, absolute=True), ox, dy.abs())
    A_w, = torch.autograd.grad(R.conv_table(x, tab, oW, absolute=True), oW, dy.abs())
    return dX, dW, A_x, A_w


def pair_counts(tab, n_in):
    """(per input row, per offset) number of present (output row, offset) pairs of the table."""
    present = tab >= 0
    return torch.bincount(tab[present], minlength=n_in), present.sum(0)


def _bf(t):
    return t.bfloat16().to(t.dtype)


class RoundOperands(torch.autograd.Function):
    """forward: the operand rounded to bf16; backward: the gradient unchanged (the product's own gradient is what is wanted)"""
    @staticmethod
    def forward(ctx, t):
        return _bf(t)

    @staticmethod
    def backward(ctx, g):
        return g


class RoundGrad(torch.autograd.Function):
    """forward: identity; backward: the gradient rounded to bf16 -- it is an operand of both backward products"""
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def tables(coords):
    C = [coords.long()] + [R.level_coords(coords, 1 << l) for l in range(1, 5)]
    return dict(C=C, t3=[R.table(C[l], 1 << l, C[l], R.offsets(3)) for l in range(5)], t5=R.table(C[0], 1, C[0], R.offsets(5)),
                dn=[R.table(C[l], 1 << l, C[l + 1], R.offsets(2)) for l in range(4)],
                up=[R.up_table(C[l + 1], C[l], 1 << l) for l in range(4)])


def train_network(params, buffers, tabs, feats, dtype, momentum, bf16=False):
    """The training-mode forward.  ``params``: {name: tensor} of every kernel / bn.weight / bn.bias (leaves that may require
    grad), ``buffers``: {name: tensor} the running statistics and counters.  Returns ([maps 16, 8, 4, 2, 1], new buffers): level
    0 in the caller's row order, coarser levels in the restatement's sorted order.  bf16: operands of every product rounded in
    the forward and in both backward products (fp32 accumulation is torch's)."""
    t3, t5, dn, up = tabs["t3"], tabs["t5"], tabs["dn"], tabs["up"]
    new = {}
    rnd = (lambda t: RoundOperands.apply(t)) if bf16 else (lambda t: t)
    gr = (lambda t: RoundGrad.apply(t)) if bf16 else (lambda t: t)

    def conv(x, tab, name):
        return gr(R.conv_table(rnd(x), tab, rnd(params[name + ".kernel"])))

    def lin(x, name):
        return gr(rnd(x) @ rnd(params[name + ".kernel"]))

    def bn(y, p):
        n = y.shape[0]
        mean, var = y.mean(0), y.var(0, unbiased=False)
        with torch.no_grad():
            unb = var * (n / (n - 1)) if n > 1 else var
            new[p + ".bn.running_mean"] = (1 - momentum) * buffers[p + ".bn.running_mean"].to(dtype) + momentum * mean
            new[p + ".bn.running_var"] = (1 - momentum) * buffers[p + ".bn.running_var"].to(dtype) + momentum * unb
            new[p + ".bn.num_batches_tracked"] = buffers[p + ".bn.num_batches_tracked"] + 1
        return (y - mean) / torch.sqrt(var + EPS) * params[p + ".bn.weight"] + params[p + ".bn.bias"]

    relu = lambda y: y.clamp_min(0)

    def layer(x, p, l, blocks):
        for j in range(blocks):
            q = f"{p}.{j}"
            y = relu(bn(conv(x, t3[l], q + ".conv1"), q + ".norm1"))
            y = bn(conv(y, t3[l], q + ".conv2"), q + ".norm2")
            res = bn(lin(x, q + ".downsample.0"), q + ".downsample.1") if q + ".downsample.0.kernel" in params else x
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
    return maps, new
