"""GPU: the launches of the grouped Linear+LayerNorm op (ops.linear_ln_group), forward and backward, as (entry point, work key)
in order -- recorded on the commit before the op's equal-rows and unequal-rows bodies became one, asserted as literals here."""
import pytest
import torch

from pq3d_amd import modules, ops
from pq3d_amd._lib import BF16, BF16X3
from tests.enc_common import DEV, _params, _record_launches, rnd

pytestmark = pytest.mark.gpu

# name: (rows per group, K, N, inputs require gradients)
CASES = {
    "equal_97": ((97, 97, 97), 256, 256, False),
    "equal_2049_dx": ((2049, 2049, 2049), 256, 256, True),
    "two_launch_n768": ((40, 40), 256, 768, False),
    "k5_fp32_dlin": ((40, 40), 5, 256, False),          # K of test_gpu_ops.py::test_linear_fwd_bwd's (129, 5, 8)
    "unequal_per_class": ((97, 2049, 33), 256, 256, False),
    "unequal_one_wgrad": ((2049, 2305, 4097), 256, 256, False),
    "unequal_dx_split": ((40, 24, 40), 256, 256, True),
}

EXPECTED = {
    "equal_97": [("pq3d_linear_ln_fwd", "R97N256K256g3"), ("pq3d_add_ln_bwd", "R97d256M3i"), ("pq3d_gemm_tt_multi", "ttmulti3")],
    "equal_2049_dx": [("pq3d_linear_ln_fwd", "R2049N256K256g3"), ("pq3d_add_ln_bwd", "R2049d256M3i"),
                      ("pq3d_gemm", "M256N256K2049g3b1TTs10ct1"), ("pq3d_gemm", "M2049N256K256g3b1NTct1")],
    "two_launch_n768": [("pq3d_gemm", "M40N768K256g2b1NNct2"), ("pq3d_add_ln_fwd", "R40d768M2i"), ("pq3d_add_ln_bwd", "R40d768M2i"),
                        ("pq3d_gemm_tt_multi", "ttmulti2")],
    "k5_fp32_dlin": [("pq3d_gemm", "M40N256K5g2b1NNct2"), ("pq3d_add_ln_fwd", "R40d256M2i"), ("pq3d_add_ln_bwd", "R40d256M2i"),
                     ("pq3d_gemm", "M256N5K40g2b1TTs2ct1"), ("pq3d_colsum", None), ("pq3d_colsum", None)],
    "unequal_per_class": [("pq3d_linear_ln_fwd", "R97+2049+33N256K256"), ("pq3d_add_ln_bwd", "R97+2049+33d256i"),
                          ("pq3d_gemm_tt_multi", "ttmulti1"), ("pq3d_gemm", "M256N256K2049g1b1TTs16ct1"),
                          ("pq3d_gemm_tt_multi", "ttmulti1")],
    "unequal_one_wgrad": [("pq3d_linear_ln_fwd", "R2049+2305+4097N256K256"), ("pq3d_add_ln_bwd", "R2049+2305+4097d256i"),
                          ("pq3d_gemm", "M256N256K2049+2305+4097TTs2ct1")],
    "unequal_dx_split": [("pq3d_linear_ln_fwd", "R40N256K256g2"), ("pq3d_linear_ln_fwd", "R24N256K256g1"),
                         ("pq3d_add_ln_bwd", "R24d256M1i"), ("pq3d_gemm_tt_multi", "ttmulti1"), ("pq3d_gemm", "M24N256K256g1b1NTct1"),
                         ("pq3d_add_ln_bwd", "R40d256M2i"), ("pq3d_gemm_tt_multi", "ttmulti2"), ("pq3d_gemm", "M40N256K256g2b1NTct1")],
    "single_encoder": [("pq3d_linear_ln_fwd", "R33N256K64g1"), ("pq3d_add_ln_bwd", "R33d256M1i"), ("pq3d_gemm_tt_multi", "ttmulti1")],
}


def _run(name, rows, K, n, need_dx, monkeypatch):
    xs = [rnd(R, K, seed=40 + g).to(DEV).requires_grad_(need_dx) for g, R in enumerate(rows)]
    par = [[t.requires_grad_(True) for t in ts] for ts in _params(len(rows), K, n)]
    gy = [rnd(R, n, seed=90 + g).to(DEV) for g, R in enumerate(rows)]
    seen = _record_launches(monkeypatch)
    ys = ops.linear_ln_group(xs, *par, ct=BF16X3)
    torch.autograd.backward(list(ys), gy)
    print(f"{name}: {seen!r}")
    return seen, xs, par


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence(name, monkeypatch):
    """Every launch of one forward + backward, in order, with the key that names it for the profiler.  equal_2049_dx ends with the
    grouped dx GEMM; two_launch_n768 takes the grouped GEMM + pq3d_add_ln_fwd forward; k5_fp32_dlin cannot carry the bias gradient
    on the product (fp32 dlin, pq3d_colsum launches follow); unequal_per_class has one weight-gradient launch per class of equal
    row count, classes in order of first appearance; unequal_one_wgrad one pq3d_gemm with a reduction length per group;
    unequal_dx_split one op per class."""
    rows, K, n, need_dx = CASES[name]
    seen, xs, par = _run(name, rows, K, n, need_dx, monkeypatch)
    assert all(p.grad is not None for ps in par for p in ps) and all((x.grad is not None) == need_dx for x in xs)
    assert seen == EXPECTED[name]
    if need_dx:
        assert seen[-1][0] == "pq3d_gemm"


def test_launch_sequence_single_encoder(monkeypatch):
    """modules.linear_ln_forward's call: G = 1, R = 33, K = 64, split-bf16 in 'bf16' mode."""
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.LayerNorm(256)).to(DEV)
    seen = _record_launches(monkeypatch)
    y = modules.linear_ln_forward(seq, rnd(33, 64, seed=40).to(DEV), BF16)
    y.backward(rnd(33, 256, seed=90).to(DEV))
    print(f"single_encoder: {seen!r}")
    assert all(p.grad is not None for p in seq.parameters())
    assert seen == EXPECTED["single_encoder"]
