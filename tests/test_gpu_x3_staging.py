"""GPU: the split-bf16 cross-attention forward (csrc/attn_x3.hip) stages its key/value slice piece by piece -- the first blocks run
while later pieces are still in flight.  The staging changes when bytes arrive, never what is computed:

  * bit equality with the kernel before the staging (tests/golden/attn_x3_parent_bits.json: SHA-256 of the outputs per case,
    written by tests/x3_staging_cases.py on that build) at key lengths around the first block, the first piece, the end of stage 1
    and stage 2, for one lane .. two query halves, with key padding that empties a piece and a stage, a 3-D mask as bit words,
    the zero key on and off, dropout, and a key split;
  * the same outputs against the float64 restatement at tests/test_gpu_x3.py's bar (a wrong fixture cannot hide a wrong kernel);
  * the same bits from call to call, also into buffers full of NaN (nothing stale is read from LDS or a previous launch)."""
import json
import os

import pytest
import torch

from tests import x3_staging_cases as XC
from tests.test_gpu_x3 import attn_ref

pytestmark = pytest.mark.gpu
IDS = [XC.case_id(c) for c in XC.CASES]
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_x3_parent_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(IDS) and len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("i", range(len(XC.CASES)), ids=IDS)
def test_bits_equal_the_kernel_before_the_staging(i):
    assert XC.result(i)[-1] == GOLDEN[IDS[i]]


@pytest.mark.parametrize("i", range(len(XC.CASES)), ids=IDS)
def test_matches_float64(i):
    c = XC.CASES[i]
    o, lse, o_bf, q_bf, _ks, _h = XC.result(i)
    q, k, v, kpm, mask = XC.inputs(c)
    (kh, kl), (vh, vl) = XC.planes(k), XC.planes(v)
    kk, vv = kh.double() + kl.double(), vh.double() + vl.double()   # the operands the kernel sees
    keep = None
    if c["drop"]:
        from pq3d_amd import ops
        keep = ops.dropout_mask(XC.B * XC.H * c["Lq"], c["Lk"], XC.drop_of("cuda")).view(XC.B, XC.H, c["Lq"], c["Lk"]).cpu().double() / 0.75
    oref, lref = attn_ref(q.double(), kk, vv, XC.H, kpm, mask, keep)
    if not c["zero"]:   # attn_ref appends the zero key: take it out of the softmax again
        w = 1.0 / (1.0 - torch.exp(-lref))
        oref = oref * w.permute(0, 2, 1)[..., None].expand(-1, -1, -1, c["dh"]).reshape(oref.shape)
        lref = lref + torch.log1p(-torch.exp(-lref))
    s = float(oref.abs().max())
    err, lerr = float((o.double() - oref).abs().max()), float((lse.double() - lref).abs().max())
    print(f"{IDS[i]}: o {err / s:.2e} of scale, lse {lerr:.2e}")
    assert err <= 2e-5 * s
    assert lerr <= 2e-5 * max(1.0, float(lref.abs().max()))
    assert torch.equal(o_bf, o.to(torch.bfloat16))
    assert torch.equal(q_bf, q.to(torch.bfloat16))


STABLE = [i for i, c in enumerate(XC.CASES) if c["Lk"] >= XC.STAGE[c["dh"]] + 64 and c["Lq"] in (100, 200)]


@pytest.mark.parametrize("i", STABLE, ids=[IDS[i] for i in STABLE])
def test_same_bits_from_call_to_call(i):
    c = XC.CASES[i]
    first = XC.run(c)
    h1 = XC.digest(*first)
    h2 = XC.digest(*XC.run(c, out=first[:4]))
    for t in first[:4]:
        t.fill_(float("nan"))
    h3 = XC.digest(*XC.run(c, out=first[:4]))
    assert h1 == h2 == h3 == XC.result(i)[-1]
