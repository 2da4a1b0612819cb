"""CPU: the attention launch plan (pq3d_amd/attn.py) -- key-split factors and workspace sizes on the shipped shapes.  Pure decisions
on integers and dtypes: nothing here launches.  The factors mirror eligibility tests of the C++ dispatchers (attn_resident.hip,
attn_x3.hip); a drift costs speed silently, so the shipped shapes are pinned here."""
import pytest
import torch

from pq3d_amd import attn as A
from pq3d_amd._lib import BF16, BF16X3, F32

bf, f32 = torch.bfloat16, torch.float32
# (stacked scenes B * M, H, Lq, Lk, dh, 3-D mask) -> factors: bf16 fwd, bf16 bwd, fp32 fwd, fp32 bwd, plane fwd (None: not asserted)
ANCHORS = {
    "c2": ((24, 8, 100, 1024, 32, False), (1, 1, 2, 2, 1)),
    "c5": ((48, 8, 100, 2048, 32, False), (2, 1, 2, 2, 2)),
    "c4": ((12, 8, 200, 4096, 32, True), (4, 2, 4, 4, 4)),
    "stage1": ((12, 12, 100, 2048, 64, False), (2, 4, 2, 2, 4)),
    "stage2": ((128, 12, 80, 80, 64, False), (1, 1, 1, 1, 1)),
    "edge_7_key_blocks": ((24, 8, 100, 448, 32, False), (1, 1, 1, 1, None)),
    "edge_8_key_blocks": ((24, 8, 100, 512, 32, False), (1, 1, 2, 2, None)),
}
# (ct, q dtype, bwd, planes) of the five columns
COLUMNS = [(BF16, bf, False, False), (BF16, bf, True, False), (F32, f32, False, False), (F32, f32, True, False),
           (BF16X3, f32, False, True)]


def factors(B, H, Lq, Lk, dh, mask, bias=False):
    return [A.key_splits(B, H, Lq, Lk, dh, ct, qdt, bwd=bwd, bias=bias, mask=mask, planes=planes)
            for ct, qdt, bwd, planes in COLUMNS]


@pytest.mark.parametrize("name", list(ANCHORS))
def test_key_split_anchors(name):
    shape, want = ANCHORS[name]
    got = factors(*shape)
    assert [g for g, w in zip(got, want) if w is not None] == [w for w in want if w is not None], (name, got)


@pytest.mark.parametrize("name", list(ANCHORS))
def test_additive_bias_forces_one_pass(name):
    # (the plane forward takes no bias at all: pq3d_attn_fwd_x3 refuses it, so that column has no bias row)
    assert factors(*ANCHORS[name][0], bias=True)[:4] == [1, 1, 1, 1]


@pytest.mark.parametrize("name", list(ANCHORS))
@pytest.mark.parametrize("mul", [2, 7])
def test_forward_factors_do_not_depend_on_the_batch(name, mul):
    (B, *rest), _ = ANCHORS[name]
    fwd = [i for i, c in enumerate(COLUMNS) if not c[2]]
    one, many = factors(B, *rest), factors(B * mul, *rest)
    assert [one[i] for i in fwd] == [many[i] for i in fwd]


def test_workspace_size():
    assert A.ws_elems(1, 24, 8, 100, 32) == 0 and A.ws_elems(0, 24, 8, 100, 32) == 0
    for ks, B, H, Lq, dh in ((2, 24, 8, 100, 32), (4, 12, 8, 200, 32), (4, 12, 12, 100, 64), (2, 2, 2, 16, 32)):
        assert A.ws_elems(ks, B, H, Lq, dh) == ks * B * H * Lq * (dh + 2)
