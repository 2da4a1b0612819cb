"""CPU: the weight-gradient launch plan (pq3d_amd/wgrad.py) -- split-K depths, path choices and queue buckets on the shipped
shapes.  Pure decisions on CPU tensors: nothing here launches."""
import pytest
import torch

from pq3d_amd import wgrad as W
from pq3d_amd._lib import BF16, F32


def tiles(N, K):
    return ((N + 63) // 64) * ((K + 63) // 64)


@pytest.mark.parametrize("N,K,R,G,ct,layer,flush,long_", [
    (256, 256, 8192, 1, BF16, 32, 48, False),    # one input encoder over config 2's 8192 rows
    (256, 256, 8192, 3, BF16, 10, 16, False),    # config 2's three input encoders in one launch
    (1024, 256, 800, 4, BF16, 2, 3, False),
    (768, 768, 10240, 16, BF16, 1, 1, True),     # stage-2 projections: bf16 operands on 128 x 128 tiles
    (256, 256, 800, 1, F32, 12, 12, False),
])
def test_splitk_and_long_path_anchors(N, K, R, G, ct, layer, flush, long_):
    assert W.splitk(tiles(N, K) * G, R, ct, W.SPLITK_CAP_LAYER) == layer
    assert W.splitk(tiles(N, K) * G, R, ct, W.SPLITK_CAP_FLUSH) == flush
    assert W.dw_long_path(N, K, R, G, ct) == long_


def test_colsum_fusable():
    g, x = torch.empty(800, 256, dtype=torch.bfloat16), torch.empty(800, 256)
    assert W.colsum_fusable([g], [x], None, 256, 256, BF16)
    assert W.colsum_fusable([g], [x], [torch.empty(800, 256)], 256, 256, BF16)
    assert not W.colsum_fusable([g], [x.bfloat16()], [torch.empty(800, 256)], 256, 256, BF16)   # x2 needs an fp32 x
    g12, x12 = torch.empty(800, 12), torch.empty(800, 12)
    assert W.colsum_fusable([g12], [x12], None, 12, 12, F32) and not W.colsum_fusable([g12], [x12], None, 12, 12, BF16)
    assert not W.colsum_fusable([torch.empty(800 * 256 + 1)[1:]], [x], None, 256, 256, BF16)   # misaligned operand


def problems(G, N, K, R):
    return [(torch.empty(R, N), torch.empty(R, K), None, torch.empty(N, K), torch.empty(N)) for _ in range(G)]


def test_tt_multi_selection():
    # the decoder's short reductions: one launch, and it pays
    dec = problems(3, 256, 256, 800)
    assert W.tt_multi_fits(dec, 256, 256, 800, BF16) and W.tt_multi_pays(dec)
    assert not W.tt_multi_fits(dec, 256, 256, 800, F32)
    # config 2's input encoders (8192 rows): long reductions stay on grouped split-K pq3d_gemm
    enc = problems(3, 256, 256, 8192)
    assert not W.tt_multi_ok(*enc[0], 256, 256, 8192) and not W.tt_multi_fits(enc, 256, 256, 8192, BF16)
    # a grouped Linear + LayerNorm backward takes tt_multi whenever it fits, without the pays check of a queue flush
    lng = problems(3, 128, 128, 300)
    assert W.tt_multi_fits(lng, 128, 128, 300, BF16) and not W.tt_multi_pays(lng)


def test_queue_buckets():
    R, N, K = 800, 256, 256
    g, x, x2, dw, db = torch.empty(R, N), torch.empty(R, K), torch.empty(R, K), torch.empty(N, K), torch.empty(N)
    for split_x2, nb in ((True, 3), (False, 2)):
        q = W.Queue(split_x2=split_x2)
        q.add([g, g], [x, x], [x2, None], [dw, dw], BF16, [db, db])
        q.add([g], [x], None, [dw], BF16)
        q.add([g], [x], None, [dw], F32)
        assert len(q.buckets) == nb + 1 and q.nbytes == 9 * R * N * 4   # 4 x (g + x), one x2
        keys = list(q.buckets)
        assert [k[6] for k in keys] == [True] * (nb - 1) + [False, False] and keys[-1][7] == F32
        first = q.buckets[keys[0]]
        assert [p[2] is not None for p in first] == ([True] if split_x2 else [True, False])
        q.flush(run=False)
        assert q.buckets == {} and q.nbytes == 0
