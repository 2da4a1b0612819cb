"""pq3d_amd.losses.bce_with_logits_mean / ground_loss / Query3DLoss (csrc/ground.hip) against the float64 restatement
tests/ground_eval_ref.py.

Bars.  The reference's own formula, F.binary_cross_entropy_with_logits(torch.clamp(x, min=-100), y) with autograd in fp32 on the
CPU, is measured against float64 on the same inputs; the kernel may miss float64 by 4 x that, with a floor for inputs where
the reference happens to be exact: 8 fp32 ulps of the loss, 4 fp32 ulps of 1 / N per gradient element.  Measured on an MI355X
(loss error / bar in fp32 ulps of the loss; largest gradient error / bar in fp32 ulps of 1 / N; the reference's own fp32 errors
in brackets -- the kernels keep everything but log1p(exp(.)) in float64 and round once, so they sit at half an ulp):

    N           loss: error  bar   (reference)      gradient: error  bar   (reference)
    1                 0.327  8.00  (0.327)                    0.142  4.00  (0.358)
    63                0.282  8.00  (0.718)                    0.492  4.00  (0.765)
    64                0.486  8.00  (0.514)                    0.246  4.00  (0.613)
    65                0.276  8.00  (0.276)                    0.499  5.35  (1.337)
    257               0.092  8.00  (0.092)                    0.500  5.98  (1.495)
    5 * 80 + 3        0.297  8.00  (0.297)                    0.494  4.72  (1.180)
    128 * 80          0.434  8.00  (0.434)                    0.500  6.31  (1.578)

Each case prints its figures (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import ground_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 257, 5 * 80 + 3, 128 * 80]
PLANTED = [-np.inf, -100.0, -100.5, -1e4, 0.0, 88.0]


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def make_case(N, seed=0):
    """Logits in [-12, 12] with the planted values, 0-1 labels with 0 to 3 ones per row of 80 slots; the -inf slot has label 0,
    the slot at exactly -100 label 1 (so that the gradient the clamp passes there is not a rounding of 0)."""
    rng = np.random.default_rng(1000 + N + seed)
    x = (rng.random(N) * 24 - 12).astype(np.float32)
    y = np.zeros(N, dtype=np.float32)
    W = min(N, 80)
    for r in range((N + W - 1) // W):
        lo, hi = r * W, min(N, (r + 1) * W)
        y[lo + rng.choice(hi - lo, min(r % 4, hi - lo), replace=False)] = 1
    if N >= 63:
        at = rng.choice(N, len(PLANTED), replace=False)
        x[at] = PLANTED
        y[at[0]] = 0
        y[at[1]] = 1
    return x, y


def reference_fp32(x, y, weight=1.0, add=None):
    """The reference's formula in fp32 on the CPU: loss and gradient."""
    t = torch.tensor(x, requires_grad=True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(torch.clamp(t, min=-100), torch.tensor(y))
    if weight != 1.0:
        loss = loss * weight
    if add is not None:
        loss = loss + add
    loss.backward()
    return float(loss.detach()), t.grad.numpy()


def run_kernel(x, y, weight=1.0, add=None, shape=None):
    from pq3d_amd.losses import bce_with_logits_mean
    t = torch.tensor(x, device=DEV).view(shape or x.shape).requires_grad_(True)
    a = None if add is None else torch.tensor(add, dtype=torch.float32, device=DEV)
    loss = bce_with_logits_mean(t, torch.tensor(y, device=DEV).view(shape or y.shape), weight, a)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    return loss.item(), t.grad.reshape(-1).cpu().numpy()


@pytest.mark.parametrize("N", SIZES)
def test_loss_and_gradient_against_float64(N):
    x, y = make_case(N)
    want, gwant = R.bce_logits_mean(x, y), R.bce_logits_grad(x, y)
    ref, gref = reference_fp32(x, y)
    bar = max(4 * abs(ref - want), 8 * ulp32(want))
    gbar = max(4 * float(np.abs(gref - gwant).max()), 4 * ulp32(1.0 / N))
    got, ggot = run_kernel(x, y, shape=(128, 80) if N == 128 * 80 else None)
    gerr = float(np.abs(ggot - gwant).max())
    print(f"N {N}: loss err {abs(got - want) / ulp32(want):.3f} ulp (bar {bar / ulp32(want):.2f}, reference {abs(ref - want) / ulp32(want):.3f}); "
          f"grad err {gerr / ulp32(1.0 / N):.3f} ulp(1/N) (bar {gbar / ulp32(1.0 / N):.2f}, reference "
          f"{float(np.abs(gref - gwant).max()) / ulp32(1.0 / N):.3f})")
    assert abs(got - want) <= bar
    assert gerr <= gbar
    # exact: no gradient below the clamp (the -inf slot included), the formula's gradient AT -100
    below = x < -100
    assert np.array_equal(ggot[below].view(np.int32), np.zeros(int(below.sum()), dtype=np.int32))
    at = x == -100
    assert np.array_equal(ggot[at], gwant[at].astype(np.float32)) and (N < 63 or (ggot[at] == np.float32(-1.0 / N)).all())
    assert (ggot[~below] != 0).all()


def test_nan_weight_add_and_determinism():
    x, y = make_case(257, seed=1)
    want = R.bce_logits_mean(x, y, 10.0, 0.375)
    ref, gref = reference_fp32(x, y, 10.0, 0.375)
    a, ga = run_kernel(x, y, 10.0, 0.375)
    b, gb = run_kernel(x, y, 10.0, 0.375)
    assert abs(a - want) <= max(4 * abs(ref - want), 8 * ulp32(want))
    gwant = R.bce_logits_grad(x, y, 10.0)
    assert np.abs(ga - gwant).max() <= max(4 * float(np.abs(gref - gwant).max()), 4 * ulp32(10.0 / 257))   # (gradients of size weight / N)
    assert a == b and np.array_equal(ga.view(np.int32), gb.view(np.int32))         # two runs: the same bits
    xn = x.copy()
    xn[7] = np.nan
    got, g = run_kernel(xn, y)
    assert np.isnan(got) and np.isnan(g[7]) and np.isfinite(np.delete(g, 7)).all()


def test_add_carries_the_gradient_and_inplace_scaling_works():
    from pq3d_amd.losses import bce_with_logits_mean
    x, y = make_case(65, seed=2)
    t = torch.tensor(x, device=DEV, requires_grad=True)
    other = torch.tensor(1.5, device=DEV, requires_grad=True)
    loss = bce_with_logits_mean(t, torch.tensor(y, device=DEV), 2.0, other * 1.0)
    loss /= 2                                                                       # in place, before backward
    loss.backward()
    assert other.grad.item() == 0.5
    gwant = R.bce_logits_grad(x, y, 2.0, 0.5)
    assert np.abs(t.grad.cpu().numpy() - gwant).max() <= 4 * ulp32(1.0 / 65)
    assert abs(loss.item() - (R.bce_logits_mean(x, y, 2.0, 1.5) / 2)) <= 8 * ulp32(loss.item())


def test_ground_loss_branches_and_query3d_loss():
    from pq3d_amd.losses import Query3DLoss, ground_loss
    rng = np.random.default_rng(3)
    B, O, T, V = 5, 7, 4, 19
    gl = (rng.random((B, O)) * 8 - 4).astype(np.float32)
    gl[:, 5:] = -np.inf
    lab = np.zeros((B, O), dtype=np.float32)
    lab[np.arange(B), rng.integers(0, 5, B)] = 1
    gen, gt = rng.standard_normal((B, T, V)).astype(np.float32), rng.integers(0, V, (B, T))
    gt[0, 3] = -100
    dd = dict(og3d_logits=torch.tensor(gl, device=DEV), tgt_object_id=torch.tensor(lab, device=DEV),
              generation_logits=torch.tensor(gen, device=DEV), generation_label=torch.tensor(gt, device=DEV))
    w_bce = R.bce_logits_mean(gl, lab)
    assert abs(ground_loss(dd).item() - w_bce) <= 8 * ulp32(w_bce)                   # og3d_logits / tgt_object_id fall-back
    idx = dict(ground_logits=dd["og3d_logits"], ground_label=torch.tensor(lab.argmax(1), device=DEV))
    w_ce = torch.nn.functional.cross_entropy(torch.clamp(torch.tensor(gl, dtype=torch.float64), min=-100), torch.tensor(lab.argmax(1))).item()
    assert abs(ground_loss(idx).item() - w_ce) <= 8 * ulp32(w_ce)                    # index labels: the CE branch
    w_gen = torch.nn.functional.cross_entropy(torch.tensor(gen, dtype=torch.float64).flatten(0, 1), torch.tensor(gt).flatten()).item()
    crit = Query3DLoss(["ground_loss", "generation_loss"], {"ground_loss": 10})
    total, losses = crit(dd)
    assert list(losses) == ["ground_loss", "generation_loss", "total_loss"] and losses["total_loss"] is total
    assert abs(losses["ground_loss"].item() - 10 * w_bce) <= 8 * ulp32(10 * w_bce)
    assert abs(losses["generation_loss"].item() - w_gen) <= 8 * ulp32(w_gen)
    assert total.item() == (losses["ground_loss"] + losses["generation_loss"]).item()
    chained = crit.total(dd).item()
    assert abs(chained - (10 * w_bce + w_gen)) <= 8 * ulp32(chained)
    with pytest.raises(NotImplementedError):
        Query3DLoss(["og3d_loss"])


def test_query3d_loss_on_a_tiny_model_in_a_captured_graph():
    """A stage-2 model with a grounding and a caption head (d = 64, L = 2, O = 3) feeds Query3DLoss; loss and gradients of the
    two heads' logits, captured and replayed on the outputs of a second batch, equal the eager result bit for bit."""
    from pq3d_amd import synth
    from pq3d_amd.losses import Query3DLoss
    from pq3d_amd.model import Query3DUnified, make_cfg
    from tests import util
    _z, a = util.load_fixture("F8_t5_head")
    model = Query3DUnified(make_cfg(d=64, H=4, L=2, memories=["voxel", "mv"], heads=["ground", "generation"], t5=a["hf_config"]),
                           compute="fp32")
    synth.fill_module(model, 0)
    model.to(DEV).train()
    crit = Query3DLoss(["ground_loss", "generation_loss"], {"ground_loss": 10})

    def outputs(seed):
        dd = synth.synth_data_dict(4, 64, 3, {"voxel": 64, "mv": 64}, seed=seed, memories=["voxel", "mv"], query_valid_min=1)
        g = torch.Generator().manual_seed(seed)
        dd["response"] = torch.randint(2, 128, (4, 6), generator=g)
        dd["tgt_object_id"] = (torch.rand(4, 3, generator=g) < 0.4).float() * dd["query_pad_masks"]
        with torch.no_grad():
            out = model({k: v.to(DEV) for k, v in dd.items()})
        assert out["ground_label"] is out["tgt_object_id"] and tuple(out["ground_logits"].shape) == (4, 3)
        return out["ground_logits"].clone(), out["generation_logits"].float().clone(), out["generation_label"].clone(), \
            out["ground_label"].clone()

    first, second = outputs(5), outputs(6)
    assert torch.isneginf(first[0]).any() or torch.isneginf(second[0]).any()
    static = [t.clone() for t in first]
    static[0].requires_grad_(True)
    static[1].requires_grad_(True)

    def step():
        dd = dict(ground_logits=static[0], generation_logits=static[1], generation_label=static[2], ground_label=static[3])
        loss = crit.total(dd)
        return (loss,) + torch.autograd.grad(loss, static[:2])

    def eager(vals):
        with torch.no_grad():
            for s, v in zip(static, vals):
                s.copy_(v)
        return [t.clone() for t in step()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        want = [eager(first), eager(second)]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    for vals, w in ((second, want[1]), (first, want[0])):
        with torch.no_grad():
            for st, v in zip(static, vals):
                st.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(res, w):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, ref.view(torch.int32))
    assert not torch.equal(want[0][0], want[1][0]) and torch.isfinite(want[0][0])
