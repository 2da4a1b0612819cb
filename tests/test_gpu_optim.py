"""GPU: the optimizer kernels of csrc/optim.hip (pq3d_sumsq_partials, pq3d_train_scalars, pq3d_adamw) against the flat
float64 restatement tests/optim_ref.py (itself checked against torch's optimizer objects by tests/test_optim_ref.py),
EVERY element, never a sample; and TrainStep end to end on a layout of awkward parameter sizes against
torch.optim.AdamW + clip_grad_norm_ + LambdaLR in float64.

Tolerances (u = 2^-24, the fp32 unit roundoff; optim.hip is compiled with -ffp-contract=off and hipcc's correctly
rounded fp32 sqrt and division).  One AdamW step from fp32 inputs p, g, m, v and fp32 scalars lr, step_size S,
inv_bc2s B, coef c, read in float64 by the restatement, rounds at these places:
  g' = c g                                   1 rounding
  p (1 - lr lm wd)                           the factor 3 roundings at a value near 1, the product 1: <= 4u |p|
  m' = m + (g' - m)(1 - b1)                  (1 - b1 is exact): <= u |m'| + 3u (1 - b1)(|g'| + |m|) =: u A
  v' = b2 v + (1 - b2) g'^2                  positive terms: <= 5u |v'|
  d = sqrt(v') B + eps                       <= 6u relative
  S lm m' / d                                m' / d <= (7u |m'| + u A) / d, two more products: <= 10u S lm A / d
  p' = p (1 - ...) - update                  1 rounding: u |p'|
so |p' - p'_64| <= 4u|p| + u|p'| + 10u S lm A / d.  The tests allow twice each bound:
  tol_p = 8u |p| + 2u |p'| + 20u S lm A / d,   tol_m = 2u A,   tol_v = 10u |v'|.
Where the restatement computes the scalars itself (TrainStep against torch), a relative error dc of the clip coefficient
and of the scalars adds dc A to m', 2 dc |v'| to v' and 2 dc S lm A / d to the update (again allowed twice).

The gradient norm is a sum of squares in fp32 along a chain of at most D = 14 + k roundings per term (the square, three
adds inside a float4, k adds of float4 sums per thread, the n % 4 tail's add in block 0, six wave_sum levels, three adds
of the four wave sums); the partials are summed in double.  Relative error of the norm <= (D / 2 + 1) u (the square root
halves it, the cast to fp32 adds u); of the clip coefficient one u more."""
import ctypes as C
import math

import pytest
import torch

from pq3d_amd import _lib as L
from pq3d_amd.trainer import TrainStep
from oracle import train_oracle as T
from tests import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SIZES = [1, 3, 4, 5, 1023, 4097, 3_000_001]     # 3 000 001 > 2048 blocks x 256 x 4: grid-stride loop and a tail
SCHEDULES = [("constant", 1.0), ("warmup_cosine", 1.0), ("warmup_exp", 0.1)]
# warmup_exp's gamma: the reference's get_scheduler (optim/scheduler.py:20-23) calls the lambda without gamma, so its
# warmup_exp cannot run there at all; gamma is train_oracle.warmup_exp's (optim/scheduler.py:11-14's formula)
WINDOWS = [(0, 10, 1), (3, 10, 1), (12, 40, 4)]    # (warmup, total, stride), as in tests/test_optim_ref.py


# -- launches ----------------------------------------------------------------------------------------------------------
def make_hp(lr=1e-2, betas=(0.9, 0.98), eps=1e-8, max_norm=0.0, sched="warmup_cosine", warmup=0, total=10, gamma=1.0,
            stride=1):
    hp = L.AdamWHp()
    hp.lr, hp.beta1, hp.beta2, hp.eps, hp.max_grad_norm = lr, betas[0], betas[1], eps, max_norm
    hp.sched, hp.warmup_steps, hp.total_steps, hp.sched_gamma, hp.sched_stride = L.SCHED[sched], warmup, total, gamma, stride
    return hp


def make_segs(table):
    s = L.OptSegments()
    s.n = len(table)
    for i, (e, lm, wd) in enumerate(table):
        s.end[i], s.lr_mul[i], s.weight_decay[i] = e, lm, wd
    return s


def table_of(segs):
    """The segment table as the kernel holds it (fp32 lr_mul / weight_decay, read back as float64)."""
    return [(segs.end[i], segs.lr_mul[i], segs.weight_decay[i]) for i in range(segs.n)]


def sumsq(g, n, partials):
    L.check(L.lib().pq3d_sumsq_partials(L.ptr(g), n, L.ptr(partials), L.stream()), "pq3d_sumsq_partials")


def train_scalars(hp, step, partials, sc):
    L.check(L.lib().pq3d_train_scalars(C.byref(hp), L.ptr(step), L.ptr(partials), L.ptr(sc), L.stream()),
            "pq3d_train_scalars")


def adamw(p, g, m, v, n, hp, segs, sc):
    L.check(L.lib().pq3d_adamw(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, C.byref(hp), C.byref(segs), L.ptr(sc),
                               L.stream()), "pq3d_adamw")


def run_steps(p0, grads, hp, segs, m0=None, v0=None):
    """TrainStep.optimizer_step's three launches on flat device buffers, once per gradient; returns per step the CPU
    copies (p, m, v, scalars[0:5], step counter)."""
    n = p0.numel()
    p = p0.to(DEV).clone()
    m = (torch.zeros(n) if m0 is None else m0).to(DEV).clone()
    v = (torch.zeros(n) if v0 is None else v0).to(DEV).clone()
    g = torch.empty(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    partials = torch.full((L.SUMSQ_PARTIALS,), float("nan"), device=DEV)
    sc = torch.full((8,), float("nan"), device=DEV)
    out = []
    for gk in grads:
        g.copy_(gk)
        sumsq(g, n, partials)
        train_scalars(hp, step, partials, sc)
        adamw(p, g, m, v, n, hp, segs, sc)
        torch.cuda.synchronize()
        out.append((p.cpu(), m.cpu(), v.cpu(), sc[:5].cpu(), int(step.item())))
    return out


# -- tolerances (module docstring) ---------------------------------------------------------------------------------------
def norm_rtol(n):
    k = -(-(n // 4) // (L.SUMSQ_PARTIALS * 256))      # float4s per thread in sumsq_kernel
    return ((14 + k) / 2 + 1) * U


def step_tol(p, m, gr, p1, m1, v1, s_lm, inv_bc2s, beta1, eps, dc=0.0):
    """(tol_p, tol_m, tol_v) of one fp32 AdamW step; every argument is float64 (a tensor or a scalar): the inputs p, m,
    the clipped gradient gr, the float64 results p1, m1, v1, step_size * lr_mul, 1 / sqrt(bc2)."""
    a = m1.abs() + 3 * (1 - beta1) * (gr.abs() + m.abs())
    d = v1.sqrt() * inv_bc2s + eps
    return (8 * U * p.abs() + 2 * U * p1.abs() + (20 * U + 4 * dc) * s_lm * a / d,
            (2 * U + 2 * dc) * a, (10 * U + 4 * dc) * v1.abs())


def assert_within(what, got, want, tol):
    err = (got.double() - want).abs()
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements off, first at {i}: got "
                             f"{float(got[i])!r} want {float(want[i])!r} (err {float(err[i]):.3e}, tol {float(tol[i]):.3e})")


def per_element(table, n):
    """lr_mul and weight_decay of every element (float64) and the mask of skipped elements."""
    lm, wd = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for s, a, b in R.segment_slices(table, n):
        lm[s], wd[s] = a, b
    return lm, wd, lm < 0


# -- pq3d_adamw, element by element --------------------------------------------------------------------------------------
GRAD_SCALES = [1.0, 0.1, 3.0, 0.5, 2.0]     # max_norm = 1.5 sqrt(n): steps 2 and 4 clip, the others do not (for n >> 1)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("table", ["one", "sixteen", "skip"])
def test_adamw_matches_float64_every_element(n, table):
    """Five consecutive steps, fresh random gradients, state carried over on the device.  Each step is restated in
    float64 from the kernel's own fp32 state before it and the scalars it consumed; the scalars are checked against
    the float64 schedule / clip / norm, the step counter against the step index.  Skipped elements and their moments
    stay bit-identical; a second run is bit-identical to the first."""
    segs = make_segs(R.segment_tables(n)[table])
    tab = table_of(segs)
    hp = make_hp(lr=1e-2, max_norm=1.5 * math.sqrt(n), sched="warmup_cosine", warmup=0, total=10)
    gen = torch.Generator().manual_seed(n)
    p0 = torch.rand(n, generator=gen) * 3 - 1.5
    grads = [torch.randn(n, generator=gen) * s for s in GRAD_SCALES]
    run = run_steps(p0, grads, hp, segs)
    again = run_steps(p0, grads, hp, segs)
    for k, (a, b) in enumerate(zip(run, again)):
        assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4], f"step {k}: runs differ"
    lm, wd, skip = per_element(tab, n)
    b1, b2, eps = hp.beta1, hp.beta2, hp.eps
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for k, (g, (pk, mk, vk, sc, stepk)) in enumerate(zip(grads, run)):
        g = g.double()
        assert stepk == k + 1
        norm = float(torch.linalg.vector_norm(g))
        want = R.scalars(lr=hp.lr, beta1=b1, beta2=b2, max_norm=hp.max_grad_norm, sched="warmup_cosine", warmup=0,
                         total=10, gamma=1.0, stride=1, done=k, norm=norm)
        sc = sc.double()
        for i, rt in enumerate([U + 1e-12] * 3 + [norm_rtol(n) + U, norm_rtol(n)]):
            assert abs(float(sc[i]) - want[i]) <= rt * abs(want[i]), (k, i, float(sc[i]), want[i])
        lr, s, inv, coef = (float(x) for x in sc[:4])
        p1, m1, v1 = p.clone(), m.clone(), v.clone()
        R.adamw_flat(p1, g, m1, v1, tab, lr=lr, step_size=s, inv_bc2s=inv, coef=coef, beta1=b1, beta2=b2, eps=eps)
        tp, tm, tv = step_tol(p, m, g * coef, p1, m1, v1, s * lm.clamp(min=0), inv, b1, eps)
        assert_within(f"step {k} p", pk, p1, tp)
        assert_within(f"step {k} exp_avg", mk, m1, tm)
        assert_within(f"step {k} exp_avg_sq", vk, v1, tv)
        assert torch.equal(pk[skip].double(), p[skip]) and torch.equal(mk[skip].double(), m[skip]) \
            and torch.equal(vk[skip].double(), v[skip]), f"step {k}: a skipped element changed"
        if k == 0:
            margin = neighbour_margin(p, g, tab, sc, hp, p1, tp)
            assert margin >= 10.0, f"an element updated with its neighbour segment's values is only {margin:.1f} tol off"
        p, m, v = pk.double(), mk.double(), vk.double()


def neighbour_margin(p, g, tab, sc, hp, p1, tp):
    """Discrimination of the segment lookup: for the two elements on either side of every boundary between non-empty
    segments, |p' with the neighbour segment's (lr_mul, weight_decay) - p'| / tol_p.  Taken on the first step, where the
    zero moments make every live update ~ lr * lr_mul * sign(g): neighbouring lr_mul differ by 2x or more (one side a
    skip: the element stays put), so the ratio is 1e3 or more, far above the 10 the test asks for.  Returns the minimum."""
    sl = R.segment_slices(tab, p.numel())
    lr, s, inv, coef = (float(x) for x in sc[:4])
    worst = float("inf")
    for (s0, lm0, wd0), (s1, lm1, wd1) in zip(sl, sl[1:]):
        for i, lm, wd in ((s0.stop - 1, lm1, wd1), (s1.start, lm0, wd0)):
            q, z, w = p[i:i + 1].clone(), torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
            R.adamw_flat(q, g[i:i + 1], z, w, [(1, lm, wd)], lr=lr, step_size=s, inv_bc2s=inv, coef=coef,
                         beta1=hp.beta1, beta2=hp.beta2, eps=hp.eps)
            worst = min(worst, float((q[0] - p1[i]).abs() / tp[i]))
    return worst


def test_adamw_all_zero_gradient_from_zero_moments():
    """g = 0 on the first step: norm 0, clip coefficient exactly 1 (max_norm / 1e-6 clamped), m' = v' = 0 and
    d = eps, so every live element is only decayed -- no 0/0, nothing non-finite."""
    n = 4097
    segs = make_segs(R.segment_tables(n)["sixteen"])
    tab = table_of(segs)
    hp = make_hp(lr=1e-2, max_norm=1.0)
    p0 = torch.rand(n, generator=torch.Generator().manual_seed(2)) - 0.5
    pk, mk, vk, sc, step = run_steps(p0, [torch.zeros(n)], hp, segs)[0]
    assert step == 1 and float(sc[3]) == 1.0 and float(sc[4]) == 0.0
    assert torch.isfinite(pk).all() and float(mk.abs().max()) == 0.0 and float(vk.abs().max()) == 0.0
    p1, z = p0.double(), torch.zeros(n, dtype=torch.float64)
    R.adamw_flat(p1, z.clone(), z.clone(), z.clone(), tab, lr=float(sc[0]), step_size=float(sc[1]),
                 inv_bc2s=float(sc[2]), coef=1.0, beta1=hp.beta1, beta2=hp.beta2, eps=hp.eps)
    assert_within("p", pk, p1, 8 * U * p0.double().abs() + 2 * U * p1.abs())
    _lm, wd, skip = per_element(tab, n)
    decayed = (wd > 0) & ~skip & (p0 != 0)
    assert bool(decayed.any()) and bool((pk != p0)[decayed].all())


# -- pq3d_sumsq_partials -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0] + SIZES)
def test_sumsq_norm_matches_float64(n):
    """The norm of the two-pass sum (1024 fp32 partials, summed in double by pq3d_train_scalars) against float64
    vector_norm, for every size.  The n % 4 tail elements are made 8x larger than the rest, so losing one moves the
    norm far beyond the tolerance at every size (at n = 3 000 001 by ~2e-5 relative against ~6e-7)."""
    gen = torch.Generator().manual_seed(100 + n)
    g = torch.randn(n, generator=gen)
    g[n - n % 4:] *= 8.0
    buf = torch.zeros(max(n, 4), device=DEV)      # n = 0 still passes a valid (aligned) pointer
    buf[:n].copy_(g)
    partials = torch.full((L.SUMSQ_PARTIALS,), float("nan"), device=DEV)
    sumsq(buf, n, partials)
    sc = torch.full((8,), float("nan"), device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    train_scalars(make_hp(sched="constant"), step, partials, sc)
    torch.cuda.synchronize()
    parts = partials.cpu().double()
    assert torch.isfinite(parts).all() and float(parts.min()) >= 0.0        # every block wrote its partial
    want = float(torch.linalg.vector_norm(g.double()))
    got = float(sc[4])
    if n == 0:
        assert got == 0.0 and float(parts.abs().max()) == 0.0
        return
    rt = norm_rtol(n)
    assert abs(got - want) <= rt * want, (got, want, rt)
    assert abs(math.sqrt(float(parts.sum())) - want) <= rt * want


# -- pq3d_train_scalars --------------------------------------------------------------------------------------------------
NORMS = [0.0, 0.5, 2.0, 7.25]     # an all-zero gradient; below max_norm = 2; at it (coef just below 1); above it


@pytest.mark.parametrize("sched,gamma", SCHEDULES)
@pytest.mark.parametrize("warmup,total,stride", WINDOWS)
@pytest.mark.parametrize("max_norm", [0.0, 2.0])
def test_train_scalars_match_float64(sched, gamma, warmup, total, stride, max_norm):
    """lr, lr / bc1, 1 / sqrt(bc2), clip coefficient and norm after every step until past total_steps, and the step
    counter.  The partials are given, so the only error is the final cast to fp32 of values computed in double:
    1 u relative (plus 1e-12 for double transcendental functions)."""
    hp = make_hp(lr=3e-4, max_norm=max_norm, sched=sched, warmup=warmup, total=total, gamma=gamma, stride=stride)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    partials = torch.empty(L.SUMSQ_PARTIALS, device=DEV)
    sc = torch.full((8,), float("nan"), device=DEV)
    gen = torch.Generator().manual_seed(5)
    for done in range(total // stride + 3):
        nrm = NORMS[done % len(NORMS)]
        parts = torch.rand(L.SUMSQ_PARTIALS, generator=gen, dtype=torch.float64)
        parts = (parts * (nrm * nrm / float(parts.sum()))).float()
        partials.copy_(parts)
        train_scalars(hp, step, partials, sc)
        torch.cuda.synchronize()
        assert int(step.item()) == done + 1
        norm = math.sqrt(float(parts.double().sum()))
        want = R.scalars(lr=hp.lr, beta1=hp.beta1, beta2=hp.beta2, max_norm=max_norm, sched=sched, warmup=warmup,
                         total=total, gamma=hp.sched_gamma, stride=stride, done=done, norm=norm)
        got = [float(x) for x in sc[:5].cpu()]
        for i in range(5):
            assert abs(got[i] - want[i]) <= (U + 1e-12) * abs(want[i]), (done, i, got[i], want[i])
        st = done * stride
        if sched != "constant" and warmup > 0 and st == warmup:
            assert got[0] == hp.lr                                  # end of warm-up: factor exactly 1
        if sched == "warmup_cosine" and st == total:
            assert got[0] == float(torch.tensor(hp.lr * 1e-5, dtype=torch.float32))   # the 1e-5 floor
        if max_norm == 0.0 or nrm < max_norm:
            assert got[3] == 1.0
        if nrm == 0.0:
            assert got[4] == 0.0


# -- argument checks -----------------------------------------------------------------------------------------------------
def test_argument_checks_raise():
    n = 4096
    bufs = [torch.zeros(n + 8, device=DEV) for _ in range(4)]
    p, g, m, v = (b[:n] for b in bufs)
    partials = torch.zeros(L.SUMSQ_PARTIALS, device=DEV)
    sc = torch.zeros(8, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    hp, segs = make_hp(), make_segs([(n, 1.0, 0.0)])
    with pytest.raises(L.Pq3dError, match="16-byte"):
        sumsq(bufs[1][1:n + 1], n, partials)                  # a view at offset 1: 4-byte aligned only
    for k in range(4):
        args = [p, g, m, v]
        args[k] = bufs[k][1:n + 1]
        with pytest.raises(L.Pq3dError, match="16-byte"):
            adamw(*args, n, hp, segs, sc)
    for table in ([(n - 1, 1.0, 0.0)], [(5, 1.0, 0.0), (n - 3, 2.0, 0.0)]):
        with pytest.raises(L.Pq3dError, match="cover"):
            adamw(p, g, m, v, n, hp, make_segs(table), sc)
    for k in (0, L.MAX_OPT_SEGMENTS + 1):
        bad = make_segs([(n, 1.0, 0.0)] * min(k, L.MAX_OPT_SEGMENTS))
        bad.n = k
        with pytest.raises(L.Pq3dError, match="cover"):
            adamw(p, g, m, v, n, hp, bad, sc)
    for sched in (-1, 3):
        bad = make_hp()
        bad.sched = sched
        with pytest.raises(L.Pq3dError, match="schedule"):
            train_scalars(bad, step, partials, sc)
    for sched in ("warmup_cosine", "warmup_exp"):
        for warmup, total in ((10, 10), (10, 4)):
            with pytest.raises(L.Pq3dError, match="total_steps"):
                train_scalars(make_hp(sched=sched, warmup=warmup, total=total), step, partials, sc)
    torch.cuda.synchronize()
    assert int(step.item()) == 0                                  # nothing was launched
    train_scalars(make_hp(sched="constant", warmup=10, total=4), step, partials, sc)   # constant ignores the window
    torch.cuda.synchronize()
    assert int(step.item()) == 1 and float(sc[0]) == float(torch.tensor(1e-2, dtype=torch.float32))
    assert all(float(b.abs().max()) == 0.0 for b in bufs)


# -- TrainStep end to end ------------------------------------------------------------------------------------------------
def ticks(shape, gen, scale=1.0):
    """Random multiples of 2^-10 in [-2, 2] (11 significant bits) times a power of two: products of two such values
    and sums of two such products are exact in fp32, so fp32 and float64 gradients of the model below are identical."""
    return torch.randint(-2048, 2049, shape, generator=gen).double() / 1024 * scale


class Awkward(torch.nn.Module):
    """Parameters of awkward sizes -- numel 1, 3, 5, 48, 201, a 7 x 13 weight and its bias -- plus ``late``, which only
    takes part when the batch says so.  The loss is linear in the parameters, so gradients are exact in fp32."""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(0)
        for name, shape in (("a", (1,)), ("b", (3,)), ("c", (5,)), ("w", (4, 12)), ("v", (201,)), ("late", (7,))):
            setattr(self, name, torch.nn.Parameter(torch.rand(shape, generator=gen) * 2 - 1))
        self.lin = torch.nn.Linear(13, 7)

    def forward(self, d):
        y = self.lin(d["x"])
        terms = [(getattr(self, k) * d["c_" + k]).sum() for k in ("a", "b", "c", "w", "v")]
        if d["late"]:
            terms.append((self.late * d["c_late"]).sum())
        return {"y": y, "terms": terms, "dy": d["dy"]}


def awkward_loss(out):
    return sum(out["terms"]) + (out["y"] * out["dy"]).sum()


def awkward_batch(model, seed, scale, late):
    gen = torch.Generator().manual_seed(seed)
    d = {"c_" + k: ticks(getattr(model, k).shape, gen, scale) for k in ("a", "b", "c", "w", "v", "late")}
    d["x"], d["dy"] = ticks((1, 13), gen), ticks((1, 7), gen, scale)
    d["late"] = late
    return d


def awkward_groups(model):
    # group boundaries at flat offsets 95 and 114 (= 3 and 2 mod 4); late's skip run 102..109 (= 2 and 1 mod 4)
    return [{"params": [model.a, model.b, model.lin.weight], "lr": 1e-2, "weight_decay": 0.05},
            {"params": [model.lin.bias, model.late, model.c], "lr": 3e-2, "weight_decay": 0.0},
            {"params": [model.w, model.v], "lr": 5e-3, "weight_decay": 0.1}]


def to(d, dev, dtype):
    return {k: (x.to(dev, dtype) if torch.is_tensor(x) else x) for k, x in d.items()}


# (gradient scale, late has a gradient, micro-batches): |g| ~ 22 x scale against max_norm 8 -- steps 0, 2, 4 clip.
# Step 0 runs at lr 0 (warm-up); late is skipped in steps 0, 1 and 3; step 4 is step([mb1, mb2]) with late only in mb2.
PLAN = [(1.0, False, 1), (0.125, False, 1), (1.0, True, 1), (0.125, False, 1), (2.0, True, 2), (0.25, True, 1)]


def test_train_step_matches_torch_adamw_on_awkward_layout():
    """TrainStep.step against torch.optim.AdamW + clip_grad_norm_ + LambdaLR (float64, the same groups) on every element
    of every parameter and moment.  Before each step the float64 copies take the device's fp32 parameters and moments
    (exact in float64), so each step is compared with the one-step tolerance of the module docstring; the step count,
    the schedule and the clip are the reference's own.  The hyperparameters are those TrainStep holds in fp32 (0.98 in
    fp32 alone moves 1 - beta2 by 1e-6 relative).

    ``late`` has no gradient in some steps: it and its moments stay bit-identical there.  When it gets one again, the
    device uses the GLOBAL step count in the bias corrections -- the divergence documented in TrainStep.__init__
    (pq3d_amd/trainer.py) -- while torch.optim.AdamW would use the parameter's own count: the test pins the global
    count and checks that torch's own would be far outside the tolerance."""
    model = Awkward().to(DEV)
    ref = Awkward().double()
    ref.load_state_dict({k: x.double() for k, x in model.state_dict().items()})
    ts = TrainStep(model, awkward_loss, opt_groups=awkward_groups(model), lr=1e-2, grad_norm=8.0,
                   sched="warmup_cosine", warmup_steps=2, total_steps=8)
    hp = ts.hp
    names = dict((id(q), k) for k, q in model.named_parameters())
    offs, off = {}, 0
    for name, k in ts.layout():
        offs[name] = (off, k)
        off += k
    assert [offs[k][0] for k in ("lin.weight", "lin.bias", "late", "c", "w")] == [4, 95, 102, 109, 114]
    rp = dict(ref.named_parameters())
    groups = [{"params": [rp[names[id(q)]] for q in g["params"]], "lr": hp.lr * ts.segs.lr_mul[s],
               "weight_decay": ts.segs.weight_decay[s]} for s, g in enumerate(ts.groups)]
    opt = torch.optim.AdamW(groups, lr=hp.lr, betas=(hp.beta1, hp.beta2), eps=hp.eps, foreach=False)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: T.lr_factor("warmup_cosine", s, 2, 8))
    dc = (norm_rtol(off) + U) + 4 * U                  # clip coefficient, the three scalars, lr * lr_mul in fp32
    late_steps = 0
    for k, (scale, late, nmb) in enumerate(PLAN):
        mbs = [awkward_batch(model, 10 * k + j, scale, late and j == nmb - 1) for j in range(nmb)]
        before = {n: (ts.flat_p[o:o + c].double().cpu(), ts.exp_avg[o:o + c].double().cpu(),
                      ts.exp_avg_sq[o:o + c].double().cpu()) for n, (o, c) in offs.items()}
        ts.step([to(mb, DEV, torch.float32) for mb in mbs] if nmb > 1 else to(mbs[0], DEV, torch.float32))
        torch.cuda.synchronize()
        # float64 reference step from the device's state before the step, global step count k
        for n, q in rp.items():
            q.data.copy_(before[n][0].view_as(q))
            opt.state[q] = {"step": torch.tensor(float(k)), "exp_avg": before[n][1].view_as(q).clone(),
                            "exp_avg_sq": before[n][2].view_as(q).clone()}
        opt.zero_grad(set_to_none=True)
        for mb in mbs:
            (awkward_loss(ref(to(mb, "cpu", torch.float64))) * (1.0 / nmb)).backward()
        live = [q for q in rp.values() if q.grad is not None]
        norm = float(torch.nn.utils.clip_grad_norm_(live, 8.0))
        lrs = {id(q): gr["lr"] for gr in opt.param_groups for q in gr["params"]}
        gr_of = {n: q.grad.detach().reshape(-1).clone() for n, q in rp.items() if q.grad is not None}
        if late:
            lq = rp["late"]
            wd = next(gr["weight_decay"] for gr in opt.param_groups if any(x is lq for x in gr["params"]))
            own = torch.optim.AdamW([lq], lr=lrs[id(lq)], weight_decay=wd, betas=(hp.beta1, hp.beta2), eps=hp.eps,
                                    foreach=False)      # late's own step count
            own.state[lq] = {"step": torch.tensor(float(late_steps)), "exp_avg": before["late"][1].view_as(lq).clone(),
                             "exp_avg_sq": before["late"][2].view_as(lq).clone()}
            p_save = lq.detach().clone()
            own.step()
            late_own = lq.detach().reshape(-1).clone()
            lq.data.copy_(p_save)
        opt.step()
        lam.step()
        assert abs(float(ts.last_grad_norm) - norm) <= norm_rtol(off) * norm
        want_lr = hp.lr * T.lr_factor("warmup_cosine", k, 2, 8)
        assert abs(float(ts.last_lr) - want_lr) <= (U + 1e-12) * want_lr
        t = k + 1
        bc1, inv = 1 - hp.beta1 ** t, 1 / math.sqrt(1 - hp.beta2 ** t)
        for n, (o, c) in offs.items():
            pk, mk, vk = ts.flat_p[o:o + c].cpu(), ts.exp_avg[o:o + c].cpu(), ts.exp_avg_sq[o:o + c].cpu()
            p0, m0, v0 = before[n]
            if n not in gr_of:
                assert n == "late" and not late
                assert torch.equal(pk.double(), p0) and torch.equal(mk.double(), m0) and torch.equal(vk.double(), v0), \
                    f"step {k}: {n} changed without a gradient"
                continue
            q = rp[n]
            p1, st = q.detach().reshape(-1), opt.state[q]
            m1, v1 = st["exp_avg"].reshape(-1), st["exp_avg_sq"].reshape(-1)
            tp, tm, tv = step_tol(p0, m0, gr_of[n], p1, m1, v1, lrs[id(q)] / bc1, inv, hp.beta1, hp.eps, dc)
            assert_within(f"step {k} {n}", pk, p1, tp)
            assert_within(f"step {k} {n} exp_avg", mk, m1, tm)
            assert_within(f"step {k} {n} exp_avg_sq", vk, v1, tv)
            if n == "late" and late_steps < k:
                # the documented divergence: torch's own count gives other bias corrections, far outside the tolerance
                assert float(((late_own - p1).abs() / tp).min()) > 10.0
        late_steps += bool(late)
    assert int(ts.step_count.item()) == len(PLAN)
