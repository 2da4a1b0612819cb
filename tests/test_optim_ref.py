"""CPU: the flat per-segment restatement of the optimizer step (tests/optim_ref.py, the checker of csrc/optim.hip)
against torch.optim.AdamW + clip_grad_norm_ + LambdaLR in float64, one torch parameter per segment, for the schedule,
clip and segment-table cases the GPU tests (tests/test_gpu_optim.py) run."""
import pytest
import torch

from oracle import train_oracle as T
from tests import optim_ref as R

BETAS, EPS = (0.9, 0.98), 1e-8


def torch_run(p0, grads, segs, *, lr, max_norm, sched, warmup, total, gamma=1.0, stride=1):
    """torch's optimizer objects driven the way train_oracle.adamw_step restates them: clip_grad_norm_ over the
    parameters with a gradient, AdamW.step(), then ``stride`` LambdaLR steps (the accelerate-prepared scheduler).
    Skip segments get grad None, as TrainStep's skipped parameters do.  Returns the flat parameters after every step."""
    sl = R.segment_slices(segs, p0.numel())
    params = [torch.nn.Parameter(p0[s].double().clone()) for s, _, _ in sl]
    live = [(q, lm, wd) for q, (_, lm, wd) in zip(params, sl) if lm >= 0]
    opt = torch.optim.AdamW([{"params": [q], "lr": lr * lm, "weight_decay": wd} for q, lm, wd in live], lr=lr,
                            betas=BETAS, eps=EPS, foreach=False)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda s: T.lr_factor(sched, s, warmup, total, gamma))
    out = []
    for g in grads:
        for q, (s, lm, _) in zip(params, sl):
            q.grad = g[s].double().clone() if lm >= 0 else None
        if max_norm:
            torch.nn.utils.clip_grad_norm_([q for q, _, _ in live], max_norm)
        opt.step()
        for _ in range(stride):
            lam.step()
        out.append(torch.cat([q.detach() for q in params]))
    return out


def flat_run(p0, grads, segs, **kw):
    ref = R.FlatAdamW(p0, lr=kw["lr"], betas=BETAS, eps=EPS, max_norm=kw["max_norm"], sched=kw["sched"],
                      warmup=kw["warmup"], total=kw["total"], gamma=kw.get("gamma", 1.0), stride=kw.get("stride", 1))
    out = []
    for g in grads:
        ref.step(g, segs)
        out.append(ref.p.clone())
    return out


def gradients(n, segs, scales, seed):
    """Fresh random gradients per step (scale 0: an all-zero gradient); zero on skip segments, as TrainStep packs them."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for sc in scales:
        g = torch.randn(n, generator=gen, dtype=torch.float64) * sc
        for s, lm, _ in R.segment_slices(segs, n):
            if lm < 0:
                g[s] = 0.0
        out.append(g)
    return out


def assert_same(got, want):
    for k, (a, b) in enumerate(zip(got, want)):
        err = float((a - b).abs().max())
        assert err <= 1e-12 * max(1.0, float(b.abs().max())), (k, err)     # float64 both: operation order only


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097])
@pytest.mark.parametrize("table", ["one", "sixteen", "skip"])
def test_flat_restatement_matches_torch_on_segment_tables(n, table):
    segs = R.segment_tables(n)[table]
    p0 = torch.rand(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64) * 3 - 1.5
    grads = gradients(n, segs, [1.0, 0.1, 3.0, 0.0, 2.0], seed=7 * n)
    kw = dict(lr=1e-2, max_norm=1.5 * n ** 0.5, sched="warmup_cosine", warmup=0, total=10)
    got, want = flat_run(p0, grads, segs, **kw), torch_run(p0, grads, segs, **kw)
    assert_same(got, want)
    for s, lm, _ in R.segment_slices(segs, n):
        if lm < 0:
            assert torch.equal(got[-1][s], p0[s])


SCHEDULES = [("constant", 1.0), ("warmup_cosine", 1.0), ("warmup_exp", 0.1)]
# (warmup already scaled by the process count, total, stride): no warm-up; a warm-up whose end (st == wu) is a step;
# stride 4 with st == wu at done = 3.  Every run goes past total, where the cosine reaches its 1e-5 floor at st == total.
WINDOWS = [(0, 10, 1), (3, 10, 1), (12, 40, 4)]


@pytest.mark.parametrize("sched,gamma", SCHEDULES)
@pytest.mark.parametrize("warmup,total,stride", WINDOWS)
@pytest.mark.parametrize("max_norm", [0.0, 3.0, 1e3])
def test_flat_restatement_matches_torch_schedule_and_clip(sched, gamma, warmup, total, stride, max_norm):
    n = 1023
    segs = R.segment_tables(n)["sixteen"]
    steps = total // stride + 3
    p0 = torch.rand(n, generator=torch.Generator().manual_seed(1), dtype=torch.float64) - 0.5
    scales = [0.0 if k == 2 else (0.05, 0.2, 1.0)[k % 3] for k in range(steps)]     # |g| ~ 1.6, 6.4, 32 and one zero
    grads = gradients(n, segs, scales, seed=11)
    kw = dict(lr=1e-3, max_norm=max_norm, sched=sched, warmup=warmup, total=total, gamma=gamma, stride=stride)
    assert_same(flat_run(p0, grads, segs, **kw), torch_run(p0, grads, segs, **kw))


def test_scalars_follow_the_lambdalr_factor_and_clip_formula():
    """The scalar restatement against the formulas it stands for: lambda(done * stride); the floor 1e-5 at st == total;
    warm-up end factor 1; clip coefficient 1 for no clipping, a norm below max_norm and a zero gradient."""
    kw = dict(lr=2e-3, beta1=0.9, beta2=0.98, gamma=1.0)
    lr, step_size, inv, coef, _ = R.scalars(max_norm=0.0, sched="warmup_cosine", warmup=0, total=10, stride=1, done=10,
                                            norm=5.0, **kw)
    assert lr == 2e-3 * 1e-5 and coef == 1.0
    assert abs(step_size - lr / (1 - 0.9 ** 11)) <= 1e-18 and abs(inv - (1 - 0.98 ** 11) ** -0.5) <= 1e-15
    assert R.scalars(max_norm=3.0, sched="warmup_cosine", warmup=12, total=40, stride=4, done=3, norm=0.0, **kw)[0] == 2e-3
    assert R.scalars(max_norm=3.0, sched="constant", warmup=0, total=0, stride=1, done=0, norm=0.0, **kw)[3] == 1.0
    assert R.scalars(max_norm=3.0, sched="constant", warmup=0, total=0, stride=1, done=0, norm=2.0, **kw)[3] == 1.0
    assert R.scalars(max_norm=3.0, sched="constant", warmup=0, total=0, stride=1, done=0, norm=6.0, **kw)[3] == \
        3.0 / (6.0 + 1e-6)
    g = torch.randn(50, dtype=torch.float64) * 4
    q = torch.nn.Parameter(torch.zeros(50, dtype=torch.float64))
    q.grad = g.clone()
    norm = float(torch.nn.utils.clip_grad_norm_([q], 3.0))
    assert abs(float(q.grad[0] / g[0]) - R.clip_coef(norm, 3.0)) <= 1e-15


def test_global_step_count_for_a_parameter_skipped_earlier():
    """TrainStep's documented divergence (pq3d_amd/trainer.py, TrainStep.__init__): the bias corrections use the ONE
    global step count, torch.optim.AdamW a per-parameter count that only advances when the parameter has a gradient.
    A segment skipped in step 1 and live in step 2 gets 1 - beta^2 in the restatement: torch's result once its step
    count is set to the global one, and visibly not torch's own result (1 - beta^1)."""
    n = 12
    live, skip = [(5, 1.0, 0.01), (n, 3.0, 0.05)], [(5, 1.0, 0.01), (n, -1.0, 0.0)]
    p0 = torch.rand(n, generator=torch.Generator().manual_seed(3), dtype=torch.float64) - 0.5
    g1, g2 = gradients(n, skip, [1.0], 5)[0], gradients(n, live, [1.0], 6)[0]
    ref = R.FlatAdamW(p0, lr=1e-2, betas=BETAS, eps=EPS, sched="constant")
    ref.step(g1, skip)
    ref.step(g2, live)

    def torch_late(step_count):
        q = torch.nn.Parameter(p0[5:].clone())
        opt = torch.optim.AdamW([q], lr=3e-2, betas=BETAS, eps=EPS, weight_decay=0.05, foreach=False)
        if step_count is not None:
            opt.state[q] = {"step": torch.tensor(float(step_count)), "exp_avg": torch.zeros_like(q),
                            "exp_avg_sq": torch.zeros_like(q)}
        q.grad = g2[5:].clone()
        opt.step()
        return q.detach()

    assert float((ref.p[5:] - torch_late(1)).abs().max()) <= 1e-15
    # own count: the first step's bias corrections (bc1 = 0.1 instead of 0.19) -- a different update by ~2x
    assert float((ref.p[5:] - torch_late(None)).abs().min()) > 1e-3
