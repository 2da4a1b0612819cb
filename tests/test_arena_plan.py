"""CPU: the gradient-arena protocol (pq3d_amd/arena.py) -- slots, the fresh / accumulate decision, take / verify, the deferred
queue's life cycle -- driven with CPU parameters, a FlatGradAllReducer on CPU and toy autograd functions.  Pure decisions on CPU
tensors: nothing here launches (the zero-fill of host tensors is .zero_())."""
import pytest
import torch

from pq3d_amd import arena
from pq3d_amd._lib import BF16
from pq3d_amd.parallel import FlatGradAllReducer


class _Use(torch.autograd.Function):
    """sum(w * x) as an arena-aware use of w: the backward takes w's slot, adds into it and returns the view or None."""

    @staticmethod
    def forward(ctx, w, x):
        ctx.x, ctx.pptr = x, w.data_ptr()
        return (w * x).sum()

    @staticmethod
    def backward(ctx, g):
        slot, give = arena.take([ctx.pptr], [ctx.x.numel()])
        if slot is None:
            return g * ctx.x, None
        slot[0].add_(g * ctx.x)
        return (slot[0] if give else None), None


class _Decoder(torch.autograd.Function):
    """Identity whose backward opens the decoder's part of the arena (inside a backward pass: queue_callback is legal there)."""

    @staticmethod
    def forward(ctx, x, box, *call):
        ctx.box, ctx.call = box, call
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.box["out"] = arena.open_decoder(*ctx.call)
        ctx.box["active_inside"] = arena.active()
        return (g,) + (None,) * (1 + len(ctx.call))


@pytest.fixture(autouse=True)
def _no_arena_left_behind():
    yield
    assert not arena.active() and not arena.zero_pending() and arena._DW_QUEUE.nbytes == 0


def _tied(fill=0.0):
    """A weight used twice and a bystander, their reducer with the flat buffers pre-filled, and the plain-autograd gradient."""
    torch.manual_seed(0)
    w, v = torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))
    x1, x2 = (torch.randint(-8, 9, (3, 5)).float() for _ in range(2))   # small integers: every sum below is exact
    red = FlatGradAllReducer([w, v])
    for f in red.flat:
        f.fill_(fill)
    loss = lambda: _Use.apply(w, x1) + _Use.apply(w, x2)
    return w, v, red, loss, x1 + x2


def test_slots_keep_their_mapping_and_know_their_views():
    w, v, red, _loss, _ref = _tied()
    slots = red.slots()
    assert isinstance(slots, arena.GradSlots) and set(slots.params) == {id(w), id(v)} and slots.params[id(w)] is w
    off = 0
    for p in red.buckets[0]:
        flat, o, n = slots[id(p)]
        assert flat is red.flat[0] and (o, n) == (off, p.numel())
        assert slots.view(p).shape == p.shape and slots.view(p).data_ptr() == flat[o:].data_ptr()
        assert slots.view(p) is not slots.view(p)   # a new object per call
        off += n
    assert not slots.aliased(w) and not slots.holds(w, None) and not slots.holds(w, w.detach().clone())
    w.grad = slots.view(w)
    assert slots.aliased(w) and not slots.aliased(v) and slots.holds(w, red.flat[0][slots[id(w)][1]:])
    w.requires_grad_(False)
    assert list(slots.by_ptr(red.flat).values()) == [v] and slots.by_ptr(red.flat, skip={id(v)}) == {} and slots.by_ptr([]) == {}


def test_tied_weight_lands_in_its_slot_accumulates_and_refuses_a_foreign_gradient():
    w, v, red, loss, ref = _tied()
    slots = red.slots()
    with arena.grad_arena(slots, red.flat):
        loss().backward()
    assert slots.aliased(w) and torch.equal(w.grad, ref) and v.grad is None
    with arena.grad_arena(slots, red.flat):   # second micro-batch: .grad still aliases the slot -> in place
        loss().backward()
    assert slots.aliased(w) and torch.equal(slots.view(w), 2 * ref)
    w.grad = None
    with pytest.raises(RuntimeError, match="gradient arena"):
        with arena.grad_arena(slots, red.flat):
            (loss() + (w * w).sum()).backward()   # a gradient from outside the arena after an in-place second use


def _decision_case(alias):
    torch.manual_seed(1)
    d0, d1, e0 = (torch.nn.Parameter(torch.randn(4)) for _ in range(3))
    red = FlatGradAllReducer([d0, d1, e0], groups=[[d0, d1], [e0]])
    slots = red.slots()
    for p in {"none": (), "all": (d0, d1, e0), "some": (d0,), "offered": (e0,)}[alias]:
        p.grad = slots.view(p)
    for f in red.flat:
        f.fill_(7.0)
    return [d0, d1], e0, red, slots


MIXED = "alias the shared gradient arena"


@pytest.mark.parametrize("alias,whole,decoder,decoder_in_whole", [
    # .grad aliasing its slot: on no parameter / on all / on one of the decoder's / only on the one outside the decoder
    ("none", "fresh", "fresh", "fresh"),
    ("all", "accumulate", "accumulate", "accumulate"),
    ("some", "accumulate", MIXED, MIXED),
    ("offered", "accumulate", MIXED, MIXED),
])
def test_fresh_or_accumulate_decision_table(alias, whole, decoder, decoder_in_whole):
    # the whole-pass arena: any alias accumulates, never an error; a fresh one still has its zero-fill pending
    _dec, _e0, red, slots = _decision_case(alias)
    with arena.grad_arena(slots, red.flat):
        assert arena.active() and arena.zero_pending() == (whole == "fresh")
    assert all(bool((f == (0.0 if whole == "fresh" else 7.0)).all()) for f in red.flat)

    def run_decoder(dec, red, slots):
        box, x, extra = {}, torch.zeros(2, requires_grad=True), torch.full((3,), 7.0)
        _Decoder.apply(x, box, slots, list(red.flat), dec, extra).sum().backward()
        gv, accumulate, in_place = box["out"]
        assert in_place and all(slots.holds(p, gv[id(p)]) for p in dec) and bool((extra == 0).all())
        return "accumulate" if accumulate else "fresh", box

    # the decoder's own parameters, no whole-pass arena open: all or nothing, the slots it offers included
    dec, e0, red, slots = _decision_case(alias)
    if decoder == MIXED:
        with pytest.raises(RuntimeError, match=MIXED):
            run_decoder(dec, red, slots)
        assert all(bool((f == 7.0).all()) for f in red.flat)   # refused before anything was zeroed
    else:
        mode, box = run_decoder(dec, red, slots)
        assert mode == decoder and box["active_inside"]   # e0's slot is on offer until the pass ends
        assert all(bool((f == (0.0 if mode == "fresh" else 7.0)).all()) for f in red.flat)
    assert not arena.active()

    # the same under an open whole-pass arena that holds them all: the arena's mode, checked against the decoder's parameters
    dec, e0, red, slots = _decision_case(alias)
    if decoder_in_whole == MIXED:
        with pytest.raises(RuntimeError, match=MIXED):
            with arena.grad_arena(slots, red.flat):
                run_decoder(dec, red, slots)
    else:
        with arena.grad_arena(slots, red.flat):
            mode, _box = run_decoder(dec, red, slots)
            assert mode == decoder_in_whole and not arena.zero_pending()   # the decoder was the first consumer
        assert all(bool((f == (0.0 if mode == "fresh" else 7.0)).all()) for f in red.flat)


def test_decoder_without_an_owner_gets_one_zeroed_buffer_of_its_own():
    dec, _e0, _red, _slots = _decision_case("none")
    box, x = {}, torch.zeros(2, requires_grad=True)
    _Decoder.apply(x, box, None, (), dec, None).sum().backward()
    gv, accumulate, in_place = box["out"]
    assert not accumulate and not in_place and not box["active_inside"]
    assert [gv[id(p)].shape for p in dec] == [p.shape for p in dec] and all(bool((gv[id(p)] == 0).all()) for p in dec)
    assert gv[id(dec[1])].data_ptr() == gv[id(dec[0])].data_ptr() + 4 * dec[0].numel()


def test_take_refuses_without_touching_the_state():
    w, v, red, _loss, _ref = _tied(fill=7.0)
    stranger = torch.randn(3, 5)
    with arena.grad_arena(red.slots(), red.flat):
        assert arena.take([w.data_ptr()], [w.numel() - 1]) == (None, False)   # only STARTS where the parameter starts
        assert arena.take([stranger.data_ptr()]) == (None, False)
        assert arena.take([w.data_ptr(), stranger.data_ptr()], [w.numel(), stranger.numel()]) == (None, False)
        assert arena.zero_pending() and bool((red.flat[0] == 7.0).all())   # nothing was zeroed for them
        slot, give = arena.take([w.data_ptr()], [w.numel()])   # still the first use
        assert give and not arena.zero_pending() and bool((slot[0] == 0).all())
        assert arena.take([w.data_ptr(), v.data_ptr()]) == (None, False)   # a partly-seen group in a fresh pass
        again, give = arena.take([w.data_ptr()])
        assert not give and again[0] is not slot[0] and again[0].data_ptr() == slot[0].data_ptr()


def test_an_exception_inside_the_pass_drops_the_queue_and_leaves_no_arena():
    w, v, red, loss, ref = _tied()
    slots = red.slots()
    g, x, dw = torch.randn(16, 8), torch.randn(16, 8), torch.zeros(8, 8)
    assert not arena.defer(g, x, None, dw, None, 8, 8, BF16)   # no whole-pass arena: nothing is queued
    with pytest.raises(ZeroDivisionError):
        with arena.grad_arena(slots, red.flat, pack_follows=True):
            assert arena.defer(g, x, None, dw, None, 8, 8, BF16) and arena._DW_QUEUE.nbytes > 0
            1 / 0
    assert not arena.active() and not arena.zero_pending() and arena._DW_QUEUE.buckets == {}
    assert bool((dw == 0).all())   # dropped, not launched
    with arena.grad_arena(slots, red.flat):   # (a product left in the queue would be launched here)
        loss().backward()
    assert slots.aliased(w) and torch.equal(w.grad, ref)


def test_verify_returned_for_autograd_grad_callers():
    w, v, red, loss, ref = _tied()
    with arena.grad_arena(red.slots(), red.flat) as a:
        gw, = torch.autograd.grad(loss(), [w])
    a.verify_returned([w], [gw])
    assert a.slots.holds(w, gw) and torch.equal(gw, ref) and w.grad is None
    with arena.grad_arena(red.slots(), red.flat) as a:   # .grad is not written: nothing to check when the context exits
        gw, = torch.autograd.grad(loss() + (w * w).sum(), [w])
    assert not a.slots.holds(w, gw)
    with pytest.raises(RuntimeError, match="gradient arena"):
        a.verify_returned([w], [gw])
    assert not arena.active()


def test_a_fresh_pass_zeroes_the_buffers_once_consumed_or_not():
    w, v, red, loss, ref = _tied(fill=7.0)
    slots = red.slots()
    with arena.grad_arena(slots, red.flat):
        loss().backward()   # one consumer took the zeroing
    assert torch.equal(slots.view(w), ref) and bool((slots.view(v) == 0).all())
    assert arena.zeroed_buffers() == set()   # no pack follows: the note ends with the context
    w.grad = None
    red.flat[0].fill_(7.0)
    with arena.grad_arena(slots, red.flat, pack_follows=True):
        (v * v).sum().backward()   # nobody consumed it: zeroed when the context exits
    assert bool((red.flat[0] == 0).all()) and not slots.aliased(v)
    assert arena.zeroed_buffers(consume=False) == {red.flat[0].data_ptr()} and arena.zeroed_buffers() and not arena.zeroed_buffers()
