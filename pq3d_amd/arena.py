"""The gradient arena: the rules by which a backward pass writes parameter gradients straight into the owner's flat fp32
buffers -- which slot a gradient goes to (GradSlots), whether the pass is fresh or accumulating (_decide), whether a
weight-gradient product may wait until the pass ends (can_defer / defer) -- and the state of the pass in flight.  Host logic only:
the one launch in here is the zero-fill (zero)."""
from __future__ import annotations

import torch

from . import wgrad


class GradSlots(dict):
    """{id(param): (flat buffer, element offset, numel)} plus ``params`` = {id(param): param}: the slot map of an owner of flat
    gradient buffers (FlatGradAllReducer.slots()), handed to the fused executor as ``encoder.grad_arena``.  ``params`` lets a pass
    offer the slots of parameters OUTSIDE the decoder (the input encoders) to their own backward functions (by_ptr)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.params = {}

    def view(self, p) -> torch.Tensor:
        """A NEW view object of p's slot per call: AccumulateGrad adopts a gradient without a copy only while nobody else
        holds the object."""
        flat, off, n = self[id(p)]
        return flat[off:off + n].view(p.shape)

    def holds(self, p, t) -> bool:
        """Is the tensor ``t`` (None: no) p's slot itself?"""
        flat, off, _n = self[id(p)]
        return t is not None and t.data_ptr() == flat.data_ptr() + 4 * off

    def aliased(self, p) -> bool:
        """Does p.grad alias p's slot: the owner has not consumed the previous micro-batch."""
        return self.holds(p, p.grad)

    def by_ptr(self, buffers, skip=()) -> dict:
        """The table a pass looks its parameters up in, {parameter data_ptr: parameter}: every parameter that wants a gradient
        and whose slot lies in one of ``buffers`` (the ones the pass zero-fills), without the ids in ``skip``."""
        held = {b.data_ptr() for b in buffers}
        return {p.data_ptr(): p for i, p in self.params.items()
                if i not in skip and p.requires_grad and self[i][0].data_ptr() in held}


def zero(tensors) -> None:
    """Every zero-fill of the arena, of the decoder's scratch and of a pack's unused slots: ONE pq3d_zero_many launch for the
    fp32 device tensors in ``tensors`` (never .zero_() / a memset there: the captured backward graphs rely on it, ops.zero_many);
    host tensors (the gloo tests of parallel.py) are filled in place."""
    ts = [t for t in tensors if t is not None]
    if ts and ts[0].is_cuda:
        from . import ops
        ops.zero_many(ts)
    else:
        for t in ts:
            t.zero_()


# ---- gradient arena offered for one backward pass ----------------------------------------------------------------------
# The fused decoder's backward zero-fills the owner's flat gradient buffers with its one zero launch and then OFFERS the
# slots of the parameters outside the decoder (the input encoders) to the backward functions that run after it in the same
# pass: they accumulate straight into the slots (no zero-fill launch of their own, no pack copy afterwards) and hand
# autograd views of them.  The offer ends with the pass (engine callback), so a later backward that does not start with
# the decoder never sees stale zeroing.  mode "fresh": slots were just zeroed, return the views (autograd adopts them);
# "accumulate": .grad already aliases the slots (second micro-batch), add in place and return None.
# Process-global state (the autograd engine runs the backward functions on its own thread, so thread-local would not reach
# them): ONE backward pass at a time may use an arena -- two models stepping concurrently from different threads must not
# both be given one.
class _ArenaState:
    """The gradient arena of the backward pass in flight, as ONE object with three transitions -- begin() (a whole-pass
    grad_arena context or the decoder's offer), end() (the pass is over: everything per-pass is dropped) and the accessors
    below -- instead of loose class attributes that every call site had to clear by hand."""

    def __init__(self):
        self.zeroed_ptrs = set()   # flat buffers the last fresh pass zero-filled (read by the gradient pack that follows it)
        self.end()

    def begin(self, mode, slots, by_ptr, whole_pass, pending=None):
        self.mode = mode                 # None | "fresh" | "accumulate"
        self.slots = slots               # the owner's GradSlots
        self.by_ptr = by_ptr             # parameter data_ptr -> parameter, for the slots offered in this pass (GradSlots.by_ptr)
        self.written = set()             # slots some function of this pass already returned (a second use adds in place)
        self.whole_pass = whole_pass     # offered by grad_arena() around the whole backward (the decoder then neither zeroes nor offers)
        self.pending = pending           # fresh whole-pass arena: buffers still to be zeroed -- by the FIRST consumer

    def end(self, keep_zeroed: bool = True):
        self.mode, self.slots, self.by_ptr, self.written, self.whole_pass, self.pending = None, None, {}, set(), False, None
        self.multi = set()               # slots that took an in-place second use in a FRESH pass: verified when the pass ends
        if not keep_zeroed:
            self.zeroed_ptrs = set()


_Arena = _ArenaState()


def active() -> bool:
    """Is a gradient arena offered right now (a whole-pass context is open, or a decoder's offer has not ended)?"""
    return _Arena.mode is not None


def zero_pending() -> bool:
    """Does a fresh whole-pass arena still wait for its first consumer to zero the buffers?"""
    return _Arena.pending is not None


_MIXED = "fused decoder backward: some parameters' .grad alias the shared gradient arena and others do not -- " \
         "zero ALL gradients (set_to_none=True) or none between micro-batches"


def _decide(slots, params, strict: bool, offered=(), given=None) -> str:
    """"fresh" or "accumulate", read off the parameters: .grad still aliasing the slot -> the owner has not consumed the
    previous micro-batch -> add in place; .grad None / foreign -> a fresh step: zero, then hand fresh views to autograd.
    strict=False (a whole-pass arena over ALL of a model's parameters): any alias means accumulate -- functions only add into
    slots whose .grad aliases them, gradients that live in tensors of their own keep accumulating through autograd and are
    packed afterwards.  strict=True (the decoder's own parameters, all written by accumulating launches): all or nothing, the
    parameters ``offered`` to later functions included; under an open whole-pass arena the mode is ``given`` and only checked."""
    alias = [slots.aliased(p) for p in params]
    if not strict:
        return "accumulate" if any(alias) else "fresh"
    if given is not None:
        if given == "accumulate" and not all(alias):
            raise RuntimeError(_MIXED)
        return given
    if params and all(alias):
        return "accumulate"
    if any(alias) or any(slots.aliased(q) for q in offered):
        raise RuntimeError(_MIXED)
    return "fresh"


def flush_zero(extra=()) -> bool:
    """Zero the whole-pass arena's buffers if that is still pending (one launch, ``extra`` buffers of the caller included);
    False when there was nothing pending (the caller zeroes its own buffers itself)."""
    if _Arena.pending is None:
        return False
    bufs, _Arena.pending = _Arena.pending, None
    zero(list(bufs) + list(extra))
    _Arena.zeroed_ptrs = {b.data_ptr() for b in bufs}
    return True


def zeroed_buffers(consume: bool = True) -> set:
    """data_ptrs of the flat buffers the last fresh whole-pass arena zero-filled: the gradient pack right after that pass need
    not zero the slots of parameters that received no gradient.  consume: forget them (one pack per pass)."""
    z = _Arena.zeroed_ptrs
    if consume:
        _Arena.zeroed_ptrs = set()
    return z


def verify(slots, multi, by_ptr, returned=None) -> None:
    """A fresh pass hands the FIRST arena-aware use of a parameter a view of its slot and lets later arena-aware uses (a tied
    weight) add into the slot in place.  That is only correct while autograd keeps that view as the gradient: a gradient
    for the same parameter from a function that is NOT arena-aware makes autograd sum out of place, .grad becomes a tensor
    of its own and the later in-place additions are lost.  Autograd gives no guarantee here, so the hand-out is CHECKED
    when the pass ends: every slot in ``multi`` (it took an in-place second use) must still be what .grad aliases.
    ``returned``: {parameter data_ptr: gradient torch.autograd.grad() returned} for callers that do not go through
    .backward() (GraphedQuery3D): checked instead of .grad."""
    bad = []
    for q in multi:
        p_ = by_ptr.get(q)
        if p_ is None:
            continue
        if returned is None and p_.grad is None:
            continue      # torch.autograd.grad(): .grad is not written -- the caller verifies what it got back (returned=...)
        if not slots.holds(p_, returned.get(q) if returned is not None else p_.grad):
            bad.append(tuple(p_.shape))
    if bad:
        raise RuntimeError(f"gradient arena: {len(bad)} parameter(s) (shapes {bad[:4]}) received gradients both in place "
                           "through their arena slot (a tied weight's second use) and through a function that does not use "
                           "the arena; autograd summed them out of place and the in-place part is lost -- run this backward "
                           "without ops.grad_arena / enc.grad_arena, or route every use of the parameter through pq3d_amd.ops")


def _slots(slots) -> GradSlots:
    return slots if isinstance(slots, GradSlots) else GradSlots(slots)   # a plain {id(param): slot} map: nothing to offer


class grad_arena:
    """``with ops.grad_arena(slots, buffers): loss.backward()`` -- the owner of the flat gradient buffers (a
    FlatGradAllReducer / TrainStep) offers every parameter's slot for the WHOLE backward pass: one zero launch up front
    (none when every .grad still aliases its slot: accumulation over micro-batches), then every arena-aware backward function
    -- the heads that run BEFORE the decoder's backward (the caption body), the decoder, the input encoders after it --
    accumulates in place.  Without this context the decoder's backward makes the offer itself (offer), which only
    reaches the functions that run after it.

    .grad IS NOT FINAL UNTIL THE CONTEXT EXITS: weight gradients of arena-aware linear layers are queued (_DW_QUEUE) and
    launched grouped at __exit__ (earlier only at the fused decoder's readiness reports, FlatGradAllReducer.launch() /
    pack(), or when the queue exceeds _DW_QUEUE_CAP); a reader of p.grad inside the pass sees zeros or partial sums.
    Parameters with gradient hooks registered are excluded from the deferral for that reason."""

    def __init__(self, slots, buffers, pack_follows: bool = False):
        # pack_follows: the owner calls FlatGradAllReducer.pack() on these buffers right after the pass; only then is the
        # "already zero-filled" note (zeroed_buffers) kept past the end of the context
        self.slots, self.buffers, self.pack_follows = _slots(slots), list(buffers), pack_follows

    def verify_returned(self, params, grads) -> None:
        """For torch.autograd.grad() callers, after the context: the gradients returned for tied parameters that took an
        in-place second use must alias their slots."""
        verify(self.slots, self.multi, self.by_ptr, {p.data_ptr(): g for p, g in zip(params, grads)})

    def __enter__(self):
        _Arena.zeroed_ptrs, _Arena.multi = set(), set()
        by_ptr = self.slots.by_ptr(self.buffers)
        # a later micro-batch of an accumulating step: the in-place gradients of the previous one are still adopted as .grad.
        # No aliasing .grad anywhere: a fresh step, one zero launch
        mode = _decide(self.slots, by_ptr.values(), strict=False)
        # fresh: the buffers are zeroed by the first consumer of the pass (with its own scratch: one launch)
        _Arena.begin(mode, self.slots, by_ptr, True, pending=list(self.buffers) if mode == "fresh" else None)
        return self

    def __exit__(self, *exc):
        self.multi, self.by_ptr = _Arena.multi, _Arena.by_ptr
        try:
            dw_deferred_flush(run=exc[0] is None)   # the queued weight-gradient products of the pass: a few grouped launches
            if exc[0] is None:
                flush_zero()    # nobody consumed it: the owner still expects zeroed buffers
                verify(self.slots, self.multi, self.by_ptr)
        finally:
            _Arena.end(keep_zeroed=self.pack_follows)
        return False


def offer(slots, by_ptr, mode) -> None:
    """The decoder's offer of the slots in ``by_ptr`` to the backward functions that run after it; ends with the pass."""
    _Arena.begin(mode, slots, by_ptr, False)

    def _end():
        if not _Arena.whole_pass:
            try:
                verify(_Arena.slots, _Arena.multi, _Arena.by_ptr)
            finally:
                _Arena.end()
    torch.autograd.Variable._execution_engine.queue_callback(_end)


def take(ptrs, numels=None):
    """Slot views for the parameters at ``ptrs`` (all of them or None) and whether to return them to autograd.  ``numels``:
    the element counts the caller is about to write -- a tensor that only STARTS where a parameter starts (the q rows of a
    stacked in_proj_weight passed as a slice) is not that parameter."""
    if _Arena.mode is None or any(q not in _Arena.by_ptr for q in ptrs):
        return None, False
    slots, ps = _Arena.slots, [_Arena.by_ptr[q] for q in ptrs]
    if numels is not None and any(slots[id(p)][2] != n for p, n in zip(ps, numels)):
        return None, False
    flush_zero()
    if _Arena.mode == "fresh":
        seen = [q in _Arena.written for q in ptrs]
        if any(seen) and not all(seen):
            return None, False
        give = not any(seen)
        if not give:
            _Arena.multi.update(ptrs)
    else:   # accumulate: only slots autograd already holds as .grad (anything else still has last step's data in it)
        if not all(slots.aliased(p) for p in ps):
            return None, False
        give = False
    _Arena.written.update(ptrs)
    return [slots.view(p) for p in ps], give   # fresh view objects per call (GradSlots.view)


def open_decoder(slots, buffers, params, extra):
    """The fused decoder's backward opens its part of the arena: ``slots`` / ``buffers`` are the owner's (enc.grad_arena /
    enc.grad_arena_buffers, slots None without an owner), ``params`` the decoder's parameters, ``extra`` scratch of its own that
    needs zeroing (None: none) and rides on the arena's zero launch.  Returns ({id(param): gradient view}, accumulate, in_place)."""
    in_place = slots is not None and all(id(p) in slots for p in params)
    if not in_place:   # no owner: one flat zeroed fp32 buffer for this pass, every parameter gradient is a view of it
        flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=params[0].device)
        slots, off = GradSlots(), 0
        for p in params:
            slots[id(p)] = (flat, off, p.numel())
            off += p.numel()
        zero([flat, extra])
        return {id(p): slots.view(p) for p in params}, False, False
    # gradients go straight into the owner's flat buffer (data-parallel bucket / optimizer arena): no pack copy.
    # torch semantics of a second backward before zero_grad: gradients ACCUMULATE (the reference trains under
    # accelerator.accumulate, trainer/query3d_trainer.py:35).  Every parameter gradient of the decoder's backward is formed
    # by accumulating launches (split-K atomics, accumulating column sums), so accumulation = not zeroing the arena.
    slots = _slots(slots)
    req = [p for p in params if p.requires_grad]
    if _Arena.whole_pass and _Arena.mode is not None and all(p.data_ptr() in _Arena.by_ptr for p in req):
        # the owner opened the arena around the whole pass (grad_arena): already zeroed / accumulating
        mode = _decide(slots, req, strict=True, given=_Arena.mode)
        if not flush_zero([extra]):   # first consumer of a fresh pass: arena + own scratch, one launch
            zero([extra])
    else:
        # parameters outside the decoder (the input encoders) with slots in the buffers zeroed here: offered to the
        # backward functions that run after this one in the same pass
        rest = slots.by_ptr(buffers, skip={id(p) for p in params})
        mode = _decide(slots, req, strict=True, offered=rest.values())
        zero((list(buffers) if mode == "fresh" else []) + [extra])
        if rest:
            offer(slots, rest, mode)
    return {id(p): slots.view(p) for p in params}, mode == "accumulate", True


# ---- deferred weight gradients of a whole-pass gradient arena ------------------------------------------------------------
# Inside ``with ops.grad_arena(...)`` every dW = g^T (x [+ x2]) of an arena-aware linear layer only feeds its slot of the flat
# gradient buffer, so nothing waits for it: the products are queued per (shape, dtype) bucket and launched as a few GROUPED
# split-K launches when the pass ends (grad_arena.__exit__) instead of one launch per layer -- the caption body's 46 launches of
# [512 x 512] / [2048 x 512] products over 512 rows at config 5 are latency chains of ~15 us each.  The decoder's own backward
# does the same for its layers with a queue of its own; this one serves everything that goes through ops.linear /
# ops.linear_group around it.
_DW_QUEUE = wgrad.Queue(split_x2=True)
_DW_QUEUE_CAP = 256 << 20   # the deferral exists for the latency-bound small-R products; big operands are not held for long


def can_defer(g, x, x2, N, K, pptrs=()) -> bool:
    """May dw[N, K] += g^T (x [+ x2]) wait until the pass ends: only under a whole-pass arena, with operands the grouped launch
    takes, and for no parameter (``pptrs``: data_ptrs, None entries skipped) that carries a gradient hook or an exclusion."""
    if not _Arena.whole_pass or _Arena.mode is None:
        return False
    if (x2 is not None and (x2.dtype != torch.float32 or x.dtype != torch.float32)) or N % 8 or K % 8 or \
            g.data_ptr() % 16 or x.data_ptr() % 16 or (x2 is not None and x2.data_ptr() % 16) or \
            not g.is_contiguous() or not x.is_contiguous():
        return False
    return not any(_param_has_hooks(q) for q in pptrs if q is not None)


_DW_NO_DEFER = set()    # id(param): never deferred (dw_defer_exclude)


def dw_defer_exclude(params, on: bool = True) -> None:
    """Exclude parameters from weight-gradient deferral.  REQUIRED for parameters whose gradient is read by a hook Python cannot see:
    torch DDP's reducer registers its bucket hooks in C++ on the AccumulateGrad node (grad_accumulator->add_post_hook), which neither
    Tensor._backward_hooks nor _post_accumulate_grad_hooks shows -- under a whole-pass gradient arena such a hook would read a slot
    whose queued product only runs when the pass ends.  (The package's own data-parallel path, parallel.FlatGradAllReducer, flushes
    the queue before a bucket leaves and needs no exclusion.)"""
    for p in params:
        (_DW_NO_DEFER.add if on else _DW_NO_DEFER.discard)(id(p))


def _param_has_hooks(q) -> bool:
    """Python-visible gradient hooks (tensor hooks, post-accumulate-grad hooks, Python hooks on the AccumulateGrad node) or an
    explicit exclusion (dw_defer_exclude: C++-side hooks such as DDP's cannot be detected from here)."""
    p_ = _Arena.by_ptr.get(q)
    if p_ is None:
        return False
    if id(p_) in _DW_NO_DEFER or getattr(p_, "_backward_hooks", None) or getattr(p_, "_post_accumulate_grad_hooks", None):
        return True
    try:   # Python hooks registered on the parameter's AccumulateGrad node itself
        acc = p_.view_as(p_).grad_fn.next_functions[0][0]
        return bool(getattr(acc, "_post_hooks", None)) or bool(getattr(acc, "_pre_hooks", None))
    except Exception:  # noqa: BLE001
        return False


def defer(g, x, x2, dw, db, N, K, ct, pptrs=()) -> bool:
    """Queue dw[N, K] += g^T (x [+ x2]) (and db[N] += column sums of g); False when the pass has no whole-pass arena.
    A parameter with Python-visible gradient hooks, or one listed through dw_defer_exclude (torch DDP: its C++ bucket hooks are
    invisible from Python), is never deferred: its hook would read the slot before the queued product has run."""
    if not can_defer(g, x, x2, N, K, pptrs):
        return False
    # the queue keeps its OWN view objects of the slots: AccumulateGrad adopts the returned gradient without a copy only when
    # nobody else references that tensor object (take) -- a second reference would turn .grad into a clone of zeros
    _DW_QUEUE.add([g], [x], [x2], [dw.view(N, K)], ct, [db.view(-1)] if db is not None else None)
    if _DW_QUEUE.nbytes > _DW_QUEUE_CAP:
        dw_deferred_flush()
    return True


def dw_deferred_flush(run: bool = True) -> None:
    """Launch (run=False: drop) the queued weight-gradient products.  Called when the pass ends (grad_arena.__exit__), from
    the fused decoder's readiness reports, from FlatGradAllReducer.launch() / pack() -- no reader of a slot gets ahead of the
    queue -- and when the queue holds more than _DW_QUEUE_CAP bytes of operands."""
    _DW_QUEUE.flush(run)
