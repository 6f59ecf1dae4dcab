"""What the event losses share on the host (iwe.py, tsimg.py; their kernels share csrc/iwe_fwd_shared.h and csrc/iwe_grad_shared.h): the
call of a *_many entry point per 32 jobs, the autograd function around a forward and a backward entry point, the windows' first and
last timestamps, and "each set rides the launch twice".

A job of the library is an event set, its flow (or None: zero flow), t0, scale and an event map (ax, bx, ay, by); every *_many entry
point starts with the same arguments for them and ends with the stream, with its own arguments in between.
"""
import collections
import ctypes
import itertools

import torch

from . import _lib

MAX_JOBS_PER_CALL = 32


def pointers(ts):
    """The (void*)[len(ts)] of some tensors' data (None: NULL)."""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def map_table(maps):
    return (ctypes.c_double * (4 * len(maps)))(*itertools.chain.from_iterable(maps))


def call_many(entry, event_sets, flows, t0s, scales, maps, h, w, dev, tail, needs_flow=False):
    """One call of the library's `entry` per 32 jobs on the current stream.  tail(sl, i0) gives the entry's own arguments for the jobs
    `sl` (a slice that starts at i0), those between the frame size and the stream; needs_flow leaves a call without any flow out."""
    with torch.cuda.device(dev):
        for i0 in range(0, len(event_sets), MAX_JOBS_PER_CALL):
            sl = slice(i0, i0 + MAX_JOBS_PER_CALL)
            c = len(event_sets[sl])
            if needs_flow and all(f is None for f in flows[sl]):
                continue
            dbl = ctypes.c_double * c
            _lib.check(getattr(_lib.lib(), entry)(
                c, pointers([e if e.shape[0] else None for e in event_sets[sl]]), (ctypes.c_int64 * c)(*[e.shape[0] for e in event_sets[sl]]),
                pointers(flows[sl]), dbl(*t0s[sl]), dbl(*scales[sl]), map_table(maps[sl]), h, w, *tail(sl, i0),
                _lib.current_stream_ptr(dev)))


def window_ends(event_sets):
    """(first timestamps, last timestamps, scales = -1 / (last - first), the span 1 where it is 0) per set, an empty set (0, 0, -1): one
    device-to-host copy for all sets."""
    live = [ev for ev in event_sets if ev.shape[0] > 0]
    ends = torch.stack([ev[0, 0] for ev in live] + [ev[-1, 0] for ev in live]).tolist() if live else []
    firsts, lasts, scales, q = [], [], [], 0
    for ev in event_sets:
        if ev.shape[0] == 0:
            firsts.append(0.0)
            lasts.append(0.0)
            scales.append(-1.0)
            continue
        first, last = ends[q], ends[len(live) + q]
        q += 1
        span = last - first
        if span == 0:
            span = 1.0
        firsts.append(first)
        lasts.append(last)
        scales.append(-1.0 / span)
    return firsts, lasts, scales


def riding_twice(*columns):
    """Each set rides a launch twice, so a library call carries 16 sets.  A column is the pair (first ride, second ride) of one per-set
    list; yields (c, the columns' lists of 2 c jobs - the c first rides, then the c second ones) per call."""
    half = MAX_JOBS_PER_CALL // 2
    for i0 in range(0, len(columns[0][0]), half):
        sl = slice(i0, i0 + half)
        yield len(columns[0][0][sl]), [first[sl] + second[sl] for first, second in columns]


def ratio_or_nan(num, den):
    return torch.where(den == 0, torch.full_like(den, float("nan")), num / den)


# forward(event_sets, flows, t0s, scales, maps, h, w, dev) -> (*images, moments); backward(event_sets, flows, t0s, scales, maps, images,
# moments, coef) -> the gradients, None where the flow is None; loss(moments) -> (k,) losses; coef(gloss, moments) -> the backward's coef
Term = collections.namedtuple("Term", "forward backward loss coef")


class _EventLoss(torch.autograd.Function):
    """(k,) losses of k jobs under a Term; backward: the term's backward entry point, one call per 32 jobs."""

    @staticmethod
    def forward(ctx, term, job, *flows):
        event_sets, slots, t0s, scales, maps, h, w, dev = job
        full = [None] * len(event_sets)                            # the flow (or None: zero flow) of every job
        for i, f in zip(slots, flows):
            full[i] = f.detach()
        *images, moments = term.forward(event_sets, full, t0s, scales, maps, h, w, dev)
        ctx.term, ctx.job, ctx.full, ctx.images, ctx.moments = term, job, full, images, moments
        ctx.mark_non_differentiable(moments)
        return term.loss(moments), moments

    @staticmethod
    def backward(ctx, gloss, _gmoments):
        event_sets, slots, t0s, scales, maps, h, w, dev = ctx.job
        wanted = [None] * len(event_sets)                          # a flow that needs no gradient is skipped like a zero flow
        for q, i in enumerate(slots):
            if ctx.needs_input_grad[2 + q]:
                wanted[i] = ctx.full[i]
        grads = ctx.term.backward(event_sets, wanted, t0s, scales, maps, ctx.images, ctx.moments, ctx.term.coef(gloss, ctx.moments))
        return (None, None) + tuple(grads[i] if wanted[i] is not None else None for i in slots)


def losses(term, event_sets, flows, t0s, scales, maps, h, w, dev):
    """((k,) losses, (k,4) moments) of the jobs under `term`, the losses differentiable with respect to every flow that requires grad."""
    slots = [i for i, f in enumerate(flows) if f is not None]
    return _EventLoss.apply(term, (event_sets, slots, t0s, scales, maps, h, w, dev), *[flows[i] for i in slots])
