"""Image of average timestamps, its loss and RSAT on the GPU: the ground-truth-free objective of event-flow learning (Zhu et al. 2019;
Hagenaars et al. 2021) and the evaluation number that goes with it.  The reference has neither; the warp underneath is its
`warp_events_flow_torch` (utils_luo/event_utils.py:9-51), exactly as in iwe.py, whose conventions (events, flows, t_ref, offset, maps,
CUDA tensors only) hold here unchanged.

Per pixel and polarity the image of average timestamps is the vote-weighted mean of the warped events' timestamp values
(eemflow_amd/csrc/tsimg.hip, unfused fp64):

    a = max(1 - |tau|, 0), tau = (t - t0) * scale, rounded to fp32 once    t_ref="end": the normalised timestamp (t - t_first) / T,
                                                                           t_ref="start": one minus it
    D = sum of the votes' weights, N = sum of weight * a                   per channel and cell; D is iwe_many's image, bit for bit
    T = N / (D + eps), stored as fp32
    moments = {H*W, sum T^2 of the stored T, active, dropped}              active: pixels with D[0] + D[1] > 0
    L = sum T^2 / (active + 1e-9)   (normalize="active", Hagenaars' scaling)   or   sum T^2   (normalize="none")

Because every pixel is divided by its own vote count, piling events onto few pixels earns nothing - which the IWE's variance rewards.
`timestamp_loss` is the training term, the mean over the samples of L(end) + L(start); RSAT = L(flow) / L(zero flow), below 1 where
the flow sharpens the events.  The backward is the library's eemflow_tsimg_grad_many: teacher-forced from the stored T and D, with
G = ((2 T) (a - T)) / (D + eps) per event and target in place of the variance's factor, then iwe_grad.hip's kernels.  `active` carries
no gradient.  EEM_IWE_DIRECT=1 takes the library's direct atomic forms.
"""
import ctypes

import torch

from . import _events, _lib
from .iwe import _check_sets, _maps, _time_refs

ACTIVE_EPS = 1e-9


def _eps(name, eps):
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: eps is a positive number") from None
    if not (eps > 0.0 and eps < float("inf")):
        raise ValueError(f"{name}: eps is a positive number, got {eps}")
    return eps


def _normalize(name, normalize):
    if normalize not in ("active", "none"):
        raise ValueError(f"{name}: normalize is 'active' or 'none', got {normalize!r}")
    return normalize


def _launch(event_sets, flows, t0s, scales, maps, h, w, eps, dev):
    """(T images, D images, (k,4) moments) of k jobs: one eemflow_tsimg_many call per 32 jobs on the current stream."""
    k = len(event_sets)
    timgs = [torch.empty(2, h, w, device=dev, dtype=torch.float32) for _ in range(k)]
    dimgs = [torch.empty(2, h, w, device=dev, dtype=torch.float32) for _ in range(k)]
    moments = torch.empty(k, 4, device=dev, dtype=torch.float64)
    _events.call_many("eemflow_tsimg_many", event_sets, flows, t0s, scales, maps, h, w, dev,
                      lambda sl, i0: (eps, _events.pointers(dimgs[sl]), _events.pointers(timgs[sl]), moments[i0:].data_ptr()))
    return timgs, dimgs, moments


def tsimg_grad_many(event_sets, flows, t0s, scales, maps, timgs, dimgs, coef, eps):
    """coef[i] * d (sum T^2)_i / d flows[i] for the jobs of a forward (`_launch`'s arguments and images): a list with one (2,H,W) float32
    tensor per job, None where the flow is None.  coef is a (k,) float64 device tensor; one eemflow_tsimg_grad_many call per 32 jobs
    on the current stream, no host synchronisation."""
    dev = coef.device
    h, w = timgs[0].shape[1], timgs[0].shape[2]
    coef = coef.detach().to(torch.float64).contiguous()
    grads = [torch.empty(2, h, w, device=dev, dtype=torch.float32) if f is not None else None for f in flows]
    _events.call_many("eemflow_tsimg_grad_many", event_sets, flows, t0s, scales, maps, h, w, dev,
                      lambda sl, i0: (eps, _events.pointers(dimgs[sl]), _events.pointers(timgs[sl]), coef[i0:].data_ptr(),
                                      _events.pointers(grads[sl])), needs_flow=True)
    return grads


def last_form():
    """What the calling thread's last library call of this module ran (eemflow_tsimg_last_form): a test observable."""
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.lib().eemflow_tsimg_last_form(buf, len(buf)))
    return buf.value.decode()


def avg_timestamps_many(event_sets, flows, t_ref="end", offset=(0, 0), maps=None, size=None, eps=1e-9):
    """Images of average timestamps of len(event_sets) event sets under their flows (None: zero flow), all of one frame size:
    `(list of (2,H,W) float32 T, list of (2,H,W) float32 D, (k,4) float64 moments {H*W, sum T^2, active, dropped})`, all on the device.
    One library call per 32 jobs on the current stream; one device-to-host copy of the sets' first and last timestamps.  No graph."""
    name = "avg_timestamps_many"
    event_sets, flows, dev, h, w = _check_sets(name, event_sets, flows, size)
    maps = _maps(name, maps, offset, len(event_sets))
    eps = _eps(name, eps)
    event_sets = [e.detach() for e in event_sets]
    flows = [f.detach() if f is not None else None for f in flows]
    t0s, scales = _time_refs(name, event_sets, t_ref, dev)
    return _launch(event_sets, flows, t0s, scales, maps, h, w, eps, dev)


def avg_timestamps(events, flow, t_ref="end", offset=(0, 0), maps=None, size=None, eps=1e-9):
    """The one-job form of avg_timestamps_many: `((2,H,W) T, (2,H,W) D, (4,) moments)`; maps is one (ax, bx, ay, by) or None."""
    t, d, m = avg_timestamps_many([events], [flow], t_ref=t_ref, offset=offset, maps=None if maps is None else [maps], size=size, eps=eps)
    return t[0], d[0], m[0]


def loss_of(moments, normalize="active"):
    """L of moments rows {n, sum T^2, active, dropped}."""
    return moments[..., 1] / (moments[..., 2] + ACTIVE_EPS) if normalize == "active" else moments[..., 1]


def _losses(event_sets, flows, t0s, scales, maps, h, w, dev, eps, normalize):
    """((k,) timestamp losses, moments) of k jobs; backward: one eemflow_tsimg_grad_many call per 32 jobs, coef computed on the device."""
    term = _events.Term(forward=lambda *job: _launch(*job[:-1], eps, job[-1]),
                        backward=lambda ev, fls, t0, sc, mp, images, moments, coef: tsimg_grad_many(ev, fls, t0, sc, mp, *images, coef, eps),
                        loss=lambda moments: loss_of(moments, normalize),
                        coef=lambda gloss, moments: gloss / (moments[:, 2] + ACTIVE_EPS) if normalize == "active" else gloss)
    return _events.losses(term, event_sets, flows, t0s, scales, maps, h, w, dev)


def timestamp_loss_many(event_sets, flows, t_ref="end", offset=(0, 0), maps=None, eps=1e-9, normalize="active"):
    """The timestamp loss L of every event set under its (2,H,W) float32 flow (None: zero flow, at least one flow names the frame): a
    (k,) float64 device tensor, differentiable with respect to every flow that requires grad.  A flow may be a view pred[i] of a
    (B,2,H,W) prediction.  One library call per 32 jobs forward, one backward."""
    name = "timestamp_loss_many"
    event_sets, flows, dev, h, w = _check_sets(name, event_sets, flows, None)
    maps = _maps(name, maps, offset, len(event_sets))
    eps, normalize = _eps(name, eps), _normalize(name, normalize)
    event_sets = [e.detach() for e in event_sets]
    t0s, scales = _time_refs(name, event_sets, t_ref, dev)
    return _losses(event_sets, flows, t0s, scales, maps, h, w, dev, eps, normalize)[0]


def timestamp_loss(event_sets, flows, offset=(0, 0), maps=None, eps=1e-9, normalize="active"):
    """Mean over the samples of L(t_ref='end') + L(t_ref='start'), Zhu's forward plus backward image: a 0-dim float64 device tensor to
    minimise, differentiable with respect to the flows.  Every set rides the launch twice, 16 sets per library call.  A sample without
    an active pixel under either reference is left out of the mean and gets a zero gradient; with every sample left out the loss is
    0.  No host synchronisation beyond the timestamps' copy."""
    name = "timestamp_loss"
    event_sets, flows = list(event_sets), list(flows)
    if any(f is None for f in flows):
        raise ValueError("timestamp_loss: every event set needs its flow")
    event_sets, flows, dev, h, w = _check_sets(name, event_sets, flows, None)
    maps = _maps(name, maps, offset, len(event_sets))
    eps, normalize = _eps(name, eps), _normalize(name, normalize)
    event_sets = [e.detach() for e in event_sets]
    t_start, t_end, scales = _events.window_ends(event_sets)
    total = torch.zeros((), device=dev, dtype=torch.float64)
    count = torch.zeros((), device=dev, dtype=torch.float64)
    for c, jobs in _events.riding_twice((event_sets, event_sets), (flows, flows), (t_end, t_start), (scales, scales), (maps, maps)):
        loss, moments = _losses(*jobs, h, w, dev, eps, normalize)
        active = moments[:, 2]
        ok = (active[:c] > 0) & (active[c:] > 0)
        total = total + torch.where(ok, loss[:c] + loss[c:], torch.zeros_like(loss[:c])).sum()
        count = count + ok.sum()
    return total / count.clamp(min=1.0)


def rsat_many(event_sets, flows, t_ref="end", offset=(0, 0), eps=1e-9):
    """RSAT of every event set under its (2,H,W) flow: a (k,) float64 device tensor, L(flow) / L(zero flow) with normalize="active", NaN
    where the denominator is 0; below 1 where the flow sharpens the events.  Each set rides the launch twice - under its flow and under
    zero flow - so a library call carries 16 sets.  No graph."""
    name = "rsat_many"
    event_sets, flows = list(event_sets), list(flows)
    if any(f is None for f in flows):
        raise ValueError("rsat_many: every event set needs its flow (zero flow is the denominator)")
    event_sets, flows, dev, h, w = _check_sets(name, event_sets, flows, None)
    maps = _maps(name, None, offset, len(event_sets))
    eps = _eps(name, eps)
    event_sets = [e.detach() for e in event_sets]
    flows = [f.detach() for f in flows]
    t0s, scales = _time_refs(name, event_sets, t_ref, dev)
    out = []
    for c, jobs in _events.riding_twice((event_sets, event_sets), (flows, [None] * len(flows)), (t0s, t0s), (scales, scales), (maps, maps)):
        loss = loss_of(_launch(*jobs, h, w, eps, dev)[2])
        out.append(_events.ratio_or_nan(loss[:c], loss[c:]))
    return torch.cat(out)


def rsat(events, flow, t_ref="end", offset=(0, 0), eps=1e-9):
    """The one-job form of rsat_many: a 0-dim float64 device tensor."""
    return rsat_many([events], [flow], t_ref=t_ref, offset=offset, eps=eps)[0]
