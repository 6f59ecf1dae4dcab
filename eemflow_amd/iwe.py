"""Image of warped events (IWE) and the flow warp loss (FWL) on the GPU: a quality number for a flow that needs no ground truth.

Move every event along the estimated flow to one reference time, accumulate the moved events into an image; FWL is the variance of
that image divided by the variance of the plain event-count image, and FWL > 1 means the flow sharpens the events.  The warp is the
reference's `warp_events_flow_torch` (utils_luo/event_utils.py:9-51), the loop around it Test.inference_img_warp_loss
(test_mvsec.py:753-852, the variance ratio at :821-824).

Events are (N,4) float64 CUDA tensors [t, x, y, p], time-sorted, as `EventSequence` holds them (nothing is normalised here); a flow is
a (2,H,W) float32 CUDA tensor in pixels, or None for zero flow.  All arithmetic is unfused fp64 (eemflow_amd/csrc/iwe.hip):

    xe = x - ox, ye = y - oy                     offset = (ox, oy): where the flow's frame starts in event coordinates (a crop)
    (u, v) = bilinear sample of the flow at (xe, ye), pixel coordinates, zero outside the frame (grid_sample, align_corners=True)
    xw = xe + u * (t - t0) * scale,  yw = ye + v * (t - t0) * scale
    four bilinear votes around (floor(yw), floor(xw)) into channel 0 (p > 0) or 1; targets outside the frame are dropped one by one,
    an event with a non-finite warped position is dropped whole and counted; a cell is the fp64 sum of its votes rounded to fp32 once

SIGN CONVENTION of `iwe` / `fwl` (`warp_events` leaves t0 and scale to the caller, as the reference's function does): the flow is the
DISPLACEMENT OVER THE WINDOW, T = t_last - t_first (T = 1 when that is 0, as the voxelizer does).  t_ref="end" (default) sets
t0 = t_last and scale = -1/T: xw = xe + u * (t_last - t) / T, every event is carried FORWARD to the window's end.  t_ref="start" sets
t0 = t_first with the same scale: xw = xe - u * (t - t_first) / T, every event is carried back to the window's start.

moments rows are {H*W, sum S, sum S^2, dropped} with S = iwe[0] + iwe[1]; var = sum S^2 / n - (sum S / n)^2;
FWL = var(IWE under the flow) / var(IWE under zero flow), NaN when the denominator is 0.  CUDA tensors only: there is no CPU path, and
no gradient.  EEM_IWE_DIRECT=1 takes the library's direct atomic form instead of the binned one.
"""
import ctypes

import torch

from . import _lib

MAX_JOBS_PER_CALL = 32


def _check_events(name, ev):
    if not torch.is_tensor(ev):
        raise TypeError(f"{name}: events are tensors")
    if not ev.is_cuda:
        raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if ev.dim() != 2 or ev.shape[1] != 4 or ev.dtype != torch.float64 or not ev.is_contiguous():
        raise ValueError(f"{name}: events are a contiguous (N,4) float64 tensor [t, x, y, p], got {tuple(ev.shape)} {ev.dtype}")


def _check_flow(name, flow, shape=None, dev=None):
    if not torch.is_tensor(flow):
        raise TypeError(f"{name}: a flow is a tensor (or None: zero flow)")
    if not flow.is_cuda:
        raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if flow.dim() != 3 or flow.shape[0] != 2 or flow.dtype != torch.float32 or not flow.is_contiguous():
        raise ValueError(f"{name}: a flow is a contiguous (2,H,W) float32 tensor, got {tuple(flow.shape)} {flow.dtype}")
    if shape is not None and tuple(flow.shape) != tuple(shape):
        raise ValueError(f"{name}: all flows share one (2,H,W) shape, got {tuple(flow.shape)} beside {tuple(shape)}")
    if dev is not None and flow.device != dev:
        raise ValueError(f"{name}: events and flows live on one device")


def _offset(name, offset):
    try:
        ox, oy = offset
        return float(ox), float(oy)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: offset is (ox, oy)") from None


def warp_events(events, flow, t0=None, scale=1.0, offset=(0, 0)):
    """(N,2) float64 [xw, yw] of the events moved along `flow` ((2,H,W) float32): xw = (x - ox) + u * (t - t0) * scale.  t0=None is the
    last event's t, as in the reference; with scale = 1 and offset = (0, 0) this is warp_events_flow_torch(x, y, t, p, flow, t0)."""
    _check_events("warp_events", events)
    _check_flow("warp_events", flow, dev=events.device)
    ox, oy = _offset("warp_events", offset)
    n = events.shape[0]
    dev = events.device
    out = torch.empty(n, 2, device=dev, dtype=torch.float64)
    if n == 0:
        return out
    events = events.detach()
    if t0 is None:
        t0 = float(events[-1, 0])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().eemflow_warp_events(events.data_ptr(), n, flow.detach().data_ptr(), flow.shape[1], flow.shape[2], float(t0),
                                                  float(scale), ox, oy, out.data_ptr(), _lib.current_stream_ptr(dev)))
    return out


def _check_sets(name, event_sets, flows, size):
    event_sets, flows = list(event_sets), list(flows)
    if len(event_sets) < 1 or len(event_sets) != len(flows):
        raise ValueError(f"{name}: one flow (or None) per event set, at least one set; got {len(event_sets)} sets and {len(flows)} flows")
    for ev in event_sets:
        _check_events(name, ev)
    dev = event_sets[0].device
    if any(ev.device != dev for ev in event_sets):
        raise ValueError(f"{name}: events and flows live on one device")
    shape = None
    for fl in flows:
        if fl is not None:
            _check_flow(name, fl, shape, dev)
            shape = tuple(fl.shape)
    if shape is None:
        if size is None:
            raise ValueError(f"{name}: with no flow at all the frame needs size=(H, W)")
        shape = (2, int(size[0]), int(size[1]))
    elif size is not None and (int(size[0]), int(size[1])) != shape[1:]:
        raise ValueError(f"{name}: size={tuple(size)} beside flows of {shape[1:]}")
    if shape[1] < 1 or shape[2] < 1:
        raise ValueError(f"{name}: empty frame {shape[1:]}")
    return event_sets, flows, dev, shape[1], shape[2]


def _time_refs(name, event_sets, t_ref, dev):
    """(t0, scale) per set of the metric convention: one device-to-host copy for all sets."""
    if t_ref not in ("end", "start"):
        raise ValueError(f"{name}: t_ref is 'end' or 'start', got {t_ref!r}")
    live = [ev for ev in event_sets if ev.shape[0] > 0]
    ends = torch.stack([ev[0, 0] for ev in live] + [ev[-1, 0] for ev in live]).tolist() if live else []
    t0s, scales, q = [], [], 0
    for ev in event_sets:
        if ev.shape[0] == 0:
            t0s.append(0.0)
            scales.append(-1.0)
            continue
        first, last = ends[q], ends[len(live) + q]
        q += 1
        span = last - first
        if span == 0:
            span = 1.0
        t0s.append(last if t_ref == "end" else first)
        scales.append(-1.0 / span)
    return t0s, scales


def _launch(event_sets, flows, t0s, scales, ox, oy, h, w, dev):
    k = len(event_sets)
    images = [torch.empty(2, h, w, device=dev, dtype=torch.float32) for _ in range(k)]
    moments = torch.empty(k, 4, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        for i0 in range(0, k, MAX_JOBS_PER_CALL):
            c = min(MAX_JOBS_PER_CALL, k - i0)
            ptr = ctypes.c_void_p * c
            dbl = ctypes.c_double * c
            _lib.check(_lib.lib().eemflow_iwe_many(
                c, ptr(*[e.data_ptr() if e.shape[0] else None for e in event_sets[i0:i0 + c]]),
                (ctypes.c_int64 * c)(*[e.shape[0] for e in event_sets[i0:i0 + c]]),
                ptr(*[f.data_ptr() if f is not None else None for f in flows[i0:i0 + c]]),
                dbl(*t0s[i0:i0 + c]), dbl(*scales[i0:i0 + c]), ox, oy, h, w, ptr(*[t.data_ptr() for t in images[i0:i0 + c]]),
                moments[i0:].data_ptr(), _lib.current_stream_ptr(dev)))
    return images, moments


def iwe_many(event_sets, flows, t_ref="end", offset=(0, 0), size=None):
    """Images of warped events of len(event_sets) event sets under their flows (None: zero flow), all of one frame size:
    `(list of (2,H,W) float32, (k,4) float64 moments)`, both on the device.  One library call per 32 jobs, on the current stream; one
    device-to-host copy of the sets' first and last timestamps.  size=(H, W) names the frame when every flow is None."""
    event_sets, flows, dev, h, w = _check_sets("iwe_many", event_sets, flows, size)
    ox, oy = _offset("iwe_many", offset)
    event_sets = [e.detach() for e in event_sets]
    flows = [f.detach() if f is not None else None for f in flows]
    t0s, scales = _time_refs("iwe_many", event_sets, t_ref, dev)
    return _launch(event_sets, flows, t0s, scales, ox, oy, h, w, dev)


def iwe(events, flow, t_ref="end", offset=(0, 0), size=None):
    """The one-job form of iwe_many: `((2,H,W) float32 image, (4,) float64 moments)`."""
    images, moments = iwe_many([events], [flow], t_ref=t_ref, offset=offset, size=size)
    return images[0], moments[0]


def variance(moments):
    """var S = sum S^2 / n - (sum S / n)^2 of moments rows {n, sum S, sum S^2, dropped}."""
    n = moments[..., 0]
    mean = moments[..., 1] / n
    return moments[..., 2] / n - mean * mean


def fwl_many(event_sets, flows, t_ref="end", offset=(0, 0)):
    """Flow warp loss of every event set under its (2,H,W) flow: a (k,) float64 device tensor, var(IWE under the flow) / var(IWE under
    zero flow), NaN where the denominator is 0.  Each set rides the launch twice - under its flow and under zero flow - so a library
    call carries 16 sets."""
    event_sets, flows = list(event_sets), list(flows)
    if any(f is None for f in flows):
        raise ValueError("fwl_many: every event set needs its flow (zero flow is the denominator)")
    event_sets, flows, dev, h, w = _check_sets("fwl_many", event_sets, flows, None)
    ox, oy = _offset("fwl_many", offset)
    event_sets = [e.detach() for e in event_sets]
    flows = [f.detach() for f in flows]
    t0s, scales = _time_refs("fwl_many", event_sets, t_ref, dev)
    out = []
    half = MAX_JOBS_PER_CALL // 2
    for i0 in range(0, len(event_sets), half):
        evs, fls = event_sets[i0:i0 + half], flows[i0:i0 + half]
        _, m = _launch(evs + evs, fls + [None] * len(evs), t0s[i0:i0 + half] * 2, scales[i0:i0 + half] * 2, ox, oy, h, w, dev)
        var = variance(m)
        num, den = var[:len(evs)], var[len(evs):]
        out.append(torch.where(den == 0, torch.full_like(den, float("nan")), num / den))
    return torch.cat(out)


def fwl(events, flow, t_ref="end", offset=(0, 0)):
    """The one-job form of fwl_many: a 0-dim float64 device tensor."""
    return fwl_many([events], [flow], t_ref=t_ref, offset=offset)[0]
