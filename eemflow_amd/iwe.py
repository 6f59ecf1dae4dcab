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
FWL = var(IWE under the flow) / var(IWE under zero flow), NaN when the denominator is 0.  CUDA tensors only: there is no CPU path.
EEM_IWE_DIRECT=1 takes the library's direct atomic form instead of the binned one.

GRADIENT (contrast maximisation).  `contrast_many` returns the variances and is differentiable with respect to the flows; `fwl_loss` is
minus the mean FWL of a batch, the self-supervised training objective (train.contrast_loss applies it to a prediction).  The backward
is the library's eemflow_iwe_grad_many (csrc/iwe_grad.hip): with G = 2 (S - mean) / (H W) per cell - the fp32 rounding of the stored
image taken as the identity - an event hands d var / d xw = sum over its in-frame targets of G * wy[dy] * (dx ? +1 : -1) (and the same
in y) times w_k * tau to each in-frame sample neighbour k of (xe, ye).  `iwe`, `iwe_many`, `fwl` and `fwl_many` build no graph.

EVENT MAPS.  `maps=` gives one affine map (ax, bx, ay, by) per event set in place of `offset`: xe = ax * x + bx, ye = ay * y + by - where
the events of an augmented (resized, flipped, cropped) sample lie in its frame (AugPlan.event_map; the datasets' get_batch hands them
out as batch['events_map']).  offset = (ox, oy) is the map (1, -ox, 1, -oy), bit for bit.

The image of average timestamps, the objective that divides every pixel by its own vote count, and RSAT are in tsimg.py: the same
warp, the same votes (its D image is this module's image, bit for bit) and the same gradient kernels under another per-target factor.
"""
import torch

from . import _events, _lib
from ._events import MAX_JOBS_PER_CALL, map_table as _map_table  # noqa: F401


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
    firsts, lasts, scales = _events.window_ends(event_sets)
    return (lasts if t_ref == "end" else firsts), scales


def _maps(name, maps, offset, k):
    if maps is None:
        ox, oy = _offset(name, offset)
        return [(1.0, -ox, 1.0, -oy)] * k
    maps = list(maps)
    if len(maps) != k:
        raise ValueError(f"{name}: one map (ax, bx, ay, by) per event set; got {len(maps)} maps for {k} sets")
    out = []
    for m in maps:
        try:
            ax, bx, ay, by = m
            out.append((float(ax), float(bx), float(ay), float(by)))
        except (TypeError, ValueError):
            raise ValueError(f"{name}: a map is (ax, bx, ay, by)") from None
    return out


def _launch_maps(event_sets, flows, t0s, scales, maps, h, w, dev):
    """(images, (k,4) moments) of k jobs: one eemflow_iwe_map_many call per 32 jobs on the current stream."""
    k = len(event_sets)
    images = [torch.empty(2, h, w, device=dev, dtype=torch.float32) for _ in range(k)]
    moments = torch.empty(k, 4, device=dev, dtype=torch.float64)
    _events.call_many("eemflow_iwe_map_many", event_sets, flows, t0s, scales, maps, h, w, dev,
                      lambda sl, i0: (_events.pointers(images[sl]), moments[i0:].data_ptr()))
    return images, moments


def iwe_many(event_sets, flows, t_ref="end", offset=(0, 0), size=None):
    """Images of warped events of len(event_sets) event sets under their flows (None: zero flow), all of one frame size:
    `(list of (2,H,W) float32, (k,4) float64 moments)`, both on the device.  One library call per 32 jobs, on the current stream; one
    device-to-host copy of the sets' first and last timestamps.  size=(H, W) names the frame when every flow is None."""
    event_sets, flows, dev, h, w = _check_sets("iwe_many", event_sets, flows, size)
    maps = _maps("iwe_many", None, offset, len(event_sets))
    event_sets = [e.detach() for e in event_sets]
    flows = [f.detach() if f is not None else None for f in flows]
    t0s, scales = _time_refs("iwe_many", event_sets, t_ref, dev)
    return _launch_maps(event_sets, flows, t0s, scales, maps, h, w, dev)


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
    maps = _maps("fwl_many", None, offset, len(event_sets))
    event_sets = [e.detach() for e in event_sets]
    flows = [f.detach() for f in flows]
    t0s, scales = _time_refs("fwl_many", event_sets, t_ref, dev)
    out = []
    for c, jobs in _events.riding_twice((event_sets, event_sets), (flows, [None] * len(flows)), (t0s, t0s), (scales, scales), (maps, maps)):
        var = variance(_launch_maps(*jobs, h, w, dev)[1])
        out.append(_events.ratio_or_nan(var[:c], var[c:]))
    return torch.cat(out)


def fwl(events, flow, t_ref="end", offset=(0, 0)):
    """The one-job form of fwl_many: a 0-dim float64 device tensor."""
    return fwl_many([events], [flow], t_ref=t_ref, offset=offset)[0]


# ------------------------------------------------------------------------------------------------ gradient: contrast maximisation
def iwe_grad_many(event_sets, flows, t0s, scales, maps, images, moments, coef):
    """coef[i] * d var_i / d flows[i] for the jobs of a forward (`_launch_maps`' arguments, its images and moments): a list with one
    (2,H,W) float32 tensor per job, None where the flow is None.  coef is a (k,) float64 device tensor; one eemflow_iwe_grad_many call
    per 32 jobs on the current stream, no host synchronisation."""
    dev = moments.device
    h, w = images[0].shape[1], images[0].shape[2]
    coef = coef.detach().to(torch.float64).contiguous()
    moments = moments.contiguous()
    grads = [torch.empty(2, h, w, device=dev, dtype=torch.float32) if f is not None else None for f in flows]
    _events.call_many("eemflow_iwe_grad_many", event_sets, flows, t0s, scales, maps, h, w, dev,
                      lambda sl, i0: (_events.pointers(images[sl]), moments[i0:].data_ptr(), coef[i0:].data_ptr(), _events.pointers(grads[sl])),
                      needs_flow=True)
    return grads


# (k,) variances of the images of warped events of k jobs; backward: one eemflow_iwe_grad_many call per 32 jobs
_CONTRAST = _events.Term(forward=_launch_maps,
                         backward=lambda ev, flows, t0s, scales, maps, images, moments, coef:
                             iwe_grad_many(ev, flows, t0s, scales, maps, images[0], moments, coef),
                         loss=variance, coef=lambda gvar, moments: gvar)


def _contrast(name, event_sets, flows, t_ref, offset, maps):
    event_sets, flows, dev, h, w = _check_sets(name, event_sets, flows, None)
    maps = _maps(name, maps, offset, len(event_sets))
    event_sets = [e.detach() for e in event_sets]
    t0s, scales = _time_refs(name, event_sets, t_ref, dev)
    return event_sets, flows, t0s, scales, maps, h, w, dev


def _variances(event_sets, flows, t0s, scales, maps, h, w, dev):
    return _events.losses(_CONTRAST, event_sets, flows, t0s, scales, maps, h, w, dev)


def contrast_many(event_sets, flows, t_ref="end", offset=(0, 0), maps=None):
    """Variance of the image of warped events of every event set under its (2,H,W) float32 flow (None: zero flow, at least one flow
    names the frame): a (k,) float64 device tensor, differentiable with respect to every flow that requires grad - the contrast that
    contrast maximisation raises.  A flow may be a view pred[i] of a (B,2,H,W) prediction: autograd adds the gradients back into the
    batch tensor.  maps: one (ax, bx, ay, by) per set in place of `offset`.  One library call per 32 jobs forward, one backward."""
    job = _contrast("contrast_many", event_sets, flows, t_ref, offset, maps)
    return _variances(*job)[0]


def fwl_loss(event_sets, flows, t_ref="end", offset=(0, 0), maps=None):
    """Minus the mean over the samples of var(IWE under the flow) / var(IWE under zero flow): a 0-dim float64 device tensor to minimise,
    differentiable with respect to the flows.  As in fwl_many each set rides the launch twice, 16 sets per library call.  A sample whose
    zero-flow variance is 0 or not finite is left out of the mean and gets a zero gradient; with every sample left out the loss is 0.
    No host synchronisation beyond the timestamps' copy."""
    event_sets, flows = list(event_sets), list(flows)
    if any(f is None for f in flows):
        raise ValueError("fwl_loss: every event set needs its flow (zero flow is the denominator)")
    event_sets, flows, t0s, scales, maps, h, w, dev = _contrast("fwl_loss", event_sets, flows, t_ref, offset, maps)
    total = torch.zeros((), device=dev, dtype=torch.float64)
    count = torch.zeros((), device=dev, dtype=torch.float64)
    for c, jobs in _events.riding_twice((event_sets, event_sets), (flows, [None] * len(flows)), (t0s, t0s), (scales, scales), (maps, maps)):
        var, _ = _variances(*jobs, h, w, dev)
        num, den = var[:c], var[c:]
        ok = torch.isfinite(den) & (den != 0)
        ratio = torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(num))
        total = total + ratio.sum()
        count = count + ok.sum()
    return -total / count.clamp(min=1.0)
