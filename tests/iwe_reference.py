"""Restatements in torch of the image of warped events (eemflow_amd/iwe.py, csrc/iwe.hip), in the dtype of their inputs:

  warp_events_reference   the reference's warp_events_flow_torch (utils_luo/event_utils.py:9-51) with the same operations in the same
                          order - normalise the coordinates to [-1, 1], grid_sample(align_corners=True), un-normalised nowhere: the
                          flow sample times (t - t0) is added to the coordinates.  tests/golden/iwe.npz holds what the reference's own
                          function returns for the same inputs (make_golden_iwe.py);
  warp_direct / iwe_reference / fwl_reference
                          the semantics the library documents: bilinear sample in pixel coordinates, four bilinear votes summed by
                          index_add_ in the inputs' dtype (the tests pass fp64), the image rounded to fp32 once, the moments of the
                          stored values, the variance ratio.
"""
import math

import torch
import torch.nn.functional as F


def warp_events_reference(x, y, t, p, flow, t0=None):
    """(xw, yw) of warp_events_flow_torch(x, y, t, p, flow, t0); flow (2,H,W) of the events' dtype."""
    if t0 is None:
        t0 = t[-1]
    field = flow
    while field.dim() < 4:
        field = field.unsqueeze(0)
    h, w = field.shape[-2], field.shape[-1]
    grid = torch.reshape(torch.transpose(torch.stack((x, y), dim=0), 0, 1), [1, 1, len(x), 2])
    grid[:, :, :, 0] = grid[:, :, :, 0] / (w - 1) * 2.0 - 1.0
    grid[:, :, :, 1] = grid[:, :, :, 1] / (h - 1) * 2.0 - 1.0
    sampled = F.grid_sample(field, grid, align_corners=True)
    dt = (t - t0).squeeze()
    return x + sampled[:, 0, :, :].squeeze() * dt, y + sampled[:, 1, :, :].squeeze() * dt


def separable_flow(u_row, v_col):
    """(2,H,W) flow whose u depends on x alone (u_row, W values) and whose v depends on y alone (v_col, H values)."""
    h, w = v_col.shape[0], u_row.shape[0]
    return torch.stack([u_row[None, :].expand(h, w), v_col[:, None].expand(h, w)]).contiguous()


def sample_flow(flow, xe, ye):
    """Bilinear sample of a (2,H,W) flow at pixel coordinates (xe, ye): weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy, summed in that
    order, a neighbour outside the frame contributing 0.  Returns (u, v) in xe's dtype."""
    h, w = flow.shape[-2], flow.shape[-1]
    flow = flow.to(xe.dtype)
    x0, y0 = torch.floor(xe), torch.floor(ye)
    fx, fy = xe - x0, ye - y0
    xi = torch.nan_to_num(x0, nan=-2.0).clamp(-2, w + 1).long()
    yi = torch.nan_to_num(y0, nan=-2.0).clamp(-2, h + 1).long()

    def tap(dx, dy, wgt):
        xx, yy = xi + dx, yi + dy
        ok = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
        val = flow[:, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]
        zero = torch.zeros((), dtype=xe.dtype)
        return torch.where(ok, wgt * val[0], zero), torch.where(ok, wgt * val[1], zero)

    taps = [tap(0, 0, (1.0 - fx) * (1.0 - fy)), tap(1, 0, fx * (1.0 - fy)), tap(0, 1, (1.0 - fx) * fy), tap(1, 1, fx * fy)]
    u = ((taps[0][0] + taps[1][0]) + taps[2][0]) + taps[3][0]
    v = ((taps[0][1] + taps[1][1]) + taps[2][1]) + taps[3][1]
    return u, v


def warp_direct(events, flow, t0, scale=1.0, ox=0.0, oy=0.0, size=None):
    """(xw, yw) of the library's warp: events (N,4) [t, x, y, p]; flow (2,H,W) or None (zero flow)."""
    t, x, y = events[:, 0], events[:, 1], events[:, 2]
    xe, ye = x - ox, y - oy
    if flow is None:
        u = v = torch.zeros_like(xe)
    else:
        u, v = sample_flow(flow, xe, ye)
    tau = (t - t0) * scale
    return xe + u * tau, ye + v * tau


def accumulate(xw, yw, p, h, w):
    """((2,H,W) image in xw's dtype, dropped count): four bilinear votes per event, channel 0 for p > 0."""
    finite = torch.isfinite(xw) & torch.isfinite(yw)
    c = torch.where(p > 0, 0, 1)
    xf, yf = torch.floor(xw), torch.floor(yw)
    gx, gy = xw - xf, yw - yf
    xi = torch.nan_to_num(xf, nan=-2.0, posinf=-2.0, neginf=-2.0).clamp(-2, w + 1).long()
    yi = torch.nan_to_num(yf, nan=-2.0, posinf=-2.0, neginf=-2.0).clamp(-2, h + 1).long()
    acc = torch.zeros(2 * h * w, dtype=xw.dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            wgt = (gx if dx else 1.0 - gx) * (gy if dy else 1.0 - gy)
            xx, yy = xi + dx, yi + dy
            ok = finite & (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
            acc.index_add_(0, (c * h * w + yy * w + xx)[ok], wgt[ok])
    return acc.view(2, h, w), int((~finite).sum())


def moments_of(image32):
    """{H*W, sum S, sum S^2} of S = iwe[0] + iwe[1] in fp64 from the stored fp32 image."""
    s = image32[0].double() + image32[1].double()
    return float(s.numel()), float(s.sum()), float((s * s).sum())


def metric_refs(events, t_ref="end"):
    """(t0, scale) of the metric convention: T = t_last - t_first (1 when 0); 'end': t0 = t_last, 'start': t0 = t_first; scale = -1/T."""
    if events.shape[0] == 0:
        return 0.0, -1.0
    first, last = float(events[0, 0]), float(events[-1, 0])
    span = last - first
    if span == 0:
        span = 1.0
    return (last if t_ref == "end" else first), -1.0 / span


def iwe_reference(events, flow, h, w, t_ref="end", offset=(0, 0), t0=None, scale=None):
    """((2,H,W) fp32 image, [H*W, sum S, sum S^2, dropped]) for CPU events (N,4) fp64 and a CPU flow (2,H,W) or None."""
    events = events.double()
    if t0 is None:
        t0, scale = metric_refs(events, t_ref)
    xw, yw = warp_direct(events, flow.double() if flow is not None else None, t0, scale, float(offset[0]), float(offset[1]))
    image, dropped = accumulate(xw, yw, events[:, 3], h, w)
    image32 = image.float()
    return image32, list(moments_of(image32)) + [float(dropped)]


def variance(m):
    return m[2] / m[0] - (m[1] / m[0]) ** 2


def fwl_reference(events, flow, t_ref="end", offset=(0, 0)):
    h, w = flow.shape[-2], flow.shape[-1]
    num = variance(iwe_reference(events, flow, h, w, t_ref, offset)[1])
    den = variance(iwe_reference(events, None, h, w, t_ref, offset)[1])
    return num / den if den != 0 else math.nan
