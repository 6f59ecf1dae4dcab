"""Restatement in torch (fp64, CPU) of the image of average timestamps, its loss and the loss's gradient (eemflow_amd/tsimg.py,
csrc/tsimg.hip), on top of tests/iwe_reference.py and tests/iwe_grad_reference.py, which it imports unchanged:

  planes           D = sum of w, N = sum of w * a and the vote count V per channel and cell; quantised=True takes the library's number
                   formats - w = floor(w * 2^31 + 0.5) / 2^31 and a rounded to fp32 once - both straight-through, so the planes stay
                   differentiable in the flow;
  loss_reference   T = N / (D + eps), its fp32 rounding, the moments of the stored values and the loss;
  grad_reference   the explicit formula the library documents - G = ((2 T) (ah - T)) / (D + eps) per event and in-frame target from
                   STORED images, the per-event derivative, w_k * tau of it to every in-frame sample neighbour - and the abs-sum map A
                   built with |G|, the scale of the rounding errors a cell may collect;
  loss_autograd    the same loss through torch autograd, teacher-forced: the value of D is the stored D32 and the value of N is
                   T32 * (D32 + eps), both straight-through, so autograd's derivative is taken where the explicit formula takes it.
"""
import torch

from iwe_grad_reference import IDENTITY, map_events
from iwe_reference import warp_direct

ACTIVE_EPS = 1e-9


def time_value(events, t0, scale, rounded=True):
    """a = max(1 - |tau|, 0) per event; rounded: to fp32 once."""
    a = (1.0 - ((events[:, 0].double() - t0) * scale).abs()).clamp(min=0.0)
    return a.float().double() if rounded else a


def planes(events, flow, t0, scale, amap=IDENTITY, quantised=False, round_a=None, size=None):
    """(D, N, V): three (2,H,W) fp64 planes.  flow (2,H,W) fp64 (it may require grad) or None with size=(H, W); V counts the votes of
    non-zero weight."""
    return _planes(events, flow, t0, scale, amap, quantised, round_a, size)[:3]


def _planes(events, flow, t0, scale, amap, quantised, round_a, size):
    """planes and the count of events with a non-finite warped position."""
    ev = map_events(events.double(), amap)
    h, w = (flow.shape[-2], flow.shape[-1]) if flow is not None else size
    xw, yw = warp_direct(ev, flow.double() if flow is not None else None, t0, scale)
    a = time_value(ev, t0, scale, quantised if round_a is None else round_a)
    finite = torch.isfinite(xw) & torch.isfinite(yw)
    c = torch.where(ev[:, 3] > 0, 0, 1)
    xf, yf = torch.floor(xw), torch.floor(yw)
    gx, gy = xw - xf, yw - yf
    xi = torch.nan_to_num(xf.detach(), nan=-2.0, posinf=-2.0, neginf=-2.0).clamp(-2, w + 1).long()
    yi = torch.nan_to_num(yf.detach(), nan=-2.0, posinf=-2.0, neginf=-2.0).clamp(-2, h + 1).long()
    D = torch.zeros(2 * h * w, dtype=torch.float64)
    N = torch.zeros(2 * h * w, dtype=torch.float64)
    V = torch.zeros(2 * h * w, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            wgt = (gy if dy else 1.0 - gy) * (gx if dx else 1.0 - gx)        # wy * wx, the library's order
            if quantised:
                wgt = wgt + (torch.floor(wgt.detach() * 2.0 ** 31 + 0.5) / 2.0 ** 31 - wgt.detach())
            xx, yy = xi + dx, yi + dy
            ok = finite & (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
            idx = (c * h * w + yy * w + xx)[ok]
            D = D.index_add(0, idx, wgt[ok])
            N = N.index_add(0, idx, (wgt * a)[ok])
            V = V.index_add(0, idx, (wgt[ok].detach() > 0).double())
    return D.view(2, h, w), N.view(2, h, w), V.view(2, h, w), int((~finite).sum())


def moments_of(D32, T32, dropped=0.0):
    """[H*W, sum T^2, active, dropped] in fp64 from STORED images."""
    t = T32.double()
    active = float(((D32[0].double() + D32[1].double()) > 0).sum())
    return [float(D32.shape[-2] * D32.shape[-1]), float((t * t).sum()), active, float(dropped)]


def loss_of(m, normalize="active"):
    return m[1] / (m[2] + ACTIVE_EPS) if normalize == "active" else m[1]


def loss_reference(events, flow, t0, scale, amap=IDENTITY, eps=1e-9, normalize="active", quantised=False, size=None):
    """dict(D, N, V, T in fp64; D32, T32 the stored roundings; moments; loss) of one job."""
    with torch.no_grad():
        D, N, V, dropped = _planes(events, flow, t0, scale, amap, quantised, None, size)
    T = N / (D + eps)
    D32, T32 = D.float(), T.float()
    m = moments_of(D32, T32, dropped)
    return dict(D=D, N=N, V=V, T=T, D32=D32, T32=T32, moments=m, loss=loss_of(m, normalize))


def grad_reference(events, flow, D32, T32, coef, eps, t0, scale, amap=IDENTITY):
    """(gradient, A), both (2,H,W) fp64: coef * d (sum T^2) / d flow by the explicit formula from the STORED images D32 and T32 (any
    float dtype), and the abs-sum map."""
    events = events.double()
    flow = flow.double()
    h, w = flow.shape[-2], flow.shape[-1]
    ev = map_events(events, amap)
    t, xe, ye = ev[:, 0], ev[:, 1], ev[:, 2]
    xw, yw = warp_direct(ev, flow, t0, scale)
    tau = (t - t0) * scale
    ah = time_value(ev, t0, scale, True)
    finite = torch.isfinite(xw) & torch.isfinite(yw)
    c = torch.where(ev[:, 3] > 0, 0, 1)
    Tf, Df = T32.double().reshape(-1), D32.double().reshape(-1)

    xf, yf = torch.floor(xw), torch.floor(yw)
    gx, gy = xw - xf, yw - yf
    X0 = torch.nan_to_num(xf, nan=-2.0, posinf=-2.0, neginf=-2.0).clamp(-2, w + 1).long()
    Y0 = torch.nan_to_num(yf, nan=-2.0, posinf=-2.0, neginf=-2.0).clamp(-2, h + 1).long()
    zero = torch.zeros_like(xw)
    dX, dY, aX, aY = zero.clone(), zero.clone(), zero.clone(), zero.clone()
    for dy in (0, 1):
        for dx in (0, 1):
            X, Y = X0 + dx, Y0 + dy
            ok = finite & (X >= 0) & (X <= w - 1) & (Y >= 0) & (Y <= h - 1)
            o = c * h * w + Y.clamp(0, h - 1) * w + X.clamp(0, w - 1)
            Tc, Dc = Tf[o], Df[o]
            g = torch.where(ok, ((2.0 * Tc) * (ah - Tc)) / (Dc + eps), zero)
            wy = torch.where(ok, gy if dy else 1.0 - gy, zero)
            wx = torch.where(ok, gx if dx else 1.0 - gx, zero)
            dX = dX + g * wy * (1.0 if dx else -1.0)
            dY = dY + g * wx * (1.0 if dy else -1.0)
            aX = aX + g.abs() * wy
            aY = aY + g.abs() * wx

    x0f, y0f = torch.floor(xe), torch.floor(ye)
    fx, fy = xe - x0f, ye - y0f
    x0 = torch.nan_to_num(x0f, nan=-2.0).clamp(-2, w + 1).long()
    y0 = torch.nan_to_num(y0f, nan=-2.0).clamp(-2, h + 1).long()
    grad = torch.zeros(2, h * w, dtype=torch.float64)
    A = torch.zeros(2, h * w, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            wk = (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)
            xx, yy = x0 + dx, y0 + dy
            ok = finite & (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
            idx = (yy * w + xx)[ok]
            grad[0].index_add_(0, idx, (coef * wk * tau * dX)[ok])
            grad[1].index_add_(0, idx, (coef * wk * tau * dY)[ok])
            A[0].index_add_(0, idx, (abs(coef) * wk * tau.abs() * aX)[ok])
            A[1].index_add_(0, idx, (abs(coef) * wk * tau.abs() * aY)[ok])
    return grad.view(2, h, w), A.view(2, h, w)


def loss_autograd(events, flow, t0, scale, amap=IDENTITY, eps=1e-9, normalize="active", D32=None, T32=None):
    """(loss, D32, T32, moments) with the loss differentiable in the fp64 `flow`.  Teacher-forced: with D32 / T32 given (the library's
    stored images) the values are theirs, else the restatement's own roundings; either way the roundings are straight-through."""
    D, N, _, dropped = _planes(events, flow, t0, scale, amap, True, None, None)
    if D32 is None:
        D32 = D.detach().float()
        T32 = (N.detach() / (D.detach() + eps)).float()
    Dv, Tv = D32.double(), T32.double()
    D_st = D + (Dv - D).detach()
    N_st = N + (Tv * (Dv + eps) - N).detach()
    T = N_st / (D_st + eps)
    m = moments_of(D32, T32, dropped)
    sumsq = (T * T).sum()
    loss = sumsq / (m[2] + ACTIVE_EPS) if normalize == "active" else sumsq
    return loss, D32, T32, m


def loss_fp64(events, flow, t0, scale, amap=IDENTITY, eps=1e-9, normalize="active"):
    """The loss with no fp32 rounding of an image and no fixed-point weight (a rounded once, as the library's): a smooth function of
    the flow between two changes of cell, for difference quotients.  Returns (loss, D, T) with D and T the fp64 images."""
    D, N, _ = planes(events, flow, t0, scale, amap, quantised=False, round_a=True)
    T = N / (D + eps)
    active = float(((D[0] + D[1]).detach() > 0).sum())
    sumsq = (T * T).sum()
    return (sumsq / (active + ACTIVE_EPS) if normalize == "active" else sumsq), D, T


def rsat_reference(events, flow, t0, scale, amap=IDENTITY, eps=1e-9, quantised=False):
    num = loss_reference(events, flow, t0, scale, amap, eps, quantised=quantised)["loss"]
    den = loss_reference(events, None, t0, scale, amap, eps, quantised=quantised, size=tuple(flow.shape[-2:]))["loss"]
    return num / den if den != 0 else float("nan")
