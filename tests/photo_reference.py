"""CPU restatement of the photometric / census warp losses (eemflow_amd/csrc/photo.hip, eemflow_amd.photo).

`warp_taps` restates csrc/warp_px.h mode 1 (tensor_tools.torch_warp, utils_luo/tools.py:2262-2306) operation by operation in float32:
the tap weights, the corner values and the warped image Yw the kernel sees.  `loss_from_warped` restates every branch of
Loss_tools.photo_loss_multi_type, photo_loss_function and census_loss_torch (utils_luo/tools.py:3112-3212) in the dtype of its inputs:
in float32 it follows the reference's operation order (tests/golden/photo.npz holds the reference's own results), in float64 on the
float32 Yw it is what the GPU is judged against.

`gradient` is the analytic dL/dflow in float64: dL/dflow(p) = sum_c dL/dYw_c(p) * dYw_c/d(ix, iy)(p) * d(ix, iy)/d(u, v), the derivative
of the bilinear blend at the float32 tap weights (corners outside the frame are zeros) times (W/2) * (2/max(W-1,1)).  Beside it `A`:
per cell the product of the abs-sums of its contributions - (sum over the channels, or for census over the stencil's taps and factors,
of absolute values) times (the abs-sum of the four corner products of the blend's derivative) - an upper bound of |g| under any order
of summation and the scale of the GPU gradient's bound.  `loss_autograd` is the same loss with the taps held fixed and the blend
differentiable in float64, for checking `gradient` against autograd.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

POINTWISE = ("abs_robust", "charbonnier", "L1")
KINDS = POINTWISE + ("census",)
GRAY_RGB = (0.2989, 0.5870, 0.1140)
# every case of the golden file: (kind, use_occ, charbonnier, average, max_distance)
CASES = [(k, occ, False, True, 0) for k in POINTWISE for occ in (False, True)] + \
        [("census", occ, ch, av, r) for r in (1, 3) for ch in (False, True) for av in (True, False) for occ in (False, True)]
Q = 0.4


def default_gray(c):
    return GRAY_RGB if c == 3 else (1.0 / c,) * c


def inputs(seed, shape, zero_mask=False):
    """(flow, img1, img2, mask) float32 arrays of shape (B,C,H,W): a flow of a few low frequencies plus noise whose border columns and
    rows point out of the frame on all four sides, two event-volume-like images (quarter-integer counts, about 65 % zeros - d == 0
    occurs) that differ by a shift and some noise, and a 0/1 mask with a masked-out block (or all zeros)."""
    b, c, h, w = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    flow = np.stack([np.stack([1.5 * np.sin(2 * np.pi * x / w + rng.uniform(0, 6)) + 0.4 * rng.standard_normal((h, w)),
                               1.2 * np.cos(2 * np.pi * y / h + rng.uniform(0, 6)) + 0.4 * rng.standard_normal((h, w))]) for _ in range(b)])
    flow[:, 0, :, 0], flow[:, 0, :, -1] = -1.75, 2.25
    flow[:, 1, 0, :], flow[:, 1, -1, :] = -1.25, 1.5
    img1 = np.round(rng.standard_normal((b, c, h, w)) * 3.0) / 4.0 * (rng.uniform(size=(b, c, h, w)) < 0.35)
    img2 = np.roll(img1, 1, axis=3)
    change = rng.uniform(size=(b, c, h, w)) < 0.3
    img2 = np.where(change, np.round(rng.standard_normal((b, c, h, w)) * 3.0) / 4.0 * (rng.uniform(size=(b, c, h, w)) < 0.35), img2)
    mask = (rng.uniform(size=(b, 1, h, w)) < 0.8).astype(np.float64)
    mask[:, :, : (h + 1) // 2, : (w + 1) // 3] = 0.0
    mask[:, :, h // 2, w // 2] = 1.0                               # (the centre stays: the one interior cell of a 7 x 7 frame at r = 3)
    if zero_mask:
        mask[:] = 0.0
    return flow.astype(np.float32), img1.astype(np.float32), img2.astype(np.float32), mask.astype(np.float32)


def warp_taps(img2, flow):
    """warp_px.h mode 1 in float32: dict of wx, wy (B,1,H,W: ix - floor(ix), iy - floor(iy)), the four weights nw, ne, sw, se, the
    corner values v = [nw, ne, sw, se] (B,C,H,W, zero outside the frame) and the warped image yw."""
    assert img2.dtype == torch.float32 and flow.dtype == torch.float32
    b, c, h, w = img2.shape
    px = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    py = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    vx, vy = px + flow[:, 0:1], py + flow[:, 1:2]
    xn = 2.0 * vx / float(max(w - 1, 1)) - 1.0
    yn = 2.0 * vy / float(max(h - 1, 1)) - 1.0
    ix = (xn + 1.0) * (float(w) / 2.0) - 0.5
    iy = (yn + 1.0) * (float(h) / 2.0) - 0.5
    x0f, y0f = torch.floor(ix), torch.floor(iy)
    wx, wy = ix - x0f, iy - y0f
    ex, ey = 1.0 - wx, 1.0 - wy
    t = {"wx": wx, "wy": wy, "nw": ey * ex, "ne": ey * wx, "sw": wy * ex, "se": wy * wx}
    x0 = x0f.clamp(-2.0, w + 1.0).long()
    y0 = y0f.clamp(-2.0, h + 1.0).long()
    flat = img2.reshape(b, c, h * w)
    v = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = x0 + dx, y0 + dy
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        off = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(b, 1, h * w).expand(b, c, h * w)
        v.append(torch.gather(flat, 2, off).reshape(b, c, h, w) * inside.to(torch.float32))
    t["v"] = v
    t["yw"] = ((v[0] * t["nw"] + v[1] * t["ne"]) + v[2] * t["sw"]) + v[3] * t["se"]
    return t


def _gray_combine(img, gray):
    g = gray[0] * img[:, 0:1]
    for c in range(1, img.shape[1]):
        g = g + gray[c] * img[:, c:c + 1]
    return g


def _patches(g, r):
    """(B,(2r+1)^2,H,W): g at every offset of the patch in row-major order, zero outside the frame (the identity conv2d)."""
    h, w = g.shape[-2:]
    p = F.pad(g, [r, r, r, r])
    return torch.cat([p[:, :, r + dy:r + dy + h, r + dx:r + dx + w] for dy, dx in itertools.product(range(-r, r + 1), repeat=2)], 1)


def _ternary(g, r):
    x = _patches(g, r) - g
    return x / torch.sqrt(0.81 + x ** 2)


def inner_mask(like, r):
    b, _, h, w = like.shape
    return F.pad(torch.ones(b, 1, h - 2 * r, w - 2 * r, dtype=like.dtype), [r, r, r, r])


def census_distance(x, y, r, gray):
    d = (_ternary(_gray_combine(x, gray), r) - _ternary(_gray_combine(y, gray), r)) ** 2
    return torch.sum(d / (0.1 + d), 1, keepdim=True)


def loss_from_warped(x, y, mask=None, kind="census", use_occ=False, q=Q, charbonnier=False, average=True, max_distance=3, gray=None):
    """The loss between x = img1 and y = Yw, a 0-dim tensor of their dtype."""
    if kind in POINTWISE:
        d = x - y
        if kind == "abs_robust":
            l = (d.abs() + 0.01).pow(0.4)
        elif kind == "charbonnier":
            l = (d ** 2 + 1e-6).pow(0.4)
        else:
            l = (d + 1e-6).abs()
        if use_occ:
            m = torch.ones_like(x[:, 0:1]) if mask is None else mask
            return torch.sum(l * m) / (torch.sum(m) + 1e-6)
        return torch.mean(l)
    assert kind == "census"
    r = max_distance
    gray = default_gray(x.shape[1]) if gray is None else gray
    dist = census_distance(x, y, r, gray)
    m = (torch.ones_like(dist) if mask is None else mask) * inner_mask(dist, r)
    if charbonnier:
        if use_occ:
            p = (dist ** 2 + 1e-6).pow(q) * m
            return (p.mean() / (m.mean() * 2 + 1e-6)) if average else (p.sum() / (m.sum() * 2 + 1e-6))
        p = (dist ** 2 + 1e-8).pow(q)
        return p.mean() if average else p.sum()
    if use_occ:
        return torch.sum((dist.abs() + 0.01).pow(q) * m) / (torch.sum(m) * 2 + 1e-6)
    p = (dist.abs() + 0.01).pow(q)
    return p.mean() if average else p.sum()


def loss(flow, img1, img2, mask=None, dtype=torch.float64, **kw):
    """The loss of float32 inputs: the float32 warp, then everything after it in `dtype`."""
    yw = warp_taps(img2, flow)["yw"]
    return loss_from_warped(img1.to(dtype), yw.to(dtype), None if mask is None else mask.to(dtype), **kw)


def term_count(shape, kind):
    b, c, h, w = shape
    return b * h * w * (c if kind in POINTWISE else 1)


def scales(shape):
    _, _, h, w = shape
    return (w / 2.0) * (2.0 / max(w - 1, 1)), (h / 2.0) * (2.0 / max(h - 1, 1))


def _blend_derivative(t):
    """(dYw/dix, dYw/diy, abs-sums of their four products), (B,C,H,W) float64, at the float32 tap weights."""
    v = [a.double() for a in t["v"]]
    ww, wn = t["wx"].double(), t["wy"].double()
    we, ws = (1.0 - t["wx"]).double(), (1.0 - t["wy"]).double()
    dx = ws * (v[1] - v[0]) + wn * (v[3] - v[2])
    dy = we * (v[2] - v[0]) + ww * (v[3] - v[1])
    ax = ws * (v[1].abs() + v[0].abs()) + wn * (v[3].abs() + v[2].abs())
    ay = we * (v[2].abs() + v[0].abs()) + ww * (v[3].abs() + v[1].abs())
    return dx, dy, ax, ay


def gradient(flow, img1, img2, mask=None, kind="census", use_occ=False, q=Q, charbonnier=False, average=True, max_distance=3, gray=None,
             coef=1.0):
    """(coef * dL/dflow, A), both (B,2,H,W) float64."""
    t = warp_taps(img2, flow)
    b, c, h, w = img1.shape
    sx, sy = scales(img1.shape)
    x, y = img1.double(), t["yw"].double()
    m = torch.ones(b, 1, h, w, dtype=torch.float64) if mask is None else mask.double()
    dx, dy, ax, ay = _blend_derivative(t)
    n = float(b * h * w)
    if kind in POINTWISE:
        d = x - y
        if kind == "abs_robust":
            a = d.abs() + 0.01
            dl = 0.4 * a.pow(0.4) / a * torch.sign(d)
        elif kind == "charbonnier":
            a = d ** 2 + 1e-6
            dl = 0.4 * a.pow(0.4) / a * (2.0 * d)
        else:
            dl = torch.sign(d + 1e-6)
        if use_occ:
            sc, mm = coef / (m.sum() + 1e-6), m
        else:
            sc, mm = coef / (n * c), torch.ones_like(m)
        gy = -(dl * mm * sc)
        gu, gv = (gy * dx).sum(1) * sx, (gy * dy).sum(1) * sy
        au, av = (gy.abs() * ax).sum(1) * sx, (gy.abs() * ay).sum(1) * sy
        return torch.stack((gu, gv), 1), torch.stack((au, av), 1)
    r = max_distance
    gray = default_gray(c) if gray is None else gray
    g1, g2 = _gray_combine(x, gray), _gray_combine(y, gray)
    x1, x2 = _patches(g1, r) - g1, _patches(g2, r) - g2
    df = x1 / torch.sqrt(0.81 + x1 ** 2) - x2 / torch.sqrt(0.81 + x2 ** 2)
    e = df ** 2
    dist = torch.sum(e / (0.1 + e), 1, keepdim=True)
    if charbonnier:
        a = dist ** 2 + (1e-6 if use_occ else 1e-8)
        drho = q * a.pow(q) / a * (2.0 * dist)
    else:
        a = dist.abs() + 0.01
        drho = q * a.pow(q) / a * torch.sign(dist)
    if use_occ:
        mm = m * inner_mask(dist, r)
        if charbonnier and average:
            n1, den = n, (mm.sum() / n) * 2 + 1e-6
        else:
            n1, den = 1.0, mm.sum() * 2 + 1e-6
    else:
        mm, n1, den = torch.ones_like(m), (n if average else 1.0), 1.0
    fac = drho * mm * ((coef / n1) / den)
    u2 = 0.81 + x2 ** 2
    s = (0.1 / (0.1 + e) ** 2) * (-2.0 * df) * (0.81 / (u2 * torch.sqrt(u2)))
    fk = _patches(fac, r)
    centre = (2 * r + 1) * r + r
    keep = torch.ones(s.shape[1], dtype=torch.float64).view(1, -1, 1, 1)
    keep[0, centre] = 0.0
    dg = -(s * (fac + fk) * keep).sum(1, keepdim=True)
    adg = (s.abs() * (fac.abs() + fk.abs()) * keep).sum(1, keepdim=True)
    gr = torch.tensor(gray, dtype=torch.float64).view(1, -1, 1, 1)
    gx, gy = (gr * dx).sum(1, keepdim=True), (gr * dy).sum(1, keepdim=True)
    agx, agy = (gr.abs() * ax).sum(1, keepdim=True), (gr.abs() * ay).sum(1, keepdim=True)
    return torch.cat((dg * gx * sx, dg * gy * sy), 1), torch.cat((adg * agx * sx, adg * agy * sy), 1)


def loss_autograd(flow64, taps, img1, mask=None, **kw):
    """The float64 loss as a differentiable function of flow64 (B,2,H,W, requires_grad) with the tap positions, weights and the warped
    VALUE held at their float32 results: Yw = yw32 + (blend(flow64) - blend(flow64).detach()), the blend's weights moving with the
    flow from their float32 values."""
    sx, sy = scales(img1.shape)
    du = (flow64[:, 0:1] - flow64[:, 0:1].detach()) * sx
    dv = (flow64[:, 1:2] - flow64[:, 1:2].detach()) * sy
    ww, we = taps["wx"].double() + du, (1.0 - taps["wx"]).double() - du
    wn, ws = taps["wy"].double() + dv, (1.0 - taps["wy"]).double() - dv
    v = [a.double() for a in taps["v"]]
    blend = ws * we * v[0] + ws * ww * v[1] + wn * we * v[2] + wn * ww * v[3]
    yw = taps["yw"].double() + (blend - blend.detach())
    return loss_from_warped(img1.double(), yw, None if mask is None else mask.double(), **kw)
