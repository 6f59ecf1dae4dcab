"""Weighted SSIM warp loss on the GPU: the structural data term of ground-truth-free training, beside the photometric and census
terms (photo.py), the contrast term (iwe.py) and the smoothness term (smooth.py).

The reference's Loss_tools.weighted_ssim (utils_luo/tools.py:2951-3006) under Loss_tools.photo_loss_multi_type's 'SSIM' kind
(3126-3135) on tensor_tools.torch_warp (2262-2306) as ONE stream-ordered library call per 16 predictions, forward and backward
(eemflow_amd/csrc/ssim.hip).  Yw = torch_warp(img2, flow) is the fp32 warp of eemplus_warp(mode=1), metrics.fb_check and photo.py,
bit for bit; everything after it is unfused fp64 on those fp32 values.  With x = img1, y = Yw, w = mask (ones when None), per channel
and per centre of [1,H-2] x [1,W-2], avg3x3 the nine values added in row-major order and divided by 9:

    aw = avg3x3(w);  wpe = w + weight_epsilon;  inv = 1 / (aw + weight_epsilon);  P[z] = avg3x3(z * wpe) * inv
    mu_x = P[x], mu_y = P[y], s_x = P[x*x] - mu_x^2, s_y = P[y*y] - mu_y^2, s_xy = P[x*y] - mu_x mu_y
    c1 = inf (the default):  n = 2 s_xy + c2,  d = s_x + s_y + c2                      - the structure term
    c2 = inf:                n = 2 mu_x mu_y + c1,  d = mu_x^2 + mu_y^2 + c1            - the luminance term
    both finite:             the products of the two n and of the two d
    l = clamp((1 - n / d) / 2, 0, 1)
    L = mean(l), or with use_occ  sum(l * aw) / (sum(aw) + 1e-6)   (numerator over B*C*(H-2)*(W-2), denominator over the B*(H-2)*(W-2)
    cells of aw)

`flow` is a (B,2,H,W), `img1` / `img2` are (B,C,H,W) with any C >= 1 and `mask` is a (B,1,H,W) float32 CUDA tensor; H and W are at
least 3.  The losses are float64 and differentiable with respect to the flows alone (the clamp passes the gradient on 0 <= v <= 1, as
torch.clamp does); the backward is the same entry point asked for the gradient, with the upstream gradient read from device memory -
nothing is saved between the passes but the inputs, and nothing synchronises with the host.  No atomics: losses and gradients are
bitwise reproducible.  CUDA tensors only: there is no CPU path.
"""
import ctypes
import math

import torch

from . import _lib
from .photo import _check

MAX_JOBS_PER_CALL = 16


def _settings(name, use_occ, c1, c2, weight_epsilon):
    c1, c2, weight_epsilon = float(c1), float(c2), float(weight_epsilon)
    if not (c1 > 0.0 and c2 > 0.0):
        raise ValueError(f"{name}: c1 and c2 are positive (inf switches a term off), got c1={c1!r}, c2={c2!r}")
    if math.isinf(c1) and math.isinf(c2):
        raise ValueError(f"{name}: c1 and c2 are both infinite - the SSIM loss would be zero")
    if not (weight_epsilon > 0.0 and math.isfinite(weight_epsilon)):
        raise ValueError(f"{name}: weight_epsilon is positive and finite, got {weight_epsilon!r}")
    return bool(use_occ), c1, c2, weight_epsilon


def _launch(flows, job, want_loss, coef):
    """One eemflow_ssim_many call per 16 jobs on the current stream: ((N,) float64 losses or None, list of gradients or None).
    flows and the job's tensors are contiguous and detached; coef: None (the loss alone) or a (N,) float64 device tensor."""
    img1, img2, masks, settings = job
    use_occ, c1, c2, eps = settings
    n = len(flows)
    b, _, h, w = flows[0].shape
    c = int(img1[0].shape[1])
    dev = flows[0].device
    lib = _lib.lib()
    loss = torch.empty(n, device=dev, dtype=torch.float64) if want_loss else None
    grads = [torch.empty_like(f) for f in flows] if coef is not None else None
    scratch = torch.empty(max(1, int(lib.eemflow_ssim_scratch_doubles(min(n, MAX_JOBS_PER_CALL), b, h, w))), device=dev, dtype=torch.float64)

    def ptrs(ts, i0, k):
        return (ctypes.c_void_p * k)(*[t.data_ptr() if t is not None else None for t in ts[i0:i0 + k]])
    with torch.cuda.device(dev):
        for i0 in range(0, n, MAX_JOBS_PER_CALL):
            k = min(MAX_JOBS_PER_CALL, n - i0)
            _lib.check(lib.eemflow_ssim_many(
                k, ptrs(flows, i0, k), ptrs(img1, i0, k), ptrs(img2, i0, k), ptrs(masks, i0, k), b, c, h, w, int(use_occ), c1, c2, eps,
                coef[i0:].data_ptr() if coef is not None else None, loss[i0:].data_ptr() if want_loss else None,
                ptrs(grads, i0, k) if grads is not None else None, scratch.data_ptr(), _lib.current_stream_ptr(dev)))
    return loss, grads


class _Ssim(torch.autograd.Function):
    """(N,) losses of N flows; backward: the same entry point asked for coef * dL/dflow (nothing saved but the inputs)."""

    @staticmethod
    def forward(ctx, job, *flows):
        flows = [f.detach() for f in flows]
        ctx.job, ctx.flows = job, flows
        return _launch(flows, job, True, None)[0]

    @staticmethod
    def backward(ctx, gloss):
        coef = gloss.detach().to(torch.float64).contiguous()
        grads = _launch(ctx.flows, ctx.job, False, coef)[1]
        return (None,) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[1:]))


def ssim_many(flows, img1, img2, mask=None, use_occ=False, c1=float("inf"), c2=9e-6, weight_epsilon=0.01):
    """Weighted SSIM losses between img1 and img2 warped back by each of `flows` (a list of (B,2,H,W) float32 CUDA tensors of one
    shape): a (N,) float64 device tensor, differentiable with respect to every flow.  img1, img2 and mask are one tensor shared by all
    flows or a list with one per flow (mask entries may be None: a weight of ones).  c1 / c2 regularise the luminance / structure term,
    inf switches one off; weight_epsilon regularises the division by the pooled weight.  One library call per 16 flows forward and one
    backward, on the current stream; non-contiguous inputs are made contiguous."""
    name = "ssim_many"
    settings = _settings(name, use_occ, c1, c2, weight_epsilon)
    flows = list(flows)
    if len(flows) < 1:
        raise ValueError(f"{name}: at least one flow")
    for f in flows:
        _check(name, "a flow", f, 2)
    shape, dev = tuple(flows[0].shape), flows[0].device
    if any(tuple(f.shape) != shape for f in flows):
        raise ValueError(f"{name}: all flows share one (B,2,H,W) shape, got {[tuple(f.shape) for f in flows]}")

    def per_flow(what, x, optional=False):
        xs = [x] * len(flows) if x is None or torch.is_tensor(x) else list(x)
        if len(xs) != len(flows):
            raise ValueError(f"{name}: one {what} per flow; got {len(xs)} for {len(flows)} flows")
        if not optional and any(t is None for t in xs):
            raise ValueError(f"{name}: {what} is required")
        return xs
    img1, img2, masks = per_flow("img1", img1), per_flow("img2", img2), per_flow("mask", mask, optional=True)
    channels = int(img1[0].shape[1]) if torch.is_tensor(img1[0]) and img1[0].dim() == 4 else None
    for what, ts in (("img1", img1), ("img2", img2)):
        for t in ts:
            _check(name, what, t)
            if (t.shape[0],) + tuple(t.shape[2:]) != (shape[0],) + shape[2:]:
                raise ValueError(f"{name}: {what} {tuple(t.shape)} beside a flow {shape}: B, H and W must agree")
            if t.shape[1] < 1 or t.shape[1] != channels:
                raise ValueError(f"{name}: img1 and img2 share one channel count C >= 1")
    for t in masks:
        if t is None:
            continue
        _check(name, "mask", t, 1)
        if (t.shape[0],) + tuple(t.shape[2:]) != (shape[0],) + shape[2:]:
            raise ValueError(f"{name}: mask {tuple(t.shape)} beside a flow {shape}: B, H and W must agree")
    if any(t.device != dev for t in flows + img1 + img2 + [m for m in masks if m is not None]):
        raise ValueError(f"{name}: flows, images and masks live on one device")
    if shape[2] < 3 or shape[3] < 3:
        raise ValueError(f"{name}: the 3 x 3 windows need H >= 3 and W >= 3, got {shape[2]}x{shape[3]}")
    made = {}                                                      # one contiguous tensor per distinct input: shared stays shared

    def cont(t):
        if t is None:
            return None
        if id(t) not in made:
            made[id(t)] = t.detach().contiguous()
        return made[id(t)]
    job = ([cont(t) for t in img1], [cont(t) for t in img2], [cont(t) for t in masks], settings)
    return _Ssim.apply(job, *[f.contiguous() for f in flows])


def ssim_loss(flow, img1, img2, mask=None, **kw):
    """The one-flow form of ssim_many: a 0-dim float64 device tensor."""
    return ssim_many([flow], img1, img2, mask, **kw)[0]
