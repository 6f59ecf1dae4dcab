"""Photometric and census warp losses on the GPU: the data term of ground-truth-free training, beside the contrast term (iwe.py)
and the smoothness term (smooth.py).

The reference's Loss_tools.photo_loss_multi_type, photo_loss_function and census_loss_torch (utils_luo/tools.py:3112-3212) on
tensor_tools.torch_warp (2262-2306) as ONE stream-ordered library call per 16 predictions, forward and backward
(eemflow_amd/csrc/photo.hip).  Yw = torch_warp(img2, flow) is the fp32 warp of eemplus_warp(mode=1) and metrics.fb_check, bit for bit;
everything after it is unfused fp64 on those fp32 values.  With d = img1 - Yw:

    'abs_robust'   l = (|d| + 0.01) ** 0.4          'charbonnier'   l = (d*d + 1e-6) ** 0.4          'L1'   l = |d + 1e-6|
    L = mean(l), or with use_occ  sum(l * mask) / (sum(mask) + 1e-6)   (numerator over B*C*H*W, denominator over the B*H*W mask cells)
    'census'       g(I) = sum_c gray[c] * I_c (0 outside the frame);  t_k(p) = tau(g(p+k) - g(p)), tau(x) = x / sqrt(0.81 + x*x), over
                   the (2 max_distance + 1)^2 offsets;  dist = sum_k e / (0.1 + e), e = (t_k(img1) - t_k(Yw))^2;  mask' = mask inside
                   the frame shrunk by max_distance, else 0;  then photo_loss_function's four branches:
                     charbonnier, use_occ:   mean((dist^2 + 1e-6)^q * mask') / (mean(mask') * 2 + 1e-6)   (sums with average=False)
                     charbonnier:            mean((dist^2 + 1e-8)^q)  - no mask, the border included        (sum with average=False)
                     abs_robust, use_occ:    sum((|dist| + 0.01)^q * mask') / (2 sum(mask') + 1e-6)        (whatever average says)
                     abs_robust:             mean((|dist| + 0.01)^q)                                         (sum with average=False)

`flow` is a (B,2,H,W), `img1` / `img2` are (B,C,H,W) with any C >= 1 and `mask` is a (B,1,H,W) float32 CUDA tensor (None with use_occ:
a mask of ones).  The losses are float64 and differentiable with respect to the flows alone; the backward is the same entry point
asked for the gradient, with the upstream gradient read from device memory - nothing is saved between the passes but the inputs, and
nothing synchronises with the host.  No atomics: losses and gradients are bitwise reproducible.  CUDA tensors only: there is no CPU
path.
"""
import ctypes

import torch

from . import _lib

MAX_JOBS_PER_CALL = 16
KINDS = {"abs_robust": 0, "charbonnier": 1, "L1": 2, "census": 3}
MAX_DISTANCES = (1, 2, 3)
GRAY_RGB = (0.2989, 0.5870, 0.1140)


def default_gray(channels):
    """The intensity weights census uses when none are given: the reference's at C == 3, else 1/C per channel."""
    return GRAY_RGB if channels == 3 else (1.0 / channels,) * channels


def _settings(name, kind, use_occ, q, charbonnier, average, max_distance):
    if kind not in KINDS:
        raise ValueError(f"{name}: kind is one of {sorted(KINDS)} (the reference's SSIM is a term of its own: eemflow_amd.ssim_loss), got {kind!r}")
    if kind == "census" and max_distance not in MAX_DISTANCES:
        raise ValueError(f"{name}: max_distance is 1, 2 or 3, got {max_distance!r}")
    return KINDS[kind], bool(use_occ), float(q), bool(charbonnier), bool(average), int(max_distance) if kind == "census" else 0


def _check(name, what, t, planes=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: {what} is a tensor")
    if not t.is_cuda:
        raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if t.dim() != 4 or (planes is not None and t.shape[1] != planes) or t.dtype != torch.float32:
        shape = f"(B,{planes},H,W)" if planes else "(B,C,H,W)"
        raise ValueError(f"{name}: {what} is a {shape} float32 tensor, got {tuple(t.shape)} {t.dtype}")


def _launch(flows, job, want_loss, coef):
    """One eemflow_photo_many call per 16 jobs on the current stream: ((N,) float64 losses or None, list of gradients or None).
    flows and the job's tensors are contiguous and detached; coef: None (the loss alone) or a (N,) float64 device tensor."""
    img1, img2, masks, gray, settings = job
    kind, use_occ, q, charbonnier, average, r = settings
    n = len(flows)
    b, _, h, w = flows[0].shape
    c = int(img1[0].shape[1])
    dev = flows[0].device
    lib = _lib.lib()
    loss = torch.empty(n, device=dev, dtype=torch.float64) if want_loss else None
    grads = [torch.empty_like(f) for f in flows] if coef is not None else None
    scratch = torch.empty(max(1, int(lib.eemflow_photo_scratch_doubles(min(n, MAX_JOBS_PER_CALL), b, h, w))), device=dev, dtype=torch.float64)

    def ptrs(ts, i0, k):
        return (ctypes.c_void_p * k)(*[t.data_ptr() if t is not None else None for t in ts[i0:i0 + k]])
    with torch.cuda.device(dev):
        for i0 in range(0, n, MAX_JOBS_PER_CALL):
            k = min(MAX_JOBS_PER_CALL, n - i0)
            _lib.check(lib.eemflow_photo_many(
                k, ptrs(flows, i0, k), ptrs(img1, i0, k), ptrs(img2, i0, k), ptrs(masks, i0, k), b, c, h, w, kind, int(use_occ),
                int(charbonnier), int(average), r, q, gray.data_ptr() if gray is not None else None,
                coef[i0:].data_ptr() if coef is not None else None, loss[i0:].data_ptr() if want_loss else None,
                ptrs(grads, i0, k) if grads is not None else None, scratch.data_ptr(), _lib.current_stream_ptr(dev)))
    return loss, grads


class _Photo(torch.autograd.Function):
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


def photo_many(flows, img1, img2, mask=None, kind="census", use_occ=False, q=0.4, charbonnier=False, average=True, max_distance=3,
               gray=None):
    """Losses between img1 and img2 warped back by each of `flows` (a list of (B,2,H,W) float32 CUDA tensors of one shape): a (N,)
    float64 device tensor, differentiable with respect to every flow.  img1, img2 and mask are one tensor shared by all flows - img1
    is then grey-combined once per tile for census - or a list with one per flow (mask entries may be None).  q, charbonnier, average
    and max_distance (1..3) belong to 'census'; gray: its C intensity weights (None: default_gray(C)).  One library call per 16 flows
    forward and one backward, on the current stream; non-contiguous inputs are made contiguous."""
    name = "photo_many"
    settings = _settings(name, kind, use_occ, q, charbonnier, average, max_distance)
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
    r = settings[5]
    if kind == "census" and (shape[2] <= 2 * r or shape[3] <= 2 * r):
        raise ValueError(f"{name}: census with max_distance {r} needs H > {2 * r} and W > {2 * r}, got {shape[2]}x{shape[3]}")
    if gray is not None:
        gray = [float(g) for g in gray]
        if len(gray) != channels:
            raise ValueError(f"{name}: gray has one weight per channel; got {len(gray)} for C = {channels}")
        gray = torch.tensor(gray, dtype=torch.float64).to(dev, non_blocking=True) if kind == "census" else None
    made = {}                                                      # one contiguous tensor per distinct input: shared stays shared

    def cont(t):
        if t is None:
            return None
        if id(t) not in made:
            made[id(t)] = t.detach().contiguous()
        return made[id(t)]
    job = ([cont(t) for t in img1], [cont(t) for t in img2], [cont(t) for t in masks], gray, settings)
    return _Photo.apply(job, *[f.contiguous() for f in flows])


def photo_loss(flow, img1, img2, mask=None, **kw):
    """The one-flow form of photo_many: a 0-dim float64 device tensor."""
    return photo_many([flow], img1, img2, mask, **kw)[0]
