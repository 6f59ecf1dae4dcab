"""Edge-aware flow smoothness loss on the GPU: the regulariser beside the contrast term of ground-truth-free training.

The reference's Loss_tools.edge_aware_smoothness_order1 / _order2 and flow_smooth_delta (utils_luo/tools.py:3008-3110) as ONE
stream-ordered library call per 16 predictions, forward and backward (eemflow_amd/csrc/smooth.hip).  For s = order in {1, 2} and both
axes (axis 2 = rows, the reference's `x`; axis 3 = columns), in unfused fp64 on the fp32 inputs:

    d = p[i] - p[i+1]                               (order 1)        d = (p[i] - p[i+1]) - (p[i+1] - p[i+2])     (order 2)
    g_c = constant * (img_c[i] - img_c[i+s]),   w = exp(-mean_c f(g_c)),   f(g) = g * g ('gauss') or |g| ('exp');   w = 1 without img
    e(d) = |d| ('L1') or (|d| + 0.01) ** 0.4 ('abs_robust')
    L = mean over the B*2*(H-s)*W axis-2 terms of e(d) * w  +  mean over the B*2*H*(W-s) axis-3 terms

`pred` is a (B,2,H,W) float32 CUDA tensor, `img` a (B,C,H,W) float32 CUDA tensor with any C >= 1 (in training: the old event volume)
or None.  flow_smooth_delta(flow) is smoothness_loss(flow): order 1, 'L1', no img.  The losses are float64 and differentiable with
respect to the predictions (img receives no gradient); the backward is the same entry point asked for the gradient, with the upstream
gradient read from device memory - nothing is saved between the passes but the inputs, and nothing synchronises with the host.  Losses
and gradients are bitwise reproducible.  CUDA tensors only: there is no CPU path.
"""
import ctypes

import torch

from . import _lib

MAX_JOBS_PER_CALL = 16
WEIGHT_TYPES = {"gauss": 0, "exp": 1}
ERROR_TYPES = {"L1": 0, "abs_robust": 1}


def _settings(name, order, constant, weight_type, error_type):
    if order not in (1, 2):
        raise ValueError(f"{name}: order is 1 or 2, got {order!r}")
    if weight_type not in WEIGHT_TYPES:
        raise ValueError(f"{name}: weight_type is 'gauss' or 'exp', got {weight_type!r}")
    if error_type not in ERROR_TYPES:
        raise ValueError(f"{name}: error_type is 'L1' or 'abs_robust', got {error_type!r}")
    return int(order), float(constant), WEIGHT_TYPES[weight_type], ERROR_TYPES[error_type]


def _check(name, what, t, planes=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: {what} is a tensor")
    if not t.is_cuda:
        raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if t.dim() != 4 or (planes is not None and t.shape[1] != planes) or t.dtype != torch.float32:
        shape = "(B,2,H,W)" if planes == 2 else "(B,C,H,W)"
        raise ValueError(f"{name}: {what} is a {shape} float32 tensor, got {tuple(t.shape)} {t.dtype}")


def _launch(preds, imgs, settings, want_loss, coef):
    """One eemflow_smoothness_many call per 16 jobs on the current stream: ((N,) float64 losses or None, list of gradients or None).
    preds / imgs are contiguous and detached; coef: None (the loss alone) or a (N,) float64 device tensor (the gradients too)."""
    order, constant, wt, et = settings
    n = len(preds)
    b, _, h, w = preds[0].shape
    dev = preds[0].device
    c = next((int(im.shape[1]) for im in imgs if im is not None), 1)
    lib = _lib.lib()
    loss = torch.empty(n, device=dev, dtype=torch.float64) if want_loss else None
    grads = [torch.empty_like(p) for p in preds] if coef is not None else None
    scratch = None
    if want_loss:
        scratch = torch.empty(max(1, int(lib.eemflow_smoothness_scratch_doubles(min(n, MAX_JOBS_PER_CALL), b, h, w))), device=dev,
                              dtype=torch.float64)
    with torch.cuda.device(dev):
        for i0 in range(0, n, MAX_JOBS_PER_CALL):
            k = min(MAX_JOBS_PER_CALL, n - i0)
            ptr = ctypes.c_void_p * k
            _lib.check(lib.eemflow_smoothness_many(
                k, ptr(*[p.data_ptr() for p in preds[i0:i0 + k]]), ptr(*[im.data_ptr() if im is not None else None for im in imgs[i0:i0 + k]]),
                b, c, h, w, order, wt, et, constant, coef[i0:].data_ptr() if coef is not None else None,
                loss[i0:].data_ptr() if want_loss else None, ptr(*[g.data_ptr() for g in grads[i0:i0 + k]]) if grads is not None else None,
                scratch.data_ptr() if want_loss else None, _lib.current_stream_ptr(dev)))
    return loss, grads


class _Smoothness(torch.autograd.Function):
    """(N,) smoothness losses of N predictions; backward: the same entry point asked for coef * dL/dpred (nothing saved but the inputs)."""

    @staticmethod
    def forward(ctx, job, *preds):
        imgs, settings = job
        preds = [p.detach() for p in preds]
        ctx.job, ctx.preds = job, preds
        return _launch(preds, imgs, settings, True, None)[0]

    @staticmethod
    def backward(ctx, gloss):
        imgs, settings = ctx.job
        coef = gloss.detach().to(torch.float64).contiguous()
        grads = _launch(ctx.preds, imgs, settings, False, coef)[1]
        return (None,) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[1:]))


def smoothness_many(preds, imgs=None, order=1, constant=1.0, weight_type="gauss", error_type="L1"):
    """Smoothness losses of the predictions `preds` (a list of (B,2,H,W) float32 CUDA tensors of one shape): a (N,) float64 device
    tensor, differentiable with respect to every prediction.  imgs: None (every weight is 1), one (B,C,H,W) tensor shared by all
    predictions - its weights are then computed once per tile, not once per prediction - or a list with a tensor or None per
    prediction.  One library call per 16 predictions forward and one backward, on the current stream; non-contiguous inputs are made
    contiguous."""
    name = "smoothness_many"
    settings = _settings(name, order, constant, weight_type, error_type)
    preds = list(preds)
    if len(preds) < 1:
        raise ValueError(f"{name}: at least one prediction")
    for p in preds:
        _check(name, "a prediction", p, 2)
    shape, dev = tuple(preds[0].shape), preds[0].device
    if any(tuple(p.shape) != shape for p in preds):
        raise ValueError(f"{name}: all predictions share one (B,2,H,W) shape, got {[tuple(p.shape) for p in preds]}")
    if any(p.device != dev for p in preds):
        raise ValueError(f"{name}: predictions and images live on one device")
    if imgs is None or torch.is_tensor(imgs):
        imgs = [imgs] * len(preds)
    else:
        imgs = list(imgs)
        if len(imgs) != len(preds):
            raise ValueError(f"{name}: one img (or None) per prediction; got {len(imgs)} for {len(preds)} predictions")
    channels = None
    for im in imgs:
        if im is None:
            continue
        _check(name, "img", im)
        if (im.shape[0],) + tuple(im.shape[2:]) != (shape[0],) + shape[2:]:
            raise ValueError(f"{name}: img {tuple(im.shape)} beside a prediction {shape}: B, H and W must agree")
        if im.shape[1] < 1 or (channels is not None and im.shape[1] != channels):
            raise ValueError(f"{name}: all imgs share one channel count C >= 1")
        channels = int(im.shape[1])
        if im.device != dev:
            raise ValueError(f"{name}: predictions and images live on one device")
    if shape[2] <= settings[0] or shape[3] <= settings[0]:
        raise ValueError(f"{name}: order {settings[0]} needs H > {settings[0]} and W > {settings[0]}, got {shape[2]}x{shape[3]}")
    made = {}                                                      # one contiguous tensor per distinct img: shared stays shared

    def cont(im):
        if im is None:
            return None
        if id(im) not in made:
            made[id(im)] = im.detach().contiguous()
        return made[id(im)]
    imgs = [cont(im) for im in imgs]
    return _Smoothness.apply((imgs, settings), *[p.contiguous() for p in preds])


def smoothness_loss(pred, img=None, **kw):
    """The one-prediction form of smoothness_many: a 0-dim float64 device tensor."""
    return smoothness_many([pred], img, **kw)[0]
