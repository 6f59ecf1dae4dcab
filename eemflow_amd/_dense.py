"""What the dense loss terms share on the host (photo.py, ssim.py, smooth.py; their kernels share csrc/dense_loss.h): the input checks,
"one per job, or one shared by all", the launch of a term's *_many entry point per 16 jobs and the autograd function around it.

A term's job is the tuple (call, scratch_doubles, inputs, scratch_for_grad):
    call             call(k, leaves, *inputs, b, h, w, coef, loss, grad, scratch, stream) runs the term's entry point for k jobs - the
                     pointer arrays of the leaves and of every input list, then the five arguments every entry point ends with; the
                     term binds its channel count and scalar arguments
    scratch_doubles  the entry point's *_scratch_doubles
    inputs           the per-job lists of contiguous detached input tensors (entries may be None)
    scratch_for_grad whether the entry point wants scratch for a launch without the loss
"""
import ctypes

import torch

from . import _lib

MAX_JOBS_PER_CALL = 16


def check(name, what, t, planes=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: {what} is a tensor")
    if not t.is_cuda:
        raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if t.dim() != 4 or (planes is not None and t.shape[1] != planes) or t.dtype != torch.float32:
        shape = f"(B,{planes},H,W)" if planes else "(B,C,H,W)"
        raise ValueError(f"{name}: {what} is a {shape} float32 tensor, got {tuple(t.shape)} {t.dtype}")


def leaves(name, unit, ts):
    """The tensors a term is differentiated by, one per job (`unit`: 'flow', 'prediction'): (B,2,H,W) float32 CUDA tensors of one shape
    on one device, as a list."""
    ts = list(ts)
    if len(ts) < 1:
        raise ValueError(f"{name}: at least one {unit}")
    for t in ts:
        check(name, f"a {unit}", t, 2)
    if any(tuple(t.shape) != tuple(ts[0].shape) for t in ts):
        raise ValueError(f"{name}: all {unit}s share one (B,2,H,W) shape, got {[tuple(t.shape) for t in ts]}")
    if any(t.device != ts[0].device for t in ts):
        raise ValueError(f"{name}: all {unit}s live on one device")
    return ts


def per_job(name, unit, what, x, like, planes=None, optional=False):
    """One `what` per job, or one shared by all: the list, each entry a (B,planes,H,W) tensor that agrees with the leaves `like` in B, H,
    W and device (None entries pass with optional)."""
    xs = [x] * len(like) if x is None or torch.is_tensor(x) else list(x)
    if len(xs) != len(like):
        raise ValueError(f"{name}: one {what}{' (or None)' if optional else ''} per {unit}; got {len(xs)} for {len(like)} {unit}s")
    if not optional and any(t is None for t in xs):
        raise ValueError(f"{name}: {what} is required")
    shape = tuple(like[0].shape)
    for t in xs:
        if t is None:
            continue
        check(name, what, t, planes)
        if (t.shape[0],) + tuple(t.shape[2:]) != (shape[0],) + shape[2:]:
            raise ValueError(f"{name}: {what} {tuple(t.shape)} beside a {unit} {shape}: B, H and W must agree")
        if t.device != like[0].device:
            raise ValueError(f"{name}: {what} and the {unit}s live on one device")
    return xs


def channels(name, what, ts):
    """The one channel count C >= 1 of the tensors `ts` (None entries aside); None where there is no tensor."""
    counts = {int(t.shape[1]) for t in ts if t is not None}
    if len(counts) > 1 or any(c < 1 for c in counts):
        raise ValueError(f"{name}: {what} share one channel count C >= 1")
    return counts.pop() if counts else None


def warp_inputs(name, flows, img1, img2, mask):
    """The inputs of a warp term as (flows, img1, img2, masks, C): lists with one entry per flow; img1 and img2 (B,C,H,W), mask
    (B,1,H,W) or None."""
    flows = leaves(name, "flow", flows)
    img1, img2 = per_job(name, "flow", "img1", img1, flows), per_job(name, "flow", "img2", img2, flows)
    masks = per_job(name, "flow", "mask", mask, flows, planes=1, optional=True)
    return flows, img1, img2, masks, channels(name, "img1 and img2", img1 + img2)


def contiguous(*lists):
    """The lists with one contiguous detached tensor per distinct input: shared stays shared (the kernels read an input that
    consecutive jobs name once)."""
    made = {}

    def cont(t):
        if t is None:
            return None
        if id(t) not in made:
            made[id(t)] = t.detach().contiguous()
        return made[id(t)]
    return [[cont(t) for t in ts] for ts in lists]


def _launch(ts, job, want_loss, coef):
    """One call of the term's entry point per 16 jobs on the current stream: ((N,) float64 losses or None, list of gradients or None).
    ts: the leaves, contiguous and detached; coef: None (the loss alone) or a (N,) float64 device tensor (the gradients alone)."""
    call, scratch_doubles, inputs, scratch_for_grad = job
    n = len(ts)
    b, _, h, w = ts[0].shape
    dev = ts[0].device
    loss = torch.empty(n, device=dev, dtype=torch.float64) if want_loss else None
    grads = [torch.empty_like(t) for t in ts] if coef is not None else None
    scratch = None
    if want_loss or scratch_for_grad:
        scratch = torch.empty(max(1, int(scratch_doubles(min(n, MAX_JOBS_PER_CALL), b, h, w))), device=dev, dtype=torch.float64)

    def ptrs(xs, i0, k):
        return (ctypes.c_void_p * k)(*[x.data_ptr() if x is not None else None for x in xs[i0:i0 + k]])
    with torch.cuda.device(dev):
        for i0 in range(0, n, MAX_JOBS_PER_CALL):
            k = min(MAX_JOBS_PER_CALL, n - i0)
            _lib.check(call(k, ptrs(ts, i0, k), *[ptrs(xs, i0, k) for xs in inputs], b, h, w,
                            coef[i0:].data_ptr() if coef is not None else None, loss[i0:].data_ptr() if want_loss else None,
                            ptrs(grads, i0, k) if grads is not None else None, scratch.data_ptr() if scratch is not None else None,
                            _lib.current_stream_ptr(dev)))
    return loss, grads


class _Term(torch.autograd.Function):
    """(N,) losses of N leaves; backward: the same entry point asked for coef * dL/dleaf (nothing saved but the inputs)."""

    @staticmethod
    def forward(ctx, job, *ts):
        ts = [t.detach() for t in ts]
        ctx.job, ctx.ts = job, ts
        return _launch(ts, job, True, None)[0]

    @staticmethod
    def backward(ctx, gloss):
        coef = gloss.detach().to(torch.float64).contiguous()
        grads = _launch(ctx.ts, ctx.job, False, coef)[1]
        return (None,) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[1:]))


def losses(job, ts):
    """The (N,) float64 losses of the leaves `ts` under the term's job, differentiable with respect to every leaf."""
    return _Term.apply(job, *[t.contiguous() for t in ts])
