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
from . import _dense, _lib
from ._dense import MAX_JOBS_PER_CALL  # noqa: F401

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


def smoothness_many(preds, imgs=None, order=1, constant=1.0, weight_type="gauss", error_type="L1"):
    """Smoothness losses of the predictions `preds` (a list of (B,2,H,W) float32 CUDA tensors of one shape): a (N,) float64 device
    tensor, differentiable with respect to every prediction.  imgs: None (every weight is 1), one (B,C,H,W) tensor shared by all
    predictions - its weights are then computed once per tile, not once per prediction - or a list with a tensor or None per
    prediction.  One library call per 16 predictions forward and one backward, on the current stream; non-contiguous inputs are made
    contiguous."""
    name = "smoothness_many"
    settings = _settings(name, order, constant, weight_type, error_type)
    preds = _dense.leaves(name, "prediction", preds)
    imgs = _dense.per_job(name, "prediction", "img", imgs, preds, optional=True)
    channels = _dense.channels(name, "all imgs", imgs) or 1
    h, w = preds[0].shape[2:]
    if h <= settings[0] or w <= settings[0]:
        raise ValueError(f"{name}: order {settings[0]} needs H > {settings[0]} and W > {settings[0]}, got {h}x{w}")
    lib = _lib.lib()

    def call(k, p, im, b, h, w, *tail):
        order, constant, wt, et = settings
        return lib.eemflow_smoothness_many(k, p, im, b, channels, h, w, order, wt, et, constant, *tail)
    return _dense.losses((call, lib.eemflow_smoothness_scratch_doubles, _dense.contiguous(imgs), False), preds)


def smoothness_loss(pred, img=None, **kw):
    """The one-prediction form of smoothness_many: a 0-dim float64 device tensor."""
    return smoothness_many([pred], img, **kw)[0]
