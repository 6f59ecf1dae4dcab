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
import math

from . import _dense, _lib
from ._dense import MAX_JOBS_PER_CALL  # noqa: F401


def _settings(name, use_occ, c1, c2, weight_epsilon):
    c1, c2, weight_epsilon = float(c1), float(c2), float(weight_epsilon)
    if not (c1 > 0.0 and c2 > 0.0):
        raise ValueError(f"{name}: c1 and c2 are positive (inf switches a term off), got c1={c1!r}, c2={c2!r}")
    if math.isinf(c1) and math.isinf(c2):
        raise ValueError(f"{name}: c1 and c2 are both infinite - the SSIM loss would be zero")
    if not (weight_epsilon > 0.0 and math.isfinite(weight_epsilon)):
        raise ValueError(f"{name}: weight_epsilon is positive and finite, got {weight_epsilon!r}")
    return bool(use_occ), c1, c2, weight_epsilon


def ssim_many(flows, img1, img2, mask=None, use_occ=False, c1=float("inf"), c2=9e-6, weight_epsilon=0.01):
    """Weighted SSIM losses between img1 and img2 warped back by each of `flows` (a list of (B,2,H,W) float32 CUDA tensors of one
    shape): a (N,) float64 device tensor, differentiable with respect to every flow.  img1, img2 and mask are one tensor shared by all
    flows or a list with one per flow (mask entries may be None: a weight of ones).  c1 / c2 regularise the luminance / structure term,
    inf switches one off; weight_epsilon regularises the division by the pooled weight.  One library call per 16 flows forward and one
    backward, on the current stream; non-contiguous inputs are made contiguous."""
    name = "ssim_many"
    settings = _settings(name, use_occ, c1, c2, weight_epsilon)
    flows, img1, img2, masks, channels = _dense.warp_inputs(name, flows, img1, img2, mask)
    h, w = flows[0].shape[2:]
    if h < 3 or w < 3:
        raise ValueError(f"{name}: the 3 x 3 windows need H >= 3 and W >= 3, got {h}x{w}")
    lib = _lib.lib()

    def call(k, f, i1, i2, m, b, h, w, *tail):
        use_occ, c1, c2, eps = settings
        return lib.eemflow_ssim_many(k, f, i1, i2, m, b, channels, h, w, int(use_occ), c1, c2, eps, *tail)
    return _dense.losses((call, lib.eemflow_ssim_scratch_doubles, _dense.contiguous(img1, img2, masks), True), flows)


def ssim_loss(flow, img1, img2, mask=None, **kw):
    """The one-flow form of ssim_many: a 0-dim float64 device tensor."""
    return ssim_many([flow], img1, img2, mask, **kw)[0]
