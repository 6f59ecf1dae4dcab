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
import torch

from . import _dense, _lib
from ._dense import MAX_JOBS_PER_CALL  # noqa: F401

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


def photo_many(flows, img1, img2, mask=None, kind="census", use_occ=False, q=0.4, charbonnier=False, average=True, max_distance=3,
               gray=None):
    """Losses between img1 and img2 warped back by each of `flows` (a list of (B,2,H,W) float32 CUDA tensors of one shape): a (N,)
    float64 device tensor, differentiable with respect to every flow.  img1, img2 and mask are one tensor shared by all flows - img1
    is then grey-combined once per tile for census - or a list with one per flow (mask entries may be None).  q, charbonnier, average
    and max_distance (1..3) belong to 'census'; gray: its C intensity weights (None: default_gray(C)).  One library call per 16 flows
    forward and one backward, on the current stream; non-contiguous inputs are made contiguous."""
    name = "photo_many"
    settings = _settings(name, kind, use_occ, q, charbonnier, average, max_distance)
    flows, img1, img2, masks, channels = _dense.warp_inputs(name, flows, img1, img2, mask)
    r = settings[5]
    h, w = flows[0].shape[2:]
    if kind == "census" and (h <= 2 * r or w <= 2 * r):
        raise ValueError(f"{name}: census with max_distance {r} needs H > {2 * r} and W > {2 * r}, got {h}x{w}")
    if gray is not None:
        gray = [float(g) for g in gray]
        if len(gray) != channels:
            raise ValueError(f"{name}: gray has one weight per channel; got {len(gray)} for C = {channels}")
        gray = torch.tensor(gray, dtype=torch.float64).to(flows[0].device, non_blocking=True) if kind == "census" else None
    lib = _lib.lib()

    def call(k, f, i1, i2, m, b, h, w, *tail):
        kind, use_occ, q, charbonnier, average, r = settings
        return lib.eemflow_photo_many(k, f, i1, i2, m, b, channels, h, w, kind, int(use_occ), int(charbonnier), int(average), r, q,
                                      gray.data_ptr() if gray is not None else None, *tail)
    return _dense.losses((call, lib.eemflow_photo_scratch_doubles, _dense.contiguous(img1, img2, masks), True), flows)


def photo_loss(flow, img1, img2, mask=None, **kw):
    """The one-flow form of photo_many: a 0-dim float64 device tensor."""
    return photo_many([flow], img1, img2, mask, **kw)[0]
