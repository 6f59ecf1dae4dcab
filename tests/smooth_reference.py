"""CPU restatement of the edge-aware smoothness loss (eemflow_amd/csrc/smooth.hip, eemflow_amd.smooth) in the dtype of its inputs.

In float32 it follows the operation order of the reference's Loss_tools.edge_aware_smoothness_order1 / _order2 (utils_luo/tools.py:
3008-3090; tests/golden/smooth.npz holds the reference's own results), in float64 it is what the GPU is judged against.  For
s = order in {1, 2} and both axes (axis 2 = rows, axis 3 = columns):

    d = p[i] - p[i+1]   or   (p[i] - p[i+1]) - (p[i+1] - p[i+2])
    w = exp(-mean_c f(constant * (img_c[i] - img_c[i+s]))),  f(g) = g^2 ('gauss') or |g| ('exp');  no img: no weight
    e(d) = |d| ('L1') or (|d| + 0.01)^0.4 ('abs_robust');    L = mean(e(d2) * w2) + mean(e(d3) * w3)

`gradient` is the analytic dL/dpred: every term hands c_k * e'(d) * w / N_axis to the s + 1 cells it reads, c = (+1, -1) or
(+1, -2, +1), e' = sign(d) (sign(0) = 0) or 0.4 e(d) / (|d| + 0.01) sign(d); beside it the abs-sum of every cell's contributions,
the scale of the GPU gradient's bound.
"""
import torch

COEFS = {1: (1.0, -1.0), 2: (1.0, -2.0, 1.0)}
SETTINGS = [(o, w, e) for o in (1, 2) for w in ("gauss", "exp") for e in ("L1", "abs_robust")]


def _step(x, axis, stride):
    n = x.shape[axis]
    return x.narrow(axis, 0, n - stride) - x.narrow(axis, stride, n - stride)


def _error(d, error_type):
    if error_type == "L1":
        return d.abs()
    if error_type == "abs_robust":
        return (d.abs() + 0.01).pow(0.4)
    raise ValueError(error_type)


def axis_terms(pred, img, axis, order, constant, weight_type):
    """(d, w) of one axis: the differences (B,2,..) and the weights (B,1,..) or None."""
    d = _step(pred, axis, 1)
    if order == 2:
        d = _step(d, axis, 1)
    if img is None:
        return d, None
    g = constant * _step(img, axis, order)
    if weight_type == "gauss":
        f = g ** 2
    elif weight_type == "exp":
        f = g.abs()
    else:
        raise ValueError(weight_type)
    return d, torch.exp(-torch.mean(f, 1, keepdim=True))


def smoothness(pred, img=None, order=1, constant=1.0, weight_type="gauss", error_type="L1"):
    """The loss, a 0-dim tensor of pred's dtype (differentiable where pred requires grad)."""
    total = 0.0
    for axis in (2, 3):
        d, w = axis_terms(pred, img, axis, order, constant, weight_type)
        e = _error(d, error_type)
        total = total + torch.mean(e if w is None else e * w)
    return total


def term_count(shape, order):
    b, _, h, w = shape
    return b * 2 * (h - order) * w + b * 2 * h * (w - order)


def gradient(pred, img=None, order=1, constant=1.0, weight_type="gauss", error_type="L1", coef=1.0):
    """(coef * dL/dpred, abs-sum of every cell's contributions), both of pred's shape and dtype."""
    grad = torch.zeros_like(pred)
    asum = torch.zeros_like(pred)
    for axis in (2, 3):
        d, w = axis_terms(pred, img, axis, order, constant, weight_type)
        a = d.abs()
        if error_type == "L1":
            de = torch.sign(d)
        else:
            de = 0.4 * (a + 0.01).pow(0.4) / (a + 0.01) * torch.sign(d)
        q = (de if w is None else de * w) / d.numel()
        n = d.shape[axis]
        for k, ck in enumerate(COEFS[order]):
            grad.narrow(axis, k, n).add_(ck * q)
            asum.narrow(axis, k, n).add_((ck * q).abs())
    return coef * grad, abs(coef) * asum
