"""fp64 STAGE CHECKER for the EEMFlow inference path.  TEST INFRASTRUCTURE ONLY (never imported by eemflow_amd/).

Every stage the library exposes (eemflow_get_stage) is compared with an fp64 evaluation of THAT ONE stage on the GPU's own input
to it, and the error is measured in units of fp32 rounding of the stage's own sums:

    z = (got - ref) / (u * mag),   u = 2^-24,   mag = the same sum over absolute values (sum |w x| + |b| for a convolution)

so a correct fp32 kernel gives |z| of a few units whatever the layer's scale, and an error confined to one tile is seen at the
tile instead of being averaged away by the 32 x 32 pooling in front of the flow.  `check` asserts four statistics of z against a
form's `Limits`: max |z|, rms(z), |mean(z)| and the least-squares slope of (got - ref) against ref in units of u (a wrong divisor
or an off-by-rounding transform constant is a scale error: small per element, large in the slope).

The decoders' inner layers are not exposed: `check_decoder` holds the GPU's error on a decoder to a multiple of what the fp32 CPU
oracle's error is on the same input (both against fp64).
"""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import eemflow_oracle as O

U = 2.0 ** -24
LEAKY = float(np.float32(0.1))          # LeakyReLU(0.1) of an fp32 model: the slope is the float nearest 0.1
MAG_FLOOR = 1e-7                        # mag is floored at this fraction of its largest value (an all-zero window is not 0 / 0)


@dataclass(frozen=True)
class Limits:
    max_z: float        # max |z|
    rms_z: float        # sqrt(mean z^2)
    mean_z: float       # |mean z|
    slope_u: float      # |slope of (got - ref) on ref| / u
    slope_min_n: int = 0    # the slope is asserted on tensors of at least this many values (see BWD_SLOPE_MIN_N)


# One limit set per form family, calibrated on an MI355X (the measured worst cases are in tests/test_gpu_stage_fp64.py's docstring;
# the path is bitwise repeatable, so they are deterministic for the committed seeds): max|z| 2x and rms(z) 1.5x the worst value seen
# across all cases, |mean z| and the slope 2x, each rounded down to two digits (up for mean and slope).
LIMITS = {
    "enc1": Limits(9.9, 0.54, 0.15, 0.72),      # pconv1_1: conv_enc1.hip, the generic kernel, the fused and deferred forms
    "direct": Limits(20.0, 0.98, 0.22, 1.9),    # fp32 MFMA direct convolutions (stride 2, EEM_WINO=0, rconv)
    "bx3": Limits(14.0, 0.68, 0.15, 2.4),       # three-piece bf16 products (conv_bx3.hip)
    "wino2": Limits(8.9, 0.47, 0.04, 0.56),     # Winograd F(2x2,3x3)
    "wino4": Limits(430.0, 3.1, 0.18, 2.3),     # Winograd F(4x4,3x3): transform entries up to 8, the worst at C = 16 (K = 144)
    "pool": Limits(7.0, 1.2, 0.28, 0.5),        # average pooling (fused epilogue partial sums or the pooling kernel)
    "corr": Limits(7.6, 1.1, 0.07, 3.8),        # 53-tap local correlation
    "out_conv": Limits(4.9, 1.1, 0.34, 1.4),    # the 1x1 6 -> 2 output conv
    "upsample": Limits(99.0, 1.0, 0.27, 2.8),   # bilinear, align_corners=False
}
KAPPA_DEC = 6.4                                  # decoders: GPU error <= KAPPA_DEC x the fp32 CPU oracle's (rms and max); 2x the worst

# The training backward (tests/test_gpu_train_fp64.py; references below).  Calibrated by the same rule on an MI355X, but the weight and
# bias gradients meet in fp32 atomics whose order changes from run to run: the backward is NOT bitwise repeatable, so each family's
# worst value is taken over four runs of every case (the table is in that module's docstring).
# A backward adjoint of random-sign upstream gradients cancels (|ref| ~ mag / sqrt(K)), so on a tensor of a few values the slope is the
# ratio of two noises: it is asserted from 256 values on (every weight tensor; not the biases, nor g_coarse below a 16-cell grid).
BWD_SLOPE_MIN_N = 256
LIMITS.update({
    "wgrad_bx3": Limits(12.0, 1.4, 0.6, 2.4, BWD_SLOPE_MIN_N),       # wgrad_enc.hip, products as bf16 pieces (16- / 32-wide tiles)
    "wgrad_fp32": Limits(9.5, 1.0, 0.53, 1.7, BWD_SLOPE_MIN_N),      # wgrad_enc.hip, fp32 MFMA (EEM_NO_WGRAD_BX3=1; pconv1_1's 5-channel form)
    "wgrad_ring": Limits(9.2, 0.9, 0.36, 0.81, BWD_SLOPE_MIN_N),      # wgrad_ring.hip (stride-2 layers; EEM_WGRAD_RING=all and its block shapes)
    "wgrad_tail": Limits(26.0, 1.7, 1.4, 2.5, BWD_SLOPE_MIN_N),      # wgrad_tail.hip: every 3x3 tail conv in one launch
    "wgrad_batched": Limits(11.0, 1.3, 0.58, 0.26, BWD_SLOPE_MIN_N),   # train.hip's batched small / generic kernels and the bias-gradient kernel
    "dgrad_wino4": Limits(320.0, 5.4, 0.035, 1.8, BWD_SLOPE_MIN_N),    # stride-1 encoder data gradients on the forward's F(4x4) kernels, gated
    "dgrad_wino2": Limits(11.0, 0.69, 0.013, 0.16, BWD_SLOPE_MIN_N),     # ... F(2x2)
    "dgrad_direct": Limits(16.0, 1.0, 0.02, 1.3, BWD_SLOPE_MIN_N),    # ... the direct kernels (EEM_WINO=0)
    "dgrad_s2": Limits(15.0, 0.95, 0.0058, 0.063, BWD_SLOPE_MIN_N),        # dgrad_s2.hip: conv^T + pooling branch + gate
    "dgrad_gconv": Limits(11.0, 0.76, 0.0027, 0.031, BWD_SLOPE_MIN_N),     # gconv conv^T, then tr_pool_bwd (pooling branch + gate)
    "tail_dgrad": Limits(7.6, 1.1, 0.3, 0.58, BWD_SLOPE_MIN_N),      # tail_conv_kernel's data-gradient jobs (gated, grouped, shuffled)
    "pool_bwd": Limits(1.8, 0.45, 0.017, 0.0023, BWD_SLOPE_MIN_N),        # poolbwd4_kernel / poolbwd_kernel (g_f13)
    "corr_bwd": Limits(6.8, 1.0, 0.19, 0.34, BWD_SLOPE_MIN_N),        # corrbwd_kernel (+ rconv's data gradient in the first volume's half)
    "ups_bwd": Limits(1.0, 0.27, 0.035, 1.4, BWD_SLOPE_MIN_N),        # the two upsample-backward forms
})

LOG = []            # every check's statistics, in order: {"name", "form", "max_z", "rms_z", "mean_z", "slope_u", ...}


def _d(t):
    return torch.as_tensor(t).detach().cpu().double()


def leaky(x):
    return torch.where(x >= 0, x, LEAKY * x)


# ----------------------------------------------------------------------------------------------------------- stage references
def conv_ref(x, w, b, stride=1, groups=1, act=True, padding=1):
    """`convrelu` (EEMFlow.py:26-30; zero padding 1) in fp64: (ref, mag) with mag = conv(|x|, |w|) + |b|."""
    x, w = _d(x), _d(w)
    b = _d(b) if b is not None else None
    ref = F.conv2d(x, w, b, stride=stride, padding=padding, groups=groups)
    mag = F.conv2d(x.abs(), w.abs(), b.abs() if b is not None else None, stride=stride, padding=padding, groups=groups)
    return (leaky(ref) if act else ref), mag


def normalise_ref(v, record):
    """loader_utils.py:527-535 as the deferred form applies it: (v - mean) / sd on the non-zero voxels, from the record
    {mean, sd, scale, any} the voxelizer wrote (scale 0: mean subtracted only; any 0: nothing to do) - in fp64."""
    v = _d(v)
    mean, sd, scale, anyv = (float(r) for r in _d(record))
    if anyv == 0:
        return v
    out = v - mean
    if scale != 0:
        out = out / sd
    return torch.where(v != 0, out, v)


def first_layer_ref(events, pad, w, b, records=None):
    """pconv1_1 on the replicate-padded input (image_utils.py:129-140, EEMFlow.py:75,135): events [N, 5, H, W] as the caller
    handed them; `records` (one per image) selects the deferred-normalisation form, which normalises before the padding."""
    x = _d(events)
    if records is not None:
        x = torch.stack([normalise_ref(x[i], records[i]) for i in range(x.shape[0])])
    return conv_ref(O.replicate_pad(x, pad), w, b, stride=2)


def avg_pool_ref(f, k):
    f = _d(f)
    return F.avg_pool2d(f, k, k), F.avg_pool2d(f.abs(), k, k)


def corr53_ref(x, y):
    """(1/C) sum_c x y over the 53 taps, zero outside the image; mag = (1/C) sum_c |x y|."""
    x, y = _d(x), _d(y)
    return O.local_corr53(x, y), O.local_corr53(x.abs(), y.abs())


def out_conv_ref(x, w, b):
    return conv_ref(x, w, b, act=False, padding=0)


def upsample_ref(coarse, size):
    """Bilinear, align_corners=False.  mag = interpolated |coarse| + the term of the fp32 source coordinate: an error of u times a
    coordinate (up to the map's height / width) moves the sample along the map's slope between the two rows / columns it reads."""
    c = _d(coarse)
    h, w = c.shape[-2:]
    gy, gx = torch.zeros_like(c), torch.zeros_like(c)
    gy[..., :-1, :] = (c[..., 1:, :] - c[..., :-1, :]).abs()
    gx[..., :, :-1] = (c[..., :, 1:] - c[..., :, :-1]).abs()
    mag = O.upsample_flow(c.abs(), size) + h * O.upsample_flow(gy, size) + w * O.upsample_flow(gx, size)
    return O.upsample_flow(c, size), mag


# -------------------------------------------------------------------------------------------------------- backward references
# Each is the fp64 adjoint of one operation on the GPU's own tensors (input activation, stored output, upstream gradient), with mag the
# same adjoint of |upstream|, |weights| and |other operand| - for a linear adjoint exactly the sum of |terms|.
def gate(y):
    """LeakyReLU' from the GPU's own STORED output: 1 where it is > 0, LEAKY elsewhere (never from a recomputed fp64 pre-activation:
    a pixel at the kink is a rounding difference, not a fault)."""
    y = _d(y)
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, LEAKY))


def shuffle(x, groups):
    """EEMFlow.py:51-57 (channel j * groups + g <- g * per + j); shuffle(x, per) undoes shuffle(x, groups)."""
    return O.channel_shuffle(_d(x), groups)


def conv_dgrad_ref(dy, w, in_hw, stride=1, groups=1, padding=1, y_gate=None, x_gate=None):
    """d / d x of conv2d(x, w, stride, padding, groups) for upstream dy (gated by LeakyReLU' of the conv's stored output y_gate, if
    given), then gated by LeakyReLU' of x's own stored value x_gate (the encoder's pre-activation form)."""
    dy, w = _d(dy), _d(w)
    if y_gate is not None:
        dy = dy * gate(y_gate)
    size = (dy.shape[0], w.shape[1] * groups, *in_hw)
    ref = torch.nn.grad.conv2d_input(size, w, dy, stride=stride, padding=padding, groups=groups)
    mag = torch.nn.grad.conv2d_input(size, w.abs(), dy.abs(), stride=stride, padding=padding, groups=groups)
    if x_gate is not None:
        gx = gate(x_gate)
        ref, mag = ref * gx, mag * gx
    return ref, mag


def conv_wgrad_ref(x, dy, wshape, stride=1, groups=1, padding=1, y_gate=None):
    """(dW, |dW| terms, db, |db| terms) of conv2d(x, W, b) for upstream dy (gated by y_gate's LeakyReLU', if given)."""
    x, dy = _d(x), _d(dy)
    if y_gate is not None:
        dy = dy * gate(y_gate)
    dw = torch.nn.grad.conv2d_weight(x, wshape, dy, stride=stride, padding=padding, groups=groups)
    mw = torch.nn.grad.conv2d_weight(x.abs(), wshape, dy.abs(), stride=stride, padding=padding, groups=groups)
    return dw, mw, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


def pool_bwd_ref(dpool, hw, k):
    """Adjoint of avg_pool2d(k, stride k) on an h x w map (floor semantics): each pooled value / k^2 over its window; the rows and
    columns that no window covers (h % k, w % k) get nothing."""
    dp = _d(dpool)
    n, c, gh, gw = dp.shape
    out = torch.zeros(n, c, *hw, dtype=torch.float64)
    out[:, :, :gh * k, :gw * k] = dp.repeat_interleave(k, 2).repeat_interleave(k, 3) / (k * k)
    return out, out.abs()


def stage_dgrad_ref(dy, w, x, dpool, k):
    """Data gradient into a stride-2 layer's input x, which is also a stage output feeding the k x k pooling: (conv^T(dy, w) + the
    pooling branch) gated by LeakyReLU' of x - the gradient w.r.t. x's own pre-activation."""
    r, m = conv_dgrad_ref(dy, w, x.shape[-2:], stride=2)
    pr, pm = pool_bwd_ref(dpool, x.shape[-2:], k)
    gx = gate(x)
    return (r + pr) * gx, (m + pm) * gx


def _vjp(fn, args, upstream):
    args = [_d(a).clone().requires_grad_(True) for a in args]
    out = fn(*args)
    return torch.autograd.grad(out, args, _d(upstream))


def corr_bwd_ref(dcv, x, y):
    """Adjoint of the 53-tap correlation (zero outside the image) for both operands: ((dx, mag), (dy, mag))."""
    dx, dy = _vjp(O.local_corr53, (x, y), dcv)
    mx, my = _vjp(O.local_corr53, (_d(x).abs(), _d(y).abs()), _d(dcv).abs())
    return (dx, mx), (dy, my)


def upsample_bwd_ref(d, hw):
    """Adjoint of the bilinear upsample (align_corners=False) from an h x w map.  mag = the adjoint of |d| times (1 + h + w): besides
    the sums' rounding, an error of u times a source coordinate (up to the map's height / width) moves a bilinear weight."""
    (ref,) = _vjp(lambda c: O.upsample_flow(c, _d(d).shape[-2:]), (torch.zeros(*_d(d).shape[:2], *hw, dtype=torch.float64),), d)
    (m,) = _vjp(lambda c: O.upsample_flow(c, _d(d).shape[-2:]), (torch.zeros(*_d(d).shape[:2], *hw, dtype=torch.float64),), _d(d).abs())
    return ref, m * (1 + hw[0] + hw[1])


def loss_grad_ref(flow, gt, valid, weight=1.0):
    """sequence_loss's d / d flow (train_mvsec.py:201-227) exactly as fp32 computes it: sign(flow - gt) * valid / (B * 2 * H * W) with
    valid = (valid >= 0.5) & (|gt| < 400)."""
    f, g, v = (torch.as_tensor(t).detach().cpu().float() for t in (flow, gt, valid))
    b, _, h, w = f.shape
    ok = (v >= 0.5) & (torch.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) < 400.0)
    s = torch.tensor(weight, dtype=torch.float32) / (torch.tensor(float(b), dtype=torch.float32) * 2.0 * float(h * w))
    return torch.sign(f - g) * torch.where(ok, s, torch.zeros_like(s))[:, None]


# ----------------------------------------------------------------------------------------------------------------- the checks
class StageError(AssertionError):
    pass


def stats(got, ref, mag):
    """The four statistics of z = (got - ref) / (u mag) and the worst element's flat index."""
    g = _d(got)
    if g.shape != ref.shape:
        raise StageError(f"shape {tuple(g.shape)} against the reference's {tuple(ref.shape)}")
    d = g - ref
    floor = max(float(mag.max()) * MAG_FLOOR, 1e-300) if mag.numel() else 1.0
    z = d / (U * mag.clamp_min(floor))
    zf = z.reshape(-1)
    bad = ~torch.isfinite(zf)
    worst = int(torch.nonzero(bad)[0]) if bool(bad.any()) else int(zf.abs().argmax())
    rr = float((ref * ref).sum())
    return {"max_z": float(zf.abs().max()) if not bool(bad.any()) else float("inf"),
            "rms_z": float(zf.pow(2).mean().sqrt()),
            "mean_z": float(zf.mean()),
            "slope_u": float((d * ref).sum()) / rr / U if rr > 0 else 0.0,
            "worst": worst, "z": z, "n": zf.numel()}


def where(shape, flat, tile=None):
    """(image, channel, y, x) of a flat index into an NCHW tensor, with its tile in a (rows, cols) tiling."""
    idx = np.unravel_index(flat, tuple(shape))
    s = "(image %d, channel %d, y %d, x %d)" % tuple(int(i) for i in idx) if len(shape) == 4 else str(tuple(int(i) for i in idx))
    if tile is not None and len(shape) == 4:
        th, tw = tile
        y, x = int(idx[2]), int(idx[3])
        s += f", tile (row {y // th}, col {x // tw}) of {th}x{tw} at offset ({y % th}, {x % tw}); {shape[2]}x{shape[3]} map = " \
             f"{-(-shape[2] // th)}x{-(-shape[3] // tw)} tiles"
    return s


def check(name, got, ref, mag, limits, tile=None, form=None):
    """Assert the four statistics of z against `limits` (a Limits or a key of LIMITS); on failure name the worst element."""
    lim = LIMITS[limits] if isinstance(limits, str) else limits
    st = stats(got, ref, mag)
    rec = {"name": name, "form": form or (limits if isinstance(limits, str) else "?"),
           **{k: st[k] for k in ("max_z", "rms_z", "mean_z", "slope_u", "n")}}
    LOG.append(rec)
    fails = []
    if not st["max_z"] <= lim.max_z:
        fails.append(f"max|z| {st['max_z']:.3g} > {lim.max_z}")
    if not st["rms_z"] <= lim.rms_z:
        fails.append(f"rms(z) {st['rms_z']:.3g} > {lim.rms_z}")
    if not abs(st["mean_z"]) <= lim.mean_z:
        fails.append(f"|mean(z)| {abs(st['mean_z']):.3g} > {lim.mean_z}")
    if not abs(st["slope_u"]) <= lim.slope_u and st["n"] >= lim.slope_min_n:
        fails.append(f"|slope| {abs(st['slope_u']):.3g} u > {lim.slope_u} u")
    if fails:
        w = st["worst"]
        g, r, m = _d(got).reshape(-1)[w], ref.reshape(-1)[w], mag.reshape(-1)[w]
        raise StageError(f"{name} [{rec['form']}]: " + "; ".join(fails) +
                         f".  Worst element {where(ref.shape, w, tile)}: z {float(st['z'].reshape(-1)[w]):.4g}, got {float(g):.9g}, "
                         f"ref {float(r):.9g}, mag {float(m):.4g}  (max|z| {st['max_z']:.3g}, rms {st['rms_z']:.3g}, "
                         f"mean {st['mean_z']:.3g}, slope {st['slope_u']:.3g} u over {st['n']} values)")
    return rec


def decoder_refs(sd, k, x, groups=5):
    """Decoder k (EEMFlow.py:59-69) on the decoders' input x, in fp64 and in fp32 (the CPU oracle)."""
    pre = f"decoder_{k}."
    w = {key: v for key, v in sd.items() if key.startswith(pre)}
    ref64 = O.decoder({key: _d(v) for key, v in w.items()}, pre, _d(x), groups)
    ref32 = O.decoder({key: torch.as_tensor(v).detach().cpu().float() for key, v in w.items()}, pre,
                      torch.as_tensor(x).detach().cpu().float(), groups)
    return ref64, ref32


def check_decoder(name, got, ref64, ref32, kappa=None):
    """rms and max of the GPU's error <= kappa x those of the fp32 CPU oracle's error on the same input, plus an absolute floor
    of one unit of fp32 rounding at the largest output."""
    kappa = KAPPA_DEC if kappa is None else kappa
    eg = _d(got) - ref64
    ec = _d(ref32) - ref64
    floor = U * float(ref64.abs().max())
    rg, rc = float(eg.pow(2).mean().sqrt()), float(ec.pow(2).mean().sqrt())
    mg, mc = float(eg.abs().max()), float(ec.abs().max())
    rec = {"name": name, "form": "decoder", "rms_ratio": rg / max(rc, 1e-300), "max_ratio": mg / max(mc, 1e-300),
           "rms_gpu": rg, "rms_cpu": rc, "max_gpu": mg, "max_cpu": mc, "n": eg.numel()}
    LOG.append(rec)
    if not (rg <= kappa * rc + floor and mg <= kappa * mc + floor):
        w = int(eg.abs().reshape(-1).argmax())
        raise StageError(f"{name} [decoder]: GPU error rms {rg:.3g} / max {mg:.3g} against the fp32 CPU oracle's {rc:.3g} / {mc:.3g} "
                         f"(kappa {kappa}, floor {floor:.3g}); worst element {where(ref64.shape, w)}")
    return rec


# ------------------------------------------------------------------------------------- the operator-level ABI (eemop_conv2d_*)
# tests/test_gpu_ops_fp64.py and tests/test_fp64_bounds_ops.py: every kernel form behind eemop_conv2d_fwd / _bwd_data / _bwd_weight /
# _bwd_weight_cat, named by eemop_last_conv_form, against the references above.  What that ABI adds to them: non-square filters and
# paddings (conv_ref & co. take padding as a pair), channel-concatenated inputs, input-channel slices, out_scale and three epilogues.
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 4         # the ABI's `act` codes that are sums' roundings (sigmoid / tanh are left out: see the tests)


def op_conv_ref(xs, w, b, stride=1, padding=(1, 1), act=ACT_NONE, out_scale=1.0):
    """out_scale * act(conv2d(cat(xs, 1), w) + b) in fp64 with mag = |out_scale| (conv(|x|, |w|) + |b|): the pre-activation's mag for
    every epilogue (ReLU and LeakyReLU never enlarge an error of their argument)."""
    x = torch.cat([_d(t) for t in xs], 1)
    pre, mag = conv_ref(x, w, b, stride=stride, act=False, padding=tuple(padding))
    ref = {ACT_NONE: pre, ACT_RELU: pre.clamp_min(0.0), ACT_LEAKY: leaky(pre)}[act]
    s = float(np.float32(out_scale))
    return ref * s, mag * abs(s)


def op_dgrad_ref(dy, w, in_hw, stride=1, padding=(1, 1), ci0=0, cic=None):
    """dx of the input-channel slice [ci0, ci0 + cic) for dy w.r.t. the conv's pre-activation (this ABI's contract: the caller has
    applied the activation's gate, eemop_act_bwd, to dy already - from the stored output, as `gate` does)."""
    w = _d(w)
    cic = w.shape[1] - ci0 if cic is None else cic
    return conv_dgrad_ref(dy, w[:, ci0:ci0 + cic], in_hw, stride=stride, padding=tuple(padding))


def op_wgrad_ref(xs, dy, wshape, stride=1, padding=(1, 1), ci0=0):
    """(dW, mag, db, mag) of a conv over cat(xs, 1), as the columns [ci0, ci0 + sum c_s) of a zero dW of shape `wshape` (the ABI writes
    an input-channel slice into a wider dw; the other columns must stay what they were)."""
    x = torch.cat([_d(t) for t in xs], 1)
    cout, cin, kh, kw = wshape
    c = x.shape[1]
    dw, mw, db, mb = conv_wgrad_ref(x, dy, (cout, c, kh, kw), stride=stride, padding=tuple(padding))
    full, fmag = torch.zeros(*wshape, dtype=torch.float64), torch.zeros(*wshape, dtype=torch.float64)
    full[:, ci0:ci0 + c], fmag[:, ci0:ci0 + c] = dw, mw
    return full, fmag, db, mb


def seeded_conv(seed, cin, cout, k, stride=1, padding=None):
    """(w, b) of an nn.Conv2d with its default initialisation under `seed` (the global generator is left as it was); k = (kh, kw)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        conv = torch.nn.Conv2d(cin, cout, tuple(k), stride=stride, padding=tuple(padding) if padding is not None else (k[0] // 2, k[1] // 2))
    return conv.weight.detach().clone(), conv.bias.detach().clone()


def random_sign(shape, generator, scale=1.0):
    """Upstream gradients as the training fp64 tests make them: unit-normal magnitudes, so an adjoint's terms cancel like a real
    backward's (|ref| ~ mag / sqrt(K))."""
    return torch.randn(*shape, generator=generator) * scale


# Form name (eemop_last_conv_form) -> family of LIMITS, by the form's arithmetic; no limit is fitted to these kernels.  A stride-1 data
# gradient is a forward launch on transposed weights (ops.hip: plan_bwd) and reports - and is held to - the forward kernel's name and
# family.  A name joined with '+' (one weight-gradient launch per input segment) is looked up part by part.
def _form_families():
    t = {}
    for k in ("1x1", "3x3", "1x5", "5x1"):
        # fp32 MFMA, LDS-tiled: tile rows x (16-cout tiles per block) x K groups.  16 couts: 4-row tiles only; 32 couts: 2 or 4 rows, and
        # its 4-row form is chosen from 2048 blocks on - more than the 256 a second K group is given
        for th, wm in [(2, 4), (3, 4), (4, 4), (5, 4), (6, 4), (2, 2), (4, 2), (4, 1)]:
            for kg in (1, 2):
                if not ((th, wm) == (4, 2) and kg == 2):
                    t[f"gconv16_{k}_th{th}_wm{wm}_kg{kg}"] = "direct"
        for th in (2, 4, 6, 8):
            t[f"gconvb_{k}_th{th}"] = "bx3"                       # bf16 matrix pipe, operands as three exact pieces
    t.update({"gconv16_3x3_s2": "direct", "gconv16_1x1_s2": "direct"})
    # (conv_stem7.hip names its launches "stem7_c<cin>", but only eraft_forward hands it its packing: this ABI serves the stems on taps_7x7)
    t.update({"taps_7x7": "direct", "taps_3x3": "direct"})
    t.update({f"fewout_{v}": "direct" for v in ("wide2", "k16_c2", "k8_c2", "k8_c4", "k16_c8", "k8_c8")})     # vector-pipe FMA
    generic = ("generic_2x2_b1", "generic_2x2_b4", "generic_1x1_b1", "generic_1x1_b4", "generic_2x2", "generic_2x1", "generic_1x1",
               "generic_splitk4", "generic_splitk8", "generic_splitk16")
    t.update({g: "direct" for g in generic})
    return t


FORM_FAMILY = _form_families()
# the transposed generic form (tstride = 2: the data gradient of a stride-2 conv the parity kernel refuses) and the parity kernel
FORM_FAMILY.update({f"dgrad_t2_{g}": "dgrad_gconv" for g in FORM_FAMILY if g.startswith("generic_")})
FORM_FAMILY.update({f"dgrad_s2w_{c}_{k}": "dgrad_s2" for c in (96, 128) for k in ("3x3", "1x1")})
# weight gradients, by kernel
FORM_FAMILY.update({f"wgrad_ring_{v}": "wgrad_ring" for v in ("s2_6464", "s2_6432", "s2_3216", "6464", "3232", "1616", "wide_1x5",
                                                                "wide_5x1_6464", "wide_5x1_6432")})
# (the one-launch form of eemop_conv2d_bwd_weight_cat: every ring block shape over two or three input segments)
FORM_FAMILY.update({f"{f}_cat{n}": "wgrad_ring" for f in list(FORM_FAMILY) if f.startswith("wgrad_ring_") for n in (2, 3)})
FORM_FAMILY.update({f"wgrad_few_c{c}": "wgrad_batched" for c in (2, 4, 8)})
for _c_ in (16, 32, 64):
    for _s_ in (1, 2):
        for _tw_ in (16, 32):
            FORM_FAMILY[f"wgrad_enc_fp32_tw{_tw_}_c{_c_}_s{_s_}"] = "wgrad_fp32"
            if _c_ > 16:                                                # (one 16-cout tile per wave stays on the fp32 MFMA)
                FORM_FAMILY[f"wgrad_enc_bx3_tw{_tw_}_c{_c_}_s{_s_}"] = "wgrad_bx3"
FORM_FAMILY["wgrad_enc_fp32_tw32_c5_c16_s2"] = "wgrad_fp32"           # (<= 5 input channels: EEMFlow's first layer)
for _k_ in ("3x3", "1x5", "5x1", "1x1"):
    for _tw_ in (16, 32):
        FORM_FAMILY[f"wgrad_wide_bx3_tw{_tw_}_{_k_}"] = "wgrad_bx3"
        FORM_FAMILY[f"wgrad_wide_fp32_tw{_tw_}_{_k_}"] = "wgrad_fp32"
for _k_ in ("3x3_s1", "3x3_s2", "1x1_s1", "1x1_s2", "1x5_s1", "5x1_s1", "7x7_s1", "7x7_s2"):
    FORM_FAMILY[f"wgrad_generic_{_k_}"] = "wgrad_batched"             # train.hip's batched kernel ...
    FORM_FAMILY[f"wgrad_generic_{_k_}_bias"] = "wgrad_batched"        # ... and the bias-gradient kernel behind it
# Forms held to check_decoder's criterion (KAPPA_DEC x the error of torch's fp32 CPU evaluation of the same operation on the same inputs,
# plus one unit of fp32 rounding) in place of a family's SLOPE, each with its reason; max|z|, rms(z) and |mean z| stay the family's
# (FORM_KAPPA_FAMILY: only the statistic the reason is about is waived).
_T2_SPLIT = ("the dispatch gives it launches of at most %d tiles of 32 pixels x 32 channels (at most %d values) of sums of >= %d terms that "
             "cancel: there the slope is the ratio of two noises - torch's own fp32 data gradient of the case reads %s u against dgrad_gconv's "
             "0.031 u, its max|z|, rms and mean inside the family.  The arithmetic is the transposed generic kernel's, which "
             "dgrad_t2_generic_splitk4 holds to dgrad_gconv at launches of a million values")
FORM_KAPPA = {
    "dgrad_t2_generic_splitk8": _T2_SPLIT % (160, 163840, 256, "0.040"),
    "dgrad_t2_generic_splitk16": _T2_SPLIT % (64, 65536, 512, "0.091"),
}
FORM_KAPPA_FAMILY = {_f_: FORM_FAMILY.pop(_f_) for _f_ in FORM_KAPPA}


def form_family(name):
    """Family of a form name; the parts of a '+'-joined name must agree.  KeyError for the forms of FORM_KAPPA."""
    fams = {FORM_FAMILY[part] for part in name.split("+")}
    if len(fams) != 1:
        raise KeyError(f"{name}: segments of different families {sorted(fams)}")
    return fams.pop()


def check_form(name, form, got, ref, mag, tile=None, ref32=None):
    """`check` under the family of the form that ran; for a form of FORM_KAPPA `check_decoder` against ref32, (a function returning)
    torch's fp32 CPU evaluation of the same operation on the same inputs."""
    if form in FORM_KAPPA:
        if ref32 is None:
            raise StageError(f"{name} [{form}]: this form is held to the fp32 CPU evaluation's error, which the caller did not pass")
        fam = LIMITS[FORM_KAPPA_FAMILY[form]]
        check(name, got, ref, mag, Limits(fam.max_z, fam.rms_z, fam.mean_z, float("inf")), tile=tile, form=form)     # all but the slope
        rec = check_decoder(name, got, ref, ref32() if callable(ref32) else ref32)
        rec["form"] = form
        return rec
    return check(name, got, ref, mag, form_family(form), tile=tile, form=form)


# --------------------------------------------------------------------------------- E-RAFT inference, launch by launch (eraft_record_stages)
# tests/test_gpu_eraft_stage_fp64.py and tests/test_fp64_bounds_eraft.py: every launch of eraft_forward the stage recorder files, against
# an fp64 evaluation of that one launch on the GPU's own recorded input to it.  Three criteria, none fitted to the kernels under test:
#   1. launches that are plain sums (every convolution whose epilogue is none / ReLU / out_scale / a residual sum, all-pairs, pooling):
#      `check` under the family of the form that ran (FORM_FAMILY; the Winograd launches "f4" -> wino4, "wnc" -> wino2, "stem7_c<n>" and
#      the all-pairs forms -> direct, the pooling forms -> pool);
#   2. launches of a short, fixed number of operations: max|z| against the count of roundings (ER_ROUNDINGS, derived below);
#   3. launches that end in a nonlinear step (instance norm, sigmoid / tanh epilogues, GEPI_ZR, GEPI_GRU, convex upsampling):
#      `check_decoder` - rms and max error at most KAPPA_DEC x those of torch's fp32 CPU evaluation (oracle/eraft_oracle.py's functions)
#      of the same launch on the same input, plus one unit of fp32 rounding at the largest output.
from . import eraft_oracle as R       # noqa: E402

# (a table of its own: FORM_FAMILY is the operator-level ABI's, and tests/test_gpu_ops_fp64.py wants every name of it produced there)
ER_FORM_FAMILY = {"f4": "wino4", "wnc": "wino2", "pool2": "pool", "pool2x3": "pool",
                  "allpairs_lds": "direct", "allpairs_l2": "direct", "allpairs_odd": "direct", "altcorr": "direct"}
ER_FORM_FAMILY.update({f"stem7_c{_c_}": "direct" for _c_ in range(1, 6)})


def er_form_family(name):
    """Family of a form the E-RAFT stage recorder reports: its own launches' names, else a gconv form's (form_family)."""
    return ER_FORM_FAMILY[name] if name in ER_FORM_FAMILY else form_family(name)


def er_check_form(name, form, got, ref, mag, tile=None):
    """Criterion 1: `check` under the family of the form that ran."""
    return check(name, got, ref, mag, er_form_family(form), tile=tile, form=form)

# Criterion 2.  Every fp32 operation returns its exact result times (1 + d), |d| <= u = 2^-24; a result that passes through k roundings is
# off by at most ((1 + u)^k - 1) <= k u (1 + k u) times the sum of |terms| = k u mag (1 + 1e-6).  The counts:
#   pool    (a + b + c + d) * 0.25: three sums (the scale by a power of two is exact)                                         -> 3
#   lookup  v00 (1 - tx)(1 - ty) + v01 tx (1 - ty) + v10 (1 - tx) ty + v11 tx ty with tx, ty given: a term is at most two weight
#           roundings (1 - tx, 1 - ty) and two products, then three sums (a fused multiply-add only removes roundings)          -> 7
#   flow = coords1 - coords0, coords1 + delta, r * h: one operation                                                             -> 1
#   altcorr the lookup's blend (7) of window cells that are themselves C-term dot products: held to criterion 1 instead
ER_ROUNDINGS = {"pool": 3, "lookup": 7, "flow": 1, "sum": 1, "mul": 1}
ER_SLACK = 1.0 + 1e-5                  # (1 + k u)'s second-order term and the fp64 reference's own rounding


def _f32(t):
    return torch.as_tensor(t).detach().cpu().float()


def check_roundings(name, got, ref, mag, kind, form=None):
    """Criterion 2: max|z| <= the number of roundings of `kind` (ER_ROUNDINGS)."""
    k = ER_ROUNDINGS[kind]
    lim = Limits(k * ER_SLACK, float("inf"), float("inf"), float("inf"))
    return check(name, got, ref, mag, lim, form=form or kind)


def er_bn_fold(sd, prefix):
    """(scale, shift) of an eval BatchNorm2d `prefix` ("cnet.norm1.") in fp64: y = x * scale + shift."""
    w, b, rm, rv = (_d(sd[prefix + k]) for k in ("weight", "bias", "running_mean", "running_var"))
    s = w / torch.sqrt(rv + 1e-5)
    return s, b - rm * s


def er_conv_ref(xs, w, b, stride=1, padding=(1, 1), bn=None, pre=None, res=None, relu=False, out_scale=1.0):
    """The pre-activation of a conv launch of eraft_forward and its plain-sum epilogues, in fp64: v = conv(cat(xs), w) + b, then the
    eval BatchNorm `bn` = (scale, shift), then + `pre` (the context features' share of a GRU conv); relu; relu(. + res) (the residual
    blocks' tail); x out_scale.  mag is the sum of |terms| of everything in front of the (error-contracting) ReLUs."""
    v, mag = op_conv_ref(xs, w, b, stride=stride, padding=padding)
    if bn is not None:
        s, t = (p.view(1, -1, 1, 1) for p in bn)
        v, mag = v * s + t, mag * s.abs() + t.abs()
    if pre is not None:
        v, mag = v + _d(pre), mag + _d(pre).abs()
    if relu:
        v = v.clamp_min(0.0)
    if res is not None:
        v, mag = (v + _d(res)).clamp_min(0.0), mag + _d(res).abs()
    s = float(np.float32(out_scale))
    return v * s, mag * abs(s)


def er_conv_f32(xs, w, b, stride=1, padding=(1, 1), bn=None, pre=None):
    """torch's fp32 CPU evaluation of the same pre-activation (criterion 3's yardstick)."""
    v = F.conv2d(torch.cat([_f32(x) for x in xs], 1), _f32(w), _f32(b) if b is not None else None, stride=stride, padding=tuple(padding))
    if bn is not None:
        v = v * bn[0].float().view(1, -1, 1, 1) + bn[1].float().view(1, -1, 1, 1)
    return v + _f32(pre) if pre is not None else v


def er_instnorm_ref(x, relu_inner, res=None, dtype=torch.float64):
    """InstanceNorm2d(affine=False, eps=1e-5) per plane with the biased variance; relu_inner: relu(.); res: relu(. + res)
    (model/extractor.py:43-57).  dtype float32: oracle/eraft_oracle.py's F.instance_norm, the fp32 CPU yardstick."""
    if dtype == torch.float32:
        v = F.instance_norm(_f32(x), eps=1e-5)
    else:
        x = _d(x)
        m = x.mean((2, 3), keepdim=True)
        var = ((x - m) ** 2).mean((2, 3), keepdim=True)
        v = (x - m) / torch.sqrt(var + 1e-5)
    if relu_inner:
        v = torch.relu(v)
    if res is not None:
        v = torch.relu(v + torch.as_tensor(res).detach().cpu().to(dtype))
    return v


def er_allpairs_ref(f1, f2):
    """model/corr.py:53-60: out[b, p1, p2] = sum_c f1[b, c, p1] f2[b, c, p2] / sqrt(C) as [B * hw, 1, h, w]; the factor is inside mag."""
    f1, f2 = _d(f1), _d(f2)
    b, c, h, w = f1.shape
    a, bb = f1.reshape(b, c, h * w), f2.reshape(b, c, h * w)
    s = 1.0 / float(np.sqrt(np.float32(c)))
    ref = torch.einsum("bcp,bcq->bpq", a, bb) * s
    mag = torch.einsum("bcp,bcq->bpq", a.abs(), bb.abs()) * s
    return ref.reshape(b * h * w, 1, h, w), mag.reshape(b * h * w, 1, h, w)


def er_lookup_geometry(coords, level, size):
    """The sample positions of CorrBlock.__call__ at one pyramid level (model/corr.py:29-50 with model_utils.py:7-21), in fp32 exactly
    as oracle/eraft_oracle.py's corr_lookup / bilinear_sampler and grid_sample compute them - they are part of the model's definition:
    coords [B, 2, H, W] -> (x0, y0, tx, ty), each [B * H * W, 9, 9] (window index [i, j] = channel i * 9 + j: x + (i - 4), y + (j - 4))."""
    h, w = size
    c = _f32(coords).permute(0, 2, 3, 1)
    n = c.shape[0] * c.shape[1] * c.shape[2]
    r = 4
    d = torch.linspace(-r, r, 2 * r + 1)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)
    pos = c.reshape(n, 1, 1, 2) / 2 ** level + delta.view(1, 9, 9, 2)
    xg, yg = pos[..., 0], pos[..., 1]
    xg = 2 * xg / (w - 1) - 1                                           # bilinear_sampler's normalisation ...
    yg = 2 * yg / (h - 1) - 1
    ix = ((xg + 1) / 2) * (w - 1)                                       # ... and grid_sample's own way back (align_corners=True)
    iy = ((yg + 1) / 2) * (h - 1)
    fx, fy = torch.floor(ix), torch.floor(iy)
    return fx.long(), fy.long(), ix - fx, iy - fy


def er_lookup_ref(pyr, coords, levels=(0, 1, 2, 3)):
    """The correlation lookup against the GPU's own pyramid: positions, floor and the two weights in fp32 (er_lookup_geometry), only
    the four-term blend in fp64; a corner outside the map is zero.  pyr[l]: [B * H * W, 1, h_l, w_l] -> (ref, mag), [B, 81 * len(levels), H, W]."""
    b, _, hh, ww = coords.shape
    refs, mags = [], []
    for l in levels:
        img = _d(pyr[l])[:, 0]
        n, h, w = img.shape
        x0, y0, tx, ty = er_lookup_geometry(coords, l, (h, w))
        tx, ty = tx.double(), ty.double()
        idx = torch.arange(n).view(n, 1, 1)
        ref = torch.zeros(n, 9, 9, dtype=torch.float64)
        mag = torch.zeros(n, 9, 9, dtype=torch.float64)
        for dy, dx, wgt in ((0, 0, (1 - tx) * (1 - ty)), (0, 1, tx * (1 - ty)), (1, 0, (1 - tx) * ty), (1, 1, tx * ty)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            v = torch.where(ok, img[idx, yy.clamp(0, h - 1), xx.clamp(0, w - 1)], torch.zeros((), dtype=torch.float64))
            ref += v * wgt
            mag += v.abs() * wgt.abs()
        refs.append(ref.view(b, hh, ww, 81).permute(0, 3, 1, 2))
        mags.append(mag.view(b, hh, ww, 81).permute(0, 3, 1, 2))
    return torch.cat(refs, 1), torch.cat(mags, 1)


def er_altcorr_ref(fmap1, f2_levels, coords):
    """The on-the-fly correlation: the lookup (er_lookup_ref) of the all-pairs volumes of fmap1 against fmap2 and its pooled levels,
    each volume in fp64 from the GPU's own feature maps.  mag: the blend of the volumes' mag."""
    b, c, h, w = fmap1.shape
    s = 1.0 / float(np.sqrt(np.float32(c)))
    a = _d(fmap1).reshape(b, c, h * w)
    vol, vmag = [], []
    for f2 in f2_levels:
        q = _d(f2)
        hl, wl = q.shape[-2:]
        q = q.reshape(b, c, hl * wl)
        vol.append((torch.einsum("bcp,bcq->bpq", a, q) * s).reshape(b * h * w, 1, hl, wl))
        vmag.append((torch.einsum("bcp,bcq->bpq", a.abs(), q.abs()) * s).reshape(b * h * w, 1, hl, wl))
    ref, _ = er_lookup_ref(vol, coords)
    mag, _ = er_lookup_ref(vmag, coords)
    return ref, mag


def er_gru_blend_ref(z, h, q):
    """(1 - z) h + z q (model/update.py:58)."""
    return (1 - z) * h + z * q


def er_convex_up_ref(flow, mask, pad, size, dtype=torch.float64):
    """ERAFT.upsample_flow (model/eraft.py:83-94) of `flow` [B, 2, h, w] with `mask` [B, 576, h, w], cropped by the padder's
    (left, right, top, bottom) to `size`: oracle/eraft_oracle.py's convex_upsample in `dtype`."""
    up = R.convex_upsample(torch.as_tensor(flow).detach().cpu().to(dtype), torch.as_tensor(mask).detach().cpu().to(dtype))
    return up[..., pad[2]:pad[2] + size[0], pad[0]:pad[0] + size[1]]


def er_pad_ref(x, pad):
    """F.pad(mode='replicate') by the padder's (left, right, top, bottom) (utils/image_utils.py:139-140): a copy, compared bitwise."""
    return F.pad(_f32(x), tuple(pad), mode="replicate")


def check_bitwise(name, got, ref):
    g, r = _f32(got), _f32(ref)
    if g.shape != r.shape:
        raise StageError(f"{name}: shape {tuple(g.shape)} against the reference's {tuple(r.shape)}")
    bad = g.view(torch.int32) != r.view(torch.int32)
    LOG.append({"name": name, "form": "bitwise", "n": g.numel(), "differ": int(bad.sum())})
    if bool(bad.any()):
        w = int(torch.nonzero(bad.reshape(-1))[0])
        raise StageError(f"{name} [bitwise]: {int(bad.sum())} of {g.numel()} values differ; the first at {where(r.shape, w)}: got "
                         f"{float(g.reshape(-1)[w]):.9g}, ref {float(r.reshape(-1)[w]):.9g}")


# --------------------------------------------------------------------------------- EEMFlow+ inference, launch by launch (eemplus_record_stages)
# tests/test_gpu_plus_stage_fp64.py and tests/test_fp64_bounds_plus.py: every launch of eemplus_forward / eemplus_level the stage recorder
# files, against an fp64 evaluation of that one launch on the GPU's own recorded input to it.  The three criteria of the E-RAFT section,
# none fitted to the kernels under test:
#   1. plain sums (every convolution whose epilogue is none / LeakyReLU / dec7's residual add, the 53-tap correlation, the pooling):
#      `check` under the family of the form that ran (PL_FORM_FAMILY);
#   2. the warps' four-term blend, the flow upsampling and the scalings: max|z| against a derived count of roundings (ER_ROUNDINGS);
#   3. launches that end in the sigmoid blend: `check_decoder` against torch's fp32 CPU evaluation of the same launch.
from . import eemflow_plus_oracle as P     # noqa: E402
import re                                  # noqa: E402

# Form -> family, by the form's arithmetic.  tail_conv_kernel / tail_conv_multi_kernel are fp32 16x16x4 MFMA sums with K split over the
# waves of a block - the direct family's class of arithmetic; conv_wnc.hip is Winograd F(2x2,3x3); the encoder forms as
# tests/test_gpu_stage_fp64.py holds them (conv_enc1.hip -> enc1, the F(2x2) kernel -> wino2, the direct MFMA kernels -> direct).
PL_FORM_FAMILY = {"wnc32": "wino2", "wnc64": "wino2", "wnc32_m16": "wino2", "wnc64_m16": "wino2",
                  "enc1": "enc1", "wino": "wino2", "enc2": "direct",
                  "corr_direct": "corr", "corr_tiled53": "corr", "pool2x3": "pool"}
PL_FORM_FAMILY.update({f"enc_c{_a_}_{_b_}_s{_s_}": "direct" for _a_, _b_, _s_ in ((5, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1))})
PL_FORM_FAMILY.update({f"tail_k1_g{_g_}": "direct" for _g_ in (2, 25)})
PL_FORM_FAMILY.update({f"tail_k3_g{_g_}": "direct" for _g_ in (5, 8, 16, 18, 25, 46)})
PL_FORM_FAMILY["tail_multi"] = "direct"
PL_FORM_FAMILY["enc_c5_16_s2"] = "enc1"      # (pconv1_1 on the generic kernel: the enc1 family holds the first layer on either kernel)
# the launches held to criteria 2 and 3 (plus_kernels.hip) and the copies: every name the recorder can report is in one of the tables
PL_OTHER_FORMS = {"warp", "upflow", "upflow_multi", "upflow_warp", "scale_flow", "blend", "warp_blend", "warp_blend_warp", "copy_channels",
                  "pad", "pad4", "pad4_pair"}
# the tile a form cuts the output map into (rows, cols), so that a failure names the tile
PL_TILE = {"wnc32": (4, 32), "wnc64": (4, 64), "wnc32_m16": (4, 32), "wnc64_m16": (4, 64), "corr_tiled53": (8, 16), "wino": (4, 32)}


def pl_base_form(name):
    """A tail form without its job count: "tail_k3_g25_j2" -> ("tail_k3_g25", 2); every other name -> (name, 1)."""
    m = re.fullmatch(r"(tail_\w+?)_j(\d+)", name)
    return (m.group(1), int(m.group(2))) if m else (name, 1)


def pl_form_family(name):
    """Family of a form the EEMFlow+ stage recorder reports: its own launches' names, else a gconv form's (form_family)."""
    base, _ = pl_base_form(name)
    return PL_FORM_FAMILY[base] if base in PL_FORM_FAMILY else form_family(base)


def pl_tile(form):
    base, _ = pl_base_form(form)
    if base in PL_TILE:
        return PL_TILE[base]
    m = re.fullmatch(r"gconv16_\dx\d_th(\d)_wm\d_kg\d", base)
    return (int(m.group(1)), 16) if m else None


def pl_check_form(name, form, got, ref, mag):
    """Criterion 1: `check` under the family of the form that ran, the failure naming the form's tile."""
    return check(name, got, ref, mag, pl_form_family(form), tile=pl_tile(form), form=form)


# Criterion 2, counted as ER_ROUNDINGS counts (every fp32 operation one factor (1 + d), |d| <= u; a fused multiply-add only removes one):
#   warp    ((v0 nw + v1 ne) + v2 sw) + v3 se with the four weights GIVEN (they and the mask are the model's definition, pl_warp_taps):
#           v0's term passes one product and three sums, the others fewer; the mask's factor 0 / 1 is exact                       -> 4
#   upflow  (1 - ly) ((1 - lx) s00 + lx s01) + ly ((1 - lx) s10 + lx s11) with lx, ly given: s00's term passes 1 - lx, a product, the
#           inner sum, 1 - ly (a rounding of its own factor), the outer product and the outer sum                                  -> 6
#   upflow_rate  the same times the fp32 rate factor ow / w (given: the reference multiplies by that float)                          -> 7
#   scale   flow * factor (scale_flow, the coarse flow's doubling inside upflow_warp): one product                                  -> 1
ER_ROUNDINGS.update({"warp": 4, "upflow": 6, "upflow_rate": 7, "scale": 1})


def pl_conv_ref(x, w, b, act=True, k=3, groups=1, res=None):
    """One convolution launch of the path in fp64: leaky(conv(x)) (act) or conv(x) [+ res: dec7's residual epilogue]; zero padding
    (k - 1) / 2.  groups > 1: the decoder's grouped layer WITH its channel shuffle - output j of group g lands at channel j * G + g
    (EEMFlow+.py:51-57).  mag: the pre-activation's sum of |terms| (+ |res|), in the output's channel order."""
    ref, mag = conv_ref(x, w, b, groups=groups, act=act, padding=(k - 1) // 2)
    if groups > 1:
        ref, mag = shuffle(ref, groups), shuffle(mag, groups)
    if res is not None:
        ref, mag = ref + _d(res), mag + _d(res).abs()
    return ref, mag


def pl_conv_f32(x, w, b, act=True, k=3, groups=1, res=None):
    """torch's fp32 CPU evaluation of the same launch (what the host tests feed the checks)."""
    y = F.conv2d(_f32(x), _f32(w), _f32(b), padding=(k - 1) // 2, groups=groups)
    if act:
        y = F.leaky_relu(y, 0.1)
    if groups > 1:
        y = O.channel_shuffle(y, groups)
    return y + _f32(res) if res is not None else y


PL_DE_OUT = (32, 32, 32, 16, 8)                 # the dense estimator's five convs: output channels ...
PL_DE_OFF = (88, 56, 24, 8, 0)                  # ... and where each lands in the 184-channel buffer [de4 | de3 | de2 | de1 | de0 | a1 | warp_a2]
PL_DENSE = 184


def pl_dense_input(a1, warp_a2, des):
    """The input of the dense estimator's conv len(des) (0..5): the buffer's slice [184 - din, 184) = [de_{i-1} .. de_0 | a1 | warp_a2]
    (cdc_utils.py:109-145: x = cat([conv_i(x), x]))."""
    return torch.cat([_f32(t) for t in list(des)[::-1] + [a1, warp_a2]], 1)


def pl_dense_buffer(a1, warp_a2, des):
    """The same stages laid out at their offsets in a zeroed 184-channel buffer (the host tests' emulation of the launch's bookkeeping)."""
    n, _, h, w = a1.shape
    buf = torch.zeros(n, PL_DENSE, h, w)
    buf[:, 120:152], buf[:, 152:184] = _f32(a1), _f32(warp_a2)
    for i, t in enumerate(des):
        buf[:, PL_DE_OFF[i]:PL_DE_OFF[i] + PL_DE_OUT[i]] = _f32(t)
    return buf


def pl_cat_input(corr, rconv, flow):
    """The decoder's 87-channel input [53 correlation taps | 32 rconv | 2 flow] (EEMFlow+.py:179,191)."""
    return torch.cat([_f32(corr), _f32(rconv), _f32(flow)], 1)


def _f32c(v):
    return torch.tensor(float(v), dtype=torch.float32)


def pl_warp_taps(flow, mode):
    """The four taps of a warp, in fp32 operation by operation as csrc/warp_px.h and ATen's CPU grid sampler form them - they and the
    mode-2 mask are the model's definition.  mode 0: align_corners=True (EEMFlow_cdc.warp); 1: align_corners=False (torch_warp); 2: the
    same + the `grid_sample(ones) >= 1` mask (WarpingLayer_no_div).  flow [B, 2, h, w] -> {"w": four fp32 weights (nw, ne, sw, se),
    "y", "x": the four corners' integer positions, "ok": inside the map, "mask": [B, h, w] bool}."""
    f = _f32(flow)
    b, _, h, w = f.shape
    px = torch.arange(w, dtype=torch.float32).view(1, 1, w).expand(b, h, w)
    py = torch.arange(h, dtype=torch.float32).view(1, h, 1).expand(b, h, w)
    vx, vy = px + f[:, 0], py + f[:, 1]
    xn = 2.0 * vx / _f32c(max(w - 1, 1)) - 1.0
    yn = 2.0 * vy / _f32c(max(h - 1, 1)) - 1.0
    if mode == 0:
        ix = (xn + 1.0) * (_f32c(w - 1) / 2.0)
        iy = (yn + 1.0) * (_f32c(h - 1) / 2.0)
    else:
        ix = (xn + 1.0) * (_f32c(w) / 2.0) - 0.5
        iy = (yn + 1.0) * (_f32c(h) / 2.0) - 0.5
    xw, yn0 = torch.floor(ix), torch.floor(iy)
    ww, wn = ix - xw, iy - yn0
    we, ws = 1.0 - ww, 1.0 - wn
    wts = (ws * we, ws * ww, wn * we, wn * ww)                          # nw, ne, sw, se
    x0 = xw.clamp(-2.0, float(w) + 1.0).long()
    y0 = yn0.clamp(-2.0, float(h) + 1.0).long()
    xs, ys = (x0, x0 + 1, x0, x0 + 1), (y0, y0, y0 + 1, y0 + 1)
    ok = tuple((ys[i] >= 0) & (ys[i] < h) & (xs[i] >= 0) & (xs[i] < w) for i in range(4))
    if mode == 2:
        o = [ok[i].float() * wts[i] for i in range(4)]
        mask = (((o[0] + o[1]) + o[2]) + o[3]) >= 1.0
    else:
        mask = torch.ones(b, h, w, dtype=torch.bool)
    assert all(t.dtype == torch.float32 for t in wts)
    return {"w": wts, "y": ys, "x": xs, "ok": ok, "mask": mask, "frac": (ww, wn)}


def pl_warp_ref(x, flow, mode):
    """A warp launch against fp64: the taps as given (pl_warp_taps), the blend ((v0 nw + v1 ne) + v2 sw) + v3 se in fp64, times the
    mask -> (ref, mag, mask); mag is the blend's sum of |terms| (NOT masked: a masked pixel must be exactly 0, see pl_check_warp)."""
    t = pl_warp_taps(flow, mode)
    xd = _d(x)
    b, c, h, w = xd.shape
    bi = torch.arange(b).view(b, 1, 1)
    ref = torch.zeros(b, c, h, w, dtype=torch.float64)
    mag = torch.zeros(b, c, h, w, dtype=torch.float64)
    for i in range(4):
        v = xd[bi, :, t["y"][i].clamp(0, h - 1), t["x"][i].clamp(0, w - 1)].permute(0, 3, 1, 2)      # [B, C, h, w]
        v = torch.where(t["ok"][i][:, None], v, torch.zeros((), dtype=torch.float64))
        wt = t["w"][i].double()[:, None]
        ref += v * wt
        mag += v.abs() * wt.abs()
    m = t["mask"][:, None]
    return ref * m, mag, t["mask"]


def pl_check_warp(name, got, x, flow, mode, form="warp"):
    """Criterion 2 for a warp launch: where the reference's mask is 0 the output is exactly 0 (so a GPU mask of 1 there shows unless
    the blend itself is 0); elsewhere max|z| <= 4 roundings of the blend (so a GPU mask of 0 there shows unless the blend is 0)."""
    ref, mag, mask = pl_warp_ref(x, flow, mode)
    g = _d(got)
    if g.shape != ref.shape:
        raise StageError(f"{name} [{form}]: shape {tuple(g.shape)} against the reference's {tuple(ref.shape)}")
    out = ~mask[:, None].expand_as(g)
    bad = out & (g != 0)
    if bool(bad.any()):
        wst = int(torch.nonzero(bad.reshape(-1))[0])
        raise StageError(f"{name} [{form}]: {int(bad.sum())} values are nonzero where the `grid_sample(ones) >= 1` mask is 0; the first at "
                         f"{where(g.shape, wst)}: {float(g.reshape(-1)[wst]):.9g}")
    return check_roundings(name, got, ref, mag, "warp", form=form)


def pl_mask_of(got):
    """The mask a mode-2 warp applied, read from its output on an input that is positive everywhere: a pixel is kept iff any channel is
    nonzero (four inside taps of positive values with weights that sum to 1 cannot give 0)."""
    return (_f32(got) != 0).any(1)


def pl_upflow_geometry(n_in, n_out):
    """Source index and weight of F.interpolate(bilinear, align_corners=True) along one axis, in fp32 as upflow_px and ATen's CPU
    kernel compute them: scale = (in - 1) / (out - 1), f = scale * i, i0 = int(f), l = f - i0 -> (i0, i1, l) with l fp32."""
    s = _f32c(n_in - 1) / _f32c(n_out - 1) if n_out > 1 else _f32c(0.0)
    f = s * torch.arange(n_out, dtype=torch.float32)
    i0 = f.long()
    i1 = i0 + (i0 < n_in - 1).long()
    return i0, i1, f - i0.float()


def pl_rate(out_hw, in_hw):
    """upsample2d_flow_as(if_rate=True)'s two factors as the fp32 numbers the multiplication uses: (su, sv) = (ow / w, oh / h)."""
    return float(_f32c(out_hw[1]) / _f32c(in_hw[1])), float(_f32c(out_hw[0]) / _f32c(in_hw[0]))


def pl_upflow_ref(coarse, out_hw, rate=True):
    """upsample2d_flow_as (cdc_utils.py:80-103): the bilinear sum in fp64 with lx, ly given (pl_upflow_geometry), channel 0 times ow / w
    and channel 1 times oh / h when `rate` -> (ref, mag)."""
    c = _d(coarse)
    h, w = c.shape[-2:]
    oh, ow = out_hw
    y0, y1, ly = pl_upflow_geometry(h, oh)
    x0, x1, lx = pl_upflow_geometry(w, ow)
    ly, lx = ly.double().view(-1, 1), lx.double().view(1, -1)

    def blend(t):
        r0 = t[..., y0, :]
        r1 = t[..., y1, :]
        a = (1 - lx) * r0[..., x0] + lx * r0[..., x1]
        bb = (1 - lx) * r1[..., x0] + lx * r1[..., x1]
        return (1 - ly) * a + ly * bb
    ref, mag = blend(c), blend(c.abs())
    if rate:
        su, sv = pl_rate(out_hw, (h, w))
        s = torch.tensor([su, sv], dtype=torch.float64).view(1, 2, 1, 1)
        ref, mag = ref * s, mag * s.abs()
    return ref, mag


def pl_scale_ref(flow, out_hw):
    """The in-place side effect of upsample2d_flow_as(if_rate=True) on its input (cdc_utils.py:85-86): channel 0 * ow / w, 1 * oh / h."""
    f = _d(flow)
    su, sv = pl_rate(out_hw, f.shape[-2:])
    s = torch.tensor([su, sv], dtype=torch.float64).view(1, 2, 1, 1)
    return f * s, (f * s).abs()


def pl_blend_ref(warped, flow_init, xout, dtype=torch.float64):
    """flow_up = warped (1 - sigmoid(m)) + flow_init sigmoid(m), m = xout[:, 2:3] (cdc_utils.py:163-173)."""
    t = lambda a: torch.as_tensor(a).detach().cpu().to(dtype)       # noqa: E731
    m = torch.sigmoid(t(xout)[:, 2:3])
    return t(warped) * (1 - m) + t(flow_init) * m


def pl_warp_blend_refs(flow_init, xout):
    """The fused launch's flow_up -> (fp64 reference: the mode-1 warp's taps as given, its blend and the sigmoid blend in fp64;
    torch's fp32 CPU evaluation: the oracle's torch_warp and the same expression)."""
    w64, _, _ = pl_warp_ref(flow_init, _f32(xout)[:, :2], 1)
    ref64 = pl_blend_ref(w64, flow_init, xout)
    fi, xo = _f32(flow_init), _f32(xout)
    ref32 = pl_blend_ref(P.torch_warp(fi, xo[:, :2]), fi, xo, torch.float32)
    return ref64, ref32


def pl_check_leaky(name, got, form=None):
    """Bitwise: every negative output of a LeakyReLU launch is fl(q * LEAKY) for some fp32 q - the activation of an fp32 pre-activation
    by the fp32 slope.  y = fl(q s) puts q within one ulp of fl(y / s) (s ~ 0.1: an ulp of y is at most 1 / 8 of q's), so seven
    candidates are tried.  Multiplying by s thins a binade to ~62 % of its values, so a slope that is not the float nearest 0.1 (0.1 in
    double is a relative 0.25 u off - beneath every family's limits) leaves values outside the image."""
    y = _f32(got).reshape(-1)
    y = y[(y < 0) & (y.abs() > 1e-30)]
    s = torch.tensor(LEAKY, dtype=torch.float32)
    q0 = y / s
    lo, hi = q0.clone(), q0.clone()
    hit = (q0 * s) == y
    ninf, pinf = torch.tensor(float("-inf")), torch.tensor(float("inf"))
    for _ in range(3):
        lo, hi = torch.nextafter(lo, ninf), torch.nextafter(hi, pinf)
        hit |= ((lo * s) == y) | ((hi * s) == y)
    LOG.append({"name": name, "form": "leaky", "n": int(y.numel()), "differ": int((~hit).sum())})
    if not bool(hit.all()):
        w = int(torch.nonzero(~hit)[0])
        raise StageError(f"{name} [{form or 'leaky'}]: {int((~hit).sum())} of {y.numel()} negative outputs are no fp32 value times the fp32 "
                         f"slope {LEAKY!r}; the first: {float(y[w]):.9g}")


# (map height, width, seed) of the direct warp checks of tests/test_gpu_plus_stage_fp64.py; tests/test_fp64_bounds_plus.py holds the tap
# reference to F.grid_sample on exactly these
PL_WARP_CASES = [(25, 37, 11), (6, 9, 12)]


def pl_position_is_plain(flow):
    """Where the sample position of modes 1 and 2, ix = (xn + 1) (w / 2) - 0.5, is the same fp32 number whether the product is rounded
    before the subtraction (csrc/warp_px.h, built without contraction) or not (a fused multiply-add: what torch's vectorised CPU grid
    sampler and its CUDA one compile to): [B, h, w] bool, both axes.  Mode 0's position has no such pair of operations."""
    f = _f32(flow)
    b, _, h, w = f.shape
    ok = torch.ones(b, h, w, dtype=torch.bool)
    for ch, n in ((0, w), (1, h)):
        p = torch.arange(n, dtype=torch.float32).view((1, 1, n) if ch == 0 else (1, n, 1)).expand(b, h, w)
        c1 = (2.0 * (p + f[:, ch]) / _f32c(max(n - 1, 1)) - 1.0) + 1.0
        plain = c1 * (_f32c(n) / 2.0) - 0.5
        fused = (c1.double() * (n / 2.0) - 0.5).float()
        ok &= plain == fused
    return ok


def pl_hostile_flows(h, w, seed, plain_only=True):
    """Flows [6, 2, h, w] for the direct warp checks (the flows a seeded network produces are small): image 0 exact integer
    displacements; 1 displacements of x.5; 2 every pixel sent just inside / outside a border of the map by 1e-3 - in the coordinates
    of mode 0 (x = px + fx against 0 and w - 1); 3 the same in the coordinates of modes 1 and 2 (ix = (px + fx) w / (w - 1) - 0.5
    against -1, 0, w - 1 and w); 4 far outside (1e4 and 1e9: the float -> int conversion) between small smooth flows; 5 random
    sub-pixel flows.  A pixel whose position depends on whether torch's build contracts the unnormalisation (pl_position_is_plain) is
    drawn again from its image's rule, so that the reference, warp_px.h and every build of F.grid_sample agree on all of them.  Both
    test modules build their warp inputs here: the host module's conditions hold for exactly what the GPU runs.  plain_only=False:
    the first draw as it is - on it a kernel that contracts the position's multiply-add differs from pl_warp_taps (and pl_warp_taps
    from a contracting torch build), so it is compared with pl_warp_taps alone."""
    g = torch.Generator().manual_seed(seed)
    px = torch.arange(w, dtype=torch.float32).view(1, w).expand(h, w)
    py = torch.arange(h, dtype=torch.float32).view(h, 1).expand(h, w)

    def pick(vals):
        return torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), (h, w), generator=g)]

    def eps():
        return torch.where(torch.rand(h, w, generator=g) < 0.5, -1e-3, 1e-3)

    def ints():
        return torch.randint(-3, 4, (2, h, w), generator=g).float()

    def border0():
        return torch.stack([pick([0.0, w - 1.0]) + eps() - px, pick([0.0, h - 1.0]) + eps() - py])

    def border1():
        tx, ty = pick([-1.0, 0.0, w - 1.0, float(w)]) + eps(), pick([-1.0, 0.0, h - 1.0, float(h)]) + eps()
        return torch.stack([(tx + 0.5) * ((w - 1) / w) - px, (ty + 0.5) * ((h - 1) / h) - py])

    def far():
        f = torch.randn(2, h, w, generator=g) * 0.3
        sel = torch.rand(h, w, generator=g)
        f[:, sel < 0.15] = 1e4
        f[:, (sel >= 0.15) & (sel < 0.3)] = -1e4
        f[0, (sel >= 0.3) & (sel < 0.4)] = 1e9
        f[1, (sel >= 0.4) & (sel < 0.5)] = -1e9
        return f
    rules = (ints, lambda: ints() + 0.5, border0, border1, far, lambda: torch.randn(2, h, w, generator=g) * 1.5)
    out = torch.stack([r() for r in rules]).float()
    if not plain_only:
        return out
    for _ in range(64):
        bad = ~pl_position_is_plain(out)
        if not bool(bad.any()):
            return out
        new = torch.stack([r() for r in rules]).float()
        out = torch.where(bad[:, None], new, out)
    raise AssertionError("pl_hostile_flows: no build-independent draw found")


# ------------------------------------------------------------- the non-convolution autograd kernels (ops.hip, bwd_ops.hip), call by call
# tests/test_gpu_opsbwd_fp64.py and tests/test_fp64_bounds_opsbwd.py: every case makes ONE ABI call on the test's own inputs (ReLU gates from
# the y passed in, the mode-2 warp mask from the GPU forward), asserts the form by eemop_last_op_form and holds each output to one of the
# three criteria above; no limit is fitted to these kernels.  Geometry (floor, the bilinear fractions, ac_taps' sy * Y) is the operators'
# definition and is taken in fp32 (er_lookup_geometry, pl_warp_taps, pl_upflow_geometry = ac_taps along one axis); all after it is fp64.
OB_FORMS = {"instnorm_bwd_t256", "instnorm_bwd_t1024", "lookup_bwd_rows", "lookup_bwd_scatter", "allpairs_bwd", "convex_up_bwd",
            "warp_bwd_m0", "warp_bwd_m1", "warp_bwd_m2", "resize_ac", "resize_ac_bwd_gather", "resize_ac_bwd_scatter", "pool2_bwd", "act_fwd",
            "act_bwd", "binary", "sum_n_v4", "sum_n_scalar", "gru_blend", "gru_blend_bwd", "copy_channels", "shuffle", "scale_flow"}
OB_FORMS |= {f"bn_{_k_}_{_t_}" for _k_ in ("train_fwd", "train_bwd", "eval_fwd", "eval_bwd") for _t_ in ("t256", "t1024")}

F64 = 2.0 ** -29        # one fp64 rounding in units of u: a statistic accumulated in double over n values adds n * F64 to a count
GACT_NONE, GACT_RELU, GACT_SIGMOID, GACT_TANH, GACT_LEAKY = 0, 1, 2, 3, 4

# Criterion 2's counts for these kernels, as ER_ROUNDINGS counts (every fp32 operation one factor (1 + d), |d| <= u, relative to the sum
# of |terms| = mag; a fused multiply-add only removes one; a product by 0, 1 or a power of two is exact):
#   gru_blend      (1 - z) h + z q: 1 - z, its product, the sum                                                                    -> 3
#   gru_dz         g (q - h): the difference, the product (mag |g| (|q| + |h|))                                                    -> 2
#   gru_dh         g (1 - z): the difference, the product                                                                          -> 2
#   gru_dq         g z                                                                                                             -> 1
#   act_bwd_gate   dy d scale with d in {0, 1} (ReLU, identity): the product by d is exact, the one by scale rounds                 -> 1
#   act_bwd_leaky  d in {1, 0.1f}: two products                                                                                    -> 2
#   act_bwd_sigmoid  d = v (1 - v): 1 - v, v (1 - v), dy d, scale (mag |dy| |v| (1 + |v|) |scale|)                                  -> 4
#   act_bwd_tanh   d = 1 - v v: v v, the difference, dy d, scale (mag |dy| (1 + v v) |scale|: the difference cancels near |v| = 1)    -> 4
#   resize_ac      the four-term blend with lx, ly given: "upflow"'s count                                                         -> 6
#   binary         a + b, a - b, a b, relu(a + b), alpha a: one operation                                                           -> 1
#   sum_n          count - 1 sums (passed by the caller)
#   bn_mean        (float) of the fp64 mean                                                              -> 1 + n F64
#   bn_running     (1 - m) r + m s: 1 - m, its product, the sum | (float) s, its product, the sum       -> 3 + n F64
#   bn_dbias       (float) of the fp64 sum of g                                                          -> 1 + n F64
#   bn_dweight     (float) of the fp64 sum of g xhat, xhat = (x - mean) rstd in fp32 with mean, rstd given: two per term + the conversion -> 3 + n F64
#   bn_eval_y      (x - mean) k + b with k = w / sqrtf(var + eps): sum, root, quotient, product, the difference, product, sum          -> 7
#   bn_eval_dweight  the same with rstd = 1 / sqrtf(var + eps) formed in fp32 (sum, root, quotient)       -> 6 + n F64
#   save_rstd is held to one conversion plus the fp64 statistic's own error carried through 1 / sqrt (ob_bn_train_fwd_ref's `extra`).
# Scatter / gather adjoints: an element that receives N contributions of k roundings each is held to k + N - 1 (N counted per element by
# the reference; the N - 1 sums in any order, atomics included).  k per contribution:
#   lookup_bwd_scatter  g ((1 - tx)(1 - ty)): two differences, two products                                                        -> 4
#   lookup_bwd_rows     wx (sum of v wy over the four candidate taps): 1 - ty, its product, three inner sums, 1 - tx, the outer product -> 7
#   warp_dx        (dout m) w with the four weights and the mask given: one product                                                 -> 1
#   resize_bwd_scatter  ((g (1 - ly)) (1 - lx)): two differences, two products                                                     -> 4
#   resize_bwd_gather   (g wy) wx with wy = (1 - ly) + ly on the last row (two roundings), wx alike                                  -> 6
#   pyr_pool       fine += 0.25 coarse: one sum per level, the coarser level's own error carried along: level 2 -> 1, 1 -> 2, 0 -> 3
#   convex_dflow   a term 8 w_k dout with w_k the kernel's own softmax: exponent difference (|l_k - max| roundings of the exponent = that
#                  many relative ones of exp), expf (2), the denominator (8 sums + its terms' 2 + sum w |l - max| <= 2 + 9 / e), the
#                  quotient, the product: 18 + |l_k - max| per term, weighted term by term by the reference (ob_convex_up_bwd_ref)
ER_ROUNDINGS.update({"gru_blend": 3, "gru_dz": 2, "gru_dh": 2, "gru_dq": 1, "act_bwd_gate": 1, "act_bwd_leaky": 2, "act_bwd_sigmoid": 4,
                     "act_bwd_tanh": 4, "resize_ac": 6, "binary": 1, "bn_mean": 1, "bn_running": 3, "bn_dbias": 1, "bn_dweight": 3,
                     "bn_eval_dweight": 6, "bn_eval_y": 7, "lookup_bwd_scatter": 4, "lookup_bwd_rows": 7, "warp_dx": 1, "resize_ac_bwd_scatter": 4,
                     "resize_ac_bwd_gather": 6, "pool2_fwd": 3, "warp_fwd": 4, "lookup_fwd": 7})
CONVEX_K = 18.0
TINY = 1e-37            # results beneath fp32's normal range are not rounded relatively


def bound_counted(mag, k, extra=None):
    """The absolute bound of criterion 2 per element: k u mag (k a number or a tensor) + extra."""
    b = torch.as_tensor(k, dtype=torch.float64) * U * mag * ER_SLACK + TINY
    return b + extra if extra is not None else b


def check_counted(name, got, ref, mag, k, form, extra=None):
    """Criterion 2 with a count per element: |got - ref| <= k u mag (+ extra, an absolute allowance per element) everywhere."""
    g = _d(got)
    if g.shape != ref.shape:
        raise StageError(f"{name} [{form}]: shape {tuple(g.shape)} against the reference's {tuple(ref.shape)}")
    d = (g - ref).abs()
    bound = bound_counted(mag, k, extra).expand_as(ref)
    bad = ~(d <= bound)
    pos = mag > 0
    z = torch.where(pos, d / (U * mag.clamp_min(1e-300)), torch.zeros_like(d))
    ratio = d / bound
    rec = {"name": name, "form": form, "max_z": float(z.max()) if z.numel() else 0.0, "rms_z": float(z.pow(2).mean().sqrt()) if z.numel() else 0.0,
           "mean_z": 0.0, "slope_u": 0.0, "n": d.numel(), "of_bound": float(ratio.max()) if ratio.numel() else 0.0,
           "k_max": float(torch.as_tensor(k, dtype=torch.float64).max())}
    LOG.append(rec)
    if bool(bad.any()):
        w = int(torch.nonzero(bad.reshape(-1))[0]) if bool(torch.isnan(d).any()) else int((ratio.reshape(-1)).argmax())
        raise StageError(f"{name} [{form}]: {int(bad.sum())} of {d.numel()} values are outside their counted bound; the worst at "
                         f"{where(ref.shape, w)}: got {float(g.reshape(-1)[w]):.9g}, ref {float(ref.reshape(-1)[w]):.9g}, |diff| "
                         f"{float(d.reshape(-1)[w]):.4g} against {float(bound.reshape(-1)[w]):.4g} (mag {float(mag.expand_as(ref).reshape(-1)[w]):.4g})")
    return rec


def check_adjoint(name, x, fx, g, ftg, bound_f, bound_ft, form):
    """|<F x, g> - <x, F^T g>| for the GPU's own F x and F^T g, accumulated in fp64, within the summed rounding bounds of both sides."""
    x, fx, g, ftg = _d(x), _d(fx), _d(g), _d(ftg)
    lhs, rhs = float((fx * g).sum()), float((x * ftg).sum())
    tol = float((g.abs() * bound_f).sum() + (x.abs() * bound_ft).sum())
    LOG.append({"name": name, "form": form + ":adjoint", "of_bound": abs(lhs - rhs) / max(tol, 1e-300), "n": x.numel()})
    if not abs(lhs - rhs) <= tol:
        raise StageError(f"{name} [{form}]: <F x, g> = {lhs!r} against <x, F^T g> = {rhs!r}: |difference| {abs(lhs - rhs):.4g} > {tol:.4g}")


def ulp32(v):
    """Spacing of fp32 at |v| (towards larger magnitudes), as fp64."""
    a = _f32(v).abs()
    return (torch.nextafter(a, torch.tensor(float("inf"))) - a).double()


# ---- elementwise
def ob_gru_blend_ref(z, h, q):
    z, h, q = _d(z), _d(h), _d(q)
    return (1 - z) * h + z * q, (1 - z).abs() * h.abs() + z.abs() * q.abs()


def ob_gru_blend_bwd_ref(g, z, h, q):
    """{dz, dh, dq: (ref, mag, kind)}."""
    g, z, h, q = _d(g), _d(z), _d(h), _d(q)
    return {"dz": (g * (q - h), g.abs() * (q.abs() + h.abs()), "gru_dz"), "dh": (g * (1 - z), g.abs() * (1 - z).abs(), "gru_dh"),
            "dq": (g * z, (g * z).abs(), "gru_dq")}


def ob_act_bwd_ref(dy, y, kind, scale):
    """scale * dy * act'(y) from the y passed in (ReLU / LeakyReLU: y > 0, so 0.0 and -0.0 are both closed) -> (ref, mag, kind of count)."""
    dy, v = _d(dy), _d(y)
    s = float(np.float32(scale))
    one = torch.ones_like(v)
    if kind == GACT_RELU:
        d, m, kk = (v > 0).double(), (v > 0).double(), "act_bwd_gate"
    elif kind == GACT_LEAKY:
        d = torch.where(v > 0, one, LEAKY * one)
        m, kk = d, "act_bwd_leaky"
    elif kind == GACT_SIGMOID:
        d, m, kk = v * (1 - v), v.abs() * (1 + v.abs()), "act_bwd_sigmoid"
    elif kind == GACT_TANH:
        d, m, kk = 1 - v * v, 1 + v * v, "act_bwd_tanh"
    else:
        d, m, kk = one, one, "act_bwd_gate"
    return dy * d * s, dy.abs() * m * abs(s), kk


def ob_binary_ref(kind, a, b, alpha):
    a = _d(a)
    if kind == 4:
        s = float(np.float32(alpha))
        return a * s, (a * s).abs()
    b = _d(b)
    ref = {0: a + b, 1: a - b, 2: a * b, 3: (a + b).clamp_min(0.0)}[kind]
    return ref, (a * b).abs() if kind == 2 else a.abs() + b.abs()


def ob_sum_ref(ts):
    """(ref, mag, count - 1 sums)."""
    ts = [_d(t) for t in ts]
    return sum(ts), sum(t.abs() for t in ts), len(ts) - 1


def ob_scale_flow_ref(x, su, sv):
    x = _d(x)
    s = torch.tensor([float(np.float32(su)), float(np.float32(sv))], dtype=torch.float64).view(1, 2, *([1] * (x.dim() - 2)))
    return x * s, (x * s).abs()


def ob_shuffle_ref(x, groups, inverse):
    """channel_shuffle (EEMFlow+.py:52-58) by the oracle's own reshape; its inverse is the shuffle by c / groups."""
    x = _f32(x)
    y = O.channel_shuffle(x.reshape(*x.shape[:2], -1, 1), x.shape[1] // groups if inverse else groups)
    return y.reshape(x.shape)


# ---- F.interpolate(bilinear, align_corners=True) and its adjoint
def ob_ac_taps(h, w, oh, ow):
    """ac_taps of ops.hip for every output row and column, in fp32: (y0, y1, ly), (x0, x1, lx)."""
    return pl_upflow_geometry(h, oh), pl_upflow_geometry(w, ow)


def ob_resize_ref(x, out_hw):
    return pl_upflow_ref(x, out_hw, rate=False)


def _ac_matrix(n_in, n_out):
    """[n_out, n_in] fp64 weights of one axis (l given in fp32) and the number of nonzero tap entries per cell."""
    i0, i1, l = pl_upflow_geometry(n_in, n_out)
    l = l.double()
    wm = torch.zeros(n_out, n_in, dtype=torch.float64)
    cm = torch.zeros(n_out, n_in, dtype=torch.float64)
    r = torch.arange(n_out)
    wm.index_put_((r, i0), 1 - l, accumulate=True)
    wm.index_put_((r, i1), l, accumulate=True)
    cm.index_put_((r, i0), (1 - l != 0).double(), accumulate=True)
    cm.index_put_((r, i1), (l != 0).double(), accumulate=True)
    return wm, cm


def ob_resize_bwd_ref(dout, in_hw):
    """Adjoint of the resize: (ref, mag, N) with N the number of (output, corner) contributions of nonzero weight per source pixel."""
    d = _d(dout)
    oh, ow = d.shape[-2:]
    wy, cy = _ac_matrix(in_hw[0], oh)
    wx, cx = _ac_matrix(in_hw[1], ow)
    ref = torch.einsum("Yy,...YX,Xx->...yx", wy, d, wx)
    mag = torch.einsum("Yy,...YX,Xx->...yx", wy, d.abs(), wx)
    n = cy.sum(0).view(-1, 1) * cx.sum(0).view(1, -1)
    return ref, mag, n.expand_as(ref)


# ---- norms
def _gate(dy, y, relu):
    return dy * (y > 0).to(dy.dtype) if relu else dy


def ob_instnorm_bwd_ref(x, y, dy, relu, dtype=torch.float64):
    """InstanceNorm2d(affine=False, eps=1e-5) [+ ReLU] backward on [planes, hw]: dx = rstd (g - mean g - xhat mean(g xhat)), g = dy [y > 0],
    the statistics (biased variance) recomputed from x.  dtype float32: the same expression evaluated by torch in fp32 on the CPU."""
    x, y, dy = (torch.as_tensor(t).detach().cpu().to(dtype) for t in (x, y, dy))
    m = x.mean(1, keepdim=True)
    var = ((x - m) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    g = _gate(dy, y, relu)
    xh = (x - m) * rstd
    return rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))


def _bn_view(p, dtype):
    return torch.as_tensor(p).detach().cpu().to(dtype).view(1, -1, 1)


def ob_bn_train_fwd_ref(x, w, b, rm, rv, momentum, eps, relu):
    """BatchNorm2d in training mode on x [n, c, hw]: {"y": fp64, "y32": torch's fp32 CPU evaluation of the same expression, and the
    counted outputs save_mean / save_rstd / running_mean / running_var: (ref, mag, k, extra)}.  One value per channel (n * hw = 1) keeps
    the biased variance for the running one, as the kernel documents."""
    xd = _d(x)
    n, c, hw = xd.shape
    cnt = n * hw
    mom, eps = float(np.float32(momentum)), float(np.float32(eps))
    mean = xd.mean((0, 2))
    var = ((xd - mean.view(1, -1, 1)) ** 2).mean((0, 2))
    rstd = 1.0 / torch.sqrt(var + eps)
    mabs = xd.abs().mean((0, 2))
    mvar = (xd * xd).mean((0, 2)) + mabs * mabs                       # the terms of E x^2 - (E x)^2
    ub = cnt / (cnt - 1.0) if cnt > 1 else 1.0
    y = (xd - mean.view(1, -1, 1)) * rstd.view(1, -1, 1) * _bn_view(w, torch.float64) + _bn_view(b, torch.float64)
    x32 = _f32(x)
    m32 = x32.mean((0, 2), keepdim=True)
    v32 = ((x32 - m32) ** 2).mean((0, 2), keepdim=True)
    y32 = (x32 - m32) * (1.0 / torch.sqrt(v32 + eps)) * _bn_view(w, torch.float32) + _bn_view(b, torch.float32)
    if relu:
        y, y32 = y.clamp_min(0.0), y32.clamp_min(0.0)
    nf = (cnt + 4) * F64
    rstd_extra = 0.5 * rstd * ((cnt + 4) * 2.0 ** -53 * mvar) / (var + eps)
    return {"y": y, "y32": y32,
            "save_mean": (mean, mabs, ER_ROUNDINGS["bn_mean"] + nf, None),
            "save_rstd": (rstd, rstd, 1.0, rstd_extra),
            "running_mean": ((1 - mom) * _d(rm) + mom * mean, abs(1 - mom) * _d(rm).abs() + mom * mabs, ER_ROUNDINGS["bn_running"] + nf, None),
            "running_var": ((1 - mom) * _d(rv) + mom * var * ub, abs(1 - mom) * _d(rv).abs() + mom * mvar * ub, ER_ROUNDINGS["bn_running"] + nf, None)}


def _bn_bwd(x, y, dy, w, mean, rstd, relu, dtype, train):
    x, y, dy = (torch.as_tensor(t).detach().cpu().to(dtype) for t in (x, y, dy))
    w, mean, rstd = _bn_view(w, dtype), _bn_view(mean, dtype), _bn_view(rstd, dtype)
    g = _gate(dy, y, relu)
    xh = (x - mean) * rstd
    sg, sgx = g.sum((0, 2)), (g * xh).sum((0, 2))
    cnt = x.shape[0] * x.shape[2]
    dx = w * rstd * (g - sg.view(1, -1, 1) / cnt - xh * sgx.view(1, -1, 1) / cnt) if train else g * (w * rstd)
    return dx, sgx, sg, (g.abs() * xh.abs()).sum((0, 2)), g.abs().sum((0, 2))


def ob_bn_train_bwd_ref(x, y, dy, w, save_mean, save_rstd, relu):
    """{"dx", "dx32", "dweight": (ref, mag, k), "dbias": (ref, mag, k)} with the saved statistics as given."""
    dx, dw, db, mw, mb = _bn_bwd(x, y, dy, w, save_mean, save_rstd, relu, torch.float64, True)
    dx32 = _bn_bwd(x, y, dy, w, save_mean, save_rstd, relu, torch.float32, True)[0]
    nf = (x.shape[0] * x.shape[2] + 4) * F64
    return {"dx": dx, "dx32": dx32, "dweight": (dw, mw, ER_ROUNDINGS["bn_dweight"] + nf), "dbias": (db, mb, ER_ROUNDINGS["bn_dbias"] + nf)}


def ob_bn_eval_fwd_ref(x, w, b, rm, rv, eps, relu, dtype=torch.float64):
    x = torch.as_tensor(x).detach().cpu().to(dtype)
    k = _bn_view(w, dtype) * (1.0 / torch.sqrt(_bn_view(rv, dtype) + float(np.float32(eps))))
    y = (x - _bn_view(rm, dtype)) * k + _bn_view(b, dtype)
    return y.clamp_min(0.0) if relu else y


def ob_bn_eval_fwd_mag(x, w, b, rm, rv, eps):
    """The sum of |terms| of the eval BatchNorm's output (ReLU never enlarges an error of its argument)."""
    k = _bn_view(w, torch.float64) / torch.sqrt(_bn_view(rv, torch.float64) + float(np.float32(eps)))
    return (_d(x) - _bn_view(rm, torch.float64)).abs() * k.abs() + _bn_view(b, torch.float64).abs()


def ob_bn_eval_bwd_ref(x, y, dy, w, rm, rv, eps, relu):
    e = float(np.float32(eps))
    out = {}
    for key, dt in (("", torch.float64), ("32", torch.float32)):
        rstd = 1.0 / torch.sqrt(torch.as_tensor(rv).detach().cpu().to(dt) + e)
        r = _bn_bwd(x, y, dy, w, rm, rstd, relu, dt, False)
        out["dx" + key] = r[0]
        if dt == torch.float64:
            nf = (x.shape[0] * x.shape[2] + 4) * F64
            out["dweight"] = (r[1], r[3], ER_ROUNDINGS["bn_eval_dweight"] + nf)
            out["dbias"] = (r[2], r[4], ER_ROUNDINGS["bn_dbias"] + nf)
    return out


# ---- correlation lookup / pyramid
def ob_lookup_bwd_ref(coords, dout, rows):
    """Adjoint of the correlation lookup for dout [B, 324, H, W]: per level (ref, mag, N, allowance, cells) on [B * H * W, h_l, w_l].
    N: the taps' corners of nonzero weight that land in the cell.  rows: the allowance of lookup_bwd_rows_kernel - a row / column of
    its 11 x 11 window serves the taps jj in [r - 2, r + 1] of its offset r from the FIRST tap's corner, so a corner that rounding moved by
    more than one cell relative to the first tap's would not be found: such a corner may lose |dout| ulp32(|ix|) (|iy|) in its cell.
    `cells`: how many cells use it (none, on every input set of the tests: the round trip through the normalised position moves a floor
    by at most one cell); `lost_over_ulp`: the largest lost weight in units of that ulp."""
    b, _, hh, ww = coords.shape
    n = b * hh * ww
    d = _d(dout)
    out = []
    ph, pw = hh, ww
    for l in range(4):
        h, w = ph, pw
        x0, y0, tx, ty = er_lookup_geometry(coords, l, (h, w))
        ix, iy = x0.float() + tx, y0.float() + ty
        txd, tyd = tx.double(), ty.double()
        g = d[:, l * 81:(l + 1) * 81].permute(0, 2, 3, 1).reshape(n, 9, 9)
        ref, mag, cnt, allow = (torch.zeros(n * h * w, dtype=torch.float64) for _ in range(4))
        base = (torch.arange(n) * (h * w)).view(n, 1, 1)
        ii = torch.arange(9).view(1, 9, 1)
        jj = torch.arange(9).view(1, 1, 9)
        yb = y0[:, :1, :1].clamp(-16, h + 16)
        xb = x0[:, :1, :1].clamp(-16, w + 16)
        worst = 0.0
        for dy, dx, wy, wx in ((0, 0, 1 - tyd, 1 - txd), (0, 1, 1 - tyd, txd), (1, 0, tyd, 1 - txd), (1, 1, tyd, txd)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            at = (base + yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1))[ok]
            wgt = wy * wx
            ref.index_put_((at,), (g * wgt)[ok], accumulate=True)
            mag.index_put_((at,), (g.abs() * wgt)[ok], accumulate=True)
            cnt.index_put_((at,), (wgt != 0).double()[ok], accumulate=True)
            if rows:
                ry, rx = yy - yb - jj, xx - xb - ii
                off_y, off_x = yy - yb, xx - xb
                lost_y = ok & ~((ry >= -1) & (ry <= 2) & (off_y >= 0) & (off_y <= 10))
                lost_x = ok & ~((rx >= -1) & (rx <= 2) & (off_x >= 0) & (off_x <= 10))
                uy, ux = ulp32(iy), ulp32(ix)
                a = g.abs() * (lost_y.double() * uy + lost_x.double() * ux)
                allow.index_put_((at,), a[ok], accumulate=True)
                for lost, wl, u in ((lost_y, wy, uy), (lost_x, wx, ux)):
                    if bool(lost.any()):
                        worst = max(worst, float((wl / u)[lost].max()))
        out.append({"ref": ref.view(n, h, w), "mag": mag.view(n, h, w), "n": cnt.view(n, h, w), "allow": allow.view(n, h, w),
                    "cells": int((allow > 0).sum()), "lost_over_ulp": worst})
        ph, pw = ph // 2, pw // 2
    return out


def ob_lookup_bound(lv, form):
    """The absolute bound of a level's cells under `form`: (k + N - 1) u mag + the rows form's allowance."""
    k = ER_ROUNDINGS[form] + (lv["n"] - 1).clamp_min(0)
    return k, (lv["allow"] if form == "lookup_bwd_rows" else None)


def ob_allpairs_scale(c):
    """1 / sqrt(C) as the fp32 number the launch multiplies by."""
    return float(np.float32(1.0) / np.sqrt(np.float32(c)))


def ob_pyramid_fold_ref(dpyr):
    """The avg_pool2d chain's adjoint folded in place (model/corr.py:24-27): level l += 0.25 * repeat(level l + 1), from level 3 down:
    [(ref, mag, k)] for levels 0, 1, 2 (dpyr[l]: [planes, h_l, w_l])."""
    lv = [_d(p) for p in dpyr]
    ref, mag = lv[3], lv[3].abs()
    out = {}
    for l in (2, 1, 0):
        up, _ = pool_bwd_ref(ref[:, None], lv[l].shape[-2:], 2)
        um, _ = pool_bwd_ref(mag[:, None], lv[l].shape[-2:], 2)
        ref, mag = lv[l] + up[:, 0], lv[l].abs() + um[:, 0]
        out[l] = (ref, mag, 3 - l)
    return [out[0], out[1], out[2]]


def ob_allpairs_bwd_ref(fmap1, fmap2, dcorr, scale=None):
    """d fmap1[c, p1] = s sum_p2 dcorr[p1, p2] fmap2[c, p2], d fmap2[c, p2] = s sum_p1 dcorr[p1, p2] fmap1[c, p1] for dcorr [B * hw, h, w]
    (the folded level 0 the call left): ((ref, mag), (ref, mag)) as [B, C, h, w]."""
    f1, f2 = _d(fmap1), _d(fmap2)
    b, c, h, w = f1.shape
    hw = h * w
    s = ob_allpairs_scale(c) if scale is None else scale
    dc = _d(dcorr).reshape(b, hw, hw)
    a1, a2 = f1.reshape(b, c, hw), f2.reshape(b, c, hw)
    r1, m1 = torch.einsum("bpq,bcq->bcp", dc, a2) * s, torch.einsum("bpq,bcq->bcp", dc.abs(), a2.abs()) * s
    r2, m2 = torch.einsum("bpq,bcp->bcq", dc, a1) * s, torch.einsum("bpq,bcp->bcq", dc.abs(), a1.abs()) * s
    return (r1.reshape(b, c, h, w), m1.reshape(b, c, h, w)), (r2.reshape(b, c, h, w), m2.reshape(b, c, h, w))


# ---- convex upsampling
def _convex_fold(t, h, w):
    """Adjoint of the 3 x 3 unfold: t [B, C, 9, h, w] (neighbour k of centre (y, x)) summed onto the neighbour's own position."""
    out = torch.zeros(t.shape[0], t.shape[1], h, w, dtype=t.dtype)
    for k in range(9):
        dy, dx = k // 3 - 1, k % 3 - 1
        ys, ye, xs, xe = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        if ys < ye and xs < xe:
            out[:, :, ys + dy:ye + dy, xs + dx:xe + dx] += t[:, :, k, ys:ye, xs:xe]
    return out


def ob_convex_weights(mask):
    """softmax over the nine neighbours in fp64 and each weight's count of roundings: w, kt [B, 9, 8, 8, h, w]."""
    m = _d(mask)
    b, _, h, w = m.shape
    lg = m.view(b, 9, 8, 8, h, w)
    mx = lg.max(1, keepdim=True).values
    return torch.softmax(lg, 1), CONVEX_K + (lg - mx).abs()


def ob_convex_up_bwd_ref(flow, mask, dout):
    """ERAFT.upsample_flow's backward: {"dflow": (ref, bound), "dmask", "dmask32"}.  dflow's bound: every term 8 w_k dout at its own count
    (CONVEX_K + |l_k - max|) plus N - 1 sums, N = 64 per neighbour inside the map; dmask and dmask32 by autograd of the oracle's
    convex_upsample in fp64 and in fp32."""
    out = {}
    for key, dt in (("", torch.float64), ("32", torch.float32)):
        f = torch.as_tensor(flow).detach().cpu().to(dt).requires_grad_(True)
        m = torch.as_tensor(mask).detach().cpu().to(dt).requires_grad_(True)
        df, dm = torch.autograd.grad(R.convex_upsample(f, m), (f, m), torch.as_tensor(dout).detach().cpu().to(dt))
        out["dflow" + key], out["dmask" + key] = df, dm
    b, _, h, w = flow.shape
    wk, kt = ob_convex_weights(mask)
    d = _d(dout).view(b, 2, h, 8, w, 8).permute(0, 1, 3, 5, 2, 4)                     # [B, 2, sy, sx, h, w]
    term = 8.0 * wk[:, None] * d[:, :, None].abs()                                      # [B, 2, 9, sy, sx, h, w]
    mag = _convex_fold(term.sum((3, 4)), h, w)
    kw = _convex_fold((term * kt[:, None]).sum((3, 4)), h, w)
    n = _convex_fold(torch.full((b, 2, 9, h, w), 64.0, dtype=torch.float64), h, w)
    out["dflow"] = (out["dflow"], U * ER_SLACK * (kw + (n - 1) * mag) + TINY)
    return out


def ob_convex_up_fwd_bound(flow, mask):
    """The forward's own bound for the adjoint identity: a term 8 w_k flow_k at its count, the product and 8 sums."""
    b, _, h, w = flow.shape
    wk, kt = ob_convex_weights(mask)
    f = F.unfold(8.0 * _d(flow).abs(), (3, 3), padding=1).view(b, 2, 9, 1, 1, h, w)
    bd = (wk[:, None] * f * (kt[:, None] + 9.0)).sum(2)                                 # [B, 2, sy, sx, h, w]
    return U * ER_SLACK * bd.permute(0, 1, 4, 2, 5, 3).reshape(b, 2, 8 * h, 8 * w)


# ---- warp
def ob_warp_bwd_ref(x, flow, dout, mode, mask=None):
    """Adjoint of the warp with the taps (and, mode 2, the mask: pass the GPU forward's) given: {"dx": (ref, mag, N), "dflow": fp64 with
    the weights' fractions and d ix / d vx in fp32 as the kernel forms them}."""
    t = pl_warp_taps(flow, mode)
    xd, dd = _d(x), _d(dout)
    b, c, h, w = xd.shape
    m = (t["mask"] if mask is None else torch.as_tensor(mask).cpu().bool()).double()[:, None]
    g = dd * m
    bi = torch.arange(b).view(b, 1, 1)
    ref, mag, cnt = (torch.zeros(b, c, h * w, dtype=torch.float64) for _ in range(3))
    v = []
    for i in range(4):
        ok = t["ok"][i]
        at = (t["y"][i].clamp(0, h - 1) * w + t["x"][i].clamp(0, w - 1)).view(b, 1, h * w).expand(b, c, h * w)
        wt = (t["w"][i].double() * ok.double())[:, None]
        ref.scatter_add_(2, at, (g * wt).reshape(b, c, h * w))
        mag.scatter_add_(2, at, (g.abs() * wt).reshape(b, c, h * w))
        cnt.scatter_add_(2, at, (wt != 0).double().expand(b, c, h, w).reshape(b, c, h * w))
        vi = xd[bi, :, t["y"][i].clamp(0, h - 1), t["x"][i].clamp(0, w - 1)].permute(0, 3, 1, 2)
        v.append(torch.where(ok[:, None], vi, torch.zeros((), dtype=torch.float64)))
    ww, wn = (f.double()[:, None] for f in t["frac"])
    gix = (g * ((v[1] - v[0]) * (1 - wn) + (v[3] - v[2]) * wn)).sum(1)
    giy = (g * ((v[2] - v[0]) * (1 - ww) + (v[3] - v[1]) * ww)).sum(1)
    one = _f32c(1.0)
    if mode == 0:
        mx, my = (2.0 * one / _f32c(max(w - 1, 1))) * (_f32c(w - 1) / 2.0), (2.0 * one / _f32c(max(h - 1, 1))) * (_f32c(h - 1) / 2.0)
    else:
        mx, my = (2.0 * one / _f32c(max(w - 1, 1))) * (_f32c(w) / 2.0), (2.0 * one / _f32c(max(h - 1, 1))) * (_f32c(h) / 2.0)
    dflow = torch.stack([gix * float(mx), giy * float(my)], 1)
    return {"dx": (ref.view(b, c, h, w), mag.view(b, c, h, w), cnt.view(b, c, h, w)), "dflow": dflow}


# ---- the inputs of tests/test_gpu_opsbwd_fp64.py; tests/test_fp64_bounds_opsbwd.py holds its conditions on exactly these
OB_LOOKUP_SHAPES = [(16, 20), (17, 19)]
OB_PYRAMID_CASES = [(256, 16, 20), (40, 18, 18), (96, 10, 10), (16, 8, 8)]          # (c, h, w)
OB_CONVEX_SHAPES = [(5, 7), (1, 1), (1, 9)]
OB_CONVEX_KINDS = ("normal", "extreme", "equal")
OB_WARP_SHAPES = [(5, 17, 23), (1, 1, 9), (3, 9, 1)]                                # (c, h, w)
OB_RESIZE_CASES = [((3, 4), (37, 50)), ((6, 8), (48, 64)), ((5, 7), (5, 7)), ((9, 11), (4, 5)), ((1, 5), (8, 5)), ((4, 4), (1, 9)), ((2, 2), (3, 3))]
OB_INSTNORM_HW = [1, 63, 437, 16383, 16384, 16385]
OB_BN_CASES = [(3, 3, 357), (2, 3, 8192), (1, 2, 16384), (1, 2, 1)]                 # (n, c, hw)
OB_ELEMENTWISE_N = [1, 255, 256, 257, 1027]
# The rows form's allowance (ob_lookup_bwd_ref) may serve fewer than this fraction of a case's cells, and none of a case without near-integer
# coordinates.  Cells that use it: 16x20 hostile 0 of 271 360, 16x20 smooth 0, 17x19 hostile 0 of 268 090, 17x19 smooth 0 (the window of ten
# rows serving two taps each, which the kernel had, would have used it in 5204 and 3038 cells of the two hostile cases).
LOOKUP_ALLOWANCE_CAP = 0.01


def ob_seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode())


def ob_lookup_coords(h, w, kind, seed):
    """coords [2, 2, h, w] for the lookup adjoint.  "smooth": the pixel grid plus a smooth sub-pixel field (no coordinate near an integer
    at any level).  "hostile": per pixel and axis one of - an exact integer, an integer +- 1 ulp, +- 2^-12, a half-integer, -0.5 or
    size - 0.5, a position whose 9 x 9 window straddles a border of the map, +-1e4, +-1e9 (the kernels' clamps)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        f = [torch.stack([2.3 * torch.sin(0.31 * yy + 0.17 * xx + 0.4 + i) + 0.3137, 1.9 * torch.cos(0.23 * xx - 0.29 * yy + i) - 0.2871]) for i in range(2)]
        return (R.coords_grid(2, h, w) + torch.stack(f)).float()
    out = torch.empty(2, 2, h, w)
    inf = torch.tensor(float("inf"))
    for ax, size in ((0, w), (1, h)):
        n = torch.randint(-3, size + 4, (2, h, w), generator=g).float()
        sgn = torch.where(torch.rand(2, h, w, generator=g) < 0.5, -1.0, 1.0)
        lo = torch.rand(2, h, w, generator=g) < 0.5
        cand = [n, torch.nextafter(n, sgn * inf), n + sgn * 2.0 ** -12, n + 0.5, torch.where(lo, -0.5, size - 0.5),
                torch.where(lo, -5.0, size - 6.0) + 10.0 * torch.rand(2, h, w, generator=g), sgn * 1e4, sgn * 1e9]
        pick = torch.multinomial(torch.tensor([4.0, 4, 3, 3, 2, 3, 0.5, 0.5]), 2 * h * w, replacement=True, generator=g).view(2, h, w)
        out[:, ax] = torch.stack(cand).gather(0, pick[None])[0]
    return out


def ob_convex_inputs(h, w, kind, seed):
    """(flow [2, 2, h, w], mask logits [2, 576, h, w], dout [2, 2, 8h, 8w] zero outside a crop, as ConvexUpsample.backward produces)."""
    g = torch.Generator().manual_seed(seed)
    flow = torch.randn(2, 2, h, w, generator=g) * 3.0
    mask = torch.randn(2, 576, h, w, generator=g)
    if kind == "extreme":
        mask[:, 2 * 64:3 * 64] += 40.0
        mask[:, 6 * 64:7 * 64] -= 40.0
    elif kind == "equal":
        mask = torch.full_like(mask, 0.7)
    dout = torch.zeros(2, 2, 8 * h, 8 * w)
    dout[:, :, 3:8 * h - 2, 5:8 * w - 1] = torch.randn(2, 2, 8 * h - 5, 8 * w - 6, generator=g)
    return flow, mask, dout


def ob_warp_flows(h, w, seed):
    """pl_hostile_flows (integers, half-integers, landing on -1 / 0 / size - 1 / size in both conventions, far outside, random) with the
    far displacements at +-1e6 and +-1e9."""
    f = pl_hostile_flows(h, w, seed)
    return torch.where(f.abs() == 1e4, torch.sign(f) * 1e6, f)


def ob_norm_input(n, c, hw, seed, constant=True):
    """x [n, c, hw]: channel 0 ordinary, channel 1 constant (var = 0; `constant`), the last channel (when c > 2) with mean / std = 100.
    The BatchNorm cases take no constant channel: criterion 3 compares error norms over a channel, and a channel that holds one distinct
    value has one error sample on either side - the ratio of two single roundings (the instance-norm gradient of a constant plane is
    rstd (g - mean g), as many samples as pixels)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, hw, generator=g) * 2.0 + 0.5
    if constant:
        x[:, 1] = 1.25
    if c > 2:
        x[:, c - 1] = 100.0 + torch.randn(n, hw, generator=g)
    return x


def ob_gated_output(y, seed):
    """A stored layer output for the gates: relu(y) with exact 0.0 and -0.0 planted."""
    g = torch.Generator().manual_seed(seed)
    y = torch.relu(_f32(y)).clone()
    r = torch.rand(y.shape, generator=g)
    y[r < 0.05] = 0.0
    y[(r >= 0.05) & (r < 0.1)] = -0.0
    return y


# ---- the composite checks: what the GPU module asserts of a call's outputs, and the host module of torch's fp32 restatements
def ob_check_lookup(name, got_levels, coords, dout, form):
    """The four levels of a lookup adjoint; returns the reference's levels (bounds included) for the adjoint identity."""
    refs = ob_lookup_bwd_ref(coords, dout, rows=form == "lookup_bwd_rows")
    for l, lv in enumerate(refs):
        k, extra = ob_lookup_bound(lv, form)
        check_counted(f"{name}.l{l}", got_levels[l], lv["ref"], lv["mag"], k, form, extra)
        lv["bound"] = bound_counted(lv["mag"], k, extra)
    return refs


def ob_check_pyramid(name, got, fmap1, fmap2, dpyr):
    """eraft_corr_pyramid_bwd: got = {"dpyr": the three folded levels, "dfmap1", "dfmap2"}; the GEMMs against the folded level 0 the
    call itself left (its own check is the fold's)."""
    for l, (ref, mag, k) in enumerate(ob_pyramid_fold_ref(dpyr)):
        check_counted(f"{name}.fold{l}", got["dpyr"][l], ref, mag, k, "allpairs_bwd")
    (r1, m1), (r2, m2) = ob_allpairs_bwd_ref(fmap1, fmap2, got["dpyr"][0])
    check(f"{name}.dfmap1", got["dfmap1"], r1, m1, "direct", form="allpairs_bwd")
    check(f"{name}.dfmap2", got["dfmap2"], r2, m2, "direct", form="allpairs_bwd")


def ob_check_convex(name, dflow, dmask, flow, mask, dout):
    r = ob_convex_up_bwd_ref(flow, mask, dout)
    ref, bound = r["dflow"]
    check_counted(f"{name}.dflow", dflow, ref, bound / (U * ER_SLACK), 1.0, "convex_up_bwd")
    if dmask is not None:
        rec = check_decoder(f"{name}.dmask", dmask, r["dmask"], r["dmask32"])
        rec["form"] = "convex_up_bwd:kappa"
    return r


def ob_check_warp_bwd(name, dx, dflow, x, flow, dout, mode, mask):
    form = f"warp_bwd_m{mode}"
    r = ob_warp_bwd_ref(x, flow, dout, mode, mask)
    ref, mag, n = r["dx"]
    k = ER_ROUNDINGS["warp_dx"] + (n - 1).clamp_min(0)
    check_counted(f"{name}.dx", dx, ref, mag, k, form)
    if dflow is not None:
        rec = check_decoder(f"{name}.dflow", dflow, r["dflow"], ob_warp_dflow_f32(x, flow, dout, mode, mask))
        rec["form"] = form + ":kappa"
    r["dx_bound"] = bound_counted(mag, k)
    return r


def ob_check_resize_bwd(name, dx, dout, in_hw, form):
    ref, mag, n = ob_resize_bwd_ref(dout, in_hw)
    k = ER_ROUNDINGS[form] + (n - 1).clamp_min(0)
    check_counted(name, dx, ref, mag, k, form)
    return bound_counted(mag, k)


def ob_check_planes(name, got, ref64, ref32, form, dim):
    """check_decoder plane by plane (channel by channel) along `dim`: an ill-conditioned plane does not cover for the others."""
    for i in range(ref64.shape[dim]):
        rec = check_decoder(f"{name}[{i}]", _d(got).select(dim, i), ref64.select(dim, i), ref32.select(dim, i))
        rec["form"] = form + ":kappa"


def ob_check_counted_map(name, got, refs, form, keys):
    """The counted outputs of a norm reference: refs[key] = (ref, mag, k[, extra])."""
    for key in keys:
        ref, mag, k, *extra = refs[key]
        check_counted(f"{name}.{key}", got[key], ref, mag, k, form, extra[0] if extra else None)


def ob_warp_dflow_f32(x, flow, dout, mode, mask=None):
    """torch's fp32 CPU autograd of the oracle's warp w.r.t. the flow (mode 2: torch_warp times the given mask, which has no gradient)."""
    xf, do = _f32(x), _f32(dout)
    fl = _f32(flow).clone().requires_grad_(True)
    if mode == 0:
        out = P.warp_align_true(xf, fl)
    else:
        out = P.torch_warp(xf, fl)
        if mode == 2:
            out = out * torch.as_tensor(mask).cpu().float()[:, None]
    return torch.autograd.grad(out, fl, do)[0]


# ------------------------------------------------------------------------- the voxelizer (voxel.hip), launch form by launch form
# tests/test_gpu_vox_fp64.py and tests/test_fp64_bounds_vox.py: every case is ONE call of eemflow_voxelize / _many, asserts the sequence
# that ran by eemflow_voxelize_last_form and holds every output to a criterion that follows from the arithmetic, none fitted:
#   indices    vox_votes restates vox_vote (the reference's order of the f64 time scaling, truncating casts, polarity 0 -> -1, dts rounded
#              to fp32): the int64 index outputs are equal, -1 where the reference masks the vote.
#   raw grid, banded path   the band kernel adds a cell's votes in fp64 and rounds once.  vox_exact gives the fp64 sum of every occupied
#              cell and its error-free residual; residual 0: the cell equals the sum rounded to fp32, bit for bit; otherwise either fp32
#              neighbour of the sum, on at most VOX_RESIDUAL_SHARE of a case's occupied cells.  Unoccupied cells are +0.0.
#   raw grid, dyadic inputs  integer timestamps in [0, 2^20] with t0 = 0, t_last = 2^20: every vote is a multiple of 2^-20, every fp64 partial
#              sum is exact, every fp32 partial sum of fewer than VOX_DYADIC_DIRECT_CAP votes too (|sum| < 8 keeps 2^-20 within 24 bits):
#              banded AND direct path bitwise the exact sum, no exception.
#   raw grid, direct path    fp32 atomics in any order: check_counted with k = votes - 1 against sum |votes|.
#   record / moments         against fp64 moments of the GPU's OWN raw grid (vox_moment_bounds).  A band thread folds K cells into fp32
#              partial sums (sum and fma'd sum of squares) that are widened once and added in fp64; K = vox_plan's "K", 1 for the direct
#              path's fp64 vox_moments_kernel.  With u = 2^-24, c non-zero voxels, m the mean:
#                 dS = K u sum|v|            dQ = (K + 1) u sum v^2
#                 |mean err| <= dS / c + u |m|                      (the record's own rounding)
#                 |m2 err|   <= dQ + 2 |m| dS + dS^2 / c            (m2 = Q - S^2 / c)
#                 |sd err|   <= m2 err / (2 sd (c - 1)) + u sd
#              `any` and `scale` are exact: flags 1 / 0, sd = 1 where scale is 0 (c = 1: sd NaN; equal voxels: sd 0).
#   normalised grid          out = fl(fl(v - m') / sd') with m' = m + em, sd' = sd (1 + es), |em| <= dmean, |es| <= dsd / sd:
#                 out - (v - m) / sd = ref (d1 + d2 - es) - em / sd + second order, |d1|, |d2| <= u, so
#                 |err| <= |ref| (2 u + dsd / sd) + dmean / sd      (scale 0: u |v - m| + dmean), times ER_SLACK; zero voxels stay 0.
#              The norm pass, the two band passes and the fp32 expression applied on the host to the deferred record take the same
#              moments and the same expression (the file is built without contraction): bitwise equal (vox_normalise_f32).
VOX_RESIDUAL_SHARE = 1e-3
VOX_DYADIC_DIRECT_CAP = 8
VOX_T_DYADIC = 2 ** 20


def vox_plan(ns, bins, h, w, aligned=True, direct=False):
    """make_plan and the launch code of voxel.hip restated: None where the direct kernel runs, else band_px, nb, BT, vec4, sgs, EPT and
    K = the cells one band thread folds in fp32 in the read-out loop (bins x its share of band_px pixels, four at a time with vec4)."""
    ns = [int(ns)] if np.isscalar(ns) else [int(n) for n in ns]
    hw = h * w
    blocks = lambda n, e: (n + 1024 * e - 1) // (1024 * e)        # noqa: E731
    if direct or bins > 64 or hw >= 2 ** 31 or any(blocks(n, 8) > 4096 for n in ns):
        return None
    band_px = max((9216 // bins) & ~3, 64)
    spread = ((hw + 511) // 512 + 3) & ~3
    if band_px > spread:
        band_px = max(spread, 64)
    if (hw + band_px - 1) // band_px > 1023:
        band_px = ((hw + 1022) // 1023 + 3) & ~3
    if band_px * bins > 19200 or band_px > 65535:
        return None
    nb = (hw + band_px - 1) // band_px
    lds = band_px * bins * 8
    bt = 256 if lds <= 24 * 1024 else 512 if lds <= 40 * 1024 else 1024
    ept = 1
    while ept < 8 and blocks(max(ns), ept) > 512:
        ept *= 2
    vec4 = band_px % 4 == 0 and hw % 4 == 0 and aligned
    lanes_x10 = 40 if 1024 * ept < 4 * nb else 17
    sgs = 2
    while sgs < 6 and (1 << sgs) * 10 * nb < lanes_x10 * 1024 * ept:
        sgs += 1
    per = 4 * -(-band_px // (4 * bt)) if vec4 else -(-band_px // bt)
    return {"band_px": band_px, "nb": nb, "bt": bt, "vec4": vec4, "sgs": sgs, "ept": ept, "K": bins * per, "last_px": hw - (nb - 1) * band_px}


def vox_form(plan, njobs, normalize, twopass=False):
    """The string eemflow_voxelize_last_form gives for vox_plan's plan."""
    if plan is None:
        return "j1:direct" + ("", "+moments+norm", "+moments+stats")[normalize]
    band = f"band{plan['bt']}_{'v4' if plan['vec4'] else 'v1'}_s{plan['sgs']}"
    head = f"j{njobs}:bin_e{plan['ept']}+{band}"
    if normalize == 1 and twopass:
        return f"{head}_moments+{band}_normalised"
    return head + ("_raw", "_raw_sums+norm", "_raw_sums+stats")[normalize]


# sgs, log2 of the lanes that share a run, is the smallest s in 2..6 with 2^s 10 nb >= L 1024 EPT, L = 40 where 1024 EPT < 4 nb, else 17.
# s = 2 needs nb >= 1024 EPT (L = 40; nb <= 1023) or nb >= 436 EPT together with nb <= 256 EPT (L = 17): unreachable.  3 .. 6 are reached.
VOX_SGS_REACHABLE = (3, 4, 5, 6)


def vox_events(kind, seed, n, h, w, bins=5):
    """Time-sorted (n, 4) f64 events [t, x, y, p].
    clustered  70 % of the events in one 40 x 40 patch (one hot band, many votes per cell), as tests/test_gpu_parity.py's;
    hostile    clustered, with 12 % strays: x in [w, w + 4), y in [h, 3 h) and y in [-2 h, 0) (flat-index semantics: votes move by whole
               planes, the t2 == -1 branch, votes that leave the grid), the image's last pixel, and eight events at t_last;
    dyadic     integer timestamps in [0, 2^20], t0 = 0, t_last = 2^20, uniform pixels, and a tenth of the events doubled by an event of
               the opposite polarity (cells that cancel to exactly 0); with strays as `hostile` when h * w > 4096;
    equal, one_voxel, same_t   the degenerate sets below (dT = 0)."""
    rng = np.random.default_rng(seed)
    if kind in ("equal", "one_voxel", "same_t"):
        # dT = 0: every event in bin 0 with a left vote of +-1.  equal: distinct pixels, polarity +1 (an all-equal grid: sd 0);
        # one_voxel: one pixel (c = 1: sd NaN); same_t: repeated pixels, both polarities (integer voxels, some cancel to 0)
        pix = {"equal": lambda: rng.choice(h * w, n, replace=False), "one_voxel": lambda: np.full(n, (h // 2) * w + w // 3),
               "same_t": lambda: rng.integers(0, h * w, n)}[kind]()
        p = rng.integers(0, 2, n) * 2.0 - 1.0 if kind == "same_t" else np.ones(n)
        return np.ascontiguousarray(np.stack([np.full(n, 7.5), (pix % w).astype(np.float64), (pix // w).astype(np.float64), p], 1))
    if kind == "dyadic":
        m = max(1, n - n // 10)
        t = rng.integers(0, VOX_T_DYADIC + 1, m).astype(np.float64)
        x = rng.integers(0, w, m).astype(np.float64)
        y = rng.integers(0, h, m).astype(np.float64)
        p = rng.integers(0, 2, m) * 2.0 - 1.0
        if h * w > 4096:
            k = rng.random(m) < 0.05
            y = np.where(k, np.where(rng.random(m) < 0.5, h + rng.integers(0, 2 * h, m), -1.0 - rng.integers(0, 2 * h, m)), y)
        twin = rng.choice(m, n - m, replace=False) if n > m else np.zeros(0, dtype=np.int64)
        ev = np.stack([np.concatenate([t, t[twin]]), np.concatenate([x, x[twin]]), np.concatenate([y, y[twin]]),
                       np.concatenate([p, -p[twin]])], 1)
        ev = ev[np.argsort(ev[:, 0], kind="stable")]
        ev[0, 0], ev[-1, 0] = 0.0, float(VOX_T_DYADIC)
        return np.ascontiguousarray(ev)
    hot = rng.random(n) < 0.7
    ph, pw = min(40, h), min(40, w)
    x = np.where(hot, rng.integers(0, pw, n) + (w - pw) // 2, rng.integers(0, w, n)).astype(np.float64)
    y = np.where(hot, rng.integers(0, ph, n) + (h - ph) // 2, rng.integers(0, h, n)).astype(np.float64)
    t = np.sort(rng.uniform(100.0, 50100.0, n))
    p = rng.integers(0, 2, n) * 2.0 - 1.0
    if kind == "hostile":
        r = rng.random(n)
        x = np.where(r < 0.04, w + rng.integers(0, 4, n), x)
        y = np.where((r >= 0.04) & (r < 0.08), h + rng.integers(0, 2 * h, n), y)
        y = np.where((r >= 0.08) & (r < 0.12), -1.0 - rng.integers(0, 2 * h, n), y)
        p = np.where(rng.random(n) < 0.1, 0.0, p)                  # polarity 0 counts as -1
        x[n // 2], y[n // 2] = w - 1.0, h - 1.0                    # the last pixel of the last band
        t[-min(8, n):] = t[-1]
    else:
        assert kind == "clustered", kind
    return np.ascontiguousarray(np.stack([t, x, y, p], 1))


def vox_votes(events, bins, h, w):
    """vox_vote of voxel.hip (loader_utils.py:476-523) restated: per event the int64 index outputs il / ir (-1 where the reference masks the
    vote), the fp32 votes vl / vr, the unmasked flat indices and `inl` / `inr`: the vote is not masked AND its own flat index lies in
    [0, bins h w) - the flat-index semantics of index_add_ on the flattened grid, under which both kernels drop the rest."""
    ev = np.asarray(events, dtype=np.float64)
    t0 = ev[0, 0]
    dT = ev[-1, 0] - t0
    if dT == 0:
        dT = 1.0
    ts = (float(bins - 1) * (ev[:, 0] - t0)) / dT
    xs, ys = ev[:, 1].astype(np.int64), ev[:, 2].astype(np.int64)              # truncation
    pol = ev[:, 3].astype(np.float32)
    pol[pol == 0] = -1
    tis = np.floor(ts)
    tl = tis.astype(np.int64)
    dts = (ts - tis).astype(np.float32)
    vl, vr = pol * (np.float32(1.0) - dts), pol * dts
    okl = (tis < bins) & (tis >= 0)
    okr = ((tis + 1) < bins) & (tis >= 0)
    plane = h * w
    total = bins * plane
    fl = xs + ys * w + tl * plane
    fr = fl + plane
    return {"il": np.where(okl, fl, -1), "ir": np.where(okr, fr, -1), "vl": vl, "vr": vr, "okl": okl, "okr": okr, "flat_l": fl, "flat_r": fr,
            "inl": okl & (fl >= 0) & (fl < total), "inr": okr & (fr >= 0) & (fr < total), "tl": tl, "pix": xs + ys * w, "total": total}


def vox_exact(events, bins, h, w, votes=None):
    """Per occupied cell (flat index in `cells`, ascending): `sum`, the fp64 sum of its votes in event order (left votes first); `res`,
    the error-free residual exact sum - `sum` (TwoSum along the way flags the cells where an addition rounded; math.fsum of the votes and
    -sum gives those cells' residual, correctly rounded); `abs`, the sum of |votes|; `count`, the votes."""
    import math
    V = votes if votes is not None else vox_votes(events, bins, h, w)
    cells = np.concatenate([V["flat_l"][V["inl"]], V["flat_r"][V["inr"]]])
    vals = np.concatenate([V["vl"][V["inl"]], V["vr"][V["inr"]]]).astype(np.float64)
    order = np.argsort(cells, kind="stable")
    c, v = cells[order], vals[order]
    uniq, start, count = np.unique(c, return_index=True, return_counts=True)
    cid = np.repeat(np.arange(len(uniq)), count)
    rank = np.arange(len(c)) - np.repeat(start, count)
    by_rank = np.argsort(rank, kind="stable")
    maxc = int(count.max()) if len(count) else 0
    edge = np.searchsorted(rank[by_rank], np.arange(maxc + 1))
    s = np.zeros(len(uniq))
    rounded = np.zeros(len(uniq), dtype=bool)
    for r in range(maxc):
        sel = by_rank[edge[r]:edge[r + 1]]
        k, x = cid[sel], v[sel]
        a = s[k]
        t = a + x
        bb = t - a
        e = (a - (t - bb)) + (x - bb)                               # TwoSum: a + x = t + e exactly
        s[k] = t
        rounded[k] |= e != 0
    res = np.zeros(len(uniq))
    for k in np.nonzero(rounded)[0]:
        res[k] = math.fsum(list(v[start[k]:start[k] + count[k]]) + [-s[k]])
    return {"cells": uniq, "sum": s, "res": res, "abs": np.bincount(cid, weights=np.abs(v), minlength=len(uniq)), "count": count,
            "total": V["total"]}


def vox_dense(E, key="sum", dtype=np.float64):
    out = np.zeros(E["total"], dtype=dtype)
    out[E["cells"]] = E[key]
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _vox_empty_cells_zero(name, form, got, g):
    """Everything outside the occupied cells is +0.0 (no stray vote, no -0.0, no sentinel left behind)."""
    stray = int(np.count_nonzero(_bits(got))) - int(np.count_nonzero(_bits(g)))
    if stray:
        raise StageError(f"{name} [{form}]: {stray} cells that received no vote are not +0.0")


def vox_check_raw_exact(name, got, E, form, allow_residual=True):
    """The banded path's contract (and, on dyadic inputs, the direct path's): a cell is the exact sum of its votes rounded once."""
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    g, s = got[E["cells"]], E["sum"]
    r32 = s.astype(np.float32)
    inexact = E["res"] != 0
    differ = _bits(g) != _bits(r32)
    bad = differ & ~inexact
    n_in = int(inexact.sum())
    if n_in:
        up, dn = np.nextafter(r32, np.float32(np.inf)), np.nextafter(r32, np.float32(-np.inf))
        below = r32.astype(np.float64) <= s
        lo, hi = np.where(below, r32, dn), np.where(below, up, r32)
        bad |= inexact & (g != lo) & (g != hi)
    LOG.append({"name": name, "form": form + ":exact", "n": len(s), "differ": int(differ.sum()), "inexact": n_in,
                "of_bound": n_in / max(1, len(s)) / VOX_RESIDUAL_SHARE})
    if n_in and not allow_residual:
        raise StageError(f"{name} [{form}]: {n_in} cells of an input that must sum exactly have a residual")
    if n_in > VOX_RESIDUAL_SHARE * len(s):
        raise StageError(f"{name} [{form}]: {n_in} of {len(s)} occupied cells have a residual: more than {VOX_RESIDUAL_SHARE:g} of them")
    if bool(bad.any()):
        i = int(np.nonzero(bad)[0][0])
        raise StageError(f"{name} [{form}]: {int(bad.sum())} of {len(s)} occupied cells are not their exact sum rounded once; the first at flat "
                         f"index {int(E['cells'][i])} ({int(E['count'][i])} votes): got {float(g[i])!r}, exact {float(s[i])!r} -> {float(r32[i])!r}")
    _vox_empty_cells_zero(name, form, got, g)


def vox_check_raw_counted(name, got, E, form):
    """The direct path on generic inputs: fp32 atomics in any order, k = votes - 1 roundings against sum |votes|."""
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    g = got[E["cells"]]
    k = torch.from_numpy(np.maximum(E["count"] - 1, 0).astype(np.float64))
    check_counted(name, torch.from_numpy(g), torch.from_numpy(E["sum"]), torch.from_numpy(E["abs"]), k, form + ":counted")
    _vox_empty_cells_zero(name, form, got, g)


def vox_moment_bounds(raw, K):
    """fp64 moments of the non-zero voxels of a raw grid and the bounds above for a path that folds K cells per thread in fp32."""
    v = np.asarray(raw, dtype=np.float64).reshape(-1)
    v = v[v != 0]
    c = v.size
    if c == 0:
        return {"c": 0, "mean": 0.0, "sd": float("nan"), "any": False, "scale": False, "dmean": 0.0, "dsd": 0.0}
    m = float(v.sum() / c)
    m2 = float(((v - m) ** 2).sum())
    sd = float(np.sqrt(m2 / (c - 1))) if c > 1 else float("nan")
    dS = K * U * float(np.abs(v).sum())
    dQ = (K + 1) * U * float((v * v).sum())
    dm2 = dQ + 2 * abs(m) * dS + dS * dS / c
    dsd = dm2 / (2 * sd * (c - 1)) + U * sd if sd > 0 else 0.0
    return {"c": c, "mean": m, "sd": sd, "any": True, "scale": bool(sd > 0), "dmean": dS / c + U * abs(m), "dsd": dsd, "dm2": dm2, "m2": m2}


def vox_check_record(name, rec, raw, K, form):
    """The deferred record {mean, sd, scale, any} against the fp64 moments of the raw grid in front of it."""
    rec = np.asarray(rec, dtype=np.float32).astype(np.float64)
    M = vox_moment_bounds(raw, K)
    if M["scale"] and not M["sd"] > 4 * M["dsd"]:
        raise StageError(f"{name} [{form}]: the case does not decide `scale`: sd {M['sd']:.3g} against its bound {M['dsd']:.3g}")
    want_any, want_scale = (1.0 if M["any"] else 0.0), (1.0 if M["scale"] else 0.0)
    if rec[3] != want_any or rec[2] != want_scale:
        raise StageError(f"{name} [{form}]: record flags scale {rec[2]}, any {rec[3]}; {M['c']} non-zero voxels, sd {M['sd']!r}")
    em, es = abs(rec[0] - M["mean"]), (abs(rec[1] - M["sd"]) if M["scale"] else 0.0)
    LOG.append({"name": name, "form": form + ":record", "n": M["c"], "of_bound": max(em / max(M["dmean"], 1e-300), es / max(M["dsd"], 1e-300)) if M["any"] else 0.0,
                "mean_share": em / max(M["dmean"], 1e-300), "sd_share": es / max(M["dsd"], 1e-300)})
    if not M["scale"] and rec[1] != 1.0:
        raise StageError(f"{name} [{form}]: scale is 0, yet the record's sd is {rec[1]!r}, not 1")
    if not em <= M["dmean"]:
        raise StageError(f"{name} [{form}]: mean {rec[0]!r} against {M['mean']!r}: |diff| {em:.4g} > {M['dmean']:.4g} (K = {K})")
    if M["scale"] and not es <= M["dsd"]:
        raise StageError(f"{name} [{form}]: sd {rec[1]!r} against {M['sd']!r}: |diff| {es:.4g} > {M['dsd']:.4g} (K = {K})")
    return M


def vox_normalise_f32(raw, rec):
    """(v - mean) / sd on the non-zero voxels in fp32, operation by operation as vox_norm_kernel, the band kernel's normalised mode and
    conv_enc1.hip's consumer of the record evaluate it."""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    mean, sd, scale, anyv = (np.float32(r) for r in rec)
    if anyv == 0:
        return raw.copy()
    out = raw - mean
    if scale != 0:
        out = out / sd
    return np.where(raw != 0, out, raw).astype(np.float32)


def vox_check_normalised(name, got, raw, K, form):
    """A normalised grid against fp64 (v - m) / sd of the raw grid, by the bound derived above."""
    got = np.asarray(got, dtype=np.float32).astype(np.float64).reshape(-1)
    v = np.asarray(raw, dtype=np.float64).reshape(-1)
    M = vox_moment_bounds(raw, K)
    nz = v != 0
    if bool((got[~nz] != 0).any()):
        raise StageError(f"{name} [{form}]: {int((got[~nz] != 0).sum())} zero voxels were changed by the normalisation")
    if not M["any"]:
        return M
    d = v[nz] - M["mean"]
    if M["scale"]:
        ref = d / M["sd"]
        bound = (np.abs(ref) * (2 * U + M["dsd"] / M["sd"]) + M["dmean"] / M["sd"]) * ER_SLACK + TINY
    else:
        ref = d
        bound = (np.abs(d) * U + M["dmean"]) * ER_SLACK + TINY
    err = np.abs(got[nz] - ref)
    LOG.append({"name": name, "form": form + ":normalised", "n": int(nz.sum()), "of_bound": float((err / bound).max())})
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(np.argmax(np.where(bad, err / bound, 0)))
        raise StageError(f"{name} [{form}]: {int(bad.sum())} of {int(nz.sum())} normalised voxels are outside their bound; the worst: got "
                         f"{got[nz][i]!r}, ref {ref[i]!r}, |diff| {err[i]:.4g} against {bound[i]:.4g}")
    return M


def vox_check_indices(name, il, ir, V, form):
    for key, got in (("il", il), ("ir", ir)):
        got = np.asarray(got)
        if got.dtype != np.int64 or not np.array_equal(got, V[key]):
            bad = np.nonzero(got != V[key])[0]
            raise StageError(f"{name} [{form}]: {len(bad)} of {len(got)} {key} indices differ; the first at event {int(bad[0])}: "
                             f"got {int(got[bad[0]])}, reference {int(V[key][bad[0]])}")


# The cases of tests/test_gpu_vox_fp64.py: name -> (kind, n (a list: the sets of one eemflow_voxelize_many call), h, w, bins, modes, options).
# Modes: raw (normalize 0, with the index outputs), deferred (2), norm (1), twopass (1 under EEM_VOX_TWOPASS=1).  Options: direct
# (EEM_VOX_DIRECT=1), misalign (the grid starts 4 bytes past a 16-byte boundary).  Shapes are the smallest that reach the form, worked out
# from vox_plan: band_px is 64 below 64 x 512 pixels, (h w / 512 rounded up to 4) above, at most 9216 / bins.
_ALL = ("raw", "deferred", "norm", "twopass")
VOX_MANY_32 = [1 + (k * 577) % 2900 for k in range(32)]          # ragged: set 0 is a single event, twelve sets fill three binning blocks, eight one
VOX_CASES = {
    # BT 256 (bands of up to 24 KiB): vec4 off by h w % 4 (37 x 53), on (260 x 346); both end in a short band (41 of 64, 24 of 176 pixels)
    "bt256_v1_s6": ("hostile", 5_000, 37, 53, 3, _ALL, {}),
    "bt256_v4_s3": ("hostile", 50_000, 260, 346, 5, _ALL, {}),
    "bt256_misaligned": ("hostile", 50_000, 260, 346, 5, ("deferred", "norm", "twopass"), {"misalign": True}),
    # BT 512 (24 .. 40 KiB): 64 bins of 64 pixels = 32 KiB; 5 bins of 752 pixels, last band 480
    "bt512_s5": ("clustered", 20_000, 64, 64, 64, _ALL, {}),
    "bt512_s4": ("hostile", 50_000, 480, 800, 5, _ALL, {}),
    # BT 1024 (above 40 KiB): 64 bins of 144 pixels and 5 bins of 1800 pixels, 72 KiB each
    "bt1024_bins64": ("clustered", 20_000, 192, 384, 64, ("deferred", "norm"), {}),
    "bt1024_720p": ("clustered", 50_000, 720, 1280, 5, _ALL, {}),
    # the binning kernel's 1, 2, 4, 8 events per thread at the smallest counts that select them, on 33 bands of 64 pixels (the last 32):
    # runs of 31 .. 250 records for 64 lanes, the clean-up loop from EPT 4 on.  Dyadic: exact whatever the count
    "ept1": ("dyadic", 524_288, 40, 52, 3, ("deferred",), {}),
    "ept2": ("dyadic", 524_289, 40, 52, 3, ("deferred",), {}),
    "ept4": ("dyadic", 1_048_577, 40, 52, 3, ("deferred",), {}),
    "ept8": ("dyadic", 2_097_153, 40, 52, 3, ("raw", "norm"), {}),
    # dyadic inputs with fewer than 8 votes per cell: banded and direct path bitwise the exact sum
    "dyadic_banded": ("dyadic", 6_000, 60, 80, 5, _ALL, {}),
    "dyadic_direct": ("dyadic", 6_000, 60, 80, 5, ("raw", "deferred", "norm"), {"direct": True}),
    # the direct kernel on generic inputs (four runs of each mode) and by size: band_px 304 x 64 bins = 19 456 cells; 65 bins
    "generic_direct": ("hostile", 20_000, 60, 80, 5, ("raw", "deferred"), {"direct": True}),
    "direct_by_cells": ("dyadic", 20_000, 480, 644, 64, ("deferred",), {}),
    "direct_by_bins": ("dyadic", 3_000, 20, 24, 65, ("raw", "norm"), {}),
    # degenerate sets
    "one_event": ("clustered", 1, 37, 53, 3, _ALL, {}),
    "one_event_direct": ("clustered", 1, 37, 53, 3, ("deferred", "norm"), {"direct": True}),
    "one_voxel": ("one_voxel", 5, 37, 53, 3, ("deferred", "norm", "twopass"), {}),
    "one_voxel_direct": ("one_voxel", 5, 37, 53, 3, ("deferred", "norm"), {"direct": True}),
    "equal_voxels": ("equal", 300, 37, 53, 3, ("deferred", "norm", "twopass"), {}),
    "same_t": ("same_t", 900, 37, 53, 3, _ALL, {}),
    "bins1": ("hostile", 1_500, 37, 53, 1, _ALL, {}),
    # eemflow_voxelize_many: 1, 2 and 32 ragged sets; a set with fewer binning blocks than the longest, a set of one event
    "many1": ("hostile", [2_500], 40, 52, 3, ("deferred",), {}),
    "many2": ("hostile", [1, 2_500], 40, 52, 3, ("deferred", "twopass"), {}),
    "many32": ("hostile", VOX_MANY_32, 40, 52, 3, ("raw", "deferred", "norm"), {}),
    "many2_direct": ("hostile", [700, 1], 20, 24, 65, ("deferred",), {}),
}
VOX_MODE_NORMALIZE = {"raw": 0, "deferred": 2, "norm": 1, "twopass": 1}


def vox_case_form(name, mode):
    kind, n, h, w, bins, modes, opt = VOX_CASES[name]
    ns = n if isinstance(n, list) else [n]
    plan = vox_plan(ns, bins, h, w, aligned=not opt.get("misalign", False), direct=opt.get("direct", False))
    # (EEM_VOX_TWOPASS=<r> takes the two band passes while the longest set has at most one event per r voxels)
    return plan, vox_form(plan, len(ns), VOX_MODE_NORMALIZE[mode], mode == "twopass" and max(ns) <= bins * h * w)


def vox_case_events(name):
    kind, n, h, w, bins, modes, opt = VOX_CASES[name]
    ns = n if isinstance(n, list) else [n]
    return [vox_events(kind, ob_seed("vox", name, k), m, h, w, bins) for k, m in enumerate(ns)]


# Every launch sequence the cases reach, as eemflow_voxelize_last_form names it (tests/test_fp64_bounds_vox.py: vox_plan gives exactly these;
# the GPU module: every one was reported).  BT 256 / 512 / 1024, vec4 on and off (by h w % 4 and by the pointer), sgs 3 .. 6, EPT 1 .. 8, the
# three modes and what follows them, 1 / 2 / 32 jobs, the direct kernel with and without moments.
VOX_FORMS = {
    "j1:bin_e1+band1024_v4_s3_moments+band1024_v4_s3_normalised", "j1:bin_e1+band1024_v4_s3_raw", "j1:bin_e1+band1024_v4_s3_raw_sums+norm",
    "j1:bin_e1+band1024_v4_s3_raw_sums+stats", "j1:bin_e1+band256_v1_s3_moments+band256_v1_s3_normalised",
    "j1:bin_e1+band256_v1_s3_raw_sums+norm", "j1:bin_e1+band256_v1_s3_raw_sums+stats",
    "j1:bin_e1+band256_v1_s6_moments+band256_v1_s6_normalised", "j1:bin_e1+band256_v1_s6_raw", "j1:bin_e1+band256_v1_s6_raw_sums+norm",
    "j1:bin_e1+band256_v1_s6_raw_sums+stats", "j1:bin_e1+band256_v4_s3_moments+band256_v4_s3_normalised", "j1:bin_e1+band256_v4_s3_raw",
    "j1:bin_e1+band256_v4_s3_raw_sums+norm", "j1:bin_e1+band256_v4_s3_raw_sums+stats",
    "j1:bin_e1+band256_v4_s5_moments+band256_v4_s5_normalised", "j1:bin_e1+band256_v4_s5_raw", "j1:bin_e1+band256_v4_s5_raw_sums+norm",
    "j1:bin_e1+band256_v4_s5_raw_sums+stats", "j1:bin_e1+band256_v4_s6_raw_sums+stats",
    "j1:bin_e1+band512_v4_s4_moments+band512_v4_s4_normalised", "j1:bin_e1+band512_v4_s4_raw", "j1:bin_e1+band512_v4_s4_raw_sums+norm",
    "j1:bin_e1+band512_v4_s4_raw_sums+stats", "j1:bin_e1+band512_v4_s5_moments+band512_v4_s5_normalised", "j1:bin_e1+band512_v4_s5_raw",
    "j1:bin_e1+band512_v4_s5_raw_sums+norm", "j1:bin_e1+band512_v4_s5_raw_sums+stats", "j1:bin_e2+band256_v4_s6_raw_sums+stats",
    "j1:bin_e4+band256_v4_s6_raw_sums+stats", "j1:bin_e8+band256_v4_s6_raw", "j1:bin_e8+band256_v4_s6_raw_sums+norm", "j1:direct",
    "j1:direct+moments+norm", "j1:direct+moments+stats", "j2:bin_e1+band256_v4_s6_moments+band256_v4_s6_normalised",
    "j2:bin_e1+band256_v4_s6_raw_sums+stats", "j32:bin_e1+band256_v4_s6_raw", "j32:bin_e1+band256_v4_s6_raw_sums+norm",
    "j32:bin_e1+band256_v4_s6_raw_sums+stats",
}
