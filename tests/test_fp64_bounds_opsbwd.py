"""The checks of tests/test_gpu_opsbwd_fp64.py bite, shown without a GPU.

Each kernel of ops.hip / bwd_ops.hip that module covers is restated here in torch fp32 on the CPU.  A mutation planted in the restatement
must be rejected by the same composite check the GPU module applies (oracle/fp64_bounds.py: ob_check_*), on the GPU module's own inputs;
the unmutated restatement must pass every criterion on every input set.  The cap on lookup_bwd_rows' sliver allowance (fewer than 1 %
of any case's cells, none without near-integer coordinates) is checked here with the reference alone: no cell of any case uses it.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fp64_bounds as B

f32 = torch.float32


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ restatements
def lookup_bwd_f32(coords, dout, rows=False, mutate=None):
    """bwd_ops.hip's lookup adjoint in fp32.  rows: as lookup_bwd_rows_kernel finds corners (a row of the 11 x 11 window serves the taps
    [r - 2, r + 1]); rows="narrow": as it did before (ten rows, the taps {r - 1, r}), which the checks must reject."""
    b, _, hh, ww = coords.shape
    n = b * hh * ww
    out = []
    ph, pw = hh, ww
    for l in range(4):
        h, w = ph, pw
        x0, y0, tx, ty = B.er_lookup_geometry(coords, l, (h, w))
        g = dout[:, l * 81:(l + 1) * 81].permute(0, 2, 3, 1).reshape(n, 9, 9).float()
        if mutate == "transpose":
            g = g.transpose(1, 2)
        img = torch.zeros(n * h * w, dtype=f32)
        base = (torch.arange(n) * (h * w)).view(n, 1, 1)
        ii, jj = torch.arange(9).view(1, 9, 1), torch.arange(9).view(1, 1, 9)
        yb, xb = y0[:, :1, :1].clamp(-16, h + 16), x0[:, :1, :1].clamp(-16, w + 16)
        for dy, dx, wy, wx in ((0, 0, 1 - ty, 1 - tx), (0, 1, 1 - ty, tx), (1, 0, ty, 1 - tx), (1, 1, ty, tx)):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            if rows == "narrow":
                ry, rx = yy - yb - jj, xx - xb - ii
                ok = ok & ((ry == 0) | (ry == 1)) & ((rx == 0) | (rx == 1))
            elif rows:
                ry, rx = yy - yb - jj, xx - xb - ii
                ok = ok & (ry >= -1) & (ry <= 2) & (rx >= -1) & (rx <= 2) & (yy - yb >= 0) & (yy - yb <= 10) & (xx - xb >= 0) & (xx - xb <= 10)
            if mutate == "drop_corner" and (dy, dx) == (0, 0):
                ok = ok & ~((xx == 0) & (ii == 4) & (jj == 4))          # the centre tap's first corner on the left border column
            at = (base + yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1))[ok]
            img.index_put_((at,), (g * (wy * wx))[ok], accumulate=mutate != "assign")
        out.append(img.view(n, h, w))
        ph, pw = ph // 2, pw // 2
    return out


def pyramid_bwd_f32(f1, f2, dpyr, mutate=None):
    lv = [p.clone().float() for p in dpyr]
    for l in (2, 1, 0):
        h, w = lv[l].shape[-2:]
        up = lv[l + 1].repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25
        lv[l][:, :up.shape[1], :up.shape[2]] += up[:, :h, :w]
    b, c, h, w = f1.shape
    hw = h * w
    s = torch.tensor(B.ob_allpairs_scale(c), dtype=f32)
    if mutate == "scale":
        for _ in range(3):
            s = torch.nextafter(s, torch.tensor(float("inf")))
    dc = lv[0].reshape(b, hw, hw)
    a1, a2 = f1.reshape(b, c, hw).float(), f2.reshape(b, c, hw).float()
    kk = hw - 4 if mutate == "tail" else hw
    d1 = torch.einsum("bpq,bcq->bcp", dc[:, :, :kk], a2[:, :, :kk]) * s
    d2 = torch.einsum("bpq,bcp->bcq", dc[:, :kk], a1[:, :, :kk]) * s
    return {"dpyr": lv[:3], "dfmap1": d1.reshape(b, c, h, w), "dfmap2": d2.reshape(b, c, h, w)}


def convex_bwd_f32(flow, mask, dout, no_max=False):
    f = flow.clone().float().requires_grad_(True)
    m = mask.clone().float().requires_grad_(True)
    n, _, h, w = f.shape
    lg = m.view(n, 1, 9, 8, 8, h, w)
    if no_max:
        e = torch.exp(lg)
        wk = e / e.sum(2, keepdim=True)
    else:
        wk = torch.softmax(lg, 2)
    up = F.unfold(8 * f, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    out = torch.sum(wk * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, 8 * h, 8 * w)
    return torch.autograd.grad(out, (f, m), dout.float())


def warp_bwd_f32(x, flow, dout, mode, mask):
    xf = x.clone().float().requires_grad_(True)
    fl = flow.clone().float().requires_grad_(True)
    out = B.P.warp_align_true(xf, fl) if mode == 0 else B.P.torch_warp(xf, fl)
    if mode == 2:
        out = out * mask.float()[:, None]
    return torch.autograd.grad(out, (xf, fl), dout.float())


def resize_bwd_f32(dout, in_hw, mutate=None):
    h, w = in_hw
    oh, ow = dout.shape[-2:]
    (y0, y1, ly), (x0, x1, lx) = B.ob_ac_taps(h, w, oh, ow)
    if mutate == "swap" and oh == ow:
        ly, lx = lx, ly
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    dx = torch.zeros(*dout.shape[:-2], h * w, dtype=f32)
    rows = oh - 1 if mutate == "last_row" else oh
    for yi, xi, wgt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x1, (1 - ly) * lx), (y1, x0, ly * (1 - lx)), (y1, x1, ly * lx)):
        at = (yi.view(-1, 1) * w + xi.view(1, -1))[:rows].reshape(-1)
        dx.index_add_(-1, at, (dout.float() * wgt)[..., :rows, :].reshape(*dout.shape[:-2], -1))
    return dx.view(*dout.shape[:-2], h, w)


def instnorm_bwd_f32(x, y, dy, relu, mutate=None):
    if mutate == "gate_x":
        y = x
    if mutate == "mean":
        xx, g = x.float(), (dy * (y > 0) if relu else dy).float()
        m = xx.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((xx - m) ** 2).mean(1, keepdim=True) + 1e-5)
        xh = (xx - m) * rstd
        return rstd * (g - g.sum(1, keepdim=True) / max(x.shape[1] - 1, 1) - xh * (g * xh).mean(1, keepdim=True))
    return B.ob_instnorm_bwd_ref(x, y, dy, relu, dtype=f32)


def bn_train_fwd_f32(x, w, b, rm, rv, mom, eps, relu, biased=False):
    n, c, hw = x.shape
    cnt = n * hw
    mean = x.mean((0, 2))
    var = ((x - mean.view(1, -1, 1)) ** 2).mean((0, 2))
    ub = var * (cnt / (cnt - 1.0)) if cnt > 1 and not biased else var
    y = (x - mean.view(1, -1, 1)) / torch.sqrt(var + eps).view(1, -1, 1) * w.view(1, -1, 1) + b.view(1, -1, 1)
    return {"y": y.clamp_min(0) if relu else y, "save_mean": mean, "save_rstd": 1.0 / torch.sqrt(var + eps),
            "running_mean": (1 - mom) * rm + mom * mean, "running_var": (1 - mom) * rv + mom * ub}


# ------------------------------------------------------------------------------------------------------------------ lookup
def _lookup_case(h, w, kind):
    coords = B.ob_lookup_coords(h, w, kind, B.ob_seed("lookup", h, w, kind))
    dout = B.random_sign((2, 324, h, w), _g(B.ob_seed("lookup.dout", h, w, kind)))
    return coords, dout


@pytest.mark.parametrize("h,w", B.OB_LOOKUP_SHAPES)
@pytest.mark.parametrize("kind", ["hostile", "smooth"])
def test_lookup_restatements_pass_and_mutations_fail(h, w, kind):
    coords, dout = _lookup_case(h, w, kind)
    B.ob_check_lookup("scatter", lookup_bwd_f32(coords, dout), coords, dout, "lookup_bwd_scatter")
    B.ob_check_lookup("rows", lookup_bwd_f32(coords, dout, rows=True), coords, dout, "lookup_bwd_rows")
    for mut in ("drop_corner", "transpose", "assign"):
        with pytest.raises(B.StageError):
            B.ob_check_lookup(mut, lookup_bwd_f32(coords, dout, mutate=mut), coords, dout, "lookup_bwd_scatter")
        with pytest.raises(B.StageError):
            B.ob_check_lookup(mut, lookup_bwd_f32(coords, dout, rows=True, mutate=mut), coords, dout, "lookup_bwd_rows")
    if kind == "hostile":                   # the kernel as it was: ten window rows, each serving the taps {r - 1, r}
        with pytest.raises(B.StageError):
            B.ob_check_lookup("narrow", lookup_bwd_f32(coords, dout, rows="narrow"), coords, dout, "lookup_bwd_rows")


@pytest.mark.parametrize("h,w", B.OB_LOOKUP_SHAPES)
@pytest.mark.parametrize("kind", ["hostile", "smooth"])
def test_rows_allowance_is_a_sliver(h, w, kind):
    """Fewer than 1 % of a case's cells use the allowance, none without near-integer coordinates.  Measured: none at all, on every case -
    the 11 x 11 window with four candidate taps per row finds every corner (the ten-row window serving two taps lost corners in 5204 of
    271 360 cells of the hostile 16 x 20 case, up to 7.0e-7 |dout| against a bound of 3.0e-8)."""
    coords, dout = _lookup_case(h, w, kind)
    refs = B.ob_lookup_bwd_ref(coords, dout, rows=True)
    cells, total = sum(lv["cells"] for lv in refs), sum(lv["ref"].numel() for lv in refs)
    print(f"lookup {h}x{w} {kind}: {cells} of {total} cells use the allowance ({[lv['cells'] for lv in refs]} per level), "
          f"largest lost weight {max(lv['lost_over_ulp'] for lv in refs):.3g} ulp")
    assert cells < B.LOOKUP_ALLOWANCE_CAP * total
    if kind == "smooth":
        assert cells == 0


# ------------------------------------------------------------------------------------------------------------------ pyramid
def _pyramid_case(c, h, w):
    g = _g(B.ob_seed("pyramid", c, h, w))
    f1, f2 = torch.randn(2, c, h, w, generator=g), torch.randn(2, c, h, w, generator=g)
    dpyr = [B.random_sign((2 * h * w, h >> l, w >> l), g) for l in range(4)]
    return f1, f2, dpyr


@pytest.mark.parametrize("c,h,w", B.OB_PYRAMID_CASES)
def test_pyramid_restatement_passes_and_mutations_fail(c, h, w):
    f1, f2, dpyr = _pyramid_case(c, h, w)
    B.ob_check_pyramid("pyr", pyramid_bwd_f32(f1, f2, dpyr), f1, f2, dpyr)
    with pytest.raises(B.StageError):
        B.ob_check_pyramid("scale", pyramid_bwd_f32(f1, f2, dpyr, "scale"), f1, f2, dpyr)
    if (h * w) % 8 == 4:
        with pytest.raises(B.StageError):
            B.ob_check_pyramid("tail", pyramid_bwd_f32(f1, f2, dpyr, "tail"), f1, f2, dpyr)


# ------------------------------------------------------------------------------------------------------------------ convex upsampling
@pytest.mark.parametrize("h,w", B.OB_CONVEX_SHAPES)
@pytest.mark.parametrize("kind", B.OB_CONVEX_KINDS)
def test_convex_restatement_passes(h, w, kind):
    flow, mask, dout = B.ob_convex_inputs(h, w, kind, B.ob_seed("convex", h, w, kind))
    df, dm = convex_bwd_f32(flow, mask, dout)
    B.ob_check_convex("convex", df, dm, flow, mask, dout)
    with pytest.raises(B.StageError):                                      # half of every cell's contributions lost
        B.ob_check_convex("half", df * 0.5, dm, flow, mask, dout)


def test_softmax_without_the_max_subtraction_is_rejected():
    """exp(l) / sum exp(l) at the +-40 logits: nothing overflows in fp32 (e^44 = 1.3e19), but the derivative of the unshifted quotient
    cancels between e^40-sized terms, and dmask leaves check_decoder's bound by ten orders of magnitude (rms 2.9e-7 against the 9.6e-16
    of torch's shifted softmax).  On the 5 x 7 map; on the two one-row maps the unshifted form stays within 0.07 of the bound and is
    not told from torch's."""
    h, w = B.OB_CONVEX_SHAPES[0]
    flow, mask, dout = B.ob_convex_inputs(h, w, "extreme", B.ob_seed("convex", h, w, "extreme"))
    df, dm = convex_bwd_f32(flow, mask, dout, no_max=True)
    with pytest.raises(B.StageError):
        B.ob_check_convex("no_max", df, dm, flow, mask, dout)


# ------------------------------------------------------------------------------------------------------------------ warp
@pytest.mark.parametrize("c,h,w", B.OB_WARP_SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_warp_restatement_passes_and_mutations_fail(c, h, w, mode):
    flows = B.ob_warp_flows(h, w, B.ob_seed("warp", h, w))
    g = _g(B.ob_seed("warp.x", c, h, w, mode))
    x = torch.randn(6, c, h, w, generator=g)
    dout = B.random_sign((6, c, h, w), g)
    mask = B.pl_warp_taps(flows, mode)["mask"]
    dx, dflow = warp_bwd_f32(x, flows, dout, mode, mask)
    B.ob_check_warp_bwd("warp", dx, dflow, x, flows, dout, mode, mask)
    if h > 1 and w > 1:
        bad = dx.clone()
        bad[:, :, 0, :] = dx[:, :, 0, :] * 0.5                              # a tap lost along the top border
        with pytest.raises(B.StageError):
            B.ob_check_warp_bwd("border", bad, dflow, x, flows, dout, mode, mask)


# ------------------------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("in_hw,out_hw", B.OB_RESIZE_CASES)
def test_resize_restatements_pass_and_mutations_fail(in_hw, out_hw):
    g = _g(B.ob_seed("resize", in_hw, out_hw))
    x = torch.randn(4, *in_hw, generator=g)
    dout = B.random_sign((4, *out_hw), g)
    y32 = F.interpolate(x[None], size=out_hw, mode="bilinear", align_corners=True)[0]
    ref, mag = B.ob_resize_ref(x, out_hw)
    B.check_roundings("resize", y32, ref, mag, "resize_ac")
    for form in ("resize_ac_bwd_gather", "resize_ac_bwd_scatter"):
        B.ob_check_resize_bwd("bwd", resize_bwd_f32(dout, in_hw), dout, in_hw, form)
        if out_hw[0] > 1:
            with pytest.raises(B.StageError):
                B.ob_check_resize_bwd("last_row", resize_bwd_f32(dout, in_hw, "last_row"), dout, in_hw, form)
    if out_hw == (3, 3):                                                    # (square maps: the swap keeps the shapes)
        gx = torch.zeros(4, 2, 2)
        gx[:, 0, 1] = 1.0
        d = torch.einsum("pyx,Yy,Xx->pYX", gx.double(), *[B._ac_matrix(2, 3)[0]] * 2).float()
        with pytest.raises(B.StageError):
            B.ob_check_resize_bwd("swap", resize_bwd_f32(d, in_hw).transpose(-1, -2).contiguous(), d, in_hw, "resize_ac_bwd_gather")


# ------------------------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("hw", B.OB_INSTNORM_HW)
@pytest.mark.parametrize("relu", [0, 1])
def test_instnorm_restatement_passes_and_mutations_fail(hw, relu):
    x = B.ob_norm_input(1, 3, hw, B.ob_seed("instnorm", hw))[0]
    y = B.ob_gated_output(F.instance_norm(x[None], eps=1e-5)[0] if hw > 1 else x * 0, B.ob_seed("instnorm.y", hw))
    dy = B.random_sign((3, hw), _g(B.ob_seed("instnorm.dy", hw)))
    ref = B.ob_instnorm_bwd_ref(x, y, dy, relu)
    B.ob_check_planes("instnorm", instnorm_bwd_f32(x, y, dy, relu), ref, B.ob_instnorm_bwd_ref(x, y, dy, relu, dtype=f32), "instnorm_bwd", 0)
    if hw in (63, 437):                        # (hw - 1 for hw moves mean(g) by 1 / hw of itself: beneath fp32's own error at 16 384)
        muts = ["mean"] + (["gate_x"] if relu else [])
        for mut in muts:
            with pytest.raises(B.StageError):
                B.ob_check_planes(mut, instnorm_bwd_f32(x, y, dy, relu, mut), ref, B.ob_instnorm_bwd_ref(x, y, dy, relu, dtype=f32), "instnorm_bwd", 0)


def _bn_case(n, c, hw, relu):
    g = _g(B.ob_seed("bn", n, c, hw, relu))
    x = B.ob_norm_input(n, c, hw, B.ob_seed("bn.x", n, c, hw), constant=False)
    w, b = torch.randn(c, generator=g), torch.randn(c, generator=g)
    w[0] = 0.0
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return x, w, b, rm, rv, g


@pytest.mark.parametrize("n,c,hw", B.OB_BN_CASES)
@pytest.mark.parametrize("relu", [0, 1])
def test_bn_restatements_pass_and_mutations_fail(n, c, hw, relu):
    x, w, b, rm, rv, g = _bn_case(n, c, hw, relu)
    mom, eps = np.float32(0.1), np.float32(1e-5)
    refs = B.ob_bn_train_fwd_ref(x, w, b, rm, rv, mom, eps, relu)
    got = bn_train_fwd_f32(x, w, b, rm, rv, float(mom), float(eps), relu)
    keys = ("save_mean", "save_rstd", "running_mean", "running_var")
    # torch's fp32 means are sums in fp32 (hw roundings), not the kernel's fp64 sums: they are held to the count with hw added
    loose = {k: (refs[k][0], refs[k][1], refs[k][2] + 2 * np.sqrt(n * hw), *refs[k][3:]) for k in keys}
    loose["save_rstd"] = (refs["save_rstd"][0], refs["save_rstd"][1], 1.0, refs["save_rstd"][3] + B.U * refs["save_rstd"][0] * 4 * np.sqrt(n * hw) *
                          (x.double() ** 2).mean((0, 2)) / (x.double().var((0, 2), unbiased=False) + 1e-5))
    B.ob_check_counted_map("bn_train_fwd", got, loose, "bn_train_fwd", keys)
    B.ob_check_planes("bn_train_fwd.y", got["y"], refs["y"], refs["y32"], "bn_train_fwd", 1)
    if n * hw > 1:
        bad = bn_train_fwd_f32(x, w, b, rm, rv, float(mom), float(eps), relu, biased=True)
        exact = {"running_var": refs["running_var"][0].float()}
        B.ob_check_counted_map("exact", exact, refs, "bn_train_fwd", ("running_var",))          # (the fp64 value rounded once passes the tight count)
        if n * hw < 8192:                                                                      # (1 / cnt is beneath a rounding from 2^13 values on)
            with pytest.raises(B.StageError):
                B.ob_check_counted_map("biased", bad, loose, "bn_train_fwd", ("running_var",))
    # backward, train and eval
    y = B.ob_gated_output(refs["y32"], B.ob_seed("bn.y", n, c, hw))
    dy = B.random_sign((n, c, hw), g)
    sm, sr = refs["save_mean"][0].float(), refs["save_rstd"][0].float()
    r = B.ob_bn_train_bwd_ref(x, y, dy, w, sm, sr, relu)
    B.ob_check_planes("bn_train_bwd.dx", r["dx32"], r["dx"], r["dx32"], "bn_train_bwd", 1)
    rv2 = rv.clone()
    rv2[c - 1] = 1e-7
    e = B.ob_bn_eval_bwd_ref(x, y, dy, w, rm, rv2, eps, relu)
    B.ob_check_planes("bn_eval_bwd.dx", e["dx32"], e["dx"], e["dx32"], "bn_eval_bwd", 1)
    y64, y32 = B.ob_bn_eval_fwd_ref(x, w, b, rm, rv2, eps, relu), B.ob_bn_eval_fwd_ref(x, w, b, rm, rv2, eps, relu, dtype=f32)
    B.ob_check_planes("bn_eval_fwd.y", y32, y64, y32, "bn_eval_fwd", 1)
    B.check_roundings("bn_eval_fwd.y", y32, y64, B.ob_bn_eval_fwd_mag(x, w, b, rm, rv2, eps), "bn_eval_y")
    for ref in (r, e):
        dw, mw, kw = ref["dweight"]
        B.check_counted("dweight", dw.float(), dw, mw, kw, "bn")
        if relu and n * hw >= 357:                                          # the gate taken from x instead of y
            gx = B.ob_bn_train_bwd_ref(x, x, dy, w, sm, sr, relu)["dbias"][0]
            with pytest.raises(B.StageError):
                B.check_counted("gate_x", gx.float(), *r["dbias"], "bn")


# ------------------------------------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("n", B.OB_ELEMENTWISE_N)
def test_elementwise_restatements_pass_and_mutations_fail(n):
    g = _g(B.ob_seed("elementwise", n))
    dy, v = B.random_sign((n,), g), torch.randn(n, generator=g)
    y = B.ob_gated_output(v, B.ob_seed("elementwise.y", n))
    for kind, yy in ((B.GACT_RELU, y), (B.GACT_LEAKY, y), (B.GACT_SIGMOID, torch.sigmoid(v)), (B.GACT_TANH, torch.tanh(v)), (B.GACT_NONE, v)):
        ref, mag, kk = B.ob_act_bwd_ref(dy, yy, kind, 1.7)
        d = {B.GACT_RELU: (yy > 0).float(), B.GACT_LEAKY: torch.where(yy > 0, 1.0, B.LEAKY).float(), B.GACT_SIGMOID: yy * (1 - yy),
             B.GACT_TANH: 1 - yy * yy, B.GACT_NONE: torch.ones(n)}[kind]
        B.check_roundings("act_bwd", dy * d * np.float32(1.7), ref, mag, kk)
    z, h, q = torch.rand(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    B.check_roundings("gru", (1 - z) * h + z * q, *B.ob_gru_blend_ref(z, h, q), "gru_blend")
    for key, got in (("dz", dy * (q - h)), ("dh", dy * (1 - z)), ("dq", dy * z)):
        ref, mag, kk = B.ob_gru_blend_bwd_ref(dy, z, h, q)[key]
        B.check_roundings(key, got, ref, mag, kk)
    if n >= 255:                                                             # ReLU gate from the pre-activation's sign of another tensor
        ref, mag, kk = B.ob_act_bwd_ref(dy, y, B.GACT_RELU, 1.0)
        with pytest.raises(B.StageError):
            B.check_roundings("gate_x", dy * (v > -0.5).float(), ref, mag, kk)


@pytest.mark.parametrize("count", [1, 2, 7, 8, 9, 17])
@pytest.mark.parametrize("n", [3, 1026, 1027])
def test_sum_n_restatement_passes_and_a_dropped_tail_fails(count, n):
    g = _g(B.ob_seed("sum_n", count, n))
    ts = [B.random_sign((n,), g) for _ in range(count)]
    ref, mag, k = B.ob_sum_ref(ts)
    got = ts[0].clone()
    for t in ts[1:]:
        got = got + t
    B.check_counted("sum_n", got, ref, mag, k, "sum_n_v4")
    if n % 4:                                                                # the (< 4) values past the last 16-byte piece left unwritten
        bad = got.clone()
        bad[n - n % 4:] = 0.0
        with pytest.raises(B.StageError):
            B.check_counted("tail", bad, ref, mag, k, "sum_n_v4")
