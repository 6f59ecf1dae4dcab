"""Every non-convolution autograd kernel of ops.hip and bwd_ops.hip against fp64, form by form.  `pytest -m gpu`.

E-RAFT and EEMFlow+ training run these kernels between the convolutions.  Every case makes ONE ABI call on inputs of its own (ReLU
gates from the y passed in, the mode-2 warp mask from the GPU forward), asserts by `eemop_last_op_form` that the intended launch form ran,
and holds each output to one of the three criteria of oracle/fp64_bounds.py, none fitted to these kernels: counted roundings (k u mag per
element; k + N - 1 for an element of a scatter / gather adjoint that receives N contributions), LIMITS["direct"] for the two all-pairs
GEMMs, and check_decoder's KAPPA_DEC against torch's fp32 CPU evaluation where a division by a computed statistic or a softmax sets the
conditioning.  Copies, the shuffle, pool2_bwd and a scaling by a power of two are compared bitwise.  Geometry (floor, the bilinear
fractions, ac_taps' sy * Y) is the operators' definition and is taken in fp32; everything after it is fp64.  Every output is written into
the middle of a larger sentinel-filled allocation whose guard regions must come back bitwise; outputs that accumulate with atomics
(lookup scatter, warp dx, convex-up dflow, resize scatter) run four times, each run held to the bounds.  The adjoint identity
|<F x, g> - <x, F^T g>| on the GPU's own forward and backward catches a geometry mismatch a shared reference geometry would hide.
tests/test_fp64_bounds_opsbwd.py shows on the CPU that these checks reject twelve planted mutations and pass torch's fp32 evaluation.

LEFT OUT, and why:
  * the convolution forms and the forward launchers er_instnorm_launch, er_allpairs_launch, er_lookup_launch, er_pool2*,
    er_convex_up_launch, the EEMFlow+ warp and upflow: held to fp64 by the stage modules (they serve here as F of the adjoint identity).
  * eemflow_local_corr53 / eemop_local_corr53_bwd: tr_corr_bwd_launch, family corr_bwd of tests/test_gpu_train_fp64.py.
  * sigmoid and tanh FORWARD accuracy: a transcendental's contract, as in tests/test_gpu_ops_fp64.py (their backward is counted here).

MEASURED worst statistics per check kind (one AMD Instinct MI355X, gfx950; over all cases and all four runs of the atomic outputs).  A record:
these numbers set no limit.  max|z|: the largest error in units of u times the sum of |terms|; of bound: the largest error as a share of
its counted bound (or of the adjoint identity's tolerance); kappa: the GPU's error over that of torch's fp32 CPU evaluation (limit 6.4).
The counted bounds of a single rounding are tight by construction (sum_n, warp dx, the pooling fold: 0.98 - 1.00 of the bound).
  form / check                      max|z| of bound kappa rms kappa max checks
  act_bwd                            1.68       -       -       -     25
  allpairs_bwd                       4.65   1.000       -       -     20
  binary                             0.99       -       -       -     25
  bitwise                               -       -       -       -     29
  bn_eval_bwd_t1024                  0.05   0.016       -       -      8
  bn_eval_bwd_t1024:kappa               -       -    2.98    2.40     10
  bn_eval_bwd_t256                   1.55   0.259       -       -      8
  bn_eval_bwd_t256:kappa                -       -    3.36    2.56     10
  bn_eval_fwd_t1024                  3.16       -       -       -      4
  bn_eval_fwd_t1024:kappa               -       -    1.73    2.30     10
  bn_eval_fwd_t256                   2.15       -       -       -      4
  bn_eval_fwd_t256:kappa                -       -    2.39    2.05     10
  bn_train_bwd_t1024                 0.02   0.016       -       -      8
  bn_train_bwd_t1024:kappa              -       -    1.00    1.00     10
  bn_train_bwd_t256                  0.06   0.043       -       -      8
  bn_train_bwd_t256:kappa               -       -    1.00    1.00     10
  bn_train_fwd_t1024                 1.44   0.480       -       -     16
  bn_train_fwd_t1024:kappa              -       -    0.67    0.95     10
  bn_train_fwd_t256                  1.04   0.897       -       -     16
  bn_train_fwd_t256:kappa               -       -    0.84    0.89     10
  convex_up_bwd                      0.20   0.200       -       -     36
  convex_up_bwd:adjoint                 -   0.002       -       -      9
  convex_up_bwd:kappa                   -       -    1.02    1.00     36
  gru_blend                          1.57       -       -       -      5
  gru_blend_bwd                      1.76       -       -       -     15
  instnorm_bwd_t1024:kappa              -       -    1.00    1.00     12
  instnorm_bwd_t256:kappa               -       -    1.04    1.06     24
  lookup_bwd_rows                    3.70   0.378       -       -     16
  lookup_bwd_rows:adjoint               -       -       -       -      4
  lookup_bwd_scatter                 3.25   0.599       -       -     64
  lookup_bwd_scatter:adjoint            -       -       -       -      4
  pool2_bwd:adjoint                     -   0.087       -       -      3
  resize_ac                          2.86       -       -       -      8
  resize_ac_bwd_gather               1.12   0.156       -       -      8
  resize_ac_bwd_gather:adjoint          -   0.011       -       -      7
  resize_ac_bwd_scatter              2.19   0.234       -       -     28
  resize_ac_bwd_scatter:adjoint         -   0.010       -       -      7
  scale_flow                         0.97       -       -       -     11
  sum_n_scalar                       2.16   0.993       -       -     12
  sum_n_v4                           2.74   0.993       -       -     14
  warp_bwd_m0                        2.61   0.979       -       -     12
  warp_bwd_m0:adjoint                   -   0.009       -       -      3
  warp_bwd_m0:kappa                     -       -    1.04    1.00     12
  warp_bwd_m1                        3.06   0.993       -       -     12
  warp_bwd_m1:adjoint                   -   0.040       -       -      3
  warp_bwd_m1:kappa                     -       -    1.06    1.00     12
  warp_bwd_m2                        2.33   0.993       -       -     12
  warp_bwd_m2:adjoint                   -   0.026       -       -      3
  warp_bwd_m2:kappa                     -       -    1.00    1.00     12
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eemflow_amd import _lib, ops
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.678
GUARD = 64                   # floats on either side of an output (256 bytes: the 16-byte alignment of the output is the allocation's)
SWITCHES = ("EEM_LOOKUP_BWD_SCATTER", "EEM_RESIZE_BWD_SCATTER")
SEEN = set()
EEM_ERR_ARG = 1


def _pin(monkeypatch, env=None):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        assert name in SWITCHES, name
        monkeypatch.setenv(name, value)


def _g(*key):
    return torch.Generator().manual_seed(B.ob_seed(*key))


def _sp():
    return _lib.current_stream_ptr(torch.device(DEV))


def _dev(t):
    return t.to(DEV).float().contiguous()


def last_form():
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.lib().eemop_last_op_form(buf, len(buf)))
    return buf.value.decode()


def ran(form):
    got = last_form()
    assert got == form, f"launch form {got!r}, expected {form!r}"
    SEEN.add(got)


class Out:
    """An output (or in-place operand, `init`) in the middle of a sentinel-filled allocation."""

    def __init__(self, *shape, init=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        s = torch.full((GUARD,), SENTINEL)
        assert torch.equal(b[:GUARD].view(torch.int32), s.view(torch.int32)), "the guard in front of the output was written"
        assert torch.equal(b[GUARD + self.n:].view(torch.int32), s.view(torch.int32)), "the guard behind the output was written"
        return b[GUARD:GUARD + self.n].view(self.t.shape).clone()


L = _lib.lib


# ----------------------------------------------------------------------------------------------------------------------- lookup
def run_lookup_bwd(coords, dout):
    b, _, h, w = coords.shape
    c, d = _dev(coords), _dev(dout)
    outs = [Out(b * h * w, h >> l, w >> l) for l in range(4)]
    _lib.check(L().eraft_corr_lookup_bwd(c.data_ptr(), d.data_ptr(), b, h, w, *[o.ptr() for o in outs], _sp()))
    return [o.cpu() for o in outs]


def run_lookup_fwd(pyr, coords):
    b, _, h, w = coords.shape
    ps, c = [_dev(p) for p in pyr], _dev(coords)
    out = Out(b, 324, h, w)
    _lib.check(L().eemop_corr_lookup_fwd(*[p.data_ptr() for p in ps], c.data_ptr(), b, h, w, out.ptr(), _sp()))
    return out.cpu()


@pytest.mark.parametrize("h,w", B.OB_LOOKUP_SHAPES)
@pytest.mark.parametrize("kind", ["hostile", "smooth"])
@pytest.mark.parametrize("form", ["lookup_bwd_rows", "lookup_bwd_scatter"])
def test_lookup_bwd(monkeypatch, form, kind, h, w):
    _pin(monkeypatch, {"EEM_LOOKUP_BWD_SCATTER": "1"} if form.endswith("scatter") else {})
    coords = B.ob_lookup_coords(h, w, kind, B.ob_seed("lookup", h, w, kind))
    dout = B.random_sign((2, 324, h, w), _g("lookup.dout", h, w, kind))
    for _ in range(4 if form.endswith("scatter") else 1):
        got = run_lookup_bwd(coords, dout)
        ran(form)
        refs = B.ob_check_lookup(f"lookup {h}x{w} {kind}", got, coords, dout, form)
    if form == "lookup_bwd_rows":
        assert sum(lv["cells"] for lv in refs) == 0
    # the adjoint identity with the GPU's own forward on a random pyramid
    g = _g("lookup.pyr", h, w, kind)
    pyr = [torch.randn(2 * h * w, h >> l, w >> l, generator=g) for l in range(4)]
    fx = run_lookup_fwd(pyr, coords)
    _, fmag = B.er_lookup_ref([p[:, None] for p in pyr], coords)
    bf = B.bound_counted(fmag, B.ER_ROUNDINGS["lookup_fwd"])
    lhs_x = torch.cat([p.reshape(-1) for p in pyr])
    B.check_adjoint(f"lookup {h}x{w} {kind}", lhs_x, fx, dout, torch.cat([t.reshape(-1) for t in got]), bf,
                    torch.cat([lv["bound"].reshape(-1) for lv in refs]), form)


# ----------------------------------------------------------------------------------------------------------------------- pyramid
def run_pyramid_bwd(f1, f2, dpyr, expect_rc=0):
    b, c, h, w = f1.shape
    a1, a2 = _dev(f1), _dev(f2)
    lv = [Out(*p.shape, init=_dev(p)) for p in dpyr]
    d1, d2 = Out(b, c, h, w), Out(b, c, h, w)
    rc = L().eraft_corr_pyramid_bwd(a1.data_ptr(), a2.data_ptr(), *[o.ptr() for o in lv], b, c, h, w, d1.ptr(), d2.ptr(), _sp())
    assert rc == expect_rc, (rc, L().eemflow_last_error())
    return {"dpyr": [o.cpu() for o in lv], "dfmap1": d1.cpu(), "dfmap2": d2.cpu()}


def _pyramid_case(c, h, w):
    g = _g("pyramid", c, h, w)
    f1, f2 = torch.randn(2, c, h, w, generator=g), torch.randn(2, c, h, w, generator=g)
    return f1, f2, [B.random_sign((2 * h * w, h >> l, w >> l), g) for l in range(4)]


@pytest.mark.parametrize("c,h,w", B.OB_PYRAMID_CASES)
def test_pyramid_bwd(monkeypatch, c, h, w):
    _pin(monkeypatch)
    f1, f2, dpyr = _pyramid_case(c, h, w)
    got = run_pyramid_bwd(f1, f2, dpyr)
    ran("allpairs_bwd")
    assert torch.equal(got["dpyr"][3], dpyr[3])
    B.ob_check_pyramid(f"pyramid c{c} {h}x{w}", got, f1, f2, dpyr)


@pytest.mark.parametrize("c", [16, 40])
def test_pyramid_bwd_refuses_a_map_of_odd_size_before_it_touches_anything(monkeypatch, c):
    """h * w = 315 is no multiple of 4 (the forward has allpairs_odd for it): EEM_ERR_ARG with all six buffers bitwise as they were."""
    _pin(monkeypatch)
    f1, f2, dpyr = _pyramid_case(c, 15, 21)
    got = run_pyramid_bwd(f1, f2, dpyr, expect_rc=EEM_ERR_ARG)
    assert "h*w must be a multiple of 4" in L().eemflow_last_error().decode()
    sent = torch.full((2, c, 15, 21), SENTINEL)
    for name, a, b in [("dfmap1", got["dfmap1"], sent), ("dfmap2", got["dfmap2"], sent)] + [(f"dpyr{l}", got["dpyr"][l], dpyr[l]) for l in range(4)]:
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


# ----------------------------------------------------------------------------------------------------------------------- convex upsampling
def run_convex_bwd(flow, mask, dout):
    b, _, h, w = flow.shape
    f, m, d = _dev(flow), _dev(mask), _dev(dout)
    df, dm = Out(b, 2, h, w), Out(b, 576, h, w)
    _lib.check(L().eraft_convex_upsample_bwd(f.data_ptr(), m.data_ptr(), d.data_ptr(), b, h, w, df.ptr(), dm.ptr(), _sp()))
    return df.cpu(), dm.cpu()


@pytest.mark.parametrize("h,w", B.OB_CONVEX_SHAPES)
@pytest.mark.parametrize("kind", B.OB_CONVEX_KINDS)
def test_convex_up_bwd(monkeypatch, kind, h, w):
    _pin(monkeypatch)
    flow, mask, dout = B.ob_convex_inputs(h, w, kind, B.ob_seed("convex", h, w, kind))
    for _ in range(4):
        df, dm = run_convex_bwd(flow, mask, dout)
        ran("convex_up_bwd")
        r = B.ob_check_convex(f"convex {h}x{w} {kind}", df, dm, flow, mask, dout)
    f, m, z = _dev(flow), _dev(mask), torch.zeros(2, 2, h, w, device=DEV)
    up = Out(2, 2, 8 * h, 8 * w)
    _lib.check(L().eemop_convex_upsample_fwd(z.data_ptr(), f.data_ptr(), m.data_ptr(), 2, h, w, up.ptr(), _sp()))
    B.check_adjoint(f"convex {h}x{w} {kind}", flow, up.cpu(), dout, df, B.ob_convex_up_fwd_bound(flow, mask), r["dflow"][1], "convex_up_bwd")


# ----------------------------------------------------------------------------------------------------------------------- warp
def run_warp_fwd(x, flow, mode):
    b, c, h, w = x.shape
    xd, fd = _dev(x), _dev(flow)
    out = Out(b, c, h, w)
    _lib.check(L().eemplus_warp(xd.data_ptr(), fd.data_ptr(), b, c, h, w, mode, out.ptr(), _sp()))
    return out.cpu()


def run_warp_bwd(x, flow, dout, mode):
    b, c, h, w = x.shape
    xd, fd, dd = _dev(x), _dev(flow), _dev(dout)
    dx, df = Out(b, c, h, w), Out(b, 2, h, w)
    _lib.check(L().eemplus_warp_bwd(xd.data_ptr(), fd.data_ptr(), dd.data_ptr(), b, c, h, w, mode, dx.ptr(), df.ptr(), _sp()))
    return dx.cpu(), df.cpu()


@pytest.mark.parametrize("c,h,w", B.OB_WARP_SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_warp_bwd(monkeypatch, mode, c, h, w):
    """Batch 6: one image per rule of the flows (integers, half-integers, the borders in both conventions, far outside, random)."""
    _pin(monkeypatch)
    flows = B.ob_warp_flows(h, w, B.ob_seed("warp", h, w))
    g = _g("warp.x", c, h, w, mode)
    x = torch.randn(6, c, h, w, generator=g)
    dout = B.random_sign((6, c, h, w), g)
    mask = B.pl_mask_of(run_warp_fwd(torch.ones(6, 1, h, w), flows, 2)) if mode == 2 else torch.ones(6, h, w, dtype=torch.bool)
    for _ in range(4):
        dx, df = run_warp_bwd(x, flows, dout, mode)
        ran(f"warp_bwd_m{mode}")
        r = B.ob_check_warp_bwd(f"warp m{mode} c{c} {h}x{w}", dx, df, x, flows, dout, mode, mask)
    fx = run_warp_fwd(x, flows, mode)
    _, fmag, _ = B.pl_warp_ref(x, flows, mode)
    B.check_adjoint(f"warp m{mode} c{c} {h}x{w}", x, fx, dout, dx, B.bound_counted(fmag, B.ER_ROUNDINGS["warp_fwd"]), r["dx_bound"],
                    f"warp_bwd_m{mode}")


# ----------------------------------------------------------------------------------------------------------------------- resize
def run_resize_fwd(x, out_hw):
    nc, h, w = x.shape
    xd = _dev(x)
    out = Out(nc, *out_hw)
    _lib.check(L().eemop_resize_ac_fwd(xd.data_ptr(), out.ptr(), nc, h, w, out_hw[0], out_hw[1], _sp()))
    return out.cpu()


def run_resize_bwd(dout, in_hw):
    nc, oh, ow = dout.shape
    dd = _dev(dout)
    dx = Out(nc, *in_hw)
    _lib.check(L().eemop_resize_ac_bwd(dd.data_ptr(), dx.ptr(), nc, in_hw[0], in_hw[1], oh, ow, _sp()))
    return dx.cpu()


@pytest.mark.parametrize("in_hw,out_hw", B.OB_RESIZE_CASES)
def test_resize_ac_fwd_and_both_adjoints(monkeypatch, in_hw, out_hw):
    g = _g("resize", in_hw, out_hw)
    x = torch.randn(4, *in_hw, generator=g)
    dout = B.random_sign((4, *out_hw), g)
    _pin(monkeypatch)
    fx = run_resize_fwd(x, out_hw)
    ran("resize_ac")
    ref, mag = B.ob_resize_ref(x, out_hw)
    B.check_roundings(f"resize {in_hw}->{out_hw}", fx, ref, mag, "resize_ac", form="resize_ac")
    for form, runs in (("resize_ac_bwd_gather", 1), ("resize_ac_bwd_scatter", 4)):
        _pin(monkeypatch, {"EEM_RESIZE_BWD_SCATTER": "1"} if form.endswith("scatter") else {})
        for _ in range(runs):
            dx = run_resize_bwd(dout, in_hw)
            ran(form)
            bound = B.ob_check_resize_bwd(f"resize_bwd {in_hw}<-{out_hw}", dx, dout, in_hw, form)
        B.check_adjoint(f"resize {in_hw}->{out_hw}", x, fx, dout, dx, B.bound_counted(mag, B.ER_ROUNDINGS["resize_ac"]), bound, form)


def test_upsample_flow_as_function(monkeypatch):
    """ops.UpsampleFlowAs with rates that are no power of two: res (the blend times ow / w, oh / h), scaled, and dx through both outputs."""
    _pin(monkeypatch)
    g = _g("upsample_flow_as")
    (h, w), (oh, ow) = (5, 7), (12, 17)
    x = torch.randn(2, 2, h, w, generator=g)
    dres, dsc = B.random_sign((2, 2, oh, ow), g), B.random_sign((2, 2, h, w), g)
    xd = _dev(x).requires_grad_(True)
    res, scaled = ops.UpsampleFlowAs.apply(xd, oh, ow)
    torch.autograd.backward([res, scaled], [_dev(dres), _dev(dsc)])
    torch.cuda.synchronize()
    ref, mag = B.pl_upflow_ref(x, (oh, ow), rate=True)
    B.check_roundings("flow_as.res", res.detach().cpu(), ref, mag, "upflow_rate", form="resize_ac")
    ref, mag = B.pl_scale_ref(x, (oh, ow))
    B.check_roundings("flow_as.scaled", scaled.detach().cpu(), ref, mag, "scale", form="scale_flow")
    su, sv = B.pl_rate((oh, ow), (h, w))
    s = torch.tensor([su, sv], dtype=torch.float64).view(1, 2, 1, 1)
    bref, bmag, n = B.ob_resize_bwd_ref(B._d(dres) * s, (h, w))
    # a contribution passes the rate's product and the gather's six roundings; then N - 1 sums, the scaled branch's product and the sum of the two
    k = B.ER_ROUNDINGS["resize_ac_bwd_gather"] + 1 + (n - 1).clamp_min(0) + 1
    B.check_counted("flow_as.dx", xd.grad.cpu(), bref + B._d(dsc) * s, bmag + (B._d(dsc) * s).abs(), k, "resize_ac_bwd_gather")


# ----------------------------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("hw", B.OB_INSTNORM_HW)
@pytest.mark.parametrize("relu", [0, 1])
def test_instnorm_bwd(monkeypatch, relu, hw):
    _pin(monkeypatch)
    x = B.ob_norm_input(1, 3, hw, B.ob_seed("instnorm", hw))[0]
    y = B.ob_gated_output(F.instance_norm(x[None], eps=1e-5)[0] if hw > 1 else x * 0, B.ob_seed("instnorm.y", hw))
    dy = B.random_sign((3, hw), _g("instnorm.dy", hw))
    xd, yd, dd = _dev(x), _dev(y), _dev(dy)
    dx = Out(3, hw)
    _lib.check(L().eemop_instnorm_bwd(xd.data_ptr(), yd.data_ptr(), dd.data_ptr(), 3, hw, relu, dx.ptr(), _sp()))
    form = "instnorm_bwd_t1024" if hw >= 16384 else "instnorm_bwd_t256"
    ran(form)
    B.ob_check_planes(f"instnorm_bwd hw{hw} relu{relu}", dx.cpu(), B.ob_instnorm_bwd_ref(x, y, dy, relu),
                      B.ob_instnorm_bwd_ref(x, y, dy, relu, dtype=torch.float32), form, 0)


def _bn_case(n, c, hw, relu):
    g = _g("bn", n, c, hw, relu)
    x = B.ob_norm_input(n, c, hw, B.ob_seed("bn.x", n, c, hw), constant=False)
    w, b = torch.randn(c, generator=g), torch.randn(c, generator=g)
    w[0] = 0.0
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return x, w, b, rm, rv, g


@pytest.mark.parametrize("n,c,hw", B.OB_BN_CASES)
@pytest.mark.parametrize("relu", [0, 1])
def test_batchnorm_train_and_eval(monkeypatch, relu, n, c, hw):
    _pin(monkeypatch)
    x, w, b, rm, rv, g = _bn_case(n, c, hw, relu)
    mom, eps = 0.1, 1e-5
    t = "t1024" if n * hw >= 16384 else "t256"
    name = f"bn n{n} c{c} hw{hw} relu{relu}"
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    # training forward
    refs = B.ob_bn_train_fwd_ref(x, w, b, rm, rv, mom, eps, relu)
    y, sm, sr = Out(n, c, hw), Out(c), Out(c)
    rmo, rvo = Out(c, init=_dev(rm)), Out(c, init=_dev(rv))
    _lib.check(L().eemop_batchnorm_train_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rmo.ptr(), rvo.ptr(), n, c, hw, mom, eps, relu, y.ptr(),
                                             sm.ptr(), sr.ptr(), _sp()))
    ran(f"bn_train_fwd_{t}")
    got = {"save_mean": sm.cpu(), "save_rstd": sr.cpu(), "running_mean": rmo.cpu(), "running_var": rvo.cpu()}
    B.ob_check_counted_map(name + " train_fwd", got, refs, f"bn_train_fwd_{t}", tuple(got))
    B.ob_check_planes(name + " train_fwd.y", y.cpu(), refs["y"], refs["y32"], f"bn_train_fwd_{t}", 1)
    # training backward on a stored output and saved statistics of the case's own
    yy = B.ob_gated_output(refs["y32"], B.ob_seed("bn.y", n, c, hw))
    dy = B.random_sign((n, c, hw), g)
    smf, srf = refs["save_mean"][0].float(), refs["save_rstd"][0].float()
    yd, dd, smd, srd = _dev(yy), _dev(dy), _dev(smf), _dev(srf)
    dx, dw, db = Out(n, c, hw), Out(c), Out(c)
    _lib.check(L().eemop_batchnorm_train_bwd(xd.data_ptr(), yd.data_ptr(), dd.data_ptr(), wd.data_ptr(), smd.data_ptr(), srd.data_ptr(),
                                             n, c, hw, relu, dx.ptr(), dw.ptr(), db.ptr(), _sp()))
    ran(f"bn_train_bwd_{t}")
    r = B.ob_bn_train_bwd_ref(x, yy, dy, w, smf, srf, relu)
    B.ob_check_counted_map(name + " train_bwd", {"dweight": dw.cpu(), "dbias": db.cpu()}, r, f"bn_train_bwd_{t}", ("dweight", "dbias"))
    B.ob_check_planes(name + " train_bwd.dx", dx.cpu(), r["dx"], r["dx32"], f"bn_train_bwd_{t}", 1)
    # eval forward and backward, the last channel's running variance near 0
    rv2 = rv.clone()
    rv2[c - 1] = 1e-7
    rmd, rvd = _dev(rm), _dev(rv2)
    ye = Out(n, c, hw)
    _lib.check(L().eemop_batchnorm_eval_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), n, c, hw, eps, relu, ye.ptr(),
                                            _sp()))
    ran(f"bn_eval_fwd_{t}")
    B.check_roundings(name + " eval_fwd.y", ye.cpu(), B.ob_bn_eval_fwd_ref(x, w, b, rm, rv2, eps, relu), B.ob_bn_eval_fwd_mag(x, w, b, rm, rv2, eps),
                      "bn_eval_y", form=f"bn_eval_fwd_{t}")
    B.ob_check_planes(name + " eval_fwd.y", ye.cpu(), B.ob_bn_eval_fwd_ref(x, w, b, rm, rv2, eps, relu),
                      B.ob_bn_eval_fwd_ref(x, w, b, rm, rv2, eps, relu, dtype=torch.float32), f"bn_eval_fwd_{t}", 1)
    dx, dw, db = Out(n, c, hw), Out(c), Out(c)
    _lib.check(L().eemop_batchnorm_eval_bwd(xd.data_ptr(), yd.data_ptr(), dd.data_ptr(), wd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), n, c, hw, eps,
                                            relu, dx.ptr(), dw.ptr(), db.ptr(), _sp()))
    ran(f"bn_eval_bwd_{t}")
    e = B.ob_bn_eval_bwd_ref(x, yy, dy, w, rm, rv2, eps, relu)
    B.ob_check_counted_map(name + " eval_bwd", {"dweight": dw.cpu(), "dbias": db.cpu()}, e, f"bn_eval_bwd_{t}", ("dweight", "dbias"))
    B.ob_check_planes(name + " eval_bwd.dx", dx.cpu(), e["dx"], e["dx32"], f"bn_eval_bwd_{t}", 1)


# ----------------------------------------------------------------------------------------------------------------------- elementwise
@pytest.mark.parametrize("n", B.OB_ELEMENTWISE_N)
def test_elementwise(monkeypatch, n):
    _pin(monkeypatch)
    g = _g("elementwise", n)
    dy, v = B.random_sign((n,), g), torch.randn(n, generator=g)
    y = B.ob_gated_output(v, B.ob_seed("elementwise.y", n))
    dd = _dev(dy)
    for kind, yy, scale in ((B.GACT_RELU, y, 1.7), (B.GACT_LEAKY, y, 0.25), (B.GACT_SIGMOID, torch.sigmoid(v), 1.7), (B.GACT_TANH, torch.tanh(v), 1.7),
                            (B.GACT_NONE, v, 0.25)):
        out, yd = Out(n), _dev(yy)
        _lib.check(L().eemop_act_bwd(dd.data_ptr(), yd.data_ptr(), n, kind, scale, out.ptr(), _sp()))
        ran("act_bwd")
        ref, mag, kk = B.ob_act_bwd_ref(dy, yy, kind, scale)
        B.check_roundings(f"act_bwd kind{kind} n{n}", out.cpu(), ref, mag, kk, form="act_bwd")
    for kind, ref in ((B.GACT_RELU, torch.relu(v)), (B.GACT_LEAKY, torch.where(v > 0, v, v * torch.tensor(B.LEAKY, dtype=torch.float32))), (B.GACT_NONE, v)):
        out, vd = Out(n), _dev(v)
        _lib.check(L().eemop_act_fwd(vd.data_ptr(), n, kind, out.ptr(), _sp()))
        ran("act_fwd")
        B.check_bitwise(f"act_fwd kind{kind} n{n}", out.cpu(), ref)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = _dev(a), _dev(b)
    for kind in range(5):
        out = Out(n)
        _lib.check(L().eemop_binary(kind, ad.data_ptr(), bd.data_ptr(), -0.3, n, out.ptr(), _sp()))
        ran("binary")
        ref, mag = B.ob_binary_ref(kind, a, b, -0.3)
        B.check_roundings(f"binary kind{kind} n{n}", out.cpu(), ref, mag, "binary", form="binary")
    z, h, q = torch.rand(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    zd, hd, qd = _dev(z), _dev(h), _dev(q)
    out = Out(n)
    _lib.check(L().eemop_gru_blend(zd.data_ptr(), hd.data_ptr(), qd.data_ptr(), n, out.ptr(), _sp()))
    ran("gru_blend")
    B.check_roundings(f"gru_blend n{n}", out.cpu(), *B.ob_gru_blend_ref(z, h, q), "gru_blend", form="gru_blend")
    dz, dh, dq = Out(n), Out(n), Out(n)
    _lib.check(L().eemop_gru_blend_bwd(dd.data_ptr(), zd.data_ptr(), hd.data_ptr(), qd.data_ptr(), n, dz.ptr(), dh.ptr(), dq.ptr(), _sp()))
    ran("gru_blend_bwd")
    for key, o in (("dz", dz), ("dh", dh), ("dq", dq)):
        ref, mag, kk = B.ob_gru_blend_bwd_ref(dy, z, h, q)[key]
        B.check_roundings(f"gru_blend_bwd.{key} n{n}", o.cpu(), ref, mag, kk, form="gru_blend_bwd")
    # scale_flow on [1, 2, n]: counted, and bitwise by a power of two
    fl = torch.randn(1, 2, n, generator=g)
    fld = _dev(fl)
    for su, sv in ((1.7, 0.3), (2.0, 0.5)):
        out = Out(1, 2, n)
        _lib.check(L().eemop_scale_flow(fld.data_ptr(), 1, n, su, sv, out.ptr(), _sp()))
        ran("scale_flow")
        ref, mag = B.ob_scale_flow_ref(fl, su, sv)
        B.check_roundings(f"scale_flow n{n}", out.cpu(), ref, mag, "scale", form="scale_flow")
        if su == 2.0:
            B.check_bitwise(f"scale_flow n{n} x2", out.cpu(), ref.float())


def test_zero_elements_launch_nothing(monkeypatch):
    """Every elementwise entry point returns EEM_OK on zero elements and launches nothing: the last form stays what it was and the
    buffers stay untouched."""
    _pin(monkeypatch)
    a = torch.ones(8, device=DEV)
    out = Out(8)
    _lib.check(L().eemop_binary(0, a.data_ptr(), a.data_ptr(), 0.0, 8, out.ptr(), _sp()))
    before = last_form()
    p, o, s = a.data_ptr(), out.ptr(), _sp()
    arr = (ctypes.c_void_p * 1)(p)
    calls = [lambda: L().eemop_act_fwd(p, 0, 1, o, s), lambda: L().eemop_act_bwd(p, p, 0, 1, 1.0, o, s), lambda: L().eemop_binary(0, p, p, 0.0, 0, o, s),
             lambda: L().eemop_sum_n(ctypes.cast(arr, ctypes.c_void_p), 1, 0, o, s), lambda: L().eemop_gru_blend(p, p, p, 0, o, s),
             lambda: L().eemop_gru_blend_bwd(p, p, p, p, 0, o, o, o, s), lambda: L().eemop_shuffle_channels(p, o, 0, 6, 3, 4, 0, s),
             lambda: L().eemop_scale_flow(p, 0, 4, 2.0, 2.0, o, s), lambda: L().eemop_pool2_bwd(p, o, 0, 2, 2, s),
             lambda: L().eemop_resize_ac_fwd(p, o, 0, 2, 2, 2, 2, s), lambda: L().eemop_resize_ac_bwd(p, o, 0, 2, 2, 2, 2, s)]
    for i, call in enumerate(calls):
        assert call() == 0, (i, L().eemflow_last_error())
        assert last_form() == before, i
    assert torch.equal(out.cpu(), torch.full((8,), 2.0))


@pytest.mark.parametrize("count", [1, 2, 7, 8])
@pytest.mark.parametrize("n", [3, 1026, 1027])
@pytest.mark.parametrize("aligned", [True, False])
def test_sum_n(monkeypatch, aligned, n, count):
    """aligned: the 16-byte path with its tail; else one input is a view one element into its allocation (the scalar path)."""
    _pin(monkeypatch)
    g = _g("sum_n", count, n)
    ts = [B.random_sign((n,), g) for _ in range(count)]
    dev = [_dev(t) for t in ts]
    if not aligned:
        hold = torch.empty(n + 1, device=DEV)
        hold[1:].copy_(dev[-1])
        dev[-1] = hold[1:]
    arr = (ctypes.c_void_p * count)(*[t.data_ptr() for t in dev])
    out = Out(n)
    _lib.check(L().eemop_sum_n(ctypes.cast(arr, ctypes.c_void_p), count, n, out.ptr(), _sp()))
    form = "sum_n_v4" if aligned else "sum_n_scalar"
    ran(form)
    ref, mag, k = B.ob_sum_ref(ts)
    B.check_counted(f"sum_n count{count} n{n}", out.cpu(), ref, mag, k, form)


@pytest.mark.parametrize("count", [9, 17])
def test_sum_tensors_of_more_than_eight(monkeypatch, count):
    _pin(monkeypatch)
    g = _g("sum_tensors", count)
    ts = [B.random_sign((3, 1027), g) for _ in range(count)]
    got = ops.sum_tensors([_dev(t) for t in ts])
    torch.cuda.synchronize()
    ref, mag, k = B.ob_sum_ref(ts)
    B.check_counted(f"sum_tensors {count}", got.cpu(), ref, mag, k, "sum_n_v4")


# ----------------------------------------------------------------------------------------------------------------------- copies
@pytest.mark.parametrize("h,w", [(7, 9), (2, 2), (3, 3)])
def test_pool2_bwd(monkeypatch, h, w):
    _pin(monkeypatch)
    g = _g("pool2", h, w)
    dy = B.random_sign((4, h // 2, w // 2), g)
    dx, dyd = Out(4, h, w), _dev(dy)
    _lib.check(L().eemop_pool2_bwd(dyd.data_ptr(), dx.ptr(), 4, h, w, _sp()))
    ran("pool2_bwd")
    got = dx.cpu()
    B.check_bitwise(f"pool2_bwd {h}x{w}", got, B.pool_bwd_ref(dy[None], (h, w), 2)[0][0].float())
    x = torch.randn(4, h, w, generator=g)
    fx, xd = Out(4, h // 2, w // 2), _dev(x)
    _lib.check(L().eemop_pool2_fwd(xd.data_ptr(), fx.ptr(), 4, h, w, _sp()))
    _, fmag = B.avg_pool_ref(x, 2)
    B.check_adjoint(f"pool2 {h}x{w}", x, fx.cpu(), dy, got, B.bound_counted(fmag, B.ER_ROUNDINGS["pool2_fwd"]), torch.zeros(4, h, w, dtype=torch.float64),
                    "pool2_bwd")


@pytest.mark.parametrize("groups", [3, 1])
@pytest.mark.parametrize("inverse", [0, 1])
def test_shuffle(monkeypatch, inverse, groups):
    _pin(monkeypatch)
    x = torch.randn(2, 6, 35, generator=_g("shuffle", groups))
    out, xd = Out(2, 6, 35), _dev(x)
    _lib.check(L().eemop_shuffle_channels(xd.data_ptr(), out.ptr(), 2, 6, groups, 35, inverse, _sp()))
    ran("shuffle")
    B.check_bitwise(f"shuffle g{groups} inv{inverse}", out.cpu(), B.ob_shuffle_ref(x, groups, inverse))


def test_copy_channels_into_and_out_of_a_slice(monkeypatch):
    _pin(monkeypatch)
    g = _g("copy_channels")
    src, wide = torch.randn(2, 3, 35, generator=g), torch.randn(2, 7, 35, generator=g)
    into, sd, wd = Out(2, 7, 35), _dev(src), _dev(wide)
    _lib.check(L().eemop_copy_channels(sd.data_ptr(), 3, 0, into.ptr(), 7, 2, 3, 2, 35, _sp()))
    ran("copy_channels")
    ref = torch.full((2, 7, 35), SENTINEL)
    ref[:, 2:5] = src
    B.check_bitwise("copy_channels into", into.cpu(), ref)
    outof = Out(2, 3, 35)
    _lib.check(L().eemop_copy_channels(wd.data_ptr(), 7, 4, outof.ptr(), 3, 0, 3, 2, 35, _sp()))
    ran("copy_channels")
    B.check_bitwise("copy_channels out of", outof.cpu(), wide[:, 4:7])


# ----------------------------------------------------------------------------------------------------------------------- the table
def test_every_form_in_the_table_ran():
    """Runs last: every name of OB_FORMS was reported by a launch above; prints the measured worst statistics per form."""
    agg = {}
    for rec in B.LOG:
        f = rec.get("form", "?")
        a = agg.setdefault(f, {"max_z": 0.0, "of_bound": 0.0, "rms_ratio": 0.0, "max_ratio": 0.0, "checks": 0})
        a["checks"] += 1
        for key in ("max_z", "of_bound", "rms_ratio", "max_ratio"):
            v = rec.get(key, 0.0)
            if isinstance(v, float) and math.isfinite(v):
                a[key] = max(a[key], abs(v))
    print("\n  form                              max|z|  of its bound  kappa rms  kappa max  checks")
    for f in sorted(agg):
        a = agg[f]
        print(f"  {f:32s} {a['max_z']:7.2f} {a['of_bound']:13.3f} {a['rms_ratio']:10.2f} {a['max_ratio']:10.2f} {a['checks']:7d}")
    assert SEEN == B.OB_FORMS, (sorted(B.OB_FORMS - SEEN), sorted(SEEN - B.OB_FORMS))
