"""Host-side checks of the gradient of the image of warped events (eemflow_amd/csrc/iwe_grad.hip, eemflow_amd.iwe.contrast_many /
fwl_loss): the explicit formula the kernels implement (tests/iwe_grad_reference.py) against torch autograd in fp64 and against a central
difference, AugPlan.event_map against apply_host, the C ABI's declarations, and the argument checks of the new entry points and of the
trainer's contrast term.  No GPU."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import eemflow_amd
from eemflow_amd import _lib
from eemflow_amd.augmentor import AugPlan, apply_host, event_map_after_offset, resize_linear
from eemflow_amd.harness import Logger, TrainRaftEvents

from iwe_grad_reference import grad_reference, integer_distance, map_events, variance_autograd, variance_fp64, warped_positions
from iwe_reference import metric_refs

iwe = importlib.import_module("eemflow_amd.iwe")        # (the package's attribute `iwe` is the one-job function)
HERE = os.path.dirname(os.path.abspath(__file__))


def wavy_flow(h, w, seed):
    """A smooth non-separable flow of a few pixels, fp32 values held in fp64."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    a = rng.uniform(0, 2 * math.pi, 4)
    u = 3.0 * np.sin(2 * math.pi * x + a[0]) * np.cos(2 * math.pi * y + a[1]) + 1.0
    v = 2.5 * np.cos(2 * math.pi * x + a[2]) * np.sin(2 * math.pi * y + a[3]) - 0.5
    return torch.from_numpy(np.stack([u, v])).float().double()


def fractional_events(seed, n, h, w):
    """Time-sorted events with fractional coordinates up to 2 px outside the frame on every side."""
    rng = np.random.default_rng(seed)
    t = np.sort(np.round(rng.uniform(0, 0.05, n) * 1e6) * 1e-6)
    x, y = rng.uniform(-2.0, w + 1.0, n), rng.uniform(-2.0, h + 1.0, n)
    p = rng.integers(0, 2, n) * 2.0 - 1.0
    return torch.from_numpy(np.stack([t, x, y, p], axis=1))


@pytest.mark.parametrize("h,w,n", [(9, 12, 600), (37, 50, 5000)])
@pytest.mark.parametrize("amap", [(1.0, 0.0, 1.0, 0.0), (-1.0, 10.25, 1.0, -1.5)])
def test_formula_equals_autograd_with_straight_through_rounding(h, w, n, amap):
    """The explicit formula against torch autograd in fp64 through warp_direct and accumulate, the image's fp32 rounding
    straight-through: 1e-12 relative to the largest gradient."""
    ev = fractional_events(11 + h, n, h, w)
    flow = wavy_flow(h, w, 5).requires_grad_(True)
    for t_ref in ("end", "start"):
        t0, scale = metric_refs(ev, t_ref)
        var, image32, moments = variance_autograd(ev, flow, t0, scale, amap)
        (auto,) = torch.autograd.grad(var, flow)
        coef = -0.37
        ref, A = grad_reference(ev, flow.detach(), image32, moments, coef, t0, scale, amap)
        big = float(auto.abs().max())
        assert big > 1e-3                                          # (a real gradient, not zeros against zeros)
        assert float((ref - coef * auto).abs().max()) <= 1e-12 * abs(coef) * big
        assert bool((A + 1e-300 >= ref.abs() * (1 - 1e-9)).all())      # the abs-sum map bounds the gradient cell by cell


def test_directional_derivative_equals_a_central_difference():
    """<gradient, d> of the fp64 variance against (var(F + eps d) - var(F - eps d)) / (2 eps) along a random direction.  Away from
    integer warped positions var is a polynomial of degree four in eps, so the central difference is off by O(eps^2) relative
    (eps = 1e-4: 1e-8) and by the cancellation 2^-53 var / eps (1e-12 relative); 1e-6 relative is asserted."""
    h, w, eps = 21, 30, 1e-4
    ev = fractional_events(4, 3000, h, w)
    flow = wavy_flow(h, w, 9)
    d = torch.from_numpy(np.random.default_rng(1).standard_normal((2, h, w)))
    t0, scale = metric_refs(ev, "end")
    keep = torch.ones(ev.shape[0], dtype=torch.bool)
    for f in (flow + eps * d, flow - eps * d, flow):               # build the case: drop events that come near an integer
        xw, yw = warped_positions(ev, f, t0, scale)
        keep &= ((xw - torch.round(xw)).abs() > 2e-3) & ((yw - torch.round(yw)).abs() > 2e-3)
    ev = ev[keep].contiguous()
    assert ev.shape[0] > 2000
    t0, scale = metric_refs(ev, "end")
    for f in (flow + eps * d, flow - eps * d):                     # the precondition, on the case as it is used
        assert integer_distance(ev, f, t0, scale) >= 1e-3
    # no cell is crossed between the probe points: the same floor at both
    xa, ya = warped_positions(ev, flow + eps * d, t0, scale)
    xb, yb = warped_positions(ev, flow - eps * d, t0, scale)
    assert bool((torch.floor(xa) == torch.floor(xb)).all() and (torch.floor(ya) == torch.floor(yb)).all())
    image = variance_image(ev, flow, t0, scale)
    S = image[0] + image[1]
    moments = [float(h * w), float(S.sum()), float((S * S).sum())]
    grad, _ = grad_reference(ev, flow, image, moments, 1.0, t0, scale)
    analytic = float((grad * d).sum())
    numeric = float(variance_fp64(ev, flow + eps * d, t0, scale) - variance_fp64(ev, flow - eps * d, t0, scale)) / (2 * eps)
    assert abs(analytic) > 1e-3
    assert abs(analytic - numeric) <= 1e-6 * abs(analytic)


def variance_image(ev, flow, t0, scale):
    from iwe_reference import accumulate
    xw, yw = warped_positions(ev, flow, t0, scale)
    return accumulate(xw, yw, ev[:, 3].double(), flow.shape[-2], flow.shape[-1])[0]


def count_image(x, y, h, w):
    img = np.zeros((h, w, 1))
    ok = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    np.add.at(img, (y[ok].astype(int), x[ok].astype(int), 0), 1.0)
    return img


@pytest.mark.parametrize("hflip", [False, True])
@pytest.mark.parametrize("vflip", [False, True])
@pytest.mark.parametrize("crop", [None, (9, 14, 3, 5)])
def test_event_map_of_flips_and_crops_is_apply_host_of_the_count_image(hflip, vflip, crop):
    h, w = 17, 23
    rng = np.random.default_rng(8)
    x, y = rng.integers(0, w, 400).astype(np.float64), rng.integers(0, h, 400).astype(np.float64)
    plan = AugPlan(h, w, hflip=hflip, vflip=vflip) if crop is None else \
        AugPlan(h, w, crop=crop[:2], y0=crop[2], x0=crop[3], hflip=hflip, vflip=vflip)
    ax, bx, ay, by = plan.event_map(h, w)
    img = count_image(x, y, h, w)
    want, _ = apply_host(plan, img, np.zeros((h, w, 2)))
    ch, cw = plan.crop
    got = count_image(ax * x + bx, ay * y + by, ch, cw)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got.sum() > 0
    with pytest.raises(ValueError, match="drawn for"):
        plan.event_map(h + 1, w)


def test_event_map_of_a_resize_inverts_resize_linears_sample_positions():
    h, w, fx, fy = 20, 30, 1.3, 0.8
    rh, rw = int(round(h * fy)), int(round(w * fx))
    plan = AugPlan(rh, rw, resized=True, scale_x=fx, scale_y=fy)
    ax, bx, ay, by = plan.event_map(h, w)
    dx, dy = np.arange(rw, dtype=np.float64), np.arange(rh, dtype=np.float64)
    sx, sy = (dx + 0.5) / fx - 0.5, (dy + 0.5) / fy - 0.5          # where resize_linear samples the source for destination pixel d
    assert np.abs(ax * sx + bx - dx).max() < 1e-12 and np.abs(ay * sy + by - dy).max() < 1e-12
    # and on pixels: a ramp resized is the ramp of the mapped coordinate (linear interpolation is exact on a ramp, away from the clamp)
    ramp = np.tile(np.arange(w, dtype=np.float64), (h, 1))[:, :, None]
    out = resize_linear(ramp, fx, fy)[:, :, 0]
    inner = (sx >= 0) & (sx <= w - 1)
    assert np.abs(ax * out[0, inner] + bx - dx[inner]).max() < 1e-9
    # resize, then flip, then crop - apply_host's order
    full = AugPlan(rh, rw, crop=(8, 10), y0=2, x0=4, hflip=True, vflip=True, resized=True, scale_x=fx, scale_y=fy)
    fa = full.event_map(h, w)
    assert fa == (-ax, (rw - 1) - bx - 4, -ay, (rh - 1) - by - 2)
    # behind a dataset's own offset
    assert event_map_after_offset(None, (3, 2), h, w) == (1.0, -3.0, 1.0, -2.0)
    assert event_map_after_offset(AugPlan(h, w, hflip=True), (3, 2), h, w) == (-1.0, (w - 1) + 3.0, 1.0, -2.0)


def test_abi_is_declared_with_its_replaces_lines():
    header = open(os.path.join(HERE, "..", "include", "eemflow_hip.h")).read()
    for name in ("eemflow_iwe_map_many", "eemflow_iwe_grad_many"):
        assert name in _lib.EXPORTS
        at = header.index(name + "(")
        comment = header[header.rindex("/*", 0, at):at]
        assert "Replaces:" in comment and "utils_luo/event_utils.py:9-51" in comment
    from eemflow_amd.build import EXTRA, SOURCES
    assert "iwe_grad.hip" in SOURCES and "-ffp-contract=off" in EXTRA["iwe_grad.hip"]
    csrc = os.path.join(HERE, "..", "eemflow_amd", "csrc")
    for src in ("iwe.hip", "iwe_grad.hip"):                        # one set of per-event device functions
        text = open(os.path.join(csrc, src)).read()
        assert '#include "iwe_shared.h"' in text and "void iwe_sample(" not in text
    assert eemflow_amd.contrast_many is iwe.contrast_many and eemflow_amd.fwl_loss is iwe.fwl_loss
    assert "no gradient" not in iwe.__doc__


class Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the shape and dtype checks run without one."""
    is_cuda = True


def cuda(t):
    return t.as_subclass(Cuda)


def test_argument_validation_of_contrast_many_and_fwl_loss():
    ev, flow = torch.zeros(5, 4, dtype=torch.float64), torch.zeros(2, 8, 8)
    for call in (lambda: iwe.contrast_many([ev], [flow]), lambda: iwe.fwl_loss([ev, ev], [flow, flow])):
        with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
            call()
    for fn in (iwe.contrast_many, iwe.fwl_loss):
        with pytest.raises(ValueError, match=r"\(N,4\) float64"):
            fn([cuda(ev.float())], [cuda(flow)])
        with pytest.raises(ValueError, match=r"\(2,H,W\) float32"):
            fn([cuda(ev)], [cuda(flow.double())])
        with pytest.raises(ValueError, match="one .2,H,W. shape"):
            fn([cuda(ev), cuda(ev)], [cuda(flow), cuda(torch.zeros(2, 8, 9))])
        with pytest.raises(ValueError, match="one flow"):
            fn([cuda(ev), cuda(ev)], [cuda(flow)])
        with pytest.raises(ValueError, match="t_ref"):
            fn([cuda(ev)], [cuda(flow)], t_ref="middle")
        with pytest.raises(ValueError, match="offset"):
            fn([cuda(ev)], [cuda(flow)], offset=3)
        with pytest.raises(ValueError, match="one map"):
            fn([cuda(ev)], [cuda(flow)], maps=[(1, 0, 1, 0), (1, 0, 1, 0)])
        with pytest.raises(ValueError, match=r"\(ax, bx, ay, by\)"):
            fn([cuda(ev)], [cuda(flow)], maps=[(1, 0, 1)])
        with pytest.raises(TypeError):
            fn([np.zeros((5, 4))], [cuda(flow)])
    with pytest.raises(ValueError, match="needs its flow"):
        iwe.fwl_loss([cuda(ev)], [None])
    with pytest.raises(ValueError, match="size="):
        iwe.contrast_many([cuda(ev)], [None])
    from eemflow_amd.train import contrast_loss
    with pytest.raises(ValueError, match=r"\(B,2,H,W\)"):
        contrast_loss(torch.zeros(2, 8, 8), [ev])
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        contrast_loss(torch.zeros(1, 2, 8, 8), [ev])
    with pytest.raises(ValueError, match="one event set per sample"):
        contrast_loss(cuda(torch.zeros(2, 2, 8, 8)), [ev])


def test_trainer_refuses_what_the_contrast_term_cannot_do():
    with pytest.raises(ValueError, match="autograd"):              # the fused engine with a weight
        TrainRaftEvents([], (64, 64), engine="fused", contrast_weight=0.5, logger=Logger(verbose=False))
    with pytest.raises(ValueError, match="autograd"):
        TrainRaftEvents([], (64, 64), engine="fused", contrast_weight=0.5, supervised=False, logger=Logger(verbose=False))
    with pytest.raises(ValueError, match="no loss"):
        TrainRaftEvents([], (64, 64), engine="autograd", supervised=False, logger=Logger(verbose=False))
    tr = TrainRaftEvents([], (64, 64), engine="autograd", contrast_weight=0.5, logger=Logger(verbose=False))
    assert tr.contrast_weight == 0.5 and tr.supervised
    assert TrainRaftEvents([], (64, 64), logger=Logger(verbose=False)).contrast_weight == 0.0
    volume = torch.zeros(2, 5, 64, 64)
    with pytest.raises(ValueError, match="with_events"):           # batches without events
        tr._contrast_term(torch.zeros(2, 2, 64, 64), {"event_volume_old": volume}, volume)
    ev = torch.zeros(5, 4, dtype=torch.float64)
    batch = {"event_volume_old": volume, "events": [ev, ev], "events_offset": [(0, 0), (3, 1)]}
    with pytest.raises(ValueError, match="out_mesh_size"):         # a mesh-size prediction
        tr._contrast_term(torch.zeros(2, 2, 16, 16), batch, volume)
    assert tr._contrast_inputs(batch)[1] == [(1.0, -0.0, 1.0, -0.0), (1.0, -3.0, 1.0, -1.0)]
    batch["events_map"] = [(-1.0, 63.0, 1.0, 0.0)] * 2
    assert tr._contrast_inputs(batch)[1] == batch["events_map"]


def test_parser_takes_the_contrast_options():
    from eemflow_amd import cli
    args = cli.build_parser().parse_args(["train"])
    assert args.contrast_weight == 0.0 and args.self_supervised is False
    args = cli.build_parser().parse_args(["train", "--contrast_weight", "0.5", "--self_supervised"])
    assert args.contrast_weight == 0.5 and args.self_supervised is True
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["test", "--contrast_weight", "0.5"])
    args = cli.build_parser().parse_args(["train", "--self_supervised"])
    with pytest.raises(SystemExit, match="contrast_weight"):
        cli.train(args)
