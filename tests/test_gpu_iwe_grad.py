"""The gradient of the image of warped events (csrc/iwe_grad.hip, eemflow_amd.iwe.contrast_many / fwl_loss, train.contrast_loss and the
trainer's contrast term) on the GPU, in both kernel forms - binned (the default) and direct (EEM_IWE_DIRECT=1) - against the fp64
restatement of tests/iwe_grad_reference.py.  Needs a real MI355X: `pytest -m gpu`.

Teacher forcing.  The reference takes the library's own stored image and moments, so only the gradient's arithmetic is compared.

Bound, per cell: |d| <= c_A * A + 2^-23 |ref| + 1e-12 max|ref|, A the abs-sum map of the cell's contributions.  A form that rounded
every gathered G and every contribution to fp32 - two stacked roundings of 2^-24 - would be held to c_A = 2^-22.  Neither form built
stores G (an event computes it in fp64 from the stored image, the same expression as the reference: the same bits), so the bound is
tighter:
  binned   c_A = 2^-23: a contribution is rounded to fp32 once when its record is made (2^-24 relative), with the same factor two of
           slack that 2^-22 has over two stacked roundings;
  direct   c_A = 2^-40: nothing is rounded before the fp64 sum; what is left are a few fp64 roundings per contribution (the order of
           the factors) and the order of the sum, n * 2^-53.
2^-23 |ref| is the one rounding of the fp64 sum to fp32 (half an ulp, doubled).  The cases keep every warped position at least 1e-6
from an integer (asserted on the reference), so that no event changes cell between library and reference; the integer convention has
its own test."""
import hashlib
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from eemflow_amd.augmentor import AugPlan, event_map_after_offset
from eemflow_amd.harness import Logger, TrainRaftEvents
from eemflow_amd import train as hip_train
from eemflow_amd.weights import seeded_state_dict, synthetic_gt, synthetic_voxel_pair

from iwe_grad_reference import grad_reference, integer_distance, map_events, warped_positions
from iwe_reference import metric_refs, separable_flow

iwe = importlib.import_module("eemflow_amd.iwe")        # (the package's attribute `iwe` is the one-job function)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iwe_forward_bits.json")
# name -> (H, W, N, fractional coordinates)
SHAPES = {"37x50": (37, 50, 5000, False), "64x61": (64, 61, 5000, True), "8x1280": (8, 1280, 3000, False),
          "260x346": (260, 346, 50000, False), "720x1280": (720, 1280, 200000, False),
          "241x40": (241, 40, 5000, True)}               # rows = 2 per band, 121 bands, the last of them one row: the short last band
C_A = {"binned": 2.0 ** -23, "direct": 2.0 ** -40}
IDENTITY = (1.0, 0.0, 1.0, 0.0)


@pytest.fixture(params=["binned", "direct"])
def form(request, monkeypatch):
    if request.param == "direct":
        monkeypatch.setenv("EEM_IWE_DIRECT", "1")
    else:
        monkeypatch.delenv("EEM_IWE_DIRECT", raising=False)
    return request.param


def smooth_flow(h, w):
    y, x = torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64)
    return separable_flow((6.0 * torch.sin(2 * math.pi * x / w) + 2.0).float(), (4.0 * torch.cos(2 * math.pi * y / h)).float())


def wavy_flow(h, w, seed=5):
    """A smooth flow whose two channels depend on x and y both."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    a = rng.uniform(0, 2 * math.pi, 4)
    u = 5.0 * np.sin(2 * math.pi * x + a[0]) * np.cos(2 * math.pi * y + a[1]) + 1.5
    v = 3.5 * np.cos(2 * math.pi * x + a[2]) * np.sin(2 * math.pi * y + a[3]) - 0.75
    return torch.from_numpy(np.stack([u, v])).float()


def raw_events(seed, n, h, w, fractional=False, span=0.05):
    rng = np.random.default_rng(seed)
    t = np.sort(np.round(rng.uniform(0, span, n) * 1e6) * 1e-6)
    if fractional:                                       # up to 2 px outside the frame on every side
        x, y = rng.uniform(-2.0, w + 1.0, n), rng.uniform(-2.0, h + 1.0, n)
    else:
        x, y = rng.integers(0, w, n).astype(np.float64), rng.integers(0, h, n).astype(np.float64)
    p = rng.integers(0, 2, n) * 2.0 - 1.0
    return torch.from_numpy(np.stack([t, x, y, p], axis=1))


def off_integer_events(seed, n, h, w, flow, fractional=False, amap=IDENTITY):
    """Events none of whose warped positions, under either time reference, comes within 2e-6 of an integer.  Integer coordinates put
    the events at the reference time (tau = 0) exactly on integers, so the events at the two end times get a fractional position; the
    others that come close (a zero of the flow) are left out - the end times, which set t0 and the span, stay."""
    ev = raw_events(seed, n, h, w, fractional)
    ends = (ev[:, 0] == ev[0, 0]) | (ev[:, 0] == ev[-1, 0])
    if not fractional:
        ev[ends, 1] += 0.37
        ev[ends, 2] += 0.41
    keep = torch.ones(ev.shape[0], dtype=torch.bool)
    for t_ref in ("end", "start"):
        t0, scale = metric_refs(ev, t_ref)
        xw, yw = warped_positions(ev, flow, t0, scale, amap)
        for v in (xw, yw):
            keep &= ~((v - torch.round(v)).abs() < 2e-6)
    assert bool(keep[ends].all())
    return ev[keep].contiguous()


_cases = {}


def case(name):
    """(events, flow, h, w) of a shape, built once."""
    if name not in _cases:
        h, w, n, fractional = SHAPES[name]
        flow = smooth_flow(h, w)
        _cases[name] = (off_integer_events(7, n, h, w, flow, fractional), flow, h, w)
    return _cases[name]


def forward(events, flows, t_ref="end", maps=None):
    """The library's forward of some jobs on CPU inputs: what the backward is teacher-forced with."""
    evs = [e.to(DEV) for e in events]
    fls = [f.to(DEV) if f is not None else None for f in flows]
    shape = next(f.shape for f in flows if f is not None)
    refs = [metric_refs(e, t_ref) for e in events]
    t0s, scales = [r[0] for r in refs], [r[1] for r in refs]
    maps = list(maps) if maps is not None else [IDENTITY] * len(evs)
    images, moments = iwe._launch_maps(evs, fls, t0s, scales, maps, shape[1], shape[2], torch.device(DEV))
    return evs, fls, t0s, scales, maps, images, moments


def library_gradients(events, flows, coefs, t_ref="end", maps=None):
    """(gradients, images, moments, t0s, scales) on the CPU; a None flow has gradient None."""
    evs, fls, t0s, scales, maps, images, moments = forward(events, flows, t_ref, maps)
    coef = torch.tensor(coefs, dtype=torch.float64, device=DEV)
    grads = iwe.iwe_grad_many(evs, fls, t0s, scales, maps, images, moments, coef)
    torch.cuda.synchronize()
    return ([g.cpu() if g is not None else None for g in grads], [i.cpu() for i in images], moments.cpu(), t0s, scales)


def check(form, got, events, flow, image, moments, coef, t0, scale, amap=IDENTITY, slack=1.0, what=""):
    """One job's gradient against the reference within the bound of the module docstring; returns the reference."""
    ref, A = grad_reference(events, flow, image, moments.tolist(), coef, t0, scale, amap)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), what
    big = float(ref.abs().max())
    bound = slack * (C_A[form] * A + 2.0 ** -23 * ref.abs() + 1e-12 * big)
    d = (got.double() - ref).abs()
    worst = float((d / (bound + 1e-300)).max())
    print(f"{what} {form}: max|ref| {big:.3e} max|d| {float(d.max()):.3e} worst |d|/bound {worst:.3f}")
    assert bool((d <= bound).all()), (what, form, float(d.max()), worst)
    return ref


@pytest.mark.parametrize("t_ref", ["end", "start"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_teacher_forced_gradient(form, name, t_ref):
    ev, flow, h, w = case(name)
    t0, scale = metric_refs(ev, t_ref)
    assert integer_distance(ev, flow, t0, scale) >= 1e-6
    coef = -0.8
    grads, images, moments, t0s, scales = library_gradients([ev], [flow], [coef], t_ref)
    ref = check(form, grads[0], ev, flow, images[0], moments[0], coef, t0s[0], scales[0], what=f"{name} {t_ref}")
    assert float(ref.abs().max()) > 0


def test_integer_warped_positions_take_the_left_pair_with_zero_weight(form):
    """Dyadic inputs put warped positions exactly on integers: the derivative is that of the pair (X0, X0 + 1) with gx = 0 - what the
    forward's floor gives, and autograd through xw - floor(xw)."""
    h, w = 12, 16
    rng = np.random.default_rng(3)
    n = 600
    t = np.sort(rng.integers(0, 5, n) / 4.0)                       # 0, 1/4 .. 1: tau = 1 - t is dyadic
    t[0], t[-1] = 0.0, 1.0
    x, y = rng.integers(0, w, n).astype(np.float64), rng.integers(0, h, n).astype(np.float64)
    ev = torch.from_numpy(np.stack([t, x, y, rng.integers(0, 2, n) * 2.0 - 1.0], axis=1))
    flow = torch.stack([torch.full((h, w), 4.0), torch.full((h, w), -8.0)])      # u tau and v tau are integers
    t0, scale = metric_refs(ev, "end")
    xw, yw = warped_positions(ev, flow, t0, scale)
    assert bool((xw == torch.round(xw)).all() and (yw == torch.round(yw)).all())
    grads, images, moments, t0s, scales = library_gradients([ev], [flow], [1.0])
    ref = check(form, grads[0], ev, flow, images[0], moments[0], 1.0, t0s[0], scales[0], what="integer positions")
    assert float(ref.abs().max()) > 0


def test_flip_map_with_crop_equals_explicitly_transformed_events(form):
    h, w = 37, 50
    flow = wavy_flow(h, w)
    plan = AugPlan(45, 64, crop=(h, w), y0=5, x0=9, hflip=True)
    amap = event_map_after_offset(plan, (2, 1), 45, 64)
    assert amap[0] == -1.0 and amap[2] == 1.0
    ev = off_integer_events(21, 6000, 45 + 1, 64 + 2, flow, fractional=True, amap=amap)
    moved = map_events(ev, amap)
    ga, ia, ma, t0s, scales = library_gradients([ev], [flow], [0.6], maps=[amap])
    gb, ib, mb, _, _ = library_gradients([moved], [flow], [0.6])
    assert torch.equal(ia[0], ib[0]) and torch.equal(ma, mb)      # -1 * x + b on the device is the host's: the same image
    ref = check(form, ga[0], moved, flow, ia[0], ma[0], 0.6, t0s[0], scales[0], what="flip map")
    check(form, gb[0], moved, flow, ia[0], ma[0], 0.6, t0s[0], scales[0], what="moved events")
    check(form, ga[0], ev, flow, ia[0], ma[0], 0.6, t0s[0], scales[0], amap=amap, what="flip map, mapped reference")
    assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("k", [16, 32])
def test_jobs_of_one_call_equal_one_job_calls(form, k):
    """k jobs of different sizes in one call, a zero-flow job and an empty set among them: every job's gradient is its one-job
    call's within the bound (twice: two runs, each within it), a None job has no gradient and disturbs no neighbour's."""
    h, w = 37, 50
    flows = [wavy_flow(h, w, seed=30 + i) for i in range(k)]
    events = [off_integer_events(40 + i, 300 + 137 * i, h, w, flows[i], fractional=i % 2 == 0) for i in range(k)]
    flows[3] = None
    events[5] = torch.zeros(0, 4, dtype=torch.float64)
    coefs = [(-1.0) ** i * (0.5 + 0.1 * i) for i in range(k)]
    grads, images, moments, t0s, scales = library_gradients(events, flows, coefs)
    assert grads[3] is None
    assert float(grads[5].abs().max()) == 0.0                      # an empty set: every cell written, all zero
    for i in range(k):
        if flows[i] is None:
            continue
        ref = check(form, grads[i], events[i], flows[i], images[i], moments[i], coefs[i], t0s[i], scales[i], what=f"job {i} of {k}")
        if i in (0, 4, 5, k - 1):
            one, im1, mo1, _, _ = library_gradients([events[i]], [flows[i]], [coefs[i]])
            assert torch.equal(im1[0], images[i]) and torch.equal(mo1[0], moments[i])
            check(form, one[0], events[i], flows[i], images[i], moments[i], coefs[i], t0s[i], scales[i], what=f"job {i} alone")
            _, A = grad_reference(events[i], flows[i], images[i], moments[i].tolist(), coefs[i], t0s[i], scales[i])
            d = (one[0].double() - grads[i].double()).abs()
            assert bool((d <= 2 * (C_A[form] * A + 2.0 ** -23 * ref.abs() + 1e-12 * float(ref.abs().max()))).all())


def test_zero_flow_job_leaves_its_buffer_alone(form):
    """At the C ABI: a NULL flow skips the job - a buffer handed in for it keeps its bytes."""
    import ctypes
    from eemflow_amd import _lib
    ev, flow, h, w = case("37x50")
    evs, fls, t0s, scales, maps, images, moments = forward([ev, ev], [flow, None])
    coef = torch.ones(2, dtype=torch.float64, device=DEV)
    out = [torch.full((2, h, w), 7.0, device=DEV), torch.full((2, h, w), 7.0, device=DEV)]
    ptr, dbl = ctypes.c_void_p * 2, ctypes.c_double * 2
    _lib.check(_lib.lib().eemflow_iwe_grad_many(
        2, ptr(*[e.data_ptr() for e in evs]), (ctypes.c_int64 * 2)(*[e.shape[0] for e in evs]), ptr(fls[0].data_ptr(), None),
        dbl(*t0s), dbl(*scales), (ctypes.c_double * 8)(*(IDENTITY * 2)), h, w, ptr(*[i.data_ptr() for i in images]), moments.data_ptr(),
        coef.data_ptr(), ptr(*[o.data_ptr() for o in out]), _lib.current_stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert bool((out[1] == 7.0).all())
    check(form, out[0].cpu(), ev, flow, images[0].cpu(), moments[0].cpu(), 1.0, t0s[0], scales[0], what="beside a zero-flow job")


def test_single_event_and_many_events_on_one_pixel(form):
    h, w = 20, 24
    flow = wavy_flow(h, w, seed=2)
    one = torch.tensor([[0.5, 7.3, 9.6, 1.0]], dtype=torch.float64)
    # one event: t0 = t, tau = 0 - the gradient is zero everywhere; under an explicit earlier t0 it is not
    grads, images, moments, t0s, scales = library_gradients([one], [flow], [1.0])
    assert float(grads[0].abs().max()) == 0.0
    evs, fls, _, _, maps, _, _ = forward([one], [flow])
    images, moments = iwe._launch_maps(evs, fls, [0.0], [1.0], maps, h, w, torch.device(DEV))
    g = iwe.iwe_grad_many(evs, fls, [0.0], [1.0], maps, images, moments, torch.ones(1, dtype=torch.float64, device=DEV))[0].cpu()
    assert integer_distance(one, flow, 0.0, 1.0) >= 1e-6
    ref = check(form, g, one, flow, images[0].cpu(), moments[0].cpu(), 1.0, 0.0, 1.0, what="single event")
    assert int((ref != 0).sum()) == 8 and int((g != 0).sum()) == 8          # four sample neighbours, two channels
    # 20000 events on one pixel at different times
    n = 20000
    t = np.sort(np.round(np.random.default_rng(1).uniform(0, 0.05, n) * 1e6) * 1e-6)
    ev = torch.from_numpy(np.stack([t, np.full(n, 11.25), np.full(n, 8.5), np.where(np.arange(n) % 3 == 0, -1.0, 1.0)], axis=1))
    keep = torch.ones(n, dtype=torch.bool)
    t0, scale = metric_refs(ev, "end")
    for v in warped_positions(ev, flow, t0, scale):
        keep &= ~((v - torch.round(v)).abs() < 2e-6)
    assert bool(keep[0] and keep[-1])
    ev = ev[keep].contiguous()
    assert integer_distance(ev, flow, t0, scale) >= 1e-6
    grads, images, moments, t0s, scales = library_gradients([ev], [flow], [-2.0])
    ref = check(form, grads[0], ev, flow, images[0], moments[0], -2.0, t0s[0], scales[0], what="one pixel")
    assert int((ref != 0).sum()) == 8


def test_nan_flow_pixel_leaves_the_gradient_finite(form):
    """The events that sample a NaN flow pixel are dropped whole by the forward and add nothing; the moments stay finite, and with
    finite moments every gradient cell is finite."""
    ev, flow, h, w = case("37x50")
    flow = flow.clone()
    flow[0, 10, 20] = float("nan")
    flow[1, 30, 5] = float("inf")
    grads, images, moments, t0s, scales = library_gradients([ev], [flow], [1.0])
    assert bool(torch.isfinite(moments).all()) and float(moments[0, 3]) > 0
    assert bool(torch.isfinite(grads[0]).all())
    check(form, grads[0], ev, flow, images[0], moments[0], 1.0, t0s[0], scales[0], what="NaN flow pixel")


def test_fwl_loss_value_and_backward(form):
    """The value is -mean(fwl_many); loss.backward() on a (B,2,H,W) leaf is the stacked teacher-forced gradients times -1/(B var0); a
    sample whose zero-flow variance is 0 (no events) is left out of the mean and gets a zero gradient."""
    h, w, b = 37, 50, 3
    flows = [wavy_flow(h, w, seed=60 + i) for i in range(b)]
    events = [off_integer_events(70 + i, 2000 + 500 * i, h, w, flows[i], fractional=True) for i in range(b)]
    pred = torch.stack(flows).to(DEV).requires_grad_(True)
    evs = [e.to(DEV) for e in events]
    loss = iwe.fwl_loss(evs, [pred[i] for i in range(b)])
    assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.is_cuda
    want = -iwe.fwl_many(evs, [pred[i].detach() for i in range(b)]).mean()
    assert abs(float(loss.detach()) - float(want)) <= 1e-14 * abs(float(want))
    loss.backward()
    assert pred.grad.shape == pred.shape
    _, _, _, _, _, images, moments = forward(events + events, flows + [None] * b)
    var = iwe.variance(moments).cpu()
    for i in range(b):
        coef = -1.0 / (b * float(var[b + i]))
        t0, scale = metric_refs(events[i], "end")
        check(form, pred.grad[i].cpu(), events[i], flows[i], images[i].cpu(), moments[i].cpu(), coef, t0, scale, what=f"fwl_loss sample {i}")
    # a degenerate sample
    evs2 = evs + [torch.zeros(0, 4, dtype=torch.float64, device=DEV)]
    pred2 = torch.cat([pred.detach(), torch.ones(1, 2, h, w, device=DEV)]).requires_grad_(True)
    loss2 = iwe.fwl_loss(evs2, [pred2[i] for i in range(b + 1)])
    assert abs(float(loss2.detach()) - float(want)) <= 1e-14 * abs(float(want))
    loss2.backward()
    assert float(pred2.grad[b].abs().max()) == 0.0
    d = (pred2.grad[:b] - pred.grad).abs()                         # (two runs: the fp64 sums' order is free)
    assert bool((d <= 2.0 ** -22 * pred.grad.abs() + 1e-9 * float(pred.grad.abs().max())).all())
    # every sample left out: the loss is 0
    p3 = torch.ones(1, 2, h, w, device=DEV, requires_grad=True)
    loss3 = iwe.fwl_loss(evs2[b:], [p3[0]])
    loss3.backward()
    assert float(loss3.detach()) == 0.0 and float(p3.grad.abs().max()) == 0.0
    # contrast_many: the variances, differentiable; a flow that needs no gradient gets none
    q = torch.stack(flows[:2]).to(DEV)
    a, c = q[0].clone().requires_grad_(True), q[1].clone()
    v = iwe.contrast_many(evs[:2], [a, c])
    assert torch.equal(v.detach(), iwe.variance(moments[:2]))
    (2.0 * v.sum()).backward()
    t0, scale = metric_refs(events[0], "end")
    check(form, a.grad.cpu(), events[0], flows[0], images[0].cpu(), moments[0].cpu(), 2.0, t0, scale, what="contrast_many")


def moving_points(seed, h, w, npts, per, F):
    """Events of points that move with the constant flow F (pixels over the window), fractional positions."""
    rng = np.random.default_rng(seed)
    px, py = rng.uniform(6, w - 7, npts), rng.uniform(6, h - 7, npts)
    t = np.sort(np.round(rng.uniform(0, 1, npts * per) * 1e6) * 1e-6)
    t[0], t[-1] = 0.0, 1.0
    k = rng.integers(0, npts, npts * per)
    x, y = px[k] + F[0] * t, py[k] + F[1] * t
    p = rng.integers(0, 2, npts * per) * 2.0 - 1.0
    return torch.from_numpy(np.stack([t, x, y, p], axis=1))


def test_gradient_steps_on_the_flow_raise_fwl(form):
    """Sign and usefulness: events made by a constant true flow, a start at half of it, ten plain gradient steps on the flow tensor
    itself - FWL never falls and ends above its start.  Step 1.0: the gradients are below 0.1 (the fp64 restatement gives 0.05), so a
    step moves a flow pixel by a twentieth of a pixel, far inside the cell it votes into."""
    h, w, F = 32, 40, (3.0, -2.0)
    ev = moving_points(5, h, w, 40, 30, F).to(DEV)
    flow = torch.stack([torch.full((h, w), F[0] / 2), torch.full((h, w), F[1] / 2)]).to(DEV)
    vals = []
    for _ in range(10):
        flow.requires_grad_(True)
        loss = iwe.fwl_loss([ev], [flow])
        vals.append(-float(loss))
        (g,) = torch.autograd.grad(loss, flow)
        flow = (flow - 1.0 * g).detach()
    vals.append(float(iwe.fwl(ev, flow)))
    print("fwl over the steps", ["%.4f" % v for v in vals])
    assert all(b >= a for a, b in zip(vals, vals[1:])) and vals[-1] > vals[0] + 0.05


# ------------------------------------------------------------------------------------------------ through the models
def eemflow_net(seed):
    from eemflow_amd import EEMFlow
    net = EEMFlow("", groups=5, n_first_channels=5)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
    return net.to(DEV).train()


def synthetic_batch(seed, b, h, w, with_flow=True):
    """A batch as the datasets' get_batch makes it for flipped and cropped samples: volumes, flow, valid, the samples' events and the
    event maps of their plans (the source frame is 8 px larger each way)."""
    e1, e2 = (torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(seed, b, h, w))
    plans = [AugPlan(h + 8, w + 8, crop=(h, w), y0=1 + i, x0=7 - i, hflip=i % 2 == 0, vflip=i % 2 == 1) for i in range(b)]
    batch = {"event_volume_old": e1, "event_volume_new": e2,
             "events": [raw_events(seed + 10 + i, 3000 + 100 * i, h + 8, w + 8, fractional=True).to(DEV) for i in range(b)],
             "events_offset": [(0, 0)] * b,
             "events_map": [event_map_after_offset(p, (0, 0), h + 8, w + 8) for p in plans]}
    if with_flow:
        gt, valid = (torch.from_numpy(a).to(DEV) for a in synthetic_gt(seed + 1, b, h, w))
        batch["flow"], batch["valid"] = gt, valid
    return batch


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


class Lines(Logger):
    def __init__(self):
        super().__init__(verbose=False)
        self.lines = []

    def write_line(self, line, *a, **k):
        self.lines.append(line)


@pytest.mark.parametrize("h,w", [(64, 64), (260, 346)])
def test_trainer_with_contrast_term(h, w):
    """TrainRaftEvents(engine='autograd', contrast_weight=0.5) on EEMFlow, batch 2, two steps: finite parameter gradients, the loss
    line, and the first step's gradients = sequence_loss's + 0.5 * the contrast term's, each computed on its own (3e-3 relative to the
    largest entry, what tests/test_gpu_autograd.py allows accumulated gradients)."""
    batches = [synthetic_batch(80, 2, h, w), synthetic_batch(90, 2, h, w)]
    net = eemflow_net(77)
    seen = []

    def loader():
        for i, b in enumerate(batches):
            if i:                                                  # (after step i's backward, before the next zero_grad)
                seen.append({k: p.grad.clone() for k, p in net.named_parameters()})
            yield b
    log = Lines()
    tr = TrainRaftEvents(loader(), (h, w), lr=1e-5, clip=1e9, logger=log, print_freq=1, engine="autograd", mixed_precision=False,
                         contrast_weight=0.5)
    tr.train_iters(net, val_iters=2)
    last = {k: p.grad for k, p in net.named_parameters()}
    assert len(seen) == 1 and all(bool(torch.isfinite(g).all()) for g in list(seen[0].values()) + list(last.values()))
    assert len(log.lines) == 2 and all("loss" in ln and "epe" in ln for ln in log.lines)
    # the two terms on their own, on a second model of the same weights
    ref = eemflow_net(77)
    ref.change_imagesize((h, w))
    b = batches[0]
    _, preds = ref(b["event_volume_old"], b["event_volume_new"])
    assert tuple(preds[-1].shape[-2:]) == (h, w)
    sup, _ = hip_train.sequence_loss(preds, b["flow"], b["valid"], 0.8)
    sup.backward()
    g_sup = {k: p.grad.clone() for k, p in ref.named_parameters()}
    ref.zero_grad()
    _, preds = ref(b["event_volume_old"], b["event_volume_new"])
    con = hip_train.contrast_loss(preds[-1], b["events"], b["events_map"])
    con.float().backward()
    g_con = {k: p.grad.clone() for k, p in ref.named_parameters()}
    assert max(float(g.abs().max()) for g in g_con.values()) > 0
    worst = max((rel_err(seen[0][k], g_sup[k] + 0.5 * g_con[k]), k) for k in g_sup)
    print("trainer", (h, w), "worst relative difference", worst, "loss", float(sup), float(con))
    assert worst[0] < 3e-3, worst
    logged = float(log.lines[0].split("loss")[1].split()[0])
    total = float(sup) + 0.5 * float(con)
    assert abs(logged - total) <= 1e-5 * (1.0 + abs(total))         # (the loop adds the two in fp32 and prints six decimals)


def test_trainer_self_supervised_reads_no_ground_truth():
    h, w = 64, 64
    batches = [synthetic_batch(100, 2, h, w, with_flow=False), synthetic_batch(110, 2, h, w, with_flow=False)]
    assert "flow" not in batches[0] and "valid" not in batches[0]
    net = eemflow_net(78)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    log = Lines()
    tr = TrainRaftEvents(batches, (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd", contrast_weight=1.0, supervised=False)
    tr.train_iters(net, val_iters=2)
    assert len(log.lines) == 2 and tr.iteration == 2
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert any(not torch.equal(p.detach(), before[k]) for k, p in net.named_parameters())


def test_contrast_loss_through_eraft():
    """E-RAFT at the size and iteration count its training tests use (128 x 160, two iterations), batch 2."""
    from eemflow_amd.eraft import ERAFT
    h, w = 128, 160
    torch.manual_seed(5)
    net = ERAFT("", n_first_channels=5).to(DEV).train()
    net.change_imagesize((h, w))
    b = synthetic_batch(120, 2, h, w, with_flow=False)
    preds = net(b["event_volume_old"], b["event_volume_new"], iters=2)[1]
    assert tuple(preds[-1].shape) == (2, 2, h, w) and preds[-1].requires_grad
    loss = hip_train.contrast_loss(preds[-1], b["events"], b["events_map"])
    loss.float().backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and max(float(g.abs().max()) for g in grads) > 0


# ------------------------------------------------------------------------------------------------ the forward's bits
def forward_digests():
    """sha256 of the forward's image and moments bytes, per case, time reference and form: tests/golden/iwe_forward_bits.json holds
    them as the library gave them BEFORE the per-event device functions moved into iwe_shared.h and the offset became an event map
    (241x40: before the forward's kernels moved into iwe_fwd_shared.h, recorded with the library of the commit before that one).
    The binned image does not depend on the order of its adds (fixed-point weights, exact fp64 sums); the direct form's fp64 atomics
    could round a cell apart once in ~1e7 cells, so it is pinned on the three small frames only."""
    out = {}
    for kind in ("binned", "direct"):
        if kind == "direct":
            os.environ["EEM_IWE_DIRECT"] = "1"
        else:
            os.environ.pop("EEM_IWE_DIRECT", None)
        for name in SHAPES:
            if kind == "direct" and name in ("260x346", "720x1280"):
                continue
            h, w, n, fractional = SHAPES[name]
            ev, flow = raw_events(7, n, h, w, fractional).to(DEV), smooth_flow(h, w).to(DEV)
            for t_ref in ("end", "start"):
                for offset in ((0, 0), (3, 2)):
                    image, moments = iwe.iwe(ev, flow, t_ref=t_ref, offset=offset)
                    zimage, zmoments = iwe.iwe(ev, None, t_ref=t_ref, offset=offset, size=(h, w))
                    dig = hashlib.sha256()
                    for t in (image, moments, zimage, zmoments):
                        dig.update(t.cpu().numpy().tobytes())
                    out[f"{kind} {name} {t_ref} {offset[0]},{offset[1]}"] = dig.hexdigest()
    os.environ.pop("EEM_IWE_DIRECT", None)
    return out


def test_forward_bits_are_the_parent_commits(monkeypatch):
    monkeypatch.delenv("EEM_IWE_DIRECT", raising=False)            # (forward_digests sets and clears it itself; restored afterwards)
    want = json.load(open(BITS))
    got = forward_digests()
    assert sorted(got) == sorted(want) and len(want) == 40
    assert [k for k in want if got[k] != want[k]] == []
