"""The image of average timestamps, its loss, the loss's gradient and RSAT on the GPU (csrc/tsimg.hip, eemflow_amd/tsimg.py,
train.timestamp_loss, the trainer's term and the evaluation loop's rsat=) in both kernel forms - binned (the default) and direct
(EEM_IWE_DIRECT=1) - against the fp64 restatement of tests/tsimg_reference.py.  Needs a real MI355X: `pytest -m gpu`.

D, bitwise.  Both forms add the fixed-point weights q / 2^31, whose fp64 sums are exact, so the stored D does not depend on the form or
on the order of the adds: it is the image eemflow_iwe_map_many's BINNED form writes (the form that votes with the same fixed-point
weights; iwe.hip's direct form adds the un-quantised products and may round a cell apart).  The comparison image is therefore always
taken with EEM_IWE_DIRECT unset, whatever form the term itself runs in.

T against the reference, per cell: |T32 - T_ref| <= (dN + T_ref dD) / (D_ref + eps) + 2^-23 T_ref, with T_ref, D_ref, N_ref and the vote
count V from the UN-quantised planes, dD = V 2^-32 + 2^-24 D_ref and dN = V 2^-31 + 2^-24 N_ref: a fixed-point weight is off by at most
2^-32, ah (rounded to fp32) by at most 2^-24 relative - N by V 2^-32 + 2^-24 N_ref from the two, doubled - and the quotient's one
rounding to fp32 is half an ulp, doubled.  |T32^2 - T_ref^2| <= (2 T_ref + b) b with the cell's bound b, summed over the cells and
divided by active + 1e-9, bounds the loss.

Gradient, teacher-forced with the library's own D and T, per cell: |d| <= c_A A + 2^-23 |ref| + 1e-12 max|ref|, A the abs-sum map;
c_A = 2^-23 for the binned form (a contribution is rounded to fp32 once when its record is made) and 2^-40 for the direct form (nothing
is rounded before the fp64 sum) - the bound of tests/test_gpu_iwe_grad.py, for the same kernels.  The cases keep every warped
position at least 1e-6 from an integer (asserted on the reference); the integer convention has its own test."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from eemflow_amd import _lib, tsimg
from eemflow_amd import train as hip_train
from eemflow_amd.augmentor import AugPlan, event_map_after_offset
from eemflow_amd.harness import Logger, TestRaftEvents, TrainRaftEvents, stream_chunks
from eemflow_amd.weights import seeded_state_dict, synthetic_gt, synthetic_voxel_pair

from iwe_grad_reference import integer_distance, map_events, warped_positions
from iwe_reference import metric_refs, separable_flow
from tsimg_reference import grad_reference, loss_autograd, loss_reference, moments_of, rsat_reference

iwe = importlib.import_module("eemflow_amd.iwe")        # (the package's attribute `iwe` is the one-job function)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-9
# name -> (H, W, N, fractional coordinates, time references)
SHAPES = {"37x50": (37, 50, 5000, False, ("end", "start")), "64x61": (64, 61, 5000, True, ("end", "start")),
          "8x1280": (8, 1280, 3000, False, ("end", "start")), "720x1280": (720, 1280, 20000, False, ("end",)),
          "3x4804": (3, 4804, 2000, False, ("end", "start")),      # 4 planes of 4804 cells pass 150 KB of LDS: the plan refuses the frame
          "241x40": (241, 40, 5000, True, ("end", "start"))}       # rows = 2 per band of 4 planes, 121 bands, the last of them one row
CASES = [(name, t_ref) for name, s in SHAPES.items() for t_ref in s[4]]
C_A = {"binned": 2.0 ** -23, "direct": 2.0 ** -40}
IDENTITY = (1.0, 0.0, 1.0, 0.0)


@pytest.fixture(params=["binned", "direct"])
def form(request, monkeypatch):
    if request.param == "direct":
        monkeypatch.setenv("EEM_IWE_DIRECT", "1")
    else:
        monkeypatch.delenv("EEM_IWE_DIRECT", raising=False)
    return request.param


# ------------------------------------------------------------------------------------------------ cases (tests/test_gpu_iwe_grad.py's helpers, re-stated)
def smooth_flow(h, w):
    y, x = torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64)
    return separable_flow((6.0 * torch.sin(2 * math.pi * x / w) + 2.0).float(), (4.0 * torch.cos(2 * math.pi * y / h)).float())


def wavy_flow(h, w, seed=5):
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
    """Events none of whose warped positions, under either time reference, comes within 2e-6 of an integer (the events at the two end
    times, which set t0 and the span, get a fractional position and stay)."""
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


_cases, _refs, _runs = {}, {}, {}


def case(name):
    """(events, flow, h, w) of a shape, built once."""
    if name not in _cases:
        h, w, n, fractional, _ = SHAPES[name]
        flow = smooth_flow(h, w)
        _cases[name] = (off_integer_events(7, n, h, w, flow, fractional), flow, h, w)
    return _cases[name]


def reference(name, t_ref):
    """The un-quantised restatement of a case, computed once and left unchanged."""
    if (name, t_ref) not in _refs:
        ev, flow, h, w = case(name)
        t0, scale = metric_refs(ev, t_ref)
        assert integer_distance(ev, flow, t0, scale) >= 1e-6
        _refs[name, t_ref] = loss_reference(ev, flow.double(), t0, scale, eps=EPS)
    return _refs[name, t_ref]


# ------------------------------------------------------------------------------------------------ the library on CPU inputs
def forward(events, flows, t_ref="end", maps=None, refs=None, size=None):
    """The library's forward of some jobs: device inputs and outputs, as the backward is teacher-forced with them."""
    evs = [e.to(DEV) for e in events]
    fls = [f.to(DEV) if f is not None else None for f in flows]
    shape = next((f.shape for f in flows if f is not None), None)
    h, w = (shape[1], shape[2]) if shape is not None else size
    refs = refs if refs is not None else [metric_refs(e, t_ref) for e in events]
    t0s, scales = [r[0] for r in refs], [r[1] for r in refs]
    maps = list(maps) if maps is not None else [IDENTITY] * len(evs)
    timgs, dimgs, moments = tsimg._launch(evs, fls, t0s, scales, maps, h, w, EPS, torch.device(DEV))
    form_ran = tsimg.last_form()
    torch.cuda.synchronize()
    return dict(evs=evs, fls=fls, t0s=t0s, scales=scales, maps=maps, timgs=timgs, dimgs=dimgs, moments=moments, form=form_ran, h=h, w=w)


def binned_iwe_images(run):
    """iwe.hip's BINNED images of a run's jobs (EEM_IWE_DIRECT unset for the call, see the module docstring)."""
    saved = os.environ.pop("EEM_IWE_DIRECT", None)
    try:
        images, _ = iwe._launch_maps(run["evs"], run["fls"], run["t0s"], run["scales"], run["maps"], run["h"], run["w"], torch.device(DEV))
        torch.cuda.synchronize()
    finally:
        if saved is not None:
            os.environ["EEM_IWE_DIRECT"] = saved
    return images


def gradients(run, coefs, flows=None):
    coef = torch.tensor(coefs, dtype=torch.float64, device=DEV)
    grads = tsimg.tsimg_grad_many(run["evs"], run["fls"] if flows is None else flows, run["t0s"], run["scales"], run["maps"], run["timgs"],
                                  run["dimgs"], coef, EPS)
    form_ran = tsimg.last_form()
    torch.cuda.synchronize()
    return [g.cpu() if g is not None else None for g in grads], form_ran


def run_of(form, name, t_ref):
    """The library's forward of a case in a form, run once."""
    if (form, name, t_ref) not in _runs:
        ev, flow, h, w = case(name)
        _runs[form, name, t_ref] = forward([ev], [flow], t_ref)
    return _runs[form, name, t_ref]


def t_bound(ref, eps=EPS):
    """The per-cell bound of the module docstring on |T32 - T_ref|."""
    dD = ref["V"] * 2.0 ** -32 + 2.0 ** -24 * ref["D"]
    dN = ref["V"] * 2.0 ** -31 + 2.0 ** -24 * ref["N"]
    return (dN + ref["T"] * dD) / (ref["D"] + eps) + 2.0 ** -23 * ref["T"]


def loss_bound(ref, eps=EPS):
    b = t_bound(ref, eps)
    return float(((2.0 * ref["T"] + b) * b).sum()) / (ref["moments"][2] + 1e-9)


def check_t(T32, moments, ref, what=""):
    """A job's stored T and its loss against the un-quantised restatement, within the bounds of the module docstring."""
    b = t_bound(ref)
    d = (T32.double() - ref["T"]).abs()
    worst = float((d / (b + 1e-300)).max())
    lib_loss = float(moments[1]) / (float(moments[2]) + 1e-9)
    lb = loss_bound(ref)
    print(f"{what}: max|dT| {float(d.max()):.3e} worst |dT|/bound {worst:.3f}; loss {lib_loss:.9f} ref {ref['loss']:.9f} "
          f"|d| {abs(lib_loss - ref['loss']):.3e} bound {lb:.3e}")
    assert bool((d <= b).all()), (what, float(d.max()), worst)
    assert float(moments[2]) == ref["moments"][2], what            # the same active pixels
    assert abs(lib_loss - ref["loss"]) <= lb, what


def check_moments(D32, T32, moments, dropped, what=""):
    """The moments row against fp64 sums of the library's own stored images."""
    m = moments_of(D32, T32, dropped)
    got = [float(v) for v in moments]
    print(f"{what}: moments {got} from the images {m}")
    assert got[0] == m[0] and got[2] == m[2] and got[3] == m[3], what
    assert abs(got[1] - m[1]) <= 1e-13 * m[1], what


def check_grad(form, got, events, flow, D32, T32, coef, t0, scale, amap=IDENTITY, slack=1.0, what=""):
    """One job's gradient against the explicit formula within the bound of the module docstring; returns (reference, bound)."""
    ref, A = grad_reference(events, flow, D32, T32, coef, EPS, t0, scale, amap)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), what
    big = float(ref.abs().max())
    bound = slack * (C_A[form] * A + 2.0 ** -23 * ref.abs() + 1e-12 * big)
    d = (got.double() - ref).abs()
    worst = float((d / (bound + 1e-300)).max())
    print(f"{what} {form}: max|ref| {big:.3e} max|d| {float(d.max()):.3e} worst |d|/bound {worst:.3f}")
    assert bool((d <= bound).all()), (what, form, float(d.max()), worst)
    return ref, bound


def expected_form(form, name):
    return "direct" if form == "direct" or name == "3x4804" else "bin_e"


# ------------------------------------------------------------------------------------------------ 1 - 4: every shape, both forms
@pytest.mark.parametrize("name,t_ref", CASES)
def test_vote_image_is_bitwise_the_image_of_warped_events(form, name, t_ref):
    run = run_of(form, name, t_ref)
    if expected_form(form, name) == "direct":
        assert run["form"] == "direct"                             # (3x4804: with the switch unset, because the plan refuses it)
    else:
        assert re.fullmatch(r"bin_e[124]\+band(256|1024)_s[2-6]\+moments", run["form"]), run["form"]
    want = binned_iwe_images(run)[0]
    assert run["dimgs"][0].dtype == torch.float32 and torch.equal(run["dimgs"][0], want)
    assert float(want.sum()) > 100.0


@pytest.mark.parametrize("name,t_ref", CASES)
def test_moments_are_those_of_the_stored_images(form, name, t_ref):
    run = run_of(form, name, t_ref)
    ref = reference(name, t_ref)
    check_moments(run["dimgs"][0].cpu(), run["timgs"][0].cpu(), run["moments"][0].cpu(), ref["moments"][3], f"{name} {t_ref}")
    assert float(run["moments"][0, 2]) > 0 and float(run["moments"][0, 1]) > 0


@pytest.mark.parametrize("name,t_ref", CASES)
def test_average_timestamps_against_the_reference(form, name, t_ref):
    run = run_of(form, name, t_ref)
    ref = reference(name, t_ref)
    assert float(ref["T"].max()) > 0.5
    check_t(run["timgs"][0].cpu(), run["moments"][0].cpu(), ref, f"{name} {t_ref} {form}")


@pytest.mark.parametrize("name,t_ref", CASES)
def test_teacher_forced_gradient(form, name, t_ref):
    ev, flow, h, w = case(name)
    run = run_of(form, name, t_ref)
    coef = -0.8 / (float(run["moments"][0, 2]) + 1e-9)
    grads, ran = gradients(run, [coef])
    assert ran == ("grad_direct" if form == "direct" else "grad_bin_e1+grad_band")      # (2 planes of 4804 cells fit: 3x4804 bins here)
    ref, _ = check_grad(form, grads[0], ev, flow, run["dimgs"][0].cpu(), run["timgs"][0].cpu(), coef, run["t0s"][0], run["scales"][0],
                        what=f"{name} {t_ref}")
    assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("ept", [1, 2, 4])
def test_every_events_per_thread_form_of_the_binning_kernel(monkeypatch, ept):
    monkeypatch.delenv("EEM_IWE_DIRECT", raising=False)
    monkeypatch.setenv("EEM_IWE_EPT", str(ept))
    ev, flow, h, w = case("64x61")
    run = forward([ev], [flow], "end")
    assert run["form"].startswith(f"bin_e{ept}+")
    assert torch.equal(run["dimgs"][0], binned_iwe_images(run)[0])
    check_t(run["timgs"][0].cpu(), run["moments"][0].cpu(), reference("64x61", "end"), f"ept {ept}")
    check_moments(run["dimgs"][0].cpu(), run["timgs"][0].cpu(), run["moments"][0].cpu(), 0.0, f"ept {ept}")


# ------------------------------------------------------------------------------------------------ 5: conventions
def test_integer_warped_positions_take_the_left_pair_with_zero_weight(form):
    """Dyadic inputs put warped positions exactly on integers: one vote of weight 1 into (Y0, X0), and the derivative of the pair
    (X0, X0 + 1) with gx = 0 - what the forward's floor gives, and autograd through xw - floor(xw)."""
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
    run = forward([ev], [flow])
    D32, T32 = run["dimgs"][0].cpu(), run["timgs"][0].cpu()
    ref = loss_reference(ev, flow.double(), t0, scale, eps=EPS)
    assert torch.equal(D32, ref["D32"]) and torch.equal(run["dimgs"][0], binned_iwe_images(run)[0])     # whole votes: exact
    assert bool((D32 == torch.round(D32)).all())
    check_t(T32, run["moments"][0].cpu(), ref, "integer positions")
    grads, _ = gradients(run, [1.0])
    gref, _ = check_grad(form, grads[0], ev, flow, D32, T32, 1.0, t0, scale, what="integer positions")
    assert float(gref.abs().max()) > 0
    # the reference's own derivative is autograd's
    f64 = flow.double().requires_grad_(True)
    loss, _, _, _ = loss_autograd(ev, f64, t0, scale, eps=EPS, normalize="none", D32=D32, T32=T32)
    (auto,) = torch.autograd.grad(loss, f64)
    assert float((auto - gref).abs().max()) <= 1e-12 * float(gref.abs().max())


def test_flip_map_with_crop_equals_explicitly_transformed_events(form):
    h, w = 37, 50
    flow = wavy_flow(h, w)
    plan = AugPlan(45, 64, crop=(h, w), y0=5, x0=9, hflip=True)
    amap = event_map_after_offset(plan, (2, 1), 45, 64)
    assert amap[0] == -1.0 and amap[2] == 1.0
    ev = off_integer_events(21, 6000, 45 + 1, 64 + 2, flow, fractional=True, amap=amap)
    moved = map_events(ev, amap)
    a = forward([ev], [flow], maps=[amap])
    b = forward([moved], [flow])
    assert torch.equal(a["dimgs"][0], b["dimgs"][0])               # -1 * x + b on the device is the host's: the same votes
    Ta, Tb = a["timgs"][0].cpu().double(), b["timgs"][0].cpu().double()
    assert bool(((Ta - Tb).abs() <= 2.0 ** -23 * Tb).all())        # (N's fp64 sums: the order of the adds is free)
    t0, scale = a["t0s"][0], a["scales"][0]
    ref = loss_reference(moved, flow.double(), t0, scale, eps=EPS)
    check_t(a["timgs"][0].cpu(), a["moments"][0].cpu(), ref, "flip map")
    check_t(a["timgs"][0].cpu(), a["moments"][0].cpu(), loss_reference(ev, flow.double(), t0, scale, amap, eps=EPS), "flip map, mapped reference")
    ga, _ = gradients(a, [0.6])
    gb, _ = gradients(b, [0.6])
    D32, T32 = a["dimgs"][0].cpu(), a["timgs"][0].cpu()
    gref, _ = check_grad(form, ga[0], moved, flow, D32, T32, 0.6, t0, scale, what="flip map")
    check_grad(form, ga[0], ev, flow, D32, T32, 0.6, t0, scale, amap=amap, what="flip map, mapped reference")
    check_grad(form, gb[0], moved, flow, b["dimgs"][0].cpu(), b["timgs"][0].cpu(), 0.6, t0, scale, what="moved events")
    assert float(gref.abs().max()) > 0


def test_nan_flow_pixel_is_counted_and_leaves_everything_finite(form):
    ev, flow, h, w = case("37x50")
    flow = flow.clone()
    flow[0, 10, 20] = float("nan")
    flow[1, 30, 5] = float("inf")
    run = forward([ev], [flow])
    t0, scale = run["t0s"][0], run["scales"][0]
    ref = loss_reference(ev, flow.double(), t0, scale, eps=EPS)
    m = run["moments"][0].cpu()
    assert ref["moments"][3] > 0 and float(m[3]) == ref["moments"][3]
    assert bool(torch.isfinite(run["timgs"][0]).all() and torch.isfinite(run["dimgs"][0]).all() and torch.isfinite(m).all())
    check_t(run["timgs"][0].cpu(), m, ref, "NaN flow pixel")
    grads, _ = gradients(run, [1.0])
    check_grad(form, grads[0], ev, flow, run["dimgs"][0].cpu(), run["timgs"][0].cpu(), 1.0, t0, scale, what="NaN flow pixel")
    pred = flow.to(DEV).requires_grad_(True)
    loss = tsimg.timestamp_loss([ev.to(DEV)], [pred])
    loss.backward()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(pred.grad).all())


def test_single_event_and_many_events_on_one_pixel(form):
    h, w = 20, 24
    flow = wavy_flow(h, w, seed=2)
    one = torch.tensor([[0.5, 7.3, 9.6, 1.0]], dtype=torch.float64)
    # one event under an explicit earlier t0: tau = 0.5, ah = 0.5; its four cells hold ah (times D / (D + eps)), the others 0
    run = forward([one], [flow], refs=[(0.0, 1.0)])
    assert integer_distance(one, flow, 0.0, 1.0) >= 1e-6
    ref = loss_reference(one, flow.double(), 0.0, 1.0, eps=EPS)
    T32, D32 = run["timgs"][0].cpu(), run["dimgs"][0].cpu()
    check_t(T32, run["moments"][0].cpu(), ref, "single event")
    hit = D32 > 0
    assert int(hit.sum()) == 4 and float(run["moments"][0, 2]) == 4.0 and bool((T32[~hit] == 0).all())
    assert bool(((T32[hit].double() - 0.5).abs() <= 0.5 * (EPS / D32[hit].double() + 2.0 ** -23)).all())
    grads, _ = gradients(run, [1.0])
    gref, _ = check_grad(form, grads[0], one, flow, D32, T32, 1.0, 0.0, 1.0, what="single event")
    # a lone event's cells all hold its own ah: G = 2 T (ah - T) / D is 0 up to T's rounding - nothing to gain by moving it
    assert float(gref.abs().max()) <= 2.0 ** -22 * 4 * 0.5 * 0.5 / float(D32[hit].min())
    # 250 events on one pixel at different times, zero flow: every cell holds the mean of their timestamp values per polarity
    n = 250
    t = np.sort(np.round(np.random.default_rng(1).uniform(0, 0.05, n) * 1e6) * 1e-6)
    pol = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
    ev = torch.from_numpy(np.stack([t, np.full(n, 11.25), np.full(n, 8.5), pol], axis=1))
    run = forward([ev], [None], size=(h, w))
    t0, scale = run["t0s"][0], run["scales"][0]
    ref = loss_reference(ev, None, t0, scale, eps=EPS, size=(h, w))
    T32 = run["timgs"][0].cpu()
    check_t(T32, run["moments"][0].cpu(), ref, "one pixel")
    a = 1.0 - np.abs((t - t0) * scale)
    for c, sel in ((0, pol > 0), (1, pol < 0)):
        cells = T32[c, 8:10, 11:13].double()
        assert bool(((cells - a[sel].mean()).abs() <= 1e-6).all())
    assert float(run["moments"][0, 2]) == 4.0
    # and with a flow: the gradient of 250 events through one pixel's four sample neighbours
    keep = torch.ones(n, dtype=torch.bool)
    for v in warped_positions(ev, flow, t0, scale):
        keep &= ~((v - torch.round(v)).abs() < 2e-6)
    assert bool(keep[0] and keep[-1])
    ev = ev[keep].contiguous()
    run = forward([ev], [flow])
    grads, _ = gradients(run, [-2.0])
    gref, _ = check_grad(form, grads[0], ev, flow, run["dimgs"][0].cpu(), run["timgs"][0].cpu(), -2.0, t0, scale, what="one pixel")
    assert int((gref != 0).sum()) == 8


def test_zero_flow_job_leaves_its_buffer_alone(form):
    """At the C ABI: a NULL flow skips the job - a buffer handed in for it keeps its bytes - and a call of zero-flow jobs alone
    launches nothing and leaves last_form as it was."""
    ev, flow, h, w = case("37x50")
    run = forward([ev, ev], [flow, None])
    coef = torch.ones(2, dtype=torch.float64, device=DEV)
    out = [torch.full((2, h, w), 7.0, device=DEV), torch.full((2, h, w), 7.0, device=DEV)]
    ptr, dbl = ctypes.c_void_p * 2, ctypes.c_double * 2

    def call(flow_ptrs):
        _lib.check(_lib.lib().eemflow_tsimg_grad_many(
            2, ptr(*[e.data_ptr() for e in run["evs"]]), (ctypes.c_int64 * 2)(*[e.shape[0] for e in run["evs"]]), ptr(*flow_ptrs),
            dbl(*run["t0s"]), dbl(*run["scales"]), (ctypes.c_double * 8)(*(IDENTITY * 2)), h, w, EPS, ptr(*[i.data_ptr() for i in run["dimgs"]]),
            ptr(*[i.data_ptr() for i in run["timgs"]]), coef.data_ptr(), ptr(*[o.data_ptr() for o in out]),
            _lib.current_stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
    before = tsimg.last_form()
    assert before == run["form"]
    call([None, None])
    assert tsimg.last_form() == before and bool((out[0] == 7.0).all() and (out[1] == 7.0).all())
    # a refused call leaves it too
    assert _lib.lib().eemflow_tsimg_many(0, None, None, None, None, None, None, h, w, EPS, None, None, None, None) != 0
    assert _lib.lib().eemflow_tsimg_last_form(None, 8) != 0
    assert tsimg.last_form() == before
    call([run["fls"][0].data_ptr(), None])
    assert tsimg.last_form().startswith("grad_")
    assert bool((out[1] == 7.0).all())
    check_grad(form, out[0].cpu(), ev, flow, run["dimgs"][0].cpu(), run["timgs"][0].cpu(), 1.0, run["t0s"][0], run["scales"][0],
               what="beside a zero-flow job")


def test_empty_event_set(form):
    h, w = 37, 50
    none = torch.zeros(0, 4, dtype=torch.float64)
    ev, flow, _, _ = case("37x50")
    run = forward([none], [flow])
    assert float(run["timgs"][0].abs().max()) == 0.0 and float(run["dimgs"][0].abs().max()) == 0.0
    assert run["moments"][0].cpu().tolist() == [float(h * w), 0.0, 0.0, 0.0]
    grads, _ = gradients(run, [1.0])
    assert float(grads[0].abs().max()) == 0.0                      # every cell written, all zero
    # left out of timestamp_loss: the mean is the other sample's, its gradient zero
    pred = torch.stack([flow, flow]).to(DEV).requires_grad_(True)
    both = tsimg.timestamp_loss([ev.to(DEV), none.to(DEV)], [pred[0], pred[1]])
    alone = tsimg.timestamp_loss([ev.to(DEV)], [flow.to(DEV)])
    assert abs(float(both) - float(alone)) <= 1e-6 * float(alone) and float(alone) > 0     # (T to one fp32 ulp from run to run)
    both.backward()
    assert float(pred.grad[1].abs().max()) == 0.0 and float(pred.grad[0].abs().max()) > 0
    # every sample left out: the loss is 0
    p3 = torch.ones(1, 2, h, w, device=DEV, requires_grad=True)
    l3 = tsimg.timestamp_loss([none.to(DEV)], [p3[0]])
    l3.backward()
    assert float(l3) == 0.0 and float(p3.grad.abs().max()) == 0.0
    assert math.isnan(float(tsimg.rsat(none.to(DEV), flow.to(DEV))))


# ------------------------------------------------------------------------------------------------ 6: batching
@pytest.mark.parametrize("k", [16, 32])
def test_jobs_of_one_call_equal_one_job_calls(form, k):
    """k jobs of different sizes in one call, a zero-flow job and an empty set among them: D bitwise the one-job call's, T within one
    fp32 ulp (N's sums are free in their order), every gradient within the bound of its own teacher."""
    h, w = 37, 50
    flows = [wavy_flow(h, w, seed=30 + i) for i in range(k)]
    events = [off_integer_events(40 + i, 300 + 137 * i, h, w, flows[i], fractional=i % 2 == 0) for i in range(k)]
    flows[3] = None
    events[5] = torch.zeros(0, 4, dtype=torch.float64)
    coefs = [(-1.0) ** i * (0.5 + 0.1 * i) for i in range(k)]
    run = forward(events, flows)
    grads, _ = gradients(run, coefs)
    assert grads[3] is None and float(grads[5].abs().max()) == 0.0
    images = binned_iwe_images(run)
    for i in range(k):
        assert torch.equal(run["dimgs"][i], images[i]), i
        D32, T32 = run["dimgs"][i].cpu(), run["timgs"][i].cpu()
        check_moments(D32, T32, run["moments"][i].cpu(), 0.0, f"job {i} of {k}")
        if flows[i] is None:
            continue
        ref, bound = check_grad(form, grads[i], events[i], flows[i], D32, T32, coefs[i], run["t0s"][i], run["scales"][i], what=f"job {i} of {k}")
        if i in (0, 4, 5, k - 1):
            one = forward([events[i]], [flows[i]])
            assert torch.equal(one["dimgs"][0], run["dimgs"][i])
            T1 = one["timgs"][0].cpu().double()
            assert bool(((T1 - T32.double()).abs() <= 2.0 ** -23 * T1).all())
            g1, _ = gradients(one, [coefs[i]])
            check_grad(form, g1[0], events[i], flows[i], one["dimgs"][0].cpu(), one["timgs"][0].cpu(), coefs[i], run["t0s"][i], run["scales"][i],
                       what=f"job {i} alone")
            # two runs of one teacher: each within the bound, so within twice the bound of each other.  (Where N's free order of adds
            # moved a T by its last bit - once in ~1e9 cells - the teachers differ and each run is held to its own, above.)
            if torch.equal(one["timgs"][0].cpu(), T32):
                assert bool(((g1[0].double() - grads[i].double()).abs() <= 2 * bound).all())


# ------------------------------------------------------------------------------------------------ 7: the training term and RSAT
def test_timestamp_loss_value_and_backward(form, monkeypatch):
    """Three samples with maps: the value is the mean over the samples of L(end) + L(start) of the restatement, within the loss bound;
    loss.backward() on a (B,2,H,W) leaf is the explicit gradient of both time references, teacher-forced with the images of the
    loss's own forward (recorded from its launch), which is autograd's."""
    h, w, b = 37, 50, 3
    flows = [wavy_flow(h, w, seed=60 + i) for i in range(b)]
    plans = [AugPlan(45, 64, crop=(h, w), y0=2 + i, x0=8 - i, hflip=i % 2 == 0, vflip=i == 1) for i in range(b)]
    maps = [event_map_after_offset(p, (0, 0), 45, 64) for p in plans]
    events = [off_integer_events(70 + i, 2000 + 500 * i, 45, 64, flows[i], fractional=True, amap=maps[i]) for i in range(b)]
    pred = torch.stack(flows).to(DEV).requires_grad_(True)
    evs = [e.to(DEV) for e in events]
    launches = []
    real = tsimg._launch

    def recording(event_sets, fls, t0s, scales, mps, *rest):
        out = real(event_sets, fls, t0s, scales, mps, *rest)
        launches.append((t0s, scales, mps) + tuple(out))
        return out
    monkeypatch.setattr(tsimg, "_launch", recording)
    loss = tsimg.timestamp_loss(evs, [pred[i] for i in range(b)], maps=maps)
    monkeypatch.setattr(tsimg, "_launch", real)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.is_cuda
    loss.backward()
    assert len(launches) == 1 and len(launches[0][3]) == 2 * b     # every set rides ONE launch twice
    want, bound = 0.0, 0.0
    for i in range(b):
        for t_ref in ("end", "start"):
            t0, scale = metric_refs(events[i], t_ref)
            ref = loss_reference(events[i], flows[i].double(), t0, scale, maps[i], eps=EPS)
            want += ref["loss"] / b
            bound += loss_bound(ref) / b
    print("timestamp_loss", float(loss), "restatement", want, "bound", bound)
    assert abs(float(loss.detach()) - want) <= bound
    # the same through timestamp_loss_many, and normalize="none"
    for normalize in ("active", "none"):
        many = sum(tsimg.timestamp_loss_many(evs, [pred[i].detach() for i in range(b)], t_ref=t_ref, maps=maps, normalize=normalize)
                   for t_ref in ("end", "start"))
        assert many.shape == (b,) and many.dtype == torch.float64
        if normalize == "active":
            assert abs(float(many.mean()) - float(loss.detach())) <= 1e-6 * float(loss.detach())   # (T to one fp32 ulp from run to run)
    # the backward.  Each job's gradient is within the per-cell bound; autograd adds the two references' fp32 gradients of a
    # sample in fp32: one more rounding of the sum
    t0s, scales, mps, timgs, dimgs, moments = launches[0]
    for i in range(b):
        total_ref, total_bound = torch.zeros(2, h, w, dtype=torch.float64), torch.zeros(2, h, w, dtype=torch.float64)
        for r, t_ref in enumerate(("end", "start")):
            j = r * b + i
            assert (t0s[j], scales[j]) == metric_refs(events[i], t_ref) and tuple(mps[j]) == tuple(maps[i])
            D32, T32 = dimgs[j].cpu(), timgs[j].cpu()
            coef = 1.0 / (b * (float(moments[j, 2]) + 1e-9))
            gref, A = grad_reference(events[i], flows[i], D32, T32, coef, EPS, t0s[j], scales[j], maps[i])
            f64 = flows[i].double().requires_grad_(True)
            la, _, _, _ = loss_autograd(events[i], f64, t0s[j], scales[j], maps[i], eps=EPS, D32=D32, T32=T32)
            (auto,) = torch.autograd.grad(la / b, f64)
            assert float((auto - gref).abs().max()) <= 1e-12 * float(gref.abs().max())
            total_ref += auto
            total_bound += C_A[form] * A + 2.0 ** -23 * gref.abs() + 1e-12 * float(gref.abs().max())
        d = (pred.grad[i].cpu().double() - total_ref).abs()
        bnd = total_bound + 2.0 ** -23 * total_ref.abs()
        print(f"sample {i}: max|ref| {float(total_ref.abs().max()):.3e} max|d| {float(d.max()):.3e} worst {float((d / (bnd + 1e-300)).max()):.3f}")
        assert float(total_ref.abs().max()) > 0 and bool((d <= bnd).all())
    # RSAT against the restatement's ratio: the relative bounds of numerator and denominator add
    for t_ref in ("end", "start"):
        got = tsimg.rsat_many(evs[:1], [pred[0].detach()], t_ref=t_ref, offset=(0, 0)).cpu()
        t0, scale = metric_refs(events[0], t_ref)
        num = loss_reference(events[0], flows[0].double(), t0, scale, eps=EPS)
        den = loss_reference(events[0], None, t0, scale, eps=EPS, size=(h, w))
        want = num["loss"] / den["loss"]
        rel = loss_bound(num) / num["loss"] + loss_bound(den) / den["loss"]
        print("rsat", t_ref, float(got[0]), "restatement", want, "relative bound", rel)
        assert abs(float(got[0]) - want) <= 1.01 * rel * want
        assert abs(want - rsat_reference(events[0], flows[0].double(), t0, scale)) <= 1e-15
        assert abs(float(tsimg.rsat(evs[0], pred[0].detach(), t_ref=t_ref)) - float(got[0])) <= 1e-6 * want


# ------------------------------------------------------------------------------------------------ 8: sign and usefulness
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


def restated_timestamp_loss(ev, flow64):
    return sum(loss_autograd(ev, flow64, *metric_refs(ev, t_ref), eps=EPS)[0] for t_ref in ("end", "start"))


def test_true_flow_lowers_the_loss_and_gradient_steps_follow(form):
    """Events made by a constant true flow F.  RSAT under F is below 0.9 for both time references; ten plain gradient steps of size 2.0
    on the flow tensor itself, from F / 2, end with a lower timestamp_loss than they began with (the descent is not monotone, and RSAT
    at F / 2 is above 1: neither is demanded).  The same conditions are asserted on the CPU restatement first, so the inputs are shown
    to be suitable whatever the library does."""
    h, w, F = 32, 40, (3.0, -2.0)
    ev = moving_points(5, h, w, 40, 30, F)
    true = torch.stack([torch.full((h, w), F[0]), torch.full((h, w), F[1])])
    for t_ref in ("end", "start"):
        want = rsat_reference(ev, true.double(), *metric_refs(ev, t_ref))
        got = float(tsimg.rsat(ev.to(DEV), true.to(DEV), t_ref=t_ref))
        print("rsat under the true flow", t_ref, got, "restatement", want)
        assert want < 0.9 and got < 0.9
    f64 = (true / 2).double()
    vals = []
    for _ in range(10):
        f64.requires_grad_(True)
        loss = restated_timestamp_loss(ev, f64)
        vals.append(float(loss))
        (g,) = torch.autograd.grad(loss, f64)
        f64 = (f64 - 2.0 * g).detach()
    vals.append(float(restated_timestamp_loss(ev, f64)))
    print("restatement over the steps", ["%.4f" % v for v in vals])
    assert vals[-1] < vals[0]
    flow = (true / 2).to(DEV)
    dev_ev = ev.to(DEV)
    got = []
    for _ in range(10):
        flow.requires_grad_(True)
        loss = tsimg.timestamp_loss([dev_ev], [flow])
        got.append(float(loss))
        (g,) = torch.autograd.grad(loss, flow)
        flow = (flow - 2.0 * g).detach()
    got.append(float(tsimg.timestamp_loss([dev_ev], [flow])))
    print("timestamp_loss over the steps", ["%.4f" % v for v in got])
    assert got[-1] < got[0]
    assert abs(got[0] - vals[0]) <= 1e-5 * vals[0]                 # the same start (bound 3 is far below this)


# ------------------------------------------------------------------------------------------------ 9: through the models
def eemflow_net(seed):
    from eemflow_amd import EEMFlow
    net = EEMFlow("", groups=5, n_first_channels=5)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(seed).items()})
    return net.to(DEV).train()


def synthetic_batch(seed, b, h, w, with_flow=True):
    """A batch as the datasets' get_batch makes it for flipped and cropped samples (the source frame is 8 px larger each way)."""
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


class Lines(Logger):
    def __init__(self):
        super().__init__(verbose=False)
        self.lines = []

    def write_line(self, line, *a, **k):
        self.lines.append(line)


def test_trainer_with_timestamp_term():
    """TrainRaftEvents(engine='autograd', timestamp_weight=0.5) on EEMFlow at 64 x 64, batch 2: the step's loss is the supervised loss
    plus 0.5 times the term computed separately, and every parameter gets a finite gradient."""
    h, w = 64, 64
    batch = synthetic_batch(80, 2, h, w)
    net = eemflow_net(77)
    log = Lines()
    tr = TrainRaftEvents([batch], (h, w), lr=1e-5, clip=1e9, logger=log, print_freq=1, engine="autograd", mixed_precision=False,
                         timestamp_weight=0.5)
    tr.train_iters(net, val_iters=1)
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and max(float(g.abs().max()) for g in grads) > 0
    assert len(log.lines) == 1 and "loss" in log.lines[0]
    ref = eemflow_net(77)
    ref.change_imagesize((h, w))
    with torch.no_grad():
        _, preds = ref(batch["event_volume_old"], batch["event_volume_new"])
        sup, _ = hip_train.sequence_loss(preds, batch["flow"], batch["valid"], 0.8)
        term = hip_train.timestamp_loss(preds[-1], batch["events"], batch["events_map"])
    assert tuple(preds[-1].shape[-2:]) == (h, w) and float(term) > 0
    logged = float(log.lines[0].split("loss")[1].split()[0])
    total = float(sup) + 0.5 * float(term)
    print("trainer: supervised", float(sup), "term", float(term), "logged", logged)
    assert abs(logged - total) <= 1e-5 * (1.0 + abs(total))         # (the loop adds the two in fp32 and prints six decimals)
    # the term's own gradient reaches the parameters
    ref.zero_grad()
    _, preds = ref(batch["event_volume_old"], batch["event_volume_new"])
    hip_train.timestamp_loss(preds[-1], batch["events"], batch["events_map"]).float().backward()
    assert max(float(p.grad.abs().max()) for p in ref.parameters() if p.grad is not None) > 0


def test_trainer_self_supervised_on_the_timestamp_term_alone():
    h, w = 64, 64
    batches = [synthetic_batch(100, 2, h, w, with_flow=False), synthetic_batch(110, 2, h, w, with_flow=False)]
    assert "flow" not in batches[0] and "valid" not in batches[0]
    net = eemflow_net(78)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    log = Lines()
    tr = TrainRaftEvents(batches, (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd", timestamp_weight=1.0, supervised=False)
    tr.train_iters(net, val_iters=2)
    assert len(log.lines) == 2 and tr.iteration == 2
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert any(not torch.equal(p.detach(), before[k]) for k, p in net.named_parameters())


def eraft_step(h, w, term):
    """One forward and backward of E-RAFT (two iterations, batch 2) under `term(prediction, batch)`: (loss, dL/d prediction, the
    names of the parameters whose gradient is not finite, the largest finite gradient entry).  term=None: the predictions alone."""
    from eemflow_amd.eraft import ERAFT
    torch.manual_seed(5)
    net = ERAFT("", n_first_channels=5).to(DEV).train()
    net.change_imagesize((h, w))
    b = synthetic_batch(120, 2, h, w, with_flow=False)
    preds = net(b["event_volume_old"], b["event_volume_new"], iters=2)[1]
    assert tuple(preds[-1].shape) == (2, 2, h, w) and preds[-1].requires_grad
    if term is None:
        return preds
    assert bool(torch.isfinite(preds[-1]).all())
    loss = term(preds[-1], b)
    (g,) = torch.autograd.grad(loss, preds[-1], retain_graph=True)
    loss.backward()
    named = [(n, p.grad) for n, p in net.named_parameters() if p.grad is not None]
    assert named
    bad = sorted(n for n, gr in named if not bool(torch.isfinite(gr).all()))
    big = max(float(torch.nan_to_num(gr, nan=0.0, posinf=0.0, neginf=0.0).abs().max()) for _, gr in named)
    return float(loss.detach()), g, bad, big


def test_timestamp_loss_through_eraft():
    """One step through E-RAFT with two iterations, batch 2, at the size E-RAFT's training tests use (128 x 160): a finite loss, a finite
    non-zero gradient into the prediction, finite gradients in every parameter.
    At 64 x 64 the coarsest level of the correlation pyramid is 1 x 1, where the reference's lookup divides by W - 1 = 0
    (bilinear_sampler, as this library restates it): its 81 features are not finite under ANY input, and since every ReLU keeps a NaN
    as torch.relu does (no kernel turns a NaN into a number) neither is any prediction - the reference's own result at that
    size.  (The ReLU behind convc1 used to map NaN to 0, which hid them in the forward and switched the correlation branch off; this
    test then held the term to what a plain loss reached there.)  So 64 x 64 is held to that: both predictions are NaN throughout."""
    def term(pred, b):
        return hip_train.timestamp_loss(pred, b["events"], b["events_map"]).float()
    preds = eraft_step(64, 64, None)
    print("E-RAFT 64x64: finite values per prediction", [int(torch.isfinite(p).sum()) for p in preds])
    assert len(preds) == 2 and not any(bool(torch.isfinite(p).any()) for p in preds)
    loss, g, bad, big = eraft_step(128, 160, term)
    print("E-RAFT 128x160: loss", loss, "max|dL/dpred|", float(g.abs().max()), "non-finite", bad)
    assert math.isfinite(loss) and loss > 0 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and big > 0
    assert bad == []


LINE = re.compile(r"^(\d{5} / \d{5}  AEE: \S+  meanAEE:\S+ 3 - mean %AEE: \S+)(?:  FWL: (\S+)  meanFWL:(\S+))?(?:  RSAT: (\S+)  meanRSAT:(\S+))?$")


def mvsec_tree(tmp_path, with_events, n_samples=5, first=40):
    """6 windows of 260 x 346 with 3000 events each: flow .npy files on disk, events from an injected reader."""
    from eemflow_amd.mvsec import MvsecEventFlow
    flow_dir = tmp_path / "dataset" / "MVSEC" / "seqA" / "flowgt_dt1"
    flow_dir.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(5)
    for i in range(first, first + n_samples):
        np.save(flow_dir / f"{i}.npy", rng.normal(0, 2, (2, 260, 346)).astype(np.float32))

    def reader(path):
        k = int(os.path.basename(path).split(".")[0])
        r = np.random.default_rng(20_000 + k)
        m = 3000
        ts = np.sort(r.uniform(k * 0.05, (k + 1) * 0.05, m))
        return np.stack([ts, r.integers(0, 346, m), r.integers(0, 260, m), r.integers(0, 2, m) * 2 - 1], axis=1).astype(np.float64)

    args = {"eval_type": "dense", "num_voxel_bins": 5, "sequence": "seqA"}
    return MvsecEventFlow(args, train=False, root=str(tmp_path), events_reader=reader, valid_time_index={"seqA": [(first, first + n_samples)]},
                          with_events=with_events)


@pytest.mark.parametrize("stream", [4, 0])
def test_harness_lines_carry_rsat(tmp_path, capsys, monkeypatch, stream):
    from eemflow_amd import EEMFlow
    monkeypatch.delenv("EEM_IWE_DIRECT", raising=False)
    monkeypatch.setenv("EEM_WINO4_LAYERS", "7")              # one encoder form whatever the call's batch (as test_gpu_stream pins it)
    monkeypatch.setenv("EEM_DEC_WNC", "1")
    ds = mvsec_tree(tmp_path, True)
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(68).items()})
    net = net.to(DEV)
    logger = Logger(verbose=False)
    tester = TestRaftEvents(ds, (256, 256), logger=logger)
    extra = {"stream": stream} if stream else {}
    capsys.readouterr()
    plain = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, **extra)
    plain_lines = [m for m in map(LINE.match, capsys.readouterr().out.splitlines()) if m]
    assert len(plain_lines) == 5 and all(m.group(2) is None and m.group(4) is None for m in plain_lines)
    assert not any(l.startswith("Mean RSAT") for l in logger.lines)

    seen = []                                                # what the loop's own rsat_many calls returned, in sample order
    real = tsimg.rsat_many
    monkeypatch.setattr(tsimg, "rsat_many", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    with_rsat = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, rsat=True, **extra)
    monkeypatch.setattr(tsimg, "rsat_many", real)
    lines = [m for m in map(LINE.match, capsys.readouterr().out.splitlines()) if m]
    assert with_rsat == plain and len(lines) == 5
    assert [m.group(1) for m in lines] == [m.group(1) for m in plain_lines]          # the lines minus the RSAT fields
    assert all(m.group(2) is None for m in lines)                                    # (no FWL was asked for)
    assert len(seen) == (2 if stream else 5)                 # one call per chunk
    values = torch.cat(seen).cpu().tolist()
    with torch.no_grad():
        if stream:
            pairs = [(t_, f_) for _, targets, flows in stream_chunks(ds, net, stream, torch.device(DEV)) for t_, f_ in zip(targets, flows)]
        else:
            net.change_imagesize((256, 256))
            pairs = []
            for idx in range(5):
                sample = ds[idx]
                pairs.append((sample, tester.run_network(net, sample, torch.device(DEV))))
    assert len(pairs) == 5
    running, count = 0.0, 0
    for i, (carrier, flow) in enumerate(pairs):
        own = tsimg.rsat_many([carrier['events']], [flow[0].contiguous()], offset=carrier['events_offset'])[0].item()
        print(i, "RSAT", values[i], "own call", own)
        assert own > 0 and abs(values[i] - own) <= 1e-6 * abs(own)  # (T to one fp32 ulp from run to run)
        running, count = running + values[i], count + 1
        assert lines[i].group(4) == '{:2.6f}'.format(values[i]) and lines[i].group(5) == '{:2.6f}'.format(running / count)
    assert [l for l in logger.lines if l.startswith("Mean RSAT")] == ["Mean RSAT: {:.6f}".format(running / count)]
    # both numbers on one line
    tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, rsat=True, fwl=True, **extra)
    both = [m for m in map(LINE.match, capsys.readouterr().out.splitlines()) if m]
    assert len(both) == 5 and all(m.group(2) is not None and m.group(4) is not None for m in both)
