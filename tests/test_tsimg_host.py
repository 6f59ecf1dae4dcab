"""Host-side checks of the image of average timestamps (eemflow_amd/csrc/tsimg.hip, eemflow_amd/tsimg.py): the explicit gradient
formula the kernels implement (tests/tsimg_reference.py) against torch autograd in fp64 and against a central difference, the C ABI's
declarations, the build's settings, and the argument checks of the Python functions, the trainer's term and the parser.  No GPU."""
import os

import numpy as np
import pytest
import torch

import eemflow_amd
from eemflow_amd import _lib, tsimg
from eemflow_amd.harness import Logger, TrainRaftEvents

from iwe_grad_reference import integer_distance, warped_positions
from iwe_reference import metric_refs
from test_iwe_grad_host import Cuda, cuda, fractional_events, wavy_flow      # noqa: F401  (helpers, re-used as they are)
from tsimg_reference import grad_reference, loss_autograd, loss_fp64, loss_reference

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("h,w,n", [(9, 12, 600), (17, 13, 1500)])
@pytest.mark.parametrize("amap", [(1.0, 0.0, 1.0, 0.0), (-1.0, 10.25, 1.0, -1.5)])
@pytest.mark.parametrize("normalize", ["active", "none"])
def test_formula_equals_autograd_with_straight_through_rounding(h, w, n, amap, normalize):
    """G = ((2 T) (ah - T)) / (D + eps) and what follows it, from the stored fp32 images, against torch autograd in fp64 through
    warp_direct and the planes with the roundings straight-through: 1e-12 relative to the largest gradient, fractional events that
    partly lie outside, both time references."""
    ev = fractional_events(11 + h, n, h, w)
    flow = wavy_flow(h, w, 5).requires_grad_(True)
    for t_ref in ("end", "start"):
        t0, scale = metric_refs(ev, t_ref)
        loss, D32, T32, m = loss_autograd(ev, flow, t0, scale, amap, normalize=normalize)
        (auto,) = torch.autograd.grad(loss, flow)
        assert m[2] > 0 and float(T32.max()) > 0.5
        upstream = -0.37
        coef = upstream / (m[2] + 1e-9) if normalize == "active" else upstream
        ref, A = grad_reference(ev, flow.detach(), D32, T32, coef, 1e-9, t0, scale, amap)
        big = float(auto.abs().max())
        assert big > 1e-3                                          # (a real gradient, not zeros against zeros)
        assert float((ref - upstream * auto).abs().max()) <= 1e-12 * abs(upstream) * big
        assert bool((A + 1e-300 >= ref.abs() * (1 - 1e-9)).all())      # the abs-sum map bounds the gradient cell by cell


def test_directional_derivative_equals_a_central_difference():
    """<gradient, d> of the fp64 loss against (L(F + s d) - L(F - s d)) / (2 s) along a random direction.  Between two changes of cell
    L is a rational function of s with denominators D + eps >= the smallest vote sum of an active cell, so the central difference is
    off by O(s^2) relative (s = 1e-5) and by the cancellation 2^-53 L / s (1e-11 relative); 1e-6 relative is asserted."""
    h, w, s = 21, 30, 1e-5
    ev = fractional_events(4, 3000, h, w)
    flow = wavy_flow(h, w, 9)
    d = torch.from_numpy(np.random.default_rng(1).standard_normal((2, h, w)))
    t0, scale = metric_refs(ev, "end")
    keep = torch.ones(ev.shape[0], dtype=torch.bool)
    for f in (flow + s * d, flow - s * d, flow):                   # build the case: drop events that come near an integer
        xw, yw = warped_positions(ev, f, t0, scale)
        keep &= ((xw - torch.round(xw)).abs() > 2e-3) & ((yw - torch.round(yw)).abs() > 2e-3)
    ev = ev[keep].contiguous()
    assert ev.shape[0] > 2000
    t0, scale = metric_refs(ev, "end")
    for f in (flow + s * d, flow - s * d):
        assert integer_distance(ev, f, t0, scale) >= 1e-3
    xa, ya = warped_positions(ev, flow + s * d, t0, scale)
    xb, yb = warped_positions(ev, flow - s * d, t0, scale)
    assert bool((torch.floor(xa) == torch.floor(xb)).all() and (torch.floor(ya) == torch.floor(yb)).all())
    for normalize in ("active", "none"):
        loss, D, T = loss_fp64(ev, flow, t0, scale, normalize=normalize)
        active = float(((D[0] + D[1]) > 0).sum())
        coef = 1.0 / (active + 1e-9) if normalize == "active" else 1.0
        grad, _ = grad_reference(ev, flow, D, T, coef, 1e-9, t0, scale)        # (the "stored" images are the fp64 ones here)
        analytic = float((grad * d).sum())
        numeric = float(loss_fp64(ev, flow + s * d, t0, scale, normalize=normalize)[0]
                        - loss_fp64(ev, flow - s * d, t0, scale, normalize=normalize)[0]) / (2 * s)
        assert abs(analytic) > 1e-4
        assert abs(analytic - numeric) <= 1e-6 * abs(analytic), (normalize, analytic, numeric)


def test_a_cell_of_one_event_holds_its_timestamp_value():
    """The quantised planes: N / D of a cell that a single event voted into is that event's ah, to fp64 round-off - no cancellation
    noise from the weights - and piling events up earns nothing: 50 copies of an event give the same T."""
    h, w = 6, 7
    ev = torch.tensor([[0.0, 1.3, 2.6, 1.0], [0.4, 4.2, 1.1, -1.0], [1.0, 5.5, 4.5, 1.0]], dtype=torch.float64)
    t0, scale = metric_refs(ev, "end")
    r = loss_reference(ev, None, t0, scale, quantised=True, size=(h, w))
    ah = (1.0 - ((ev[:, 0] - t0) * scale).abs()).float().double()
    assert r["moments"][2] == 12.0                                 # three events, four cells each, no cell shared
    T = r["N"] / (r["D"] + 1e-300)
    assert abs(float(T[1, 1, 4]) - float(ah[1])) <= 1e-15
    piled = torch.cat([ev[:1]] + [ev[1:2]] * 50 + [ev[2:]])
    r2 = loss_reference(piled, None, t0, scale, quantised=True, size=(h, w))
    # (what is left is eps = 1e-9 beside D: T changes by at most eps / D relative, D >= 0.2 * 0.1 here, and T^2 by twice that)
    assert float((r2["T"] - r["T"]).abs().max()) <= 1e-9 / 0.02
    assert abs(r2["loss"] - r["loss"]) <= 2 * 1e-9 / 0.02 * r["loss"]


def test_abi_is_declared_with_its_replaces_lines():
    header = open(os.path.join(HERE, "..", "include", "eemflow_hip.h")).read()
    for name in ("eemflow_tsimg_many", "eemflow_tsimg_grad_many", "eemflow_tsimg_last_form"):
        assert name in _lib.EXPORTS
        at = header.index(name + "(")
        comment = header[header.rindex("/*", 0, at):at]
        assert "Replaces:" in comment and "utils_luo/event_utils.py:9-51" in comment
        assert "has no counterpart in the reference" in " ".join(comment.replace("\n *", " ").split())
    from eemflow_amd.build import EXTRA, SOURCES
    assert "tsimg.hip" in SOURCES and "-ffp-contract=off" in EXTRA["tsimg.hip"]
    assert "-ffp-contract=off" in EXTRA["iwe_grad.hip"] and "-ffp-contract=off" in EXTRA["iwe.hip"]
    csrc = os.path.join(HERE, "..", "eemflow_amd", "csrc")
    text = open(os.path.join(csrc, "tsimg.hip")).read()
    # the per-event functions and the gradient kernels are shared, not copied
    assert '#include "iwe_grad_shared.h"' in text and "void iwe_sample(" not in text and "iwe_grad_event(" not in text.split("namespace {", 1)[1]
    assert '#include "iwe_grad_shared.h"' in open(os.path.join(csrc, "iwe_grad.hip")).read()
    assert '#include "iwe_shared.h"' in open(os.path.join(csrc, "iwe_grad_shared.h")).read()
    # one forward: both objectives instantiate iwe_fwd_shared.h's kernels and define none of their own (iwe.hip: the warp alone)
    iwe_text = open(os.path.join(csrc, "iwe.hip")).read()
    assert '#include "iwe_fwd_shared.h"' in text and '#include "iwe_fwd_shared.h"' in iwe_text
    assert text.count("__global__") == 0 and iwe_text.count("__global__") == 1 and "iwe_warp_kernel" in iwe_text
    switches = open(os.path.join(csrc, "switches.def.h")).read()
    assert "TSIMG" not in switches.upper() and "TIMESTAMP" not in switches.upper()      # no new switch: the IWE's two apply
    for name in ("avg_timestamps", "avg_timestamps_many", "timestamp_loss", "timestamp_loss_many", "rsat", "rsat_many"):
        assert getattr(eemflow_amd, name) is getattr(tsimg, name)


def test_argument_validation():
    ev, flow = torch.zeros(5, 4, dtype=torch.float64), torch.zeros(2, 8, 8)
    many = (tsimg.avg_timestamps_many, tsimg.timestamp_loss_many, tsimg.timestamp_loss, tsimg.rsat_many)
    for fn in many:
        with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
            fn([ev], [flow])
        with pytest.raises(ValueError, match=r"\(N,4\) float64"):
            fn([cuda(ev.float())], [cuda(flow)])
        with pytest.raises(ValueError, match=r"\(2,H,W\) float32"):
            fn([cuda(ev)], [cuda(flow.double())])
        with pytest.raises(ValueError, match="one .2,H,W. shape"):
            fn([cuda(ev), cuda(ev)], [cuda(flow), cuda(torch.zeros(2, 8, 9))])
        with pytest.raises(ValueError, match="one flow"):
            fn([cuda(ev), cuda(ev)], [cuda(flow)])
        with pytest.raises(ValueError, match="offset"):
            fn([cuda(ev)], [cuda(flow)], offset=3)
        with pytest.raises(ValueError, match="eps"):
            fn([cuda(ev)], [cuda(flow)], eps=0.0)
        with pytest.raises(ValueError, match="eps"):
            fn([cuda(ev)], [cuda(flow)], eps="tiny")
        with pytest.raises(TypeError):
            fn([np.zeros((5, 4))], [cuda(flow)])
    for fn in (tsimg.avg_timestamps_many, tsimg.timestamp_loss_many, tsimg.rsat_many):
        with pytest.raises(ValueError, match="t_ref"):
            fn([cuda(ev)], [cuda(flow)], t_ref="middle")
    for fn in (tsimg.avg_timestamps_many, tsimg.timestamp_loss_many, tsimg.timestamp_loss):
        with pytest.raises(ValueError, match="one map"):
            fn([cuda(ev)], [cuda(flow)], maps=[(1, 0, 1, 0), (1, 0, 1, 0)])
        with pytest.raises(ValueError, match=r"\(ax, bx, ay, by\)"):
            fn([cuda(ev)], [cuda(flow)], maps=[(1, 0, 1)])
    for fn in (tsimg.timestamp_loss_many, tsimg.timestamp_loss):
        with pytest.raises(ValueError, match="normalize"):
            fn([cuda(ev)], [cuda(flow)], normalize="pixels")
    for fn in (tsimg.timestamp_loss, tsimg.rsat_many):
        with pytest.raises(ValueError, match="needs its flow"):
            fn([cuda(ev)], [None])
    for fn in (tsimg.avg_timestamps_many, tsimg.timestamp_loss_many):
        with pytest.raises(ValueError, match="size="):
            fn([cuda(ev)], [None])
    # the one-job forms hand on to the many-job forms
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        tsimg.avg_timestamps(ev, flow)
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        tsimg.rsat(ev, flow)
    with pytest.raises(ValueError, match="t_ref"):
        tsimg.rsat(cuda(ev), cuda(flow), t_ref="middle")
    with pytest.raises(ValueError, match=r"\(ax, bx, ay, by\)"):
        tsimg.avg_timestamps(cuda(ev), cuda(flow), maps=(1, 0, 1))
    from eemflow_amd.train import timestamp_loss
    with pytest.raises(ValueError, match=r"\(B,2,H,W\)"):
        timestamp_loss(torch.zeros(2, 8, 8), [ev])
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        timestamp_loss(torch.zeros(1, 2, 8, 8), [ev])
    with pytest.raises(ValueError, match="one event set per sample"):
        timestamp_loss(cuda(torch.zeros(2, 2, 8, 8)), [ev])


def test_trainer_refuses_what_the_timestamp_term_cannot_do():
    quiet = Logger(verbose=False)
    with pytest.raises(ValueError, match="autograd"):              # the fused engine with a weight
        TrainRaftEvents([], (64, 64), engine="fused", timestamp_weight=0.5, logger=quiet)
    with pytest.raises(ValueError, match="no loss"):               # still no loss without any term
        TrainRaftEvents([], (64, 64), engine="autograd", supervised=False, logger=quiet)
    tr = TrainRaftEvents([], (64, 64), engine="autograd", timestamp_weight=0.5, supervised=False, logger=quiet)   # the only term
    assert tr.timestamp_weight == 0.5 and tr.contrast_weight == 0.0 and not tr.supervised
    assert TrainRaftEvents([], (64, 64), logger=quiet).timestamp_weight == 0.0
    volume = torch.zeros(2, 5, 64, 64)
    with pytest.raises(ValueError, match="timestamp_weight needs batches.*with_events"):     # batches without events
        tr._timestamp_term(torch.zeros(2, 2, 64, 64), {"event_volume_old": volume}, volume)
    ev = torch.zeros(5, 4, dtype=torch.float64)
    batch = {"event_volume_old": volume, "events": [ev, ev], "events_offset": [(0, 0), (3, 1)]}
    with pytest.raises(ValueError, match="out_mesh_size"):         # a mesh-size prediction
        tr._timestamp_term(torch.zeros(2, 2, 16, 16), batch, volume)
    # the first batch of a loader without events is refused before any GPU work
    with pytest.raises(ValueError, match="with_events"):
        tr._contrast_inputs({"event_volume_old": volume}, "timestamp_weight")


def test_parser_takes_the_timestamp_options():
    from eemflow_amd import cli
    args = cli.build_parser().parse_args(["train"])
    assert args.timestamp_weight == 0.0
    args = cli.build_parser().parse_args(["train", "--timestamp_weight", "0.5", "--self_supervised"])
    assert args.timestamp_weight == 0.5 and args.self_supervised is True and args.contrast_weight == 0.0
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["test", "--timestamp_weight", "0.5"])
    assert cli.build_parser().parse_args(["test"]).rsat is False
    assert cli.build_parser().parse_args(["test", "--rsat"]).rsat is True
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["train", "--rsat"])
    with pytest.raises(SystemExit, match="timestamp_weight"):      # --self_supervised still needs a term, and names this one
        cli.train(cli.build_parser().parse_args(["train", "--self_supervised"]))


def test_evaluation_refuses_rsat_without_events():
    from eemflow_amd.harness import TestRaftEvents

    class NoEvents:
        with_events = False
    ev = TestRaftEvents.__new__(TestRaftEvents)
    ev.dataset = NoEvents()
    with pytest.raises(ValueError, match="rsat= needs a dataset"):
        ev.test_multi_sequence(None, rsat=True)


def test_last_form_is_empty_before_any_call_and_refused_calls_leave_it():
    """eemflow_tsimg_last_form in a thread that made no call: "" - and argument errors, which are refused before any launch, leave it
    (no GPU is touched: the refusals come first)."""
    import ctypes
    import threading
    got = {}

    def fresh():
        L = _lib.lib()
        got["before"] = tsimg.last_form()
        got["rc_many"] = L.eemflow_tsimg_many(0, None, None, None, None, None, None, 8, 8, 1e-9, None, None, None, None)
        got["rc_grad"] = L.eemflow_tsimg_grad_many(33, None, None, None, None, None, None, 8, 8, 1e-9, None, None, None, None, None)
        got["rc_form"] = L.eemflow_tsimg_last_form(None, 8)
        small = ctypes.create_string_buffer(1)
        got["rc_small"] = L.eemflow_tsimg_last_form(small, 1)
        got["after"] = tsimg.last_form()
    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert got["before"] == "" and got["after"] == ""
    assert got["rc_many"] != 0 and got["rc_grad"] != 0 and got["rc_form"] != 0 and got["rc_small"] == 0
