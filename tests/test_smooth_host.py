"""The edge-aware smoothness loss on the host: the reference's own results (tests/golden/smooth.npz, made by executing its sources)
against the restatement of tests/smooth_reference.py, the restatement's analytic gradient against fp64 autograd, and the argument
checks of eemflow_amd.smooth, the trainer and the CLI.  No GPU needed."""
import numpy as np
import pytest
import torch

from eemflow_amd import _lib, smooth
from eemflow_amd.harness import Logger, TrainRaftEvents

from smooth_reference import SETTINGS, gradient, smoothness, term_count


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("smooth.npz")
    assert g["settings"].tolist() == ["%d/%s/%s" % s for s in SETTINGS]
    return g


def test_golden_matches_the_fp32_restatement(cases):
    """The reference's fp32 losses against the restatement run in fp32: 4 * ref_gap relative, ref_gap the largest relative distance
    between a reference value and the fp64 restatement (about 1.2e-7: fp32 summation noise at these sizes)."""
    gap = float(cases["ref_gap"])
    assert 0.0 < gap < 2.0 ** -22
    assert int(cases["ncases"]) == 3 and cases["constants"].tolist() == [1.0, 0.7]
    shapes, worst = [], 0.0
    for k in range(3):
        pred, img = torch.from_numpy(cases[f"pred_{k}"]), torch.from_numpy(cases[f"img_{k}"])
        shapes.append(tuple(img.shape))
        assert pred.dtype == img.dtype == torch.float32 and pred.shape[1] == 2
        for ci, constant in enumerate(cases["constants"].tolist()):
            for si, (order, wt, et) in enumerate(SETTINGS):
                mine = smoothness(pred, img, order, constant, wt, et)
                assert mine.dtype == torch.float32
                ref = float(cases[f"loss_{k}"][ci, si])
                worst = max(worst, abs(float(mine) - ref) / abs(ref))
                wide = float(smoothness(pred.double(), img.double(), order, constant, wt, et))
                assert abs(wide - ref) <= gap * abs(wide) * (1 + 1e-9)
    print("restatement against the reference, worst relative difference %.3e (ref_gap %.3e)" % (worst, gap))
    assert shapes == [(1, 1, 3, 3), (2, 5, 5, 7), (3, 15, 37, 50)]
    assert worst <= 4 * gap


def test_flow_smooth_delta_is_the_unweighted_first_order_term(cases):
    gap = float(cases["ref_gap"])
    for k in range(3):
        pred = torch.from_numpy(cases[f"pred_{k}"])
        ref = float(cases[f"delta_{k}"])
        assert abs(float(smoothness(pred, None, 1, 1.0, "gauss", "L1")) - ref) <= 4 * gap * abs(ref)
        # without differences in img every weight is exp(-0) = 1
        ones = torch.ones(pred.shape[0], 3, *pred.shape[2:])
        assert abs(float(smoothness(pred, ones, 1, 1.0, "exp", "L1")) - ref) <= 4 * gap * abs(ref)


def test_inputs_hold_a_patch_of_constant_flow(cases):
    for k in range(3):
        pred = torch.from_numpy(cases[f"pred_{k}"])
        assert int((pred[:, :, :-1] == pred[:, :, 1:]).sum()) >= 2 and int((pred[..., :-1] == pred[..., 1:]).sum()) >= 2


@pytest.mark.parametrize("order,wt,et", SETTINGS)
def test_analytic_gradient_matches_fp64_autograd(cases, order, wt, et):
    for k in range(3):
        pred, img = torch.from_numpy(cases[f"pred_{k}"]).double(), torch.from_numpy(cases[f"img_{k}"]).double()
        for im, constant in ((img, 0.7), (None, 1.0)):
            p = pred.clone().requires_grad_(True)
            smoothness(p, im, order, constant, wt, et).backward()
            g, a = gradient(pred, im, order, constant, wt, et, coef=-1.5)
            assert float((g - (-1.5) * p.grad).abs().max()) <= 1e-14 * max(1.0, float(p.grad.abs().max()))
            assert bool((a >= g.abs() * (1 - 1e-12)).all())
    assert term_count((2, 2, 5, 7), order) == 2 * 2 * (5 - order) * 7 + 2 * 2 * 5 * (7 - order)


class Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the shape and dtype checks run without one."""
    is_cuda = True


def cuda(t):
    return t.as_subclass(Cuda)


def test_argument_validation():
    pred, img = torch.zeros(2, 2, 8, 8), torch.zeros(2, 5, 8, 8)
    for call in (lambda: smooth.smoothness_many([pred]), lambda: smooth.smoothness_loss(pred, img), lambda: smooth.smoothness_loss(cuda(pred), img)):
        with pytest.raises(_lib.EEMFlowHipError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match=r"\(B,2,H,W\) float32"):
        smooth.smoothness_many([cuda(torch.zeros(2, 8, 8))])
    with pytest.raises(ValueError, match=r"\(B,2,H,W\) float32"):
        smooth.smoothness_many([cuda(torch.zeros(2, 3, 8, 8))])
    with pytest.raises(ValueError, match=r"\(B,2,H,W\) float32"):
        smooth.smoothness_many([cuda(pred.double())])
    with pytest.raises(ValueError, match=r"\(B,C,H,W\) float32"):
        smooth.smoothness_loss(cuda(pred), cuda(img.double()))
    with pytest.raises(ValueError, match=r"\(B,C,H,W\) float32"):
        smooth.smoothness_loss(cuda(pred), cuda(img[0]))
    for bad in (torch.zeros(1, 5, 8, 8), torch.zeros(2, 5, 7, 8), torch.zeros(2, 5, 8, 9)):
        with pytest.raises(ValueError, match="B, H and W"):
            smooth.smoothness_loss(cuda(pred), cuda(bad))
    with pytest.raises(ValueError, match="share one"):
        smooth.smoothness_many([cuda(pred), cuda(torch.zeros(2, 2, 8, 9))])
    with pytest.raises(ValueError, match="per prediction"):
        smooth.smoothness_many([cuda(pred), cuda(pred)], [cuda(img)])
    with pytest.raises(ValueError, match="at least one"):
        smooth.smoothness_many([])
    with pytest.raises(TypeError):
        smooth.smoothness_many([np.zeros((2, 2, 8, 8), np.float32)])
    with pytest.raises(ValueError, match="order"):
        smooth.smoothness_loss(cuda(pred), order=3)
    with pytest.raises(ValueError, match="weight_type"):
        smooth.smoothness_loss(cuda(pred), weight_type="box")
    with pytest.raises(ValueError, match="error_type"):
        smooth.smoothness_loss(cuda(pred), error_type="L2")
    with pytest.raises(ValueError, match="H > 2"):
        smooth.smoothness_loss(cuda(torch.zeros(1, 2, 2, 8)), order=2)
    with pytest.raises(ValueError, match="W > 1"):
        smooth.smoothness_loss(cuda(torch.zeros(1, 2, 4, 1)), order=1)
    from eemflow_amd import smoothness_loss, smoothness_many
    assert smoothness_many is smooth.smoothness_many and smoothness_loss is smooth.smoothness_loss
    from eemflow_amd.train import smoothness_loss as train_term
    with pytest.raises(_lib.EEMFlowHipError, match="no CPU path"):
        train_term([pred, pred], img, gamma=0.8)
    with pytest.raises(ValueError, match="at least one"):
        train_term([], img)


def test_library_refuses_bad_calls_before_any_launch():
    """The C entry point's own checks (they return before a kernel is launched, so no GPU is needed): k, the shape, the enums."""
    import ctypes
    lib = _lib.lib()
    one = (ctypes.c_void_p * 1)(16)
    out = ctypes.c_void_p(16)

    def call(k=1, b=1, c=1, h=8, w=8, order=1, wt=0, et=0, loss=out, grad=None):
        return lib.eemflow_smoothness_many(k, one, None, b, c, h, w, order, wt, et, 1.0, None, loss, grad, out, None)
    for kw, word in ((dict(k=0), "jobs"), (dict(k=17), "jobs"), (dict(order=3), "order"), (dict(wt=2), "weight_type"), (dict(et=-1), "error_type"),
                     (dict(h=1), "H > 1"), (dict(w=2, order=2), "W > 2"), (dict(h=2, order=2), "H > 2"), (dict(b=0), "shape"),
                     (dict(loss=None), "neither")):
        assert call(**kw) != 0
        assert word in lib.eemflow_last_error().decode(), (kw, lib.eemflow_last_error())
    assert lib.eemflow_smoothness_scratch_doubles(0, 1, 8, 8) == 0 and lib.eemflow_smoothness_scratch_doubles(17, 1, 8, 8) == 0
    assert lib.eemflow_smoothness_scratch_doubles(3, 2, 17, 65) == 3 * (2 * 2 * 2) * 2          # 16 x 64 tiles, {axis 2, axis 3} per block
    assert lib.eemflow_smoothness_scratch_doubles(16, 8, 720, 1280) == 16 * 2048 * 2            # the grid is capped at 2048 blocks


def test_trainer_takes_the_smoothness_arguments():
    quiet = Logger(verbose=False)
    with pytest.raises(ValueError, match="autograd"):              # the fused engine with a weight
        TrainRaftEvents([], (64, 64), engine="fused", smooth_weight=0.1, logger=quiet)
    with pytest.raises(ValueError, match="no loss"):               # smoothness alone is minimised by a constant flow
        TrainRaftEvents([], (64, 64), engine="autograd", supervised=False, smooth_weight=0.1, logger=quiet)
    with pytest.raises(ValueError, match="order"):
        TrainRaftEvents([], (64, 64), engine="autograd", smooth_weight=0.1, smooth_order=3, logger=quiet)
    with pytest.raises(ValueError, match="error_type"):
        TrainRaftEvents([], (64, 64), engine="autograd", smooth_weight=0.1, smooth_error="L2", logger=quiet)
    tr = TrainRaftEvents([], (64, 64), logger=quiet)
    assert tr.smooth_weight == 0.0 and tr.smooth_all is False and tr.engine == "fused"
    tr = TrainRaftEvents([], (64, 64), engine="autograd", smooth_weight=0.1, smooth_order=2, smooth_constant=0.7, smooth_weight_type="exp",
                         smooth_error="abs_robust", smooth_all=True, logger=quiet)
    assert tr.smooth_weight == 0.1 and tr.smooth_all is True
    assert tr.smooth_kw == dict(order=2, constant=0.7, weight_type="exp", error_type="abs_robust")


def test_trainer_hands_the_volume_or_nothing_as_edge_image(monkeypatch):
    from eemflow_amd import harness
    seen = []
    monkeypatch.setattr(harness, "smoothness_loss", lambda preds, img, gamma=None, **kw: seen.append((len(preds), img, gamma, kw)) or torch.zeros(()))
    volume = torch.zeros(2, 5, 64, 64)
    full, mesh = [torch.zeros(2, 2, 64, 64)] * 3, [torch.zeros(2, 2, 16, 16)]
    tr = TrainRaftEvents([], (64, 64), engine="autograd", smooth_weight=0.1, gamma=0.85, logger=Logger(verbose=False))
    tr._smooth_term(full, volume)
    tr._smooth_term(mesh, volume)
    tr.smooth_all = True
    tr._smooth_term(full, volume)
    kw = dict(order=1, constant=1.0, weight_type="gauss", error_type="L1")
    assert seen[0] == (3, volume, None, kw) and seen[0][1] is volume
    assert seen[1] == (1, None, None, kw)                          # a mesh-size prediction: unweighted
    assert seen[2][2] == 0.85


def test_cli_flags_reach_the_trainer():
    from eemflow_amd import cli
    args = cli.build_parser().parse_args(["train"])
    assert cli.smooth_kw(args) == dict(smooth_weight=0.0, smooth_order=1, smooth_constant=1.0, smooth_weight_type="gauss", smooth_error="L1",
                                       smooth_all=False)
    args = cli.build_parser().parse_args(["train", "--smooth_weight", "0.1", "--smooth_order", "2", "--smooth_constant", "0.7",
                                          "--smooth_weight_type", "exp", "--smooth_error", "abs_robust", "--smooth_all", "-model", "eraft"])
    kw = cli.smooth_kw(args)
    assert kw == dict(smooth_weight=0.1, smooth_order=2, smooth_constant=0.7, smooth_weight_type="exp", smooth_error="abs_robust", smooth_all=True)
    tr = TrainRaftEvents([], (64, 64), engine="autograd", logger=Logger(verbose=False), **kw)
    assert tr.smooth_weight == 0.1 and tr.smooth_kw["order"] == 2 and tr.smooth_all
    for bad in (["--smooth_order", "3"], ["--smooth_weight_type", "box"], ["--smooth_error", "L2"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["train"] + bad)
    with pytest.raises(SystemExit):                                # a training flag
        cli.build_parser().parse_args(["test", "--smooth_weight", "0.1"])
    import inspect
    src = inspect.getsource(cli.train)
    assert "**smooth_kw(args)" in src and 'smooth == 0.0 else "autograd"' in src      # every model: the autograd engine with the term
