"""The weighted SSIM warp loss on the host: the reference's own results (tests/golden/ssim.npz, made by executing its sources) against
the restatement of tests/ssim_reference.py, the restatement's analytic gradient against fp64 autograd of an independent composition,
and the argument checks of eemflow_amd.ssim, the C entry point, the trainer and the CLI.  No GPU needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from eemflow_amd import _lib, ssim
from eemflow_amd.harness import Logger, TrainRaftEvents

import ssim_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 3, 7, 7), (2, 5, 9, 11), (2, 15, 37, 50), (2, 3, 33, 129)]
INF = float("inf")


def case_kw(case):
    occ, c1, c2 = case
    return dict(use_occ=occ, c1=c1, c2=c2)


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("ssim.npz")
    assert g["cases"].tolist() == [R.case_id(c) for c in R.CASES] and len(R.CASES) == 6
    assert int(g["ncases"]) == len(SHAPES)
    return g


def tensors(g, i):
    return tuple(torch.from_numpy(g[f"{n}_{i}"]) for n in ("flow", "img1", "img2", "mask"))


def test_golden_matches_the_fp32_restatement(cases):
    """The reference's fp32 losses against the restatement run in fp32 (its own fp32 warp, then every branch in fp32): 4 * ref_gap
    relative, ref_gap the largest relative distance between a reference value and the fp64 restatement - the fp32 rounding of the
    moments and of the sums at these sizes.  A ref_gap above 1e-6 would make the comparison vacuous."""
    gap = float(cases["ref_gap"])
    assert 0.0 < gap <= 1e-6
    worst = 0.0
    for i in range(len(SHAPES)):
        flow, img1, img2, mask = tensors(cases, i)
        assert tuple(img1.shape) == SHAPES[i] and flow.dtype == img1.dtype == img2.dtype == mask.dtype == torch.float32
        regenerated = R.inputs(int(cases["seed"]) + i, SHAPES[i])
        assert all(np.array_equal(a, b.numpy()) for a, b in zip(regenerated, (flow, img1, img2, mask)))
        for ci, case in enumerate(R.CASES):
            mine = R.loss(flow, img1, img2, mask, dtype=torch.float32, **case_kw(case))
            assert mine.dtype == torch.float32
            ref = float(cases[f"loss_{i}"][ci])
            worst = max(worst, abs(float(mine) - ref) / abs(ref))
            wide = float(R.loss(flow, img1, img2, mask, **case_kw(case)))
            assert abs(wide - ref) <= gap * abs(ref) * (1 + 1e-9)
    print("restatement against the reference, worst relative difference %.3e (ref_gap %.3e)" % (worst, gap))
    assert worst <= 4 * gap


def test_inputs_reach_the_clamp_and_the_mask(cases):
    """The golden inputs hold cells exactly on the clamp's lower end (windows where img1 and the warped img2 agree), cells strictly
    inside, pooled weights of 0, of 1 and in between, and the three branches differ."""
    for i in range(1, len(SHAPES)):
        flow, img1, img2, mask = tensors(cases, i)
        yw = R.warp_taps(img2, flow)["yw"]
        l, aw = R.cells_from_warped(img1.double(), yw.double(), mask.double())
        if l.numel() > 10000:                                      # (about one cell in a thousand)
            assert bool((l == 0).any())
        assert bool(((l > 0) & (l < 1)).any()) and float(l.max()) <= 1.0
        assert bool((aw == 0).any()) and bool((aw == 1).any()) and bool(((aw > 0) & (aw < 1)).any())
        values = [float(R.loss(flow, img1, img2, mask, **case_kw(c))) for c in R.CASES]
        assert len(set(values)) == len(values)
    with pytest.raises(ValueError, match="infinite"):
        R.loss(*tensors(cases, 0), c1=INF, c2=INF)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_analytic_gradient_matches_fp64_autograd(cases, case):
    """gradient() against autograd of loss_autograd (F.avg_pool2d, torch.clamp; the tap positions, weights and warped values held at
    their fp32 results): the two losses within (terms + 16) * 2^-52 + cancellation / loss relative, every gradient cell within
    cancellation * A of autograd's (ssim_reference.cancellation: the moments' rounding divided by min(c1, c2) - 1e-9 or so, where the
    photometric losses have 1e-14), and A bounds |g|."""
    kw = case_kw(case)
    for i in range(len(SHAPES)):
        flow, img1, img2, mask = tensors(cases, i)
        taps = R.warp_taps(img2, flow)
        tol = R.cancellation(img1, taps["yw"], kw["c1"], kw["c2"])
        for m in (mask, None):
            f = flow.double().requires_grad_(True)
            auto = R.loss_autograd(f, taps, img1, m, **kw)
            auto.backward()
            mine = float(R.loss(flow, img1, img2, m, **kw))
            assert abs(float(auto.detach()) - mine) <= ((R.term_count(img1.shape) + 16) * 2.0 ** -52) * mine + tol
            g, a = R.gradient(flow, img1, img2, m, coef=-1.5, **kw)
            assert g.shape == a.shape == f.grad.shape
            ratio = float(((g - (-1.5) * f.grad).abs() / a.clamp(min=1e-300)).max())
            assert bool(((g - (-1.5) * f.grad).abs() <= tol * a).all()), (ratio, tol)
            assert bool((a >= g.abs() * (1 - 1e-12)).all())
            assert float(g.abs().max()) > 0.0


def test_all_zero_mask_gives_zero_with_use_occ_and_a_loss_without():
    flow, img1, img2, mask = (torch.from_numpy(a) for a in R.inputs(5, (2, 5, 9, 11), zero_mask=True))
    for occ, c1, c2 in R.CASES:
        value = float(R.loss(flow, img1, img2, mask, use_occ=occ, c1=c1, c2=c2))
        g = R.gradient(flow, img1, img2, mask, use_occ=occ, c1=c1, c2=c2)[0]
        if occ:
            assert value == 0.0 and float(g.abs().max()) == 0.0
        else:                                                      # every weight is weight_epsilon: the unweighted moments
            assert value > 0.0 and float(g.abs().max()) > 0.0 and bool(torch.isfinite(g).all())


class Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the shape and dtype checks run without one."""
    is_cuda = True


def cuda(t):
    return t.as_subclass(Cuda)


def test_argument_validation():
    flow, img = torch.zeros(2, 2, 8, 8), torch.zeros(2, 5, 8, 8)
    mask = torch.zeros(2, 1, 8, 8)
    for call in (lambda: ssim.ssim_many([flow], img, img), lambda: ssim.ssim_loss(flow, img, img),
                 lambda: ssim.ssim_loss(cuda(flow), img, img), lambda: ssim.ssim_loss(cuda(flow), cuda(img), cuda(img), mask, use_occ=True)):
        with pytest.raises(_lib.EEMFlowHipError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="both infinite"):
        ssim.ssim_loss(flow, img, img, c1=INF, c2=INF)
    for bad in (dict(c1=0.0), dict(c2=-1.0), dict(c2=float("nan")), dict(c1=-INF)):
        with pytest.raises(ValueError, match="positive"):
            ssim.ssim_loss(flow, img, img, **bad)
    for bad in (0.0, -0.01, INF, float("nan")):
        with pytest.raises(ValueError, match="weight_epsilon"):
            ssim.ssim_loss(flow, img, img, weight_epsilon=bad)
    with pytest.raises(TypeError):                                 # the photometric kinds belong to photo_many
        ssim.ssim_loss(flow, img, img, kind="SSIM")
    with pytest.raises(ValueError, match=r"\(B,2,H,W\) float32"):
        ssim.ssim_many([cuda(torch.zeros(2, 3, 8, 8))], cuda(img), cuda(img))
    with pytest.raises(ValueError, match=r"\(B,2,H,W\) float32"):
        ssim.ssim_many([cuda(flow.double())], cuda(img), cuda(img))
    with pytest.raises(ValueError, match=r"\(B,C,H,W\) float32"):
        ssim.ssim_loss(cuda(flow), cuda(img.double()), cuda(img))
    with pytest.raises(ValueError, match=r"\(B,1,H,W\) float32"):
        ssim.ssim_loss(cuda(flow), cuda(img), cuda(img), cuda(torch.zeros(2, 2, 8, 8)), use_occ=True)
    for bad in (torch.zeros(1, 5, 8, 8), torch.zeros(2, 5, 7, 8), torch.zeros(2, 5, 8, 9)):
        with pytest.raises(ValueError, match="B, H and W"):
            ssim.ssim_loss(cuda(flow), cuda(img), cuda(bad))
    with pytest.raises(ValueError, match="B, H and W"):
        ssim.ssim_loss(cuda(flow), cuda(img), cuda(img), cuda(torch.zeros(2, 1, 8, 9)))
    with pytest.raises(ValueError, match="channel count"):
        ssim.ssim_loss(cuda(flow), cuda(img), cuda(torch.zeros(2, 3, 8, 8)))
    with pytest.raises(ValueError, match="share one"):
        ssim.ssim_many([cuda(flow), cuda(torch.zeros(2, 2, 8, 9))], cuda(img), cuda(img))
    with pytest.raises(ValueError, match="per flow"):
        ssim.ssim_many([cuda(flow), cuda(flow)], [cuda(img)], cuda(img))
    with pytest.raises(ValueError, match="required"):
        ssim.ssim_many([cuda(flow)], None, cuda(img))
    with pytest.raises(ValueError, match="at least one"):
        ssim.ssim_many([], img, img)
    with pytest.raises(TypeError):
        ssim.ssim_many([np.zeros((2, 2, 8, 8), np.float32)], img, img)
    with pytest.raises(ValueError, match="H >= 3"):
        ssim.ssim_loss(cuda(torch.zeros(1, 2, 2, 8)), cuda(torch.zeros(1, 3, 2, 8)), cuda(torch.zeros(1, 3, 2, 8)))
    with pytest.raises(ValueError, match="W >= 3"):
        ssim.ssim_loss(cuda(torch.zeros(1, 2, 8, 2)), cuda(torch.zeros(1, 3, 8, 2)), cuda(torch.zeros(1, 3, 8, 2)))
    from eemflow_amd import ssim_loss, ssim_many
    assert ssim_many is ssim.ssim_many and ssim_loss is ssim.ssim_loss
    from eemflow_amd.train import ssim_loss as train_term
    with pytest.raises(_lib.EEMFlowHipError, match="no CPU path"):
        train_term([flow, flow], img, img, gamma=0.8)
    with pytest.raises(ValueError, match="at least one"):
        train_term([], img, img)
    with pytest.raises(ValueError, match="both infinite"):
        train_term([flow], img, img, c1=INF, c2=INF)


def test_photo_many_points_to_the_term():
    """photo_many still refuses kind='SSIM'; its message names the kinds that exist and where SSIM lives."""
    from eemflow_amd import photo
    flow, img = torch.zeros(2, 2, 8, 8), torch.zeros(2, 5, 8, 8)
    with pytest.raises(ValueError, match=r"abs_robust.*census.*SSIM.*eemflow_amd\.ssim_loss"):
        photo.photo_loss(flow, img, img, kind="SSIM")


def test_library_refuses_bad_calls_before_any_launch():
    """The C entry point's own checks (they return before a kernel is launched, so no GPU is needed)."""
    lib = _lib.lib()
    one = (ctypes.c_void_p * 1)(16)
    none = (ctypes.c_void_p * 1)(None)
    out = ctypes.c_void_p(16)

    def call(k=1, b=1, c=3, h=8, w=8, c1=INF, c2=9e-6, eps=0.01, loss=out, grad=None, scratch=out, flow=one, img1=one, img2=one):
        return lib.eemflow_ssim_many(k, flow, img1, img2, None, b, c, h, w, 0, c1, c2, eps, None, loss, grad, scratch, None)
    for kw, word in ((dict(k=0), "jobs"), (dict(k=17), "jobs"), (dict(h=2), "H >= 3"), (dict(w=2), "W >= 3"), (dict(b=0), "shape"),
                     (dict(c=0), "channel"), (dict(c1=0.0), "positive"), (dict(c2=-1.0), "positive"), (dict(c2=float("nan")), "positive"),
                     (dict(c1=INF, c2=INF), "both infinite"), (dict(eps=0.0), "weight_epsilon"), (dict(eps=INF), "weight_epsilon"),
                     (dict(loss=None), "neither"), (dict(scratch=None), "scratch"), (dict(flow=None), "NULL"), (dict(img1=None), "NULL"),
                     (dict(img2=None), "NULL"), (dict(img2=none), "NULL"), (dict(flow=none), "NULL"), (dict(grad=none), "NULL")):
        assert call(**kw) != 0, kw
        assert word in lib.eemflow_last_error().decode(), (kw, lib.eemflow_last_error())
    assert lib.eemflow_ssim_scratch_doubles(0, 1, 8, 8) == 0 and lib.eemflow_ssim_scratch_doubles(17, 1, 8, 8) == 0
    assert lib.eemflow_ssim_scratch_doubles(1, 1, 2, 8) == 0 and lib.eemflow_ssim_scratch_doubles(1, 1, 8, 2) == 0
    assert lib.eemflow_ssim_scratch_doubles(3, 2, 17, 65) == 16 + 3 * (2 * 2 * 2)              # 16 denominators, then 16 x 64 tiles per job
    assert lib.eemflow_ssim_scratch_doubles(16, 8, 720, 1280) == 16 + 16 * 2048                # the grid is capped at 2048 blocks


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(HERE, "..", "include", "eemflow_hip.h")).read()
    for name in ("eemflow_ssim_many", "eemflow_ssim_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert "SSIM excepted" not in header
    build = open(os.path.join(HERE, "..", "eemflow_amd", "build.py")).read()
    assert '"ssim.hip"' in build and re.search(r'"ssim\.hip": \["-ffp-contract=off"\]', build)


def test_trainer_takes_the_ssim_arguments():
    quiet = Logger(verbose=False)
    with pytest.raises(ValueError, match="autograd"):              # the fused engine with a weight
        TrainRaftEvents([], (64, 64), engine="fused", ssim_weight=0.1, logger=quiet)
    with pytest.raises(ValueError, match="no loss.*contrast_weight or a photo_weight.*ssim_weight"):
        TrainRaftEvents([], (64, 64), engine="autograd", supervised=False, logger=quiet)
    with pytest.raises(ValueError, match="both infinite"):
        TrainRaftEvents([], (64, 64), engine="autograd", ssim_weight=0.1, ssim_c2=INF, logger=quiet)
    with pytest.raises(ValueError, match="positive"):
        TrainRaftEvents([], (64, 64), engine="autograd", ssim_weight=0.1, ssim_c1=0.0, logger=quiet)
    tr = TrainRaftEvents([], (64, 64), logger=quiet)               # the defaults: nothing asked for, the fused engine
    assert tr.ssim_weight == 0.0 and tr.ssim_occ is False and tr.ssim_all is False and tr.engine == "fused"
    assert tr.ssim_kw == dict(c1=INF, c2=9e-6)
    assert tr.photo_kw == dict(kind="census", q=0.4, charbonnier=False, max_distance=3)
    tr = TrainRaftEvents([], (64, 64), engine="autograd", supervised=False, ssim_weight=0.5, logger=quiet)      # a loss of its own
    assert tr.ssim_weight == 0.5 and tr.photo_weight == 0.0 and tr.ssim_kw == dict(c1=INF, c2=9e-6)
    tr = TrainRaftEvents([], (64, 64), engine="autograd", ssim_weight=0.1, ssim_occ=True, ssim_all=True, ssim_c1=1e-4, ssim_c2=INF, logger=quiet)
    assert tr.ssim_occ and tr.ssim_all and tr.ssim_kw == dict(c1=1e-4, c2=INF)
    assert tr.photo_kw == dict(kind="census", q=0.4, charbonnier=False, max_distance=3)


def test_trainer_hands_both_volumes_and_the_mask(monkeypatch):
    from eemflow_amd import harness
    seen = []
    monkeypatch.setattr(harness, "ssim_loss", lambda preds, a, b, gamma=None, mask=None, **kw: seen.append((len(preds), a, b, gamma, mask, kw))
                        or torch.zeros(()))
    e1, e2 = torch.zeros(2, 5, 64, 64), torch.ones(2, 5, 64, 64)
    full, mesh = [torch.zeros(2, 2, 64, 64)] * 3, [torch.zeros(2, 2, 16, 16)]
    tr = TrainRaftEvents([], (64, 64), engine="autograd", ssim_weight=0.1, ssim_c1=1e-4, gamma=0.85, logger=Logger(verbose=False))
    tr._ssim_term(full, e1, e2, None)
    with pytest.raises(ValueError, match="frame's size"):
        tr._ssim_term(mesh, e1, e2, None)
    tr.ssim_all = True
    tr._ssim_term(full, e1, e2, None)
    assert seen[0][0] == 3 and seen[0][1] is e1 and seen[0][2] is e2 and seen[0][3] is None and seen[0][4] is None
    assert seen[0][5] == dict(use_occ=False, c1=1e-4, c2=9e-6)
    assert seen[1][3] == 0.85


class Twice(torch.nn.Module):
    """A model of one parameter that counts its passes: flow = p * (old - new) over two channels."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.tensor(0.5))
        self.calls = []

    def change_imagesize(self, size):
        pass

    def forward(self, a, b):
        self.calls.append((a, b, torch.is_grad_enabled()))
        return None, [self.p * (a - b)[:, :2]]


@pytest.mark.parametrize("photo_occ, ssim_occ, passes", [(True, True, 1), (True, False, 1), (False, True, 1), (False, False, 0)])
def test_trainer_runs_one_exchanged_pass_for_both_masks(monkeypatch, photo_occ, ssim_occ, passes):
    """One step of the autograd loop on the CPU with the two terms and the forward-backward check replaced by recorders: the exchanged
    gradient-free pass runs once when photo_occ and ssim_occ are both set (and once when either is), before the differentiated pass,
    and both terms receive the mask made from its flow."""
    from eemflow_amd import harness, metrics
    checks, terms = [], []

    def fake_fb(fw, bw):
        checks.append((fw, bw))
        return torch.full_like(fw[:, :1], float(len(checks))), None
    monkeypatch.setattr(metrics, "fb_check", fake_fb)
    for name in ("photo_loss", "ssim_loss"):
        monkeypatch.setattr(harness, name, lambda preds, a, b, gamma=None, mask=None, _n=name, **kw:
                            terms.append((_n, mask, kw["use_occ"])) or preds[-1].sum() * 0.0 + 1.0)
    monkeypatch.setattr(harness, "_device_of", lambda model: torch.device("cpu"))
    e1, e2 = torch.rand(1, 5, 8, 8), torch.rand(1, 5, 8, 8)
    model = Twice()
    tr = TrainRaftEvents([{"event_volume_old": e1, "event_volume_new": e2}], (8, 8), engine="autograd", supervised=False, mixed_precision=False,
                         photo_weight=0.5, photo_kind="L1", photo_occ=photo_occ, ssim_weight=0.25, ssim_occ=ssim_occ, logger=Logger(verbose=False))
    tr._train_iters_autograd(model, 0, 1)
    exchanged = [c for c in model.calls if c[0] is not e1 and torch.equal(c[0], e2) and torch.equal(c[1], e1)]
    assert len(exchanged) == passes and len(model.calls) == 1 + passes
    if passes:
        assert model.calls[0][2] is False and torch.equal(model.calls[0][0], e2)        # first, and without a gradient
        assert model.calls[1][2] is True
    assert [t[0] for t in terms] == ["photo_loss", "ssim_loss"] and [t[2] for t in terms] == [photo_occ, ssim_occ]
    assert len(checks) == int(photo_occ) + int(ssim_occ)
    back = 0.5 * (e2 - e1)[:, :2]
    for (name, mask, occ) in terms:
        assert (mask is not None) == occ
    for fw, bw in checks:
        assert torch.equal(bw, back) and not bw.requires_grad
    assert tr.iteration == 1


def test_zero_ssim_weight_computes_nothing(monkeypatch):
    from eemflow_amd import harness
    monkeypatch.setattr(harness, "ssim_loss", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the term was computed")))
    monkeypatch.setattr(harness, "_device_of", lambda model: torch.device("cpu"))
    monkeypatch.setattr(harness, "photo_loss", lambda preds, a, b, gamma=None, mask=None, **kw: preds[-1].sum() * 0.0 + 1.0)
    e1, e2 = torch.rand(1, 5, 8, 8), torch.rand(1, 5, 8, 8)
    model = Twice()
    tr = TrainRaftEvents([{"event_volume_old": e1, "event_volume_new": e2}], (8, 8), engine="autograd", supervised=False, mixed_precision=False,
                         photo_weight=0.5, photo_kind="L1", ssim_weight=0.0, ssim_occ=True, ssim_all=True, ssim_c1=1e-4,
                         logger=Logger(verbose=False))
    tr._train_iters_autograd(model, 0, 1)
    assert len(model.calls) == 1                                   # no exchanged pass for a term that is off


def test_cli_flags_reach_the_trainer():
    from eemflow_amd import cli
    args = cli.build_parser().parse_args(["train"])
    assert cli.ssim_kw(args) == dict(ssim_weight=0.0, ssim_occ=False, ssim_all=False, ssim_c1=INF, ssim_c2=9e-6)
    assert cli.photo_kw(args) == dict(photo_weight=0.0, photo_kind="census", photo_occ=False, photo_all=False, photo_q=0.4,
                                      photo_charbonnier=False, photo_max_distance=3)
    for model in ("EEMFlow", "eraft", "EEMFlow+"):
        args = cli.build_parser().parse_args(["train", "--ssim_weight", "0.5", "--ssim_occ", "--ssim_all", "--ssim_c1", "1e-4", "--ssim_c2", "inf",
                                              "-model", model])
        kw = cli.ssim_kw(args)
        assert kw == dict(ssim_weight=0.5, ssim_occ=True, ssim_all=True, ssim_c1=1e-4, ssim_c2=INF) and math.isinf(kw["ssim_c2"])
        tr = TrainRaftEvents([], (64, 64), engine="autograd", logger=Logger(verbose=False), **kw, **cli.photo_kw(args))
        assert tr.ssim_weight == 0.5 and tr.ssim_kw == dict(c1=1e-4, c2=INF) and tr.ssim_all and tr.ssim_occ and tr.photo_weight == 0.0
    for flag in (["--ssim_weight", "0.1"], ["--ssim_occ"], ["--ssim_all"], ["--ssim_c1", "1e-4"], ["--ssim_c2", "1e-5"]):
        with pytest.raises(SystemExit):                            # training flags
            cli.build_parser().parse_args(["test"] + flag)
    import inspect
    src = inspect.getsource(cli.train)
    assert "**ssim_kw(args)" in src and "ssim == 0.0" in src and "mesh=contrast == 0.0 and photo == 0.0 and ssim == 0.0" in src
    assert 'ssim == 0.0 and smooth == 0.0 else "autograd"' in src  # every model: the autograd engine with the term
