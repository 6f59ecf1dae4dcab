"""The photometric / census warp losses on the host: the reference's own results (tests/golden/photo.npz, made by executing its
sources) against the restatement of tests/photo_reference.py, the restatement's analytic gradient against fp64 autograd, the
conditions the test inputs must meet, and the argument checks of eemflow_amd.photo, the trainer and the CLI.  No GPU needed."""
import numpy as np
import pytest
import torch

from eemflow_amd import _lib, photo
from eemflow_amd.harness import Logger, TrainRaftEvents

import photo_reference as R

SHAPES = [(1, 3, 7, 7), (2, 3, 9, 11), (3, 3, 37, 50)]


def case_kw(case):
    kind, occ, ch, av, r = case
    if kind in R.POINTWISE:
        return dict(kind=kind, use_occ=occ)
    return dict(kind=kind, use_occ=occ, q=R.Q, charbonnier=ch, average=av, max_distance=r)


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("photo.npz")
    assert g["cases"].tolist() == ["%s/%d/%d/%d/%d" % c for c in R.CASES]
    assert len(R.CASES) == 6 + 16 and float(g["q"]) == R.Q
    return g


def tensors(g, i):
    return tuple(torch.from_numpy(g[f"{n}_{i}"]) for n in ("flow", "img1", "img2", "mask"))


def test_golden_matches_the_fp32_restatement(cases):
    """The reference's fp32 losses against the restatement run in fp32 (its own fp32 warp, then every branch in fp32): 4 * ref_gap
    relative, ref_gap the largest relative distance between a reference value and the fp64 restatement - fp32 rounding of the
    per-element terms and the summation order at these sizes."""
    gap = float(cases["ref_gap"])
    assert 0.0 < gap < 2.0 ** -20
    assert int(cases["ncases"]) == 3
    worst = 0.0
    for i in range(3):
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


def test_restated_warp_is_grid_sample(cases):
    """The operation-by-operation fp32 warp against torch's own grid_sample on the reference's grid.  grid_sample may unnormalise the
    coordinate in another order ((x + 1) * W - 1) / 2), so ix and iy may differ by a few fp32 ulp at their magnitude (< max(H, W) + 2),
    and a coordinate error e moves the blend by at most 2 max|img| e per axis: 4 ulp on each axis."""
    import torch.nn.functional as F
    for i in range(3):
        flow, _, img2, _ = tensors(cases, i)
        b, c, h, w = img2.shape
        xx = torch.arange(w).view(1, 1, 1, w).expand(b, 1, h, w).float()
        yy = torch.arange(h).view(1, 1, h, 1).expand(b, 1, h, w).float()
        v = torch.cat((xx, yy), 1) + flow
        grid = torch.stack((2.0 * v[:, 0] / max(w - 1, 1) - 1.0, 2.0 * v[:, 1] / max(h - 1, 1) - 1.0), 3)
        want = F.grid_sample(img2, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        got = R.warp_taps(img2, flow)["yw"]
        assert float((got - want).abs().max()) <= 2 * (4 * 2.0 ** -23 * (max(h, w) + 2)) * 2 * float(img2.abs().max())


def test_inputs_meet_their_conditions(cases):
    """Samples leave the frame on each of the four sides, a region is masked out, d == 0 occurs, about 65 % of the image cells are
    zero and all are quarter-integers; the all-zero-mask variant is all zero."""
    for i in range(3):
        flow, img1, img2, mask = tensors(cases, i)
        b, c, h, w = img1.shape
        x = torch.arange(w).view(1, 1, w) + flow[:, 0]
        y = torch.arange(h).view(1, h, 1) + flow[:, 1]
        assert bool((x < 0).any()) and bool((x > w - 1).any()) and bool((y < 0).any()) and bool((y > h - 1).any())
        assert bool((mask == 0).any()) and bool((mask == 1).any()) and bool(((mask == 0) | (mask == 1)).all())
        assert float(mask[:, :, : (h + 1) // 2, : (w + 1) // 3].abs().max()) == 0.0
        assert bool((mask[:, :, h // 2, w // 2] == 1).all())
        for im in (img1, img2):
            assert bool((im * 4 == torch.round(im * 4)).all())
            if im.numel() > 1000:
                assert 0.55 < float((im == 0).float().mean()) < 0.75
        assert bool((img1 - R.warp_taps(img2, flow)["yw"] == 0).any())
    zero = R.inputs(5, (2, 3, 9, 11), zero_mask=True)[3]
    assert float(np.abs(zero).max()) == 0.0


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-occ%d-ch%d-av%d-r%d" % c)
def test_analytic_gradient_matches_fp64_autograd(cases, case):
    """gradient() against autograd of the fp64 restatement with the tap positions, weights and warped values held at their fp32
    results: every cell within 1e-14 of A, the cell's abs-sum (relative to the cell's own scale: stricter than relative to the
    largest gradient), and A bounds |g|."""
    kw = case_kw(case)
    for i in range(3):
        flow, img1, img2, mask = tensors(cases, i)
        taps = R.warp_taps(img2, flow)
        for m in ((mask, None) if kw["use_occ"] else (mask,)):
            f = flow.double().requires_grad_(True)
            R.loss_autograd(f, taps, img1, m, **kw).backward()
            g, a = R.gradient(flow, img1, img2, m, coef=-1.5, **kw)
            assert g.shape == a.shape == f.grad.shape
            assert bool(((g - (-1.5) * f.grad).abs() <= 1e-14 * a).all()), float(((g - (-1.5) * f.grad).abs() / a.clamp(min=1e-300)).max())
            assert bool((a >= g.abs() * (1 - 1e-12)).all())
            assert float(g.abs().max()) > 0.0


def test_all_zero_mask_gives_zero():
    flow, img1, img2, mask = (torch.from_numpy(a) for a in R.inputs(5, (2, 3, 9, 11), zero_mask=True))
    for case in R.CASES:
        kw = case_kw(case)
        if not kw["use_occ"]:
            continue
        assert float(R.loss(flow, img1, img2, mask, **kw)) == 0.0
        assert float(R.gradient(flow, img1, img2, mask, **kw)[0].abs().max()) == 0.0


class Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the shape and dtype checks run without one."""
    is_cuda = True


def cuda(t):
    return t.as_subclass(Cuda)


def test_argument_validation():
    flow, img = torch.zeros(2, 2, 8, 8), torch.zeros(2, 5, 8, 8)
    mask = torch.zeros(2, 1, 8, 8)
    for call in (lambda: photo.photo_many([flow], img, img), lambda: photo.photo_loss(flow, img, img),
                 lambda: photo.photo_loss(cuda(flow), img, img), lambda: photo.photo_loss(cuda(flow), cuda(img), cuda(img), mask, kind="L1")):
        with pytest.raises(_lib.EEMFlowHipError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="abs_robust.*census"):      # SSIM is out of scope; the message names the kinds that exist
        photo.photo_loss(flow, img, img, kind="SSIM")
    with pytest.raises(ValueError, match="max_distance"):
        photo.photo_loss(flow, img, img, max_distance=4)
    with pytest.raises(ValueError, match="max_distance"):
        photo.photo_loss(flow, img, img, max_distance=0)
    with pytest.raises(ValueError, match=r"\(B,2,H,W\) float32"):
        photo.photo_many([cuda(torch.zeros(2, 3, 8, 8))], cuda(img), cuda(img))
    with pytest.raises(ValueError, match=r"\(B,2,H,W\) float32"):
        photo.photo_many([cuda(flow.double())], cuda(img), cuda(img))
    with pytest.raises(ValueError, match=r"\(B,C,H,W\) float32"):
        photo.photo_loss(cuda(flow), cuda(img.double()), cuda(img))
    with pytest.raises(ValueError, match=r"\(B,1,H,W\) float32"):
        photo.photo_loss(cuda(flow), cuda(img), cuda(img), cuda(torch.zeros(2, 2, 8, 8)), use_occ=True)
    for bad in (torch.zeros(1, 5, 8, 8), torch.zeros(2, 5, 7, 8), torch.zeros(2, 5, 8, 9)):
        with pytest.raises(ValueError, match="B, H and W"):
            photo.photo_loss(cuda(flow), cuda(img), cuda(bad))
    with pytest.raises(ValueError, match="B, H and W"):
        photo.photo_loss(cuda(flow), cuda(img), cuda(img), cuda(torch.zeros(2, 1, 8, 9)))
    with pytest.raises(ValueError, match="channel count"):
        photo.photo_loss(cuda(flow), cuda(img), cuda(torch.zeros(2, 3, 8, 8)))
    with pytest.raises(ValueError, match="share one"):
        photo.photo_many([cuda(flow), cuda(torch.zeros(2, 2, 8, 9))], cuda(img), cuda(img))
    with pytest.raises(ValueError, match="per flow"):
        photo.photo_many([cuda(flow), cuda(flow)], [cuda(img)], cuda(img))
    with pytest.raises(ValueError, match="required"):
        photo.photo_many([cuda(flow)], None, cuda(img))
    with pytest.raises(ValueError, match="at least one"):
        photo.photo_many([], img, img)
    with pytest.raises(TypeError):
        photo.photo_many([np.zeros((2, 2, 8, 8), np.float32)], img, img)
    with pytest.raises(ValueError, match="H > 6"):
        photo.photo_loss(cuda(torch.zeros(1, 2, 6, 8)), cuda(torch.zeros(1, 3, 6, 8)), cuda(torch.zeros(1, 3, 6, 8)))
    with pytest.raises(ValueError, match="W > 2"):
        photo.photo_loss(cuda(torch.zeros(1, 2, 6, 2)), cuda(torch.zeros(1, 3, 6, 2)), cuda(torch.zeros(1, 3, 6, 2)), max_distance=1)
    with pytest.raises(ValueError, match="one weight per channel"):
        photo.photo_loss(cuda(flow), cuda(img), cuda(img), gray=(0.5, 0.5))
    assert photo.default_gray(3) == R.GRAY_RGB == (0.2989, 0.5870, 0.1140) and photo.default_gray(5) == (0.2,) * 5 == R.default_gray(5)
    from eemflow_amd import photo_loss, photo_many
    assert photo_many is photo.photo_many and photo_loss is photo.photo_loss
    from eemflow_amd.train import photo_loss as train_term
    with pytest.raises(_lib.EEMFlowHipError, match="no CPU path"):
        train_term([flow, flow], img, img, gamma=0.8)
    with pytest.raises(ValueError, match="at least one"):
        train_term([], img, img)


def test_library_refuses_bad_calls_before_any_launch():
    """The C entry point's own checks (they return before a kernel is launched, so no GPU is needed): k, the shape, the enums."""
    import ctypes
    lib = _lib.lib()
    one = (ctypes.c_void_p * 1)(16)
    out = ctypes.c_void_p(16)

    def call(k=1, b=1, c=3, h=8, w=8, kind=3, r=3, loss=out, scratch=out, img1=one):
        return lib.eemflow_photo_many(k, one, img1, one, None, b, c, h, w, kind, 0, 0, 1, r, 0.4, None, None, loss, None, scratch, None)
    for kw, word in ((dict(k=0), "jobs"), (dict(k=17), "jobs"), (dict(kind=4), "kind"), (dict(kind=-1), "kind"), (dict(r=0), "max_distance"),
                     (dict(r=4), "max_distance"), (dict(h=6), "H > 6"), (dict(w=2, r=1), "W > 2"), (dict(b=0), "shape"), (dict(c=0), "channel"),
                     (dict(loss=None), "neither"), (dict(scratch=None), "scratch"), (dict(img1=None), "NULL")):
        assert call(**kw) != 0
        assert word in lib.eemflow_last_error().decode(), (kw, lib.eemflow_last_error())
    assert lib.eemflow_photo_scratch_doubles(0, 1, 8, 8) == 0 and lib.eemflow_photo_scratch_doubles(17, 1, 8, 8) == 0
    assert lib.eemflow_photo_scratch_doubles(3, 2, 17, 65) == 16 + 3 * (2 * 2 * 2)             # 16 denominators, then 16 x 64 tiles per job
    assert lib.eemflow_photo_scratch_doubles(16, 8, 720, 1280) == 16 + 16 * 2048               # the grid is capped at 2048 blocks


def test_trainer_takes_the_photo_arguments():
    quiet = Logger(verbose=False)
    with pytest.raises(ValueError, match="autograd"):              # the fused engine with a weight
        TrainRaftEvents([], (64, 64), engine="fused", photo_weight=0.1, logger=quiet)
    with pytest.raises(ValueError, match="no loss"):
        TrainRaftEvents([], (64, 64), engine="autograd", supervised=False, logger=quiet)
    with pytest.raises(ValueError, match="SSIM"):
        TrainRaftEvents([], (64, 64), engine="autograd", photo_weight=0.1, photo_kind="SSIM", logger=quiet)
    with pytest.raises(ValueError, match="max_distance"):
        TrainRaftEvents([], (64, 64), engine="autograd", photo_weight=0.1, photo_max_distance=5, logger=quiet)
    tr = TrainRaftEvents([], (64, 64), logger=quiet)
    assert tr.photo_weight == 0.0 and tr.photo_occ is False and tr.photo_all is False and tr.engine == "fused"
    tr = TrainRaftEvents([], (64, 64), engine="autograd", supervised=False, photo_weight=0.5, logger=quiet)     # a loss of its own
    assert tr.photo_weight == 0.5 and tr.photo_kw == dict(kind="census", q=0.4, charbonnier=False, max_distance=3)
    tr = TrainRaftEvents([], (64, 64), engine="autograd", photo_weight=0.1, photo_kind="census", photo_occ=True, photo_all=True, photo_q=0.3,
                         photo_charbonnier=True, photo_max_distance=1, logger=quiet)
    assert tr.photo_occ and tr.photo_all and tr.photo_kw == dict(kind="census", q=0.3, charbonnier=True, max_distance=1)


def test_trainer_hands_both_volumes_and_the_mask(monkeypatch):
    from eemflow_amd import harness
    seen = []
    monkeypatch.setattr(harness, "photo_loss", lambda preds, a, b, gamma=None, mask=None, **kw: seen.append((len(preds), a, b, gamma, mask, kw))
                        or torch.zeros(()))
    e1, e2 = torch.zeros(2, 5, 64, 64), torch.ones(2, 5, 64, 64)
    full, mesh = [torch.zeros(2, 2, 64, 64)] * 3, [torch.zeros(2, 2, 16, 16)]
    tr = TrainRaftEvents([], (64, 64), engine="autograd", photo_weight=0.1, photo_kind="L1", gamma=0.85, logger=Logger(verbose=False))
    tr._photo_term(full, e1, e2, None)
    with pytest.raises(ValueError, match="frame's size"):
        tr._photo_term(mesh, e1, e2, None)
    tr.photo_all = True
    tr._photo_term(full, e1, e2, None)
    assert seen[0][0] == 3 and seen[0][1] is e1 and seen[0][2] is e2 and seen[0][3] is None and seen[0][4] is None
    assert seen[0][5] == dict(use_occ=False, kind="L1", q=0.4, charbonnier=False, max_distance=3)
    assert seen[1][3] == 0.85

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.bn = torch.nn.BatchNorm2d(2)
    net = Net().train()
    with pytest.raises(ValueError, match="BatchNorm"):             # the second pass would move the running statistics
        tr._photo_backward_flow(net, e1, e2)


def test_cli_flags_reach_the_trainer():
    from eemflow_amd import cli
    args = cli.build_parser().parse_args(["train"])
    assert cli.photo_kw(args) == dict(photo_weight=0.0, photo_kind="census", photo_occ=False, photo_all=False, photo_q=0.4,
                                      photo_charbonnier=False, photo_max_distance=3)
    args = cli.build_parser().parse_args(["train", "--photo_weight", "0.5", "--photo_kind", "census", "--photo_occ", "--photo_all", "--photo_q",
                                          "0.3", "--photo_charbonnier", "--photo_max_distance", "2", "-model", "eraft"])
    kw = cli.photo_kw(args)
    assert kw == dict(photo_weight=0.5, photo_kind="census", photo_occ=True, photo_all=True, photo_q=0.3, photo_charbonnier=True,
                      photo_max_distance=2)
    tr = TrainRaftEvents([], (64, 64), engine="autograd", logger=Logger(verbose=False), **kw)
    assert tr.photo_weight == 0.5 and tr.photo_kw["max_distance"] == 2 and tr.photo_all and tr.photo_occ
    for bad in (["--photo_kind", "SSIM"], ["--photo_max_distance", "4"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["train"] + bad)
    with pytest.raises(SystemExit):                                # a training flag
        cli.build_parser().parse_args(["test", "--photo_weight", "0.1"])
    import inspect
    src = inspect.getsource(cli.train)
    assert "**photo_kw(args)" in src and "photo == 0.0" in src and "mesh=contrast == 0.0 and photo == 0.0" in src
