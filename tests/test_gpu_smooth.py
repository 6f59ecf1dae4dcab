"""The edge-aware smoothness loss and its gradient on the GPU (csrc/smooth.hip, eemflow_amd.smooth, train.smoothness_loss and the
trainer's smoothness term) against the fp64 restatement of tests/smooth_reference.py on the same fp32 inputs.  Needs a real MI355X:
`pytest -m gpu`.

Bounds, each derived and none tuned:
  loss      relative error <= (terms + 16) * 2^-52: the worst case of summing `terms` non-negative fp64 numbers in any order (one
            rounding of 2^-53 per add, doubled) plus a few ulp of exp and pow per term, which a mean of non-negative terms passes on
            unamplified;
  golden    the reference's own fp32 losses: 4 * ref_gap relative, ref_gap (about 1.2e-7) the reference's distance from the fp64
            restatement - its fp32 summation-order noise at these sizes;
  gradient  every cell within 2^-23 * A, A the abs-sum of the cell's contributions: the one rounding of the fp64 sum to fp32 is
            2^-24 |g| <= 2^-24 A, doubled; the fp64 arithmetic in front of it is ten orders below.
The kernel's tile is 16 rows x 64 columns; (33, 129) is one row and one column more than two tiles each way."""
import ctypes

import pytest
import torch

from eemflow_amd import _lib, smooth
from eemflow_amd import train as hip_train
from eemflow_amd.harness import Logger, TrainRaftEvents
from eemflow_amd.weights import synthetic_gt, synthetic_voxel_pair

from smooth_reference import SETTINGS, gradient, smoothness, term_count

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_H, TILE_W = 16, 64


def make_inputs(seed, b, c, h, w):
    """A flow with a patch of constant flow (differences of exactly 0) and an event-volume-like edge image, float32 on the host."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    pred = torch.cat([3.0 * torch.sin(0.37 * x + 0.11 * y), 2.0 * torch.cos(0.23 * y - 0.05 * x)], 1).expand(b, 2, h, w).clone()
    pred = pred + 0.3 * torch.randn(b, 2, h, w, generator=g, dtype=torch.float64)
    pred[:, 0, :(h + 1) // 2, :(w + 1) // 2] = 0.75
    pred[:, 1, :(h + 1) // 2, :(w + 1) // 2] = -1.5
    img = torch.round(torch.randn(b, c, h, w, generator=g) * 3.0) / 4.0 * (torch.rand(b, c, h, w, generator=g) < 0.35)
    return pred.float(), img.float()


def run_gpu(preds, imgs, order, constant, wt, et, coefs=None):
    """(losses, gradients) of smoothness_many through autograd, on the host; coefs: the upstream gradient per job."""
    leaves = [p.to(DEV).requires_grad_(True) for p in preds]
    if imgs is not None and not torch.is_tensor(imgs):
        imgs = [im.to(DEV) if im is not None else None for im in imgs]
    elif imgs is not None:
        imgs = imgs.to(DEV)
    losses = smooth.smoothness_many(leaves, imgs, order=order, constant=constant, weight_type=wt, error_type=et)
    assert losses.dtype == torch.float64 and tuple(losses.shape) == (len(preds),)
    up = torch.ones(len(preds), dtype=torch.float64) if coefs is None else torch.tensor(coefs, dtype=torch.float64)
    (losses * up.to(DEV)).sum().backward()
    return losses.detach().cpu(), [p.grad.cpu() for p in leaves]


def check(tag, pred, img, order, constant, wt, et, loss, grad, coef=1.0):
    p64, i64 = pred.double(), img.double() if img is not None else None
    ref = float(smoothness(p64, i64, order, constant, wt, et))
    terms = term_count(pred.shape, order)
    rel = abs(float(loss) - ref) / abs(ref)
    g, a = gradient(p64, i64, order, constant, wt, et, coef=coef)
    assert grad.dtype == torch.float32 and grad.shape == pred.shape
    ratio = float(((grad.double() - g).abs() / (2.0 ** -23 * a).clamp(min=1e-300)).max())
    print(tag, (order, wt, et, constant), "loss rel %.2e of bound %.2e, gradient worst |d| / bound %.3f" % (rel, (terms + 16) * 2.0 ** -52, ratio))
    assert rel <= (terms + 16) * 2.0 ** -52, (tag, rel)
    assert bool(((grad.double() - g).abs() <= 2.0 ** -23 * a).all()), (tag, ratio)
    assert bool(torch.isfinite(grad).all())


SHAPES = {"5x7": (2, 5, 5, 7), "37x50": (3, 15, 37, 50), "tile+1": (2, 3, 2 * TILE_H + 1, 2 * TILE_W + 1)}


@pytest.fixture(scope="module")
def inputs():
    out = {name: make_inputs(7 + i, *s) for i, (name, s) in enumerate(SHAPES.items())}
    out["one1"] = make_inputs(3, 1, 1, 2, 2)                       # one term per line, order 1
    out["one2"] = make_inputs(4, 1, 1, 3, 3)                       # one term per line, order 2
    out["one1"][0][0, :, 0, 0] += 0.5                              # (not the constant patch alone)
    out["one2"][0][0, :, 0, 0] += 0.5
    return out


@pytest.mark.parametrize("constant", [1.0, 0.7])
@pytest.mark.parametrize("order,wt,et", SETTINGS)
def test_loss_and_gradient_match_the_fp64_restatement(inputs, order, wt, et, constant):
    for name in ("one%d" % order, "5x7", "37x50", "tile+1"):
        pred, img = inputs[name]
        for im in (img, None):
            losses, grads = run_gpu([pred], im, order, constant, wt, et)
            check(name + ("" if im is not None else " no img"), pred, im, order, constant, wt, et, losses[0], grads[0])


def test_losses_match_the_reference_own_values(golden):
    g = golden("smooth.npz")
    gap = float(g["ref_gap"])
    worst = 0.0
    for k in range(int(g["ncases"])):
        pred, img = torch.from_numpy(g[f"pred_{k}"]), torch.from_numpy(g[f"img_{k}"])
        for ci, constant in enumerate(g["constants"].tolist()):
            for si, (order, wt, et) in enumerate(SETTINGS):
                if pred.shape[2] <= order:
                    continue
                mine = float(smooth.smoothness_loss(pred.to(DEV), img.to(DEV), order=order, constant=constant, weight_type=wt, error_type=et))
                ref = float(g[f"loss_{k}"][ci, si])
                worst = max(worst, abs(mine - ref) / abs(ref))
        delta = float(smooth.smoothness_loss(pred.to(DEV)))            # flow_smooth_delta: order 1, L1, no img
        worst = max(worst, abs(delta - float(g[f"delta_{k}"])) / abs(float(g[f"delta_{k}"])))
    print("against the reference's fp32 values: worst relative difference %.3e, bound %.3e" % (worst, 4 * gap))
    assert worst <= 4 * gap


@pytest.mark.parametrize("k", [1, 3, 16, 20])
def test_many_jobs_share_one_img_bitwise(inputs, k):
    """k predictions against ONE img tensor (20: two library calls), each with its own upstream gradient: every job within the
    bounds, and bitwise what a one-job call gives."""
    base, img = inputs["tile+1"]
    order, constant, wt, et = 2, 0.7, "exp", "abs_robust"
    preds = [base + 0.01 * i * torch.flip(base, dims=[3]) for i in range(k)]
    coefs = [(-1.0) ** i * (0.25 + 0.5 * i) for i in range(k)]
    losses, grads = run_gpu(preds, img, order, constant, wt, et, coefs)
    for i in (0, k // 2, k - 1):
        check(f"job {i} of {k}", preds[i], img, order, constant, wt, et, losses[i], grads[i], coef=coefs[i])
    for i in range(k):
        one_l, one_g = run_gpu([preds[i]], img, order, constant, wt, et, [coefs[i]])
        assert torch.equal(one_l[0], losses[i]) and torch.equal(one_g[0], grads[i]), i


def test_mixed_imgs_in_one_call(inputs):
    """A list of imgs: shared, another tensor, none - the weights follow the job, and the results are the one-job results."""
    base, img = inputs["37x50"]
    other = torch.flip(img, dims=[2])
    preds = [base, base * 0.5, base + 0.1, base * -1.0, base * 2.0]
    imgs = [img, img, None, other, img]
    losses, grads = run_gpu(preds, imgs, 1, 1.0, "gauss", "L1")
    for i, (p, im) in enumerate(zip(preds, imgs)):
        check(f"mixed {i}", p, im, 1, 1.0, "gauss", "L1", losses[i], grads[i])
        one_l, one_g = run_gpu([p], im, 1, 1.0, "gauss", "L1")
        assert torch.equal(one_l[0], losses[i]) and torch.equal(one_g[0], grads[i])


def test_two_runs_give_the_same_bits(inputs):
    pred, img = inputs["tile+1"]
    for order, wt, et in ((1, "gauss", "L1"), (2, "exp", "abs_robust")):
        a = run_gpu([pred, pred * 0.5, pred + 1.0], img, order, 0.7, wt, et, [1.0, -2.0, 0.5])
        b = run_gpu([pred, pred * 0.5, pred + 1.0], img, order, 0.7, wt, et, [1.0, -2.0, 0.5])
        assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_full_frame_720p():
    pred, img = make_inputs(21, 1, 5, 720, 1280)
    losses, grads = run_gpu([pred], img, 2, 0.7, "gauss", "abs_robust", [1.5])
    check("720x1280", pred, img, 2, 0.7, "gauss", "abs_robust", losses[0], grads[0], coef=1.5)


def test_non_contiguous_inputs_are_made_contiguous(inputs):
    pred, img = inputs["37x50"]
    wide_p = torch.zeros(3, 2, 37, 60)
    wide_p[..., 5:55] = pred
    wide_i = torch.zeros(3, 15, 37, 60)
    wide_i[..., 5:55] = img
    leaf = wide_p.to(DEV).requires_grad_(True)
    view_p, view_i = leaf[..., 5:55], wide_i.to(DEV)[..., 5:55]
    assert not view_p.is_contiguous() and not view_i.is_contiguous()
    loss = smooth.smoothness_loss(view_p, view_i, order=1, constant=1.0, weight_type="exp", error_type="L1")
    loss.backward()
    ref_l, ref_g = run_gpu([pred], img, 1, 1.0, "exp", "L1")
    assert torch.equal(loss.detach().cpu(), ref_l[0]) and torch.equal(leaf.grad.cpu()[..., 5:55], ref_g[0])
    assert float(leaf.grad[..., :5].abs().max()) == 0.0


def test_training_term_with_gamma(inputs):
    """train.smoothness_loss: the last prediction alone, or sum_i gamma^(n-1-i) L_i over all - value and gradients."""
    base, img = inputs["5x7"]
    preds = [base * (1.0 + 0.1 * i) for i in range(5)]
    kw = dict(order=2, constant=0.7, weight_type="gauss", error_type="abs_robust")
    refs = [float(smoothness(p.double(), img.double(), 2, 0.7, "gauss", "abs_robust")) for p in preds]
    terms = term_count(base.shape, 2)
    leaves = [p.to(DEV).requires_grad_(True) for p in preds]
    last = hip_train.smoothness_loss(leaves, img.to(DEV), **kw)
    assert last.dtype == torch.float64 and abs(float(last.detach()) - refs[-1]) <= (terms + 16) * 2.0 ** -52 * refs[-1]
    gamma = 0.8
    total = hip_train.smoothness_loss(leaves, img.to(DEV), gamma=gamma, **kw)
    want = sum(gamma ** (4 - i) * r for i, r in enumerate(refs))
    assert abs(float(total.detach()) - want) <= (terms + 16 + 8) * 2.0 ** -52 * want        # (five products and adds more)
    total.backward()
    for i, (p, leaf) in enumerate(zip(preds, leaves)):
        g, a = gradient(p.double(), img.double(), 2, 0.7, "gauss", "abs_robust", coef=gamma ** (4 - i))
        assert bool(((leaf.grad.cpu().double() - g).abs() <= 2.0 ** -23 * a).all()), i


def test_non_finite_input_propagates_and_short_axes_raise(inputs):
    pred, img = inputs["5x7"]
    bad = pred.clone()
    bad[1, 0, 2, 3] = float("inf")
    losses, grads = run_gpu([bad, pred], img, 1, 1.0, "gauss", "L1")
    assert not bool(torch.isfinite(losses[0])) and bool(torch.isfinite(losses[1]))
    check("beside an inf", pred, img, 1, 1.0, "gauss", "L1", losses[1], grads[1])
    with pytest.raises(ValueError, match="H > 2"):
        smooth.smoothness_loss(torch.zeros(1, 2, 2, 8, device=DEV), order=2)
    with pytest.raises(ValueError, match="W > 1"):
        smooth.smoothness_loss(torch.zeros(1, 2, 8, 1, device=DEV), order=1)
    # the library's own check, past the Python one
    p = torch.zeros(1, 2, 2, 8, device=DEV)
    out = torch.zeros(1, device=DEV, dtype=torch.float64)
    rc = _lib.lib().eemflow_smoothness_many(1, (ctypes.c_void_p * 1)(p.data_ptr()), None, 1, 1, 2, 8, 2, 0, 0, 1.0, None, out.data_ptr(), None,
                                            out.data_ptr(), _lib.current_stream_ptr(p.device))
    assert rc != 0 and "H > 2" in _lib.lib().eemflow_last_error().decode()


# ------------------------------------------------------------------------------------------------ the trainer
def eemflow_net(seed):
    """EEMFlow under its own initialisation (the seeded fixture weights predict a spatially constant flow at this size, which no
    smoothness term can tell from any other)."""
    from eemflow_amd import EEMFlow
    torch.manual_seed(seed)
    return EEMFlow("", groups=5, n_first_channels=5).to(DEV).train()


def supervised_batch(seed, b, h, w):
    e1, e2 = (torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(seed, b, h, w))
    gt, valid = (torch.from_numpy(a).to(DEV) for a in synthetic_gt(seed + 1, b, h, w))
    return {"event_volume_old": e1, "event_volume_new": e2, "flow": gt, "valid": valid}


class Lines(Logger):
    def __init__(self):
        super().__init__(verbose=False)
        self.lines = []

    def write_line(self, line, *a, **k):
        self.lines.append(line)


def spy(monkeypatch, name, seen):
    from eemflow_amd import harness
    real = getattr(harness, name)

    def wrapped(*a, **k):
        out = real(*a, **k)
        seen.append((a, k, out))
        return out
    monkeypatch.setattr(harness, name, wrapped)


def test_trainer_adds_the_smoothness_term(monkeypatch):
    """Two autograd steps of EEMFlow at 64 x 64, batch 2, smooth_weight=0.1 beside the supervised loss: the term is the restatement's
    value on the very prediction and the old event volume (the loss bound), the logged loss is sequence loss + 0.1 * term (added in
    fp32 and printed with six decimals), parameters change.  (At this size EEMFlow's prediction is constant over each plane, so this
    pins the wiring - which prediction, which img, which settings, which weight; the E-RAFT test below has a flow that varies.)"""
    h = w = 64
    batches = [supervised_batch(130, 2, h, w), supervised_batch(140, 2, h, w)]
    net = eemflow_net(79)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    seq, smo = [], []
    spy(monkeypatch, "sequence_loss", seq)
    spy(monkeypatch, "smoothness_loss", smo)
    log = Lines()
    tr = TrainRaftEvents(batches, (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd", mixed_precision=False, smooth_weight=0.1,
                         smooth_order=2, smooth_weight_type="exp", smooth_error="abs_robust", smooth_constant=0.7)
    tr.train_iters(net, val_iters=2)
    assert len(log.lines) == 2 and len(seq) == 2 and len(smo) == 2 and tr.iteration == 2
    for step in range(2):
        (preds, img), kw, term = smo[step]
        assert img is not None and tuple(img.shape) == (2, 5, h, w) and tuple(preds[-1].shape) == (2, 2, h, w)
        assert torch.equal(img, batches[step]["event_volume_old"]) and kw["gamma"] is None
        ref = float(smoothness(preds[-1].detach().cpu().double(), img.cpu().double(), 2, 0.7, "exp", "abs_robust"))
        terms = term_count(preds[-1].shape, 2)
        print("trainer step", step, "term", float(term.detach()), "restatement", ref)
        assert term.dtype == torch.float64                         # (the trainer casts it to fp32 when it adds)
        assert abs(float(term.detach()) - ref) <= (terms + 16) * 2.0 ** -52 * ref
        total = float(seq[step][2][0].detach()) + 0.1 * ref
        logged = float(log.lines[step].split("loss")[1].split()[0])
        assert abs(logged - total) <= 1e-5 * (1.0 + abs(total))
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert any(not torch.equal(p.detach(), before[k]) for k, p in net.named_parameters())


def test_term_through_eraft_reaches_the_parameters():
    """train.smoothness_loss over ALL predictions of E-RAFT (128 x 160, two iterations, batch 2 - the size its training tests use)
    under a gamma, against the old event volume: the value within the loss bound of every prediction, and a gradient in the
    parameters.  (EEMFlow's prediction at 64 x 64 is constant over each plane: its smoothness gradient is exactly zero.)"""
    from eemflow_amd.eraft import ERAFT
    h, w = 128, 160
    torch.manual_seed(5)
    net = ERAFT("", n_first_channels=5).to(DEV).train()
    net.change_imagesize((h, w))
    e1, e2 = (torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(150, 2, h, w))
    preds = net(e1, e2, iters=2)[1]
    assert len(preds) == 2 and tuple(preds[-1].shape) == (2, 2, h, w) and preds[-1].requires_grad
    assert float(preds[-1].detach().std(dim=(2, 3)).min()) > 0.0       # (a flow that varies in space)
    gamma = 0.8
    term = hip_train.smoothness_loss(preds, e1, gamma=gamma, order=1, weight_type="exp", constant=0.7)
    refs = [float(smoothness(p.detach().cpu().double(), e1.cpu().double(), 1, 0.7, "exp")) for p in preds]
    want = gamma * refs[0] + refs[1]
    print("term through E-RAFT", float(term.detach()), "restatement", want)
    assert abs(float(term.detach()) - want) <= (term_count(preds[-1].shape, 1) + 16 + 4) * 2.0 ** -52 * want      # (two products, one add)
    term.float().backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and max(float(g.abs().max()) for g in grads) > 0


def test_zero_smooth_weight_changes_nothing(monkeypatch):
    h = w = 64
    seq, smo = [], []
    spy(monkeypatch, "sequence_loss", seq)
    spy(monkeypatch, "smoothness_loss", smo)
    lines = []
    for kw in ({}, dict(smooth_weight=0.0, smooth_order=2, smooth_all=True)):
        log = Lines()
        tr = TrainRaftEvents([supervised_batch(130, 2, h, w)], (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd",
                             mixed_precision=False, **kw)
        tr.train_iters(eemflow_net(79), val_iters=1)
        lines.append(log.lines)
    assert not smo and len(seq) == 2
    assert torch.equal(seq[0][2][0], seq[1][2][0]) and lines[0] == lines[1] and len(lines[0]) == 1
