"""The weighted SSIM warp loss and its gradient on the GPU (csrc/ssim.hip, eemflow_amd.ssim, train.ssim_loss and the trainer's SSIM
term) against the fp64 restatement of tests/ssim_reference.py on the same fp32 inputs.  Needs a real MI355X: `pytest -m gpu`.

Bounds, each derived and none tuned:
  warp      the kernel's fp32 warped values are warp_px.h's, which tests/test_gpu_photo.py holds equal to the restatement's bit for bit;
  loss      per cell, mu and P[.] carry some 16 roundings each: nine products with wpe, their sum, the division by 9 and the product
            with inv, of numbers up to M^2 = max(1, x^2, y^2) - 16 * 2^-53 * M^2 absolute.  s = P[z z'] - mu mu' cancels, so that
            absolute error stays and n / d divides it by d >= min(c1, c2), for n and for d: l = (1 - n / d) / 2 is off by at most
            E = 2 * 16 * 2^-53 * M^2 / min(c1, c2) (ssim_reference.cancellation; with both terms n / d is the product of two ratios of
            size at most 1, each off by its own share).  mean(l) is off by E, and sum(l aw) / (sum(aw) + 1e-6), whose numerator runs
            over C times the cells of its denominator, by C E; the sums of `terms` non-negative numbers add (terms + 16) * 2^-52
            relative, as for the photometric kinds.  Relative bound: (terms + 16) * 2^-52 + (C with use_occ, else 1) * E / L - about
            1e-8 at c2 = 9e-6, 1e-9 for the luminance term; an all-zero mask with use_occ gives exactly 0;
  golden    the reference's own fp32 losses: 4 * ref_gap relative, ref_gap (about 1.5e-7) the reference's distance from the fp64
            restatement;
  gradient  every cell within 2^-23 * A, A the product of the abs-sums of the cell's contributions: the one rounding of the fp64 value
            to fp32 is 2^-24 |g| <= 2^-24 A, doubled; the fp64 arithmetic in front of it is relative E, two orders below.
The kernel's tile is 16 rows x 64 columns; (33, 129) is one row and one column more than two tiles each way."""
import pytest
import torch

from eemflow_amd import ssim
from eemflow_amd import train as hip_train
from eemflow_amd.harness import Logger, TrainRaftEvents
from eemflow_amd.metrics import fb_check
from eemflow_amd.weights import synthetic_gt, synthetic_voxel_pair

import ssim_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_H, TILE_W = 16, 64
SHAPES = {"3x3": (1, 1, 3, 3), "7x7": (1, 3, 7, 7), "9x11": (2, 5, 9, 11), "37x50": (2, 15, 37, 50),
          "tile+1": (2, 3, 2 * TILE_H + 1, 2 * TILE_W + 1)}
INF = float("inf")


def case_kw(case):
    occ, c1, c2 = case
    return dict(use_occ=occ, c1=c1, c2=c2)


def loss_bound(flow, img1, img2, ref, kw):
    yw = R.warp_taps(img2, flow)["yw"]
    e = R.cancellation(img1, yw, kw["c1"], kw["c2"])
    return (R.term_count(img1.shape) + 16) * 2.0 ** -52 + (img1.shape[1] if kw["use_occ"] else 1) * e / ref


@pytest.fixture(scope="module")
def inputs():
    out = {name: tuple(torch.from_numpy(a) for a in R.inputs(11 + i, s)) for i, (name, s) in enumerate(SHAPES.items())}
    out["zero"] = tuple(torch.from_numpy(a) for a in R.inputs(5, SHAPES["9x11"], zero_mask=True))
    flow, img1, img2, mask = out["3x3"]                            # (inputs' border flows leave a 3 x 3 frame everywhere: also one that stays)
    out["3x3 inside"] = (flow * 0.125, img1, img2, torch.ones_like(mask))
    return out


def run_gpu(flows, img1, img2, mask, coefs=None, **kw):
    """(losses, gradients) of ssim_many through autograd, on the host; coefs: the upstream gradient per job."""
    leaves = [f.to(DEV).requires_grad_(True) for f in flows]
    losses = ssim.ssim_many(leaves, img1.to(DEV), img2.to(DEV), mask.to(DEV) if mask is not None else None, **kw)
    assert losses.dtype == torch.float64 and tuple(losses.shape) == (len(flows),)
    up = torch.ones(len(flows), dtype=torch.float64) if coefs is None else torch.tensor(coefs, dtype=torch.float64)
    (losses * up.to(DEV)).sum().backward()
    return losses.detach().cpu(), [f.grad.cpu() for f in leaves]


def check(tag, flow, img1, img2, mask, loss, grad, coef=1.0, **kw):
    ref = float(R.loss(flow, img1, img2, mask, **kw))
    g, a = R.gradient(flow, img1, img2, mask, coef=coef, **kw)
    assert grad.dtype == torch.float32 and grad.shape == flow.shape
    ratio = float(((grad.double() - g).abs() / (2.0 ** -23 * a).clamp(min=1e-300)).max())
    if ref == 0.0:
        print(tag, sorted(kw.items()), "loss %r for 0, gradient worst |d| / bound %.3f" % (float(loss), ratio))
        assert float(loss) == 0.0, (tag, float(loss))
    else:
        bound = loss_bound(flow, img1, img2, ref, kw)
        rel = abs(float(loss) - ref) / abs(ref)
        print(tag, sorted(kw.items()), "loss rel %.2e of bound %.2e, gradient worst |d| / bound %.3f" % (rel, bound, ratio))
        assert rel <= bound, (tag, rel, bound)
    assert bool(((grad.double() - g).abs() <= 2.0 ** -23 * a).all()), (tag, ratio)
    assert bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_loss_and_gradient_match_the_fp64_restatement(inputs, case):
    """Every shape, with its mask, without one and with an all-zero mask."""
    kw = case_kw(case)
    seen = 0.0
    for name in list(SHAPES) + ["3x3 inside"]:
        flow, img1, img2, mask = inputs[name]
        for tag, m in (("", mask), (" no mask", None), (" zero mask", torch.zeros_like(mask))):
            losses, grads = run_gpu([flow], img1, img2, m, **kw)
            check(name + tag, flow, img1, img2, m, losses[0], grads[0], **kw)
            seen = max(seen, float(grads[0].abs().max()))
    assert seen > 0.0
    flow, img1, img2, _ = inputs["3x3 inside"]
    assert float(run_gpu([flow], img1, img2, None, **kw)[1][0].abs().max()) > 0.0      # the one centre has a gradient


def test_more_tiles_than_blocks():
    """520 samples of 2 x 2 tiles: 2080 tiles on the grid's cap of 2048 blocks, so 32 blocks walk a second tile and add it to their
    loss slots; the structure branch with its mask.  The same bounds as everywhere."""
    flow, img1, img2, mask = (torch.from_numpy(a) for a in R.inputs(23, (520, 2, TILE_H + 1, TILE_W + 1)))
    kw = dict(use_occ=True, c1=INF, c2=9e-6)
    losses, grads = run_gpu([flow], img1, img2, mask, **kw)
    check("520 x 17x65", flow, img1, img2, mask, losses[0], grads[0], **kw)


def test_losses_match_the_reference_own_values(golden):
    g = golden("ssim.npz")
    gap = float(g["ref_gap"])
    assert 0.0 < gap <= 1e-6                                       # (above that the comparison would be vacuous)
    worst = 0.0
    for i in range(int(g["ncases"])):
        flow, img1, img2, mask = (torch.from_numpy(g[f"{n}_{i}"]).to(DEV) for n in ("flow", "img1", "img2", "mask"))
        for ci, case in enumerate(R.CASES):
            mine = float(ssim.ssim_loss(flow, img1, img2, mask, **case_kw(case)))
            ref = float(g[f"loss_{i}"][ci])
            worst = max(worst, abs(mine - ref) / abs(ref))
    print("against the reference's fp32 values: worst relative difference %.3e, bound %.3e" % (worst, 4 * gap))
    assert worst <= 4 * gap


@pytest.mark.parametrize("k", [1, 3, 16, 20])
def test_many_jobs_share_the_images_bitwise(inputs, k):
    """k flows against ONE pair of images and one mask (20: two library calls), each with its own upstream gradient: jobs within the
    bounds, bitwise what a one-job call gives, and bitwise the same in a second run."""
    base, img1, img2, mask = inputs["tile+1"]
    kw = dict(use_occ=True, c1=1e-4, c2=9e-6)
    flows = [base + 0.01 * i * torch.flip(base, dims=[3]) for i in range(k)]
    coefs = [(-1.0) ** i * (0.25 + 0.5 * i) for i in range(k)]
    losses, grads = run_gpu(flows, img1, img2, mask, coefs, **kw)
    again_l, again_g = run_gpu(flows, img1, img2, mask, coefs, **kw)
    assert torch.equal(losses, again_l) and all(torch.equal(a, b) for a, b in zip(grads, again_g))
    for i in sorted({0, k // 2, k - 1}):
        check(f"job {i} of {k}", flows[i], img1, img2, mask, losses[i], grads[i], coef=coefs[i], **kw)
    for i in range(k):
        one_l, one_g = run_gpu([flows[i]], img1, img2, mask, [coefs[i]], **kw)
        assert torch.equal(one_l[0], losses[i]) and torch.equal(one_g[0], grads[i]), i


def test_mixed_images_and_masks_in_one_call(inputs):
    """Lists of images and masks: shared img1, another img1, no mask, the all-zero mask - every job is its one-job result, and the
    all-zero mask with use_occ gives exactly 0 and an exactly zero gradient."""
    flow, img1, img2, mask = inputs["9x11"]
    zero = inputs["zero"][3]
    other = torch.flip(img1, dims=[2])
    d = DEV
    i1 = [img1.to(d)] * 2 + [other.to(d)] + [img1.to(d)] * 2
    i2 = [img2.to(d)] * 5
    ms = [mask.to(d), None, mask.to(d), zero.to(d), mask.to(d)]
    fl = [flow, flow * 0.5, flow + 0.1, flow, flow * -1.0]
    for kw in (dict(use_occ=True, c1=INF, c2=9e-6), dict(use_occ=False, c1=1e-4, c2=INF)):
        leaves = [f.to(d).requires_grad_(True) for f in fl]
        losses = ssim.ssim_many(leaves, i1, i2, ms, **kw)
        losses.sum().backward()
        for j in range(5):
            m = ms[j].cpu() if ms[j] is not None else None
            check(f"mixed {j}", fl[j], i1[j].cpu(), img2, m, losses[j].detach().cpu(), leaves[j].grad.cpu(), **kw)
            one_l, one_g = run_gpu([fl[j]], i1[j].cpu(), img2, m, **kw)
            assert torch.equal(one_l[0], losses[j].detach().cpu()) and torch.equal(one_g[0], leaves[j].grad.cpu()), j
        if kw["use_occ"]:
            assert float(losses[3].detach()) == 0.0 and float(leaves[3].grad.abs().max()) == 0.0


def test_non_contiguous_inputs_are_made_contiguous(inputs):
    flow, img1, img2, mask = inputs["37x50"]
    wide = torch.zeros(2, 2, 37, 60)
    wide[..., 5:55] = flow
    wide_i = torch.zeros(2, 15, 37, 60)
    wide_i[..., 5:55] = img1
    leaf = wide.to(DEV).requires_grad_(True)
    view_f, view_i = leaf[..., 5:55], wide_i.to(DEV)[..., 5:55]
    assert not view_f.is_contiguous() and not view_i.is_contiguous()
    loss = ssim.ssim_loss(view_f, view_i, img2.to(DEV), mask.to(DEV), use_occ=True)
    loss.backward()
    ref_l, ref_g = run_gpu([flow], img1, img2, mask, use_occ=True)
    assert torch.equal(loss.detach().cpu(), ref_l[0]) and torch.equal(leaf.grad.cpu()[..., 5:55], ref_g[0])
    assert float(leaf.grad[..., :5].abs().max()) == 0.0


def test_flow_that_leaves_the_frame_everywhere(inputs):
    """A flow that points wholly out of the frame: Yw = 0, so the loss is that of img1 against zeros, and every result is finite."""
    _, img1, img2, mask = inputs["37x50"]
    b, c, h, w = img1.shape
    away = torch.full((b, 2, h, w), 1000.0)
    assert float(R.warp_taps(img2, away)["yw"].abs().max()) == 0.0
    for case in R.CASES:
        kw = case_kw(case)
        losses, grads = run_gpu([away], img1, img2, mask, **kw)
        assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(grads[0]).all())
        check("away", away, img1, img2, mask, losses[0], grads[0], **kw)
        assert float(grads[0].abs().max()) == 0.0                  # every corner is outside: the blend has no slope
        zeros = float(R.loss_from_warped(img1.double(), torch.zeros_like(img1).double(), mask.double(), **kw))
        assert float(R.loss(away, img1, img2, mask, **kw)) == zeros


def test_training_term_with_gamma(inputs):
    """train.ssim_loss: the last prediction alone, or sum_i gamma^(n-1-i) L_i over all - value and gradients."""
    base, img1, img2, mask = inputs["9x11"]
    flows = [base * (1.0 + 0.1 * i) for i in range(5)]
    kw = dict(use_occ=True, c1=1e-4, c2=9e-6)
    refs = [float(R.loss(f, img1, img2, mask, **kw)) for f in flows]
    bounds = [loss_bound(f, img1, img2, r, kw) for f, r in zip(flows, refs)]
    leaves = [f.to(DEV).requires_grad_(True) for f in flows]
    last = hip_train.ssim_loss(leaves, img1.to(DEV), img2.to(DEV), mask=mask.to(DEV), **kw)
    assert last.dtype == torch.float64 and abs(float(last.detach()) - refs[-1]) <= bounds[-1] * refs[-1]
    gamma = 0.8
    total = hip_train.ssim_loss(leaves, img1.to(DEV), img2.to(DEV), gamma=gamma, mask=mask.to(DEV), **kw)
    want = sum(gamma ** (4 - i) * r for i, r in enumerate(refs))
    assert abs(float(total.detach()) - want) <= (max(bounds) + 8 * 2.0 ** -52) * want            # (five products and adds more)
    total.backward()
    for i, (f, leaf) in enumerate(zip(flows, leaves)):
        g, a = R.gradient(f, img1, img2, mask, coef=gamma ** (4 - i), **kw)
        assert bool(((leaf.grad.cpu().double() - g).abs() <= 2.0 ** -23 * a).all()), i


# ------------------------------------------------------------------------------------------------ the trainer
def eemflow_net(seed):
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


@pytest.mark.parametrize("occ", [False, True])
def test_trainer_adds_the_ssim_term(monkeypatch, occ):
    """One autograd step of EEMFlow at 64 x 64, batch 2, ssim_weight=0.25 beside the supervised loss: the term is the restatement's
    value on the very prediction and the two event volumes (the loss bound), the logged loss is sequence loss + 0.25 * term (added in
    fp32 and printed with six decimals), the gradients are finite and the parameters change.  With ssim_occ the mask is mask_fw of
    fb_check on the prediction and the final flow of a twin network run on the exchanged volumes."""
    h = w = 64
    batch = supervised_batch(130, 2, h, w)
    net = eemflow_net(79)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    back = None
    if occ:
        twin = eemflow_net(79)
        twin.change_imagesize((h, w))
        with torch.no_grad():
            back = twin(batch["event_volume_new"], batch["event_volume_old"])[1][-1].float().contiguous()
    seq, term_calls = [], []
    spy(monkeypatch, "sequence_loss", seq)
    spy(monkeypatch, "ssim_loss", term_calls)
    log = Lines()
    tr = TrainRaftEvents([batch], (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd", mixed_precision=False, ssim_weight=0.25,
                         ssim_c1=1e-4, ssim_occ=occ)
    tr.train_iters(net, val_iters=1)
    assert len(log.lines) == 1 and len(seq) == 1 and len(term_calls) == 1 and tr.iteration == 1
    (preds, a, b), k, term = term_calls[0]
    assert torch.equal(a, batch["event_volume_old"]) and torch.equal(b, batch["event_volume_new"]) and k["gamma"] is None
    assert tuple(preds[-1].shape) == (2, 2, h, w) and k["use_occ"] is occ and k["c1"] == 1e-4 and k["c2"] == 9e-6
    mask = k["mask"]
    if occ:
        want = fb_check(preds[-1].detach().float().contiguous(), back)[0]
        assert mask is not None and tuple(mask.shape) == (2, 1, h, w) and torch.equal(mask, want)
    else:
        assert mask is None
    full = dict(use_occ=occ, c1=1e-4, c2=9e-6)
    flow = preds[-1].detach().float().cpu()
    ref = float(R.loss(flow, a.cpu(), b.cpu(), mask.cpu() if occ else None, **full))
    print("trainer term", float(term.detach()), "restatement", ref, "mask share", float(mask.mean()) if occ else 1.0)
    assert term.dtype == torch.float64 and ref > 0.0
    assert abs(float(term.detach()) - ref) <= loss_bound(flow, a.cpu(), b.cpu(), ref, full) * ref
    total = float(seq[0][2][0].detach()) + 0.25 * ref
    logged = float(log.lines[0].split("loss")[1].split()[0])
    assert abs(logged - total) <= 1e-5 * (1.0 + abs(total))
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    assert any(not torch.equal(p.detach(), before[n]) for n, p in net.named_parameters())


def test_zero_ssim_weight_changes_nothing(monkeypatch):
    """ssim_weight=0 with every other SSIM argument set: no call of the term, no second pass, and the step's loss and log line are
    bitwise those of a trainer without the arguments."""
    h = w = 64
    seq, term_calls = [], []
    spy(monkeypatch, "sequence_loss", seq)
    spy(monkeypatch, "ssim_loss", term_calls)
    lines = []
    for kw in ({}, dict(ssim_weight=0.0, ssim_occ=True, ssim_all=True, ssim_c1=1e-4)):
        log = Lines()
        tr = TrainRaftEvents([supervised_batch(130, 2, h, w)], (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd",
                             mixed_precision=False, **kw)
        tr.train_iters(eemflow_net(79), val_iters=1)
        lines.append(log.lines)
    assert not term_calls and len(seq) == 2
    assert torch.equal(seq[0][2][0], seq[1][2][0]) and lines[0] == lines[1] and len(lines[0]) == 1
