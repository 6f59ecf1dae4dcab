"""The photometric / census warp losses and their gradient on the GPU (csrc/photo.hip, eemflow_amd.photo, train.photo_loss and the
trainer's photometric term) against the fp64 restatement of tests/photo_reference.py on the same fp32 inputs.  Needs a real MI355X:
`pytest -m gpu`.

Bounds, each derived and none tuned:
  warp      the kernel's fp32 warped values are eemplus_warp(mode=1)'s and the restatement's, bit for bit (compared as such);
  loss, pointwise kinds
            relative error <= (terms + 16) * 2^-52: the worst case of summing `terms` non-negative fp64 numbers in any order (one
            rounding of 2^-53 per add, doubled) plus a few ulp of pow per term, which a mean of non-negative terms passes on
            unamplified (the masked form divides two such sums);
  loss, census
            per tap t = x / sqrt(0.81 + x*x) carries at most 3 roundings, |t| < 1, so t1 - t2 is off by at most 6 * 2^-53 (absolute:
            the difference cancels); e = (t1 - t2)^2 with |t1 - t2| < 2 is off by 4 * 6 * 2^-53 and e / (0.1 + e), whose slope is at
            most 10, by 240 * 2^-53.  dist sums T = (2r+1)^2 - 1 such taps: absolute error T * 240 * 2^-53, plus the order of the sum,
            T * 2^-53 relative.  rho passes an absolute error d of dist on with relative factor q d / (dist + 0.01) <= 100 q d
            (abs_robust) or 2 q dist d / (dist^2 + eps) <= q d / sqrt(eps) (charbonnier), the summation part with factor <= 2 q.
            Then the sum over the centres as above:  (terms + 16) * 2^-52 + amp * T * 240 * 2^-53 + 2 q T * 2^-53, amp = q / 0.01 or
            q / sqrt(eps) - 5e-11 for abs_robust at r = 3, 5e-10 / 5e-9 for charbonnier with eps = 1e-6 / 1e-8;
  golden    the reference's own fp32 losses: 4 * ref_gap relative, ref_gap (about 3.6e-7) the reference's distance from the fp64
            restatement;
  gradient  every cell within 2^-23 * A, A the product of the abs-sums of the cell's contributions: the one rounding of the fp64 value
            to fp32 is 2^-24 |g| <= 2^-24 A, doubled; the fp64 arithmetic in front of it is eight orders below.
The kernel's tile is 16 rows x 64 columns; (33, 129) is one row and one column more than two tiles each way."""
import ctypes

import pytest
import torch

from eemflow_amd import _lib, photo
from eemflow_amd import train as hip_train
from eemflow_amd.harness import Logger, TrainRaftEvents
from eemflow_amd.metrics import fb_check
from eemflow_amd.weights import synthetic_gt, synthetic_voxel_pair

import photo_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_H, TILE_W = 16, 64
SHAPES = {"7x7": (1, 3, 7, 7), "3x3": (1, 1, 3, 3), "9x11": (2, 5, 9, 11), "37x50": (2, 15, 37, 50),
          "tile+1": (2, 3, 2 * TILE_H + 1, 2 * TILE_W + 1)}


def case_kw(case):
    kind, occ, ch, av, r = case
    if kind in R.POINTWISE:
        return dict(kind=kind, use_occ=occ)
    return dict(kind=kind, use_occ=occ, q=R.Q, charbonnier=ch, average=av, max_distance=r)


def loss_bound(shape, kw):
    terms = R.term_count(shape, kw["kind"])
    if kw["kind"] in R.POINTWISE:
        return (terms + 16) * 2.0 ** -52
    taps = (2 * kw["max_distance"] + 1) ** 2 - 1
    q = kw["q"]
    amp = q / ((1e-6 if kw["use_occ"] else 1e-8) ** 0.5) if kw["charbonnier"] else q / 0.01
    return (terms + 16) * 2.0 ** -52 + amp * taps * 240 * 2.0 ** -53 + 2 * q * taps * 2.0 ** -53


@pytest.fixture(scope="module")
def inputs():
    out = {name: tuple(torch.from_numpy(a) for a in R.inputs(11 + i, s)) for i, (name, s) in enumerate(SHAPES.items())}
    out["zero"] = tuple(torch.from_numpy(a) for a in R.inputs(5, SHAPES["9x11"], zero_mask=True))
    return out


def run_gpu(flows, img1, img2, mask, coefs=None, **kw):
    """(losses, gradients) of photo_many through autograd, on the host; coefs: the upstream gradient per job."""
    leaves = [f.to(DEV).requires_grad_(True) for f in flows]
    losses = photo.photo_many(leaves, img1.to(DEV), img2.to(DEV), mask.to(DEV) if mask is not None else None, **kw)
    assert losses.dtype == torch.float64 and tuple(losses.shape) == (len(flows),)
    up = torch.ones(len(flows), dtype=torch.float64) if coefs is None else torch.tensor(coefs, dtype=torch.float64)
    (losses * up.to(DEV)).sum().backward()
    return losses.detach().cpu(), [f.grad.cpu() for f in leaves]


def check(tag, flow, img1, img2, mask, loss, grad, coef=1.0, **kw):
    ref = float(R.loss(flow, img1, img2, mask, **kw))
    bound = loss_bound(img1.shape, kw)
    rel = abs(float(loss) - ref) / abs(ref) if ref != 0.0 else abs(float(loss))
    g, a = R.gradient(flow, img1, img2, mask, coef=coef, **kw)
    assert grad.dtype == torch.float32 and grad.shape == flow.shape
    ratio = float(((grad.double() - g).abs() / (2.0 ** -23 * a).clamp(min=1e-300)).max())
    print(tag, sorted(kw.items()), "loss rel %.2e of bound %.2e, gradient worst |d| / bound %.3f" % (rel, bound, ratio))
    assert rel <= bound, (tag, rel, bound)
    assert bool(((grad.double() - g).abs() <= 2.0 ** -23 * a).all()), (tag, ratio)
    assert bool(torch.isfinite(grad).all())


def test_warped_values_are_those_of_eemplus_warp_and_of_the_restatement(inputs):
    for name in SHAPES:
        flow, _, img2, _ = inputs[name]
        x, f = img2.to(DEV), flow.to(DEV)
        out = torch.empty_like(x)
        b, c, h, w = x.shape
        _lib.check(_lib.lib().eemplus_warp(x.data_ptr(), f.data_ptr(), b, c, h, w, 1, out.data_ptr(), _lib.current_stream_ptr(x.device)))
        assert torch.equal(out.cpu(), R.warp_taps(img2, flow)["yw"]), name


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-occ%d-ch%d-av%d-r%d" % c)
def test_loss_and_gradient_match_the_fp64_restatement(inputs, case):
    kw = case_kw(case)
    r = kw.get("max_distance", 0)
    for name, shape in SHAPES.items():
        if kw["kind"] == "census" and (shape[2] <= 2 * r or shape[3] <= 2 * r):
            continue                                               # (3 x 3 takes r = 1 alone; photo_many refuses the rest, tested below)
        flow, img1, img2, mask = inputs[name]
        for m in ((mask, None) if kw["use_occ"] else (mask,)):
            losses, grads = run_gpu([flow], img1, img2, m, **kw)
            check(name + ("" if m is not None else " no mask"), flow, img1, img2, m, losses[0], grads[0], **kw)


@pytest.mark.parametrize("kw", [dict(kind="census", use_occ=True, q=R.Q, charbonnier=True, average=True, max_distance=3),
                                dict(kind="abs_robust", use_occ=False)], ids=["census", "abs_robust"])
def test_more_tiles_than_blocks(kw):
    """520 samples of 2 x 2 tiles: 2080 tiles on the grid's cap of 2048 blocks, so 32 blocks walk a second tile and add it to their
    loss slots; census with its mask, abs_robust without one.  The same bounds as everywhere."""
    flow, img1, img2, mask = (torch.from_numpy(a) for a in R.inputs(23, (520, 3, TILE_H + 1, TILE_W + 1)))
    m = mask if kw["use_occ"] else None
    losses, grads = run_gpu([flow], img1, img2, m, **kw)
    check("520 x 17x65", flow, img1, img2, m, losses[0], grads[0], **kw)


def test_losses_match_the_reference_own_values(golden):
    g = golden("photo.npz")
    gap = float(g["ref_gap"])
    worst = 0.0
    for i in range(int(g["ncases"])):
        flow, img1, img2, mask = (torch.from_numpy(g[f"{n}_{i}"]).to(DEV) for n in ("flow", "img1", "img2", "mask"))
        for ci, case in enumerate(R.CASES):
            mine = float(photo.photo_loss(flow, img1, img2, mask, **case_kw(case)))
            ref = float(g[f"loss_{i}"][ci])
            worst = max(worst, abs(mine - ref) / abs(ref))
    print("against the reference's fp32 values: worst relative difference %.3e, bound %.3e" % (worst, 4 * gap))
    assert worst <= 4 * gap


@pytest.mark.parametrize("k", [1, 3, 16, 20])
@pytest.mark.parametrize("kind", ["census", "abs_robust"])
def test_many_jobs_share_the_images_bitwise(inputs, k, kind):
    """k flows against ONE pair of images and one mask (20: two library calls), each with its own upstream gradient: jobs within the
    bounds, and bitwise what a one-job call gives."""
    base, img1, img2, mask = inputs["tile+1"]
    kw = dict(kind="census", use_occ=True, q=R.Q, charbonnier=True, average=True, max_distance=2) if kind == "census" else \
        dict(kind=kind, use_occ=True)
    flows = [base + 0.01 * i * torch.flip(base, dims=[3]) for i in range(k)]
    coefs = [(-1.0) ** i * (0.25 + 0.5 * i) for i in range(k)]
    losses, grads = run_gpu(flows, img1, img2, mask, coefs, **kw)
    for i in sorted({0, k // 2, k - 1}):
        check(f"job {i} of {k}", flows[i], img1, img2, mask, losses[i], grads[i], coef=coefs[i], **kw)
    for i in range(k):
        one_l, one_g = run_gpu([flows[i]], img1, img2, mask, [coefs[i]], **kw)
        assert torch.equal(one_l[0], losses[i]) and torch.equal(one_g[0], grads[i]), i


def test_mixed_images_and_masks_in_one_call(inputs):
    """Lists of images and masks: shared img1, another img1, no mask, the all-zero mask - every job is its one-job result, and the
    all-zero mask gives exactly 0 and an exactly zero gradient."""
    flow, img1, img2, mask = inputs["9x11"]
    zero = inputs["zero"][3]
    other = torch.flip(img1, dims=[2])
    d = DEV
    i1 = [img1.to(d)] * 2 + [other.to(d)] + [img1.to(d)] * 2
    i2 = [img2.to(d)] * 5
    ms = [mask.to(d), None, mask.to(d), zero.to(d), mask.to(d)]
    fl = [flow, flow * 0.5, flow + 0.1, flow, flow * -1.0]
    for kw in (dict(kind="census", use_occ=True, max_distance=3), dict(kind="census", use_occ=True, charbonnier=True, average=False, max_distance=1),
               dict(kind="charbonnier", use_occ=True)):
        leaves = [f.to(d).requires_grad_(True) for f in fl]
        losses = photo.photo_many(leaves, i1, i2, ms, **kw)
        losses.sum().backward()
        for j in range(5):
            m = ms[j].cpu() if ms[j] is not None else None
            full = {**dict(q=R.Q, charbonnier=False, average=True), **kw} if kw["kind"] == "census" else kw
            check(f"mixed {j}", fl[j], i1[j].cpu(), img2, m, losses[j].detach().cpu(), leaves[j].grad.cpu(), **full)
            one_l, one_g = run_gpu([fl[j]], i1[j].cpu(), img2, m, **kw)
            assert torch.equal(one_l[0], losses[j].detach().cpu()) and torch.equal(one_g[0], leaves[j].grad.cpu()), j
        assert float(losses[3].detach()) == 0.0 and float(leaves[3].grad.abs().max()) == 0.0


def test_two_runs_give_the_same_bits(inputs):
    flow, img1, img2, mask = inputs["tile+1"]
    for kw in (dict(kind="census", use_occ=True, max_distance=3), dict(kind="census", charbonnier=True, max_distance=2), dict(kind="L1"),
               dict(kind="abs_robust", use_occ=True)):
        a = run_gpu([flow, flow * 0.5, flow + 1.0], img1, img2, mask, [1.0, -2.0, 0.5], **kw)
        b = run_gpu([flow, flow * 0.5, flow + 1.0], img1, img2, mask, [1.0, -2.0, 0.5], **kw)
        assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_explicit_default_gray_equals_the_default(inputs):
    for name in ("7x7", "9x11", "37x50"):
        flow, img1, img2, mask = inputs[name]
        c = img1.shape[1]
        a = run_gpu([flow], img1, img2, mask, kind="census", use_occ=True, max_distance=3)
        b = run_gpu([flow], img1, img2, mask, kind="census", use_occ=True, max_distance=3, gray=photo.default_gray(c))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    flow, img1, img2, mask = inputs["9x11"]
    gray = (0.5, 0.0, -0.25, 0.125, 1.0)                           # another weighting: the restatement with the same weights
    losses, grads = run_gpu([flow], img1, img2, mask, [0.75], kind="census", max_distance=2, gray=gray)
    check("gray", flow, img1, img2, mask, losses[0], grads[0], coef=0.75, kind="census", use_occ=False, q=R.Q, charbonnier=False, average=True,
          max_distance=2, gray=gray)


def test_non_contiguous_inputs_are_made_contiguous(inputs):
    flow, img1, img2, mask = inputs["37x50"]
    wide = torch.zeros(2, 2, 37, 60)
    wide[..., 5:55] = flow
    wide_i = torch.zeros(2, 15, 37, 60)
    wide_i[..., 5:55] = img1
    leaf = wide.to(DEV).requires_grad_(True)
    view_f, view_i = leaf[..., 5:55], wide_i.to(DEV)[..., 5:55]
    assert not view_f.is_contiguous() and not view_i.is_contiguous()
    loss = photo.photo_loss(view_f, view_i, img2.to(DEV), mask.to(DEV), kind="census", use_occ=True, max_distance=1)
    loss.backward()
    ref_l, ref_g = run_gpu([flow], img1, img2, mask, kind="census", use_occ=True, max_distance=1)
    assert torch.equal(loss.detach().cpu(), ref_l[0]) and torch.equal(leaf.grad.cpu()[..., 5:55], ref_g[0])
    assert float(leaf.grad[..., :5].abs().max()) == 0.0


def test_training_term_with_gamma(inputs):
    """train.photo_loss: the last prediction alone, or sum_i gamma^(n-1-i) L_i over all - value and gradients."""
    base, img1, img2, mask = inputs["9x11"]
    flows = [base * (1.0 + 0.1 * i) for i in range(5)]
    kw = dict(kind="census", use_occ=True, q=R.Q, charbonnier=False, average=True, max_distance=2)
    refs = [float(R.loss(f, img1, img2, mask, **kw)) for f in flows]
    bound = loss_bound(img1.shape, kw)
    leaves = [f.to(DEV).requires_grad_(True) for f in flows]
    last = hip_train.photo_loss(leaves, img1.to(DEV), img2.to(DEV), mask=mask.to(DEV), **kw)
    assert last.dtype == torch.float64 and abs(float(last.detach()) - refs[-1]) <= bound * refs[-1]
    gamma = 0.8
    total = hip_train.photo_loss(leaves, img1.to(DEV), img2.to(DEV), gamma=gamma, mask=mask.to(DEV), **kw)
    want = sum(gamma ** (4 - i) * r for i, r in enumerate(refs))
    assert abs(float(total.detach()) - want) <= (bound + 8 * 2.0 ** -52) * want             # (five products and adds more)
    total.backward()
    for i, (f, leaf) in enumerate(zip(flows, leaves)):
        g, a = R.gradient(f, img1, img2, mask, coef=gamma ** (4 - i), **kw)
        assert bool(((leaf.grad.cpu().double() - g).abs() <= 2.0 ** -23 * a).all()), i


def test_small_frames_raise_and_non_finite_flows_stay_in_their_job(inputs):
    flow, img1, img2, mask = inputs["9x11"]
    bad = flow.clone()
    bad[1, 0, 2, 3] = float("nan")
    losses, grads = run_gpu([bad, flow], img1, img2, mask, kind="L1")
    assert not bool(torch.isfinite(losses[0])) and bool(torch.isfinite(losses[1]))
    check("beside a nan", flow, img1, img2, mask, losses[1], grads[1], kind="L1", use_occ=False)
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(ValueError, match="H > 6"):
        photo.photo_loss(z(1, 2, 6, 8), z(1, 3, 6, 8), z(1, 3, 6, 8))
    with pytest.raises(ValueError, match="W > 2"):
        photo.photo_loss(z(1, 2, 8, 2), z(1, 3, 8, 2), z(1, 3, 8, 2), max_distance=1)
    with pytest.raises(ValueError, match="SSIM"):
        photo.photo_loss(z(1, 2, 8, 8), z(1, 3, 8, 8), z(1, 3, 8, 8), kind="SSIM")
    with pytest.raises(_lib.EEMFlowHipError, match="no CPU path"):
        photo.photo_loss(torch.zeros(1, 2, 8, 8), z(1, 3, 8, 8), z(1, 3, 8, 8))
    # the library's own check, past the Python one
    p, im = z(1, 2, 6, 8), z(1, 3, 6, 8)
    out = torch.zeros(64, device=DEV, dtype=torch.float64)
    one = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    rc = _lib.lib().eemflow_photo_many(1, one(p), one(im), one(im), None, 1, 3, 6, 8, 3, 0, 0, 1, 3, 0.4, None, None, out.data_ptr(), None,
                                       out.data_ptr(), _lib.current_stream_ptr(p.device))
    assert rc != 0 and "H > 6" in _lib.lib().eemflow_last_error().decode()


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
def test_trainer_adds_the_photometric_term(monkeypatch, occ):
    """One autograd step of EEMFlow at 64 x 64, batch 2, photo_weight=0.25 beside the supervised loss: the term is the restatement's
    value on the very prediction and the two event volumes (the loss bound), the logged loss is sequence loss + 0.25 * term (added in
    fp32 and printed with six decimals), parameters change.  With photo_occ the mask is mask_fw of fb_check on the prediction and the
    final flow of a twin network run on the exchanged volumes."""
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
    seq, pho = [], []
    spy(monkeypatch, "sequence_loss", seq)
    spy(monkeypatch, "photo_loss", pho)
    log = Lines()
    kw = dict(kind="census", q=0.4, charbonnier=True, max_distance=2)
    tr = TrainRaftEvents([batch], (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd", mixed_precision=False, photo_weight=0.25,
                         photo_kind="census", photo_charbonnier=True, photo_max_distance=2, photo_occ=occ)
    tr.train_iters(net, val_iters=1)
    assert len(log.lines) == 1 and len(seq) == 1 and len(pho) == 1 and tr.iteration == 1
    (preds, a, b), k, term = pho[0]
    assert torch.equal(a, batch["event_volume_old"]) and torch.equal(b, batch["event_volume_new"]) and k["gamma"] is None
    assert tuple(preds[-1].shape) == (2, 2, h, w) and k["use_occ"] is occ and {n: k[n] for n in kw} == kw
    mask = k["mask"]
    if occ:
        want = fb_check(preds[-1].detach().float().contiguous(), back)[0]
        assert mask is not None and tuple(mask.shape) == (2, 1, h, w) and torch.equal(mask, want)
    else:
        assert mask is None
    full = dict(use_occ=occ, average=True, **kw)
    ref = float(R.loss(preds[-1].detach().float().cpu(), a.cpu(), b.cpu(), mask.cpu() if occ else None, **full))
    print("trainer term", float(term.detach()), "restatement", ref, "mask share", float(mask.mean()) if occ else 1.0)
    assert term.dtype == torch.float64 and ref > 0.0
    assert abs(float(term.detach()) - ref) <= loss_bound(a.shape, full) * ref
    total = float(seq[0][2][0].detach()) + 0.25 * ref
    logged = float(log.lines[0].split("loss")[1].split()[0])
    assert abs(logged - total) <= 1e-5 * (1.0 + abs(total))
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    assert any(not torch.equal(p.detach(), before[n]) for n, p in net.named_parameters())


def test_zero_photo_weight_changes_nothing(monkeypatch):
    """photo_weight=0 with every other photo argument set: no call of the term, no second pass, and the step's loss and log line are
    bitwise those of a trainer without the arguments."""
    h = w = 64
    seq, pho = [], []
    spy(monkeypatch, "sequence_loss", seq)
    spy(monkeypatch, "photo_loss", pho)
    lines = []
    for kw in ({}, dict(photo_weight=0.0, photo_kind="L1", photo_occ=True, photo_all=True)):
        log = Lines()
        tr = TrainRaftEvents([supervised_batch(130, 2, h, w)], (h, w), lr=1e-4, logger=log, print_freq=1, engine="autograd",
                             mixed_precision=False, **kw)
        tr.train_iters(eemflow_net(79), val_iters=1)
        lines.append(log.lines)
    assert not pho and len(seq) == 2
    assert torch.equal(seq[0][2][0], seq[1][2][0]) and lines[0] == lines[1] and len(lines[0]) == 1
