"""A NaN or an infinity in a training step reaches the loss and the gradient, and the optimizer skips the step: the reason
the non-finite contract exists.  `pytest -m gpu`; the kernels' own cases are in tests/test_gpu_nonfinite_ops.py, the inference stages in
tests/test_gpu_nonfinite_models.py.

EEMFlow (the C training step, eemflow_forward_backward + eemflow_optimizer_step) with a poisoned input voxel, a poisoned ground-truth
flow at a valid pixel and one poisoned weight; E-RAFT (two iterations) and EEMFlow+ under autograd with a poisoned input voxel, at their
training tests' smallest shapes.  In every case, against oracle/train_oracle.py's loss and torch's autograd through the oracle on the
CPU (tests/test_nonfinite_host.py runs the same oracle and proves its loss non-finite, and finite without the poison):
  * the loss is non-finite (the ground-truth case: see LEFT OUT);
  * every parameter whose oracle gradient holds a non-finite value has one on the GPU;
  * EEMFlow: the optimizer step that follows is skipped exactly when the oracle's gradient is non-finite - GradScaler.step's rule in the
    reference loop - `skipped_steps()` rises by one, and weights, moments and the bias-correction count stay bitwise what they were
    (a second trainer that never saw the poisoned step stays bitwise equal through a following step on a fixed gradient).

LEFT OUT, and why: the LOSS under a poisoned GROUND TRUTH.  |gt| < 400 fails for a NaN or an infinity, so the pixel is invalid;
the reference's valid * |flow - gt| = 0 * NaN makes its loss NaN while its gradient, valid * sign(.), stays finite (torch: sign(NaN)
= 0) - the reference logs a NaN loss and steps.  The loss kernel (train.hip) SELECTS the valid pixels on purpose: MVSEC's ground truth
holds an infinity at every pixel without a measurement and the loaders hand it on as it is (tests/test_gpu_augment.py trains on such
batches and requires finite losses), so an invalid pixel's ground truth never reaches the loss.  Documented in the kernel's header.  The
case stays for what both sides agree on: finite gradients and a step that is taken, and the loss is the clean batch's with that pixel
marked invalid.
"""
import functools

import pytest
import torch

from oracle import eemflow_oracle as O
from oracle import eemflow_plus_oracle as P
from oracle import eraft_oracle as R
from oracle import nonfinite as N
from oracle import train_oracle as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# model, what is poisoned, batch, h, w (the training tests' smallest shapes), seed
CASES = [{"id": "eemflow-voxel", "model": "eemflow", "poison": "voxel", "b": 2, "h": 64, "w": 64, "seed": 23},
         {"id": "eemflow-gt", "model": "eemflow", "poison": "gt", "b": 2, "h": 64, "w": 64, "seed": 23},
         {"id": "eemflow-weight", "model": "eemflow", "poison": "weight", "b": 2, "h": 64, "w": 64, "seed": 23},
         {"id": "eraft-voxel", "model": "eraft", "poison": "voxel", "b": 1, "h": 136, "w": 200, "seed": 31, "iters": 2},
         {"id": "plus-voxel", "model": "plus", "poison": "voxel", "b": 1, "h": 128, "w": 192, "seed": 13}]
POISONED_WEIGHT = ("pconv2_2.0.weight", (3, 5, 1, 1))


def seeded_sd(case):
    """The model's seeded state dict as numpy arrays (what the GPU module loads) - no GPU needed."""
    if case["model"] == "eemflow":
        from eemflow_amd.weights import seeded_state_dict
        return seeded_state_dict(case["seed"])
    if case["model"] == "eraft":
        from eemflow_amd.eraft import ERAFT
        from eemflow_amd.eraft_weights import seeded_from_shapes
        net = ERAFT("", 5)
    else:
        from eemflow_amd.eemflow_plus import EEMFlow_cdc
        from eemflow_amd.plus_weights import seeded_from_shapes
        net = EEMFlow_cdc("", 3, 5)
    return seeded_from_shapes({k: tuple(v.shape) for k, v in net.state_dict().items()}, case["seed"])


def build(case, poisoned=True):
    """(state dict as numpy, e1, e2, gt, valid) on the CPU, with the case's poison."""
    from eemflow_amd.weights import synthetic_gt, synthetic_voxel_pair
    b, h, w, seed = case["b"], case["h"], case["w"], case["seed"]
    sd = {k: v.copy() for k, v in seeded_sd(case).items()}
    e1, e2 = (torch.from_numpy(a).clone() for a in synthetic_voxel_pair(seed + 1, b, h, w))
    gt, valid = (torch.from_numpy(a).clone() for a in synthetic_gt(seed + 2, b, h, w))
    if poisoned and case["poison"] == "voxel":
        e1[0, 2, h // 2 + 1, w // 2 - 3] = N.NAN
    elif poisoned and case["poison"] == "gt":
        y, x = (int(v) for v in torch.nonzero(valid[b - 1] >= 0.5)[7])
        gt[b - 1, 1, y, x] = N.PINF
    elif poisoned and case["poison"] == "weight":
        name, at = POISONED_WEIGHT
        sd[name][at] = N.NAN
    return sd, e1, e2, gt, valid


def _flag(t):
    return t is not None and not bool(torch.isfinite(t).all())


@functools.lru_cache(maxsize=None)
def oracle(case_id, poisoned=True):
    """(loss, {parameter: its oracle gradient holds a non-finite value}) by torch's autograd through the oracle, fp32 on the CPU."""
    case = next(c for c in CASES if c["id"] == case_id)
    sdn, e1, e2, gt, valid = build(case, poisoned)
    sd = O.to_torch_sd(sdn)
    if case["model"] == "eemflow":
        loss, _, grads, _ = T.loss_and_grads(sd, e1, e2, gt, valid, image_size=(case["h"], case["w"]))
        return float(loss), {k: _flag(g) for k, g in grads.items()}
    params = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone()) for k, v in sd.items()}
    if case["model"] == "eraft":
        preds, _ = R.eraft_forward(params, e1, e2, iters=case["iters"], image_size=(case["h"], case["w"]), bn_training=True)
    else:
        preds = P.eemflow_plus_forward(params, e1, e2, image_size=(case["h"], case["w"]))
        preds = preds[0] if isinstance(preds, tuple) else preds
    loss, _ = T.sequence_loss(list(preds), gt, valid, 0.8)
    loss.backward()
    return float(loss), {k: _flag(v.grad) for k, v in params.items() if v.is_floating_point() and v.requires_grad and v.grad is not None}


def premises(case):
    """On the CPU: the oracle's loss is non-finite with the poison and finite without it; a poisoned voxel or weight reaches a gradient."""
    loss, flags = oracle(case["id"])
    clean, cflags = oracle(case["id"], False)
    assert clean == clean and abs(clean) < float("inf") and not any(cflags.values()), (clean, [k for k, f in cflags.items() if f])
    assert not (loss == loss and abs(loss) < float("inf")), f"{case['id']}: the oracle's loss {loss} is finite - the case is vacuous"
    if case["poison"] == "gt":
        assert not any(flags.values()), "valid * sign(NaN) = 0: the reference's gradient is finite under a poisoned ground truth"
    else:
        assert any(flags.values())


# ------------------------------------------------------------------------------------------------------------------ EEMFlow, the C step
def _eemflow(sdn, h, w):
    from eemflow_amd import EEMFlow
    net = EEMFlow("", groups=5, n_first_channels=5)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()})
    net = net.to(DEV).train()
    net.change_imagesize((h, w))
    return net


def _weights(tr, net):
    tr.sync_parameters()
    return torch.cat([v.reshape(-1).float() for v in net.state_dict().values()]).view(torch.int32).cpu()


def _split(flat, sdn):
    out, off = {}, 0
    for k, v in sdn.items():
        out[k] = flat[off:off + v.size]
        off += v.size
    return out


@pytest.mark.parametrize("case", [c for c in CASES if c["model"] == "eemflow"], ids=lambda c: c["id"])
def test_eemflow_step_is_skipped_exactly_when_the_oracle_gradient_is_non_finite(case):
    from eemflow_amd import _lib
    from eemflow_amd.train import EEMFlowTrainer
    h, w = case["h"], case["w"]
    rloss, rflags = oracle(case["id"])
    sdn, e1, e2, gt, valid = build(case)
    _, c1, c2, cgt, cvalid = build(case, poisoned=False)
    L, sp = _lib.lib(), _lib.current_stream_ptr(torch.device(DEV))
    # a finite gradient to step on, from the clean batch (on the poisoned weights where the case poisons one: only its finite entries count)
    nets = [_eemflow(sdn, h, w) for _ in range(2)]
    trs = [EEMFlowTrainer(n, lr=1e-3, wdecay=5e-5, epsilon=1e-8, num_steps=20, clip=1.0) for n in nets]
    clean_net = _eemflow(build(case, poisoned=False)[0], h, w)
    ctr = EEMFlowTrainer(clean_net, lr=0.0, wdecay=0.0, clip=0.0)
    closs, _, _ = ctr.step(c1.to(DEV), c2.to(DEV), cgt.to(DEV), cvalid.to(DEV))
    g0 = ctr.grad.clone()
    assert closs == closs and bool(torch.isfinite(g0).all())
    for n, tr in zip(nets, trs):                                   # both trainers: one real step on g0 (moments and the step count now nonzero)
        n._context(torch.device(DEV))
        _lib.check(L.eemflow_optimizer_step(n._ctx, g0.data_ptr(), 1e-3, 5e-5, 1e-8, 1.0, sp))
    w0 = _weights(trs[0], nets[0])
    assert torch.equal(w0, _weights(trs[1], nets[1])) and trs[0].skipped_steps() == 0
    # the poisoned step on the first trainer only
    loss, _, flow = trs[0].step(e1.to(DEV), e2.to(DEV), gt.to(DEV), valid.to(DEV))
    grads = _split(trs[0].grad.cpu(), sdn)
    print(f"{case['id']}: loss {loss} (oracle {rloss}); non-finite gradients {sum(_flag(g) for g in grads.values())} of {len(grads)} "
          f"(oracle {sum(rflags.values())}); skipped {trs[0].skipped_steps()}")
    if case["poison"] == "gt":
        # (LEFT OUT above: the kernel selects the valid pixels; the poisoned one is dropped exactly as a pixel marked invalid is)
        _, _, _, pgt, pvalid = build(case)
        dropped = pvalid * torch.isfinite(pgt).all(1).float()
        ref_loss, _, _ = trs[1].step(c1.to(DEV), c2.to(DEV), cgt.to(DEV), dropped.to(DEV))     # (the same weights: one step on g0)
        # (the loss's blocks meet in fp64 atomics: equal to a few units of fp64 rounding; one pixel's share is ~1e-5 of the loss)
        assert ref_loss == ref_loss and abs(loss - ref_loss) <= 1e-9 * abs(ref_loss), (loss, ref_loss)
    else:
        assert not (loss == loss and abs(loss) < float("inf")), f"the loss {loss} is finite; the oracle's is {rloss}"
    missing = [k for k, f in rflags.items() if f and not _flag(grads[k])]
    assert not missing, f"finite on the GPU, non-finite in the oracle: {missing}"
    want_skip = any(rflags.values())
    assert any(_flag(g) for g in grads.values()) == want_skip
    assert trs[0].skipped_steps() == int(want_skip)
    if want_skip:
        assert torch.equal(_weights(trs[0], nets[0]), w0), "a skipped step changed the weights"
        # moments and the bias-correction count: one more step on g0 leaves both trainers bitwise equal
        for n in nets:
            _lib.check(L.eemflow_optimizer_step(n._ctx, g0.data_ptr(), 1e-3, 5e-5, 1e-8, 1.0, sp))
        assert torch.equal(_weights(trs[0], nets[0]), _weights(trs[1], nets[1])), "a skipped step changed the moments or the step count"
        assert trs[0].skipped_steps() == 1 and trs[1].skipped_steps() == 0
    else:
        assert not torch.equal(_weights(trs[0], nets[0]), w0)      # the reference steps on a finite gradient whatever the loss; so does this


# ------------------------------------------------------------------------------------------------------------------ E-RAFT, EEMFlow+: autograd
def _autograd_model(case, sdn):
    if case["model"] == "eraft":
        from eemflow_amd.eraft import ERAFT
        net = ERAFT("", 5)
    else:
        from eemflow_amd.eemflow_plus import EEMFlow_cdc
        net = EEMFlow_cdc("", 3, 5)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()})
    net = net.to(DEV).train()
    net.change_imagesize((case["h"], case["w"]))
    return net


@pytest.mark.parametrize("case", [c for c in CASES if c["model"] != "eemflow"], ids=lambda c: c["id"])
def test_autograd_training_keeps_the_poison(case):
    from eemflow_amd import train as hip_train
    rloss, rflags = oracle(case["id"])
    sdn, e1, e2, gt, valid = build(case)
    net = _autograd_model(case, sdn)
    kw = {"iters": case["iters"]} if case["model"] == "eraft" else {}
    _, preds = net(e1.to(DEV), e2.to(DEV), **kw)
    loss, _ = hip_train.sequence_loss(list(preds), gt.to(DEV), valid.to(DEV), 0.8)
    loss.backward()
    torch.cuda.synchronize()
    named = dict(net.named_parameters())
    bad = {k: _flag(p.grad) for k, p in named.items()}
    print(f"{case['id']}: loss {float(loss)} (oracle {rloss}); non-finite gradients {sum(bad.values())} of {len(bad)} (oracle {sum(rflags.values())})")
    assert not bool(torch.isfinite(loss)), f"the loss {float(loss)} is finite; the oracle's is {rloss}"
    missing = [k for k, f in rflags.items() if f and k in named and not bad[k]]
    assert not missing, f"finite on the GPU, non-finite in the oracle: {missing}"
    assert any(bad.values())
