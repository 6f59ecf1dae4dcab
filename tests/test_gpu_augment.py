"""Augmentation on the GPU (eemflow_augment_many through eemflow_amd.augment_many) against the host route bit for bit: the reference's
own flip / crop outputs, the full flip x offset x crop matrix on both store forms, the rescaling form, batching, the argument errors,
and the datasets' get_batch / the loader's device batches against the stacked per-sample route.  `pytest -m gpu`."""
import itertools
import os

import numpy as np
import pytest
import torch

from eemflow_amd import _lib, augment_many, hrem, mvsec
from eemflow_amd.augmentor import AugPlan, DenseSparseAugmentor, FlowAugmentor, apply_host
from eemflow_amd.loader import ThreadedBatchLoader

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ helpers
def chw(a):
    """HWC numpy -> (C,H,W) tensor, as the datasets hand the augmentors' arrays back (mvsec.py / hrem.py)."""
    return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)


def host_route(plan, old, new, flow):
    """What the datasets' host route makes of one sample: (old, new, flow, valid) CPU tensors.  old, new, flow: HWC numpy."""
    o, n, f = apply_host(plan, old, new, flow)
    fl = chw(f).float()
    valid = (~torch.isinf(fl[0]) & ~torch.isinf(fl[1]) & (torch.linalg.norm(fl, dim=0) > 0)).float()         # mvsec.py:248
    return chw(o).float().contiguous(), chw(n).float().contiguous(), fl.contiguous(), valid


def first_difference(got, want, equal_nan):
    """None when got and want hold the same bits (NaNs in the same places with equal_nan), else a description of the first element
    that differs."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{got.dtype} {tuple(got.shape)} against {want.dtype} {tuple(want.shape)}"
    bad = got.view(torch.int32) != want.view(torch.int32)
    if equal_nan:
        bad &= ~(torch.isnan(got) & torch.isnan(want))
    if not bool(bad.any()):
        return None
    at = tuple(int(v) for v in bad.nonzero()[0])
    return f"first difference at {at}: got {got[at].item()!r} ({got[at].item().hex()}), want {want[at].item()!r} ({want[at].item().hex()}); {int(bad.sum())} differ"


def assert_same(got, want, what, equal_nan=False):
    for name, g, w in zip(("old", "new", "flow", "valid"), got, want):
        diff = first_difference(g, w, equal_nan)
        assert diff is None, f"{what}: {name}: {diff}"


def device_route(plans, samples, **kw):
    """samples: (old, new, flow) HWC numpy per plan -> augment_many's four batch tensors."""
    up = lambda a: chw(a).contiguous().to(DEV)                    # noqa: E731
    return augment_many(plans, [up(s[0]) for s in samples], [up(s[1]) for s in samples], [up(s[2]) for s in samples], **kw)


def stacked_host(plans, samples):
    rows = [host_route(p, *s) for p, s in zip(plans, samples)]
    return tuple(torch.stack([r[k] for r in rows]) for k in range(4))


def make_sample(seed, h, w, c, flow_dtype, special=False):
    rng = np.random.default_rng(seed)
    old, new = (rng.standard_normal((h, w, c)).astype(np.float32) for _ in range(2))
    flow = rng.standard_normal((h, w, 2)).astype(flow_dtype)
    if special:                                                   # an infinity, an exact (0, 0) patch, squares that underflow in fp32
        flow[3, 4, 0] = np.inf
        flow[h - 2, w - 3, 1] = -np.inf
        flow[8:14, 10:19] = 0.0
        tiny = 2.0 ** -75                                          # tiny * tiny = 2^-150 rounds to 0 in fp32, (1.0001 tiny)^2 to 2^-149
        flow[15, 5:11] = [[tiny, 0], [tiny * 1.0001, 0], [tiny, tiny], [0, -tiny * 1.0001], [1e-20, 0], [1e-30, 1e-30]]
        flow[16, 5] = [np.nan, 1.0]
    return old, new, flow


# ------------------------------------------------------------------------------------------------ the reference's own outputs
def test_flips_and_crops_equal_the_reference_classes_outputs(golden):
    g = golden("augmentor.npz")
    for k, (seed, h, w, ch, cw, flip) in enumerate(g["cases"].tolist()):
        rng = np.random.default_rng(100 + seed)                  # the inputs the golden was made from (tests/test_data_rows.py)
        a, b, da, db = (rng.standard_normal((h, w, 3)).astype(np.float32) for _ in range(4))
        fl = rng.standard_normal((h, w, 2))
        np.random.seed(seed)
        plan = FlowAugmentor(crop_size=[ch, cw], do_flip=bool(flip)).draw(h, w, without_resize=True)
        old, new, flow, _ = device_route([plan], [(a, b, fl)])
        want = [g[f"flow_nr_{k}_{i}"] for i in range(3)]
        assert torch.equal(old[0].cpu(), chw(want[0])) and torch.equal(new[0].cpu(), chw(want[1])), k
        assert torch.equal(flow[0].cpu(), chw(want[2].astype(np.float32))), k
        np.random.seed(seed)
        plan = DenseSparseAugmentor(crop_size=[ch, cw], do_flip=bool(flip)).draw(h, w)
        want = [g[f"dense_{k}_{i}"] for i in range(5)]
        for (x, y), (wx, wy) in (((a, b), want[0:2]), ((da, db), want[2:4])):
            old, new, flow, _ = device_route([plan], [(x, y, fl)])
            assert tuple(old.shape) == (1, 3, ch, cw)
            assert torch.equal(old[0].cpu(), chw(wx)) and torch.equal(new[0].cpu(), chw(wy)), k
            assert torch.equal(flow[0].cpu(), chw(want[4].astype(np.float32))), k


# ------------------------------------------------------------------------------------------------ flip x offset x crop, both store forms
@pytest.mark.parametrize("h,w", [(37, 53), (36, 52)])               # rows of 212 bytes and of 208
@pytest.mark.parametrize("flow_dtype", [np.float32, np.float64])
def test_flip_offset_crop_matrix_is_bitwise_the_host_route(h, w, flow_dtype):
    samples = [make_sample(10 + i, h, w, 5, flow_dtype, special=(i == 1)) for i in range(3)]
    for crop in ((16, 24), (16, 21), (h, w)):                       # 16-byte stores, dword stores, the whole frame
        offsets = [(0, 0)] if crop == (h, w) else list(itertools.product((0, 5), (0, 1, 3)))
        plans = [AugPlan(h, w, crop=crop, y0=y0, x0=x0, hflip=hf, vflip=vf)
                 for (y0, x0), hf, vf in itertools.product(offsets, (False, True), (False, True))]
        for i0 in range(0, len(plans), 16):
            group = plans[i0:i0 + 16]
            used = [samples[(i0 + j) % 3] for j in range(len(group))]
            got = device_route(group, used)
            assert_same(got, stacked_host(group, used), f"{h}x{w} crop {crop} plans {i0}..", equal_nan=True)


# ------------------------------------------------------------------------------------------------ rescaling
def border_plans(h, w, crop):
    """Hand-made rescaling plans whose crop touches each of the four borders of the resized image, with and without the mirrors."""
    plans = []
    for (sx, sy), (hf, vf) in itertools.product(((1.3, 0.8), (0.71, 1.45), (2.0, 2.0)), ((False, False), (True, True))):
        rh, rw = int(round(h * sy)), int(round(w * sx))
        for y0, x0 in ((0, 2), (rh - crop[0], 1), (3, 0), (2, rw - crop[1])):          # top, bottom, left, right
            plans.append(AugPlan(rh, rw, crop=crop, y0=y0, x0=x0, hflip=hf, vflip=vf, resized=True, scale_x=np.float64(sx),
                                 scale_y=np.float64(sy)))
    return plans


@pytest.mark.parametrize("crop", [(16, 24), (16, 21)])
@pytest.mark.parametrize("flow_dtype", [np.float32, np.float64])
def test_rescaling_is_bitwise_the_host_route(crop, flow_dtype):
    """Every step of the resize is a correctly rounded fp64 operation in the host's order, so the comparison is on bits: a difference
    names its first element (a changed order of operations or a contraction shows there)."""
    h, w = 37, 53
    plans = []
    for seed in range(20):                                           # the seeded plans of tests/test_augment_host.py
        np.random.seed(seed)
        plans.append(FlowAugmentor(crop_size=list(crop), do_flip=True).draw(h, w))
    plans += border_plans(h, w, crop)
    # scale_x = 1 samples the source columns themselves (tx = 0): the left neighbour of an infinity blends inf * 0, a NaN on both routes
    plans.append(AugPlan(int(round(h * 1.3)), w, crop=crop, resized=True, scale_x=np.float64(1.0), scale_y=np.float64(1.3)))
    assert any(p.resized for p in plans[:20]) and any(not p.resized for p in plans[:20])
    samples = [make_sample(30 + i, h, w, 5, flow_dtype, special=(i != 0)) for i in range(3)]
    samples[(len(plans) - 1) % 3][2][16, 5] = 1.0                    # the last plan's sample: no NaN of its own
    seen = set()
    for i0 in range(0, len(plans), 16):                              # resized and un-resized samples share launches
        group = plans[i0:i0 + 16]
        used = [samples[(i0 + j) % 3] for j in range(len(group))]
        got = device_route(group, used)
        want = stacked_host(group, used)
        assert_same(got, want, f"crop {crop} plans {i0}..", equal_nan=True)
        assert torch.equal(torch.isnan(got[2]).cpu(), torch.isnan(want[2]))
        seen |= {("valid", v) for v in want[3].unique().tolist()}
    assert bool(torch.isnan(want[2][-1]).any())                      # inf * 0 in the last plan's interpolation
    assert seen == {("valid", 0.0), ("valid", 1.0)}


# ------------------------------------------------------------------------------------------------ batching, out=, errors
def test_batched_calls_equal_single_calls_and_fill_out_slices():
    h, w, crop = 37, 53, (16, 24)
    plans = []
    for seed in range(20):
        np.random.seed(100 + seed)
        plans.append(FlowAugmentor(crop_size=list(crop), do_flip=True).draw(h, w))
    samples = [make_sample(50 + i, h, w, 5, np.float32, special=(i % 4 == 0)) for i in range(20)]
    singles = [device_route([p], [s]) for p, s in zip(plans, samples)]
    one_by_one = tuple(torch.cat([r[k] for r in singles]) for k in range(4))
    for n in (1, 3, 16):
        got = device_route(plans[:n], samples[:n])
        assert_same(got, tuple(t[:n] for t in one_by_one), f"n = {n}", equal_nan=True)
    batch = (torch.full((20, 5, *crop), -7.0, device=DEV), torch.full((20, 5, *crop), -7.0, device=DEV),
             torch.full((20, 2, *crop), -7.0, device=DEV), torch.full((20, *crop), -7.0, device=DEV))
    for i0, k in ((0, 16), (16, 4)):
        ret = device_route(plans[i0:i0 + k], samples[i0:i0 + k], out=tuple(t[i0:i0 + k] for t in batch))
        assert all(r.data_ptr() == t[i0:].data_ptr() for r, t in zip(ret, batch))
    assert_same(batch, one_by_one, "out= slices of a 20-sample batch", equal_nan=True)


def test_refused_calls_raise_and_launch_nothing():
    h, w, crop = 20, 30, (8, 12)
    vol = torch.randn(3, h, w, device=DEV)
    flow = torch.randn(2, h, w, device=DEV)
    plan = AugPlan(h, w, crop=crop)
    with pytest.raises(_lib.EEMFlowHipError, match="1..16 samples"):
        augment_many([plan] * 17, [vol] * 17, [vol] * 17, [flow] * 17)
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        augment_many([plan], [vol.cpu()], [vol], [flow])
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        augment_many([plan], [vol], [vol], [flow.cpu()])
    with pytest.raises(ValueError, match="contiguous"):
        augment_many([plan], [vol.permute(0, 2, 1).contiguous().permute(0, 2, 1)], [vol], [flow])
    with pytest.raises(ValueError, match="share one"):
        augment_many([plan, plan], [vol, vol[:, :-1].contiguous()], [vol, vol], None)
    with pytest.raises(ValueError, match="flows share"):
        augment_many([plan], [vol], [vol], [flow[:, :-1].contiguous()])
    with pytest.raises(ValueError, match="one crop size"):
        augment_many([plan, AugPlan(h, w, crop=(8, 16))], [vol, vol], [vol, vol], None)
    out = tuple(torch.full(s, -7.0, device=DEV) for s in ((1, 3, *crop), (1, 3, *crop), (1, 2, *crop), (1, *crop)))
    for bad in (AugPlan(h, w, crop=crop, y0=13), AugPlan(h, w, crop=crop, x0=19), AugPlan(h + 4, w, crop=crop, y0=14),
                AugPlan(16, 40, crop=crop, resized=True, scale_x=1.3, scale_y=0.8)):       # round(30 * 1.3) is 39
        with pytest.raises(_lib.EEMFlowHipError, match="leaves the|not resized|is not round"):
            augment_many([bad], [vol], [vol], [flow], out=out)
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in out)                # nothing was launched
    good = augment_many([plan], [vol], [vol], [flow], out=out)      # and the library still works
    assert torch.equal(good[0][0], vol[:, :8, :12]) and torch.equal(good[2][0], flow[:, :8, :12])


# ------------------------------------------------------------------------------------------------ datasets and loader
class SmallHREM(hrem.HREMEventFlow):
    image_width = 96
    image_height = 64


def hrem_tree(root, count):
    for i in range(count):
        d = os.path.join(root, "dataset/HREM/train/dt1/%06d" % i)
        os.makedirs(d)
        hrem.write_events_npz(os.path.join(d, "events1.npz"), hrem.synthetic_hrem_events(300 + i, 4000, 64, 96))
        hrem.write_events_npz(os.path.join(d, "events2.npz"), hrem.synthetic_hrem_events(400 + i, 4000, 64, 96))
        hrem.write_flo(os.path.join(d, "flow.flo"), hrem.synthetic_flow(500 + i, 64, 96))


def mvsec_tree(root, seq, frames, flow_dtype):
    """Synthetic MVSEC tree as tests/test_gpu_data_rows.py builds it; the flows carry an infinity and an exact (0, 0) patch."""
    ev_dir = os.path.join(root, "dataset/MVSEC", seq, "event")
    fl_dir = os.path.join(root, "dataset/MVSEC", seq, "flowgt_dt1")
    os.makedirs(ev_dir)
    os.makedirs(fl_dir)
    for f in range(frames[0] + 1, frames[1] + 3):
        ev = hrem.synthetic_hrem_events(100 + f, 3000 + 10 * f, 260, 346, t_span=0.02)
        ev = ev[np.argsort(ev[:, 0], kind="stable")]
        ev[:, 0] += 0.02 * f
        np.savez(os.path.join(ev_dir, "%06d.npz" % f), ts=ev[:, 0], x=ev[:, 1], y=ev[:, 2], p=ev[:, 3])
    for i in range(*frames):
        fl = hrem.synthetic_flow(200 + i, 260, 346).astype(flow_dtype)
        fl[100:140, 150:200] = 0.0
        fl[30, 40, 0] = np.inf
        np.save(os.path.join(fl_dir, "%d.npy" % i), fl)


def stacked(samples):
    """ThreadedBatchLoader's (and DataLoader's) collation of per-sample dicts."""
    return {k: (torch.stack([s[k] for s in samples]) if torch.is_tensor(samples[0][k]) else [s[k] for s in samples]) for k in samples[0]}


def assert_same_batch(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        if torch.is_tensor(w):
            assert got[k].is_cuda and got[k].dtype == w.dtype, (what, k, got[k].dtype, w.dtype)
            diff = first_difference(got[k], w, equal_nan=True)
            assert diff is None, f"{what}: {k}: {diff}"
        else:
            assert got[k] == w, (what, k)


def test_hrem_get_batch_equals_the_stacked_host_samples(tmp_path):
    root = str(tmp_path)
    hrem_tree(root, 5)
    args = {"eval_type": "dense", "event_interval": "dt1", "num_voxel_bins": 5, "aug_params": {"crop_size": [64, 96], "do_flip": True}}
    ds = SmallHREM(args, train=True, root=root, device=DEV)
    idxs = [3, 0, 4, 1, 2] * 4                                       # 20 samples: a group of 16 and one of 4
    np.random.seed(11)
    plans = ds.draw_plans(idxs)
    assert {p.hflip for p in plans} == {True, False} and {p.vflip for p in plans} == {True, False}
    np.random.seed(11)
    want = stacked([ds[i] for i in idxs])
    state = np.random.get_state()
    np.random.seed(11)
    got = ds.get_batch(idxs)
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
    assert_same_batch(got, want, "HREM")
    assert tuple(got["event_volume_old"].shape) == (20, 5, 64, 96) and tuple(got["flow"].shape) == (20, 2, 16, 16)
    assert bool((got["valid"] == 1).all()) and got["names"] == ["%06d" % i for i in idxs]
    assert_same_batch(ds.get_batch(idxs, plans=plans), want, "HREM, plans given")
    # the training loop's `.to(dev).float()` on such a batch returns the tensor itself: no copy
    t = got["event_volume_old"]
    assert t.to(torch.device(DEV)).float().data_ptr() == t.data_ptr()
    with pytest.raises(ValueError, match="training datasets only"):
        os.makedirs(os.path.join(root, "dataset/HREM/test/dt1/seqA"))
        SmallHREM(args, train=False, root=root, device=DEV).get_batch([0])
    with pytest.raises(ValueError, match="host route"):
        SmallHREM(args, train=True, root=root, device=DEV, augmentor=lambda a, b, f, without_resize=False: (a, b, f)).get_batch([0])


@pytest.mark.parametrize("route", ["aug_params", "rescaling", "none"])
def test_mvsec_get_batch_equals_the_stacked_host_samples(tmp_path, route):
    root, frames = str(tmp_path), (10, 14)
    mvsec_tree(root, "indoor_flying2", frames, np.float64 if route == "rescaling" else np.float32)
    args = {"eval_type": "sparse", "num_voxel_bins": 5, "sequence": "indoor_flying2"}
    kw = dict(train=True, root=root, device=DEV, valid_time_index={"indoor_flying2": [frames]})
    if route == "aug_params":
        ds = mvsec.MvsecEventFlow(dict(args, aug_params={"crop_size": [256, 256], "do_flip": True}), **kw)
    elif route == "rescaling":
        ds = mvsec.MvsecEventFlow(args, augmentor=FlowAugmentor(crop_size=[192, 256], do_flip=True), **kw)
    else:
        ds = mvsec.MvsecEventFlow(args, **kw)
    idxs = [2, 0, 3, 1]
    seed = 7                                                         # flips of both kinds; resized and un-resized samples
    if route != "none":
        np.random.seed(seed)
        plans = ds.draw_plans(idxs)
        assert any(p.hflip for p in plans) and (route != "rescaling" or any(p.resized for p in plans))
    np.random.seed(seed)
    want = stacked([ds[i] for i in idxs])
    np.random.seed(seed)
    got = ds.get_batch(idxs)
    assert_same_batch(got, want, route)
    assert bool((got["valid"] == 0).any()) and bool((got["valid"] == 1).any())
    if route == "aug_params":
        assert got["d_event_volume_old"] is got["event_volume_old"] and tuple(got["flow"].shape) == (4, 2, 256, 256)
    with pytest.raises(ValueError, match="host route"):
        mvsec.MvsecEventFlow(args, augmentor=lambda a, b, f: (a, b, f), **kw).get_batch([0])
    with pytest.raises(ValueError, match="training datasets only"):
        mvsec.MvsecEventFlow(args, **dict(kw, train=False)).get_batch([0])


def test_trainer_steps_fed_by_the_device_loader_equal_the_host_loader(tmp_path):
    """Two EEMFlowTrainer.step calls fed by each loader under one seed: bitwise the same batches, identical losses.
    The learning rate is 0 on purpose.  The backward's weight and bias gradients meet in fp32 atomics whose order changes from run to
    run (oracle/fp64_bounds.py: "the backward is NOT bitwise repeatable"), so after a non-zero update the weights - and every later
    loss - differ in the last bits between ANY two runs, whatever feeds them: with lr = 1e-4 and bitwise identical batches this test
    measured losses [2.0667624120279147, 2.24210125985801] (host loader) against [2.0667624120279147, 2.2421012593384146] (device
    loader), the first step's equal, the second's 2e-10 apart - and three runs of one trainer on the very same resident tensors gave
    second-step losses 1.3110099874357601, 1.311009985525328, 1.3110099878350394 after an identical first.  With lr = 0 both steps still run whole (forward, backward, optimizer
    launch, statistics) and each loss is a function of its batch alone, which is what the loaders are compared on."""
    from eemflow_amd import EEMFlow
    from eemflow_amd.train import EEMFlowTrainer
    from eemflow_amd.weights import seeded_state_dict
    root, frames = str(tmp_path), (10, 14)
    mvsec_tree(root, "indoor_flying2", frames, np.float32)
    args = {"eval_type": "sparse", "num_voxel_bins": 5, "sequence": "indoor_flying2", "aug_params": {"crop_size": [256, 256], "do_flip": True}}
    ds = mvsec.MvsecEventFlow(args, train=True, root=root, device=DEV, valid_time_index={"indoor_flying2": [frames]})
    dev = torch.device(DEV)
    losses, batches = {}, {}
    for device_batches in (False, True):
        net = EEMFlow("", 5, 5)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(3).items()})
        net = net.to(dev).train()
        net.change_imagesize((256, 256))
        tr = EEMFlowTrainer(net, lr=0.0, num_steps=100)
        loader = ThreadedBatchLoader(ds, 2, shuffle=False, threads=1, drop_last=True, device_batches=device_batches)
        np.random.seed(7)
        losses[device_batches], batches[device_batches] = [], []
        for batch in loader:                                         # two batches of two: two steps
            e1, e2 = batch['event_volume_old'].to(dev).float(), batch['event_volume_new'].to(dev).float()
            loss, _, _ = tr.step(e1, e2, batch['flow'].to(dev).float(), batch['valid'].to(dev).float())
            losses[device_batches].append(loss)
            batches[device_batches].append(batch)
        loader.close()
    assert len(losses[True]) == 2
    for got, want in zip(batches[True], batches[False]):
        assert_same_batch(got, want, "loader batch")
    print("losses: host loader", losses[False], "device loader", losses[True])
    assert losses[True] == losses[False] and losses[True][0] != losses[True][1] and all(np.isfinite(losses[True]))
