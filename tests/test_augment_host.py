"""Augmentation plans separated from pixels (eemflow_amd/augmentor.py: draw / apply_host), the declaration of the GPU form and the
device-batch route of the threaded loader.  CPU only."""
import os
import re

import numpy as np
import pytest

from eemflow_amd import augmentor as A
from eemflow_amd.augmentor import DenseSparseAugmentor, FlowAugmentor, apply_host
from eemflow_amd.loader import ThreadedBatchLoader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def golden_inputs(seed, h, w):
    """The inputs tests/golden/augmentor.npz was made from (tests/test_data_rows.py)."""
    rng = np.random.default_rng(100 + seed)
    a, b, da, db = (rng.standard_normal((h, w, 3)).astype(np.float32) for _ in range(4))
    return a, b, da, db, rng.standard_normal((h, w, 2))


def test_draw_and_apply_host_reproduce_the_reference_outputs(golden):
    g = golden("augmentor.npz")
    for k, (seed, h, w, ch, cw, flip) in enumerate(g["cases"].tolist()):
        a, b, da, db, fl = golden_inputs(seed, h, w)
        aug = FlowAugmentor(crop_size=[ch, cw], do_flip=bool(flip))
        np.random.seed(seed)
        aug(a, b, fl, without_resize=True)
        after_call = np.random.get_state()
        np.random.seed(seed)
        plan = aug.draw(h, w, without_resize=True)
        assert same_state(np.random.get_state(), after_call), k
        for i, arr in enumerate(apply_host(plan, a, b, fl)):
            want = g[f"flow_nr_{k}_{i}"]
            assert arr.flags["C_CONTIGUOUS"] and arr.dtype == want.dtype and np.array_equal(arr, want), (k, i)
        aug = DenseSparseAugmentor(crop_size=[ch, cw], do_flip=bool(flip))
        np.random.seed(seed)
        aug(a, b, da, db, fl)
        after_call = np.random.get_state()
        np.random.seed(seed)
        plan = aug.draw(h, w)
        assert same_state(np.random.get_state(), after_call), k
        assert plan.crop == (ch, cw) and not plan.resized
        for i, arr in enumerate(apply_host(plan, a, b, da, db, fl)):
            want = g[f"dense_{k}_{i}"]
            assert arr.flags["C_CONTIGUOUS"] and arr.dtype == want.dtype and np.array_equal(arr, want), (k, i)


def reads_clamped_neighbour(plan, h, w):
    """Whether some row or column of the crop blends a neighbour clamped to the source's border - which only the first and last rows and
    columns of the resized image can (randint's exclusive bound keeps an un-mirrored crop off the last ones: a mirror brings them in)."""
    if not plan.resized:
        return False

    def clamped(d, f, n):
        i0 = int(np.floor((d + 0.5) / float(f) - 0.5))
        return i0 < 0 or i0 + 1 > n - 1
    ch, cw = plan.crop
    rows = [plan.RH - 1 - (plan.y0 + r) if plan.vflip else plan.y0 + r for r in range(ch)]
    cols = [plan.RW - 1 - (plan.x0 + c) if plan.hflip else plan.x0 + c for c in range(cw)]
    return any(clamped(r, plan.scale_y, h) for r in rows) or any(clamped(c, plan.scale_x, w) for c in cols)


RESCALE_CASES = ((120, 160, (64, 96)), (37, 53, (16, 24)))


def rescale_inputs(seed, h, w):
    rng = np.random.default_rng(seed)
    a, b = (rng.standard_normal((h, w, 3)).astype(np.float32) for _ in range(2))
    fl = rng.standard_normal((h, w, 2))
    return a, b, fl.astype(np.float32) if seed % 2 else fl         # both flow types the datasets hold


def test_rescaling_flow_augmentor_draw_and_apply_host_equal_call():
    seen = {"resized": set(), "hflip": set(), "vflip": set(), "stretch": False, "clamped": False}
    for h, w, crop in RESCALE_CASES:
        for seed in range(20):
            a, b, fl = rescale_inputs(seed, h, w)
            aug = FlowAugmentor(crop_size=list(crop), do_flip=True)
            np.random.seed(seed)
            want = aug(a, b, fl)
            after_call = np.random.get_state()
            np.random.seed(seed)
            plan = aug.draw(h, w)
            assert same_state(np.random.get_state(), after_call), (h, seed)
            got = apply_host(plan, a, b, fl)
            for i, (x, y) in enumerate(zip(got, want)):
                assert x.dtype == y.dtype and x.shape == y.shape and x.flags["C_CONTIGUOUS"], (h, seed, i)
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (h, seed, i)          # bitwise
            assert plan.crop == crop and 0 <= plan.y0 <= plan.RH - crop[0] and 0 <= plan.x0 <= plan.RW - crop[1]
            seen["resized"].add(plan.resized)
            seen["hflip"].add(plan.hflip)
            seen["vflip"].add(plan.vflip)
            seen["stretch"] |= plan.resized and float(plan.scale_x) != float(plan.scale_y)
            seen["clamped"] |= reads_clamped_neighbour(plan, h, w)
    assert seen["resized"] == {True, False} and seen["hflip"] == {True, False} and seen["vflip"] == {True, False}, seen
    assert seen["stretch"] and seen["clamped"], seen


def test_header_declares_the_gpu_form():
    header = open(os.path.join(REPO, "include", "eemflow_hip.h")).read()
    at = header.index("int eemflow_augment_many(")
    block = header[header.rindex("\n\n", 0, at):at]               # the declaration's own paragraph: comment, limit, plan struct
    assert block.lstrip().startswith("/*") and "Replaces:" in block and "utils/augumentor.py:158-257,389-419" in block
    assert "loader/HREM.py:252" in block and "loader/MVSEC.py:170-187" in block
    limit = re.search(r"#define EEMFLOW_AUGMENT_MAX (\d+)", block)
    assert limit and int(limit.group(1)) == A.AUGMENT_MAX == 16
    from eemflow_amd import _lib
    assert "eemflow_augment_many" in _lib.EXPORTS
    import eemflow_amd
    assert eemflow_amd.augment_many is A.augment_many


class FakeDataset:
    """In-memory dataset with the device-batch protocol: plans are numbers drawn from numpy.random, get_batch records its calls."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        raise AssertionError("the device route builds whole batches")

    def draw_plans(self, idxs):
        return [float(np.random.rand()) for _ in idxs]

    def read_sample(self, i):
        return ("read", i)

    def get_batch(self, idxs, plans=None, reads=None):
        assert reads == [("read", i) for i in idxs]
        self.calls.append((list(idxs), list(plans)))
        return {"idx": list(idxs), "plans": list(plans)}


@pytest.mark.parametrize("drop_last", [True, False])
def test_device_batches_draw_plans_in_sampler_order_for_any_thread_count(drop_last):
    runs = {}
    for threads in (1, 4):
        ds = FakeDataset(11)
        loader = ThreadedBatchLoader(ds, 4, shuffle=True, threads=threads, drop_last=drop_last, seed=5, device_batches=True)
        assert len(loader) == (2 if drop_last else 3)
        assert len(loader) == len(ThreadedBatchLoader(ds, 4, shuffle=True, threads=threads, drop_last=drop_last, seed=5))
        np.random.seed(123)
        batches = list(loader)
        loader.close()
        assert len(batches) == len(loader)
        order = loader_order = [i for b in batches for i in b["idx"]]
        assert [len(b["idx"]) for b in batches] == ([4, 4] if drop_last else [4, 4, 3])
        np.random.seed(123)
        want = [float(np.random.rand()) for _ in order]            # drawn in the order the sampler gave the samples out
        assert [p for b in batches for p in b["plans"]] == want
        assert sorted(map(tuple, (c[0] for c in ds.calls))) == sorted(tuple(b["idx"]) for b in batches)
        runs[threads] = (loader_order, want)
    assert runs[1] == runs[4]


def test_device_batches_need_a_dataset_with_get_batch():
    class Plain:
        def __len__(self):
            return 4

        def __getitem__(self, i):
            return {"x": i}
    with pytest.raises(ValueError, match="get_batch"):
        ThreadedBatchLoader(Plain(), 2, device_batches=True)
    assert len(ThreadedBatchLoader(Plain(), 2)) == 2


def test_an_abandoned_device_epoch_leaves_nothing_queued():
    ds = FakeDataset(40)
    loader = ThreadedBatchLoader(ds, 4, threads=1, device_batches=True)
    np.random.seed(1)
    it = iter(loader)
    first = next(it)
    it.close()                                                     # the training loop's `break`
    loader.close()
    assert first["idx"] == [0, 1, 2, 3] and len(ds.calls) <= 1 + loader.ahead + 1


def test_argument_errors_are_reported_before_any_launch():
    """Every refused call returns the argument error code with its reason in eemflow_last_error, before the device is touched (the
    pointers here are not device addresses)."""
    import ctypes

    import torch

    from eemflow_amd import _lib
    lib = _lib.lib()
    arr = (ctypes.c_void_p * 17)(*([0x1000] * 17))
    C, H, W = 3, 20, 30

    def call(n, plans, old=arr, new=arr, out_old=0x1000, out_new=0x1000, flow=None, out_flow=None, ch=8, cw=12):
        table = (_lib.AugPlanC * len(plans))(*[_lib.AugPlanC(*p) for p in plans])
        rc = lib.eemflow_augment_many(n, old, new, flow, 0, table, C, H, W, ch, cw, out_old, out_new, out_flow, None, None)
        return rc, lib.eemflow_last_error().decode()
    ok = (1.0, 1.0, 0, H, W, 0, 0, 0, 0, 0)
    for n in (0, 17):
        rc, msg = call(n, [ok] * 17)
        assert rc == 1 and "1..16 samples" in msg, msg
    rc, msg = call(1, [ok], old=None)
    assert rc == 1 and "NULL" in msg, msg
    rc, msg = call(1, [ok], out_new=None)
    assert rc == 1 and "NULL" in msg, msg
    rc, msg = call(2, [ok, ok], old=(ctypes.c_void_p * 2)(0x1000, None))
    assert rc == 1 and "sample 1 has a NULL volume" in msg, msg
    rc, msg = call(1, [ok], flow=arr)                              # a flow without its destinations
    assert rc == 1 and "out_flow" in msg, msg
    for y0, x0 in ((13, 0), (0, 19), (-1, 0), (0, -1)):            # 8x12 at (12, 18) is the last crop inside 20x30
        rc, msg = call(1, [(1.0, 1.0, 0, H, W, 0, 0, y0, x0, 0)])
        assert rc == 1 and "leaves the 20x30 image" in msg, msg
    rc, msg = call(1, [(1.0, 1.0, 0, H + 1, W, 0, 0, 0, 0, 0)])    # not resized, yet another size
    assert rc == 1 and "not resized" in msg, msg
    rc, msg = call(1, [(1.3, 0.8, 1, 16, 40, 0, 0, 0, 0, 0)])      # round(30 * 1.3) is 39
    assert rc == 1 and "is not round" in msg, msg
    rc, msg = call(1, [(1.3, 0.8, 1, 16, 39, 0, 0, 9, 0, 0)])      # the crop is checked against the RESIZED image
    assert rc == 1 and "leaves the 16x39 image" in msg, msg
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        v = torch.zeros(C, H, W)
        A.augment_many([A.AugPlan(H, W)], [v], [v])
