"""Event preparation on the GPU (eemflow_pack_events_many through eemflow_amd.events.pack_events_many) against the host route bit for
bit: the kernel on its own, batching and the argument errors, the HREM dataset with device_events=True against device_events=False,
and the loader's device batches.  `pytest -m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from eemflow_amd import _lib, events as E, hrem
from eemflow_amd.loader import ThreadedBatchLoader

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
BASES = (0, 123456789, 1700000000000000123)                         # the last one is above 2^53: int64 -> double rounds
SIZES = (1, 2, 63, 64, 65, 257, 4099)                               # one event, wave and block edges, odd tails
CANARY = -12345.678


# ------------------------------------------------------------------------------------------------ helpers
def hrem_columns(seed, n, base, p_dtype):
    """What read_event_columns returns for a sorted HREM file: t int64 [ns] with ties, x and y uint16, p = 2*p - 1 in p's own dtype."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, 50_000_000, n)).astype(np.int64) + base
    if n >= 8:
        t[n // 2:n // 2 + 3] = t[n // 2]
        t[1] = t[0]
    p = rng.integers(0, 2, n).astype(p_dtype)
    return t, rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16), 2 * p - 1


def mvsec_columns(seed, n):
    """An MVSEC-like set: four float64 columns, absolute timestamps in seconds, p in {-1, +1}."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 0.02, n)) + 1504645177.4
    return t, rng.integers(0, W, n).astype(np.float64), rng.integers(0, H, n).astype(np.float64), (rng.integers(0, 2, n) * 2 - 1).astype(np.float64)


def guarded(n):
    """An (n,4) float64 output with four more doubles behind it, the whole buffer holding the canary."""
    buf = torch.full((n * 4 + 4,), CANARY, dtype=torch.float64, device=DEV)
    return buf, buf[:n * 4].view(n, 4)


def assert_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    bad = got.view(np.int64) != want.view(np.int64)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {tuple(np.argwhere(bad)[0])}: got " \
                          f"{got[tuple(np.argwhere(bad)[0])].hex()}, want {want[tuple(np.argwhere(bad)[0])].hex()}"


def check_set(cols, what, **scales):
    assert E.route_of(cols) == 'device', what
    want = E.host_events(cols, **scales)
    n = cols[0].shape[0]
    buf, out = guarded(n)
    before = dict(E.route_counts)
    res = E.pack_events_many([cols], device=DEV, out=[out], **scales)
    assert res[0] is out and E.route_counts['device'] == before['device'] + 1 and E.route_counts['host'] == before['host']
    assert_bits(out, want, what)
    assert bool((buf[n * 4:] == CANARY).all()), f"{what}: the doubles behind the output were written"


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n", SIZES)
def test_pack_equals_the_host_route_bitwise(n):
    for base in BASES:
        for p_dtype in (np.int8, np.uint8, np.bool_):
            check_set(hrem_columns(n, n, base, p_dtype), f"n={n} base={base} p={np.dtype(p_dtype).name}")
    check_set(mvsec_columns(n, n), f"n={n} float64 columns", scale_a=1.0, scale_b=1.0, relative=True)
    check_set(mvsec_columns(n + 1, n), f"n={n} float64 columns, absolute", scale_a=1.0, scale_b=1.0, relative=False)


def test_every_dtype_code_converts_as_astype_float64():
    n = 1031
    rng = np.random.default_rng(9)
    for dt in (np.uint8, np.int8, np.uint16, np.int16, np.int32, np.int64, np.float32, np.float64):
        info = np.iinfo(dt) if np.dtype(dt).kind in "iu" else None
        if info is not None:
            v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
            v[:2] = (info.min, info.max)
        else:
            v = (rng.normal(0, 1e3, n)).astype(dt)
        t = np.sort(rng.integers(0, 2 ** 40, n)).astype(np.int64)
        check_set((t, v, v[::-1].copy(), v), np.dtype(dt).name)
    tv = np.sort(rng.integers(-2 ** 31, 2 ** 31 - 1, n)).astype(np.int32)          # a narrow, signed t column
    check_set((tv, np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.ones(n, np.int8)), "int32 t")


# ------------------------------------------------------------------------------------------------ batching
def mixed_sets(count):
    sets = []
    for k in range(count):
        n = (1, 64, 65, 257, 1000, 2049, 4099, 63)[k % 8] + k
        if k % 4 == 3:
            sets.append(mvsec_columns(50 + k, n))
        else:
            sets.append(hrem_columns(50 + k, n, BASES[k % 3], (np.int8, np.uint8, np.bool_)[k % 3]))
    return sets


def test_32_sets_in_one_call_equal_32_single_calls():
    sets = mixed_sets(32)
    singles = [E.pack_events_many([cols], 1e-9, 1e6, True, device=DEV)[0] for cols in sets]
    bufs = [guarded(cols[0].shape[0]) for cols in sets]
    before = dict(E.route_counts)
    many = E.pack_events_many(sets, 1e-9, 1e6, True, device=DEV, out=[o for _, o in bufs])
    assert E.route_counts['device'] == before['device'] + 32
    for k, (one, got, (buf, _)) in enumerate(zip(singles, many, bufs)):
        assert torch.equal(one.view(torch.int64), got.view(torch.int64)), k
        assert_bits(got, E.host_events(sets[k]), f"set {k}")
        assert bool((buf[got.numel():] == CANARY).all()), k
    # more than 32 sets: the Python front-end splits them into calls of 32
    more = E.pack_events_many(sets + sets[:3], device=DEV)
    assert len(more) == 35 and all(torch.equal(a, b) for a, b in zip(more, singles + singles[:3]))


def c_call(nsets, ptrs, codes, counts, outs):
    """eemflow_pack_events_many with one device column (of `codes[k]`) standing for all four columns of set k."""
    arr = ctypes.c_void_p * nsets
    col = arr(*ptrs)
    return _lib.lib().eemflow_pack_events_many(nsets, col, col, col, col, (ctypes.c_int * (4 * nsets))(*[c for c in codes for _ in range(4)]),
                                               (ctypes.c_int64 * nsets)(*counts), 1e-9, 1e6, 1, arr(*outs), _lib.current_stream_ptr(torch.device(DEV)))


def test_argument_errors_come_before_any_launch_and_empty_jobs_write_nothing():
    n = 100
    src = torch.arange(n, dtype=torch.float64, device=DEV)
    bufs = [torch.full((n * 4 + 4,), CANARY, dtype=torch.float64, device=DEV) for _ in range(33)]
    with torch.cuda.device(DEV):
        assert c_call(33, [src.data_ptr()] * 33, [7] * 33, [n] * 33, [b.data_ptr() for b in bufs]) != 0           # 33 sets
        assert b"1..32" in _lib.lib().eemflow_last_error()
        assert c_call(0, [], [], [], []) != 0
        assert c_call(2, [src.data_ptr()] * 2, [7, 8], [n, n], [b.data_ptr() for b in bufs[:2]]) != 0             # an unknown code
        assert b"unknown dtype code" in _lib.lib().eemflow_last_error()
        assert c_call(2, [src.data_ptr()] * 2, [7, -1], [n, 0], [b.data_ptr() for b in bufs[:2]]) != 0            # also on an empty set
        assert c_call(1, [src.data_ptr() + 4], [7], [n - 1], [bufs[0].data_ptr()]) != 0                           # misaligned column
        assert c_call(1, [src.data_ptr()], [7], [n], [bufs[0].data_ptr() + 8]) != 0                               # misaligned output
        torch.cuda.synchronize()
        assert all(bool((b == CANARY).all()) for b in bufs)                                                       # nothing was launched
        # n = 0 jobs (NULL columns allowed) beside a real one: only the real one's rows are written
        assert c_call(3, [None, src.data_ptr(), None], [7, 7, 2], [0, n, 0], [bufs[0].data_ptr(), bufs[1].data_ptr(), None]) == 0
        assert c_call(1, [None], [5], [0], [bufs[2].data_ptr()]) == 0                                             # a call of empty jobs only
        torch.cuda.synchronize()
    assert bool((bufs[0] == CANARY).all()) and bool((bufs[2] == CANARY).all()) and bool((bufs[1][n * 4:] == CANARY).all())
    v = np.arange(n, dtype=np.float64)
    tt = (v * 1e-9) * 1e6
    assert_bits(bufs[1][:n * 4].view(n, 4), np.stack([tt - tt[0], v, v, v], axis=1), "the real job")
    with pytest.raises(ValueError, match="out must be"):
        E.pack_events_many([hrem_columns(1, 10, 0, np.int8)], device=DEV, out=[torch.empty(11, 4, dtype=torch.float64, device=DEV)])


def test_unsorted_and_sorted_sets_of_one_call_take_their_routes():
    a, b = hrem_columns(70, 500, BASES[1], np.int8), hrem_columns(71, 300, BASES[2], np.uint8)
    t = b[0].copy()
    t[[10, 200]] = t[[200, 10]]
    b = (t,) + b[1:]
    counts = {'device': 0, 'host': 0}
    got = E.pack_events_many([a, b], device=DEV, counts=counts)
    assert counts == {'device': 1, 'host': 1}
    assert_bits(got[0], E.host_events(a), "sorted")
    assert_bits(got[1], E.host_events(b), "unsorted")


# ------------------------------------------------------------------------------------------------ the HREM dataset and the loader
class SmallHREM(hrem.HREMEventFlow):
    image_width = W
    image_height = H


ARGS = {"eval_type": "dense", "event_interval": "dt1", "num_voxel_bins": 5, "aug_params": {"crop_size": [H, W], "do_flip": True}}


def hrem_tree(root, counts, unsorted=()):
    """One training sample per entry of `counts`, with that many events per file, sorted by time except the samples listed in
    `unsorted` (their events1.npz stays as synthetic_hrem_events draws it)."""
    for i, n in enumerate(counts):
        d = os.path.join(root, "dataset/HREM/train/dt1/%06d" % i)
        os.makedirs(d)
        for name, seed in (("events1.npz", 300 + i), ("events2.npz", 400 + i)):
            ev = hrem.synthetic_hrem_events(seed, n, H, W)
            if not (i in unsorted and name == "events1.npz"):
                ev = ev[np.argsort(ev[:, 0], kind="stable")]
            hrem.write_events_npz(os.path.join(d, name), ev)
        hrem.write_flo(os.path.join(d, "flow.flo"), hrem.synthetic_flow(500 + i, H, W))


def assert_same_sample(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.device == w.device and torch.equal(g, w), (what, k)
        elif isinstance(w, (list, tuple)) and w and torch.is_tensor(w[0]):
            assert len(g) == len(w) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(g, w)), (what, k)
        else:
            assert g == w, (what, k)


@pytest.mark.parametrize("with_events", [False, True])
def test_hrem_dataset_with_device_events_equals_the_host_route(tmp_path, with_events):
    root = str(tmp_path)
    hrem_tree(root, [4000] * 5)
    host = SmallHREM(ARGS, train=True, root=root, device=DEV, with_events=with_events)
    dev = SmallHREM(ARGS, train=True, root=root, device=DEV, with_events=with_events, device_events=True)
    assert host.device_events is False and host.event_routes == {'device': 0, 'host': 0}
    for i in range(5):
        np.random.seed(20 + i)
        want = host[i]
        np.random.seed(20 + i)
        assert_same_sample(dev[i], want, f"ds[{i}]")
    assert dev.event_routes == {'device': 10, 'host': 0}
    idxs = [3, 0, 4, 1, 2]
    np.random.seed(5)
    want = host.get_samples(idxs)
    np.random.seed(5)
    for k, (g, w) in enumerate(zip(dev.get_samples(idxs), want)):
        assert_same_sample(g, w, f"get_samples[{k}]")
    np.random.seed(11)
    plans = host.draw_plans(idxs)
    assert {p.hflip for p in plans} == {True, False} and {p.vflip for p in plans} == {True, False}
    np.random.seed(11)
    want = host.get_batch(idxs)
    np.random.seed(11)
    assert_same_sample(dev.get_batch(idxs), want, "get_batch")
    assert dev.event_routes == {'device': 30, 'host': 0} and host.event_routes == {'device': 0, 'host': 0}
    if with_events:
        ev = dev.read_sample(2)[0]['events']
        assert ev.is_cuda and ev.dtype == torch.float64 and tuple(ev.shape) == (4000, 4)
        assert_bits(ev, E.host_events(E.read_event_columns(os.path.join(root, "dataset/HREM/train/dt1/000002/events1.npz"))), "events")


def test_an_unsorted_file_keeps_the_host_route(tmp_path):
    root = str(tmp_path)
    hrem_tree(root, [4000] * 3, unsorted=(1,))
    host = SmallHREM(ARGS, train=True, root=root, device=DEV, with_events=True)
    dev = SmallHREM(ARGS, train=True, root=root, device=DEV, with_events=True, device_events=True)
    for i in range(3):
        np.random.seed(30 + i)
        want = host[i]
        np.random.seed(30 + i)
        assert_same_sample(dev[i], want, f"ds[{i}]")
        assert dev.event_routes == {'device': 2 * (i + 1) - (1 if i >= 1 else 0), 'host': 1 if i >= 1 else 0}


def test_loader_device_batches_with_device_events_equal_the_host_route(tmp_path):
    """Two seeded epochs of ThreadedBatchLoader(device_batches=True, threads=3, batch_size=2) over files of 1000 .. 9000 events: the
    pool threads' staging buffers grow and are reused."""
    root = str(tmp_path)
    counts = [1000, 9000, 2000, 8000, 3000, 7000, 4000, 6000, 5000]
    hrem_tree(root, counts)
    batches = {}
    for device_events in (False, True):
        ds = SmallHREM(ARGS, train=True, root=root, device=DEV, with_events=True, device_events=device_events)
        loader = ThreadedBatchLoader(ds, 2, shuffle=True, threads=3, drop_last=True, seed=3, device_batches=True)
        np.random.seed(17)
        batches[device_events] = [b for _ in range(2) for b in loader]
        loader.close()
        torch.cuda.synchronize()
        assert ds.event_routes == ({'device': 2 * 2 * 8, 'host': 0} if device_events else {'device': 0, 'host': 0})
    assert len(batches[True]) == 8 and len({tuple(b['names']) for b in batches[True]}) > 4
    for k, (got, want) in enumerate(zip(batches[True], batches[False])):
        assert_same_sample(got, want, f"batch {k}")
