"""Windows of a device-resident recording voxelized straight from its raw columns (eemflow_voxelize_windows, csrc/voxel_cols.hip,
eemflow_amd/recording.py), harness.run_recording and `cli run`.  The oracle of every grid is the existing route on the same slice,
voxelize_many_device(pack_events_many([slice])) - itself pinned to the reference goldens and to exact sums - and equality is BITWISE:
the same votes, the same fp64 cell sums, one rounding.  `pytest -m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eemflow_amd
from eemflow_amd import _lib, cli, events as E, harness, hrem, recording as R
from eemflow_amd.iwe import fwl_many
from eemflow_amd.voxelizer import norm_record, voxelize_many_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = -12345.678
N = 20000
# a one-event window; two events of one timestamp (dT = 0 -> 1); a window from the odd element 3 that is longer than one slab (1024
# events); another one-event window; a window from the odd element 4101; the rest.  Timestamps tie across the edges 4100 / 4101 and 9000
OFFSETS = [0, 1, 3, 4100, 4101, 9000, N]
GRIDS = [(5, 33, 47), (5, 64, 96)]                                  # hw no multiple of 4: scalar read-out; 16-byte read-out
# hrem_u8 and hrem_i8 are HREM's own dtypes (vox_bin_cols_kernel<EPT, true>, both conversions of its one-byte p); the others take the
# generic instantiation behind pk_load's dtype switch
KINDS = ("hrem_u8", "hrem_i8", "bool_p", "f64_i32_i8", "i32_i16")


# ------------------------------------------------------------------------------------------------ helpers
def columns(kind, seed, n, h, w, stray=True):
    """(t, x, y, p) as read_event_columns would return them, in time order with ties, and the (scale_a, scale_b) that go with them.
    stray: a few events with x >= W or y >= H (the reference's flat index puts them into a neighbouring row or plane)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, w, n)
    y = rng.integers(0, h, n)
    if stray:
        x[rng.integers(0, n, 40)] = w + rng.integers(0, 5, 40)
        y[rng.integers(0, n, 40)] = h + rng.integers(0, 3, 40)
    ticks = np.sort(rng.integers(0, 50_000_000, n))
    for a in (1, 4099, 4100, 8999):                                 # t[1] == t[2], t[4099] == t[4100] == t[4101], t[8999] == t[9000]
        if a + 1 < n:
            ticks[a + 1] = ticks[a]
    pol = rng.integers(0, 2, n)
    if kind == "hrem_u8":                                           # the npz of HREM: above 2^53 ns, uint8 p with 2 * 0 - 1 = 255
        return (ticks.astype(np.int64) + 1700000000000000123, x.astype(np.uint16), y.astype(np.uint16), 2 * pol.astype(np.uint8) - 1), (1e-9, 1e6)
    if kind == "hrem_i8":                                           # an int8 p beside HREM's other dtypes
        return (ticks.astype(np.int64) + 1700000000000000123, x.astype(np.uint16), y.astype(np.uint16), (2 * pol - 1).astype(np.int8)), (1e-9, 1e6)
    if kind == "bool_p":                                            # a bool p: 2 * p - 1 is int64
        return (ticks.astype(np.int64) + 123456789, x.astype(np.uint16), y.astype(np.uint16), 2 * pol.astype(np.bool_) - 1), (1e-9, 1e6)
    if kind == "f64_i32_i8":
        return (ticks.astype(np.float64) * 1e-9 + 1504645177.4, x.astype(np.int32), y.astype(np.int32), (2 * pol - 1).astype(np.int8)), (1.0, 1e6)
    return (ticks.astype(np.int32), x.astype(np.int16), y.astype(np.int16), (2 * pol - 1).astype(np.int8)), (1e-9, 1e6)


def recording_of(cols, scales, h, w):
    return R.EventRecording(*cols, h, w, device=DEV, scale_a=scales[0], scale_b=scales[1])


def composition(cols, scales, offsets, bins, h, w, normalize, relative=True):
    """The oracle: per non-empty window pack_events_many of the host slice, then voxelize_many_device, 32 sets per call; None for an
    empty window (the existing route refuses one)."""
    spans = [(a, b) for a, b in zip(offsets, offsets[1:])]
    live = [i for i, (a, b) in enumerate(spans) if b > a]
    tables = E.pack_events_many([tuple(c[spans[i][0]:spans[i][1]] for c in cols) for i in live], scale_a=scales[0], scale_b=scales[1],
                                relative=relative, device=DEV)
    out = [None] * len(spans)
    for i0 in range(0, len(live), 32):
        for i, g in zip(live[i0:i0 + 32], voxelize_many_device(tables[i0:i0 + 32], bins, h, w, normalize)):
            out[i] = g
    return out


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def last_form():
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().eemflow_voxelize_last_form(buf, len(buf)))
    return buf.value.decode()


def assert_windows_equal(got, want, normalize, what):
    assert len(got) == len(want)
    for k, (g, r) in enumerate(zip(got, want)):
        assert g.shape == (1,) + tuple(r.shape) and g.dtype == torch.float32, (what, k)
        assert same(g[0], r), (what, k, float((g[0] - r).abs().max()))
        if normalize == "deferred":
            assert same(norm_record(g), norm_record(r)), (what, k, norm_record(g).tolist(), norm_record(r).tolist())


# ------------------------------------------------------------------------------------------------ 1. bitwise against the composition
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bins,h,w", GRIDS)
def test_windows_equal_the_composition_bitwise(bins, h, w, kind):
    cols, scales = columns(kind, 11, N, h, w)
    assert int((cols[1].astype(np.int64) >= w).sum()) > 0 and int((cols[2].astype(np.int64) >= h).sum()) > 0
    t = cols[0]
    assert t[1] == t[2] and t[4099] == t[4100] == t[4101] and t[8999] == t[9000]
    if kind == "hrem_u8":
        assert set(np.unique(cols[3])) == {1, 255}
    if kind == "bool_p":
        assert cols[3].dtype == np.int64
    rec = recording_of(cols, scales, h, w)
    assert rec.route == 'device' and rec.dtypes == tuple(c.dtype for c in cols)
    for normalize in (False, True, "deferred"):
        for relative in (False, True):
            got = R.voxelize_windows(rec, OFFSETS, bins, normalize=normalize, relative=relative)
            form = last_form()
            want = composition(cols, scales, OFFSETS, bins, h, w, normalize, relative)
            assert_windows_equal(got, want, normalize, (kind, normalize, relative))
            vec = "v4" if (h * w) % 4 == 0 else "v1"
            assert form.startswith(f"j6:colbin_e1+band") and f"_{vec}_" in form, form
            assert form.endswith({False: "_raw", True: "_raw_sums+norm", "deferred": "_raw_sums+stats"}[normalize]), form
    assert float(got[2].abs().max()) > 0.5 and float(got[0].abs().sum()) > 0.5


# ------------------------------------------------------------------------------------------------ 2. every EPT form
@pytest.mark.parametrize("kind", ["hrem_u8", "bool_p"])             # both instantiations of every EPT: HREM's dtypes and the generic one
@pytest.mark.parametrize("n,ept", [(600_000, 2), (512 * 2048 + 1, 4), (512 * 4096 + 1, 8)])
def test_large_windows_take_every_events_per_thread_form(n, ept, kind):
    bins, h, w = 5, 64, 96
    cols, scales = columns(kind, 12, n, h, w)
    rec = recording_of(cols, scales, h, w)
    got = R.voxelize_windows(rec, [0, n], bins, normalize="deferred")
    form = last_form()
    assert form.startswith(f"j1:colbin_e{ept}+band"), form
    assert_windows_equal(got, composition(cols, scales, [0, n], bins, h, w, "deferred"), "deferred", n)
    assert last_form().startswith(f"j1:bin_e{ept}+band")            # the oracle ran the table's kernel in the same form


# ------------------------------------------------------------------------------------------------ 3. more windows than a launch takes
def test_33_windows_in_one_call_equal_one_window_per_call():
    bins, h, w = 5, 33, 47
    cols, scales = columns("hrem_u8", 13, N, h, w)
    rec = recording_of(cols, scales, h, w)
    offsets = rec.window_offsets(count=600)                          # 33 full windows of 600 events
    assert len(offsets) == 34
    for normalize in (True, "deferred"):
        together = R.voxelize_windows(rec, offsets, bins, normalize=normalize)
        assert last_form().startswith("j1:colbin_e1")               # the second launch sequence held the 33rd window
        alone = [R.voxelize_windows(rec, offsets[k:k + 2], bins, normalize=normalize)[0] for k in range(33)]
        assert_windows_equal(together, [a[0] for a in alone], normalize, normalize)
    assert_windows_equal(together[30:], composition(cols, scales, offsets.tolist()[30:], bins, h, w, "deferred"), "deferred", "tail")


# ------------------------------------------------------------------------------------------------ 4. empty windows
@pytest.mark.parametrize("bins,h,w", GRIDS)
def test_an_empty_window_is_a_zero_grid_and_leaves_its_neighbours_alone(bins, h, w):
    cols, scales = columns("hrem_u8", 14, 5000, h, w)
    rec = recording_of(cols, scales, h, w)
    for normalize in (False, True, "deferred"):
        with_gap = R.voxelize_windows(rec, [7, 2001, 2001, 5000], bins, normalize=normalize)
        without = R.voxelize_windows(rec, [7, 2001, 5000], bins, normalize=normalize)
        assert_windows_equal([with_gap[0], with_gap[2]], [g[0] for g in without], normalize, normalize)
        assert torch.equal(bits(with_gap[1]), torch.zeros_like(bits(with_gap[1])))          # +0.0 everywhere
        if normalize == "deferred":
            assert norm_record(with_gap[1]).tolist() == [0.0, 1.0, 0.0, 0.0]
    only = R.voxelize_windows(rec, [5, 5], bins, normalize="deferred")                       # a call of nothing but an empty window
    assert torch.equal(bits(only[0]), torch.zeros_like(bits(only[0]))) and norm_record(only[0]).tolist() == [0.0, 1.0, 0.0, 0.0]
    assert R.voxelize_windows(rec, [9], bins) == []


# ------------------------------------------------------------------------------------------------ 5. guards and argument errors
def call_abi(rec, offsets, bins, h, w, code, grid_ptrs, nwin=None, cols=None, codes=None, relative=1):
    k = len(offsets) - 1 if nwin is None else nwin
    cols = cols if cols is not None else [rec.column_ptr(c) for c in range(4)]
    with torch.cuda.device(DEV):
        return _lib.lib().eemflow_voxelize_windows(
            k, *[ctypes.c_void_p(c) for c in cols], (ctypes.c_int * 4)(*(codes or rec.codes)), (ctypes.c_int64 * len(offsets))(*offsets),
            rec.scale_a, rec.scale_b, relative, bins, h, w, code, (ctypes.c_void_p * max(len(grid_ptrs), 1))(*grid_ptrs),
            _lib.current_stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize("bins,h,w", GRIDS)
@pytest.mark.parametrize("code", [0, 1, 2])
def test_nothing_is_written_outside_the_grids(bins, h, w, code):
    cols, scales = columns("hrem_u8", 15, 6000, h, w)
    rec = recording_of(cols, scales, h, w)
    offsets = [1, 2, 2, 1501, 6000]                                  # one event, empty, odd start, the rest
    total = bins * h * w
    # 33 x 47: an odd pitch, the grids at any 4-byte alignment; 64 x 96: every grid on a 16-byte boundary, as the oracle's own tensors
    # are, so that both run the 16-byte read-out (a thread's share of the moments follows the read-out form)
    pitch = total + 4 + (60 if total % 4 == 0 else 61)
    buf = torch.full((64 + 4 * pitch,), CANARY, dtype=torch.float32, device=DEV)
    ptrs = [buf.data_ptr() + 4 * (64 + k * pitch) for k in range(4)]
    assert call_abi(rec, offsets, bins, h, w, code, ptrs) == 0
    want = composition(cols, scales, offsets, bins, h, w, {0: False, 1: True, 2: "deferred"}[code])
    canary = int(torch.full((1,), CANARY, dtype=torch.float32).view(torch.int32)[0])
    written = total + (4 if code == 2 else 0)
    host = bits(buf).cpu()
    assert bool((host[:64] == canary).all())
    for k in range(4):
        at = 64 + k * pitch
        assert bool((host[at + written:at + pitch] == canary).all()), k                    # behind the grid / behind the record
        grid = buf[at:at + total].view(bins, h, w)
        if want[k] is None:
            assert not bool(bits(grid).any())
        else:
            assert same(grid, want[k]), k
            if code == 2:
                assert same(buf[at + total:at + total + 4], norm_record(want[k])), k


def test_argument_errors_return_before_any_launch():
    bins, h, w = 5, 33, 47
    cols, scales = columns("hrem_u8", 16, 3000, h, w)
    rec = recording_of(cols, scales, h, w)
    R.voxelize_windows(rec, [0, 3000], bins)
    before = last_form()
    total = bins * h * w
    buf = torch.full((2 * total + 8,), CANARY, dtype=torch.float32, device=DEV)
    ptrs = [buf.data_ptr(), buf.data_ptr() + 4 * (total + 4)]
    good = [0, 1000, 3000]
    base = [rec.column_ptr(c) for c in range(4)]
    bad_calls = [
        dict(offsets=good, nwin=0), dict(offsets=[0] * 34, grid_ptrs=ptrs[:1] * 33, nwin=33), dict(offsets=good, code=3), dict(offsets=good, code=-1),
        dict(offsets=[0, 2000, 1000]), dict(offsets=[-1, 10, 20]), dict(offsets=good, bins=0), dict(offsets=good, h=0),
        dict(offsets=good, codes=(5, 2, 2, 9)), dict(offsets=good, cols=[base[0], base[1] + 1, base[2], base[3]]),
        dict(offsets=good, cols=[base[0] + 4, base[1], base[2], base[3]]), dict(offsets=good, cols=[0, base[1], base[2], base[3]]),
        dict(offsets=good, grid_ptrs=[ptrs[0], 0]), dict(offsets=good, grid_ptrs=[ptrs[0], ptrs[1] + 2]),
    ]
    for kw in bad_calls:
        args = dict(offsets=good, bins=bins, h=h, w=w, code=1, grid_ptrs=ptrs)
        args.update(kw)
        assert call_abi(rec, **args) != 0, kw
        assert _lib.lib().eemflow_last_error().decode().startswith("eemflow_voxelize_windows"), kw
    torch.cuda.synchronize()
    assert last_form() == before
    assert bool((bits(buf).cpu() == int(torch.full((1,), CANARY, dtype=torch.float32).view(torch.int32)[0])).all())
    for bad in ([0, 3001], [5, 4], [-1, 4]):
        with pytest.raises(ValueError):
            R.voxelize_windows(rec, bad, bins)
    with pytest.raises(ValueError):
        R.voxelize_windows(rec, good, bins, normalize="later")
    with pytest.raises(_lib.EEMFlowHipError):
        R.EventRecording(*cols, h, w, device="cpu")


# ------------------------------------------------------------------------------------------------ 6. beyond the LDS layout
def test_a_grid_beyond_the_band_layout_packs_and_takes_the_direct_kernel(monkeypatch):
    bins, h, w = 65, 8, 8                                           # more than 64 bins: make_plan refuses
    cols, scales = columns("hrem_u8", 17, 3000, h, w)
    rec = recording_of(cols, scales, h, w)
    offsets = [0, 1, 1, 1200, 3000]
    tails = {False: "", True: "+moments+norm", "deferred": "+moments+stats"}
    for normalize in (False, True, "deferred"):
        got = R.voxelize_windows(rec, offsets, bins, normalize=normalize)
        assert last_form() == "j4:pack+direct" + tails[normalize]
        want = composition(cols, scales, offsets, bins, h, w, normalize)
        assert last_form() == "j1:direct" + tails[normalize]       # the oracle's sets fall to the same kernel, one after the other
        for k, (g, r) in enumerate(zip(got, want)):
            if r is None:
                assert not bool(bits(g).any())
                if normalize == "deferred":
                    assert norm_record(g).tolist() == [0.0, 1.0, 0.0, 0.0]
                continue
            # the direct kernel adds with fp32 atomics in no defined order: the route's own tolerance (tests/test_gpu_parity.py)
            assert float((g[0] - r).abs().max()) < 2e-4, (normalize, k)
            if normalize == "deferred":
                assert float((norm_record(g) - norm_record(r)).abs().max()) < 2e-4
        assert float(got[3].abs().max()) > 0.5
    monkeypatch.setenv("EEM_VOX_DIRECT", "1")                        # the switch sends a grid the bands could take the same way
    rec2 = recording_of(*columns("hrem_u8", 18, 3000, 33, 47), 33, 47)
    R.voxelize_windows(rec2, [0, 1500, 3000], 5)
    assert last_form() == "j2:pack+direct+moments+norm"


# ------------------------------------------------------------------------------------------------ 7. run_recording
def stream_recording(h, w, windows, per_window, seed):
    cols, scales = columns("hrem_u8", seed, windows * per_window, h, w, stray=False)
    rec = recording_of(cols, scales, h, w)
    return cols, scales, rec, rec.window_offsets(count=per_window)


def volumes_of(cols, scales, offsets, bins, h, w):
    return [g[None] for g in composition(cols, scales, offsets.tolist(), bins, h, w, True)]


def check_run_recording(net, h, w, seed, **kw):
    cols, scales, rec, offsets = stream_recording(h, w, 7, 3000, seed)
    assert len(offsets) == 8
    vols = volumes_of(cols, scales, offsets, net.n_first_channels, h, w)
    with torch.no_grad():
        runs = {chunk: list(harness.run_recording(net, rec, offsets, chunk=chunk, **kw)) for chunk in (3, 7)}
        ref = net.forward_many([(vols[i], vols[i + 1]) for i in range(6)], **kw)
    for chunk, items in runs.items():
        assert [it['k'] for it in items] == list(range(6)), chunk
        for it, (_, preds) in zip(items, ref):
            assert it['flow'].shape == (1, 2, h, w) and same(it['flow'], preds[-1]), (chunk, it['k'], float((it['flow'] - preds[-1]).abs().max()))
    assert float(ref[0][1][-1].abs().max()) > 1e-4
    return rec, offsets, vols


def test_run_recording_eemflow(monkeypatch):
    from test_gpu_stream import make_net, pin_forms
    pin_forms(monkeypatch, "1")
    net, _ = make_net(81)
    h, w = 64, 96                                                   # pads to 64 x 128
    rec, offsets, vols = check_run_recording(net, h, w, 21)
    with torch.no_grad():
        items = list(harness.run_recording(net, rec, offsets, bidirectional=True))
        net.reset_stream()
        ref = net.forward_stream(vols, bidirectional=True)
        checked = list(harness.run_recording(net, rec, offsets, fb_check=(1.0, 0.05), fwl=True, rsat=True))
    assert len(items) == len(ref) == len(checked) == 6
    for it, (_, fw, bw) in zip(items, ref):
        assert same(it['flow'], fw[-1]) and same(it['flow_bw'], bw[-1]), it['k']
    tables = rec.tables(offsets[:7])
    want = fwl_many(tables, [it['flow'][0] for it in checked])
    for it, v in zip(checked, want):
        assert it['mask_fw'].shape == (1, 1, h, w) and it['mask_bw'].shape == (1, 1, h, w)
        assert float(it['FWL']) == float(v) and float(it['RSAT']) == float(it['RSAT'])
    with pytest.raises(ValueError, match="chunk is 1..8"):
        next(harness.run_recording(net, rec, offsets, chunk=9, bidirectional=True))
    with pytest.raises(ValueError, match="iters= needs a model .*EEMFlow has none"):
        next(harness.run_recording(net, rec, offsets, iters=2))


def test_run_recording_eraft(monkeypatch):
    from test_gpu_eraft_stream import make_net, pin_forms
    pin_forms(monkeypatch)
    net, _ = make_net(82)
    rec, offsets, _ = check_run_recording(net, 136, 200, 22, iters=2)
    with pytest.raises(ValueError, match="ERAFT has none"):
        next(harness.run_recording(net, rec, offsets, fb_check=(1.0, 0.05)))


def test_run_recording_eemflow_plus(monkeypatch):
    from test_gpu_plus_stream import make_net, pin_forms
    net, _ = make_net(83, 5)
    pin_forms(monkeypatch, net)
    check_run_recording(net, 256, 320, 23)


def test_tables_equal_the_packed_slices():
    h, w = 64, 96
    cols, scales = columns("bool_p", 24, 5000, h, w)
    rec = recording_of(cols, scales, h, w)
    offsets = [3, 4, 4, 2001, 5000]
    for relative in (True, False):
        got = rec.tables(offsets, relative=relative)
        for (a, b), g in zip(zip(offsets, offsets[1:]), got):
            assert g.shape == (b - a, 4) and g.dtype == torch.float64
            if b > a:
                want = E.host_events(tuple(c[a:b] for c in cols), scale_a=scales[0], scale_b=scales[1], relative=relative)
                assert np.array_equal(g.cpu().numpy().view(np.int64), want.view(np.int64)), (a, b, relative)


def test_an_unsorted_recording_takes_one_host_argsort():
    h, w = 33, 47
    cols, scales = columns("i32_i16", 25, 4000, h, w)
    perm = np.random.default_rng(1).permutation(4000)
    before = dict(E.route_counts)
    rec = recording_of(tuple(c[perm] for c in cols), scales, h, w)
    assert rec.route == 'host' and E.route_counts['host'] == before['host'] + 1 and E.route_counts['device'] == before['device']
    order = np.argsort(cols[0][perm], kind='stable')
    ordered = tuple(c[perm][order] for c in cols)
    assert np.array_equal(rec.t_host, ordered[0])
    offsets = rec.window_offsets(window=10_000_000)
    assert_windows_equal(R.voxelize_windows(rec, offsets, 5), composition(ordered, scales, offsets.tolist(), 5, h, w, True), True, "sorted")


# ------------------------------------------------------------------------------------------------ 8. cli run
def test_cli_run_writes_the_flows_of_run_recording(tmp_path, capsys, monkeypatch):
    from eemflow_amd.weights import seeded_state_dict
    h, w = 64, 96
    cols, scales = columns("hrem_u8", 26, 5 * 3000 + 700, h, w, stray=False)
    p01 = (cols[3] == 1).astype(np.uint8)                           # the file holds p in {0, 1}; the reader forms 2 * p - 1
    npz = str(tmp_path / "recording.npz")
    np.savez(npz, t=cols[0], x=cols[1], y=cols[2], p=p01)
    config = cli.load_config(None)
    net = cli.build_model("EEMFlow", config, training=False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(84).items()})
    ckpt = str(tmp_path / "ckpt.pth.tar")
    harness.save_checkpoint(ckpt, net, 0)
    out = str(tmp_path / "flows")
    summary = cli.main(['run', '--events', npz, '--height', str(h), '--width', str(w), '--checkpoint', ckpt, '--window_events', '3000',
                        '--out', out, '--fwl', '--device', DEV])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('pair')]
    assert summary['windows'] == 5 and summary['pairs'] == 4 and summary['events'] == 15000 and summary['frames_per_s'] > 0
    assert sorted(os.listdir(out)) == ['%06d.flo' % k for k in range(4)] and len(lines) == 4
    rec = R.EventRecording.from_npz(npz, h, w, device=DEV)
    offsets = rec.window_offsets(count=3000)
    net = net.to(DEV).eval()
    with torch.no_grad():
        items = list(harness.run_recording(net, rec, offsets))
    want_fwl = fwl_many(rec.tables(offsets[:5]), [it['flow'][0] for it in items]).tolist()
    for it, line, fwl in zip(items, lines, want_fwl):
        flo = hrem.read_flo(os.path.join(out, '%06d.flo' % it['k']))
        assert np.array_equal(flo.view(np.int32), it['flow'][0].permute(1, 2, 0).contiguous().cpu().numpy().view(np.int32)), it['k']
        assert abs(float(line.split('FWL:')[1].split()[0]) - fwl) < 1e-6, line
    assert summary['meanFWL'] == pytest.approx(sum(want_fwl) / 4, rel=1e-12) and summary['meanRSAT'] is None
    assert eemflow_amd.voxelize_recording_windows is R.voxelize_windows
