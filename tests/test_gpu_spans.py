"""Windows by span of a device-resident recording (eemflow_voxelize_spans, eemflow_event_mask_spans, recording.voxelize_windows(spans=),
EventRecording.tables(spans=), mvsec_raw.event_mask_windows(spans=)), pairs at a lag (harness.run_recording(spans=, lag=)), MVSEC's dt4
protocol from a raw sequence (MvsecRaw.frame_spans(reference_pairs=True)) and the two command lines.  The oracle of every grid is the
existing route on the host slice, voxelize_many_device(pack_events_many([slice])); of every flow the model's own forward_many on the two
volumes; of the dt4 samples the dataset route (MvsecEventFlow_dt4 over files).  Equality is BITWISE everywhere except the direct form,
whose fp32 atomics have no defined order.  `pytest -m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from eemflow_amd import _lib, cli, events as E, harness, hrem, mvsec, mvsec_raw as M, recording as R
from eemflow_amd.metrics import flow_error_from_sums, flow_error_sums_many
from eemflow_amd.voxelizer import norm_record, voxelize_many_device

from mvsec_dt4_sequence import make_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = -12345.678
N = 20000
# one event; two events of one timestamp (dT = 0 -> 1); a long window from the odd element 3; two REPEATED windows that overlap it;
# an EMPTY window at the odd element 4101; a window that NESTS all of them; a window nested in the repeated ones.  No order between them
SPANS = [(0, 1), (1, 3), (3, 4100), (2000, 9000), (2000, 9000), (4101, 4101), (100, 20000), (5000, 6000)]
GRIDS = [(5, 33, 47), (5, 64, 96)]                                  # hw no multiple of 4: scalar read-out; 16-byte read-out


# ------------------------------------------------------------------------------------------------ helpers
def columns(kind, seed, n, h, w, stray=True):
    """tests/test_gpu_recording.py's recipe: (t, x, y, p) as read_event_columns would return them, in time order with ties, and the
    (scale_a, scale_b) that go with them.  stray: a few events with x >= W or y >= H."""
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
    assert kind == "i32_i16"                                        # the generic instantiation behind pk_load's dtype switch
    return (ticks.astype(np.int32), x.astype(np.int16), y.astype(np.int16), (2 * pol - 1).astype(np.int8)), (1e-9, 1e6)


def recording_of(cols, scales, h, w):
    return R.EventRecording(*cols, h, w, device=DEV, scale_a=scales[0], scale_b=scales[1])


def composition(cols, scales, spans, bins, h, w, normalize, relative=True):
    """The oracle: per non-empty span pack_events_many of the HOST slice, then voxelize_many_device, 32 sets per call; None for an
    empty span (the existing route refuses one)."""
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
        assert g.dtype == torch.float32, (what, k)
        if r is None:                                               # an empty span: +0.0 everywhere, the record of no voxels
            assert not bool(bits(g).any()), (what, k)
            if normalize == "deferred":
                assert norm_record(g).tolist() == [0.0, 1.0, 0.0, 0.0], (what, k)
            continue
        assert g.shape == (1,) + tuple(r.shape), (what, k)
        assert same(g[0], r), (what, k, float((g[0] - r).abs().max()))
        if normalize == "deferred":
            assert same(norm_record(g), norm_record(r)), (what, k, norm_record(g).tolist(), norm_record(r).tolist())


# ------------------------------------------------------------------------------------------------ G1. bitwise against the composition
@pytest.mark.parametrize("kind", ["hrem_u8", "i32_i16"])            # both instantiations of vox_bin_cols_kernel
@pytest.mark.parametrize("bins,h,w", GRIDS)
def test_spans_equal_the_composition_bitwise(bins, h, w, kind):
    cols, scales = columns(kind, 11, N, h, w)
    t = cols[0]
    assert t[1] == t[2] and t[4099] == t[4100] == t[4101] and t[8999] == t[9000]
    rec = recording_of(cols, scales, h, w)
    assert rec.route == 'device'
    for normalize in (False, True, "deferred"):
        for relative in (False, True):
            got = R.voxelize_windows(rec, spans=np.asarray(SPANS, dtype=np.int64), num_bins=bins, normalize=normalize, relative=relative)
            form = last_form()
            want = composition(cols, scales, SPANS, bins, h, w, normalize, relative)
            assert_windows_equal(got, want, normalize, (kind, normalize, relative))
            assert same(got[3], got[4])                             # the repeated span: each job has its own records, the same grid
            assert form.startswith("j8:colbin_e1+band"), form
            assert form.endswith({False: "_raw", True: "_raw_sums+norm", "deferred": "_raw_sums+stats"}[normalize]), form
    assert float(got[6].abs().max()) > 0.5 and float(got[0].abs().sum()) > 0.5 and float(got[1].abs().sum()) > 0.5


# ------------------------------------------------------------------------------------------------ G2. launches, forms, guards
def test_33_spans_in_one_call_equal_one_span_per_call():
    bins, h, w = 5, 33, 47
    cols, scales = columns("hrem_u8", 13, N, h, w)
    rec = recording_of(cols, scales, h, w)
    spans = rec.sliding_spans(count=1200, stride_count=500)[:33]     # every window overlaps its two neighbours on either side
    assert spans.shape == (33, 2) and spans[1, 0] < spans[0, 1] and spans[2, 0] < spans[0, 1]
    for normalize in (True, "deferred"):
        together = R.voxelize_windows(rec, spans=spans, num_bins=bins, normalize=normalize)
        assert last_form().startswith("j1:colbin_e1")               # the second launch sequence held the 33rd span
        alone = [R.voxelize_windows(rec, spans=spans[k:k + 1], num_bins=bins, normalize=normalize)[0] for k in range(33)]
        assert_windows_equal(together, [a[0] for a in alone], normalize, normalize)
    assert_windows_equal(together[30:], composition(cols, scales, spans.tolist()[30:], bins, h, w, "deferred"), "deferred", "tail")
    assert R.voxelize_windows(rec, spans=np.zeros((0, 2), np.int64), num_bins=bins) == []


def test_a_long_span_and_a_short_one_inside_it_share_a_call():
    bins, h, w, n = 5, 64, 96, 600_000
    cols, scales = columns("hrem_u8", 12, n, h, w)
    rec = recording_of(cols, scales, h, w)
    spans = [(0, n), (1001, 3000)]
    got = R.voxelize_windows(rec, spans=spans, num_bins=bins, normalize="deferred")
    assert last_form().startswith("j2:colbin_e2+band"), last_form()  # one events-per-thread form for the call: the longest span's
    assert_windows_equal(got, composition(cols, scales, spans, bins, h, w, "deferred"), "deferred", "long+short")


def test_overlapping_spans_in_the_direct_form(monkeypatch):
    bins, h, w = 5, 33, 47
    cols, scales = columns("hrem_u8", 18, 3000, h, w)
    rec = recording_of(cols, scales, h, w)
    spans = [(0, 2000), (500, 3000), (500, 3000), (7, 7), (1000, 1500)]
    want = composition(cols, scales, spans, bins, h, w, "deferred")  # (banded: the bitwise oracle of the values)
    monkeypatch.setenv("EEM_VOX_DIRECT", "1")
    got = R.voxelize_windows(rec, spans=spans, num_bins=bins, normalize="deferred")
    assert last_form() == "j5:pack+direct+moments+stats"
    for k, (g, r) in enumerate(zip(got, want)):
        if r is None:
            assert not bool(bits(g).any()) and norm_record(g).tolist() == [0.0, 1.0, 0.0, 0.0]
            continue
        # the direct kernel adds with fp32 atomics in no defined order: the route's own tolerance (tests/test_gpu_recording.py, test_gpu_parity.py)
        assert float((g[0] - r).abs().max()) < 2e-4, k
        assert float((norm_record(g) - norm_record(r)).abs().max()) < 2e-4, k
    assert float(got[1].abs().max()) > 0.5


def call_abi(rec, spans, bins, h, w, code, grid_ptrs, nwin=None, starts_null=False, ends_null=False):
    k = len(spans) if nwin is None else nwin
    starts = None if starts_null else (ctypes.c_int64 * max(len(spans), 1))(*[a for a, _ in spans])
    ends = None if ends_null else (ctypes.c_int64 * max(len(spans), 1))(*[b for _, b in spans])
    with torch.cuda.device(DEV):
        return _lib.lib().eemflow_voxelize_spans(
            k, *[ctypes.c_void_p(rec.column_ptr(c)) for c in range(4)], (ctypes.c_int * 4)(*rec.codes), starts, ends, rec.scale_a, rec.scale_b, 1,
            bins, h, w, code, (ctypes.c_void_p * max(len(grid_ptrs), 1))(*grid_ptrs), _lib.current_stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize("bins,h,w", GRIDS)
@pytest.mark.parametrize("code", [0, 1, 2])
def test_nothing_is_written_outside_the_grids(bins, h, w, code):
    cols, scales = columns("hrem_u8", 15, 6000, h, w)
    rec = recording_of(cols, scales, h, w)
    spans = [(1501, 6000), (1, 2), (2, 2), (1, 6000)]                # out of order, one event, empty, everything
    total = bins * h * w
    pitch = total + 4 + (60 if total % 4 == 0 else 61)              # (tests/test_gpu_recording.py: both alignments of the read-out)
    buf = torch.full((64 + 4 * pitch,), CANARY, dtype=torch.float32, device=DEV)
    ptrs = [buf.data_ptr() + 4 * (64 + k * pitch) for k in range(4)]
    assert call_abi(rec, spans, bins, h, w, code, ptrs) == 0
    want = composition(cols, scales, spans, bins, h, w, {0: False, 1: True, 2: "deferred"}[code])
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
    R.voxelize_windows(rec, spans=[(0, 3000)], num_bins=bins)
    before = last_form()
    total = bins * h * w
    buf = torch.full((2 * total + 8,), CANARY, dtype=torch.float32, device=DEV)
    ptrs = [buf.data_ptr(), buf.data_ptr() + 4 * (total + 4)]
    good = [(500, 3000), (0, 1000)]
    bad_calls = [dict(spans=[(-1, 10), (0, 5)]), dict(spans=[(0, 5), (10, 9)]), dict(starts_null=True), dict(ends_null=True), dict(nwin=0),
                 dict(spans=[(0, 1)] * 33, grid_ptrs=ptrs[:1] * 33), dict(code=3), dict(bins=0), dict(grid_ptrs=[ptrs[0], 0]),
                 dict(grid_ptrs=[ptrs[0], ptrs[1] + 2])]
    for kw in bad_calls:
        args = dict(spans=good, bins=bins, h=h, w=w, code=1, grid_ptrs=ptrs)
        args.update(kw)
        assert call_abi(rec, **args) != 0, kw
        assert _lib.lib().eemflow_last_error().decode().startswith("eemflow_voxelize_spans"), (kw, _lib.lib().eemflow_last_error().decode())
    torch.cuda.synchronize()
    assert last_form() == before
    assert bool((bits(buf).cpu() == int(torch.full((1,), CANARY, dtype=torch.float32).view(torch.int32)[0])).all())
    one = ctypes.c_int64 * 1
    mask = torch.full((h * w,), CANARY, dtype=torch.float32, device=DEV)
    for starts, ends, nwin in ((one(-1), one(5), 1), (one(6), one(5), 1), (None, one(5), 1), (one(0), None, 1), (one(0), one(5), 0), (one(0), one(5), 33)):
        with torch.cuda.device(DEV):
            rc = _lib.lib().eemflow_event_mask_spans(nwin, ctypes.c_void_p(rec.column_ptr(1)), ctypes.c_void_p(rec.column_ptr(2)), rec.codes[1],
                                                     rec.codes[2], starts, ends, h, w, (ctypes.c_void_p * 1)(mask.data_ptr()),
                                                     _lib.current_stream_ptr(torch.device(DEV)))
        assert rc != 0 and _lib.lib().eemflow_last_error().decode().startswith("eemflow_event_mask_spans")
    torch.cuda.synchronize()
    assert bool((mask == CANARY).all())
    for kw in (dict(spans=[(0, 3001)]), dict(spans=[(5, 4)]), dict(spans=[(-1, 4)]), dict(), dict(offsets=[0, 3000], spans=[(0, 3000)])):
        with pytest.raises(ValueError):
            R.voxelize_windows(rec, num_bins=bins, **kw)
        with pytest.raises(ValueError):
            rec.tables(**kw)
        with pytest.raises(ValueError):
            M.event_mask_windows(rec, **kw)
    with pytest.raises(TypeError, match="num_bins"):
        R.voxelize_windows(rec, spans=[(0, 3000)])


# ------------------------------------------------------------------------------------------------ G3. offsets are spans
def test_offsets_and_their_spans_give_the_same_grids_masks_and_tables():
    bins, h, w = 5, 33, 47
    cols, scales = columns("hrem_u8", 19, N, h, w)
    rec = recording_of(cols, scales, h, w)
    offsets = [0, 1, 3, 4100, 4101, 4101, 9000, N]
    spans = list(zip(offsets, offsets[1:]))
    for normalize in (False, True, "deferred"):
        for relative in (False, True):
            by_offsets = R.voxelize_windows(rec, offsets, bins, normalize=normalize, relative=relative)
            form = last_form()
            by_spans = R.voxelize_windows(rec, spans=spans, num_bins=bins, normalize=normalize, relative=relative)
            assert last_form() == form and form.startswith("j7:colbin_e1+band")
            for k, (a, b) in enumerate(zip(by_offsets, by_spans)):
                assert same(a, b), (normalize, relative, k)
                if normalize == "deferred":
                    assert same(norm_record(a), norm_record(b)), (relative, k)
    # the masks: mvsec.event_mask of every slice, in the spans' order
    odd = [(2000, 9000), (0, 1), (4101, 4101), (100, N), (2000, 9000)] + [(k, k + 700) for k in range(0, 30 * 500, 500)]      # 35: two calls
    got = M.event_mask_windows(rec, spans=odd).cpu().numpy()
    assert got.shape == (35, h, w) and got.dtype == np.float32
    for k, (a, b) in enumerate(odd):
        feats = np.stack([c[a:b].astype(np.float64) for c in cols], axis=1)
        assert np.array_equal(got[k], mvsec.event_mask(feats, h, w).astype(np.float32)), k
    assert got[1].sum() == 1 and not got[2].any() and np.array_equal(got[0], got[4])
    assert torch.equal(M.event_mask_windows(rec, offsets), M.event_mask_windows(rec, spans=spans))
    # the tables: pack_events_many of the slices
    for relative in (True, False):
        tabs = rec.tables(spans=odd, relative=relative)
        live = [k for k, (a, b) in enumerate(odd) if b > a]
        want = []
        for i0 in range(0, len(live), 32):
            want += E.pack_events_many([tuple(c[odd[k][0]:odd[k][1]] for c in cols) for k in live[i0:i0 + 32]], scale_a=scales[0],
                                       scale_b=scales[1], relative=relative, device=DEV)
        for k, r in zip(live, want):
            assert tabs[k].dtype == torch.float64 and tabs[k].shape == r.shape and torch.equal(tabs[k].view(torch.int64), r.view(torch.int64)), k
        assert tabs[2].shape == (0, 4)
        for a, b in zip(rec.tables(offsets, relative=relative), rec.tables(spans=spans, relative=relative)):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ------------------------------------------------------------------------------------------------ G4. the dt4 protocol
@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    return make_sequence(tmp_path_factory.mktemp("mvsec_dt4"))


@pytest.fixture(scope="module")
def net():
    from eemflow_amd import EEMFlow
    from eemflow_amd.weights import seeded_state_dict
    model = EEMFlow("", 5, 5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(3).items()})
    return model.to(DEV).eval()


@pytest.mark.parametrize("eval_type", ["dense", "sparse"])
def test_raw_route_at_dt4_equals_the_dataset_route_bit_for_bit(sequence, net, eval_type):
    s = sequence
    first, last, crop = s["first"], s["last"], (256, 256)
    ds = mvsec.MvsecEventFlow_dt4({"eval_type": eval_type, "num_voxel_bins": 5, "sequence": "seqA"}, train=False, root=s["root"], device=DEV,
                                  valid_time_index={"seqA": [(first, last + 1)]})
    assert len(ds) == 8
    want, calls = {}, 0
    with torch.no_grad():
        net.change_imagesize(crop)
        for chunk, targets, flows, vol_pairs in harness.stream_chunks(ds, net, 4, torch.device(DEV), with_volumes=True):
            calls += 1
            f_gts = [t["flow"].to(DEV)[None].float() for t in targets]                          # as TestRaftEvents scores a chunk
            evs = [t["event_valid"].to(DEV).sum(0) for t in targets] if eval_type == "sparse" else None
            sums = flow_error_sums_many(f_gts, flows, evs, evaluation_type=eval_type)
            for i, idx in enumerate(chunk):
                want[idx] = dict(flow=flows[i].clone(), gt=f_gts[i], ev=targets[i]["event_valid"][0].float(), sums=sums[i].clone(),
                                 old=vol_pairs[i][0].clone(), new=vol_pairs[i][1].clone())
    assert sorted(want) == list(range(8)) and calls == 3               # the carried window is crossed twice

    gt = M.MvsecGroundTruth(s["stack"], s["gt_ts"], device=DEV)
    raw = M.MvsecRaw(s["events"], s["img_ts"], s["inds"], gt, height=s["h"], width=s["w"], device=DEV)
    spans, t_spans, lag = raw.frame_spans(first, last, 4, reference_pairs=True)
    assert lag == 1 and spans.shape == (9, 2) and t_spans.shape == (8, 2)
    assert spans[0].tolist() == [s["inds"][1], s["inds"][5]] and spans[1, 0] < spans[0, 1]        # the windows overlap by three frames
    grids = [mvsec.center_crop(g, crop) for g in R.voxelize_windows(raw.recording, spans=spans, num_bins=5)]
    with torch.no_grad():
        items = list(harness.run_recording(net, raw.recording, spans=spans, t_spans=t_spans, gt=gt, crop=crop, eval_type=eval_type, chunk=4))
    assert [it["k"] for it in items] == list(range(8)) and [it["k2"] for it in items] == list(range(1, 9))
    torch.cuda.synchronize()
    for it in items:
        k, w_ = it["k"], want[it["k"]]
        assert torch.equal(grids[k], w_["old"]) and torch.equal(grids[k + 1], w_["new"]), k       # both volumes of the sample
        assert tuple(it["flow"].shape) == (1, 2, 256, 256) and torch.equal(it["flow"], w_["flow"]), k
        file32 = np.load(ds.flow_list[k]).astype(np.float32)                                      # the fp32 of flowgt_dt4/<first + k>.npy
        assert torch.equal(it["flow_gt"].cpu()[0], mvsec.center_crop(torch.from_numpy(file32), crop)), k
        assert torch.equal(it["flow_gt"], w_["gt"]), k
        if eval_type == "sparse":
            assert torch.equal(it["event_valid"].cpu(), w_["ev"]), k                               # the masks
            assert 0.2 < float(it["event_valid"].mean()) < 0.9
        else:
            assert "event_valid" not in it
        assert it["err_sums"].dtype == torch.float64 and torch.equal(it["err_sums"], w_["sums"]), (k, it["err_sums"], w_["sums"])
    assert all(float(it["err_sums"][2]) > 1000 for it in items)
    assert float(items[0]["flow"].abs().max()) > 1e-4 and not torch.equal(items[0]["flow"], items[1]["flow"])


# ------------------------------------------------------------------------------------------------ G5. pairs at a lag
def sliding_recording(h, w, seed):
    """Nine windows of 3000 events that slide by a third of their length, and their volumes from the host slices."""
    cols, scales = columns("hrem_u8", seed, 11_000, h, w, stray=False)
    rec = recording_of(cols, scales, h, w)
    spans = rec.sliding_spans(count=3000, stride_count=1000)
    assert spans.shape == (9, 2) and spans[3, 0] == spans[0, 1]
    vols = [g[None] for g in composition(cols, scales, spans.tolist(), 5, h, w, True)]
    return rec, spans, vols


def counted_stream(monkeypatch, net, vols):
    """forward_stream behind a wrapper that notes which windows (by their bits) every call was given."""
    import functools
    seen = []
    inner = net.forward_stream

    @functools.wraps(inner)                                          # (run_recording reads the signature for iters=)
    def forward_stream(windows, *a, **kw):
        for v in windows:
            seen.append([i for i, r in enumerate(vols) if same(v, r)])
        return inner(windows, *a, **kw)
    monkeypatch.setattr(net, "forward_stream", forward_stream)
    return seen


def check_lag(monkeypatch, net, h, w, seed, lags, chunk, **kw):
    rec, spans, vols = sliding_recording(h, w, seed)
    for lag in lags:
        want_pairs = [(a, a + lag) for r in range(lag) for a in range(r, 9 - lag, lag)]           # class-major
        with monkeypatch.context() as m, torch.no_grad():
            seen = counted_stream(m, net, vols)
            items = list(harness.run_recording(net, rec, spans=spans, lag=lag, chunk=chunk, **kw))
        assert [(it['k'], it['k2']) for it in items] == want_pairs, lag
        assert sorted(seen) == [[i] for i in range(9)], (lag, seen)                               # every window voxelized and encoded once
        with torch.no_grad():
            ref = net.forward_many([(vols[a], vols[b]) for a, b in want_pairs], **kw)
        for it, (_, preds) in zip(items, ref):
            assert it['flow'].shape == (1, 2, h, w) and same(it['flow'], preds[-1]), (lag, it['k'], float((it['flow'] - preds[-1]).abs().max()))
        assert float(ref[0][1][-1].abs().max()) > 1e-4 and not same(ref[0][1][-1], ref[1][1][-1])
    return rec, spans, vols


def test_pairs_at_a_lag_eemflow(monkeypatch):
    from test_gpu_stream import make_net, pin_forms
    pin_forms(monkeypatch, "1")
    net, _ = make_net(81)
    h, w = 64, 96
    rec, spans, vols = check_lag(monkeypatch, net, h, w, 31, (2, 3), 3)
    # offsets at a lag: consecutive windows, pairs (a, a + 2); FWL of window k's events; both directions pass through
    from eemflow_amd.iwe import fwl_many
    offsets = rec.window_offsets(count=1000)
    assert len(offsets) == 12
    with torch.no_grad():
        items = list(harness.run_recording(net, rec, offsets, lag=2, fwl=True, fb_check=(1.0, 0.05)))      # a class per call (6 and 5 windows)
        thirds = R.voxelize_windows(rec, offsets, 5)
        tables = rec.tables(offsets)
        assert [it['k'] for it in items] == [0, 2, 4, 6, 8, 1, 3, 5, 7] and all('k2' not in it for it in items)
        at = 0
        for members in ([0, 2, 4, 6, 8, 10], [1, 3, 5, 7, 9]):
            net.reset_stream()
            ref = net.forward_stream([thirds[i] for i in members], bidirectional=True, fb_check=(1.0, 0.05))
            mine = items[at:at + len(ref)]
            at += len(ref)
            want_fwl = fwl_many([tables[i] for i in members[:-1]], [it['flow'][0] for it in mine])      # window k's events
            for it, (_, fw, bw, masks), v in zip(mine, ref, want_fwl):
                assert same(it['flow'], fw[-1]) and same(it['flow_bw'], bw[-1]) and same(it['mask_fw'], masks[0]), it['k']
                assert float(it['FWL']) == float(v), it['k']
        assert at == 9


def test_pairs_at_a_lag_eraft(monkeypatch):
    from test_gpu_eraft_stream import make_net, pin_forms
    pin_forms(monkeypatch)
    net, _ = make_net(82)                                            # cold: every pair starts from zero flow, as forward_many does
    check_lag(monkeypatch, net, 136, 200, 32, (2,), 3, iters=2)


def test_pairs_at_a_lag_eemflow_plus(monkeypatch):
    from test_gpu_plus_stream import make_net, pin_forms
    net, _ = make_net(83, 5)
    pin_forms(monkeypatch, net)
    check_lag(monkeypatch, net, 256, 320, 33, (2,), 3)


# ------------------------------------------------------------------------------------------------ G6. the command lines
def test_cli_mvsec_reference_pairs_and_the_default(sequence, net, tmp_path, capsys):
    s = sequence
    data, gtz, ckpt, out = (str(tmp_path / n) for n in ("data.npz", "gt.npz", "ckpt.pth.tar", "flows"))
    np.savez(data, events=s["events"], image_raw_ts=s["img_ts"], image_raw_event_inds=s["inds"])
    np.savez(gtz, flow_dist=s["stack"], flow_dist_ts=s["gt_ts"])
    harness.save_checkpoint(ckpt, net, 0)
    base = ['mvsec', '--data', data, '--gt', gtz, '--checkpoint', ckpt, '--first', '1', '--eval_type', 'sparse', '--crop', '256', '256', '--stream', '4',
            '--device', DEV, '--dt', '4']
    fmt = 'pair {:6d}  frame {:6d}  events {:9d}  AEE: {:2.6f}  %1px: {:.6f}  %3px: {:.6f}'
    raw = M.MvsecRaw.from_npz(data, gtz, device=DEV)

    summary = cli.main(base + ['--reference_pairs', '--out', out])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('pair ')]
    assert summary['pairs'] == 8 == len(lines)                         # --last defaults to the last pair frames and ground truth allow: 8
    assert summary['events'] == int(s["inds"][13] - s["inds"][1])
    spans, t_spans, lag = raw.frame_spans(1, 8, 4, reference_pairs=True)
    with torch.no_grad():
        items = list(harness.run_recording(net, raw.recording, spans=spans, lag=lag, t_spans=t_spans, chunk=4, gt=raw.gt, crop=(256, 256),
                                           eval_type='sparse'))
    aees = []
    for it, line in zip(items, lines):
        aee, p1, p3 = flow_error_from_sums(it['err_sums'])[:3]
        aees.append(aee)
        assert line == fmt.format(it['k'], 1 + it['k'], int(spans[it['k'], 1] - spans[it['k'], 0]), aee, 1.0 - p1, 1.0 - p3)
        assert np.array_equal(hrem.read_flo(os.path.join(out, '%06d_gt.flo' % it['k'])), it['flow_gt'][0].permute(1, 2, 0).cpu().numpy())
        assert np.array_equal(hrem.read_flo(os.path.join(out, '%06d.flo' % it['k'])), it['flow'][0].permute(1, 2, 0).cpu().numpy())
    assert abs(summary['meanAEE'] - sum(aees) / 8) < 1e-12 and summary['meanAEE'] > 0

    # a flow over four frames every two frames: pairs (m, m + 2), printed in the order they arrive
    summary = cli.main(base + ['--stride', '2'])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('pair ')]
    spans2, t_spans2, lag2 = raw.frame_spans(1, 5, 4, stride=2)
    with torch.no_grad():
        items = list(harness.run_recording(net, raw.recording, spans=spans2, lag=lag2, t_spans=t_spans2, chunk=4, gt=raw.gt, crop=(256, 256),
                                           eval_type='sparse'))
    assert lag2 == 2 and [it['k'] for it in items] == [0, 2, 1] and summary['pairs'] == 3 == len(lines)
    for it, line in zip(items, lines):
        aee, p1, p3 = flow_error_from_sums(it['err_sums'])[:3]
        assert line == fmt.format(it['k'], 1 + 2 * it['k'], int(spans2[it['k'], 1] - spans2[it['k'], 0]), aee, 1.0 - p1, 1.0 - p3)

    # without the new flags: consecutive windows of four frames, through offsets, as before
    summary = cli.main(base)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('pair ')]
    offsets, t_edges = raw.frame_windows(1, 5, 4)
    with torch.no_grad():
        items = list(harness.run_recording(net, raw.recording, offsets, chunk=4, gt=raw.gt, t_edges=t_edges, crop=(256, 256), eval_type='sparse'))
    assert summary['pairs'] == 2 == len(lines) == len(items) and summary['events'] == int(offsets[-1] - offsets[0])
    for it, line in zip(items, lines):
        aee, p1, p3 = flow_error_from_sums(it['err_sums'])[:3]
        assert line == fmt.format(it['k'], 1 + 4 * it['k'], int(offsets[it['k'] + 1] - offsets[it['k']]), aee, 1.0 - p1, 1.0 - p3)
        assert sorted(it) == ['err_sums', 'event_valid', 'flow', 'flow_gt', 'k']


def test_cli_run_at_a_stride_writes_the_flows_at_the_lag(tmp_path, capsys):
    from eemflow_amd.weights import seeded_state_dict
    h, w = 64, 96
    cols, scales = columns("hrem_u8", 26, 11_000 + 700, h, w, stray=False)
    p01 = (cols[3] == 1).astype(np.uint8)                           # the file holds p in {0, 1}; the reader forms 2 * p - 1
    npz = str(tmp_path / "recording.npz")
    np.savez(npz, t=cols[0], x=cols[1], y=cols[2], p=p01)
    net = cli.build_model("EEMFlow", cli.load_config(None), training=False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(84).items()})
    ckpt = str(tmp_path / "ckpt.pth.tar")
    harness.save_checkpoint(ckpt, net, 0)
    out = str(tmp_path / "flows")
    summary = cli.main(['run', '--events', npz, '--height', str(h), '--width', str(w), '--checkpoint', ckpt, '--window_events', '3000',
                        '--stride_events', '1000', '--out', out, '--device', DEV])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('pair')]
    assert summary['windows'] == 9 and summary['pairs'] == 6 and summary['events'] == 11000 and summary['frames_per_s'] > 0
    assert sorted(os.listdir(out)) == ['%06d.flo' % k for k in range(6)]
    rec = R.EventRecording.from_npz(npz, h, w, device=DEV)
    spans = rec.sliding_spans(count=3000, stride_count=1000)
    net = net.to(DEV).eval()
    with torch.no_grad():
        items = list(harness.run_recording(net, rec, spans=spans, lag=3))
    assert [it['k'] for it in items] == [0, 3, 1, 4, 2, 5]
    assert lines == ['pair {:6d}  events {:9d}'.format(it['k'], 3000) for it in items]          # in the order the items arrive
    for it in items:
        flo = hrem.read_flo(os.path.join(out, '%06d.flo' % it['k']))
        assert np.array_equal(flo.view(np.int32), it['flow'][0].permute(1, 2, 0).contiguous().cpu().numpy().view(np.int32)), it['k']
    # by duration: 20 ms windows every 10 ms of the 50 ms recording
    summary = cli.main(['run', '--events', npz, '--height', str(h), '--width', str(w), '--checkpoint', ckpt, '--window_ms', '20', '--stride_ms', '10',
                        '--device', DEV])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('pair')]
    by_time = rec.sliding_spans(window=20_000_000, stride=10_000_000)
    assert summary['windows'] == len(by_time) >= 3 and summary['pairs'] == len(by_time) - 2 == len(lines)
