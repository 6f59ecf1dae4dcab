"""The image of warped events and the flow warp loss on the GPU (eemflow_amd/iwe.py, csrc/iwe.hip) against the fp64 restatement of
tests/iwe_reference.py, in both kernel forms - binned (the default) and direct (EEM_IWE_DIRECT=1).  Needs a real MI355X: `pytest -m gpu`.

Tolerances.  Warp: |d| <= 1e-9 px against the reference function's fp64 output - the fp64 headroom of a few operations on coordinates of
about 1e3 (a direct bilinear sample against the reference's normalise / un-normalise round trip differs by 2.3e-13 px at most up to
720 x 1280).  Image: per cell |d| <= 2^-23 |ref| + 1e-6 - one fp32 ulp for two fp64 sums that round apart, plus up to 250 votes per cell
each off by the 4e-9 the coordinate bound allows; the cases keep every cell under 250 votes.  Moments: 1e-9 relative to the fp64 sums of
the returned image (n 2^-53 for 9.2e5 cells, times ten)."""
import functools
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from eemflow_amd import EEMFlow
from eemflow_amd.harness import Logger, TestRaftEvents, stream_chunks
from eemflow_amd.mvsec import MvsecEventFlow
from eemflow_amd.weights import seeded_state_dict

from iwe_reference import fwl_reference, iwe_reference, metric_refs, moments_of, separable_flow

iwe = importlib.import_module("eemflow_amd.iwe")        # (the package's attribute `iwe` is the one-job function)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iwe.npz")
# name -> (H, W, N, fractional coordinates)
SHAPES = {"37x50": (37, 50, 5000, False), "64x61": (64, 61, 5000, True), "260x346": (260, 346, 50000, False),
          "8x1280": (8, 1280, 3000, False), "720x1280": (720, 1280, 200000, False),
          "241x40": (241, 40, 5000, True)}               # rows = 2 per band, 121 bands, the last of them one row: the short last band


@pytest.fixture(params=["binned", "direct"])
def form(request, monkeypatch):
    if request.param == "direct":
        monkeypatch.setenv("EEM_IWE_DIRECT", "1")
    else:
        monkeypatch.delenv("EEM_IWE_DIRECT", raising=False)
    return request.param


def smooth_flow(h, w):
    y, x = torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64)
    return separable_flow((6.0 * torch.sin(2 * math.pi * x / w) + 2.0).float(), (4.0 * torch.cos(2 * math.pi * y / h)).float())


def make_events(seed, n, h, w, fractional=False, span=0.05):
    rng = np.random.default_rng(seed)
    t = np.sort(np.round(rng.uniform(0, span, n) * 1e6) * 1e-6)
    if fractional:                                       # up to 2 px outside the frame on every side
        x, y = rng.uniform(-2.0, w + 1.0, n), rng.uniform(-2.0, h + 1.0, n)
    else:
        x, y = rng.integers(0, w, n).astype(np.float64), rng.integers(0, h, n).astype(np.float64)
    p = rng.integers(0, 2, n) * 2.0 - 1.0
    return torch.from_numpy(np.stack([t, x, y, p], axis=1))


@functools.lru_cache(maxsize=None)
def case(name):
    h, w, n, fractional = SHAPES[name]
    return make_events(sum(map(ord, name)), n, h, w, fractional), smooth_flow(h, w), h, w


@functools.lru_cache(maxsize=None)
def reference(name, t_ref):
    ev, flow, h, w = case(name)
    img, m = iwe_reference(ev, flow, h, w, t_ref=t_ref)
    return img, m


def close(got, ref):
    """The per-cell bound; returns the worst excess for the message."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape
    excess = (got - ref).abs() - (2.0 ** -23 * ref.abs() + 1e-6)
    print("max |d| = %.3e, worst excess over the bound = %.3e" % (float((got - ref).abs().max()), float(excess.max())))
    return bool((excess <= 0).all())


def check_moments(image, moments, dropped=0.0):
    n, s, q = moments_of(image.cpu())
    m = moments.cpu().tolist()
    print("moments", m, "from the image", (n, s, q))
    assert m[0] == n and m[3] == dropped
    assert abs(m[1] - s) <= 1e-9 * abs(s) and abs(m[2] - q) <= 1e-9 * abs(q)


# ------------------------------------------------------------------------------------------------ warp
def test_warp_against_the_reference_functions_fp64_output(form):
    z = np.load(GOLDEN)
    for k in range(int(z["ncases"])):
        ev = torch.from_numpy(z[f"events_{k}"])
        flow = separable_flow(torch.from_numpy(z[f"u_row_{k}"]), torch.from_numpy(z[f"v_col_{k}"]))
        for j, t0 in enumerate(z[f"t0_{k}"]):
            got = iwe.warp_events(ev.to(DEV), flow.to(DEV), t0=None if np.isnan(t0) else float(t0)).cpu()
            assert got.shape == (ev.shape[0], 2) and got.dtype == torch.float64
            dx = (got[:, 0] - torch.from_numpy(z[f"xw_{k}_{j}_f64"])).abs().max()
            dy = (got[:, 1] - torch.from_numpy(z[f"yw_{k}_{j}_f64"])).abs().max()
            print(k, j, "max |d|: %.3e %.3e px" % (float(dx), float(dy)))
            assert dx <= 1e-9 and dy <= 1e-9
    # scale and offset: the metric convention's warp, against the restatement
    ev, flow, h, w = case("64x61")
    t0, scale = metric_refs(ev, "end")
    from iwe_reference import warp_direct
    xw, yw = warp_direct(ev, flow.double(), t0, scale, 3.0, -2.0)
    got = iwe.warp_events(ev.to(DEV), flow.to(DEV), t0=t0, scale=scale, offset=(3, -2)).cpu()
    assert (got[:, 0] - xw).abs().max() <= 1e-9 and (got[:, 1] - yw).abs().max() <= 1e-9
    assert iwe.warp_events(ev[:0].to(DEV), flow.to(DEV)).shape == (0, 2)


# ------------------------------------------------------------------------------------------------ image and moments
@pytest.mark.parametrize("t_ref", ["end", "start"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_iwe_against_the_fp64_restatement(form, name, t_ref):
    ev, flow, h, w = case(name)
    ref, ref_m = reference(name, t_ref)
    assert ref.max() < 250                               # the bound's premise: every cell under 250 votes
    image, moments = iwe.iwe(ev.to(DEV), flow.to(DEV), t_ref=t_ref)
    assert image.shape == (2, h, w) and image.dtype == torch.float32 and moments.shape == (4,) and moments.dtype == torch.float64
    assert close(image, ref)
    check_moments(image, moments)
    assert abs(moments[1].item() - ref_m[1]) <= 2.0 ** -23 * ref_m[1] + 2e-6 * h * w      # (the image bound, summed over the cells)


@pytest.mark.parametrize("ept", ["1", "2", "4"])
def test_every_events_per_thread_form_of_the_binning_kernel(monkeypatch, ept):
    """The binning kernel handles 1, 2 or 4 events per thread by event count (4 from 1e6 events on); EEM_IWE_EPT picks the form, so a
    set of 5e4 events checks each of them: more than one binning block and several bands in every form."""
    monkeypatch.delenv("EEM_IWE_DIRECT", raising=False)
    monkeypatch.setenv("EEM_IWE_EPT", ept)
    ev, flow, h, w = case("260x346")
    ref, _ = reference("260x346", "end")
    image, moments = iwe.iwe(ev.to(DEV), flow.to(DEV))
    assert close(image, ref)
    check_moments(image, moments)
    frac, flow2, h2, w2 = case("64x61")                     # targets leaving the frame on all four sides
    image, moments = iwe.iwe(frac.to(DEV), flow2.to(DEV))
    assert close(image, reference("64x61", "end")[0])
    check_moments(image, moments)


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_flow_with_integer_coordinates_is_the_count_image(form, name):
    h, w, n, _ = SHAPES[name]
    ev = make_events(7 + n, n, h, w, fractional=False)
    x, y, c = ev[:, 1].long(), ev[:, 2].long(), (ev[:, 3] <= 0).long()
    count = torch.zeros(2 * h * w).index_add_(0, c * h * w + y * w + x, torch.ones(n)).view(2, h, w)
    none, m0 = iwe.iwe(ev.to(DEV), None, size=(h, w))
    zero, m1 = iwe.iwe(ev.to(DEV), torch.zeros(2, h, w, device=DEV))
    assert torch.equal(none.cpu(), count) and torch.equal(zero.cpu(), count)
    assert m0.cpu().tolist() == m1.cpu().tolist() and m0[1].item() == float(n)
    check_moments(none, m0)


def test_offset_moves_the_frame(form):
    """offset=(ox, oy) is a crop: the image of the shifted events in the cropped flow's frame."""
    ev, flow, h, w = case("260x346")
    crop = flow[:, 2:258, 45:301].contiguous()
    ref, _ = iwe_reference(ev, crop, 256, 256, offset=(45, 2))
    image, moments = iwe.iwe(ev.to(DEV), crop.to(DEV), offset=(45, 2))
    assert close(image, ref)
    check_moments(image, moments)
    assert moments[1].item() < ev.shape[0]               # the events outside the crop are gone


# ------------------------------------------------------------------------------------------------ edge cases
def test_no_events(form):
    h, w = 37, 50
    image = torch.full((2, h, w), 7.0, device=DEV)       # every cell is written: nothing of an earlier image survives
    images, moments = iwe.iwe_many([torch.zeros(0, 4, dtype=torch.float64, device=DEV)], [smooth_flow(h, w).to(DEV)])
    assert torch.count_nonzero(images[0]) == 0 and moments.cpu().tolist() == [[float(h * w), 0.0, 0.0, 0.0]]
    assert math.isnan(iwe.fwl(torch.zeros(0, 4, dtype=torch.float64, device=DEV), smooth_flow(h, w).to(DEV)).item())
    del image


def test_one_event(form):
    h, w = 37, 50
    ev = torch.tensor([[0.5, 10.25, 20.5, 1.0]], dtype=torch.float64)
    flow = smooth_flow(h, w)
    ref, _ = iwe_reference(ev, flow, h, w)
    image, moments = iwe.iwe(ev.to(DEV), flow.to(DEV))
    assert close(image, ref) and abs(moments[1].item() - 1.0) < 1e-6
    assert image[0, 20, 10].item() == 0.375 and image[0, 21, 11].item() == 0.125     # T = 0: no motion, four exact votes
    check_moments(image, moments)


def test_all_timestamps_equal(form):
    ev, flow, h, w = case("64x61")
    ev = ev.clone()
    ev[:, 0] = 0.125                                     # T = 0 counts as 1; t_last - t = 0: nothing moves
    ref, _ = iwe_reference(ev, flow, h, w)
    still, _ = iwe_reference(ev, None, h, w)
    assert torch.equal(ref, still)
    image, moments = iwe.iwe(ev.to(DEV), flow.to(DEV))
    assert close(image, ref)
    check_moments(image, moments)


def test_warped_positions_exactly_on_integers(form):
    """A constant integer flow and events at the window's two ends: tau is exactly 1 or 0, every vote has weight exactly 1 or 0."""
    h, w, n = 64, 61, 4000
    ev = make_events(11, n, h, w)
    ev[: n // 2, 0], ev[n // 2:, 0] = 0.0, 0.5
    flow = torch.tensor([3.0, -2.0]).view(2, 1, 1).expand(2, h, w).contiguous()
    x = ev[:, 1] + torch.where(ev[:, 0] == 0.0, 3.0, 0.0)
    y = ev[:, 2] - torch.where(ev[:, 0] == 0.0, 2.0, 0.0)
    ok = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    c = (ev[:, 3] <= 0).long()
    exact = torch.zeros(2 * h * w).index_add_(0, (c * h * w + y.long() * w + x.long())[ok], torch.ones(int(ok.sum()))).view(2, h, w)
    image, moments = iwe.iwe(ev.to(DEV), flow.to(DEV))
    assert 0 < int(ok.sum()) < n                         # some targets leave the frame
    assert torch.equal(image.cpu(), exact)
    assert moments[1].item() == float(ok.sum()) and moments[3].item() == 0.0


def test_nan_flow_pixel_drops_its_events_and_counts_them(form):
    ev, flow, h, w = case("37x50")
    flow = flow.clone()
    flow[0, 17, 23] = float("nan")
    ref, ref_m = iwe_reference(ev, flow, h, w)
    assert 0 < ref_m[3] < ev.shape[0]
    image, moments = iwe.iwe(ev.to(DEV), flow.to(DEV))
    assert moments[3].item() == ref_m[3]
    assert not torch.isnan(image).any()
    assert close(image, ref)
    check_moments(image, moments, dropped=ref_m[3])


def test_twenty_thousand_events_on_one_pixel(form):
    h, w, n = 37, 50, 20000
    ev = torch.zeros(n, 4, dtype=torch.float64)
    ev[:, 0] = torch.arange(n, dtype=torch.float64) * 1e-6
    ev[:, 1], ev[:, 2] = 31.0, 19.0
    ev[:, 3] = torch.where(torch.arange(n) % 3 == 0, 1.0, -1.0)
    pos = int((ev[:, 3] > 0).sum())
    image, moments = iwe.iwe(ev.to(DEV), None, size=(h, w))
    image = image.cpu()
    assert image[0, 19, 31].item() == float(pos) and image[1, 19, 31].item() == float(n - pos)
    assert image.sum().item() == 20000.0 and int(torch.count_nonzero(image)) == 2
    assert moments.cpu().tolist() == [float(h * w), 20000.0, 20000.0 ** 2, 0.0]


# ------------------------------------------------------------------------------------------------ batching
@pytest.mark.parametrize("jobs", [16, 32])
def test_batched_jobs_equal_the_one_job_calls(form, jobs):
    h, w = 64, 61
    flow = smooth_flow(h, w).to(DEV)
    rng = np.random.default_rng(jobs)
    sets, flows = [], []
    for k in range(jobs):
        n = 0 if k % 7 == 3 else int(rng.integers(1, 6000))
        sets.append(make_events(100 + k, n, h, w, fractional=True).to(DEV) if n else torch.zeros(0, 4, dtype=torch.float64, device=DEV))
        flows.append(None if k % 5 == 1 else flow * (1.0 + 0.1 * k))
    assert any(f is None for f in flows) and any(s.shape[0] == 0 for s in sets) and len({s.shape[0] for s in sets}) > jobs // 2
    images, moments = iwe.iwe_many(sets, flows, size=(h, w))
    assert len(images) == jobs and moments.shape == (jobs, 4)
    for k in range(jobs):
        one, m = iwe.iwe(sets[k], flows[k], size=(h, w))
        assert close(images[k], one.cpu()), k
        for a, b in zip(moments[k].cpu().tolist(), m.cpu().tolist()):
            assert abs(a - b) <= 1e-9 * abs(b), k


@functools.lru_cache(maxsize=None)
def stream_sets():
    h, w = 260, 346
    flow = smooth_flow(h, w)
    sets = [make_events(700 + k, 40_000 + 500 * k, h, w) for k in range(4)]
    return h, w, flow, sets, [iwe_reference(ev, flow, h, w, t_ref="end") for ev in sets]


@pytest.mark.parametrize("nstreams", [2, 10])
def test_alternating_streams_share_the_scratch_safely(form, nstreams):
    """Calls from one thread on several streams: up to eight streams keep a scratch arena each, further ones take over the least
    recently used arena behind an event (the ninth and tenth stream here)."""
    h, w, flow, sets, refs = stream_sets()
    streams = [torch.cuda.Stream(DEV) for _ in range(nstreams)]
    outs = []
    for rep in range(3):
        for k, ev in enumerate(sets):
            with torch.cuda.stream(streams[(rep * len(sets) + k) % nstreams]):
                images, moments = iwe.iwe_many([ev.to(DEV)], [flow.to(DEV)])
                outs.append((k, images[0], moments[0]))
    torch.cuda.synchronize(DEV)
    for k, image, moments in outs:
        assert close(image, refs[k][0]), k
        check_moments(image, moments)


def test_fwl_many_rides_each_set_twice(form):
    h, w = 64, 61
    flow = smooth_flow(h, w)
    sets = [make_events(300 + k, 2000 + 100 * k, h, w, fractional=True) for k in range(18)]           # more than one call of 16
    got = iwe.fwl_many([s.to(DEV) for s in sets], [(flow * (k % 3 - 1.0)).to(DEV) for k in range(18)])
    assert got.shape == (18,) and got.dtype == torch.float64 and got.is_cuda
    for k in range(18):
        ref = fwl_reference(sets[k], flow * (k % 3 - 1.0))
        assert abs(got[k].item() - ref) <= 1e-6 * abs(ref), k
        if k % 3 == 1:
            assert abs(got[k].item() - 1.0) <= 1e-9      # zero flow over zero flow


# ------------------------------------------------------------------------------------------------ known answer
def test_known_answer_constant_flow(form):
    """200 points moving with the constant flow (7, -3): 16 events each at t_j = j T / 15 at p + (u, v) t_j / T.  Warped to the window's
    start they stack on p, warped to its end on p + (7, -3)."""
    h, w, u, v = 64, 96, 7.0, -3.0
    rng = np.random.default_rng(42)
    cells = rng.choice((h - 16 - 3) * (w - 16 - 7), 200, replace=False)       # p and p + (7, -3) both at least 8 px inside
    px = (cells % (w - 16 - 7) + 8).astype(np.float64)
    py = (cells // (w - 16 - 7) + 8 + 3).astype(np.float64)
    T = 0.03
    tj = np.arange(16) * T / 15
    ev = np.stack([np.repeat(tj, 200), np.tile(px, 16) + u * np.repeat(tj, 200) / T, np.tile(py, 16) + v * np.repeat(tj, 200) / T,
                   np.ones(3200)], axis=1)
    ev = torch.from_numpy(ev)
    flow = torch.tensor([u, v]).view(2, 1, 1).expand(2, h, w).contiguous()
    for t_ref, sx, sy in (("start", 0, 0), ("end", 7, -3)):
        expect = torch.zeros(2, h, w, dtype=torch.float64)
        expect[0, torch.from_numpy(py).long() + sy, torch.from_numpy(px).long() + sx] = 16.0
        image, moments = iwe.iwe(ev.to(DEV), flow.to(DEV), t_ref=t_ref)
        d = (image.cpu().double() - expect).abs().max().item()
        print(t_ref, "max |d| = %.3e" % d)
        assert d <= 1e-6
        check_moments(image, moments)
    good = iwe.fwl(ev.to(DEV), flow.to(DEV)).item()
    bad = iwe.fwl(ev.to(DEV), (-flow).to(DEV)).item()
    ref = fwl_reference(ev, flow)
    print("FWL", good, "restatement", ref, "negated flow", bad)
    assert abs(good - ref) <= 1e-6 * ref and good > 1 > bad


# ------------------------------------------------------------------------------------------------ harness
LINE = re.compile(r"^(\d{5} / \d{5}  AEE: \S+  meanAEE:\S+ 3 - mean %AEE: \S+)(?:  FWL: (\S+)  meanFWL:(\S+))?$")


def mvsec_tree(tmp_path, with_events, n_samples=5, first=40):
    """6 windows of 260 x 346 with 3000 events each: flow .npy files on disk, events from an injected reader."""
    flow_dir = tmp_path / "dataset" / "MVSEC" / "seqA" / "flowgt_dt1"
    flow_dir.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(5)
    for i in range(first, first + n_samples):
        np.save(flow_dir / f"{i}.npy", rng.normal(0, 2, (2, 260, 346)).astype(np.float32))

    def reader(path):
        k = int(os.path.basename(path).split(".")[0])
        r = np.random.default_rng(20_000 + k)
        m = 3000
        ts = np.sort(r.uniform(k * 0.05, (k + 1) * 0.05, m))
        return np.stack([ts, r.integers(0, 346, m), r.integers(0, 260, m), r.integers(0, 2, m) * 2 - 1], axis=1).astype(np.float64)

    args = {"eval_type": "dense", "num_voxel_bins": 5, "sequence": "seqA"}
    return MvsecEventFlow(args, train=False, root=str(tmp_path), events_reader=reader, valid_time_index={"seqA": [(first, first + n_samples)]},
                          with_events=with_events)


@pytest.mark.parametrize("stream", [4, 0])
def test_harness_lines_carry_the_flow_warp_loss(form, tmp_path, capsys, monkeypatch, stream):
    monkeypatch.setenv("EEM_WINO4_LAYERS", "7")              # one encoder form whatever the call's batch (as test_gpu_stream pins it)
    monkeypatch.setenv("EEM_DEC_WNC", "1")
    ds = mvsec_tree(tmp_path, True)
    sd = seeded_state_dict(68)
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV)
    logger = Logger(verbose=False)
    tester = TestRaftEvents(ds, (256, 256), logger=logger)
    extra = {"stream": stream} if stream else {}
    capsys.readouterr()
    plain = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, **extra)
    plain_lines = [m for m in map(LINE.match, capsys.readouterr().out.splitlines()) if m]
    assert len(plain_lines) == 5 and all(m.group(2) is None for m in plain_lines)
    assert not any(l.startswith("Mean FWL") for l in logger.lines)

    seen = []                                                # what the loop's own fwl_many calls returned, in sample order
    real = iwe.fwl_many
    monkeypatch.setattr(iwe, "fwl_many", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    with_fwl = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, fwl=True, **extra)
    monkeypatch.setattr(iwe, "fwl_many", real)
    lines = [m for m in map(LINE.match, capsys.readouterr().out.splitlines()) if m]
    assert with_fwl == plain and len(lines) == 5
    assert [m.group(1) for m in lines] == [m.group(1) for m in plain_lines]          # the lines minus the FWL fields
    assert len(seen) == (2 if stream else 5)                 # one call per chunk
    values = torch.cat(seen).cpu().tolist()

    # the same numbers from fwl_many on each sample's events, offset and flow
    with torch.no_grad():
        if stream:
            triples = [(t_, f_) for _, targets, flows in stream_chunks(ds, net, stream, torch.device(DEV)) for t_, f_ in zip(targets, flows)]
        else:
            net.change_imagesize((256, 256))
            triples = []
            for idx in range(5):
                sample = ds[idx]
                triples.append((sample, tester.run_network(net, sample, torch.device(DEV))))
    assert len(triples) == 5
    running, count = 0.0, 0
    for i, (carrier, flow) in enumerate(triples):
        assert carrier['events_offset'] == (45, 2) and carrier['events'].shape == (3000, 4) and carrier['events'].is_cuda
        own = iwe.fwl_many([carrier['events']], [flow[0].contiguous()], offset=carrier['events_offset'])[0].item()
        print(i, "FWL", values[i], "own call", own)
        assert abs(values[i] - own) <= 1e-9 * abs(own)
        running, count = running + values[i], count + 1
        assert lines[i].group(2) == '{:2.6f}'.format(values[i]) and lines[i].group(3) == '{:2.6f}'.format(running / count)
    summary = [l for l in logger.lines if l.startswith("Mean FWL")]
    assert summary == ["Mean FWL: {:.6f}".format(running / count)]
