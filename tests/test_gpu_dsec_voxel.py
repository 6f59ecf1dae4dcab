"""The DSEC trilinear voxelizer (csrc/voxel_tri.hip, eemflow_amd/dsec.py) against exact sums and fp64 moments.  `pytest -m gpu`.

Every case is ONE call of eemflow_voxelize_trilinear_many on inputs of its own, written into the middle of a sentinel-filled allocation
whose guards must come back bitwise; it asserts by `eemflow_voxelize_last_form` which launch sequence ran (restated from the plan below,
never read back from the library) and holds the grid to criteria that follow from the arithmetic (tests/dsec_reference.py):
  * raw grid, banded AND direct (fp64 atomics) form: every occupied cell is bitwise fp32(exact sum of its fp32 votes) - either fp32
    neighbour only where the exact sum lies within k 2^-53 sum|w| of a rounding tie, taken on at most 1e-3 of a case's occupied cells;
    every other cell +0.0;
  * normalised grid: the criterion of tests/test_gpu_vox_fp64.py (oracle/fp64_bounds.py: vox_check_normalised) - against fp64
    (v - m) / sd of the GPU's OWN raw grid, the moment bounds of K cells folded per thread in fp32 carried through; zeros stay zero;
  * several sets per call: each grid bitwise the single call's; rectified int16 / int32 input: bitwise the float path on
    map[y, x] gathered by torch;
  * the Python layer: bitwise the ABI's grids; argument errors raise; the 16-bit flow round trip is exact for multiples of 1/128.
Every set carries the quirks: coordinates in (-1.5, W + 0.5) (x0 + 1 == W, y0 + 1 == H, negative x and y with their negative
weights), unsorted t with events before t[0] (tn < 0, b0 == -1 included) and after t[n-1] (b0 >= C), the last event at tn == C - 1.

SHAPES, the smallest that reach each mechanism (the plan is vox_plan of oracle/fp64_bounds.py - voxel.hip's make_plan, which voxel_tri.hip
shares - with the binning kernel's own events per thread and four records per event):
  rows64      5 x 24 x 64: 24 bands of 64 pixels = one image row each, so the two rows of EVERY event fall into different bands; 3 000
              events = three binning blocks, block boundaries in mid-set
  odd         5 x 13 x 19: h w % 4 != 0 (scalar read-out), last band 55 of 64 pixels; 1 500 events, two blocks
  short_last  5 x 10 x 20: last band 8 of 64 pixels with the 16-byte read-out; 700 events, one block; also at a grid pointer 4 bytes
              off 16-byte alignment (read-out and vox_norm_kernel fall to their scalar paths)
  bins1       1 x 12 x 16: tn == 0 for every event, bin b0 + 1 == C always masked
  one_event, dt0: the grid is all +0.0, guards intact
  bins65      65 x 8 x 8: direct form by size;  rows64 with EEM_VOX_DIRECT=1: direct form by the switch
  e2          rows64's grid with 524 289 events: the first count at which the binning kernel takes two events per thread (8 192-record
              slabs, 96 KB of LDS); ~700 votes per cell
  dsec        15 x 480 x 640, E-RAFT's DSEC grid: 512 bands of 600 pixels x 15 bins = 70 KB of fp64 cells, the band kernel's 1024-thread
              form, 16 lanes per run; 3 000 events
  bt512       6 x 480 x 640: the same bands at 28 KB: the 512-thread form
  ragged      1, 2 and 32 sets per call, one of a single event, sets of one, two and three binning blocks
Every other shape runs the band kernel's 256-thread form with 64 lanes per run.

MEASURED (one AMD Instinct MI355X, gfx950; a record, these numbers set no limit): in every case and set, banded and direct, 0 occupied
cells differ from fp32(exact sum) - rows64 6 958 cells of which 673 lie AT a rounding tie (exact ties of two-vote cells: the fp64 sum is
exact there and rounds to even as fp32(exact) does), e2 7 680 cells with ~550 votes each, bins65 3 478 cells through the fp64 atomics.
Run time of this module alone: 30 s, of which 26 s are the process's first use of the GPU; the slowest test 0.5 s (e2, host reference
included).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dsec_reference as R
import eemflow_amd
from eemflow_amd import _lib, dsec
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = np.float32(-12345.678)
GUARD = 64

# name: (C, H, W, [events per set], seed, options)
CASES = {
    "rows64": (5, 24, 64, [3000], 11, {}),
    "odd": (5, 13, 19, [1500], 12, {}),
    "short_last": (5, 10, 20, [700], 13, {}),
    "short_last_misaligned": (5, 10, 20, [700], 13, {"misalign": True}),
    "bins1": (1, 12, 16, [500], 14, {}),
    "one_event": (5, 12, 16, [1], 15, {"zero": True}),
    "dt0": (5, 12, 16, [50], 16, {"dt0": True, "zero": True}),
    "bins65": (65, 8, 8, [2000], 17, {}),
    "rows64_direct": (5, 24, 64, [3000], 11, {"direct": True}),
    "e2": (5, 24, 64, [524289], 18, {}),
    "dsec": (15, 480, 640, [3000], 21, {}),
    "bt512": (6, 480, 640, [2000], 22, {}),
    "pair": (5, 13, 19, [1500, 40], 19, {}),
    "ragged32": (5, 10, 20, [1, 5, 100, 1024, 1025, 2049, 2500, 3] + [17 + 61 * i for i in range(24)], 20, {}),
}


def L():
    return _lib.lib()


def _sp():
    return _lib.current_stream_ptr(torch.device(DEV))


def last_form():
    buf = ctypes.create_string_buffer(160)
    _lib.check(L().eemflow_voxelize_last_form(buf, len(buf)))
    return buf.value.decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_events(seed, n, C, H, W, dt0=False):
    """x, y in (-1.5, W + 0.5) x (-1.5, H + 0.5); t unsorted in (0, 1) around t[0] = 0.1 and t[n-1] = 0.9, so about a tenth of the events
    lie before t[0] (tn down to -0.5 (C-1)/... : b0 = 0 with a negative right weight, and b0 = -1) and a tenth after t[n-1]."""
    r = np.random.default_rng(seed)
    x = r.uniform(-1.5, W + 0.5, n).astype(np.float32)
    y = r.uniform(-1.5, H + 0.5, n).astype(np.float32)
    t = r.uniform(-0.3, 1.0, n).astype(np.float32)
    t[0], t[-1] = np.float32(0.1), np.float32(0.9)
    p = r.integers(0, 2, n).astype(np.float32)
    if n >= 8:                                   # the quirks by hand as well: x = -0.5, x0 + 1 == W, y0 + 1 == H, negative y
        x[1], y[1] = -0.5, 3.0
        x[2], y[2] = W - 0.75, 2.25
        x[3], y[3] = 4.5, H - 0.5
        x[4], y[4] = 2.0, -0.25
    if dt0:
        t[:] = np.float32(0.5)
    return x, y, t, p


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per set of the case: ((x, y, t, p), exact) - computed once, shared by the modes, never written to."""
    C, H, W, ns, seed, opt = CASES[name]
    out = []
    for k, n in enumerate(ns):
        ev = make_events(seed * 100 + k, n, C, H, W, opt.get("dt0", False))
        out.append((ev, R.exact(*ev, C, H, W)))
    return out


def plan_of(ns, C, H, W, aligned=True, direct=False):
    """voxel_tri.hip's choice restated: None for the direct form, else vox_plan's bands with EPT 1 / 2 and lanes per run from the slab
    of 4096 EPT records."""
    blocks = lambda n, e: (n + 1024 * e - 1) // (1024 * e)        # noqa: E731
    P = B.vox_plan(1, C, H, W, aligned, direct)
    if P is None or any(blocks(n, 2) > 4096 for n in ns):
        return None
    P = dict(P)
    P["ept"] = 2 if blocks(max(ns), 1) > 512 else 1
    slab = 4096 * P["ept"]
    lanes_x10 = 40 if slab < 4 * P["nb"] else 17
    P["sgs"] = 2
    while P["sgs"] < 6 and (1 << P["sgs"]) * 10 * P["nb"] < lanes_x10 * slab:
        P["sgs"] += 1
    return P


def form_of(P, k, normalize, xy=""):
    if P is None:
        return f"tri:j1:direct64{xy}+finish" + ("+norm" if normalize else "")
    return (f"tri:j{k}:bin_e{P['ept']}{xy}+band{P['bt']}_{'v4' if P['vec4'] else 'v1'}_s{P['sgs']}_" + ("raw_sums+norm" if normalize else "raw"))


def call(sets, C, H, W, normalize, misalign=False, maps=None, xy_type=0):
    """ONE ABI call into sentinel-guarded allocations; returns (form, [host grid per set]) after checking the guards."""
    total = C * H * W
    off = GUARD + (1 if misalign else 0)
    k = len(sets)
    bufs = [torch.full((off + total + GUARD,), float(SENTINEL), device=DEV) for _ in sets]
    ptrs = [b.data_ptr() + 4 * off for b in bufs]
    assert all((q % 16 == 0) != misalign for q in ptrs)
    arr = ctypes.c_void_p * k
    cols = [arr(*[s[j].data_ptr() for s in sets]) for j in range(4)]
    mp = arr(*[m.data_ptr() for m in maps]) if maps is not None else None
    mh, mw = (maps[0].shape[0], maps[0].shape[1]) if maps is not None else (0, 0)
    _lib.check(L().eemflow_voxelize_trilinear_many(k, cols[0], cols[1], cols[2], cols[3], (ctypes.c_int64 * k)(*[s[2].shape[0] for s in sets]),
                                                   xy_type, mp, mh, mw, C, H, W, normalize, arr(*ptrs), _sp()))
    form = last_form()
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        host = b.cpu().numpy()
        assert bool((_bits(host[:off]) == _bits(SENTINEL)).all()), "the guard in front of the grid was written"
        assert bool((_bits(host[off + total:]) == _bits(SENTINEL)).all()), "the guard behind the grid was written"
        out.append(host[off:off + total].copy())
    return form, out


def upload(ev):
    return tuple(torch.from_numpy(a).to(DEV) for a in ev)


def run_case(name, normalize, monkeypatch):
    C, H, W, ns, seed, opt = CASES[name]
    monkeypatch.delenv("EEM_VOX_DIRECT", raising=False)
    if opt.get("direct"):
        monkeypatch.setenv("EEM_VOX_DIRECT", "1")
    P = plan_of(ns, C, H, W, aligned=not opt.get("misalign"), direct=bool(opt.get("direct")))
    sets = [upload(ev) for ev, _ in reference(name)]
    form, grids = call(sets, C, H, W, normalize, misalign=bool(opt.get("misalign")))
    assert form == form_of(P, len(ns), normalize), f"{name}: launch sequence {form!r}"
    return P, form, grids


@pytest.mark.parametrize("name", list(CASES))
def test_raw_grid_is_the_exact_sum_rounded_once(monkeypatch, name):
    C, H, W, ns, seed, opt = CASES[name]
    P, form, grids = run_case(name, 0, monkeypatch)
    for k, (got, (ev, E)) in enumerate(zip(grids, reference(name))):
        differ, near = R.check_rounded_once(f"{name}[{k}] {form}", got, E)
        print(f"{name}[{k}] {form}: {len(E['cells'])} occupied cells, {differ} differ from fp32(exact), {near} at a tie")
        if opt.get("zero"):
            assert len(E["cells"]) == 0 and np.count_nonzero(_bits(got)) == 0


def test_the_shapes_reach_what_they_are_for():
    P = plan_of([3000], 5, 24, 64)
    assert P["band_px"] == 64 and P["nb"] == 24 and P["ept"] == 1                # one image row per band
    P = plan_of([1500], 5, 13, 19)
    assert not P["vec4"] and P["last_px"] == 55
    P = plan_of([700], 5, 10, 20)
    assert P["vec4"] and P["last_px"] == 8
    assert not plan_of([700], 5, 10, 20, aligned=False)["vec4"]
    assert plan_of([2000], 65, 8, 8) is None and plan_of([3000], 5, 24, 64, direct=True) is None
    assert plan_of([524288], 5, 24, 64)["ept"] == 1 and plan_of([524289], 5, 24, 64)["ept"] == 2
    P = plan_of([3000], 15, 480, 640)
    assert (P["bt"], P["band_px"], P["sgs"]) == (1024, 600, 4) and plan_of([2000], 6, 480, 640)["bt"] == 512
    for name in ("rows64", "odd", "e2"):                                        # the quirks are in the sets
        C, H, W = CASES[name][:3]
        (x, y, t, p), E = reference(name)[0]
        idx, w, m = R.votes(x, y, t, p, C, H, W)
        tn = np.float32(C - 1) * (t - t[0]) / (t[-1] - t[0])
        assert bool((w[m] < 0).any()) and bool(((x.astype(np.int64) + 1 == W) & (x > 0)).any()) and bool(((y.astype(np.int64) + 1 == H) & (y > 0)).any())
        assert bool((tn < -1).any()) and bool(((tn > -1) & (tn < 0)).any()) and bool((tn > C - 1).any()) and tn[-1] == C - 1
        assert bool((x < 0).any()) and bool((y < 0).any())


@pytest.mark.parametrize("name", ["rows64", "odd", "short_last", "short_last_misaligned", "bins1", "dt0", "bins65", "rows64_direct", "e2", "dsec", "bt512", "pair"])
def test_normalised_grid_against_fp64_of_the_raw_grid(monkeypatch, name):
    C, H, W, ns, seed, opt = CASES[name]
    P, _, raws = run_case(name, 0, monkeypatch)
    P, form, grids = run_case(name, 1, monkeypatch)
    K = P["K"] if P else 1
    for k, (got, raw) in enumerate(zip(grids, raws)):
        M = B.vox_check_normalised(f"{name}[{k}]", got, raw, K, form)
        if opt.get("zero"):
            assert np.count_nonzero(_bits(got)) == 0
        else:
            assert M["any"] and M["scale"]


@pytest.mark.parametrize("name", ["pair", "ragged32"])
@pytest.mark.parametrize("normalize", [0, 1])
def test_sets_of_one_call_are_bitwise_the_single_calls(monkeypatch, name, normalize):
    C, H, W, ns, seed, opt = CASES[name]
    P, form, grids = run_case(name, normalize, monkeypatch)
    assert form.startswith(f"tri:j{len(ns)}:")
    for k, (ev, E) in enumerate(reference(name)):
        f1, one = call([upload(ev)], C, H, W, normalize)
        assert f1 == form_of(plan_of([ns[k]], C, H, W), 1, normalize)
        assert np.array_equal(_bits(one[0]), _bits(grids[k])), f"{name}: set {k} ({ns[k]} events) differs from its single call"


@pytest.mark.parametrize("dtype,xy,code", [(torch.int16, "_i16", 1), (torch.int32, "_i32", 2)])
@pytest.mark.parametrize("direct", [False, True])
def test_fused_rectification_is_bitwise_the_float_path(monkeypatch, dtype, xy, code, direct):
    C, H, W, n, Hm, Wm = 5, 13, 19, 1500, 10, 14
    monkeypatch.delenv("EEM_VOX_DIRECT", raising=False)
    if direct:
        monkeypatch.setenv("EEM_VOX_DIRECT", "1")
    r = np.random.default_rng(31)
    rmap = np.stack([r.uniform(-1.5, W + 0.5, (Hm, Wm)), r.uniform(-1.5, H + 0.5, (Hm, Wm))], axis=2).astype(np.float32)
    xr, yr = r.integers(-1, Wm + 1, n), r.integers(-1, Hm + 1, n)            # some raw coordinates outside the map
    xr[[0, -1]], yr[[0, -1]] = 3, 4                                          # t[0] and t[n-1] set the scale: keep them in both paths
    _, _, t, p = make_events(32, n, C, H, W)
    inside = (xr >= 0) & (xr < Wm) & (yr >= 0) & (yr < Hm)
    assert 0 < int((~inside).sum()) < n // 2
    P = plan_of([n], C, H, W, direct=direct)
    dmap = torch.from_numpy(rmap).to(DEV)
    raw = (torch.from_numpy(xr).to(DEV, dtype), torch.from_numpy(yr).to(DEV, dtype), torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV))
    keep = torch.from_numpy(inside).to(DEV)
    xy_f = dmap[raw[1][keep].long(), raw[0][keep].long()]                    # torch indexing, then the float path
    flt = (xy_f[:, 0].contiguous(), xy_f[:, 1].contiguous(), raw[2][keep].contiguous(), raw[3][keep].contiguous())
    for normalize in (0, 1):
        form, fused = call([raw], C, H, W, normalize, maps=[dmap], xy_type=code)
        assert form == form_of(P, 1, normalize, xy)
        form, plain = call([flt], C, H, W, normalize)
        assert form == form_of(P, 1, normalize)
        assert np.array_equal(_bits(fused[0]), _bits(plain[0]))
    E = R.exact(rmap[yr[inside], xr[inside], 0], rmap[yr[inside], xr[inside], 1], t[inside], p[inside], C, H, W)
    R.check_rounded_once(f"rectified{xy}", call([raw], C, H, W, 0, maps=[dmap], xy_type=code)[1][0], E)


def test_refused_calls_launch_nothing_and_keep_the_form(monkeypatch):
    monkeypatch.delenv("EEM_VOX_DIRECT", raising=False)
    ev = upload(make_events(1, 16, 5, 12, 16))
    call([ev], 5, 12, 16, 0)
    before = last_form()
    grid = torch.full((5 * 12 * 16,), float(SENTINEL), device=DEV)
    arr = ctypes.c_void_p * 1
    cols = [arr(c.data_ptr()) for c in ev]

    def refused(n=16, xy_type=0, maps=None, bins=5, normalize=0, nsets=1):
        return L().eemflow_voxelize_trilinear_many(nsets, cols[0], cols[1], cols[2], cols[3], (ctypes.c_int64 * 1)(n), xy_type, maps, 4, 4, bins,
                                                   12, 16, normalize, arr(grid.data_ptr()), _sp()) != 0
    assert refused(n=0) and refused(xy_type=1) and refused(xy_type=7) and refused(bins=0) and refused(normalize=2) and refused(nsets=0)
    assert refused(nsets=33) and refused(maps=arr(grid.data_ptr()))                      # fp32 coordinates with a map
    torch.cuda.synchronize()
    assert bool((_bits(grid.cpu().numpy()) == _bits(SENTINEL)).all()) and last_form() == before


# ----------------------------------------------------------------------------------------------------------------------- the Python layer
def _dicts(name):
    return [dict(zip("xytp", upload(ev))) for ev, _ in reference(name)]


def test_python_layer_is_bitwise_the_abi(monkeypatch):
    monkeypatch.delenv("EEM_VOX_DIRECT", raising=False)
    assert eemflow_amd.VoxelGrid is dsec.VoxelGrid and eemflow_amd.voxelize_windows is dsec.voxelize_windows
    C, H, W, ns, seed, opt = CASES["pair"]
    evs = _dicts("pair")
    for normalize in (False, True):
        _, want = call([tuple(e[k] for k in "xytp") for e in evs], C, H, W, int(normalize))
        g = dsec.VoxelGrid((C, H, W), normalize).convert(evs[0])
        assert g.shape == (C, H, W) and g.dtype == torch.float32 and g.is_cuda
        assert np.array_equal(_bits(g.cpu().numpy().reshape(-1)), _bits(want[0]))
        many = dsec.voxel_grid_many(evs, (C, H, W), normalize)
        out = [torch.empty(C, H, W, device=DEV) for _ in evs]
        assert dsec.voxel_grid_many(evs, (C, H, W), normalize, out=out)[1] is out[1]
        for a, b, w in zip(many, out, want):
            assert np.array_equal(_bits(a.cpu().numpy().reshape(-1)), _bits(w)) and torch.equal(a, b)


def test_voxelize_windows_both_edge_forms(monkeypatch):
    monkeypatch.delenv("EEM_VOX_DIRECT", raising=False)
    C, H, W, n = 5, 13, 19, 4000
    x, y, _, p = make_events(41, n, C, H, W)
    t = np.sort(np.random.default_rng(42).uniform(0, 1, n)).astype(np.float32)
    ev = dict(zip("xytp", upload((x, y, t, p))))
    offsets = [0, 700, 701, 2500, 4000]                                       # a one-event window among them: all zeros
    by_off = dsec.voxelize_windows(ev, (C, H, W), offsets=offsets, normalize=True)
    assert last_form().startswith("tri:j4:")
    edges = [float(t[0])] + [float(t[o]) for o in offsets[1:-1]] + [2.0]
    assert np.searchsorted(t, np.array(edges, np.float32)).tolist() == offsets
    by_t = dsec.voxelize_windows(ev, (C, H, W), t_edges=edges, normalize=True)
    assert len(by_off) == 4 and all(g.shape == (1, C, H, W) for g in by_off)
    for k, (a, b) in enumerate(zip(offsets, offsets[1:])):
        _, want = call([tuple(ev[c][a:b] for c in "xytp")], C, H, W, 1)
        assert np.array_equal(_bits(by_off[k].cpu().numpy().reshape(-1)), _bits(want[0])) and torch.equal(by_off[k], by_t[k])
    assert not bool(by_off[1].any())


def test_python_layer_refuses_bad_arguments():
    C, H, W = 5, 12, 16
    ev = dict(zip("xytp", upload(make_events(1, 16, C, H, W))))
    vg = dsec.VoxelGrid((C, H, W), True)
    with pytest.raises(_lib.EEMFlowHipError):
        vg.convert({k: v.cpu() for k, v in ev.items()})                       # no CPU path
    with pytest.raises(TypeError):
        vg.convert(dict(ev, t=ev["t"].double()))                              # the reference raises on float64 too
    with pytest.raises(TypeError):
        vg.convert(dict(ev, x=ev["x"].int()))
    with pytest.raises(ValueError):
        vg.convert({k: v[:0] for k, v in ev.items()})                         # empty
    with pytest.raises(ValueError):
        vg.convert(dict(ev, p=ev["p"][:5]))                                   # mismatched lengths
    with pytest.raises(ValueError):
        vg.convert({"x": ev["x"]})
    with pytest.raises(ValueError):
        dsec.voxel_grid_many([ev] * 33, (C, H, W))
    with pytest.raises(ValueError):
        dsec.voxel_grid_many([ev], (C, H, W), out=[torch.empty(C, H, W + 1, device=DEV)])
    with pytest.raises(TypeError):
        dsec.voxel_grid_many([ev], (C, H, W), rectify_maps=torch.zeros(4, 4, 2, device=DEV))      # a map needs raw integer coordinates
    with pytest.raises(ValueError):
        dsec.voxelize_windows(ev, (C, H, W))
    with pytest.raises(ValueError):
        dsec.voxelize_windows(ev, (C, H, W), offsets=[0, 4, 4, 16])           # an empty window
    with pytest.raises(ValueError):
        dsec.voxelize_windows(ev, (C, H, W), offsets=[0, 17])


def test_flow_16bit_round_trip_and_golden():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsec_voxel_flow16.npz"))
    flow, valid = dsec.flow_16bit_to_float(z["flow_16bit"])
    assert flow.dtype == torch.float64 and valid.dtype == torch.bool and flow.is_cuda
    assert np.array_equal(flow.cpu().numpy(), z["flow"]) and np.array_equal(valid.cpu().numpy(), z["valid"])
    back = dsec.flow_float_to_16bit(flow, valid)
    want = z["flow_16bit"].astype(np.int32) * z["valid"][..., None]                           # invalid pixels: all zero
    assert np.array_equal(back.cpu().numpy(), want)
    r = np.random.default_rng(5)
    exact = torch.from_numpy(r.integers(-32768, 32768, (7, 5, 2)) / 128.0).to(DEV)            # every multiple of 1/128 in range
    ok = torch.from_numpy(r.integers(0, 2, (7, 5)).astype(bool)).to(DEV)
    f2, v2 = dsec.flow_16bit_to_float(dsec.flow_float_to_16bit(exact, ok))
    assert torch.equal(v2, ok) and torch.equal(f2, exact * ok[..., None])
    assert dsec.flow_float_to_16bit(torch.tensor([[[1e9, -1e9]]], device=DEV), torch.ones(1, 1, dtype=torch.bool, device=DEV)).tolist() == [[[65535, 0, 1]]]
    bad = z["flow_16bit"].copy()
    bad[1, 1, 2] = 2
    with pytest.raises(ValueError):
        dsec.flow_16bit_to_float(bad)
    with pytest.raises(ValueError):
        dsec.flow_16bit_to_float(z["flow_16bit"].astype(np.int32))
    with pytest.raises(ValueError):
        dsec.flow_16bit_to_float(torch.zeros(4, 4, 2, dtype=torch.int32, device=DEV))
