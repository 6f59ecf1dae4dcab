"""Every launch form of the voxelizer (voxel.hip) against exact sums and fp64 moments.  `pytest -m gpu`.

voxel.hip turns events into the grids every model and all of training consume.  Every case here (oracle/fp64_bounds.py: VOX_CASES) is ONE
call of eemflow_voxelize or eemflow_voxelize_many on inputs of its own; it asserts by `eemflow_voxelize_last_form` which launch sequence
ran (the binning kernel's events per thread, the band kernel's block size, vec4, lanes per run and mode, what followed, the job count)
and holds every output to a criterion that follows from the arithmetic (derived beside the functions in fp64_bounds.py, none fitted):
  * index outputs: equal to vox_votes, the reference's integer work restated, -1 where it masks a vote;
  * raw grid, banded path: every occupied cell is the fp64 sum of its votes (vox_exact) rounded to fp32 ONCE, bit for bit; either fp32
    neighbour where the fp64 sum has an error-free residual, on at most 1e-3 of a case's occupied cells (no cell of any case has one);
    every other cell is +0.0;
  * dyadic inputs (integer timestamps in [0, 2^20]: all partial sums exact, in fp32 too below 8 votes per cell): banded AND direct path
    bitwise the exact sum, cells where +1 and -1 votes cancel to 0 included - they count as zero voxels in the moments;
  * raw grid, direct path, generic inputs: votes - 1 roundings against sum |votes| (check_counted), four runs (atomics in any order);
  * deferred record {mean, sd, scale, any}, directly behind the grid: against fp64 moments of the GPU's own raw grid with the bound of K
    cells folded per thread in fp32 (K from vox_plan; 1 for the direct path's fp64 moments); flags exact, sd = 1 where scale is 0;
  * normalised grids (norm pass, and the two band passes of EEM_VOX_TWOPASS): against fp64 (v - m) / sd of the raw grid the same path is
    held to bit for bit above, two roundings plus the moment bounds carried through; zero voxels stay zero;
  * the norm pass, the two band passes and (v - mean) / sd applied in fp32 on the host to the deferred record: bitwise equal.
Every grid is written into the middle of a sentinel-filled allocation whose guards must come back bitwise (the record's guard directly
behind it), also at a pointer 4 bytes off 16-byte alignment (vec4 and vox_norm_kernel's vector path off).
tests/test_fp64_bounds_vox.py shows on the CPU that these checks reject ten planted faults and that the inputs keep their conditions.

FORMS REACHED (VOX_FORMS, 40 sequences): BT 256 / 512 / 1024; vec4 on, off by h w % 4 and off by the pointer; EPT 1, 2, 4, 8 at 524 288,
524 289, 1 048 577 and 2 097 153 events on 33 bands of 64 pixels (runs of up to 250 records for 64 lanes: the clean-up loop); sgs 3 .. 6
(sgs = 2 is unreachable: it needs nb >= 1024 EPT bands, or nb >= 436 EPT with nb <= 256 EPT; nb <= 1023); a last band shorter than
band_px in both read-out forms; events at t_last, x >= w, y >= h, y < 0 with the t2 == -1 branch and votes that leave the grid; one event,
dT = 0, one non-zero voxel (sd NaN), an all-equal grid (sd 0), bins = 1; EEM_VOX_DIRECT=1 and the two shapes that fall to the direct
kernel by size (304 pixels x 64 bins > 19 200 cells; 65 bins); 1, 2 and 32 ragged sets per call (one of a single event, sets of one, two
and three binning blocks), each set held to the single call's criteria.
LEFT OUT: EEM_VOX_BAND_FLOATS (read once per process; the shapes reach every BT without it), the EEM_VOX_STAMPS build, more than 33.5 M
events (the third route to the direct kernel: 1 GiB of events), event_pack.hip and augment.hip (their own modules).

MEASURED (one AMD Instinct MI355X, gfx950; a record, these numbers set no limit).  The worst share of each bound over all cases of a
path and mode; "differ": occupied cells whose bits differ from the exact sum rounded once.
  path / mode : check                        of bound  mean share  sd share  cells differ  with residual  checks
  band1024_v4/deferred:exact                  0.00e+00    0.00e+00  0.00e+00             0              0       2
  band1024_v4/deferred:record                 5.72e-03    6.29e-04  5.72e-03             0              0       2
  band1024_v4/norm:normalised                 8.16e-02    0.00e+00  0.00e+00             0              0       2
  band1024_v4/raw:exact                       0.00e+00    0.00e+00  0.00e+00             0              0       1
  band1024_v4/twopass:normalised              8.16e-02    0.00e+00  0.00e+00             0              0       1
  band256_v1/deferred:exact                   0.00e+00    0.00e+00  0.00e+00             0              0       7
  band256_v1/deferred:record                  3.02e-01    3.11e-02  3.02e-01             0              0       7
  band256_v1/norm:normalised                  2.68e-01    0.00e+00  0.00e+00             0              0       7
  band256_v1/raw:exact                        0.00e+00    0.00e+00  0.00e+00             0              0       4
  band256_v1/twopass:normalised               2.68e-01    0.00e+00  0.00e+00             0              0       7
  band256_v4/deferred:exact                   0.00e+00    0.00e+00  0.00e+00             0              0      40
  band256_v4/deferred:record                  9.66e-02    1.12e-02  9.66e-02             0              0      40
  band256_v4/norm:normalised                  1.43e-01    0.00e+00  0.00e+00             0              0      35
  band256_v4/raw:exact                        0.00e+00    0.00e+00  0.00e+00             0              0      35
  band256_v4/twopass:normalised               1.02e-01    0.00e+00  0.00e+00             0              0       4
  band512_v4/deferred:exact                   0.00e+00    0.00e+00  0.00e+00             0              0       2
  band512_v4/deferred:record                  1.06e-02    2.27e-03  1.06e-02             0              0       2
  band512_v4/norm:normalised                  8.64e-02    0.00e+00  0.00e+00             0              0       2
  band512_v4/raw:exact                        0.00e+00    0.00e+00  0.00e+00             0              0       2
  band512_v4/twopass:normalised               8.64e-02    0.00e+00  0.00e+00             0              0       2
  direct/deferred:counted                     1.00e+00    0.00e+00  0.00e+00             0              0      10
  direct/deferred:exact                       0.00e+00    0.00e+00  0.00e+00             0              0       3
  direct/deferred:record                      3.53e-01    9.40e-02  3.53e-01             0              0      13
  direct/norm:normalised                      5.43e-01    0.00e+00  0.00e+00             0              0       7
  direct/raw:counted                          1.00e+00    0.00e+00  0.00e+00             0              0       4
  direct/raw:exact                            0.00e+00    0.00e+00  0.00e+00             0              0       2
The counted bound of a cell with two votes is a single rounding: tight by construction (1.00).
Run time of this module alone: 30 s, of which 25 s are the process's first use of the GPU (library and context); the 90 tests take 4.5 s,
the slowest 0.8 s (2 097 153 events, host reference included).
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from eemflow_amd import _lib
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = np.float32(-12345.678)
IDX_SENTINEL = -77
GUARD = 64                   # floats (and int64 indices) on either side of an output: the grid keeps the allocation's 16-byte alignment
SEEN = set()
CASE_MODES = [(name, mode) for name, case in B.VOX_CASES.items() for mode in case[5]]
DIRECT_RUNS = 4              # the fp32 atomics' order changes from run to run


def L():
    return _lib.lib()


def _sp():
    return _lib.current_stream_ptr(torch.device(DEV))


def _pin(monkeypatch, direct=False, twopass=False):
    assert "EEM_VOX_BAND_FLOATS" not in os.environ, "EEM_VOX_BAND_FLOATS is read once per process: the shapes here assume the default bands"
    for name in ("EEM_VOX_DIRECT", "EEM_VOX_TWOPASS"):
        monkeypatch.delenv(name, raising=False)
    if direct:
        monkeypatch.setenv("EEM_VOX_DIRECT", "1")
    if twopass:
        monkeypatch.setenv("EEM_VOX_TWOPASS", "1")


def last_form():
    buf = ctypes.create_string_buffer(128)
    _lib.check(L().eemflow_voxelize_last_form(buf, len(buf)))
    return buf.value.decode()


@functools.lru_cache(maxsize=2)
def reference(name):
    """Per event set of the case: (events, vox_votes, vox_exact) - computed once, shared by the case's modes, never written to."""
    kind, n, h, w, bins, modes, opt = B.VOX_CASES[name]
    out = []
    for ev in B.vox_case_events(name):
        V = B.vox_votes(ev, bins, h, w)
        out.append((ev, V, B.vox_exact(ev, bins, h, w, V)))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def voxelize(name, mode, monkeypatch):
    """ONE ABI call of the case in the mode; asserts the reported form and the guards.  Per set: [grid, record or None, il, ir] (il, ir: the
    index outputs of a single call, else None)."""
    kind, n, h, w, bins, modes, opt = B.VOX_CASES[name]
    many = isinstance(n, list)
    _pin(monkeypatch, opt.get("direct", False), mode == "twopass")
    normalize = B.VOX_MODE_NORMALIZE[mode]
    total, nrec = bins * h * w, (4 if normalize == 2 else 0)
    off = GUARD + (1 if opt.get("misalign") else 0)
    evs = [torch.from_numpy(ev).to(DEV) for ev, _, _ in reference(name)]
    bufs = [torch.full((off + total + nrec + GUARD,), float(SENTINEL), device=DEV) for _ in evs]
    ptrs = [b.data_ptr() + 4 * off for b in bufs]
    assert all((p % 16 == 0) != bool(opt.get("misalign")) and e.data_ptr() % 16 == 0 for p, e in zip(ptrs, evs))
    idx = None
    if many:
        k = len(evs)
        arr = ctypes.c_void_p * k
        _lib.check(L().eemflow_voxelize_many(k, arr(*[e.data_ptr() for e in evs]), (ctypes.c_int64 * k)(*[e.shape[0] for e in evs]), bins, h, w,
                                             normalize, arr(*ptrs), _sp()))
    else:
        # (only the single call has index outputs)
        idx = [torch.full((evs[0].shape[0] + 2 * GUARD,), IDX_SENTINEL, dtype=torch.int64, device=DEV) for _ in range(2)]
        _lib.check(L().eemflow_voxelize(evs[0].data_ptr(), evs[0].shape[0], bins, h, w, normalize, ptrs[0],
                                        idx[0].data_ptr() + 8 * GUARD, idx[1].data_ptr() + 8 * GUARD, _sp()))
    form = last_form()
    torch.cuda.synchronize()
    plan, want = B.vox_case_form(name, mode)
    assert form == want, f"{name} {mode}: launch sequence {form!r}, expected {want!r}"
    assert form in B.VOX_FORMS
    SEEN.add(form)
    out = []
    for b in bufs:
        host = b.cpu().numpy()
        assert bool((_bits(host[:off]) == _bits(SENTINEL)).all()), f"{name} {mode}: the guard in front of the grid was written"
        assert bool((_bits(host[off + total + nrec:]) == _bits(SENTINEL)).all()), f"{name} {mode}: the guard behind the grid was written"
        out.append([host[off:off + total], host[off + total:off + total + 4] if nrec else None, None, None])
    if idx:
        for j in (0, 1):
            host = idx[j].cpu().numpy()
            assert bool((host[:GUARD] == IDX_SENTINEL).all()) and bool((host[-GUARD:] == IDX_SENTINEL).all()), f"{name}: index guard written"
            out[0][2 + j] = host[GUARD:-GUARD]
    return plan, form, out


def label(plan, mode):
    return (f"band{plan['bt']}_{'v4' if plan['vec4'] else 'v1'}" if plan else "direct") + "/" + mode


def hold(name, mode, plan, got, rec, il, ir, V, E):
    """Every criterion of the mode on one set's outputs."""
    kind = B.VOX_CASES[name][0]
    generic = kind in ("clustered", "hostile")
    K = plan["K"] if plan else 1
    lab = label(plan, mode)
    if il is not None:
        B.vox_check_indices(name, il, ir, V, lab)
    if mode in ("raw", "deferred"):
        if plan is None and generic:
            B.vox_check_raw_counted(f"{name}.grid", got, E, lab)
        else:
            B.vox_check_raw_exact(f"{name}.grid", got, E, lab, allow_residual=generic)
        if mode == "deferred":
            B.vox_check_record(f"{name}.record", rec, got, K, lab)
        return
    # normalised: against the raw grid the same path is held to bit for bit in its raw modes - the exact sums rounded once
    assert not bool((E["res"] != 0).any()), "a normalised case needs an input whose raw grid is decided bit for bit"
    assert plan is not None or not generic or int(E["count"].max()) <= 1
    B.vox_check_normalised(f"{name}.grid", got, B.vox_dense(E).astype(np.float32), K, lab)


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_voxelizer_form(monkeypatch, name, mode):
    kind, n, h, w, bins, modes, opt = B.VOX_CASES[name]
    runs = DIRECT_RUNS if opt.get("direct") and kind in ("clustered", "hostile") else 1
    for _ in range(runs):
        plan, form, sets = voxelize(name, mode, monkeypatch)
        for (got, rec, il, ir), (ev, V, E) in zip(sets, reference(name)):
            hold(name, mode, plan, got, rec, il, ir, V, E)


@pytest.mark.parametrize("name", [n for n, c in B.VOX_CASES.items() if "deferred" in c[5] and "norm" in c[5]])
def test_normalised_forms_are_bitwise_the_record_applied(monkeypatch, name):
    """The norm pass, the two band passes and (v - mean) / sd applied in fp32 to the raw grid with the deferred record: the same moments,
    the same expression, the same bits."""
    modes = B.VOX_CASES[name][5]
    _, _, deferred = voxelize(name, "deferred", monkeypatch)
    _, _, norm = voxelize(name, "norm", monkeypatch)
    two = voxelize(name, "twopass", monkeypatch)[2] if "twopass" in modes else None
    for k, ((raw, rec, _, _), (got, _, _, _)) in enumerate(zip(deferred, norm)):
        want = B.vox_normalise_f32(raw, rec)
        B.check_bitwise(f"{name}[{k}] norm pass against the record applied", torch.from_numpy(got.copy()), torch.from_numpy(want))
        if two is not None:
            B.check_bitwise(f"{name}[{k}] two band passes against the norm pass", torch.from_numpy(two[k][0].copy()), torch.from_numpy(got.copy()))


def test_last_form_refuses_bad_arguments_and_survives_a_refused_call(monkeypatch):
    _pin(monkeypatch)
    voxelize("one_event", "raw", monkeypatch)
    before = last_form()
    assert L().eemflow_voxelize_last_form(None, 8) != 0
    ev = torch.zeros(4, 4, dtype=torch.float64, device=DEV)
    grid = torch.zeros(8, device=DEV)
    assert L().eemflow_voxelize(ev.data_ptr(), 0, 2, 2, 2, 0, grid.data_ptr(), None, None, _sp()) != 0          # no events: refused
    assert last_form() == before
    small = ctypes.create_string_buffer(6)
    _lib.check(L().eemflow_voxelize_last_form(small, len(small)))
    assert small.value.decode() == before[:5]


# ----------------------------------------------------------------------------------------------------------------------- the table
def test_every_form_in_the_table_ran():
    """Runs last: every sequence of VOX_FORMS was reported by a call above; prints the measured worst share of each bound per form."""
    agg = {}
    for rec in B.LOG:
        f = rec.get("form", "?")
        if not f.startswith(("band", "direct")):
            continue
        a = agg.setdefault(f, {"of_bound": 0.0, "mean_share": 0.0, "sd_share": 0.0, "differ": 0, "inexact": 0, "checks": 0})
        a["checks"] += 1
        a["differ"] += rec.get("differ", 0)
        a["inexact"] += rec.get("inexact", 0)
        for key in ("of_bound", "mean_share", "sd_share"):
            v = rec.get(key, 0.0)
            if isinstance(v, float) and math.isfinite(v):
                a[key] = max(a[key], abs(v))
    print("\n  path / mode : check                        of bound  mean share  sd share  cells differ  with residual  checks")
    for f in sorted(agg):
        a = agg[f]
        print(f"  {f:42s} {a['of_bound']:9.2e} {a['mean_share']:11.2e} {a['sd_share']:9.2e} {a['differ']:13d} {a['inexact']:14d} {a['checks']:7d}")
    assert SEEN == B.VOX_FORMS, (sorted(B.VOX_FORMS - SEEN), sorted(SEEN - B.VOX_FORMS))
