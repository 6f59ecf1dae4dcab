"""tests/dsec_reference.py against what the reference's own VoxelGrid.convert and flow_16bit_to_float returned (tests/golden/dsec_voxel_*.npz,
written by tools/make_dsec_goldens.py), and the checks against planted faults.  No GPU.

The reference sums a cell's votes in fp32 in an order of its own (put_ with accumulate), so an occupied cell of a golden grid is held to
|golden - exact| <= (k - 1) 2^-24 sum|w| (k votes: k - 1 roundings of partial sums below sum|w|) - exact where a cell has one vote - and
every other cell to +0.0.  Measured: the worst cell at 0.94 of that bound on the `random` fixture (233 occupied cells, up to 3 votes), 0.55 on `edges`."""
import os

import numpy as np
import pytest

import dsec_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = ("random", "edges", "dt0")


def load(name):
    z = np.load(os.path.join(GOLDEN, f"dsec_voxel_{name}.npz"))
    C, H, W = (int(v) for v in z["shape"])
    return z, (z["x"], z["y"], z["t"], z["p"], C, H, W)


@pytest.mark.parametrize("name", SETS)
def test_restatement_reproduces_the_reference_grid(name):
    z, args = load(name)
    E = R.exact(*args)
    share = R.check_sequential(name, z["raw"], E)
    print(f"{name}: {len(E['cells'])} occupied cells, up to {int(E['count'].max()) if len(E['cells']) else 0} votes, worst share of the bound {share:.3f}")
    assert share <= 1.0


def test_fixtures_hold_what_they_are_for():
    z, (x, y, t, p, C, H, W) = load("random")
    assert x.min() < -1 and x.max() > W and y.min() < -1 and y.max() > H              # coordinates in (-1.5, W + 0.5)
    assert bool((np.diff(t) < 0).any()) and bool((t < t[0]).any()) and bool((t > t[-1]).any())    # unsorted; tn < 0 and tn > C - 1
    assert all(a.dtype == np.float32 for a in (x, y, t, p, z["raw"], z["normalised"]))
    E = R.exact(x, y, t, p, C, H, W)
    assert int((E["count"] == 1).sum()) > 50 and int(E["count"].max()) >= 3          # single votes (exact) and real sums
    z, (x, y, t, p, C, H, W) = load("dt0")
    assert t[0] == t[-1]


def test_truncation_gives_a_negative_weight():
    """x = -0.5 truncates to column 0: +0.5 there, -0.5 in column 1 (floor would give column -1, masked, and +0.5 in column 0)."""
    x, y = np.array([-0.5, 3.0], np.float32), np.array([4.0, 5.0], np.float32)
    t, p = np.array([0.0, 1.0], np.float32), np.array([1.0, 1.0], np.float32)
    E = R.exact(x, y, t, p, 2, 8, 8)
    g = R.dense(E).reshape(2, 8, 8)
    assert g[0, 4, 0] == 0.5 and g[0, 4, 1] == -0.5
    assert g[1, 5, 3] == 1.0 and np.count_nonzero(g) == 3       # the last event: tn == C - 1, one vote, nothing in bin C
    z, (x, y, t, p, C, H, W) = load("edges")
    assert x[1] == -0.5
    raw = z["raw"].reshape(C, H, W)
    tn = np.float32(C - 1) * (t[1] - t[0]) / (t[-1] - t[0])
    b0 = int(tn)
    assert raw[b0, 4, 0] == np.float32(0.5) * np.float32(1 - (tn - b0)) and raw[b0, 4, 1] == -raw[b0, 4, 0]


def test_dt_zero_drops_every_vote():
    z, args = load("dt0")
    _, _, mask = R.votes(*args)
    assert not bool(mask.any())
    assert np.count_nonzero(z["raw"].view(np.uint32)) == 0 and np.count_nonzero(z["normalised"].view(np.uint32)) == 0
    one = tuple(a[:1] for a in args[:4]) + args[4:]
    assert not bool(R.votes(*one)[2].any())                     # a single event is the same case


def test_out_of_range_values_are_dropped_whole():
    x = np.array([1.0, np.nan, np.inf, -3e9, 2.0, 2.0 ** 31, 5.0], np.float32)
    y = np.array([1.0, 1.0, 1.0, 1.0, np.nan, 1.0, 5.0], np.float32)
    t = np.linspace(0, 1, 7).astype(np.float32)
    p = np.ones(7, np.float32)
    _, _, mask = R.votes(x, y, t, p, 3, 8, 8)
    assert mask[:, 1:6].sum() == 0 and mask[:, 0].any() and mask[:, 6].any()


@pytest.mark.parametrize("name", SETS)
def test_normalised_goldens_against_fp64(name):
    """(v - m) / sd of the golden RAW grid in fp64 against the reference's fp32 normalisation: the mean and sd of c values carry c
    roundings at most, the expression two more; zeros stay zero."""
    z, _ = load(name)
    raw, got = z["raw"].astype(np.float64), z["normalised"].astype(np.float64)
    want = R.normalised_f64(raw)
    nz = raw != 0
    assert not bool(got[~nz].any())
    if nz.any():
        c = int(nz.sum())
        sd = raw[nz].std(ddof=1)
        bound = (c + 4) * 2.0 ** -24 * (np.abs(want[nz]) + np.abs(raw[nz]).max() / sd)
        assert bool((np.abs(got[nz] - want[nz]) <= bound).all())


@pytest.mark.parametrize("fault", R.FAULTS)
def test_checks_reject_planted_faults(fault):
    """A grid built with the fault - summed exactly, so the fault is all that is wrong with it - fails both criteria on the fixtures."""
    caught_seq = caught_once = False
    for name in ("random", "edges"):
        z, args = load(name)
        E = R.exact(*args)
        wrong = R.dense(R.exact(*args, fault=fault)).astype(np.float32)
        right = R.dense(E).astype(np.float32)
        R.check_rounded_once(name, right, E)                    # the faultless grid passes
        R.check_sequential(name, right, E)
        try:
            R.check_sequential(name, wrong, E)
        except AssertionError:
            caught_seq = True
        try:
            R.check_rounded_once(name, wrong, E)
        except AssertionError:
            caught_once = True
    assert caught_seq and caught_once


def test_rounded_once_accepts_a_neighbour_only_at_a_tie():
    E = {"cells": np.array([0, 1]), "sum": np.array([1.0 + 2.0 ** -24, 3.0]), "abs": np.array([2.0, 3.0]), "count": np.array([2, 1]), "total": 4}
    lo, hi = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    many = {k: (np.tile(v, 1000) if k != "total" else 4000) for k, v in E.items()}
    many["cells"] = np.arange(2000)
    many["sum"][2:] = 3.0                                         # one tie among 2000 cells: inside the cap
    many["abs"][2:], many["count"][2:] = 3.0, 1
    for v in (lo, hi):
        g = np.zeros(4000, np.float32)
        g[:2000] = 3.0
        g[0] = v
        R.check_rounded_once("tie", g, many)
    g[0] = np.nextafter(hi, np.float32(2.0))
    with pytest.raises(AssertionError):
        R.check_rounded_once("tie", g, many)
    R.check_rounded_once("tie", np.array([lo, 3.0, 0, 0], np.float32), E)       # at a tie, on its exact side: no exception taken
    with pytest.raises(AssertionError):                           # one of two cells takes the exception: over the cap
        R.check_rounded_once("tie", np.array([hi, 3.0, 0, 0], np.float32), E)


def test_flow_16bit_to_float_golden():
    z = np.load(os.path.join(GOLDEN, "dsec_voxel_flow16.npz"))
    flow, valid = R.flow_16bit_to_float(z["flow_16bit"])
    assert flow.dtype == np.float64 and np.array_equal(flow, z["flow"]) and np.array_equal(valid, z["valid"])
    assert tuple(flow[0, 0]) == (0.0, 1.0) and bool(valid[0, 0])
