"""Recordings cut into windows, host side (eemflow_amd/recording.py, `cli run`; no GPU): the window cutting on the raw t column, the
stable ordering of an unsorted recording, the command line's refusals, and the new entry point's declaration and binding."""
import os
import re

import numpy as np
import pytest

from eemflow_amd import _lib, cli, events as E, recording as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = np.array([100, 110, 110, 120, 135, 150, 150, 199], dtype=np.int64)       # ties ON the edges 110 and 150, nothing in [140, 150)


# ------------------------------------------------------------------------------------------------ window_offsets
def test_duration_windows_ties_on_an_edge_and_empty_windows():
    offs = R.window_offsets(T, window=10)
    # edges 100, 110, ..., 190 (floor(99 / 10) = 9 full windows); an event ON an edge belongs to the later window (side 'left')
    assert offs.dtype == np.int64 and offs.tolist() == [0, 1, 3, 4, 5, 5, 7, 7, 7, 7]
    assert offs[4] == offs[5]                                       # [140, 150) is empty, in the middle
    for k, (a, b) in enumerate(zip(offs, offs[1:])):
        lo, hi = 100 + 10 * k, 110 + 10 * k
        assert np.all((T[a:b] >= lo) & (T[a:b] < hi))
    kept = R.window_offsets(T, window=10, keep_partial=True)        # the trailing partial window: what follows the last edge
    assert kept.tolist() == offs.tolist() + [8] and T[kept[-2]:kept[-1]].tolist() == [199]
    assert R.window_offsets(T, window=1000).tolist() == [0] and R.window_offsets(T, window=1000, keep_partial=True).tolist() == [0, 8]


def test_duration_windows_of_a_float_column_and_of_nanosecond_integers():
    tf = T.astype(np.float64) * 0.25                                # (binary fractions: the edges t[0] + k * window are exact)
    assert R.window_offsets(tf, window=2.5).tolist() == R.window_offsets(T, window=10).tolist()
    base = 1700000000000000123                                      # above 2^53: a float64 search would round the edges
    big = np.array([0, 1, 2, 3, 4, 5, 6, 7], dtype=np.int64) + base
    assert R.window_offsets(big, window=2).tolist() == [0, 2, 4, 6]
    assert R.window_offsets(big, window=2.5).tolist() == [0, 3, 5]  # edges base + ceil(2.5 k): t >= e is t >= ceil(e) for integers
    assert R.window_offsets(big, t_edges=[base, base + 3, base + 3, base + 8]).tolist() == [0, 3, 3, 8]


def test_count_windows_and_explicit_edges():
    assert R.window_offsets(T, count=3).tolist() == [0, 3, 6]
    assert R.window_offsets(T, count=3, keep_partial=True).tolist() == [0, 3, 6, 8]
    assert R.window_offsets(T, count=4, keep_partial=True).tolist() == [0, 4, 8]           # no partial window to keep
    assert R.window_offsets(T, count=9).tolist() == [0]
    assert R.window_offsets(T, t_edges=[100, 110, 110.5, 150, 200]).tolist() == [0, 1, 3, 5, 8]
    assert R.window_offsets(T, t_edges=np.array([0, 1000])).tolist() == [0, 8]


@pytest.mark.parametrize("kw", [{}, {"window": 10, "count": 3}, {"window": 10, "t_edges": [0, 1]}, {"count": 1, "t_edges": [0, 1]},
                                {"window": 0}, {"window": -1.0}, {"count": 0}, {"count": 2.5}, {"t_edges": [5, 3]}, {"t_edges": []}])
def test_bad_argument_combinations(kw):
    with pytest.raises(ValueError):
        R.window_offsets(T, **kw)


def test_offsets_are_checked_against_the_recording():
    assert R._check_offsets("x", np.array([0, 3, 3, 8]), 8) == [0, 3, 3, 8]
    for bad in ([], [-1, 2], [0, 9], [3, 2]):
        with pytest.raises(ValueError):
            R._check_offsets("x", bad, 8)


# ------------------------------------------------------------------------------------------------ ordering
def test_an_unsorted_recording_is_argsorted_stably():
    rng = np.random.default_rng(5)
    n = 4000
    t = rng.integers(0, 50, n).astype(np.int64)                      # many ties, out of order
    x = np.arange(n, dtype=np.int32)                                 # the original position
    y = rng.integers(0, 64, n).astype(np.uint16)
    p = (2 * rng.integers(0, 2, n) - 1).astype(np.int8)
    (ts, xs, ys, ps), route = R.order_columns(t, x, y, p)
    assert route == 'host' and E.route_of((t, x, y, p)) == 'host'
    assert bool(np.all(ts[:-1] <= ts[1:]))
    same = ts[:-1] == ts[1:]
    assert same.any() and bool(np.all(xs[:-1][same] < xs[1:][same]))  # stable: events of one timestamp keep their order
    assert np.array_equal(ts, t[xs]) and np.array_equal(ys, y[xs]) and np.array_equal(ps, p[xs])
    assert (ts.dtype, xs.dtype, ys.dtype, ps.dtype) == (np.int64, np.int32, np.uint16, np.int8)
    (t2, x2, _, _), route2 = R.order_columns(ts, xs, ys, ps)         # in order: the columns go up as they are
    assert route2 == 'device' and t2 is ts and x2 is xs


def test_columns_the_kernels_cannot_read_are_refused():
    ok = (np.arange(4, dtype=np.int64), np.zeros(4, np.uint16), np.zeros(4, np.uint16), np.ones(4, np.int8))
    with pytest.raises(TypeError, match="float64"):
        R.order_columns(ok[0].astype(np.float32), *ok[1:])
    with pytest.raises(TypeError, match="column x"):
        R.order_columns(ok[0], ok[1].astype(np.uint32), *ok[2:])
    with pytest.raises(ValueError):
        R.order_columns(ok[0][:0], ok[1][:0], ok[2][:0], ok[3][:0])
    with pytest.raises(ValueError):
        R.order_columns(ok[0], ok[1][:3], *ok[2:])


# ------------------------------------------------------------------------------------------------ cli run
BASE = ['run', '--events', 'missing.npz', '--height', '64', '--width', '96', '--checkpoint', 'missing.pth.tar']


@pytest.mark.parametrize("extra,message", [
    ([], "exactly one of --window_ms MS and --window_events N"),
    (['--window_ms', '5', '--window_events', '100'], "exactly one of --window_ms MS and --window_events N"),
    (['--window_ms', '0'], "--window_ms MS: MS > 0"),
    (['--window_events', '0'], "--window_events N: N >= 1"),
    (['--window_ms', '5', '-v'], "needs --out DIR"),
    (['--window_ms', '5', '--fb_check', '1', '0.05', '--model_name', 'eraft'], "eraft has none"),
    (['--window_ms', '5', '--stream', '1'], "--stream N: N >= 2"),
    (['--window_ms', '5'], "--events missing.npz: no such file"),
])
def test_cli_run_refusals(extra, message):
    with pytest.raises(SystemExit) as e:
        cli.main(BASE + extra)
    assert message in str(e.value)


def test_cli_run_needs_its_required_flags_and_knows_its_units(capsys):
    with pytest.raises(SystemExit):
        cli.main(['run', '--window_ms', '5'])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.main(['run', '--events', 'a.npz', '--height', '0', '--width', '96', '--checkpoint', 'c', '--window_ms', '5'])
    assert "sensor size" in str(e.value)
    assert cli.T_UNITS['ns'] == (1e-9, 1_000_000) and cli.T_UNITS['us'] == (1e-6, 1_000) and cli.T_UNITS['s'] == (1.0, 1e-3)
    args = cli.build_parser().parse_args(BASE + ['--window_ms', '5'])
    assert args.t_unit == 'ns' and args.stream == 0 and args.out is None and not args.fwl and not args.rsat


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_and_lib_binds_the_entry_point():
    header = open(os.path.join(REPO, "include", "eemflow_hip.h")).read()
    at = header.index("int eemflow_voxelize_windows(")
    block = header[header.rindex("/*", 0, at):at]
    for word in ("Replaces", "{0, 1, 0, 0}", "colbin_e", "pack+direct", "scale_a) * scale_b", "no host synchronisation"):
        assert word in block, word
    decl = header[at:header.index(";", at)]
    assert re.sub(r"\s+", " ", decl) == ("int eemflow_voxelize_windows(int nwin, const void* t, const void* x, const void* y, const void* p, "
                                         "const int codes[4], const int64_t* offsets, double scale_a, double scale_b, int relative, int bins, "
                                         "int h, int w, int normalize, float* const* grids, void* stream)")
    assert "eemflow_voxelize_windows" in _lib.EXPORTS
    res, args = _lib._SIGNATURES["eemflow_voxelize_windows"]
    assert len(args) == 16
    import eemflow_amd
    assert eemflow_amd.voxelize_recording_windows is R.voxelize_windows and eemflow_amd.EventRecording is R.EventRecording
    assert eemflow_amd.voxelize_windows is not R.voxelize_windows   # the DSEC form keeps its name
    assert R.MAX_WINDOWS_PER_CALL == 32
    from eemflow_amd.build import EXTRA, SOURCES
    assert "voxel_cols.hip" in SOURCES and "-ffp-contract=off" in EXTRA["voxel_cols.hip"]
