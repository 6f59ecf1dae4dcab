"""Windows by span, host side (eemflow_amd/recording.py, mvsec_raw.py, harness.lag_plan / run_recording, `cli run`, `cli mvsec`; no GPU):
sliding windows on the raw t column against window_offsets and against a count of the events inside each window; the grey-frame spans
against generate_fimage's slices and the samples of MvsecEventFlow / MvsecEventFlow_dt4; the class walk that turns pairs at a lag into
ordinary streams; the refusals; the declarations and bindings of the two entry points."""
import os
import re

import numpy as np
import pytest

from eemflow_amd import _lib, cli, harness, mvsec_raw as M, recording as R

import gt_prop_reference as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = np.array([100, 110, 110, 120, 135, 150, 150, 199], dtype=np.int64)       # ties ON the edges 110 and 150, nothing in [140, 150)


def counted(t, lo, hi):
    """[first, end) of the events lo <= t < hi, by counting."""
    return [int(np.sum(t < lo)), int(np.sum(t < hi))]


# ------------------------------------------------------------------------------------------------ H1. sliding_spans
def test_stride_equal_to_the_window_gives_window_offsets():
    for t, window in ((T, 10), (T, 25), (T.astype(np.float64) * 0.25, 2.5), (T, 1000)):
        offs = R.window_offsets(t, window=window)
        spans = R.sliding_spans(t, window=window, stride=window)
        assert spans.dtype == np.int64 and spans.shape == (len(offs) - 1, 2)
        assert spans.tolist() == [[int(a), int(b)] for a, b in zip(offs, offs[1:])]
    assert R.sliding_spans(T, window=10, stride=10).tolist()[3:6] == [[4, 5], [5, 5], [5, 7]]      # a tie on 150 goes to the later window; [140, 150) is empty
    offs = R.window_offsets(T, count=3)
    assert R.sliding_spans(T, count=3, stride_count=3).tolist() == [[0, 3], [3, 6]] == [[int(a), int(b)] for a, b in zip(offs, offs[1:])]


def test_sliding_windows_hold_exactly_their_events():
    spans = R.sliding_spans(T, window=20, stride=10)                 # [100 + 10 m, 120 + 10 m), the last full one ends at 190 <= 199
    assert spans.tolist() == [counted(T, 100 + 10 * m, 120 + 10 * m) for m in range(8)]
    assert spans[0].tolist() == [0, 3] and spans[1].tolist() == [1, 4]          # both events ON the edge 110 start window 1
    assert np.array_equal(spans[:-2, 1], spans[2:, 0])               # a window of two strides ends where the window two later starts
    odd = R.sliding_spans(T, window=25, stride=10)                   # a stride that does not divide the window
    assert odd.tolist() == [counted(T, 100 + 10 * m, 125 + 10 * m) for m in range(8)]
    wide = R.sliding_spans(T, window=10, stride=30)                  # gaps between the windows
    assert wide.tolist() == [counted(T, 100 + 30 * m, 110 + 30 * m) for m in range(3)]        # [190, 200) would end behind t[-1] = 199
    tf = T.astype(np.float64) * 0.25
    assert R.sliding_spans(tf, window=5.0, stride=2.5).tolist() == spans.tolist()
    assert R.sliding_spans(T, window=99, stride=1).tolist() == [[0, 7]]          # exactly one full window: it ends ON t[-1], which stays outside
    assert R.sliding_spans(T, window=100, stride=1).shape == (0, 2)


def test_integer_nanoseconds_beyond_2_53_are_searched_as_integers():
    base = 1700000000000000123
    big = np.arange(8, dtype=np.int64) + base
    assert float(base) != base                                       # a float64 edge would be rounded
    assert R.sliding_spans(big, window=4, stride=2).tolist() == [[0, 4], [2, 6]]
    assert R.sliding_spans(big, window=2.5, stride=2.5).tolist() == [[0, 3], [3, 5]]        # window_offsets' edges base + ceil(2.5 k)
    assert R.sliding_spans(big, window=2.5, stride=1).tolist() == [[m, m + 3] for m in range(5)]       # t >= e is t >= ceil(e)


def test_count_form_and_refusals():
    assert R.sliding_spans(T, count=3, stride_count=2).tolist() == [[0, 3], [2, 5], [4, 7]]
    assert R.sliding_spans(T, count=8, stride_count=1).tolist() == [[0, 8]]
    assert R.sliding_spans(T, count=9, stride_count=1).shape == (0, 2)
    for kw in ({}, {"window": 10}, {"stride": 10}, {"count": 3}, {"window": 10, "stride": 5, "count": 3, "stride_count": 1},
               {"window": 10, "stride_count": 2}, {"window": 0, "stride": 1}, {"window": 10, "stride": 0}, {"window": 10, "stride": -1.0},
               {"count": 2.5, "stride_count": 1}, {"count": 3, "stride_count": 0}, {"count": 0, "stride_count": 1}):
        with pytest.raises(ValueError):
            R.sliding_spans(T, **kw)
    with pytest.raises(ValueError):
        R.sliding_spans(T[:0], window=10, stride=5)


def test_spans_are_checked_against_the_recording():
    assert R._check_spans("x", np.array([[3, 8], [0, 0], [3, 8], [2, 4]]), 8) == [(3, 8), (0, 0), (3, 8), (2, 4)]       # any order, repeats
    assert R._check_spans("x", np.zeros((0, 2), np.int64), 8) == []
    for bad in ([[0, 9]], [[-1, 2]], [[3, 2]], [0, 3], [[0, 1, 2]], [[0.0, 2.0]]):
        with pytest.raises(ValueError):
            R._check_spans("x", bad, 8)
    assert R._windows_of("x", [0, 3, 8], None, 8) == ([0, 3, 8], [(0, 3), (3, 8)])
    assert R._windows_of("x", None, [[2, 5]], 8) == (None, [(2, 5)])
    for offsets, spans in ((None, None), ([0, 8], [[0, 8]])):
        with pytest.raises(ValueError, match="exactly one of offsets and spans"):
            R._windows_of("x", offsets, spans, 8)


# ------------------------------------------------------------------------------------------------ H2. frame_spans
INDS = np.array([-1, -1, 0, 40, 95, 95, 160, 230, 300, 380, 450, 520, 600, 690], dtype=np.int64)     # MVSEC: -1 before the first event
TS = 10.0 + 0.03 * np.arange(INDS.shape[0]) + 0.001 * np.arange(INDS.shape[0]) ** 2


def test_frame_spans_are_generate_fimages_slices():
    files = G.generate_fimage_slices(INDS, 1)                          # dt_time = 1, as MVSEC_encoder.py:199 sets it
    for dt, first, last in ((4, 1, 7), (1, 1, 7), (4, 0, 0)):
        spans, t_spans, lag = M.frame_spans(TS, INDS, first, last, dt, reference_pairs=True)
        pairs = last - first + 1
        assert lag == 1 and spans.dtype == np.int64 and spans.shape == (pairs + 1, 2) and t_spans.shape == (pairs, 2)
        for m in range(pairs + 1):
            # sample i of MvsecEventFlow_dt4 concatenates the event files i+1 .. i+4 (old) and i+2 .. i+5 (new); of MvsecEventFlow file i+1, i+2
            assert tuple(spans[m]) == (files[first + m + 1][0], files[first + m + dt][1]), (dt, m)
        for m in range(pairs):
            assert tuple(t_spans[m]) == (TS[first + m], TS[first + m + dt])      # flowgt_dt<dt>/<first + m>.npy
    assert M.frame_spans(TS, INDS, 0, 0, 4, reference_pairs=True)[0].tolist() == [[0, 95], [0, 95]]       # the index < 0 counted as 0
    assert M.frame_spans(TS, INDS, 1, 7, 4, stride=1, reference_pairs=True)[0].shape == (8, 2)


def test_frame_spans_at_a_stride():
    for dt, first, last in ((1, 1, 7), (4, 1, 4), (2, 2, 7)):
        offsets, edges = M.frame_windows(TS, INDS, first, last, dt)
        for stride in (None, dt):
            spans, t_spans, lag = M.frame_spans(TS, INDS, first, last, dt, stride=stride)
            assert lag == 1 and spans.tolist() == [[int(a), int(b)] for a, b in zip(offsets, offsets[1:])]
            assert t_spans.tolist() == [[a, b] for a, b in zip(edges, edges[1:-1])]
    for dt, stride, first, last in ((4, 1, 1, 5), (4, 2, 0, 5), (3, 1, 2, 7), (6, 3, 1, 1)):
        spans, t_spans, lag = M.frame_spans(TS, INDS, first, last, dt, stride=stride)
        pairs = (last - first) // stride + 1
        assert lag == dt // stride and spans.shape == (pairs + lag, 2) and t_spans.shape == (pairs, 2)
        for m in range(pairs + lag):
            f = first + m * stride
            assert tuple(spans[m]) == (max(INDS[f], 0), max(INDS[f + dt], 0))
        for m in range(pairs):
            assert spans[m, 1] == spans[m + lag, 0]                  # the pair's second window starts where its first ends
            assert tuple(t_spans[m]) == (TS[first + m * stride], TS[first + m * stride + dt])


@pytest.mark.parametrize("kw", [dict(first=1, last=5, dt=4, stride=3), dict(first=1, last=5, dt=4, stride=8), dict(first=1, last=5, dt=4, stride=0),
                                dict(first=1, last=9, dt=4, reference_pairs=True), dict(first=1, last=8, dt=4, reference_pairs=True, stride=2),
                                dict(first=1, last=9, dt=4), dict(first=0, last=12, dt=1), dict(first=3, last=2, dt=1), dict(first=-1, last=2, dt=1),
                                dict(first=1, last=2, dt=0)])
def test_frame_spans_refusals(kw):
    with pytest.raises(ValueError):
        M.frame_spans(TS, INDS, **kw)


def test_frame_spans_refuses_descending_indices_and_the_docstring_points_here():
    down = INDS.copy()
    down[6] = 80                                                       # below inds[4] = 95
    with pytest.raises(ValueError, match="does not ascend"):
        M.frame_spans(TS, down, 3, 5, 2, stride=1)
    assert M.frame_spans(TS, INDS, 1, 8, 4, reference_pairs=True)[0].shape == (9, 2)        # the last pair the 14 frames allow: 8 + 1 + 4 = 13
    assert "frame_spans" in M.frame_windows.__doc__ and "reproduced here only" not in M.frame_windows.__doc__


# ------------------------------------------------------------------------------------------------ H3. the class walk
def test_the_class_walk_puts_every_window_into_one_call_and_gives_every_pair_once():
    for nwin in range(2, 41):
        for lag in range(1, 6):
            for chunk in range(2, 17):
                plan = harness.lag_plan(nwin, lag, chunk)
                seen, pairs, carried, cls = [], [], None, None
                for reset, wins, out in plan:
                    assert 1 <= len(wins) <= chunk
                    assert all(b - a == lag for a, b in zip(wins, wins[1:]))                # one class, neighbours at the lag
                    if reset:
                        assert wins[0] < lag and wins[0] != cls                            # a class starts at its first window, once
                        cls, chain = wins[0], list(wins)
                    else:
                        assert wins[0] == carried + lag                                    # the stream goes on behind the carried window
                        chain = [carried] + list(wins)
                    assert out == list(zip(chain, chain[1:]))                              # what forward_stream gives for these windows
                    carried = wins[-1]
                    seen += wins
                    pairs += out
                assert sorted(seen) == list(range(nwin)), (nwin, lag, chunk)
                assert pairs == [(a, a + lag) for r in range(lag) for a in range(r, nwin - lag, lag)], (nwin, lag, chunk)      # class-major
                assert sorted(pairs) == [(a, a + lag) for a in range(nwin - lag)]
    assert harness.lag_plan(7, 1, 3) == [(True, [0, 1, 2], [(0, 1), (1, 2)]), (False, [3, 4, 5], [(2, 3), (3, 4), (4, 5)]), (False, [6], [(5, 6)])]
    # lag 1 is the walk over consecutive windows
    assert [(wins[0], len(wins), len(out)) for _, wins, out in harness.lag_plan(12, 1, 4)] == [(w0, cnt, nflow) for w0, cnt, _, nflow in
                                                                                                harness.stream_plan(11, 4)]
    assert harness.lag_plan(0, 2, 4) == [] and harness.lag_plan(1, 3, 4) == [(True, [0], [])]
    for bad in ((5, 0, 4), (5, 1, 0)):
        with pytest.raises(ValueError):
            harness.lag_plan(*bad)


# ------------------------------------------------------------------------------------------------ H4. run_recording's refusals
def test_run_recording_refusals():
    import inspect
    params = inspect.signature(harness.run_recording).parameters
    assert [params[k].default for k in ("offsets", "spans", "lag", "t_spans")] == [None, None, 1, None]
    assert list(params)[:3] == ["model", "recording", "offsets"]

    class Rec:
        n, height, width = 10, 8, 8
        device = "cuda:0"

    class Gt:
        height, width, device = 8, 8, "cuda:0"

        def plan(self, a, b):
            return M.plan_window(np.array([0.0, 1.0, 2.0, 3.0]), a, b)

    class Model:
        MAX_STREAM = 16

        def forward_stream(self, vols):
            raise AssertionError("refused before any launch")
    spans = [[0, 4], [2, 6], [4, 8], [6, 10]]
    for args, kw, msg in (((), {}, "exactly one of offsets and spans"), (([0, 5, 10],), dict(spans=spans), "exactly one of offsets and spans"),
                          ((), dict(spans=spans, lag=0), "lag is a positive"), ((), dict(spans=spans, lag=1.5), "lag is a positive"),
                          (([0, 5, 10],), dict(lag=-1), "lag is a positive"),
                          ((), dict(spans=[[2, 6], [0, 4]]), "non-decreasing"), ((), dict(spans=[[0, 6], [2, 5]]), "non-decreasing"),
                          ((), dict(spans=[[0, 11]]), "inside the recording"),
                          ((), dict(spans=spans, lag=2, gt=Gt(), t_spans=[[0.1, 0.2]] * 3), "one .start, end. per pair .2 for 4 spans at lag 2"),
                          ((), dict(spans=spans, gt=Gt()), "needs t_spans="), ((), dict(spans=spans, gt=Gt(), t_edges=[0.0] * 5), "t_edges= goes with offsets"),
                          (([0, 5, 10],), dict(gt=Gt(), t_edges=[0.1, 0.2, 0.3], t_spans=[[0.1, 0.2]]), "t_spans= goes with spans="),
                          ((), dict(spans=spans, t_spans=[[0.1, 0.2]] * 3), "qualify gt="),
                          ((), dict(spans=spans, gt=Gt(), t_spans=[[0.1, 0.2], [0.1, 0.2], [2.5, 3.5]]), "beyond the last"),     # planned before any launch
                          ((), dict(spans=spans, chunk=17), "chunk is 1..16")):
        with pytest.raises(ValueError, match=msg):
            next(harness.run_recording(Model(), Rec(), *args, **kw))


# ------------------------------------------------------------------------------------------------ H5. command line, declarations
RUN = ['run', '--events', 'missing.npz', '--height', '64', '--width', '96', '--checkpoint', 'missing.pth.tar']
MVSEC = ['mvsec', '--data', 'missing_data.npz', '--gt', 'missing_gt.npz', '--checkpoint', 'missing.pth.tar']


@pytest.mark.parametrize("base,extra,message", [
    (RUN, ['--window_ms', '40', '--stride_events', '10'], "--stride_events N with --window_events"),
    (RUN, ['--window_events', '3000', '--stride_ms', '10'], "--stride_ms MS goes with --window_ms"),
    (RUN, ['--window_ms', '40', '--stride_ms', '15'], "divides --window_ms"),
    (RUN, ['--window_ms', '40', '--stride_ms', '0'], "divides --window_ms"),
    (RUN, ['--window_ms', '40', '--stride_ms', '80'], "divides --window_ms"),
    (RUN, ['--window_events', '3000', '--stride_events', '700'], "divides --window_events"),
    (RUN, ['--window_events', '3000', '--stride_events', '0'], "divides --window_events"),
    (RUN, ['--window_events', '3000', '--stride_events', '1000'], "--events missing.npz: no such file"),
    (RUN, ['--window_ms', '40', '--stride_ms', '10'], "--events missing.npz: no such file"),
    (MVSEC, ['--dt', '4', '--stride', '3'], "S divides --dt 4"),
    (MVSEC, ['--dt', '4', '--stride', '0'], "S divides --dt 4"),
    (MVSEC, ['--dt', '4', '--reference_pairs', '--stride', '2'], "--stride does not apply"),
    (MVSEC, ['--dt', '4', '--reference_pairs'], "--data missing_data.npz: no such file"),
    (MVSEC, ['--dt', '4', '--stride', '2'], "--data missing_data.npz: no such file"),
])
def test_cli_refusals(base, extra, message):
    with pytest.raises(SystemExit) as e:
        cli.main(base + extra)
    assert message in str(e.value)


def test_cli_parser_defaults_and_pair_range():
    run_args = cli.build_parser().parse_args(RUN + ['--window_ms', '5'])
    assert run_args.stride_ms is None and run_args.stride_events is None
    assert not hasattr(run_args, 'gt') and not hasattr(run_args, 'crop')                  # `cli run` keeps to flows
    got = cli.build_parser().parse_args(RUN + ['--window_events', '3000', '--stride_events', '1000'])
    assert (got.window_events, got.stride_events) == (3000, 1000)
    assert cli.build_parser().parse_args(RUN + ['--window_ms', '40', '--stride_ms', '2.5']).stride_ms == 2.5
    args = cli.build_parser().parse_args(MVSEC)
    assert (args.dt, args.stride, args.reference_pairs) == (1, None, False)
    args = cli.build_parser().parse_args(MVSEC + ['--dt', '4', '--stride', '2', '--reference_pairs'])
    assert (args.dt, args.stride, args.reference_pairs) == (4, 2, True)
    gt_ts = 100.0 + 0.05 * np.arange(10)
    img_ts = 99.9 + 0.031 * np.arange(24)
    assert cli.mvsec_pair_range(img_ts, 24, gt_ts, None, None, 1) == (4, 17)              # the positional form and its results stay
    assert cli.mvsec_pair_range(img_ts, 24, gt_ts, None, None, 4) == (4, 13)              # [img_ts[13], img_ts[17]] is the last one covered
    # --reference_pairs at dt 4: a pair needs the frames i .. i + 5, not i .. i + 8, and pairs start at every frame
    assert cli.mvsec_pair_range(img_ts, 24, gt_ts, None, None, 4, frames_needed=5, step=1) == (4, 13)
    with pytest.raises(SystemExit, match="pairs start at grey frames 0..15"):
        cli.mvsec_pair_range(img_ts, 24, gt_ts, 4, 16, 4)
    with pytest.raises(SystemExit, match="does not cover"):
        cli.mvsec_pair_range(img_ts, 24, gt_ts, 4, 16, 4, frames_needed=5, step=1)         # frames allow it (top 18), the ground truth does not
    with pytest.raises(SystemExit, match="pairs start at grey frames 0..18"):
        cli.mvsec_pair_range(img_ts, 24, gt_ts, 4, 19, 4, frames_needed=5, step=1)
    # the last pair checked is the last one on the stride's grid: 4 + (12 - 4) // 4 * 4 = 12 at the default step, 12 itself at step 1
    assert cli.mvsec_pair_range(img_ts, 24, gt_ts, 4, 12, 4) == (4, 12) == cli.mvsec_pair_range(img_ts, 24, gt_ts, 4, 12, 4, step=2)


def test_header_declares_and_lib_binds_the_span_entry_points():
    header = open(os.path.join(REPO, "include", "eemflow_hip.h")).read()
    want = {
        "eemflow_voxelize_spans": ("int eemflow_voxelize_spans(int nwin, const void* t, const void* x, const void* y, const void* p, const int codes[4], "
                                   "const int64_t* starts, const int64_t* ends, double scale_a, double scale_b, int relative, int bins, int h, int w, "
                                   "int normalize, float* const* grids, void* stream)", 17, "eemflow_voxelize_windows"),
        "eemflow_event_mask_spans": ("int eemflow_event_mask_spans(int nwin, const void* x, const void* y, int code_x, int code_y, const int64_t* starts, "
                                     "const int64_t* ends, int h, int w, float* const* masks, void* stream)", 11, "eemflow_event_mask_windows"),
    }
    for name, (decl, nargs, older) in want.items():
        at = header.index(f"int {name}(")
        assert re.sub(r"\s+", " ", header[at:header.index(";", at)]) == decl
        block = header[header.rindex("/*", 0, at):at]                # a comment block of its own, behind the older declaration
        for word in ("starts[k], ends[k]", "overlap", "repeat", "empty", older):
            assert word in block, (name, word)
        assert header.index(f"int {older}(") < header.rindex("/*", 0, at) < at
        assert name in _lib.EXPORTS
        res, args = _lib._SIGNATURES[name]
        assert len(args) == nargs == decl.count(",") + 1
        assert len(_lib._SIGNATURES[older][1]) == nargs - 1
    for src, names in (("voxel_cols.hip", ("eemflow_voxelize_windows", "eemflow_voxelize_spans")),
                       ("gt_prop.hip", ("eemflow_event_mask_windows", "eemflow_event_mask_spans"))):
        text = open(os.path.join(REPO, "eemflow_amd", "csrc", src)).read()
        for name in names:
            assert text.count(f'extern "C" int {name}(') == 1 and text.count(f'"{name}"') == 1      # one body, told the entry point's name once
    import inspect
    assert list(inspect.signature(R.voxelize_windows).parameters) == ["recording", "offsets", "num_bins", "normalize", "relative", "spans"]
    assert list(inspect.signature(R.EventRecording.tables).parameters) == ["self", "offsets", "relative", "spans"]
    assert list(inspect.signature(M.event_mask_windows).parameters) == ["recording", "offsets", "out", "spans"]
