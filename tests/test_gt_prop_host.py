"""MVSEC ground-truth propagation, host side (eemflow_amd/mvsec_raw.py, tests/gt_prop_reference.py, `cli mvsec`; no GPU): the NumPy
restatement against the golden outputs of the reference's own lines (tests/golden/make_golden_gt_prop.py), bit for bit; that the
golden cases are not vacuous (ties, leaving the frame, the scale-0 step, enough surviving cells, six planted faults); the host plan's
refusals; the frame windows against generate_fimage's slices; the declarations, bindings and command-line refusals.

A note on the cases: a window that merely ENDS on a ground-truth timestamp has a last step of scale 1 (the reference's loop stops at
`ts[i+1] < end` and the last interval is covered whole); the last step has scale 0 only for a window that is exactly one interval
[ts[g], ts[g+1]] (gt_dt == dt takes the long branch, a = 1, b = 0).  Both kinds are golden cases."""
import os
import re

import numpy as np
import pytest

from eemflow_amd import _lib, cli, mvsec_raw as M

import gt_prop_reference as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("gt_prop.npz")
    ts = g["ts"]
    out = []
    for i, name in enumerate(g["names"]):
        stack = g["stack_" + str(g["stacks"][i])]
        out.append(dict(name=str(name), stack=stack, start=float(g["starts"][i]), end=float(g["ends"][i]), ref=g[f"ref_{i}"],
                        plan=G.plan(ts, g["starts"][i], g["ends"][i])))
    return ts, out


def _case(cases, name):
    return next(c for c in cases[1] if c["name"] == name)


# ------------------------------------------------------------------------------------------------ the restatement against the reference
def test_the_case_set_is_the_one_the_feature_was_specified_with(cases):
    ts, cs = cases
    assert ts.dtype == np.float64 and ts.shape == (10,) and bool(np.all(np.diff(ts) > 0))
    plans = {c["name"]: c["plan"] for c in cs}
    assert plans["inside_one_interval"][1] == 0 and plans["short_across_a_boundary"][1] == 0
    assert plans["crossing_one"][:2] == (3, 2) and plans["crossing_four"][:2] == (1, 5)
    assert plans["starting_on_a_timestamp"][1:3] == (3, 1.0)
    assert plans["ending_on_a_timestamp"][1] == 3 and plans["ending_on_a_timestamp"][3] == 1.0
    assert plans["exactly_one_interval"][1:] == (2, 1.0, 0.0) and plans["exactly_one_interval_early"][1:] == (2, 1.0, 0.0)
    assert plans["first_interval_spanning_eight"][:2] == (0, 9)
    for c in cs:
        assert c["stack"].dtype == np.float32 and c["stack"].shape == (10, 2, 20, 28)
        assert c["ref"].dtype == (np.float64 if c["plan"][1] == 0 else np.float32)
    share = (_case(cases, "crossing_one")["stack"] == 0).mean()
    assert 0.005 < share < 0.02                                      # 1 % planted zeros


def test_restatement_equals_the_reference_bitwise(cases):
    for c in cases[1]:
        frame0, nsteps, a, b = c["plan"]
        if nsteps == 0:                                               # float64 equal before the one fp32 rounding
            assert np.array_equal(G.short64(c["stack"], frame0, a, b), c["ref"]), c["name"]
            assert np.array_equal(G.walk(c["stack"], frame0, nsteps, a, b), c["ref"].astype(np.float32))
        else:
            got = G.walk(c["stack"], frame0, nsteps, a, b)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), c["ref"].view(np.uint32)), c["name"]


def test_library_plan_is_the_restatements(cases):
    ts, cs = cases
    for c in cs:
        assert M.plan_window(ts, c["start"], c["end"]) == c["plan"], c["name"]


def test_long_cases_keep_half_of_their_cells(cases):
    """In the reference's own output; at 3 % planted zeros the eight-interval case falls to 0.46 - 0.48, hence 1 %."""
    longs = [c for c in cases[1] if c["plan"][1] >= 2]
    assert len(longs) >= 8
    for c in longs:
        assert (c["ref"][0] != 0).mean() >= 0.5 and (c["ref"][1] != 0).mean() >= 0.5, c["name"]


def test_tie_case_visits_a_tie_where_the_roundings_differ(cases):
    c = _case(cases, "tie")
    visited = []
    G.walk(c["stack"], *c["plan"], visited=visited)
    x, y = visited[1]                                                 # the positions the second step rounds
    assert x.dtype == np.float32
    differ = (np.rint(x.astype(np.float64)) != np.floor(x.astype(np.float64) + 0.5)) | (np.rint(y.astype(np.float64)) != np.floor(y.astype(np.float64) + 0.5))
    assert differ.any() and x[7, 10] == 10.5 and y[7, 10] == 8.5


def test_border_case_leaves_the_frame(cases):
    c = _case(cases, "leaving_the_frame")
    visited = []
    G.walk(c["stack"], *c["plan"], visited=visited)
    x, y = visited[1]
    assert (y[0] < -0.5).all() and (x[:, -1] > 27.5).all()
    assert (c["ref"][:, 0] == 0).all() and (c["ref"][:, :, -1] == 0).all()


@pytest.mark.parametrize("fault", G.FAULTS)
def test_planted_faults_change_a_golden_cell(cases, fault):
    changed = []
    for c in cases[1]:
        if c["plan"][1] >= 2 and not np.array_equal(G.walk(c["stack"], *c["plan"], fault=fault), c["ref"]):
            changed.append(c["name"])
    assert changed, fault
    if fault == "skip_scale0":
        assert set(changed) == {"exactly_one_interval", "exactly_one_interval_early"}
    if fault == "half_up":
        assert "tie" in changed


def test_nonfinite_values_stay_nonfinite_in_the_restatement(cases):
    c = _case(cases, "crossing_four")
    st = c["stack"].copy()
    st[1, 0, 5, 5], st[3, 1, 9, 9], st[5, 0, 2, 20] = np.nan, np.inf, np.nan       # first step, a middle step, the last step
    clean, got = G.walk(c["stack"], *c["plan"]), G.walk(st, *c["plan"])
    # pixel (5, 5) reads the NaN at its first step: u stays NaN through the later steps (they find no cell for the position, read 0 and
    # leave the non-finite component's mask alone), v - whose coordinate is finite - is cleared by that border read
    assert np.isnan(got[0, 5, 5]) and got[1, 5, 5] == 0
    assert (~np.isfinite(got)).sum() >= 2
    differ = got.view(np.uint32) != clean.view(np.uint32)
    assert differ.sum() <= 12                                          # only the few walks that read a poisoned cell


# ------------------------------------------------------------------------------------------------ plan
def test_plan_refusals_and_edges(cases):
    ts, _ = cases
    d = np.diff(ts)
    with pytest.raises(ValueError, match="before the first"):
        M.plan_window(ts, ts[0] - 1e-6, ts[1])
    with pytest.raises(ValueError, match="beyond the last"):
        M.plan_window(ts, ts[7], ts[9] + 1e-6)
    with pytest.raises(ValueError, match="beyond the last"):
        M.plan_window(ts, ts[9], ts[9] + 0.01)                        # starts in (on) the last timestamp: no interval follows
    with pytest.raises(ValueError, match="end .* < start"):
        M.plan_window(ts, ts[3], ts[3] - 1e-3)
    assert M.plan_window(ts, ts[0], ts[0] + 0.5 * d[0]) == (0, 0, float(ts[0] + 0.5 * d[0] - ts[0]), float(d[0]))   # a start ON ts[0]
    assert M.plan_window(ts, ts[0], ts[2])[:3] == (0, 2, 1.0)
    last = M.plan_window(ts, ts[7] + 0.5 * d[7], ts[9])               # the last legal window ends ON the last timestamp
    assert last[:2] == (7, 2) and last[3] == 1.0
    assert M.plan_window(ts, ts[3], ts[3])[:3] == (3, 0, 0.0)         # an empty window: the short branch with dt = 0
    for f in G.plan, M.plan_window:
        assert f(ts, ts[2], ts[4] + 0.5 * d[4]) == G.plan(ts, ts[2], ts[4] + 0.5 * d[4])


# ------------------------------------------------------------------------------------------------ frame windows
def test_frame_windows_are_generate_fimages_slices():
    inds = np.array([-1, -1, 0, 40, 95, 95, 160, 230, 300, 380, 450, 520], dtype=np.int64)     # MVSEC: -1 before the first event
    ts = 10.0 + 0.03 * np.arange(inds.shape[0])
    files = G.generate_fimage_slices(inds, 1)                          # dt_time = 1, as MVSEC_encoder.py:199 sets it
    offsets, edges = M.frame_windows(ts, inds, 1, 7)
    assert offsets.dtype == np.int64 and len(offsets) == len(edges) == 7 + 2
    for m in range(len(offsets) - 1):
        # sample i of MvsecEventFlow reads event file i + 1 (old) and i + 2 (new); flowgt_dt1/i.npy covers [ts[i], ts[i+1]]
        assert (int(offsets[m]), int(offsets[m + 1])) == files[1 + m + 1], m
        assert edges[m] == ts[1 + m]
    assert offsets[0] == 0 and inds[1] < 0                             # the index < 0 counted as 0
    off4, edges4 = M.frame_windows(ts, inds, 2, 2, dt=4)               # one pair of consecutive windows of four frames
    assert off4.tolist() == [0, 160, 450] and edges4.tolist() == [ts[2], ts[6], ts[10]]
    four = G.generate_fimage_slices(inds, 1)
    assert (four[3][0], four[6][1]) == (off4[0], off4[1])              # = the files 3..6 MvsecEventFlow_dt4's sample 2 concatenates (old)
    for bad in (dict(first=0, last=11), dict(first=3, last=2), dict(first=0, last=1, dt=0), dict(first=-1, last=1)):
        with pytest.raises(ValueError):
            M.frame_windows(ts, inds, **bad)


# ------------------------------------------------------------------------------------------------ cli mvsec
BASE = ['mvsec', '--data', 'missing_data.npz', '--gt', 'missing_gt.npz', '--checkpoint', 'missing.pth.tar']


@pytest.mark.parametrize("extra,message", [
    (['--dt', '0'], "--dt N: N >= 1"),
    (['--crop', '300', '256'], "must fit the 260 x 346 sensor"),
    (['--stream', '1'], "--stream N: N >= 2"),
    (['--first', '5', '--last', '4'], "0 <= I <= J"),
    (['--height', '0'], "sensor size"),
    ([], "--data missing_data.npz: no such file"),
])
def test_cli_mvsec_refusals(extra, message):
    with pytest.raises(SystemExit) as e:
        cli.main(BASE + extra)
    assert message in str(e.value)


def test_cli_mvsec_parser_and_pair_range(capsys):
    with pytest.raises(SystemExit):
        cli.main(['mvsec', '--data', 'a.npz'])
    with pytest.raises(SystemExit):
        cli.main(BASE + ['--eval_type', 'other'])
    capsys.readouterr()
    args = cli.build_parser().parse_args(BASE)
    assert (args.dt, args.eval_type, args.crop, args.first, args.last, args.is_car, args.model_name) == (1, 'dense', None, None, None, False, 'EEMFlow')
    assert cli.build_parser().parse_args(BASE + ['--crop', '256', '256']).crop == [256, 256]
    gt_ts = 100.0 + 0.05 * np.arange(10)
    img_ts = 99.9 + 0.031 * np.arange(24)
    first, last = cli.mvsec_pair_range(img_ts, 24, gt_ts, None, None, 1)
    # img_ts[4] = 100.024 is the first >= 100.0; [img_ts[17], img_ts[18]] = [100.427, 100.458] starts inside the last interval and is
    # shorter than it - the short branch, which the reference serves too - and img_ts[18] lies behind the last timestamp
    assert (first, last) == (4, 17)
    assert img_ts[first] >= gt_ts[0] > img_ts[first - 1]
    M.plan_window(gt_ts, img_ts[last], img_ts[last + 1])
    with pytest.raises(ValueError):
        M.plan_window(gt_ts, img_ts[last + 1], img_ts[last + 2])
    with pytest.raises(SystemExit, match="does not cover"):
        cli.mvsec_pair_range(img_ts, 24, gt_ts, 0, 5, 1)
    with pytest.raises(SystemExit, match="pairs start at grey frames"):
        cli.mvsec_pair_range(img_ts, 24, gt_ts, 5, 22, 1)
    run_args = cli.build_parser().parse_args(['run', '--events', 'e.npz', '--height', '4', '--width', '4', '--checkpoint', 'c', '--window_ms', '5'])
    assert not hasattr(run_args, 'gt') and not hasattr(run_args, 'crop')              # `cli run` keeps its parser


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_and_lib_binds_the_entry_points():
    header = open(os.path.join(REPO, "include", "eemflow_hip.h")).read()
    at = header.index("int eemflow_gt_flow_many(")
    block = header[header.rindex("/*", 0, at):at]
    for word in ("Replaces: estimate_corresponding_gt_flow and prop_flow (loader/loader_utils.py:70-161", "round half to even", "BORDER_CONSTANT",
                 "independent and sticky", "(float)((double)x + (double)fu * scale)", "(float)(((double)gt[frame0] * a) / b)", "scale 0",
                 "no host synchronisation", "no NaN or infinity"):
        assert word in block, word
    decl = re.sub(r"\s+", " ", header[at:header.index(";", at)])
    assert decl == ("int eemflow_gt_flow_many(int njobs, const float* gt, int nframes, int h, int w, const int* frame0, const int* nsteps, "
                    "const double* a, const double* b, float* const* out, void* stream)")
    at = header.index("int eemflow_event_mask_windows(")
    block = header[header.rindex("/*", 0, at):at]
    for word in ("Replaces", "plain stores", "zero-filled", "0 <= x <= w"):
        assert word in block, word
    for name, nargs in (("eemflow_gt_flow_many", 11), ("eemflow_event_mask_windows", 10)):
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][1]) == nargs
    from eemflow_amd.build import EXTRA, SOURCES
    assert "gt_prop.hip" in SOURCES and "-ffp-contract=off" in EXTRA["gt_prop.hip"]
    import eemflow_amd
    assert eemflow_amd.MvsecGroundTruth is M.MvsecGroundTruth and eemflow_amd.MvsecRaw is M.MvsecRaw
    assert M.MAX_JOBS_PER_CALL == 32


def test_run_recording_refuses_what_it_cannot_score():
    import inspect
    from eemflow_amd import harness
    params = inspect.signature(harness.run_recording).parameters
    assert [params[k].default for k in ("gt", "t_edges", "crop", "eval_type", "is_car")] == [None, None, None, 'dense', False]

    class Rec:
        n, height, width = 10, 8, 8

    class Model:
        MAX_STREAM = 16

        def forward_stream(self, vols):
            return []
    for kw, msg in ((dict(crop=(4, 4), fwl=True), "crop= with fwl= or rsat="), (dict(crop=(4, 4), rsat=True), "crop= with fwl= or rsat="),
                    (dict(t_edges=[0.0, 1.0]), "qualify gt="), (dict(eval_type='sparse'), "qualify gt="), (dict(eval_type='other'), "eval_type"),
                    (dict(crop=(9, 4)), "does not fit")):
        with pytest.raises(ValueError, match=msg):
            next(harness.run_recording(Model(), Rec(), [0, 5, 10], **kw))
