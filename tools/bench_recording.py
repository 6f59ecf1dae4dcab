#!/usr/bin/env python3
"""Windows of a resident recording voxelized straight from its columns, against the composition through the float64 table.
tools/bench_recording.py [--calls N] [--rounds R] [--out FILE] [--kernels-only] [--no-model]

Microseconds per WINDOW (normalised grid; wall clock around N back-to-back calls and a device synchronisation, so host work counts)
at 5 x 720 x 1280 with 2e6 events per window and 5 x 260 x 346 with 2e5, at 1, 10 and 32 windows per call; HREM-style columns
(t int64 ns, x and y uint16, p uint8).  In ONE process the routes alternate inside every round; the median (min, max) of R rounds:
  fused      eemflow_amd.recording.voxelize_windows on the resident recording (eemflow_voxelize_windows: vox_bin_cols_kernel's
             instantiation for HREM's dtypes, no dtype switch)
  generic    the same events with x and y stored as int16 instead of uint16 - the same 13 B per event, the same grids bitwise - which
             takes vox_bin_cols_kernel's generic instantiation behind pk_load's dtype switch: the A/B of the two instantiations
  host       what cutting a recording costs without it: per call events.pack_events_many on the windows' HOST slices (pinned staging,
             upload, event_pack_kernel, a synchronisation) and voxelizer.voxelize_many_device on the tables
  device     the composition without staging: EventRecording.tables (event_pack_kernel on views of the resident columns), then
             voxelize_many_device
Before timing, the fused grid of the first window is held bitwise against the composition's.
Then (unless --no-model) frames per second of harness.run_recording with a seeded EEMFlow at 1280 x 720 over 32 windows, against
EEMFlow.forward_stream on the same windows' volumes already resident.
Writes the lines and one JSON line to --out (default profiles/recording_bench.txt beside this tool) and to stdout.
--spans: windows by span instead (eemflow_voxelize_spans), written to profiles/spans_bench.txt: at 5 x 260 x 346 with 8e4 events per window and
5 x 720 x 1280 with 2e6, 32 windows that overlap by 3/4 of their length -
  spans        all 32 by one call of voxelize_windows(spans=)
  one_by_one   the same 32 spans, one call of voxelize_windows(offsets) each: all the consecutive-window entry point can do for them
  consecutive  32 consecutive windows of the same length by one call of voxelize_windows(offsets): the same kernels as `spans`
then frames per second of MVSEC's dt4 protocol on the synthetic sequence of tests/test_gpu_spans.py (8 samples, 260 x 346, crop 256 x 256):
harness.run_recording on MvsecRaw.frame_spans(reference_pairs=True) with ground truth and scoring - the loop of `cli mvsec --dt 4
--reference_pairs` - against MvsecEventFlow_dt4 over files through harness.stream_chunks, scored the same way.
--kernels-only: just `fused`, `generic` and `device` at 10 windows per call, a few calls (for a `rocprofv3 --kernel-trace --stats` run of its own:
vox_bin_cols_kernel beside event_pack_kernel + vox_bin_kernel)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
from eemflow_amd import events as E, harness, recording as R      # noqa: E402
from eemflow_amd.voxelizer import voxelize_many_device            # noqa: E402

SIZES = (((5, 720, 1280), 2_000_000), ((5, 260, 346), 200_000))
COUNTS = (1, 10, 32)
DEV = "cuda:0"


def make_columns(seed, n, windows, H, W):
    """`windows` windows of n events each: one window's columns repeated, its timestamps moved on by 50 ms per window."""
    r = np.random.default_rng(seed)
    t1 = np.sort(r.integers(0, 50_000_000, n)).astype(np.int64)
    x1, y1 = r.integers(0, W, n).astype(np.uint16), r.integers(0, H, n).astype(np.uint16)
    p1 = (2 * r.integers(0, 2, n).astype(np.uint8) - 1)
    t = np.concatenate([t1 + 1700000000000000000 + 50_000_000 * k for k in range(windows)])
    return t, np.tile(x1, windows), np.tile(y1, windows), np.tile(p1, windows)


def wall_us(call, calls, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (calls * per)


def alternate(routes, calls, rounds, per):
    """{name: (median, min, max)}: every round times every route once, in turn."""
    for name, (call, _) in routes.items():
        call()
    us = {name: [] for name in routes}
    for _ in range(rounds):
        for name, (call, share) in routes.items():
            us[name].append(wall_us(call, max(1, int(calls * share)), per))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in us.items()}


SPAN_SIZES = (((5, 260, 346), 80_000), ((5, 720, 1280), 2_000_000))


def spans_mode(a, say, res):
    for (C, H, W), n in SPAN_SIZES:
        k, stride = 32, n // 4
        cols = make_columns(4, n, k, H, W)                             # 32 n events: the consecutive windows need them all
        rec = R.EventRecording(*cols, H, W, device=DEV)
        spans = rec.sliding_spans(count=n, stride_count=stride)[:k]
        offsets = rec.window_offsets(count=n)
        assert spans.shape == (k, 2) and len(offsets) == k + 1 and spans[1, 0] == stride
        got = R.voxelize_windows(rec, spans=spans[1:2], num_bins=C)[0][0]
        want = voxelize_many_device(rec.tables(spans=spans[1:2]), C, H, W)[0]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "a span's grid is not the composition's, bit for bit"
        pairs = [[int(s), int(e)] for s, e in spans]
        routes = {"spans": (lambda: R.voxelize_windows(rec, spans=spans, num_bins=C), 1.0),
                  "one_by_one": (lambda: [R.voxelize_windows(rec, se, C) for se in pairs], 1.0),
                  "consecutive": (lambda: R.voxelize_windows(rec, offsets, C), 1.0)}
        out = alternate(routes, a.calls, a.rounds, k)
        tag = f"{C}x{H}x{W}_{n:.0e}".replace("+0", "")
        text = f"{C} x {H} x {W}, {n:.0e} events per window, 32 windows, overlap 3/4:"
        for name, (med, lo, hi) in out.items():
            text += f"   {name} {med:8.1f} ({lo:.1f}, {hi:.1f})"
            res[f"{tag}_{name}_us"] = med
            res[f"{tag}_{name}_spread_us"] = hi - lo
        text += f"   one_by_one / spans {out['one_by_one'][0] / out['spans'][0]:5.2f} x   spans / consecutive {out['spans'][0] / out['consecutive'][0]:5.2f} x"
        res[f"{tag}_one_by_one_over_spans"] = out["one_by_one"][0] / out["spans"][0]
        res[f"{tag}_spans_over_consecutive"] = out["spans"][0] / out["consecutive"][0]
        say(text)
        del rec
        torch.cuda.empty_cache()
    if a.no_model:
        return
    import pathlib
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from mvsec_dt4_sequence import make_sequence                       # the sequence of the dt4 test: raw arrays and the dataset's files
    from eemflow_amd import EEMFlow, mvsec, mvsec_raw as M
    from eemflow_amd.metrics import flow_error_sums_many
    from eemflow_amd.weights import seeded_state_dict
    with tempfile.TemporaryDirectory() as tmp:
        s = make_sequence(pathlib.Path(tmp))
        first, last, crop = s["first"], s["last"], (256, 256)
        net = EEMFlow("", 5, 5)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(3).items()})
        net = net.to(DEV).eval()
        net.change_imagesize(crop)
        ds = mvsec.MvsecEventFlow_dt4({"eval_type": "dense", "num_voxel_bins": 5, "sequence": "seqA"}, train=False, root=s["root"], device=DEV,
                                      valid_time_index={"seqA": [(first, last + 1)]})
        gt = M.MvsecGroundTruth(s["stack"], s["gt_ts"], device=DEV)
        raw = M.MvsecRaw(s["events"], s["img_ts"], s["inds"], gt, height=s["h"], width=s["w"], device=DEV)
        spans, t_spans, lag = raw.frame_spans(first, last, 4, reference_pairs=True)

        def raw_route():
            for _ in harness.run_recording(net, raw.recording, spans=spans, lag=lag, t_spans=t_spans, gt=gt, crop=crop, chunk=4):
                pass

        def dataset_route():
            for _, targets, flows in harness.stream_chunks(ds, net, 4, torch.device(DEV)):
                flow_error_sums_many([t["flow"].to(DEV)[None].float() for t in targets], flows, None, evaluation_type="dense")

        with torch.no_grad():
            out = alternate({"raw": (raw_route, 1.0), "dataset": (dataset_route, 1.0)}, 3, a.rounds, len(t_spans))
    text = f"EEMFlow, MVSEC dt4 protocol, {len(t_spans)} samples of 260 x 346 (crop 256 x 256, 4 windows per call), frames per second:"
    for name, (med, lo, hi) in out.items():
        text += f"   {name} {1e6 / med:8.1f} ({1e6 / hi:.1f}, {1e6 / lo:.1f})"
        res[f"mvsec_dt4_{name}_fps"] = 1e6 / med
    say(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timed run (the host route: a fifth of it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/recording_bench.txt, or profiles/spans_bench.txt with --spans")
    ap.add_argument("--spans", action="store_true", help="windows by span: 32 overlapping spans per call against one call each and against consecutive windows")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "spans_bench.txt" if a.spans else "recording_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("bench_recording.py measures on the GPU: no device found")
    lines, res = [], {"calls_per_run": a.calls, "rounds": a.rounds}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/bench_recording.py{' --spans' if a.spans else ''} --calls {a.calls} --rounds {a.rounds} (MI355X, one process, routes alternating; us per window, wall clock, "
        f"median (min, max) of the rounds)")
    big = None
    if a.spans:
        spans_mode(a, say, res)
    for (C, H, W), n in () if a.spans else SIZES:
        kmax = 10 if a.kernels_only else max(COUNTS)
        cols = make_columns(3, n, kmax, H, W)
        rec = R.EventRecording(*cols, H, W, device=DEV)
        rec16 = R.EventRecording(cols[0], cols[1].astype(np.int16), cols[2].astype(np.int16), cols[3], H, W, device=DEV)
        offsets = rec.window_offsets(count=n)
        assert len(offsets) == kmax + 1
        got = R.voxelize_windows(rec, offsets[:2], C)[0][0]
        want = voxelize_many_device(rec.tables(offsets[:2]), C, H, W)[0]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "the fused grid is not the composition's, bit for bit"
        assert torch.equal(R.voxelize_windows(rec16, offsets[:2], C)[0][0].view(torch.int32), want.view(torch.int32)), "generic != composition"
        tag = f"{C}x{H}x{W}_{n:.0e}".replace("+0", "")
        say(f"{C} x {H} x {W}, {n:.0e} events per window (fused == composition bitwise on window 0)")
        for k in ((10,) if a.kernels_only else COUNTS):
            offs = offsets[:k + 1]
            slices = [tuple(c[s:e] for c in cols) for s, e in zip(offs, offs[1:])]
            routes = {"fused": (lambda: R.voxelize_windows(rec, offs, C), 1.0),
                      "generic": (lambda: R.voxelize_windows(rec16, offs, C), 1.0),
                      "host": (lambda: voxelize_many_device(E.pack_events_many(slices, device=DEV), C, H, W), 0.2),
                      "device": (lambda: voxelize_many_device(rec.tables(offs), C, H, W), 1.0)}
            if a.kernels_only:
                del routes["host"]
            out = alternate(routes, 3 if a.kernels_only else a.calls, 1 if a.kernels_only else a.rounds, k)
            text = f"  {k:2d} windows per call:"
            for name, (med, lo, hi) in out.items():
                text += f"   {name} {med:8.1f} ({lo:.1f}, {hi:.1f})"
                res[f"{tag}_k{k}_{name}_us"] = med
                res[f"{tag}_k{k}_{name}_spread_us"] = hi - lo
            if "host" in out:
                text += f"   host / fused {out['host'][0] / out['fused'][0]:5.2f} x"
            text += f"   device / fused {out['device'][0] / out['fused'][0]:5.2f} x   generic / fused {out['generic'][0] / out['fused'][0]:5.2f} x"
            res[f"{tag}_k{k}_generic_over_fused"] = out["generic"][0] / out["fused"][0]
            res[f"{tag}_k{k}_device_over_fused"] = out["device"][0] / out["fused"][0]
            say(text)
        if H == 720:
            big = (rec, offsets)
        torch.cuda.empty_cache()
    if not a.kernels_only and not a.no_model and not a.spans:
        from eemflow_amd import EEMFlow
        from eemflow_amd.weights import seeded_state_dict
        rec, offsets = big
        net = EEMFlow("", groups=5, n_first_channels=5).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(5).items()})
        net = net.to(DEV)
        net.change_imagesize((720, 1280))
        pairs = len(offsets) - 2
        vols = R.voxelize_windows(rec, offsets, 5)

        def from_recording():
            for _ in harness.run_recording(net, rec, offsets):
                pass

        def from_volumes():
            net.reset_stream()
            for i in range(0, len(vols), net.MAX_STREAM):
                net.forward_stream(vols[i:i + net.MAX_STREAM])

        with torch.no_grad():
            out = alternate({"run_recording": (from_recording, 1.0), "resident_volumes": (from_volumes, 1.0)}, 3, a.rounds, pairs)
        text = f"EEMFlow 1280 x 720, {pairs} pairs of 2e6-event windows, frames per second:"
        for name, (med, lo, hi) in out.items():
            text += f"   {name} {1e6 / med:8.1f} ({1e6 / hi:.1f}, {1e6 / lo:.1f})"
            res[f"eemflow_720p_{name}_fps"] = 1e6 / med
        say(text)
    line = json.dumps(res)
    print(line, flush=True)
    if not a.kernels_only:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
