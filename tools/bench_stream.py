#!/usr/bin/env python3
"""Streaming inference against pairwise inference on one context: tools/bench_stream.py [--calls N] [--rounds R] [--frames F]

At 1280x720 with seeded weights and synthetic volumes, a stream of consecutive windows is timed two ways in the same process:
  stream  EEMFlow.forward_stream: F new windows per call, the window before them carried - F flows, F windows encoded;
  many    EEMFlow.forward_many:   the same F pairs (v_i, v_{i+1}) as independent samples - F flows, 2 F windows encoded.
Both run N calls per round after a warm-up, alternating round by round, with HIP events around each run of N calls (the graph replays
are enqueued back to back).  Prints frames/s of each per round, the median ratio and the spread over the rounds, and one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                      # noqa: E402
from eemflow_amd import EEMFlow                                   # noqa: E402
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40, help="calls per timed run")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of both forms")
    ap.add_argument("--frames", type=int, default=10, help="flows per call")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    a = ap.parse_args()
    h, w, F = a.height, a.width, a.frames
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    net = net.cuda()
    net.change_imagesize((h, w))
    # a ring of distinct windows (as many as a run of calls touches would not fit: 2 F + 1 distinct volumes, reused call after call)
    vols = [torch.from_numpy(synthetic_voxel_pair(100 + i, 1, h, w)[0]).cuda() for i in range(2 * F + 1)]
    chunks = [vols[1:F + 1], vols[F + 1:2 * F + 1]]               # stream calls alternate between the two halves of the ring
    pairs = [[(vols[i], vols[i + 1]) for i in range(F)], [(vols[F + i], vols[F + i + 1]) for i in range(F)]]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(form, calls):
        start.record()
        for c in range(calls):
            if form == "stream":
                net.forward_stream(chunks[c % 2])
            else:
                net.forward_many(pairs[c % 2])
        stop.record()
        stop.synchronize()
        return calls * F / (start.elapsed_time(stop) * 1e-3)

    with torch.no_grad():
        net.reset_stream()
        net.forward_stream(vols[:1])                              # the stream starts with window 0 carried
        for form in ("stream", "many", "stream", "many"):         # warm-up: graph captures of every key, clocks
            run(form, 6)
        res = {"stream": [], "many": []}
        for r in range(a.rounds):
            for form in (("stream", "many") if r % 2 == 0 else ("many", "stream")):
                res[form].append(run(form, a.calls))
            print(f"round {r}: stream {res['stream'][-1]:8.1f} frames/s   forward_many {res['many'][-1]:8.1f} frames/s   "
                  f"ratio {res['stream'][-1] / res['many'][-1]:.3f}", flush=True)
    ratios = [s / m for s, m in zip(res["stream"], res["many"])]
    out = {"size": f"{w}x{h}", "frames_per_call": F, "calls_per_run": a.calls, "rounds": a.rounds,
           "stream_fps": statistics.median(res["stream"]), "many_fps": statistics.median(res["many"]),
           "ratio": statistics.median(ratios), "ratio_min": min(ratios), "ratio_max": max(ratios),
           "stream_fps_all": [round(v, 1) for v in res["stream"]], "many_fps_all": [round(v, 1) for v in res["many"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
