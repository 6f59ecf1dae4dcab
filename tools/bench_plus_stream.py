#!/usr/bin/env python3
"""EEMFlow+ streaming inference against pairwise inference on one context:
tools/bench_plus_stream.py [--calls N] [--rounds R] [--frames F ...]

At 1280x720, n_first_channels = 5, seeded weights and synthetic volumes, a stream of consecutive windows is timed two ways in the same
process, for each F (flows per call):
  stream  EEMFlow_cdc.forward_stream: F new windows per call, the window before them carried - F windows padded and encoded;
  many    EEMFlow_cdc.forward_many on the same F pairs (v_i, v_{i+1}) - 2 F windows padded and encoded, the same batch-F levels.
The forms run N calls per round after a warm-up, in an order that alternates round by round, with HIP events around each run of N
calls.  Prints frames/s per round, the median ratio stream / many with its min / max, and one JSON line per F."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                      # noqa: E402
from eemflow_amd.eemflow_plus import EEMFlow_cdc                  # noqa: E402
from eemflow_amd.plus_weights import seeded_from_shapes           # noqa: E402
from eemflow_amd.weights import synthetic_voxel_pair              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="calls per timed run")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the forms")
    ap.add_argument("--frames", type=int, nargs="+", default=[4, 8], help="flows per call")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    a = ap.parse_args()
    h, w = a.height, a.width
    net = EEMFlow_cdc("", 3, 5).eval()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_from_shapes(shapes, 0).items()})
    net = net.cuda()
    net.change_imagesize((h, w))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for F in a.frames:
        vols = [torch.from_numpy(synthetic_voxel_pair(100 + i, 1, h, w)[0]).cuda() for i in range(2 * F + 1)]
        chunks = [vols[1:F + 1], vols[F + 1:2 * F + 1]]           # stream calls alternate between the two halves of the ring
        pairs = [[(vols[i], vols[i + 1]) for i in range(F)], [(vols[F + i], vols[F + i + 1]) for i in range(F)]]

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

        forms = ("stream", "many")
        with torch.no_grad():
            net.reset_stream()
            net.forward_stream(vols[:1])                          # the stream starts with window 0 carried
            for form in forms:                                    # warm-up: workspace, clocks
                run(form, 2)
            res = {f: [] for f in forms}
            for r in range(a.rounds):
                for form in (forms if r % 2 == 0 else forms[::-1]):
                    res[form].append(run(form, a.calls))
                print(f"F={F} round {r}: " + "   ".join(f"{f} {res[f][-1]:7.1f}" for f in forms) + " frames/s", flush=True)
        rs = [s / m for s, m in zip(res["stream"], res["many"])]
        out = {"size": f"{w}x{h}", "n_first_channels": 5, "frames_per_call": F, "calls_per_run": a.calls, "rounds": a.rounds,
               **{f"{f}_fps": round(statistics.median(res[f]), 1) for f in forms},
               "stream_over_many": round(statistics.median(rs), 4), "stream_over_many_min": round(min(rs), 4),
               "stream_over_many_max": round(max(rs), 4), "stream_over_many_all": [round(x, 4) for x in rs],
               **{f"{f}_fps_all": [round(v, 1) for v in res[f]] for f in forms}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
