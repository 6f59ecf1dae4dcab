#!/usr/bin/env python3
"""E-RAFT streaming inference against pairwise inference on one context:
tools/bench_eraft_stream.py [--calls N] [--rounds R] [--frames F ...]

At 640x480, 12 iterations, final_only, seeded weights and synthetic volumes, a stream of consecutive windows is timed four ways in
the same process, for each F (flows per call):
  cold    ERAFT.forward_stream (warm_start False): F new windows per call, the window before them carried - F windows through fnet;
  many    ERAFT.forward_many on the same F pairs (v_i, v_{i+1}) - 2 F windows through fnet, the same batch-F update loop;
  warm    ERAFT.forward_stream (warm_start True): the same calls, the pairs' update loops at batch 1, each from the previous pair's
          forward-interpolated flow_low;
  chain   F batch-1 ERAFT.forward calls chained through forward_interpolate(stage("flow_low")) - E-RAFT's warm start done by hand.
The forms run N calls per round after a warm-up, in an order that alternates round by round, with HIP events around each run of N
calls.  Prints frames/s per round, the median ratios cold / many and warm / chain with their spread, and one JSON line per F."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                      # noqa: E402
from eemflow_amd.eraft import ERAFT, forward_interpolate          # noqa: E402
from eemflow_amd.eraft_weights import seeded_from_shapes          # noqa: E402
from eemflow_amd.weights import synthetic_voxel_pair              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="calls per timed run")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the forms")
    ap.add_argument("--frames", type=int, nargs="+", default=[4, 8], help="flows per call")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--iters", type=int, default=12)
    a = ap.parse_args()
    h, w, iters = a.height, a.width, a.iters
    net = ERAFT("", n_first_channels=5).eval()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_from_shapes(shapes, 0).items()})
    net = net.cuda()
    net.change_imagesize((h, w))
    net.final_only = True
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for F in a.frames:
        vols = [torch.from_numpy(synthetic_voxel_pair(100 + i, 1, h, w)[0]).cuda() for i in range(2 * F + 1)]
        chunks = [vols[1:F + 1], vols[F + 1:2 * F + 1]]           # stream calls alternate between the two halves of the ring
        pairs = [[(vols[i], vols[i + 1]) for i in range(F)], [(vols[F + i], vols[F + i + 1]) for i in range(F)]]
        state = {"init": None}

        def run(form, calls):
            net.warm_start = form == "warm"
            start.record()
            for c in range(calls):
                if form in ("cold", "warm"):
                    net.forward_stream(chunks[c % 2], iters=iters)
                elif form == "many":
                    net.forward_many(pairs[c % 2], iters=iters)
                else:
                    for e1, e2 in pairs[c % 2]:
                        net(e1, e2, iters=iters, flow_init=state["init"])
                        state["init"] = forward_interpolate(net.stage("flow_low"))
            stop.record()
            stop.synchronize()
            return calls * F / (start.elapsed_time(stop) * 1e-3)

        forms = ("cold", "many", "warm", "chain")
        with torch.no_grad():
            net.reset_stream()
            net.forward_stream(vols[:1], iters=iters)             # the stream starts with window 0 carried
            for form in forms:                                    # warm-up: workspace, clocks
                run(form, 2)
            res = {f: [] for f in forms}
            for r in range(a.rounds):
                for form in (forms if r % 2 == 0 else forms[::-1]):
                    res[form].append(run(form, a.calls))
                print(f"F={F} round {r}: " + "   ".join(f"{f} {res[f][-1]:7.1f}" for f in forms) + " frames/s", flush=True)
        rc = [c / m for c, m in zip(res["cold"], res["many"])]
        rw = [x / y for x, y in zip(res["warm"], res["chain"])]
        out = {"size": f"{w}x{h}", "iters": iters, "final_only": True, "frames_per_call": F, "calls_per_run": a.calls, "rounds": a.rounds,
               **{f"{f}_fps": round(statistics.median(res[f]), 1) for f in forms},
               "cold_over_many": round(statistics.median(rc), 4), "cold_over_many_min": round(min(rc), 4), "cold_over_many_max": round(max(rc), 4),
               "warm_over_chain": round(statistics.median(rw), 4), "warm_over_chain_min": round(min(rw), 4),
               "warm_over_chain_max": round(max(rw), 4),
               **{f"{f}_fps_all": [round(v, 1) for v in res[f]] for f in forms}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
