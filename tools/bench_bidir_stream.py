#!/usr/bin/env python3
"""Bidirectional streaming inference on one context: tools/bench_bidir_stream.py [--calls N] [--rounds R] [--frames F] [--fb-only]
[--only FORM]

At 1280x720 with seeded weights and synthetic volumes, F pairs of consecutive windows per call are timed three ways in one process:
  bidir   EEMFlow.forward_stream(bidirectional=True): F new windows per call, the window before them carried - 2 F flows, F windows
          encoded;
  many2   EEMFlow.forward_many on the F pairs plus forward_many on the F swapped pairs - the same 2 F flows, 4 F windows encoded (the
          only way to get them without the bidirectional stream);
  uni     EEMFlow.forward_stream: the same windows, F forward flows - what the backward direction is added to.
Each form runs N calls per round after a warm-up, the order rotating round by round, with HIP events around each run of N calls (the
graph replays are enqueued back to back).  Then the mask kernel alone: N calls of eemflow_fb_check_many on the last call's F pairs.
Prints pairs/s of each form per round, the median ratios with their spread, and one JSON line.
--fb-only: just the mask kernel's calls (for a `rocprofv3 --kernel-trace --stats` run of its own).
--only bidir | many2 | uni: N calls of that form alone after a warm-up (for a kernel trace of one form: its launches per call)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                      # noqa: E402
from eemflow_amd import EEMFlow                                   # noqa: E402
from eemflow_amd.metrics import fb_check_many                     # noqa: E402
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="calls per timed run")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the three forms")
    ap.add_argument("--frames", type=int, default=7, help="pairs per call (at most 8)")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--alpha", type=float, nargs=2, default=(0.01, 0.5))
    ap.add_argument("--fb-only", action="store_true", help="only the mask kernel's calls")
    ap.add_argument("--only", choices=("bidir", "many2", "uni"), default=None, help="only this form's calls")
    a = ap.parse_args()
    h, w, F = a.height, a.width, a.frames
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    net = net.cuda()
    net.change_imagesize((h, w))
    # a ring of 2 F + 1 distinct windows, reused call after call: stream calls alternate between its two halves
    vols = [torch.from_numpy(synthetic_voxel_pair(100 + i, 1, h, w)[0]).cuda() for i in range(2 * F + 1)]
    chunks = [vols[1:F + 1], vols[F + 1:2 * F + 1]]
    pairs = [[(vols[i], vols[i + 1]) for i in range(F)], [(vols[F + i], vols[F + i + 1]) for i in range(F)]]
    swapped = [[(b, c) for c, b in p] for p in pairs]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(form, calls, lead=2):
        # (the context caches four graphs and the three forms need five: `lead` untimed calls bring this form's back first)
        for c in range(lead):
            step(form, c)
        start.record()
        for c in range(calls):
            step(form, c)
        stop.record()
        stop.synchronize()
        return calls * F / (start.elapsed_time(stop) * 1e-3)

    def step(form, c):
        if form == "bidir":
            net.forward_stream(chunks[c % 2], bidirectional=True)
        elif form == "uni":
            net.forward_stream(chunks[c % 2])
        else:
            net.forward_many(pairs[c % 2])
            net.forward_many(swapped[c % 2])

    with torch.no_grad():
        net.reset_stream()
        net.forward_stream(vols[:1])                              # the stream starts with window 0 carried
        outs = net.forward_stream(chunks[0], bidirectional=True)
        fws, bws = [o[1][0] for o in outs], [o[2][0] for o in outs]

        def run_fb(calls):
            start.record()
            for _ in range(calls):
                fb_check_many(fws, bws, a.alpha[0], a.alpha[1], "all")
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) * 1e3 / (calls * F)   # us per pair, launch gaps included

        if a.fb_only:
            run_fb(10)
            print(json.dumps({"size": f"{w}x{h}", "pairs_per_call": F, "fb_check_us_per_pair_wall": run_fb(a.calls)}))
            return
        if a.only:
            run(a.only, 6)
            print(json.dumps({"size": f"{w}x{h}", "pairs_per_call": F, "form": a.only, "calls": a.calls + 10,
                              "pairs_per_s": run(a.only, a.calls)}))
            return
        forms = ("bidir", "many2", "uni")
        for form in forms * 2:                                    # warm-up: graph captures of every key, clocks
            run(form, 6)
        res = {f: [] for f in forms}
        for r in range(a.rounds):
            for form in forms[r % 3:] + forms[:r % 3]:
                res[form].append(run(form, a.calls))
            print(f"round {r}: bidir {res['bidir'][-1]:8.1f} pairs/s   2 x forward_many {res['many2'][-1]:8.1f} pairs/s   "
                  f"uni {res['uni'][-1]:8.1f} pairs/s   bidir / many2 {res['bidir'][-1] / res['many2'][-1]:.3f}   "
                  f"bidir / uni {res['bidir'][-1] / res['uni'][-1]:.3f}", flush=True)
        run_fb(10)
        fb = [run_fb(a.calls) for _ in range(a.rounds)]
    r_many = [b / m for b, m in zip(res["bidir"], res["many2"])]
    r_uni = [b / u for b, u in zip(res["bidir"], res["uni"])]
    med = statistics.median
    per_pair_bytes = 24.0 * h * w                                 # 16 B read (two flows) + 8 B written (two masks) per pixel
    out = {"size": f"{w}x{h}", "pairs_per_call": F, "calls_per_run": a.calls, "rounds": a.rounds,
           "bidir_pairs_per_s": med(res["bidir"]), "many2_pairs_per_s": med(res["many2"]), "uni_pairs_per_s": med(res["uni"]),
           "bidir_over_many2": med(r_many), "bidir_over_many2_min": min(r_many), "bidir_over_many2_max": max(r_many),
           "bidir_over_uni": med(r_uni), "bidir_over_uni_min": min(r_uni), "bidir_over_uni_max": max(r_uni),
           "backward_direction_us_per_pair": 1e6 / med(res["bidir"]) - 1e6 / med(res["uni"]),
           "fb_check_us_per_pair_wall": med(fb), "fb_check_tb_per_s_wall": per_pair_bytes / (med(fb) * 1e-6) / 1e12,
           "bidir_all": [round(v, 1) for v in res["bidir"]], "many2_all": [round(v, 1) for v in res["many2"]],
           "uni_all": [round(v, 1) for v in res["uni"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
