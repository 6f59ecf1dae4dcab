#!/usr/bin/env python3
"""Visualisation kernels and their cost inside the stream evaluation: tools/bench_viz.py [--calls N] [--rounds R] [--out FILE]
[--kernels-only] [--samples S]

(a) At 1280x720 and n = 1, 10 and 16 frames per call: microseconds per frame of eemflow_flow_to_image_many and of
    eemflow_event_image_many (5 bins), HIP events around N back-to-back library calls after a warm-up (outputs and stats preallocated:
    the two launches and the memset of a call, launch gaps included), the median of R rounds, and the share of the 5.5 TB/s copy rate
    the project's other rows use that the algorithmic bytes amount to: per flow frame 2 x 7.37 MB read (both passes read both planes)
    + 2.76 MB written; per event frame 2 x 18.43 MB read + 2.76 MB written.
(b) The stream evaluation (TestRaftEvents.test_multi_sequence(stream=16)) on a synthetic MVSEC sequence of S samples (260x346 windows
    cropped to 256x256, events from an injected reader, flow files in a temporary folder): frames/s without visualisation, and with
    visualize_map=True, vis_events=True and a writer that copies every image to pinned host memory but does not encode it - what the
    conversions and copies add to the loop; alternating, R rounds.
Writes the lines and one JSON line to --out (default profiles/r13_viz_bench.txt beside this tool) and to stdout.
--kernels-only: just (a)'s calls at n = 10 (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import tempfile
import time
import contextlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
from eemflow_amd import EEMFlow, _lib, viz                        # noqa: E402
from eemflow_amd.harness import Logger, TestRaftEvents            # noqa: E402
from eemflow_amd.mvsec import MvsecEventFlow                      # noqa: E402
from eemflow_amd.weights import seeded_state_dict                 # noqa: E402

COPY_RATE = 5.5e12                                                # B/s: the copy rate of profiles/r05_dma_pieces.txt's best row
H, W, BINS = 720, 1280, 5


def kernel_rows(calls, rounds, sizes, say):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    sp = _lib.current_stream_ptr(dev)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = torch.Generator(device="cpu").manual_seed(1)
    out = {}
    for n in sizes:
        flows = [(torch.randn(2, H, W, generator=g) * 8).to(dev) for _ in range(n)]
        vols = [(torch.randn(BINS, H, W, generator=g) * (torch.rand(BINS, H, W, generator=g) < 0.1)).to(dev) for _ in range(n)]
        imgs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
        stats = torch.empty(n, 4, dtype=torch.float64, device=dev)
        arr = ctypes.c_void_p * n
        af, av, ai = arr(*[t.data_ptr() for t in flows]), arr(*[t.data_ptr() for t in vols]), arr(*[t.data_ptr() for t in imgs])

        def flow_call():
            _lib.check(L.eemflow_flow_to_image_many(n, af, ai, stats.data_ptr(), H, W, 0, sp))

        def event_call():
            _lib.check(L.eemflow_event_image_many(n, av, None, BINS, H, W, ai, stats.data_ptr(), 0, sp))

        for name, call, nbytes in (("flow", flow_call, 2 * 2 * H * W * 4 + 3 * H * W), ("event", event_call, 2 * BINS * H * W * 4 + 3 * H * W)):
            for _ in range(10):
                call()
            us = []
            for _ in range(rounds):
                start.record()
                for _ in range(calls):
                    call()
                stop.record()
                stop.synchronize()
                us.append(start.elapsed_time(stop) * 1e3 / (calls * n))
            med = statistics.median(us)
            out[f"{name}_n{n}_us_per_frame"] = med
            out[f"{name}_n{n}_us_per_frame_min_max"] = [min(us), max(us)]
            out[f"{name}_n{n}_share_of_copy_rate"] = nbytes / (med * 1e-6) / COPY_RATE
            say(f"{name:5s} image  n = {n:2d}: {med:8.2f} us per frame (min {min(us):.2f}, max {max(us):.2f} over {rounds} rounds of {calls} calls)   "
                f"{nbytes / 1e6:.2f} MB per frame -> {nbytes / (med * 1e-6) / 1e12:.3f} TB/s = {nbytes / (med * 1e-6) / COPY_RATE:.3f} of the copy rate")
    return out


def mvsec_dataset(root, n_samples, first=40):
    flow_dir = os.path.join(root, "dataset", "MVSEC", "seqA", "flowgt_dt1")
    os.makedirs(flow_dir)
    rng = np.random.default_rng(5)
    for i in range(first, first + n_samples):
        np.save(os.path.join(flow_dir, f"{i}.npy"), rng.normal(0, 2, (2, 260, 346)).astype(np.float32))

    def reader(path):
        k = int(os.path.basename(path).split(".")[0])
        r = np.random.default_rng(10_000 + k)
        m = 20000
        ts = np.sort(r.uniform(k * 0.05, (k + 1) * 0.05, m))
        return np.stack([ts, r.integers(0, 346, m), r.integers(0, 260, m), r.integers(0, 2, m) * 2 - 1], axis=1).astype(np.float64)

    args = {"eval_type": "dense", "num_voxel_bins": 5, "sequence": "seqA"}
    return MvsecEventFlow(args, train=False, root=root, events_reader=reader, valid_time_index={"seqA": [(first, first + n_samples)]})


class CopyOnlyWriter(viz.ImageWriter):
    """Copies to pinned memory and waits for the copy like the real writer; encodes nothing."""

    def encode(self, path, array):
        pass


def evaluation_rows(samples, rounds, say):
    out = {}
    with tempfile.TemporaryDirectory() as root:
        ds = mvsec_dataset(root, samples)
        net = EEMFlow("", groups=5, n_first_channels=5).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(68).items()})
        net = net.cuda()
        tester = TestRaftEvents(ds, (256, 256), logger=Logger(verbose=False))
        real = viz.ImageWriter
        viz.ImageWriter = CopyOnlyWriter
        try:
            def run(visualize):
                extra = dict(visualize_map=True, vis_events=True, save_path=os.path.join(root, "out")) if visualize else {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=16, **extra)
                torch.cuda.synchronize()
                return samples / (time.perf_counter() - t0)

            run(False), run(True)                                 # warm-up: graph captures, pinned buffers, threads
            res = {False: [], True: []}
            for r in range(rounds):
                for v in ((False, True) if r % 2 == 0 else (True, False)):
                    res[v].append(run(v))
                say(f"round {r}: stream evaluation {res[False][-1]:8.1f} frames/s   with visualize_map + vis_events (copy, no encode) "
                    f"{res[True][-1]:8.1f} frames/s   ratio {res[True][-1] / res[False][-1]:.3f}")
        finally:
            viz.ImageWriter = real
    out["stream_eval_frames_per_s"] = statistics.median(res[False])
    out["stream_eval_visualize_frames_per_s"] = statistics.median(res[True])
    out["stream_eval_visualize_ratio"] = statistics.median([a / b for a, b in zip(res[True], res[False])])
    out["stream_eval_all"] = [round(v, 1) for v in res[False]]
    out["stream_eval_visualize_all"] = [round(v, 1) for v in res[True]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="library calls per timed run")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=96, help="samples of the synthetic MVSEC sequence")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r13_viz_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_viz.py measures on the GPU: no device found")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if a.kernels_only:
        print(json.dumps(kernel_rows(a.calls, 1, (10,), say)))
        return
    say(f"tools/bench_viz.py --calls {a.calls} --rounds {a.rounds} --samples {a.samples} (MI355X, one process): {W}x{H}, HIP events around "
        f"{a.calls} back-to-back library calls per round after a warm-up, launch gaps included")
    res = {"size": f"{W}x{H}", "calls_per_run": a.calls, "rounds": a.rounds}
    res.update(kernel_rows(a.calls, a.rounds, (1, 10, 16), say))
    res.update(evaluation_rows(a.samples, a.rounds, say))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
