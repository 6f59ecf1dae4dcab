#!/usr/bin/env python3
"""Image of warped events / flow warp loss: kernel cost and cost inside the stream evaluation.
tools/bench_iwe.py [--calls N] [--rounds R] [--samples S] [--out FILE] [--kernels-only] [--grad]

(a) Microseconds per EVENT SET of eemflow_iwe_many at 1280x720 with 2e6 events per set and at 346x260 with 2e5, for 1, 10 and 16 sets
    per call, in the binned form and in the direct form (EEM_IWE_DIRECT=1): `iwe` = one job per set under a smooth flow; `fwl` = what
    fwl_many launches, every set twice - under its flow and under zero flow.  HIP events around N back-to-back library calls after a
    warm-up (images, moments, t0 and scale prepared: the launches of a call, launch gaps included), the median of R rounds.  In the same
    run, the yardstick: voxelize_many_device(normalize=False, 5 bins) on the same event sets.  Events have integer coordinates and
    uniformly random pixels, time-sorted, as a sensor delivers them; the flow moves them by up to 8 px, so nearly every event makes two
    row records (the voxelizer: one record per event).
(b) The stream evaluation (TestRaftEvents.test_multi_sequence(stream=16)) on a synthetic MVSEC sequence of S samples (260x346 windows of
    20 000 events cropped to 256x256, a dataset built with with_events=True): frames/s without and with fwl=True; alternating, R rounds.
Writes the lines and one JSON line to --out (default profiles/r14_iwe_bench.txt beside this tool) and to stdout.
--kernels-only: just (a)'s binned calls at 10 sets (for a `rocprofv3 --kernel-trace --stats` run of its own).
--grad: the contrast loss instead of (a) and (b) (default --out profiles/r16_iwe_grad_bench.txt):
(c) microseconds per event set of iwe.fwl_loss FORWARD PLUS BACKWARD (loss.backward() into a (k,2,H,W) leaf) at the same sizes, event
    counts, sets per call and forms, and beside it, in the same run, iwe.fwl_many - the forward alone.  Both are the Python calls, their
    one copy of the sets' end timestamps to the host included;
(d) the training step (TrainRaftEvents, engine='autograd', EEMFlow at 346x260, batch 8, batches of 20 000 events per sample with
    flip-and-crop event maps, fed from a list): milliseconds per step without and with contrast_weight=0.5; alternating, R rounds."""
import argparse
import contextlib
import ctypes
import io
import json
import math
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
from eemflow_amd import EEMFlow, _lib                             # noqa: E402
from eemflow_amd.harness import Logger, TestRaftEvents            # noqa: E402
from eemflow_amd.mvsec import MvsecEventFlow                      # noqa: E402
from eemflow_amd.voxelizer import voxelize_many_device            # noqa: E402
from eemflow_amd.weights import seeded_state_dict                 # noqa: E402

SIZES = ((720, 1280, 2_000_000), (260, 346, 200_000))


def event_sets(k, n, h, w, dev):
    g = torch.Generator(device=dev).manual_seed(k * 1000 + h)
    sets = []
    for _ in range(k):
        ev = torch.empty(n, 4, dtype=torch.float64, device=dev)
        ev[:, 0] = torch.sort(torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 0.05).values
        ev[:, 1] = torch.randint(0, w, (n,), generator=g, device=dev).double()
        ev[:, 2] = torch.randint(0, h, (n,), generator=g, device=dev).double()
        ev[:, 3] = torch.randint(0, 2, (n,), generator=g, device=dev).double() * 2 - 1
        sets.append(ev)
    return sets


def smooth_flow(h, w, dev):
    y, x = torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64)
    u, v = 6.0 * torch.sin(2 * math.pi * x / w) + 2.0, 4.0 * torch.cos(2 * math.pi * y / h)
    return torch.stack([u[None, :].expand(h, w), v[:, None].expand(h, w)]).float().contiguous().to(dev)


def timed(call, calls, rounds, per):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        start.record()
        for _ in range(calls):
            call()
        stop.record()
        stop.synchronize()
        us.append(start.elapsed_time(stop) * 1e3 / (calls * per))
    return statistics.median(us), min(us), max(us)


def kernel_rows(calls, rounds, counts, forms, say):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    sp = _lib.current_stream_ptr(dev)
    out = {}
    for h, w, n in SIZES:
        flow = smooth_flow(h, w, dev)
        all_sets = event_sets(max(counts), n, h, w, dev)
        images = [torch.empty(2, h, w, dtype=torch.float32, device=dev) for _ in range(2 * max(counts))]
        moments = torch.empty(2 * max(counts), 4, dtype=torch.float64, device=dev)
        ncalls = max(2, calls // 10) if n >= 1_000_000 else calls
        for k in counts:
            sets = all_sets[:k]
            ends = torch.stack([e[-1, 0] for e in sets]).tolist()
            firsts = torch.stack([e[0, 0] for e in sets]).tolist()

            def args(jobs_sets, jobs_flows):
                c = len(jobs_sets)
                ptr, dbl = ctypes.c_void_p * c, ctypes.c_double * c
                t0 = ends * (c // k)
                sc = [-1.0 / (a - b) for a, b in zip(ends, firsts)] * (c // k)
                return (c, ptr(*[e.data_ptr() for e in jobs_sets]), (ctypes.c_int64 * c)(*[e.shape[0] for e in jobs_sets]),
                        ptr(*[f.data_ptr() if f is not None else None for f in jobs_flows]), dbl(*t0), dbl(*sc), 0.0, 0.0, h, w,
                        ptr(*[t.data_ptr() for t in images[:c]]), moments.data_ptr(), sp)
            a_iwe = args(sets, [flow] * k)
            a_fwl = args(sets + sets, [flow] * k + [None] * k)
            tag = f"{w}x{h}_n{k}"
            for form in forms:
                os.environ["EEM_IWE_DIRECT"] = "1" if form == "direct" else "0"
                for name, a in (("iwe", a_iwe), ("fwl", a_fwl)):
                    med, lo, hi = timed(lambda: _lib.check(L.eemflow_iwe_many(*a)), ncalls, rounds, k)
                    out[f"{name}_{form}_{tag}_us_per_set"] = med
                    say(f"{name} {form:6s} {w}x{h} {n:.0e} events  {k:2d} sets per call: {med:9.2f} us per event set "
                        f"(min {lo:.2f}, max {hi:.2f} over {rounds} rounds of {ncalls} calls)")
            os.environ.pop("EEM_IWE_DIRECT", None)
            grids = [torch.empty(5, h, w, dtype=torch.float32, device=dev) for _ in range(k)]
            med, lo, hi = timed(lambda: voxelize_many_device(sets, 5, h, w, normalize=False, out=grids), ncalls, rounds, k)
            out[f"voxelize_{tag}_us_per_set"] = med
            say(f"voxelize_many_device(normalize=False, 5 bins) {w}x{h} {n:.0e} events  {k:2d} sets per call: {med:9.2f} us per event set "
                f"(min {lo:.2f}, max {hi:.2f})   iwe binned / voxelize = {out[f'iwe_binned_{tag}_us_per_set'] / med:.2f}"
                if "binned" in forms else f"voxelize {tag}: {med:.2f} us per event set")
        del all_sets, images
        torch.cuda.empty_cache()
    return out


def grad_rows(calls, rounds, counts, forms, say):
    import importlib
    iwe = importlib.import_module("eemflow_amd.iwe")
    dev = torch.device("cuda:0")
    out = {}
    for h, w, n in SIZES:
        flow = smooth_flow(h, w, dev)
        all_sets = event_sets(max(counts), n, h, w, dev)
        ncalls = max(2, calls // 10) if n >= 1_000_000 else calls
        for k in counts:
            sets = all_sets[:k]
            pred = flow[None].repeat(k, 1, 1, 1).requires_grad_(True)
            flows = [pred[i] for i in range(k)]
            plain = [f.detach() for f in flows]

            def both():
                pred.grad = None
                iwe.fwl_loss(sets, flows).backward()
            tag = f"{w}x{h}_n{k}"
            for form in forms:
                os.environ["EEM_IWE_DIRECT"] = "1" if form == "direct" else "0"
                fwd, flo, fhi = timed(lambda: iwe.fwl_many(sets, plain), ncalls, rounds, k)
                med, lo, hi = timed(both, ncalls, rounds, k)
                out[f"fwl_many_{form}_{tag}_us_per_set"] = fwd
                out[f"fwl_loss_fwd_bwd_{form}_{tag}_us_per_set"] = med
                say(f"fwl_loss forward + backward {form:6s} {w}x{h} {n:.0e} events  {k:2d} sets per call: {med:9.2f} us per event set "
                    f"(min {lo:.2f}, max {hi:.2f} over {rounds} rounds of {ncalls} calls)   fwl_many, forward alone: {fwd:9.2f} "
                    f"(min {flo:.2f}, max {fhi:.2f})")
            os.environ.pop("EEM_IWE_DIRECT", None)
        del all_sets
        torch.cuda.empty_cache()
    return out


def training_rows(rounds, say, h=260, w=346, batch=8, steps=20):
    from eemflow_amd.augmentor import AugPlan, event_map_after_offset
    from eemflow_amd.harness import TrainRaftEvents
    from eemflow_amd.weights import synthetic_gt, synthetic_voxel_pair
    dev = torch.device("cuda:0")

    def make_batch(seed):
        e1, e2 = (torch.from_numpy(a).to(dev) for a in synthetic_voxel_pair(seed, batch, h, w))
        gt, valid = (torch.from_numpy(a).to(dev) for a in synthetic_gt(seed + 1, batch, h, w))
        plans = [AugPlan(h + 8, w + 8, crop=(h, w), y0=i % 8, x0=(3 * i) % 8, hflip=i % 2 == 0) for i in range(batch)]
        return {"event_volume_old": e1, "event_volume_new": e2, "flow": gt, "valid": valid,
                "events": event_sets(batch, 20000, h + 8, w + 8, dev),
                "events_map": [event_map_after_offset(p, (0, 0), h + 8, w + 8) for p in plans]}
    batches = [make_batch(200 + 10 * i) for i in range(4)] * (steps // 4)
    res = {0.0: [], 0.5: []}
    nets = {}
    for wgt in res:
        net = EEMFlow("", groups=5, n_first_channels=5)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(68).items()})
        nets[wgt] = (net.cuda().train(), TrainRaftEvents(batches, (h, w), lr=1e-6, logger=Logger(verbose=False), engine="autograd",
                                                         contrast_weight=wgt))

    def run(wgt):
        net, tr = nets[wgt]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_iters(net, val_iters=len(batches))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches)
    run(0.0), run(0.5)                                            # warm-up: workspaces, scratch arenas
    for r in range(rounds):
        for wgt in ((0.0, 0.5) if r % 2 == 0 else (0.5, 0.0)):
            res[wgt].append(run(wgt))
        say(f"round {r}: training step {w}x{h} batch {batch}, autograd engine: {res[0.0][-1]:8.2f} ms   with contrast_weight=0.5 "
            f"{res[0.5][-1]:8.2f} ms   ratio {res[0.5][-1] / res[0.0][-1]:.3f}")
    return {"train_step_ms": statistics.median(res[0.0]), "train_step_contrast_ms": statistics.median(res[0.5])}


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
    return MvsecEventFlow(args, train=False, root=root, events_reader=reader, valid_time_index={"seqA": [(first, first + n_samples)]},
                          with_events=True)


def evaluation_rows(samples, rounds, say):
    out = {}
    with tempfile.TemporaryDirectory() as root:
        ds = mvsec_dataset(root, samples)
        net = EEMFlow("", groups=5, n_first_channels=5).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(68).items()})
        net = net.cuda()
        tester = TestRaftEvents(ds, (256, 256), logger=Logger(verbose=False))

        def run(fwl):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=16, fwl=fwl)
            torch.cuda.synchronize()
            return samples / (time.perf_counter() - t0)

        run(False), run(True)                                     # warm-up: graph captures, scratch arenas
        res = {False: [], True: []}
        for r in range(rounds):
            for v in ((False, True) if r % 2 == 0 else (True, False)):
                res[v].append(run(v))
            say(f"round {r}: stream evaluation {res[False][-1]:8.1f} frames/s   with fwl=True {res[True][-1]:8.1f} frames/s   "
                f"ratio {res[True][-1] / res[False][-1]:.3f}")
    out["stream_eval_frames_per_s"] = statistics.median(res[False])
    out["stream_eval_fwl_frames_per_s"] = statistics.median(res[True])
    out["stream_eval_fwl_ratio"] = statistics.median([a / b for a, b in zip(res[True], res[False])])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="library calls per timed run (a tenth of it at 2e6 events per set)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=96, help="samples of the synthetic MVSEC sequence")
    ap.add_argument("--out", default=None, help="default: profiles/r14_iwe_bench.txt, with --grad profiles/r16_iwe_grad_bench.txt")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--grad", action="store_true", help="measure the contrast loss (fwl_loss forward + backward, the training step) instead")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "r16_iwe_grad_bench.txt" if a.grad else "r14_iwe_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("bench_iwe.py measures on the GPU: no device found")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if a.kernels_only:
        print(json.dumps(kernel_rows(a.calls, 1, (10,), ("binned",), say)))
        return
    say(f"tools/bench_iwe.py{' --grad' if a.grad else ''} --calls {a.calls} --rounds {a.rounds} --samples {a.samples} (MI355X, one process): HIP events around "
        f"back-to-back library calls per round after a warm-up, launch gaps included")
    res = {"calls_per_run": a.calls, "rounds": a.rounds}
    if a.grad:
        res.update(grad_rows(a.calls, a.rounds, (1, 10, 16), ("binned", "direct"), say))
        res.update(training_rows(a.rounds, say))
    else:
        res.update(kernel_rows(a.calls, a.rounds, (1, 10, 16), ("binned", "direct"), say))
        res.update(evaluation_rows(a.samples, a.rounds, say))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
