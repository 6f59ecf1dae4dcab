#!/usr/bin/env python3
"""HREM event sets prepared on the GPU from the npz columns: kernel cost, read_sample, and what the loader delivers with and without it.
tools/bench_event_pack.py [--calls N] [--rounds R] [--samples S] [--out FILE] [--kernels-only]

(a) Microseconds per event SET of eemflow_pack_events_many (the C entry point on columns already resident on the device: the launch of
    a call, launch gaps included) at 2e5 and 2e6 events per set and 1, 10 and 32 sets per call, HREM's column dtypes (t int64, x and
    y uint16, p int8).  HIP events around N back-to-back calls after a warm-up, the median of R rounds.  Bytes moved = 13 B read + 32 B
    written per event, set against the chip's 5.5 TB/s copy rate (read + write bytes per second).  Every set has its own columns and
    output.
(b) Milliseconds per sample until both event sets of a sample are (N,4) float64 tensors on the device, single thread, host clock
    around a call that ends synchronised: the host route (read_sample's NumPy passes, then the voxelizer front-end's astype and
    upload from pageable memory) against device_events=True (read_sample: columns, pinned staging, one copy, one launch).  Both include
    the .flo file and the mesh flow of read_sample.  Best of R rounds over S samples, files in the page cache.
(c) Samples/s that ThreadedBatchLoader(device_batches=True) delivers for hrem_1280x720 at batch 8 with 4 threads over sorted synthetic
    files, and the wall time per EEMFlowTrainer.step when the training loop is fed by it, with device_events off and on.  Both routes
    in one process, alternating, R rounds, every round's value printed.
Writes the lines and one JSON line to --out (default profiles/r17_event_pack_bench.txt beside this tool) and to stdout.
--kernels-only: just (a) at 32 sets per call (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
from eemflow_amd import EEMFlow, _lib, hrem                       # noqa: E402
from eemflow_amd import events as E                               # noqa: E402
from eemflow_amd.loader import ThreadedBatchLoader                # noqa: E402
from eemflow_amd.train import EEMFlowTrainer                      # noqa: E402
from eemflow_amd.weights import seeded_state_dict                 # noqa: E402

COPY_RATE = 5.5e12                                                # bytes read + written per second by a plain device copy
BATCH, THREADS = 8, 4
H, W = 720, 1280
BYTES_PER_EVENT = 13 + 32


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


def sorted_columns(seed, n):
    rng = np.random.default_rng(seed)
    t = np.sort(np.round(rng.uniform(0, 0.05, n) * 1e9).astype(np.int64)) + 123456789
    return t, rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16), (rng.integers(0, 2, n) * 2 - 1).astype(np.int8)


def kernel_rows(calls, rounds, counts, sizes, say):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    stream = _lib.current_stream_ptr(dev)
    out = {}
    for n in sizes:
        kmax = max(counts)
        host = sorted_columns(n, n)
        cols = [[torch.from_numpy(c.copy()).to(dev) for c in host] for _ in range(kmax)]      # every set its own buffers
        outs = [torch.empty(n, 4, dtype=torch.float64, device=dev) for _ in range(kmax)]
        ncalls = calls if n < 1_000_000 else max(4, calls // 5)
        for k in counts:
            arr = ctypes.c_void_p * k
            ptrs = [arr(*[cols[i][c].data_ptr() for i in range(k)]) for c in range(4)]
            codes = (ctypes.c_int * (4 * k))(*[E.DTYPE_CODES[c.dtype] for _ in range(k) for c in host])
            ns = (ctypes.c_int64 * k)(*[n] * k)
            po = arr(*[o.data_ptr() for o in outs[:k]])

            def call():
                _lib.check(L.eemflow_pack_events_many(k, ptrs[0], ptrs[1], ptrs[2], ptrs[3], codes, ns, 1e-9, 1e6, 1, po, stream))
            med, lo, hi = timed(call, ncalls, rounds, k)
            moved = n * BYTES_PER_EVENT
            rate = moved / (med * 1e-6)
            key = f"pack_{n:.0e}_k{k}".replace("+0", "")
            out[key + "_us_per_set"], out[key + "_copy_rate_fraction"] = med, rate / COPY_RATE
            say(f"pack_events_many {n:.0e} events per set {k:2d} sets per call: {med:9.2f} us per set (min {lo:.2f}, max {hi:.2f} over {rounds} "
                f"rounds of {ncalls} calls)  {moved / 1e6:6.1f} MB moved per set (13 B in + 32 B out per event) = {rate / 1e12:5.2f} TB/s = "
                f"{rate / COPY_RATE:.2f} of the copy rate")
        want = torch.from_numpy(E.host_events(host)).to(dev)
        assert torch.equal(outs[0].view(torch.int64), want.view(torch.int64)), "the timed kernel's output is not the host route's"
        del cols, outs
        torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------ (b), (c): files
def hrem_tree(root, samples, events):
    flows = [hrem.synthetic_flow(900 + i, H, W) for i in range(2)]
    for i in range(samples):
        d = os.path.join(root, "dataset/HREM/train/dt1/%06d" % i)
        os.makedirs(d)
        for name, seed in (("events1.npz", 2 * i), ("events2.npz", 2 * i + 1)):
            ev = hrem.synthetic_hrem_events(seed, events, H, W)
            hrem.write_events_npz(os.path.join(d, name), ev[np.argsort(ev[:, 0], kind="stable")])     # recordings are in time order
        hrem.write_flo(os.path.join(d, "flow.flo"), flows[i % 2])


def dataset(root, device_events):
    args = {"eval_type": "dense", "event_interval": "dt1", "num_voxel_bins": 5, "aug_params": {"crop_size": [H, W], "do_flip": True}}
    return hrem.HREMEventFlow(args, train=True, root=root, device_events=device_events)


def events_on_device(ds, i):
    """read_sample, then what the voxelizer's front-end does first: both event sets as (N,4) float64 device tensors; synchronised."""
    _, seqs = ds.read_sample(i)
    evs = [s.features if isinstance(s.features, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s.features.astype('float'))).to(ds.device)
           for s in seqs]
    torch.cuda.synchronize()
    return evs


def read_rows(tag, sets, rounds, say):
    out = {}
    n = len(sets[False])
    for v in (False, True):
        for i in range(n):
            events_on_device(sets[v], i)                          # warm-up: page cache, the pinned staging buffer
    a, b = events_on_device(sets[False], 0), events_on_device(sets[True], 0)
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b)), "the routes disagree"
    res = {False: [], True: []}
    for r in range(rounds):
        for v in ((False, True) if r % 2 == 0 else (True, False)):
            t0 = time.perf_counter()
            for i in range(n):
                events_on_device(sets[v], i)
            res[v].append((time.perf_counter() - t0) / n * 1e3)
    out[f"{tag}_read_host_ms_per_sample"], out[f"{tag}_read_device_ms_per_sample"] = min(res[False]), min(res[True])
    say(f"read_sample + events on the device, {tag} events per set, one thread: host route {min(res[False]):8.2f} ms per sample   device_events "
        f"{min(res[True]):8.2f} ms per sample   ratio {min(res[False]) / min(res[True]):.2f}   (best of rounds: host "
        f"{[round(t, 2) for t in res[False]]}, device {[round(t, 2) for t in res[True]]})")
    return out


def loader_rows(tag, sets, trainer, rounds, say):
    dev = torch.device("cuda:0")
    loaders = {v: ThreadedBatchLoader(sets[v], BATCH, shuffle=True, threads=THREADS, drop_last=True, device_batches=True) for v in (False, True)}

    def epoch(v, step):
        np.random.seed(1)
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        for batch in loaders[v]:
            e1, e2 = batch['event_volume_old'].to(dev).float(), batch['event_volume_new'].to(dev).float()
            fl, va = batch['flow'].to(dev).float(), batch['valid'].to(dev).float()
            if step:
                trainer.step(e1, e2, fl, va)
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n                      # seconds per batch

    out = {}
    for step in (False, True):
        for v in (False, True):
            epoch(v, step)                                        # warm-up: file cache, scratch arenas, staging buffers, the step's workspaces
        res = {False: [], True: []}
        for r in range(rounds):
            for v in ((False, True) if r % 2 == 0 else (True, False)):
                res[v].append(epoch(v, step))
        host, devb = statistics.median(res[False]), statistics.median(res[True])
        if not step:
            per = {v: [round(BATCH / t, 1) for t in res[v]] for v in res}
            out[f"{tag}_host_samples_per_s"], out[f"{tag}_device_samples_per_s"] = BATCH / host, BATCH / devb
            out[f"{tag}_host_samples_per_s_rounds"], out[f"{tag}_device_samples_per_s_rounds"] = per[False], per[True]
            out[f"{tag}_device_slowest_above_host_fastest"] = min(per[True]) > max(per[False])
            say(f"loader hrem_1280x720 {tag} events per set, batch {BATCH}, {THREADS} threads, device_batches, {len(sets[False])} samples per epoch: "
                f"device_events off {BATCH / host:8.1f} samples/s   on {BATCH / devb:8.1f} samples/s   ratio {host / devb:.2f}   (rounds: off "
                f"{per[False]}, on {per[True]}; slowest on-round above fastest off-round: {min(per[True]) > max(per[False])})")
        else:
            per = {v: [round(t * 1e3, 2) for t in res[v]] for v in res}
            out[f"{tag}_host_fed_step_ms"], out[f"{tag}_device_fed_step_ms"] = host * 1e3, devb * 1e3
            out[f"{tag}_host_fed_step_ms_rounds"], out[f"{tag}_device_fed_step_ms_rounds"] = per[False], per[True]
            say(f"trainer.step hrem_1280x720 {tag} events per set, batch {BATCH} fed by the loader: device_events off {host * 1e3:8.2f} ms per step   "
                f"on {devb * 1e3:8.2f} ms per step   ratio {host / devb:.2f}   (rounds: off {per[False]}, on {per[True]})")
    for ld in loaders.values():
        ld.close()
    say(f"event_routes {tag}: device_events off {sets[False].event_routes}, on {sets[True].event_routes}")
    out[f"{tag}_event_routes_on"] = dict(sets[True].event_routes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="library calls per timed run (a fifth of it at 2e6 events)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16, help="samples of each synthetic dataset (one epoch = samples / 8 batches)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17_event_pack_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_event_pack.py measures on the GPU: no device found")
    if a.rounds < 3 and not a.kernels_only:
        raise SystemExit("--rounds: at least three rounds per route")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    sizes = (200_000, 2_000_000)
    if a.kernels_only:
        print(json.dumps(kernel_rows(a.calls, 1, (32,), sizes, say)))
        return
    say(f"tools/bench_event_pack.py --calls {a.calls} --rounds {a.rounds} --samples {a.samples} (MI355X, one process)")
    res = {"calls_per_run": a.calls, "rounds": a.rounds, "samples": a.samples}
    res.update(kernel_rows(a.calls, a.rounds, (1, 10, 32), sizes, say))
    dev = torch.device("cuda:0")
    net = EEMFlow("", 5, 5, out_mesh_size=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    net = net.to(dev).train()
    net.change_imagesize((H, W))
    trainer = EEMFlowTrainer(net, lr=1e-4, num_steps=100000)
    for n in sizes:
        tag = f"{n:.0e}".replace("+0", "")
        with tempfile.TemporaryDirectory() as root:
            hrem_tree(root, a.samples, n)
            sets = {v: dataset(root, v) for v in (False, True)}
            res.update(read_rows(tag, sets, a.rounds, say))
            for ds in sets.values():
                ds.event_routes.update(device=0, host=0)
            res.update(loader_rows(tag, sets, trainer, a.rounds, say))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
