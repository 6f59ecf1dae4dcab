#!/usr/bin/env python3
"""Training-sample augmentation on the GPU: kernel cost, and what the loader delivers with and without device batches.
tools/bench_augment.py [--calls N] [--rounds R] [--samples S] [--events E] [--out FILE] [--kernels-only]

(a) Microseconds per SAMPLE of eemflow_augment_many (through eemflow_amd.augment_many, batch tensors preallocated: the launch of a call,
    launch gaps included) at 1, 10 and 16 samples per call: 1280x720x5 flips only (HREM: no flow), 346x260x5 -> 256x256 crop + flips with
    an fp32 flow (MVSEC), 1280x720x5 -> 512x960 rescaled + flipped + cropped with an fp32 flow.  HIP events around N back-to-back calls
    after a warm-up, the median of R rounds.  Bytes moved = every output byte written plus as many read (the least a copy can read;
    the rescaling form reads up to four neighbours per output, mostly from cache), set against the chip's 5.5 TB/s copy rate
    (read + write bytes per second).  Every sample has its own source buffers; at 1 sample per call source and destination (74 MB at
    1280x720) stay in the 256 MB Infinity Cache between calls, at 10 and 16 they do not.
(b) Samples/s that ThreadedBatchLoader delivers at batch 8 with 4 threads over synthetic files (write_events_npz / write_flo / npy) at
    both frame sizes - HREM 1280x720 with flips, MVSEC 346x260 with the 256x256 crop and flips - on the host route (per-sample
    __getitem__: volumes to the host, numpy, stacked, uploaded by the consumer) and with device_batches=True; then the wall time per
    EEMFlowTrainer.step when the training loop is fed by each (the loop of TrainRaftEvents.train_iters: .to(dev).float() + step).
    Routes alternate, R rounds, medians.
Writes the lines and one JSON line to --out (default profiles/r15_augment_bench.txt beside this tool) and to stdout.
--kernels-only: just (a) at 16 samples per call (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
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
from eemflow_amd import EEMFlow, augment_many, hrem               # noqa: E402
from eemflow_amd.augmentor import AugPlan                         # noqa: E402
from eemflow_amd.loader import ThreadedBatchLoader                # noqa: E402
from eemflow_amd.mvsec import MvsecEventFlow                      # noqa: E402
from eemflow_amd.train import EEMFlowTrainer                      # noqa: E402
from eemflow_amd.weights import seeded_state_dict                 # noqa: E402

COPY_RATE = 5.5e12                                                # bytes read + written per second by a plain device copy
BATCH, THREADS = 8, 4


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


def kernel_cases():
    """(name, C, H, W, with_flow, plan of sample i)"""
    def flips(i):
        return AugPlan(720, 1280, hflip=i % 2 == 0, vflip=i % 4 == 1)

    def crop(i):
        return AugPlan(260, 346, crop=(256, 256), y0=i % 4, x0=(7 * i) % 90, hflip=i % 2 == 0, vflip=i % 4 == 1)

    def rescale(i):
        sx, sy = np.float64(1.0 + 0.05 * (i % 5)), np.float64(0.9 + 0.07 * (i % 4))
        rh, rw = int(round(720 * sy)), int(round(1280 * sx))
        return AugPlan(rh, rw, crop=(512, 960), y0=(13 * i) % (rh - 512), x0=(29 * i) % (rw - 960), hflip=i % 2 == 0, vflip=i % 4 == 1,
                       resized=True, scale_x=sx, scale_y=sy)
    return (("flips 1280x720x5", 5, 720, 1280, False, flips), ("crop+flips 346x260x5 -> 256x256", 5, 260, 346, True, crop),
            ("rescale 1280x720x5 -> 512x960", 5, 720, 1280, True, rescale))


def kernel_rows(calls, rounds, counts, say):
    dev = torch.device("cuda:0")
    out = {}
    for name, C, H, W, with_flow, plan_of in kernel_cases():
        kmax = max(counts)
        olds = [torch.randn(C, H, W, device=dev) for _ in range(kmax)]
        news = [torch.randn(C, H, W, device=dev) for _ in range(kmax)]
        flows = [torch.randn(2, H, W, device=dev) for _ in range(kmax)] if with_flow else None
        plans = [plan_of(i) for i in range(kmax)]
        ch, cw = plans[0].crop
        ncalls = calls if H * W < 500_000 else max(4, calls // 5)
        for k in counts:
            dst = (torch.empty(k, C, ch, cw, device=dev), torch.empty(k, C, ch, cw, device=dev),
                   torch.empty(k, 2, ch, cw, device=dev) if with_flow else None, torch.empty(k, ch, cw, device=dev) if with_flow else None)
            written = (2 * C + (3 if with_flow else 0)) * ch * cw * 4
            moved = 2 * written
            med, lo, hi = timed(lambda: augment_many(plans[:k], olds[:k], news[:k], flows[:k] if with_flow else None, out=dst), ncalls, rounds, k)
            rate = moved / (med * 1e-6)
            key = name.split()[0] + f"_{W}x{H}_n{k}"
            out[key + "_us_per_sample"], out[key + "_copy_rate_fraction"] = med, rate / COPY_RATE
            say(f"augment_many {name:34s} {k:2d} samples per call: {med:9.2f} us per sample (min {lo:.2f}, max {hi:.2f} over {rounds} rounds of "
                f"{ncalls} calls)  {moved / 1e6:6.1f} MB moved per sample = {rate / 1e12:5.2f} TB/s = {rate / COPY_RATE:.2f} of the copy rate")
        del olds, news, flows
        torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------ (b) the loader
def hrem_dataset(root, samples, events):
    flows = [hrem.synthetic_flow(900 + i, 720, 1280) for i in range(2)]
    for i in range(samples):
        d = os.path.join(root, "dataset/HREM/train/dt1/%06d" % i)
        os.makedirs(d)
        hrem.write_events_npz(os.path.join(d, "events1.npz"), hrem.synthetic_hrem_events(2 * i, events, 720, 1280))
        hrem.write_events_npz(os.path.join(d, "events2.npz"), hrem.synthetic_hrem_events(2 * i + 1, events, 720, 1280))
        hrem.write_flo(os.path.join(d, "flow.flo"), flows[i % 2])
    args = {"eval_type": "dense", "event_interval": "dt1", "num_voxel_bins": 5, "aug_params": {"crop_size": [720, 1280], "do_flip": True}}
    return hrem.HREMEventFlow(args, train=True, root=root)


def mvsec_dataset(root, samples, events, first=40):
    ev_dir, fl_dir = os.path.join(root, "dataset/MVSEC/seqA/event"), os.path.join(root, "dataset/MVSEC/seqA/flowgt_dt1")
    os.makedirs(ev_dir)
    os.makedirs(fl_dir)
    for f in range(first + 1, first + samples + 3):
        ev = hrem.synthetic_hrem_events(f, events, 260, 346, t_span=0.02)
        ev = ev[np.argsort(ev[:, 0], kind="stable")]
        ev[:, 0] += 0.02 * f
        np.savez(os.path.join(ev_dir, "%06d.npz" % f), ts=ev[:, 0], x=ev[:, 1], y=ev[:, 2], p=ev[:, 3])
    for i in range(first, first + samples):
        np.save(os.path.join(fl_dir, "%d.npy" % i), hrem.synthetic_flow(i, 260, 346))
    args = {"eval_type": "dense", "num_voxel_bins": 5, "sequence": "seqA", "aug_params": {"crop_size": [256, 256], "do_flip": True}}
    return MvsecEventFlow(args, train=True, root=root, valid_time_index={"seqA": [(first, first + samples)]})


def loader_rows(tag, ds, size, mesh, rounds, say):
    dev = torch.device("cuda:0")
    loaders = {False: ThreadedBatchLoader(ds, BATCH, shuffle=True, threads=THREADS, drop_last=True),
               True: ThreadedBatchLoader(ds, BATCH, shuffle=True, threads=THREADS, drop_last=True, device_batches=True)}
    net = EEMFlow("", 5, 5, out_mesh_size=mesh)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(0).items()})
    net = net.to(dev).train()
    net.change_imagesize(size)
    trainer = EEMFlowTrainer(net, lr=1e-4, num_steps=100000)

    def epoch(device_batches, step):
        loader = loaders[device_batches]
        np.random.seed(1)
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        for batch in loader:
            e1, e2 = batch['event_volume_old'].to(dev).float(), batch['event_volume_new'].to(dev).float()
            fl, va = batch['flow'].to(dev).float(), batch['valid'].to(dev).float()
            if step:
                trainer.step(e1, e2, fl, va)
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n                      # seconds per batch, upload (host route) included

    out = {}
    for step in (False, True):
        for v in (False, True):
            epoch(v, step)                                        # warm-up: file cache, scratch arenas, the step's workspaces
        res = {False: [], True: []}
        for r in range(rounds):
            for v in ((False, True) if r % 2 == 0 else (True, False)):
                res[v].append(epoch(v, step))
        host, devb = statistics.median(res[False]), statistics.median(res[True])
        if not step:
            out[f"{tag}_host_samples_per_s"], out[f"{tag}_device_samples_per_s"] = BATCH / host, BATCH / devb
            say(f"loader {tag} batch {BATCH}, {THREADS} threads, {len(ds)} samples per epoch: host route {BATCH / host:8.1f} samples/s   "
                f"device_batches {BATCH / devb:8.1f} samples/s   ratio {host / devb:.2f}   (rounds: host "
                f"{[round(BATCH / t, 1) for t in res[False]]}, device {[round(BATCH / t, 1) for t in res[True]]})")
        else:
            out[f"{tag}_host_fed_step_ms"], out[f"{tag}_device_fed_step_ms"] = host * 1e3, devb * 1e3
            say(f"trainer.step {tag} batch {BATCH} fed by the loader: host route {host * 1e3:8.2f} ms per step   device_batches "
                f"{devb * 1e3:8.2f} ms per step   ratio {host / devb:.2f}")
    for ld in loaders.values():
        ld.close()
    # the step alone on resident tensors, for scale
    batch = ds.get_batch(list(range(BATCH)))
    args = (batch['event_volume_old'], batch['event_volume_new'], batch['flow'], batch['valid'])
    for _ in range(3):
        trainer.step(*args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        trainer.step(*args)
    torch.cuda.synchronize()
    out[f"{tag}_resident_step_ms"] = (time.perf_counter() - t0) * 100
    say(f"trainer.step {tag} batch {BATCH} on resident tensors: {out[f'{tag}_resident_step_ms']:8.2f} ms per step")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="library calls per timed run (a fifth of it at 1280x720)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=32, help="samples of each synthetic dataset (one epoch = samples / 8 batches)")
    ap.add_argument("--events", type=int, default=200_000, help="events per HREM event set (a tenth of it per MVSEC frame)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15_augment_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU: no device found")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if a.kernels_only:
        print(json.dumps(kernel_rows(a.calls, 1, (16,), say)))
        return
    say(f"tools/bench_augment.py --calls {a.calls} --rounds {a.rounds} --samples {a.samples} --events {a.events} (MI355X, one process)")
    res = {"calls_per_run": a.calls, "rounds": a.rounds}
    res.update(kernel_rows(a.calls, a.rounds, (1, 10, 16), say))
    with tempfile.TemporaryDirectory() as root:
        res.update(loader_rows("hrem_1280x720", hrem_dataset(root, a.samples, a.events), (720, 1280), True, a.rounds, say))
    with tempfile.TemporaryDirectory() as root:
        res.update(loader_rows("mvsec_346x260", mvsec_dataset(root, a.samples, a.events // 10), (256, 256), False, a.rounds, say))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
