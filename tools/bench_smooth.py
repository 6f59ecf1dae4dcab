#!/usr/bin/env python3
"""Edge-aware smoothness loss: cost of the library call, of the same term composed from torch slices, and inside the training step.
tools/bench_smooth.py [--calls N] [--rounds R] [--out FILE] [--skip-training]

(a) Microseconds per JOB (one (8,2,H,W) prediction) of eemflow_smoothness_many at 1280x720 and at 346x260, batch 8, against one
    5-channel img shared by all jobs of a call: the loss alone, and loss plus gradient in ONE call (what a fused consumer would ask
    for; smoothness_many's backward is a second, gradient-only call - timed in (b)); order 1 and 2, 'L1' and 'abs_robust' ('gauss'
    weights), 1, 5 and 12 jobs per call.  HIP events around N back-to-back library calls after a warm-up (launch gaps included), the
    median of R rounds.  Achieved bytes per second count (2 + C) planes read - the shared img once per call - plus 2 planes written
    with a gradient, beside the 5.5 TB/s copy rate of this card.
(b) The same term forward + backward through autograd: smooth.smoothness_many(...).sum().backward() against the composition from
    torch slice operations on the same tensors (what a user ran before), microseconds per job.
(c) The training step (TrainRaftEvents, engine='autograd', EEMFlow at 346x260, batch 8, contrast_weight=0.5, batches of 20 000
    events per sample fed from a list): milliseconds per step without and with smooth_weight=0.1; alternating, R rounds.
Writes the lines and one JSON line to --out (default profiles/r18_smooth_bench.txt beside this tool) and to stdout."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch                                                      # noqa: E402
from eemflow_amd import EEMFlow, _lib, smooth                     # noqa: E402
from eemflow_amd.harness import Logger, TrainRaftEvents           # noqa: E402
from eemflow_amd.weights import seeded_state_dict                 # noqa: E402

SIZES = ((720, 1280), (260, 346))
BATCH, CHANNELS = 8, 5
COPY_RATE = 5.5e12


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


def inputs(k, h, w, dev):
    g = torch.Generator(device=dev).manual_seed(h + k)
    y = torch.arange(h, device=dev, dtype=torch.float32).view(1, 1, h, 1)
    x = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, 1, w)
    base = torch.cat([3.0 * torch.sin(0.02 * x + 0.01 * y), 2.0 * torch.cos(0.03 * y - 0.01 * x)], 1).expand(BATCH, 2, h, w)
    preds = [(base + 0.3 * torch.randn(BATCH, 2, h, w, generator=g, device=dev)).contiguous() for _ in range(k)]
    img = torch.round(torch.randn(BATCH, CHANNELS, h, w, generator=g, device=dev) * 3.0) / 4.0
    img = (img * (torch.rand(BATCH, CHANNELS, h, w, generator=g, device=dev) < 0.35)).contiguous()
    return preds, img


def torch_term(pred, img, order, constant, error_type):
    """The term from torch slices, as a user composes it ('gauss' weights)."""
    total = 0.0
    for axis in (2, 3):
        n = pred.shape[axis]
        d = pred.narrow(axis, 0, n - 1) - pred.narrow(axis, 1, n - 1)
        if order == 2:
            d = d.narrow(axis, 0, n - 2) - d.narrow(axis, 1, n - 2)
        g = constant * (img.narrow(axis, 0, n - order) - img.narrow(axis, order, n - order))
        wgt = torch.exp(-torch.mean(g ** 2, 1, keepdim=True))
        e = d.abs() if error_type == "L1" else (d.abs() + 0.01).pow(0.4)
        total = total + torch.mean(e * wgt)
    return total


def kernel_rows(calls, rounds, counts, say):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    sp = _lib.current_stream_ptr(dev)
    out = {}
    for h, w in SIZES:
        preds, img = inputs(max(counts), h, w, dev)
        grads = [torch.empty_like(p) for p in preds]
        plane = BATCH * h * w * 4
        ncalls = max(2, calls // 10) if h >= 720 else calls
        for k in counts:
            ptr = ctypes.c_void_p * k
            loss = torch.empty(k, device=dev, dtype=torch.float64)
            coef = torch.ones(k, device=dev, dtype=torch.float64)
            scratch = torch.empty(int(L.eemflow_smoothness_scratch_doubles(k, BATCH, h, w)), device=dev, dtype=torch.float64)
            pp, ip = ptr(*[p.data_ptr() for p in preds[:k]]), ptr(*[img.data_ptr()] * k)
            gp = ptr(*[g.data_ptr() for g in grads[:k]])
            for order in (1, 2):
                for et, name in ((0, "L1"), (1, "abs_robust")):
                    def fwd():
                        _lib.check(L.eemflow_smoothness_many(k, pp, ip, BATCH, CHANNELS, h, w, order, 0, et, 1.0, None, loss.data_ptr(), None,
                                                             scratch.data_ptr(), sp))

                    def both():
                        _lib.check(L.eemflow_smoothness_many(k, pp, ip, BATCH, CHANNELS, h, w, order, 0, et, 1.0, coef.data_ptr(), loss.data_ptr(),
                                                             gp, scratch.data_ptr(), sp))
                    f_med, f_lo, f_hi = timed(fwd, ncalls, rounds, k)
                    b_med, b_lo, b_hi = timed(both, ncalls, rounds, k)
                    f_bytes = (2 * k + CHANNELS) * plane / k
                    b_bytes = (4 * k + CHANNELS) * plane / k
                    tag = f"{w}x{h}_o{order}_{name}_k{k}"
                    out[f"loss_{tag}_us_per_job"], out[f"loss_grad_{tag}_us_per_job"] = f_med, b_med
                    say(f"{w}x{h} B={BATCH} C={CHANNELS} order {order} {name:10s} {k:2d} jobs per call: loss {f_med:8.2f} us per job "
                        f"(min {f_lo:.2f}, max {f_hi:.2f}) = {f_bytes / f_med * 1e6 / 1e12:5.2f} TB/s, {f_bytes / f_med * 1e6 / COPY_RATE * 100:5.1f} % "
                        f"of the copy rate;   loss + gradient {b_med:8.2f} us per job (min {b_lo:.2f}, max {b_hi:.2f}) = "
                        f"{b_bytes / b_med * 1e6 / 1e12:5.2f} TB/s, {b_bytes / b_med * 1e6 / COPY_RATE * 100:5.1f} %   "
                        f"({rounds} rounds of {ncalls} calls)")
        del preds, grads, img
        torch.cuda.empty_cache()
    return out


def autograd_rows(calls, rounds, counts, say):
    dev = torch.device("cuda:0")
    out = {}
    for h, w in SIZES:
        preds, img = inputs(max(counts), h, w, dev)
        leaves = [p.requires_grad_(True) for p in preds]
        ncalls = max(2, calls // 10) if h >= 720 else calls
        for k in counts:
            for order in (1, 2):
                for name in ("L1", "abs_robust"):
                    def ours():
                        for p in leaves[:k]:
                            p.grad = None
                        smooth.smoothness_many(leaves[:k], img, order=order, error_type=name).sum().backward()

                    def composed():
                        for p in leaves[:k]:
                            p.grad = None
                        sum(torch_term(p, img, order, 1.0, name) for p in leaves[:k]).backward()
                    o_med, o_lo, o_hi = timed(ours, ncalls, rounds, k)
                    t_med, t_lo, t_hi = timed(composed, max(2, ncalls // 4), rounds, k)
                    tag = f"{w}x{h}_o{order}_{name}_k{k}"
                    out[f"autograd_{tag}_us_per_job"], out[f"torch_slices_{tag}_us_per_job"] = o_med, t_med
                    say(f"{w}x{h} B={BATCH} C={CHANNELS} order {order} {name:10s} {k:2d} jobs, forward + backward: smoothness_many {o_med:9.2f} us per job "
                        f"(min {o_lo:.2f}, max {o_hi:.2f});   torch slices {t_med:9.2f} us per job (min {t_lo:.2f}, max {t_hi:.2f});   "
                        f"ratio {t_med / o_med:.2f}x")
        del preds, leaves, img
        torch.cuda.empty_cache()
    return out


def training_rows(rounds, say, h=260, w=346, batch=8, steps=20):
    from bench_iwe import event_sets
    from eemflow_amd.augmentor import AugPlan, event_map_after_offset
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
    res = {0.0: [], 0.1: []}
    nets = {}
    for wgt in res:
        net = EEMFlow("", groups=5, n_first_channels=5)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(68).items()})
        nets[wgt] = (net.cuda().train(), TrainRaftEvents(batches, (h, w), lr=1e-6, logger=Logger(verbose=False), engine="autograd",
                                                         contrast_weight=0.5, smooth_weight=wgt))

    def run(wgt):
        net, tr = nets[wgt]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_iters(net, val_iters=len(batches))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches)
    run(0.0), run(0.1)                                            # warm-up: workspaces, scratch arenas
    for r in range(rounds):
        for wgt in ((0.0, 0.1) if r % 2 == 0 else (0.1, 0.0)):
            res[wgt].append(run(wgt))
        say(f"round {r}: training step {w}x{h} batch {batch}, autograd engine, contrast_weight=0.5: {res[0.0][-1]:8.2f} ms   with "
            f"smooth_weight=0.1 {res[0.1][-1]:8.2f} ms   ratio {res[0.1][-1] / res[0.0][-1]:.3f}")
    return {"train_step_contrast_ms": statistics.median(res[0.0]), "train_step_contrast_smooth_ms": statistics.median(res[0.1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="library calls per timed run (a tenth of it at 1280x720)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r18_smooth_bench.txt"))
    ap.add_argument("--skip-training", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth.py measures on the GPU: no device found")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say(f"tools/bench_smooth.py --calls {a.calls} --rounds {a.rounds} (MI355X, one process): HIP events around back-to-back calls per round after "
        f"a warm-up, launch gaps included")
    res = {"calls_per_run": a.calls, "rounds": a.rounds}
    res.update(kernel_rows(a.calls, a.rounds, (1, 5, 12), say))
    res.update(autograd_rows(a.calls, a.rounds, (1, 5, 12), say))
    if not a.skip_training:
        res.update(training_rows(a.rounds, say))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
