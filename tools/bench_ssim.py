#!/usr/bin/env python3
"""Weighted SSIM warp loss: cost of the library term, of the same term composed from torch operators, and inside the training step.
tools/bench_ssim.py [--calls N] [--rounds R] [--out FILE] [--skip-training]

(a) Microseconds per PREDICTION (one (8,2,H,W) flow) of ssim.ssim_many(...).sum().backward() - forward plus backward through autograd,
    two library calls per 16 predictions - at 1280x720 and at 346x260, batch 8, C = 5, against one pair of event-volume-like images
    shared by all predictions of a call: the three c1 / c2 branches, without and with the occlusion mask, 1, 5 and 12 predictions per
    call.  HIP events around N back-to-back forward + backward passes after a warm-up (launch gaps and the autograd engine included),
    the median of R rounds.
(b) The same term composed from torch operators as the reference writes it - F.grid_sample on its grid, then weighted_ssim's
    F.avg_pool2d moments and torch.clamp - forward + backward, one prediction at a time, in fp32.
(c) torch.cuda.max_memory_allocated above the inputs during one forward + backward of one prediction (its gradient included), both ways.
(d) The training step (TrainRaftEvents, engine='autograd', EEMFlow at 346x260, batch 8, supervised): milliseconds per step without
    the term, with ssim_weight=0.5 and with ssim_occ=True as well; alternating, R rounds.
Writes the lines and one JSON line to --out (default profiles/r21_ssim_bench.txt beside this tool) and to stdout."""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch                                                      # noqa: E402
import torch.nn.functional as F                                   # noqa: E402
from eemflow_amd import EEMFlow, ssim                             # noqa: E402
from eemflow_amd.harness import Logger, TrainRaftEvents           # noqa: E402
from eemflow_amd.weights import seeded_state_dict                 # noqa: E402

SIZES = ((720, 1280), (260, 346))
BATCH, CHANNELS = 8, 5
INF = float("inf")
BRANCHES = (("structure", INF, 9e-6), ("luminance", 1e-4, INF), ("both", 1e-4, 9e-6))


def timed(call, calls, rounds, per):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
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
    flows = [(base + 0.3 * torch.randn(BATCH, 2, h, w, generator=g, device=dev)).contiguous() for _ in range(k)]

    def volume():
        v = torch.round(torch.randn(BATCH, CHANNELS, h, w, generator=g, device=dev) * 3.0) / 4.0
        return (v * (torch.rand(BATCH, CHANNELS, h, w, generator=g, device=dev) < 0.35)).contiguous()
    mask = (torch.rand(BATCH, 1, h, w, generator=g, device=dev) < 0.8).float()
    return flows, volume(), volume(), mask


def torch_term(flow, img1, img2, mask, c1, c2, occ, eps=0.01):
    """The term from torch operators: grid_sample, then the moments by avg_pool2d (mask: the weight, ones without use_occ)."""
    b, c, h, w = img1.shape
    xx = torch.arange(w, device=flow.device, dtype=flow.dtype).view(1, 1, w).expand(b, h, w)
    yy = torch.arange(h, device=flow.device, dtype=flow.dtype).view(1, h, 1).expand(b, h, w)
    grid = torch.stack((2.0 * (xx + flow[:, 0]) / max(w - 1, 1) - 1.0, 2.0 * (yy + flow[:, 1]) / max(h - 1, 1) - 1.0), 3)
    y = F.grid_sample(img2, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    x = img1
    pool = lambda z: F.avg_pool2d(z, (3, 3), (1, 1))
    aw = pool(mask)
    wpe = mask + eps
    inv = 1.0 / (aw + eps)
    wpool = lambda z: pool(z * wpe) * inv
    mu_x, mu_y = wpool(x), wpool(y)
    if math.isinf(c2):
        n, d = 2 * mu_x * mu_y + c1, mu_x ** 2 + mu_y ** 2 + c1
    else:
        sigma_x, sigma_y, sigma_xy = wpool(x ** 2) - mu_x ** 2, wpool(y ** 2) - mu_y ** 2, wpool(x * y) - mu_x * mu_y
        n, d = 2 * sigma_xy + c2, sigma_x + sigma_y + c2
        if not math.isinf(c1):
            n, d = (2 * mu_x * mu_y + c1) * n, (mu_x ** 2 + mu_y ** 2 + c1) * d
    l = torch.clamp((1 - n / d) / 2, 0, 1)
    return torch.sum(l * aw) / (torch.sum(aw) + 1e-6) if occ else torch.mean(l)


def peak_above_inputs(call, leaf):
    call()
    leaf.grad = None                                              # (the gradient counts: it is allocated inside the pass)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    call()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def term_rows(calls, rounds, counts, say):
    dev = torch.device("cuda:0")
    out = {}
    for h, w in SIZES:
        flows, img1, img2, mask = inputs(max(counts), h, w, dev)
        ones = torch.ones_like(mask)
        leaves = [f.requires_grad_(True) for f in flows]
        ncalls = max(2, calls // 5) if h >= 720 else calls
        for name, c1, c2 in BRANCHES:
            for occ in (False, True):
                kw = dict(use_occ=occ, c1=c1, c2=c2)

                def composed():
                    leaves[0].grad = None
                    torch_term(leaves[0], img1, img2, mask if occ else ones, c1, c2, occ).backward()
                t_med, t_lo, t_hi = timed(composed, max(2, ncalls // 2), rounds, 1)
                tag = f"{w}x{h}_{name}_occ{int(occ)}"
                out[f"torch_ops_{tag}_us_per_pred"] = t_med
                for k in counts:
                    def ours():
                        for p in leaves[:k]:
                            p.grad = None
                        ssim.ssim_many(leaves[:k], img1, img2, mask if occ else None, **kw).sum().backward()
                    o_med, o_lo, o_hi = timed(ours, ncalls, rounds, k)
                    out[f"ssim_many_{tag}_k{k}_us_per_pred"] = o_med
                    say(f"{w}x{h} B={BATCH} C={CHANNELS} {name:9s} occ {int(occ)} {k:2d} predictions per call, forward + backward: ssim_many "
                        f"{o_med:10.2f} us per prediction (min {o_lo:.2f}, max {o_hi:.2f});   torch operators {t_med:10.2f} us "
                        f"(min {t_lo:.2f}, max {t_hi:.2f});   ratio {t_med / o_med:.2f}x   ({rounds} rounds of {ncalls} calls)")
                if not occ:
                    def one():
                        leaves[0].grad = None
                        ssim.ssim_many(leaves[:1], img1, img2, None, **kw).sum().backward()
                    mo, mt = peak_above_inputs(one, leaves[0]), peak_above_inputs(composed, leaves[0])
                    out[f"ssim_many_{tag}_peak_mib"], out[f"torch_ops_{tag}_peak_mib"] = mo, mt
                    say(f"{w}x{h} B={BATCH} C={CHANNELS} {name:9s} peak memory above the inputs, one prediction forward + backward: ssim_many "
                        f"{mo:9.1f} MiB;   torch operators {mt:9.1f} MiB")
        del flows, leaves, img1, img2, mask, ones
        torch.cuda.empty_cache()
    return out


def training_rows(rounds, say, h=260, w=346, batch=8, steps=20):
    from eemflow_amd.weights import synthetic_gt, synthetic_voxel_pair
    dev = torch.device("cuda:0")

    def make_batch(seed):
        e1, e2 = (torch.from_numpy(a).to(dev) for a in synthetic_voxel_pair(seed, batch, h, w))
        gt, valid = (torch.from_numpy(a).to(dev) for a in synthetic_gt(seed + 1, batch, h, w))
        return {"event_volume_old": e1, "event_volume_new": e2, "flow": gt, "valid": valid}
    batches = [make_batch(200 + 10 * i) for i in range(4)] * (steps // 4)
    forms = {"plain": {}, "ssim": dict(ssim_weight=0.5), "ssim_occ": dict(ssim_weight=0.5, ssim_occ=True)}
    res = {name: [] for name in forms}
    nets = {}
    for name, kw in forms.items():
        net = EEMFlow("", groups=5, n_first_channels=5)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(68).items()})
        nets[name] = (net.cuda().train(), TrainRaftEvents(batches, (h, w), lr=1e-6, logger=Logger(verbose=False), engine="autograd", **kw))

    def run(name):
        net, tr = nets[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.train_iters(net, val_iters=len(batches))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches)
    for name in forms:                                            # warm-up: workspaces, scratch arenas
        run(name)
    order = list(forms)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            res[name].append(run(name))
        say(f"round {r}: training step {w}x{h} batch {batch}, autograd engine, supervised: {res['plain'][-1]:8.2f} ms   with ssim_weight=0.5 "
            f"{res['ssim'][-1]:8.2f} ms   with ssim_occ as well {res['ssim_occ'][-1]:8.2f} ms")
    return {f"train_step_{name}_ms": statistics.median(v) for name, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40, help="forward + backward passes per timed run (a fifth at 1280x720)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r21_ssim_bench.txt"))
    ap.add_argument("--skip-training", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py measures on the GPU: no device found")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say(f"tools/bench_ssim.py --calls {a.calls} --rounds {a.rounds} (MI355X, one process): HIP events around back-to-back forward + backward "
        f"passes per round after a warm-up, launch gaps included")
    res = {"calls_per_run": a.calls, "rounds": a.rounds}
    res.update(term_rows(a.calls, a.rounds, (1, 5, 12), say))
    if not a.skip_training:
        res.update(training_rows(a.rounds, say))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
