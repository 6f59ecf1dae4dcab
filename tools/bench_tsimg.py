#!/usr/bin/env python3
"""Image of average timestamps / timestamp loss / RSAT: cost per event set beside the image of warped events, and inside a training step.
tools/bench_tsimg.py [--calls N] [--rounds R] [--out FILE] [--no-training]

(a) Microseconds per EVENT SET at 1280x720 with 2e6 events per set and at 346x260 with 2e5, for 1, 10 and 16 sets per call, in the
    binned form and in the direct form (EEM_IWE_DIRECT=1), all in one run:
      avg_timestamps_many        the forward alone (one job per set under a smooth flow)
      timestamp_loss fwd + bwd   loss.backward() into a (k,2,H,W) leaf; every set rides the launches twice (t_ref end and start)
      fwl_many / fwl_loss        the same two measurements of the contrast term (iwe.py), the yardstick
      iwe_many                   the image of warped events alone, the yardstick of avg_timestamps_many
    These are the Python calls, their one copy of the sets' end timestamps to the host included.  HIP events around N back-to-back
    calls after a warm-up, the median of R rounds (a tenth of N at 2e6 events per set).
(b) The same term composed from torch operations under autograd (fp64 on the GPU: gathers for the flow sample, index_add_ for the two
    planes, forward plus backward, both time references), a loop over the sets of a call; 2 calls per round.
(c) The training step (TrainRaftEvents, engine='autograd', EEMFlow at 346x260, batch 8, 20 000 events per sample with flip-and-crop event
    maps, fed from a list): milliseconds per step without and with timestamp_weight=0.5; alternating, R rounds.
Events have integer coordinates and uniformly random pixels, time-sorted; the flow moves them by up to 8 px.
Writes the lines and one JSON line to --out (default profiles/r22_tsimg_bench.txt beside this tool) and to stdout."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import torch                                                      # noqa: E402
from bench_iwe import SIZES, event_sets, smooth_flow, timed       # noqa: E402
from eemflow_amd import EEMFlow, tsimg                            # noqa: E402
from eemflow_amd.harness import Logger                            # noqa: E402
from eemflow_amd.weights import seeded_state_dict                 # noqa: E402

iwe = importlib.import_module("eemflow_amd.iwe")


def torch_term(ev, flow, eps=1e-9):
    """L(end) + L(start) of one event set from torch operations in fp64, differentiable in `flow` ((2,H,W) fp64)."""
    h, w = flow.shape[-2], flow.shape[-1]
    t, x, y, p = ev[:, 0], ev[:, 1], ev[:, 2], ev[:, 3]
    first, last = t[0], t[-1]
    scale = -1.0 / (last - first)
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    xi, yi = x0.long(), y0.long()
    u = torch.zeros_like(x)
    v = torch.zeros_like(x)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = xi + dx, yi + dy
            ok = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
            wk = torch.where(ok, (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy), torch.zeros_like(x))
            val = flow[:, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]
            u = u + wk * val[0]
            v = v + wk * val[1]
    c = torch.where(p > 0, 0, 1)
    total = 0.0
    for t0 in (last, first):
        tau = (t - t0) * scale
        a = (1.0 - tau.abs()).clamp(min=0.0)
        xw, yw = x + u * tau, y + v * tau
        xf, yf = torch.floor(xw), torch.floor(yw)
        gx, gy = xw - xf, yw - yf
        X0, Y0 = xf.detach().long(), yf.detach().long()
        D = torch.zeros(2 * h * w, dtype=torch.float64, device=ev.device)
        N = torch.zeros(2 * h * w, dtype=torch.float64, device=ev.device)
        for dy in (0, 1):
            for dx in (0, 1):
                xx, yy = X0 + dx, Y0 + dy
                ok = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
                wgt = torch.where(ok, (gy if dy else 1.0 - gy) * (gx if dx else 1.0 - gx), torch.zeros_like(x))
                idx = c * h * w + yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)
                D = D.index_add(0, idx, wgt)
                N = N.index_add(0, idx, wgt * a)
        T = N / (D + eps)
        Dv = D.view(2, h, w).detach()
        active = ((Dv[0] + Dv[1]) > 0).sum()
        total = total + (T * T).sum() / (active + 1e-9)
    return total


def kernel_rows(calls, rounds, counts, forms, say):
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

            def ts_both():
                pred.grad = None
                tsimg.timestamp_loss(sets, flows).backward()

            def fwl_both():
                pred.grad = None
                iwe.fwl_loss(sets, flows).backward()
            tag = f"{w}x{h}_n{k}"
            for form in forms:
                os.environ["EEM_IWE_DIRECT"] = "1" if form == "direct" else "0"
                rows = (("iwe_many", lambda: iwe.iwe_many(sets, plain)),
                        ("avg_timestamps_many", lambda: tsimg.avg_timestamps_many(sets, plain)),
                        ("fwl_many", lambda: iwe.fwl_many(sets, plain)),
                        ("rsat_many", lambda: tsimg.rsat_many(sets, plain)),
                        ("fwl_loss_fwd_bwd", fwl_both),
                        ("timestamp_loss_fwd_bwd", ts_both))
                for name, call in rows:
                    med, lo, hi = timed(call, ncalls, rounds, k)
                    out[f"{name}_{form}_{tag}_us_per_set"] = med
                    say(f"{name:24s} {form:6s} {w}x{h} {n:.0e} events  {k:2d} sets per call: {med:10.2f} us per event set "
                        f"(min {lo:.2f}, max {hi:.2f} over {rounds} rounds of {ncalls} calls)")
            os.environ.pop("EEM_IWE_DIRECT", None)
            pred64 = pred.detach().double().requires_grad_(True)

            def torch_both():
                pred64.grad = None
                sum(torch_term(sets[i], pred64[i]) for i in range(k)).backward()
            med, lo, hi = timed(torch_both, 2, rounds, k)
            out[f"torch_index_add_fwd_bwd_{tag}_us_per_set"] = med
            say(f"{'torch index_add_ fwd + bwd':24s}        {w}x{h} {n:.0e} events  {k:2d} sets per call: {med:10.2f} us per event set "
                f"(min {lo:.2f}, max {hi:.2f} over {rounds} rounds of 2 calls)   / timestamp_loss binned = "
                f"{med / out[f'timestamp_loss_fwd_bwd_binned_{tag}_us_per_set']:.1f}" if "binned" in forms else f"torch {tag}: {med:.2f}")
            # the two values side by side (the torch composition neither quantises its weights nor rounds T to fp32)
            lib = float(tsimg.timestamp_loss(sets[:1], plain[:1]))
            ref = float(torch_term(sets[0], pred64[0].detach()))
            say(f"{'agreement':24s}        {w}x{h} first set: timestamp_loss {lib:.9f}, its torch composition {ref:.9f} "
                f"(relative difference {abs(lib - ref) / abs(ref):.1e})")
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
                                                         timestamp_weight=wgt))

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
        say(f"round {r}: training step {w}x{h} batch {batch}, autograd engine: {res[0.0][-1]:8.2f} ms   with timestamp_weight=0.5 "
            f"{res[0.5][-1]:8.2f} ms   ratio {res[0.5][-1] / res[0.0][-1]:.3f}")
    return {"train_step_ms": statistics.median(res[0.0]), "train_step_timestamp_ms": statistics.median(res[0.5])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="calls per timed run (a tenth of it at 2e6 events per set)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_tsimg_bench.txt"))
    ap.add_argument("--no-training", action="store_true", help="(a) and (b) only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsimg.py measures on the GPU: no device found")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/bench_tsimg.py --calls {a.calls} --rounds {a.rounds} (MI355X, one process): HIP events around back-to-back Python calls per "
        f"round after a warm-up, launch gaps and the timestamps' host copy included")
    res = {"calls_per_run": a.calls, "rounds": a.rounds}
    res.update(kernel_rows(a.calls, a.rounds, (1, 10, 16), ("binned", "direct"), say))
    if not a.no_training:
        res.update(training_rows(a.rounds, say))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
