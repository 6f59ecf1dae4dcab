#!/usr/bin/env python3
"""MVSEC ground truth for any window on the GPU (eemflow_gt_flow_many), against the same walk on the host and composed in torch.
tools/bench_gt_prop.py [--calls N] [--rounds R] [--out FILE] [--no-model]

Microseconds per WINDOW at 260 x 346 (wall clock around N back-to-back calls and a device synchronisation, so host work - the plans
among it - counts), for windows that span under 1 (the short branch), 3 and 16 ground-truth frames, at 1, 10 and 32 windows per call.
In ONE process the routes alternate inside every round; the median (min, max) of R rounds:
  kernel   eemflow_amd.mvsec_raw.MvsecGroundTruth.flow_many on the resident stack
  host     the NumPy restatement of the reference's walk (tests/gt_prop_reference.py, vectorised over the pixels - the reference itself
           needs cv2) per window, plus the upload of its result
  torch    the same walk composed from torch operations on the GPU (round, gathers, where, float64 adds), window by window
Before timing, kernel and torch are held bitwise against the restatement on one window of every length.
Then (unless --no-model) frames per second of harness.run_recording with a seeded EEMFlow over a synthetic 260 x 346 sequence (33
windows of 2e4 events 60 ms long - every ground truth takes the long branch - centre crop 256 x 256) with gt= (dense, then sparse) against the same run without it.
Writes the lines and one JSON line to --out (default profiles/gt_prop_bench.txt beside this tool) and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
import gt_prop_reference as G                                     # noqa: E402
from eemflow_amd import harness, mvsec_raw as M                   # noqa: E402

H, W, FRAMES = 260, 346, 20
COUNTS = (1, 10, 32)
DEV = "cuda:0"


def make_stack(seed, frames):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    st = np.empty((frames, 2, H, W))
    for k in range(frames):
        st[k, 0] = 2.0 * np.sin(0.05 * y + 0.3 * k) + 0.2 * rng.standard_normal((H, W))
        st[k, 1] = 2.0 * np.cos(0.04 * x - 0.2 * k) + 0.2 * rng.standard_normal((H, W))
    st[rng.uniform(size=st.shape) < 0.01] = 0.0
    return st.astype(np.float32), 50.0 + np.cumsum(0.05 + 0.002 * rng.uniform(size=frames))


def torch_walk(stack, frame0, nsteps, a, b):
    """tests/gt_prop_reference.walk in torch operations on the stack's device."""
    if nsteps == 0:
        return ((stack[frame0].double() * a) / b).float()
    ys, xs = torch.meshgrid(torch.arange(H, device=stack.device), torch.arange(W, device=stack.device), indexing="ij")
    x0, y0 = xs.float(), ys.float()
    x, y = x0.clone(), y0.clone()
    mx, my = torch.ones_like(x, dtype=torch.bool), torch.ones_like(x, dtype=torch.bool)
    for s in range(nsteps):
        scale = a if s == 0 else (b if s == nsteps - 1 else 1.0)
        finx, finy = torch.isfinite(x), torch.isfinite(y)
        rx, ry = torch.round(x), torch.round(y)                        # half to even
        inside = finx & finy & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
        at = (ry.clamp(0, H - 1).long() * W + rx.clamp(0, W - 1).long()).view(-1)
        frame = stack[frame0 + s].view(2, -1)
        zero = torch.zeros((), device=stack.device)
        fu = torch.where(inside, frame[0][at].view(H, W), zero)
        fv = torch.where(inside, frame[1][at].view(H, W), zero)
        mx &= ~((fu == 0) & finx)
        my &= ~((fv == 0) & finy)
        x = (x.double() + fu.double() * scale).float()
        y = (y.double() + fv.double() * scale).float()
    return torch.stack([torch.where(mx, x - x0, zero), torch.where(my, y - y0, zero)])


def wall_us(call, calls, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (calls * per)


def alternate(routes, calls, rounds, per):
    """{name: (median, min, max)}: every round times every route once, in turn."""
    for name, (call, _) in routes.items():
        call()
    us = {name: [] for name in routes}
    for _ in range(rounds):
        for name, (call, share) in routes.items():
            us[name].append(wall_us(call, max(1, int(calls * share)), per))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in us.items()}


def synthetic_sequence(seed, frames, per_frame, stack_ts):
    """(events (N,4) [x, y, t, p], image_raw_ts, image_raw_event_inds): grey frames every 60 ms from the stack's first timestamp, so every
    window is longer than a ground-truth interval and takes the long branch (2 or 3 steps)."""
    rng = np.random.default_rng(seed)
    img_ts = stack_ts[0] + 0.001 + 0.06 * np.arange(frames)
    parts, inds, prev = [], [], img_ts[0] - 0.06
    for j in range(frames):
        t = np.sort(rng.uniform(prev, img_ts[j], per_frame))
        parts.append(np.stack([rng.integers(0, W, per_frame), rng.integers(0, H, per_frame), t, 2 * rng.integers(0, 2, per_frame) - 1],
                              axis=1).astype(np.float64))
        inds.append(per_frame * (j + 1))
        prev = img_ts[j]
    return np.concatenate(parts), img_ts, np.array(inds, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timed run (the host route: a tenth of it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gt_prop_bench.txt"))
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gt_prop.py measures on the GPU: no device found")
    lines, res = [], {"calls_per_run": a.calls, "rounds": a.rounds}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/bench_gt_prop.py --calls {a.calls} --rounds {a.rounds} (MI355X, one process, routes alternating; us per window, wall clock, "
        f"median (min, max) of the rounds)")
    stack, ts = make_stack(7, FRAMES)
    gt = M.MvsecGroundTruth(stack, ts, device=DEV)
    d = np.diff(ts)
    spans = {"under 1 frame": (ts[1] + 0.2 * d[1], ts[1] + 0.8 * d[1]), "3 frames": (ts[1] + 0.5 * d[1], ts[3] + 0.5 * d[3]),
             "16 frames": (ts[1] + 0.5 * d[1], ts[16] + 0.5 * d[16])}
    for name, (t0, t1) in spans.items():
        pl = gt.plan(t0, t1)
        ref = G.walk(stack, *pl)
        assert np.array_equal(gt.flow(t0, t1).cpu().numpy().view(np.uint32), ref.view(np.uint32)), f"kernel != restatement ({name})"
        assert np.array_equal(torch_walk(gt.stack, *pl).cpu().numpy().view(np.uint32), ref.view(np.uint32)), f"torch != restatement ({name})"
    say(f"{H} x {W}, a stack of {FRAMES} frames (kernel == restatement == torch composition bitwise on one window of every length)")
    for name, (t0, t1) in spans.items():
        pl = gt.plan(t0, t1)
        tag = name.replace(" ", "_")
        say(f"windows spanning {name} ({pl[1]} steps)")
        for k in COUNTS:
            starts, ends = [t0] * k, [t1] * k
            routes = {"kernel": (lambda: gt.flow_many(starts, ends), 1.0),
                      "host": (lambda: [torch.from_numpy(G.walk(stack, *G.plan(ts, s, e))).to(DEV) for s, e in zip(starts, ends)], 0.1),
                      "torch": (lambda: [torch_walk(gt.stack, *gt.plan(s, e)) for s, e in zip(starts, ends)], 0.25)}
            out = alternate(routes, a.calls, a.rounds, k)
            text = f"  {k:2d} windows per call:"
            for route, (med, lo, hi) in out.items():
                text += f"   {route} {med:9.1f} ({lo:.1f}, {hi:.1f})"
                res[f"{tag}_k{k}_{route}_us"] = med
                res[f"{tag}_k{k}_{route}_spread_us"] = hi - lo
            text += f"   host / kernel {out['host'][0] / out['kernel'][0]:7.1f} x   torch / kernel {out['torch'][0] / out['kernel'][0]:6.1f} x"
            res[f"{tag}_k{k}_host_over_kernel"] = out["host"][0] / out["kernel"][0]
            res[f"{tag}_k{k}_torch_over_kernel"] = out["torch"][0] / out["kernel"][0]
            say(text)
    if not a.no_model:
        from eemflow_amd import EEMFlow
        from eemflow_amd.weights import seeded_state_dict
        stack40, ts40 = make_stack(9, 48)
        gt40 = M.MvsecGroundTruth(stack40, ts40, device=DEV)
        events, img_ts, inds = synthetic_sequence(13, 36, 20000, ts40)
        raw = M.MvsecRaw(events, img_ts, inds, gt40, height=H, width=W, device=DEV)
        offsets, t_edges = raw.frame_windows(1, 32)
        pairs = len(offsets) - 2
        net = EEMFlow("", groups=5, n_first_channels=5).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(5).items()})
        net = net.to(DEV)

        def run(**kw):
            def call():
                for _ in harness.run_recording(net, raw.recording, offsets, crop=(256, 256), **kw):
                    pass
            return call

        with torch.no_grad():
            out = alternate({"without_gt": (run(), 1.0), "gt_dense": (run(gt=gt40, t_edges=t_edges), 1.0),
                             "gt_sparse": (run(gt=gt40, t_edges=t_edges, eval_type='sparse'), 1.0)}, 3, a.rounds, pairs)
        text = f"EEMFlow 260 x 346 cropped to 256 x 256, {pairs} pairs of 2e4-event windows, run_recording, frames per second:"
        for name, (med, lo, hi) in out.items():
            text += f"   {name} {1e6 / med:8.1f} ({1e6 / hi:.1f}, {1e6 / lo:.1f})"
            res[f"run_recording_{name}_fps"] = 1e6 / med
        say(text)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
