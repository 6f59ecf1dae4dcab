#!/usr/bin/env python3
"""The DSEC trilinear voxelizer against the torch composition it replaces and against the two-vote voxelizer.
tools/bench_dsec_voxel.py [--calls N] [--rounds R] [--out FILE] [--kernels-only]

Microseconds per event SET (normalised grid, launch gaps included) at 15 x 480 x 640 with 1e6 events per set (DSEC / E-RAFT) and
5 x 260 x 346 with 2e5 (MVSEC's sensor), at 1, 4 and 16 sets per call, every set with buffers of its own, events time-sorted with
sub-pixel coordinates uniform over the sensor.  HIP events around N back-to-back calls on the stream after a warm-up, the median of R
rounds.  In one process, per size and set count:
  tri        eemflow_amd.dsec.voxel_grid_many (eemflow_voxelize_trilinear_many): fp32 columns, eight votes per event
  tri_rect   the same with raw int16 coordinates and a sensor-sized rectification map looked up by the kernel   (reported only)
  torch      (a) the reference's VoxelGrid.convert statement for statement (utils/dsec_utils.py:26-64) in torch on the same GPU, once
             per set - what a user composes today
  two_vote   (b) eemflow_amd.voxelizer.voxelize_many_device on the same event counts and grid: (N,4) float64 rows, integer pixels, ONE
             record per event - the floor of the band machinery; the trilinear form writes four records per event   (ratio reported only)
Before timing, the tri grid is held against the torch composition's (fp32 sums in another order: a few 1e-6 of the largest cell).
Writes the lines and one JSON line to --out (default profiles/dsec_voxel_bench.txt beside this tool) and to stdout.
--kernels-only: just `tri` at 4 sets per call (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np                                                # noqa: E402
import torch                                                      # noqa: E402
from eemflow_amd import dsec                                      # noqa: E402
from eemflow_amd.voxelizer import voxelize_many_device            # noqa: E402

SIZES = (((15, 480, 640), 1_000_000), ((5, 260, 346), 200_000))
COUNTS = (1, 4, 16)


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


def torch_convert(events, C, H, W, normalize=True):
    """utils/dsec_utils.py:26-64, statement for statement, on the events' device."""
    with torch.no_grad():
        voxel_grid = torch.zeros((C, H, W), dtype=torch.float, device=events['p'].device)
        t_norm = events['t']
        t_norm = (C - 1) * (t_norm - t_norm[0]) / (t_norm[-1] - t_norm[0])
        x0 = events['x'].int()
        y0 = events['y'].int()
        t0 = t_norm.int()
        value = 2 * events['p'] - 1
        for xlim in [x0, x0 + 1]:
            for ylim in [y0, y0 + 1]:
                for tlim in [t0, t0 + 1]:
                    mask = (xlim < W) & (xlim >= 0) & (ylim < H) & (ylim >= 0) & (tlim >= 0) & (tlim < C)
                    interp_weights = value * (1 - (xlim - events['x']).abs()) * (1 - (ylim - events['y']).abs()) * (1 - (tlim - t_norm).abs())
                    index = H * W * tlim.long() + W * ylim.long() + xlim.long()
                    voxel_grid.put_(index[mask], interp_weights[mask], accumulate=True)
        if normalize:
            mask = torch.nonzero(voxel_grid, as_tuple=True)
            if mask[0].size()[0] > 0:
                mean = voxel_grid[mask].mean()
                std = voxel_grid[mask].std()
                if std > 0:
                    voxel_grid[mask] = (voxel_grid[mask] - mean) / std
                else:
                    voxel_grid[mask] = voxel_grid[mask] - mean
    return voxel_grid


def make_set(seed, n, H, W, dev):
    r = np.random.default_rng(seed)
    t = np.sort(r.uniform(0.0, 0.1, n)).astype(np.float32)
    x, y = r.uniform(0, W - 1, n).astype(np.float32), r.uniform(0, H - 1, n).astype(np.float32)
    p = r.integers(0, 2, n).astype(np.float32)
    flt = {k: torch.from_numpy(v).to(dev) for k, v in zip("xytp", (x, y, t, p))}
    raw = dict(flt, x=torch.from_numpy(x.astype(np.int16)).to(dev), y=torch.from_numpy(y.astype(np.int16)).to(dev))
    rows = torch.from_numpy(np.stack([t, np.floor(x), np.floor(y), 2 * p - 1], axis=1).astype(np.float64)).to(dev)
    return flt, raw, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40, help="library calls per timed run (the torch composition: a tenth of it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dsec_voxel_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dsec_voxel.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lines, res = [], {"calls_per_run": a.calls, "rounds": a.rounds}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tools/bench_dsec_voxel.py --calls {a.calls} --rounds {a.rounds} (MI355X, one process; us per event set, median (min, max) of the rounds)")
    for (C, H, W), n in SIZES:
        kmax = 4 if a.kernels_only else max(COUNTS)
        sets = [make_set(1000 + i, n, H, W, dev) for i in range(kmax)]
        r = np.random.default_rng(7)
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        rmap = torch.from_numpy(np.stack([xx + r.uniform(-0.5, 0.5, (H, W)), yy + r.uniform(-0.5, 0.5, (H, W))], axis=2).astype(np.float32)).to(dev)
        grids = [torch.empty(C, H, W, device=dev) for _ in range(kmax)]
        got, want = dsec.voxel_grid_many([sets[0][0]], (C, H, W), True)[0], torch_convert(sets[0][0], C, H, W)
        err = float((got - want).abs().max() / want.abs().max())
        assert err < 1e-4, f"the timed kernel's grid is not the torch composition's: {err:.3g} of the largest cell"
        tag = f"{C}x{H}x{W}_{n:.0e}".replace("+0", "")
        say(f"{C} x {H} x {W}, {n:.0e} events per set; tri against the torch composition: max |diff| {err:.2e} of the largest cell")
        for k in ((4,) if a.kernels_only else COUNTS):
            flt, raw, rows = ([s[j] for s in sets[:k]] for j in range(3))
            tri = timed(lambda: dsec.voxel_grid_many(flt, (C, H, W), True, out=grids[:k]), a.calls, a.rounds, k)
            res[f"{tag}_k{k}_tri_us"] = tri[0]
            if a.kernels_only:
                continue
            rect = timed(lambda: dsec.voxel_grid_many(raw, (C, H, W), True, rectify_maps=rmap, out=grids[:k]), a.calls, a.rounds, k)
            two = timed(lambda: voxelize_many_device(rows, C, H, W, True, out=grids[:k]), a.calls, a.rounds, k)
            ref = timed(lambda: [torch_convert(e, C, H, W) for e in flt], max(2, a.calls // 10), a.rounds, k)
            res.update({f"{tag}_k{k}_tri_rect_us": rect[0], f"{tag}_k{k}_two_vote_us": two[0], f"{tag}_k{k}_torch_us": ref[0],
                        f"{tag}_k{k}_torch_over_tri": ref[0] / tri[0], f"{tag}_k{k}_tri_over_two_vote": tri[0] / two[0]})
            say(f"  {k:2d} sets per call: tri {tri[0]:8.1f} ({tri[1]:.1f}, {tri[2]:.1f})   tri_rect {rect[0]:8.1f} ({rect[1]:.1f}, {rect[2]:.1f})   "
                f"torch {ref[0]:9.1f} ({ref[1]:.1f}, {ref[2]:.1f})   two_vote {two[0]:8.1f} ({two[1]:.1f}, {two[2]:.1f})   "
                f"torch / tri {ref[0] / tri[0]:6.1f} x   tri / two_vote {tri[0] / two[0]:5.2f} x")
        del sets, grids
        torch.cuda.empty_cache()
    if not a.kernels_only:
        res["tri_faster_than_torch_everywhere"] = all(v > 1 for k, v in res.items() if k.endswith("_torch_over_tri"))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
