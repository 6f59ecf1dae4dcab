#!/usr/bin/env python3
"""Golden vectors for the event warp (tests/iwe_reference.py, eemflow_warp_events) - produced by EXECUTING THE REFERENCE'S OWN SOURCE
(build container only).  utils_luo/event_utils.py cannot be imported (it needs cv2, pandas and matplotlib), so
`warp_events_flow_torch` is taken out of it with `ast` and executed unmodified, in fp32 and in fp64.  Nothing of the reference is copied
into the repository; the stored inputs are this script's own.

Three cases, each with N events over a window of T seconds and the flow [6 sin(2 pi x / W) + 2, 4 cos(2 pi y / H)] scaled by -1 / T
(the reference's function multiplies the flow by t - t0, so this is a displacement over the window): u depends on x alone and v on y
alone, and the file stores one row / one column of them.  Explicit t0 values: the default (the last event's t), t[0], and mid-window.

Usage:  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_iwe.py <reference root>
"""
import ast
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
N = 1000
CASES = ((21, 37, 50, "integer"), (22, 64, 61, "fractional"), (23, 260, 346, "integer"))   # seed, H, W, coordinates


def ref_warp(path):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "warp_events_flow_torch"]
    assert len(keep) == 1
    env = {"torch": torch, "F": F}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), env)
    return env["warp_events_flow_torch"]


def case(seed, h, w, kind):
    rng = np.random.default_rng(seed)
    span = 0.05
    t = np.sort(np.round(rng.uniform(0, span, N) * 1e6) * 1e-6)
    if kind == "integer":
        x, y = rng.integers(0, w, N).astype(np.float64), rng.integers(0, h, N).astype(np.float64)
    else:                                              # up to 2 px outside the frame on every side
        x, y = rng.uniform(-2.0, w + 1.0, N), rng.uniform(-2.0, h + 1.0, N)
        x[:4] = [-2.0, w + 1.0, 0.25, w - 1.0]
        y[:4] = [0.5, h - 1.0, -2.0, h + 1.0]
    p = rng.integers(0, 2, N) * 2.0 - 1.0
    T = t[-1] - t[0]
    u_row = ((6.0 * np.sin(2 * np.pi * np.arange(w) / w) + 2.0) * (-1.0 / T)).astype(np.float32)
    v_col = ((4.0 * np.cos(2 * np.pi * np.arange(h) / h)) * (-1.0 / T)).astype(np.float32)
    return np.stack([t, x, y, p], axis=1), u_row, v_col


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EEMFLOW_REFERENCE_ROOT", "")
    path = os.path.join(root, "utils_luo", "event_utils.py")
    warp = ref_warp(path)
    warnings.simplefilter("ignore")
    out = {"ncases": np.array(len(CASES))}
    for k, (seed, h, w, kind) in enumerate(CASES):
        ev, u_row, v_col = case(seed, h, w, kind)
        out[f"events_{k}"], out[f"u_row_{k}"], out[f"v_col_{k}"] = ev, u_row, v_col
        flow = torch.stack([torch.from_numpy(u_row)[None, :].expand(h, w), torch.from_numpy(v_col)[:, None].expand(h, w)]).contiguous()
        t0s = np.array([np.nan, ev[0, 0], 0.5 * (ev[0, 0] + ev[-1, 0])])         # NaN: the default (t0=None)
        out[f"t0_{k}"] = t0s
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            e = torch.from_numpy(ev).to(dt)
            for j, t0 in enumerate(t0s):
                xw, yw = warp(e[:, 1].clone(), e[:, 2].clone(), e[:, 0].clone(), e[:, 3].clone(), flow.to(dt).clone(),
                              None if np.isnan(t0) else float(t0))
                out[f"xw_{k}_{j}_{name}"], out[f"yw_{k}_{j}_{name}"] = xw.numpy(), yw.numpy()
                print(k, kind, name, "t0", t0, "moved by up to %.3f px" % float((xw - e[:, 1]).abs().max()))
    dst = os.path.join(HERE, "iwe.npz")
    np.savez_compressed(dst, **out)
    print("wrote iwe.npz:", len(out), "arrays,", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
