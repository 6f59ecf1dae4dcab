#!/usr/bin/env python3
"""Golden vectors for the MVSEC ground-truth propagation (tests/gt_prop_reference.py, eemflow_gt_flow_many) - produced by EXECUTING THE
REFERENCE'S OWN LINES (build container only).  loader/loader_utils.py cannot be imported (cv2, pandas, h5py, torchvision are absent),
so `prop_flow` and `estimate_corresponding_gt_flow` are taken out of it with `ast` and executed unmodified.  cv2 is not installed: the
`cv2` the two functions see is a stub whose `remap` is THIS script's NumPy nearest neighbour - round half to even (cvRound) and a
constant border of 0 (remap's default BORDER_CONSTANT), OpenCV's documented behaviour, which cannot be checked against a cv2 run here.
Nothing of the reference is copied into the repository; the stored inputs are this script's own.

Usage:  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_gt_prop.py <reference root>
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
T, H, W = 10, 20, 28
ZERO_SHARE = 0.01            # at 3 % the eight-interval case keeps under half of its cells (0.46 - 0.48)


def remap_nearest(src, map_x, map_y, interpolation):
    assert interpolation == "nearest" and map_x.dtype == np.float32 and map_y.dtype == np.float32
    h, w = src.shape
    out = np.zeros(map_x.shape, dtype=src.dtype)
    for r in range(map_x.shape[0]):
        for c in range(map_x.shape[1]):
            fx, fy = float(map_x[r, c]), float(map_y[r, c])
            ix, iy = int(round(fx)), int(round(fy))          # Python's round: half to even
            if 0 <= ix < w and 0 <= iy < h:
                out[r, c] = src[iy, ix]
    return out


def reference_functions(path):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("prop_flow", "estimate_corresponding_gt_flow")]
    assert len(keep) == 2
    cv2 = types.SimpleNamespace(remap=remap_nearest, INTER_NEAREST="nearest")
    env = {"numpy": np, "cv2": cv2}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), env)
    return env["estimate_corresponding_gt_flow"]


def stacks():
    rng = np.random.default_rng(20)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.empty((T, 2, H, W), dtype=np.float64)
    for k in range(T):
        base[k, 0] = 1.2 * np.sin(0.3 * y + 0.2 * k) + 0.2 * rng.standard_normal((H, W))
        base[k, 1] = 1.2 * np.cos(0.25 * x - 0.1 * k) + 0.2 * rng.standard_normal((H, W))
    base[rng.uniform(size=base.shape) < ZERO_SHARE] = 0.0
    base = base.astype(np.float32)
    ts = 100.0 + np.cumsum(0.05 + 0.002 * rng.uniform(size=T))
    tie = base.copy()                                   # (u, v) = (0.5, 1.5) in frame 4: a walk that starts ON ts[4] (scale 1) puts these
    for py, px in ((7, 10), (12, 3), (4, 21)):          # pixels on exact .5 ties for its second step
        tie[4, 0, py, px], tie[4, 1, py, px] = 0.5, 1.5
    border = base.copy()
    border[:, 1, 0, :] = -2.7                           # the top row flows out of the frame, the right column too
    border[:, 0, :, W - 1] = 3.1
    return {"base": base, "tie": tie, "border": border}, ts


def cases(ts):
    d = np.diff(ts)
    return [
        ("inside_one_interval", "base", ts[2] + 0.2 * d[2], ts[2] + 0.7 * d[2]),                 # short branch
        ("short_across_a_boundary", "base", ts[5] + 0.6 * d[5], ts[6] + 0.3 * d[6]),             # dt < gt_dt although a boundary is crossed
        ("crossing_one", "base", ts[3] + 0.3 * d[3], ts[4] + 0.8 * d[4]),
        ("crossing_four", "base", ts[1] + 0.5 * d[1], ts[5] + 0.25 * d[5]),
        ("starting_on_a_timestamp", "base", ts[2], ts[4] + 0.5 * d[4]),
        ("ending_on_a_timestamp", "base", ts[3] + 0.4 * d[3], ts[6]),
        ("exactly_one_interval", "base", ts[6], ts[7]),                                          # gt_dt == dt: long branch, last step of scale 0
        ("exactly_one_interval_early", "base", ts[1], ts[2]),
        ("first_interval_spanning_eight", "base", ts[0] + 0.4 * d[0], ts[8] + 0.3 * d[8]),
        ("tie", "tie", ts[4], ts[6] + 0.3 * d[6]),
        ("leaving_the_frame", "border", ts[2] + 0.5 * d[2], ts[4] + 0.5 * d[4]),
    ]


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EEMFLOW_REFERENCE_ROOT", "")
    path = os.path.join(root, "loader", "loader_utils.py")
    estimate = reference_functions(path)
    st, ts = stacks()
    out = {"ts": ts}
    for name, arr in st.items():
        out["stack_" + name] = arr
    cs = cases(ts)
    out["names"] = np.array([c[0] for c in cs])
    out["stacks"] = np.array([c[1] for c in cs])
    out["starts"] = np.array([c[2] for c in cs], dtype=np.float64)
    out["ends"] = np.array([c[3] for c in cs], dtype=np.float64)
    for i, (name, which, start, end) in enumerate(cs):
        gt = np.float32(st[which])                           # MVSEC_encoder.py:133 reads flow_dist as float32
        u, v = estimate(np.array(gt[:, 0]), np.array(gt[:, 1]), ts, np.array(start), np.array(end))
        assert u.dtype == v.dtype
        out[f"ref_{i}"] = np.stack([u, v])
        print("%-32s %-8s nonzero u %.3f v %.3f" % (name, u.dtype, (u != 0).mean(), (v != 0).mean()))
    np.savez_compressed(os.path.join(HERE, "gt_prop.npz"), **out)
    print("wrote gt_prop.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "gt_prop.npz")), "bytes")


if __name__ == "__main__":
    main()
