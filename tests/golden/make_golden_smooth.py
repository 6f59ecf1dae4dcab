#!/usr/bin/env python3
"""Golden vectors for the edge-aware smoothness loss (tests/smooth_reference.py, eemflow_smoothness_many) - produced by EXECUTING THE
REFERENCE'S OWN SOURCES (build container only).  utils_luo/tools.py cannot be imported (cv2, imageio, png, matplotlib are absent and
`collections.Iterable` is gone), so `edge_aware_smoothness_order1`, `edge_aware_smoothness_order2` and `flow_smooth_delta` are taken
out of its `Loss_tools` class with `ast` and executed unmodified.  Nothing of the reference is copied into the repository; the stored
inputs are this script's own.

Usage:  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_smooth.py <reference root>
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from smooth_reference import SETTINGS, smoothness  # noqa: E402

NAMES = ("edge_aware_smoothness_order1", "edge_aware_smoothness_order2", "flow_smooth_delta")
CONSTANTS = (1.0, 0.7)
SHAPES = ((1, 1, 3, 3), (2, 5, 5, 7), (3, 15, 37, 50))              # (B, C, H, W)


def ref_loss_tools(path):
    """A `Loss_tools` class holding the reference's three smoothness functions alone."""
    tree = ast.parse(open(path).read())
    outer = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Loss_tools")
    keep = [n for n in outer.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in keep) == sorted(NAMES)
    outer.body = keep
    outer.bases, outer.keywords, outer.decorator_list = [], [], []
    env = {"torch": torch}
    exec(compile(ast.Module(body=[outer], type_ignores=[]), path, "exec"), env)
    return env["Loss_tools"]


def inputs(seed, shape):
    """A flow of a few low frequencies plus noise with a patch of CONSTANT flow (differences of exactly 0: sign(0) = 0), and an edge
    image like an event volume: mostly empty, quarter-integer counts elsewhere (it also keeps the file small)."""
    b, c, h, w = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    pred = np.stack([np.stack([3.0 * np.sin(2 * np.pi * x / w + rng.uniform(0, 6)) + 0.3 * rng.standard_normal((h, w)),
                               2.0 * np.cos(2 * np.pi * y / h + rng.uniform(0, 6)) + 0.3 * rng.standard_normal((h, w))]) for _ in range(b)])
    ph, pw = max(2, (h + 1) // 2), max(2, (w + 1) // 2)
    pred[:, 0, :ph, :pw] = 0.75
    pred[:, 1, :ph, :pw] = -1.5
    img = np.round(rng.standard_normal((b, c, h, w)) * 3.0) / 4.0 * (rng.uniform(size=(b, c, h, w)) < 0.35)
    return pred.astype(np.float32), img.astype(np.float32)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EEMFLOW_REFERENCE_ROOT", "")
    path = os.path.join(root, "utils_luo", "tools.py")
    lt = ref_loss_tools(path)
    fn = {1: lt.edge_aware_smoothness_order1, 2: lt.edge_aware_smoothness_order2}
    out = {"ncases": np.array(len(SHAPES)), "constants": np.array(CONSTANTS, dtype=np.float64),
           "settings": np.array(["%d/%s/%s" % s for s in SETTINGS])}
    gap = 0.0
    for k, shape in enumerate(SHAPES):
        pred, img = inputs(31 + k, shape)
        out[f"pred_{k}"], out[f"img_{k}"] = pred, img
        tp, ti = torch.from_numpy(pred), torch.from_numpy(img)
        table = np.zeros((len(CONSTANTS), len(SETTINGS)), dtype=np.float32)
        for ci, constant in enumerate(CONSTANTS):
            for si, (order, wt, et) in enumerate(SETTINGS):
                v = fn[order](ti, tp, constant=constant, weight_type=wt, error_type=et)
                assert v.dtype == torch.float32
                table[ci, si] = v.item()
                r64 = float(smoothness(tp.double(), ti.double(), order, constant, wt, et))
                gap = max(gap, abs(float(table[ci, si]) - r64) / abs(r64))
        out[f"loss_{k}"] = table
        d = lt.flow_smooth_delta(tp)
        out[f"delta_{k}"] = np.array(d.item(), dtype=np.float32)
        r64 = float(smoothness(tp.double(), None, 1, 1.0, "gauss", "L1"))
        gap = max(gap, abs(float(out[f"delta_{k}"]) - r64) / abs(r64))
        print(shape, "losses", table[0], "delta", float(d))
    out["ref_gap"] = np.array(gap, dtype=np.float64)
    dst = os.path.join(HERE, "smooth.npz")
    np.savez_compressed(dst, **out)
    print("wrote smooth.npz:", len(out), "arrays,", os.path.getsize(dst), "bytes, ref_gap %.3e" % gap)


if __name__ == "__main__":
    main()
