#!/usr/bin/env python3
"""Golden vectors for the photometric / census warp losses (tests/photo_reference.py, eemflow_photo_many) - produced by EXECUTING THE
REFERENCE'S OWN SOURCES (build container only).  utils_luo/tools.py cannot be imported (cv2, imageio, png, matplotlib are absent and
`collections.Iterable` is gone), so `photo_loss_multi_type`, `photo_loss_function` and `census_loss_torch` are taken out of its
`Loss_tools` class and `torch_warp` out of `tensor_tools` with `ast` and executed unmodified on the CPU.  Nothing of the reference is
copied into the repository; the stored inputs are this script's own (photo_reference.inputs).

Usage:  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_photo.py <reference root>
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from photo_reference import CASES, POINTWISE, Q, inputs, loss  # noqa: E402

WANTED = {"Loss_tools": ("photo_loss_multi_type", "photo_loss_function", "census_loss_torch"), "tensor_tools": ("torch_warp",)}
SHAPES = ((1, 3, 7, 7), (2, 3, 9, 11), (3, 3, 37, 50))               # (B, C, H, W): the reference's census takes C == 3 only
SEED = 71


def ref_classes(path):
    """`Loss_tools` and `tensor_tools` holding the wanted functions alone (the classes may be nested in another class)."""
    tree = ast.parse(open(path).read())
    env = {"torch": torch, "np": np, "nn": nn, "F": F}
    for cname, names in WANTED.items():
        outer = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cname)
        keep = [n for n in outer.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in keep) == sorted(names), (cname, [n.name for n in keep])
        outer.body = keep
        outer.bases, outer.keywords, outer.decorator_list = [], [], []
        exec(compile(ast.Module(body=[outer], type_ignores=[]), path, "exec"), env)
    return env["Loss_tools"], env["tensor_tools"]


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EEMFLOW_REFERENCE_ROOT", "")
    path = os.path.join(root, "utils_luo", "tools.py")
    lt, tt = ref_classes(path)
    out = {"ncases": np.array(len(SHAPES)), "seed": np.array(SEED), "q": np.array(Q),
           "cases": np.array(["%s/%d/%d/%d/%d" % (k, occ, ch, av, r) for k, occ, ch, av, r in CASES])}
    gap = 0.0
    for i, shape in enumerate(SHAPES):
        flow, img1, img2, mask = inputs(SEED + i, shape)
        out[f"flow_{i}"], out[f"img1_{i}"], out[f"img2_{i}"], out[f"mask_{i}"] = flow, img1, img2, mask
        tf, t1, t2, tm = (torch.from_numpy(a) for a in (flow, img1, img2, mask))
        yw = tt.torch_warp(t2, tf)
        table = np.zeros(len(CASES), dtype=np.float32)
        for ci, (kind, occ, ch, av, r) in enumerate(CASES):
            if kind in POINTWISE:
                v = lt.photo_loss_multi_type(t1, yw, tm, photo_loss_type=kind, photo_loss_use_occ=occ)
                kw = dict(kind=kind, use_occ=occ)
            else:
                v = lt.census_loss_torch(t1, yw, tm, Q, ch, occ, averge=av, max_distance=r)
                kw = dict(kind=kind, use_occ=occ, q=Q, charbonnier=ch, average=av, max_distance=r)
            assert v.dtype == torch.float32
            table[ci] = v.item()
            r64 = float(loss(tf, t1, t2, tm, **kw))
            gap = max(gap, abs(float(table[ci]) - r64) / abs(r64))
        out[f"loss_{i}"] = table
        print(shape, "losses", table)
    out["ref_gap"] = np.array(gap, dtype=np.float64)
    dst = os.path.join(HERE, "photo.npz")
    np.savez_compressed(dst, **out)
    print("wrote photo.npz:", len(out), "arrays,", os.path.getsize(dst), "bytes, ref_gap %.3e" % gap)


if __name__ == "__main__":
    main()
