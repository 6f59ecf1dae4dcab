#!/usr/bin/env python3
"""Golden vectors for the weighted SSIM warp loss (tests/ssim_reference.py, eemflow_ssim_many) - produced by EXECUTING THE REFERENCE'S
OWN SOURCES (build container only).  utils_luo/tools.py cannot be imported (cv2, imageio, png, matplotlib are absent and
`collections.Iterable` is gone), so `weighted_ssim` and `photo_loss_multi_type` are taken out of its `Loss_tools` class and `torch_warp`
out of `tensor_tools` with `ast` and executed unmodified on the CPU.  photo_loss_multi_type hands weighted_ssim no c1 / c2, so the two
other branches are reached through a subclass whose weighted_ssim passes them on to the reference's own function.  Nothing of the
reference is copied into the repository; the stored inputs are this script's own (photo_reference.inputs).

Usage:  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_ssim.py <reference root>
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
from ssim_reference import CASES, case_id, inputs, loss  # noqa: E402

WANTED = {"Loss_tools": ("weighted_ssim", "photo_loss_multi_type"), "tensor_tools": ("torch_warp",)}
SHAPES = ((1, 3, 7, 7), (2, 5, 9, 11), (2, 15, 37, 50), (2, 3, 33, 129))            # (B, C, H, W)
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


def with_constants(lt, c1, c2):
    """Loss_tools whose photo_loss_multi_type reaches the reference's weighted_ssim with these c1 and c2."""
    class Branch(lt):
        @classmethod
        def weighted_ssim(cls, x, y, weight):
            return lt.weighted_ssim.__func__(cls, x, y, weight, c1=c1, c2=c2)
    return Branch


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EEMFLOW_REFERENCE_ROOT", "")
    path = os.path.join(root, "utils_luo", "tools.py")
    lt, tt = ref_classes(path)
    out = {"ncases": np.array(len(SHAPES)), "seed": np.array(SEED), "cases": np.array([case_id(c) for c in CASES])}
    gap = 0.0
    for i, shape in enumerate(SHAPES):
        flow, img1, img2, mask = inputs(SEED + i, shape)
        out[f"flow_{i}"], out[f"img1_{i}"], out[f"img2_{i}"], out[f"mask_{i}"] = flow, img1, img2, mask
        tf, t1, t2, tm = (torch.from_numpy(a) for a in (flow, img1, img2, mask))
        yw = tt.torch_warp(t2, tf)
        table = np.zeros(len(CASES), dtype=np.float32)
        for ci, (occ, c1, c2) in enumerate(CASES):
            v = with_constants(lt, c1, c2).photo_loss_multi_type(t1, yw, tm, photo_loss_type="SSIM", photo_loss_use_occ=occ)
            assert v.dtype == torch.float32
            table[ci] = v.item()
            r64 = float(loss(tf, t1, t2, tm, use_occ=occ, c1=c1, c2=c2))
            gap = max(gap, abs(float(table[ci]) - r64) / abs(r64))
        if i == 0:                                                   # the defaults of the reference are the first branch
            plain = lt.photo_loss_multi_type(t1, yw, tm, photo_loss_type="SSIM", photo_loss_use_occ=False)
            assert float(plain) == float(table[0]), (float(plain), table[0])
        out[f"loss_{i}"] = table
        print(shape, "losses", table)
    out["ref_gap"] = np.array(gap, dtype=np.float64)
    dst = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(dst, **out)
    print("wrote ssim.npz:", len(out), "arrays,", os.path.getsize(dst), "bytes, ref_gap %.3e" % gap)


if __name__ == "__main__":
    main()
