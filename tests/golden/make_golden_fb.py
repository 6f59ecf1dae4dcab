#!/usr/bin/env python3
"""Golden vectors for the forward-backward consistency check (tests/fb_reference.py, eemflow_fb_check_many) - produced by EXECUTING
THE REFERENCE'S OWN SOURCES (build container only).  utils_luo/tools.py cannot be imported (cv2, imageio, png, matplotlib are absent
and `collections.Iterable` is gone), so `occ_check_model` and `torch_warp` are taken out of its `tensor_tools` class with `ast` and
executed unmodified.  Nothing of the reference is copied into the repository; the stored inputs are this script's own.

Usage:  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_fb.py <reference root>
"""
import ast
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("all", "obj", "out")
ALPHAS = ((1.0, 0.05), (0.01, 0.5))          # the reference's constructor defaults; the setting the GPU tests use


def ref_tensor_tools(path):
    """A `tensor_tools` class holding the reference's occ_check_model and torch_warp alone."""
    tree = ast.parse(open(path).read())
    outer = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "tensor_tools")
    keep = [n for n in outer.body if (isinstance(n, ast.ClassDef) and n.name == "occ_check_model")
            or (isinstance(n, ast.FunctionDef) and n.name == "torch_warp")]
    assert len(keep) == 2
    outer.body = keep
    env = {"torch": torch, "nn": nn}
    exec(compile(ast.Module(body=[outer], type_ignores=[]), path, "exec"), env)
    return env["tensor_tools"]


def pairs():
    """Three small flow pairs whose targets leave the frame on every side; (h, w) with w % 4 != 0 among them."""
    out = []
    for seed, h, w, amp in ((11, 24, 32, 4.0), (12, 37, 50, 9.0), (13, 64, 61, 2.5)):
        rng = np.random.default_rng(seed)
        # smooth fields (a few low frequencies) plus noise: backward ~ -forward with a disturbance, so both mask values occur
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        fw = np.stack([amp * np.sin(2 * np.pi * x / w + rng.uniform(0, 6)) + rng.uniform(-2, 2),
                       amp * np.cos(2 * np.pi * y / h + rng.uniform(0, 6)) + rng.uniform(-2, 2)])
        bw = -fw + rng.standard_normal((2, h, w)) * 0.15 * amp * (rng.uniform(size=(1, h, w)) < 0.5)
        out.append((fw[None].astype(np.float32), bw[None].astype(np.float32)))
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EEMFLOW_REFERENCE_ROOT", "")
    path = os.path.join(root, "utils_luo", "tools.py")
    tt = ref_tensor_tools(path)
    out = {"alphas": np.array(ALPHAS, dtype=np.float64), "modes": np.array(MODES)}
    warnings.simplefilter("ignore")                 # grid_sample's align_corners default notice
    for k, (fw, bw) in enumerate(pairs()):
        out[f"fw_{k}"], out[f"bw_{k}"] = fw, bw
        for ai, (a1, a2) in enumerate(ALPHAS):
            for mode in MODES:
                m1, m2 = tt.occ_check_model(occ_alpha_1=a1, occ_alpha_2=a2, obj_out_all=mode)(torch.from_numpy(fw), torch.from_numpy(bw))
                out[f"mask_fw_{k}_{ai}_{mode}"] = m1.numpy().astype(np.uint8)
                out[f"mask_bw_{k}_{ai}_{mode}"] = m2.numpy().astype(np.uint8)
                print(k, (a1, a2), mode, "consistent: %.3f %.3f" % (m1.mean().item(), m2.mean().item()))
    out["npairs"] = np.array(3)
    np.savez_compressed(os.path.join(HERE, "fb_check.npz"), **out)
    print("wrote fb_check.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "fb_check.npz")), "bytes")


if __name__ == "__main__":
    main()
