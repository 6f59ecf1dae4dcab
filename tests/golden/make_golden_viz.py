#!/usr/bin/env python3
"""Golden vectors for the flow and event visualisations (tests/viz_reference.py, eemflow_flow_to_image_many, eemflow_event_image_many) -
produced by EXECUTING THE REFERENCE'S OWN SOURCES (build container only).  utils_luo/tools.py and test_mvsec.py cannot be imported (cv2,
imageio, png, matplotlib are absent), so `flow_to_image_dmax` is taken out of the `tensor_tools` class and `vis_map_RGB` out of the `Test`
class with `ast` and executed unmodified; `vis_map_RGB` runs against a stand-in `cv2` whose `imwrite` keeps the array (and the file name,
which carries the density) instead of encoding it.  Nothing of the reference is copied into the repository; the stored inputs are this
script's own.

Usage:  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_viz.py <reference root>
"""
import ast
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-4                        # no event pixel this close to a threshold: summation order cannot decide it


def take(path, class_name, func_name, env):
    """`class_name` holding `func_name` alone, executed in `env`."""
    tree = ast.parse(open(path).read())
    outer = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    keep = [n for n in outer.body if isinstance(n, ast.FunctionDef) and n.name == func_name]
    assert len(keep) == 1, (class_name, func_name)
    outer.body, outer.bases, outer.keywords, outer.decorator_list = keep, [], [], []
    exec(compile(ast.Module(body=[outer], type_ignores=[]), path, "exec"), env)
    return env[class_name]


def grid(values, step):
    """float32 values on a grid of `step` (a power of two): inputs that compress, exactly representable."""
    return (np.round(np.asarray(values, dtype=np.float64) / step) * step).astype(np.float32)


def flow_cases():
    """[(name, (2,H,W) float32)]"""
    out = []
    hand = np.zeros((2, 4, 6), dtype=np.float32)
    vectors = [(2, 0), (-2, 0), (0, -2), (0, 2), (3, 0.0), (3, -0.0),
               (5, 0), (3, 4), (-4, 3), (0, 0), (1, 1), (-1, -1),
               (0.5, -0.25), (-0.125, 0.75), (4.5, -1), (-2, -4), (1, -3), (-3, 1),
               (0, 4.75), (4.75, 0), (-4.75, 0), (0, -4.75), (2.5, 2.5), (-0.0, 2)]
    for k, (u, v) in enumerate(vectors):
        hand[0].flat[k], hand[1].flat[k] = u, v
    assert np.signbit(hand[1].flat[5]) and not np.signbit(hand[1].flat[4])
    out.append(("hand", hand))
    out.append(("zero", np.zeros((2, 8, 8), dtype=np.float32)))
    rng = np.random.default_rng(20)
    one_nan = grid(rng.standard_normal((2, 8, 8)) * 3, 2.0 ** -6)
    one_nan[0, 3, 5] = np.nan
    out.append(("nan", one_nan))
    unknown = grid(rng.standard_normal((2, 8, 8)) * 3, 2.0 ** -6)
    unknown[1, 2, 2] = np.inf
    unknown[0, 6, 1] = 2e7
    out.append(("unknown", unknown))
    for k in range(40):
        r = np.random.default_rng(100 + k)
        out.append((f"rand{k:02d}", (r.standard_normal((2, 8, 8)) * r.uniform(0.1, 50)).astype(np.float32)))
    for seed, h, w, amp in ((31, 37, 50, 6.0), (32, 64, 61, 2.5), (33, 260, 346, 20.0)):
        r = np.random.default_rng(seed)
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        f = np.stack([amp * np.sin(2 * np.pi * x / w + r.uniform(0, 6)) + r.uniform(-1, 1),
                      amp * np.cos(2 * np.pi * y / h + r.uniform(0, 6)) + r.uniform(-1, 1)])
        f += r.standard_normal((2, h, w)) * 0.05 * amp
        out.append((f"smooth_{h}x{w}", grid(f, 2.0 ** -7)))
    return out


def normalised(raw, record):
    """The volume the first convolution sees: (x - mean) * (1 / sd) on the non-zero voxels, fp32."""
    mean, sd = np.float32(record[0]), np.float32(record[1])
    return np.where(raw != 0, (raw - mean) * (np.float32(1) / sd), raw).astype(np.float32)


def event_cases():
    """[(name, volume (5,H,W) float32 as the reference sees it, raw volume or None, record or None)]"""
    out = []
    for name, seed, h, w, keep_raw in (("norm_37x50", 41, 37, 50, False), ("norm_260x346", 42, 260, 346, False), ("raw_64x61", 43, 64, 61, True)):
        r = np.random.default_rng(seed)
        raw = np.zeros((5, h, w), dtype=np.float32)
        dense = r.uniform(size=(h, w)) < 0.2
        for c in range(5):
            on = dense & (r.uniform(size=(h, w)) < 0.45)
            raw[c][on] = (r.integers(1, 9, size=int(on.sum())) * 0.25 * r.choice([-1.0, 1.0], size=int(on.sum()))).astype(np.float32)
        nz = raw[raw != 0].astype(np.float64)
        record = np.array([nz.mean(), nz.std(), 1.0, 1.0], dtype=np.float32)
        for _ in range(20):                                   # empty the pixels that sit on a threshold (the record stays as it is)
            s = normalised(raw, record).astype(np.float64).sum(0)
            mean = s.mean()
            close = (np.abs(s - (mean - 0.2)) < 10 * MARGIN) | (np.abs(s - (mean + 0.2)) < 10 * MARGIN) | (np.abs(s - 0.1) < 10 * MARGIN)
            if not close.any():
                break
            raw[:, close] = 0
        out.append((name, normalised(raw, record), raw if keep_raw else None, record if keep_raw else None))
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EEMFLOW_REFERENCE_ROOT", "")
    tt = take(os.path.join(root, "utils_luo", "tools.py"), "tensor_tools", "flow_to_image_dmax", {"np": np})
    written = []
    fake_cv2 = types.SimpleNamespace(imwrite=lambda path, img: written.append((os.path.basename(path), np.array(img))))
    tester = take(os.path.join(root, "test_mvsec.py"), "Test", "vis_map_RGB", {"np": np, "torch": torch, "os": os, "cv2": fake_cv2})
    out = {"numpy_version": np.array(np.__version__)}
    names = []
    for name, flow in flow_cases():
        hw2 = np.ascontiguousarray(flow.transpose(1, 2, 0)).copy()             # the harness's f_est[0].numpy().transpose(1,2,0), float32
        assert hw2.dtype == np.float32
        with np.errstate(all="ignore"):
            img = tt.flow_to_image_dmax(hw2)
        assert img.dtype == np.uint8 and img.shape == flow.shape[1:] + (3,)
        out[f"flow_{name}"], out[f"flow_image_{name}"] = flow, img
        names.append(name)
        print(name, flow.shape, "mean colour", img.reshape(-1, 3).mean(0).round(1))
    out["flow_names"] = np.array(names)
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        self = types.SimpleNamespace(save_path=tmp)
        for name, vol, raw, record in event_cases():
            s = vol.astype(np.float64).sum(0)
            mean = s.mean()
            margin = min(np.abs(s - (mean - 0.2)).min(), np.abs(s - (mean + 0.2)).min(), np.abs(s - 0.1).min())
            assert margin >= MARGIN, (name, margin)
            del written[:]
            tester.vis_map_RGB(self, torch.from_numpy(vol)[None], "x.jpg")
            (fname, img), = written
            density = float(fname[len("x_"):-len(".jpg")])
            count = int(np.sum(vol.sum(0) > 0.1))
            assert abs(count / s.size - density) <= 5e-4                        # the file name's three decimals
            out[f"event_image_{name}"], out[f"event_count_{name}"] = img.astype(np.uint8), np.array(count)
            if raw is None:
                out[f"event_volume_{name}"] = vol
            else:
                out[f"event_raw_{name}"], out[f"event_record_{name}"] = raw, record
            names.append(name)
            print(name, vol.shape, "density %.3f" % density, "margin %.2e" % margin, "red %.3f blue %.3f" % (
                (img[..., 2] == 0).mean(), (img[..., 0] == 0).mean()))
    out["event_names"] = np.array(names)
    path = os.path.join(HERE, "viz.npz")
    np.savez_compressed(path, **out)
    print("wrote viz.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
