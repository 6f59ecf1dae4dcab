"""Writes tests/golden/dsec_voxel_*.npz from the reference's own utils/dsec_utils.py (VoxelGrid.convert, flow_16bit_to_float), on the CPU.

    python tools/make_dsec_goldens.py /path/to/reference/utils/dsec_utils.py

The reference file is loaded by path and only run, never copied; the fixtures hold inputs and what the reference returned for them
(raw and normalised fp32 grids, a decoded 16-bit flow), a few KB each.  tests/test_dsec_host.py holds tests/dsec_reference.py to them."""
import importlib.util
import os
import sys

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
C, H, W = 5, 12, 16


def load(path):
    spec = importlib.util.spec_from_file_location("dsec_utils_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def convert(ref, ev, normalize):
    grid = ref.VoxelGrid((C, H, W), normalize=normalize).convert({k: torch.from_numpy(v) for k, v in ev.items()})
    return grid.numpy().astype(np.float32)


def random_set(seed, n):
    """Sub-pixel coordinates in (-1.5, W + 0.5) x (-1.5, H + 0.5), UNSORTED t (some before t[0], some after t[n-1]), p in {0, 1}."""
    r = np.random.default_rng(seed)
    return {"x": r.uniform(-1.5, W + 0.5, n).astype(np.float32), "y": r.uniform(-1.5, H + 0.5, n).astype(np.float32),
            "t": r.uniform(0.0, 1.0, n).astype(np.float32), "p": r.integers(0, 2, n).astype(np.float32)}


def edge_set():
    """One event per quirk: x = -0.5 (votes +0.5 / -0.5), x0 + 1 == W, y0 + 1 == H, the last event (tn == C - 1), negative y, t < t[0]."""
    x = np.array([3.25, -0.5, W - 0.75, 5.5, 7.0, 2.5, 9.75, 4.0], dtype=np.float32)
    y = np.array([2.5, 4.0, 6.25, H - 0.5, -0.25, 3.5, 1.0, 8.0], dtype=np.float32)
    t = np.array([0.25, 0.5, 0.625, 0.75, 0.875, 0.125, 0.03125, 1.0], dtype=np.float32)
    p = np.array([1, 1, 0, 1, 0, 1, 0, 1], dtype=np.float32)
    return {"x": x, "y": y, "t": t, "p": p}


def dt0_set():
    ev = random_set(7, 40)
    ev["t"][:] = np.float32(0.5)
    return ev


def main():
    ref = load(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    for name, ev in (("random", random_set(1, 300)), ("edges", edge_set()), ("dt0", dt0_set())):
        np.savez_compressed(os.path.join(OUT, f"dsec_voxel_{name}.npz"), shape=np.array([C, H, W]), raw=convert(ref, ev, False),
                            normalised=convert(ref, ev, True), **ev)
    r = np.random.default_rng(3)
    f16 = r.integers(0, 65536, (6, 9, 3)).astype(np.uint16)
    f16[..., 2] = r.integers(0, 2, (6, 9))
    f16[0, 0] = (2 ** 15, 2 ** 15 + 128, 1)
    flow, valid = ref.flow_16bit_to_float(f16)
    np.savez_compressed(os.path.join(OUT, "dsec_voxel_flow16.npz"), flow_16bit=f16, flow=flow, valid=valid)


if __name__ == "__main__":
    main()
