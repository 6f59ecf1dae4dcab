"""Host-side checks of E-RAFT's stream and warm start (ERAFT.forward_stream, forward_interpolate, the harness's stream=n): no GPU.

fi_restated is the CPU restatement of forward_interpolate_pytorch (utils/image_utils.py:11-84) the GPU tests compare the kernel with:
four passes in the reference's order, each adding z * w and w in source order in fp32 (np.add.at adds in the order it is given),
then sum / (weight sum + 1e-15f)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from eemflow_amd import _lib
from eemflow_amd.eraft import ERAFT, forward_interpolate
from eemflow_amd.harness import Logger, TestRaftEvents

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HEADER = os.path.join(os.path.dirname(HERE), "include", "eemflow_hip.h")
NEW_SYMBOLS = ("eraft_forward_interpolate", "eraft_forward_stream", "eraft_stream_reset", "eraft_stream_pending")
RANDOM_CASES = ("rand60x80", "rand92x160")
SPECIAL_CASES = ("integer", "leave", "converge", "zero", "near1px")


def fi_restated(flow):
    """forward_interpolate_pytorch on a [B, 2, h, w] float32 array, in the reference's fp32 operations and summation order."""
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    b, _, h, w = flow.shape
    y0, x0 = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x0, y0 = x0.ravel().astype(np.float32), y0.ravel().astype(np.float32)
    one, eps = np.float32(1), np.float32(1e-15)
    out = np.zeros_like(flow)
    for i in range(b):
        dx, dy = flow[i, 0].ravel(), flow[i, 1].ravel()
        x1, y1 = x0 + dx, y0 + dy
        vx, vy, ws = (np.zeros(h * w, np.float32) for _ in range(3))
        with np.errstate(invalid="ignore"):
            for xv in (np.floor(x1), np.ceil(x1)):
                for yv in (np.floor(y1), np.ceil(y1)):
                    m = (xv < w) & (xv >= 0) & (yv < h) & (yv >= 0)
                    wt = (one - np.abs(x1 - xv)) * (one - np.abs(y1 - yv))
                    idx = (xv[m] + np.float32(w) * yv[m]).astype(np.int64)
                    np.add.at(vx, idx, (dx * wt)[m])
                    np.add.at(vy, idx, (dy * wt)[m])
                    np.add.at(ws, idx, wt[m])
        den = ws + eps
        out[i, 0] = (vx / den).reshape(h, w)
        out[i, 1] = (vy / den).reshape(h, w)
    return out


def rand_flow(g, name):
    seed, b, h, w = (int(x) for x in g[f"{name}_seed"])
    return (np.random.default_rng(seed).standard_normal((b, 2, h, w)) * float(g[f"{name}_scale"])).astype(np.float32)


def golden_cases():
    """(name, input, reference output) of forward_interpolate.npz."""
    g = np.load(os.path.join(GOLDEN, "forward_interpolate.npz"))
    return ([(n, rand_flow(g, n), g[f"{n}_out"]) for n in RANDOM_CASES] +
            [(n, g[f"{n}_in"], g[f"{n}_out"]) for n in SPECIAL_CASES])


@pytest.mark.parametrize("case", range(len(RANDOM_CASES) + len(SPECIAL_CASES)))
def test_restated_interpolation_matches_reference_bitwise(case):
    name, flow, ref = golden_cases()[case]
    got = fi_restated(flow)
    assert got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{name}: {int((got != ref).sum())} cells differ"


def test_golden_cases_cover_the_edges():
    """The fixture exercises what the kernel must reproduce: integer landings, off-grid sources, many sources per cell, weight sums
    below 1e-8 (where + 1e-15 shows), unreached cells."""
    cases = {n: (f, r) for n, f, r in golden_cases()}
    f, _ = cases["integer"]
    assert np.array_equal(f, np.round(f))
    f, r = cases["leave"]
    h, w = f.shape[2:]
    x1 = np.arange(w)[None, :] + f[0, 0]
    assert ((x1 < -1) | (x1 >= w)).mean() > 0.3 and (r == 0).any()
    f, _ = cases["converge"]
    y0, x0 = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cells = (np.floor(y0 + f[0, 1]) * w + np.floor(x0 + f[0, 0])).astype(np.int64).ravel()
    assert np.bincount(cells[(cells >= 0) & (cells < h * w)]).max() >= 24
    f, r = cases["near1px"]
    lat = f[0, 0] < 2                                                      # the lattice sources; their own cells' weight sums:
    x1, y1 = (x0 + f[0, 0])[lat].astype(np.float32), (y0 + f[0, 1])[lat].astype(np.float32)
    wsum = (1 - (x1 - np.floor(x1))).astype(np.float64) * (1 - (y1 - np.floor(y1)))
    assert (wsum < 1e-8).mean() > 0.5 and (wsum > 0).all()
    assert np.isfinite(r).all() and (r[0][:, lat] != 0).all()


def test_forward_interpolate_refuses_cpu_tensors():
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        forward_interpolate(torch.zeros(1, 2, 4, 4))


def _module():
    net = ERAFT("", n_first_channels=5).eval()
    net.change_imagesize((64, 64))
    return net


def test_forward_stream_refuses_cpu_tensors():
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        _module().forward_stream([torch.zeros(1, 5, 64, 64), torch.zeros(1, 5, 64, 64)])


def test_forward_stream_volume_count():
    net = _module()
    with pytest.raises(ValueError, match="1..16"):
        net.forward_stream([])
    with pytest.raises(ValueError, match="1..16"):
        net.forward_stream([torch.zeros(1, 5, 8, 8)] * 17)


class _CudaLike:
    """Just enough of a CUDA tensor for the argument checks that come before any device work."""

    def __init__(self, shape, device="cuda:0"):
        self.shape, self.device, self.is_cuda = torch.Size(shape), device, True

    def contiguous(self):
        return self

    def float(self):
        return self

    def dim(self):
        return len(self.shape)


def test_forward_stream_refuses_mixed_shapes_and_bad_volumes():
    net = _module()
    with pytest.raises(ValueError, match="share one shape"):
        net.forward_stream([_CudaLike((1, 5, 64, 64)), _CudaLike((1, 5, 64, 32))])
    with pytest.raises(ValueError, match=r"\(1,5,H,W\)"):
        net.forward_stream([_CudaLike((2, 5, 64, 64))])


def test_forward_stream_is_inference_only():
    net = ERAFT("", n_first_channels=5)                                    # train mode: BatchNorm in train
    net.change_imagesize((64, 64))
    with pytest.raises(RuntimeError, match="BatchNorm"):
        net.forward_stream([_CudaLike((1, 5, 64, 64))])
    net.eval()
    with pytest.raises(RuntimeError, match="no_grad"):
        net.forward_stream([_CudaLike((1, 5, 64, 64))])
    net.alternate_corr = True
    with torch.no_grad(), pytest.raises(ValueError, match="alternate_corr"):
        net.forward_stream([_CudaLike((1, 5, 64, 64))])


def test_warm_start_attribute_and_replicate():
    net = _module()
    assert net.warm_start is False
    net.warm_start = True
    assert net.replicate().warm_start is True


def test_reset_stream_without_context():
    net = _module()
    net._stream_prev = object()
    net.reset_stream()                                                     # no context yet: a no-op on the device side
    assert net._stream_prev is None
    net._stream_prev = object()
    net.change_imagesize((64, 64))                                         # the same size keeps the carry
    assert net._stream_prev is not None
    net.change_imagesize((32, 32))                                         # a new size resets it
    assert net._stream_prev is None


class _FakeStreamModel(torch.nn.Module):
    """forward_stream on CPU tensors (an E-RAFT-like model: a list of predictions per pair): flow p = the ids of its two windows."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.prev, self.final_only, self.resets = None, False, 0

    def reset_stream(self):
        self.prev, self.resets = None, self.resets + 1

    def forward_stream(self, volumes):
        vols = list(volumes)
        seq = ([self.prev] if self.prev is not None else []) + vols
        self.prev = vols[-1]
        return [((a, b), [torch.zeros(2), torch.stack([a.flatten()[0], b.flatten()[0]])]) for a, b in zip(seq[:-1], seq[1:])]


class _FakeNoStream(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


class _Windows:
    consecutive_windows = True

    def __init__(self, n_samples):
        self.n = n_samples

    def __len__(self):
        return self.n

    def get_windows(self, first, count):
        return [torch.full((5, 4, 4), float(j)) for j in range(first, first + count)], [{"idx": j} for j in range(first, first + count)]


def test_harness_stream_accepts_any_model_with_forward_stream():
    from eemflow_amd.harness import stream_chunks
    model, seen = _FakeStreamModel(), []
    for idx, targets, flows in stream_chunks(_Windows(9), model, 4, torch.device("cpu")):
        for i, t, f in zip(idx, targets, flows):
            assert t["idx"] == i and f.tolist() == [float(i), float(i + 1)]    # the LAST prediction of each pair
        seen += idx
    assert seen == list(range(9)) and model.resets == 1
    t = TestRaftEvents(_Windows(9), (4, 4), logger=Logger(verbose=False))
    try:                                                                   # (past the model check the CPU-only run may stop anywhere)
        t.test_multi_sequence(model, sequence_list=(), stride=1, stream=4)
    except ValueError as e:
        assert "forward_stream" not in str(e)
    except Exception:
        pass


def test_harness_stream_refuses_a_model_without_forward_stream():
    t = TestRaftEvents(_Windows(9), (4, 4), logger=Logger(verbose=False))
    with pytest.raises(ValueError, match=r"forward_stream \(EEMFlow, ERAFT\); _FakeNoStream has none"):
        t.test_multi_sequence(_FakeNoStream(), sequence_list=("a",), stride=1, stream=4)


def test_new_symbols_in_header_and_library():
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        m = re.search(rf"\bint {name}\(", text)
        assert m, f"{name} is not declared in include/eemflow_hip.h"
        block = text[:m.start()].rsplit("*/", 1)[0].rsplit("/*", 1)[-1]
        assert "Replaces:" in block, f"{name}'s comment has no Replaces: line"
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
