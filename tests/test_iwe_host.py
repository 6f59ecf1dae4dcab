"""Host-side checks of the image of warped events and the flow warp loss: the torch restatement of the reference's warp
(tests/iwe_reference.py) against the fixture made from the reference's own function (tests/golden/iwe.npz, make_golden_iwe.py), the
restated semantics on cases with known answers, the C ABI's declarations, and the argument checks of eemflow_amd.iwe, the datasets,
the harness hook and the command line.  No GPU."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import eemflow_amd
from eemflow_amd import _lib
from eemflow_amd.harness import Logger, TestRaftEvents

from iwe_reference import (accumulate, fwl_reference, iwe_reference, metric_refs, separable_flow, warp_direct, warp_events_reference)

iwe = importlib.import_module("eemflow_amd.iwe")        # (the package's attribute `iwe` is the one-job function)
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "iwe.npz")
SHAPES = ((37, 50), (64, 61), (260, 346))


def _case(z, k, dtype):
    ev = torch.from_numpy(z[f"events_{k}"]).to(dtype)
    flow = separable_flow(torch.from_numpy(z[f"u_row_{k}"]), torch.from_numpy(z[f"v_col_{k}"])).to(dtype)
    return ev, flow


def test_fixture_is_small_and_has_the_three_cases():
    assert os.path.getsize(GOLDEN) < 300 * 1024
    z = np.load(GOLDEN)
    assert int(z["ncases"]) == 3
    for k, (h, w) in enumerate(SHAPES):
        ev = z[f"events_{k}"]
        assert ev.shape[1] == 4 and 2 <= ev.shape[0] <= 2000 and np.all(np.diff(ev[:, 0]) >= 0)
        assert z[f"u_row_{k}"].shape == (w,) and z[f"v_col_{k}"].shape == (h,)
        t0 = z[f"t0_{k}"]
        assert np.isnan(t0[0]) and t0[1] == ev[0, 0] and ev[0, 0] < t0[2] < ev[-1, 0]       # default, t[0], mid-window
        integer = np.all(ev[:, 1:3] == np.round(ev[:, 1:3]))
        assert integer == (k != 1)
    x, y = z["events_1"][:, 1], z["events_1"][:, 2]                      # fractional: 2 px outside the frame on every side
    assert x.min() == -2.0 and x.max() == 61 + 1.0 and y.min() == -2.0 and y.max() == 64 + 1.0


@pytest.mark.parametrize("name,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_restated_warp_equals_the_reference_function(name, dtype):
    z = np.load(GOLDEN)
    for k in range(3):
        ev, flow = _case(z, k, dtype)
        for j, t0 in enumerate(z[f"t0_{k}"]):
            xw, yw = warp_events_reference(ev[:, 1], ev[:, 2], ev[:, 0], ev[:, 3], flow, None if np.isnan(t0) else float(t0))
            assert xw.dtype == dtype
            assert torch.equal(xw, torch.from_numpy(z[f"xw_{k}_{j}_{name}"])), (k, j)
            assert torch.equal(yw, torch.from_numpy(z[f"yw_{k}_{j}_{name}"])), (k, j)


def test_pixel_coordinate_warp_is_the_reference_warp_in_fp64():
    """The library samples in pixel coordinates; the reference normalises to [-1, 1] and grid_sample un-normalises: in fp64 the two are
    the same warp far inside the 1e-9 px the GPU test allows."""
    z = np.load(GOLDEN)
    for k in range(3):
        ev, flow = _case(z, k, torch.float64)
        for j, t0 in enumerate(z[f"t0_{k}"]):
            t0 = float(ev[-1, 0]) if np.isnan(t0) else float(t0)
            xw, yw = warp_direct(ev, flow, t0)
            assert (xw - torch.from_numpy(z[f"xw_{k}_{j}_f64"])).abs().max() < 1e-11
            assert (yw - torch.from_numpy(z[f"yw_{k}_{j}_f64"])).abs().max() < 1e-11


def test_restated_accumulation_on_cases_with_known_answers():
    # integer positions: the per-polarity count image, exactly
    xw = torch.tensor([3.0, 3.0, 0.0, 9.0, 9.0], dtype=torch.float64)
    yw = torch.tensor([2.0, 2.0, 0.0, 4.0, 4.0], dtype=torch.float64)
    p = torch.tensor([1.0, -1.0, 1.0, 0.0, 1.0], dtype=torch.float64)
    img, dropped = accumulate(xw, yw, p, 5, 10)
    assert dropped == 0 and img.sum() == 5.0
    assert img[0, 2, 3] == 1 and img[1, 2, 3] == 1 and img[0, 0, 0] == 1 and img[1, 4, 9] == 1 and img[0, 4, 9] == 1
    # a fractional position splits into four votes; targets outside the frame are dropped one by one, without wrapping
    img, dropped = accumulate(torch.tensor([9.25, -0.5, float("nan")], dtype=torch.float64), torch.tensor([1.5, 0.0, 1.0], dtype=torch.float64),
                              torch.ones(3, dtype=torch.float64), 5, 10)
    assert dropped == 1
    assert img[0, 1, 9] == 0.375 and img[0, 2, 9] == 0.375 and img[0, 0, 0] == 0.5
    assert img.sum() == 1.25 and img[0, 2, 0] == 0 and img[0, 3, 0] == 0              # nothing wrapped into the next row


def test_restated_fwl_tells_the_right_flow_from_the_wrong_one():
    """Points moving with a constant flow: warping along it stacks each point's events on one cell (FWL > 1), against it smears them."""
    rng = np.random.default_rng(3)
    pts = rng.choice(40 * 70, 60, replace=False)
    px, py = (pts % 70 + 12).astype(np.float64), (pts // 70 + 12).astype(np.float64)
    ts = np.arange(16) / 15.0
    ev = np.stack([np.repeat(ts, 60), np.tile(px, 16) + 7.0 * np.repeat(ts, 60), np.tile(py, 16) - 3.0 * np.repeat(ts, 60),
                   np.ones(16 * 60)], axis=1)
    ev = torch.from_numpy(ev)
    flow = torch.tensor([7.0, -3.0]).view(2, 1, 1).expand(2, 64, 96).contiguous()
    img, m = iwe_reference(ev, flow, 64, 96, t_ref="start")
    assert m[0] == 64 * 96 and m[3] == 0 and abs(m[1] - 960) < 1e-6
    assert (img[0, py.astype(int), px.astype(int)] - 16).abs().max() < 1e-6
    assert fwl_reference(ev, flow) > 1 > fwl_reference(ev, -flow)
    assert metric_refs(ev, "end") == (1.0, -1.0) and metric_refs(ev, "start") == (0.0, -1.0)
    assert metric_refs(ev[:1], "end") == (0.0, -1.0)                     # T = 0 counts as 1
    assert math.isnan(fwl_reference(ev[:0], flow))                       # no events: a constant count image


def test_abi_is_declared_with_its_replaces_lines():
    header = open(os.path.join(HERE, "..", "include", "eemflow_hip.h")).read()
    for name in ("eemflow_warp_events", "eemflow_iwe_many"):
        assert name in _lib.EXPORTS
        at = header.index(name + "(")
        comment = header[header.rindex("/*", 0, at):at]
        assert "Replaces:" in comment and "utils_luo/event_utils.py:9-51" in comment and "test_mvsec.py:753-852" in comment
    from eemflow_amd.build import EXTRA, SOURCES
    assert "iwe.hip" in SOURCES and "-ffp-contract=off" in EXTRA["iwe.hip"]


def test_package_exports_the_entry_points():
    for name in ("warp_events", "iwe", "iwe_many", "fwl", "fwl_many"):
        assert getattr(eemflow_amd, name) is getattr(iwe, name)


def test_cpu_tensors_raise():
    ev, flow = torch.zeros(5, 4, dtype=torch.float64), torch.zeros(2, 8, 8)
    for call in (lambda: iwe.warp_events(ev, flow), lambda: iwe.iwe(ev, flow), lambda: iwe.iwe_many([ev], [None], size=(8, 8)),
                 lambda: iwe.fwl(ev, flow), lambda: iwe.fwl_many([ev, ev], [flow, flow])):
        with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
            call()


def test_argument_validation():
    ev, flow = torch.zeros(5, 4, dtype=torch.float64), torch.zeros(2, 8, 8)

    class Cuda(torch.Tensor):
        """A CPU tensor that says it is on the GPU: the shape and dtype checks run without one."""
        is_cuda = True

    def cuda(t):
        return t.as_subclass(Cuda)
    with pytest.raises(ValueError, match=r"\(N,4\) float64"):
        iwe.iwe(cuda(ev.float()), cuda(flow))
    with pytest.raises(ValueError, match=r"\(N,4\) float64"):
        iwe.warp_events(cuda(torch.zeros(5, 3, dtype=torch.float64)), cuda(flow))
    with pytest.raises(ValueError, match=r"\(2,H,W\) float32"):
        iwe.iwe(cuda(ev), cuda(flow.double()))
    with pytest.raises(ValueError, match=r"\(2,H,W\) float32"):
        iwe.fwl(cuda(ev), cuda(torch.zeros(1, 2, 8, 8)))
    with pytest.raises(ValueError, match="one .2,H,W. shape"):
        iwe.iwe_many([cuda(ev), cuda(ev)], [cuda(flow), cuda(torch.zeros(2, 8, 9))])
    with pytest.raises(ValueError, match="one flow"):
        iwe.iwe_many([cuda(ev), cuda(ev)], [cuda(flow)])
    with pytest.raises(ValueError, match="size="):
        iwe.iwe_many([cuda(ev)], [None])
    with pytest.raises(ValueError, match="t_ref"):
        iwe.iwe(cuda(ev), cuda(flow), t_ref="middle")
    with pytest.raises(ValueError, match="offset"):
        iwe.iwe(cuda(ev), cuda(flow), offset=3)
    with pytest.raises(ValueError, match="needs its flow"):
        iwe.fwl_many([cuda(ev)], [None])
    with pytest.raises(TypeError):
        iwe.iwe(np.zeros((5, 4)), cuda(flow))


def test_parser_takes_fwl():
    from eemflow_amd import cli
    assert cli.build_parser().parse_args(["test"]).fwl is False
    args = cli.build_parser().parse_args(["test", "--fwl", "--stream", "8", "--fb_check", "0.01", "0.5"])
    assert args.fwl is True and args.stream == 8
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["train", "--fwl"])


class _NoEvents:
    consecutive_windows = True

    def __len__(self):
        return 3

    def get_windows(self, first, count):
        return [], []


def test_fwl_without_events_raises():
    tester = TestRaftEvents(_NoEvents(), (256, 256), logger=Logger(verbose=False))
    for extra in ({}, {"stream": 4}):
        with pytest.raises(ValueError, match="with_events"):
            tester.test_multi_sequence(torch.nn.Identity(), sequence_list=("a",), stride=1, fwl=True, **extra)


def test_datasets_take_with_events(tmp_path):
    import inspect
    from eemflow_amd.hrem import HREMEventFlow
    from eemflow_amd.mvsec import MvsecEventFlow, MvsecEventFlow_dt4
    for cls in (MvsecEventFlow, MvsecEventFlow_dt4, HREMEventFlow):
        assert inspect.signature(cls.__init__).parameters["with_events"].default is False
    (tmp_path / "dataset" / "MVSEC" / "seqA" / "flowgt_dt1").mkdir(parents=True)
    args = {"eval_type": "dense", "num_voxel_bins": 5, "sequence": "seqA"}
    for flag in (False, True):
        ds = MvsecEventFlow(args, train=False, root=str(tmp_path), valid_time_index={"seqA": [(3, 6)]}, with_events=flag)
        assert ds.with_events is flag
    assert ds._crop_offset() == (45, 2)                                  # center_crop of 260 x 346 to 256 x 256: left 45, top 2
