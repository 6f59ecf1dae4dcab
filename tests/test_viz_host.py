"""Host-side checks of the visualisation: the CPU restatement (tests/viz_reference.py) against the fixture made from the reference's own
flow_to_image_dmax and vis_map_RGB (tests/golden/viz.npz, make_golden_viz.py), the ABI declarations, the JPEG writer and the command
line.  No GPU."""
import os
import threading

import numpy as np
import pytest
import torch

from eemflow_amd import _lib, cli
from eemflow_amd.viz import ImageWriter

import viz_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "viz.npz")


def test_restatement_equals_every_golden_flow_image():
    z = np.load(GOLDEN)
    names = list(z["flow_names"])
    assert {"hand", "zero", "nan", "unknown", "smooth_37x50", "smooth_64x61", "smooth_260x346"} <= set(names)
    assert sum(n.startswith("rand") for n in names) == 40
    for n in names:
        flow, want = z[f"flow_{n}"], z[f"flow_image_{n}"]
        assert flow.dtype == np.float32 and want.dtype == np.uint8 and want.shape == flow.shape[1:] + (3,)
        assert np.array_equal(R.flow_image(flow), want), n
        assert np.array_equal(R.flow_image(flow, bgr=True), want[..., ::-1]), n


def test_fixture_carries_the_discontinuities():
    z = np.load(GOLDEN)
    hand, img = z["flow_hand"], z["flow_image_hand"]
    assert hand.shape == (2, 4, 6)
    # (3, +0.0) and (3, -0.0): the sign of a zero v picks the other end of the wheel
    assert hand[0].flat[4] == hand[0].flat[5] == 3 and not np.signbit(hand[1].flat[4]) and np.signbit(hand[1].flat[5])
    a, b = img.reshape(-1, 3)[4], img.reshape(-1, 3)[5]
    assert a[2] != b[2] and abs(int(a[2]) - int(b[2])) > 1
    # three pixels share the maximum radius 5
    rad = np.sqrt(hand[0].astype(np.float64) ** 2 + hand[1].astype(np.float64) ** 2).reshape(-1)
    assert rad.max() == 5 and int((rad == 5).sum()) == 3 and int((rad == 0).sum()) == 1
    assert np.all(img.reshape(-1, 3)[rad == 0] == 255)
    # an all-zero frame divides by 2^-52 and is white; a NaN frame divides by -1 + 2^-52
    assert np.all(z["flow_image_zero"] == 255)
    assert R.flow_divisor(z["flow_zero"]) == 2.0 ** -52
    assert R.flow_divisor(z["flow_nan"]) == -1.0 + 2.0 ** -52
    nan = np.isnan(z["flow_nan"]).any(0)
    assert nan.sum() == 1 and np.all(z["flow_image_nan"][nan] == 0) and z["flow_image_nan"][~nan].any()
    unk = (np.abs(z["flow_unknown"]) > 1e7).any(0)
    assert unk.sum() == 2 and np.all(z["flow_image_unknown"][unk] == 0)
    # among the random frames the maximum-radius pixel falls on both sides of rad <= 1 after the fp64 normalisation
    sides = set()
    for k in range(40):
        f = z[f"flow_rand{k:02d}"]
        d = R.flow_divisor(f)
        u, v = f[0].astype(np.float64) / d, f[1].astype(np.float64) / d
        sides.add(bool(np.sqrt(u * u + v * v).max() <= 1))
    assert sides == {True, False}
    assert str(z["numpy_version"])


def test_an_fp32_angle_stays_inside_the_gpu_rule():
    """The GPU rule (no byte off by more than 1, at most 1 % of a frame's bytes differ) has room for a less exact arctangent: the
    restatement with the angle alone in fp32 meets it on every larger golden frame."""
    z = np.load(GOLDEN)
    for n in ("smooth_37x50", "smooth_64x61", "smooth_260x346"):
        d = np.abs(R.flow_image(z[f"flow_{n}"], angle_dtype=np.float32).astype(int) - z[f"flow_image_{n}"].astype(int))
        assert d.max() <= 1 and (d != 0).mean() <= 0.01, n


def test_restatement_equals_every_golden_event_image():
    z = np.load(GOLDEN)
    names = list(z["event_names"])
    assert len(names) == 3 and sum(f"event_raw_{n}" in z for n in names) == 1
    for n in names:
        if f"event_raw_{n}" in z:
            args = (z[f"event_raw_{n}"], z[f"event_record_{n}"])
        else:
            args = (z[f"event_volume_{n}"],)
        assert args[0].shape[0] == 5
        img, count = R.event_image(*args)
        assert np.array_equal(img, z[f"event_image_{n}"]), n
        assert count == int(z[f"event_count_{n}"]) and 0 < count < args[0][0].size
        assert R.event_threshold_margin(*args) >= 1e-4, n     # summation order cannot decide a pixel
        colours = {tuple(c) for c in img.reshape(-1, 3)}
        assert colours == {(255, 255, 255), (255, 0, 0), (0, 0, 255)}


def test_golden_file_is_small():
    assert os.path.getsize(GOLDEN) < 1000000


def test_abi_is_declared_with_what_it_replaces():
    header = open(os.path.join(HERE, "..", "include", "eemflow_hip.h")).read()
    for name in ("eemflow_flow_to_image_many", "eemflow_event_image_many"):
        assert name in _lib.EXPORTS
        at = header.index(name + "(")
        comment = header[header.rindex("/*", 0, at):at]
        assert "Replaces:" in comment and comment.rstrip().endswith("int"), name
    from eemflow_amd import build
    assert "viz.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA["viz.hip"]


def smooth_image(h=48, w=64):
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([40 + 3 * x, 30 + 4 * y, 200 - 2 * x - y], axis=-1)      # three different, smooth channels
    return np.clip(img, 0, 255).astype(np.uint8)


def test_writer_writes_files_pil_reopens_in_the_reference_channel_order(tmp_path):
    from PIL import Image
    img = smooth_image()
    # the bound: what a JPEG round trip of this very array costs with PIL alone, at the writer's quality
    def round_trip_error(arr):
        probe = tmp_path / "probe.jpg"
        Image.fromarray(arr, "RGB").save(probe, format="JPEG", quality=95)
        return np.abs(np.asarray(Image.open(probe).convert("RGB")).astype(int) - arr.astype(int)).mean()
    bound = max(round_trip_error(img), round_trip_error(img[:, :, ::-1].copy()))       # (in either channel order: JPEG treats them alike)
    with ImageWriter(str(tmp_path / "out" / "test"), threads=2) as wr:
        wr.submit("1_flow_est.jpg", torch.from_numpy(img))
        wr.submit("1_flow_gt.jpg", torch.from_numpy(img[:, :, ::-1].copy()))
    assert sorted(os.listdir(tmp_path / "out" / "test")) == ["1_flow_est.jpg", "1_flow_gt.jpg"]
    assert sorted(wr.written) == ["1_flow_est.jpg", "1_flow_gt.jpg"]
    back = np.asarray(Image.open(tmp_path / "out" / "test" / "1_flow_est.jpg").convert("RGB"))
    assert back.shape == img.shape
    # cv2.imwrite reads the array it is given as BGR: the array's channel 0 is the file's blue
    err_swapped = np.abs(back[:, :, ::-1].astype(int) - img.astype(int)).mean()
    err_same = np.abs(back.astype(int) - img.astype(int)).mean()
    print(f"JPEG round trip: PIL alone {bound:.3f}, writer (file read as BGR) {err_swapped:.3f}, read as RGB {err_same:.3f}")
    assert err_swapped <= bound
    assert err_same > 10 * bound


def test_writer_blocks_at_max_pending_and_drains(tmp_path):
    gate, started = threading.Event(), threading.Event()

    class Held(ImageWriter):
        def encode(self, path, array):
            started.set()
            gate.wait()
            super().encode(path, array)

    wr = Held(str(tmp_path), threads=1, max_pending=2)
    img = torch.from_numpy(smooth_image(8, 8))
    try:
        wr.submit("0.jpg", img)
        assert started.wait(30)                                # the worker holds image 0
        wr.submit("1.jpg", img)
        wr.submit("2.jpg", img)                                # max_pending images are queued now
        assert wr._queue.full()
        blocked = threading.Thread(target=wr.submit, args=("3.jpg", img), daemon=True)
        blocked.start()
        blocked.join(0.05)
        assert blocked.is_alive()                              # the fourth submit waits for room
        assert not os.listdir(tmp_path)
    finally:
        gate.set()
    blocked.join(30)
    assert not blocked.is_alive()
    wr.close()
    assert sorted(os.listdir(tmp_path)) == ["0.jpg", "1.jpg", "2.jpg", "3.jpg"]
    with pytest.raises(RuntimeError, match="close"):
        wr.submit("4.jpg", img)


def test_writer_reraises_the_first_worker_error_on_close(tmp_path):
    class Failing(ImageWriter):
        def encode(self, path, array):
            if path.endswith("bad.jpg"):
                raise OSError("disk full (test)")
            super().encode(path, array)

    wr = Failing(str(tmp_path), threads=1, max_pending=4)
    img = torch.from_numpy(smooth_image(8, 8))
    wr.submit("good.jpg", img)
    wr.submit("bad.jpg", img)
    for k in range(8):                                         # later submits do not hang behind a failed worker
        wr.submit(f"later{k}.jpg", img)
    with pytest.raises(OSError, match="disk full"):
        wr.close()
    assert "good.jpg" in os.listdir(tmp_path) and "bad.jpg" not in os.listdir(tmp_path)
    with pytest.raises(ValueError, match="uint8"):
        ImageWriter(str(tmp_path)).submit("x.jpg", torch.zeros(4, 4, 3))


def test_writer_without_pil_raises(tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL' (test)")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(RuntimeError, match="PIL"):
        ImageWriter(str(tmp_path))


def test_conversions_refuse_cpu_tensors():
    import eemflow_amd
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        eemflow_amd.flow_to_image(torch.zeros(1, 2, 8, 8))
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        eemflow_amd.flow_to_image_many([torch.zeros(1, 2, 8, 8)])
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        eemflow_amd.event_image(torch.zeros(1, 5, 8, 8))
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        eemflow_amd.event_image_many([torch.zeros(1, 5, 8, 8)])


def test_cli_parses_the_visualisation_flags():
    parser = cli.build_parser()
    args = parser.parse_args(["test", "-v", "--vis_events", "--print_epe", "--visualize_every", "5"])
    assert args.visualize and args.vis_events and args.print_epe and args.visualize_every == 5
    args = parser.parse_args(["test"])
    assert not args.visualize and not args.vis_events and not args.print_epe and args.visualize_every == 1
    sub = next(a for a in parser._actions if hasattr(a, "choices") and a.choices and "test" in a.choices)
    for name in ("train", "test"):
        text = sub.choices[name].format_help()
        assert "not built" not in text and "--visualize" in text
    assert "--vis_events" in sub.choices["test"].format_help() and "--vis_events" not in sub.choices["train"].format_help()
    assert "Dropped: visualisation" not in cli.__doc__.replace("\n", " ")
    with pytest.raises(SystemExit, match="qualify"):
        cli.test(parser.parse_args(["test", "--vis_events"]))


def test_harness_visualisation_argument_checks():
    from eemflow_amd.harness import Logger, TestRaftEvents
    tester = TestRaftEvents(None, (256, 256), logger=Logger(verbose=False))
    with pytest.raises(ValueError, match="save_path"):
        tester.test_multi_sequence(None, sequence_list=("a",), visualize_map=True)
    with pytest.raises(ValueError, match="visualize_map"):
        tester.test_multi_sequence(None, sequence_list=("a",), vis_events=True)
    with pytest.raises(ValueError, match="visualize_every"):
        tester.test_multi_sequence(None, sequence_list=("a",), visualize_map=True, save_path="x", visualize_every=0)
