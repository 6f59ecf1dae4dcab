"""Visualisation on the GPU (eemflow_amd.viz / eemflow_flow_to_image_many, eemflow_event_image_many) against the fixture made from the
reference's own flow_to_image_dmax and vis_map_RGB (tests/golden/viz.npz) and the CPU restatement tests/viz_reference.py.

The rule for a flow image: no byte differs from the reference by more than 1 and at most 1 % of a frame's bytes differ at all (the
device's fp64 arctangent is not the host's, bit for bit; a byte is a floor, so a last-bit difference may move it by one - the restatement
with an fp32 angle stays inside this rule with room, test_viz_host).  Frames smaller than 10x10 are equal exactly: they carry the
discontinuities (rad <= 1 at the maximum-radius pixel, the sign of a zero v, the divisor of an all-zero or NaN frame), where a wrong
decision moves a byte by far more than 1.  Event images are equal exactly (the fixture keeps every pixel 1e-4 away from a threshold).
Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import eemflow_amd
from eemflow_amd import EEMFlow, _lib, viz
from eemflow_amd.harness import Logger, TestRaftEvents
from eemflow_amd.weights import seeded_state_dict

import viz_reference as R
from test_gpu_harness_fb_check import dataset, sample_lines

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz.npz")


def gpu_flow(flow):
    """(2,H,W) float32 numpy -> the (1,2,H,W) device tensor the conversions take."""
    return torch.from_numpy(np.ascontiguousarray(flow))[None].to(DEV)


def check_flow_image(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8
    d = np.abs(got.astype(int) - want.astype(int))
    share = (d != 0).mean()
    print(f"{name} {want.shape}: max byte difference {d.max()}, bytes that differ {100 * share:.4f} %")
    if want.shape[0] < 10 and want.shape[1] < 10:
        assert d.max() == 0, f"{name}: a small frame must be equal exactly"
    assert d.max() <= 1 and share <= 0.01, name


def test_golden_flow_images():
    z = np.load(GOLDEN)
    for n in z["flow_names"]:
        img = eemflow_amd.flow_to_image(gpu_flow(z[f"flow_{n}"]))
        assert img.shape == (1,) + z[f"flow_image_{n}"].shape and img.dtype == torch.uint8 and img.is_cuda
        check_flow_image(str(n), img[0].cpu().numpy(), z[f"flow_image_{n}"])


def test_golden_event_images():
    z = np.load(GOLDEN)
    for n in z["event_names"]:
        if f"event_raw_{n}" in z:
            raw = torch.from_numpy(z[f"event_raw_{n}"])[None].to(DEV)
            img, density = eemflow_amd.event_image(raw, norm=torch.from_numpy(z[f"event_record_{n}"]).to(DEV))
        else:
            img, density = eemflow_amd.event_image(torch.from_numpy(z[f"event_volume_{n}"])[None].to(DEV))
        want = z[f"event_image_{n}"]
        assert img.dtype == torch.uint8 and density.dtype == torch.float64 and density.shape == (1,)
        assert np.array_equal(img[0].cpu().numpy(), want), n
        assert float(density[0]) * want.shape[0] * want.shape[1] == int(z[f"event_count_{n}"]), n
        assert float(density[0]) == int(z[f"event_count_{n}"]) / (want.shape[0] * want.shape[1])


def test_event_images_many_bgr_and_record_list():
    z = np.load(GOLDEN)
    vol = torch.from_numpy(z["event_volume_norm_37x50"])[None].to(DEV)
    imgs, dens = viz.event_image_many([vol.clone() for _ in range(17)], bgr=True)      # two library calls
    assert len(imgs) == 17 and dens.shape == (17,)
    want = z["event_image_norm_37x50"][..., ::-1]
    for im in imgs:
        assert np.array_equal(im.cpu().numpy(), want)
    assert torch.all(dens == dens[0]) and float(dens[0]) * 37 * 50 == int(z["event_count_norm_37x50"])
    # a raw grid with the voxelizer's record behind it, as the deferred-normalisation loader hands it over
    from eemflow_amd.voxelizer import _grid_buffers, norm_record
    raw = _grid_buffers(1, 5, 64, 61, torch.device(DEV), True)[0]
    raw.copy_(torch.from_numpy(z["event_raw_raw_64x61"]))
    norm_record(raw).copy_(torch.from_numpy(z["event_record_raw_64x61"]))
    imgs, dens = viz.event_image_many([raw[None]], [norm_record(raw)])
    assert np.array_equal(imgs[0].cpu().numpy(), z["event_image_raw_64x61"])


def test_every_frame_of_a_call_has_its_own_divisor():
    """Three frames of magnitudes 0.5, 7 and 300 and the NaN frame among sixteen, in one call: bitwise the single-frame calls."""
    z = np.load(GOLDEN)
    rng = np.random.default_rng(7)
    frames = [gpu_flow((rng.standard_normal((2, 8, 8)) * s).astype(np.float32)) for s in (0.5, 7.0, 300.0)]
    frames.append(gpu_flow(z["flow_nan"]))
    frames += [gpu_flow((rng.standard_normal((2, 8, 8)) * rng.uniform(0.1, 50)).astype(np.float32)) for _ in range(12)]
    assert len(frames) == 16
    many, divisors = viz.flow_to_image_many(frames, return_divisors=True)
    divisors = divisors.cpu().numpy()
    for i, f in enumerate(frames):
        single, d1 = viz.flow_to_image_many([f], return_divisors=True)
        assert torch.equal(many[i], single[0]), i
        assert divisors[i] == float(d1[0]) == R.flow_divisor(f[0].cpu().numpy()), i
        assert np.array_equal(many[i].cpu().numpy(), R.flow_image(f[0].cpu().numpy())), i      # (8x8: exact)
    assert divisors[3] == -1.0 + 2.0 ** -52 and divisors[0] < divisors[1] < divisors[2]
    # 17 frames: one call per 16
    imgs = viz.flow_to_image_many(frames + [frames[2]])
    assert len(imgs) == 17 and torch.equal(imgs[16], many[2]) and torch.equal(imgs[0], many[0])


def test_bgr_is_the_channel_flip():
    z = np.load(GOLDEN)
    for n in ("hand", "smooth_37x50", "smooth_64x61"):
        f = gpu_flow(z[f"flow_{n}"])
        assert torch.equal(eemflow_amd.flow_to_image(f, bgr=True), eemflow_amd.flow_to_image(f).flip(-1)), n


def test_large_frame_against_the_restatement():
    h, w = 720, 1280
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(3)
    flow = np.stack([30 * np.sin(2 * np.pi * x / w + 0.3) + 4, 18 * np.cos(2 * np.pi * y / h + 1.1) - 2]) + rng.standard_normal((2, h, w))
    flow = flow.astype(np.float32)
    flow[0, 100, 200] = np.inf                                       # an unknown pixel; no NaN: the maximum stays the frame's
    img = eemflow_amd.flow_to_image(gpu_flow(flow))
    check_flow_image("720x1280", img[0].cpu().numpy(), R.flow_image(flow))
    assert not img[0, 100, 200].any()


@pytest.mark.parametrize("h,w", [(5, 7), (3, 1), (3, 2), (1, 3), (9, 4)])
def test_layouts_with_partial_groups(h, w):
    """Plane sizes that are no multiple of 4 (one-pixel loads, a last partial group of byte stores), widths 1, 2 and 3, and an
    aligned plane read at an odd offset."""
    rng = np.random.default_rng(100 * h + w)
    flow = (rng.standard_normal((2, h, w)) * 4).astype(np.float32)
    canvas = torch.full((h * w * 3 + 64,), 77, dtype=torch.uint8, device=DEV)
    img = eemflow_amd.flow_to_image(gpu_flow(flow))
    assert np.array_equal(img[0].cpu().numpy(), R.flow_image(flow))                        # (smaller than 10x10: exact)
    vol = (rng.standard_normal((5, h, w)) * (rng.uniform(size=(5, h, w)) < 0.4)).astype(np.float32)
    assert R.event_threshold_margin(vol) > 1e-5
    ev, dens = eemflow_amd.event_image(torch.from_numpy(vol)[None].to(DEV))
    want, count = R.event_image(vol)
    assert np.array_equal(ev[0].cpu().numpy(), want) and float(dens[0]) == count / (h * w)
    # a flow that starts 4 bytes into its allocation and an image that starts at an odd byte: the unaligned forms, nothing written outside
    base = torch.zeros(2 * h * w + 1, device=DEV)
    base[1:].copy_(torch.from_numpy(flow).reshape(-1))
    arr = ctypes.c_void_p * 1
    stats = torch.empty(1, 4, dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().eemflow_flow_to_image_many(1, arr(base.data_ptr() + 4), arr(canvas.data_ptr() + 1), stats.data_ptr(), h, w, 0,
                                                     _lib.current_stream_ptr(torch.device(DEV))))
    out = canvas.cpu().numpy()
    assert np.array_equal(out[1:1 + h * w * 3].reshape(h, w, 3), R.flow_image(flow))
    assert out[0] == 77 and np.all(out[1 + h * w * 3:] == 77)


def test_errors():
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        eemflow_amd.flow_to_image(torch.zeros(1, 2, 8, 8))
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        eemflow_amd.event_image(torch.zeros(1, 5, 8, 8))
    with pytest.raises(ValueError, match="contiguous"):
        eemflow_amd.flow_to_image(torch.zeros(1, 2, 8, 16, device=DEV)[..., ::2])
    with pytest.raises(ValueError, match="contiguous"):
        viz.flow_to_image_many([torch.zeros(1, 8, 8, 2, device=DEV).permute(0, 3, 1, 2)])
    with pytest.raises(ValueError, match="contiguous"):
        eemflow_amd.event_image(torch.zeros(1, 5, 8, 16, device=DEV)[..., ::2])
    with pytest.raises(ValueError, match="shape"):
        viz.flow_to_image_many([torch.zeros(1, 2, 8, 8, device=DEV), torch.zeros(1, 2, 8, 9, device=DEV)])
    L = _lib.lib()
    f, im = torch.zeros(2, 8, 8, device=DEV), torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    stats = torch.zeros(16, 4, dtype=torch.float64, device=DEV)
    arr = ctypes.c_void_p * 17
    af, ai, sp = arr(*[f.data_ptr()] * 17), arr(*[im.data_ptr()] * 17), _lib.current_stream_ptr(torch.device(DEV))
    assert L.eemflow_flow_to_image_many(17, af, ai, stats.data_ptr(), 8, 8, 0, sp) != 0
    assert L.eemflow_flow_to_image_many(0, af, ai, stats.data_ptr(), 8, 8, 0, sp) != 0
    assert L.eemflow_flow_to_image_many(1, af, ai, None, 8, 8, 0, sp) != 0
    assert L.eemflow_flow_to_image_many(1, af, ai, stats.data_ptr(), 0, 8, 0, sp) != 0
    assert L.eemflow_event_image_many(17, af, None, 2, 8, 4, ai, stats.data_ptr(), 0, sp) != 0
    assert L.eemflow_event_image_many(1, af, None, 0, 8, 8, ai, stats.data_ptr(), 0, sp) != 0
    assert L.eemflow_event_image_many(1, af, (ctypes.c_void_p * 1)(None), 2, 8, 4, ai, stats.data_ptr(), 0, sp) != 0
    assert L.eemflow_flow_to_image_many(1, af, ai, stats.data_ptr(), 8, 8, 0, sp) == 0
    assert L.eemflow_event_image_many(1, af, None, 2, 8, 8, ai, stats.data_ptr(), 0, sp) == 0
    torch.cuda.synchronize()


def test_writer_takes_device_images(tmp_path):
    from PIL import Image
    z = np.load(GOLDEN)
    img = eemflow_amd.flow_to_image(gpu_flow(z["flow_smooth_64x61"]))[0]
    with viz.ImageWriter(str(tmp_path), threads=2, max_pending=4) as wr:
        for k in range(10):                                          # more than max_pending: submit waits for the encoders
            wr.submit(f"{k}.jpg", img)
    direct = tmp_path / "direct.jpg"
    wr.encode(str(direct), img.cpu().numpy())
    want = np.asarray(Image.open(direct))
    for k in range(10):
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"{k}.jpg")), want)


# ------------------------------------------------------------------------------------------------ the evaluation loop
def evaluate_twice(tmp_path, capsys, monkeypatch, loop):
    """The tiny MVSEC sequence through one loop of test_multi_sequence, without and with the visualisation keywords: the same lines,
    nothing written without them, exactly the reference's file names with them.  Returns what the file checks need."""
    monkeypatch.setenv("EEM_WINO4_LAYERS", "7")              # one encoder form whatever the call's batch (as test_gpu_stream pins it)
    monkeypatch.setenv("EEM_DEC_WNC", "1")
    ds = dataset(tmp_path, "dense", n_samples=5)
    sd = seeded_state_dict(68)
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV)
    tester = TestRaftEvents(ds, (256, 256), logger=Logger(verbose=False))
    capsys.readouterr()
    save = tmp_path / "out"
    plain = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, **loop)
    plain_text = capsys.readouterr().out
    assert not save.exists()                                 # without the keywords nothing is written
    got = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, visualize_map=True, vis_events=True, print_epe=True,
                                     visualize_every=2, save_path=str(save), **loop)
    text = capsys.readouterr().out
    assert got == plain and text == plain_text               # identical lines
    lines = sample_lines(text)
    assert len(lines) == 5
    folder = save / "seqA" / "test"
    files = sorted(os.listdir(folder))
    est_names = {}
    for idx in (0, 2, 4):                                    # every second sample; the file carries the line's number and AEE
        est_names[idx] = f"{idx + 1}_flow_est_{float(lines[idx].group(2)):.3f}.jpg"
    assert sorted([f for f in files if "_flow_" in f]) == sorted(list(est_names.values()) + [f"{i + 1}_flow_gt.jpg" for i in (0, 2, 4)])
    event_files = [f for f in files if "_events" in f]
    assert len(event_files) == 6 and len(files) == 12
    for idx in (0, 2, 4):
        for j in (1, 2):
            assert sum(bool(re.fullmatch(rf"{idx + 1}_events{j}_0\.\d{{3}}\.jpg", f)) for f in event_files) == 1
    return ds, net, folder, est_names, event_files


def assert_file_is_the_encoding_of(path, image, tmp_path):
    """The file decodes to what the writer's own encoding of `image` ((H,W,3) uint8 device tensor) decodes to."""
    from PIL import Image
    wr = viz.ImageWriter(str(tmp_path / "again"))
    wr.close()
    again = str(tmp_path / "again" / os.path.basename(path))
    wr.encode(again, image.cpu().numpy())
    have = np.asarray(Image.open(path))
    assert have.shape == tuple(image.shape)
    assert np.array_equal(have, np.asarray(Image.open(again))), os.path.basename(path)


def test_harness_one_sample_loop_writes_the_reference_files(tmp_path, capsys, monkeypatch):
    ds, net, folder, est_names, event_files = evaluate_twice(tmp_path, capsys, monkeypatch, {})
    for idx in (0, 2, 4):
        sample = ds[idx]
        e1, e2 = sample['event_volume_old'].to(DEV)[None].float(), sample['event_volume_new'].to(DEV)[None].float()
        with torch.no_grad():
            _, preds = net(events1=e1, events2=e2)
        assert_file_is_the_encoding_of(folder / est_names[idx], eemflow_amd.flow_to_image(preds[-1].contiguous())[0], tmp_path)
        assert_file_is_the_encoding_of(folder / f"{idx + 1}_flow_gt.jpg",
                                       eemflow_amd.flow_to_image(sample['flow'].to(DEV)[None].float().contiguous())[0], tmp_path)
        for j, vol in ((1, e1), (2, e2)):
            img, dens = eemflow_amd.event_image(vol.contiguous())
            name = f"{idx + 1}_events{j}_{float(dens[0]):.3f}.jpg"
            assert name in event_files
            assert_file_is_the_encoding_of(folder / name, img[0], tmp_path)


def test_harness_stream_loop_writes_the_reference_files(tmp_path, capsys, monkeypatch):
    from eemflow_amd.harness import stream_chunks
    ds, net, folder, est_names, event_files = evaluate_twice(tmp_path, capsys, monkeypatch, {"stream": 4})
    ds.change_test_sequence("seqA")
    seen = 0
    with torch.no_grad():
        for chunk, targets, flows, volumes in stream_chunks(ds, net, 4, torch.device(DEV), with_volumes=True):
            for i, idx in enumerate(chunk):
                if idx % 2:
                    continue
                seen += 1
                assert_file_is_the_encoding_of(folder / est_names[idx], eemflow_amd.flow_to_image(flows[i].contiguous())[0], tmp_path)
                assert_file_is_the_encoding_of(folder / f"{idx + 1}_flow_gt.jpg",
                                               eemflow_amd.flow_to_image(targets[i]['flow'].to(DEV)[None].float().contiguous())[0], tmp_path)
                for j in (1, 2):
                    img, dens = eemflow_amd.event_image(volumes[i][j - 1].contiguous())
                    name = f"{idx + 1}_events{j}_{float(dens[0]):.3f}.jpg"
                    assert name in event_files
                    assert_file_is_the_encoding_of(folder / name, img[0], tmp_path)
    assert seen == 3


def test_harness_frames_in_flight_loop_writes_the_same_names(tmp_path, capsys, monkeypatch):
    ds, net, folder, est_names, event_files = evaluate_twice(tmp_path, capsys, monkeypatch, {"frames_in_flight": 2})
    for idx in (0, 2, 4):                                    # (the ground truth does not depend on the replica's kernel forms)
        assert_file_is_the_encoding_of(folder / f"{idx + 1}_flow_gt.jpg",
                                       eemflow_amd.flow_to_image(ds[idx]['flow'].to(DEV)[None].float().contiguous())[0], tmp_path)


def test_harness_coalesced_loop_visualises_raw_volumes(tmp_path, capsys):
    """coalesce=2 on deferred-normalisation HREM samples: the event images come from the RAW volumes and their records."""
    from eemflow_amd import hrem
    from eemflow_amd.voxelizer import norm_record
    root = str(tmp_path)
    for i in range(3):
        d = os.path.join(root, "dataset/HREM/test/dt1/seqV/%06d" % (i + 1))
        os.makedirs(d)
        hrem.write_events_npz(os.path.join(d, "events1.npz"), hrem.synthetic_hrem_events(140 + i, 30000, 720, 1280))
        hrem.write_events_npz(os.path.join(d, "events2.npz"), hrem.synthetic_hrem_events(160 + i, 30000, 720, 1280))
        hrem.write_flo(os.path.join(d, "flow.flo"), hrem.synthetic_flow(180 + i, 720, 1280))
    net = EEMFlow("", 5, 5)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(5).items()})
    net = net.to(DEV)
    ds = hrem.HREMEventFlow({"eval_type": "dense", "event_interval": "dt1", "num_voxel_bins": 5}, train=False, root=root, deferred_norm=True)
    tester = TestRaftEvents(ds, (720, 1280), logger=Logger(verbose=False))
    save = tmp_path / "out"
    tester.test_multi_sequence(net, sequence_list=["seqV"], stride=1, coalesce=2, visualize_map=True, vis_events=True, save_path=str(save))
    capsys.readouterr()
    files = sorted(os.listdir(save / "seqV" / "test"))
    assert len(files) == 12 and [f for f in files if "_flow_" in f] == sorted(
        [f"{i}_flow_est.jpg" for i in (1, 2, 3)] + [f"{i}_flow_gt.jpg" for i in (1, 2, 3)])
    ds.change_test_sequence("seqV")
    sample = ds.get_samples([1])[0]
    assert sample["deferred_norm"]
    for j, key in ((1, 'event_volume_old'), (2, 'event_volume_new')):
        raw = sample[key]
        img, dens = eemflow_amd.event_image(raw[None], norm=norm_record(raw))
        name = f"2_events{j}_{float(dens[0]):.3f}.jpg"
        assert name in files
        assert_file_is_the_encoding_of(save / "seqV" / "test" / name, img[0], tmp_path)
