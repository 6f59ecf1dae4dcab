"""Host-side checks of the bidirectional stream and the forward-backward consistency check: the CPU restatement (tests/fb_reference.py)
against the fixture made from the reference's own occ_check_model (tests/golden/fb_check.npz, make_golden_fb.py), and the argument
checks of EEMFlow.forward_stream(bidirectional=, fb_check=), eemflow_amd.fb_check and the harness hook.  No GPU."""
import os

import numpy as np
import pytest
import torch

import eemflow_amd
from eemflow_amd import _lib
from eemflow_amd.eemflow import EEMFlow
from eemflow_amd.harness import Logger, TestRaftEvents, stream_chunks

from fb_reference import MODES, fb_check_margins, fb_check_reference, synthetic_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fb_check.npz")


def _module():
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.change_imagesize((64, 64))
    return net


def test_restatement_reproduces_every_fixture_mask():
    z = np.load(GOLDEN)
    assert tuple(z["modes"]) == MODES and int(z["npairs"]) >= 2
    values = set()
    for k in range(int(z["npairs"])):
        fw, bw = torch.from_numpy(z[f"fw_{k}"]), torch.from_numpy(z[f"bw_{k}"])
        assert fw.shape[-1] <= 64 and fw.shape[-2] <= 64
        for ai, (a1, a2) in enumerate(z["alphas"]):
            for mode in MODES:
                mf, mb = fb_check_reference(fw, bw, float(a1), float(a2), mode)
                assert mf.shape == (1, 1) + fw.shape[2:] and mf.dtype == torch.float32
                assert np.array_equal(mf.numpy().astype(np.uint8), z[f"mask_fw_{k}_{ai}_{mode}"]), (k, ai, mode)
                assert np.array_equal(mb.numpy().astype(np.uint8), z[f"mask_bw_{k}_{ai}_{mode}"]), (k, ai, mode)
                values |= set(np.unique(z[f"mask_fw_{k}_{ai}_{mode}"]).tolist())
    assert values == {0, 1}


def test_fixture_has_targets_leaving_the_frame_and_both_settings():
    z = np.load(GOLDEN)
    assert z["alphas"].tolist() == [[1.0, 0.05], [0.01, 0.5]]
    for k in range(int(z["npairs"])):
        out = z[f"mask_fw_{k}_0_out"]
        assert 0 < out.mean() < 1                            # some targets leave the frame, some stay
        # 'obj' is 'all' with the leaving pixels forced to 1
        assert np.array_equal(z[f"mask_fw_{k}_1_obj"], np.maximum(z[f"mask_fw_{k}_1_all"], 1 - out))


def test_fp64_restatement_is_far_from_the_margin_on_the_synthetic_pair():
    """The small synthetic pair of the GPU test: few borderline pixels, both mask values present (what that test asserts before it
    compares), and the fp32 restatement agrees with the fp64 one outside the margin."""
    fw, bw = synthetic_pair(260, 346)
    m64 = fb_check_reference(fw.double(), bw.double(), 0.01, 0.5)
    m32 = fb_check_reference(fw, bw, 0.01, 0.5)
    for m, a, g in zip(m64, m32, fb_check_margins(fw, bw, 0.01, 0.5)):
        near = g < 1e-3
        assert near.double().mean() <= 0.005
        assert 0.05 <= m.mean() <= 0.95
        assert torch.equal(m[~near], a.double()[~near])


def test_bidirectional_stream_takes_at_most_eight_volumes():
    net = _module()
    with pytest.raises(ValueError, match="1..8"):
        net.forward_stream([torch.zeros(1, 5, 64, 64)] * 9, bidirectional=True)
    with pytest.raises(ValueError, match="1..8"):
        net.forward_stream([torch.zeros(1, 5, 64, 64)] * 16, bidirectional=True)
    assert EEMFlow.MAX_STREAM_BIDIR == 8 and EEMFlow.MAX_STREAM == 16


def test_fb_check_needs_bidirectional():
    net = _module()
    with pytest.raises(ValueError, match="bidirectional"):
        net.forward_stream([torch.zeros(1, 5, 64, 64)] * 2, fb_check=(1.0, 0.05))
    with pytest.raises(ValueError, match="obj_out_all"):
        net.forward_stream([torch.zeros(1, 5, 64, 64)] * 2, bidirectional=True, fb_check=(1.0, 0.05, "some"))


def test_bidirectional_stream_refuses_cpu_tensors():
    net = _module()
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        net.forward_stream([torch.zeros(1, 5, 64, 64)] * 2, bidirectional=True, fb_check=(1.0, 0.05, "obj"))


def test_fb_check_refuses_cpu_tensors_and_bad_shapes():
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        eemflow_amd.fb_check(torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8))
    from eemflow_amd.metrics import fb_check_args, fb_check_many
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        fb_check_many([torch.zeros(1, 2, 8, 8)], [torch.zeros(1, 2, 8, 8)])
    assert fb_check_args() == (1.0, 0.05, "all")            # the reference's constructor defaults
    with pytest.raises(ValueError):
        fb_check_args(1.0, 0.05, "inside")


def test_abi_is_declared():
    for name in ("eemflow_forward_stream_bidir", "eemflow_fb_check_many"):
        assert name in _lib.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "eemflow_hip.h")).read()
    assert "#define EEM_STREAM_BIDIR_MAX_VOLUMES 8" in header
    assert "eemflow_forward_stream_bidir(" in header and "eemflow_fb_check_many(" in header


class _FakeBidir(torch.nn.Module):
    """forward_stream on CPU tensors: flows and masks carry the ids of their windows."""
    MAX_STREAM_BIDIR = 8

    def __init__(self):
        super().__init__()
        self.prev, self.calls = None, []

    def reset_stream(self):
        self.prev = None

    def forward_stream(self, volumes, bidirectional=False, fb_check=None):
        vols = list(volumes)
        self.calls.append((len(vols), bidirectional, fb_check))
        seq = ([self.prev] if self.prev is not None else []) + vols
        self.prev = vols[-1]
        ids = [(a.flatten()[0], b.flatten()[0]) for a, b in zip(seq[:-1], seq[1:])]
        return [((seq[i], seq[i + 1]), [torch.stack([a, b])], [torch.stack([b, a])], (a + 100, b + 100)) for i, (a, b) in enumerate(ids)]


class _FakeWindows:
    consecutive_windows = True

    def __init__(self, n_samples):
        self.n = n_samples

    def __len__(self):
        return self.n

    def get_windows(self, first, count):
        return [torch.full((5, 4, 4), float(j)) for j in range(first, first + count)], [{'idx': j} for j in range(first, first + count)]


def test_stream_chunks_runs_bidirectionally_with_fb_check():
    ds, model = _FakeWindows(21), _FakeBidir()
    seen = []
    for idx, targets, flows, masks in stream_chunks(ds, model, 16, torch.device("cpu"), fb_check=(0.01, 0.5)):
        for i, t, f, m in zip(idx, targets, flows, masks):
            assert t['idx'] == i and f.tolist() == [float(i), float(i + 1)] and float(m) == 100.0 + i     # the forward flow, its mask
        seen += idx
    assert seen == list(range(21))
    assert all(c[0] <= 8 and c[1] is True and c[2] == (0.01, 0.5) for c in model.calls)    # the bidirectional call's volume limit


def test_harness_fb_check_argument_checks():
    tester = TestRaftEvents(_FakeWindows(3), (256, 256), logger=Logger(verbose=False))
    with pytest.raises(ValueError, match="stream"):
        tester.test_multi_sequence(_module(), sequence_list=("a",), stride=1, fb_check=(0.01, 0.5))

    class _NoBidir(torch.nn.Module):
        def forward_stream(self, volumes):
            return []
    with pytest.raises(ValueError, match="bidirectional"):
        tester.test_multi_sequence(_NoBidir(), sequence_list=("a",), stride=1, stream=8, fb_check=(0.01, 0.5))


def test_cli_fb_check_requires_stream():
    from eemflow_amd import cli
    args = cli.build_parser().parse_args(["test", "--fb_check", "0.01", "0.5"])
    assert args.fb_check == [0.01, 0.5] and args.stream == 0
    with pytest.raises(SystemExit, match="--stream"):
        cli.test(args)
    args = cli.build_parser().parse_args(["test", "--stream", "8", "--fb_check", "0.01", "0.5"])
    assert args.stream == 8
