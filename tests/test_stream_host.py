"""Host-side checks of the streaming inference path (EEMFlow.forward_stream, TestRaftEvents.test_multi_sequence(stream=n)): no GPU."""
import pytest
import torch

from eemflow_amd import _lib
from eemflow_amd.eemflow import EEMFlow
from eemflow_amd.harness import Logger, TestRaftEvents, stream_chunks, stream_plan
from eemflow_amd.hrem import HREMEventFlow
from eemflow_amd.mvsec import MvsecEventFlow, MvsecEventFlow_dt4


def _module():
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.change_imagesize((64, 64))
    return net


def test_forward_stream_refuses_cpu_tensors():
    net = _module()
    with pytest.raises(_lib.EEMFlowHipError, match="CUDA"):
        net.forward_stream([torch.zeros(1, 5, 64, 64), torch.zeros(1, 5, 64, 64)])


def test_forward_stream_volume_count():
    net = _module()
    with pytest.raises(ValueError, match="1..16"):
        net.forward_stream([])
    with pytest.raises(ValueError, match="1..16"):
        net.forward_stream([torch.zeros(1, 5, 8, 8)] * 17)


def test_reset_stream_without_context():
    net = _module()
    net.reset_stream()                                   # nothing carried, no context yet: a no-op
    net.change_imagesize((32, 32))                       # a new size resets (no context to tell either)
    assert net._stream_prev is None


class _FakeModel(torch.nn.Module):
    """forward_stream on CPU tensors: flow p = the ids of its two windows (each volume holds its window id)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.prev, self.calls, self.resets = None, [], 0

    def reset_stream(self):
        self.prev, self.resets = None, self.resets + 1

    def forward_stream(self, volumes):
        vols = list(volumes)
        self.calls.append(len(vols))
        seq = ([self.prev] if self.prev is not None else []) + vols
        self.prev = vols[-1]
        return [((a, b), [torch.stack([a.flatten()[0], b.flatten()[0]])]) for a, b in zip(seq[:-1], seq[1:])]


class _FakeWindows:
    consecutive_windows = True

    def __init__(self, n_samples):
        self.n, self.read = n_samples, []

    def __len__(self):
        return self.n

    def get_windows(self, first, count):
        self.read += list(range(first, first + count))
        vols = [torch.full((5, 4, 4), float(j)) for j in range(first, first + count)]
        return vols, [{'idx': j} if j < self.n else None for j in range(first, first + count)]


@pytest.mark.parametrize("n_samples", [1, 2, 9, 10, 11, 25, 31])
@pytest.mark.parametrize("n", [2, 3, 10, 16])
def test_stream_plan_covers_every_sample_once(n_samples, n):
    ds, model = _FakeWindows(n_samples), _FakeModel()
    seen = []
    for idx, targets, flows in stream_chunks(ds, model, n, torch.device("cpu")):
        assert len(idx) == len(targets) == len(flows) >= 1
        for i, t, f in zip(idx, targets, flows):
            assert t['idx'] == i                                         # the target of sample i ...
            assert f.tolist() == [float(i), float(i + 1)]                # ... meets the flow of windows i and i + 1
        seen += idx
    assert seen == list(range(n_samples))
    assert ds.read == list(range(n_samples + 1))                        # every window read once, in order
    assert max(model.calls) <= n and model.resets == 1
    plan = stream_plan(n_samples, n)
    assert sum(p[1] for p in plan) == n_samples + 1 and sum(p[3] for p in plan) == n_samples


def test_stream_plan_empty_sequence():
    assert stream_plan(0, 10) == []


def _tester(dataset):
    return TestRaftEvents(dataset, (256, 256), logger=Logger(verbose=False))


def test_stream_refuses_hrem_dataset():
    ds = HREMEventFlow.__new__(HREMEventFlow)          # (no files needed: the refusal comes before any sample is read)
    with pytest.raises(ValueError, match="HREM"):
        _tester(ds).test_multi_sequence(_module(), sequence_list=("a",), stride=1, stream=10)


def test_stream_refuses_stride():
    ds = MvsecEventFlow.__new__(MvsecEventFlow)
    with pytest.raises(ValueError, match="stride == 1"):
        _tester(ds).test_multi_sequence(_module(), sequence_list=("a",), stride=10, stream=10)


def test_mvsec_declares_consecutive_windows():
    assert MvsecEventFlow.consecutive_windows and MvsecEventFlow_dt4.consecutive_windows
    assert not getattr(HREMEventFlow, "consecutive_windows", False)


def test_stream_abi_is_declared():
    for name in ("eemflow_forward_stream", "eemflow_stream_reset", "eemflow_stream_pending"):
        assert name in _lib.EXPORTS
