"""Host-side checks of EEMFlow+'s streaming inference (EEMFlow_cdc.forward_stream, TestRaftEvents.test_multi_sequence(stream=n) on an
EEMFlow_cdc): no GPU."""
import os
import re

import pytest
import torch

from eemflow_amd import _lib
from eemflow_amd.eemflow_plus import EEMFlow_cdc
from eemflow_amd.harness import Logger, TestRaftEvents, stream_chunks
from eemflow_amd.hrem import HREMEventFlow
from eemflow_amd.mvsec import MvsecEventFlow


def _module():
    net = EEMFlow_cdc("", 3, 5).eval()
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


def test_forward_stream_refuses_mixed_shapes():
    net = _module()

    class _Cuda(torch.Tensor):                           # (CPU tensors that pass the device check: the shape checks come after it)
        is_cuda = True
    a = torch.zeros(1, 5, 64, 64).as_subclass(_Cuda)
    b = torch.zeros(1, 5, 32, 64).as_subclass(_Cuda)
    with pytest.raises(ValueError, match="one shape"):
        net.forward_stream([a, b])
    with pytest.raises(ValueError, match=r"\(1,5,H,W\)"):
        net.forward_stream([torch.zeros(2, 5, 64, 64).as_subclass(_Cuda)])


def test_reset_stream_without_context():
    net = _module()
    net.reset_stream()                                   # nothing carried, no context yet: a no-op
    net._stream_prev = torch.zeros(1)                    # (as a stream call leaves it)
    net.change_imagesize((64, 64))                       # the same size keeps the carry ...
    assert net._stream_prev is not None
    net.change_imagesize((32, 32))                       # ... a new size resets (no context to tell either)
    assert net._stream_prev is None


def test_replica_starts_without_carry():
    net = _module()
    net._stream_prev = torch.zeros(1)
    twin = net.replicate()
    assert twin._stream_prev is None and twin._ctx is None


def test_stream_abi_is_declared():
    for name in ("eemplus_forward_stream", "eemplus_stream_reset", "eemplus_stream_pending"):
        assert name in _lib.EXPORTS


class _Windows:
    """A stride-1 MVSEC-like sequence (consecutive_windows, get_windows) of n_samples samples on the CPU."""
    consecutive_windows = True

    def __init__(self, n_samples):
        self.n, self.read = n_samples, []

    def __len__(self):
        return self.n

    def change_test_sequence(self, name):
        pass

    def get_windows(self, first, count):
        self.read += list(range(first, first + count))
        vols = [torch.zeros(5, 64, 64) for _ in range(count)]
        return vols, [{'idx': j, 'flow': torch.zeros(2, 64, 64)} for j in range(first, first + count)]


def _tester(dataset):
    return TestRaftEvents(dataset, (64, 64), logger=Logger(verbose=False))


def test_stream_walk_accepts_eemflow_plus(monkeypatch):
    """test_multi_sequence(stream=n) takes an EEMFlow_cdc on a stride-1 MVSEC dataset: past the argument checks, the walk itself is
    entered with the stream setting (recorded here: the walk needs a GPU)."""
    seen = []
    monkeypatch.setattr(TestRaftEvents, "_test_multi_sequence", lambda self, model, *a: seen.append((model, a)) or 0.0)
    net = _module()
    ds = MvsecEventFlow.__new__(MvsecEventFlow)
    assert _tester(ds).test_multi_sequence(net, sequence_list=("a",), stride=1, stream=10) == 0.0
    assert len(seen) == 1 and seen[0][0] is net and seen[0][1][-1] == 10


def test_stream_chunks_reach_eemflow_plus_forward_stream():
    """The walk's first call hands its windows, read once, to EEMFlow_cdc.forward_stream (here CPU tensors, which forward_stream refuses
    for the device)."""
    ds = _Windows(5)
    with pytest.raises(_lib.EEMFlowHipError, match="EEMFlow_cdc.forward_stream.*CUDA"):
        next(stream_chunks(ds, _module(), 3, torch.device("cpu")))
    assert ds.read == [0, 1, 2]


def test_stream_refuses_hrem_dataset_for_eemflow_plus():
    ds = HREMEventFlow.__new__(HREMEventFlow)            # (no files needed: the refusal comes before any sample is read)
    with pytest.raises(ValueError, match="HREM"):
        _tester(ds).test_multi_sequence(_module(), sequence_list=("a",), stride=1, stream=10)


def test_stream_symbols_declared_with_replaces_line():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eemflow_hip.h")).read()
    for name in ("eemplus_forward_stream", "eemplus_stream_reset", "eemplus_stream_pending"):
        m = re.search(rf"\bint {name}\(", text)
        assert m, f"{name} is not declared in include/eemflow_hip.h"
        block = text[:m.start()].rsplit("*/", 1)[0].rsplit("/*", 1)[-1]
        assert "Replaces:" in block, f"{name}'s comment has no Replaces: line"
