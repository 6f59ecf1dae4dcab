"""The stage recorder E-RAFT and EEMFlow+ share (csrc/stagerec.h, DevStageRecorder in csrc/devstate_hip.h), on the GPU: its arena
across growth, its invisibility, and contexts that come and go.  `pytest -m gpu`.

The fp64 stage suites check every recorded value; tests/stagerec_check.cpp the recorder's decisions on the CPU.  What is left for here:
  * the arena grows with the largest recording call and is reused by smaller ones: 64x64, 64x128, 64x64 again must file the same names
    and, bit for bit, the same tensors the third time as the first;
  * with the recorder off the same forward returns bitwise the same flow (the stream tests hold these forwards to bitwise
    repeatability: tests/test_gpu_eraft_stream.py, tests/test_gpu_plus_stream.py);
  * switching the recorder off: EEMFlow+ drops its records at once, E-RAFT keeps them until its next call;
  * twenty contexts made, run and destroyed in one process (every buffer goes with its context; nothing is asserted on free memory,
    which other processes move).

64x64 at batch 1 (E-RAFT: two iterations, the first recorded) is the smallest input at which every pyramid level of both models exists.
"""
import pytest
import torch

from eemflow_amd import EEMFlow
from eemflow_amd import eraft_weights, plus_weights
from eemflow_amd.eemflow_plus import EEMFlow_cdc
from eemflow_amd.eraft import ERAFT
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERS = 2
RECORD = {"eraft": (("",), 1), "eemplus": ("",)}


def make_net(kind, record=True):
    if kind == "eemflow":
        net = EEMFlow("", groups=5, n_first_channels=5).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(7).items()})
        return net.to(DEV)
    net, seeded = (ERAFT("", 5), eraft_weights.seeded_from_shapes) if kind == "eraft" else (EEMFlow_cdc("", 3, 5), plus_weights.seeded_from_shapes)
    sd = seeded({k: tuple(v.shape) for k, v in net.state_dict().items()}, 7)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.record_stages = RECORD[kind] if record else None
    return net.eval().to(DEV)


def inputs(seed, h, w):
    return tuple(torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(seed, 1, h, w))


def forward(kind, net, e1, e2):
    """The final full-resolution flow of one forward at the inputs' size, on the CPU."""
    net.change_imagesize(tuple(e1.shape[2:]))
    with torch.no_grad():
        preds = net(e1, e2, iters=ITERS)[1] if kind == "eraft" else net(e1, e2)[1]
    torch.cuda.synchronize()
    return preds[-1].cpu()


def same_bits(a, b):
    """Bit for bit.  (E-RAFT's coarsest correlation level is one cell wide at 64x64: its sampler divides by w - 1 = 0, as the reference's
    does, and the NaN that follows must come out the same too - torch.equal would call it different from itself.)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def recorded(net):
    torch.cuda.synchronize()
    names = net.stage_names()
    return names, {name: net.stage(name).cpu() for name, _, _ in names}


@pytest.mark.parametrize("kind", ["eraft", "eemplus"])
def test_arena_across_growth_and_invisibility(kind):
    small, large = inputs(11, 64, 64), inputs(12, 64, 128)
    net = make_net(kind)
    flow1 = forward(kind, net, *small)                         # (the arena starts empty: this call measures, then runs again)
    names1, stages1 = recorded(net)
    assert len(names1) > 40 and len({n for n, _, _ in names1}) == len(names1), names1
    forward(kind, net, *large)
    names2 = net.stage_names()
    assert sum(d[0] * d[1] * d[2] * d[3] for _, _, d in names2) > sum(d[0] * d[1] * d[2] * d[3] for _, _, d in names1)
    flow3 = forward(kind, net, *small)                         # (a smaller call in the grown arena)
    names3, stages3 = recorded(net)
    assert names3 == names1
    for name, t in stages1.items():
        assert same_bits(stages3[name], t), name
    assert same_bits(flow3, flow1)

    # a context that never recorded gives the same flow
    off = make_net(kind, record=False)
    assert same_bits(forward(kind, off, *small), flow1) and off.stage_names() == []

    # switching it off: the setting reaches the context with the next call's settings
    net.record_stages = None
    assert net.stage_names() == names1
    net._context(torch.device(DEV))
    assert net.stage_names() == ([] if kind == "eemplus" else names1)      # EEMFlow+ drops its records at once, E-RAFT with its next call
    assert same_bits(forward(kind, net, *small), flow1)
    assert net.stage_names() == []
    net.record_stages = RECORD[kind]                                        # ... and on again, in the arena it has
    assert same_bits(forward(kind, net, *small), flow1)
    names5, stages5 = recorded(net)
    assert names5 == names1 and all(same_bits(stages5[n], t) for n, t in stages1.items())


@pytest.mark.parametrize("kind", ["eraft", "eemplus", "eemflow"])
def test_contexts_come_and_go(kind):
    e1, e2 = inputs(11, 128, 192) if kind == "eemflow" else inputs(11, 64, 64)     # (EEMFlow: the streams tests' small size)
    net = make_net(kind)
    first = forward(kind, net, e1, e2)
    for _ in range(20):
        net._release()                                          # (the next forward makes a new context and loads the weights into it)
        assert net._ctx is None
        assert same_bits(forward(kind, net, e1, e2), first)
    net._release()
