"""Streaming inference (EEMFlow.forward_stream / eemflow_forward_stream): each event window encoded once, its pooled maps carried to
the next pair.  Flow i of a stream must be forward(v_i, v_{i+1}) - bitwise what forward_many computes for that pair in the same encoder
and decoder forms - whatever the call boundaries, whatever ran on the module in between.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from eemflow_amd import EEMFlow, _lib
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair
from oracle import eemflow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_net(seed):
    sd = seeded_state_dict(seed)
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV), sd


def volumes(seed, n, h, w):
    return [torch.from_numpy(synthetic_voxel_pair(seed + i, 1, h, w)[0]).to(DEV) for i in range(n)]


def flows_of(outs):
    return [preds[-1] for _, preds in outs]


def pending(net):
    v = ctypes.c_int()
    _lib.check(_lib.lib().eemflow_stream_pending(net._ctx, ctypes.byref(v)))
    return v.value


def graph_stats(net):
    gs = (ctypes.c_longlong * 3)()
    _lib.check(_lib.lib().eemflow_graph_stats(net._ctx, ctypes.byref(gs)))
    return list(gs)


def pin_forms(monkeypatch, mask):
    """The encoder's Winograd form (read when the weights are loaded) and the decoders' conv1 / conv5 kernel (read per call) both follow
    the batch by default; calls of different sizes compare bitwise only with both pinned."""
    monkeypatch.setenv("EEM_WINO4_LAYERS", mask)
    monkeypatch.setenv("EEM_DEC_WNC", "1")


SIZES = [(720, 1280, "7"), (260, 346, "1")]


@pytest.mark.parametrize("h,w,mask", SIZES)
def test_stream_equals_pairwise_forward_many(monkeypatch, h, w, mask):
    pin_forms(monkeypatch, mask)
    net, sd = make_net(61)
    net.change_imagesize((h, w))
    v = volumes(700, 11, h, w)
    with torch.no_grad():
        outs = net.forward_stream(v)
        ref = flows_of(net.forward_many([(v[i], v[i + 1]) for i in range(10)]))
    assert len(outs) == 10
    for i, ((a, b), preds) in enumerate(outs):
        assert a is v[i] and b is v[i + 1]
        assert preds[0].shape == (1, 2, h, w)
        assert torch.equal(preds[0], ref[i]), i
    # against the oracle's EEMFlow.forward on the pair (all ten pairs at the small size, three at 1280x720 - the CPU oracle is slow there)
    tsd = O.to_torch_sd(sd)
    for i in (range(10) if h < 720 else (0, 4, 9)):
        r, _ = O.eemflow_forward(tsd, v[i].cpu(), v[i + 1].cpu())
        assert float((outs[i][1][0].cpu() - r).abs().max()) < 1e-4, i


@pytest.mark.parametrize("h,w,mask", SIZES)
def test_carry_across_calls(monkeypatch, h, w, mask):
    pin_forms(monkeypatch, mask)
    net, _ = make_net(62)
    net.change_imagesize((h, w))
    v = volumes(800, 11, h, w)
    with torch.no_grad():
        whole = flows_of(net.forward_stream(v))
        net.reset_stream()
        assert pending(net) == 0
        got, at = [], 0
        for size in (1, 3, 1, 6):
            outs = net.forward_stream(v[at:at + size])
            assert len(outs) == (size - 1 if at == 0 else size)
            if at > 0:
                assert outs[0][0][0] is v[at - 1]                    # events1 of the carried pair: the previous call's last tensor
            got += flows_of(outs)
            at += size
            assert pending(net) == 1
    assert len(got) == len(whole) == 10
    for i in range(10):
        assert torch.equal(got[i], whole[i]), i


def test_interleaved_calls_leave_the_carry_intact(monkeypatch):
    h, w = 720, 1280
    pin_forms(monkeypatch, "7")
    net, _ = make_net(63)
    net.change_imagesize((h, w))
    v = volumes(900, 8, h, w)
    o = volumes(950, 6, h, w)
    with torch.no_grad():
        whole = flows_of(net.forward_stream(v))
        net.reset_stream()
        first = flows_of(net.forward_stream(v[:4]))
        net(o[0], o[1])                                              # the shared workspace is rewritten by other batch sizes
        net.forward_many([(o[2], o[3]), (o[4], o[5]), (o[1], o[0])])
        second = flows_of(net.forward_stream(v[4:]))
    got = first + second
    assert len(got) == 7
    for i in range(7):
        assert torch.equal(got[i], whole[i]), i


def test_reset_weights_size_and_abi_errors():
    h, w = 260, 346
    net, _ = make_net(64)
    net.change_imagesize((h, w))
    v = volumes(1000, 4, h, w)
    with torch.no_grad():
        assert len(net.forward_stream(v)) == 3
        assert len(net.forward_stream(v[:2])) == 2                   # carried: as many flows as volumes
        net.reset_stream()
        assert pending(net) == 0
        assert len(net.forward_stream(v[:3])) == 2
    # a weight change between calls: refused until reset_stream()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    for p in net.parameters():
        p.grad = torch.full_like(p, 1e-2)
    opt.step()
    with torch.no_grad():
        with pytest.raises(_lib.EEMFlowHipError, match="reset_stream"):
            net.forward_stream(v[:2])
        with pytest.raises(_lib.EEMFlowHipError, match="reset_stream"):
            net.forward_stream(v[:2])                                # still refused: nothing was reset
        net.reset_stream()
        outs = net.forward_stream(v[:2])
        assert len(outs) == 1
        assert torch.equal(outs[0][1][0], net.forward_many([(v[0], v[1])])[0][1][0])
        # a new image size resets the stream
        assert pending(net) == 1
        net.change_imagesize((128, 192))
        assert pending(net) == 0
        s = volumes(1100, 3, 128, 192)
        assert len(net.forward_stream(s)) == 2
        # the ABI refuses a wrong flow count and too many volumes, and keeps the carry
        L = _lib.lib()
        arr = (ctypes.c_void_p * 17)(*([s[0].data_ptr()] * 17))
        f = torch.empty(1, 2, 128, 192, device=DEV)
        fo = (ctypes.c_void_p * 17)(*([f.data_ptr()] * 17))
        sp = _lib.current_stream_ptr(torch.device(DEV))
        assert L.eemflow_forward_stream(net._ctx, 2, arr, fo, 1, 128, 192, 128, 192, sp) != 0      # carried: 2 volumes, 2 flows
        assert b"nflow" in L.eemflow_last_error()
        assert L.eemflow_forward_stream(net._ctx, 17, arr, fo, 17, 128, 192, 128, 192, sp) != 0
        assert L.eemflow_forward_stream(net._ctx, 0, arr, fo, 0, 128, 192, 128, 192, sp) != 0
        assert pending(net) == 1
        # volumes of another size than the carried window: refused, naming the reset
        assert L.eemflow_forward_stream(net._ctx, 1, arr, fo, 1, 64, 96, 64, 96, sp) != 0
        assert b"eemflow_stream_reset" in L.eemflow_last_error()
    with pytest.raises(ValueError):
        net.forward_stream([torch.zeros(1, 5, 8, 8, device=DEV)] * 17)


def test_replica_starts_without_carry():
    net, _ = make_net(65)
    net.change_imagesize((128, 192))
    v = volumes(1200, 3, 128, 192)
    with torch.no_grad():
        net.forward_stream(v)
        twin = net.replicate()
        assert len(twin.forward_stream(v)) == 2


def test_deferred_normalisation_stream():
    from eemflow_amd import EventSequence
    from eemflow_amd.hrem import synthetic_hrem_events
    from eemflow_amd.voxelizer import voxelize_many_device
    h, w, bins, n = 720, 1280, 5, 5
    net, _ = make_net(66)
    net.change_imagesize((h, w))
    sets = []
    for k in range(n):
        seq = EventSequence(None, {"height": h, "width": w}, features=synthetic_hrem_events(300 + k, 200000, h, w),
                            timestamp_multiplier=1e6, convert_to_relative=True)
        sets.append(torch.from_numpy(np.ascontiguousarray(seq.features)).to(DEV))
    raw = voxelize_many_device(sets, bins, h, w, normalize="deferred")
    normed = voxelize_many_device(sets, bins, h, w, normalize=True)
    with torch.no_grad():
        a = flows_of(net.forward_stream([r[None] for r in raw[:3]], deferred_norm=True))
        a += flows_of(net.forward_stream([r[None] for r in raw[3:]], deferred_norm=True))
        net.reset_stream()
        b = flows_of(net.forward_stream([x[None] for x in normed]))
        with pytest.raises(ValueError):
            net.forward_stream([x[None].clone() for x in normed[:2]], deferred_norm=True)
    assert len(a) == len(b) == 4
    for i in range(4):
        assert float((a[i] - b[i]).abs().max()) < 2e-5, i


def test_graph_reuse_with_fresh_tensors():
    h, w = 720, 1280
    net, _ = make_net(67)
    net.change_imagesize((h, w))
    base = volumes(1300, 10, h, w)
    with torch.no_grad():
        for call in range(20):
            fresh = [b.clone() for b in base]                       # new buffers every call: the io table, not a new capture
            outs = net.forward_stream(fresh)
            assert len(outs) == (9 if call == 0 else 10)
            if call == 2:
                caps = graph_stats(net)[0]
                assert caps <= 3                                     # no carry / carry into slot 1 / carry into slot 0
        cap, rep, io = graph_stats(net)
    assert cap == caps and rep == 20 and io >= 20


def test_mvsec_harness_stream(tmp_path, monkeypatch):
    """A synthetic MVSEC sequence (flow .npy files on disk, events from an injected reader): the stream walk gives the one-sample loop's
    mean AEE and voxelizes every window once - len + 1 windows instead of 2 * len."""
    from eemflow_amd.harness import Logger, TestRaftEvents
    from eemflow_amd.mvsec import MvsecEventFlow
    pin_forms(monkeypatch, "7")
    n_samples, first = 23, 40
    flow_dir = tmp_path / "dataset" / "MVSEC" / "seqA" / "flowgt_dt1"
    flow_dir.mkdir(parents=True)
    rng = np.random.default_rng(5)
    for i in range(first, first + n_samples):
        np.save(flow_dir / f"{i}.npy", rng.normal(0, 2, (2, 260, 346)).astype(np.float32))

    def reader(path):
        k = int(os.path.basename(path).split(".")[0])
        r = np.random.default_rng(10_000 + k)
        m = 20000
        ts = np.sort(r.uniform(k * 0.05, (k + 1) * 0.05, m))
        return np.stack([ts, r.integers(0, 346, m), r.integers(0, 260, m), r.integers(0, 2, m) * 2 - 1], axis=1).astype(np.float64)

    args = {"eval_type": "sparse", "num_voxel_bins": 5, "sequence": "seqA"}
    ds = MvsecEventFlow(args, train=False, root=str(tmp_path), events_reader=reader, valid_time_index={"seqA": [(first, first + n_samples)]})
    counted = {"n": 0}
    many, pair = ds.voxel.many, ds.voxel.pair

    def many_c(seqs):
        seqs = list(seqs)
        counted["n"] += len(seqs)
        return many(seqs)

    def pair_c(a, b):
        counted["n"] += 2
        return pair(a, b)
    ds.voxel.many, ds.voxel.pair = many_c, pair_c
    net, _ = make_net(68)
    tester = TestRaftEvents(ds, (256, 256), logger=Logger(verbose=False))
    ref = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1)
    assert counted["n"] == 2 * n_samples
    counted["n"] = 0
    got = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=10)
    assert counted["n"] == n_samples + 1
    assert abs(got - ref) < 1e-5, (got, ref)
    again = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=10)     # a second walk starts from a reset stream
    assert again == got
