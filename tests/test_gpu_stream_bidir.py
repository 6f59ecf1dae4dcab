"""Bidirectional streaming inference (EEMFlow.forward_stream(bidirectional=True) / eemflow_forward_stream_bidir): the encoder runs once
per window, the 1/64-grid tail over every pair twice - the second time with the two windows' roles exchanged.  flow_fw of pair p must be
forward_many(v_p, v_p+1) and flow_bw forward_many(v_p+1, v_p), bitwise in the same encoder and decoder forms, whatever the call
boundaries, whichever of the two stream calls came before, whatever ran on the module in between.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes

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


def fw_of(outs):
    return [o[1][-1] for o in outs]


def bw_of(outs):
    return [o[2][-1] for o in outs]


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
    the batch by default - and a bidirectional call decodes 2 x its pairs; calls compare bitwise only with both pinned."""
    monkeypatch.setenv("EEM_WINO4_LAYERS", mask)
    monkeypatch.setenv("EEM_DEC_WNC", "1")


SIZES = [(720, 1280, "7"), (260, 346, "1")]


@pytest.mark.parametrize("h,w,mask", SIZES)
def test_both_directions_equal_pairwise_forward_many(monkeypatch, h, w, mask):
    pin_forms(monkeypatch, mask)
    net, sd = make_net(61)
    net.change_imagesize((h, w))
    v = volumes(700, 8, h, w)
    with torch.no_grad():
        outs = net.forward_stream(v, bidirectional=True)
        ref_fw = [p[-1] for _, p in net.forward_many([(v[i], v[i + 1]) for i in range(7)])]
        ref_bw = [p[-1] for _, p in net.forward_many([(v[i + 1], v[i]) for i in range(7)])]
    assert len(outs) == 7
    for i, item in enumerate(outs):
        assert len(item) == 3
        (a, b), pf, pb = item
        assert a is v[i] and b is v[i + 1]
        assert pf[0].shape == pb[0].shape == (1, 2, h, w)
        assert torch.equal(pf[0], ref_fw[i]), i
        assert torch.equal(pb[0], ref_bw[i]), i
        assert not torch.equal(pf[0], pb[0])
    # the backward flow against the oracle's EEMFlow.forward on the swapped pair (all pairs at the small size, three at 1280x720 - the
    # CPU oracle is slow there)
    tsd = O.to_torch_sd(sd)
    for i in (range(7) if h < 720 else (0, 3, 6)):
        r, _ = O.eemflow_forward(tsd, v[i + 1].cpu(), v[i].cpu())
        err = float((outs[i][2][0].cpu() - r).abs().max())
        print(f"{h}x{w} pair {i}: backward flow against the oracle, max |diff| = {err:.3e}")
        assert err < 1e-4, i


@pytest.mark.parametrize("h,w,mask", SIZES)
def test_carry_across_bidirectional_calls(monkeypatch, h, w, mask):
    pin_forms(monkeypatch, mask)
    net, _ = make_net(62)
    net.change_imagesize((h, w))
    v = volumes(800, 8, h, w)
    with torch.no_grad():
        whole = net.forward_stream(v, bidirectional=True)
        net.reset_stream()
        assert pending(net) == 0
        got, at = [], 0
        for size in (1, 3, 1, 3):
            outs = net.forward_stream(v[at:at + size], bidirectional=True)
            assert len(outs) == (size - 1 if at == 0 else size)
            if at > 0:
                assert outs[0][0][0] is v[at - 1]                    # events1 of the carried pair: the previous call's last tensor
            got += outs
            at += size
            assert pending(net) == 1
    assert len(got) == len(whole) == 7
    for i in range(7):
        assert torch.equal(got[i][1][0], whole[i][1][0]), i
        assert torch.equal(got[i][2][0], whole[i][2][0]), i


@pytest.mark.parametrize("h,w,mask", SIZES)
def test_unidirectional_and_bidirectional_calls_share_the_stream(monkeypatch, h, w, mask):
    pin_forms(monkeypatch, mask)
    net, _ = make_net(63)
    net.change_imagesize((h, w))
    v = volumes(900, 8, h, w)
    with torch.no_grad():
        whole = net.forward_stream(v, bidirectional=True)
        net.reset_stream()
        uni_before = net.forward_stream(v)                          # the unidirectional stream is what it was
        net.reset_stream()
        first = net.forward_stream(v[:3])                           # pairs 0, 1
        second = net.forward_stream(v[3:6], bidirectional=True)     # pairs 2, 3, 4: the first starts at the unidirectional call's carry
        third = net.forward_stream(v[6:])                           # pairs 5, 6: the first starts at the bidirectional call's carry
    assert [len(x) for x in (first, second, third)] == [2, 3, 2]
    assert all(len(o) == 2 for o in first + third) and all(len(o) == 3 for o in second)
    for i in range(7):
        assert torch.equal(uni_before[i][1][0], whole[i][1][0]), i
    for j, o in enumerate(first):
        assert torch.equal(o[1][0], whole[j][1][0]), j
    for j, o in enumerate(second):
        assert torch.equal(o[1][0], whole[2 + j][1][0]), j
        assert torch.equal(o[2][0], whole[2 + j][2][0]), j
    for j, o in enumerate(third):
        assert torch.equal(o[1][0], whole[5 + j][1][0]), j


def test_interleaved_calls_leave_the_carry_intact(monkeypatch):
    h, w = 720, 1280
    pin_forms(monkeypatch, "7")
    net, _ = make_net(63)
    net.change_imagesize((h, w))
    v = volumes(900, 8, h, w)
    o = volumes(950, 6, h, w)
    with torch.no_grad():
        whole = net.forward_stream(v, bidirectional=True)
        net.reset_stream()
        first = net.forward_stream(v[:4], bidirectional=True)
        net(o[0], o[1])                                              # the shared workspace is rewritten by other batch sizes
        net.forward_many([(o[2], o[3]), (o[4], o[5]), (o[1], o[0])])
        second = net.forward_stream(v[4:], bidirectional=True)
    got = first + second
    assert len(got) == 7
    for i in range(7):
        assert torch.equal(got[i][1][0], whole[i][1][0]), i
        assert torch.equal(got[i][2][0], whole[i][2][0]), i


def test_weight_change_limit_and_abi_errors():
    h, w = 260, 346
    net, _ = make_net(64)
    net.change_imagesize((h, w))
    v = volumes(1000, 4, h, w)
    with torch.no_grad():
        assert len(net.forward_stream(v, bidirectional=True)) == 3
        assert len(net.forward_stream(v[:2], bidirectional=True)) == 2      # carried: as many pairs as volumes
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    for p in net.parameters():
        p.grad = torch.full_like(p, 1e-2)
    opt.step()
    with torch.no_grad():
        with pytest.raises(_lib.EEMFlowHipError, match="reset_stream"):
            net.forward_stream(v[:2], bidirectional=True)
        with pytest.raises(_lib.EEMFlowHipError, match="reset_stream"):
            net.forward_stream(v[:2], bidirectional=True)            # still refused: nothing was reset
        net.reset_stream()
        outs = net.forward_stream(v[:2], bidirectional=True)
        assert len(outs) == 1
        assert torch.equal(outs[0][1][0], net.forward_many([(v[0], v[1])])[0][1][0])
        assert torch.equal(outs[0][2][0], net.forward_many([(v[1], v[0])])[0][1][0])
        # the ABI refuses more than EEM_STREAM_BIDIR_MAX_VOLUMES volumes and a wrong flow count, and keeps the carry
        L = _lib.lib()
        arr = (ctypes.c_void_p * 9)(*([v[0].data_ptr()] * 9))
        f = torch.empty(1, 2, h, w, device=DEV)
        fo = (ctypes.c_void_p * 9)(*([f.data_ptr()] * 9))
        sp = _lib.current_stream_ptr(torch.device(DEV))
        assert pending(net) == 1
        assert L.eemflow_forward_stream_bidir(net._ctx, 9, arr, fo, fo, 9, h, w, h, w, sp) != 0
        assert b"1..8" in L.eemflow_last_error()
        assert L.eemflow_forward_stream_bidir(net._ctx, 2, arr, fo, fo, 1, h, w, h, w, sp) != 0       # carried: 2 volumes, 2 pairs
        assert b"nflow" in L.eemflow_last_error()
        assert L.eemflow_forward_stream_bidir(net._ctx, 2, arr, fo, None, 2, h, w, h, w, sp) != 0
        assert pending(net) == 1
        assert L.eemflow_forward_stream_bidir(net._ctx, 1, arr, fo, fo, 1, 64, 96, 64, 96, sp) != 0
        assert b"eemflow_stream_reset" in L.eemflow_last_error()
    with pytest.raises(ValueError, match="1..8"):
        net.forward_stream([torch.zeros(1, 5, 8, 8, device=DEV)] * 9, bidirectional=True)


def test_deferred_normalisation_bidirectional_stream():
    import numpy as np
    from eemflow_amd import EventSequence
    from eemflow_amd.hrem import synthetic_hrem_events
    from eemflow_amd.voxelizer import voxelize_many_device
    h, w, bins, n = 720, 1280, 5, 4
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
        a = net.forward_stream([r[None] for r in raw], deferred_norm=True, bidirectional=True)
        net.reset_stream()
        b = net.forward_stream([x[None] for x in normed], bidirectional=True)
    assert len(a) == len(b) == 3
    for i in range(3):
        assert float((a[i][1][0] - b[i][1][0]).abs().max()) < 2e-5, i
        assert float((a[i][2][0] - b[i][2][0]).abs().max()) < 2e-5, i


def test_graph_reuse_of_repeated_bidirectional_calls():
    h, w = 720, 1280
    net, _ = make_net(67)
    net.change_imagesize((h, w))
    base = volumes(1300, 8, h, w)
    with torch.no_grad():
        for call in range(12):
            fresh = [b.clone() for b in base]                       # new buffers every call: the io table, not a new capture
            outs = net.forward_stream(fresh, bidirectional=True)
            assert len(outs) == (7 if call == 0 else 8)
            if call == 2:
                caps = graph_stats(net)[0]
                assert caps <= 3                                     # no carry / carry into slot 1 / carry into slot 0
        cap, rep, io = graph_stats(net)
        assert cap == caps and rep == 12 and io >= 12
        # the direction mode is part of the graph key: a unidirectional call of the same volumes is another graph, and going back is not
        net.forward_stream([b.clone() for b in base])
        assert graph_stats(net)[0] == caps + 1
        net.forward_stream([b.clone() for b in base], bidirectional=True)
        assert graph_stats(net)[0] == caps + 1


def test_masks_of_the_stream_are_those_of_fb_check(monkeypatch):
    import eemflow_amd
    h, w = 260, 346
    net, _ = make_net(61)
    net.change_imagesize((h, w))
    v = volumes(700, 4, h, w)
    with torch.no_grad():
        outs = net.forward_stream(v, bidirectional=True, fb_check=(0.01, 0.5, "obj"))
    assert len(outs) == 3
    for (a, b), pf, pb, (mf, mb) in outs:
        assert mf.shape == mb.shape == (1, 1, h, w)
        rf, rb = eemflow_amd.fb_check(pf[0], pb[0], 0.01, 0.5, "obj")
        assert torch.equal(mf, rf) and torch.equal(mb, rb)
        assert set(torch.unique(mf).tolist()) <= {0.0, 1.0}
