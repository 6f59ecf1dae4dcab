"""Streaming EEMFlow+ inference (EEMFlow_cdc.forward_stream / eemplus_forward_stream): each event window padded and encoded once, its
pyramid levels 2..6 carried to the next pair.  Pair p of a stream must be forward(v_p, v_p+1) - bitwise what forward_many computes for
that pair in the same kernel forms - whatever the call boundaries, whatever ran on the module in between.  Needs a real MI355X:
`pytest -m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from eemflow_amd import _lib
from eemflow_amd.eemflow_plus import EEMFlow_cdc
from eemflow_amd.plus_weights import seeded_from_shapes
from eemflow_amd.weights import synthetic_voxel_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOW_TOL = 1e-3      # the project's flow tolerance


def make_net(seed, cin):
    net = EEMFlow_cdc("", 3, cin).eval()
    sd = seeded_from_shapes({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV), sd


def volumes(seed, n, h, w, cin=5):
    return [torch.from_numpy(synthetic_voxel_pair(seed + i, 1, h, w, bins=cin)[0]).to(DEV) for i in range(n)]


def preds_of(outs):
    return [torch.stack(preds) for _, preds in outs]            # [5][1][2][h][w] per pair


def pending(net):
    v = ctypes.c_int()
    _lib.check(_lib.lib().eemplus_stream_pending(net._ctx, ctypes.byref(v)))
    return v.value


def pin_forms(monkeypatch, net):
    """The kernel forms of plus_api.hip and of the conv dispatch it calls that follow the batch (the pairs B of the levels) or the
    encoder's image count (n windows in a stream call against 2 B in forward_many), pinned so that calls of different sizes compare bitwise:
    - plus_api.hip wnc_wanted (the fine levels' Winograd kernel, run_decoder's grouped Winograd launch, rconv riding the mask estimator's
      first launch, and the generic encoder's stride-1 layers through conv()): by (tile, job, sample) count - EEM_PLUS_WNC_MINPX /
      EEM_PLUS_WNC_MINPX_JOBS = 0 send every eligible map through the Winograd kernel whatever the count (read per call);
    - gconvb.hip (bf16-piece kernel): taken from EEM_GCONVB_MINBLK blocks on, its row tile by block count - EEM_NO_GCONVB=1 (per call);
    - gconv.hip split-K: below EEM_SPLITK_MAX plain blocks, its wave count by tile count - EEM_NO_SPLITK=1 (per call);
    - tail.hip tail_conv_launch's multi-tile form: from 40 (tile x batch) blocks - EEM_NO_TAIL_MULTI=1 (per call);
    - gconv16.hip's two-k-group form (blocks <= CUs) and row tile: fixed by frames_in_flight >= 3 (eemplus_set_frames_in_flight).
    Not batch-dependent: the 5-channel encoder's dispatch (enc_conv_launch: by layer shape and width only), the small-grid kernel's
    choice in plus_api.hip (map size), the generic kernel's tile per wave (gconv_kernel<2,1> / <1,1>: the same k order per output).
    Batch-dependent but not reached here: fewout's `small` split (gconv.hip) takes the dense estimator's last two layers only on maps above
    4 096 pixels whose width is no multiple of 4 once the Winograd kernel is pinned - no level of the sizes below."""
    for k, v in (("EEM_PLUS_WNC_MINPX", "0"), ("EEM_PLUS_WNC_MINPX_JOBS", "0"), ("EEM_NO_GCONVB", "1"), ("EEM_NO_SPLITK", "1"),
                 ("EEM_NO_TAIL_MULTI", "1")):
        monkeypatch.setenv(k, v)
    net.frames_in_flight = 3


# (h, w, cin, pairs): 200 x 300 pads to 256 x 320 (the padder); 15 channels take the generic encoder through conv()
EQ_SIZES = [(256, 320, 5, 6), (720, 1280, 5, 4), (200, 300, 15, 4)]


@pytest.mark.parametrize("h,w,cin,npairs", EQ_SIZES)
def test_stream_equals_forward_many(monkeypatch, h, w, cin, npairs):
    """k windows give k - 1 pairs; all five predictions of pair p are forward_many on [(v_p, v_p+1) ...] in ONE call (the same B).  The
    5-channel encoder's dispatch does not look at the image count, so no switch is set there.  The 15-channel (generic) encoder runs its
    layers through conv() over n images here and 2 B there: wnc_wanted, gconvb's block count, split-K, the small-grid kernel's
    multi-tile form and gconv16's k groups follow that count, so pin_forms pins them."""
    net, _ = make_net(41, cin)
    if cin != 5:
        pin_forms(monkeypatch, net)
    net.change_imagesize((h, w))
    v = volumes(600, npairs + 1, h, w, cin)
    with torch.no_grad():
        outs = net.forward_stream(v)
        got = [p.clone() for p in preds_of(outs)]
        ref = preds_of(net.forward_many([(v[i], v[i + 1]) for i in range(npairs)]))
    assert len(outs) == npairs
    for p, ((a, b), preds) in enumerate(outs):
        assert a is v[p] and b is v[p + 1] and len(preds) == 5 and preds[0].shape == (1, 2, h, w)
        assert torch.equal(got[p], ref[p]), p
    assert float(ref[0].abs().max()) > 1e-3


CARRY_SIZES = [(256, 320), (720, 1280)]


@pytest.mark.parametrize("h,w", CARRY_SIZES)
def test_carry_across_calls(monkeypatch, h, w):
    """Windows fed as calls of 1, 3, 1 and 6 volumes (0, 3, 1 and 6 pairs; the stream's buffers grow with the carried window in them)
    give the flows of one call over all eleven, bitwise - B differs, so every batch-dependent form is pinned (pin_forms)."""
    net, _ = make_net(42, 5)
    pin_forms(monkeypatch, net)
    net.change_imagesize((h, w))
    v = volumes(700, 11, h, w)
    with torch.no_grad():
        whole = [p.clone() for p in preds_of(net.forward_stream(v))]
        net.reset_stream()
        assert pending(net) == 0
        got, at = [], 0
        for size in (1, 3, 1, 6):
            outs = net.forward_stream(v[at:at + size])
            assert len(outs) == (size - 1 if at == 0 else size)
            if at > 0:
                assert outs[0][0][0] is v[at - 1]                    # events1 of the carried pair: the previous call's last tensor
            got += [p.clone() for p in preds_of(outs)]
            at += size
            assert pending(net) == 1
    assert len(got) == len(whole) == 10
    for i in range(10):
        assert torch.equal(got[i], whole[i]), i


def test_interleaved_calls_leave_the_carry_intact(monkeypatch):
    """forward and forward_many at other batch sizes between two stream calls rewrite the shared workspace and pyramid, not the carry."""
    h, w = 720, 1280
    net, _ = make_net(43, 5)
    pin_forms(monkeypatch, net)
    net.change_imagesize((h, w))
    v = volumes(800, 8, h, w)
    o = volumes(850, 6, h, w)
    with torch.no_grad():
        whole = [p.clone() for p in preds_of(net.forward_stream(v))]
        net.reset_stream()
        first = [p.clone() for p in preds_of(net.forward_stream(v[:4]))]
        net(torch.cat([o[0], o[2]]), torch.cat([o[1], o[3]]))
        net.forward_many([(o[2], o[3]), (o[4], o[5]), (o[1], o[0])])
        second = [p.clone() for p in preds_of(net.forward_stream(v[4:]))]
    got = first + second
    assert len(got) == 7
    for i in range(7):
        assert torch.equal(got[i], whole[i]), i


def test_reset_weights_size_and_abi_errors():
    h, w = 256, 320
    net, _ = make_net(44, 5)
    net.change_imagesize((h, w))
    v = volumes(900, 4, h, w)
    with torch.no_grad():
        assert len(net.forward_stream(v)) == 3
        assert len(net.forward_stream(v[:2])) == 2                   # carried: as many pairs as volumes
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
        assert torch.equal(torch.stack(outs[0][1]), torch.stack(net.forward_many([(v[0], v[1])])[0][1]))
        # a new image size resets the stream
        assert pending(net) == 1
        net.change_imagesize((128, 192))
        assert pending(net) == 0
        s = volumes(1000, 3, 128, 192)
        assert len(net.forward_stream(s)) == 2
        # the ABI refuses a wrong flow count, no volumes and too many, and keeps the carry
        L = _lib.lib()
        arr = (ctypes.c_void_p * 17)(*([s[0].data_ptr()] * 17))
        f = torch.empty(5, 1, 2, 128, 192, device=DEV)
        fo = (ctypes.c_void_p * 17)(*([f.data_ptr()] * 17))
        padc = (ctypes.c_int * 4)(*net.image_padder._pad)
        sp = _lib.current_stream_ptr(torch.device(DEV))
        assert L.eemplus_forward_stream(net._ctx, 2, arr, 128, 192, padc, fo, 1, sp) != 0      # carried: 2 volumes, 2 pairs
        assert b"nflow" in L.eemflow_last_error()
        assert L.eemplus_forward_stream(net._ctx, 17, arr, 128, 192, padc, fo, 17, sp) != 0
        assert L.eemplus_forward_stream(net._ctx, 0, arr, 128, 192, padc, fo, 0, sp) != 0
        assert pending(net) == 1
        # volumes of another size than the carried window: refused, naming the reset
        assert L.eemplus_forward_stream(net._ctx, 1, arr, 64, 96, padc, fo, 1, sp) != 0
        assert b"eemplus_stream_reset" in L.eemflow_last_error()
        assert pending(net) == 1
        torch.cuda.synchronize()
    with pytest.raises(ValueError):
        net.forward_stream([torch.zeros(1, 5, 8, 8, device=DEV)] * 17)


def test_replica_starts_without_carry():
    net, _ = make_net(45, 5)
    net.change_imagesize((128, 192))
    v = volumes(1100, 3, 128, 192)
    with torch.no_grad():
        net.forward_stream(v)
        twin = net.replicate()
        assert len(twin.forward_stream(v)) == 2
        assert pending(twin) == 1 and pending(net) == 1


def test_single_window_is_carried_without_flow():
    """A first call with one window encodes it, carries it and returns no flow; the next call's first pair starts at it."""
    net, _ = make_net(46, 5)
    net.change_imagesize((256, 320))
    v = volumes(1200, 3, 256, 320)
    with torch.no_grad():
        assert net.forward_stream(v[:1]) == []
        assert pending(net) == 1
        outs = net.forward_stream(v[1:])
        ref = preds_of(net.forward_many([(v[0], v[1]), (v[1], v[2])]))
    assert len(outs) == 2 and outs[0][0][0] is v[0]
    for p in range(2):
        assert torch.equal(torch.stack(outs[p][1]), ref[p]), p


# Against the oracle, teacher-forced, per pair of one stream call.  Windows synthetic_voxel_pair(500 + i, 1, h, w, bins=cin)[0], weights
# seeded_from_shapes(..., 91).  On these inputs the reference, run at 1 and at 8 CPU threads and teacher-forced from the same
# flow_init<l>, differs from itself by at most 1.5e-6 at 256x320 (5 pairs), 5.7e-7 at 200x300 with 15 channels (3 pairs) and 3.8e-6 at
# 1280x720 (2 pairs); no pixel of any level above 1e-3.
ORACLE_CASES = [(256, 320, 5, 5), (200, 300, 15, 3), (720, 1280, 5, 2)]


@pytest.mark.parametrize("h,w,cin,npairs", ORACLE_CASES)
def test_stream_levels_vs_oracle(h, w, cin, npairs):
    """flow6 of every pair within FLOW_TOL of the oracle (no warp upstream).  For l = 5..2 the teacher-forced level(l, flow_init<l>) -
    on the stream call's own pyramid and layout - returns the stream's flow_up<l> bitwise, and both of its outputs are held to the
    oracle's l-block run from the same flow_init (P.level_from_init): below FLOW_TOL at the small sizes; at 1280x720 at most 5e-4 of a
    level's pixels above FLOW_TOL and the max below 2e-2 (the warp mask's `>= 1.0` discontinuity, tests/test_gpu_plus.py)."""
    from oracle import eemflow_oracle as O
    from oracle import eemflow_plus_oracle as P
    net, sdn = make_net(91, cin)
    sd = O.to_torch_sd(sdn)
    net.change_imagesize((h, w))
    cpu = [torch.from_numpy(synthetic_voxel_pair(500 + i, 1, h, w, bins=cin)[0]) for i in range(npairs + 1)]
    with torch.no_grad():
        outs = net.forward_stream([x.to(DEV) for x in cpu])
        assert len(outs) == npairs
        st = [P.eemflow_plus_forward(sd, cpu[p], cpu[p + 1], keep=True)[1] for p in range(npairs)]
        f6 = net.stage("flow6").cpu()
        assert f6.shape[0] == npairs
        for p in range(npairs):
            assert float((f6[p:p + 1] - st[p]["flow6"]).abs().max()) < FLOW_TOL, p
        for l in (5, 4, 3, 2):
            init = net.stage(f"flow_init{l}")
            up_gpu = net.stage(f"flow_up{l}")
            up2, fl_gpu = net.level(l, init)
            assert torch.equal(up2, up_gpu), l
            for p in range(npairs):
                up_ref, fl_ref = P.level_from_init(sd, l, st[p]["f1"][l], st[p]["f2"][l], init[p:p + 1].cpu())
                d_up, d_fl = (up_gpu[p:p + 1].cpu() - up_ref).abs(), (fl_gpu[p:p + 1].cpu() - fl_ref).abs()
                e_up, e_fl = float(d_up.max()), float(d_fl.max())
                print(f"{h}x{w} c{cin} l{l} p{p}: flow_up {e_up:.3g} flow {e_fl:.3g}")
                if h * w < 512 * 512:
                    assert e_up < FLOW_TOL and e_fl < FLOW_TOL, (l, p, e_up, e_fl)
                else:
                    assert float((d_up > FLOW_TOL).float().mean()) < 5e-4 and float((d_fl > FLOW_TOL).float().mean()) < 5e-4, (l, p, e_up, e_fl)
                    assert e_up < 2e-2 and e_fl < 2e-2, (l, p, e_up, e_fl)


def test_mvsec_harness_stream(tmp_path, monkeypatch):
    """A synthetic MVSEC sequence (flow .npy files on disk, events from an injected reader) through EEMFlow_cdc: with the forms pinned,
    stream=10 gives the one-sample loop's mean AEE and voxelizes every window once - len + 1 windows instead of 2 * len."""
    from eemflow_amd.harness import Logger, TestRaftEvents
    from eemflow_amd.mvsec import MvsecEventFlow
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
    net, _ = make_net(47, 5)
    pin_forms(monkeypatch, net)
    tester = TestRaftEvents(ds, (256, 256), logger=Logger(verbose=False))
    ref = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1)
    assert counted["n"] == 2 * n_samples
    counted["n"] = 0
    got = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=10)
    assert counted["n"] == n_samples + 1
    assert abs(got - ref) < 1e-5, (got, ref)
    again = tester.test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=10)     # a second walk starts from a reset stream
    assert again == got
