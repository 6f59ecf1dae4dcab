"""E-RAFT's stream and warm start on the GPU: eraft_forward_interpolate against the reference function, ERAFT.forward_stream against
forward_many, the manual warm-start loop, the oracle and a reference warm chain.  `pytest -m gpu`.

Bitwise comparisons between calls whose encoder batches differ pin the batch-dependent kernel forms with the per-call switches
(pin_forms): EEM_ERAFT_NO_F4=1 and EEM_ERAFT_NO_WNC=1 (the encoders' Winograd convs qualify from a tile count on, so the feature
network's nvol images and forward_many's 2 nflow can take different forms), EEM_NO_SPLITK=1 (split-K of the small deep convs from a
block count on), EEM_NO_GCONV16=1 and EEM_NO_GCONVB=1 (the LDS-tiled kernels pick their K-groups and tile heights from the block
count).  With the first three alone the cold stream differed from forward_many by up to 2e-5; with all five it is bitwise."""
import ctypes
import os

import numpy as np
import pytest
import torch

from eemflow_amd import _lib
from eemflow_amd.eraft import ERAFT, forward_interpolate
from eemflow_amd.eraft_weights import seeded_from_shapes
from eemflow_amd.weights import synthetic_voxel_pair
from oracle import eemflow_oracle as O
from oracle import eraft_oracle as R
from test_eraft_stream_host import fi_restated, golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_net(seed, final_only=False, warm=False):
    net = ERAFT("", 5).eval()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = seeded_from_shapes(shapes, seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.final_only, net.warm_start = final_only, warm
    return net.to(DEV), O.to_torch_sd(sd)


def volumes(seed, n, h, w):
    return [torch.from_numpy(synthetic_voxel_pair(seed + k, 1, h, w)[0]).to(DEV) for k in range(n)]


def pending(net):
    out = ctypes.c_int()
    _lib.check(_lib.lib().eraft_stream_pending(net._ctx, ctypes.byref(out)))
    return out.value


def pin_forms(monkeypatch):
    for k in ("EEM_ERAFT_NO_F4", "EEM_ERAFT_NO_WNC", "EEM_NO_SPLITK", "EEM_NO_GCONV16", "EEM_NO_GCONVB"):
        monkeypatch.setenv(k, "1")


def same(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def diff(a, b):
    return float((a.detach().cpu() - b.detach().cpu()).abs().max())


# ---------------------------------------------------------------------------------------------------- forward interpolation
def test_interpolation_kernel_equals_the_reference_bitwise():
    for name, flow, ref in golden_cases():
        got = forward_interpolate(torch.from_numpy(flow).to(DEV)).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{name}: {int((got != ref).sum())} cells differ"


@pytest.mark.parametrize("h,w", [(480, 640), (720, 1280)])
def test_interpolation_kernel_on_real_flow_low(h, w):
    """The GPU's own flow_low from real forwards (two samples), against the CPU restatement; two runs are bitwise identical."""
    net, _ = make_net(71)
    net.change_imagesize((h, w))
    v = volumes(900, 3, h, w)
    with torch.no_grad():
        net(torch.cat(v[:2]), torch.cat(v[1:]), iters=4)
        low = net.stage("flow_low")
        a = forward_interpolate(low)
        b = forward_interpolate(low)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        one = low[:1].contiguous()
        for _ in range(5):
            forward_interpolate(one)
        start.record()
        for _ in range(50):
            forward_interpolate(one)
        stop.record()
        torch.cuda.synchronize()
    print(f"forward_interpolate {tuple(one.shape)}: {start.elapsed_time(stop) / 50 * 1e3:.1f} us per call (with its allocations)")
    assert same(a, b)
    ref = fi_restated(low.cpu().numpy())
    got = a.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), int((got != ref).sum())


# ---------------------------------------------------------------------------------------------------- cold stream
@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("h,w", [(480, 640), (136, 200)])
def test_cold_stream_equals_forward_many(monkeypatch, h, w, final):
    pin_forms(monkeypatch)
    net, _ = make_net(72, final_only=final)
    net.change_imagesize((h, w))
    v = volumes(1000, 8, h, w)
    with torch.no_grad():
        got = net.forward_stream(v, iters=3)
        ref = net.forward_many([(v[i], v[i + 1]) for i in range(7)], iters=3)
    assert len(got) == 7
    for p, ((e1, e2), preds) in enumerate(got):
        assert e1 is v[p] and e2 is v[p + 1]
        assert len(preds) == (1 if final else 3)
        for k, (a, b) in enumerate(zip(preds, ref[p][1])):
            assert same(a, b), (p, k, diff(a, b))


# ---------------------------------------------------------------------------------------------------- carry
@pytest.mark.parametrize("warm", [False, True])
def test_calls_of_1_3_1_6_windows_equal_one_call_of_11(monkeypatch, warm):
    """Calls of 1, 3, 1 and 6 windows give what one call of 11 gives, with forward / forward_many calls in between: bitwise when warm
    (every pair's update loop runs at batch 1 in both).  Cold, a call's update loop runs at the batch of its pairs (1, 3, 1, 6 against
    10), whose kernel forms differ: each call is then bitwise forward_many on its own pairs - the carried window's feature map and
    volume are exact - and within 1e-4 of the one call."""
    pin_forms(monkeypatch)
    h, w = 256, 320
    net, _ = make_net(73, final_only=True, warm=warm)
    net.change_imagesize((h, w))
    v = volumes(1100, 11, h, w)
    with torch.no_grad():
        one = net.forward_stream(v, iters=3)
        net.reset_stream()
        parts, j = [], 0
        for n in (1, 3, 1, 6):
            got = net.forward_stream(v[j:j + n], iters=3)
            if got and not warm:
                ref = net.forward_many([(a, b) for (a, b), _ in got], iters=3)
                for (_, pa), (_, pb) in zip(got, ref):
                    assert same(pa[0], pb[0]), diff(pa[0], pb[0])
            parts += got
            j += n
            assert pending(net) == 1
            net(v[0], v[5], iters=2)                                   # the carry survives the other entry points
            net.forward_many([(v[1], v[2]), (v[3], v[4])], iters=2)
    assert len(one) == len(parts) == 10
    for p in range(10):
        assert parts[p][0][0] is v[p] and parts[p][0][1] is v[p + 1]
        if warm:
            assert same(parts[p][1][0], one[p][1][0]), (p, diff(parts[p][1][0], one[p][1][0]))
        else:
            assert diff(parts[p][1][0], one[p][1][0]) < 1e-4, p
    net.reset_stream()
    assert pending(net) == 0


# ---------------------------------------------------------------------------------------------------- warm start
def test_warm_stream_equals_the_manual_loop(monkeypatch):
    """forward(v_p, v_p+1, flow_init=forward_interpolate(stage("flow_low"))) pair by pair - the first pair cold - across a call boundary."""
    pin_forms(monkeypatch)
    h, w = 480, 640
    net, _ = make_net(74, warm=True)
    net.change_imagesize((h, w))
    v = volumes(1200, 6, h, w)
    with torch.no_grad():
        got = net.forward_stream(v[:3], iters=3) + net.forward_stream(v[3:], iters=3)
        net.reset_stream()
        ref, init = [], None
        for p in range(5):
            _, preds = net(v[p], v[p + 1], iters=3, flow_init=init)
            ref.append(preds)
            init = forward_interpolate(net.stage("flow_low"))
    assert len(got) == 5
    for p in range(5):
        for k in range(3):
            assert same(got[p][1][k], ref[p][k]), (p, k, diff(got[p][1][k], ref[p][k]))


@pytest.mark.parametrize("h,w", [(128, 160), (136, 200)])
def test_warm_stream_against_the_oracle(h, w):
    """Each pair within 1e-3 of the oracle run from the restated interpolation of the GPU's own flow_low of the pair before."""
    net, sd = make_net(75, warm=True)
    net.change_imagesize((h, w))
    v = volumes(1300, 5, h, w)
    with torch.no_grad():
        got = net.forward_stream(v[:2], iters=4) + net.forward_stream(v[2:], iters=4)
        lows = [net.stage("flow_low")]                                 # pairs 1..3 of the second call
    net.reset_stream()
    with torch.no_grad():
        net.forward_stream(v[:2], iters=4)
        lows.insert(0, net.stage("flow_low"))                          # pair 0 (the first call alone is deterministic)
    low = torch.cat(lows).cpu()
    assert low.shape[0] == 4
    for p in range(4):
        init = None if p == 0 else torch.from_numpy(fi_restated(low[p - 1:p].numpy()))
        ref, _ = R.eraft_forward(sd, v[p].cpu(), v[p + 1].cpu(), iters=4, flow_init=init)
        assert diff(got[p][1][-1], ref[-1]) < 1e-3, (p, diff(got[p][1][-1], ref[-1]))


def test_warm_stream_against_the_reference_chain(golden):
    g = golden("eraft_warm_128x160.npz")
    h, w = (int(x) for x in g["hw"])
    iters = int(g["iters"])
    net, _ = make_net(int(g["seed"]), warm=True)
    net.change_imagesize((h, w))
    s0, s1 = (int(x) for x in g["input_seeds"])
    v0, v1 = (torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(s0, 1, h, w))
    v2 = torch.from_numpy(synthetic_voxel_pair(s1, 1, h, w)[0]).to(DEV)
    with torch.no_grad():
        out = net.forward_stream([v0, v1, v2], iters=iters)
        low = net.stage("flow_low")
        fi1 = forward_interpolate(low[:1])
    assert diff(low[:1], torch.from_numpy(g["flow_low0"])) < 1e-4
    assert diff(fi1, torch.from_numpy(g["flow_init1"])) < 1e-4
    assert diff(out[0][1][-1], torch.from_numpy(g["pred0_last"])) < 1e-3
    assert diff(out[1][1][-1], torch.from_numpy(g["pred1_last"])) < 1e-3


def test_warm_start_changes_what_it_should(monkeypatch):
    """Warm equals cold for the first pair of a stream and differs for the later ones."""
    pin_forms(monkeypatch)
    h, w = 128, 160
    cold, _ = make_net(76, final_only=True)
    warm, _ = make_net(76, final_only=True, warm=True)
    for n in (cold, warm):
        n.change_imagesize((h, w))
    v = volumes(1400, 4, h, w)
    with torch.no_grad():
        a, b = cold.forward_stream(v, iters=3), warm.forward_stream(v, iters=3)
        cold.reset_stream()
        warm.reset_stream()
        a0, b0 = cold.forward_stream(v[:2], iters=3), warm.forward_stream(v[:2], iters=3)
    assert same(a0[0][1][0], b0[0][1][0])                               # one pair: the same batch-1 chain
    print("first pair, batch-3 cold loop against the batch-1 warm one:", diff(a[0][1][0], b[0][1][0]))
    assert diff(a[0][1][0], b[0][1][0]) < 1e-4
    for p in (1, 2):
        print(f"pair {p}: warm - cold {diff(a[p][1][0], b[p][1][0]):.3e}")
        assert diff(a[p][1][0], b[p][1][0]) > 1e-2, p


# ---------------------------------------------------------------------------------------------------- refusals
def test_weight_change_and_new_size():
    h, w = 128, 160
    net, _ = make_net(77)
    net.change_imagesize((h, w))
    v = volumes(1500, 3, h, w)
    with torch.no_grad():
        net.forward_stream(v[:2], iters=2)
        net.load_state_dict(net.state_dict())
        with pytest.raises(Exception, match="reset_stream"):
            net.forward_stream(v[2:], iters=2)
        with pytest.raises(Exception, match="reset_stream"):
            net.forward_stream(v[2:], iters=2)
        net.reset_stream()
        assert len(net.forward_stream(v, iters=2)) == 2
        net.change_imagesize((136, 200))                                # a new size resets the carry
        assert pending(net) == 0
        assert len(net.forward_stream(volumes(1600, 2, 136, 200), iters=2)) == 1


# ---------------------------------------------------------------------------------------------------- harness
def test_mvsec_harness_stream(tmp_path, monkeypatch):
    """test_multi_sequence(stream=4) on a synthetic MVSEC sequence prints the one-sample loop's per-sample AEE with a cold ERAFT."""
    from eemflow_amd.harness import Logger, TestRaftEvents
    from eemflow_amd.mvsec import MvsecEventFlow
    pin_forms(monkeypatch)
    n_samples, first = 9, 40
    flow_dir = tmp_path / "dataset" / "MVSEC" / "seqA" / "flowgt_dt1"
    flow_dir.mkdir(parents=True)
    rng = np.random.default_rng(6)
    for i in range(first, first + n_samples):
        np.save(flow_dir / f"{i}.npy", rng.normal(0, 2, (2, 260, 346)).astype(np.float32))

    def reader(path):
        k = int(os.path.basename(path).split(".")[0])
        r = np.random.default_rng(20_000 + k)
        m = 20000
        ts = np.sort(r.uniform(k * 0.05, (k + 1) * 0.05, m))
        return np.stack([ts, r.integers(0, 346, m), r.integers(0, 260, m), r.integers(0, 2, m) * 2 - 1], axis=1).astype(np.float64)

    args = {"eval_type": "sparse", "num_voxel_bins": 5, "sequence": "seqA"}
    ds = MvsecEventFlow(args, train=False, root=str(tmp_path), events_reader=reader, valid_time_index={"seqA": [(first, first + n_samples)]})
    net, _ = make_net(78)
    la, lb = Logger(verbose=False), Logger(verbose=False)
    ref = TestRaftEvents(ds, (256, 256), logger=la).test_multi_sequence(net, sequence_list=["seqA"], stride=1, loader_threads=0)
    got = TestRaftEvents(ds, (256, 256), logger=lb).test_multi_sequence(net, sequence_list=["seqA"], stride=1, stream=4)
    assert len(la.lines) == len(lb.lines)
    assert la.lines == lb.lines, [(a, b) for a, b in zip(la.lines, lb.lines) if a != b][:3]
    assert got == ref
