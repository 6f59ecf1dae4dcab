"""Batched launches under several frames in flight: the encoder's blocks take SEVERAL tiles each, dealt by the interleaved walk
(conv_wino4.hip, reverse == 3) on the grids of the frames-in-flight hint, and pconv1_1's blocks walk contiguous ranges that cross image
and frame-buffer boundaries (conv_enc1.hip).  Every stage against fp64 under the limits of oracle/fp64_bounds.py (no tolerance of this
module's own), and bitwise between the settings that only change the dealing.  Needs a real MI355X: `pytest -m gpu`.

The helpers are those of tests/test_gpu_stage_fp64.py; the grids, the tiles per block and the checked frames come from the host restatement
of the dealing, tests/test_tile_walk_host.py, which proves the dealing and that these cases reach what they are here for.  Every case pins
EEM_WINO4_LAYERS=7 (F(4x4) on every stride-1 layer at either setting) before the weights load and asserts, from eemflow_time_kernels, the
form and the grid (KernelStat.blocks) of every encoder launch against that restatement - never against a number read back from the library.

CASES (blocks = grid; 1_2 / 2_x / 3_x = the stride-1 F(4x4) layers at C = 16 / 32 / 64; fif = frames_in_flight):
  hint_c16    192x256, batch 16 / 15 / 13, fif 4 (and 1 for the bitwise comparison).  1/2 map 96x128 = 6 tiles of 16x128 per image, T = 192 /
              180 / 156.  fif 4: pconv1_2 on 96 / 96 / 80 blocks (gb = 12 / 12 / 10), every block tiles kb and kb + gb, each step passes
              two whole images, the last XCD's range is short at batch 15 and 13; pconv1_1 on 96 blocks of 8 / 8 / 7 contiguous tiles
              (24 per image: ranges cross images at batch 15 and 13); 2_x 96 / 96 / 80 and 3_x 64 / 64 / 56 blocks of one tile; the
              stride-2 layers one tile per block (768 / 720 / 624 and 192 / 184 / 160).  fif 1: pconv1_1 256, pconv1_2 192 / 184 / 160 blocks
              of one tile.  Batch 16 once as a batch tensor and once as forward_many of 16 single-frame buffers, graph and eager.
              fp64 on frames 0 2 3 6 7 10 11 14 15 (batch 16), 0 2-7 9-11 13 14 (15), 0-3 5 6 8-12 (13): every frame with a second tile.
  many_tiles  64x256, batch 136 (272 images), fif 1 and 4.  T = 544 / 272 / 272 at C = 16 / 32 / 64.  fif 1: every stride-1 layer on 256
              blocks (gb = 32), three tiles per block at C = 16 (kb < 4), two elsewhere; fif 4: pconv1_2 on 272 blocks (gb = 34: more
              blocks per XCD than CUs), pconv1_1 on 96 blocks of 23 tiles (8 per image).  tiles_x = 1: a step of gb wraps 32 / 34 times
              and passes 16 / 17 images at C = 16, 32 at C = 32 / 64.  No launcher refuses batch 136.  fp64 on 17 frames (each XCD's first
              and last image with a later tile, per layer and setting: the full list is all 136); EVERY frame is compared bitwise with
              batch-8 forwards of the same frames, whose blocks take one tile each.
  many_16     320x576 (the smallest padded size at which 32 images give T > 256 at all three widths with more than one tile column:
              T = 960 / 480 / 288), forward_many of 16 frames, fif 1 and 4: 256 blocks per stride-1 layer, pconv1_2 480 under the hint
              (60 per XCD), up to four tiles per block, tiles_x = 3; every frame bitwise between the settings, fp64 on frames 0, 3, 15.
  stream      192x384, forward_stream of 16 windows (the most a call takes), fif 4: 16 images where the pairwise call of the same 15
              pairs has 30 - pconv1_2 96 blocks (gb = 12, tiles_x = 2, two tiles per block) against 184; flows bitwise the pairwise
              forward_many's, whose stages go against fp64 on frames 0-3 5-7 9-11 13 14.  (A stream call's own stages cannot be read;
              its grids are asserted on a forward of 8 pairs = 16 images, the same nimg and enc_batch.)

MEASURED on one MI355X (a record: the limits are those of oracle/fp64_bounds.py and these numbers set none), worst max|z| per family:

    case         enc1   wino4 C=16  C=32   C=64   bx3    pool   corr   rconv  out_conv  upsample
                 a1     f11         b2 f12 b3 f13 a2 a3
    hint_c16     4.47   119         103    79.8   6.91   2.51   3.29   1.88   2.05      2.70
    many_tiles   3.94   150         66.7   43.1   5.31   2.37   2.65   1.47   1.17      1.42
    many_16      4.19   78.6        88.7   47.8   5.72   2.46   2.68   0.84   1.59      2.24
    stream       4.32   191         72.4   49.4   6.54   2.44   2.88   1.43   1.70      1.76
    limit        9.9    430                       14     7.0    7.6    20     4.9       99
  over all cases: wino4 rms(z) 2.04, |mean z| 0.064, |slope| 1.06 u; decoders 1.13 (rms) and 1.37 (max) of the fp32 CPU oracle's error
  (KAPPA_DEC 6.4).  Every bitwise comparison holds; no kernel changed.
Run time of this module alone: 36 s, of which 27 s are the process's first use of the GPU; the slowest test 1.7 s (stream), every other
0.7 - 1.3 s.  tests/test_gpu_stage_fp64.py (54 tests) on the same machine in the same call: 33 s.
"""
import pytest
import torch

from eemflow_amd.weights import synthetic_voxel_pair
from test_gpu_stage_fp64 import DEV, ENC, assert_forms, check_stages, forms_of, launches, make_net, pin
from test_tile_walk_host import CASES, expected_blocks, frames_to_check, later_tiles

pytestmark = pytest.mark.gpu

ENV = {"EEM_WINO4_LAYERS": "7"}
STAGES = ("a1", "f11", "b2", "f12", "b3", "f13")


def assert_launches(net, size, d1, d2, fif):
    """Forms and grids of a forward of these tensors' batch at this setting, from eemflow_time_kernels."""
    b = d1.shape[0]
    net.frames_in_flight = fif
    ks = launches(net, d1, d2, blocks=True)
    assert_forms([k[:2] for k in ks], forms_of(ENV, b, fif), ENV, (size[1] // 2) // 32, b)
    want = expected_blocks(size, 2 * b, fif)
    got = {layer: [n for name, _, n in ks if name.startswith(f"enc.{layer} ")] for _, _, layer, _, _ in ENC}
    assert got == {layer: [n] for layer, n in want.items()}, (fif, got, want)


def encoder_stages(net):
    return {s: net.stage(s).cpu() for s in STAGES}


def assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def batch_case(monkeypatch, name, k, seed, fifs):
    """One batch tensor through `forward` at each setting: grids asserted, fp64 after the first, bitwise between them."""
    size, b = CASES[name]["size"], CASES[name]["launches"][k][1]
    pin(monkeypatch, ENV)
    net, sd = make_net(seed, *size, fif=fifs[0])
    e1, e2 = (torch.from_numpy(a) for a in synthetic_voxel_pair(seed + 1, b, *size))
    d1, d2 = e1.to(DEV), e2.to(DEV)
    runs = []
    with torch.no_grad():
        for fif in fifs:
            assert_launches(net, size, d1, d2, fif)
            flow = net(d1, d2)[1][0].cpu()
            if not runs:
                check_stages(net, sd, e1, e2, flow, forms_of(ENV, b, fif), frames_to_check(name, k), f"{name} b{b} fif{fif}")
            runs.append({"flow": flow, **encoder_stages(net)})
    for other in runs[1:]:
        assert_same(runs[0], other, f"{name} b{b}: frames_in_flight {fifs[0]} against {fifs[1]}")
    return net, (e1, e2), (d1, d2), runs[0]


@pytest.mark.parametrize("k", [0, 1, 2], ids=["b16", "b15", "b13"])
def test_hint_c16_batch(monkeypatch, k):
    batch_case(monkeypatch, "hint_c16", k, 200 + k, (4, 1))


def test_hint_c16_forward_many_graph_eager_replay(monkeypatch):
    """16 single-frame buffers (pconv1_1's ranges read through the per-frame io table): capture, replay, an eager run and the batch
    tensor's forward are bitwise equal; the stages of the forward_many go against fp64."""
    size, n = CASES["hint_c16"]["size"], 16
    pin(monkeypatch, ENV)
    net, sd = make_net(210, *size, fif=4)
    pairs = [tuple(torch.from_numpy(a) for a in synthetic_voxel_pair(211 + i, 1, *size)) for i in range(n)]
    e1, e2 = torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs])
    dev = [(a.to(DEV), b.to(DEV)) for a, b in pairs]
    d1, d2 = e1.to(DEV), e2.to(DEV)
    with torch.no_grad():
        assert_launches(net, size, d1, d2, 4)
        capture = torch.cat([o[1][0] for o in net.forward_many(dev)]).cpu()
        st = encoder_stages(net)
        check_stages(net, sd, e1, e2, capture, forms_of(ENV, n, 4), frames_to_check("hint_c16", 0), "hint_c16 forward_many")
        replay = torch.cat([o[1][0] for o in net.forward_many(dev)]).cpu()
        assert torch.equal(capture, replay)
        assert_same(st, encoder_stages(net), "replay")
        assert torch.equal(capture, net(d1, d2)[1][0].cpu())
        assert_same(st, encoder_stages(net), "batch tensor")
        eager, _ = make_net(210, *size, graph=False, fif=4)
        assert torch.equal(capture, torch.cat([o[1][0] for o in eager.forward_many(dev)]).cpu())
        assert_same(st, encoder_stages(eager), "eager")


def test_many_tiles(monkeypatch):
    """Batch 136: two and three tiles per block, steps that pass 16 to 32 images.  Besides the fp64 frames, every frame's encoder
    stages are bitwise those of batch-8 forwards, in which every block takes one tile."""
    net, _, (d1, d2), big = batch_case(monkeypatch, "many_tiles", 0, 220, (1, 4))
    size, b = CASES["many_tiles"]["size"], 136
    assert max(later_tiles(size, 16, 4)[1].values()) == 1                            # batch 8: T = 32 / 16 / 16, one tile per block
    with torch.no_grad():
        for i in range(0, b, 8):
            net(d1[i:i + 8], d2[i:i + 8])
            for s in STAGES:
                small = net.stage(s).cpu()
                assert torch.equal(small[:8], big[s][i:i + 8]) and torch.equal(small[8:], big[s][b + i:b + i + 8]), (s, i)


def test_many_16(monkeypatch):
    size, n = CASES["many_16"]["size"], 16
    pin(monkeypatch, ENV)
    net, sd = make_net(230, *size, fif=1)
    pairs = [tuple(torch.from_numpy(a) for a in synthetic_voxel_pair(231 + i, 1, *size)) for i in range(n)]
    e1, e2 = torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs])
    dev = [(a.to(DEV), b.to(DEV)) for a, b in pairs]
    d1, d2 = e1.to(DEV), e2.to(DEV)
    runs = []
    with torch.no_grad():
        for fif in (1, 4):
            assert_launches(net, size, d1, d2, fif)
            flow = torch.cat([o[1][0] for o in net.forward_many(dev)]).cpu()
            if fif == 1:
                check_stages(net, sd, e1, e2, flow, forms_of(ENV, n, fif), frames_to_check("many_16"), "many_16 fif1")
            runs.append({"flow": flow, **encoder_stages(net)})
    assert_same(runs[0], runs[1], "many_16: frames_in_flight 1 against 4")


def test_stream_of_16_windows(monkeypatch):
    size, nvol = CASES["stream"]["size"], 16
    pin(monkeypatch, ENV)
    net, sd = make_net(240, *size, fif=4)
    vols = [torch.from_numpy(synthetic_voxel_pair(241 + i, 1, *size)[0]) for i in range(nvol)]
    dv = [v.to(DEV) for v in vols]
    e1, e2 = torch.cat(vols[:-1]), torch.cat(vols[1:])
    with torch.no_grad():
        assert_launches(net, size, torch.cat(dv[:8]), torch.cat(dv[8:]), 4)          # 16 images: the stream call's encoder batch
        assert_launches(net, size, e1.to(DEV), e2.to(DEV), 4)                        # 30 images: the pairwise call's
        stream = [p[1][0] for p in net.forward_stream(dv)]
        net.reset_stream()
        outs = net.forward_many([(dv[i], dv[i + 1]) for i in range(nvol - 1)])
        assert len(stream) == nvol - 1
        for i in range(nvol - 1):
            assert torch.equal(stream[i], outs[i][1][0]), i
        flow = torch.cat([o[1][0] for o in outs]).cpu()
        check_stages(net, sd, e1, e2, flow, forms_of(ENV, nvol - 1, 4), frames_to_check("stream", 1), "stream: pairwise forward_many")
