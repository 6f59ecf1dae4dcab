"""The two forms of the 1/64-grid tail head (csrc/tail_fused.hip) give the same bits.

tail_head_kernel gathers the conv epilogues' pooling partial sums once per tap; tail_head_lds_kernel (batched launches, schedule.hip
tail_head_lds_wanted) pools every value once per block and correlates from LDS.  Each case runs the same inputs through
EEM_TAIL_HEAD_LDS=0 and =1 on a fresh context each (the switch is read when the schedule is built) and requires torch.equal on
cat_1..3 ([cv 53 | r 16]), pool_1..3 and the flow.  Which form ran is read from the launch record (eemflow_time_kernels' block
count of the launch), so a switch that switches nothing fails here: the grids below mirror tail_head_prepare / tail_head_lds_launch.

Grids: 2x3 (every 9x9 window leaves the grid, one ragged 16-pixel tile), 5x7 (three tiles, the last ragged; an odd batch so that
every split of frames or taps over blocks has a remainder; one tensor and five separate buffers), 12x20 (240 cells: the largest the
LDS chunk holds) and 13x20 (refused: =1 falls back)."""
import ctypes

import pytest
import torch

from eemflow_amd import EEMFlow, _lib
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEAD = "tail head: pool+corr53+rconv"
STAGES = ("cat_1", "cat_2", "cat_3", "pool_1", "pool_2", "pool_3")


def cdiv(a, b):
    return -(-a // b)


def old_blocks(batch, g):
    """tail_head_prepare: a box of grid_x x 53 blocks for each of the seven roles"""
    tiles = cdiv(g, 16) * batch
    pool = cdiv(2 * batch * (16 + 32 + 64) * g, 576)
    return max(cdiv(tiles, 9), cdiv(tiles, 53), cdiv(pool, 53)) * 53 * 7


def lds_blocks(batch, g):
    """tail_head_lds_launch: per (frame, stage) five groups of 11 taps and one rconv block per four 16-pixel tiles"""
    return batch * 3 * (cdiv(53, 11) + cdiv(cdiv(g, 16), 4))


def make_net(h, w):
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(41).items()})
    net = net.to(DEV)
    net.change_imagesize((h, w))
    return net


def head_blocks(net, e1, e2):
    """block count of the tail-head launch of a forward of this batch on the module's context (one timed pass)"""
    b, _, h, w = e1.shape
    out = torch.empty(b, 2, h, w, device=DEV)
    st = (_lib.KernelStat * 128)()
    n = ctypes.c_int(0)
    ctx = net._context(e1.device)
    _lib.check(_lib.lib().eemflow_time_kernels(ctx, e1.data_ptr(), e2.data_ptr(), b, h, w, out.data_ptr(), h, w, 1, st, 128,
                                               ctypes.byref(n), _lib.current_stream_ptr(e1.device)))
    torch.cuda.synchronize()
    hit = [st[i].blocks for i in range(n.value) if st[i].name.decode() == HEAD]
    assert len(hit) == 1, [st[i].name.decode() for i in range(n.value)]
    return hit[0]


def run(monkeypatch, mode, e1, e2, many=False):
    """flow, the six stage tensors and the head's block count of one forward under EEM_TAIL_HEAD_LDS=mode (None: unset)"""
    if mode is None:
        monkeypatch.delenv("EEM_TAIL_HEAD_LDS", raising=False)
    else:
        monkeypatch.setenv("EEM_TAIL_HEAD_LDS", mode)
    net = make_net(*e1.shape[-2:])
    with torch.no_grad():
        if many:
            outs = net.forward_many([(e1[i:i + 1].clone(), e2[i:i + 1].clone()) for i in range(e1.shape[0])])
            flow = torch.cat([o[1][0] for o in outs])
        else:
            flow = net(e1, e2)[1][0]
    torch.cuda.synchronize()
    st = {name: net.stage(name).clone() for name in STAGES}
    return flow.clone(), st, head_blocks(net, e1, e2)


def assert_same(a, b, tag):
    assert torch.equal(a[0], b[0]), f"{tag}: flow differs, max {float((a[0] - b[0]).abs().max())}"
    for name in STAGES:
        assert a[1][name].shape == b[1][name].shape
        assert torch.equal(a[1][name], b[1][name]), f"{tag}: {name} differs, max {float((a[1][name] - b[1][name]).abs().max())}"


def inputs(seed, b, h, w):
    return tuple(torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(seed, b, h, w))


def test_grid_2x3_batch4(monkeypatch):
    b, h, w = 4, 128, 192
    e1, e2 = inputs(42, b, h, w)
    old = run(monkeypatch, "0", e1, e2)
    new = run(monkeypatch, "1", e1, e2)
    assert old[2] == old_blocks(b, 6) and new[2] == lds_blocks(b, 6), (old[2], new[2])
    assert float(old[1]["cat_1"][:, :53].abs().max()) > 0 and float(old[0].abs().max()) > 0
    assert_same(old, new, "2x3")


def test_grid_5x7_batch5_one_tensor_and_separate_buffers(monkeypatch):
    b, h, w = 5, 320, 448
    e1, e2 = inputs(43, b, h, w)
    old = run(monkeypatch, "0", e1, e2)
    new = run(monkeypatch, "1", e1, e2)
    # the switch switches: the launch record shows two different grids
    assert old[2] == old_blocks(b, 35) and new[2] == lds_blocks(b, 35) and old[2] != new[2], (old[2], new[2])
    assert_same(old, new, "5x7 forward")
    old_many = run(monkeypatch, "0", e1, e2, many=True)
    new_many = run(monkeypatch, "1", e1, e2, many=True)
    assert_same(old_many, new_many, "5x7 forward_many")
    assert_same(old, old_many, "5x7 old form, one tensor against separate buffers")
    assert_same(new, new_many, "5x7 LDS form, one tensor against separate buffers")
    for i in range(b):
        assert torch.equal(new[0][i], new_many[0][i]) and torch.equal(new_many[0][i], old[0][i]), i


def test_largest_grid_12x20_and_refused_13x20(monkeypatch):
    b = 4
    for h, w, g, accepted in ((768, 1280, 240, True), (832, 1280, 260, False)):
        e1, e2 = inputs(44, b, h, w)
        old = run(monkeypatch, "0", e1, e2)
        new = run(monkeypatch, "1", e1, e2)
        assert old[2] == old_blocks(b, g), (g, old[2])
        assert new[2] == (lds_blocks(b, g) if accepted else old_blocks(b, g)), (g, new[2])     # refused: =1 falls back
        assert_same(old, new, f"g={g}")
        del e1, e2, old, new


def test_threshold_switch_unset(monkeypatch):
    """Unset: one frame alone launches tail_head_kernel's grid (the F(4x4) encoder forms, whose partial sums the LDS form reads, are
    pinned so that only the frame count decides), four frames per launch the LDS form's."""
    monkeypatch.setenv("EEM_WINO4_LAYERS", "7")
    h, w = 128, 192
    for b, want in ((1, old_blocks(1, 6)), (4, lds_blocks(4, 6))):
        e1, e2 = inputs(45, b, h, w)
        assert run(monkeypatch, None, e1, e2)[2] == want, b
    e1, e2 = inputs(45, 1, h, w)
    one_old = run(monkeypatch, "0", e1, e2)
    one_new = run(monkeypatch, "1", e1, e2)                   # forced: supported at one frame too
    assert one_new[2] == lds_blocks(1, 6) and one_old[2] == old_blocks(1, 6)
    assert_same(one_old, one_new, "one frame")
