"""The two forms of the 64-channel F(4x4,3x3) kernel (csrc/conv_wino4.hip) give the same bits.

In the shared-V form a tile group's input transform V = B^T d B is computed once, a k-step ahead (two of the group's four waves,
half the Winograd rows each), and handed to the four waves through LDS (three raw input slots, two U slots, two V slots); in the
other form every wave computes it for itself.  Every V value comes from the same expressions and every accumulator sees the same MFMA
sequence, so EEM_W4_VSHARE=1 against =0 (read per launch) is compared with torch.equal, no tolerance: b3 (pconv3_2: plain epilogue,
no pooling), f13 (pconv3_3: the store-free launch of the forward, then stage("f13")'s re-run with stores and pooling), the three
pooled maps and the flow.  Every forward also reads back the launch record: both layers on F(4x4) and on the form the switch names
(tests/wino4_vshare_worker.py holds the comparison).

F(4x4) is pinned on every stride-1 layer (EEM_WINO4_LAYERS=7).  In this process, at the library's default grid (one block per CU) and
tile walk:
  64x64, batch 4      one partial tile per image, one tile per block: prologue and last-step paths only
  64x64, batch 1      two tiles for a grid of eight blocks: six blocks leave before their first barrier
  192x320, batch 33   66 images x 4 tiles = 264 tiles for 256 blocks: one block per XCD walks on to a second tile, of another image
In a fresh child process each, because EEM_ENC_PER_XCD_F64, EEM_WALK3 and EEM_COLWALK are read once per process - the child gets them
in its environment, before its first launch:
  192x320, batch 4    32 tiles (partial in both directions) on 8 blocks of 4 tiles each (the child checks the grid in the launch record),
                      under the interleaved walk and in row order (EEM_WALK3=0 EEM_COLWALK=0): an inference forward and a training
                      forward (activations kept: pconv3_3 with stores and pooling)."""
import os
import subprocess
import sys

import pytest

from wino4_vshare_worker import assert_same, forward, inputs

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "wino4_vshare_worker.py")


@pytest.fixture
def pinned(monkeypatch):
    monkeypatch.setenv("EEM_WINO4_LAYERS", "7")
    return monkeypatch


def test_one_partial_tile_per_block(pinned):
    e1, e2 = inputs(62, 4, 64, 64)
    assert_same(forward(pinned.setenv, "0", e1, e2), forward(pinned.setenv, "1", e1, e2), "64x64 batch 4")


def test_blocks_without_a_tile(pinned):
    e1, e2 = inputs(63, 1, 64, 64)
    old, new = forward(pinned.setenv, "0", e1, e2), forward(pinned.setenv, "1", e1, e2)
    assert all(blocks == 8 for blocks, _, _ in new[2].values()), new[2]           # two tiles, eight blocks
    assert_same(old, new, "64x64 batch 1")


def test_a_second_tile_of_another_image_by_shape(pinned):
    e1, e2 = inputs(67, 33, 192, 320)
    assert_same(forward(pinned.setenv, "0", e1, e2), forward(pinned.setenv, "1", e1, e2), "192x320 batch 33")


@pytest.mark.parametrize("walk", ["interleaved", "rows"])
def test_four_tiles_per_block_in_a_fresh_process(walk):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EEM_") or k in ("EEM_LIB_PATH",)}
    env.update({"EEM_WINO4_LAYERS": "7", "EEM_ENC_PER_XCD_F64": "1"})
    if walk == "rows":
        env.update({"EEM_WALK3": "0", "EEM_COLWALK": "0"})
    r = subprocess.run([sys.executable, WORKER, walk], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and f"OK wino4 vshare {walk}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
