"""What tests/test_gpu_wino4_vshare.py runs: one forward under EEM_W4_VSHARE=0 and one under =1, the stage tensors and the flow
compared with torch.equal, and the launch record read back (eemflow_time_kernels: the grid and the instantiation tag of the two
64-channel layers), so that a switch that switches nothing fails.  Not collected by pytest (no test_ prefix).

As a program - `python tests/wino4_vshare_worker.py <interleaved|rows>` - it is the CHILD PROCESS of the cases whose switches the
library reads once per process (EEM_ENC_PER_XCD_F64, EEM_WALK3, EEM_COLWALK): the parent test puts them into the child's environment,
so they are set before the library's first 64-channel launch.  192x320, batch 4: the level-3 map is 24x40 = two tile columns (the second
with 8 valid columns) x two tile rows (the second with 8 valid rows) x 8 images = 32 tiles, and EEM_ENC_PER_XCD_F64=1 makes 8 blocks
walk 4 tiles each - the rings, the duty passes and the pooling finish cross tile and image boundaries.  The child checks that grid in
the launch record, compares an inference forward (pconv3_2 plain; pconv3_3 store-free, then stage("f13")'s re-run with stores and
pooling) and one training forward (activations kept), and prints OK."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch                                                                  # noqa: E402

from eemflow_amd import EEMFlow, _lib                                         # noqa: E402
from eemflow_amd.train import EEMFlowTrainer                                  # noqa: E402
from eemflow_amd.weights import seeded_state_dict, synthetic_gt, synthetic_voxel_pair    # noqa: E402

DEV = "cuda:0"
STAGES = ("b3", "f13", "pool_1", "pool_2", "pool_3")
LAYERS = ("enc.pconv3_2 ", "enc.pconv3_3 ")


def make_net(h, w, train=False):
    net = EEMFlow("", groups=5, n_first_channels=5)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(61).items()})
    net.use_graph = False                                          # the switch is read per launch: no cached schedule in between
    net = net.to(DEV)
    net = net.train() if train else net.eval()
    net.change_imagesize((h, w))
    return net


def inputs(seed, b, h, w):
    return tuple(torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(seed, b, h, w))


def launch_record(net, e1, e2):
    """{layer: (blocks, pipe, instantiation tag)} of the two 64-channel layers in a forward of this batch, as the library launches it
    now (one timed pass on the module's context)"""
    b, _, h, w = e1.shape
    out = torch.empty(b, 2, h, w, device=DEV)
    st = (_lib.KernelStat * 128)()
    n = ctypes.c_int(0)
    ctx = net._context(e1.device)
    _lib.check(_lib.lib().eemflow_time_kernels(ctx, e1.data_ptr(), e2.data_ptr(), b, h, w, out.data_ptr(), h, w, 1, st, 128,
                                               ctypes.byref(n), _lib.current_stream_ptr(e1.device)))
    torch.cuda.synchronize()
    rec = {}
    for layer in LAYERS:
        hit = [(st[i].blocks, st[i].pipe, st[i].reserved) for i in range(n.value) if st[i].name.decode().startswith(layer)]
        assert len(hit) == 1, (layer, [st[i].name.decode() for i in range(n.value)])
        rec[layer] = hit[0]
    return rec


def forward(setenv, vshare, e1, e2):
    """flow, the stage tensors and the launch record of one inference forward under EEM_W4_VSHARE=vshare, on a fresh context;
    the record must show F(4x4) (pipe 2) and the form the switch names"""
    setenv("EEM_W4_VSHARE", vshare)
    net = make_net(*e1.shape[-2:])
    with torch.no_grad():
        flow = net(e1, e2)[1][0].clone()
    out = {name: net.stage(name).clone() for name in STAGES}
    torch.cuda.synchronize()
    rec = launch_record(net, e1, e2)
    for layer, (_, pipe, tag) in rec.items():
        assert pipe == 2 and tag == int(vshare), (layer, vshare, pipe, tag)
    return flow, out, rec


def training_forward(setenv, vshare, e1, e2, gt, valid):
    setenv("EEM_W4_VSHARE", vshare)
    net = make_net(*e1.shape[-2:], train=True)
    tr = EEMFlowTrainer(net, lr=0.0, wdecay=0.0, clip=0.0)        # lr 0: the step leaves the weights unchanged
    loss, _, flow = tr.step(e1, e2, gt, valid)
    out = {name: net.stage(name).clone() for name in STAGES}
    torch.cuda.synchronize()
    return flow.clone(), out, loss


def assert_same(old, new, tag):
    assert float(old[1]["b3"].abs().max()) > 1e-3 and float(old[1]["f13"].abs().max()) > 1e-3 and float(old[0].abs().max()) > 0, tag
    for name in STAGES:
        a, b = old[1][name], new[1][name]
        assert a.shape == b.shape and torch.isfinite(a).all()
        assert torch.equal(a, b), f"{tag}: {name} differs at {int((a != b).sum())} of {a.numel()}, max {float((a - b).abs().max())}"
    assert torch.equal(old[0], new[0]), f"{tag}: flow differs, max {float((old[0] - new[0]).abs().max())}"


def child(walk):
    env = os.environ
    assert env.get("EEM_WINO4_LAYERS") == "7" and env.get("EEM_ENC_PER_XCD_F64") == "1", "the parent test sets the child's switches"
    assert (env.get("EEM_WALK3"), env.get("EEM_COLWALK")) == (("0", "0") if walk == "rows" else (None, None)), walk
    b, h, w = 4, 192, 320
    e1, e2 = inputs(64, b, h, w)
    old = forward(env.__setitem__, "0", e1, e2)
    new = forward(env.__setitem__, "1", e1, e2)
    assert old[1]["b3"].shape == (8, 64, 24, 40)
    for rec in (old[2], new[2]):
        assert all(blocks == 8 for blocks, _, _ in rec.values()), rec          # 32 tiles on 8 blocks: four tiles per block
    assert_same(old, new, f"192x320 batch 4, {walk}")
    gt, valid = (torch.from_numpy(a).to(DEV) for a in synthetic_gt(66, b, h, w))
    t_old = training_forward(env.__setitem__, "0", e1, e2, gt, valid)
    t_new = training_forward(env.__setitem__, "1", e1, e2, gt, valid)
    assert_same(t_old, t_new, f"training forward, {walk}")
    assert t_old[2] == t_new[2]
    print(f"OK wino4 vshare {walk}")


if __name__ == "__main__":
    child(sys.argv[1])
