"""Forward-backward consistency check on the GPU (eemflow_amd.fb_check / eemflow_fb_check_many) against the CPU restatement of the
reference's occ_check_model (tests/fb_reference.py, pinned by tests/golden/fb_check.npz).

A mask is a comparison, so a pixel whose two sides are closer than the arithmetic's round-off may fall either way.  The rule here: a GPU
mask may differ from the fp64 restatement only at pixels whose fp64 margin |len(diff) - thresh| is below 1e-3 (flows of a few pixels
in fp32 carry ~1e-6 of round-off: three orders of room); the test first asserts ON THE RESTATEMENT ALONE that such pixels are at most
0.5 % of the image and that both mask values occur in at least 5 % of the pixels, then exact equality everywhere else.
Needs a real MI355X: `pytest -m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import eemflow_amd
from eemflow_amd import EEMFlow, _lib
from eemflow_amd.metrics import fb_check_many
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair

from fb_reference import MODES, fb_check_margins, fb_check_reference, outgoing, synthetic_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fb_check.npz")
MARGIN = 1e-3
ALPHA = (0.01, 0.5)


def compare_outside_margin(name, got, fw, bw, a1, a2, mode="all", need_both=True):
    """got = (mask_fw, mask_bw) from the GPU, fw / bw the CPU copies of the fp32 flows it was given."""
    want = fb_check_reference(fw.double(), bw.double(), a1, a2, mode)
    margins = fb_check_margins(fw, bw, a1, a2)
    outs = (outgoing(fw.double()), outgoing(bw.double()))
    for d, (g, m, mg, out) in enumerate(zip(got, want, margins, outs)):
        g = g.cpu().double()
        assert g.shape == m.shape
        assert set(torch.unique(g).tolist()) <= {0.0, 1.0}
        near = mg < MARGIN
        if mode == "obj":
            near = near & (out == 1)                       # a leaving pixel is 1 whatever the comparison says
        if mode == "out":
            near = torch.zeros_like(near)                  # no comparison of rounded sums: exact
        share, ones = near.double().mean().item(), m.mean().item()
        differ = int((g != m).sum())
        print(f"{name} dir {d} mode {mode}: within margin {100 * share:.4f} %, consistent {100 * ones:.2f} %, GPU != fp64 at {differ} pixels")
        assert share <= 0.005
        if need_both:
            assert 0.05 <= ones <= 0.95
        assert torch.equal(g[~near], m[~near]), f"{name} dir {d}: {int((g[~near] != m[~near]).sum())} pixels differ outside the margin"


def test_fixture_inputs_in_all_three_modes():
    z = np.load(GOLDEN)
    for k in range(int(z["npairs"])):
        fw, bw = torch.from_numpy(z[f"fw_{k}"]), torch.from_numpy(z[f"bw_{k}"])
        for ai, (a1, a2) in enumerate(z["alphas"]):
            for mode in MODES:
                got = eemflow_amd.fb_check(fw.to(DEV), bw.to(DEV), float(a1), float(a2), mode)
                assert got[0].shape == (1, 1) + fw.shape[2:] and got[0].dtype == torch.float32
                # the fixture's small images and default alphas are mostly one value: the both-values condition is the synthetic pairs'
                compare_outside_margin(f"fixture {k} alphas {ai}", got, fw, bw, float(a1), float(a2), mode, need_both=False)
                if mode == "out":                           # no rounding involved: the reference's own mask, exactly
                    assert np.array_equal(got[0].cpu().numpy().astype(np.uint8), z[f"mask_fw_{k}_{ai}_out"])
                    assert np.array_equal(got[1].cpu().numpy().astype(np.uint8), z[f"mask_bw_{k}_{ai}_out"])
                else:                                        # the fp32 reference may only differ inside the margin too
                    mg = fb_check_margins(fw, bw, float(a1), float(a2))
                    for g, name, m in zip(got, ("fw", "bw"), mg):
                        ref = torch.from_numpy(z[f"mask_{name}_{k}_{ai}_{mode}"].astype(np.float32))
                        far = m >= MARGIN
                        assert torch.equal(g.cpu()[far], ref[far])


@pytest.mark.parametrize("h,w", [(260, 346), (720, 1280)])
@pytest.mark.parametrize("mode", MODES)
def test_synthetic_pair(h, w, mode):
    fw, bw = synthetic_pair(h, w)
    got = eemflow_amd.fb_check(fw.to(DEV), bw.to(DEV), *ALPHA, mode)
    compare_outside_margin(f"synthetic {h}x{w}", got, fw, bw, *ALPHA, mode, need_both=mode == "all")


def model_pair():
    h, w = 260, 346
    sd = seeded_state_dict(61)
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV)
    net.change_imagesize((h, w))
    v = [torch.from_numpy(synthetic_voxel_pair(700 + i, 1, h, w)[0]).to(DEV) for i in range(2)]
    with torch.no_grad():
        (_, pf, pb, masks), = net.forward_stream(v, bidirectional=True, fb_check=ALPHA)
    return pf[0], pb[0], masks


def test_model_pair():
    """The GPU's own two flows of one pair of seeded weights (under 0.4 px: the reference's default alphas would call every pixel
    consistent, hence (0.01, 0.5)); masks from forward_stream(fb_check=) against the restatement on those same flows."""
    fw, bw, masks = model_pair()
    compare_outside_margin("model pair 260x346", masks, fw.cpu(), bw.cpu(), *ALPHA)


def warp(x, flow):
    out = torch.empty_like(x)
    b, c, h, w = x.shape
    _lib.check(_lib.lib().eemplus_warp(x.data_ptr(), flow.data_ptr(), b, c, h, w, 1, out.data_ptr(), _lib.current_stream_ptr(x.device)))
    return out


@pytest.mark.parametrize("h,w", [(260, 346), (720, 1280)])
def test_warped_values_are_those_of_eemplus_warp(h, w):
    """Masks formed on the device from eemplus_warp(mode=1)'s outputs - the remaining steps as separate fp32 tensor operations (no fused
    multiply-add between them, as in the kernel, which is built without contraction) - against the kernel's: the same margin rule, and
    the count of differing pixels printed (0 when the two paths round alike)."""
    fw, bw = (t.to(DEV) for t in synthetic_pair(h, w))
    got = eemflow_amd.fb_check(fw, bw, *ALPHA)

    def length(x):
        return torch.sqrt(x[:, 0:1] * x[:, 0:1] + x[:, 1:2] * x[:, 1:2])
    thresh = ALPHA[0] * (length(fw) + length(bw)) + ALPHA[1]
    via = ((length(fw + warp(bw, fw)) < thresh).float(), (length(bw + warp(fw, bw)) < thresh).float())
    margins = fb_check_margins(fw.cpu(), bw.cpu(), *ALPHA)
    for d in range(2):
        near = (margins[d] < MARGIN).to(DEV)
        print(f"{h}x{w} dir {d}: kernel != masks from eemplus_warp at {int((got[d] != via[d]).sum())} pixels")
        assert near.float().mean().item() <= 0.005
        assert torch.equal(got[d][~near], via[d][~near])


def test_sixteen_pairs_in_one_call_equal_sixteen_single_calls():
    h, w = 260, 346
    base_fw, base_bw = synthetic_pair(h, w)
    g = torch.Generator().manual_seed(3)
    fws = [(base_fw + 0.3 * i + 0.2 * torch.randn(1, 2, h, w, generator=g)).to(DEV) for i in range(16)]
    bws = [(base_bw - 0.3 * i + 0.2 * torch.randn(1, 2, h, w, generator=g)).to(DEV) for i in range(16)]
    many = fb_check_many(fws, bws, *ALPHA)
    assert len(many) == 16
    for i in range(16):
        one, = fb_check_many([fws[i]], [bws[i]], *ALPHA)
        assert torch.equal(many[i][0], one[0]) and torch.equal(many[i][1], one[1]), i
    assert not torch.equal(many[0][0], many[15][0])
    # a batch through the public call is the same sixteen pairs
    bf, bb = eemflow_amd.fb_check(torch.cat(fws), torch.cat(bws), *ALPHA)
    assert bf.shape == (16, 1, h, w)
    for i in range(16):
        assert torch.equal(bf[i:i + 1], many[i][0]) and torch.equal(bb[i:i + 1], many[i][1])


def test_unaligned_sizes_take_the_scalar_path():
    """h * w not a multiple of 4: one pixel per lane; the same masks as the restatement."""
    h, w = 37, 51
    fw, bw = synthetic_pair(h, w)
    got = eemflow_amd.fb_check(fw.to(DEV), bw.to(DEV), *ALPHA)
    compare_outside_margin("synthetic 37x51", got, fw, bw, *ALPHA, need_both=False)


def test_abi_errors():
    L = _lib.lib()
    fw, bw = torch.zeros(1, 2, 8, 8, device=DEV), torch.zeros(1, 2, 8, 8, device=DEV)
    mf, mb = torch.full((1, 1, 8, 8), -1.0, device=DEV), torch.full((1, 1, 8, 8), -1.0, device=DEV)

    def table(t):
        return (ctypes.c_void_p * 17)(*([t.data_ptr()] * 17))       # (only entry 0 is read by the calls that launch)
    afw, abw, amf, amb = table(fw), table(bw), table(mf), table(mb)
    sp = _lib.current_stream_ptr(torch.device(DEV))
    assert L.eemflow_fb_check_many(17, afw, abw, amf, amb, 8, 8, 1.0, 0.05, 0, sp) != 0
    assert L.eemflow_fb_check_many(0, afw, abw, amf, amb, 8, 8, 1.0, 0.05, 0, sp) != 0
    assert L.eemflow_fb_check_many(1, afw, abw, amf, amb, 8, 8, 1.0, 0.05, 3, sp) != 0
    assert b"mode" in L.eemflow_last_error()
    assert L.eemflow_fb_check_many(1, afw, abw, amf, None, 8, 8, 1.0, 0.05, 0, sp) != 0
    assert L.eemflow_fb_check_many(1, afw, abw, amf, amb, 8, 8, 1.0, 0.05, 0, sp) == 0
    torch.cuda.synchronize()
    assert bool((mf == 1).all()) and bool((mb == 1).all())          # zero flows agree everywhere: 0 < alpha2
    with pytest.raises(ValueError):
        eemflow_amd.fb_check(torch.zeros(1, 2, 8, 8, device=DEV), torch.zeros(1, 2, 8, 9, device=DEV))
