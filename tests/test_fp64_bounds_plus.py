"""The proof that tests/test_gpu_plus_stage_fp64.py would fail on a subtly wrong kernel - on the CPU, with torch alone.

Every reference and criterion that module applies to a recorded launch of eemplus_forward (oracle/fp64_bounds.py: pl_*_ref, `check` under
the form's family, `check_roundings`, `check_decoder`, the bitwise checks) is applied here to

  pass   torch's fp32 evaluation of the same launch on the same inputs, which must sit inside with room to spare;
  fail   an fp32 emulation of the launch with one fault planted at a time: the last 8 of 184 input channels dropped; the dense
         estimator's output written one channel off; the shuffle's j * G + g written as g * per + j; LeakyReLU's slope 0.1 in double;
         one 4 x 32 tile of a Winograd layer off by three units of rounding of its |terms| sum; dec7's residual left out; rconv of
         feature_2; warp weights formed from an unrounded (contracted) position; warp modes 0 and 1 exchanged; the upsampling's su / sv
         exchanged at 12x18 -> 25x37; the coarse flow's doubling lost; one correlation tap exchanged with its neighbour; the blend's m
         and 1 - m exchanged; nonzero flow channels at level 6; the pooled level divided by 2; the warp's position formed by a fused
         multiply-add (on the unfiltered draw of the hostile flows).

and the condition the warp checks rest on: the fp32 tap and mask reference (pl_warp_taps) agrees exactly with F.grid_sample - values
within the derived roundings, `grid_sample(ones) >= 1.0` bit for bit - on every flow the GPU module hands a direct warp check
(pl_hostile_flows with WARP_CASES' seeds).  Shapes are a few tiles each.
"""
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import eemflow_oracle as O
from oracle import eemflow_plus_oracle as P
from oracle import fp64_bounds as B

ROOM = 1.5          # a correct evaluation: every statistic x ROOM inside its limit
FACTOR = 1.5        # a planted fault: some statistic beyond FACTOR x its limit
WARP_CASES = B.PL_WARP_CASES       # (map height, width, seed) of the GPU module's direct warp checks

warnings.filterwarnings("ignore", message="Default grid_sample")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _family_ratios(rec, lim):
    r = [rec["max_z"] / lim.max_z, rec["rms_z"] / lim.rms_z, abs(rec["mean_z"]) / lim.mean_z]
    if rec["n"] >= lim.slope_min_n:
        r.append(abs(rec["slope_u"]) / lim.slope_u)
    return max(r)


def family_passes(name, form, got, ref, mag):
    lim = B.LIMITS[B.pl_form_family(form)]
    rec = B.pl_check_form(name, form, got, ref, mag)
    print(name, {k: round(rec[k], 4) for k in ("max_z", "rms_z", "mean_z", "slope_u")}, lim)
    assert _family_ratios(rec, lim) * ROOM <= 1.0, (name, rec, lim)


def family_rejects(name, form, got, ref, mag):
    lim = B.LIMITS[B.pl_form_family(form)]
    with pytest.raises(B.StageError, match=name):
        B.pl_check_form(name, form, got, ref, mag)
    assert _family_ratios(B.LOG[-1], lim) >= FACTOR, (name, B.LOG[-1], lim)


def roundings_pass(name, got, ref, mag, kind):
    rec = B.check_roundings(name, got, ref, mag, kind)
    print(name, "max|z|", round(rec["max_z"], 4), "of", B.ER_ROUNDINGS[kind])
    return rec


def roundings_reject(name, got, ref, mag, kind):
    with pytest.raises(B.StageError, match=name):
        B.check_roundings(name, got, ref, mag, kind)
    assert B.LOG[-1]["max_z"] >= FACTOR * B.ER_ROUNDINGS[kind], (name, B.LOG[-1])


def kappa_rejects(name, got, ref64, ref32):
    with pytest.raises(B.StageError, match=name):
        B.check_decoder(name, got, ref64, ref32)
    rec = B.LOG[-1]
    floor = B.U * float(ref64.abs().max())
    assert rec["rms_gpu"] >= FACTOR * (B.KAPPA_DEC * rec["rms_cpu"] + floor) or rec["max_gpu"] >= FACTOR * (B.KAPPA_DEC * rec["max_cpu"] + floor), rec


def features(seed, n, c, h, w):
    """Activations as a LeakyReLU leaves them: mostly positive, with a per-channel mean."""
    g = gen(seed)
    return F.leaky_relu(torch.randn(n, c, h, w, generator=g) + torch.randn(1, c, 1, 1, generator=g) * 0.5, 0.1)


def conv_wb(seed, cin, cout, k=3, groups=1):
    w, b = B.seeded_conv(seed, cin // groups, cout, (k, k))
    return w, b + torch.randn(cout, generator=gen(seed + 1)) * 0.05


# ------------------------------------------------------------------------------------------ the dense estimator (criterion 1)
H, W = 13, 37                          # odd, no multiple of 4: one 4 x 32 tile and a cut one beside it, a cut row of tiles below


@pytest.fixture(scope="module")
def dense_case():
    a1, warp_a2 = features(1, 1, 32, H, W), features(2, 1, 32, H, W) * (torch.rand(1, 1, H, W, generator=gen(3)) > 0.2)
    des, ws = [], []
    for i in range(5):
        w, b = conv_wb(10 + i, 64 + sum(B.PL_DE_OUT[:i]), B.PL_DE_OUT[i])
        ws.append((w, b))
        des.append(B.pl_conv_f32(B.pl_dense_input(a1, warp_a2, des), w, b))
    ws.append(conv_wb(20, 184, 3))
    return a1, warp_a2, des, ws


@pytest.mark.parametrize("i,form", [(0, "tail_k3_g16_j2"), (1, "tail_k3_g25_j1"), (2, "tail_k3_g46_j1"), (3, "gconv16_3x3_th4_wm1_kg1"),
                                    (4, "fewout_k8_c8"), (5, "wnc32_m16")])
def test_dense_estimator_passes(dense_case, i, form):
    a1, warp_a2, des, ws = dense_case
    x = B.pl_dense_input(a1, warp_a2, des[:i])
    assert x.shape[1] == (64, 96, 128, 160, 176, 184)[i]
    ref, mag = B.pl_conv_ref(x, *ws[i], act=i < 5)
    got = B.pl_conv_f32(x, *ws[i], act=i < 5)
    family_passes(f"de{i}", form, got, ref, mag)
    if i < 5:
        B.pl_check_leaky(f"de{i}", got)


def test_dense_estimator_last_channels_dropped(dense_case):
    """The 184-channel head reads 176: the slice [8, 184) instead of [0, 184) - de4's eight channels never arrive."""
    a1, warp_a2, des, ws = dense_case
    x = B.pl_dense_input(a1, warp_a2, des)
    w, b = ws[5]
    ref, mag = B.pl_conv_ref(x, w, b, act=False)
    faulty = F.conv2d(x[:, 8:], w[:, 8:], b, padding=1)
    family_rejects("l5.xout", "tail_k3_g46_j1", faulty, ref, mag)
    family_rejects("l5.xout", "wnc32_m16", faulty, ref, mag)
    faulty = F.conv2d(x[:, :176], w[:, :176], b, padding=1)           # (the same at the other end of the weight's K: warp_a2's last 8)
    family_rejects("l5.xout", "tail_k3_g46_j1", faulty, ref, mag)


def test_dense_estimator_output_one_channel_off(dense_case):
    """de2 writes its 32 channels at offset 25 instead of 24: the stage read back at [24, 56) holds de3's last channel and 31 of de2's."""
    a1, warp_a2, des, ws = dense_case
    x = B.pl_dense_input(a1, warp_a2, des[:2])
    ref, mag = B.pl_conv_ref(x, *ws[2])
    buf = B.pl_dense_buffer(a1, warp_a2, des)
    good = buf[:, B.PL_DE_OFF[2]:B.PL_DE_OFF[2] + 32].clone()
    family_passes("l4.de2", "tail_k3_g46_j1", good, ref, mag)
    buf[:, B.PL_DE_OFF[2] + 1:B.PL_DE_OFF[2] + 33] = des[2]
    family_rejects("l4.de2", "tail_k3_g46_j1", buf[:, B.PL_DE_OFF[2]:B.PL_DE_OFF[2] + 32], ref, mag)


def test_leaky_slope_in_double(dense_case):
    """v * 0.1 with the slope a double: a relative 0.25 u on the negative outputs, beneath every family's limits - the sums' check
    passes it, the bitwise image check (pl_check_leaky) does not."""
    a1, warp_a2, des, ws = dense_case
    x = B.pl_dense_input(a1, warp_a2, des[:1])
    w, b = ws[1]
    pre = F.conv2d(x, w, b, padding=1)
    faulty = torch.where(pre >= 0, pre, (pre.double() * 0.1).float())
    ref, mag = B.pl_conv_ref(x, w, b)
    B.pl_check_form("l3.de1", "tail_k3_g25_j1", faulty, ref, mag)                       # (invisible to criterion 1)
    with pytest.raises(B.StageError, match="l3.de1"):
        B.pl_check_leaky("l3.de1", faulty)
    assert B.LOG[-1]["differ"] >= 0.02 * B.LOG[-1]["n"], B.LOG[-1]
    B.pl_check_leaky("l3.de1", torch.where(pre >= 0, pre, pre * torch.tensor(0.1)))


def test_winograd_tile_off(dense_case):
    """One 4 x 32 tile of a Winograd launch 3 u of its |terms| sum high (a transform constant off by rounding): 8 % of the map, seen
    in the mean; the failure names a tile of the form's 4 x 32 tiling."""
    a1, warp_a2, des, ws = dense_case
    x = B.pl_dense_input(a1, warp_a2, des[:1])
    ref, mag = B.pl_conv_ref(x, *ws[1])
    got = B.pl_conv_f32(x, *ws[1])
    family_passes("l2.de1", "wnc32", got, ref, mag)
    faulty = got.double()
    faulty[:, :, 4:8, 0:32] += 3 * B.U * mag[:, :, 4:8, 0:32]
    with pytest.raises(B.StageError, match=r"l2\.de1 \[wnc32\].*tile \(row \d, col \d\) of 4x32"):
        B.pl_check_form("l2.de1", "wnc32", faulty.float(), ref, mag)
    family_rejects("l2.de1", "wnc32", faulty.float(), ref, mag)


# -------------------------------------------------------------------------------------------------- the decoder (criterion 1)
@pytest.fixture(scope="module")
def decoder_case():
    f1, f2 = features(30, 1, 64, H, W), features(31, 1, 64, H, W)
    corr = O.local_corr53(f1, f2)
    wr = conv_wb(32, 64, 32)
    rconv = B.pl_conv_f32(f1, *wr)
    flow_up = torch.randn(1, 2, H, W, generator=gen(33)) * 2
    return f1, f2, corr, wr, rconv, flow_up


def test_decoder_layers_pass(decoder_case):
    f1, f2, corr, wr, rconv, flow_up = decoder_case
    x = B.pl_cat_input(corr, rconv, flow_up)
    assert x.shape[1] == 87
    w1 = conv_wb(40, 87, 96)
    d0 = B.pl_conv_f32(x, *w1)
    family_passes("dec1", "tail_k3_g25_j1", d0, *B.pl_conv_ref(x, *w1))
    for G, form in ((3, "tail_k3_g8_j3"), (1, "tail_k3_g25_j1")):
        wg = conv_wb(41, 96, 96, groups=G)
        family_passes(f"decg0 G={G}", form, B.pl_conv_f32(d0, *wg, groups=G), *B.pl_conv_ref(d0, *wg, groups=G))
    w7 = conv_wb(44, 32, 2)
    t32 = features(45, 1, 32, H, W)
    family_passes("flow", "tail_k3_g8_j1", B.pl_conv_f32(t32, *w7, act=False, res=flow_up), *B.pl_conv_ref(t32, *w7, act=False, res=flow_up))
    family_passes("rconv", "tail_k3_g16_j2", rconv, *B.pl_conv_ref(f1, *wr))


def test_decoder_shuffle_not_applied(decoder_case):
    """Group g's output j left at g * per + j (no channel_shuffle) instead of j * G + g."""
    d0 = features(50, 1, 96, H, W)
    wg = conv_wb(41, 96, 96, groups=3)
    ref, mag = B.pl_conv_ref(d0, *wg, groups=3)
    faulty = F.leaky_relu(F.conv2d(d0, *wg, padding=1, groups=3), 0.1)
    family_rejects("l3.decg1", "tail_k3_g8_j3", faulty, ref, mag)
    assert torch.equal(faulty[:, 0], B.pl_conv_f32(d0, *wg, groups=3)[:, 0])        # (channel 0 = group 0's output 0 either way)


def test_decoder_residual_left_out(decoder_case):
    flow_up = decoder_case[5]
    w7 = conv_wb(44, 32, 2)
    t32 = features(45, 1, 32, H, W)
    ref, mag = B.pl_conv_ref(t32, *w7, act=False, res=flow_up)
    family_rejects("l4.flow", "tail_k3_g8_j1", B.pl_conv_f32(t32, *w7, act=False), ref, mag)


def test_rconv_of_feature_2(decoder_case):
    f1, f2, corr, wr, rconv, flow_up = decoder_case
    ref, mag = B.pl_conv_ref(f1, *wr)
    family_rejects("l5.rconv", "tail_k3_g16_j2", B.pl_conv_f32(f2, *wr), ref, mag)


def test_level6_flow_channels(decoder_case):
    """Channels 85..86 of level 6's decoder input are zeros, bit for bit: a stale value (or -0.0) is rejected."""
    z = torch.zeros(2, 2, 2, 3)
    B.check_bitwise("l6.cat_flow", z, torch.zeros_like(z))
    for v in (1e-30, -0.0):
        bad = z.clone()
        bad[1, 1, 1, 2] = v
        with pytest.raises(B.StageError, match="l6.cat_flow"):
            B.check_bitwise("l6.cat_flow", bad, torch.zeros_like(z))


# ------------------------------------------------------------------------------------------- correlation, pooling (criterion 1)
def test_correlation_passes_and_tap_exchanged(decoder_case):
    f1, f2, corr, *_ = decoder_case
    ref, mag = B.corr53_ref(f1, f2)
    for form in ("corr_direct", "corr_tiled53"):
        family_passes("l3.corr", form, corr, ref, mag)
    faulty = corr.clone()
    faulty[:, [20, 21]] = corr[:, [21, 20]]                              # taps 22 and 23 of the 9 x 9 window: horizontal neighbours
    family_rejects("l3.corr", "corr_direct", faulty, ref, mag)


def test_pooling_passes_and_wrong_divisor():
    f = features(60, 2, 64, 7, 9)                                        # odd both ways: the last row and column fall outside every window
    ref, mag = B.avg_pool_ref(f, 2)
    got = F.avg_pool2d(f, 2, 2)
    family_passes("pool4", "pool2x3", got, ref, mag)
    roundings_pass("pool4", got, ref, mag, "pool")
    family_rejects("pool4", "pool2x3", got * 2, ref, mag)                 # (a + b + c + d) / 2
    roundings_reject("pool4", got * 2, ref, mag, "pool")


# -------------------------------------------------------------------------------------------------------- the warps (criterion 2)
def warp_emulated(x, flow, mode, fault=None):
    """warp_kernel in fp32: pl_warp_taps' taps (or, fault "contracted": weights taken from the UNROUNDED position, as a fused
    multiply-add forms them), the blend ((v0 nw + v1 ne) + v2 sw) + v3 se, times the mode-2 mask."""
    t = B.pl_warp_taps(flow, mode)
    b, c, h, w = x.shape
    if fault == "fused_position":
        # ix = fma(xn + 1, w / 2, -0.5): the product unrounded into the subtraction, everything behind it as the model has it
        f = flow.float()
        px = torch.arange(w, dtype=torch.float32).view(1, 1, w).expand(b, h, w)
        py = torch.arange(h, dtype=torch.float32).view(1, h, 1).expand(b, h, w)
        xn = 2.0 * (px + f[:, 0]) / torch.tensor(float(max(w - 1, 1))) - 1.0
        yn = 2.0 * (py + f[:, 1]) / torch.tensor(float(max(h - 1, 1))) - 1.0
        ix, iy = ((xn + 1.0).double() * (w / 2.0) - 0.5).float(), ((yn + 1.0).double() * (h / 2.0) - 0.5).float()
        xw, yn0 = ix.floor(), iy.floor()
        ww, wn = ix - xw, iy - yn0
        we, ws = 1.0 - ww, 1.0 - wn
        wts = (ws * we, ws * ww, wn * we, wn * ww)
        x0, y0 = xw.clamp(-2.0, w + 1.0).long(), yn0.clamp(-2.0, h + 1.0).long()
        t = dict(t, x=(x0, x0 + 1, x0, x0 + 1), y=(y0, y0, y0 + 1, y0 + 1))
        t["ok"] = tuple((t["y"][i] >= 0) & (t["y"][i] < h) & (t["x"][i] >= 0) & (t["x"][i] < w) for i in range(4))
        o = [t["ok"][i].float() * wts[i] for i in range(4)]
        mask = ((((o[0] + o[1]) + o[2]) + o[3]) >= 1.0) if mode == 2 else t["mask"]
    elif fault == "contracted":
        f = flow.float()
        px = torch.arange(w, dtype=torch.float32).view(1, 1, w).expand(b, h, w)
        py = torch.arange(h, dtype=torch.float32).view(1, h, 1).expand(b, h, w)
        xn = 2.0 * (px + f[:, 0]) / torch.tensor(float(max(w - 1, 1))) - 1.0
        yn = 2.0 * (py + f[:, 1]) / torch.tensor(float(max(h - 1, 1))) - 1.0
        ixd, iyd = (xn + 1.0).double() * (w / 2.0) - 0.5, (yn + 1.0).double() * (h / 2.0) - 0.5
        ww, wn = (ixd - ixd.float().floor().double()).float(), (iyd - iyd.float().floor().double()).float()
        we, ws = 1.0 - ww, 1.0 - wn
        wts = (ws * we, ws * ww, wn * we, wn * ww)
        o = [t["ok"][i].float() * wts[i] for i in range(4)]
        mask = ((((o[0] + o[1]) + o[2]) + o[3]) >= 1.0) if mode == 2 else t["mask"]
    else:
        wts, mask = t["w"], t["mask"]
    bi = torch.arange(b).view(b, 1, 1)
    v = []
    for i in range(4):
        g = x[bi, :, t["y"][i].clamp(0, h - 1), t["x"][i].clamp(0, w - 1)].permute(0, 3, 1, 2)
        v.append(torch.where(t["ok"][i][:, None], g, torch.zeros(())) * wts[i][:, None])
    return (((v[0] + v[1]) + v[2]) + v[3]) * mask[:, None]


@pytest.fixture(scope="module", params=WARP_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def warp_case(request):
    h, w, seed = request.param
    flow = B.pl_hostile_flows(h, w, seed)
    x = torch.rand(flow.shape[0], 5, h, w, generator=gen(seed)) + 0.5          # positive: the applied mask shows in the output (pl_mask_of)
    return x, flow


def test_hostile_flows_hold_what_they_promise(warp_case):
    x, flow = warp_case
    h, w = x.shape[-2:]
    assert torch.equal(flow[0], flow[0].round()) and bool(((flow[1] * 2) % 2 == 1).all())
    assert bool(B.pl_position_is_plain(flow).all())
    m = B.pl_warp_taps(flow, 2)["mask"]
    assert 0.1 < float(m.float().mean()) < 0.9 and bool(m[3].any()) and bool((~m[3]).any())    # (image 3: the borders in mode 2's coordinates)
    inside0 = torch.stack(B.pl_warp_taps(flow, 0)["ok"]).all(0)[2]                               # (image 2: in mode 0's)
    assert bool(inside0.any()) and bool((~inside0).any())
    assert not bool(m[4][flow[4].abs().amax(0) > 1e3].any())
    assert h * w % 256 != 0                                                  # the last block of pixels is partial


def test_tap_reference_is_grid_samples(warp_case):
    """The CONDITION of the warp checks: on every flow the GPU module hands a direct warp check, the fp32 tap reference is
    F.grid_sample's - the mask `grid_sample(ones) >= 1.0` bit for bit, the three warps within the blend's four roundings."""
    x, flow = warp_case
    taps = B.pl_warp_taps(flow, 2)
    ones = F.grid_sample(torch.ones_like(x), P._grid(x, flow))
    assert torch.equal(taps["mask"], (ones >= 1.0)[:, 0])
    assert torch.equal(taps["mask"], (ones >= 1.0).all(1))
    for mode, fn in ((0, P.warp_align_true), (1, P.torch_warp), (2, P.warping_layer_no_div)):
        got = fn(x, flow)
        B.pl_check_warp(f"warp mode {mode}", got, x, flow, mode)
        if mode == 2:
            assert torch.equal(B.pl_mask_of(got), taps["mask"])
        got = warp_emulated(x, flow, mode)
        B.pl_check_warp(f"warp emulated mode {mode}", got, x, flow, mode)


def test_warp_weights_contracted(warp_case):
    """Weights from the unrounded position: beside integer positions a neighbour gets a weight of 1e-7 where the model gives 0, and the
    weights' sum - the mask - flips."""
    x, flow = warp_case
    got = warp_emulated(x, flow, 2, fault="contracted")
    assert not torch.equal(B.pl_mask_of(got), B.pl_warp_taps(flow, 2)["mask"])
    with pytest.raises(B.StageError, match="l3.warp_a2"):
        B.pl_check_warp("l3.warp_a2", got, x, flow, 2)


@pytest.mark.parametrize("h,w,seed", WARP_CASES[:1], ids=["25x37"])       # (the 6x9 map's 15 such pixels move no output past a bound)
def test_position_contracted_shows_on_unfiltered_flows(h, w, seed):
    """A kernel that contracts ix = (xn + 1) (w / 2) - 0.5 is the model's own on the flows drawn build-independent (they cannot see
    it); on the first draw as it is (plain_only=False), which the GPU module checks against pl_warp_taps alone, it is rejected."""
    x = torch.rand(6, 5, h, w, generator=gen(seed)) + 0.5
    flow = B.pl_hostile_flows(h, w, seed)
    for mode in (1, 2):
        assert torch.equal(warp_emulated(x, flow, mode, fault="fused_position"), warp_emulated(x, flow, mode))
    raw = B.pl_hostile_flows(h, w, seed, plain_only=False)
    assert not bool(B.pl_position_is_plain(raw).all())
    rejected = set()
    for mode in (1, 2):
        B.pl_check_warp("plain", warp_emulated(x, raw, mode), x, raw, mode)
        try:
            B.pl_check_warp("fused", warp_emulated(x, raw, mode, fault="fused_position"), x, raw, mode)
        except B.StageError:
            rejected.add(mode)
    assert rejected == {1, 2}, rejected


def test_warp_modes_exchanged(warp_case):
    x, flow = warp_case
    for want, ran in ((0, 1), (1, 0)):
        with pytest.raises(B.StageError, match="l2.fw"):
            B.pl_check_warp("l2.fw", warp_emulated(x, flow, ran), x, flow, want)
        assert B.LOG[-1]["max_z"] >= FACTOR * B.ER_ROUNDINGS["warp"]


# ---------------------------------------------------------------------------------- flow upsampling and the doubling (criterion 2)
def test_upsampling_passes_and_rates_exchanged():
    c = torch.randn(2, 2, 12, 18, generator=gen(70)) * 3
    for out_hw in ((25, 37), (24, 36), (194, 290)):
        ref, mag = B.pl_upflow_ref(c, out_hw)
        got = P.upsample2d_flow_as(c.clone(), out_hw, if_rate=True)
        roundings_pass(f"flow_init {out_hw}", got, ref, mag, "upflow_rate")
        ref0, mag0 = B.pl_upflow_ref(c, out_hw, rate=False)
        roundings_pass(f"upflow {out_hw}", F.interpolate(c, list(out_hw), mode="bilinear", align_corners=True), ref0, mag0, "upflow")
    out_hw = (25, 37)                                                     # 25 / 12 != 37 / 18
    ref, mag = B.pl_upflow_ref(c, out_hw)
    su, sv = B.pl_rate(out_hw, (12, 18))
    assert su != sv
    plain = F.interpolate(c, list(out_hw), mode="bilinear", align_corners=True)
    faulty = torch.cat([plain[:, :1] * sv, plain[:, 1:] * su], 1)
    roundings_reject("l4.flow_init", faulty, ref, mag, "upflow_rate")


def test_coarse_doubling_passes_and_lost():
    c = torch.randn(2, 2, 12, 18, generator=gen(71)) * 3
    ref, mag = B.pl_scale_ref(c, (25, 37))
    after = c.clone()
    P.upsample2d_flow_as(after, (25, 37), if_rate=True)                  # scales `after` in place
    roundings_pass("coarse_scaled", after, ref, mag, "scale")
    roundings_reject("l4.coarse_scaled", c, ref, mag, "scale")           # the swap with flow_alt forgotten: the plain coarse flow stays


# ------------------------------------------------------------------------------------------------ the sigmoid blend (criterion 3)
def test_blend_passes_and_mask_exchanged():
    h, w = 25, 37
    g = gen(80)
    fi = torch.randn(2, 2, h, w, generator=g) * 4
    xout = torch.cat([torch.randn(2, 2, h, w, generator=g) * 1.5, torch.randn(2, 1, h, w, generator=g) * 2], 1)
    ref64, ref32 = B.pl_warp_blend_refs(fi, xout)
    # the kernel's way: the emulated mode-1 warp, 1 / (1 + exp(-m)), then warped (1 - mk) + flow_init mk in fp32
    mk = 1.0 / (1.0 + torch.exp(-xout[:, 2:3]))
    warped = warp_emulated(fi, xout[:, :2], 1)
    rec = B.check_decoder("flow_up", warped * (1.0 - mk) + fi * mk, ref64, ref32)
    assert rec["rms_ratio"] * ROOM <= B.KAPPA_DEC and rec["max_ratio"] * ROOM <= B.KAPPA_DEC, rec
    kappa_rejects("l3.flow_up", warped * mk + fi * (1.0 - mk), ref64, ref32)
    # the separate blend launch on a recorded warp
    r64, r32 = B.pl_blend_ref(warped, fi, xout), B.pl_blend_ref(warped, fi, xout, torch.float32)
    B.check_decoder("flow_up (blend)", warped * (1.0 - mk) + fi * mk, r64, r32)
    kappa_rejects("l3.flow_up", warped * mk + fi * (1.0 - mk), r64, r32)


# ------------------------------------------------------------------------------------------------------------- the form tables
def test_form_tables():
    assert B.pl_base_form("tail_k3_g46_j2") == ("tail_k3_g46", 2) and B.pl_base_form("tail_multi_j3") == ("tail_multi", 3)
    assert B.pl_base_form("gconv16_3x3_th4_wm4_kg1") == ("gconv16_3x3_th4_wm4_kg1", 1)
    assert B.pl_form_family("tail_k1_g2_j2") == "direct" and B.pl_form_family("wnc64_m16") == "wino2" and B.pl_form_family("fewout_k8_c8") == "direct"
    assert B.pl_tile("wnc64") == (4, 64) and B.pl_tile("gconv16_3x3_th6_wm4_kg1") == (6, 16) and B.pl_tile("tail_k3_g5_j3") is None
    with pytest.raises(KeyError):
        B.pl_form_family("tail_k3_g7_j1")
    assert all(f in B.LIMITS for f in set(B.PL_FORM_FAMILY.values()))
    assert not (set(B.PL_FORM_FAMILY) & B.PL_OTHER_FORMS)
