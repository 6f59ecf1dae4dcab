"""The proof that tests/test_gpu_ops_fp64.py would fail on a subtly wrong kernel - on the CPU, with torch alone.

For four of that module's shapes an emulated result goes through the same references (oracle/fp64_bounds.py: op_conv_ref, op_dgrad_ref,
op_wgrad_ref), the same `check_form` and the same form -> family table as a GPU result would:

  pass   torch's fp32 convolution / data gradient / weight gradient; the exact three-piece emulation (operands as three bf16 pieces -
         which is every bit of an fp32 - products and sums in fp64, one rounding to fp32 at the end)
  fail   operands cut to two bf16 pieces; one tap dropped in the last column of one ragged tile; the result scaled by 1 + 3 u; two input
         segments swapped in the weight layout; a weight gradient missing one image; a dw slice written one channel off; a stride-2 data
         gradient with one parity class zeroed; `+=` replaced by `=`

Every passing case asserts through `_passes`, whose message carries the four statistics and the family's limits, and requires ROOM x the
statistic <= the limit (the fp32 evaluation must sit inside with room to spare); every fault must be outside a limit by FACTOR.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import fp64_bounds as B

ROOM = 1.5          # a correct emulation: every statistic x ROOM inside its limit
FACTOR = 1.5        # a planted fault: some statistic beyond FACTOR x its limit (most are beyond it by orders of magnitude)


def _f32(t):
    return torch.as_tensor(t).detach().float()


def _stats_line(rec, lim):
    return (f"{rec['name']} [{rec['form']}]: max|z| {rec['max_z']:.3g} / {lim.max_z}, rms {rec['rms_z']:.3g} / {lim.rms_z}, "
            f"|mean| {abs(rec['mean_z']):.3g} / {lim.mean_z}, |slope| {abs(rec['slope_u']):.3g} / {lim.slope_u} u over {rec['n']} values")


def _ratios(rec, lim):
    r = [rec["max_z"] / lim.max_z, rec["rms_z"] / lim.rms_z, abs(rec["mean_z"]) / lim.mean_z]
    if rec["n"] >= lim.slope_min_n:
        r.append(abs(rec["slope_u"]) / lim.slope_u)
    return r


def _passes(name, form, got, ref, mag, tile=None):
    lim = B.LIMITS[B.form_family(form)]
    rec = B.check_form(name, form, got, ref, mag, tile=tile)
    line = _stats_line(rec, lim)
    print(line)
    assert max(_ratios(rec, lim)) * ROOM <= 1.0, "no room to spare: " + line
    return rec


def _rejected(name, form, got, ref, mag, tile=None):
    lim = B.LIMITS[B.form_family(form)]
    with pytest.raises(B.StageError) as e:
        B.check_form(name, form, got, ref, mag, tile=tile)
    rec = B.LOG[-1]
    line = _stats_line(rec, lim)
    print("rejected: " + line)
    assert max(_ratios(rec, lim)) >= FACTOR, "a fault this close to the limits proves nothing: " + line
    return str(e.value)


# -------------------------------------------------------------------------------------------------------------- the emulations
def pieces(x, n):
    """The sum of the first n bf16 pieces of an fp32 tensor, each piece the top 16 bits of what is left (gconvb.hip: gconvb_pack) -
    in fp64, exactly.  Three pieces are all 24 bits of the mantissa."""
    rest = _f32(x).clone()
    total = torch.zeros_like(rest, dtype=torch.float64)
    for _ in range(n):
        p = (rest.view(torch.int32) & -65536).view(torch.float32)
        total += p.double()
        rest = rest - p
    return total


def conv_pieces(xs, w, b, n, **kw):
    """Operands as n bf16 pieces, products and sums in fp64, the result rounded to fp32 once."""
    ref, _ = B.op_conv_ref([pieces(x, n) for x in xs], pieces(w, n), b, **kw)
    return ref.float()


def conv_f32(xs, w, b, stride=1, padding=(1, 1), act=B.ACT_NONE, out_scale=1.0):
    y = F.conv2d(torch.cat([_f32(x) for x in xs], 1), _f32(w), _f32(b) if b is not None else None, stride=stride, padding=tuple(padding))
    if act == B.ACT_RELU:
        y = y.clamp_min(0.0)
    elif act == B.ACT_LEAKY:
        y = torch.where(y >= 0, y, y * torch.tensor(B.LEAKY, dtype=torch.float32))
    return y * torch.tensor(out_scale, dtype=torch.float32)


def dgrad_f32(dy, w, in_hw, stride, padding, ci0=0, cic=None):
    w = _f32(w)
    cic = w.shape[1] - ci0 if cic is None else cic
    return torch.nn.grad.conv2d_input((dy.shape[0], cic, *in_hw), w[:, ci0:ci0 + cic].contiguous(), _f32(dy), stride=stride, padding=tuple(padding))


def wgrad_f32(xs, dy, wshape, stride, padding, ci0=0):
    """(dw, db) as the ABI leaves them in a zeroed dw of shape wshape: the columns [ci0, ci0 + c) written."""
    x = torch.cat([_f32(t) for t in xs], 1)
    c = x.shape[1]
    dw = torch.zeros(*wshape)
    dw[:, ci0:ci0 + c] = torch.nn.grad.conv2d_weight(x, (wshape[0], c, *wshape[2:]), _f32(dy), stride=stride, padding=tuple(padding))
    return dw, _f32(dy).sum((0, 2, 3))


# ---------------------------------------------------------------------------------------------------------------------- shapes
# (name, input segments, cout, (kh, kw), stride, n, h, w, forward form, tile, data-gradient form, weight-gradient forms (fp32 MFMA / bf16 pieces / ring))
SHAPES = {
    # E-RAFT's 128 -> 128 3x3 layers; 72 columns: the fifth 16-column tile is half
    "res3x3": dict(cs=[128], cout=128, k=(3, 3), stride=1, n=1, h=50, wd=72, fwd=("gconv16_3x3_th2_wm4_kg2", "gconvb_3x3_th2"), tile=(2, 16),
                   wgrad=("wgrad_wide_fp32_tw16_3x3", "wgrad_wide_bx3_tw16_3x3", "wgrad_ring_6464")),
    # the GRU's (1, 5) conv over [h | inp | motion]
    "gru1x5": dict(cs=[128, 128, 128], cout=128, k=(1, 5), stride=1, n=2, h=30, wd=40, fwd=("gconv16_1x5_th2_wm4_kg2", "gconvb_1x5_th2"), tile=(2, 16),
                   wgrad=("wgrad_wide_fp32_tw16_1x5+wgrad_wide_fp32_tw16_1x5+wgrad_wide_fp32_tw16_1x5",
                          "wgrad_wide_bx3_tw16_1x5+wgrad_wide_bx3_tw16_1x5+wgrad_wide_bx3_tw16_1x5", "wgrad_ring_wide_1x5_cat3")),
    # the flow head 256 -> 2 on the vector pipe
    "head3x3": dict(cs=[256], cout=2, k=(3, 3), stride=1, n=2, h=30, wd=41, fwd=("fewout_wide2", "generic_splitk8"), tile=(1, 32),
                    wgrad=("wgrad_few_c2",)),
    # an encoder's downsampling conv, odd output height and a ragged right edge
    "down3x3": dict(cs=[64], cout=128, k=(3, 3), stride=2, n=2, h=91, wd=136, fwd=("gconv16_3x3_s2", "generic_splitk4"), tile=(4, 16),
                    dgrad=("dgrad_s2w_128_3x3", "dgrad_t2_generic_splitk4"), wgrad=("wgrad_ring_s2_6464", "wgrad_generic_3x3_s2_bias")),
}
_cache = {}


def data(name):
    """Seeded inputs, weights (nn.Conv2d default initialisation) and a random-sign upstream gradient of a shape, with the fp64
    references of all three operations."""
    if name not in _cache:
        s = SHAPES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        k, pad = s["k"], (s["k"][0] // 2, s["k"][1] // 2)
        w, b = B.seeded_conv(17, sum(s["cs"]), s["cout"], k, s["stride"])
        xs = [torch.randn(s["n"], c, s["h"], s["wd"], generator=g) for c in s["cs"]]
        ref, mag = B.op_conv_ref(xs, w, b, stride=s["stride"], padding=pad)
        dy = B.random_sign(ref.shape, g)
        d = dict(s, pad=pad, w=w, b=b, xs=xs, ref=ref, mag=mag, dy=dy)
        d["dref"], d["dmag"] = B.op_dgrad_ref(dy, w, (s["h"], s["wd"]), stride=s["stride"], padding=pad)
        d["wref"], d["wmag"], d["bref"], d["bmag"] = B.op_wgrad_ref(xs, dy, tuple(w.shape), stride=s["stride"], padding=pad)
        _cache[name] = d
    return _cache[name]


def fwd_forms():
    return [(n, f) for n, s in SHAPES.items() for f in s["fwd"]]


def dgrad_forms():
    # a stride-1 data gradient runs on - and is held to - the forward kernels
    return [(n, f) for n, s in SHAPES.items() for f in s.get("dgrad", s["fwd"] if s["cout"] > 8 else ("taps_3x3",))]


def wgrad_forms():
    return [(n, f) for n, s in SHAPES.items() for f in s["wgrad"]]


# --------------------------------------------------------------------------------------------------------------- what must pass
@pytest.mark.parametrize("name,form", fwd_forms())
def test_fp32_forward_passes(name, form):
    d = data(name)
    _passes(f"{name}.fwd fp32", form, conv_f32(d["xs"], d["w"], d["b"], stride=d["stride"], padding=d["pad"]), d["ref"], d["mag"], tile=d["tile"])


@pytest.mark.parametrize("name,form", fwd_forms())
def test_three_piece_forward_passes(name, form):
    d = data(name)
    assert torch.equal(pieces(d["w"], 3), d["w"].double())              # three pieces are the whole operand
    _passes(f"{name}.fwd three pieces", form, conv_pieces(d["xs"], d["w"], d["b"], 3, stride=d["stride"], padding=d["pad"]), d["ref"], d["mag"],
            tile=d["tile"])


@pytest.mark.parametrize("act", [B.ACT_RELU, B.ACT_LEAKY])
def test_fp32_forward_with_an_epilogue_passes(act):
    """out_scale and the ReLU / LeakyReLU epilogues go through the same mag (the pre-activation's, scaled)."""
    d = data("res3x3")
    ref, mag = B.op_conv_ref(d["xs"], d["w"], d["b"], padding=d["pad"], act=act, out_scale=0.25)
    _passes("res3x3.fwd fp32 act", "gconv16_3x3_th2_wm4_kg2", conv_f32(d["xs"], d["w"], d["b"], padding=d["pad"], act=act, out_scale=0.25), ref, mag)


@pytest.mark.parametrize("name,form", dgrad_forms())
def test_fp32_data_gradient_passes(name, form):
    d = data(name)
    _passes(f"{name}.dgrad fp32", form, dgrad_f32(d["dy"], d["w"], (d["h"], d["wd"]), d["stride"], d["pad"]), d["dref"], d["dmag"])


@pytest.mark.parametrize("name,form", wgrad_forms())
def test_fp32_weight_gradient_passes(name, form):
    d = data(name)
    dw, db = wgrad_f32(d["xs"], d["dy"], tuple(d["w"].shape), d["stride"], d["pad"])
    _passes(f"{name}.wgrad fp32", form, dw, d["wref"], d["wmag"])
    _passes(f"{name}.bgrad fp32", form, db, d["bref"], d["bmag"])


@pytest.mark.parametrize("name,form", [(n, f) for n, f in wgrad_forms() if "bx3" in f])
def test_three_piece_weight_gradient_passes(name, form):
    d = data(name)
    dw, _, _, _ = B.op_wgrad_ref([pieces(x, 3) for x in d["xs"]], pieces(d["dy"], 3), tuple(d["w"].shape), stride=d["stride"], padding=d["pad"])
    _passes(f"{name}.wgrad three pieces", form, dw.float(), d["wref"], d["wmag"])


# ------------------------------------------------------------------------------------------------------ what must be rejected
@pytest.mark.parametrize("name,form", fwd_forms())
def test_two_piece_operands_are_rejected(name, form):
    """The third bf16 piece of both operands dropped: a quarter of the suite's absolute tolerances, 4x .. 100x these limits."""
    d = data(name)
    _rejected(f"{name}.fwd two pieces", form, conv_pieces(d["xs"], d["w"], d["b"], 2, stride=d["stride"], padding=d["pad"]), d["ref"], d["mag"])


@pytest.mark.parametrize("name,form", [(n, f) for n, f in wgrad_forms() if "bx3" in f])
def test_two_piece_weight_gradient_is_rejected(name, form):
    d = data(name)
    dw, _, _, _ = B.op_wgrad_ref([pieces(x, 2) for x in d["xs"]], pieces(d["dy"], 2), tuple(d["w"].shape), stride=d["stride"], padding=d["pad"])
    _rejected(f"{name}.wgrad two pieces", form, dw.float(), d["wref"], d["wmag"])


@pytest.mark.parametrize("name,form", fwd_forms())
def test_a_tap_dropped_at_a_ragged_tile_edge_is_rejected(name, form):
    """One tap of the filter missing in the last column of the last (ragged) tile of the second tile row, first image - and the
    failure names that tile."""
    d = data(name)
    th, tw = d["tile"]
    got = conv_f32(d["xs"], d["w"], d["b"], stride=d["stride"], padding=d["pad"]).clone()
    one = torch.zeros_like(d["w"])
    ky, kx = d["k"][0] - 1, 0
    one[:, :, ky, kx] = d["w"][:, :, ky, kx]
    tap = conv_f32(d["xs"], one, None, stride=d["stride"], padding=d["pad"])
    wout = got.shape[3]
    got[0, :, th:2 * th, wout - 1] -= tap[0, :, th:2 * th, wout - 1]
    msg = _rejected(f"{name}.fwd tap dropped", form, got, d["ref"], d["mag"], tile=d["tile"])
    assert f"tile (row 1, col {(wout - 1) // tw})" in msg and "image 0" in msg


@pytest.mark.parametrize("name,form", fwd_forms())
def test_a_scale_error_of_three_units_is_rejected(name, form):
    """Invisible to a maximum-absolute test; the slope statistic sees it."""
    d = data(name)
    got = conv_f32(d["xs"], d["w"], d["b"], stride=d["stride"], padding=d["pad"]).double() * (1.0 + 3.0 * B.U)
    lim = B.LIMITS[B.form_family(form)]
    with pytest.raises(B.StageError, match="slope"):
        B.check_form(f"{name}.fwd x (1 + 3u)", form, got, d["ref"], d["mag"])
    rec = B.LOG[-1]
    assert abs(rec["slope_u"]) > 1.2 * lim.slope_u, _stats_line(rec, lim)      # (3 u against 1.9 u / 2.4 u: the size the issue sets)


def test_swapped_input_segments_are_rejected():
    d = data("gru1x5")
    h, inp, motion = d["xs"]
    for form in d["fwd"]:
        _rejected("gru1x5.fwd segments swapped", form, conv_f32([inp, h, motion], d["w"], d["b"], padding=d["pad"]), d["ref"], d["mag"])
    for form in d["wgrad"]:
        dw, _ = wgrad_f32([inp, h, motion], d["dy"], tuple(d["w"].shape), 1, d["pad"])
        _rejected("gru1x5.wgrad segments swapped", form, dw, d["wref"], d["wmag"])


@pytest.mark.parametrize("name,form", [(n, f) for n, f in wgrad_forms() if SHAPES[n]["n"] > 1])
def test_a_weight_gradient_missing_an_image_is_rejected(name, form):
    d = data(name)
    dw, db = wgrad_f32([x[:-1] for x in d["xs"]], d["dy"][:-1], tuple(d["w"].shape), d["stride"], d["pad"])
    _rejected(f"{name}.wgrad image missing", form, dw, d["wref"], d["wmag"])
    _rejected(f"{name}.bgrad image missing", form, db, d["bref"], d["bmag"])


@pytest.mark.parametrize("name,form", wgrad_forms())
def test_a_dw_slice_one_channel_off_is_rejected(name, form):
    """An input-channel slice [ci0, ci0 + cic) of a wider dw, written at ci0 + 1."""
    d = data(name)
    cin = sum(d["cs"])
    wide = (d["cout"], cin + 8, *d["k"])
    ref, mag, _, _ = B.op_wgrad_ref(d["xs"], d["dy"], wide, stride=d["stride"], padding=d["pad"], ci0=3)
    good, _ = wgrad_f32(d["xs"], d["dy"], wide, d["stride"], d["pad"], ci0=3)
    _passes(f"{name}.wgrad slice", form, good, ref, mag)
    off, _ = wgrad_f32(d["xs"], d["dy"], wide, d["stride"], d["pad"], ci0=4)
    _rejected(f"{name}.wgrad slice one off", form, off, ref, mag)


@pytest.mark.parametrize("form", SHAPES["down3x3"]["dgrad"])
@pytest.mark.parametrize("parity", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_a_stride_2_data_gradient_missing_a_parity_class_is_rejected(form, parity):
    d = data("down3x3")
    got = dgrad_f32(d["dy"], d["w"], (d["h"], d["wd"]), 2, d["pad"]).clone()
    got[:, :, parity[0]::2, parity[1]::2] = 0.0
    _rejected("down3x3.dgrad parity class zeroed", form, got, d["dref"], d["dmag"])


@pytest.mark.parametrize("name,form", wgrad_forms())
def test_assignment_in_place_of_accumulation_is_rejected(name, form):
    """The ABI's contract is dw += and db +=: the GPU test prefills both and checks got - prefill."""
    d = data(name)
    g = torch.Generator().manual_seed(3)
    dw, db = wgrad_f32(d["xs"], d["dy"], tuple(d["w"].shape), d["stride"], d["pad"])
    pre_w = torch.randn(dw.shape, generator=g) * float(d["wref"].abs().mean())
    pre_b = torch.randn(db.shape, generator=g) * float(d["bref"].abs().mean())
    # accumulated in fp32 on top of the prefill: got - prefill carries one more rounding, at the prefill's size - inside the limits
    _passes(f"{name}.wgrad +=", form, (pre_w + dw).double() - pre_w.double(), d["wref"], d["wmag"] + pre_w.double().abs())
    _rejected(f"{name}.wgrad = for +=", form, dw.double() - pre_w.double(), d["wref"], d["wmag"] + pre_w.double().abs())
    _rejected(f"{name}.bgrad = for +=", form, db.double() - pre_b.double(), d["bref"], d["bmag"] + pre_b.double().abs())


def test_every_form_of_these_shapes_is_in_the_table():
    for _, f in fwd_forms() + dgrad_forms() + wgrad_forms():
        assert B.form_family(f) in B.LIMITS
    assert not B.FORM_KAPPA or all(isinstance(r, str) and r for r in B.FORM_KAPPA.values())
