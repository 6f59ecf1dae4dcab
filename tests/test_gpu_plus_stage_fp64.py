"""Every launch of EEMFlow+'s inference path against fp64, kernel form by kernel form.  `pytest -m gpu`.

eemplus_forward drives a pad, eight encoder layers, one pooling launch and about 25 launches per pyramid level.  Every case here pins the
EEM_* switches the EEMFlow+ dispatch reads, runs ONE forward with the stage recorder on (eemplus_record_stages: a device copy of each
launch's output behind the launch, filed with the kernel form that wrote it), asserts from the recorder's list that the intended forms
ran, and holds every recorded launch to an fp64 evaluation of THAT launch on the GPU's own recorded input to it (oracle/fp64_bounds.py).
tests/test_fp64_bounds_plus.py shows on the CPU that these checks reject sixteen planted faults and pass torch's fp32 evaluation.

LIMITS - none is fitted to the kernels under test:
  reused    plain sums (every convolution whose epilogue is none / LeakyReLU / dec7's residual add, the 53-tap correlation, the pooling) go
            through `check` under the family of the form that ran, in units of fp32 rounding of the launch's own sum of |terms|: gconv
            names as tests/test_gpu_ops_fp64.py maps them, "wnc*" and the encoder's "wino" -> wino2, "enc1" -> enc1, "enc2" / "enc_c*" and
            every "tail_*" -> direct, both correlation forms -> corr, "pool2x3" -> pool.  The sigmoid blend (blend, warp_blend_warp's
            flow_up) goes through `check_decoder`: rms and max error at most KAPPA_DEC = 6.4 x those of torch's fp32 CPU evaluation of the
            same launch on the same input, plus one unit of rounding at the largest output.
  derived   the warps' four-term blend 4 roundings (taps, weights and the mode-2 mask computed in fp32 as csrc/warp_px.h does - the
            model's definition; a masked pixel must be exactly 0), the flow upsampling 6 + 1 for the rate factor, scale_flow and the
            coarse flow's doubling 1, the pooling 3 (fp64_bounds.ER_ROUNDINGS, derived there).
  bitwise   replicate padding; copy_channels and the fused launch's copy of flow_up into the decoder's input; the zero flow channels of
            level 6; a teacher-forced flow_init; every prediction with the recorder on against off; l2.flow against the stage flow2;
            every negative output of a LeakyReLU launch is an fp32 value times the fp32 slope (pl_check_leaky).

SHAPES are the smallest that reach a form with tiles cut on the right and at the bottom, worked out from the dispatch code and confirmed
by the recorder.  What the recorder corrected: 128x192 under EEM_PLUS_TAIL_MAXCIN=100 puts the wide dense-estimator convs on
generic_splitk16 at levels 3..5 and on gconv16 / fewout only at level 2; 194x290 keeps the fused upflow_warp at every level (a map is
always >= twice its coarser one) - its odd maps show in the encoder instead, whose layers 3..7 leave the Winograd / enc2 kernels for the
generic launch<> forms; the model upsamples its padded-grid flows straight to the unpadded size, so there is no crop and no crop offset;
384x352 is a multiple of 8 already (pad 0); with EEM_PLUS_WNC_MINPX = 0 the 3-cout head does run on conv_wnc.hip (wnc32_m16) - only
dec7 stays off it.

LEFT OUT, and why:
  * tail_k1_g2, tail_k3_g5, tail_k3_g18 and tail_conv_multi_kernel: no layer of EEMFlow+ has <= 8 (1x1), <= 20 or 65..72 input
    channels - they are EEMFlow's tail's (tests/test_gpu_stage_fp64.py).  enc_c16_16_s1 and enc_c16_32_s2: layers 1 and 2 leave the
    Winograd kernel / conv_enc2.hip only on a level-1 map whose width is no multiple of 4, and a padded width (a multiple of 8 at the
    least) is always halved to one.
  * pl_warp_blend_launch without the second warp ("warp_blend"): no call site in eemplus_forward.
  * eemplus_forward_stream: it records nothing; its flows are bitwise forward_many's (tests/test_gpu_plus_stream.py).
  * one launch per group (EEM_PLUS_NO_GROUPED=1) reports the same gconv16 form as the grouped launch; both are checked, the recorder
    cannot tell them apart.
  * F.grid_sample's own position arithmetic: torch's vectorised CPU kernel and its CUDA kernel compile ix = (xn + 1) (w / 2) - 0.5 to a
    fused multiply-add, csrc/warp_px.h rounds the product first (built with -ffp-contract=off, as the goldens' torch did).  The two
    differ in the last bit on ~2 % of sub-pixel positions and the `>= 1.0` mask then flips on ~0.2 % of pixels.  The reference here
    is warp_px.h's definition; the direct warp cases draw their flows so that both forms agree (fp64_bounds.pl_hostile_flows).

FOUND AND FIXED by this module:
  * corr_tiled53_kernel (maps from 8192 cells on) gave rms(z) 1.50 and max|z| 8.93 at level 2 of 384x352 (96x88 cells, 32 channels)
    against the corr family's 1.1 / 7.6; corr_kernel reads 0.77 / 3.75.  Each tap's sum was ONE chain of fused multiply-adds over all
    32 / 64 channels, and feature maps have a per-channel mean, so a tap's products mostly share a sign (the worst element: sum of terms
    = 0.99 x sum of |terms|) and every addition rounded a partial sum that had grown steadily - the fault the E-RAFT module found in the
    all-pairs kernels.  The kernel now adds each chunk of eight channels into a sum of its own that then joins the running one (the
    figures are in the table below).  Cost, tools/bench_plus_stream.py at 1280x720, four flows per call, three interleaved runs of
    five rounds each on the two libraries: stream 1489 -> 1440 frames/s, many 1363 -> 1324 (-3 %; 53 more registers per thread).
    Summing tap by tap into one register instead measured -5 % and was dropped.
  * the dense estimator's 176 -> 8 conv on conv_wnc.hip's 16-cout form (wnc32_m16 / wnc64_m16) read a slope of 0.74 / 0.76 / 1.72 u
    at 64x80 / 32x40 / 16x20 cells against wino2's 0.56 u, with max|z| 1.9 and rms 0.15 .. 0.21 well inside the family.  conv_wnc.hip
    stores the transformed weights G g G^T in fp32: a FIXED perturbation of the layer's kernel, the same at every pixel; the layer's
    inputs have a per-channel mean and its sums cancel (|ref| ~ 0.03 mag), so the perturbation shows as a scale error over the
    layer's 8 output channels, not as noise over its pixels.  wnc_pack_quad formed the transform in fp32, up to four roundings per
    weight; it now forms it in double and rounds once (host and device pack alike, a one-off cost at weight load): 0.52 u on these
    launches, and the 32-cout form's worst slope went from 0.50 to 0.25 u.  No launch changed, so no forward time did.

MEASURED worst statistics per form (one AMD Instinct MI355X, gfx950, 256 CUs).  A record: these numbers set no limit.
Sums and short operation counts (criteria 1 and 2), the worst over all checks of the module:
    form                               held to        max|z|    rms   |mean|  |slope| u  checks
    corr_direct                        corr             3.75  0.765   0.0225     0.103      51
    corr_tiled53                       corr             3.35  0.779   0.0003     0.001       1
    enc1                               enc1             3.99  0.314   0.0021     0.004       7
    enc2                               direct           8.09  0.460   0.0026     0.054      15
    enc_c32_32_s1                      direct           5.48  0.487   0.0012     0.055       2
    enc_c32_64_s2                      direct           4.86  0.373   0.0011     0.010       1
    enc_c5_16_s2                       enc1             3.13  0.311   0.0021     0.003       1
    enc_c64_64_s1                      direct           7.29  0.452   0.0013     0.047       2
    fewout_k16_c8                      direct           0.88  0.178   0.0048     0.198      10
    fewout_k8_c2                       direct           1.18  0.287   0.0044     0.012       6
    gconv16_1x1_th2_wm2_kg1            direct           5.39  0.399   0.0039     0.057      12
    gconv16_3x3_s2                     direct           4.04  0.383   0.0045     0.140       2
    gconv16_3x3_th2_wm2_kg1            direct           7.96  0.541   0.0047     0.243      13
    gconv16_3x3_th2_wm2_kg2            direct           4.87  0.345   0.0053     0.258       9
    gconv16_3x3_th2_wm4_kg2            direct           4.28  0.353   0.0036     0.119       2
    gconv16_3x3_th3_wm4_kg2            direct           2.24  0.232   0.0022     0.100       2
    gconv16_3x3_th4_wm1_kg2            direct           2.98  0.313   0.0039     0.177       4
    generic_1x1                        direct           5.52  0.447   0.0035     0.082       5
    generic_1x1_b4                     direct           3.59  0.353   0.0067     0.056       1
    generic_splitk16                   direct           0.81  0.189   0.0259     0.390      10
    pool2x3                            pool             2.56  0.608   0.0352     0.073      27
    pool2x3 roundings                  roundings 3      2.56  0.608   0.0352     0.073      27
    scale_flow scale                   roundings 1      0.99  0.426   0.0257     0.083       8
    tail_k1_g25_j1                     direct           4.42  0.455   0.0204     0.205       8
    tail_k1_g25_j2                     direct           6.12  0.455   0.0240     0.340      66
    tail_k3_g16_j1                     direct           1.79  0.225   0.0238     0.407      72
    tail_k3_g16_j2                     direct           1.79  0.225   0.0099     0.259      52
    tail_k3_g25_j1                     direct           1.87  0.227   0.0100     0.459     140
    tail_k3_g46_j1                     direct           1.89  0.297   0.0432     0.707     116
    tail_k3_g8_j1                      direct           1.68  0.337   0.1341     0.315      51
    tail_k3_g8_j3                      direct           1.98  0.230   0.0101     0.205     123
    upflow                             roundings 6/7    3.76  0.864   0.2212     0.532      17
    upflow_multi                       roundings 7      3.42  0.787   0.0325     0.054      35
    upflow_warp                        roundings 4/7    3.31  0.817   0.2212     0.532      74
    upflow_warp scale                  roundings 1      0.97  0.419   0.0659     0.039      37
    warp                               roundings 4      3.21  0.696   0.0821     0.084      26
    warp_blend_warp                    roundings 4      3.35  0.738   0.0157     0.068      39
    wino                               wino2            4.14  0.314   0.0121     0.208      36
    wnc32                              wino2            4.98  0.243   0.0086     0.248      33
    wnc32_m16                          wino2            3.26  0.321   0.0084     0.521      12
    wnc64                              wino2            3.25  0.243   0.0086     0.248      18
    wnc64_m16                          wino2            3.26  0.321   0.0084     0.521       9
Launches that end in the sigmoid blend (criterion 3): the GPU's error and the fp32 CPU evaluation's own, both against fp64
    form of the launch                 GPU rms    GPU max    CPU rms    CPU max  rms ratio  max ratio  checks
    blend                             4.72e-08   2.15e-07   4.71e-08   2.15e-07       1.00       1.00       4
    warp_blend_warp                   6.21e-08   3.84e-07   7.12e-08   1.16e-06       1.12       1.50      39
Bitwise comparisons: 868, all equal.
"""
import ctypes

import pytest
import torch

from eemflow_amd import _lib
from eemflow_amd.eemflow_plus import EEMFlow_cdc
from eemflow_amd.padder import InputPadder
from eemflow_amd.plus_weights import seeded_from_shapes
from eemflow_amd.weights import synthetic_voxel_pair
from oracle import eemflow_oracle as O
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every EEM_* switch this path reads: plus_api.hip's seven, conv_wnc.hip's and tail.hip's, what enc_conv_launch and conv() -> gconv_launch
# can reach (gconv*.hip)
SWITCHES = ("EEM_PLUS_GENERIC_ENC", "EEM_PLUS_WNC_MINPX", "EEM_PLUS_WNC_MINPX_JOBS", "EEM_PLUS_TAIL_MAXCIN", "EEM_PLUS_NO_GROUPED",
            "EEM_PLUS_NO_FUSE", "EEM_PLUS_SIDE", "EEM_NO_WNC", "EEM_WNC_SMALL_MAXPX", "EEM_NO_TAIL_MULTI", "EEM_NO_ENC1", "EEM_WINO",
            "EEM_FEWOUT_SMALL_BLOCKS", "EEM_FEWOUT_WIDE", "EEM_GB_DBG", "EEM_GCONVB_1X1", "EEM_GCONVB_MINBLK", "EEM_GCONVB_RING",
            "EEM_NO_FEWOUT", "EEM_NO_G16_S2", "EEM_NO_GCONV16", "EEM_NO_GCONVB", "EEM_NO_SPLITK", "EEM_NO_TAPS_KERNEL", "EEM_SPLITK_MAX")

# the forms of this path's own launch functions and its fused launches: the last test wants every one of them seen
PL_FORMS = {"tail_k1_g25", "tail_k3_g8", "tail_k3_g16", "tail_k3_g25", "tail_k3_g46", "wnc32", "wnc64", "wnc32_m16", "wnc64_m16",
            "enc1", "wino", "enc2", "enc_c5_16_s2", "enc_c32_32_s1", "enc_c32_64_s2", "enc_c64_64_s1", "corr_direct", "corr_tiled53", "pool2x3",
            "warp", "upflow", "upflow_multi", "upflow_warp", "scale_flow", "blend", "warp_blend_warp", "copy_channels",
            "pad4", "pad4_pair"}
FUSED = {"paired projections", "de0 + rconv", "groups as tail jobs", "groups as wnc jobs", "grouped gconv16", "upflow_warp",
         "warp_blend_warp", "forced_init", "side stream"}
CASES = {"default", "nofuse", "maxcin100", "odd", "wnc", "many", "nownc", "nogrouped", "wnc64", "tiled53", "g1c15", "generic_enc",
         "side", "fif4", "level", "warps", "upsample", "zeros", "noenc1"}
SEEN, SEEN_FUSED, RAN = set(), set(), set()
ERRS = []
MYLOG = []          # this module's share of B.LOG (the other fp64 modules of a whole-suite run log there too)


def soft(check, *args, **kw):
    """A check whose StageError is kept for `flush`: one run names every failing launch of a forward, not the first."""
    n = len(B.LOG)
    try:
        return check(*args, **kw)
    except B.StageError as e:
        ERRS.append(str(e))
        return None
    finally:
        MYLOG.extend(B.LOG[n:])


def flush():
    errs, ERRS[:] = list(ERRS), []
    if errs:
        raise B.StageError(f"{len(errs)} launches outside their limits:\n" + "\n".join(errs))


def pin(monkeypatch, env):
    ERRS.clear()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def make_net(seed, h, w, record, groups=3, cin=5, pad8=False, **attrs):
    net = EEMFlow_cdc("", groups, cin).eval()
    sd = seeded_from_shapes({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.record_stages = tuple(record) if record is not None else None
    for k, v in attrs.items():
        setattr(net, k, v)
    net = net.to(DEV)
    net.change_imagesize((h, w))
    if pad8:
        # the module's padder fills up to multiples of 64: every map even, level 2 a multiple of 16 wide.  eemplus_forward and the
        # oracle take any padding; up to 8 on all four sides gives odd maps (50x74, 25x37, ..., 3x4) and a ratio 12 -> 25
        net.image_padder = InputPadder((h, w), mode="sintel", eval_pad_rate=8)
    return net, O.to_torch_sd(sd)


class Stages:
    """The recorder's list of the module's last call, and its tensors on the CPU (fetched once each)."""

    def __init__(self, net, prefixes=()):
        torch.cuda.synchronize()
        self.net = net
        self.prefixes = tuple(prefixes)
        self.names = {name: (form, dims) for name, form, dims in net.stage_names()}
        self.cache = {}
        for name, (form, _) in self.names.items():
            if form:
                SEEN.add(B.pl_base_form(form)[0])

    def __contains__(self, name):
        return name in self.names

    def has(self, name):
        """Whether the recorder filed `name`; a name the case's prefixes cover MUST have been filed (a launch the recorder stopped
        filing fails here instead of going unchecked)."""
        if name in self.names:
            return True
        assert not any(name.startswith(p) for p in self.prefixes), f"'{name}' is covered by the prefixes {self.prefixes} but was not recorded"
        return False

    def form(self, name):
        return self.names[name][0]

    def base(self, name):
        return B.pl_base_form(self.names[name][0])[0]

    def get(self, name):
        if name not in self.cache:
            assert name in self.names, (name, sorted(self.names))
            t = self.net.stage(name).cpu()
            assert tuple(t.shape) == self.names[name][1], (name, t.shape, self.names[name])
            self.cache[name] = t
        return self.cache[name]


def inputs(seed, b, h, w, cin=5):
    return tuple(torch.from_numpy(a) for a in synthetic_voxel_pair(seed, b, h, w, bins=cin))


def forward(net, e1, e2, many=False):
    with torch.no_grad():
        if many:
            outs = net.forward_many([(e1[i:i + 1].to(DEV), e2[i:i + 1].to(DEV)) for i in range(e1.shape[0])])
            preds = [torch.cat([o[1][k] for o in outs]) for k in range(5)]
        else:
            preds = net(e1.to(DEV), e2.to(DEV))[1]
    torch.cuda.synchronize()
    return [p.cpu() for p in preds]


def conv_w(sd, name, groups=1):
    return sd[name + ".weight"], sd[name + ".bias"]


def kappa(name, form, got, ref64, ref32):
    n = len(B.LOG)
    rec = soft(B.check_decoder, name, got, ref64, ref32)
    if len(B.LOG) > n:                                   # (a failure raised before anything was logged leaves the log alone)
        B.LOG[-1]["form"] = form
    return rec


def conv_check(st, tag, nm, x, w, b, sel, act=True, k=3, groups=1, res=None, stride=1):
    """One recorded convolution launch `nm` on its input x (already restricted to the images `sel`)."""
    if not st.has(nm):
        return
    if stride == 1:
        ref, mag = B.pl_conv_ref(x, w, b, act=act, k=k, groups=groups, res=res)
    else:
        ref, mag = B.conv_ref(x, w, b, stride=stride, act=act)
    got = st.get(nm)[sel]
    soft(B.pl_check_form, f"{tag} {nm}", st.form(nm), got, ref, mag)
    if act:
        soft(B.pl_check_leaky, f"{tag} {nm}", got, st.form(nm))


ENC = [("pconv1_1", 2), ("pconv1_2", 1), ("pconv2_1", 2), ("pconv2_2", 1), ("pconv2_3", 1), ("pconv3_1", 2), ("pconv3_2", 1), ("pconv3_3", 1)]


def check_pyramid(st, sd, tag, e1, e2, pad, imgs):
    """pad (bitwise), the eight encoder layers and the pooling for the encoder's images `imgs` (of [events1; events2])."""
    x = B.er_pad_ref(torch.cat([e1, e2]), pad)
    if st.has("pad"):
        soft(B.check_bitwise, f"{tag} pad", st.get("pad"), x)
        x = st.get("pad")
    x = x[imgs]
    for i, (name, stride) in enumerate(ENC):
        nm = f"enc{i}"
        if not st.has(nm):
            x = None
            continue
        if x is not None:
            conv_check(st, tag, nm, x, *conv_w(sd, name + ".0"), imgs, stride=stride)
        x = st.get(nm)[imgs]
    src = x
    for l in (4, 5, 6):
        nm = f"pool{l}"
        if not st.has(nm):
            src = None
            continue
        if src is not None:
            ref, mag = B.avg_pool_ref(src, 2)
            soft(B.pl_check_form, f"{tag} {nm}", st.form(nm), st.get(nm)[imgs], ref, mag)
            soft(B.check_roundings, f"{tag} {nm} roundings", st.get(nm)[imgs], ref, mag, "pool", form=st.form(nm) + " roundings")
        src = st.get(nm)[imgs]


def features(st, l, batch, sel):
    """(feature_1, feature_2) of level l for the samples `sel`, from the recorded pyramid."""
    f = st.get({2: "enc4", 3: "enc7", 4: "pool4", 5: "pool5", 6: "pool6"}[l])
    return f[:batch][sel], f[batch:][sel]


def check_decoder_chain(st, sd, tag, l, G, sel, corr, rconv, cat_flow, residual):
    p = f"l{l}."
    d = f"decoder{l}."
    conv_check(st, tag, p + "dec1", B.pl_cat_input(corr, rconv, cat_flow), *conv_w(sd, d + "conv1.0"), sel)
    prev = p + "dec1"
    for j in range(3):
        nm = p + f"decg{j}"
        if st.has(nm) and st.has(prev):
            conv_check(st, tag, nm, st.get(prev)[sel], *conv_w(sd, d + f"conv{j + 2}.0"), sel, groups=G)
            if G > 1:
                SEEN_FUSED.add({"tai": "groups as tail jobs", "wnc": "groups as wnc jobs", "gco": "grouped gconv16"}[st.form(nm)[:3]])
        prev = nm
    if st.has(p + "dec5"):
        conv_check(st, tag, p + "dec5", st.get(p + "decg2")[sel], *conv_w(sd, d + "conv5.0"), sel)
        conv_check(st, tag, p + "dec6", st.get(p + "dec5")[sel], *conv_w(sd, d + "conv6.0"), sel)
        conv_check(st, tag, p + "flow", st.get(p + "dec6")[sel], *conv_w(sd, d + "conv7"), sel, act=False, res=residual)


def check_level6(st, sd, tag, G, batch, sel):
    f1, f2 = features(st, 6, batch, sel)
    ref, mag = B.corr53_ref(f1, f2)
    soft(B.pl_check_form, f"{tag} l6.corr", st.form("l6.corr"), st.get("l6.corr")[sel], ref, mag)
    z = st.get("l6.cat_flow")
    soft(B.check_bitwise, f"{tag} l6.cat_flow", z, torch.zeros_like(z))               # (every sample: the fill is per buffer layout)
    conv_check(st, tag, "l6.rconv", f1, *conv_w(sd, "rconv6.0"), sel)
    check_decoder_chain(st, sd, tag, 6, G, sel, st.get("l6.corr")[sel], st.get("l6.rconv")[sel], z[sel], None)


def check_level(st, sd, tag, l, G, batch, sel, forced=None):
    """Every recorded launch of level l = 5..2 for the samples `sel`; forced: the flow_init an eemplus_level call was given."""
    p = f"l{l}."
    f1, f2 = features(st, l, batch, sel)
    h, w = f1.shape[-2:]
    w1 = conv_w(sd, f"conv_1x1.{l}.0")
    conv_check(st, tag, p + "a1", f1, *w1, sel, k=1)
    conv_check(st, tag, p + "a2", f2, *w1, sel, k=1)
    if B.pl_base_form(st.form(p + "a1")) == ("tail_k1_g25", 2):
        SEEN_FUSED.add("paired projections")
    conv_check(st, tag, p + "rconv", f1, *conv_w(sd, f"rconv{l}.0"), sel)
    if st.form(p + "rconv") == st.form(p + "de0") and B.pl_base_form(st.form(p + "de0"))[1] == 2:
        SEEN_FUSED.add("de0 + rconv")
    # ---- cdc_model's upsampling: flow_init from the coarser level's flow as the launch read it (recorded before the doubling)
    fi = st.get(p + "flow_init")[sel]
    if forced is not None:
        soft(B.check_bitwise, f"{tag} {p}flow_init", fi, forced[sel])
        assert st.form(p + "flow_init") == "" and p + "coarse_scaled" not in st
        SEEN_FUSED.add("forced_init")
    elif f"l{l + 1}.flow" in st:
        coarse = st.get(f"l{l + 1}.flow")[sel]
        assert st.form(p + "flow_init") in ("upflow_warp", "upflow"), st.form(p + "flow_init")
        ref, mag = B.pl_upflow_ref(coarse, (h, w))
        soft(B.check_roundings, f"{tag} {p}flow_init", fi, ref, mag, "upflow_rate", form=st.form(p + "flow_init"))
        ref, mag = B.pl_scale_ref(coarse, (h, w))
        soft(B.check_roundings, f"{tag} {p}coarse_scaled", st.get(p + "coarse_scaled")[sel], ref, mag, "scale",
             form=st.form(p + "coarse_scaled") + " scale")
        if st.form(p + "flow_init") == "upflow_warp":
            SEEN_FUSED.add("upflow_warp")
    a1, a2 = st.get(p + "a1")[sel], st.get(p + "a2")[sel]
    soft(B.pl_check_warp, f"{tag} {p}warp_a2", st.get(p + "warp_a2")[sel], a2, fi, 2, form=st.form(p + "warp_a2"))
    # ---- the dense estimator: each conv reads the slice [184 - din, 184) and writes its own slice of the same buffer
    warp_a2 = st.get(p + "warp_a2")[sel]
    des = []
    for i in range(5):
        conv_check(st, tag, p + f"de{i}", B.pl_dense_input(a1, warp_a2, des), *conv_w(sd, f"cdc_model.dense_estimator_mask.conv{i + 1}.0"), sel)
        des.append(st.get(p + f"de{i}")[sel])
    conv_check(st, tag, p + "xout", B.pl_dense_input(a1, warp_a2, des), *conv_w(sd, "cdc_model.dense_estimator_mask.conv_last.0"), sel, act=False)
    xout = st.get(p + "xout")[sel]
    # ---- warp + sigmoid blend (+ copy + warp)
    fup = st.get(p + "flow_up")[sel]
    if st.form(p + "flow_up") == "warp_blend_warp":
        r64, r32 = B.pl_warp_blend_refs(fi, xout)
        kappa(f"{tag} {p}flow_up", "warp_blend_warp", fup, r64, r32)
        SEEN_FUSED.add("warp_blend_warp")
    else:
        assert st.form(p + "flow_up") == "blend" and st.form(p + "tw") == "warp"
        tw = st.get(p + "tw")[sel]
        soft(B.pl_check_warp, f"{tag} {p}tw", tw, fi, xout[:, :2], 1, form="warp")
        kappa(f"{tag} {p}flow_up", "blend", fup, B.pl_blend_ref(tw, fi, xout), B.pl_blend_ref(tw, fi, xout, torch.float32))
    soft(B.check_bitwise, f"{tag} {p}cat_flow", st.get(p + "cat_flow")[sel], fup)
    soft(B.pl_check_warp, f"{tag} {p}fw", st.get(p + "fw")[sel], f2, fup, 0, form=st.form(p + "fw"))
    ref, mag = B.corr53_ref(f1, st.get(p + "fw")[sel])
    soft(B.pl_check_form, f"{tag} {p}corr", st.form(p + "corr"), st.get(p + "corr")[sel], ref, mag)
    check_decoder_chain(st, sd, tag, l, G, sel, st.get(p + "corr")[sel], st.get(p + "rconv")[sel], st.get(p + "cat_flow")[sel], fup)


def check_predictions(st, tag, preds, batch, sel, hw, many):
    """The five full-resolution predictions from the level flows as the launch read them: flow6..flow3 doubled, flow2 plain."""
    srcs = ["l5.coarse_scaled", "l4.coarse_scaled", "l3.coarse_scaled", "l2.coarse_scaled", "l2.flow"]
    if not all([st.has(s) for s in srcs + [f"pred{sel[0]}" if many else "pred"]]):
        return
    for b in sel:
        got = st.get(f"pred{b}") if many else st.get("pred").view(5, batch, 2, *hw)[:, b]
        form = st.form(f"pred{b}" if many else "pred")
        for i, s in enumerate(srcs):
            ref, mag = B.pl_upflow_ref(st.get(s)[b:b + 1], hw)
            soft(B.check_roundings, f"{tag} pred[{i}] sample {b}", got[i:i + 1], ref, mag, "upflow_rate", form=form)
            soft(B.check_bitwise, f"{tag} pred[{i}] sample {b} returned", preds[i][b:b + 1], got[i:i + 1])
    soft(B.check_bitwise, f"{tag} l2.flow is the stage flow2", st.net.stage("flow2").cpu(), st.get("l2.flow"))


def run_case(monkeypatch, tag, env, h, w, batch=1, sel=(0,), record=("",), levels=(6, 5, 4, 3, 2), many=False, pyramid=True, seed=3,
             expect=None, **net_kw):
    """One forward with the recorder on; every recorded launch checked; the predictions bitwise a forward's with the recorder off."""
    pin(monkeypatch, env)
    G, cin = net_kw.get("groups", 3), net_kw.get("cin", 5)
    net, sd = make_net(seed, h, w, record, **net_kw)
    e1, e2 = inputs(5, batch, h, w, cin)
    preds = forward(net, e1, e2, many)
    st = Stages(net, record)
    for nm, want in (expect or {}).items():
        assert st.form(nm) == want, (nm, st.form(nm), want)
    sel = list(sel)
    if pyramid:
        check_pyramid(st, sd, tag, e1, e2, net.image_padder._pad, sel + [batch + s for s in sel])
    for l in levels:
        if l == 6:
            check_level6(st, sd, tag, G, batch, sel)
        else:
            check_level(st, sd, tag, l, G, batch, sel)
    check_predictions(st, tag, preds, batch, sel, (h, w), many)
    net.record_stages = None
    off = forward(net, e1, e2, many)
    assert net.stage_names() == [] and all(torch.equal(a, b) for a, b in zip(preds, off)), "the recorder changed a prediction"
    flush()
    RAN.add(tag)
    return net, sd, st


SMALL = {"l3.a1": "tail_k1_g25_j2", "l3.de0": "tail_k3_g16_j2", "l3.rconv": "tail_k3_g16_j2", "l2.de1": "tail_k3_g25_j1",
         "l2.xout": "tail_k3_g46_j1", "l2.decg0": "tail_k3_g8_j3", "l2.flow": "tail_k3_g8_j1", "l6.rconv": "tail_k3_g16_j1",
         "l2.flow_init": "upflow_warp", "l2.flow_up": "warp_blend_warp", "l2.corr": "corr_direct", "pool4": "pool2x3",
         "enc0": "enc1", "enc1": "wino", "enc2": "enc2", "pad": "pad4_pair", "pred": "upflow_multi"}


def test_small_grid_default(monkeypatch):
    """128x192, levels 32x48 .. 2x3: every layer on the small-grid kernel, the paired projections, rconv riding de[0]."""
    run_case(monkeypatch, "default", {}, 128, 192, expect=SMALL)


def test_small_grid_unfused(monkeypatch):
    """EEM_PLUS_NO_FUSE=1: upflow + scale_flow + warp, warp + blend + warp + copy_channels, one launch per projection."""
    run_case(monkeypatch, "nofuse", {"EEM_PLUS_NO_FUSE": "1"}, 128, 192,
             expect={"l3.a1": "tail_k1_g25_j1", "l3.de0": "tail_k3_g16_j1", "l3.flow_init": "upflow", "l3.coarse_scaled": "scale_flow",
                     "l3.warp_a2": "warp", "l3.tw": "warp", "l3.flow_up": "blend", "l3.fw": "warp", "l3.cat_flow": "copy_channels"})


def test_small_grid_wide_convs_off_tail(monkeypatch):
    """EEM_PLUS_TAIL_MAXCIN=100: the 128 .. 184-channel convs on the LDS-tiled / few-cout / split-K kernels."""
    run_case(monkeypatch, "maxcin100", {"EEM_PLUS_TAIL_MAXCIN": "100"}, 128, 192,
             expect={"l2.de2": "gconv16_3x3_th2_wm2_kg2", "l2.de3": "gconv16_3x3_th4_wm1_kg2", "l2.de4": "fewout_k16_c8",
                     "l2.xout": "fewout_k16_c8", "l4.de2": "generic_splitk16", "l4.xout": "generic_splitk16", "l2.de1": "tail_k3_g25_j1"})


def test_odd_maps(monkeypatch):
    """194x290 padded to 200x296: maps 50x74, 25x37, 12x18, 6x9, 3x4 (12 -> 25: a ratio that is not 2); the output width 290 sends
    upflow_multi to its per-job launches; the encoder's layers 3..7 on the generic launch<> forms."""
    net, _, st = run_case(monkeypatch, "odd", {}, 194, 290, pad8=True,
                          expect={"pred": "upflow", "enc3": "enc_c32_32_s1", "enc5": "enc_c32_64_s2", "enc6": "enc_c64_64_s1",
                                  "l3.flow_init": "upflow_warp", "l2.decg1": "tail_k3_g8_j3"})
    assert net.image_padder._pad == [3, 3, 3, 3]
    assert [st.names[f"l{l}.corr"][1][2:] for l in (2, 3, 4, 5, 6)] == [(50, 74), (25, 37), (12, 18), (6, 9), (3, 4)]


WNC = {"l2.de0": "wnc32", "l2.rconv": "wnc32", "l2.de3": "wnc32_m16", "l2.xout": "wnc32_m16", "l2.dec1": "wnc32", "l2.decg0": "wnc32",
       "l2.dec6": "wnc32", "l2.flow": "fewout_k8_c2", "l4.de1": "wnc32", "l2.a1": "gconv16_1x1_th2_wm2_kg1", "l5.de0": "tail_k3_g16_j2"}


def test_every_level_on_winograd(monkeypatch):
    """256x320 (level 2: 64x80 = 5120 cells, 2.5 tiles of 32 wide) with EEM_PLUS_WNC_MINPX = _JOBS = 0: every level whose width is a
    multiple of 4 through conv_wnc.hip, groups as the jobs of one launch - the 3-cout head included, on the 16-cout form; only dec7 (2
    couts, a residual epilogue) stays off it, on the few-cout kernel."""
    run_case(monkeypatch, "wnc", {"EEM_PLUS_WNC_MINPX": "0", "EEM_PLUS_WNC_MINPX_JOBS": "0"}, 256, 320, expect=WNC)


def test_wide_block_tile(monkeypatch):
    """EEM_WNC_SMALL_MAXPX=0: the 4 x 64 block tile (80 columns: one whole tile and a quarter of one)."""
    run_case(monkeypatch, "wnc64", {"EEM_PLUS_WNC_MINPX": "0", "EEM_PLUS_WNC_MINPX_JOBS": "0", "EEM_WNC_SMALL_MAXPX": "0"}, 256, 320,
             levels=(4, 3, 2), record=("enc", "pool", "l"), pyramid=False,
             expect={k: v.replace("wnc32", "wnc64") for k, v in WNC.items()})


def test_batch_four_forward_many(monkeypatch):
    """Four samples through forward_many under the default block-count rule (level 2 on conv_wnc.hip); the first and last checked."""
    run_case(monkeypatch, "many", {}, 256, 320, batch=4, sel=(0, 3), many=True,
             expect={"pad": "pad4", "l2.de0": "wnc32", "l2.decg2": "wnc32", "l3.de0": "tail_k3_g16_j2", "pred3": "upflow_multi"})


def test_no_winograd(monkeypatch):
    """EEM_NO_WNC=1: level 2 on the LDS-tiled kernel, its grouped layers as one grouped gconv16 launch."""
    run_case(monkeypatch, "nownc", {"EEM_NO_WNC": "1"}, 256, 320, levels=(3, 2), record=("enc", "pool", "l"), pyramid=False,
             expect={"l2.decg0": "gconv16_3x3_th2_wm2_kg1", "l2.dec1": "gconv16_3x3_th3_wm4_kg2", "l2.de3": "gconv16_3x3_th4_wm1_kg2",
                     "l2.de4": "fewout_k16_c8"})


def test_one_launch_per_group(monkeypatch):
    run_case(monkeypatch, "nogrouped", {"EEM_NO_WNC": "1", "EEM_PLUS_NO_GROUPED": "1"}, 256, 320, levels=(2,), record=("enc", "pool", "l"),
             pyramid=False, expect={"l2.decg0": "gconv16_3x3_th2_wm2_kg1", "l2.decg2": "gconv16_3x3_th2_wm2_kg1"})


def test_tiled_correlation(monkeypatch):
    """384x352: level 2 is 96x88 = 8448 cells, the first size on corr_tiled53 (5.5 tiles of 16 wide); l2. and the pyramid only."""
    run_case(monkeypatch, "tiled53", {}, 384, 352, pad8=True, levels=(2,), record=("pad", "enc", "pool", "l2.", "l3.flow"),
             expect={"l2.corr": "corr_tiled53", "l2.dec1": "wnc32", "l2.de0": "gconv16_3x3_th2_wm2_kg1"})


def test_groups_one_fifteen_channels(monkeypatch):
    """groups=1 (one 96 -> 96 job per grouped layer) and n_first_channels=15: the encoder on the generic conv kernels."""
    run_case(monkeypatch, "g1c15", {}, 128, 192, groups=1, cin=15,
             expect={"enc0": "generic_1x1", "enc3": "tail_k3_g8_j1", "enc5": "gconv16_3x3_s2", "l3.decg0": "tail_k3_g25_j1"})


def test_generic_encoder_five_channels(monkeypatch):
    run_case(monkeypatch, "generic_enc", {"EEM_PLUS_GENERIC_ENC": "1"}, 128, 192, levels=(), record=("pad", "enc", "pool"),
             expect={"enc0": "generic_1x1_b4", "enc7": "tail_k3_g16_j1"})


def test_first_layer_off_enc1(monkeypatch):
    """EEM_NO_ENC1: pconv1_1 on the generic launch<5, 16, 2> form."""
    run_case(monkeypatch, "noenc1", {"EEM_NO_ENC1": "1"}, 128, 192, levels=(), record=("pad", "enc"), expect={"enc0": "enc_c5_16_s2", "enc1": "wino"})


def test_side_stream(monkeypatch):
    """EEM_PLUS_SIDE=1: the projections and rconv of every level on the context's side stream, recorded on that stream."""
    run_case(monkeypatch, "side", {"EEM_PLUS_SIDE": "1"}, 256, 320, levels=(6, 5, 4, 3), record=("enc7", "pool", "l3.", "l4.", "l5.", "l6."),
             pyramid=False, expect={"l3.rconv": "tail_k3_g16_j1", "l3.de0": "tail_k3_g16_j1", "l3.a1": "tail_k1_g25_j2"})
    SEEN_FUSED.add("side stream")


def test_frames_in_flight(monkeypatch):
    run_case(monkeypatch, "fif4", {}, 256, 320, levels=(6, 5, 4, 3), record=("enc7", "pool", "l3.", "l4.", "l5.", "l6."), pyramid=False,
             frames_in_flight=4)


def test_teacher_forced_level(monkeypatch):
    """One eemplus_level call with the recorder on: the forced_init branch - no upsampling, the separate mode-2 warp launch."""
    pin(monkeypatch, {})
    net, sd = make_net(3, 128, 192, ("enc", "pool", "l"))
    e1, e2 = inputs(5, 2, 128, 192)
    forward(net, e1, e2)
    pyr = Stages(net)
    for nm in ("enc4", "enc7", "pool4", "pool5", "pool6"):
        pyr.get(nm)
    g = torch.Generator().manual_seed(9)
    for l, hw in ((3, (16, 24)), (5, (4, 6))):
        forced = torch.randn(2, 2, *hw, generator=g) * 1.5
        with torch.no_grad():
            up, out = net.level(l, forced.to(DEV))
        st = Stages(net, ("enc", "pool", f"l{l}."))
        assert set(n.split(".")[0] for n in st.names) == {f"l{l}"} and st.form(f"l{l}.warp_a2") == "warp"
        st.cache.update(pyr.cache)
        st.names.update({k: v for k, v in pyr.names.items() if not k.startswith("l")})
        check_level(st, sd, "level", l, 3, 2, [0, 1], forced=forced)
        soft(B.check_bitwise, f"level l{l} flow_up returned", up.cpu(), st.get(f"l{l}.flow_up"))
        soft(B.check_bitwise, f"level l{l} flow returned", out.cpu(), st.get(f"l{l}.flow"))
    flush()
    RAN.add("level")


def test_level6_zeros_survive_other_shapes(monkeypatch):
    """The zero fill of level 6's flow channels is launched once per (batch, map size): forward at shape A, at B, at A again, one
    eemplus_level call, A once more - the channels hold zeros every time."""
    pin(monkeypatch, {})
    net, _ = make_net(3, 128, 192, ("l6.", "l5.flow_init"))
    shapes = {"A": (1, 128, 192), "B": (2, 192, 256)}
    for step in ("A", "B", "A", "level", "A"):
        if step == "level":
            with torch.no_grad():
                net.level(5, net.stage("l5.flow_init") * 1.25)
            torch.cuda.synchronize()
            continue
        b, h, w = shapes[step]
        net.change_imagesize((h, w))
        forward(net, *inputs(7, b, h, w))
        z = net.stage("l6.cat_flow").cpu()
        assert z.shape[:2] == (b, 2)
        soft(B.check_bitwise, f"zeros after {step}", z, torch.zeros_like(z))
    flush()
    RAN.add("zeros")


# ------------------------------------------------------------------------------------------ the warps and the upsampling, directly
def last_form():
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.lib().eemplus_last_form(buf, 64))
    return buf.value.decode()


def stream():
    return _lib.current_stream_ptr(torch.device(DEV))


@pytest.mark.parametrize("h,w,seed", B.PL_WARP_CASES, ids=[f"{c[0]}x{c[1]}" for c in B.PL_WARP_CASES])
def test_warps_on_hostile_flows(monkeypatch, h, w, seed):
    """eemplus_warp, all three modes, on exact integer displacements, x.5, 1e-3 inside and outside every border, far outside, and the
    last partial block of pixels (fp64_bounds.pl_hostile_flows; tests/test_fp64_bounds_plus.py holds the reference to F.grid_sample
    on these very flows).  The input is positive, so the applied mask shows in the output and must equal the reference's exactly.
    Those flows are drawn so that the position (xn + 1) (w / 2) - 0.5 is the same number fused or not: on them a kernel that contracts
    that multiply-add cannot show.  So the first, unfiltered draw runs too (plain_only=False: 536 of 5550 positions at 25x37 depend
    on the contraction), against pl_warp_taps alone - warp_px.h's definition, with no F.grid_sample condition behind it; the host
    module shows that a contracting kernel fails there."""
    pin(monkeypatch, {})
    for plain_only in (True, False):
        flow = B.pl_hostile_flows(h, w, seed, plain_only=plain_only)
        n = flow.shape[0]
        x = torch.rand(n, 5, h, w, generator=torch.Generator().manual_seed(seed)) + 0.5
        xd, fd = x.to(DEV), flow.to(DEV)
        for mode in (0, 1, 2):
            out = torch.empty_like(xd)
            _lib.check(_lib.lib().eemplus_warp(xd.data_ptr(), fd.data_ptr(), n, 5, h, w, mode, out.data_ptr(), stream()))
            torch.cuda.synchronize()
            assert last_form() == "warp"
            SEEN.add("warp")
            soft(B.pl_check_warp, f"warp mode {mode} {h}x{w}{'' if plain_only else ' unfiltered'}", out.cpu(), x, flow, mode)
            if mode == 2:
                assert torch.equal(B.pl_mask_of(out.cpu()), B.pl_warp_taps(flow, 2)["mask"]), "the GPU's mask differs from the reference's"
    flush()
    RAN.add("warps")


@pytest.mark.parametrize("hw,out_hw", [((12, 18), (25, 37)), ((6, 9), (25, 37)), ((25, 37), (194, 290)), ((3, 4), (6, 9))])
def test_upsample_flow_as(monkeypatch, hw, out_hw):
    pin(monkeypatch, {})
    c = torch.randn(3, 2, *hw, generator=torch.Generator().manual_seed(21)) * 3
    for rate in (1, 0):
        inp = c.to(DEV).clone()
        out = torch.empty(3, 2, *out_hw, device=DEV)
        _lib.check(_lib.lib().eemplus_upsample_flow_as(inp.data_ptr(), 3, hw[0], hw[1], out_hw[0], out_hw[1], rate, out.data_ptr(), stream()))
        torch.cuda.synchronize()
        assert last_form() == ("scale_flow" if rate else "upflow")
        SEEN.update({"upflow", "scale_flow"})
        ref, mag = B.pl_upflow_ref(c, out_hw, rate=bool(rate))
        soft(B.check_roundings, f"upflow {hw} -> {out_hw} rate {rate}", out.cpu(), ref, mag, "upflow_rate" if rate else "upflow", form="upflow")
        if rate:
            ref, mag = B.pl_scale_ref(c, out_hw)
            soft(B.check_roundings, f"scale_flow {hw} -> {out_hw}", inp.cpu(), ref, mag, "scale", form="scale_flow scale")
        else:
            soft(B.check_bitwise, "the input without if_rate", inp.cpu(), c)
    flush()
    RAN.add("upsample")


# ------------------------------------------------------------------------------------------------------------------ coverage
def table():
    """The measured worst statistics per form, in the layout of the module docstring's table."""
    sums, kap, bit = {}, {}, [0, 0]
    for r in MYLOG:
        if "max_z" in r:
            s = sums.setdefault(r["form"], [0.0, 0.0, 0.0, 0.0, 0])
            for i, k in enumerate(("max_z", "rms_z", "mean_z", "slope_u")):
                s[i] = max(s[i], abs(r[k]))
            s[4] += 1
        elif "rms_ratio" in r:
            s = kap.setdefault(r["form"], [0.0] * 6 + [0])
            for i, k in enumerate(("rms_gpu", "max_gpu", "rms_cpu", "max_cpu", "rms_ratio", "max_ratio")):
                s[i] = max(s[i], r[k])
            s[6] += 1
        elif "differ" in r:
            bit[0] += 1
            bit[1] += r["differ"] > 0
    lines = ["    form                               held to        max|z|    rms   |mean|  |slope| u  checks"]
    for f, s in sorted(sums.items()):
        base = B.pl_base_form(f.split(" ")[0])[0]
        kind = f.split(" ")[1] if " " in f else None
        held = {"roundings": "roundings 3", "scale": "roundings 1"}.get(kind) or \
            {"warp": "roundings 4", "upflow": "roundings 6/7", "upflow_warp": "roundings 4/7", "upflow_multi": "roundings 7",
             "warp_blend_warp": "roundings 4", "scale_flow": "roundings 1"}.get(base)
        if held is None:
            held = B.pl_form_family(base)
        lines.append(f"    {f:<34} {held:<13} {s[0]:7.2f} {s[1]:6.3f} {s[2]:8.4f} {s[3]:9.3f} {s[4]:7d}")
    lines.append("Launches that end in the sigmoid blend (criterion 3): the GPU's error and the fp32 CPU evaluation's own, both against fp64")
    lines.append("    form of the launch                 GPU rms    GPU max    CPU rms    CPU max  rms ratio  max ratio  checks")
    for f, s in sorted(kap.items()):
        lines.append(f"    {f:<32} {s[0]:9.2e}  {s[1]:9.2e}  {s[2]:9.2e}  {s[3]:9.2e}  {s[4]:9.2f}  {s[5]:9.2f} {s[6]:7d}")
    lines.append(f"Bitwise comparisons: {bit[0]}, {'all equal' if not bit[1] else str(bit[1]) + ' differ'}.")
    return "\n".join(lines)


def test_every_form_is_known_and_was_seen():
    """Every form name the recorder reported is in the family tables; when the whole module ran, every form and fused launch of the
    path was exercised (what is not reachable is listed in the module docstring under LEFT OUT)."""
    print(table())
    for f in SEEN:
        assert f in B.PL_OTHER_FORMS or B.pl_form_family(f) in B.LIMITS, f
    if RAN >= CASES:
        assert PL_FORMS <= SEEN, sorted(PL_FORMS - SEEN)
        assert FUSED <= SEEN_FUSED, sorted(FUSED - SEEN_FUSED)
        jobs = {B.pl_base_form(r["form"]) for r in MYLOG if r.get("form", "").startswith("tail_")}
        assert {("tail_k1_g25", 1), ("tail_k1_g25", 2), ("tail_k3_g16", 2), ("tail_k3_g8", 3)} <= jobs, sorted(jobs)
