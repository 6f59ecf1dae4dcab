"""Every launch of E-RAFT's inference path against fp64, kernel form by kernel form.  `pytest -m gpu`.

eraft_forward drives about 45 encoder launches, the correlation pyramid and about 20 launches per update iteration.  Every case here pins
the EEM_* switches the E-RAFT dispatch reads, runs ONE forward with the stage recorder on (eraft_record_stages: a device copy of each
launch's output behind the launch, filed with the kernel form that wrote it), asserts from the recorder's list that the intended forms
ran, and holds every recorded launch to an fp64 evaluation of THAT launch on the GPU's own recorded input to it (oracle/fp64_bounds.py).
tests/test_fp64_bounds_eraft.py shows on the CPU that these checks reject fifteen planted faults and pass torch's fp32 evaluation.

LIMITS - none is fitted to the kernels under test:
  reused    launches that are plain sums (every convolution whose epilogue is none / ReLU / out_scale / the residual sum, all-pairs,
            pooling, the on-the-fly correlation's dot products) go through `check` under the family of the form that ran, in units of
            fp32 rounding of the launch's own sum of |terms|: gconv form names as tests/test_gpu_ops_fp64.py maps them (direct, bx3),
            "f4" -> wino4, "wnc" -> wino2, "stem7_c5" / "taps_7x7" / "allpairs_*" / "altcorr" -> direct, "pool2" / "pool2x3" -> pool.
            Launches that end in a nonlinear step (instance norm, the sigmoid and tanh epilogues, GEPI_ZR, GEPI_GRU, the softmax of the
            convex upsampling) go through `check_decoder`: rms and max error at most KAPPA_DEC = 6.4 x those of torch's fp32 CPU evaluation
            of the same launch on the same input, plus one unit of rounding at the largest output.
  derived   launches of a short fixed operation count are held to max|z| <= their number of roundings (fp64_bounds.ER_ROUNDINGS, derived
            there): pooling 3, the lookup's four-term blend 7, flow = coords1 - coords0 / coords1 + delta / r * h 1.  The lookup's sample
            position, floor and weights are the model's definition and are computed in fp32 as oracle/eraft_oracle.py does.
  bitwise   replicate padding; the recorder on against off.

SHAPES are the smallest that reach a form with tiles cut on the right and at the bottom, worked out from the dispatch code and confirmed
by the recorder; h / 8 and w / 8 stay >= 16 so that no pyramid level is one cell wide.  At the larger sizes the first and the last image
are checked.  The module's own padder fills up to multiples of 32, which makes every map a multiple of 4 cells a side: the forms for odd
maps (instnorm_plain, allpairs_l2 without its switch, allpairs_odd, ragged 25x37-cell update blocks) are reached by padding up to 8 on all
four sides instead, which eraft_forward accepts (make_net); the crop offsets of every prediction are then nonzero too.

LEFT OUT, and why:
  * 1/4-resolution planes above 81920 values (the two-pass instance norm at 96 channels): they need inputs above 1152 px a side.
  * eraft_forward_stream: it refuses the recorder (as it refuses eraft_get_stage's kept stages); its launches are those of
    forward_many, which tests/test_gpu_eraft_stream.py compares bit for bit.
  * the 64-channel convolutions of the 584x576 case: checked at the smaller sizes (the same kernels); that case checks the stem and
    every instance norm.
  * r itself under GEPI_ZR (the default): the launch stores only r * h; r is recorded and checked under EEM_ERAFT_NO_ZR=1.
  * an update block of fewer than 256 cells (16x15 for a 128x120 input): its coarsest pyramid level is one cell wide and the model divides by
    size - 1 = 0 there - every value behind the lookup is NaN, on the GPU as in the reference.  The launches that size selects (the
    generic kernel and er_sum_launch in place of GEPI_SUM2) run at 16x20 cells under EEM_NO_FEWOUT=1 (test_update_block_sum2_fallback).
  * the 60x80-cell update block (480x640) runs under the default configuration only; the other configurations run at 25x37 cells,
    where every launch of the block takes the same kernels with ragged tiles.

FOUND AND FIXED by this module:
  * the all-pairs kernels (allpairs_lds, allpairs_l2, allpairs_odd) gave rms(z) 2.84 / 2.84 / 2.83 / 2.85 in test_allpairs's four cases
    against the `direct` family's 0.98 (max|z| 13.6 - 16.4 of 20).  Each value was ONE chain of 128 v_mfma_f32_32x32x2_f32 accumulations
    over the 256 channels, and the feature maps have a per-channel mean, so the 256 products mostly share a sign (sum of terms = 0.8 x
    sum of |terms|): every addition rounded a partial sum that had grown steadily, 0.29 sqrt(256 / 3) = 2.7 u of sum |terms| rms.  The
    kernels now add the channels in runs of 32 into a second set of accumulators (ap_flush in eraft_kernels.hip): rms(z) 0.69, max|z|
    3.0 - 5.9, the three forms still bit for bit the same, E-RAFT's forward time unchanged (640x480 and 1280x720 x 12, within 0.5 %).
    The same arithmetic in altcorr_kernel's dot product measured 1.9 - 2.0 and is 0.53 since it adds eight partial sums pairwise.
  * the lookup's FLAT instantiations formed the bilinear weight tx = ix - floor(ix) by a fused multiply-add
from the unrounded product ix = ((xn + 1) / 2) (w - 1): beside an integer coordinate - every pixel of the first iteration - a neighbouring
cell got a weight of +-1e-6 instead of 0 (max|z| 11 - 33 at benign coordinates, 1e4 - 6e6 where the neighbour is much larger or a weight
is 1e-3), where the model rounds ix first.  sample_axis() in eraft_kernels.hip now keeps contraction out of the position arithmetic.

MEASURED worst statistics per form (one AMD Instinct MI355X, gfx950, 256 CUs).  A record: these numbers set no limit.
Sums and short operation counts (criteria 1 and 2), the worst over all checks of the module:
    form                               held to        max|z|    rms   |mean|  |slope| u  checks
    allpairs_l2                        direct           4.53  0.695   0.0029     0.582       5
    allpairs_lds                       direct           2.99  0.695   0.0025     0.003       1
    allpairs_odd                       direct           5.93  0.694   0.0004     0.573       4
    altcorr                            direct           8.82  0.531   0.0080     0.019       4
    axpy sum                           roundings 1      0.99  0.434   0.0118     0.014       3
    convex_up_fused sum                roundings 1      0.99  0.434   0.0118     0.014       5
    f4                                 wino4           76.68  2.248   0.0271     0.959      10
    fewout_wide2                       direct           0.78  0.125   0.0089     0.167      32
    fewout_wide2 sum                   roundings 1      1.00  0.439   0.0118     0.026      24
    flow flow                          roundings 1      0.00  0.000   0.0000     0.000       6
    gconv16_1x1_s2                     direct           6.67  0.485   0.0161     0.364      13
    gconv16_1x1_th2_wm4_kg1            direct           4.41  0.312   0.0015     0.038       2
    gconv16_1x1_th2_wm4_kg2            direct           3.43  0.345   0.0020     0.027       4
    gconv16_1x1_th3_wm4_kg2            direct           2.79  0.335   0.0013     0.010       2
    gconv16_1x1_th5_wm4_kg1            direct           5.38  0.495   0.0011     0.040       2
    gconv16_1x1_th5_wm4_kg2            direct           3.62  0.202   0.0002     0.022       2
    gconv16_1x1_th6_wm4_kg1            direct           5.45  0.481   0.0021     0.013       2
    gconv16_1x5_th2_wm4_kg2            direct           2.27  0.320   0.0033     0.080       2
    gconv16_3x3_s2                     direct           6.36  0.464   0.0050     0.072      13
    gconv16_3x3_th2_wm4_kg2            direct           3.78  0.347   0.0411     1.716      31
    gconv16_3x3_th3_wm4_kg2            direct           4.51  0.345   0.0046     0.389       6
    gconv16_3x3_th4_wm4_kg1            direct           5.00  0.323   0.0095     0.104       4
    gconv16_3x3_th4_wm4_kg2            direct           3.60  0.345   0.0015     0.036       4
    gconv16_3x3_th6_wm4_kg1            direct           6.70  0.485   0.0091     0.098      10
    gconv16_5x1_th2_wm4_kg2            direct           2.26  0.324   0.0024     0.091       2
    gconvb_3x3_th4                     bx3              5.67  0.425   0.0547     2.360      13
    generic_1x1                        direct           4.76  0.471   0.0021     0.032       2
    generic_splitk16                   direct           0.51  0.124   0.0041     0.207       2
    generic_splitk4                    direct           2.30  0.263   0.0033     0.170     167
    generic_splitk8                    direct           1.18  0.181   0.0089     0.097      32
    lookup_cond16                      roundings 7      3.69  0.655   0.0088     0.012       3
    lookup_cond16 flow                 roundings 1      0.00  0.000   0.0000     0.000       2
    lookup_cond32                      roundings 7      3.69  0.655   0.0088     0.012       3
    lookup_cond32 flow                 roundings 1      0.00  0.000   0.0000     0.000       2
    lookup_cond64                      roundings 7      3.69  0.655   0.0088     0.012       3
    lookup_cond64 flow                 roundings 1      0.00  0.000   0.0000     0.000       2
    lookup_flat16                      roundings 7      4.03  0.600   0.0043     0.005      39
    lookup_flat16 flow                 roundings 1      0.86  0.053   0.0009     0.000      36
    lookup_flat32                      roundings 7      3.20  0.455   0.0021     0.003       3
    lookup_flat32 flow                 roundings 1      0.00  0.000   0.0000     0.000       2
    lookup_flat64                      roundings 7      3.20  0.465   0.0008     0.003       3
    lookup_flat64 flow                 roundings 1      0.00  0.000   0.0000     0.000       2
    mul_channels                       roundings 1      1.00  0.253   0.0010     0.008       4
    pool2                              pool             2.25  0.659   0.0082     0.037       9
    pool2 roundings                    roundings 3      2.25  0.659   0.0082     0.037       9
    pool2x3                            pool             2.17  0.659   0.0211     0.020      84
    pool2x3 roundings                  roundings 3      2.17  0.659   0.0211     0.020      84
    stem7_c5                           direct           6.88  0.454   0.0219     0.240      11
    sum sum                            roundings 1      1.00  0.425   0.0156     0.003       2
    taps_7x7                           direct           5.39  0.452   0.0226     0.237      36
    wnc                                wino2            3.57  0.358   0.0101     0.518      24
Launches that end in a nonlinear step (criterion 3): the GPU's error and the fp32 CPU oracle's own on the same input, both against fp64
(worst over the checks; the ratios are the worst of any one check, at most KAPPA_DEC = 6.4):
    form of the launch                 GPU rms    GPU max    CPU rms    CPU max  rms ratio  max ratio  checks
    convex_up                         3.90e-07   2.94e-06   4.17e-07   3.70e-06       0.98       1.13      27
    convex_up_fused                   2.59e-07   2.59e-06   2.66e-07   2.28e-06       0.97       1.13       5
    gconv16_1x1_th2_wm4_kg2           1.78e-07   3.52e-06   1.63e-07   3.02e-06       1.09       1.17       1
    gconv16_1x5_th2_wm4_kg2           5.04e-07   2.55e-05   3.08e-07   1.03e-05       1.65       2.55       6
    gconv16_1x5_th3_wm4_kg2           4.94e-07   3.36e-05   3.22e-07   2.29e-05       1.53       2.07       2
    gconv16_1x5_th4_wm4_kg2           6.34e-07   5.26e-05   3.89e-07   1.94e-05       1.63       2.81       2
    gconv16_5x1_th2_wm4_kg2           4.80e-07   2.03e-05   3.20e-07   1.33e-05       1.61       2.28       6
    gconv16_5x1_th3_wm4_kg2           6.35e-07   3.66e-05   3.54e-07   1.99e-05       1.84       1.98       2
    gconv16_5x1_th4_wm4_kg2           5.80e-07   3.46e-05   3.65e-07   2.24e-05       1.60       1.54       2
    gconvb_1x5_th4                    4.12e-07   1.44e-05   1.99e-07   7.17e-06       2.09       2.67       8
    gconvb_5x1_th4                    3.51e-07   2.11e-05   1.86e-07   6.37e-06       1.99       3.81       8
    generic_splitk4                   7.70e-07   4.67e-05   3.67e-07   2.55e-05       2.37       3.41     168
    instnorm_2pass                    1.58e-07   1.41e-06   2.41e-07   1.09e-06       1.33       1.77       6
    instnorm_plain                    7.46e-08   7.90e-07   5.12e-08   6.56e-07       1.51       1.59       5
    instnorm_reg20                    5.28e-07   2.30e-06   2.25e-07   9.74e-07       2.35       2.41       9
    instnorm_reg5                     1.05e-07   1.05e-06   5.71e-08   7.10e-07       2.03       2.30      54
Bitwise comparisons: 14, all equal.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from eemflow_amd import _lib, ops
from eemflow_amd.eraft import ERAFT
from eemflow_amd.eraft_weights import seeded_from_shapes
from eemflow_amd.padder import InputPadder
from eemflow_amd.weights import synthetic_voxel_pair
from oracle import eemflow_oracle as O
from oracle import eraft_oracle as R
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every EEM_* switch the E-RAFT dispatch reads (eraft_api.hip, eraft_kernels.hip, gconv*.hip, conv_stem7.hip, conv_wnc.hip, conv_wino4.hip)
SWITCHES = ("EEM_ALLPAIRS_L2", "EEM_ERAFT_NO_F4", "EEM_ERAFT_NO_FUSE", "EEM_ERAFT_NO_LAG", "EEM_ERAFT_NO_OVERLAP", "EEM_ERAFT_NO_PRE",
            "EEM_ERAFT_NO_STACK", "EEM_ERAFT_NO_WNC", "EEM_ERAFT_NO_ZR", "EEM_ERAFT_WNC_UPD", "EEM_FEWOUT_SMALL_BLOCKS", "EEM_FEWOUT_WIDE",
            "EEM_GB_DBG", "EEM_GCONVB_1X1", "EEM_GCONVB_MINBLK", "EEM_GCONVB_RING", "EEM_LOOKUP_PX", "EEM_NO_FEWOUT", "EEM_NO_G16_S2",
            "EEM_NO_GCONV16", "EEM_NO_GCONVB", "EEM_NO_SPLITK", "EEM_NO_STEM7", "EEM_NO_TAPS_KERNEL", "EEM_NO_WNC", "EEM_POOL_CHAIN",
            "EEM_SPLITK_MAX")

# the forms of the E-RAFT helper launches and of the Winograd / stem launches: the last test wants every one of them seen
ER_FORMS = {"instnorm_plain", "instnorm_reg5", "instnorm_reg20", "instnorm_2pass", "allpairs_lds", "allpairs_l2", "allpairs_odd",
            "pool2x3", "pool2", "lookup_flat16", "lookup_flat32", "lookup_flat64", "lookup_cond16", "lookup_cond32", "lookup_cond64",
            "altcorr", "convex_up", "convex_up_fused", "f4", "wnc", "stem7_c5", "taps_7x7", "pad", "pad4", "pad4_pair"}
# ... and every fused epilogue eraft_forward uses
EPILOGUES = {"GEPI_ZR", "GEPI_GRU", "GEPI_MUL", "GEPI_ADD_RELU", "GEPI_SUM2", "pre", "sigmoid", "tanh", "out_scale"}
SEEN, SEEN_EPI, RAN = set(), set(), set()


ERRS = []


def soft(check, *args, **kw):
    """A check whose StageError is kept for `flush`: one run names every failing launch of a forward, not the first."""
    try:
        return check(*args, **kw)
    except B.StageError as e:
        ERRS.append(str(e))
        return None


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


def make_net(seed, h, w, record, iters=2, **attrs):
    net = ERAFT("", 5).eval()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = seeded_from_shapes(shapes, seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.record_stages = (tuple(record), iters) if record is not None else None
    for k, v in attrs.items():
        setattr(net, k, v)
    net = net.to(DEV)
    net.change_imagesize((h, w))
    # E-RAFT's own padder fills up to multiples of 32, which makes every map a multiple of 4 cells a side; eraft_forward takes any padding
    # to a multiple of 8, and the forms for odd maps (17x25, 25x37 cells) are reached with exactly that: up to 8, on all four sides
    net.image_padder = InputPadder((h, w), mode="sintel", eval_pad_rate=8)
    return net, O.to_torch_sd(sd)


class Stages:
    """The recorder's list of the module's last forward, and its tensors on the CPU (fetched once each)."""

    def __init__(self, net):
        torch.cuda.synchronize()
        self.net = net
        self.names = {name: (form, dims) for name, form, dims in net.stage_names()}
        self.cache = {}
        for name, (form, _) in self.names.items():
            if form:
                SEEN.add(form)

    def __contains__(self, name):
        return name in self.names

    def form(self, name):
        return self.names[name][0]

    def forms(self, prefix=""):
        return {f for n, (f, _) in self.names.items() if n.startswith(prefix) and f}

    def get(self, name):
        if name not in self.cache:
            assert name in self.names, (name, sorted(self.names))
            t = self.net.stage(name).cpu()
            assert tuple(t.shape) == self.names[name][1], (name, t.shape, self.names[name])
            self.cache[name] = t
        return self.cache[name]


def forward(net, e1, e2, iters=2, flow_init=None, many=False):
    with torch.no_grad():
        if many:
            outs = net.forward_many([(e1[i:i + 1].to(DEV), e2[i:i + 1].to(DEV)) for i in range(e1.shape[0])], iters=iters)
            preds = [torch.cat([o[1][k] for o in outs]) for k in range(len(outs[0][1]))]
        else:
            preds = net(e1.to(DEV), e2.to(DEV), iters=iters, flow_init=flow_init.to(DEV) if flow_init is not None else None)[1]
    torch.cuda.synchronize()
    return [p.cpu() for p in preds]


def inputs(seed, b, h, w):
    return tuple(torch.from_numpy(a) for a in synthetic_voxel_pair(seed, b, h, w))


def conv_w(sd, name, co=None, ci=None):
    w, b = sd[name + ".weight"], sd[name + ".bias"]
    if co is not None:
        w, b = w[co], b[co]
    if ci is not None:
        w = w[:, ci]
    return w, b


def kappa(name, form, got, ref64, ref32):
    rec = soft(B.check_decoder, name, got, ref64, ref32)
    B.LOG[-1]["form"] = form
    return rec


# ----------------------------------------------------------------------------------------------------------------- the encoders
BLOCKS = [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)]


def check_encoder(st, sd, tag, x, imgs, cimgs=None, blocks=BLOCKS, stem=True, convs=True, name=""):
    """Every recorded launch of one encoder (tag "fnet." / "cnet.") on its input x, the padded volumes [n, 5, hp, wp] (CPU), for the
    images `imgs` (the convolutions: `cimgs`).  fnet: conv, then the instance norm in its three roles; cnet: conv with the eval
    BatchNorm, ReLU and the residual sum folded in."""
    inst = tag == "fnet."
    cimgs = imgs if cimgs is None else cimgs
    sub = [imgs.index(i) for i in cimgs]                                    # (cimgs within imgs)
    roles = set()

    def bn(prefix):
        return None if inst else B.er_bn_fold(sd, prefix)

    def conv(nm, src, wname, stride, padding, bnp, res=None):
        if not (convs or nm == tag + "conv1") or nm not in st:
            return
        w, b = conv_w(sd, wname)
        ref, mag = B.er_conv_ref([src[sub]], w, b, stride=stride, padding=padding, bn=bn(bnp), relu=not inst, res=res[sub] if res is not None else None)
        soft(B.er_check_form, f"{name} {nm}", st.form(nm), st.get(nm)[cimgs], ref, mag)
        if res is not None:
            SEEN_EPI.add("GEPI_ADD_RELU")

    def norm(nm, src, relu, res=None):
        if nm not in st:
            return None
        kappa(f"{name} {nm}", st.form(nm), st.get(nm)[imgs], B.er_instnorm_ref(src, relu, res), B.er_instnorm_ref(src, relu, res, torch.float32))
        roles.add((st.form(nm), "residual" if res is not None else "relu" if relu else "plain"))
        return st.get(nm)[imgs]

    def out(nm_conv, nm_norm):
        """The tensor the next launch reads: the norm's output (fnet) or the conv's own (cnet), as recorded."""
        nm = nm_norm if inst else nm_conv
        return st.get(nm)[imgs] if nm in st else None

    if stem:
        conv(tag + "conv1", x[imgs], tag + "conv1", 2, (3, 3), tag + "norm1.")
        if inst and tag + "conv1" in st:
            norm(tag + "norm1", st.get(tag + "conv1")[imgs], True)
    cur = out(tag + "conv1", tag + "norm1")
    for l, r in blocks:
        p = f"{tag}layer{l}.{r}."
        if cur is None:                                                      # (the block's input was not recorded: start at the next)
            cur = out(p + "conv2", p + "norm2")
            continue
        stride = 2 if (r == 0 and l > 1) else 1
        conv(p + "conv1", cur, p + "conv1", stride, (1, 1), p + "norm1.")
        if inst and p + "conv1" in st:
            norm(p + "norm1", st.get(p + "conv1")[imgs], True)
        y = out(p + "conv1", p + "norm1")
        res = cur
        if stride == 2:
            if inst:
                w, b = conv_w(sd, p + "downsample.0")
                if convs and p + "down" in st:
                    ref, mag = B.er_conv_ref([cur[sub]], w, b, stride=2, padding=(0, 0))
                    soft(B.er_check_form, f"{name} {p}down", st.form(p + "down"), st.get(p + "down")[cimgs], ref, mag)
                res = norm(p + "norm3", st.get(p + "down")[imgs], False) if p + "down" in st else None
            else:
                if convs and p + "down" in st:
                    w, b = conv_w(sd, p + "downsample.0")
                    ref, mag = B.er_conv_ref([cur[sub]], w, b, stride=2, padding=(0, 0), bn=bn(p + "norm3."))
                    soft(B.er_check_form, f"{name} {p}down", st.form(p + "down"), st.get(p + "down")[cimgs], ref, mag)
                res = st.get(p + "down")[imgs] if p + "down" in st else None
        if y is not None and res is not None:
            if inst:
                conv(p + "conv2", y, p + "conv2", 1, (1, 1), None)
                if p + "conv2" in st:
                    norm(p + "norm2", st.get(p + "conv2")[imgs], True, res)
            else:
                conv(p + "conv2", y, p + "conv2", 1, (1, 1), p + "norm2.", res=res)
        cur = out(p + "conv2", p + "norm2")
    return roles, cur


def check_heads(st, sd, feat_f, feat_c, fimgs, cimgs, name):
    """fmap, net0 (tanh), inp (ReLU) and the context features' share of the GRU convs (czr / cq)."""
    if feat_f is not None and "fmap" in st:
        w, b = conv_w(sd, "fnet.conv2")
        ref, mag = B.er_conv_ref([feat_f], w, b, padding=(0, 0))
        soft(B.er_check_form, f"{name} fmap", st.form("fmap"), st.get("fmap")[fimgs], ref, mag)
    if feat_c is not None and "net0" in st:
        w, b = conv_w(sd, "cnet.conv2", co=slice(0, 128))
        v64, _ = B.er_conv_ref([feat_c], w, b, padding=(0, 0))
        kappa(f"{name} net0", st.form("net0"), st.get("net0")[cimgs], torch.tanh(v64), torch.tanh(B.er_conv_f32([feat_c], w, b, padding=(0, 0))))
        SEEN_EPI.add("tanh")
        w, b = conv_w(sd, "cnet.conv2", co=slice(128, 256))
        ref, mag = B.er_conv_ref([feat_c], w, b, padding=(0, 0), relu=True)
        soft(B.er_check_form, f"{name} inp", st.form("inp"), st.get("inp")[cimgs], ref, mag)
    for p, (k, padding) in enumerate((("1", (0, 2)), ("2", (2, 0)))):
        if f"czr{p}" not in st:
            continue
        inp = st.get("inp")[cimgs]
        wz, bz = conv_w(sd, "update_block.gru.convz" + k, ci=slice(128, 256))
        wr, br = conv_w(sd, "update_block.gru.convr" + k, ci=slice(128, 256))
        ref, mag = B.er_conv_ref([inp], torch.cat([wz, wr]), torch.cat([bz, br]), padding=padding)
        soft(B.er_check_form, f"{name} czr{p}", st.form(f"czr{p}"), st.get(f"czr{p}")[cimgs], ref, mag)
        wq, bq = conv_w(sd, "update_block.gru.convq" + k, ci=slice(128, 256))
        ref, mag = B.er_conv_ref([inp], wq, bq, padding=padding)
        soft(B.er_check_form, f"{name} cq{p}", st.form(f"cq{p}"), st.get(f"cq{p}")[cimgs], ref, mag)


# ------------------------------------------------------------------------------------------------------- pyramid, lookup, update
def rows(t, imgs, hw):
    """The [B * hw, ...] rows of the images `imgs`."""
    return torch.cat([t[i * hw:(i + 1) * hw] for i in imgs])


def check_pyramid(st, b, imgs, name, fmap=True):
    h8, w8 = st.names["pyr0"][1][2:]
    hw = h8 * w8
    pyr = [rows(st.get(f"pyr{l}"), imgs, hw) for l in range(4)]
    if fmap:
        fm = st.get("fmap")
        ref, mag = B.er_allpairs_ref(fm[imgs], fm[[b + i for i in imgs]])
        soft(B.er_check_form, f"{name} pyr0", st.form("pyr0"), pyr[0], ref, mag)
    for l in (1, 2, 3):
        ref, mag = B.avg_pool_ref(pyr[l - 1], 2)
        soft(B.er_check_form, f"{name} pyr{l}", st.form(f"pyr{l}"), pyr[l], ref, mag)
        soft(B.check_roundings, f"{name} pyr{l}", pyr[l], ref, mag, "pool", form=st.form(f"pyr{l}") + " roundings")
    return pyr


def check_lookup(st, it, pyr, imgs, c0, name, alt=None):
    """it<K>.corr from it<K>.coords1_in and the GPU's own pyramid (alt: (fmap1, [fmap2 and its pooled levels]): the on-the-fly form),
    and the flow = coords1 - coords0 the same launch (or er_flow_launch) writes."""
    c1 = st.get(f"it{it}.coords1_in")[imgs]
    corr = st.get(f"it{it}.corr")[imgs]
    form = st.form(f"it{it}.corr")
    if alt is not None:
        ref, mag = B.er_altcorr_ref(alt[0], alt[1], c1)
        soft(B.er_check_form, f"{name} it{it}.corr", form, corr, ref, mag)
    else:
        ref, mag = B.er_lookup_ref(pyr, c1)
        soft(B.check_roundings, f"{name} it{it}.corr", corr, ref, mag, "lookup", form=form)
    flow = st.get(f"it{it}.flow")[imgs]
    soft(B.check_roundings, f"{name} it{it}.flow", flow, c1.double() - c0.double(), c1.double().abs() + c0.double().abs(), "flow",
                      form=st.form(f"it{it}.flow") + " flow")
    return c1, corr, flow


def check_iteration(st, sd, it, hprev, pyr, imgs, c0, pad, size, name, emit=True, alt=None):
    """Every recorded launch of update iteration `it` (model/update.py:97-106, model/eraft.py:141-157); hprev: the hidden state it
    reads.  Returns the state it leaves."""
    p = f"it{it}."
    u = "update_block."
    g = lambda n: st.get(p + n)[imgs]                                        # noqa: E731
    f = lambda n: st.form(p + n)                                             # noqa: E731
    c1, corr, flow = check_lookup(st, it, pyr, imgs, c0, name, alt)

    def plain(nm, xs, wname, padding, relu=True, out_scale=1.0, co=None):
        w, b = conv_w(sd, u + wname, co=co)
        ref, mag = B.er_conv_ref(xs, w, b, padding=padding, relu=relu, out_scale=out_scale)
        soft(B.er_check_form, f"{name} {p}{nm}", f(nm), g(nm), ref, mag)

    plain("flo1", [flow], "encoder.convf1", (3, 3))
    plain("corflo.f", [g("flo1")], "encoder.convf2", (1, 1))
    plain("cor1", [corr], "encoder.convc1", (0, 0))
    plain("corflo.c", [g("cor1")], "encoder.convc2", (1, 1))
    plain("motion", [g("corflo.c"), g("corflo.f")], "encoder.conv", (1, 1))
    motion = torch.cat([g("motion"), flow], 1)
    inp = st.get("inp")[imgs]
    h = hprev
    for k, (sfx, padding) in enumerate((("1", (0, 2)), ("2", (2, 0)))):
        gp = f"gru{k}."
        wz, bz = conv_w(sd, u + "gru.convz" + sfx)
        wr, br = conv_w(sd, u + "gru.convr" + sfx)
        wq, bq = conv_w(sd, u + "gru.convq" + sfx)
        hm = lambda w: torch.cat([w[:, :128], w[:, 256:]], 1)                # noqa: E731  (the [h | motion] columns)
        use_pre = f"czr{k}" in st
        if use_pre:                                                          # the context share comes from the GPU's own czr / cq
            czr, cq = st.get(f"czr{k}")[imgs], st.get(f"cq{k}")[imgs]
            vz64, _ = B.er_conv_ref([h, motion], hm(torch.cat([wz, wr])), None, padding=padding, pre=czr)
            vz32 = B.er_conv_f32([h, motion], hm(torch.cat([wz, wr])), None, padding=padding, pre=czr)
            SEEN_EPI.add("pre")
        else:
            vz64, _ = B.er_conv_ref([h, inp, motion], torch.cat([wz, wr]), torch.cat([bz, br]), padding=padding)
            vz32 = B.er_conv_f32([h, inp, motion], torch.cat([wz, wr]), torch.cat([bz, br]), padding=padding)
        kappa(f"{name} {p}{gp}z", f(gp + "z"), g(gp + "z"), torch.sigmoid(vz64[:, :128]), torch.sigmoid(vz32[:, :128]))
        SEEN_EPI.add("sigmoid")
        if p + gp + "r" in st:                                               # r stored by itself, r * h by the elementwise launch
            r = g(gp + "r")
            kappa(f"{name} {p}{gp}r", f(gp + "r"), r, torch.sigmoid(vz64[:, 128:]), torch.sigmoid(vz32[:, 128:]))
            ref = r.double() * h.double()
            soft(B.check_roundings, f"{name} {p}{gp}rh", g(gp + "rh"), ref, ref.abs(), "mul", form=f(gp + "rh"))
        else:
            kappa(f"{name} {p}{gp}rh", f(gp + "rh"), g(gp + "rh"), torch.sigmoid(vz64[:, 128:]) * h.double(), torch.sigmoid(vz32[:, 128:]) * h)
            SEEN_EPI.add("GEPI_ZR" if STACKED[0] else "GEPI_MUL")         # (z | r as one launch, or r's own launch)
        z, rh = g(gp + "z"), g(gp + "rh")
        if use_pre:
            vq64, _ = B.er_conv_ref([rh, motion], hm(wq), None, padding=padding, pre=cq)
            vq32 = B.er_conv_f32([rh, motion], hm(wq), None, padding=padding, pre=cq)
        else:
            vq64, _ = B.er_conv_ref([rh, inp, motion], wq, bq, padding=padding)
            vq32 = B.er_conv_f32([rh, inp, motion], wq, bq, padding=padding)
        kappa(f"{name} {p}{gp}h", f(gp + "h"), g(gp + "h"), B.er_gru_blend_ref(z.double(), h.double(), torch.tanh(vq64)),
              B.er_gru_blend_ref(z, h, torch.tanh(vq32)))
        SEEN_EPI.add("GEPI_GRU")
        h = g(gp + "h")
    plain("fhid", [h], "flow_head.conv1", (1, 1))
    plain("delta", [g("fhid")], "flow_head.conv2", (1, 1), relu=False)
    delta, c1n = g("delta"), g("coords1_out")
    soft(B.check_roundings, f"{name} {p}coords1_out", c1n, c1.double() + delta.double(), c1.double().abs() + delta.double().abs(), "sum",
                      form=f("coords1_out") + " sum")
    if f("coords1_out").startswith("fewout"):
        SEEN_EPI.add("GEPI_SUM2")
    if emit:
        plain("mhid", [h], "mask.0", (1, 1))
        plain("mask", [g("mhid")], "mask.2", (0, 0), relu=False, out_scale=0.25)
        SEEN_EPI.add("out_scale")
        fl = c1n.double() - c0.double()                                     # (exact in fp64; the model rounds it to fp32 once)
        ref64 = B.er_convex_up_ref(fl.float(), g("mask"), pad, size)
        ref32 = B.er_convex_up_ref(fl.float(), g("mask"), pad, size, torch.float32)
        kappa(f"{name} {p}pred", f("pred"), g("pred"), ref64, ref32)
    else:
        assert p + "mask" not in st and p + "pred" not in st
    return h


STACKED = [True]        # whether the running case stacks z | r into one launch (EEM_ERAFT_NO_STACK unset): tells GEPI_ZR from GEPI_MUL

UPDATE_RECORD = ("net0", "inp", "czr", "cq", "pyr", "it")


def run_update_case(monkeypatch, env, b, h, w, seed, imgs, iters=2, attrs=None, flow_init=False, many=False, name="", want=(), record=UPDATE_RECORD):
    pin(monkeypatch, env)
    STACKED[0] = env.get("EEM_ERAFT_NO_STACK") != "1"
    net, sd = make_net(seed, h, w, record, iters, **(attrs or {}))
    e1, e2 = inputs(seed + 1, b, h, w)
    pad = net.image_padder._pad
    h8, w8 = (h + pad[2] + pad[3]) // 8, (w + pad[0] + pad[1]) // 8
    fi = None
    if flow_init:
        fi = torch.randn(b, 2, h8, w8, generator=torch.Generator().manual_seed(seed + 2)) * 1.5
    preds = forward(net, e1, e2, iters, fi, many)
    st = Stages(net)
    final_only = bool((attrs or {}).get("final_only"))
    assert len(preds) == (1 if final_only else iters)
    for f in want:
        assert f in st.forms(), (f, sorted(st.forms()))
    c0 = R.coords_grid(len(imgs), h8, w8)
    pyr = check_pyramid(st, b, imgs, name, fmap=False)
    if fi is not None:
        c1 = st.get("it0.coords1_in")[imgs]
        assert torch.equal(c1, c0 + fi[imgs]), "coords1 = coords0 + flow_init is one exact fp32 sum"
    hid = st.get("net0")[imgs]
    for it in range(iters):
        if it:
            assert torch.equal(st.get(f"it{it}.coords1_in"), st.get(f"it{it - 1}.coords1_out")), "the rotating coords1 buffers"
        emit = not final_only or it == iters - 1
        hid = check_iteration(st, sd, it, hid, pyr, imgs, c0, pad, (h, w), name, emit=emit)
        if emit:                                                             # what the caller got is what the recorder saw
            assert torch.equal(st.get(f"it{it}.pred"), preds[0 if final_only else it])
    flush()
    return st


def test_update_block_60x80(monkeypatch):
    run_update_case(monkeypatch, {}, 1, 480, 640, 31, [0], name="upd 60x80", want=("lookup_flat16", "convex_up"))
    RAN.add("upd 60x80")


UPD_CONFIGS = {
    "default": ({}, {}, ("convex_up",)),
    "no_overlap": ({"EEM_ERAFT_NO_OVERLAP": "1"}, {}, ("convex_up_fused",)),
    "no_lag": ({"EEM_ERAFT_NO_LAG": "1"}, {}, ("convex_up_fused",)),
    "no_fuse": ({"EEM_ERAFT_NO_FUSE": "1"}, {}, ("convex_up", "axpy", "flow")),
    "no_stack": ({"EEM_ERAFT_NO_STACK": "1"}, {}, ()),
    "no_pre": ({"EEM_ERAFT_NO_PRE": "1"}, {}, ()),
    "no_zr": ({"EEM_ERAFT_NO_ZR": "1"}, {}, ("mul_channels",)),
    "wnc_upd7": ({"EEM_ERAFT_WNC_UPD": "7"}, {}, ()),
    "wnc_upd0": ({"EEM_ERAFT_WNC_UPD": "0"}, {}, ()),
    "final_only": ({}, {"final_only": True}, ()),
    "final_only_no_lag": ({"EEM_ERAFT_NO_LAG": "1"}, {"final_only": True}, ("axpy",)),
    "forward_many": ({}, {}, ("pad4",)),
    "frames_in_flight4": ({}, {"frames_in_flight": 4}, ()),
    "flow_init": ({}, {}, ()),
}


@pytest.mark.parametrize("config", list(UPD_CONFIGS))
def test_update_block_25x37(monkeypatch, config):
    """194x290 is padded to 200x296 (3 px a side: the prediction's crop offsets are nonzero), 25x37 cells: every tile of the block ragged."""
    env, attrs, want = UPD_CONFIGS[config]
    st = run_update_case(monkeypatch, env, 2, 194, 290, 41, [1], attrs=attrs, flow_init=config == "flow_init", many=config == "forward_many",
                         name=f"upd 25x37 {config}", want=want, record=UPDATE_RECORD + (("pad",) if config == "forward_many" else ()))
    RAN.add(f"upd {config}")
    if config == "wnc_upd7":                                                 # 37 columns: w % 4 != 0, the Winograd kernel does not qualify
        assert "wnc" not in st.forms("it0."), st.forms("it0.")
    if config == "no_stack":
        assert "GEPI_MUL" in SEEN_EPI


def test_update_block_wnc_all_three(monkeypatch):
    """EEM_ERAFT_WNC_UPD=7 where the F(2x2) kernel qualifies (w % 4 == 0 and 128 (tile, slice) pairs: 32x40 cells at batch 4, the
    second 32-column tile cut at 8): convc2, convf2 and conv, each into its channel slice of a wider buffer.  The last image is checked."""
    st = run_update_case(monkeypatch, {"EEM_ERAFT_WNC_UPD": "7"}, 4, 256, 320, 43, [3], name="upd 32x40 wnc7")
    assert {st.form("it0.corflo.c"), st.form("it0.corflo.f"), st.form("it0.motion")} == {"wnc"}, st.forms("it0.")
    pin(monkeypatch, {})                                                     # the default mask: convf2 alone
    net, _ = make_net(43, 256, 320, ("it0.corflo", "it0.motion"), 1)
    forward(net, *inputs(44, 4, 256, 320), iters=1)
    st = Stages(net)
    assert st.form("it0.corflo.f") == "wnc" and st.form("it0.corflo.c") != "wnc" and st.form("it0.motion") != "wnc", st.names
    RAN.add("upd wnc7")


def test_update_block_sum2_fallback(monkeypatch):
    """Where the few-cout kernel does not serve the flow head's last conv, GEPI_SUM2 falls back to the generic kernel and coords1 + delta
    to the separate sum launch.  The dispatch takes that path below 256 cells - but a map of fewer than 256 cells has a side below 16
    (16x15 for a 128x120 input), its coarsest pyramid level is one cell wide, and there the model itself divides by size - 1 = 0: every
    value behind the lookup is NaN, on the GPU as in the reference.  EEM_NO_FEWOUT=1 takes the same path at 16x20 cells."""
    st = run_update_case(monkeypatch, {"EEM_NO_FEWOUT": "1"}, 2, 128, 160, 45, [0, 1], name="upd 16x20 no fewout")
    assert st.form("it0.coords1_out") == "sum" and not st.form("it0.delta").startswith("fewout"), (st.form("it0.coords1_out"), st.form("it0.delta"))
    RAN.add("sum2 fallback")


# --------------------------------------------------------------------------------------------------------------- encoder cases
def offset_stem_bias(net, sd, e1, sds=10.0):
    """A stem bias that puts every plane's mean about `sds` standard deviations from zero (a legitimate state dict: where one-pass
    variance loses digits)."""
    pad = net.image_padder._pad
    y = F.conv2d(O.replicate_pad(e1[:1], pad), sd["fnet.conv1.weight"], None, stride=2, padding=3)
    bias = sds * y.std((0, 2, 3)) * torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    sd = dict(sd)
    sd["fnet.conv1.bias"] = bias.float()
    with torch.no_grad():
        net.fnet.conv1.bias.copy_(bias.to(DEV))
    return sd


ENC_CASES = {
    # name: (env, batch, h, w, record, iterations of `iters`, images, conv images, offset, forms that must have run)
    "reg5_stem7": ({}, 1, 128, 160, ("pad", "fnet.", "cnet.", "fmap", "net0", "inp", "czr", "cq"), [0], None, False, {"instnorm_reg5", "stem7_c5", "pad4_pair"}),
    "taps": ({"EEM_NO_STEM7": "1"}, 1, 128, 160, ("pad", "fnet.conv1", "cnet.conv1"), [0], None, False, {"taps_7x7"}),
    "reg20": ({}, 1, 256, 352, ("pad", "fnet."), [0], None, False, {"instnorm_reg20", "instnorm_reg5"}),
    "reg20_offset": ({}, 1, 256, 352, ("pad", "fnet.conv1", "fnet.norm1"), [0], None, True, {"instnorm_reg20"}),
    "plain": ({}, 1, 136, 200, ("pad", "fnet.", "fmap"), [0], None, False, {"instnorm_plain", "instnorm_reg5"}),
    "2pass": ({}, 1, 580, 572, ("pad", "fnet.conv1", "fnet.norm1", "fnet.layer1.", "fnet.layer2.0."), [0], None, False, {"instnorm_2pass", "instnorm_reg20"}),
    "2pass_offset": ({}, 1, 580, 572, ("pad", "fnet.conv1", "fnet.norm1"), [0], None, True, {"instnorm_2pass"}),
    "f4_b4": ({}, 4, 200, 296, ("pad", "fnet.norm1", "fnet.layer1.", "cnet.conv1", "cnet.layer1."), [0, 3], [3], False, {"f4"}),
    "f4_b2": ({}, 2, 200, 296, ("pad", "fnet.norm1", "fnet.layer1.0", "cnet.conv1", "cnet.layer1."), [1], None, False, {"f4"}),
    "wnc_b3": ({}, 3, 200, 320, ("fnet.layer1.1.norm2", "fnet.layer2.", "fnet.layer3.", "cnet.layer1.1.conv2", "cnet.layer2.", "cnet.layer3."), [2], None, False, {"wnc"}),
    "no_f4_no_wnc": ({"EEM_ERAFT_NO_F4": "1", "EEM_ERAFT_NO_WNC": "1"}, 3, 200, 320,
                     ("pad", "fnet.conv1", "fnet.norm1", "fnet.layer1.0", "cnet."), [2], None, False, set()),
}
NORM_ROLES = set()


@pytest.mark.parametrize("case", list(ENC_CASES))
def test_encoder(monkeypatch, case):
    env, b, h, w, record, imgs, cimgs, offset, want = ENC_CASES[case]
    pin(monkeypatch, env)
    net, sd = make_net(51, h, w, record, 1)
    e1, e2 = inputs(52, b, h, w)
    if offset:
        sd = offset_stem_bias(net, sd, e1)
    forward(net, e1, e2, 1)
    st = Stages(net)
    assert want <= st.forms(), (sorted(want - st.forms()), sorted(st.forms()))
    pad = net.image_padder._pad
    x = B.er_pad_ref(torch.cat([e1, e2]), pad)
    if "pad" in st:
        soft(B.check_bitwise, f"enc {case} pad", st.get("pad"), x)
    big = case.startswith("2pass")
    fimgs = imgs + [b + i for i in imgs]                                   # both event volumes of each image
    fc = None if cimgs is None else cimgs + [b + i for i in cimgs]
    roles, feat_f = check_encoder(st, sd, "fnet.", x, fimgs, fc, convs=not big, name=f"enc {case}")
    NORM_ROLES.update(roles)
    _, feat_c = check_encoder(st, sd, "cnet.", x[:b], imgs, cimgs, name=f"enc {case}")
    check_heads(st, sd, feat_f, feat_c, fimgs, imgs, f"enc {case}")
    if case == "f4_b4":
        assert st.form("fnet.layer1.0.conv1") == "f4" and st.form("cnet.layer1.1.conv2") == "f4", st.names
    if case == "f4_b2":                                                      # cnet at batch 2 stays on gconv with the residual epilogue
        assert st.form("fnet.layer1.0.conv1") == "f4" and st.form("cnet.layer1.1.conv2").startswith("gconv"), st.names
    if case == "wnc_b3":
        assert st.form("fnet.layer3.1.conv2") == "wnc" and st.form("cnet.layer2.1.conv2") == "wnc" and st.form("cnet.layer3.0.conv2") == "wnc", st.names
    if case == "no_f4_no_wnc":
        assert not ({"f4", "wnc"} & st.forms()), st.forms()
    if case == "2pass":                                                      # 292 x 288 = 84096 values: three chunks, the last partial
        assert st.names["fnet.norm1"][1] == (2, 64, 292, 288)
        assert {r for f, r in roles if f == "instnorm_2pass"} == {"relu", "residual"}
        assert ("instnorm_reg20", "plain") in roles                          # (146 x 144 = 21024 values: the downsample norm of layer2)
    flush()
    RAN.add(f"enc {case}")


# --------------------------------------------------------------------------------------------------------------- pyramid cases
PYR_CASES = {
    "lds": ({}, 2, 128, 160, {"allpairs_lds", "pool2x3"}),                  # 16x20 = 320 cells: hw % 4 == 0, not a multiple of 128
    "l2": ({"EEM_ALLPAIRS_L2": "1"}, 2, 128, 160, {"allpairs_l2", "pool2x3"}),
    "l2_even": ({}, 2, 136, 176, {"allpairs_l2", "pool2x3"}),               # 17x22 = 374: even, not a multiple of 4; levels 17 -> 8 -> 4 -> 2
    "odd": ({}, 2, 136, 200, {"allpairs_odd", "pool2x3"}),                   # 17x25 = 425
    "odd_chain": ({"EEM_POOL_CHAIN": "1"}, 2, 136, 200, {"allpairs_odd", "pool2"}),
}


@pytest.mark.parametrize("case", list(PYR_CASES))
def test_pyramid(monkeypatch, case):
    env, b, h, w, want = PYR_CASES[case]
    pin(monkeypatch, env)
    net, _ = make_net(61, h, w, ("fmap", "pyr"), 1)
    forward(net, *inputs(62, b, h, w), iters=1)
    st = Stages(net)
    assert st.forms("pyr") == want, (st.forms("pyr"), want)
    check_pyramid(st, b, list(range(b)), f"pyr {case}", fmap=False)
    flush()
    RAN.add(f"pyr {case}")


@pytest.mark.parametrize("case", [c for c in PYR_CASES if c != "odd_chain"])
def test_allpairs(monkeypatch, case):
    """Level 0 from the GPU's own fmap: an fp32-MFMA sum of 256 products per value, held to the `direct` family.
    (Before the kernels added the channels in runs of 32 this measured rms(z) 2.83 - 2.85 against 0.98: the module docstring.)"""
    env, b, h, w, want = PYR_CASES[case]
    pin(monkeypatch, env)
    net, _ = make_net(61, h, w, ("fmap", "pyr0"), 1)
    forward(net, *inputs(62, b, h, w), iters=1)
    st = Stages(net)
    assert {st.form("pyr0")} == want - {"pool2x3"}, st.names
    fm = st.get("fmap")
    ref, mag = B.er_allpairs_ref(fm[:b], fm[b:])
    soft(B.er_check_form, f"allpairs {case}", st.form("pyr0"), st.get("pyr0"), ref, mag)
    RAN.add(f"allpairs {case}")
    flush()


# ---------------------------------------------------------------------------------------------------------------- lookup cases
LOOKUP_FWD = {
    "flat16": ({}, 2, 128, 160, "lookup_flat16"),
    "flat32": ({"EEM_LOOKUP_PX": "32"}, 2, 128, 160, "lookup_flat32"),
    "flat64": ({"EEM_LOOKUP_PX": "64"}, 2, 136, 200, "lookup_flat64"),
    "cond64": ({}, 4, 512, 512, "lookup_cond64"),                            # 64x64 cells at batch 4: ceil(hw / 64) * 4 * B = 1024, the threshold
    "cond32": ({"EEM_LOOKUP_PX": "32"}, 4, 512, 512, "lookup_cond32"),
    "cond16": ({"EEM_LOOKUP_PX": "16"}, 4, 512, 512, "lookup_cond16"),
    "under": ({}, 4, 504, 512, "lookup_flat16"),                             # 63x64 cells: 1008 blocks, just under it
}


@pytest.mark.parametrize("case", list(LOOKUP_FWD))
def test_lookup_in_a_forward(monkeypatch, case):
    env, b, h, w, want = LOOKUP_FWD[case]
    pin(monkeypatch, env)
    net, _ = make_net(71, h, w, ("pyr", "it0.co", "it0.flow", "it1.co", "it1.flow"), 2)
    forward(net, *inputs(72, b, h, w), iters=2)
    st = Stages(net)
    imgs = [0, b - 1]
    assert st.form("it0.corr") == want and st.form("it1.corr") == want and st.form("it0.flow") == want, st.names
    h8, w8 = st.names["pyr0"][1][2:]
    pyr = check_pyramid(st, b, imgs, f"lookup {case}", fmap=False)
    c0 = R.coords_grid(len(imgs), h8, w8)
    for it in (0, 1):
        check_lookup(st, it, pyr, imgs, c0, f"lookup {case}")
    flush()
    RAN.add(f"lookup {case}")


def hostile_coords(b, h, w, seed):
    """Sample centres that are exact integers, x.5, negative, just inside and outside each border, and far enough outside for the
    whole window to miss at every level."""
    g = torch.Generator().manual_seed(seed)
    base = R.coords_grid(b, h, w)
    c = base + torch.randn(b, 2, h, w, generator=g) * 3
    c[:, :, 0] = base[:, :, 0]
    c[:, :, 1] = base[:, :, 1] + 0.5
    c[:, :, 2] = -base[:, :, 2] - 0.25
    eps = 1e-3
    c[:, 0, 3, 0::4], c[:, 0, 3, 1::4], c[:, 0, 3, 2::4], c[:, 0, 3, 3::4] = -eps, eps, w - 1 - eps, w - 1 + eps
    c[:, 1, 4, 0::4], c[:, 1, 4, 1::4], c[:, 1, 4, 2::4], c[:, 1, 4, 3::4] = -eps, eps, h - 1 - eps, h - 1 + eps
    c[:, :, 5] = base[:, :, 5] + 8 * max(h, w) + 40.3
    c[:, :, 6] = -40.7
    c[:, :, -1, -3:] = base[:, :, -1, -3:] + 0.75                            # the last, partial block of pixels
    return c


LOOKUP_DIRECT = {
    # 17x22 = 374 cells: the last block holds 6 / 22 / 54 pixels;  31x33 = 1023 cells at batch 16: 16 * 4 * 16 = 1024 blocks, the last of 15 / 31 / 63
    "flat16": ({}, 2, 17, 22, "lookup_flat16"), "flat32": ({"EEM_LOOKUP_PX": "32"}, 2, 17, 22, "lookup_flat32"),
    "flat64": ({"EEM_LOOKUP_PX": "64"}, 2, 17, 22, "lookup_flat64"),
    "cond16": ({"EEM_LOOKUP_PX": "16"}, 16, 31, 33, "lookup_cond16"), "cond32": ({"EEM_LOOKUP_PX": "32"}, 16, 31, 33, "lookup_cond32"),
    "cond64": ({}, 16, 31, 33, "lookup_cond64"),
}


@pytest.mark.parametrize("case", list(LOOKUP_DIRECT))
def test_lookup_at_hostile_coordinates(monkeypatch, case):
    env, b, h, w, want = LOOKUP_DIRECT[case]
    pin(monkeypatch, env)
    net, _ = make_net(81, 128, 160, ("pyr", "corr"), 1)
    ctx = net._context(torch.device(DEV))
    g = torch.Generator().manual_seed(82)
    f1, f2 = torch.randn(b, 32, h, w, generator=g), torch.randn(b, 32, h, w, generator=g)
    coords = hostile_coords(b, h, w, 83)
    d1, d2, dc = f1.to(DEV), f2.to(DEV), coords.to(DEV)
    out = torch.empty(b, 324, h, w, device=DEV)
    _lib.check(_lib.lib().eraft_corr_lookup(ctx, d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), b, 32, h, w, out.data_ptr(),
                                            _lib.current_stream_ptr(torch.device(DEV))))
    st = Stages(net)
    assert st.form("corr") == want, st.names
    imgs = [0, b - 1]
    pyr = [rows(st.get(f"pyr{l}"), imgs, h * w) for l in range(4)]
    ref, mag = B.er_allpairs_ref(f1[imgs], f2[imgs])
    soft(B.er_check_form, f"direct {case} pyr0", st.form("pyr0"), pyr[0], ref, mag)
    ref, mag = B.er_lookup_ref(pyr, coords[imgs])
    assert torch.equal(st.get("corr"), out.cpu())
    soft(B.check_roundings, f"direct {case} corr", out.cpu()[imgs], ref, mag, "lookup", form=want)
    flush()
    RAN.add(f"direct {case}")


@pytest.mark.parametrize("b,h,w", [(1, 128, 160), (2, 136, 200)])
def test_alternate_corr(monkeypatch, b, h, w):
    """The on-the-fly correlation against its definition on the GPU's own fmap: a small and a ragged (17x25) size."""
    pin(monkeypatch, {})
    net, _ = make_net(91, h, w, ("fmap", "f2l", "it0.co", "it0.flow", "it1.co", "it1.flow"), 2, alternate_corr=True)
    forward(net, *inputs(92, b, h, w), iters=2)
    st = Stages(net)
    assert st.form("it0.corr") == "altcorr" and st.forms("f2l") == {"pool2"} and "pyr0" not in st, st.names
    imgs = list(range(b))
    fm = st.get("fmap")
    levels = [fm[b:]] + [st.get(f"f2l{l}") for l in (1, 2, 3)]
    for l in (1, 2, 3):
        ref, mag = B.avg_pool_ref(levels[l - 1], 2)
        soft(B.er_check_form, f"alt f2l{l}", "pool2", levels[l], ref, mag)
        soft(B.check_roundings, f"alt f2l{l}", levels[l], ref, mag, "pool", form="pool2 roundings")
    h8, w8 = fm.shape[-2:]
    c0 = R.coords_grid(b, h8, w8)
    for it in (0, 1):
        check_lookup(st, it, None, imgs, c0, f"alt {h}x{w}", alt=(fm[:b], levels))
    flush()
    RAN.add(f"alt {h}")


# ---------------------------------------------------------------------------------------------------------- padding, recorder
def last_form():
    buf = ctypes.create_string_buffer(64)
    _lib.check(_lib.lib().eraft_last_form(buf, 64))
    return buf.value.decode()


@pytest.mark.parametrize("w,pad,want", [(157, (2, 1, 3, 4), "pad4"), (158, (1, 2, 0, 5), "pad"), (160, (0, 0, 4, 4), "pad4"), (19, (3, 3, 2, 1), "pad")])
def test_padding_is_bitwise(w, pad, want):
    """pad_kernel and pad4_kernel (padded widths that are and are not multiples of 4) against F.pad(mode='replicate'); the two-input
    form is every forward's first launch (test_encoder)."""
    x = torch.randn(3, 5, 37, w, generator=torch.Generator().manual_seed(w))
    got = ops.replicate_pad(x.to(DEV), pad)
    form = last_form()
    assert form == want, form
    SEEN.add(form)
    ERRS.clear()
    soft(B.check_bitwise, f"pad {w}", got.cpu(), B.er_pad_ref(x, pad))
    flush()
    RAN.add(f"pad {w}")


@pytest.mark.parametrize("env", [{}, {"EEM_ERAFT_NO_LAG": "1", "EEM_ERAFT_NO_STACK": "1"}], ids=["default", "no_lag_no_stack"])
def test_recorder_leaves_the_predictions_bitwise(monkeypatch, env):
    pin(monkeypatch, env)
    e1, e2 = inputs(102, 2, 194, 290)
    off, _ = make_net(101, 194, 290, None)
    ref = forward(off, e1, e2, 3)
    assert off.stage_names() == []
    on, _ = make_net(101, 194, 290, ("",), 3)                               # every name, every iteration
    got = forward(on, e1, e2, 3)
    names = [n for n, _, _ in on.stage_names()]
    assert len(names) == len(set(names)) and "it2.pred" in names and "fnet.layer3.1.norm2" in names and "cnet.layer2.0.down" in names, names
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    again = forward(on, e1, e2, 3)                                          # (the arena is sized now: one pass)
    assert all(torch.equal(a, b) for a, b in zip(again, ref))
    on.record_stages = None
    assert all(torch.equal(a, b) for a, b in zip(forward(on, e1, e2, 3), ref)) and on.stage_names() == []


def test_every_form_in_the_table_ran():
    """The form names seen over the module: none the family table lacks, and - when the whole module ran - every E-RAFT helper form,
    both Winograd kernels, both stems, every fused epilogue and every instance-norm role of every form that can see it."""
    table = set(B.FORM_FAMILY) | set(B.ER_FORM_FAMILY) | ER_FORMS | {"flow", "axpy", "sum", "mul_channels", "coords_init"}
    assert SEEN <= table, sorted(SEEN - table)
    every = {f"upd {c}" for c in UPD_CONFIGS} | {"sum2 fallback", "upd 60x80", "upd wnc7"} | {f"enc {c}" for c in ENC_CASES} | {f"pyr {c}" for c in PYR_CASES} | {f"allpairs {c}" for c in PYR_CASES if c != "odd_chain"} | \
            {f"lookup {c}" for c in LOOKUP_FWD} | {f"direct {c}" for c in LOOKUP_DIRECT} | {"alt 128", "alt 136"} | {f"pad {w}" for w in (157, 158, 160, 19)}
    if RAN != every:                                                         # (only a part of the module ran)
        return
    assert ER_FORMS <= SEEN, sorted(ER_FORMS - SEEN)
    assert EPILOGUES <= SEEN_EPI, sorted(EPILOGUES - SEEN_EPI)
    want = {(f, r) for f in ("instnorm_reg5", "instnorm_reg20", "instnorm_2pass") for r in ("relu", "residual")}
    want |= {("instnorm_reg5", "plain"), ("instnorm_reg20", "plain"), ("instnorm_plain", "relu"), ("instnorm_plain", "residual"), ("instnorm_plain", "plain")}
    assert want <= NORM_ROLES, sorted(want - NORM_ROLES)
