"""The proof that tests/test_gpu_eraft_stage_fp64.py would fail on a subtly wrong kernel - on the CPU, with torch alone.

Every reference and criterion that module applies to a recorded launch of eraft_forward (oracle/fp64_bounds.py: er_*_ref, `check` under
the form's family, `check_roundings`, `check_decoder`) is applied here to

  pass   an fp32 evaluation of the same launch, written the kernel's way where that differs from torch's (one-pass chunked statistics,
         1 / (1 + exp(-v)), the four-term blend, softmax as exp / sum), which must sit inside with room to spare;
  fail   that evaluation with one fault planted at a time: an instance norm that takes a neighbouring plane's mean in one chunk; a
         variance without its - m * m term; the residual added in front of the inner ReLU; an all-pairs tile without its last 16
         channels; a level-3 pooled value from the wrong 2 x 2 cell; a lookup with dx and dy swapped, with the level scale off by one
         level, with an outside corner clamped instead of zeroed; GEPI_GRU with z and 1 - z exchanged; GEPI_ZR multiplying the wrong
         half; `pre` dropped in one 16-column tile; the mask's 0.25 missing; convex upsampling with the 3 x 3 neighbourhood transposed
         and with the crop one pixel off; a replicate pad that repeats the second column.

Shapes are a few tiles each.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import eraft_oracle as R
from oracle import fp64_bounds as B

ROOM = 1.5          # a correct evaluation: every statistic x ROOM inside its limit
FACTOR = 1.5        # a planted fault: some statistic beyond FACTOR x its limit


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _family_ratios(rec, lim):
    r = [rec["max_z"] / lim.max_z, rec["rms_z"] / lim.rms_z, abs(rec["mean_z"]) / lim.mean_z]
    if rec["n"] >= lim.slope_min_n:
        r.append(abs(rec["slope_u"]) / lim.slope_u)
    return max(r)


def family_passes(name, form, got, ref, mag):
    lim = B.LIMITS[B.er_form_family(form)]
    rec = B.er_check_form(name, form, got, ref, mag)
    print(name, {k: round(rec[k], 4) for k in ("max_z", "rms_z", "mean_z", "slope_u")}, lim)
    assert _family_ratios(rec, lim) * ROOM <= 1.0, (name, rec, lim)


def family_rejects(name, form, got, ref, mag):
    lim = B.LIMITS[B.er_form_family(form)]
    with pytest.raises(B.StageError):
        B.er_check_form(name, form, got, ref, mag)
    assert _family_ratios(B.LOG[-1], lim) >= FACTOR, (name, B.LOG[-1], lim)


def roundings_pass(name, got, ref, mag, kind):
    rec = B.check_roundings(name, got, ref, mag, kind)
    print(name, "max|z|", round(rec["max_z"], 4), "of", B.ER_ROUNDINGS[kind])
    return rec


def roundings_reject(name, got, ref, mag, kind):
    with pytest.raises(B.StageError):
        B.check_roundings(name, got, ref, mag, kind)
    assert B.LOG[-1]["max_z"] >= FACTOR * B.ER_ROUNDINGS[kind], (name, B.LOG[-1])


def kappa_passes(name, got, ref64, ref32):
    rec = B.check_decoder(name, got, ref64, ref32)
    print(name, "rms ratio", round(rec["rms_ratio"], 3), "max ratio", round(rec["max_ratio"], 3))
    floor = B.U * float(ref64.abs().max())
    assert rec["rms_gpu"] * ROOM <= B.KAPPA_DEC * rec["rms_cpu"] + floor and rec["max_gpu"] * ROOM <= B.KAPPA_DEC * rec["max_cpu"] + floor, rec


def kappa_rejects(name, got, ref64, ref32):
    with pytest.raises(B.StageError):
        B.check_decoder(name, got, ref64, ref32)
    rec = B.LOG[-1]
    floor = B.U * float(ref64.abs().max())
    assert rec["rms_gpu"] >= FACTOR * (B.KAPPA_DEC * rec["rms_cpu"] + floor) or rec["max_gpu"] >= FACTOR * (B.KAPPA_DEC * rec["max_cpu"] + floor), rec


# ------------------------------------------------------------------------------------------------------------------ instance norm
CHUNK = 4 * 8192                        # instnorm_stats_kernel: 8192 float4 per block


def instnorm_emulated(x, relu_inner, res=None, fault=None):
    """The two-pass kernel's arithmetic: per chunk fp32 sums of 32-value runs added in double, mean and Q / hw - m * m in double, the
    apply step in fp32."""
    n, c, h, w = x.shape
    hw = h * w
    p = x.reshape(n * c, hw).float()
    pad = (-hw) % 32
    runs = F.pad(p, (0, pad)).reshape(n * c, -1, 32)
    s = runs.sum(2).double().sum(1)
    q = (runs * runs).sum(2).double().sum(1)
    m = s / hw
    var = q / hw if fault == "no_mm" else q / hw - m * m
    mean = m.float()[:, None].expand(-1, hw).clone()
    if fault == "neighbour_mean":
        mean[3, CHUNK:2 * CHUNK] = m.float()[4]
    rstd = 1.0 / torch.sqrt(var.clamp_min(0).float() + 1e-5)
    v = ((p - mean) * rstd[:, None]).reshape(n, c, h, w)
    if fault == "res_first":
        return torch.relu(torch.relu(v + res.float())) if relu_inner else torch.relu(v + res.float())
    if relu_inner:
        v = torch.relu(v)
    if res is not None:
        v = torch.relu(v + res.float())
    return v


@pytest.fixture(scope="module")
def norm_case():
    g = gen(1)
    x = torch.randn(1, 6, 292, 288, generator=g) * torch.tensor([1.0, 0.3, 2.0, 1.0, 0.7, 1.5]).view(1, 6, 1, 1) + \
        torch.tensor([0.1, -0.4, 10.0, 0.3, -0.2, 0.05]).view(1, 6, 1, 1)       # (84096 values: three chunks, the last partial; one plane 5 sd off)
    res = torch.relu(torch.randn(1, 6, 292, 288, generator=g))
    return x, res


@pytest.mark.parametrize("role", ["relu", "plain", "residual"])
def test_instance_norm_passes(norm_case, role):
    x, res = norm_case
    relu, r = role != "plain", res if role == "residual" else None
    kappa_passes(f"instnorm {role}", instnorm_emulated(x, relu, r), B.er_instnorm_ref(x, relu, r), B.er_instnorm_ref(x, relu, r, torch.float32))


@pytest.mark.parametrize("fault", ["neighbour_mean", "no_mm", "res_first"])
def test_instance_norm_faults(norm_case, fault):
    x, res = norm_case
    kappa_rejects(f"instnorm {fault}", instnorm_emulated(x, True, res, fault), B.er_instnorm_ref(x, True, res),
                  B.er_instnorm_ref(x, True, res, torch.float32))


# ------------------------------------------------------------------------------------------------------ all-pairs and the pyramid
@pytest.fixture(scope="module")
def corr_case():
    g = gen(2)
    f1, f2 = torch.randn(2, 64, 17, 22, generator=g), torch.randn(2, 64, 17, 22, generator=g)      # hw = 374: three 128-pixel tiles a side
    pyr = R.corr_pyramid(f1, f2)
    return f1, f2, pyr


def test_allpairs(corr_case):
    f1, f2, pyr = corr_case
    ref, mag = B.er_allpairs_ref(f1, f2)
    family_passes("allpairs", "allpairs_lds", pyr[0], ref, mag)
    b, c, h, w = f1.shape
    part = torch.matmul(f1[:, :c - 16].reshape(b, c - 16, h * w).transpose(1, 2), f2[:, :c - 16].reshape(b, c - 16, h * w)) / 8.0
    bad = pyr[0].clone().view(b, h * w, h * w)
    bad[1, 256:, 128:256] = part[1, 256:, 128:256]                          # the ragged last row of tiles, one tile
    family_rejects("allpairs: a tile without its last 16 channels", "allpairs_lds", bad.view_as(pyr[0]), ref, mag)


def test_pooling(corr_case):
    _, _, pyr = corr_case
    for l in (1, 2, 3):
        ref, mag = B.avg_pool_ref(pyr[l - 1], 2)
        family_passes(f"pyr{l}", "pool2x3", pyr[l], ref, mag)
        roundings_pass(f"pyr{l}", pyr[l], ref, mag, "pool")
    bad = pyr[3].clone()
    bad[700, 0, 1, 0] = pyr[2][700, 0, 2:4, 2:4].mean()                     # the cell to the right
    ref, mag = B.avg_pool_ref(pyr[2], 2)
    roundings_reject("pyr3: a value from the wrong 2x2 cell", bad, ref, mag, "pool")
    family_rejects("pyr3: a value from the wrong 2x2 cell", "pool2x3", bad, ref, mag)


def hostile_coords(b, h, w, seed):
    """Sample centres that are exact integers, x.5, negative, just inside and outside each border and more than four cells outside."""
    g = gen(seed)
    base = R.coords_grid(b, h, w)
    c = base + torch.randn(b, 2, h, w, generator=g) * 3
    c[:, :, 0] = base[:, :, 0]                                               # exact integers
    c[:, :, 1] = base[:, :, 1] + 0.5                                         # x.5
    c[:, :, 2] = -base[:, :, 2] - 0.25                                       # negative
    eps = 1e-3
    c[:, 0, 3, 0::4], c[:, 0, 3, 1::4], c[:, 0, 3, 2::4], c[:, 0, 3, 3::4] = -eps, eps, w - 1 - eps, w - 1 + eps
    c[:, 1, 4, 0::4], c[:, 1, 4, 1::4], c[:, 1, 4, 2::4], c[:, 1, 4, 3::4] = -eps, eps, h - 1 - eps, h - 1 + eps
    c[:, :, 5] = base[:, :, 5] + 8 * max(h, w) + 40.3                        # the whole window misses at every level
    c[:, :, 6] = -40.7
    return c


def lookup_f32(pyr, coords, swap=False, level_shift=0, clamp=False):
    """The kernel's arithmetic in fp32: er_lookup_geometry's positions, the four-term blend as sample_bilinear writes it."""
    b, _, hh, ww = coords.shape
    outs = []
    for l in range(4):
        img = pyr[l][:, 0].float()
        n, h, w = img.shape
        co = coords
        if level_shift:
            co = coords * 2.0 ** (-level_shift)
        x0, y0, tx, ty = B.er_lookup_geometry(co, l, (h, w))
        if swap:
            x0, y0, tx, ty = (t.transpose(1, 2) for t in (x0, y0, tx, ty))    # channel i * 9 + j samples x + (j - 4), y + (i - 4)
        idx = torch.arange(n).view(n, 1, 1)

        def at(yy, xx):
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            v = img[idx, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]
            return v if clamp else torch.where(ok, v, torch.zeros(()))
        v = at(y0, x0) * (1 - tx) * (1 - ty) + at(y0, x0 + 1) * tx * (1 - ty) + at(y0 + 1, x0) * (1 - tx) * ty + at(y0 + 1, x0 + 1) * tx * ty
        outs.append(v.reshape(b, hh, ww, 81).permute(0, 3, 1, 2))
    return torch.cat(outs, 1)


def test_lookup(corr_case):
    _, _, pyr = corr_case
    for name, coords in (("benign", R.coords_grid(2, 17, 22) + torch.randn(2, 2, 17, 22, generator=gen(3))), ("hostile", hostile_coords(2, 17, 22, 4))):
        ref, mag = B.er_lookup_ref(pyr, coords)
        roundings_pass(f"lookup {name}: grid_sample", R.corr_lookup(pyr, coords), ref, mag, "lookup")
        roundings_pass(f"lookup {name}: the kernel's blend", lookup_f32(pyr, coords), ref, mag, "lookup")
    coords = hostile_coords(2, 17, 22, 4)
    ref, mag = B.er_lookup_ref(pyr, coords)
    roundings_reject("lookup: dx and dy swapped", lookup_f32(pyr, coords, swap=True), ref, mag, "lookup")
    roundings_reject("lookup: level scale off by one level", lookup_f32(pyr, coords, level_shift=1), ref, mag, "lookup")
    roundings_reject("lookup: an outside corner clamped", lookup_f32(pyr, coords, clamp=True), ref, mag, "lookup")


def test_altcorr(corr_case):
    f1, f2, pyr = corr_case
    coords = hostile_coords(2, 17, 22, 5)
    levels = [f2]
    for _ in range(3):
        levels.append(F.avg_pool2d(levels[-1], 2))
    ref, mag = B.er_altcorr_ref(f1, levels, coords)
    vols = [torch.matmul(f1.reshape(2, 64, -1).transpose(1, 2), q.reshape(2, 64, -1)).reshape(2 * 374, 1, *q.shape[-2:]) / 8.0 for q in levels]
    family_passes("altcorr", "altcorr", lookup_f32(vols, coords), ref, mag)
    family_rejects("altcorr: an outside corner clamped", "altcorr", lookup_f32(vols, coords, clamp=True), ref, mag)


# ------------------------------------------------------------------------------------------------------------- the update block
def sigmoid_k(v):
    return 1.0 / (1.0 + torch.exp(-v))                                      # (as the epilogue writes it)


@pytest.fixture(scope="module")
def gru_case():
    g = gen(6)
    n, hh, ww = 2, 15, 40                                                    # 40 columns: two and a half 16-column tiles
    h = torch.tanh(torch.randn(n, 128, hh, ww, generator=g))
    motion = torch.relu(torch.randn(n, 128, hh, ww, generator=g))
    inp = torch.relu(torch.randn(n, 128, hh, ww, generator=g))
    wzr, bzr = B.seeded_conv(7, 384, 256, (1, 5))
    wq, bq = B.seeded_conv(8, 384, 128, (1, 5))
    return h, motion, inp, wzr, bzr, wq, bq


def split_ctx(w):
    """The GRU conv over [h | inp | motion] as the `hm` conv over [h | motion] and the `ctx` conv over inp."""
    return torch.cat([w[:, :128], w[:, 256:]], 1), w[:, 128:256]


def test_gru_zr_and_pre(gru_case):
    h, motion, inp, wzr, bzr, _, _ = gru_case
    whm, wc = split_ctx(wzr)
    pre = F.conv2d(inp, wc, bzr, padding=(0, 2))
    ref, mag = B.op_conv_ref([inp], wc, bzr, padding=(0, 2))
    family_passes("czr", "gconv16_1x5_th2_wm4_kg2", pre, ref, mag)
    v64, _ = B.er_conv_ref([h, motion], whm, None, padding=(0, 2), pre=pre)
    v32 = B.er_conv_f32([h, motion], whm, None, padding=(0, 2), pre=pre)
    z64, rh64 = torch.sigmoid(v64[:, :128]), torch.sigmoid(v64[:, 128:]) * h.double()
    z32, rh32 = torch.sigmoid(v32[:, :128]), torch.sigmoid(v32[:, 128:]) * h
    vk = F.conv2d(torch.cat([h, motion], 1), whm, None, padding=(0, 2)) + pre
    kappa_passes("gru.z", sigmoid_k(vk[:, :128]), z64, z32)
    kappa_passes("gru.rh", sigmoid_k(vk[:, 128:]) * h, rh64, rh32)
    kappa_rejects("GEPI_ZR multiplying the wrong half: z", sigmoid_k(vk[:, :128]) * h, z64, z32)
    kappa_rejects("GEPI_ZR multiplying the wrong half: rh", sigmoid_k(vk[:, 128:]), rh64, rh32)
    dropped = vk.clone()
    dropped[1, :, 14:, 32:] -= pre[1, :, 14:, 32:]                           # the ragged last tile of the last row
    kappa_rejects("pre dropped in one 16-column tile", sigmoid_k(dropped[:, :128]), z64, z32)


def test_gru_blend(gru_case):
    h, motion, inp, wzr, bzr, wq, bq = gru_case
    z = torch.sigmoid(torch.randn(h.shape, generator=gen(9)))
    rh = torch.sigmoid(torch.randn(h.shape, generator=gen(10))) * h
    v64, _ = B.er_conv_ref([rh, inp, motion], wq, bq, padding=(0, 2))
    v32 = B.er_conv_f32([rh, inp, motion], wq, bq, padding=(0, 2))
    ref64 = B.er_gru_blend_ref(z.double(), h.double(), torch.tanh(v64))
    ref32 = B.er_gru_blend_ref(z, h, torch.tanh(v32))
    q = torch.tanh(F.conv2d(torch.cat([rh, inp, motion], 1), wq, bq, padding=(0, 2)))
    kappa_passes("gru.h", h + z * (q - h), ref64, ref32)                     # (another fp32 order of the same blend)
    kappa_rejects("GEPI_GRU with z and 1 - z exchanged", z * h + (1 - z) * q, ref64, ref32)
    r = torch.sigmoid(torch.randn(h.shape, generator=gen(10)))
    ref = r.double() * h.double()
    roundings_pass("r * h", r * h, ref, ref.abs(), "mul")
    roundings_reject("r * h: z for r", z * h, ref, ref.abs(), "mul")


def test_mask_scale():
    g = gen(11)
    x = torch.relu(torch.randn(1, 256, 15, 40, generator=g))
    w, b = B.seeded_conv(12, 256, 576, (1, 1))
    ref, mag = B.er_conv_ref([x], w, b, padding=(0, 0), out_scale=0.25)
    family_passes("mask", "gconv16_1x1_th2_wm4_kg2", 0.25 * F.conv2d(x, w, b), ref, mag)
    family_rejects("mask: the 0.25 missing", "gconv16_1x1_th2_wm4_kg2", F.conv2d(x, w, b), ref, mag)


def test_cnet_conv_with_batch_norm_and_residual():
    g = gen(13)
    x, res = torch.relu(torch.randn(2, 64, 20, 40, generator=g)), torch.relu(torch.randn(2, 64, 20, 40, generator=g))
    w, b = B.seeded_conv(14, 64, 64, (3, 3))
    sd = {"n.weight": torch.rand(64, generator=g) * 0.4 + 0.8, "n.bias": torch.randn(64, generator=g) * 0.05,
          "n.running_mean": torch.randn(64, generator=g) * 0.2, "n.running_var": torch.rand(64, generator=g) + 0.5}
    bn = B.er_bn_fold(sd, "n.")
    ref, mag = B.er_conv_ref([x], w, b, bn=bn, relu=True, res=res)
    y = F.batch_norm(F.conv2d(x, w, b, padding=1), sd["n.running_mean"], sd["n.running_var"], sd["n.weight"], sd["n.bias"], False, 0.1, 1e-5)
    got = torch.relu(res + torch.relu(y))
    for form in ("f4", "gconv16_3x3_th2_wm4_kg2"):
        family_passes(f"cnet conv2 [{form}]", form, got, ref, mag)
        family_rejects(f"cnet conv2 [{form}]: the residual in front of the inner ReLU", form, torch.relu(res + y), ref, mag)


# ------------------------------------------------------------------------------------------------- convex upsampling and padding
def convex_up_f32(flow, mask, pad, size, transpose=False, shift=0):
    """convex_up_kernel's arithmetic: softmax as exp(l - max) / sum, the nine neighbours of 8 * flow, zero outside."""
    n, _, h, w = flow.shape
    m = mask.view(n, 9, 8, 8, h, w)
    e = torch.exp(m - m.max(1, keepdim=True).values)
    wgt = e / e.sum(1, keepdim=True)
    fp = F.pad(8 * flow, (1, 1, 1, 1))
    up = torch.zeros(n, 2, 8, 8, h, w)
    for k in range(9):
        dy, dx = (k % 3, k // 3) if transpose else (k // 3, k % 3)
        up += wgt[:, k:k + 1] * fp[:, :, dy:dy + h, dx:dx + w].view(n, 2, 1, 1, h, w)
    up = up.permute(0, 1, 4, 2, 5, 3).reshape(n, 2, 8 * h, 8 * w)
    return up[..., pad[2] + shift:pad[2] + shift + size[0], pad[0]:pad[0] + size[1]]


def test_convex_upsampling():
    g = gen(15)
    flow = torch.randn(2, 2, 17, 22, generator=g) * 3
    mask = torch.randn(2, 576, 17, 22, generator=g)
    pad, size = (3, 3, 3, 3), (130, 170)
    ref64 = B.er_convex_up_ref(flow, mask, pad, size)
    ref32 = B.er_convex_up_ref(flow, mask, pad, size, torch.float32)
    kappa_passes("convex_up", convex_up_f32(flow, mask, pad, size), ref64, ref32)
    kappa_rejects("convex_up: the 3x3 neighbourhood transposed", convex_up_f32(flow, mask, pad, size, transpose=True), ref64, ref32)
    kappa_rejects("convex_up: the crop one pixel off", convex_up_f32(flow, mask, pad, size, shift=1), ref64, ref32)


def test_elementwise_roundings():
    g = gen(16)
    c0 = R.coords_grid(2, 17, 22)
    c1 = c0 + torch.randn(2, 2, 17, 22, generator=g) * 5
    d = torch.randn(2, 2, 17, 22, generator=g) * 0.1
    roundings_pass("flow", c1 - c0, c1.double() - c0.double(), c1.double().abs() + c0.double().abs(), "flow")
    roundings_pass("coords1 + delta", c1 + d, c1.double() + d.double(), c1.double().abs() + d.double().abs(), "sum")
    roundings_reject("flow: coords0 - coords1", c0 - c1, c1.double() - c0.double(), c1.double().abs() + c0.double().abs(), "flow")


def test_replicate_pad_is_bitwise():
    from oracle import eemflow_oracle as O
    x = torch.randn(2, 5, 13, 19, generator=gen(17))
    pad = (3, 2, 1, 2)
    ref = B.er_pad_ref(x, pad)
    B.check_bitwise("pad", O.replicate_pad(x, pad), ref)
    bad = ref.clone()
    bad[..., :3] = ref[..., 4:5]                                            # the second column repeated
    with pytest.raises(B.StageError):
        B.check_bitwise("pad: the second column repeated", bad, ref)
