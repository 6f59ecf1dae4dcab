"""Self-tests of the fp64 stage checker (oracle/fp64_bounds.py), on the CPU: correct fp32 arithmetic passes at the limits of the
forms it stands for, and each planted fault - the kinds of bug a tiled HIP kernel has - is rejected at the limits of the form it
imitates.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fp64_bounds as B

KAIMING = np.sqrt(2.0)


def operands(seed, n, cin, cout, h, w, sparse=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    if sparse:                                          # voxel-grid statistics: ~20 % non-zero
        x = x * (torch.rand(n, cin, h, w, generator=g) < 0.2)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (KAIMING / np.sqrt(cin * 9))
    b = torch.randn(cout, generator=g) * 0.05
    return x.float(), wt.float(), b.float()


def leaky32(v):
    return torch.where(v >= 0, v, v * torch.tensor(0.1, dtype=torch.float32))


def im2col_conv32(x, w, b, stride=1, pad=(1, 1, 1, 1), mode="constant"):
    """fp32 3x3 convolution as an im2col matrix product (fp32 accumulation), + bias, LeakyReLU(0.1)."""
    xp = F.pad(x, pad, mode=mode) if mode != "constant" else F.pad(x, pad)
    n, cin, hp, wp = xp.shape
    ho, wo = (hp - 3) // stride + 1, (wp - 3) // stride + 1
    cols = F.unfold(xp, 3, stride=stride)                               # [n, cin * 9, ho * wo]
    out = torch.matmul(w.reshape(w.shape[0], -1), cols) + b[:, None]
    return leaky32(out.view(n, w.shape[0], ho, wo))


def split3(a):
    """a = hi + mid + lo EXACTLY, each a bf16 value: truncation a - (a & 0xffff0000), as conv_bx3.hip cuts its operands."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = (a - hi).astype(np.float32)
    mid = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    lo = (r - mid).astype(np.float32)
    return hi, mid, lo


SIX = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]


def bx3_conv32(x, w, b, stride=1, drop=None):
    """conv_bx3.hip's arithmetic in numpy: every operand as three bf16 pieces, the six products of SIX (fp32-exact), summed in fp32;
    `drop` removes one of them."""
    n = x.shape[0]
    cols = F.unfold(F.pad(x, (1, 1, 1, 1)), 3, stride=stride).numpy()           # [n, K, L]
    wa = split3(w.reshape(w.shape[0], -1).numpy())
    out = np.zeros((n, w.shape[0], cols.shape[2]), np.float32)
    for i in range(n):
        cb = split3(cols[i])
        for p, q in SIX:
            if (p, q) != drop:
                out[i] += np.matmul(wa[p], cb[q]).astype(np.float32)
    out += b.numpy()[None, :, None]
    ho = (x.shape[2] + 2 - 3) // stride + 1
    return leaky32(torch.from_numpy(out).view(n, w.shape[0], ho, -1))


CASES = [(45, 5, 16, 2), (144, 16, 32, 2), (288, 32, 32, 1), (576, 64, 64, 1)]       # K = cin * 9, cin, cout, stride


@pytest.mark.parametrize("form", ["direct", "bx3"])
@pytest.mark.parametrize("K,cin,cout,stride", CASES)
def test_fp32_im2col_convolution_passes(K, cin, cout, stride, form):
    x, w, b = operands(K, 2, cin, cout, 40, 72, sparse=cin == 5)
    got = im2col_conv32(x, w, b, stride)
    ref, mag = B.conv_ref(x, w, b, stride)
    rec = B.check(f"im2col K={K}", got, ref, mag, form)
    assert rec["max_z"] > 0                                  # (fp32 arithmetic: not bitwise the fp64 values)


@pytest.mark.parametrize("K,cin,cout", [(144, 16, 32), (576, 64, 64)])
def test_three_piece_products_pass_and_one_dropped_cross_product_fails(K, cin, cout):
    x, w, b = operands(K + 1, 2, cin, cout, 24, 40)
    ref, mag = B.conv_ref(x, w, b)
    B.check(f"bx3 six products K={K}", bx3_conv32(x, w, b), ref, mag, "bx3")
    with pytest.raises(B.StageError):
        B.check(f"bx3 without hi*lo K={K}", bx3_conv32(x, w, b, drop=(0, 2)), ref, mag, "bx3")


def test_one_pixel_moved_by_2e16_relative_fails():
    x, w, b = operands(7, 2, 16, 32, 40, 72)
    ref, mag = B.conv_ref(x, w, b)
    got = im2col_conv32(x, w, b)
    B.check("clean", got, ref, mag, "direct")
    i = int((ref.abs() / mag).reshape(-1).argmax())          # the output whose sum is least cancelled
    bad = got.clone().reshape(-1)
    bad[i] = bad[i] * (1.0 + 2.0 ** -16)
    with pytest.raises(B.StageError):
        B.check("moved pixel", bad.view_as(got), ref, mag, "direct")


def test_tile_of_another_image_fails_and_is_named():
    x, w, b = operands(8, 2, 32, 32, 40, 80)
    ref, mag = B.conv_ref(x, w, b)
    got = im2col_conv32(x, w, b).clone()
    got[0, :, 16:20, 64:68] = got[1, :, 16:20, 64:68]        # a walk / indexing bug: image 1's 4 x 4 outputs in image 0
    with pytest.raises(B.StageError, match=r"image 0, .*y 1[6-9], x 6[4-7]\), tile \(row 1, col 1\) of 16x64"):
        B.check("swapped tile", got, ref, mag, "wino4", tile=(16, 64))


@pytest.mark.parametrize("edge,fill", [("col", "zero"), ("col", "stale"), ("row", "zero"), ("row", "stale")])
def test_last_partial_tile_left_unwritten_fails(edge, fill):
    """F(4x4) at C = 32: 16 x 64 tiles on a 40 x 80 map - the last tile row (y 32..39) and column (x 64..79) are partial."""
    x, w, b = operands(9, 2, 32, 32, 40, 80)
    ref, mag = B.conv_ref(x, w, b)
    got = im2col_conv32(x, w, b).clone()
    stale = im2col_conv32(operands(10, 2, 32, 32, 40, 80)[0], w, b)           # the previous frame's outputs
    sl = (slice(None), slice(None), slice(32, 40), slice(None)) if edge == "row" else (slice(None), slice(None), slice(None), slice(64, 80))
    got[sl] = 0.0 if fill == "zero" else stale[sl]
    with pytest.raises(B.StageError):
        B.check(f"partial {edge} {fill}", got, ref, mag, "wino4", tile=(16, 64))


@pytest.mark.parametrize("side", [0, 1, 2, 3])
def test_replicate_instead_of_zero_padding_on_one_border_fails(side):
    x, w, b = operands(11, 2, 5, 16, 41, 73, sparse=True)         # (odd: the stride-2 windows reach the right and bottom padding)
    ref, mag = B.conv_ref(x, w, b, 2)
    pad = [0, 0, 0, 0]
    pad[side] = 1
    rest = [1 - p for p in pad]
    got = im2col_conv32(F.pad(x, pad, mode="replicate"), w, b, 2, pad=tuple(rest))
    with pytest.raises(B.StageError):
        B.check("replicate border", got, ref, mag, "enc1")
    with pytest.raises(B.StageError):
        B.check("replicate border", got, ref, mag, "direct")


@pytest.mark.parametrize("k", [32, 16, 8])
def test_pooling_by_k2_minus_1_fails(k):
    g = torch.Generator().manual_seed(k)
    f = leaky32(torch.randn(2, 16, 3 * k, 5 * k, generator=g))
    ref, mag = B.avg_pool_ref(f, k)
    B.check("pool", ref.float(), ref, mag, "pool")                     # (correctly rounded fp32 means pass)
    bad = F.avg_pool2d(f, k, k, divisor_override=k * k - 1)
    with pytest.raises(B.StageError):
        B.check("pool / (k^2 - 1)", bad, ref, mag, "pool")


def test_stage_references_match_the_oracle():
    """The fp64 references are the oracle's operations: rounded to fp32 they agree with the oracle's fp32 results."""
    from oracle import eemflow_oracle as O
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 16, 6, 7, generator=g), torch.randn(2, 16, 6, 7, generator=g)
    ref, mag = B.corr53_ref(x, y)
    assert float((ref.float() - O.local_corr53(x, y)).abs().max()) < 1e-5 and bool((mag >= ref.abs()).all())
    c = torch.randn(1, 2, 5, 6, generator=g)
    ref, mag = B.upsample_ref(c, (260, 346))
    assert float((ref.float() - O.upsample_flow(c, (260, 346))).abs().max()) < 1e-5 and bool((mag >= ref.abs() - 1e-12).all())
    ev = torch.randn(1, 5, 19, 23, generator=g)
    pad = O.input_padder_pad(19, 23)
    xw, xb = torch.randn(16, 5, 3, 3, generator=g), torch.randn(16, generator=g)
    ref, _ = B.first_layer_ref(ev, pad, xw, xb)
    assert float((ref.float() - O.convrelu(O.replicate_pad(ev, pad), xw, xb, 2)).abs().max()) < 1e-5
    rec = torch.tensor([0.25, 2.0, 1.0, 1.0])
    ref_n, _ = B.first_layer_ref(ev, pad, xw, xb, records=[rec])
    v = torch.where(ev != 0, (ev - 0.25) / 2.0, ev)
    assert float((ref_n.float() - O.convrelu(O.replicate_pad(v, pad), xw, xb, 2)).abs().max()) < 1e-5


def test_decoder_criterion():
    from eemflow_amd.weights import seeded_state_dict
    sd = {k: torch.from_numpy(v) for k, v in seeded_state_dict(3).items()}
    x = torch.randn(2, 69, 5, 6, generator=torch.Generator().manual_seed(4))
    ref64, ref32 = B.decoder_refs(sd, 1, x)
    B.check_decoder("fp32 CPU decoder", ref32, ref64, ref32)
    with pytest.raises(B.StageError):
        B.check_decoder("scaled decoder", ref32 * (1 + 2.0 ** -14), ref64, ref32)
