"""Self-tests of the fp64 BACKWARD references of oracle/fp64_bounds.py, on the CPU: fp32 arithmetic of each adjoint passes at the limits of
the backward forms it stands for (torch autograd, a weight gradient summed in 32-pixel K steps whose partials meet in shuffled order as
the kernels' atomics add them, the six-product bf16-piece weight gradient), and each planted fault - the kinds of bug a tiled backward
kernel has - is rejected with its worst element named.  The weight gradients run at K = 10^5 pixels and more, as the training step's
do.  torch's CPU data gradients are direct fp32 convolutions: they are held to the direct form's limits (the stride-2 kernels' slope
limit, 0.063 u, is calibrated on their own unbiased sums; torch's CPU sums show up to 0.055 u depending on the thread count).

How far outside its family's limits each fault lands (max|z| against the limit; the dropped bf16 cross product by its slope):
hi*lo dropped: slope 123 u (2.4); a skipped last K step: 1.2e4 (9.5); an image missing from a bias: 1.7e5 (11); odd/odd parity a row
off: 1.4e7 (16); the wrong tensor's gate: 4.8e7 (11); pooling over the truncated rows: 9.4e4 (16); corr clamped at the border: 5.1e7
(6.8); the last column's upsample weight dropped: 3.3e4 (1.0); one group's shuffle inverted: 1.4e7 (7.6).
No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import eemflow_oracle as O
from oracle import fp64_bounds as B

KAIMING = np.sqrt(2.0)
WORST = r"Worst element \(image \d+, channel \d+, y \d+, x \d+\)"


def rnd(seed, *shape, scale=1.0, sparse=None):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    if sparse is not None:
        t = t * (torch.rand(*shape, generator=g) < sparse)
    return t.float()


def leaky32(v):
    return torch.where(v >= 0, v, v * torch.tensor(0.1, dtype=torch.float32))


def layer(seed, n, cin, cout, h, w, stride=1):
    """A gated conv layer's operands: input x (a LeakyReLU output), weights, the stored output y and its (pre-activation) gradient."""
    x = leaky32(rnd(seed, n, cin, h, w))
    wt = rnd(seed + 1, cout, cin, 3, 3, scale=KAIMING / np.sqrt(cin * 9))
    y = leaky32(F.conv2d(x, wt, stride=stride, padding=1))
    dy = rnd(seed + 2, *y.shape) * B.gate(y).float()
    return x, wt, y, dy


def dgrad32(dy, w, in_hw, stride=1, groups=1, padding=1):
    size = (dy.shape[0], w.shape[1] * groups, *in_hw)
    return torch.nn.grad.conv2d_input(size, w, dy, stride=stride, padding=padding, groups=groups)


def blocked_wgrad32(x, dy, stride=1, skip=None, seed=0):
    """fp32 weight gradient as the kernels form it: per image, 32-pixel K steps (fp32 products summed in fp32), the partials added in a
    shuffled order (the atomics' order).  skip = (image, step) drops that partial."""
    n, cout = dy.shape[:2]
    cols = F.unfold(x, 3, padding=1, stride=stride)                      # [n, cin * 9, L]
    g = dy.reshape(n, cout, -1)
    L = g.shape[2]
    parts = []
    for i in range(n):
        steps = -(-L // 32)
        for j in range(steps):
            if skip is not None and (i, j if skip[1] >= 0 else j - steps) == skip:
                continue
            parts.append(torch.matmul(g[i, :, j * 32:(j + 1) * 32], cols[i, :, j * 32:(j + 1) * 32].T))
    order = torch.randperm(len(parts), generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros_like(parts[0])
    for k in order.tolist():
        acc = acc + parts[k]
    return acc.view(cout, x.shape[1], 3, 3)


def split3(a):
    """a = hi + mid + lo exactly, each a bf16 value (truncation), as the bf16-piece kernels cut their operands."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = (a - hi).astype(np.float32)
    mid = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return hi, mid, (r - mid).astype(np.float32)


SIX = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]


def bx3_wgrad32(x, dy, drop=None):
    """The bf16-piece weight gradient: both operands as three bf16 pieces, the six products of SIX (fp32-exact) accumulated in fp32 per
    32-pixel step, the steps added in fp32; `drop` removes one product."""
    n, cout = dy.shape[:2]
    cols = F.unfold(x, 3, padding=1).numpy()
    g = dy.reshape(n, cout, -1).numpy()
    acc = np.zeros((cout, cols.shape[1]), np.float32)
    for i in range(n):
        gp, cp = split3(g[i]), split3(cols[i])
        for j in range(0, g.shape[2], 32):
            step = np.zeros_like(acc)
            for p, q in SIX:
                if (p, q) != drop:
                    step += np.matmul(gp[p][:, j:j + 32], cp[q][:, j:j + 32].T).astype(np.float32)
            acc += step
    return torch.from_numpy(acc).view(cout, x.shape[1], 3, 3)


# ------------------------------------------------------------------------------------------------------------------- passes
def test_fp32_autograd_of_each_adjoint_passes():
    x, w, y, dy = layer(1, 2, 32, 32, 40, 72)
    ref, mag = B.conv_dgrad_ref(dy, w, x.shape[-2:], x_gate=x)
    B.check("dgrad s1", dgrad32(dy, w, x.shape[-2:]) * B.gate(x).float(), ref, mag, "dgrad_direct")
    x, w, y, dy = layer(2, 2, 16, 32, 46, 36, stride=2)
    dpool = rnd(3, 2, 16, 1, 1)
    ref, mag = B.stage_dgrad_ref(dy, w, x, dpool, 32)
    pool = torch.zeros_like(x)
    pool[:, :, :32, :32] = dpool.repeat_interleave(32, 2).repeat_interleave(32, 3) / 1024
    got = (dgrad32(dy, w, x.shape[-2:], 2) + pool) * B.gate(x).float()
    B.check("dgrad s2 + pool", got, ref, mag, "dgrad_direct")
    gy = rnd(4, 2, 100, 5, 6)
    wg = rnd(5, 100, 20, 3, 3, scale=KAIMING / np.sqrt(180))
    ref, mag = B.conv_dgrad_ref(gy, wg, (5, 6), groups=5)
    B.check("grouped dgrad", dgrad32(gy, wg, (5, 6), groups=5), ref, mag, "tail_dgrad")
    w1 = rnd(6, 2, 6, 1, 1)
    gc = rnd(7, 2, 2, 5, 6)
    ref, mag = B.conv_dgrad_ref(gc, w1, (5, 6), padding=0)
    B.check("out_conv dgrad", dgrad32(gc, w1, (5, 6), padding=0), ref, mag, "tail_dgrad")
    dp = rnd(8, 4, 64, 5, 6)
    ref, mag = B.pool_bwd_ref(dp, (43, 50), 8)
    got = torch.zeros(4, 64, 43, 50)
    got[:, :, :40, :48] = dp.repeat_interleave(8, 2).repeat_interleave(8, 3) / 64
    B.check("pool bwd", got, ref, mag, "pool_bwd")
    p1, p2, dcv = rnd(9, 2, 32, 5, 6), rnd(10, 2, 32, 5, 6), rnd(11, 2, 53, 5, 6)
    a, b = p1.clone().requires_grad_(), p2.clone().requires_grad_()
    O.local_corr53(a, b).backward(dcv)
    (rx, mx), (ry, my) = B.corr_bwd_ref(dcv, p1, p2)
    B.check("corr bwd x", a.grad, rx, mx, "corr_bwd")
    B.check("corr bwd y", b.grad, ry, my, "corr_bwd")
    d = rnd(12, 2, 2, 260, 346)
    c = torch.zeros(2, 2, 5, 6, requires_grad=True)
    O.upsample_flow(c, (260, 346)).backward(d)
    ref, mag = B.upsample_bwd_ref(d, (5, 6))
    B.check("ups bwd", c.grad, ref, mag, "ups_bwd")
    B.check("ups bwd (manual)", ups_bwd32(d, (5, 6)), ref, mag, "ups_bwd")


@pytest.mark.parametrize("stride,n,h,w", [(1, 4, 160, 192), (2, 2, 320, 384)])        # K = 122 880 output pixels
def test_blocked_fp32_weight_gradient_in_shuffled_order_passes(stride, n, h, w):
    x, _, y, dy = layer(20 + stride, n, 16, 32, h, w, stride)
    dw, mw, db, mb = B.conv_wgrad_ref(x, dy, (32, 16, 3, 3), stride=stride)
    for fam in ("wgrad_fp32", "wgrad_bx3"):                # (the tile kernels of the long-K encoder layers)
        B.check(f"blocked wgrad s{stride}", blocked_wgrad32(x, dy, stride), dw, mw, fam)
        B.check("bias", dy.sum((0, 2, 3)), db, mb, fam)


def test_six_product_bf16_weight_gradient_passes():
    x, _, y, dy = layer(30, 4, 32, 32, 160, 192)                            # K = 122 880
    dw, mw, _, _ = B.conv_wgrad_ref(x, dy, (32, 32, 3, 3))
    B.check("bx3 wgrad", bx3_wgrad32(x, dy), dw, mw, "wgrad_bx3")


# -------------------------------------------------------------------------------------------------------------- planted faults
def test_bf16_weight_gradient_without_one_cross_product_fails():
    x, _, y, dy = layer(31, 4, 32, 32, 160, 192)
    dw, mw, _, _ = B.conv_wgrad_ref(x, dy, (32, 32, 3, 3))
    with pytest.raises(B.StageError, match=r"slope.*Worst element"):
        B.check("bx3 wgrad without hi*lo", bx3_wgrad32(x, dy, drop=(0, 2)), dw, mw, "wgrad_bx3")


@pytest.mark.parametrize("stride,n,h,w", [(1, 15, 70, 100), (2, 15, 140, 200)])        # 70 x 100 outputs per image: K = 105 000
def test_skipped_last_partial_k_step_of_one_image_fails(stride, n, h, w):
    """The last 32-pixel step of image 1 (a partial one: the image's pixel count is not a multiple of 32) never added."""
    x, _, y, dy = layer(40 + stride, n, 16, 32, h, w, stride)
    assert (dy.shape[2] * dy.shape[3]) % 32 != 0
    dw, mw, _, _ = B.conv_wgrad_ref(x, dy, (32, 16, 3, 3), stride=stride)
    B.check("blocked", blocked_wgrad32(x, dy, stride), dw, mw, "wgrad_fp32")
    with pytest.raises(B.StageError, match=r"max\|z\|.*" + WORST):                  # (for a weight: cout, cin, ky, kx)
        B.check("skipped K step", blocked_wgrad32(x, dy, stride, skip=(1, -1)), dw, mw, "wgrad_fp32")


def test_bias_gradient_missing_one_image_fails():
    x, _, y, dy = layer(50, 4, 16, 32, 80, 96)
    _, _, db, mb = B.conv_wgrad_ref(x, dy, (32, 16, 3, 3))
    with pytest.raises(B.StageError, match=r"Worst element \(\d+,\)"):
        B.check("bias without image 2", dy[[0, 1, 3]].sum((0, 2, 3)), db, mb, "wgrad_batched")


def test_stride2_odd_odd_parity_reading_the_next_dy_row_fails():
    x, w, y, dy = layer(60, 2, 32, 64, 40, 48, stride=2)
    dpool = rnd(61, 2, 32, 2, 3)
    ref, mag = B.stage_dgrad_ref(dy, w, x, dpool, 16)
    pool = torch.zeros_like(x)
    pool[:, :, :32, :48] = dpool.repeat_interleave(16, 2).repeat_interleave(16, 3) / 256
    good = (dgrad32(dy, w, x.shape[-2:], 2) + pool) * B.gate(x).float()
    B.check("dgrad_s2", good, ref, mag, "dgrad_direct")
    shifted = torch.cat([dy[:, :, 1:], torch.zeros_like(dy[:, :, :1])], 2)      # dY row + 1
    bad = good.clone()
    bad[:, :, 1::2, 1::2] = ((dgrad32(shifted, w, x.shape[-2:], 2) + pool) * B.gate(x).float())[:, :, 1::2, 1::2]
    with pytest.raises(B.StageError, match=r"Worst element \(image \d+, channel \d+, y \d*[13579], x \d*[13579]\)"):
        B.check("odd/odd parity off by a row", bad, ref, mag, "dgrad_direct")


def test_gate_from_the_wrong_tensor_fails():
    """g_b3 = conv^T(g_f13) * LeakyReLU'(b3); the planted form gates with a3 (the layer before's output, same shape)."""
    a3 = leaky32(rnd(70, 2, 64, 24, 32))
    w2 = rnd(71, 64, 64, 3, 3, scale=KAIMING / 24)
    b3 = leaky32(F.conv2d(a3, w2, padding=1))
    w3 = rnd(72, 64, 64, 3, 3, scale=KAIMING / 24)
    g = rnd(73, 2, 64, 24, 32)
    ref, mag = B.conv_dgrad_ref(g, w3, (24, 32), x_gate=b3)
    B.check("gate b3", dgrad32(g, w3, (24, 32)) * B.gate(b3).float(), ref, mag, "dgrad_wino2")
    with pytest.raises(B.StageError, match=WORST):
        B.check("gate a3", dgrad32(g, w3, (24, 32)) * B.gate(a3).float(), ref, mag, "dgrad_wino2")


def test_pooling_branch_spread_over_the_truncated_rows_fails():
    """A ragged 46 x 36 map under 32 x 32 pooling (the 92 x 72 padded size): rows 32..45 and columns 32..35 get no pooling term."""
    x, w, y, dy = layer(80, 2, 16, 32, 46, 36, stride=2)
    dpool = rnd(81, 2, 16, 1, 1)
    ref, mag = B.stage_dgrad_ref(dy, w, x, dpool, 32)
    conv = dgrad32(dy, w, x.shape[-2:], 2)
    spread = conv + (dpool / 1024).expand(-1, -1, 46, 36)                          # py = min(y / k, gh - 1): every pixel
    good = conv.clone()
    good[:, :, :32, :32] += dpool / 1024
    B.check("pool branch", good * B.gate(x).float(), ref, mag, "dgrad_direct")
    with pytest.raises(B.StageError, match=r"Worst element \(image \d+, channel \d+, y (3[2-9]|4[0-5]|\d+), x (3[2-5]|\d+)\)"):
        B.check("pool branch spread", spread * B.gate(x).float(), ref, mag, "dgrad_direct")


def corr53_clamped(x, y):
    """The correlation with y read at clamped coordinates (replicate) instead of zero outside the image."""
    b, c, h, w = x.shape
    yp = F.pad(y, (4, 4, 4, 4), mode="replicate")
    out = []
    for t in O.CORR_TAPS_53:
        dy, dx = t // 9 - 4, t % 9 - 4
        out.append((x * yp[:, :, 4 + dy:4 + dy + h, 4 + dx:4 + dx + w]).sum(1))
    return torch.stack(out, 1) / c


def test_corr_backward_clamping_at_the_border_fails():
    p1, p2, dcv = rnd(90, 2, 32, 5, 6), rnd(91, 2, 32, 5, 6), rnd(92, 2, 53, 5, 6)
    a, b = p1.clone().requires_grad_(), p2.clone().requires_grad_()
    corr53_clamped(a, b).backward(dcv)
    (rx, mx), (ry, my) = B.corr_bwd_ref(dcv, p1, p2)
    with pytest.raises(B.StageError, match=WORST):
        B.check("clamped corr bwd x", a.grad, rx, mx, "corr_bwd")
    with pytest.raises(B.StageError, match=WORST):
        B.check("clamped corr bwd y", b.grad, ry, my, "corr_bwd")


def ups_bwd32(d, hw, drop_last_col=False):
    """fp32 adjoint of the bilinear upsample, separable (x, then y), with align_corners=False's source coordinates; drop_last_col
    loses the weight that interior outputs give the map's last column."""
    n, c, oh, ow = d.shape
    h, w = hw

    def axis(src_n, dst_n):
        s = torch.clamp((torch.arange(dst_n, dtype=torch.float32) + 0.5) * (src_n / dst_n) - 0.5, min=0.0)
        i0 = s.floor().long()
        i1 = torch.clamp(i0 + 1, max=src_n - 1)
        l1 = s - i0.float()
        return i0, i1, 1 - l1, l1
    x0, x1, wx0, wx1 = axis(w, ow)
    if drop_last_col:
        wx1 = torch.where((x1 == w - 1) & (x0 != x1), torch.zeros_like(wx1), wx1)
    tmp = torch.zeros(n, c, oh, w)
    tmp.index_add_(3, x0, d * wx0)
    tmp.index_add_(3, x1, d * wx1)
    y0, y1, wy0, wy1 = axis(h, oh)
    out = torch.zeros(n, c, h, w)
    out.index_add_(2, y0, tmp * wy0[:, None])
    out.index_add_(2, y1, tmp * wy1[:, None])
    return out


def test_upsample_adjoint_without_the_last_column_weight_fails():
    d = rnd(100, 2, 2, 260, 346)
    ref, mag = B.upsample_bwd_ref(d, (5, 6))
    with pytest.raises(B.StageError, match=r"Worst element \(image \d+, channel \d+, y \d+, x 5\)"):
        B.check("ups bwd, last column", ups_bwd32(d, (5, 6), drop_last_col=True), ref, mag, "ups_bwd")


def test_one_decoder_group_with_its_shuffle_inverted_fails():
    """conv4's data gradient: the gated gradient of the SHUFFLED output goes back to the conv's channel order first; group 1 skips it."""
    td = leaky32(rnd(110, 2, 100, 5, 6))
    g_td = rnd(111, 2, 100, 5, 6)
    w4 = rnd(112, 100, 20, 3, 3, scale=KAIMING / np.sqrt(180))
    pre = g_td * B.gate(td).float()
    dy = O.channel_shuffle(pre, 20)
    ref, mag = B.conv_dgrad_ref(B.shuffle(B._d(g_td) * B.gate(td), 20), w4, (5, 6), groups=5)
    B.check("grouped", dgrad32(dy, w4, (5, 6), groups=5), ref, mag, "tail_dgrad")
    bad = dy.clone()
    bad[:, 20:40] = pre[:, 20:40]
    with pytest.raises(B.StageError, match=r"Worst element \(image \d+, channel (2\d|3\d), y \d+, x \d+\)"):
        B.check("group 1 unshuffled", dgrad32(bad, w4, (5, 6), groups=5), ref, mag, "tail_dgrad")


def test_loss_gradient_reference_is_exact():
    """sign(flow - gt) valid / (B 2 H W): the valid mask and the |gt| < 400 edge, in fp32 as the loss kernel computes them."""
    flow = rnd(120, 2, 2, 6, 7)
    gt = rnd(121, 2, 2, 6, 7)
    gt[0, 0, 0, :3] = 500.0
    gt[1, :, 2, 2] = torch.tensor([0.0, 399.99997])
    gt[1, :, 3, 3] = torch.tensor([0.0, 400.0])
    flow[1, :, 4, 4] = gt[1, :, 4, 4]
    valid = (rnd(122, 2, 6, 7) > -0.5).float()
    valid[0, 5, 6] = 0.5
    valid[1, 5, 6] = 0.49999997
    g = B.loss_grad_ref(flow, gt, valid)
    s = 1.0 / (2 * 2 * 6 * 7)
    assert bool((g[0, :, 0, :3] == 0).all()) and bool((g[1, :, 2, 2].abs() == np.float32(s)).all()) and bool((g[1, :, 3, 3] == 0).all())
    assert bool((g[1, :, 4, 4] == 0).all()) and bool((g[0, :, 5, 6].abs() == np.float32(s)).all()) and bool((g[1, :, 5, 6] == 0).all())
    ok = (valid >= 0.5) & (gt.double().norm(dim=1) < 400)
    assert torch.equal(g, torch.sign(flow - gt) * ok[:, None].float() * np.float32(s))
