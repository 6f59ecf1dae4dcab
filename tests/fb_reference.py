"""CPU restatement of the forward-backward consistency check (the reference's occ_check_model on tensor_tools.torch_warp,
utils_luo/tools.py:1136-1309 / :2262-2306), in the dtype of its inputs: fp32 reproduces the reference's masks (pinned by
tests/golden/fb_check.npz), fp64 is what the GPU kernel's masks are judged against, with the margin of every pixel's decision.

    thresh  = alpha1 * (len(fw) + len(bw)) + alpha2                  len(x) = sqrt(x_u^2 + x_v^2)
    mask_fw = len(fw + torch_warp(bw, fw)) < thresh
    mask_bw = len(bw + torch_warp(fw, bw)) < thresh
"""
import torch
import torch.nn.functional as F

MODES = ("all", "obj", "out")


def torch_warp(x, flo):
    """x [B,C,H,W] sampled at pixel + flo [B,2,H,W]: coordinates normalised by W - 1 / H - 1, then grid_sample's default
    align_corners=False with zero padding (so the sample sits half a pixel off - the reference's own behaviour)."""
    b, _, h, w = x.shape
    xx = torch.arange(0, w).view(1, -1).repeat(h, 1).view(1, 1, h, w).repeat(b, 1, 1, 1)
    yy = torch.arange(0, h).view(-1, 1).repeat(1, w).view(1, 1, h, w).repeat(b, 1, 1, 1)
    vgrid = torch.cat((xx, yy), 1).to(flo.dtype) + flo
    gx = 2.0 * vgrid[:, 0] / max(w - 1, 1) - 1.0
    gy = 2.0 * vgrid[:, 1] / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((gx, gy), dim=3), mode="bilinear", padding_mode="zeros", align_corners=False)


def length(x):
    return torch.pow(torch.sum(x ** 2, dim=1, keepdim=True), 0.5)


def outgoing(flow):
    """1 where pixel + flow stays inside [0, W-1] x [0, H-1], 0 where it leaves."""
    b, _, h, w = flow.shape
    xx = torch.arange(0, w).view(1, 1, 1, w).to(flow.dtype)
    yy = torch.arange(0, h).view(1, 1, h, 1).to(flow.dtype)
    pos_x, pos_y = xx + flow[:, 0:1], yy + flow[:, 1:2]
    return (~((pos_x > w - 1) | (pos_x < 0) | (pos_y > h - 1) | (pos_y < 0))).to(flow.dtype)


def fb_check_terms(flow_fw, flow_bw, alpha1, alpha2):
    """(len(diff_fw), len(diff_bw), thresh), each [B,1,H,W]."""
    thresh = alpha1 * (length(flow_fw) + length(flow_bw)) + alpha2
    diff_fw = flow_fw + torch_warp(flow_bw, flow_fw)
    diff_bw = flow_bw + torch_warp(flow_fw, flow_bw)
    return length(diff_fw), length(diff_bw), thresh


def fb_check_reference(flow_fw, flow_bw, alpha1=1.0, alpha2=0.05, obj_out_all="all"):
    """(mask_fw, mask_bw) [B,1,H,W] holding 0 / 1 in the flows' dtype."""
    assert obj_out_all in MODES
    if obj_out_all == "out":
        return outgoing(flow_fw), outgoing(flow_bw)
    lf, lb, thresh = fb_check_terms(flow_fw, flow_bw, alpha1, alpha2)
    mf, mb = (lf < thresh).to(flow_fw.dtype), (lb < thresh).to(flow_fw.dtype)
    if obj_out_all == "obj":
        mf = torch.where(outgoing(flow_fw) == 0, torch.ones_like(mf), mf)
        mb = torch.where(outgoing(flow_bw) == 0, torch.ones_like(mb), mb)
    return mf, mb


def fb_check_margins(flow_fw, flow_bw, alpha1, alpha2):
    """|len(diff) - thresh| per pixel and direction in fp64: how far each pixel's decision is from flipping."""
    lf, lb, thresh = fb_check_terms(flow_fw.double(), flow_bw.double(), alpha1, alpha2)
    return (lf - thresh).abs(), (lb - thresh).abs()


def synthetic_pair(h, w, dtype=torch.float32):
    """fw = [6 sin(2 pi x / W) + 2, 4 cos(2 pi y / H)], bw = -fw + 3 sin(2 pi (x + y) / 97) [1, -1]: flows of a few pixels that leave the
    frame at the borders and disagree by up to 3 px, so both mask values occur.  Built in fp64, rounded once."""
    import math
    y = torch.arange(h, dtype=torch.float64).view(h, 1).expand(h, w)
    x = torch.arange(w, dtype=torch.float64).view(1, w).expand(h, w)
    fw = torch.stack((6 * torch.sin(2 * math.pi * x / w) + 2, 4 * torch.cos(2 * math.pi * y / h)))
    d = 3 * torch.sin(2 * math.pi * (x + y) / 97)
    bw = -fw + torch.stack((d, -d))
    return fw[None].to(dtype).contiguous(), bw[None].to(dtype).contiguous()
