"""Evaluation metrics on the GPU: the reference's Test.flow_error (test_mvsec.py:291-346) behind its call shape.

`flow_error(flow_gt, flow_pred, event_img, is_car=False, evaluation_type='dense')` takes the (1,2,H,W) CUDA tensors the
harness holds and returns the reference's 7-tuple (AEE, percent_1_AEE, percent_3_AEE, n_points, AEE_sum, AEE_gt,
AEE_gt_sum); the reduction runs in libeemflow_hip.so (eemflow_flow_error).  CUDA tensors only.

`fb_check(flow_fw, flow_bw, alpha1, alpha2, obj_out_all)` is the reference's forward-backward consistency check (occ_check_model,
utils_luo/tools.py:1136-1309): the masks of a bidirectional flow pair, by eemflow_fb_check_many.  A mask is a valid `event_img` of the
'sparse' `flow_error`: the statistics over the consistent pixels."""
import torch

from . import _lib


def flow_error_sums(flow_gt, flow_pred, event_img=None, is_car=False, evaluation_type="dense"):
    """The reduction only, no host synchronisation: a device tensor of 5 doubles (sum EE, sum |gt|, n, count(EE < 1),
    count(EE < 3 or EE < 0.1 |gt|)) on the current stream; `flow_error_from_sums` turns it into the reference's 7-tuple."""
    if not (flow_gt.is_cuda and flow_pred.is_cuda):
        raise _lib.EEMFlowHipError("flow_error: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    gt = flow_gt[0].contiguous().float()
    pr = flow_pred[0].contiguous().float()
    _, h, w = gt.shape
    max_row = 190 if is_car else w                         # the reference crops rows with shape[1] = the WIDTH (:296)
    ev = None
    if evaluation_type == "sparse":
        ev = event_img.to(gt.device).reshape(h, w).contiguous().float()
    elif evaluation_type != "dense":
        raise ValueError(f"evaluation_type {evaluation_type!r}")
    out = torch.empty(5, dtype=torch.float64, device=gt.device)
    with torch.cuda.device(gt.device):
        _lib.check(_lib.lib().eemflow_flow_error(gt.data_ptr(), pr.data_ptr(), ev.data_ptr() if ev is not None else None, h, w,
                                                 max_row, out.data_ptr(), _lib.current_stream_ptr(gt.device)))
    return out


def flow_error_sums_many(flow_gts, flow_preds, event_imgs=None, is_car=False, evaluation_type="dense"):
    """`[flow_error_sums(g, p, e) for ...]` for up to 16 samples of one size by ONE launch (eemflow_flow_error_many): returns an (n, 5)
    float64 device tensor, row i = sample i's five sums."""
    import ctypes
    n = len(flow_gts)
    if not 1 <= n <= 16 or len(flow_preds) != n:
        raise ValueError("flow_error_sums_many: 1..16 samples, as many predictions as ground truths")
    if not all(t.is_cuda for t in list(flow_gts) + list(flow_preds)):
        raise _lib.EEMFlowHipError("flow_error: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    gts = [g[0].contiguous().float() for g in flow_gts]
    prs = [p[0].contiguous().float() for p in flow_preds]
    _, h, w = gts[0].shape
    if any(tuple(t.shape) != (2, h, w) for t in gts + prs):
        raise ValueError("flow_error_sums_many: all samples share one (2,H,W) shape")
    max_row = 190 if is_car else w
    evs = None
    if evaluation_type == "sparse":
        evs = [e.to(gts[0].device).reshape(h, w).contiguous().float() for e in event_imgs]
    elif evaluation_type != "dense":
        raise ValueError(f"evaluation_type {evaluation_type!r}")
    dev = gts[0].device
    out = torch.empty(n, 5, dtype=torch.float64, device=dev)
    arr = ctypes.c_void_p * n
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().eemflow_flow_error_many(n, arr(*[t.data_ptr() for t in gts]), arr(*[t.data_ptr() for t in prs]),
                                                      arr(*[t.data_ptr() for t in evs]) if evs is not None else None, h, w, max_row,
                                                      out.data_ptr(), _lib.current_stream_ptr(dev)))
    return out


def flow_error_from_sums(sums):
    s_ee, s_gt, n, n1, n3 = sums.cpu().tolist() if torch.is_tensor(sums) else sums
    p1 = n1 / (n + 1e-5)
    p3 = n3 / (n + 1e-5)
    if s_ee == 0:
        return 0.0, p1, p3, int(n), 0.0, 0.0, 0.0
    return s_ee / n, p1, p3, int(n), s_ee, s_gt / n, s_gt


def flow_error(flow_gt, flow_pred, event_img=None, is_car=False, evaluation_type="dense"):
    return flow_error_from_sums(flow_error_sums(flow_gt, flow_pred, event_img, is_car, evaluation_type))


FB_MODES = {"all": 0, "obj": 1, "out": 2}


def fb_check_args(alpha1=1.0, alpha2=0.05, obj_out_all="all"):
    """(alpha1, alpha2, obj_out_all) checked: the reference's constructor arguments (occ_check_model.__init__, its defaults)."""
    if obj_out_all not in FB_MODES:
        raise ValueError(f"fb_check: obj_out_all must be one of {sorted(FB_MODES)}, got {obj_out_all!r}")
    return float(alpha1), float(alpha2), obj_out_all


def fb_check_many(flows_fw, flows_bw, alpha1=1.0, alpha2=0.05, obj_out_all="all"):
    """The masks of len(flows_fw) pairs of [1, 2, H, W] CUDA flows of one size: a list of (mask_fw, mask_bw), each [1, 1, H, W] float32
    holding 1.0 (consistent) or 0.0.  One launch per 16 pairs, on the current stream."""
    import ctypes
    alpha1, alpha2, obj_out_all = fb_check_args(alpha1, alpha2, obj_out_all)
    n = len(flows_fw)
    if n < 1 or len(flows_bw) != n:
        raise ValueError("fb_check: as many backward flows as forward flows, at least one")
    if not all(t.is_cuda for t in list(flows_fw) + list(flows_bw)):
        raise _lib.EEMFlowHipError("fb_check: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    fws = [t.contiguous().float() for t in flows_fw]
    bws = [t.contiguous().float() for t in flows_bw]
    shape, dev = tuple(fws[0].shape), fws[0].device
    if len(shape) != 4 or shape[0] != 1 or shape[1] != 2 or any(tuple(t.shape) != shape or t.device != dev for t in fws + bws):
        raise ValueError("fb_check: all flows share one (1,2,H,W) shape and one device")
    h, w = shape[2], shape[3]
    masks = [(torch.empty(1, 1, h, w, device=dev, dtype=torch.float32), torch.empty(1, 1, h, w, device=dev, dtype=torch.float32))
             for _ in range(n)]
    with torch.cuda.device(dev):
        for i0 in range(0, n, 16):
            k = min(16, n - i0)
            arr = ctypes.c_void_p * k
            _lib.check(_lib.lib().eemflow_fb_check_many(
                k, arr(*[t.data_ptr() for t in fws[i0:i0 + k]]), arr(*[t.data_ptr() for t in bws[i0:i0 + k]]),
                arr(*[m[0].data_ptr() for m in masks[i0:i0 + k]]), arr(*[m[1].data_ptr() for m in masks[i0:i0 + k]]), h, w,
                alpha1, alpha2, FB_MODES[obj_out_all], _lib.current_stream_ptr(dev)))
    return masks


def fb_check(flow_fw, flow_bw, alpha1=1.0, alpha2=0.05, obj_out_all="all"):
    """Forward-backward consistency masks of two CUDA flows [B, 2, H, W] (any model's: EEMFlow's bidirectional stream, E-RAFT's or
    EEMFlow+'s two passes): `(mask_fw, mask_bw)`, each [B, 1, H, W] float32, 1.0 where
        |fw + torch_warp(bw, fw)| < alpha1 * (|fw| + |bw|) + alpha2          (mask_bw: the two flows exchanged)
    and 0.0 where the pixel is occluded or the flows disagree.  obj_out_all: 'all' these masks; 'obj' pixels whose target leaves the
    frame are forced to 1; 'out' the outgoing mask alone.  Defaults: the reference's constructor defaults
    (occ_check_model.__init__, utils_luo/tools.py:1138).  No gradient (the reference's mask is a comparison)."""
    if not (torch.is_tensor(flow_fw) and torch.is_tensor(flow_bw)):
        raise TypeError("fb_check: flow_fw and flow_bw are tensors")
    if not (flow_fw.is_cuda and flow_bw.is_cuda):
        raise _lib.EEMFlowHipError("fb_check: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if flow_fw.dim() != 4 or flow_fw.shape[1] != 2 or flow_fw.shape != flow_bw.shape:
        raise ValueError(f"fb_check: two (B,2,H,W) flows of one shape, got {tuple(flow_fw.shape)} and {tuple(flow_bw.shape)}")
    fw = flow_fw.detach().contiguous().float()
    bw = flow_bw.detach().contiguous().float()
    b = fw.shape[0]
    pairs = fb_check_many([fw[i:i + 1] for i in range(b)], [bw[i:i + 1] for i in range(b)], alpha1, alpha2, obj_out_all)
    return torch.cat([m for m, _ in pairs], 0), torch.cat([m for _, m in pairs], 0)
