"""The two augmentors the dataset front-ends use, as they behave in the reference as shipped (utils/augumentor.py).

`FlowAugmentor` as loader/HREM.py:148,252 calls it (`without_resize=True`, :202-257) and `DenseSparseAugmentor` (:329-433, the
one loader/MVSEC.py:57,176 means to use): on these paths every rescaling branch of the reference is commented out and the
eraser / colour jitter are never called, so what runs is random flips and - for DenseSparseAugmentor - a random crop, all on
HWC numpy arrays.  `FlowAugmentor` with rescaling (no loader of the path calls it) goes through cv2.resize(INTER_LINEAR) in the
reference; cv2 is absent here, so `resize_linear` restates its rule for floating-point arrays (half-pixel centres, edge clamp, output
size round(src * scale)) - PARITY UNPINNED against cv2 itself, checked against torch's bilinear interpolation which follows the
same convention (tests/test_data_rows.py).  The random draws are made with `numpy.random` in the reference's order, so a seeded run reproduces the reference's
output bit for bit (tests/golden/augmentor.npz is produced by executing the reference classes).  cv2 / torchvision, which
the reference imports for the dead branches, are not needed.

Plans apart from pixels: `FlowAugmentor.draw` / `DenseSparseAugmentor.draw` make the random draws of `__call__` (the same calls in the
same order) and return an `AugPlan`; `apply_host(plan, *arrays)` does the pixel work in numpy, `augment_many(plans, ...)` does it on
the GPU for up to 16 samples by one launch, straight into the batch tensors (csrc/augment.hip) - bit for bit the same arrays, so the
datasets' `get_batch` and `ThreadedBatchLoader(device_batches=True)` deliver the host route's batches without the event volumes ever
visiting host memory.  `__call__` itself is as the reference has it.
"""
import numpy as np


def resize_linear(img, fx, fy):
    """cv2.resize(img, None, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR) for a floating-point HWC (or HW) array: output size
    (round(h * fy), round(w * fx)); destination pixel d samples the source at (d + 0.5) / f - 0.5 with f the GIVEN factor (cv2 uses
    fx / fy only to round the output size and maps with 1 / fx, 1 / fy - not with src / dst, which drifts by a sub-pixel towards the far
    edge whenever src * f is not an integer), the two neighbours clamped to the image."""
    a = np.asarray(img)
    h, w = a.shape[:2]
    oh, ow = int(round(h * fy)), int(round(w * fx))
    if oh < 1 or ow < 1:
        raise ValueError("resize_linear: empty output")

    def axis(n_src, n_dst, f):
        s = (np.arange(n_dst, dtype=np.float64) + 0.5) / float(f) - 0.5
        i0 = np.floor(s).astype(np.int64)
        t = s - i0
        lo = np.clip(i0, 0, n_src - 1)
        hi = np.clip(i0 + 1, 0, n_src - 1)
        return lo, hi, t

    y0, y1, ty = axis(h, oh, fy)
    x0, x1, tx = axis(w, ow, fx)
    f = a.astype(np.float64)
    tx = tx.reshape((1, ow) + (1,) * (a.ndim - 2))
    ty = ty.reshape((oh, 1) + (1,) * (a.ndim - 2))
    top = f[y0][:, x0] * (1.0 - tx) + f[y0][:, x1] * tx
    bot = f[y1][:, x0] * (1.0 - tx) + f[y1][:, x1] * tx
    return (top * (1.0 - ty) + bot * ty).astype(a.dtype if a.dtype.kind == "f" else np.float64)


AUGMENT_MAX = 16                                                   # samples per eemflow_augment_many call (EEMFLOW_AUGMENT_MAX)


class AugPlan:
    """What an augmentor's random draws decide for one sample, apart from the pixels: `resized` with the factors (scale_x, scale_y)
    and the resized size (RH, RW) - the source's when not resized -, the two flips, the crop's corner (y0, x0) and size `crop` = (ch, cw).
    The host applies it with `apply_host`, the GPU with `augment_many`; both resize first, then flip, then crop."""
    __slots__ = ("resized", "scale_x", "scale_y", "RH", "RW", "hflip", "vflip", "y0", "x0", "crop")

    def __init__(self, RH, RW, crop=None, y0=0, x0=0, hflip=False, vflip=False, resized=False, scale_x=1.0, scale_y=1.0):
        self.resized, self.scale_x, self.scale_y = bool(resized), scale_x, scale_y
        self.RH, self.RW, self.hflip, self.vflip = int(RH), int(RW), bool(hflip), bool(vflip)
        self.y0, self.x0 = int(y0), int(x0)
        self.crop = (int(crop[0]), int(crop[1])) if crop is not None else (self.RH, self.RW)

    def astuple(self):
        return (self.resized, float(self.scale_x), float(self.scale_y), self.RH, self.RW, self.hflip, self.vflip, self.y0, self.x0, self.crop)

    def event_map(self, h, w):
        """(ax, bx, ay, by): where an event at (x, y) of the h x w source frame lies in the augmented frame, x' = ax * x + bx and
        y' = ay * y + by - resize, then flip, then crop, in apply_host's order.  The resize is x' = (x + 0.5) * scale_x - 0.5, the
        inverse of the sample position (d + 0.5) / f - 0.5 that resize_linear uses; the horizontal flip x' = RW - 1 - x'; the crop
        x' -= x0; the same in y.  What eemflow_amd.iwe takes as `maps=`."""
        if not self.resized and (int(h), int(w)) != (self.RH, self.RW):
            raise ValueError(f"AugPlan.event_map: the plan was drawn for a {self.RH}x{self.RW} frame, not {h}x{w}")
        ax = ay = 1.0
        bx = by = 0.0
        if self.resized:
            ax, bx = float(self.scale_x), 0.5 * float(self.scale_x) - 0.5
            ay, by = float(self.scale_y), 0.5 * float(self.scale_y) - 0.5
        if self.hflip:
            ax, bx = -ax, (self.RW - 1) - bx
        if self.vflip:
            ay, by = -ay, (self.RH - 1) - by
        return ax, bx - self.x0, ay, by - self.y0

    def __repr__(self):
        return "AugPlan(resized=%r, scale_x=%r, scale_y=%r, RH=%d, RW=%d, hflip=%r, vflip=%r, y0=%d, x0=%d, crop=%r)" % self.astuple()


def event_map_after_offset(plan, offset, h, w):
    """The event map of a dataset sample: the dataset's own events_offset (ox, oy) first, x - ox, then the plan's map on the h x w frame;
    plan=None gives the pure offset map (1, -ox, 1, -oy)."""
    ox, oy = float(offset[0]), float(offset[1])
    if plan is None:
        return (1.0, -ox, 1.0, -oy)
    ax, bx, ay, by = plan.event_map(h, w)
    return (ax, bx - ax * ox, ay, by - ay * oy)


def apply_host(plan, *arrays):
    """The augmentors' pixel work for a drawn plan, in numpy: `arrays` are HWC images and, LAST, the HW2 flow, as the augmentors'
    __call__ takes them; returns them resized (resize_linear; the flow times the factors), flipped (the flow's sign with it) and
    cropped, C-contiguous - bit for bit what __call__ returns under the same draws."""
    *imgs, flow = arrays
    if plan.resized:
        imgs = [resize_linear(a, plan.scale_x, plan.scale_y) for a in imgs]
        flow = resize_linear(flow, plan.scale_x, plan.scale_y) * [plan.scale_x, plan.scale_y]
    if plan.hflip:
        imgs = [a[:, ::-1] for a in imgs]
        flow = flow[:, ::-1] * [-1.0, 1.0]
    if plan.vflip:
        imgs = [a[::-1, :] for a in imgs]
        flow = flow[::-1, :] * [1.0, -1.0]
    ch, cw = plan.crop
    sl = (slice(plan.y0, plan.y0 + ch), slice(plan.x0, plan.x0 + cw))
    return tuple(np.ascontiguousarray(a[sl]) for a in (*imgs, flow))


def augment_many(plans, vols_old, vols_new, flows=None, out=None):
    """`apply_host` of len(plans) (1..16) samples on the GPU, assembled as a batch by one launch (eemflow_augment_many): vols_old[i],
    vols_new[i] are (C,H,W) float32 CUDA tensors of one shape, flows None or one (2,H,W) float32 / float64 CUDA tensor per sample (one
    dtype), plans[i] an AugPlan, all of one crop size.  Returns `(old, new, flow, valid)`: (n,C,ch,cw), (n,C,ch,cw), (n,2,ch,cw),
    (n,ch,cw) float32 CUDA tensors, `valid` by MVSEC's rule ~isinf(u) & ~isinf(v) & (norm > 0); flow and valid are None without flows.
    `out=(old, new, flow, valid)` - e.g. slices [i0:i0+n] of a larger batch - is filled instead of fresh tensors.  Bit for bit the host
    route (a float64 flow is rounded to float32 once, after scaling and sign).  On the current stream, no host synchronisation.  CUDA
    tensors only: there is no CPU path."""
    import ctypes

    import torch

    from . import _lib
    name = "augment_many"
    plans, vols_old, vols_new = list(plans), list(vols_old), list(vols_new)
    n = len(plans)
    if n < 1 or len(vols_old) != n or len(vols_new) != n or (flows is not None and len(flows) != n):
        raise ValueError(f"{name}: one plan, one old and one new volume (and one flow) per sample, at least one sample")
    flows = list(flows) if flows is not None else None
    tensors = vols_old + vols_new + (flows or [])
    if not all(torch.is_tensor(t) for t in tensors):
        raise TypeError(f"{name}: volumes and flows are tensors")
    if not all(t.is_cuda for t in tensors):
        raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    shape, dev = tuple(vols_old[0].shape), vols_old[0].device
    if len(shape) != 3 or any(tuple(t.shape) != shape or t.device != dev for t in vols_old + vols_new):
        raise ValueError(f"{name}: all volumes share one (C,H,W) shape and one device, got {[tuple(t.shape) for t in vols_old + vols_new]}")
    if not all(t.is_contiguous() and t.dtype == torch.float32 for t in vols_old + vols_new):
        raise ValueError(f"{name}: volumes are contiguous float32 tensors (the kernel reads them where they are)")
    C, H, W = shape
    if flows is not None:
        if any(tuple(t.shape) != (2, H, W) or t.device != dev or t.dtype != flows[0].dtype for t in flows):
            raise ValueError(f"{name}: all flows share the (2,{H},{W}) shape of the volumes, one dtype and their device, got "
                             f"{[(tuple(t.shape), t.dtype) for t in flows]}")
        if flows[0].dtype not in (torch.float32, torch.float64) or not all(t.is_contiguous() for t in flows):
            raise ValueError(f"{name}: flows are contiguous float32 or float64 tensors (the kernel reads them where they are)")
    crop = plans[0].crop
    if any(p.crop != crop for p in plans):
        raise ValueError(f"{name}: all plans share one crop size, got {[p.crop for p in plans]}")
    ch, cw = crop
    shapes = ((n, C, ch, cw), (n, C, ch, cw), (n, 2, ch, cw), (n, ch, cw))
    if out is None:
        out = tuple(torch.empty(s, device=dev, dtype=torch.float32) if (k < 2 or flows is not None) else None for k, s in enumerate(shapes))
    else:
        out = tuple(out)
        if len(out) != 4 or any(not torch.is_tensor(t) for t in out[:2 if flows is None else 4]):
            raise TypeError(f"{name}: out is (old, new, flow, valid) tensors")
        for k, (t, s) in enumerate(zip(out, shapes)):
            if t is None and k >= 2 and flows is None:
                continue
            if not t.is_cuda:
                raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
            if tuple(t.shape) != s or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{name}: out[{k}] is a contiguous float32 {s} tensor on {dev}, got {tuple(t.shape)} {t.dtype}")
    table = (_lib.AugPlanC * n)()
    for i, p in enumerate(plans):
        table[i] = _lib.AugPlanC(float(p.scale_x), float(p.scale_y), int(p.resized), p.RH, p.RW, int(p.hflip), int(p.vflip), p.y0, p.x0, 0)
    arr = ctypes.c_void_p * n
    ptr = lambda t: t.data_ptr() if t is not None else None       # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().eemflow_augment_many(n, arr(*[t.data_ptr() for t in vols_old]), arr(*[t.data_ptr() for t in vols_new]),
                                                   arr(*[t.data_ptr() for t in flows]) if flows is not None else None,
                                                   1 if (flows is not None and flows[0].dtype == torch.float64) else 0, table, C, H, W, ch, cw,
                                                   ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), _lib.current_stream_ptr(dev)))
    return out[0], out[1], (out[2] if flows is not None else None), (out[3] if flows is not None else None)


class FlowAugmentor:
    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=False):
        self.crop_size = crop_size
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.do_flip = do_flip
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1
        self.spatial_aug_prob = 0.8                                # utils/augumentor.py:23-25
        self.stretch_prob = 0.8
        self.max_stretch = 0.2

    def spatial_transform(self, img1, img2, flow):
        """utils/augumentor.py:158-200: random rescale (the draws in the reference's order), flips, random crop."""
        ht, wd = img1.shape[:2]
        min_scale = np.maximum((self.crop_size[0] + 8) / float(ht), (self.crop_size[1] + 8) / float(wd))
        scale = 2 ** np.random.uniform(self.min_scale, self.max_scale)
        scale_x = scale_y = scale
        if np.random.rand() < self.stretch_prob:
            scale_x *= 2 ** np.random.uniform(-self.max_stretch, self.max_stretch)
            scale_y *= 2 ** np.random.uniform(-self.max_stretch, self.max_stretch)
        scale_x = np.clip(scale_x, min_scale, None)
        scale_y = np.clip(scale_y, min_scale, None)
        if np.random.rand() < self.spatial_aug_prob:
            img1 = resize_linear(img1, scale_x, scale_y)
            img2 = resize_linear(img2, scale_x, scale_y)
            flow = resize_linear(flow, scale_x, scale_y) * [scale_x, scale_y]
        if self.do_flip:
            if np.random.rand() < self.h_flip_prob:
                img1, img2 = img1[:, ::-1], img2[:, ::-1]
                flow = flow[:, ::-1] * [-1.0, 1.0]
            if np.random.rand() < self.v_flip_prob:
                img1, img2 = img1[::-1, :], img2[::-1, :]
                flow = flow[::-1, :] * [1.0, -1.0]
        y0 = np.random.randint(0, img1.shape[0] - self.crop_size[0])
        x0 = np.random.randint(0, img1.shape[1] - self.crop_size[1])
        ch, cw = self.crop_size[0], self.crop_size[1]
        return img1[y0:y0 + ch, x0:x0 + cw], img2[y0:y0 + ch, x0:x0 + cw], flow[y0:y0 + ch, x0:x0 + cw]

    def spatial_transform_no_resize(self, img1, img2, flow):
        if self.do_flip:                                           # :225-234
            if np.random.rand() < self.h_flip_prob:
                img1 = img1[:, ::-1]
                img2 = img2[:, ::-1]
                flow = flow[:, ::-1] * [-1.0, 1.0]
            if np.random.rand() < self.v_flip_prob:
                img1 = img1[::-1, :]
                img2 = img2[::-1, :]
                flow = flow[::-1, :] * [1.0, -1.0]
        return img1, img2, flow

    def draw(self, ht, wd, without_resize=False):
        """The random draws of __call__ for an ht x wd sample - the same numpy.random calls in the same order, those whose result goes
        unused included - as an AugPlan; no pixel is touched.  `apply_host(plan, img1, img2, flow)` is then __call__'s result."""
        if without_resize:
            hflip = vflip = False
            if self.do_flip:
                hflip = np.random.rand() < self.h_flip_prob
                vflip = np.random.rand() < self.v_flip_prob
            return AugPlan(ht, wd, hflip=hflip, vflip=vflip)
        min_scale = np.maximum((self.crop_size[0] + 8) / float(ht), (self.crop_size[1] + 8) / float(wd))
        scale = 2 ** np.random.uniform(self.min_scale, self.max_scale)
        scale_x = scale_y = scale
        if np.random.rand() < self.stretch_prob:
            scale_x *= 2 ** np.random.uniform(-self.max_stretch, self.max_stretch)
            scale_y *= 2 ** np.random.uniform(-self.max_stretch, self.max_stretch)
        scale_x = np.clip(scale_x, min_scale, None)
        scale_y = np.clip(scale_y, min_scale, None)
        resized = np.random.rand() < self.spatial_aug_prob
        rh, rw = (int(round(ht * scale_y)), int(round(wd * scale_x))) if resized else (ht, wd)      # resize_linear's output size
        hflip = vflip = False
        if self.do_flip:
            hflip = np.random.rand() < self.h_flip_prob
            vflip = np.random.rand() < self.v_flip_prob
        y0 = np.random.randint(0, rh - self.crop_size[0])
        x0 = np.random.randint(0, rw - self.crop_size[1])
        return AugPlan(rh, rw, crop=self.crop_size, y0=y0, x0=x0, hflip=hflip, vflip=vflip, resized=resized, scale_x=scale_x, scale_y=scale_y)

    def __call__(self, img1, img2, flow, without_resize=False):
        if without_resize:
            img1, img2, flow = self.spatial_transform_no_resize(img1, img2, flow)
        else:
            img1, img2, flow = self.spatial_transform(img1, img2, flow)
        return np.ascontiguousarray(img1), np.ascontiguousarray(img2), np.ascontiguousarray(flow)


class DenseSparseAugmentor:
    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=False):
        self.crop_size = crop_size
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.do_flip = do_flip
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1

    def spatial_transform(self, img1, img2, dimg1, dimg2, flow):
        if self.do_flip:                                           # :389-403
            if np.random.rand() < self.h_flip_prob:
                img1, img2, dimg1, dimg2 = img1[:, ::-1], img2[:, ::-1], dimg1[:, ::-1], dimg2[:, ::-1]
                flow = flow[:, ::-1] * [-1.0, 1.0]
            if np.random.rand() < self.v_flip_prob:
                img1, img2, dimg1, dimg2 = img1[::-1, :], img2[::-1, :], dimg1[::-1, :], dimg2[::-1, :]
                flow = flow[::-1, :] * [1.0, -1.0]
        ch, cw = self.crop_size                                    # :405-419
        y0 = 0 if img1.shape[0] == ch else np.random.randint(0, img1.shape[0] - ch)
        x0 = 0 if img1.shape[1] == cw else np.random.randint(0, img1.shape[1] - cw)
        sl = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        return img1[sl], img2[sl], dimg1[sl], dimg2[sl], flow[sl]

    def draw(self, ht, wd):
        """The random draws of __call__ for an ht x wd sample as an AugPlan (no crop draw along an axis the crop already fills);
        `apply_host(plan, img1, img2, dimg1, dimg2, flow)` is then __call__'s result."""
        hflip = vflip = False
        if self.do_flip:
            hflip = np.random.rand() < self.h_flip_prob
            vflip = np.random.rand() < self.v_flip_prob
        ch, cw = self.crop_size
        y0 = 0 if ht == ch else np.random.randint(0, ht - ch)
        x0 = 0 if wd == cw else np.random.randint(0, wd - cw)
        return AugPlan(ht, wd, crop=(ch, cw), y0=y0, x0=x0, hflip=hflip, vflip=vflip)

    def __call__(self, img1, img2, dimg1, dimg2, flow):
        out = self.spatial_transform(img1, img2, dimg1, dimg2, flow)
        return tuple(np.ascontiguousarray(a) for a in out)
