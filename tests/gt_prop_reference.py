"""NumPy restatement of the MVSEC ground-truth propagation (eemflow_gt_flow_many, csrc/gt_prop.hip): estimate_corresponding_gt_flow /
prop_flow of the reference (loader/loader_utils.py:70-161), written fresh - the plan in float64, the walk vectorised over the pixels.

    plan(ts, start, end)                 -> (frame0, nsteps, a, b)        the host part; ValueError where the reference raises IndexError
    walk(stack, frame0, nsteps, a, b)    -> (2,H,W) float32               what the kernel writes
    short64(stack, frame0, a, b)         -> (2,H,W) float64               the short branch before its one fp32 rounding
    gt_flow(stack, ts, start, end)       -> walk(stack, *plan(...))

`fault=` plants one deliberate mistake in the walk (tests/test_gt_prop_host.py: each must change a cell of a golden case).
cv2 is not installed: nearest-neighbour rounding (half to even, cvRound) and the zero border (BORDER_CONSTANT) rest on OpenCV's
documented behaviour."""
import numpy as np

FAULTS = ("half_up", "joint_mask", "fp32_product", "clamped_border", "bilinear", "skip_scale0")


def plan(ts, start, end):
    ts = np.asarray(ts, dtype=np.float64)
    start, end = np.float64(start), np.float64(end)
    if end < start:
        raise ValueError("end < start")
    it = int(np.searchsorted(ts, start, side='right')) - 1
    if it < 0:
        raise ValueError("the window starts before the first ground-truth timestamp")
    if it + 1 >= ts.shape[0]:
        raise ValueError("the window needs a frame beyond the last")
    gt_dt = ts[it + 1] - ts[it]
    dt = end - start
    if gt_dt > dt:
        return it, 0, float(dt), float(gt_dt)
    a = (ts[it + 1] - start) / gt_dt
    frame0 = it
    it += 1
    while True:
        if it + 1 >= ts.shape[0]:
            raise ValueError("the window needs a frame beyond the last")
        if not ts[it + 1] < end:
            break
        it += 1
    b = (end - ts[it]) / (ts[it + 1] - ts[it])
    return frame0, it - frame0 + 1, float(a), float(b)


def nearest(img, x, y, fault=None):
    """cv2.remap(img, x, y, INTER_NEAREST) with the default constant border 0, on float32 maps x, y; a non-finite position finds no cell."""
    h, w = img.shape
    fin = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(fin, x, 0).astype(np.float64), np.where(fin, y, 0).astype(np.float64)
    if fault == "bilinear":
        x0, y0 = np.floor(xs), np.floor(ys)
        out = np.zeros(x.shape, dtype=np.float64)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            wx = (xs - x0) if dx else 1.0 - (xs - x0)
            wy = (ys - y0) if dy else 1.0 - (ys - y0)
            xi, yi = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            out += np.where(ok, img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], 0.0) * wx * wy
        return np.where(fin, out, 0.0)
    rx, ry = (np.floor(xs + 0.5), np.floor(ys + 0.5)) if fault == "half_up" else (np.rint(xs), np.rint(ys))
    inside = fin & (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
    xi, yi = np.clip(rx, 0, w - 1).astype(np.int64), np.clip(ry, 0, h - 1).astype(np.int64)
    val = img[yi, xi].astype(np.float64)
    if fault == "clamped_border":
        return np.where(fin, val, 0.0)
    return np.where(inside, val, 0.0)


def short64(stack, frame0, a, b):
    return stack[frame0].astype(np.float64) * np.float64(a) / np.float64(b)


def walk(stack, frame0, nsteps, a, b, fault=None, visited=None):
    """stack: (T,2,H,W) float32.  visited: a list that receives every step's (x, y) float32 position arrays before the step."""
    stack = np.asarray(stack)
    assert stack.dtype == np.float32 and stack.ndim == 4 and stack.shape[1] == 2
    if nsteps == 0:
        return short64(stack, frame0, a, b).astype(np.float32)
    assert nsteps >= 2 and frame0 + nsteps <= stack.shape[0]
    h, w = stack.shape[2:]
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x0, y0 = x0.astype(np.float32), y0.astype(np.float32)
    x, y = x0.copy(), y0.copy()
    mx, my = np.ones((h, w), dtype=bool), np.ones((h, w), dtype=bool)
    for s in range(nsteps):
        scale = np.float64(a if s == 0 else (b if s == nsteps - 1 else 1.0))
        if fault == "skip_scale0" and scale == 0.0:
            continue
        if visited is not None:
            visited.append((x.copy(), y.copy()))
        fu = nearest(stack[frame0 + s, 0], x, y, fault)
        fv = nearest(stack[frame0 + s, 1], x, y, fault)
        # a read of 0 clears the mask of a component whose own coordinate is finite; a non-finite component keeps its value (no NaN
        # or infinity becomes a number - cv2's integer conversion of such a coordinate is undefined)
        cx, cy = (fu == 0) & np.isfinite(x), (fv == 0) & np.isfinite(y)
        if fault == "joint_mask":
            cx = cy = cx | cy
        mx &= ~cx
        my &= ~cy
        with np.errstate(invalid="ignore", over="ignore"):
            if fault == "fp32_product":
                x = (x.astype(np.float64) + (fu * scale).astype(np.float32)).astype(np.float32)
                y = (y.astype(np.float64) + (fv * scale).astype(np.float32)).astype(np.float32)
            else:
                x = (x.astype(np.float64) + fu * scale).astype(np.float32)
                y = (y.astype(np.float64) + fv * scale).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.stack([np.where(mx, x - x0, np.float32(0)), np.where(my, y - y0, np.float32(0))]).astype(np.float32)


def gt_flow(stack, ts, start, end, fault=None):
    return walk(stack, *plan(ts, start, end), fault=fault)


def generate_fimage_slices(inds, dt):
    """The event slices loader/MVSEC_encoder.py's generate_fimage writes, restated literally: file i holds events
    [inds[i - 1] (0 where that is negative), inds[i + dt - 1])."""
    out = {}
    for i in range(len(inds) - (dt - 1)):
        lo = 0 if inds[i - 1] < 0 else int(inds[i - 1])
        out[i] = (lo, int(inds[i + (dt - 1)]))
    return out
