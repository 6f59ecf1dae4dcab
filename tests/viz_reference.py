"""CPU restatement of the two visualisations the evaluation loop writes (tests/golden/viz.npz pins it to the reference's own output):

flow_image(flow)      tensor_tools.flow_to_image_dmax (utils_luo/tools.py:2385-2523) for a float32 flow: the Middlebury colour wheel,
                      normalised by the frame's maximum radius.  The maximum is fp32; from the division by maxrad + 2^-52 on, everything
                      is fp64.  |u| or |v| > 1e7 is unknown: zero for the maximum, black in the image.  A NaN in the frame makes the
                      maximum -1 (Python's max(-1, nan)); NaN pixels are black.
event_image(volume)   Test.vis_map_RGB (test_mvsec.py:175-233) up to the array it writes: white, red where the channel sum is at most
                      mean - 0.2, blue where it is at least mean + 0.2.
"""
import numpy as np

NCOLS = 55
UNKNOWN = np.float32(1e7)


def color_wheel():
    """(55, 3) integers: six ramps RY 15, YG 6, GC 4, CB 11, BM 13, MR 6."""
    rows = []
    for n, fixed, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True)):
        for i in range(n):
            c = [0, 0, 0]
            c[fixed] = 255
            c[ramp] = 255 - (255 * i) // n if down else (255 * i) // n
            rows.append(c)
    return np.array(rows, dtype=np.float64)


def flow_divisor(flow):
    """The frame's divisor (float64): fp32 maximum radius (unknown pixels zero; -1 when a NaN is present) + 2^-52."""
    u, v = flow_components(flow)[:2]
    rad = np.sqrt(u * u + v * v)                                  # fp32
    top = np.max(rad)
    maxrad = np.float64(-1.0) if not top > -1 else np.float64(top)
    return maxrad + np.float64(2.0 ** -52)


def flow_components(flow):
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[0] == 2, "flow: (2,H,W) float32"
    u, v = flow[0].copy(), flow[1].copy()
    unknown = (np.abs(u) > UNKNOWN) | (np.abs(v) > UNKNOWN)
    u[unknown] = 0
    v[unknown] = 0
    return u, v, unknown


def flow_image(flow, bgr=False, angle_dtype=np.float64):
    """(2,H,W) float32 -> (H,W,3) uint8.  angle_dtype=np.float32 takes the angle alone in fp32: the size of the disagreement a kernel
    with a less exact arctangent may show (test_viz_host measures it)."""
    u32, v32, unknown = flow_components(flow)
    d = flow_divisor(flow)
    with np.errstate(invalid="ignore"):
        u = u32.astype(np.float64) / d
        v = v32.astype(np.float64) / d
        nan = np.isnan(u) | np.isnan(v)
        u[nan] = 0
        v[nan] = 0
        rad = np.sqrt(u * u + v * v)
        a = (np.arctan2((-v).astype(angle_dtype), (-u).astype(angle_dtype)).astype(np.float64)) / np.pi
        fk = (a + 1) / 2 * (NCOLS - 1) + 1
        k0 = np.floor(fk).astype(np.int64)
        k1 = np.where(k0 + 1 == NCOLS + 1, 1, k0 + 1)
        f = fk - k0
        wheel = color_wheel() / 255
        img = np.zeros(u.shape + (3,), dtype=np.uint8)
        near = rad <= 1
        for ch in range(3):
            col = (1 - f) * wheel[k0 - 1, ch] + f * wheel[k1 - 1, ch]
            col = np.where(near, 1 - rad * (1 - col), col * 0.75)
            img[..., ch] = np.floor(255 * col).astype(np.int64).astype(np.uint8)
    img[nan | unknown] = 0
    return img[..., ::-1].copy() if bgr else img


def normalise_raw(volume, record):
    """A raw voxel grid and its record {mean, sd, scale, any} -> the volume the first convolution sees: non-zero voxels become
    (x - mean) * (1 / sd) in fp32 (x - mean where scale is 0), nothing changes where any is 0."""
    volume = np.asarray(volume, dtype=np.float32)
    mean, sd, scale, any_ = (np.float32(x) for x in record)
    if any_ == 0:
        return volume.copy()
    inv = np.float32(1) / sd if scale != 0 else np.float32(1)
    return np.where(volume != 0, (volume - mean) * inv, volume).astype(np.float32)


def event_sum(volume):
    volume = np.asarray(volume, dtype=np.float32)
    s = volume[0].copy()
    for c in range(1, volume.shape[0]):
        s = s + volume[c]                                            # fp32, channel order
    return s


def event_image(volume, record=None, bgr=False):
    """(bins,H,W) float32 -> ((H,W,3) uint8, count of pixels whose sum exceeds 0.1).  The density is count / (H*W)."""
    if record is not None:
        volume = normalise_raw(volume, record)
    s = event_sum(volume)
    count = int(np.sum(s > np.float32(0.1)))
    mean = np.float32(np.mean(s.astype(np.float64)))                # fp64 mean, rounded once
    img = np.full(s.shape + (3,), 255, dtype=np.uint8)
    img[s <= mean - np.float32(0.2)] = (255, 0, 0)
    img[s >= mean + np.float32(0.2)] = (0, 0, 255)
    return (img[..., ::-1].copy() if bgr else img), count


def event_threshold_margin(volume, record=None):
    """Smallest distance of a pixel's sum from either threshold and from 0.1: summation order cannot decide a pixel above ~1e-5."""
    if record is not None:
        volume = normalise_raw(volume, record)
    s = event_sum(volume).astype(np.float64)
    mean = s.mean()
    return float(min(np.abs(s - (mean - 0.2)).min(), np.abs(s - (mean + 0.2)).min(), np.abs(s - 0.1).min()))
