"""The DSEC trilinear voxel grid (reference: utils/dsec_utils.py:19-64, VoxelGrid.convert) restated in NumPy, operation by operation in
fp32, with the contract of eemflow_voxelize_trilinear_many for what the reference leaves undefined:

    dT  = t[n-1] - t[0];  tn = ((float)(C-1) * (t_i - t[0])) / dT
    x0  = (int)x_i, y0 = (int)y_i, b0 = (int)tn          truncation toward zero
    val = 2 p_i - 1
    for xl in (x0, x0+1), yl in (y0, y0+1), bl in (b0, b0+1), kept iff 0 <= xl < W, 0 <= yl < H, 0 <= bl < C:
        grid[bl, yl, xl] += ((val * (1 - |float(xl) - x_i|)) * (1 - |float(yl) - y_i|)) * (1 - |float(bl) - tn|)

An event whose x, y or tn is not finite or not below 2^31 in magnitude is dropped whole (dT == 0: every event).  `votes` gives the
eight votes per event, `exact` the correctly rounded sum (math.fsum) of every occupied cell, `check_*` the criteria the tests hold
grids to.  The `fault` argument of `votes` plants the mistakes the checks are shown to reject (tests/test_dsec_host.py); nothing else
uses it."""
import math

import numpy as np

LIM = np.float32(2.0 ** 31)
FAULTS = ("floor", "wrap_x", "order", "drop_eighth")


def votes(x, y, t, p, C, H, W, fault=None):
    """(idx [8][n] int64 flat indices bl*H*W + yl*W + xl, w [8][n] fp32 weights, mask [8][n] bool); corner order x0/x0+1 outermost,
    then y, then bin - the reference's loop order."""
    assert fault is None or fault in FAULTS
    x, y, t, p = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, y, t, p))
    one = np.float32(1)
    with np.errstate(all="ignore"):
        dT = t[-1] - t[0]
        tn = (np.float32(C - 1) * (t - t[0])) / dT
        ok = (np.abs(x) < LIM) & (np.abs(y) < LIM) & (np.abs(tn) < LIM)          # False for NaN and inf
        cut = np.floor if fault == "floor" else np.trunc
        xs, ys, ts = (np.where(ok, a, np.float32(0)) for a in (x, y, tn))
        x0, y0, b0 = (cut(a).astype(np.int64) for a in (xs, ys, ts))
        val = np.float32(2) * p - one
        idx, wgt, mask = [], [], []
        for xl in (x0, x0 + 1):
            for yl in (y0, y0 + 1):
                for bl in (b0, b0 + 1):
                    m = ok & (yl < H) & (yl >= 0) & (bl >= 0) & (bl < C)
                    m &= (xl >= 0) & ((xl <= W) if fault == "wrap_x" else (xl < W))          # wrap_x: xl == W lands in the next row
                    wx = one - np.abs(xl.astype(np.float32) - xs)
                    wy = one - np.abs(yl.astype(np.float32) - ys)
                    wt = one - np.abs(bl.astype(np.float32) - ts)
                    w = (val * wx) * (wy * wt) if fault == "order" else ((val * wx) * wy) * wt      # (val = +-1: only the other two products round)
                    flat = H * W * bl + W * yl + xl
                    m &= (flat >= 0) & (flat < C * H * W)
                    idx.append(flat)
                    wgt.append(w.astype(np.float32))
                    mask.append(m)
        if fault == "drop_eighth":
            mask[7] = np.zeros_like(mask[7])
    return np.stack(idx), np.stack(wgt), np.stack(mask)


def exact(x, y, t, p, C, H, W, fault=None):
    """Per occupied cell, ascending: `cells` (flat index), `sum` (the exact sum of its votes, correctly rounded to fp64 by math.fsum),
    `abs` (sum |w|), `count` (votes k); `total` = C*H*W."""
    idx, w, m = votes(x, y, t, p, C, H, W, fault)
    c, v = idx[m], w[m].astype(np.float64)
    order = np.argsort(c, kind="stable")
    c, v = c[order], v[order]
    cells, start, count = np.unique(c, return_index=True, return_counts=True)
    s = np.array([math.fsum(v[a:a + k]) for a, k in zip(start, count)], dtype=np.float64).reshape(-1)
    ab = np.add.reduceat(np.abs(v), start) if len(start) else np.zeros(0)
    return {"cells": cells, "sum": s + 0.0, "abs": ab, "count": count, "total": C * H * W}      # (+ 0.0: a grid starts at +0.0)


def dense(E, dtype=np.float64):
    out = np.zeros(E["total"], dtype=dtype)
    out[E["cells"]] = E["sum"]
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rest_is_zero(name, got, E):
    rest = np.ones(E["total"], dtype=bool)
    rest[E["cells"]] = False
    stray = int(np.count_nonzero(_bits(got)[rest]))
    assert stray == 0, f"{name}: {stray} cells that received no vote are not +0.0"


def check_sequential(name, got, E):
    """A grid summed in fp32 in SOME order (the reference's put_): |got - exact| <= (k - 1) 2^-24 sum|w| per occupied cell, the bound of
    k - 1 roundings of partial sums that never exceed sum|w|; every other cell exactly +0.0.  Returns the worst share of the bound."""
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    assert got.size == E["total"]
    g = got[E["cells"]].astype(np.float64)
    bound = (E["count"] - 1) * 2.0 ** -24 * E["abs"]
    err = np.abs(g - E["sum"])
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {len(g)} occupied cells are outside (k-1) 2^-24 sum|w|; the first at flat index "
                                 f"{int(E['cells'][bad][0])}: got {g[bad][0]!r}, exact {E['sum'][bad][0]!r}")
    _rest_is_zero(name, got, E)
    return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0


TIE_SHARE = 1e-3


def check_rounded_once(name, got, E):
    """The GPU's contract: every occupied cell is bitwise fp32(exact sum).  An fp64 accumulation of k votes is off the exact sum by at
    most k 2^-53 sum|w|; only where the exact sum lies that close to a rounding tie - the midpoint of two neighbouring fp32 values - may
    the cell be either of the two, and a case may use that on TIE_SHARE of its occupied cells at most.  (The cap counts the cells that
    TAKE the exception, not the cells at a tie: the sum of two fp32 votes of neighbouring exponents has 25 significant bits half of the
    time, so exact ties are a few per cent of the two-vote cells of any input - there the fp64 sum is exact too and rounds to even like
    fp32(exact), which is why no cell of a correct grid needs the exception.)  Every other cell is +0.0.
    Returns (cells that differ from fp32(exact), cells near a tie)."""
    got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    assert got.size == E["total"]
    g, s = got[E["cells"]], E["sum"]
    r32 = s.astype(np.float32)
    differ = _bits(g) != _bits(r32)
    below = r32.astype(np.float64) <= s                       # the exact sum lies between r32 and its neighbour on this side
    other = np.where(below, np.nextafter(r32, np.float32(np.inf)), np.nextafter(r32, np.float32(-np.inf)))
    mid = (r32.astype(np.float64) + other.astype(np.float64)) / 2
    near = np.abs(s - mid) <= E["count"] * 2.0 ** -53 * E["abs"]
    excused = differ & near & (_bits(g) == _bits(other))
    bad = differ & ~excused
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {len(s)} occupied cells are not their exact sum rounded once; the first at flat "
                                 f"index {int(E['cells'][bad][0])} ({int(E['count'][bad][0])} votes): got {float(g[bad][0])!r}, exact "
                                 f"{float(s[bad][0])!r}")
    assert int(excused.sum()) <= TIE_SHARE * len(s), f"{name}: {int(excused.sum())} of {len(s)} occupied cells took the other side of a tie"
    _rest_is_zero(name, got, E)
    return int(differ.sum()), int(near.sum())


def normalised_f64(raw):
    """loader_utils.py:527-535 / dsec_utils.py:54-62 in fp64 on a raw grid: (v - mean) / sd over the non-zero voxels (unbiased sd; the
    mean alone unless sd > 0)."""
    v = np.asarray(raw, dtype=np.float64)
    nz = v != 0
    out = v.copy()
    if nz.any():
        m = v[nz].mean()
        sd = v[nz].std(ddof=1) if nz.sum() > 1 else float("nan")
        out[nz] = (v[nz] - m) / sd if sd > 0 else v[nz] - m
    return out


def flow_16bit_to_float(flow_16bit):
    """dsec_utils.py:66-83."""
    assert flow_16bit.dtype == np.uint16 and flow_16bit.ndim == 3 and flow_16bit.shape[2] == 3
    valid = flow_16bit[..., 2] == 1
    assert np.all(flow_16bit[~valid, -1] == 0)
    f = flow_16bit.astype("float")
    flow = np.zeros(flow_16bit.shape[:2] + (2,))
    flow[valid] = (f[valid][:, :2] - 2 ** 15) / 128
    return flow, valid
