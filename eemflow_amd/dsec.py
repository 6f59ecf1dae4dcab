"""E-RAFT's DSEC input stage on the GPU (reference: utils/dsec_utils.py).

`VoxelGrid(input_size, normalize).convert(events)` keeps the reference's constructor and call: `events` is a dict of the columns
'x', 'y', 't', 'p' - here float32 CUDA tensors - and the result the (C,H,W) fp32 grid with EIGHT trilinear votes per event that
E-RAFT's published weights were trained on (sub-pixel x and y; `EventSequenceToVoxelGrid_Pytorch` of this package is the other,
MVSEC / HREM representation: integer pixels, two votes).  The voting and the normalisation run in libeemflow_hip.so
(eemflow_voxelize_trilinear_many, csrc/voxel_tri.hip); there is no CPU path: without a GPU this raises.

What the kernel reproduces of the reference, and where it decides what the reference leaves open (include/eemflow_hip.h has the
arithmetic): `.int()` truncates toward zero, so x = -0.5 votes +0.5 into column 0 and -0.5 into column 1; corners at x == W, y == H and
bin == C are masked, nothing wraps; only t[0] and t[-1] set the time scale, the events need not be sorted; with t[-1] == t[0] (one
event included) every vote is dropped and the grid is all zeros; an event with a non-finite or huge (>= 2^31) x, y or scaled t is
dropped whole.  A cell is the fp64 sum of its votes rounded to fp32 once (the reference: fp32 in put_'s order).

`voxel_grid_many` voxelizes up to 32 sets in one launch sequence, `voxelize_windows` the consecutive windows of one device-resident
stream (the form `ERAFT.forward_stream` takes), both optionally with DSEC's rectification lookup fused into the read of raw sensor
coordinates.  `flow_16bit_to_float` / `flow_float_to_16bit` are DSEC's 16-bit flow encoding on the device.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_SETS_PER_CALL = 32
_XY_CODE = {torch.float32: 0, torch.int16: 1, torch.int32: 2}
_COLUMNS = ("x", "y", "t", "p")


def _check_set(who, ev, rectified):
    """The four columns of one event set as 1-d contiguous CUDA tensors of one length >= 1 on one device; returns (x, y, t, p)."""
    try:
        cols = tuple(ev[k] for k in _COLUMNS)
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"{who}: an event set is a dict of the columns 'x', 'y', 't', 'p'") from None
    for k, c in zip(_COLUMNS, cols):
        if not isinstance(c, torch.Tensor) or not c.is_cuda:
            raise _lib.EEMFlowHipError(f"{who}: column {k!r} must be a CUDA tensor - the voxelizer has no CPU path here")
        if c.dim() != 1 or not c.is_contiguous():
            raise ValueError(f"{who}: column {k!r} must be 1-d and contiguous")
    x, y, t, p = cols
    if t.dtype != torch.float32 or p.dtype != torch.float32:
        raise TypeError(f"{who}: 't' and 'p' must be float32 (the reference raises on float64 too), got {t.dtype}, {p.dtype}")
    want = (torch.int16, torch.int32) if rectified else (torch.float32,)
    if x.dtype not in want or y.dtype != x.dtype:
        raise TypeError(f"{who}: 'x' and 'y' must both be " + ("int16 or int32 raw coordinates (rectify_maps given)" if rectified else "float32")
                        + f", got {x.dtype}, {y.dtype}")
    n = t.shape[0]
    if n < 1:
        raise ValueError(f"{who}: an empty event set (the reference indexes t[-1])")
    if any(c.shape[0] != n for c in cols):
        raise ValueError(f"{who}: the columns have different lengths: " + ", ".join(str(c.shape[0]) for c in cols))
    if any(c.device != t.device for c in cols):
        raise ValueError(f"{who}: the columns lie on different devices")
    return cols


def _check_maps(who, maps, k, dev):
    maps = [maps] * k if isinstance(maps, torch.Tensor) else list(maps)
    if len(maps) != k:
        raise ValueError(f"{who}: one rectification map per event set (or one tensor for all), got {len(maps)} for {k}")
    for m in maps:
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.device == dev and m.dtype == torch.float32 and m.dim() == 3 and m.shape[2] == 2
                and m.is_contiguous() and tuple(m.shape) == tuple(maps[0].shape)):
            raise ValueError(f"{who}: rectify_maps are contiguous (Hmap,Wmap,2) float32 CUDA tensors of one shape on the events' device")
    return maps


def _launch(who, sets, input_size, normalize, rectify_maps, out):
    """sets: [(x, y, t, p)] already checked; one launch sequence per 32 of them.  Returns the list of (C,H,W) grids."""
    if len(input_size) != 3:
        raise ValueError(f"{who}: input_size is (C, H, W)")
    C, H, W = (int(v) for v in input_size)
    k = len(sets)
    dev = sets[0][2].device
    if any(s[2].device != dev for s in sets):
        raise ValueError(f"{who}: the event sets lie on different devices")
    maps = _check_maps(who, rectify_maps, k, dev) if rectify_maps is not None else None
    with torch.no_grad(), torch.cuda.device(dev):
        grids = list(out) if out is not None else list(torch.empty(k, C, H, W, dtype=torch.float32, device=dev).unbind(0))
        if len(grids) != k or any(not isinstance(g, torch.Tensor) or tuple(g.shape) != (C, H, W) or g.dtype != torch.float32 or not g.is_contiguous()
                                  or g.device != dev for g in grids):
            raise ValueError(f"{who}: out must be one contiguous (C,H,W) fp32 tensor per event set, on the events' device")
        for a in range(0, k, MAX_SETS_PER_CALL):
            part = sets[a:a + MAX_SETS_PER_CALL]
            m = len(part)
            ptr = ctypes.c_void_p * m
            col = [ptr(*[s[j].data_ptr() for s in part]) for j in range(4)]
            mp = ptr(*[t.data_ptr() for t in maps[a:a + m]]) if maps is not None else None
            _lib.check(_lib.lib().eemflow_voxelize_trilinear_many(
                m, col[0], col[1], col[2], col[3], (ctypes.c_int64 * m)(*[s[2].shape[0] for s in part]), _XY_CODE[part[0][0].dtype], mp,
                maps[0].shape[0] if maps is not None else 0, maps[0].shape[1] if maps is not None else 0, C, H, W, 1 if normalize else 0,
                ptr(*[g.data_ptr() for g in grids[a:a + m]]), _lib.current_stream_ptr(dev)))
    return grids


class VoxelGrid(object):
    """utils/dsec_utils.py:19-64 with the reference's constructor and call; `convert` makes no host copy and does not synchronise."""

    def __init__(self, input_size, normalize):
        assert len(input_size) == 3
        self.input_size = tuple(int(v) for v in input_size)
        self.nb_channels = self.input_size[0]
        self.normalize = normalize

    def convert(self, events):
        return _launch("VoxelGrid.convert", [_check_set("VoxelGrid.convert", events, False)], self.input_size, self.normalize, None, None)[0]


def voxel_grid_many(event_sets, input_size, normalize=True, rectify_maps=None, out=None):
    """Up to 32 event sets of one grid shape in ONE launch sequence: a list of column dicts -> a list of (C,H,W) fp32 tensors (`out`: the
    tensors to fill), each bitwise what `VoxelGrid.convert` gives for that set alone.  rectify_maps (one (Hmap,Wmap,2) float32 tensor,
    or one per set): 'x' and 'y' are then RAW int16 / int32 sensor coordinates and the kernel looks (x', y') = map[y, x] up as it
    reads them (DSEC's rectification, without the round trip of the rectified columns); an event whose raw coordinate lies outside
    the map is dropped.  All sets of a call share the coordinate dtype."""
    event_sets = list(event_sets)
    if not 1 <= len(event_sets) <= MAX_SETS_PER_CALL:
        raise ValueError(f"voxel_grid_many: 1..{MAX_SETS_PER_CALL} event sets per call, got {len(event_sets)}")
    sets = [_check_set("voxel_grid_many", ev, rectify_maps is not None) for ev in event_sets]
    if any(s[0].dtype != sets[0][0].dtype for s in sets):
        raise TypeError("voxel_grid_many: the sets of a call share one coordinate dtype")
    return _launch("voxel_grid_many", sets, input_size, normalize, rectify_maps, out)


def voxelize_windows(events, input_size, t_edges=None, offsets=None, normalize=True, rectify_map=None):
    """The K consecutive windows of ONE long device-resident event stream (a column dict, time-sorted) as K grids: window k holds the
    events [offsets[k], offsets[k+1]), every window's columns are views into the stream's (nothing is copied), and up to 32 windows
    share a launch sequence.  Give the K + 1 window edges as
      offsets: K + 1 host integers (ascending event indices) - costs no synchronisation; or
      t_edges: K + 1 timestamps (a sequence or tensor, in the units of events['t']) - ONE torch.searchsorted on the device (side
               'left': window k is t_edges[k] <= t < t_edges[k+1]) and ONE small device-to-host read of the K + 1 indices, which
               waits for the stream.
    Every window needs at least one event.  Each window's time scale runs from its own first to its own last event, as if the reference
    had been handed the slice.  Returns a list of K [1,C,H,W] fp32 tensors (views of one allocation) in time order - what
    `ERAFT.forward_stream` takes."""
    if (t_edges is None) == (offsets is None):
        raise ValueError("voxelize_windows: give either t_edges or offsets")
    x, y, t, p = _check_set("voxelize_windows", events, rectify_map is not None)
    if offsets is None:
        edges = torch.as_tensor(t_edges, dtype=torch.float32).to(t.device)
        if edges.dim() != 1:
            raise ValueError("voxelize_windows: t_edges is a 1-d sequence of K + 1 timestamps")
        offsets = torch.searchsorted(t, edges).tolist()                 # the one synchronising read
    offsets = [int(o) for o in offsets]
    if len(offsets) < 2:
        raise ValueError("voxelize_windows: K + 1 >= 2 window edges")
    if offsets[0] < 0 or offsets[-1] > t.shape[0] or any(b <= a for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"voxelize_windows: the edges must ascend inside the stream with at least one event per window, got offsets {offsets}")
    sets = [(x[a:b], y[a:b], t[a:b], p[a:b]) for a, b in zip(offsets, offsets[1:])]
    C, H, W = (int(v) for v in input_size)
    buf = torch.empty(len(sets), 1, C, H, W, dtype=torch.float32, device=t.device)
    _launch("voxelize_windows", sets, input_size, normalize, rectify_map, [b[0] for b in buf.unbind(0)])
    return list(buf.unbind(0))


def flow_16bit_to_float(flow_16bit):
    """utils/dsec_utils.py:66-83 on the device: an (H,W,3) integer tensor with values in [0, 65535] - or a NumPy uint16 array, which is
    uploaded - -> ((H,W,2) float64 flow = (v - 2^15) / 128 on the valid pixels, 0 elsewhere; (H,W) bool valid = channel 2 == 1).  The
    reference's assertions raise ValueError (the check of channel 2 reads one flag back)."""
    if isinstance(flow_16bit, np.ndarray):
        if flow_16bit.dtype != np.uint16:
            raise ValueError(f"flow_16bit_to_float: a NumPy input must be uint16, got {flow_16bit.dtype}")
        if not torch.cuda.is_available():
            raise _lib.EEMFlowHipError("flow_16bit_to_float: no GPU")
        flow_16bit = torch.from_numpy(flow_16bit.astype(np.int32)).cuda()
    if not isinstance(flow_16bit, torch.Tensor) or flow_16bit.is_floating_point() or flow_16bit.dtype == torch.bool:
        raise ValueError("flow_16bit_to_float: an integer tensor or a NumPy uint16 array")
    if not flow_16bit.is_cuda:
        raise _lib.EEMFlowHipError("flow_16bit_to_float: the tensor must live on the GPU")
    if flow_16bit.dim() != 3 or flow_16bit.shape[2] != 3:
        raise ValueError(f"flow_16bit_to_float: expected (H,W,3), got {tuple(flow_16bit.shape)}")
    v = flow_16bit.to(torch.int64)
    valid = v[..., 2] == 1
    if bool(((v[..., 2] != 0) & ~valid).any()) or bool(((v < 0) | (v > 65535)).any()):
        raise ValueError("flow_16bit_to_float: channel 2 must be 0 or 1 and every value a 16-bit one")
    flow = (v[..., :2].to(torch.float64) - 2 ** 15) / 128
    return torch.where(valid[..., None], flow, torch.zeros_like(flow)), valid


def flow_float_to_16bit(flow, valid):
    """The inverse - DSEC's submission encoding: (H,W,2) flow and (H,W) bool valid on the device -> (H,W,3) int32 with
    rint(flow * 128 + 2^15) clamped to [0, 65535] in channels 0 and 1 and 1 in channel 2 on the valid pixels, all zero elsewhere (int32
    holds the 16-bit range; `.cpu().numpy().astype(np.uint16)` is what a PNG writer takes).  Exact for multiples of 1/128 in
    [-256, 256 - 1/128]."""
    if not (isinstance(flow, torch.Tensor) and isinstance(valid, torch.Tensor) and flow.is_cuda and valid.is_cuda):
        raise _lib.EEMFlowHipError("flow_float_to_16bit: flow and valid must be CUDA tensors")
    if flow.dim() != 3 or flow.shape[2] != 2 or not flow.is_floating_point() or tuple(valid.shape) != tuple(flow.shape[:2]) or valid.dtype != torch.bool:
        raise ValueError("flow_float_to_16bit: expected an (H,W,2) floating-point flow and an (H,W) bool mask")
    q = torch.round(flow.to(torch.float64) * 128 + 2 ** 15).clamp_(0, 65535).to(torch.int32)       # torch.round: half to even, as rint
    out = torch.cat([q, torch.ones_like(q[..., :1])], dim=2)
    return torch.where(valid[..., None], out, torch.zeros_like(out))
