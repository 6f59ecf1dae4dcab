"""Raw MVSEC sequences scored on the GPU: ground-truth flow for ANY window (eemflow_gt_flow_many, csrc/gt_prop.hip), and the raw
arrays of a sequence as a resident recording.

The reference evaluates MVSEC through files that loader/MVSEC_encoder.py writes first - `event/%06d.h5` and `flowgt_dt{1,4}/%d.npy` -
propagating the ground truth with per-frame cv2.remap calls on the CPU (estimate_corresponding_gt_flow / prop_flow,
loader/loader_utils.py:70-161) for two window lengths.  Here the 20 Hz ground-truth stack goes to the device once and the target of
any window [t0, t1] is one job of a launch:

    gt = MvsecGroundTruth(flow_dist, flow_dist_ts, device)            the (T,2,H,W) stack, uploaded once in pinned chunks
    flows = gt.flow_many(starts, ends)                                (n,2,H,W) fp32, 32 windows per launch, no synchronisation
    raw = MvsecRaw(events, image_raw_ts, image_raw_event_inds, gt)    MVSEC's (N,4) [x, y, t, p] events as an EventRecording
    offsets, t_edges = raw.frame_windows(first, last, dt=1)           host only
    for item in harness.run_recording(model, raw.recording, offsets, gt=gt, t_edges=t_edges, crop=(256, 256)): ...

`plan` is the host part (NumPy float64): the reference's searchsorted(side='right') - 1, its `gt_dt > dt` test and its three scale
factors.  The kernel walks every pixel through the frames of the plan; the arithmetic is stated at eemflow_gt_flow_many in
include/eemflow_hip.h and restated in tests/gt_prop_reference.py.  Differences from the reference, all deliberate:
  * the short branch (`gt_dt > dt`) returns float64 there; here it is rounded to fp32 once, like every other target;
  * where the reference raises IndexError or silently misbehaves - a start before the first timestamp (it indexes [-1]), a window
    that needs a frame beyond the last, end < start - `plan` raises ValueError;
  * a non-finite ground-truth value stays non-finite in the output (cv2's conversion of a NaN coordinate is undefined).
cv2 is not installed where this was built: the nearest-neighbour rounding (half to even, cvRound) and the zero border
(BORDER_CONSTANT) follow OpenCV's documentation and were not checked against a cv2 run.
"""
import ctypes

import numpy as np
import torch

from . import _lib, events
from .recording import EventRecording, _check_offsets, _check_spans, _windows_of

MAX_JOBS_PER_CALL = 32                                             # GT_MAX_JOBS
UPLOAD_CHUNK_BYTES = 64 << 20


def plan_window(ts, start, end):
    """(frame0, nsteps, a, b) of the window [start, end] on the float64 timestamps ts: loader_utils.py:102-111 (nsteps == 0: a = dt,
    b = gt_dt) and :125-152 (nsteps >= 2: a, b the scale of the first and of the last step).  Host only."""
    start, end = np.float64(start), np.float64(end)
    if not (np.isfinite(start) and np.isfinite(end)):
        raise ValueError(f"MvsecGroundTruth.plan: the window [{start}, {end}] is not finite")
    if end < start:
        raise ValueError(f"MvsecGroundTruth.plan: end {end} < start {start}")
    n = ts.shape[0]
    gt_iter = int(np.searchsorted(ts, start, side='right')) - 1
    if gt_iter < 0:
        raise ValueError(f"MvsecGroundTruth.plan: the window starts at {start}, before the first ground-truth timestamp {ts[0]} "
                         "(the reference would index the last frame)")
    if gt_iter + 1 >= n:
        raise ValueError(f"MvsecGroundTruth.plan: the window starts at {start}, in or after the last ground-truth interval: it needs a "
                         f"frame beyond the last ({n} timestamps)")
    gt_dt = ts[gt_iter + 1] - ts[gt_iter]
    dt = end - start
    if gt_dt > dt:                                                  # no need to propagate
        return gt_iter, 0, float(dt), float(gt_dt)
    frame0 = gt_iter
    a = (ts[gt_iter + 1] - start) / gt_dt
    gt_iter += 1
    while True:
        if gt_iter + 1 >= n:
            raise ValueError(f"MvsecGroundTruth.plan: the window ends at {end}: it needs a frame beyond the last ground-truth "
                             f"timestamp {ts[-1]}")
        if not ts[gt_iter + 1] < end:
            break
        gt_iter += 1
    final_dt = end - ts[gt_iter]
    final_gt_dt = ts[gt_iter + 1] - ts[gt_iter]
    return frame0, gt_iter - frame0 + 1, float(a), float(final_dt / final_gt_dt)


class MvsecGroundTruth:
    """The ground-truth stack of one MVSEC sequence, resident on `device`.  flow_dist: (T,2,H,W), read as float32 (as
    MVSEC_encoder.py:133 reads it; an h5py dataset or a memory-mapped array is sliced chunk by chunk); flow_dist_ts: (T,) strictly
    increasing, kept as float64 on the host.  frames=(lo, hi): upload frames lo..hi-1 only - plans still use all timestamps, and a
    window whose frames leave the uploaded range is refused."""

    def __init__(self, flow_dist, flow_dist_ts, device="cuda:0", frames=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.EEMFlowHipError("MvsecGroundTruth: the stack lives on a GPU - there is no CPU path")
        ts = np.ascontiguousarray(np.asarray(flow_dist_ts, dtype=np.float64))
        shape = tuple(int(v) for v in flow_dist.shape)
        if len(shape) != 4 or shape[1] != 2 or shape[0] < 1 or shape[2] < 1 or shape[3] < 1:
            raise ValueError(f"MvsecGroundTruth: flow_dist is (T,2,H,W), got {shape}")
        if ts.ndim != 1 or ts.shape[0] != shape[0]:
            raise ValueError(f"MvsecGroundTruth: {shape[0]} frames need as many timestamps, got {ts.shape}")
        if not bool(np.all(np.isfinite(ts))) or not bool(np.all(ts[1:] > ts[:-1])):
            raise ValueError("MvsecGroundTruth: flow_dist_ts must be finite and strictly increasing")
        lo, hi = (0, shape[0]) if frames is None else (int(frames[0]), int(frames[1]))
        if not 0 <= lo < hi <= shape[0]:
            raise ValueError(f"MvsecGroundTruth: frames=({lo}, {hi}) is not a range inside the stack's {shape[0]} frames")
        self.ts, self.frames = ts, (lo, hi)
        self.height, self.width = shape[2], shape[3]
        frame_bytes = 2 * self.height * self.width * 4
        per = max(1, min(hi - lo, UPLOAD_CHUNK_BYTES // frame_bytes))
        with torch.cuda.device(self.device):
            self.stack = torch.empty(hi - lo, 2, self.height, self.width, dtype=torch.float32, device=self.device)
            stage = torch.empty(per, 2, self.height, self.width, dtype=torch.float32, pin_memory=True)
            done = torch.cuda.Event()
            for f0 in range(lo, hi, per):
                k = min(per, hi - f0)
                np.copyto(stage.numpy()[:k], np.asarray(flow_dist[f0:f0 + k], dtype=np.float32))
                self.stack[f0 - lo:f0 - lo + k].copy_(stage[:k], non_blocking=True)
                done.record(torch.cuda.current_stream(self.device))
                done.synchronize()                                  # the staging buffer is reused by the next chunk

    @classmethod
    def from_npz(cls, path, device="cuda:0", frames=None):
        """The stack of an npz with the arrays flow_dist (T,2,H,W) and flow_dist_ts (T,)."""
        with np.load(path) as f:
            return cls(f["flow_dist"], f["flow_dist_ts"], device=device, frames=frames)

    @classmethod
    def from_hdf5(cls, path, device="cuda:0", frames=None, camera="left"):
        """The stack of MVSEC's `*_gt.hdf5` (davis/<camera>/flow_dist, flow_dist_ts), read chunk by chunk.  UNTESTED: h5py is not
        installed where this was written; the import is made here so that nothing else depends on it."""
        import h5py
        with h5py.File(path, 'r') as f:
            group = f['davis'][camera]
            return cls(group['flow_dist'], np.float64(group['flow_dist_ts']), device=device, frames=frames)

    def __len__(self):
        return self.ts.shape[0]

    # ------------------------------------------------------------------ host
    def plan(self, start, end):
        """(frame0, nsteps, a, b) of the window [start, end] (plan_window; frame0 counts from the sequence's first frame).  ValueError for
        a start before the first timestamp, a window that needs a frame beyond the last, and end < start.  Host only."""
        return plan_window(self.ts, start, end)

    def _resident(self, pl, start, end):
        frame0, nsteps = pl[0], pl[1]
        lo, hi = self.frames
        if frame0 < lo or frame0 + max(nsteps, 1) > hi:
            raise ValueError(f"MvsecGroundTruth: the window [{start}, {end}] reads frames {frame0}..{frame0 + max(nsteps, 1) - 1}; "
                             f"frames {lo}..{hi - 1} are resident")
        return frame0 - lo

    # ------------------------------------------------------------------ device
    def flow_many(self, starts, ends, out=None):
        """The ground-truth displacement over each window [starts[i], ends[i]]: an (n,2,H,W) fp32 tensor on the device (or `out`: such a
        tensor, or a list of n contiguous (2,H,W) fp32 device tensors, which is returned).  Any number of windows, 32 per launch, planned
        on the host first (a refused window launches nothing).  Stream-ordered, no synchronisation."""
        starts = np.atleast_1d(np.asarray(starts, dtype=np.float64))
        ends = np.atleast_1d(np.asarray(ends, dtype=np.float64))
        n = starts.shape[0]
        if starts.ndim != 1 or ends.shape != starts.shape or n < 1:
            raise ValueError("MvsecGroundTruth.flow_many: as many ends as starts, at least one window")
        plans = [self.plan(s, e) for s, e in zip(starts, ends)]
        firsts = [self._resident(pl, s, e) for pl, s, e in zip(plans, starts, ends)]
        h, w, dev = self.height, self.width, self.device
        if out is None:
            out = torch.empty(n, 2, h, w, dtype=torch.float32, device=dev)
        outs = list(out)
        if len(outs) != n or any((not torch.is_tensor(o)) or o.device != dev or o.dtype != torch.float32 or tuple(o.shape) != (2, h, w)
                                 or not o.is_contiguous() for o in outs):
            raise ValueError(f"MvsecGroundTruth.flow_many: out is {n} contiguous (2,{h},{w}) float32 tensors on {dev}")
        with torch.no_grad(), torch.cuda.device(dev):
            for i0 in range(0, n, MAX_JOBS_PER_CALL):
                k = min(MAX_JOBS_PER_CALL, n - i0)
                part = plans[i0:i0 + k]
                _lib.check(_lib.lib().eemflow_gt_flow_many(
                    k, self.stack.data_ptr(), self.stack.shape[0], h, w, (ctypes.c_int * k)(*firsts[i0:i0 + k]),
                    (ctypes.c_int * k)(*[p[1] for p in part]), (ctypes.c_double * k)(*[p[2] for p in part]),
                    (ctypes.c_double * k)(*[p[3] for p in part]), (ctypes.c_void_p * k)(*[o.data_ptr() for o in outs[i0:i0 + k]]),
                    _lib.current_stream_ptr(dev)))
        return out

    def flow(self, start, end):
        """The (2,H,W) fp32 displacement over [start, end]."""
        return self.flow_many([start], [end])[0]


def estimate_corresponding_gt_flow(x_flow_in, y_flow_in, gt_timestamps, start_time, end_time, device="cuda:0"):
    """The reference's call (loader_utils.py:94): (x_shift, y_shift), two (H,W) fp32 tensors on the device.  Uploads the whole stack for
    one window - for more than one, keep a MvsecGroundTruth."""
    stack = np.stack([np.asarray(x_flow_in, dtype=np.float32), np.asarray(y_flow_in, dtype=np.float32)], axis=1)
    out = MvsecGroundTruth(stack, gt_timestamps, device=device).flow(float(start_time), float(end_time))
    return out[0], out[1]


def event_mask_windows(recording, offsets=None, out=None, spans=None):
    """The event masks of the windows [offsets[k], offsets[k+1]) of a resident recording: a (K,H,W) fp32 tensor of 0 / 1, mask k
    `mvsec.event_mask` of window k's events (eemflow_event_mask_windows).  32 windows per call, no synchronisation.  Instead of
    offsets, spans=: a (K, 2) array of [start, end) event indices in any order (eemflow_event_mask_spans).  Exactly one of the two."""
    if not isinstance(recording, EventRecording):
        raise TypeError("event_mask_windows: recording is an EventRecording")
    offs, span_list = _windows_of("event_mask_windows", offsets, spans, recording.n)
    k_all, h, w, dev = len(span_list), recording.height, recording.width, recording.device
    if k_all < 1:
        raise ValueError("event_mask_windows: offsets are K + 1 >= 2 event indices" if offs is not None else
                         "event_mask_windows: spans are K >= 1 windows")
    if out is None:
        out = torch.empty(k_all, h, w, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (k_all, h, w) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"event_mask_windows: out is a contiguous ({k_all},{h},{w}) float32 tensor on {dev}")
    with torch.no_grad(), torch.cuda.device(dev):
        xy = (ctypes.c_void_p(recording.column_ptr(1)), ctypes.c_void_p(recording.column_ptr(2)), recording.codes[1], recording.codes[2])
        for i0 in range(0, k_all, MAX_JOBS_PER_CALL):
            part = span_list[i0:i0 + MAX_JOBS_PER_CALL]
            k = len(part)
            ptrs = (ctypes.c_void_p * k)(*[out[i0 + i].data_ptr() for i in range(k)])
            if offs is None:
                _lib.check(_lib.lib().eemflow_event_mask_spans(k, *xy, (ctypes.c_int64 * k)(*[a for a, _ in part]),
                                                               (ctypes.c_int64 * k)(*[b for _, b in part]), h, w, ptrs,
                                                               _lib.current_stream_ptr(dev)))
            else:
                _lib.check(_lib.lib().eemflow_event_mask_windows(k, *xy, (ctypes.c_int64 * (k + 1))(*offs[i0:i0 + k + 1]), h, w, ptrs,
                                                                 _lib.current_stream_ptr(dev)))
    return out


class MvsecRaw:
    """One raw MVSEC sequence: events (N,4) [x, y, t seconds, p = +-1] (davis/left/events), image_raw_ts and image_raw_event_inds of the
    grey frames, and its MvsecGroundTruth.  The events become an EventRecording - x, y uint16, p int8, t float64 with scale_a = 1.0 and
    scale_b = 1e6, so a window's timestamps are (t * 1.0) * 1e6, the dataset route's `t * 1e6` (EventSequence's timestamp multiplier)."""

    def __init__(self, events, image_raw_ts, image_raw_event_inds, gt, height=260, width=346, device="cuda:0"):
        ev = np.asarray(events)
        if ev.ndim != 2 or ev.shape[1] != 4 or ev.shape[0] < 1:
            raise ValueError(f"MvsecRaw: events is (N,4) [x, y, t, p], got {ev.shape}")
        if gt is not None and (gt.height, gt.width) != (int(height), int(width)):
            raise ValueError(f"MvsecRaw: the ground truth is {gt.height} x {gt.width}, the sensor {height} x {width}")
        x, y, p = ev[:, 0], ev[:, 1], ev[:, 3]
        if x.min() < 0 or y.min() < 0 or x.max() > 65535 or y.max() > 65535 or np.any(x != np.floor(x)) or np.any(y != np.floor(y)):
            raise ValueError("MvsecRaw: event coordinates are non-negative integers")
        if np.any(np.abs(p) != 1):
            raise ValueError("MvsecRaw: polarities are +1 / -1")
        self.image_raw_ts = np.ascontiguousarray(np.asarray(image_raw_ts, dtype=np.float64))
        self.image_raw_event_inds = np.asarray(image_raw_event_inds).astype(np.int64)
        if self.image_raw_ts.ndim != 1 or self.image_raw_event_inds.shape != self.image_raw_ts.shape:
            raise ValueError("MvsecRaw: image_raw_ts and image_raw_event_inds are 1-d arrays of one length")
        self.gt = gt
        self.recording = EventRecording(np.ascontiguousarray(ev[:, 2], dtype=np.float64), x.astype(np.uint16), y.astype(np.uint16),
                                        p.astype(np.int8), height, width, device=device, scale_a=1.0, scale_b=1e6)
        if self.recording.route != 'device':
            raise ValueError("MvsecRaw: the events are not in time order - image_raw_event_inds would not index the sorted recording")

    @classmethod
    def from_npz(cls, data_npz, gt_npz, height=260, width=346, device="cuda:0"):
        """data_npz: the arrays events, image_raw_ts, image_raw_event_inds; gt_npz: flow_dist, flow_dist_ts."""
        gt = MvsecGroundTruth.from_npz(gt_npz, device=device)
        with np.load(data_npz) as f:
            return cls(f["events"], f["image_raw_ts"], f["image_raw_event_inds"], gt, height=height, width=width, device=device)

    def frame_windows(self, first, last, dt=1):
        """frame_windows(image_raw_ts, image_raw_event_inds, first, last, dt) checked against this sequence's events."""
        offsets, t_edges = frame_windows(self.image_raw_ts, self.image_raw_event_inds, first, last, dt)
        _check_offsets("MvsecRaw.frame_windows", offsets, self.recording.n)
        return offsets, t_edges

    def frame_spans(self, first, last, dt=1, stride=None, reference_pairs=False):
        """frame_spans(image_raw_ts, image_raw_event_inds, first, last, dt, stride, reference_pairs) checked against this sequence's
        events."""
        spans, t_spans, lag = frame_spans(self.image_raw_ts, self.image_raw_event_inds, first, last, dt, stride=stride,
                                          reference_pairs=reference_pairs)
        _check_spans("MvsecRaw.frame_spans", spans, self.recording.n)
        return spans, t_spans, lag


def frame_spans(image_raw_ts, image_raw_event_inds, first, last, dt=1, stride=None, reference_pairs=False):
    """Windows of dt grey frames that start every `stride` frames, and the pairs to run on them: (spans, t_spans, lag).  Window m starts
    at grey frame f_m = first + m*stride and is the events [inds[f_m], inds[f_m + dt]) (an index < 0 counts as 0): spans is (K, 2) int64.
    Pair m is windows (m, m + lag), its ground truth covers [t_spans[m, 0], t_spans[m, 1]] (t_spans: (P, 2) float64), K = P + lag:
      stride = None or dt    lag 1, P = (last - first) // dt + 1: the windows and edges of frame_windows - consecutive windows;
      stride dividing dt     lag = dt // stride, P = (last - first) // stride + 1: pair m compares window m with the window that starts
                             where it ends, t_spans[m] = (ts[f_m], ts[f_m + dt]) - a flow over dt frames every `stride` frames;
      reference_pairs        stride is 1, lag 1, P = last - first + 1: pair m compares window m with the window ONE frame later and its
                             ground truth covers (ts[first + m], ts[first + m + dt]).  For dt = 4 these are exactly the samples
                             first..last of MvsecEventFlow_dt4 (loader/MVSEC.py:201-283: files i+1..i+4 against i+2..i+5, flowgt_dt4/i.npy),
                             for dt = 1 those of MvsecEventFlow.
    Refused: a stride that does not divide dt, frames beyond the sequence, descending indices.  Host only."""
    ts = np.asarray(image_raw_ts, dtype=np.float64)
    inds = np.asarray(image_raw_event_inds).astype(np.int64)
    first, last, dt = int(first), int(last), int(dt)
    if dt < 1:
        raise ValueError(f"frame_spans: dt is a positive number of frames, got {dt}")
    if first < 0 or last < first:
        raise ValueError(f"frame_spans: 0 <= first <= last, got {first}, {last}")
    if reference_pairs:
        if stride is not None and int(stride) != 1:
            raise ValueError(f"frame_spans: reference_pairs slide by one frame; got stride={stride}")
        stride, lag = 1, 1
    else:
        stride = dt if stride is None else int(stride)
        if stride < 1 or dt % stride != 0:
            raise ValueError(f"frame_spans: the stride must divide dt={dt}, got {stride}")
        lag = dt // stride
    pairs = (last - first) // stride + 1
    f = first + stride * np.arange(pairs + lag)
    if f[-1] + dt >= inds.shape[0]:
        raise ValueError(f"frame_spans: pairs {first}..{last} at dt={dt}, stride={stride} need grey frame {int(f[-1] + dt)}; the sequence "
                         f"has {inds.shape[0]}")
    spans = np.stack([np.maximum(inds[f], 0), np.maximum(inds[f + dt], 0)], axis=1).astype(np.int64)
    if np.any(spans[:, 1] < spans[:, 0]) or np.any(spans[1:] < spans[:-1]):
        raise ValueError("frame_spans: image_raw_event_inds does not ascend over these frames")
    t_spans = np.ascontiguousarray(np.stack([ts[f[:pairs]], ts[f[:pairs] + dt]], axis=1))
    return spans, t_spans, lag


def frame_windows(image_raw_ts, image_raw_event_inds, first, last, dt=1):
    """The windows of the pairs first, first + dt, ..., <= last, cut on the grey frames: (offsets, t_edges), K + 1 event indices and K + 1
    timestamps for K = P + 1 windows of P = (last - first) // dt + 1 pairs.  Window m is the events
    [inds[first + m*dt], inds[first + (m+1)*dt]) - the slices MVSEC_encoder.py's generate_fimage writes (file i holds
    [inds[i-1], inds[i+dt-1]); an index < 0 counts as 0) - and edge m is image_raw_ts[first + m*dt]; pair m runs from window m to
    window m + 1 and its ground truth covers [t_edges[m], t_edges[m+1]].  With dt = 1 these are exactly the samples first..last of
    MvsecEventFlow (sample i: event files i + 1 and i + 2, flowgt_dt1/i.npy over [ts[i], ts[i+1]]).
    With dt > 1 the windows are CONSECUTIVE: pair m compares frames [first + m*dt, first + (m+1)*dt) with the dt frames after them.
    MvsecEventFlow_dt4 pairs windows that OVERLAP by three frames (sample i: files i+1..i+4 against i+2..i+5, flowgt_dt4/i.npy over
    [ts[i], ts[i+4]]): that is another protocol, and these windows do not reproduce it.  `frame_spans(..., dt=4, reference_pairs=True)`
    does, sample for sample; frame_spans also gives windows that slide by less than dt.  Host only."""
    ts = np.asarray(image_raw_ts, dtype=np.float64)
    inds = np.asarray(image_raw_event_inds).astype(np.int64)
    first, last, dt = int(first), int(last), int(dt)
    if dt < 1:
        raise ValueError(f"frame_windows: dt is a positive number of frames, got {dt}")
    if first < 0 or last < first:
        raise ValueError(f"frame_windows: 0 <= first <= last, got {first}, {last}")
    pairs = (last - first) // dt + 1
    idx = first + dt * np.arange(pairs + 2)
    if idx[-1] >= inds.shape[0]:
        raise ValueError(f"frame_windows: pairs {first}..{last} at dt={dt} need grey frame {int(idx[-1])}; the sequence has {inds.shape[0]}")
    offsets = np.maximum(inds[idx], 0).astype(np.int64)
    if np.any(offsets[1:] < offsets[:-1]):
        raise ValueError("frame_windows: image_raw_event_inds does not ascend over these frames")
    return offsets, np.ascontiguousarray(ts[idx])
