"""One long event recording on the GPU, cut into windows and voxelized straight from its columns (eemflow_voxelize_windows,
csrc/voxel_cols.hip).

A recording is the four columns of an HREM-style events npz (t, x, y, p) in their file dtypes - 13 B per event for int64 / uint16 /
uint16 / one byte.  It is uploaded ONCE, as it is; every window of it is then a pair of host integers:

    rec = EventRecording.from_npz(path, height, width)         one pinned staging copy, one asynchronous upload
    offsets = rec.window_offsets(window=50_000_000)            np.searchsorted on the raw host t column: no device work
    grids = voxelize_windows(rec, offsets, num_bins=5)         32 windows per launch sequence, no host memory touched, no synchronisation
    tables = rec.tables(offsets)                               the windows' (N,4) float64 tables for fwl_many / rsat_many / event_image

Windows need not be consecutive.  SPANS are a (K, 2) int64 host array of [start, end) event indices, in any order: they may overlap,
nest, repeat or be empty (eemflow_voxelize_spans: the same kernels, every job's first element and length travel separately anyway):

    spans = rec.sliding_spans(window=40_000_000, stride=10_000_000)    40 ms windows every 10 ms
    grids = voxelize_windows(rec, spans=spans, num_bins=5)     each window voxelized once, as if it were a recording of its own

The binning kernel reads the raw columns and forms each event's scaled, window-relative float64 timestamp in registers - what
events.pack_events_many writes into a table for voxelizer.voxelize_many_device to read again - so every grid is bitwise what that
composition gives for the same slice, without the 64 B per event of table traffic.  Each window's time scale runs from its own first
to its own last event, as if the reference had been handed the slice.

Route rule (events.route_of): a recording whose RAW t column is non-decreasing goes up as it is; any other is put in order on the host
first by ONE stable argsort of the whole recording (counted under events.route_counts['host']).  A t column of float32 / float16 is
refused: NumPy would scale it in the column's own precision, which the kernel does not reproduce - convert it to float64.

An EMPTY window is allowed (a pause of the sensor inside a recording cut by duration): its grid is all zeros and its deferred record
{0, 1, 0, 0} - the reference cannot be asked about one, it indexes events[-1].
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, events
from .voxelizer import _grid_buffers, _norm_code

MAX_WINDOWS_PER_CALL = 32                                          # VOX_MAX_JOBS


def _check_offsets(who, offsets, n):
    """Window edges as a list of host integers: ascending (equal neighbours: an empty window) inside [0, n]."""
    offs = [int(o) for o in (offsets.tolist() if isinstance(offsets, np.ndarray) else offsets)]
    if len(offs) < 1:
        raise ValueError(f"{who}: offsets are K + 1 >= 1 event indices")
    if offs[0] < 0 or offs[-1] > n or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError(f"{who}: the offsets must ascend inside the recording's {n} events")
    return offs


def _check_spans(who, spans, n):
    """Spans as a list of (start, end) host integers, 0 <= start <= end <= n each; no ordering between spans."""
    arr = np.asarray(spans)
    if arr.size == 0:
        arr = arr.reshape(0, 2)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype.kind not in 'iu':
        raise ValueError(f"{who}: spans are a (K, 2) integer array of [start, end) event indices")
    out = [(int(a), int(b)) for a, b in arr.tolist()]
    if any(a < 0 or b < a or b > n for a, b in out):
        raise ValueError(f"{who}: every span is 0 <= start <= end inside the recording's {n} events")
    return out


def _windows_of(who, offsets, spans, n):
    """Exactly one of offsets (K + 1 ascending edges) and spans ((K, 2)) -> (offsets as a list or None, the (start, end) list)."""
    if (offsets is None) == (spans is None):
        raise ValueError(f"{who}: give exactly one of offsets and spans=")
    if spans is not None:
        return None, _check_spans(who, spans, n)
    offs = _check_offsets(who, offsets, n)
    return offs, list(zip(offs, offs[1:]))


def _edges_for(t, edges):
    """Timestamps to search the raw t column for.  An integer column is searched with integers (t >= e is t >= ceil(e)): a float64
    comparison would round nanosecond timestamps beyond 2^53."""
    if t.dtype.kind in 'iub':
        return np.array([int(e) if isinstance(e, (int, np.integer)) else int(math.ceil(float(e))) for e in edges], dtype=np.int64)
    return np.asarray(edges, dtype=np.float64)


def order_columns(t, x, y, p):
    """The checked columns of a recording in time order -> ((t, x, y, p), route).  route 'device': the raw t column was non-decreasing
    and the columns are returned as they came; 'host': ONE stable argsort of t reordered all four (events of one timestamp keep their
    order).  Host only."""
    cols = tuple(np.asarray(c) for c in (t, x, y, p))
    n = cols[0].shape[0] if cols[0].ndim == 1 else -1
    if n < 1 or any(c.ndim != 1 or c.shape[0] != n for c in cols):
        raise ValueError("EventRecording: t, x, y, p are 1-d columns of one length, at least one event")
    for name, c in zip("txyp", cols):
        if c.dtype not in events.DTYPE_CODES:
            raise TypeError(f"EventRecording: column {name} has dtype {c.dtype}; the kernels read {sorted(str(d) for d in events.DTYPE_CODES)}")
    if cols[0].dtype.kind == 'f' and cols[0].dtype != np.float64:
        raise TypeError(f"EventRecording: a {cols[0].dtype} t column is scaled by NumPy in its own precision; convert it to float64")
    route = events.route_of(cols)
    if route == 'host':
        order = np.argsort(cols[0], kind='stable')
        cols = tuple(np.ascontiguousarray(c[order]) for c in cols)
    return cols, route


class EventRecording:
    """The columns of one recording, resident on `device` in their file dtypes; `t_host` keeps the raw (ordered) t column for cutting.
    t, x, y, p: 1-d numpy arrays of one length, of the dtypes of events.DTYPE_CODES (t: an integer type or float64), p already 2*p - 1
    as events.read_event_columns gives it.  scale_a, scale_b: the two factors of the reference's timestamp ((t * scale_a) * scale_b:
    get_compressed_events' 1e-9, then EventSequence's timestamp multiplier)."""

    def __init__(self, t, x, y, p, height, width, device="cuda:0", scale_a=1e-9, scale_b=1e6):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.EEMFlowHipError("EventRecording: a recording lives on a GPU - there is no CPU path")
        if int(height) < 1 or int(width) < 1:
            raise ValueError(f"EventRecording: bad sensor size {height} x {width}")
        cols, self.route = order_columns(t, x, y, p)
        n = cols[0].shape[0]
        events._count(self.route, 1, None)
        self.t_host = np.ascontiguousarray(cols[0])
        self.n = n
        self.height, self.width = int(height), int(width)
        self.scale_a, self.scale_b = float(scale_a), float(scale_b)
        self.dtypes = tuple(c.dtype for c in cols)
        self.codes = tuple(events.DTYPE_CODES[d] for d in self.dtypes)
        (self._col_offsets,), total = events.staging_layout([cols])
        with torch.cuda.device(self.device):
            stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            events._fill_stage(stage.numpy(), [cols], [self._col_offsets])
            self._bytes = torch.empty(total, dtype=torch.uint8, device=self.device)
            self._bytes.copy_(stage, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            done.synchronize()                                     # the staging buffer goes away with this call

    @classmethod
    def from_npz(cls, path, height, width, device="cuda:0", scale_a=1e-9, scale_b=1e6):
        """The recording of an HREM-style events npz (arrays t, x, y, p)."""
        return cls(*events.read_event_columns(path), height, width, device=device, scale_a=scale_a, scale_b=scale_b)

    def __len__(self):
        return self.n

    def column_ptr(self, c, first=0):
        """Device address of element `first` of column c (0..3: t, x, y, p)."""
        return self._bytes.data_ptr() + self._col_offsets[c] + int(first) * self.dtypes[c].itemsize

    # ------------------------------------------------------------------ cutting (host only)
    def window_offsets(self, window=None, count=None, t_edges=None, keep_partial=False):
        """Window edges as K + 1 host int64 event indices, window k = events [offsets[k], offsets[k+1]).  Exactly one of
          window   a duration in the units of the raw t column: the edges are t[0] + k * window, searched with side 'left' - window k
                   holds edge_k <= t < edge_{k+1}, an event ON an edge belongs to the later window, a window without events is empty.
                   floor((t[-1] - t[0]) / window) full windows; what follows the last edge (the last event at least) is the trailing
                   partial window: dropped, or with keep_partial one more window up to the recording's end;
          count    events per window; the trailing n % count events are dropped, or kept as one more window with keep_partial;
          t_edges  K + 1 explicit timestamps, ascending (side 'left' as above; keep_partial does not apply).
        np.searchsorted on the raw host column: no device work."""
        return window_offsets(self.t_host, window=window, count=count, t_edges=t_edges, keep_partial=keep_partial)

    def sliding_spans(self, window=None, stride=None, count=None, stride_count=None):
        """Windows that slide by less (or more) than their length, as a (K, 2) host int64 array of [start, end) event indices.  Either
          window, stride        durations in the units of the raw t column: window m is t[0] + m*stride <= t < t[0] + m*stride + window,
                                both edges searched with side 'left' as window_offsets does (an event ON an edge belongs to the window
                                that starts there, a window without events is empty).  Only full windows: the last one ends at or
                                before t[-1].  With stride == window these are zip(offs, offs[1:]) of window_offsets(window=);
          count, stride_count   events per window and events between two starts; only full windows.
        np.searchsorted on the raw host column: no device work."""
        return sliding_spans(self.t_host, window=window, stride=stride, count=count, stride_count=stride_count)

    # ------------------------------------------------------------------ the windows' float64 tables
    def tables(self, offsets=None, relative=True, spans=None):
        """The (N_k,4) float64 CUDA tables [t, x, y, p] of the windows - what fwl_many / rsat_many / event_image take - bitwise what
        events.pack_events_many gives for the slices: eemflow_pack_events_many on views of the resident columns, 32 windows per launch,
        no staging, no synchronisation.  Exactly one of offsets (K + 1 ascending edges) and spans ((K, 2) [start, end), any order)."""
        _, spans = _windows_of("EventRecording.tables", offsets, spans, self.n)
        with torch.no_grad(), torch.cuda.device(self.device):
            outs = [torch.empty(b - a, 4, dtype=torch.float64, device=self.device) for a, b in spans]
            for i0 in range(0, len(spans), events.PACK_MAX):
                part, k = spans[i0:i0 + events.PACK_MAX], len(spans[i0:i0 + events.PACK_MAX])
                ptr = ctypes.c_void_p * k
                cols = [ptr(*[self.column_ptr(c, a) for a, _ in part]) for c in range(4)]
                _lib.check(_lib.lib().eemflow_pack_events_many(
                    k, cols[0], cols[1], cols[2], cols[3], (ctypes.c_int * (4 * k))(*(list(self.codes) * k)),
                    (ctypes.c_int64 * k)(*[b - a for a, b in part]), self.scale_a, self.scale_b, 1 if relative else 0,
                    ptr(*[o.data_ptr() if o.shape[0] else None for o in outs[i0:i0 + k]]), _lib.current_stream_ptr(self.device)))
        return outs


def window_offsets(t, window=None, count=None, t_edges=None, keep_partial=False):
    """EventRecording.window_offsets on a raw, ordered host t column."""
    if sum(v is not None for v in (window, count, t_edges)) != 1:
        raise ValueError("window_offsets: give exactly one of window=, count= and t_edges=")
    t = np.asarray(t)
    n = t.shape[0]
    if t.ndim != 1 or n < 1:
        raise ValueError("window_offsets: t is a 1-d column with at least one event")
    if count is not None:
        if int(count) != count or int(count) < 1:
            raise ValueError(f"window_offsets: count is a positive number of events, got {count!r}")
        offs = list(range(0, n + 1, int(count)))
        if keep_partial and offs[-1] < n:
            offs.append(n)
        return np.asarray(offs, dtype=np.int64)
    if window is not None:
        if not window > 0:
            raise ValueError(f"window_offsets: window is a positive duration in the units of t, got {window!r}")
        integral = t.dtype.kind in 'iub'
        t0, t1 = (int(t[0]), int(t[-1])) if integral else (float(t[0]), float(t[-1]))
        full = int((t1 - t0) // window)
        edges = [t0 + (k * window if not integral or isinstance(window, (int, np.integer)) else int(math.ceil(k * window))) for k in range(full + 1)]
        offs = np.searchsorted(t, _edges_for(t, edges), side='left').astype(np.int64)
        if keep_partial:
            offs = np.append(offs, np.int64(n))
        return offs
    edges = list(t_edges.tolist() if isinstance(t_edges, np.ndarray) else t_edges)
    if len(edges) < 1 or any(b < a for a, b in zip(edges, edges[1:])):
        raise ValueError("window_offsets: t_edges are K + 1 ascending timestamps")
    return np.searchsorted(t, _edges_for(t, edges), side='left').astype(np.int64)


def sliding_spans(t, window=None, stride=None, count=None, stride_count=None):
    """EventRecording.sliding_spans on a raw, ordered host t column."""
    by_time, by_count = window is not None or stride is not None, count is not None or stride_count is not None
    if by_time == by_count or (by_time and (window is None or stride is None)) or (by_count and (count is None or stride_count is None)):
        raise ValueError("sliding_spans: give window= and stride=, or count= and stride_count=")
    t = np.asarray(t)
    n = t.shape[0] if t.ndim == 1 else 0
    if n < 1:
        raise ValueError("sliding_spans: t is a 1-d column with at least one event")
    if by_count:
        if int(count) != count or int(count) < 1 or int(stride_count) != stride_count or int(stride_count) < 1:
            raise ValueError(f"sliding_spans: count and stride_count are positive numbers of events, got {count!r} and {stride_count!r}")
        starts = np.arange(0, n - int(count) + 1, int(stride_count), dtype=np.int64)
        return np.stack([starts, starts + int(count)], axis=1).reshape(-1, 2)
    if not window > 0 or not stride > 0:
        raise ValueError(f"sliding_spans: window and stride are positive durations in the units of t, got {window!r} and {stride!r}")
    integral = t.dtype.kind in 'iub'
    t0, t1 = (int(t[0]), int(t[-1])) if integral else (float(t[0]), float(t[-1]))

    def edge(m, extra):                                                # window_offsets' own edge arithmetic: exact integers where it can be
        d = m * stride + extra
        return t0 + (d if not integral or isinstance(d, (int, np.integer)) else int(math.ceil(d)))

    # a window of q whole strides ends ON the start edge of window m + q - the same number, so neighbours at that lag share the edge
    # (and stride == window gives window_offsets' edges t0 + k * window); any other window ends at t0 + m*stride + window
    q = int(window // stride)
    whole = q >= 1 and q * stride == window

    def end_edge(m):
        return edge(m + q, 0) if whole else edge(m, window)

    if t1 - t0 < window:
        return np.zeros((0, 2), dtype=np.int64)
    full = int((t1 - t0 - window) // stride) + 2                       # the last full window ends at or before t[-1]
    while full > 0 and end_edge(full - 1) > t1:                        # (a float quotient may round past the last full window)
        full -= 1
    starts = np.searchsorted(t, _edges_for(t, [edge(m, 0) for m in range(full)]), side='left').astype(np.int64)
    ends = np.searchsorted(t, _edges_for(t, [end_edge(m) for m in range(full)]), side='left').astype(np.int64)
    return np.stack([starts, ends], axis=1).reshape(-1, 2)


def voxelize_windows(recording, offsets=None, num_bins=None, normalize=True, relative=True, spans=None):
    """The K windows [offsets[k], offsets[k+1]) of a resident recording as a list of K [1, num_bins, H, W] fp32 tensors in time order -
    what forward_stream takes - each bitwise `voxelize_many_device(pack_events_many([slice]))` of its slice.  Any number of windows, 32
    per launch sequence; normalize: True, False or "deferred" (raw grids with their record behind them, `voxelizer.norm_record`);
    relative: the window's timestamps start at 0, as EventSequence(convert_to_relative=True) leaves them.  An empty window gives an
    all-zero grid (deferred record {0, 1, 0, 0}).  No host memory touched, no synchronisation.
    Instead of offsets, spans=: a (K, 2) array of [start, end) event indices in any order - overlapping, nested, repeated or empty
    windows, the list in the spans' order (eemflow_voxelize_spans).  Exactly one of the two."""
    if not isinstance(recording, EventRecording):
        raise TypeError("voxelize_windows: recording is an EventRecording")
    offs, span_list = _windows_of("voxelize_windows", offsets, spans, recording.n)
    if num_bins is None:
        raise TypeError("voxelize_windows: num_bins is required")
    code = _norm_code(normalize)
    num_bins = int(num_bins)
    if num_bins < 1:
        raise ValueError(f"voxelize_windows: num_bins must be positive, got {num_bins}")
    dev, h, w = recording.device, recording.height, recording.width
    out = []
    with torch.no_grad(), torch.cuda.device(dev):
        cols = [ctypes.c_void_p(recording.column_ptr(c)) for c in range(4)]
        codes = (ctypes.c_int * 4)(*recording.codes)
        for i0 in range(0, len(span_list), MAX_WINDOWS_PER_CALL):
            part = span_list[i0:i0 + MAX_WINDOWS_PER_CALL]
            k = len(part)
            grids = _grid_buffers(k, num_bins, h, w, dev, code == 2)
            ptrs = (ctypes.c_void_p * k)(*[g.data_ptr() for g in grids])
            if offs is None:
                _lib.check(_lib.lib().eemflow_voxelize_spans(
                    k, cols[0], cols[1], cols[2], cols[3], codes, (ctypes.c_int64 * k)(*[a for a, _ in part]),
                    (ctypes.c_int64 * k)(*[b for _, b in part]), recording.scale_a, recording.scale_b, 1 if relative else 0, num_bins, h, w, code,
                    ptrs, _lib.current_stream_ptr(dev)))
            else:
                _lib.check(_lib.lib().eemflow_voxelize_windows(
                    k, cols[0], cols[1], cols[2], cols[3], codes, (ctypes.c_int64 * (k + 1))(*offs[i0:i0 + k + 1]), recording.scale_a,
                    recording.scale_b, 1 if relative else 0, num_bins, h, w, code, ptrs, _lib.current_stream_ptr(dev)))
            out.extend(g[None] for g in grids)
    return out
