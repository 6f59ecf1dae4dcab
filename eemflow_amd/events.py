"""Event sets prepared on the GPU from the columns of their npz (eemflow_pack_events_many, csrc/event_pack.hip).

The reference builds every event set on the host: get_compressed_events (loader/loader_utils.py:26-37) fills an (N,4) float64 table,
32 B per event, from columns that hold 13 B per event (t int64, x and y uint16, p one byte), EventSequence.__init__ (:352-397)
checks the order, scales the timestamps and subtracts the start, and the voxelizer's front-end copies the table once more
(astype('float')) before it uploads it from pageable memory.  Here the columns go up as they are in the file and one launch writes
the table on the device, bit for bit the host's:

    read_event_columns(path)        the npz's four arrays in their file dtypes, p already 2*p - 1 (formed in the column's own dtype,
                                    as the reference forms it: uint8 0 -> 255, bool -> int64)
    pack_events_many(column_sets)   a list of (N,4) float64 CUDA tensors [t, x, y, p]: up to 32 sets per launch, all their columns
                                    staged in one pinned buffer and moved by one asynchronous copy

Route rule, decided on the host from the RAW t column: with np.all(t[:-1] <= t[1:]) the set takes the device route - the map to the
scaled float time is monotone, so the float times are in order too and tt[0] is the minimum the reference asserts.  Any other set
(NaN timestamps included, which compare false) takes the host route unchanged, argsort and all; so does an empty set, which raises
there what it raises today, a column of a dtype the kernel has no code for, and a float32 / float16 t column (NumPy forms t * 1e-9 in
the column's own precision).  `route_counts` counts the sets of this process by route.
"""
import ctypes
import threading

import numpy as np
import torch

from . import _lib
from .voxelizer import EventSequence

PACK_MAX = 32                                                      # event sets per eemflow_pack_events_many call (EEMFLOW_PACK_MAX)
# dtype -> EEMFLOW_PACK_* code of include/eemflow_hip.h (a bool column is uploaded as u8: its bytes are 0 / 1)
DTYPE_CODES = {np.dtype(np.uint8): 0, np.dtype(np.int8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3, np.dtype(np.int32): 4,
               np.dtype(np.int64): 5, np.dtype(np.float32): 6, np.dtype(np.float64): 7, np.dtype(np.bool_): 0}
STAGE_ALIGN = 16                                                   # every column of the staging buffer starts on a 16-byte boundary

route_counts = {'device': 0, 'host': 0}
_count_lock = threading.Lock()
_tls = threading.local()                                           # .stage: this thread's pinned staging buffer (uint8 tensor)


def read_event_columns(path):
    """events npz -> (t, x, y, p): the file's arrays in their file dtypes, p already 2*p - 1 (loader_utils.py:34, in the array's own
    dtype).  No float64 table is built."""
    d = np.load(path)
    return d["t"], d["x"], d["y"], 2 * d["p"] - 1


def route_of(columns):
    """'device' or 'host' for one (t, x, y, p) column set - the rule of this module's docstring."""
    t = columns[0]
    n = t.shape[0]
    if n == 0 or any(c.ndim != 1 or c.shape[0] != n or c.dtype not in DTYPE_CODES for c in columns):
        return 'host'
    if t.dtype.kind == 'f' and t.dtype != np.float64:
        return 'host'
    return 'device' if bool(np.all(t[:-1] <= t[1:])) else 'host'


def host_events(columns, scale_a=1e-9, scale_b=1e6, relative=True):
    """The host route: get_compressed_events' table (t * scale_a, x, y, p) through EventSequence(timestamp_multiplier=scale_b,
    convert_to_relative=relative) and the voxelizer front-end's astype('float') -> (N,4) float64 numpy."""
    t, x, y, p = columns
    out = np.empty((t.shape[0], 4), dtype=np.float64)
    out[:, 0] = t * scale_a
    out[:, 1] = x
    out[:, 2] = y
    out[:, 3] = p
    seq = EventSequence(None, {'height': 0, 'width': 0}, features=out, timestamp_multiplier=scale_b, convert_to_relative=relative)
    return np.ascontiguousarray(seq.features.astype('float'))


def device_sequence(features, params):
    """An EventSequence around an (N,4) float64 CUDA tensor that is already ordered, scaled and relative: what the voxelizer takes as
    device-resident `features` (EventSequence.__init__ would order and scale it on the host)."""
    seq = EventSequence.__new__(EventSequence)
    seq.feature_names = np.array(['ts', 'x', 'y', 'p'], dtype=object)
    seq.features = features
    seq.image_height, seq.image_width = params['height'], params['width']
    return seq


def staging_layout(column_sets):
    """Byte offsets of every column in the staging buffer: per set t | x | y | p, each column start rounded up to 16 bytes.
    -> ([(off_t, off_x, off_y, off_p), ...], total bytes)."""
    offsets, at = [], 0
    for cols in column_sets:
        offs = []
        for c in cols:
            at = (at + STAGE_ALIGN - 1) // STAGE_ALIGN * STAGE_ALIGN
            offs.append(at)
            at += c.shape[0] * c.dtype.itemsize
        offsets.append(tuple(offs))
    return offsets, at


def _stage(nbytes):
    """This thread's pinned staging buffer, at least nbytes long: grown geometrically, reused by every later call of the thread."""
    buf = getattr(_tls, "stage", None)
    if buf is None or buf.numel() < nbytes:
        cap = max(nbytes, 2 * buf.numel() if buf is not None else 1 << 16)
        _tls.stage = buf = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
    return buf


def _fill_stage(host, column_sets, offsets):
    for cols, offs in zip(column_sets, offsets):
        for c, off in zip(cols, offs):
            raw = c.view(np.uint8) if c.dtype == np.bool_ else c
            np.copyto(host[off:off + raw.nbytes].view(raw.dtype), raw)


def _count(route, n, counts):
    with _count_lock:
        route_counts[route] += n
        if counts is not None:
            counts[route] = counts.get(route, 0) + n


def _pack_call(column_sets, outs, scale_a, scale_b, relative, dev):
    """One eemflow_pack_events_many call: 1..32 device-route sets -> outs; returns when the copy and the launch are complete."""
    k = len(column_sets)
    offsets, total = staging_layout(column_sets)
    stage = _stage(total)
    _fill_stage(stage.numpy(), column_sets, offsets)
    stream = torch.cuda.current_stream(dev)
    staged = torch.empty(total, dtype=torch.uint8, device=dev)
    staged.copy_(stage[:total], non_blocking=True)
    base = staged.data_ptr()
    ptr = ctypes.c_void_p * k
    cols = [ptr(*[base + offs[c] for offs in offsets]) for c in range(4)]
    codes = (ctypes.c_int * (4 * k))(*[DTYPE_CODES[c.dtype] for cs in column_sets for c in cs])
    _lib.check(_lib.lib().eemflow_pack_events_many(k, cols[0], cols[1], cols[2], cols[3], codes,
                                                   (ctypes.c_int64 * k)(*[cs[0].shape[0] for cs in column_sets]), float(scale_a),
                                                   float(scale_b), 1 if relative else 0, ptr(*[o.data_ptr() for o in outs]),
                                                   ctypes.c_void_p(stream.cuda_stream)))
    done = torch.cuda.Event()
    done.record(stream)
    done.synchronize()               # the tensors are ready and the staging buffer is free for this thread's next call, as after a blocking .to()


def pack_events_many(column_sets, scale_a=1e-9, scale_b=1e6, relative=True, device="cuda:0", out=None, counts=None):
    """Column sets [(t, x, y, p), ...] (numpy, any of the dtypes of DTYPE_CODES; p already 2*p - 1) -> a list of (N,4) float64 CUDA
    tensors [((t * scale_a) * scale_b) - its first value when `relative`, x, y, p], each bitwise what the host route gives.  Sets in time
    order go through eemflow_pack_events_many, up to 32 per call; the others take the host route (route_of) and are uploaded as today.
    Returns with every tensor complete on the calling thread's current stream.  out: the tensors to fill (contiguous (N,4) float64
    on `device`); counts: a dict {'device': n, 'host': m} to add this call's sets to, beside the module's route_counts."""
    column_sets = [tuple(np.asarray(c) for c in cols) for cols in column_sets]
    if any(len(cols) != 4 for cols in column_sets):
        raise ValueError("pack_events_many: every column set is (t, x, y, p)")
    dev = torch.device(device)
    routes = [route_of(cols) for cols in column_sets]
    host = {i: host_events(cols, scale_a, scale_b, relative) for i, (cols, r) in enumerate(zip(column_sets, routes)) if r == 'host'}
    if out is not None:
        out = list(out)
        if len(out) != len(column_sets) or any(
                not (isinstance(o, torch.Tensor) and o.device == dev and o.dtype == torch.float64 and o.is_contiguous()
                     and tuple(o.shape) == (cols[0].shape[0], 4)) for o, cols in zip(out, column_sets)):
            raise ValueError("pack_events_many: out must be one contiguous (N,4) float64 tensor on the device per column set")
    with torch.no_grad(), torch.cuda.device(dev):
        res = out if out is not None else [torch.empty(cols[0].shape[0], 4, dtype=torch.float64, device=dev) for cols in column_sets]
        on_device = [i for i, r in enumerate(routes) if r == 'device']
        for i0 in range(0, len(on_device), PACK_MAX):
            part = on_device[i0:i0 + PACK_MAX]
            _pack_call([column_sets[i] for i in part], [res[i] for i in part], scale_a, scale_b, relative, dev)
        for i, table in host.items():
            res[i].copy_(torch.from_numpy(table))
    _count('device', len(on_device), counts)
    _count('host', len(host), counts)
    return res
