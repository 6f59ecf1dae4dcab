"""What EEMFlow, EEMFlow+ and E-RAFT share on the host: the library context's lifecycle, `change_imagesize`, `replicate`, the input
checks of `forward_many` / `forward_stream` and the bookkeeping of the window a stream carries from call to call.

`HipModel` is a mixin in front of nn.Module (`class EEMFlow(HipModel, nn.Module)`).  A model names its ABI prefix and its padder,
loads its weights (`_load_weights`), sets its per-call switches (`_configure`) and makes its own forward calls; the entry points the
three prefixes have in common (`<prefix>_create`, `_destroy`, `_stream_pending`, `_stream_reset`, `_get_stage`) are called from here.
"""
import ctypes

import torch

from . import _lib
from .padder import InputPadder


def ptr_table(tensors):
    """The tensors' device addresses as a C array of pointers (one null slot when there are none: a stream call that only carries)."""
    return (ctypes.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


class HipModel:
    _ABI = None                     # "eemflow" | "eemplus" | "eraft": the prefix of this model's entry points in include/eemflow_hip.h
    _PADDER = {}                    # InputPadder's keyword arguments
    _REPLICATED = ()                # attributes `replicate` copies besides weights, device, image size, mode and frames_in_flight
    MAX_COALESCE = 16               # forward_many: frames per call
    MAX_STREAM = 16                 # forward_stream: volumes per call (tests/test_hipmodel_host.py holds it to include/eemflow_hip.h)

    _ctx = None                     # the library's context, made by the first forward on a device
    _ctx_device = None
    _weights_version = None         # `_weights_fingerprint()` of the weights the context holds
    _stream_prev = None             # forward_stream: the caller's tensor of the window the context carries (events1 of the next pair)
    frames_in_flight = 1            # >= 3: this module is one of several replicas kept busy on separate streams (throughput over latency)

    def _abi(self, name):
        return getattr(_lib.lib(), f"{self._ABI}_{name}")

    # ------------------------------------------------------------------ reference interface
    def change_imagesize(self, img_size):
        old = getattr(self, "image_size", None)
        if old is not None and tuple(int(v) for v in old) != tuple(int(v) for v in img_size):
            self.reset_stream()                                  # a carried window of another size cannot start the next pair
        self.image_size = img_size
        self.image_padder = InputPadder(img_size, **self._PADDER)

    def replicate(self, frames_in_flight=None):
        """A second module with the same weights, device, image size and mode and a context of its own: what keeps one more frame
        in flight on another HIP stream (harness.TestRaftEvents(frames_in_flight=...))."""
        twin = self._twin()
        twin.load_state_dict(self.state_dict())
        twin = twin.to(next(self.parameters()).device)
        if hasattr(self, "image_size"):
            twin.change_imagesize(self.image_size)
        twin.train(self.training)
        twin.frames_in_flight = self.frames_in_flight if frames_in_flight is None else frames_in_flight
        for name in self._REPLICATED:
            setattr(twin, name, getattr(self, name))
        return twin

    # ------------------------------------------------------------------ input checks
    def _require_cuda(self, method, *tensors):
        if not all(t.is_cuda for t in tensors):
            raise _lib.EEMFlowHipError(f"{type(self).__name__}.{method}: inputs must be CUDA (ROCm) tensors - there is no CPU path")

    def _check_frames(self, frames, each=None):
        """forward_many's `frames` -> their contiguous fp32 pairs, the device, h, w.  `each(tensor)`: one more check per tensor."""
        if not 1 <= len(frames) <= self.MAX_COALESCE:
            raise ValueError(f"forward_many: 1..{self.MAX_COALESCE} frames per call, got {len(frames)}")
        if not hasattr(self, "image_padder"):
            raise AttributeError("call change_imagesize(img_size) before forward (as the reference requires)")
        keep, shape = [], None
        for a, b in frames:
            self._require_cuda("forward_many", a, b)
            a, b = a.contiguous().float(), b.contiguous().float()
            if a.shape != b.shape or a.dim() != 4 or a.shape[0] != 1 or a.shape[1] != self.n_first_channels:
                raise ValueError(f"forward_many: every frame is two (1,{self.n_first_channels},H,W) tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
            if shape is not None and a.shape != shape:
                raise ValueError("forward_many: all frames of a call share one shape")
            if each is not None:
                each(a)
                each(b)
            shape = a.shape
            keep.append((a, b))
        return keep, keep[0][0].device, int(shape[2]), int(shape[3])

    def _check_volumes(self, vols, max_vols, mode="", each=None):
        """forward_stream's `vols` -> their contiguous fp32 versions, the device, h, w.  `mode` names what lowered `max_vols`."""
        if not 1 <= len(vols) <= max_vols:
            raise ValueError(f"forward_stream: 1..{max_vols} volumes per call{mode}, got {len(vols)}")
        if not hasattr(self, "image_padder"):
            raise AttributeError("call change_imagesize(img_size) before forward (as the reference requires)")
        keep, shape = [], None
        for v in vols:
            self._require_cuda("forward_stream", v)
            v = v.contiguous().float()
            if v.dim() != 4 or v.shape[0] != 1 or v.shape[1] != self.n_first_channels:
                raise ValueError(f"forward_stream: every volume is a (1,{self.n_first_channels},H,W) tensor, got {tuple(v.shape)}")
            if shape is not None and (v.shape != shape or v.device != keep[0].device):
                raise ValueError("forward_stream: all volumes of a call share one shape and one device")
            if each is not None:
                each(v)
            shape = v.shape
            keep.append(v)
        return keep, keep[0].device, int(shape[2]), int(shape[3])

    # ------------------------------------------------------------------ the window a stream carries
    def _stream_begin(self, ctx, n):
        """Before a stream call of n volumes -> (the caller's tensor of the carried window or None, the number of pairs the call gives)."""
        pending = ctypes.c_int()
        _lib.check(self._abi("stream_pending")(ctx, ctypes.byref(pending)))
        carried = self._stream_prev if pending.value else None
        if carried is None and pending.value:
            _lib.check(self._abi("stream_reset")(ctx))            # (no tensor to name as events1: start over)
        return carried, (n if carried is not None else n - 1)

    def _stream_end(self, rc, vols, carried):
        """After the stream call returned rc: raise its error, or take vols[-1] as the carried window -> the (events1, events2) pairs,
        made of the caller's own tensors."""
        if rc != 0:
            msg = _lib.lib().eemflow_last_error().decode("utf-8", "replace")
            if f"{self._ABI}_stream_reset" in msg:
                raise _lib.EEMFlowHipError(f"{type(self).__name__}.forward_stream: {msg} - call reset_stream() on the module")
            raise _lib.EEMFlowHipError(msg)
        self._stream_prev = vols[-1]
        return list(zip(vols[:-1], vols[1:])) if carried is None else list(zip([carried] + vols[:-1], vols))

    def reset_stream(self):
        """Drop the window (E-RAFT: and the flow) `forward_stream` carries: its next call starts a new stream, with len(volumes) - 1
        pairs."""
        self._stream_prev = None
        if self._ctx is not None:
            _lib.check(self._abi("stream_reset")(self._ctx))

    # ------------------------------------------------------------------ HIP context plumbing
    def _weights_fingerprint(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _context(self, device):
        """The context on `device`, holding the current weights and this call's settings."""
        if self._ctx is None or self._ctx_device != device:
            self._release()
            handle = ctypes.c_void_p()
            _lib.check(self._abi("create")(device.index if device.index is not None else torch.cuda.current_device(),
                                           ctypes.byref(handle)))
            self._ctx, self._ctx_device, self._weights_version = handle, device, None
        fp = self._weights_fingerprint()
        if fp != self._weights_version:
            self._load_weights(device)
            self._weights_version = fp
        self._configure()
        return self._ctx

    def stage(self, name):
        """Intermediate tensor of the last forward (parity tests): see <prefix>_get_stage."""
        get_stage = self._abi("get_stage")
        dims = (ctypes.c_int * 4)()
        _lib.check(get_stage(self._ctx, name.encode(), None, 0, ctypes.byref(dims), None))
        out = torch.empty(*list(dims), device=self._ctx_device, dtype=torch.float32)
        with torch.cuda.device(self._ctx_device):
            _lib.check(get_stage(self._ctx, name.encode(), out.data_ptr(), out.numel(), ctypes.byref(dims),
                                 _lib.current_stream_ptr(self._ctx_device)))
        return out

    def stage_names(self):
        """[(name, form, (n, c, h, w))] of everything the stage recorder (`record_stages`; EEMFlow+ and E-RAFT) filed in the last call,
        in launch order."""
        stage_list = self._abi("stage_list")
        need = ctypes.c_size_t()
        _lib.check(stage_list(self._ctx, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        _lib.check(stage_list(self._ctx, buf, need.value, ctypes.byref(need)))
        out = []
        for line in buf.value.decode().splitlines():
            name, form, *dims = line.split()
            out.append((name, "" if form == "-" else form, tuple(int(d) for d in dims)))
        return out

    def _release(self):
        if self._ctx is not None:
            self._abi("destroy")(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass
