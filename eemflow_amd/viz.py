"""Visualisation on the GPU: the images the reference's evaluation loop writes with `visualize_map` (test_mvsec.py:618-637).

`flow_to_image(flow, bgr=False)` is the Middlebury colour wheel of tensor_tools.flow_to_image_dmax (utils_luo/tools.py:2385-2523, what
Test.visualize_optical_flow_light calls): a (B,2,H,W) CUDA flow -> a (B,H,W,3) uint8 CUDA tensor, every frame normalised by its own
maximum radius.  `event_image(volume, norm=None, bgr=False)` is Test.vis_map_RGB (test_mvsec.py:175-233): a (B,bins,H,W) CUDA volume ->
`(image, density)`, white with red / blue pixels where the channel sum leaves mean -+ 0.2, and the share of pixels whose sum exceeds 0.1.
The `_many` forms take lists of single frames in unrelated buffers, 16 per library call (eemflow_flow_to_image_many,
eemflow_event_image_many: two launches each).  CUDA tensors only: there is no CPU path.

`ImageWriter` writes such images as JPEG files off the evaluation's critical path: `submit` copies to pinned host memory on the current
stream and returns, worker threads encode.  The reference hands its RGB array to cv2.imwrite, which reads it as BGR - the files hold
that: the array's channel 0 is the file's blue."""
import ctypes
import os
import queue
import threading

import torch

from . import _lib


def _check_frames(name, frames, channels):
    if len(frames) < 1:
        raise ValueError(f"{name}: at least one frame")
    if not all(torch.is_tensor(t) for t in frames):
        raise TypeError(f"{name}: frames are tensors")
    if not all(t.is_cuda for t in frames):
        raise _lib.EEMFlowHipError(f"{name}: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    shape, dev = tuple(frames[0].shape), frames[0].device
    if len(shape) != 4 or shape[0] != 1 or (channels is not None and shape[1] != channels) or \
            any(tuple(t.shape) != shape or t.device != dev for t in frames):
        raise ValueError(f"{name}: all frames share one (1,{channels or 'bins'},H,W) shape and one device, got {[tuple(t.shape) for t in frames]}")
    if not all(t.is_contiguous() and t.dtype == torch.float32 for t in frames):
        raise ValueError(f"{name}: frames are contiguous float32 tensors (the kernel reads them where they are)")
    return shape, dev


def flow_to_image_many(flows, bgr=False, return_divisors=False):
    """Colour images of len(flows) (1,2,H,W) float32 CUDA flows of one size, in unrelated buffers: a list of (H,W,3) uint8 CUDA tensors
    (RGB; BGR with bgr=True).  One library call per 16 frames, on the current stream, no host synchronisation.  return_divisors: also
    the (n,) float64 device tensor of the frames' divisors (maximum radius + 2^-52; -1 + 2^-52 for a frame that holds a NaN)."""
    flows = [t.detach() for t in flows]
    shape, dev = _check_frames("flow_to_image", flows, 2)
    n, h, w = len(flows), shape[2], shape[3]
    images = [torch.empty(h, w, 3, device=dev, dtype=torch.uint8) for _ in range(n)]
    stats = torch.empty(n, 4, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        for i0 in range(0, n, 16):
            k = min(16, n - i0)
            arr = ctypes.c_void_p * k
            _lib.check(_lib.lib().eemflow_flow_to_image_many(k, arr(*[t.data_ptr() for t in flows[i0:i0 + k]]),
                                                             arr(*[t.data_ptr() for t in images[i0:i0 + k]]), stats[i0:].data_ptr(), h, w,
                                                             1 if bgr else 0, _lib.current_stream_ptr(dev)))
    return (images, stats[:, 0]) if return_divisors else images


def flow_to_image(flow, bgr=False):
    """(B,2,H,W) CUDA flow -> (B,H,W,3) uint8 CUDA tensor: the reference's flow_to_image_dmax of every frame."""
    if not torch.is_tensor(flow):
        raise TypeError("flow_to_image: flow is a tensor")
    if not flow.is_cuda:
        raise _lib.EEMFlowHipError("flow_to_image: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.dtype != torch.float32 or not flow.is_contiguous():
        raise ValueError(f"flow_to_image: a contiguous float32 (B,2,H,W) flow, got {tuple(flow.shape)} {flow.dtype}"
                         f"{'' if flow.is_contiguous() else ' (not contiguous)'}")
    return torch.stack(flow_to_image_many([flow[i:i + 1] for i in range(flow.shape[0])], bgr=bgr), 0)


def event_image_many(volumes, norms=None, bgr=False):
    """Event images of len(volumes) (1,bins,H,W) float32 CUDA volumes of one size: `(images, densities)` - a list of (H,W,3) uint8 CUDA
    tensors and an (n,) float64 device tensor.  norms: None (normalised volumes) or one 4-float CUDA record {mean, sd, scale, any} per
    volume (voxelizer.norm_record of a raw `normalize="deferred"` grid): its non-zero voxels are normalised as the first convolution
    does.  One library call per 16 volumes, on the current stream, no host synchronisation."""
    volumes = [t.detach() for t in volumes]
    shape, dev = _check_frames("event_image", volumes, None)
    n, bins, h, w = len(volumes), shape[1], shape[2], shape[3]
    if norms is not None:
        norms = list(norms)
        if len(norms) != n or not all(torch.is_tensor(r) and r.is_cuda and r.device == dev and r.dtype == torch.float32 and r.numel() == 4
                                      and r.is_contiguous() for r in norms):
            raise ValueError("event_image: norm is one contiguous 4-float CUDA record {mean, sd, scale, any} per volume")
    images = [torch.empty(h, w, 3, device=dev, dtype=torch.uint8) for _ in range(n)]
    stats = torch.empty(n, 4, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        for i0 in range(0, n, 16):
            k = min(16, n - i0)
            arr = ctypes.c_void_p * k
            _lib.check(_lib.lib().eemflow_event_image_many(k, arr(*[t.data_ptr() for t in volumes[i0:i0 + k]]),
                                                           arr(*[r.data_ptr() for r in norms[i0:i0 + k]]) if norms is not None else None,
                                                           bins, h, w, arr(*[t.data_ptr() for t in images[i0:i0 + k]]),
                                                           stats[i0:].data_ptr(), 1 if bgr else 0, _lib.current_stream_ptr(dev)))
    return images, stats[:, 0]


def event_image(volume, norm=None, bgr=False):
    """(B,bins,H,W) CUDA volume -> `(image (B,H,W,3) uint8, density (B,) float64)`, both on the device.  norm: None, or the record(s) of
    raw volumes - one 4-float tensor (B == 1) or a (B,4) tensor / list."""
    if not torch.is_tensor(volume):
        raise TypeError("event_image: volume is a tensor")
    if not volume.is_cuda:
        raise _lib.EEMFlowHipError("event_image: inputs must be CUDA (ROCm) tensors - there is no CPU path")
    if volume.dim() != 4 or volume.dtype != torch.float32 or not volume.is_contiguous():
        raise ValueError(f"event_image: a contiguous float32 (B,bins,H,W) volume, got {tuple(volume.shape)} {volume.dtype}"
                         f"{'' if volume.is_contiguous() else ' (not contiguous)'}")
    b = volume.shape[0]
    if norm is not None:
        norm = [norm.reshape(4)] if (torch.is_tensor(norm) and norm.numel() == 4) else [r for r in norm]
    images, density = event_image_many([volume[i:i + 1] for i in range(b)], norm, bgr=bgr)
    return torch.stack(images, 0), density


class ImageWriter:
    """JPEG files of (H,W,3) uint8 CUDA images, written behind the GPU work: `submit(name, image_cuda)` enqueues an asynchronous copy into
    pinned host memory on the current stream, records an event and returns; one of `threads` workers waits for the event and encodes
    `<directory>/<name>` with PIL at `quality` (95: cv2.imwrite's default).  The array's channel 0 becomes the file's BLUE, as
    cv2.imwrite reads the array it is given.  `submit` blocks while `max_pending` images are queued; `close()` (or leaving the `with`
    block) joins the workers and re-raises the first error a worker met (`reraise=False`: joins only)."""

    def __init__(self, directory, threads=4, max_pending=64, quality=95):
        try:
            from PIL import Image
        except ImportError as e:                                  # nothing is skipped silently
            raise RuntimeError("ImageWriter needs PIL (Pillow) to encode JPEG files") from e
        if threads < 1 or max_pending < 1:
            raise ValueError("ImageWriter: threads >= 1 and max_pending >= 1")
        self._Image = Image
        self.directory, self.quality = directory, int(quality)
        os.makedirs(directory, exist_ok=True)
        self._queue = queue.Queue(maxsize=int(max_pending))
        self._error, self._lock, self._closed = None, threading.Lock(), False
        self.written = []                                         # file names, in the order they were finished
        self._workers = [threading.Thread(target=self._work, daemon=True) for _ in range(int(threads))]
        for t in self._workers:
            t.start()

    def encode(self, path, array):
        """Write the (H,W,3) uint8 numpy array as cv2.imwrite would: channel 0 is blue."""
        self._Image.fromarray(array[:, :, ::-1].copy(), "RGB").save(path, format="JPEG", quality=self.quality)

    def _work(self):
        while True:
            item = self._queue.get()
            try:
                if item is None:
                    return
                name, host, ready = item
                if self._error is not None:                      # after a failure the queue is only drained
                    continue
                if ready is not None:
                    ready.synchronize()
                self.encode(os.path.join(self.directory, name), host.numpy())
                with self._lock:
                    self.written.append(name)
            except BaseException as e:                            # kept for close(); the worker goes on draining
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                self._queue.task_done()

    def submit(self, name, image):
        if self._closed:
            raise RuntimeError("ImageWriter.submit after close()")
        if not (torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3):
            raise ValueError("ImageWriter.submit: an (H,W,3) uint8 tensor")
        if image.is_cuda:
            host = torch.empty(image.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(image, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(image.device))
        else:
            host, ready = image.contiguous(), None
        self._queue.put((name, host, ready))                     # blocks while max_pending are queued

    def close(self, reraise=True):
        if not self._closed:
            self._closed = True
            for _ in self._workers:
                self._queue.put(None)
            for t in self._workers:
                t.join()
        err, self._error = self._error, None
        if err is not None and reraise:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                                     # the body's error wins; the workers still stop
            self.close(reraise=False)
        return False
