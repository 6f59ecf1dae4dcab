"""EEMFlow with the reference's nn.Module interface, computed by libeemflow_hip.so on MI355X.

Drop-in for `model.EEMFlow.EEMFlow.EEMFlow` (reference: model/EEMFlow/EEMFlow.py:71-183):
same constructor, `change_imagesize`, `forward(events1, events2) -> ((events1, events2), [flow])`,
`upsample_flow`, and the same 66-tensor state_dict, so test_EEMFlow_HREM.py / train_mvsec.py's
run_network call it unchanged.  The parameters are ordinary nn.Parameters (checkpoint layout and
optimizers keep working); the forward hands them, flattened, to the HIP library, which packs them
into MFMA fragment order once per weight version.

Two routes through the library, chosen as nn.Module semantics dictate:
* no gradient needed (torch.no_grad() / no parameter requires grad): `eemflow_forward`, the HIP-graph replay;
* gradient needed: `_EEMFlowFunction`, a torch.autograd.Function over `eemflow_forward_train` / `eemflow_backward`,
  so the reference trainer's own sequence (train_mvsec.py:245-258: model(im1, im2) -> sequence_loss ->
  scaler.scale(loss).backward() -> clip_grad_norm_ -> optimizer.step()) fills nn.Parameter.grad and works with any
  torch optimizer / loss.  After an optimizer step the changed parameters reach the device copy by one
  device-to-device gather (`eemflow_update_weights`), detected through the parameters' version counters.
forward() requires CUDA (ROCm) tensors: there is no CPU path.  Writes that bypass the version counter
(`p.data.copy_`, `torch.distributed.broadcast(p.data)`) need `model.invalidate_weights()`.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._hipmodel import HipModel, ptr_table
from .weights import CORR_TAPS_53, eemflow_param_shapes


def convrelu(in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, bias=True):
    # parameter container only (keys '<name>.0.weight' / '<name>.0.bias' as in EEMFlow.py:26-30)
    return nn.Sequential(
        nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias=bias),
        nn.LeakyReLU(0.1, inplace=True))


class Decoder(nn.Module):
    """Parameter container mirroring EEMFlow.py:37-46."""

    def __init__(self, in_channels, groups):
        super().__init__()
        self.in_channels = in_channels
        self.groups = groups
        self.conv1 = convrelu(in_channels, 100, 3, 1)
        self.conv2 = convrelu(100, 100, 3, 1, groups=groups)
        self.conv3 = convrelu(100, 100, 3, 1, groups=groups)
        self.conv4 = convrelu(100, 100, 3, 1, groups=groups)
        self.conv5 = convrelu(100, 64, 3, 1)
        self.conv6 = convrelu(64, 32, 3, 1)
        self.conv7 = nn.Conv2d(32, 2, 3, 1, 1)


class _EEMFlowFunction(torch.autograd.Function):
    """autograd through the HIP forward: d loss / d flow -> d loss / d parameter (autograd of EEMFlow.py:122-183).
    The event volumes get no gradient (the reference never asks for one: they are data)."""

    @staticmethod
    def forward(ctx, module, e1, e2, out_size, *params):
        handle = module._context(e1.device)
        b, _, h, w = e1.shape
        flow = torch.empty(b, 2, out_size[0], out_size[1], device=e1.device, dtype=torch.float32)
        serial = ctypes.c_int64()
        with torch.cuda.device(e1.device):
            _lib.check(_lib.lib().eemflow_forward_train(handle, e1.data_ptr(), e2.data_ptr(), b, h, w, flow.data_ptr(),
                                                        out_size[0], out_size[1], ctypes.byref(serial),
                                                        _lib.current_stream_ptr(e1.device)))
        ctx.module, ctx.serial, ctx.out_size = module, serial.value, out_size
        ctx.image_size = (int(module.image_size[0]), int(module.image_size[1]))     # the padder this forward ran with
        ctx.weights_version = module._weights_fingerprint()      # the tuple itself: the module's cache field may be reset (invalidate_weights, reload)
        ctx.save_for_backward(e1, e2)
        return flow

    @staticmethod
    def backward(ctx, dflow):
        m = ctx.module
        e1, e2 = ctx.saved_tensors
        L = _lib.lib()
        if m._weights_fingerprint() != ctx.weights_version:
            raise _lib.EEMFlowHipError("EEMFlow backward: a parameter was modified in place between forward and backward")
        dflow = dflow.contiguous().float()
        n = sum(p.numel() for p in m.parameters())
        grad = torch.empty(n, device=e1.device, dtype=torch.float32)
        b, _, h, w = e1.shape
        with torch.cuda.device(e1.device):
            s = _lib.current_stream_ptr(e1.device)
            if L.eemflow_backward(m._ctx, ctx.serial, e1.data_ptr(), e2.data_ptr(), dflow.data_ptr(), grad.data_ptr(), s) != 0:
                # another forward of this module ran in between and reused the workspace: recompute the activations, with the
                # padder of THIS graph's forward (a validation forward may have brought another image size; the module's next
                # forward sets its own again in _context)
                _lib.check(L.eemflow_set_image_size(m._ctx, ctx.image_size[0], ctx.image_size[1], None))
                scratch = torch.empty(b, 2, ctx.out_size[0], ctx.out_size[1], device=e1.device, dtype=torch.float32)
                serial = ctypes.c_int64()
                _lib.check(L.eemflow_forward_train(m._ctx, e1.data_ptr(), e2.data_ptr(), b, h, w, scratch.data_ptr(),
                                                   ctx.out_size[0], ctx.out_size[1], ctypes.byref(serial), s))
                _lib.check(L.eemflow_backward(m._ctx, serial.value, e1.data_ptr(), e2.data_ptr(), dflow.data_ptr(),
                                              grad.data_ptr(), s))
        grads, off = [], 0
        for i, p in enumerate(m.parameters()):
            k = p.numel()
            grads.append(grad[off:off + k].view_as(p) if ctx.needs_input_grad[4 + i] else None)
            off += k
        return (None, None, None, None, *grads)


def _needs_norm_record(method):
    """The per-tensor check of `method`(deferred_norm=True)."""
    from .voxelizer import has_norm_record

    def check(v):
        if not has_norm_record(v):
            raise ValueError(f"{method}(deferred_norm=True): every volume needs its four-float record behind it "
                             "(voxelize with normalize='deferred')")
    return check


class EEMFlow(HipModel, nn.Module):
    _ABI = "eemflow"
    _PADDER = dict(mode='chairs', eval_pad_rate=64)
    MAX_STREAM_BIDIR = 8                # forward_stream(bidirectional=True): both directions share the 16-frame pointer table

    def __init__(self, config, groups=5, n_first_channels=5, out_mesh_size=False):
        super().__init__()
        self.groups = groups
        self.n_first_channels = n_first_channels
        self.pconv1_1 = convrelu(n_first_channels, 16, 3, 2)
        self.pconv1_2 = convrelu(16, 16, 3, 1)
        self.pconv2_1 = convrelu(16, 32, 3, 2)
        self.pconv2_2 = convrelu(32, 32, 3, 1)
        self.pconv2_3 = convrelu(32, 32, 3, 1)
        self.pconv3_1 = convrelu(32, 64, 3, 2)
        self.pconv3_2 = convrelu(64, 64, 3, 1)
        self.pconv3_3 = convrelu(64, 64, 3, 1)
        # 53-tap diamond (EEMFlow+.py:89-97); the 49-entry list of EEMFlow.py:85-94 cannot feed
        # Decoder(69).  Plain attribute, not a buffer: it is not part of the checkpoint.
        self.index = torch.tensor(CORR_TAPS_53)
        self.rconv_1 = convrelu(16, 16, 3, 1)
        self.rconv_2 = convrelu(32, 16, 3, 1)
        self.rconv_3 = convrelu(64, 16, 3, 1)
        self.decoder_1 = Decoder(69, groups)
        self.decoder_2 = Decoder(69, groups)
        self.decoder_3 = Decoder(69, groups)
        self.out_conv = nn.Conv2d(6, 2, 1, 1)
        self.out_mesh_size = out_mesh_size
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        assert list(self.state_dict().keys()) == list(eemflow_param_shapes(n_first_channels, groups).keys())
        self._layout_loaded = False     # the context holds the packed weight layout: changed values reach it device to device
        self.use_graph = True

    # ------------------------------------------------------------------ reference interface
    def _twin(self):
        return EEMFlow("", groups=self.groups, n_first_channels=self.n_first_channels, out_mesh_size=self.out_mesh_size)

    def upsample_flow(self, flow, orig_size):
        if not flow.is_cuda:
            raise _lib.EEMFlowHipError("EEMFlow.upsample_flow: the HIP path needs a CUDA (ROCm) tensor")
        flow = flow.contiguous().float()
        b, c, h, w = flow.shape
        out = torch.empty(b, c, int(orig_size[0]), int(orig_size[1]), device=flow.device, dtype=torch.float32)
        with torch.cuda.device(flow.device):
            _lib.check(_lib.lib().eemflow_upsample_bilinear(
                flow.data_ptr(), out.data_ptr(), b * c, h, w, out.shape[2], out.shape[3],
                _lib.current_stream_ptr(flow.device)))
        return out

    def _out_size(self, h, w):
        return (16, 16) if (self.training and self.out_mesh_size) else (h, w)      # EEMFlow.py:126-130

    def forward(self, events1, events2):
        self._require_cuda("forward", events1, events2)
        if not hasattr(self, "image_padder"):
            raise AttributeError("call change_imagesize(img_size) before forward (as the reference requires)")
        e1 = events1.contiguous().float()
        e2 = events2.contiguous().float()
        if e1.shape != e2.shape or e1.dim() != 4 or e1.shape[1] != self.n_first_channels:
            raise ValueError(f"expected two (B,{self.n_first_channels},H,W) tensors, got {tuple(e1.shape)} and {tuple(e2.shape)}")
        b, _, h, w = e1.shape
        out_size = self._out_size(int(h), int(w))
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            flow = _EEMFlowFunction.apply(self, e1, e2, out_size, *self.parameters())
            return (events1, events2), [flow]
        ctx = self._context(e1.device)
        flow = torch.empty(b, 2, out_size[0], out_size[1], device=e1.device, dtype=torch.float32)
        with torch.cuda.device(e1.device):
            _lib.check(_lib.lib().eemflow_forward(ctx, e1.data_ptr(), e2.data_ptr(), b, h, w, flow.data_ptr(),
                                                  out_size[0], out_size[1], _lib.current_stream_ptr(e1.device)))
        return (events1, events2), [flow]

    def forward_many(self, frames, deferred_norm=False):
        """Several INDEPENDENT samples of the evaluation loop (test_mvsec.py:580-597: one `model(events1, events2)` per sample at batch 1)
        as one batch-n chain of launches, each frame staying in its own tensors: `frames` is a sequence of (events1, events2) pairs of
        [1, C, H, W] tensors; returns one `((events1, events2), [flow])` per frame - flow [1, 2, H, W], bitwise what `forward` gives for
        the frames stacked into one batch.  Inference only (no autograd graph is recorded).
        deferred_norm=True: the frames are RAW voxel grids with their normalisation record behind them (the voxelizer's
        normalize="deferred"); pconv1_1 applies loader_utils.py:527-535's (v - mean) / sd as it reads them."""
        frames = list(frames)
        keep, dev, h, w = self._check_frames(frames, _needs_norm_record("forward_many") if deferred_norm else None)
        out_size = self._out_size(h, w)
        ctx = self._context(dev)
        _lib.check(_lib.lib().eemflow_set_deferred_input_norm(ctx, 1 if deferred_norm else 0))
        n = len(keep)
        flows = [torch.empty(1, 2, out_size[0], out_size[1], device=dev, dtype=torch.float32) for _ in range(n)]
        p1, p2, po = ptr_table([a for a, _ in keep]), ptr_table([b for _, b in keep]), ptr_table(flows)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().eemflow_forward_many(ctx, n, p1, p2, po, h, w, out_size[0], out_size[1], _lib.current_stream_ptr(dev)))
        return [((frames[i][0], frames[i][1]), [flows[i]]) for i in range(n)]

    def forward_stream(self, volumes, deferred_norm=False, bidirectional=False, fb_check=None):
        """Flow along a stream of CONSECUTIVE event windows, each window encoded once (the MVSEC evaluation walks a sequence this way:
        sample i is windows i and i + 1, loader/MVSEC.py:115-116).  `volumes` are 1..16 [1, C, H, W] tensors in time order, on one
        device with one shape.  Returns one `((events1, events2), [flow])` per pair of neighbouring windows - flow [1, 2, H, W] (the
        `forward` rule for the output size), bitwise what `forward_many` gives for those pairs.  The last window is carried to the next
        call, whose first pair starts at it: a call after a carried window returns len(volumes) pairs (events1 of the first is the
        previous call's last tensor), otherwise len(volumes) - 1.  `reset_stream()` drops the carried window; `change_imagesize` to a
        new size does too.  After a weight change (optimizer step, load_state_dict) the next call raises until `reset_stream()`.
        Inference only (no autograd graph is recorded).  deferred_norm: as in `forward_many`.
        bidirectional=True: both directions of every pair for the price of the forward one plus the 1/64-grid tail (the encoder still
        runs once per window) - each item is `((events1, events2), [flow_fw], [flow_bw])`, flow_bw the flow from events2 to events1,
        bitwise `forward_many` on the swapped pair.  At most 8 volumes per call (both directions share the 16-frame pointer table).
        Calls with and without it may alternate on one stream.
        fb_check=(alpha1, alpha2) or (alpha1, alpha2, 'all' | 'obj' | 'out') (needs bidirectional=True): a fourth element
        `(mask_fw, mask_bw)`, the forward-backward consistency masks of `eemflow_amd.metrics.fb_check` ([1, 1, H, W], 1 = consistent),
        by one more launch on the same stream."""
        vols = list(volumes)
        if fb_check is not None and not bidirectional:
            raise ValueError("forward_stream: fb_check needs bidirectional=True (the check compares the two directions' flows)")
        if fb_check is not None:
            from .metrics import fb_check_args
            fb_check = fb_check_args(*fb_check)
        keep, dev, h, w = self._check_volumes(vols, self.MAX_STREAM_BIDIR if bidirectional else self.MAX_STREAM,
                                              " with bidirectional=True" if bidirectional else "",
                                              _needs_norm_record("forward_stream") if deferred_norm else None)
        out_size = self._out_size(h, w)
        L = _lib.lib()
        ctx = self._context(dev)
        n = len(keep)
        carried, nflow = self._stream_begin(ctx, n)
        _lib.check(L.eemflow_set_deferred_input_norm(ctx, 1 if deferred_norm else 0))
        flows = [torch.empty(1, 2, out_size[0], out_size[1], device=dev, dtype=torch.float32) for _ in range(nflow)]
        pv, po = ptr_table(keep), ptr_table(flows)
        if bidirectional:
            flows_bw = [torch.empty_like(f) for f in flows]
            pb = ptr_table(flows_bw)
        with torch.cuda.device(dev):
            if bidirectional:
                rc = L.eemflow_forward_stream_bidir(ctx, n, pv, po, pb, nflow, h, w, out_size[0], out_size[1], _lib.current_stream_ptr(dev))
            else:
                rc = L.eemflow_forward_stream(ctx, n, pv, po, nflow, h, w, out_size[0], out_size[1], _lib.current_stream_ptr(dev))
        pairs = self._stream_end(rc, vols, carried)
        if not bidirectional:
            return [(pairs[i], [flows[i]]) for i in range(nflow)]
        if fb_check is None or nflow == 0:
            return [(pairs[i], [flows[i]], [flows_bw[i]]) for i in range(nflow)]
        from .metrics import fb_check_many
        masks = fb_check_many(flows, flows_bw, *fb_check)
        return [(pairs[i], [flows[i]], [flows_bw[i]], masks[i]) for i in range(nflow)]

    # ------------------------------------------------------------------ HIP context plumbing
    def _flat_weights(self, device=None):
        # state_dict order == parameter registration order (the module has no buffers)
        return torch.cat([v.detach().reshape(-1).to(torch.float32) for v in self.state_dict().values()]).to(device or "cpu")

    def invalidate_weights(self):
        """Force the next forward to re-read the nn.Parameters (after writes through `.data`, which bypass the
        version counter the staleness check reads)."""
        self._weights_version = None

    def _load_weights(self, device):
        L = _lib.lib()
        if self._layout_loaded and all(p.device == device for p in self.parameters()):
            flat = self._flat_weights(device).contiguous()          # e.g. after optimizer.step(): device to device
            with torch.cuda.device(device):
                _lib.check(L.eemflow_update_weights(self._ctx, flat.data_ptr(), flat.numel(), _lib.current_stream_ptr(device)))
        else:
            flat = self._flat_weights().contiguous()
            _lib.check(L.eemflow_load_weights(self._ctx, flat.data_ptr(), flat.numel(), self.n_first_channels, self.groups))
            self._layout_loaded = True

    def _configure(self):
        L = _lib.lib()
        pad = (ctypes.c_int * 4)()
        _lib.check(L.eemflow_set_image_size(self._ctx, int(self.image_size[0]), int(self.image_size[1]), ctypes.byref(pad)))
        assert list(pad) == self.image_padder._pad
        _lib.check(L.eemflow_use_graph(self._ctx, 1 if self.use_graph else 0))
        _lib.check(L.eemflow_set_frames_in_flight(self._ctx, max(1, int(self.frames_in_flight))))
        _lib.check(L.eemflow_set_deferred_input_norm(self._ctx, 0))       # (forward_many(deferred_norm=True) turns it on for its call)

    def _release(self):
        super()._release()
        self._layout_loaded = False                              # (the packed layout went with the context)

    def backward_forms(self):
        """{"<layer>.<wgrad | dgrad | bwd>": kernel form} of the last backward (see eemflow_backward_forms)."""
        buf = ctypes.create_string_buffer(8192)
        _lib.check(_lib.lib().eemflow_backward_forms(self._ctx, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)
