"""Host-side checks of what EEMFlow, EEMFlow+ and E-RAFT share (eemflow_amd/_hipmodel.py): the context's lifecycle, the carried
window of forward_stream, replicate and change_imagesize, through a stand-in for the library that records every ABI call.  No GPU.

Only public methods and the fields other modules rely on (_ctx, _ctx_device, _weights_version, _stream_prev, _context, _release) are
used, so the file describes the wrappers' behaviour independently of how they are written."""
import contextlib
import ctypes
import gc
import os
import re
import weakref

import pytest
import torch

from eemflow_amd import _lib
from eemflow_amd.eemflow import EEMFlow
from eemflow_amd.eemflow_plus import EEMFlow_cdc
from eemflow_amd.eraft import ERAFT

MODELS = {"eemflow": lambda: EEMFlow("", 5, 5), "eemplus": lambda: EEMFlow_cdc("", 3, 5), "eraft": lambda: ERAFT("", 5)}
SETTERS = {"eemflow": ["set_image_size", "use_graph", "set_frames_in_flight", "set_deferred_input_norm"],
           "eemplus": ["set_frames_in_flight"],
           "eraft": ["keep_stages", "set_frames_in_flight", "set_alternate_corr", "set_final_only"]}
# EEMFlow switches the deferred input normalisation once more for the call itself
BEFORE_FORWARD = {"eemflow": ["set_deferred_input_norm"], "eemplus": [], "eraft": []}
CPU = torch.device("cpu")


class _Cuda(torch.Tensor):                               # (CPU tensors that pass the device check)
    is_cuda = True


def _volumes(n):
    return [torch.zeros(1, 5, 64, 64).as_subclass(_Cuda) for _ in range(n)]


class _RecordingLib:
    """Every attribute is an entry point that records its name (without the model's prefix) and succeeds."""

    def __init__(self):
        self.calls, self.handles = [], 0
        self.pending = 0                                 # what <prefix>_stream_pending reports: the context carries a window
        self.stream_rc, self.error = 0, b""
        self.pad = None                                  # what eemflow_set_image_size reports

    def __getattr__(self, symbol):
        name = re.sub(r"^(eemflow|eemplus|eraft)_", "", symbol)

        def entry(*args):
            if name == "last_error":
                return self.error
            self.calls.append(name)
            if name == "create":
                self.handles += 1
                args[1]._obj.value = 0x1000 * self.handles
            elif name == "stream_pending":
                args[1]._obj.value = self.pending
            elif name == "stream_reset":
                self.pending = 0
            elif name in ("forward_stream", "forward_stream_bidir"):
                if self.stream_rc == 0:
                    self.pending = 1
                return self.stream_rc
            elif name == "set_image_size" and args[3] is not None:
                args[3]._obj[:] = self.pad
            return None if name == "destroy" else 0
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def rig(monkeypatch):
    """(recording library, make(kind) -> module in eval mode at 64x64).  Every context is released before the real library returns."""
    lib, made = _RecordingLib(), []
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)

    def make(kind):
        net = MODELS[kind]().eval()
        net.change_imagesize((64, 64))
        lib.pad = list(net.image_padder._pad)
        made.append(weakref.ref(net))
        return net
    with torch.no_grad():                                # (stays in force while the test runs: E-RAFT's stream refuses grad mode)
        yield lib, make
    for ref in made:
        if ref() is not None:
            ref()._release()


@pytest.mark.parametrize("kind", list(MODELS))
def test_abi_call_sequences(rig, kind):
    lib, make = rig
    net = make(kind)
    setters, pre = SETTERS[kind], BEFORE_FORWARD[kind]
    first = net.forward_stream(_volumes(3))
    assert lib.take() == ["create", "load_weights"] + setters + ["stream_pending"] + pre + ["forward_stream"]
    assert len(first) == 2
    second = net.forward_stream(_volumes(3))
    assert lib.take() == setters + ["stream_pending"] + pre + ["forward_stream"]
    assert len(second) == 3
    v = _volumes(2)
    many = net.forward_many([(v[0], v[1])])
    assert lib.take() == setters + pre + ["forward_many"]
    assert len(many) == 1 and many[0][0][0] is v[0] and many[0][0][1] is v[1]


@pytest.mark.parametrize("kind", list(MODELS))
def test_pairs_are_the_callers_tensors(rig, kind):
    lib, make = rig
    net = make(kind)
    a = _volumes(3)
    out = net.forward_stream(a)
    assert len(out) == 2
    assert all(p[0][0] is a[i] and p[0][1] is a[i + 1] for i, p in enumerate(out))
    assert net._stream_prev is a[2]
    b = _volumes(2)
    out = net.forward_stream(b)
    assert len(out) == 2
    assert out[0][0][0] is a[2] and out[0][0][1] is b[0]         # the carried window opens the next call's first pair
    assert out[1][0][0] is b[0] and out[1][0][1] is b[1]
    assert net._stream_prev is b[1]
    assert net.forward_stream(_volumes(1))[0][0][0] is b[1]


@pytest.mark.parametrize("kind", list(MODELS))
def test_pending_context_without_a_tensor_starts_over(rig, kind):
    lib, make = rig
    net = make(kind)
    net.forward_stream(_volumes(2))
    net._stream_prev = None                              # the context carries a window the module cannot name as events1
    lib.take()
    out = net.forward_stream(_volumes(3))
    calls = lib.take()
    assert calls[calls.index("stream_pending") + 1] == "stream_reset" and calls[-1] == "forward_stream"
    assert len(out) == 2


@pytest.mark.parametrize("kind", list(MODELS))
def test_stale_stream_error_names_reset_stream(rig, kind):
    lib, make = rig
    net = make(kind)
    lib.stream_rc = 1
    lib.error = f"{kind}_forward_stream: the weights changed - call {kind}_stream_reset first".encode()
    with pytest.raises(_lib.EEMFlowHipError, match=r"reset_stream\(\)"):
        net.forward_stream(_volumes(2))
    assert net._stream_prev is None
    lib.error = b"some other failure"
    with pytest.raises(_lib.EEMFlowHipError, match="some other failure") as err:
        net.forward_stream(_volumes(2))
    assert "reset_stream()" not in str(err.value)


@pytest.mark.parametrize("kind", list(MODELS))
def test_changed_parameter_reloads_once(rig, kind):
    lib, make = rig
    net = make(kind)
    net.forward_stream(_volumes(2))
    net.forward_stream(_volumes(2))
    assert "load_weights" not in lib.take()[2:]          # (only the first call loaded)
    next(net.parameters()).add_(0)                       # in place: the version counter moves
    net.forward_many([tuple(_volumes(2))])
    net.forward_many([tuple(_volumes(2))])
    loads = [c for c in lib.take() if c in ("load_weights", "update_weights")]
    # EEMFlow: the layout is loaded and the parameters live on the context's device, so the values go device to device
    assert loads == (["update_weights"] if kind == "eemflow" else ["load_weights"])


@pytest.mark.parametrize("kind", list(MODELS))
def test_second_device_destroys_then_creates(rig, kind):
    lib, make = rig
    net = make(kind)
    first = net._context(CPU)
    assert net._ctx is first and net._ctx_device == CPU and net._weights_version is not None
    assert lib.take()[:2] == ["create", "load_weights"]
    other = torch.device("cuda", 1)
    second = net._context(other)
    assert lib.take()[:3] == ["destroy", "create", "load_weights"]       # (the parameters are not on that device: a full load)
    assert second is not first and net._ctx_device == other
    net._release()
    assert lib.take() == ["destroy"] and net._ctx is None
    net._release()
    assert lib.take() == []


@pytest.mark.parametrize("kind", list(MODELS))
def test_deleting_the_module_destroys_its_context(rig, kind):
    lib, make = rig
    net = make(kind)
    net.forward_stream(_volumes(2))
    lib.take()
    del net
    gc.collect()
    assert lib.take() == ["destroy"]


@pytest.mark.parametrize("kind", list(MODELS))
def test_replicate(rig, kind):
    lib, make = rig
    net = make(kind)
    net.frames_in_flight = 3
    if kind == "eraft":
        net.final_only, net.warm_start = True, True
    net.forward_stream(_volumes(2))
    twin = net.replicate()
    assert type(twin) is type(net) and twin._ctx is None and twin._stream_prev is None
    assert not twin.training and tuple(twin.image_size) == (64, 64) and twin.image_padder._pad == net.image_padder._pad
    assert twin.frames_in_flight == 3 and net.replicate(frames_in_flight=5).frames_in_flight == 5
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
    if kind == "eraft":
        assert (twin.final_only, twin.alternate_corr, twin.warm_start) == (True, False, True)
    assert net.train().replicate().training
    assert net._ctx is not None and net._stream_prev is not None         # the original keeps its own


@pytest.mark.parametrize("kind", list(MODELS))
def test_change_imagesize_and_the_carry(rig, kind):
    lib, make = rig
    fresh = MODELS[kind]()
    fresh.change_imagesize((64, 64))                     # the very first call: nothing to reset, no context to tell
    assert lib.take() == [] and fresh._stream_prev is None
    net = make(kind)
    vols = _volumes(2)
    net.forward_stream(vols)
    lib.take()
    net.change_imagesize((64, 64))                       # the same size keeps the carry ...
    assert net._stream_prev is vols[1] and lib.take() == []
    net.change_imagesize([64, 64])
    assert net._stream_prev is vols[1] and lib.take() == []
    net.change_imagesize((128, 64))                      # ... a new size drops it, in the context too
    assert net._stream_prev is None and lib.take() == ["stream_reset"]
    net.reset_stream()
    assert lib.take() == ["stream_reset"]


def test_what_only_eemflow_can_do():
    """harness and cli detect these with hasattr."""
    for name in ("MAX_STREAM_BIDIR", "invalidate_weights"):
        assert hasattr(EEMFlow, name)
        assert not hasattr(EEMFlow_cdc, name) and not hasattr(ERAFT, name)


def test_stage_names_is_shared():
    """The recorder's list is read in one place, through the model's own <prefix>_stage_list."""
    from eemflow_amd._hipmodel import HipModel
    assert "stage_names" in vars(HipModel)
    assert "stage_names" not in vars(ERAFT) and "stage_names" not in vars(EEMFlow_cdc)
    pkg = os.path.dirname(_lib.__file__)
    for name in ("eraft.py", "eemflow_plus.py"):
        assert "stage_list" not in open(os.path.join(pkg, name), encoding="utf-8").read(), name


@pytest.mark.parametrize("kind", ["eemplus", "eraft"])
def test_stage_names_parses_the_list(rig, kind, monkeypatch):
    lib, make = rig
    net = make(kind)
    net._context(CPU)
    text = b"pad pad 2 5 64 64\nl6.cat_flow - 1 2 1 1\n\x00"

    def stage_list(ctx, buf, cap, need):
        need._obj.value = len(text)
        if buf is not None:
            assert cap == len(text)
            ctypes.memmove(buf, text, len(text))
        return 0
    monkeypatch.setattr(lib, f"{kind}_stage_list", stage_list, raising=False)
    assert net.stage_names() == [("pad", "pad", (2, 5, 64, 64)), ("l6.cat_flow", "", (1, 2, 1, 1))]


def test_stream_limits_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    defines = dict(re.findall(r"^#define (\w+_MAX_VOLUMES) (\d+)$", open(os.path.join(root, "include", "eemflow_hip.h")).read(), re.M))
    assert EEMFlow.MAX_STREAM == EEMFlow_cdc.MAX_STREAM == int(defines["EEM_STREAM_MAX_VOLUMES"])
    assert ERAFT.MAX_STREAM == int(defines["ERAFT_STREAM_MAX_VOLUMES"])
    assert EEMFlow.MAX_STREAM_BIDIR == int(defines["EEM_STREAM_BIDIR_MAX_VOLUMES"])
