"""No operator kernel turns a NaN or an infinity into a number: every convolution form of the operator-level ABI and every
other operator of ops.hip, bwd_ops.hip and eraft_kernels.hip on poisoned inputs, one ABI call each.  `pytest -m gpu`.

Every case builds a clean input and a copy with three poisons - NaN, +inf, -inf - placed by oracle/nonfinite.py:`sites` (the corner, the
last row and column, either side of the form's own tile boundary, channel 0 and the last channel / the last channel of the first
concatenated segment; different images where the batch allows; the classes rotate over a table's cases).  It runs the call on both,
asserts the form that ran (`eemop_last_conv_form` / `eemop_last_op_form`, where the operator reports one), and holds the poisoned
output to `check_nonfinite` against torch's fp32 CPU evaluation of the same operation on the same inputs:
  (a) non-finite wherever torch's is (NaN for an infinity allowed), (b) nowhere else, (c) bitwise the clean run's output wherever the
  reference says the poison does not reach.  Outputs accumulated with atomics (weight gradients, the warp's dx, the scatter adjoints) are
  held to (a) and (b) only.
The convolution cases are the FWD / DGRAD / WGRAD tables of tests/test_gpu_ops_fp64.py at their shapes: every forward form under each of
its epilogues (none, ReLU, LeakyReLU) with a poisoned x, the gradients with a poisoned dy; PARAM poisons a weight and a bias (the weight
gradients: x), one form per family of FORM_FAMILY.  tests/test_nonfinite_host.py proves on the CPU that every case's reference holds a
non-finite value and a finite one (or is marked whole-output), that a ReLU case has a NaN pre-activation, and that the criterion rejects
six planted faults.

The reference of a bf16-piece form (family bx3 / wgrad_bx3 / dgrad_s2: conv_bx3.hip, gconvb.hip and their gradients) is torch's on the
operand those kernels multiply: every infinity of x / dy / w replaced by a NaN (a - (a & 0xffff0000) is inf - inf; the documented
contract).  Without an activation the masks are the same; under ReLU torch's relu(-inf) = 0 is a NaN there - the conservative side.

LEFT OUT, and why:
  * NaN or infinite lookup / warp COORDINATES: grid_sample on such coordinates is not a defined reference; the kernels clamp before the
    float -> int conversion, which is deliberate.
  * a poison whose partner is the ZERO PADDING - a weight gradient's dy (or x) at the border, a border tap of a poisoned filter: whether
    0 * NaN is taken (a zero-filled halo, an im2col) or the tap skipped is the implementation's choice, in torch as well.  The weight
    gradients' poisons stay one filter radius inside the map and PARAM poisons the filter's centre tap.  The transposed generic form
    (dgrad_t2_*) reads dy dilated with zeros, so a NaN WEIGHT takes the whole plane of its input channel where torch's col2im takes one
    parity class: documented in gconv.h, and PARAM's reference for that family is torch on the dilated dy.
  * a poisoned dy under a CLOSED ReLU gate: eemop_act_bwd multiplies by the gate (0 * NaN = NaN) where torch's threshold_backward selects
    0 - documented in ops.hip; the poisons of the gated backward cases sit where y > 0.
  * the voxelizers, IWE, tsimg, viz and augment: their non-finite behaviour is specified case by case and tested bitwise elsewhere.
  * sigmoid / tanh accuracy, as in the other modules (their masks are checked here).

RESULTS.  The parent commit's library fails every ReLU case of this module (all 126 forward forms under ReLU, the four forward PARAM
cases, act_fwd / binary / instance norm / batch norm with ReLU) and the gather form of the resize adjoint; the ids are listed in
tests/test_gpu_nonfinite_models.py.  This build passes every case.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops_fp64 as OPS
import test_gpu_opsbwd_fp64 as OB
from eemflow_amd import _lib
from oracle import eemflow_oracle as O
from oracle import eemflow_plus_oracle as P
from oracle import eraft_oracle as R
from oracle import fp64_bounds as B
from oracle import nonfinite as N

pytestmark = pytest.mark.gpu
DEV = OPS.DEV
SEEN = set()
RAN = set()
BX3_FAMILIES = ("bx3", "wgrad_bx3", "dgrad_s2")
ACT_NAME = {B.ACT_NONE: "none", B.ACT_RELU: "relu", B.ACT_LEAKY: "leaky"}


def _g(*key):
    return torch.Generator().manual_seed(B.ob_seed("nonfinite", *key))


def _family(form):
    return B.FORM_KAPPA_FAMILY.get(form) or B.form_family(form)


def _operand(form, *ts):
    """The tensors as the form's kernels multiply them: a bf16-piece form sees every infinity as a NaN."""
    if _family(form) in BX3_FAMILIES:
        return [N.inf_to_nan(t) for t in ts]
    return list(ts)


def site_tile(form):
    """The (rows, cols) at whose boundaries a form's poisons are placed: its output tile where the name tells, else 8 x 32."""
    t = OPS._tile(form)
    if t is None and "_tw" in form:
        t = (8, int(form.split("_tw")[1].split("_")[0]))
    return t or (8, 32)


def _act(pre, act):
    return {B.ACT_NONE: pre, B.ACT_RELU: torch.relu(pre), B.ACT_LEAKY: torch.where(pre >= 0, pre, pre * 0.1)}[act]


# =============================================================================================== the convolution tables
def fwd_inputs(idx):
    form, cs, cout, k, stride, pad, n, h, w, env = OPS.FWD[idx]
    g = _g("fwd", idx)
    wt, b = B.seeded_conv(B.ob_seed("nonfinite-fwd-w", idx) % 2**31, sum(cs), cout, k, stride, pad)
    xs = [torch.randn(n, c, h, w, generator=g) for c in cs]
    th, tw = site_tile(form)
    where_ = N.sites(idx, n, sum(cs), h, w, tile=(th * stride, tw * stride), first_seg=cs[0], snap=stride)
    return xs, N.poison_segments(xs, where_), wt, (b if idx % 5 else None)


@functools.lru_cache(maxsize=2)
def fwd_pre(idx):
    """torch's fp32 pre-activation of forward case idx on the poisoned input (shared by the case's three epilogues)."""
    form, cs, cout, k, stride, pad, n, h, w, env = OPS.FWD[idx]
    _, xp, wt, b = fwd_inputs(idx)
    x, wt = _operand(form, torch.cat(xp, 1), wt)
    return F.conv2d(x, wt, b, stride=stride, padding=pad)


def fwd_ref(idx, act):
    """{"out": reference, "pre:out": the pre-activation (ReLU), "reached:out": where the poison arrives}."""
    pre = fwd_pre(idx)
    out_scale = 0.25 if idx % 4 == 1 else 1.0
    r = {"out": _act(pre, act) * out_scale, "reached:out": ~torch.isfinite(pre)}
    if act == B.ACT_RELU:
        r["pre:out"] = pre
    return r


def dgrad_inputs(idx):
    form, cin, ci0, cic, cout, k, stride, pad, n, h, w, env = OPS.DGRAD[idx]
    g = _g("dgrad", idx)
    wt, _ = B.seeded_conv(B.ob_seed("nonfinite-dgrad-w", idx) % 2**31, cin, cout, k, stride, pad)
    hout, wout = (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1
    dy = B.random_sign((n, cout, hout, wout), g)
    th, tw = site_tile(form)
    where_ = N.sites(idx, n, cout, hout, wout, tile=(max(th // stride, 1), max(tw // stride, 1)))
    return dy, N.poison(dy, where_), wt


def dgrad_ref(idx):
    form, cin, ci0, cic, cout, k, stride, pad, n, h, w, env = OPS.DGRAD[idx]
    _, dyp, wt = dgrad_inputs(idx)
    dyp, wt = _operand(form, dyp, wt)
    return {"dx": torch.nn.grad.conv2d_input((n, cic, h, w), wt[:, ci0:ci0 + cic].contiguous(), dyp, stride=stride, padding=pad)}


def _interior(h, k, pad, stride):
    """The output rows (columns) all of whose taps lie inside the input: (lo, hi)."""
    return -(-pad // stride), (h - 1 + pad - (k - 1)) // stride


def wgrad_inputs(idx, poison_x=False):
    form, cs, cout, k, stride, pad, n, h, w, env, cat, ci0, cin = OPS.WGRAD[idx]
    g = _g("wgrad", idx)
    xs = [torch.randn(n, c, h, w, generator=g) for c in cs]
    hout, wout = (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1
    dy = B.random_sign((n, cout, hout, wout), g)
    pre_w, pre_b = torch.randn(cout, cin, *k, generator=g) * 0.01, torch.randn(cout, generator=g) * 0.01
    tile = site_tile(form.split("+")[0])
    if poison_x:
        # x at least a filter's reach inside the map: every dy it meets exists
        where_ = N.sites(idx, n, sum(cs), h, w, tile=tile, first_seg=cs[0], ylim=(k[0] * stride, h - 1 - k[0] * stride),
                         xlim=(k[1] * stride, w - 1 - k[1] * stride), channel=(0, sum(cs) - 1, cs[0] - 1)[idx % 3])
        return xs, dy, N.poison_segments(xs, where_), dy, pre_w, pre_b
    where_ = N.sites(idx, n, cout, hout, wout, tile=tile, ylim=_interior(h, k[0], pad[0], stride), xlim=_interior(w, k[1], pad[1], stride),
                     channel=(0, cout - 1, cout // 2)[idx % 3])
    return xs, dy, xs, N.poison(dy, where_), pre_w, pre_b


def wgrad_ref(idx, poison_x=False):
    form, cs, cout, k, stride, pad, n, h, w, env, cat, ci0, cin = OPS.WGRAD[idx]
    _, _, xp, dyp, pre_w, pre_b = wgrad_inputs(idx, poison_x)
    x, dyo = _operand(form.split("+")[0], torch.cat(xp, 1), dyp)
    c = x.shape[1]
    dw = pre_w.clone()
    dw[:, ci0:ci0 + c] += torch.nn.grad.conv2d_weight(x, (cout, c, *k), dyo, stride=stride, padding=pad)
    if poison_x:
        return {"dw": dw}                                           # (the bias gradient does not see x)
    return {"dw": dw, "db": pre_b + dyp.sum((0, 2, 3))}             # (the bias gradient is summed in fp32: an infinity stays one)


def wgrad_whole(idx, poison_x=False):
    form, cs, cout = OPS.WGRAD[idx][:3]
    return {"dw", "db"} if (cout == 1 and not poison_x) else set()


# (table, index, family): a poisoned weight (centre tap) and bias for the forward and data-gradient families, a poisoned x for the
# weight-gradient families - one form per family of FORM_FAMILY
def _first(table, name):
    return next(i for i, c in enumerate(table) if c[0] == name)


PARAM = [("fwd", _first(OPS.FWD, "gconv16_3x3_th2_wm4_kg1"), "direct"), ("fwd", _first(OPS.FWD, "gconvb_3x3_th4"), "bx3"),
         ("fwd", _first(OPS.FWD, "generic_splitk4"), "direct"), ("fwd", _first(OPS.FWD, "fewout_k8_c4"), "direct"),
         ("dgrad", _first(OPS.DGRAD, "dgrad_t2_generic_splitk4"), "dgrad_gconv"), ("dgrad", _first(OPS.DGRAD, "dgrad_s2w_96_3x3"), "dgrad_s2"),
         ("wgrad", _first(OPS.WGRAD, "wgrad_ring_6464"), "wgrad_ring"), ("wgrad", _first(OPS.WGRAD, "wgrad_enc_fp32_tw16_c32_s1"), "wgrad_fp32"),
         ("wgrad", _first(OPS.WGRAD, "wgrad_enc_bx3_tw16_c32_s1"), "wgrad_bx3"), ("wgrad", _first(OPS.WGRAD, "wgrad_generic_3x3_s1_bias"), "wgrad_batched")]


def param_poisoned(kind, idx):
    """(w, b) of a forward / data-gradient case with NaN and -inf at two filters' centre taps (the last and the second output channel; input
    channel 0 and the last) and +inf in bias 0."""
    if kind == "fwd":
        form, cs, cout, k, stride, pad = OPS.FWD[idx][:6]
        _, _, wt, b = fwd_inputs(idx)
        cin = sum(cs)
    else:
        form, cin, ci0, cic, cout, k, stride, pad = OPS.DGRAD[idx][:8]
        _, _, wt = dgrad_inputs(idx)
        b = None
    wp = wt.clone()
    wp[cout - 1, 0, k[0] // 2, k[1] // 2] = N.NAN
    wp[min(1, cout - 1), cin - 1, k[0] // 2, k[1] // 2] = N.NINF
    if b is None and kind == "fwd":
        b = torch.zeros(cout)
    bp = None
    if b is not None:
        bp = b.clone()
        bp[0] = N.PINF
    return wt, b, wp, bp


def param_ref(kind, idx):
    if kind == "fwd":
        form, cs, cout, k, stride, pad = OPS.FWD[idx][:6]
        xs = fwd_inputs(idx)[0]
        _, _, wp, bp = param_poisoned(kind, idx)
        (wo,) = _operand(form, wp)
        pre = F.conv2d(torch.cat(xs, 1), wo, bp, stride=stride, padding=pad)
        return {"out": torch.relu(pre), "pre:out": pre, "reached:out": ~torch.isfinite(pre)}
    if kind == "dgrad":
        form, cin, ci0, cic, cout, k, stride, pad, n, h, w, env = OPS.DGRAD[idx]
        dy = dgrad_inputs(idx)[0]
        (wo,) = _operand(form, param_poisoned(kind, idx)[2])
        if form.startswith("dgrad_t2_"):
            # the transposed generic form IS a stride-1 correlation of dy dilated with zeros (gconv.h: tstride), and a NaN weight times
            # such a zero is a NaN: torch on the operation as the kernel states it - the whole plane, not one parity class of it
            hd, wd = h + 2 * pad[0] - k[0] + 1, w + 2 * pad[1] - k[1] + 1
            dil = torch.zeros(n, cout, hd, wd)
            dil[:, :, :(dy.shape[2] - 1) * stride + 1:stride, :(dy.shape[3] - 1) * stride + 1:stride] = dy
            dy, stride = dil, 1
        return {"dx": torch.nn.grad.conv2d_input((n, cic, h, w), wo[:, ci0:ci0 + cic].contiguous(), dy, stride=stride, padding=pad)}
    return wgrad_ref(idx, poison_x=True)


def _ids(cases):
    return [f"{i:03d}-{c[0]}" for i, c in enumerate(cases)]


def _note(kind, idx, ran):
    SEEN.update(ran.split("+"))
    RAN.add((kind, idx))


def _check(tag, got, ref, clean, tile=None, atomic=()):
    for name in (k for k in ref if ":" not in k):
        reached = ref.get("reached:" + name)
        N.check_nonfinite(f"{tag}.{name}", got[name], ref[name], None if name in atomic else clean[name], tile=tile, reached=reached)


@pytest.mark.parametrize("act", [B.ACT_NONE, B.ACT_RELU, B.ACT_LEAKY], ids=lambda a: ACT_NAME[a])
@pytest.mark.parametrize("idx", range(len(OPS.FWD)), ids=_ids(OPS.FWD))
def test_forward(monkeypatch, idx, act):
    form, cs, cout, k, stride, pad, n, h, w, env = OPS.FWD[idx]
    OPS._pin(monkeypatch, env)
    xs, xp, wt, b = fwd_inputs(idx)
    out_scale, coff, ctotal = (0.25 if idx % 4 == 1 else 1.0), (idx % 3) * 4, cout + 8
    outs = []
    for x in (xp, xs):
        out, ran = OPS.run_fwd(x, wt, b, stride, pad, act, out_scale, ctotal, coff)
        assert ran == form, f"{ran} ran, not {form}"
        rest = torch.cat([out[:, :coff], out[:, coff + cout:]], 1)
        assert torch.equal(rest, torch.full_like(rest, OPS.SENTINEL)), "channels outside [out_coff, out_coff + cout) were written"
        outs.append({"out": out[:, coff:coff + cout].contiguous()})
    _note("fwd", idx, form)
    _check(f"fwd[{idx}] {form} {ACT_NAME[act]} {cs}->{cout} {n}x{h}x{w}", outs[0], fwd_ref(idx, act), outs[1])


@pytest.mark.parametrize("idx", range(len(OPS.DGRAD)), ids=_ids(OPS.DGRAD))
def test_data_gradient(monkeypatch, idx):
    form, cin, ci0, cic, cout, k, stride, pad, n, h, w, env = OPS.DGRAD[idx]
    OPS._pin(monkeypatch, env)
    dy, dyp, wt = dgrad_inputs(idx)
    outs = []
    for d in (dyp, dy):
        dx, ran = OPS.run_dgrad(d, wt, (h, w), stride, pad, ci0, cic)
        assert ran == form, f"{ran} ran, not {form}"
        outs.append({"dx": dx})
    _note("dgrad", idx, form)
    _check(f"dgrad[{idx}] {form} {cin}[{ci0}:{ci0 + cic}]<-{cout} {n}x{h}x{w}", outs[0], dgrad_ref(idx), outs[1])


def _run_wgrad_case(idx, xs, dy, pre_w, pre_b):
    form, cs, cout, k, stride, pad, n, h, w, env, cat, ci0, cin = OPS.WGRAD[idx]
    dw, db, ran = OPS.run_wgrad(xs, dy, (cout, cin, *k), stride, pad, ci0, pre_w, pre_b, cat)
    assert ran == form, f"{ran} ran, not {form}"
    return {"dw": dw, "db": db}


@pytest.mark.parametrize("idx", range(len(OPS.WGRAD)), ids=_ids(OPS.WGRAD))
def test_weight_gradient(monkeypatch, idx):
    form = OPS.WGRAD[idx][0]
    OPS._pin(monkeypatch, OPS.WGRAD[idx][9])
    _, _, xp, dyp, pre_w, pre_b = wgrad_inputs(idx)
    got = _run_wgrad_case(idx, xp, dyp, pre_w, pre_b)
    _note("wgrad", idx, form)
    _check(f"wgrad[{idx}] {form}", got, wgrad_ref(idx), None, atomic=("dw", "db"))


@pytest.mark.parametrize("kind,idx,family", PARAM, ids=[f"{k}-{i:03d}-{f}" for k, i, f in PARAM])
def test_poisoned_weight_and_bias(monkeypatch, kind, idx, family):
    table = {"fwd": OPS.FWD, "dgrad": OPS.DGRAD, "wgrad": OPS.WGRAD}[kind]
    form = table[idx][0]
    assert _family(form.split("+")[0]) == family
    OPS._pin(monkeypatch, table[idx][9] if kind != "dgrad" else table[idx][11])
    if kind == "fwd":
        form, cs, cout, k, stride, pad, n, h, w, env = table[idx]
        xs = fwd_inputs(idx)[0]
        wt, b, wp, bp = param_poisoned(kind, idx)
        outs = []
        for ww, bb in ((wp, bp), (wt, b)):
            out, ran = OPS.run_fwd(xs, ww, bb, stride, pad, B.ACT_RELU, 1.0, cout, 0)
            assert ran == form, f"{ran} ran, not {form}"
            outs.append({"out": out})
        _check(f"param fwd[{idx}] {form}", outs[0], param_ref(kind, idx), outs[1])
    elif kind == "dgrad":
        form, cin, ci0, cic, cout, k, stride, pad, n, h, w, env = table[idx]
        dy = dgrad_inputs(idx)[0]
        wt, _, wp, _ = param_poisoned(kind, idx)
        outs = []
        for ww in (wp, wt):
            dx, ran = OPS.run_dgrad(dy, ww, (h, w), stride, pad, ci0, cic)
            assert ran == form, f"{ran} ran, not {form}"
            outs.append({"dx": dx})
        _check(f"param dgrad[{idx}] {form}", outs[0], param_ref(kind, idx), outs[1])
    else:
        _, _, xp, dyp, pre_w, pre_b = wgrad_inputs(idx, poison_x=True)
        got = _run_wgrad_case(idx, xp, dyp, pre_w, pre_b)
        _check(f"param wgrad[{idx}] {form}", got, param_ref(kind, idx), None, atomic=("dw", "db"))


def test_every_form_in_the_table_ran():
    """As tests/test_gpu_ops_fp64.py: when the whole module ran, every form of the family table was produced under the poison."""
    table = set(B.FORM_FAMILY) | set(B.FORM_KAPPA)
    assert SEEN <= table, sorted(SEEN - table)
    every = {("fwd", i) for i in range(len(OPS.FWD))} | {("dgrad", i) for i in range(len(OPS.DGRAD))} | {("wgrad", i) for i in range(len(OPS.WGRAD))}
    if RAN >= every:
        missing = sorted(table - SEEN - {f for f in table if f.startswith("wgrad_generic") and not f.endswith("_bias")})
        assert not missing, f"{len(missing)} forms of the table never ran: {missing}"       # (every case here passes db: the *_bias names)


# =============================================================================================== the other operators
class Case:
    """One ABI call: build() -> (clean inputs, poisoned inputs); ref(inputs) -> {output: torch's, "pre:<output>", "reached:<output>"};
    run(inputs) -> {output: the GPU's}.  whole: outputs that are non-finite everywhere; atomic: outputs held to (a) and (b) only."""

    def __init__(self, name, build, ref, run, form=None, whole=(), atomic=(), env=None):
        self.name, self.build, self.ref, self.run, self.form = name, build, ref, run, form
        self.whole, self.atomic, self.env = set(whole), set(atomic), env or {}


CASES = []
L = _lib.lib
_dev, _sp, Out = OB._dev, OB._sp, OB.Out
N_EL = 1027                                     # B.OB_ELEMENTWISE_N's largest: five blocks, the 16-byte path's tail


def _idx3(k, n=N_EL):
    """Three flat positions of a vector: the first, the last (the tail) and either side of the first block boundary, rotating."""
    c = [0, n - 1, 255, 256]
    return [(c[(k + j) % 4],) for j in range(3)]


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _vec(*key, n=N_EL):
    return torch.randn(n, generator=_g(*key))


def _one(fn, key="y"):
    return lambda t: {key: fn(*t)}


# ---- activations
ACT_TORCH = {B.GACT_NONE: lambda v: v, B.GACT_RELU: torch.relu, B.GACT_SIGMOID: torch.sigmoid, B.GACT_TANH: torch.tanh,
             B.GACT_LEAKY: lambda v: torch.where(v > 0, v, v * torch.tensor(B.LEAKY, dtype=torch.float32))}


def _act_fwd(kind):
    def build():
        v = _vec("act_fwd", kind)
        return (v,), (N.poison(v, _idx3(kind)),)

    def ref(t):
        r = {"y": ACT_TORCH[kind](t[0]), "reached:y": ~torch.isfinite(t[0])}
        if kind == B.GACT_RELU:
            r["pre:y"] = t[0]
        return r

    def run(t):
        out, v = Out(N_EL), _dev(t[0])
        _lib.check(L().eemop_act_fwd(v.data_ptr(), N_EL, kind, out.ptr(), _sp()))
        return {"y": out.cpu()}
    _add(f"act_fwd_kind{kind}", build, ref, run, form="act_fwd")


def _open_gates(y, k):
    """Three positions where the stored output is > 0 (the gate is open), spread over the vector."""
    pos = torch.nonzero(y.reshape(-1) > 0).reshape(-1)
    return [(int(pos[(k + j) % 3]),) if j == 0 else (int(pos[-1 - (k + j) % 3]),) if j == 1 else (int(pos[len(pos) // 2]),) for j in range(3)]


def _act_bwd(kind):
    scale = 1.7 if kind != B.GACT_LEAKY else 0.25

    def build():
        g = _g("act_bwd", kind)
        dy, v = B.random_sign((N_EL,), g), torch.randn(N_EL, generator=g)
        y = {B.GACT_SIGMOID: torch.sigmoid(v), B.GACT_TANH: torch.tanh(v), B.GACT_NONE: v}.get(kind)
        if y is None:
            y = B.ob_gated_output(v, B.ob_seed("nonfinite.act_bwd.y", kind))
        where_ = _open_gates(y, kind) if kind == B.GACT_RELU else _idx3(kind)
        return (dy, y), (N.poison(dy, where_), y)

    def ref(t):
        return {"dx": B.ob_act_bwd_ref(t[0], t[1], kind, scale)[0].float()}

    def run(t):
        out, d, y = Out(N_EL), _dev(t[0]), _dev(t[1])
        _lib.check(L().eemop_act_bwd(d.data_ptr(), y.data_ptr(), N_EL, kind, scale, out.ptr(), _sp()))
        return {"dx": out.cpu()}
    _add(f"act_bwd_kind{kind}", build, ref, run, form="act_bwd")


def _binary(kind, which):
    def build():
        a, b = _vec("binary.a", kind), _vec("binary.b", kind)
        bad = (N.poison(a, _idx3(kind + which)), b) if which == 0 else (a, N.poison(b, _idx3(kind + which)))
        return (a, b), bad

    def ref(t):
        a, b = t
        alpha = torch.tensor(-0.3, dtype=torch.float32)
        pre = {0: a + b, 1: a - b, 2: a * b, 3: a + b, 4: alpha * a}[kind]
        r = {"y": torch.relu(pre) if kind == 3 else pre, "reached:y": ~torch.isfinite(pre)}
        if kind == 3:
            r["pre:y"] = pre
        return r

    def run(t):
        out, a, b = Out(N_EL), _dev(t[0]), _dev(t[1])
        _lib.check(L().eemop_binary(kind, a.data_ptr(), b.data_ptr(), -0.3, N_EL, out.ptr(), _sp()))
        return {"y": out.cpu()}
    _add(f"binary_kind{kind}_{'ab'[which]}", build, ref, run, form="binary")


def _sum_n(aligned):
    count = 3

    def build():
        ts = [_vec("sum_n", aligned, i) for i in range(count)]
        where_ = _idx3(int(aligned))
        return tuple(ts), tuple(N.poison(t, [where_[i]], [N.POISONS[i]]) for i, t in enumerate(ts))

    def run(t):
        dev = [_dev(x) for x in t]
        if not aligned:
            hold = torch.empty(N_EL + 1, device=DEV)
            hold[1:].copy_(dev[-1])
            dev[-1] = hold[1:]
        arr = (ctypes.c_void_p * count)(*[x.data_ptr() for x in dev])
        out = Out(N_EL)
        _lib.check(L().eemop_sum_n(ctypes.cast(arr, ctypes.c_void_p), count, N_EL, out.ptr(), _sp()))
        return {"y": out.cpu()}
    _add(f"sum_n_{'v4' if aligned else 'scalar'}", build, lambda t: {"y": (t[0] + t[1]) + t[2]}, run, form="sum_n_v4" if aligned else "sum_n_scalar")


def _gru():
    def build():
        g = _g("gru")
        z, h, q, d = torch.rand(N_EL, generator=g) * 0.9 + 0.05, torch.randn(N_EL, generator=g), torch.randn(N_EL, generator=g), B.random_sign((N_EL,), g)
        w = _idx3(1)
        bad = (N.poison(z, [w[0]], [N.NAN]), N.poison(h, [w[1]], [N.PINF]), N.poison(q, [w[2]], [N.NINF]), d)
        return (z, h, q, d), bad

    def run(t):
        out, z, h, q = Out(N_EL), _dev(t[0]), _dev(t[1]), _dev(t[2])
        _lib.check(L().eemop_gru_blend(z.data_ptr(), h.data_ptr(), q.data_ptr(), N_EL, out.ptr(), _sp()))
        return {"y": out.cpu()}
    _add("gru_blend", build, lambda t: {"y": (1 - t[0]) * t[1] + t[0] * t[2]}, run, form="gru_blend")

    def build_b():
        (z, h, q, d), _ = build()
        return (z, h, q, d), (z, h, q, N.poison(d, _idx3(2)))

    def ref_b(t):
        z, h, q, d = t
        return {"dz": d * (q - h), "dh": d * (1 - z), "dq": d * z}

    def run_b(t):
        z, h, q, d = (_dev(x) for x in t)
        dz, dh, dq = Out(N_EL), Out(N_EL), Out(N_EL)
        _lib.check(L().eemop_gru_blend_bwd(d.data_ptr(), z.data_ptr(), h.data_ptr(), q.data_ptr(), N_EL, dz.ptr(), dh.ptr(), dq.ptr(), _sp()))
        return {"dz": dz.cpu(), "dh": dh.cpu(), "dq": dq.cpu()}
    _add("gru_blend_bwd", build_b, ref_b, run_b, form="gru_blend_bwd")


# ---- norms: a poisoned value takes its whole plane (instance norm) or channel (batch norm, with the statistics)
def _plane_sites(k, planes, hw):
    """NaN, +inf, -inf in three different planes of [planes, hw]; the last plane stays clean."""
    p = _idx3(k, hw)
    return [((k + j) % (planes - 1), p[j][0]) for j in range(3)]


def _instnorm_fwd(hw, relu, res):
    planes = 4

    def build():
        g = _g("instnorm", hw, relu, res)
        x = B.ob_norm_input(1, planes, hw, B.ob_seed("nonfinite.instnorm", hw))[0]
        r = torch.randn(planes, hw, generator=g) if res else None
        if res == 2:                                            # the poison arrives with the residual: its own element only
            return (x, r), (x, N.poison(r, [(planes - 1, s[1]) for s in _plane_sites(relu, planes, hw)]))
        return (x, r), (N.poison(x, _plane_sites(relu + hw, planes, hw)), r)

    def ref(t):
        x, r = t
        v = F.instance_norm(x[None], eps=1e-5)[0]
        if relu:
            v = torch.relu(v)
        pre = v + r if r is not None else v
        out = {"y": torch.relu(pre) if r is not None else v, "reached:y": ~torch.isfinite(pre)}
        if r is not None or relu:
            out["pre:y"] = pre if r is not None else F.instance_norm(x[None], eps=1e-5)[0]
        return out

    def run(t):
        x, r = _dev(t[0]), (_dev(t[1]) if t[1] is not None else None)
        out = Out(planes, hw)
        _lib.check(L().eemop_instnorm_fwd(x.data_ptr(), r.data_ptr() if r is not None else None, planes, hw, relu, out.ptr(), _sp()))
        return {"y": out.cpu()}
    _add(f"instnorm_fwd_hw{hw}_relu{relu}_res{res}", build, ref, run)


def _instnorm_bwd(hw, relu):
    planes = 4

    def build():
        x = B.ob_norm_input(1, planes, hw, B.ob_seed("nonfinite.instnorm", hw))[0]
        y = torch.relu(F.instance_norm(x[None], eps=1e-5)[0]) if relu else F.instance_norm(x[None], eps=1e-5)[0]
        dy = B.random_sign((planes, hw), _g("instnorm.dy", hw))
        where_ = []
        for j in (0, 2, 3):                                     # one poison per plane, at an open gate; the constant plane 1 stays clean
            pos = torch.nonzero(y[j] > 0).reshape(-1) if relu else torch.arange(hw)
            where_.append((j, int(pos[(0, -1, len(pos) // 2)[(j + relu) % 3]])))
        return (x, y, dy), (x, y, N.poison(dy, where_))

    def ref(t):
        return {"dx": B.ob_instnorm_bwd_ref(t[0], t[1], t[2], relu, dtype=torch.float32)}

    def run(t):
        x, y, d = (_dev(v) for v in t)
        dx = Out(planes, hw)
        _lib.check(L().eemop_instnorm_bwd(x.data_ptr(), y.data_ptr(), d.data_ptr(), planes, hw, relu, dx.ptr(), _sp()))
        return {"dx": dx.cpu()}
    _add(f"instnorm_bwd_hw{hw}_relu{relu}", build, ref, run, form="instnorm_bwd_t1024" if hw >= 16384 else "instnorm_bwd_t256")


def _bn_inputs(n, c, hw, relu):
    x, w, b, rm, rv, g = OB._bn_case(n, c, hw, relu)
    return x, w, b, rm, rv, B.random_sign((n, c, hw), g)


def _bn_train_fwd(n, c, hw, relu):
    t_ = "t1024" if n * hw >= 16384 else "t256"

    def build():
        x, w, b, rm, rv, _ = _bn_inputs(n, c, hw, relu)
        xp = N.poison(x, [(0, 1, 0), (n - 1, 1, hw - 1), (0, 1, hw // 2)])         # all in channel 1: the other channels stay clean
        return (x, w, b, rm, rv), (xp, w, b, rm, rv)

    def ref(t):
        r = B.ob_bn_train_fwd_ref(*t, 0.1, 1e-5, relu)
        return {"y": r["y32"], **{k: r[k][0].float() for k in ("save_mean", "save_rstd", "running_mean", "running_var")}}

    def run(t):
        x, w, b = (_dev(v) for v in t[:3])
        y, sm, sr, rmo, rvo = Out(n, c, hw), Out(c), Out(c), Out(c, init=_dev(t[3])), Out(c, init=_dev(t[4]))
        _lib.check(L().eemop_batchnorm_train_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), rmo.ptr(), rvo.ptr(), n, c, hw, 0.1, 1e-5, relu, y.ptr(),
                                                 sm.ptr(), sr.ptr(), _sp()))
        return {"y": y.cpu(), "save_mean": sm.cpu(), "save_rstd": sr.cpu(), "running_mean": rmo.cpu(), "running_var": rvo.cpu()}
    _add(f"bn_train_fwd_n{n}c{c}hw{hw}_relu{relu}", build, ref, run, form=f"bn_train_fwd_{t_}")


def _bn_eval_fwd(n, c, hw, relu):
    t_ = "t1024" if n * hw >= 16384 else "t256"

    def build():
        x, w, b, rm, rv, _ = _bn_inputs(n, c, hw, relu)
        w = w.clone()
        w[0] = 0.5                                               # (a zero weight times an infinity is a NaN in torch and on the GPU alike; not the point here)
        return (x, w, b, rm, rv), (N.poison(x, [(0, 0, 0), (n - 1, c - 1, hw - 1), (0, 1, min(256, hw - 1))]), w, b, rm, rv)

    def ref(t):
        pre = B.ob_bn_eval_fwd_ref(*t, 1e-5, 0, dtype=torch.float32)
        r = {"y": torch.relu(pre) if relu else pre, "reached:y": ~torch.isfinite(pre)}
        if relu:
            r["pre:y"] = pre
        return r

    def run(t):
        x, w, b, rm, rv = (_dev(v) for v in t)
        y = Out(n, c, hw)
        _lib.check(L().eemop_batchnorm_eval_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), n, c, hw, 1e-5, relu, y.ptr(), _sp()))
        return {"y": y.cpu()}
    _add(f"bn_eval_fwd_n{n}c{c}hw{hw}_relu{relu}", build, ref, run, form=f"bn_eval_fwd_{t_}")


def _bn_bwd(n, c, hw, relu, train):
    t_ = "t1024" if n * hw >= 16384 else "t256"

    def build():
        x, w, b, rm, rv, dy = _bn_inputs(n, c, hw, relu)
        refs = B.ob_bn_train_fwd_ref(x, w, b, rm, rv, 0.1, 1e-5, relu)
        y = refs["y32"]
        sm, sr = refs["save_mean"][0].float(), refs["save_rstd"][0].float()
        pos = torch.nonzero(y[:, 1].reshape(-1) > 0).reshape(-1) if relu else torch.arange(n * hw)
        where_ = [(int(p) // hw, 1, int(p) % hw) for p in (pos[0], pos[-1], pos[len(pos) // 2])]         # channel 1, open gates
        return (x, y, dy, w, sm, sr, rm, rv), (x, y, N.poison(dy, where_), w, sm, sr, rm, rv)

    def ref(t):
        x, y, dy, w, sm, sr, rm, rv = t
        if train:
            dx, dw, db = B._bn_bwd(x, y, dy, w, sm, sr, relu, torch.float32, True)[:3]
        else:
            dx, dw, db = B._bn_bwd(x, y, dy, w, rm, 1.0 / torch.sqrt(rv + 1e-5), relu, torch.float32, False)[:3]
        return {"dx": dx, "dweight": dw, "dbias": db}

    def run(t):
        x, y, dy, w, sm, sr, rm, rv = (_dev(v) for v in t)
        dx, dw, db = Out(n, c, hw), Out(c), Out(c)
        if train:
            _lib.check(L().eemop_batchnorm_train_bwd(x.data_ptr(), y.data_ptr(), dy.data_ptr(), w.data_ptr(), sm.data_ptr(), sr.data_ptr(), n, c, hw,
                                                     relu, dx.ptr(), dw.ptr(), db.ptr(), _sp()))
        else:
            _lib.check(L().eemop_batchnorm_eval_bwd(x.data_ptr(), y.data_ptr(), dy.data_ptr(), w.data_ptr(), rm.data_ptr(), rv.data_ptr(), n, c, hw, 1e-5,
                                                    relu, dx.ptr(), dw.ptr(), db.ptr(), _sp()))
        return {"dx": dx.cpu(), "dweight": dw.cpu(), "dbias": db.cpu()}
    k = "train" if train else "eval"
    _add(f"bn_{k}_bwd_n{n}c{c}hw{hw}_relu{relu}", build, ref, run, form=f"bn_{k}_bwd_{t_}")


# ---- the correlation pyramid, the lookup, convex upsampling
PYR_C, PYR_H, PYR_W = 40, 18, 18                # B.OB_PYRAMID_CASES: c = 40 leaves a remainder of the 16-channel chunks


def _pyramid(which):
    b = 2

    def build():
        g = _g("pyramid", which)
        f1, f2 = torch.randn(b, PYR_C, PYR_H, PYR_W, generator=g), torch.randn(b, PYR_C, PYR_H, PYR_W, generator=g)
        where_ = N.sites(which, b, PYR_C, PYR_H, PYR_W, tile=(8, 8))
        return (f1, f2), ((N.poison(f1, where_), f2) if which == 0 else (f1, N.poison(f2, where_)))

    def ref(t):
        return {f"pyr{l}": p[:, 0] for l, p in enumerate(R.corr_pyramid(*t))}

    def run(t):
        f1, f2 = _dev(t[0]), _dev(t[1])
        outs = [Out(b * PYR_H * PYR_W, PYR_H >> l, PYR_W >> l) for l in range(4)]
        _lib.check(L().eemop_corr_pyramid_fwd(f1.data_ptr(), f2.data_ptr(), b, PYR_C, PYR_H, PYR_W, *[o.ptr() for o in outs], _sp()))
        return {f"pyr{l}": o.cpu() for l, o in enumerate(outs)}
    _add(f"corr_pyramid_fmap{which + 1}", build, ref, run)


def _lookup():
    h, w = B.OB_LOOKUP_SHAPES[1]                 # 17 x 19

    def build():
        g = _g("lookup")
        coords = B.ob_lookup_coords(h, w, "smooth", B.ob_seed("nonfinite.lookup"))
        pyr = [torch.randn(2 * h * w, h >> l, w >> l, generator=g) for l in range(4)]
        bad = []
        for l, p in enumerate(pyr):                             # a poisoned cell in three rows of every level
            hl, wl = p.shape[1:]
            bad.append(N.poison(p, [(0, 0, 0), (h * w + 5, hl - 1, wl - 1), (2 * h * w - 1, hl // 2, wl // 2)]))
        return (pyr, coords), (bad, coords)

    def ref(t):
        return {"out": R.corr_lookup([p[:, None] for p in t[0]], t[1])}

    def run(t):
        ps, c = [_dev(p) for p in t[0]], _dev(t[1])
        out = Out(2, 324, h, w)
        _lib.check(L().eemop_corr_lookup_fwd(*[p.data_ptr() for p in ps], c.data_ptr(), 2, h, w, out.ptr(), _sp()))
        return {"out": out.cpu()}
    _add("corr_lookup_fwd", build, ref, run)


def _convex(which):
    h, w = B.OB_CONVEX_SHAPES[0]                 # 5 x 7

    def build():
        flow, mask, _ = B.ob_convex_inputs(h, w, "normal", B.ob_seed("nonfinite.convex"))
        if which == "mask":
            # logits: NaN and +inf make the softmax of their nine NaN; -inf is a weight of exactly 0 - a number, legitimately
            return (flow, mask), (flow, N.poison(mask, [(0, 0, 0, 0), (1, 575, h - 1, w - 1), (0, 4 * 64 + 9, 2, 3)]))
        return (flow, mask), (N.poison(flow, [(0, 0, 0, 0), (1, 1, h - 1, w - 1), (0, 1, 2, 3)]), mask)

    def ref(t):
        out = R.convex_upsample(t[0], t[1])
        bad = ~torch.isfinite(t[0]).all(1, keepdim=True) if which == "flow" else ~torch.isfinite(t[1]).view(2, 9, 8, 8, h, w).all(1)
        if which == "flow":                                      # a flow pixel reaches the 8 x 8 blocks of its 3 x 3 neighbours
            reach = F.max_pool2d(bad.float(), 3, 1, 1).bool().repeat_interleave(8, 2).repeat_interleave(8, 3).expand(2, 2, 8 * h, 8 * w)
        else:
            reach = bad.permute(0, 3, 1, 4, 2).reshape(2, 1, 8 * h, 8 * w).expand(2, 2, 8 * h, 8 * w)
        return {"out": out, "reached:out": reach}

    def run(t):
        f, m, z = _dev(t[0]), _dev(t[1]), torch.zeros(2, 2, h, w, device=DEV)
        up = Out(2, 2, 8 * h, 8 * w)
        _lib.check(L().eemop_convex_upsample_fwd(z.data_ptr(), f.data_ptr(), m.data_ptr(), 2, h, w, up.ptr(), _sp()))
        return {"out": up.cpu()}
    _add(f"convex_upsample_fwd_{which}", build, ref, run)


# ---- pooling, resizing, warps, the 53-tap correlation
def _pool2(bwd):
    h, w = 7, 9

    def build():
        g = _g("pool2", bwd)
        if bwd:
            dy = B.random_sign((4, h // 2, w // 2), g)
            return (dy,), (N.poison(dy, [(0, 0, 0), (1, h // 2 - 1, w // 2 - 1), (2, 1, 2)]),)
        x = torch.randn(4, h, w, generator=g)
        return (x,), (N.poison(x, [(0, 0, 0), (1, h - 2, w - 2), (2, 3, 4)]),)

    def ref(t):
        if bwd:
            return {"dx": B.pool_bwd_ref(t[0][None], (h, w), 2)[0][0].float()}
        return {"y": F.avg_pool2d(t[0][None], 2, 2)[0]}

    def run(t):
        a = _dev(t[0])
        if bwd:
            dx = Out(4, h, w)
            _lib.check(L().eemop_pool2_bwd(a.data_ptr(), dx.ptr(), 4, h, w, _sp()))
            return {"dx": dx.cpu()}
        y = Out(4, h // 2, w // 2)
        _lib.check(L().eemop_pool2_fwd(a.data_ptr(), y.ptr(), 4, h, w, _sp()))
        return {"y": y.cpu()}
    _add("pool2_bwd" if bwd else "pool2_fwd", build, ref, run, form="pool2_bwd" if bwd else None)


def _resize(in_hw, out_hw, form):
    nc = 4

    def build():
        g = _g("resize", in_hw, out_hw)
        if form == "resize_ac":
            x = torch.randn(nc, *in_hw, generator=g)
            return (x,), (N.poison(x, [(0, 0, 0), (1, in_hw[0] - 1, in_hw[1] - 1), (2, in_hw[0] // 2, in_hw[1] // 2)]),)
        d = B.random_sign((nc, *out_hw), g)
        return (d,), (N.poison(d, [(0, 0, 0), (1, out_hw[0] - 1, out_hw[1] - 1), (2, out_hw[0] // 2, out_hw[1] // 2 + 1)]),)

    def ref(t):
        if form == "resize_ac":
            return {"y": F.interpolate(t[0][None], list(out_hw), mode="bilinear", align_corners=True)[0]}
        x = torch.zeros(1, nc, *in_hw, requires_grad=True)
        F.interpolate(x, list(out_hw), mode="bilinear", align_corners=True).backward(t[0][None])
        return {"dx": x.grad[0]}

    def run(t):
        if form == "resize_ac":
            return {"y": OB.run_resize_fwd(t[0], out_hw)}
        return {"dx": OB.run_resize_bwd(t[0], in_hw)}
    _add(f"{form}_{in_hw[0]}x{in_hw[1]}_{out_hw[0]}x{out_hw[1]}", build, ref, run, form=form,
         env={"EEM_RESIZE_BWD_SCATTER": "1"} if form.endswith("scatter") else {}, atomic=("dx",) if form.endswith("scatter") else ())


WARP_TORCH = {0: P.warp_align_true, 1: P.torch_warp, 2: P.warping_layer_no_div}


def _warp(mode, bwd):
    c, h, w = B.OB_WARP_SHAPES[0]                # 5 x 17 x 23, batch 6: one image per rule of the flows

    def build():
        g = _g("warp", mode)
        flows = B.ob_warp_flows(h, w, B.ob_seed("nonfinite.warp"))
        x = torch.randn(6, c, h, w, generator=g)
        dout = B.random_sign((6, c, h, w), g)
        xp = N.poison(x, [(5, 0, 8, 11), (5, c - 1, h - 2, w - 2), (4, 2, 3, 5)])          # (image 5: the random flows; 4: far outside)
        return (x, flows, dout), (xp, flows, dout)

    def ref(t):
        x, flows, dout = t
        if not bwd:
            return {"out": WARP_TORCH[mode](x, flows)}
        xr, fr = x.clone().requires_grad_(True), flows.clone().requires_grad_(True)
        WARP_TORCH[mode](xr, fr).backward(dout)
        return {"dflow": fr.grad}                                # (dx does not see x: the scatter of dout alone)

    def run(t):
        if not bwd:
            return {"out": OB.run_warp_fwd(t[0], t[1], mode)}
        dx, df = OB.run_warp_bwd(t[0], t[1], t[2], mode)
        return {"dx": dx, "dflow": df}
    _add(f"warp_{'bwd' if bwd else 'fwd'}_m{mode}", build, ref, run, form=f"warp_bwd_m{mode}" if bwd else None, atomic=("dx",) if bwd else ())


def _upflow():
    (h, w), (oh, ow) = (5, 7), (12, 17)

    def build():
        x = torch.randn(2, 2, h, w, generator=_g("upflow"))
        return (x,), (N.poison(x, [(0, 0, 0, 0), (1, 1, h - 1, w - 1), (0, 1, 2, 3)]),)

    def ref(t):
        x = t[0].clone()
        res = P.upsample2d_flow_as(x, (oh, ow), if_rate=True)
        return {"res": res, "scaled": x}

    def run(t):
        x = _dev(t[0]).clone()
        out = Out(2, 2, oh, ow)
        _lib.check(L().eemplus_upsample_flow_as(x.data_ptr(), 2, h, w, oh, ow, 1, out.ptr(), _sp()))
        torch.cuda.synchronize()
        return {"res": out.cpu(), "scaled": x.cpu()}
    _add("upsample_flow_as", build, ref, run)


def _corr53(bwd):
    b, c, h, w = 2, 24, 9, 13

    def build():
        g = _g("corr53", bwd)
        f1, f2 = torch.randn(b, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g)
        d = B.random_sign((b, 53, h, w), g)
        if bwd:
            return (f1, f2, d), (f1, f2, N.poison(d, [(0, 0, 4, 6), (1, 52, 4, 5), (0, 26, 4, 8)]))
        # (the poisons of f1 and f2 stay four pixels inside: at the border a tap's partner is the zero padding - see LEFT OUT)
        return (f1, f2, d), (N.poison(f1, [(0, 0, 4, 4), (1, c - 1, 4, 8)]), N.poison(f2, [(1, 0, 4, 4)], [N.NINF]), d)

    def ref(t):
        if not bwd:
            return {"out": O.local_corr53(t[0], t[1])}
        f1, f2 = t[0].clone().requires_grad_(True), t[1].clone().requires_grad_(True)
        O.local_corr53(f1, f2).backward(t[2])
        return {"df1": f1.grad, "df2": f2.grad}

    def run(t):
        f1, f2, d = (_dev(v) for v in t)
        if not bwd:
            out = Out(b, 53, h, w)
            _lib.check(L().eemflow_local_corr53(f1.data_ptr(), f2.data_ptr(), b, c, h, w, out.ptr(), _sp()))
            return {"out": out.cpu()}
        d1, d2 = Out(b, c, h, w), Out(b, c, h, w)
        _lib.check(L().eemop_local_corr53_bwd(d.data_ptr(), f1.data_ptr(), f2.data_ptr(), b, c, h, w, d1.ptr(), d2.ptr(), _sp()))
        return {"df1": d1.cpu(), "df2": d2.cpu()}
    _add("local_corr53_bwd" if bwd else "local_corr53_fwd", build, ref, run)


# ---- copies and the shuffle: bitwise, the poisons' payloads included
def _copies():
    def build():
        g = _g("copies")
        src, wide, x = torch.randn(2, 3, 35, generator=g), torch.randn(2, 7, 35, generator=g), torch.randn(2, 6, 35, generator=g)
        bad = (N.poison(src, [(0, 0, 0), (1, 2, 34), (0, 1, 17)]), N.poison(wide, [(0, 4, 0), (1, 6, 34), (0, 3, 5)]),
               N.poison(x, [(0, 0, 0), (1, 5, 34), (0, 3, 17)]))
        return (src, wide, x), bad

    def ref(t):
        src, wide, x = t
        into = torch.full((2, 7, 35), OB.SENTINEL)
        into[:, 2:5] = src
        return {"into": into, "outof": wide[:, 4:7].contiguous(), "shuffle": B.ob_shuffle_ref(x, 3, 0), "unshuffle": B.ob_shuffle_ref(x, 3, 1),
                "pad": F.pad(x.view(1, 12, 5, 7), (1, 2, 3, 0), mode="replicate")[0]}

    def run(t):
        s, wd, x = (_dev(v) for v in t)
        into, outof, sh, ush, pad = Out(2, 7, 35), Out(2, 3, 35), Out(2, 6, 35), Out(2, 6, 35), Out(12, 8, 10)
        _lib.check(L().eemop_copy_channels(s.data_ptr(), 3, 0, into.ptr(), 7, 2, 3, 2, 35, _sp()))
        _lib.check(L().eemop_copy_channels(wd.data_ptr(), 7, 4, outof.ptr(), 3, 0, 3, 2, 35, _sp()))
        _lib.check(L().eemop_shuffle_channels(x.data_ptr(), sh.ptr(), 2, 6, 3, 35, 0, _sp()))
        _lib.check(L().eemop_shuffle_channels(x.data_ptr(), ush.ptr(), 2, 6, 3, 35, 1, _sp()))
        _lib.check(L().eemop_replicate_pad(x.data_ptr(), pad.ptr(), 12, 5, 7, 1, 2, 3, 0, _sp()))
        return {"into": into.cpu(), "outof": outof.cpu(), "shuffle": sh.cpu(), "unshuffle": ush.cpu(), "pad": pad.cpu()}
    _add("copies_and_shuffle", build, ref, run)


def _build_cases():
    for kind in (B.GACT_RELU, B.GACT_SIGMOID, B.GACT_TANH, B.GACT_LEAKY, B.GACT_NONE):
        _act_fwd(kind)
        _act_bwd(kind)
    for kind in range(5):
        for which in ((0, 1) if kind != 4 else (0,)):
            _binary(kind, which)
    _sum_n(True)
    _sum_n(False)
    _gru()
    for hw, relu, res in ((437, 0, 0), (437, 1, 0), (437, 1, 1), (437, 1, 2), (16384, 1, 0)):
        _instnorm_fwd(hw, relu, res)
    for hw, relu in ((437, 0), (437, 1), (16384, 1)):
        _instnorm_bwd(hw, relu)
    for n, c, hw in (B.OB_BN_CASES[0], B.OB_BN_CASES[2]):        # (3, 3, 357): t256; (1, 2, 16384): t1024
        for relu in (0, 1):
            _bn_train_fwd(n, c, hw, relu)
            _bn_eval_fwd(n, c, hw, relu)
            _bn_bwd(n, c, hw, relu, True)
            _bn_bwd(n, c, hw, relu, False)
    _pyramid(0)
    _pyramid(1)
    _lookup()
    _convex("mask")
    _convex("flow")
    _pool2(False)
    _pool2(True)
    _resize((6, 8), (48, 64), "resize_ac")
    _resize((9, 11), (4, 5), "resize_ac")
    _resize((6, 8), (48, 64), "resize_ac_bwd_gather")
    _resize((6, 8), (48, 64), "resize_ac_bwd_scatter")
    for mode in (0, 1, 2):
        _warp(mode, False)
        _warp(mode, True)
    _upflow()
    _corr53(False)
    _corr53(True)
    _copies()


_build_cases()
BITWISE = {"copies_and_shuffle"}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_operator(monkeypatch, case):
    OB._pin(monkeypatch, case.env)
    clean_in, bad_in = case.build()
    ref = case.ref(bad_in)
    got = case.run(bad_in)
    if case.form:
        OB.ran(case.form)
    clean = case.run(clean_in)
    _check(case.name, got, ref, clean, atomic=case.atomic)
    if case.name in BITWISE:
        for name in got:
            B.check_bitwise(f"{case.name}.{name}", got[name], ref[name])
