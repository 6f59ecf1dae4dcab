"""Every EEMFlow training backward stage against the fp64 adjoint of THAT operation on the GPU's own tensors (oracle/fp64_bounds.py),
kernel form by kernel form.  Each case runs one training forward + backward, reads every gradient buffer (eemflow_get_stage("g_..."))
and the activations it was computed from, and scores the error per element as z = (got - ref) / (2^-24 sum|terms|), so a fault
confined to one tile, one K step, one parity class or one border is seen where it is instead of in the flat gradient's max norm.
Needs a real MI355X: `pytest -m gpu`.

Stage -> its reference (the upstream gradient is the GPU's own buffer; "gate" = LeakyReLU' of the GPU's stored output):
  g_flow    <- flow, gt, valid: sign(flow - gt) valid / (B 2 H W), bitwise (EEMFlowTrainer.step case)
  g_coarse  <- d flow (the seeded Gaussian, or g_flow): the bilinear adjoint                            ups_bwd
  g_flowcat <- g_coarse, out_conv; g_t32_k <- g_flowcat (conv7); g_t64_k <- g_t32_k * gate(t32_k) (conv6); g_td_k <- conv5;
  g_tc_k / g_tb_k / g_ta_k <- the grouped conv4 / conv3 / conv2 in the buffers' shuffled layout; g_cat_k <- conv1         tail_dgrad
  g_pool_k  <- the corr adjoint of g_cat_k[:53] (+ rconv's data gradient from g_cat_k[53:] in the first volume's half)    corr_bwd
  g_f13     <- g_pool_3 through the 8 x 8 pooling adjoint, gated by f13                                                pool_bwd
  g_b3, g_a3, g_b2, g_a2, g_a1 <- conv^T of the next layer's g_, gated by the tensor itself            dgrad_wino4 / wino2 / direct
  g_f12, g_f11 <- conv^T (stride 2) + the pooling branch of g_pool_2 / g_pool_1, gated                       dgrad_s2 / dgrad_gconv
  every weight and bias of the flat gradient <- its layer's input activation and gated output gradient
                                                        wgrad_bx3 / wgrad_fp32 / wgrad_ring / wgrad_tail / wgrad_batched
  padded    <- the inputs, replicate-padded: bitwise
Each case asserts the kernel every layer took (EEMFlow.backward_forms) against `expected_forms`, a mirror of the dispatch predicates in
train_api.hip, wgrad_enc.hip, wgrad_ring.hip, wgrad_tail.hip, dgrad_s2.hip and train.hip, so a switch that silently falls back fails.

Left out, and why: EEM_NO_WGRAD_FEW (wgrad_few_kernel serves the autograd operators of E-RAFT / EEMFlow+, which test_gpu_bwd_ops.py
covers; no EEMFlow backward launch reaches it - the case that sets it asserts the forms did not move); the once-per-process switches
(EEM_WALK3_TRAIN, EEM_WGRAD_LAST_SIDE, EEM_TRAIN_SIDE_PREP, EEM_NO_PREPAD_FWD, EEM_WGRAD_BX3_MT1: batch 1 against batch >= 2 covers
both tile walks); the optimizer step.

Measured on an MI355X (seeds as committed; the weight and bias gradients are summed by fp32 atomics in an order that changes from run to
run, so the worst value of each family is taken over four runs of every case -> the limit in oracle/fp64_bounds.py, by the forward's
rule: max|z| 2x and rms(z) 1.5x, rounded down to two digits, |mean z| and the slope 2x, rounded up; the slope counts from 256 values):

    family          max|z|          rms(z)          |mean z|           |slope| / u        worst max|z| at
    wgrad_bx3        6.27 ->  12    1.00  -> 1.4    0.297  -> 0.6      1.17  -> 2.4       pconv2_3 weight, 70x100 b3
    wgrad_fp32       4.79 ->   9.5  0.695 -> 1.0    0.264  -> 0.53     0.801 -> 1.7       pconv2_3 weight, 70x100 b3 fp32 form
    wgrad_ring       4.65 ->   9.2  0.605 -> 0.9    0.176  -> 0.36     0.403 -> 0.81      pconv3_3 weight, MVSEC b4 rings
    wgrad_tail      13.1  ->  26    1.19  -> 1.7    0.689  -> 1.4      1.21  -> 2.5       decoder_2.conv2 weight, 720x1280
    wgrad_batched    5.87 ->  11    0.910 -> 1.3    0.286  -> 0.58     0.129 -> 0.26      pconv3_2 weight (generic), 92x72 padded
    dgrad_wino4    161    -> 320    3.61  -> 5.4    0.0172 -> 0.035    0.899 -> 1.8       g_a3 (C = 64), MVSEC b4
    dgrad_wino2      5.92 ->  11    0.466 -> 0.69   0.0061 -> 0.013    0.078 -> 0.16      g_b3, 128x192 b1
    dgrad_direct     8.38 ->  16    0.682 -> 1.0    0.0098 -> 0.02     0.646 -> 1.3       g_b2, 92x72 padded
    dgrad_s2         7.53 ->  15    0.637 -> 0.95   0.0029 -> 0.0058   0.031 -> 0.063     g_f11, 720x1280
    dgrad_gconv      5.71 ->  11    0.513 -> 0.76   0.0013 -> 0.0027   0.015 -> 0.031     g_f11, 128x192 b1 EEM_NO_DGRAD_S2
    tail_dgrad       3.80 ->   7.6  0.740 -> 1.1    0.146  -> 0.3      0.288 -> 0.58      g_td_1, 92x72 padded (1x1 grid)
    pool_bwd         0.95 ->   1.8  0.304 -> 0.45   0.0082 -> 0.017    0.0011 -> 0.0023   g_f13, 70x100 b3
    corr_bwd         3.45 ->   6.8  0.667 -> 1.0    0.092  -> 0.19     0.169 -> 0.34      g_pool_2 (events2), 720x1280
    ups_bwd          0.54 ->   1.0  0.180 -> 0.27   0.0171 -> 0.035    0.697 -> 1.4       g_coarse, 70x100 b3 (trainer)

No stage showed an error outside fp32 rounding: no kernel changed.  The module adds about 30 s to `pytest -m gpu` (measured alone: 25 tests
in 31 s, 22 s of it the first test's setup - the library and device initialisation the rest of the suite pays anyway - and 10 s in a
second run; the cases take 0.1 to 3 s each, the 720x1280 one the longest).
"""
import pytest
import torch

from eemflow_amd import EEMFlow, _lib
from eemflow_amd.train import EEMFlowTrainer
from eemflow_amd.weights import seeded_state_dict, synthetic_gt, synthetic_voxel_pair
from oracle import eemflow_oracle as O
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SWITCHES = ("EEM_NO_WGRAD_STREAM", "EEM_NO_WGRAD_BX3", "EEM_WGRAD_RING", "EEM_WGRAD_RING_BLOCK", "EEM_NO_WGRAD_RING", "EEM_WINO",
            "EEM_WINO4_LAYERS", "EEM_NO_DGRAD_S2", "EEM_NO_WGRAD_TAIL", "EEM_NO_WGRAD_SMALL", "EEM_NO_WGRAD_FEW", "EEM_NO_WGRAD_ENC",
            "EEM_UPBWD_THREADS", "EEM_DEC_WNC")
# layer, its input activation, the g_ buffer of its output (gradient w.r.t. its pre-activation), stride
ENC = [("pconv3_3", "b3", "g_f13", 1), ("pconv3_2", "a3", "g_b3", 1), ("pconv3_1", "f12", "g_a3", 2), ("pconv2_3", "b2", "g_f12", 1),
       ("pconv2_2", "a2", "g_b2", 1), ("pconv2_1", "f11", "g_a2", 2), ("pconv1_2", "a1", "g_f11", 1), ("pconv1_1", "padded", "g_a1", 2)]
WG_FAMILY = {"enc_bx3": "wgrad_bx3", "enc_fp32": "wgrad_fp32", "ring": "wgrad_ring", "wgrad_tail": "wgrad_tail", "small": "wgrad_batched",
             "generic": "wgrad_batched"}


def conv_out(n):
    return (n - 1) // 2 + 1


def shapes(b, hp, wp, out_hw):
    h1, w1 = conv_out(hp), conv_out(wp)
    h2, w2 = conv_out(h1), conv_out(w1)
    h3, w3 = conv_out(h2), conv_out(w2)
    return {"b": b, "hp": hp, "wp": wp, "h1": h1, "w1": w1, "h2": h2, "w2": w2, "h3": h3, "w3": w3, "gh": h1 // 32, "gw": w1 // 32,
            "out": out_hw}


def _small_ok(env, jobs, h, w, k):
    """train.hip tr_wgrad_launch_batch: whole images per 128-pixel tile when two fit and the LDS does ((cout, cin) per job)."""
    if env.get("EEM_NO_WGRAD_SMALL") == "1" or 2 * h * w > 128:
        return False
    ipt, pl = 128 // (h * w), (h + 2 * (k // 2)) * (w + 2 * (k // 2))
    lb = max(((co + 31) // 32 * 32 * 129 + min(ci, 32) * ipt * pl + 128) * 4 for co, ci in jobs)
    return lb <= 160 * 1024


def expected_forms(env, s, groups, cin0, fif=1):
    """The kernel form of every layer's gradients under these switches (the mirror of the backward's dispatch)."""
    b = s["b"]
    gh, gw = s["gh"], s["gw"]
    f = {"upsample.bwd": "rows" if 64 <= s["out"][1] <= 8192 and env.get("EEM_UPBWD_THREADS") != "1" else "threads",
         "corr.bwd": "corrbwd"}
    per = 100 // groups
    tail_jobs = {"out_conv": [(2, 6)], "conv7": [(2, 32)] * 3, "conv6": [(32, 64)] * 3, "conv5": [(64, 100)] * 3,
                 "conv4": [(per, per)] * 3 * groups, "conv3": [(per, per)] * 3 * groups, "conv2": [(per, per)] * 3 * groups,
                 "conv1": [(100, 69)] * 3, "rconv": [(16, 16), (16, 32), (16, 64)]}
    one_launch = env.get("EEM_NO_WGRAD_TAIL") != "1" and gh * gw <= 256
    for layer, jobs in tail_jobs.items():
        k = 1 if layer == "out_conv" else 3
        f[f"{layer}.dgrad"] = "tail_conv"
        if one_launch and k == 3:
            f[f"{layer}.wgrad"] = "wgrad_tail"
        else:
            f[f"{layer}.wgrad"] = "small" if _small_ok(env, jobs, gh, gw, k) else "generic"
    dims = {"padded": (cin0, s["hp"], s["wp"]), "a1": (16, s["h1"], s["w1"]), "f11": (16, s["h1"], s["w1"]), "a2": (32, s["h2"], s["w2"]),
            "b2": (32, s["h2"], s["w2"]), "f12": (32, s["h2"], s["w2"]), "a3": (64, s["h3"], s["w3"]), "b3": (64, s["h3"], s["w3"]),
            "f13": (64, s["h3"], s["w3"])}
    out_of = {"pconv3_3": "f13", "pconv3_2": "b3", "pconv3_1": "a3", "pconv2_3": "f12", "pconv2_2": "b2", "pconv2_1": "a2",
              "pconv1_2": "f11", "pconv1_1": "a1"}
    ring = env.get("EEM_WGRAD_RING")
    for layer, xin, _, stride in ENC:
        cin, hin, win = dims[xin]
        cout, hout, wout = dims[out_of[layer]]
        aligned = win % 4 == 0 and wout % 4 == 0 and (hin * win) % 4 == 0 and (hout * wout) % 4 == 0
        ring_ok = env.get("EEM_NO_WGRAD_RING") != "1" and aligned and cin >= 16 and cout >= 16
        ring_pref = ring.startswith("a") if ring else stride == 2 and cin >= 64
        tw32 = wout % 32 == 0 or wout >= 256
        enc_ok = env.get("EEM_NO_WGRAD_ENC") != "1" and aligned and (cin <= 16 or cin % 16 == 0)
        bx3 = env.get("EEM_NO_WGRAD_BX3") != "1"
        if ring_ok and ring_pref:
            blk = env.get("EEM_WGRAD_RING_BLOCK")
            if stride == 1 and blk in ("6464", "3232", "1616"):
                form = f"ring_{blk}"
            elif stride == 2:
                form = "ring_s2_3216" if cout <= 32 and cin <= 16 else "ring_s2_6432" if cout <= 64 and cin <= 32 else "ring_s2_6464"
            else:
                form = "ring_1616" if cout <= 16 and cin <= 16 else "ring_3232" if cout <= 32 and cin <= 32 else "ring_6464"
        elif enc_ok:
            if stride == 2 and cout == 16 and cin <= 5 and tw32:
                form = "enc_fp32_tw32_c5"
            else:
                form = f"enc_{'bx3' if cout >= 32 and bx3 else 'fp32'}_tw{32 if tw32 else 16}"
        else:
            form = "small" if stride == 1 and _small_ok(env, [(cout, cin)], hout, wout, 3) else "generic"
        f[f"{layer}.wgrad"] = form
        if layer == "pconv1_1":
            continue
        if stride == 1:
            if env.get("EEM_WINO") != "0" and wout % 4 == 0:
                mask = 0 if env.get("EEM_WINO") == "2" else int(env["EEM_WINO4_LAYERS"]) & 7 if "EEM_WINO4_LAYERS" in env else \
                    (7 if fif >= 3 or b >= 4 else 1)
                f[f"{layer}.dgrad"] = "wino4" if (mask >> {16: 0, 32: 1, 64: 2}[cin]) & 1 else "wino2"
            else:
                f[f"{layer}.dgrad"] = "direct"
        else:
            s2 = env.get("EEM_NO_DGRAD_S2") != "1" and wout % 4 == 0 and win % 2 == 0 and hout == (hin + 1) // 2 and wout == (win + 1) // 2
            f[f"{layer}.dgrad"] = "dgrad_s2" if s2 else "gconv"
            if not s2:
                k, w_ = (16, s["w2"]) if layer == "pconv3_1" else (32, s["w1"])
                f[f"pool_{'2' if layer == 'pconv3_1' else '1'}.bwd"] = "poolbwd4" if w_ % 4 == 0 and k % 4 == 0 else "poolbwd"
    f["pool_3.bwd"] = "poolbwd4" if s["w3"] % 4 == 0 else "poolbwd"
    return f


def wg_family(form):
    return next(v for k, v in WG_FAMILY.items() if form.startswith(k))


def dg_family(form):
    return {"wino4": "dgrad_wino4", "wino2": "dgrad_wino2", "direct": "dgrad_direct", "dgrad_s2": "dgrad_s2", "gconv": "dgrad_gconv"}[form]


def pin(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def make_net(seed, size, groups=5, cin0=5, mesh=False):
    sd = seeded_state_dict(seed, n_first_channels=cin0, groups=groups)
    net = EEMFlow("", groups=groups, n_first_channels=cin0, out_mesh_size=mesh)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(DEV).train()
    net.change_imagesize(size)
    return net, O.to_torch_sd(sd)


def check_w(tag, grads, name, ref, family):
    """weight and bias of one conv: ref = (dW, mag, db, mag)"""
    dw, mw, db, mb = ref
    B.check(f"{tag} d {name}.weight", grads[f"{name}.weight"], dw, mw, family)
    B.check(f"{tag} d {name}.bias", grads[f"{name}.bias"], db, mb, family)


def tail_key(k, layer):
    if layer == "rconv":
        return f"rconv_{k}.0"
    if layer == "conv7":
        return f"decoder_{k}.conv7"
    return f"decoder_{k}.{layer}.0"


def check_case(net, sd, grads, forms, e1, e2, dflow, s, groups, tag, parts):
    b, gh, gw = s["b"], s["gh"], s["gw"]
    per = 100 // groups
    cache = {}

    def st(name):
        if name not in cache:
            cache[name] = net.stage(name).cpu()
        return cache[name]

    if "ups" in parts:
        ref, mag = B.upsample_bwd_ref(dflow, (gh, gw))
        B.check(f"{tag} g_coarse", st("g_coarse"), ref, mag, "ups_bwd")
    if "tail_d" in parts:
        ref, mag = B.conv_dgrad_ref(st("g_coarse"), sd["out_conv.weight"], (gh, gw), padding=0)
        B.check(f"{tag} g_flowcat", st("g_flowcat"), ref, mag, "tail_dgrad")
    if "tail_w" in parts:
        check_w(tag, grads, "out_conv", B.conv_wgrad_ref(st("flowcat"), st("g_coarse"), sd["out_conv.weight"].shape, padding=0),
                wg_family(forms["out_conv.wgrad"]))
    for k in (1, 2, 3) if "tail_d" in parts or "tail_w" in parts else ():
        # conv j reads x_in, writes (through its LeakyReLU, conv7 without) the tensor whose gradient buffer is g_out; the grouped layers'
        # outputs are stored channel-shuffled, so their gated gradients go back to the conv's own channel order first
        chain = [("t32", "conv7", None, st("g_flowcat")[:, 2 * k - 2:2 * k], 1), ("t64", "conv6", "t32", None, 1),
                 ("td", "conv5", "t64", None, 1), ("tc", "conv4", "td", None, groups), ("tb", "conv3", "tc", None, groups),
                 ("ta", "conv2", "tb", None, groups), ("cat", "conv1", "ta", None, 1)]
        for xin, layer, yout, gy, g in chain:
            wkey = tail_key(k, layer) + ".weight"
            dy = B._d(gy) if yout is None else B._d(st(f"g_{yout}_{k}")) * B.gate(st(f"{yout}_{k}"))
            if g > 1:
                dy = B.shuffle(dy, per)
            if "tail_d" in parts:
                ref, mag = B.conv_dgrad_ref(dy, sd[wkey], (gh, gw), groups=g)
                B.check(f"{tag} g_{xin}_{k}", st(f"g_{xin}_{k}"), ref, mag, "tail_dgrad")
            if "tail_w" in parts:
                check_w(tag, grads, tail_key(k, layer), B.conv_wgrad_ref(st(f"{xin}_{k}"), dy, sd[wkey].shape, groups=g),
                        wg_family(forms[f"{layer}.wgrad"]))
        # rconv_k: the first volume's pooled features -> channels 53.. of cat_k; the correlation reads both volumes' pool_k
        p = st(f"pool_{k}")
        dy = B._d(st(f"g_cat_{k}"))[:, 53:] * B.gate(st(f"cat_{k}")[:, 53:])
        if "tail_w" in parts:
            check_w(tag, grads, f"rconv_{k}.0", B.conv_wgrad_ref(p[:b], dy, sd[f"rconv_{k}.0.weight"].shape),
                    wg_family(forms["rconv.wgrad"]))
        if "tail_d" in parts:
            rr, rm = B.conv_dgrad_ref(dy, sd[f"rconv_{k}.0.weight"], (gh, gw))
            (dx, mx), (dyy, my) = B.corr_bwd_ref(st(f"g_cat_{k}")[:, :53], p[:b], p[b:])
            gp = st(f"g_pool_{k}")
            B.check(f"{tag} g_pool_{k} (events1)", gp[:b], rr + dx, rm + mx, "corr_bwd")
            B.check(f"{tag} g_pool_{k} (events2)", gp[b:], dyy, my, "corr_bwd")
    if "enc_d" in parts:
        ref, mag = B.pool_bwd_ref(st("g_pool_3"), (s["h3"], s["w3"]), 8)
        gx = B.gate(st("f13"))
        B.check(f"{tag} g_f13", st("g_f13"), ref * gx, mag * gx, "pool_bwd")
        for layer, xin, gy, stride in ENC[:-1]:
            w = sd[f"{layer}.0.weight"]
            if stride == 1:
                ref, mag = B.conv_dgrad_ref(st(gy), w, st(xin).shape[-2:], x_gate=st(xin))
            else:
                k, pk = (2, 16) if layer == "pconv3_1" else (1, 32)
                ref, mag = B.stage_dgrad_ref(st(gy), w, st(xin), st(f"g_pool_{k}"), pk)
            B.check(f"{tag} g_{xin}", st(f"g_{xin}"), ref, mag, dg_family(forms[f"{layer}.dgrad"]))
    if "enc_w" in parts:
        for layer, xin, gy, stride in ENC:
            check_w(tag, grads, f"{layer}.0", B.conv_wgrad_ref(st(xin), st(gy), sd[f"{layer}.0.weight"].shape, stride=stride),
                    wg_family(forms[f"{layer}.wgrad"]))
        pad = O.input_padder_pad(*net.image_size)
        want = O.replicate_pad(torch.cat([e1, e2]), pad)
        assert torch.equal(st("padded"), want), f"{tag}: padded is not the replicate-padded inputs"


ALL = ("ups", "tail_d", "tail_w", "enc_d", "enc_w")


def run_case(monkeypatch, env, b, h, w, seed, size=None, groups=5, cin0=5, mesh=False, trainer=False, parts=ALL, moves=True):
    """One training step under `env`; every stage of `parts` against fp64.  moves: the switches change some layer's form (EEM_NO_WGRAD_STREAM
    moves launches between streams, EEM_DEC_WNC the forward's decoder kernel, EEM_NO_WGRAD_FEW nothing the EEMFlow backward reaches)."""
    pin(monkeypatch, env)
    net, sd = make_net(seed, size or (h, w), groups, cin0, mesh)
    e1, e2 = (torch.from_numpy(a) for a in synthetic_voxel_pair(seed + 1, b, h, w, bins=cin0))
    d1, d2 = e1.to(DEV), e2.to(DEV)
    oh, ow = (16, 16) if mesh else (h, w)
    if trainer:
        gt, valid = (torch.from_numpy(a) for a in synthetic_gt(seed + 2, b, oh, ow))
        tr = EEMFlowTrainer(net, lr=0.0, wdecay=0.0, clip=0.0)     # lr 0: the step leaves the weights unchanged
        _, _, flow = tr.step(d1, d2, gt.to(DEV), valid.to(DEV))
        torch.cuda.synchronize()
        flat = tr.grad.cpu()
        dflow = net.stage("g_flow").cpu()
        ref = B.loss_grad_ref(flow.cpu(), gt, valid)
        assert torch.equal(dflow, ref), f"g_flow differs from sign(flow - gt) valid / (B 2 H W) at {int((dflow != ref).sum())} values"
        grads, off = {}, 0
        for k, v in sd.items():
            grads[k] = flat[off:off + v.numel()].view_as(v)
            off += v.numel()
    else:
        for p in net.parameters():
            p.grad = None
        flow = net(d1, d2)[1][0]
        dflow = torch.randn(flow.shape, generator=torch.Generator().manual_seed(seed + 3)).to(DEV)
        flow.backward(dflow)
        torch.cuda.synchronize()
        dflow = dflow.cpu()
        grads = {k: p.grad.cpu() for k, p in net.named_parameters()}
    hp, wp = net.stage("padded").shape[-2:]
    s = shapes(b, hp, wp, (oh, ow))
    want = expected_forms(env, s, groups, cin0)
    got = net.backward_forms()
    assert not env or (want != expected_forms({}, s, groups, cin0)) == moves, f"{env}: the case's switches {'move no' if moves else 'move a'} form"
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    tag = f"{h}x{w} b{b} g{groups} c{cin0}{' mesh' if mesh else ''}{' trainer' if trainer else ''} {env}"
    check_case(net, sd, grads, got, e1, e2, dflow, s, groups, tag, parts)
    return got


MVSEC, SMALL, HD = (260, 346), (128, 192), (720, 1280)
ENC_W = ("enc_w",)
TAIL = ("tail_d", "tail_w")
CASES = [
    # id, env, batch, h, w, kwargs
    ("default-70x100", {}, 3, 70, 100, {}),
    ("trainer-70x100", {}, 3, 70, 100, {"trainer": True}),
    ("no_stream_fp32-70x100", {"EEM_NO_WGRAD_STREAM": "1", "EEM_NO_WGRAD_BX3": "1"}, 3, 70, 100, {"parts": ENC_W + ("tail_w",)}),
    ("no_stream-70x100", {"EEM_NO_WGRAD_STREAM": "1"}, 3, 70, 100, {"parts": ENC_W + ("tail_w",), "moves": False}),
    ("default-mvsec", {}, 4, *MVSEC, {}),
    ("ring_all-mvsec", {"EEM_WGRAD_RING": "all"}, 4, *MVSEC, {"parts": ENC_W}),
    ("ring_3232-mvsec", {"EEM_WGRAD_RING": "all", "EEM_WGRAD_RING_BLOCK": "3232"}, 4, *MVSEC, {"parts": ENC_W}),
    ("ring_1616-mvsec", {"EEM_WGRAD_RING": "all", "EEM_WGRAD_RING_BLOCK": "1616"}, 4, *MVSEC, {"parts": ENC_W}),
    ("default-b1", {}, 1, *SMALL, {}),
    ("wino2-b1", {"EEM_WINO": "2"}, 1, *SMALL, {"parts": ("enc_d",)}),
    ("direct_gconv-b1", {"EEM_WINO": "0", "EEM_NO_DGRAD_S2": "1"}, 1, *SMALL, {"parts": ("enc_d",)}),
    ("ragged-64x64", {}, 2, 64, 64, {"size": (100, 120)}),
    ("groups4-200x300", {}, 3, 200, 300, {"groups": 4, "parts": TAIL}),
    ("groups1", {}, 2, *SMALL, {"groups": 1, "parts": TAIL}),
    ("groups2", {}, 2, *SMALL, {"groups": 2, "parts": TAIL}),
    ("cin3", {}, 2, *SMALL, {"cin0": 3, "parts": ("enc_d", "enc_w")}),
    ("cin7", {}, 2, *SMALL, {"cin0": 7, "parts": ("enc_d", "enc_w")}),
    ("no_tail", {"EEM_NO_WGRAD_TAIL": "1"}, 2, *SMALL, {"parts": ("tail_w",)}),
    ("no_tail_small", {"EEM_NO_WGRAD_TAIL": "1", "EEM_NO_WGRAD_SMALL": "1"}, 2, *SMALL, {"parts": ("tail_w",)}),
    ("no_tail_small_few", {"EEM_NO_WGRAD_TAIL": "1", "EEM_NO_WGRAD_SMALL": "1", "EEM_NO_WGRAD_FEW": "1"}, 2, *SMALL, {"parts": ("tail_w",)}),
    ("upbwd_threads", {"EEM_UPBWD_THREADS": "1"}, 2, *SMALL, {"parts": ("ups",)}),
    ("dec_wnc-256", {"EEM_DEC_WNC": "1"}, 4, 256, 256, {"parts": TAIL, "moves": False}),
    ("mesh-128", {}, 2, 128, 128, {"mesh": True, "parts": ("ups", "tail_d")}),
    ("headline-720x1280", {}, 1, *HD, {}),
]


@pytest.mark.parametrize("env,b,h,w,kw", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_backward_stages_against_fp64(monkeypatch, env, b, h, w, kw):
    run_case(monkeypatch, env, b, h, w, seed=40 + b + h % 7, **kw)


def test_upsample_backward_rows_of_more_than_64_kb(monkeypatch):
    """An output width of 4100 is the first whose row form stages more than 64 KB of LDS (4 waves x 4100 floats): the launch has to raise
    the kernel's limit first.  Both forms against fp64 under the `ups_bwd` limits, as the `upbwd_threads` case compares them, and
    against each other: they add the same <= 4 products per column in another order and the same two rows, 16 u of the adjoint of |d|
    covers both sums' rounding (3 u each in x, and the y pass on inputs that differ by that)."""
    nc, oh, ow, h, w = 1, 2, 4100, 1, 2050
    d = torch.randn(1, nc, oh, ow, generator=torch.Generator().manual_seed(77))
    dd = d.to(DEV)
    got = {}
    for form, env in (("rows", {}), ("threads", {"EEM_UPBWD_THREADS": "1"})):
        pin(monkeypatch, env)
        tmp, out = torch.empty(nc, oh, w, device=DEV), torch.empty(1, nc, h, w, device=DEV)
        _lib.check(_lib.lib().eemflow_upsample_bilinear_bwd(dd.data_ptr(), tmp.data_ptr(), out.data_ptr(), nc, oh, ow, h, w,
                                                            _lib.current_stream_ptr(dd.device)))
        got[form] = out.cpu()
    ref, mag = B.upsample_bwd_ref(d, (h, w))
    for form, out in got.items():
        B.check(f"upsample.bwd {form} {oh}x{ow} -> {h}x{w}", out, ref, mag, "ups_bwd", form=form)
    diff = (got["rows"].double() - got["threads"].double()).abs()
    bound = 16 * B.U * mag / (1 + h + w)
    print("rows against threads: max |d| %.3e, worst d / bound %.3f" % (float(diff.max()), float((diff / bound).max())))
    assert float(ref.abs().max()) > 1.0 and bool((diff <= bound).all())


def test_gradient_buffers_refuse_when_stale(monkeypatch):
    """g_ buffers are readable only after a backward of the CURRENT training forward; the training activations only while the workspace
    holds that forward."""
    pin(monkeypatch, {})
    net, _ = make_net(5, SMALL)
    e1, e2 = (torch.from_numpy(a).to(DEV) for a in synthetic_voxel_pair(6, 1, *SMALL))
    with torch.no_grad():
        net.eval()
        net(e1, e2)
    for name in ("g_a1", "g_coarse", "td_2", "padded"):
        with pytest.raises(_lib.EEMFlowHipError, match="training"):
            net.stage(name)                                   # an inference forward, and no training one yet
    net.train()
    flow = net(e1, e2)[1][0]
    with pytest.raises(_lib.EEMFlowHipError, match="stale"):
        net.stage("g_a1")                                     # training forward, no backward yet
    assert net.stage("ta_1").shape == (1, 100, 2, 3)
    flow.backward(torch.ones_like(flow))
    assert net.stage("g_a1").shape == (2, 16, 64, 96)
    with pytest.raises(_lib.EEMFlowHipError, match="g_flow"):
        net.stage("g_flow")                                   # (eemflow_backward: the caller's d flow, not a loss kernel's)
    with torch.no_grad():
        net.eval()
        net(e1, e2)
    for name in ("g_a1", "g_pool_1", "ta_1", "padded"):
        with pytest.raises(_lib.EEMFlowHipError, match="training"):
            net.stage(name)
    net.train()
    flow = net(e1, e2)[1][0]                                  # a new training forward: the old backward's buffers are stale
    with pytest.raises(_lib.EEMFlowHipError, match="stale"):
        net.stage("g_f13")
