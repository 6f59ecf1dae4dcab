"""Every EEMFlow inference stage against an fp64 evaluation of THAT stage on the GPU's own input to it (oracle/fp64_bounds.py), kernel
form by kernel form, in every launch configuration that changes the tile walk or the grid, at sizes whose tiles are cut by the right
and bottom edges.  The error is z = (got - ref) / (2^-24 sum|terms|) per element: a few units for correct fp32 arithmetic, so one
wrong tile is seen at the tile (the flow alone divides it by the 32 x 32 pooling).  Needs a real MI355X: `pytest -m gpu`.

Stage -> what its fp64 reference is computed from: a1 <- the replicate-padded input (normalised from the voxelizer's record in the
deferred form); f11 <- a1; a2 <- f11; b2 <- a2; f12 <- b2; a3 <- f12; b3 <- a3; f13 <- b3; pool_k <- f1k; cat_k = [cv | r] <- the
two volumes' pool_k / the first volume's pool_k; flowcat <- cat_k (decoder criterion: the GPU's error at most KAPPA_DEC x the fp32 CPU
oracle's); coarse <- flowcat; flow <- coarse.  Before each checked forward, `eemflow_time_kernels` lists the launches of the same
configuration and the test asserts that the intended form ran (its `pipe` field: 0 fp32 MFMA, 1 bf16 pieces, 2 F(4x4), 3 F(2x2); the
fused first layers by name; the decoders' Winograd conv1 by pipe 3), so a dispatch fallback cannot test another kernel.

Sizes (input -> padded -> 1/2, 1/4, 1/8): 260x346 -> 320x384 -> 160x192 / 80x96 / 40x48 (MVSEC: 1.5 F(4x4) tiles wide at C = 32,
2.5 tile rows at 1/8, replicate padding 19 px left and right); 480x640 -> 512x640 (2.5 tiles wide at 1/2); 130x70 -> 192x128 (24x16
at 1/8); 64x64 (8x8 at 1/8: smaller than any tile); 720x1280 (headline, a few cases).

Left out, and why: the stride-2 and fused / deferred first-layer forms at batch > 1 (the stride-2 kernels take one tile per block at
any batch; pconv1_1's contiguous ranges and the stride-1 kernels' interleaved walk DO depend on the batch and on the in-flight grids -
tests/test_tile_walk_host.py proves the dealing on the host, tests/test_gpu_walk_batched.py runs the batches and settings at which
blocks take two, three and four tiles; this module's batches 3, 4, 10 and 16 give the interleaved walk one tile per block except at
720x1280); F(2x2) and the direct forms at 720x1280 (the same tiles as at 480x640, whose width is not a tile multiple); every image of
the 720x1280 batches (the fp64 references cost ~1 s per image there: the first and the last frame are checked); `forward_stream`'s
own stages (after a stream call the workspace holds windows, not pairs, and eemflow_get_stage refuses - its flows are compared
bitwise with a forward_many whose stages are all checked here).

Measured on an MI355X (seeds as committed, bitwise repeatable; the worst value over all cases of the family -> the limit in
oracle/fp64_bounds.py):

    family     max|z|          rms(z)         |mean z|       |slope| / u     worst max|z| at
    enc1        4.96 ->   9.9  0.366 -> 0.54  0.071 -> 0.15  0.36 -> 0.72
    direct     10.3  ->  20    0.658 -> 0.98  0.107 -> 0.22  0.92 -> 1.9    f12 (EEM_WINO=0); rconv 3.35
    bx3         7.23 ->  14    0.458 -> 0.68  0.074 -> 0.15  1.16 -> 2.4    a2
    wino2       4.47 ->   8.9  0.316 -> 0.47  0.020 -> 0.04  0.28 -> 0.56
    wino4     217    -> 430    2.12  -> 3.1   0.088 -> 0.18  1.14 -> 2.3    f11 (C = 16); C = 32: 157, C = 64: 93
    pool        3.53 ->   7.0  0.844 -> 1.2   0.139 -> 0.28  0.25 -> 0.5
    corr        3.82 ->   7.6  0.792 -> 1.1   0.035 -> 0.07  1.87 -> 3.8
    out_conv    2.47 ->   4.9  0.779 -> 1.1   0.168 -> 0.34  0.66 -> 1.4
    upsample   49.9  ->  99    0.728 -> 1.0   0.134 -> 0.27  1.38 -> 2.8
    decoders: GPU error / fp32 CPU oracle error, worst rms ratio 2.76, worst max ratio 3.21 -> KAPPA_DEC 6.4
"""
import ctypes

import numpy as np
import pytest
import torch

from eemflow_amd import EEMFlow, EventSequence, _lib
from eemflow_amd.weights import seeded_state_dict, synthetic_voxel_pair
from oracle import eemflow_oracle as O
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# stage, its input stage, layer, stride, channels out
ENC = [("a1", None, "pconv1_1", 2, 16), ("f11", "a1", "pconv1_2", 1, 16), ("a2", "f11", "pconv2_1", 2, 32),
       ("b2", "a2", "pconv2_2", 1, 32), ("f12", "b2", "pconv2_3", 1, 32), ("a3", "f12", "pconv3_1", 2, 64),
       ("b3", "a3", "pconv3_2", 1, 64), ("f13", "b3", "pconv3_3", 1, 64)]
PIPE = {"enc1": 0, "direct": 0, "bx3": 1, "wino4": 2, "wino2": 3}
TILE = {("wino4", 16): (16, 128), ("wino4", 32): (16, 64), ("wino4", 64): (16, 32), ("wino2", 16): (8, 64), ("wino2", 32): (4, 64),
        ("wino2", 64): (4, 32), ("enc1", 16): (8, 64), ("bx3", 32): (4, 32), ("bx3", 64): (4, 32), ("direct", 16): (4, 32),
        ("direct", 32): (4, 32), ("direct", 64): (4, 32)}

SWITCHES = ("EEM_WINO", "EEM_WINO4_LAYERS", "EEM_NO_ENC1", "EEM_BX3_S1", "EEM_NO_BX3", "EEM_NO_S2W", "EEM_S2R", "EEM_FUSE12",
            "EEM_DEC_WNC", "EEM_NO_TAIL_MULTI")


def forms_of(env, batch, fif):
    """The form every encoder stage takes under these switches (ctx.h f4_mask, schedule.hip bx3_wanted, conv_enc.hip's dispatch)."""
    def s1(c):
        if env.get("EEM_WINO") == "0":
            return "direct"
        if env.get("EEM_WINO") == "2":
            return "wino2"
        mask = int(env["EEM_WINO4_LAYERS"]) if "EEM_WINO4_LAYERS" in env else (7 if fif >= 3 or batch >= 4 else 1)
        return "wino4" if (mask >> {16: 0, 32: 1, 64: 2}[c]) & 1 else "wino2"
    s2 = "direct" if env.get("EEM_S2R") == "1" or env.get("EEM_NO_BX3") == "1" else "bx3"
    bx = int(env.get("EEM_BX3_S1", "0"))
    return {"a1": "enc1", "f11": s1(16), "a2": s2, "b2": "bx3" if bx & 1 else s1(32), "f12": s1(32), "a3": s2,
            "b3": "bx3" if bx & 2 else s1(64), "f13": s1(64)}


def make_net(seed, h, w, graph=True, fif=1):
    sd = seeded_state_dict(seed)
    net = EEMFlow("", groups=5, n_first_channels=5).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.use_graph = graph
    net.frames_in_flight = fif
    net = net.to(DEV)
    net.change_imagesize((h, w))
    return net, O.to_torch_sd(sd)


def pin(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def launches(net, e1, e2, blocks=False):
    """(name, pipe) of every launch of a forward of this batch in the module's configuration (eemflow_time_kernels, one pass);
    blocks=True: (name, pipe, blocks of the launch's grid)."""
    b, _, h, w = e1.shape
    out = torch.empty(b, 2, h, w, device=DEV)
    st = (_lib.KernelStat * 128)()
    n = ctypes.c_int(0)
    ctx = net._context(e1.device)
    _lib.check(_lib.lib().eemflow_time_kernels(ctx, e1.data_ptr(), e2.data_ptr(), b, h, w, out.data_ptr(), h, w, 1, st, 128,
                                               ctypes.byref(n), _lib.current_stream_ptr(e1.device)))
    torch.cuda.synchronize()
    return [(st[i].name.decode(), st[i].pipe) + ((st[i].blocks,) if blocks else ()) for i in range(n.value)]


def assert_forms(ks, forms, env, gw, batch):
    names = [k for k, _ in ks]
    fused = any(k.startswith("enc.pconv1_1+1_2 fused") for k in names)
    assert fused == (env.get("EEM_FUSE12") == "1"), names
    for stage, _, layer, _, _ in ENC:
        hit = [p for k, p in ks if k.startswith(f"enc.{layer} ")]
        if fused and stage in ("a1", "f11"):
            assert not hit, (stage, names)
            continue
        assert len(hit) == 1 and hit[0] == PIPE[forms[stage]], (stage, forms[stage], hit)
    wnc = env.get("EEM_DEC_WNC")
    want = gw % 4 == 0 and (wnc == "1" or (wnc is None and batch >= 4))
    assert [p for k, p in ks if k.startswith("dec.conv1 ")] == [3 if want else 0], (want, names)


def check_stages(net, sd, ev1, ev2, flows, forms, frames, tag, records=None, encoder=True):
    """Every stage of the module's last forward against fp64 (see the module docstring).  ev1 / ev2: that forward's [B,5,H,W] inputs
    (CPU), flows: its [B,2,H,W] flow (CPU); `frames`: the batch entries to check (both event volumes of each)."""
    b, _, h, w = ev1.shape
    imgs = list(frames) + [b + f for f in frames]
    pad = O.input_padder_pad(*net.image_size)
    st = {}

    def get(name):
        if name not in st:
            st[name] = net.stage(name).cpu()
        return st[name]
    if encoder:
        x = torch.cat([ev1, ev2])[imgs]
        rec = [records[i] for i in imgs] if records is not None else None
        ref, mag = B.first_layer_ref(x, pad, sd["pconv1_1.0.weight"], sd["pconv1_1.0.bias"], rec)
        B.check(f"{tag} a1", get("a1")[imgs], ref, mag, forms["a1"], TILE[(forms["a1"], 16)])
        for stage, src, layer, stride, cout in ENC[1:]:
            ref, mag = B.conv_ref(get(src)[imgs], sd[f"{layer}.0.weight"], sd[f"{layer}.0.bias"], stride)
            B.check(f"{tag} {stage}", get(stage)[imgs], ref, mag, forms[stage], TILE[(forms[stage], cout)])
    for k, (f, ps) in enumerate((("f11", 32), ("f12", 16), ("f13", 8)), 1):
        ref, mag = B.avg_pool_ref(get(f)[imgs], ps)
        B.check(f"{tag} pool_{k}", get(f"pool_{k}")[imgs], ref, mag, "pool")
    fl = list(frames)
    fb = [b + i for i in frames]
    dec = []
    for k in (1, 2, 3):
        pool, cat = get(f"pool_{k}"), get(f"cat_{k}")
        ref, mag = B.corr53_ref(pool[fl], pool[fb])
        B.check(f"{tag} cat_{k}.cv", cat[fl, :53], ref, mag, "corr")
        ref, mag = B.conv_ref(pool[fl], sd[f"rconv_{k}.0.weight"], sd[f"rconv_{k}.0.bias"])
        B.check(f"{tag} cat_{k}.r", cat[fl, 53:], ref, mag, "direct")
        r64, r32 = B.decoder_refs(sd, k, cat[fl])
        dec.append((k, r64, r32))
    flowcat = get("flowcat")[fl]
    for k, r64, r32 in dec:
        B.check_decoder(f"{tag} flowcat.{k}", flowcat[:, 2 * (k - 1):2 * k], r64, r32)
    ref, mag = B.out_conv_ref(flowcat, sd["out_conv.weight"], sd["out_conv.bias"])
    B.check(f"{tag} coarse", get("coarse")[fl], ref, mag, "out_conv")
    ref, mag = B.upsample_ref(get("coarse")[fl], (h, w))
    B.check(f"{tag} flow", flows[fl], ref, mag, "upsample")


def run_case(monkeypatch, env, b, h, w, seed, frames=None, graph=True, fif=1, encoder=True):
    pin(monkeypatch, env)
    net, sd = make_net(seed, h, w, graph, fif)
    e1, e2 = (torch.from_numpy(a) for a in synthetic_voxel_pair(seed + 1, b, h, w))
    d1, d2 = e1.to(DEV), e2.to(DEV)
    with torch.no_grad():
        gw = (((w + 63) // 64) * 64 // 2) // 32
        assert_forms(launches(net, d1, d2), forms_of(env, b, fif), env, gw, b)
        flow = net(d1, d2)[1][0].cpu()
    tag = f"{h}x{w} b{b} fif{fif} {'graph' if graph else 'eager'} {env}"
    check_stages(net, sd, e1, e2, flow, forms_of(env, b, fif), range(b) if frames is None else frames, tag, encoder=encoder)


MVSEC, VGA, TALL, TINY, HD = (260, 346), (480, 640), (130, 70), (64, 64), (720, 1280)
FORM_ENVS = {
    "default": {},
    "wino4": {"EEM_WINO4_LAYERS": "7"},
    "wino2": {"EEM_WINO": "2"},
    "direct": {"EEM_WINO": "0", "EEM_NO_ENC1": "1"},
    "bx3_s1": {"EEM_BX3_S1": "3"},
    "s2_light": {"EEM_NO_BX3": "1"},
    "s2_chunked": {"EEM_NO_BX3": "1", "EEM_NO_S2W": "1"},
    "s2_ring": {"EEM_S2R": "1"},
    "fused12": {"EEM_FUSE12": "1"},                         # bottom-only padding: 480x640, 64x64, 720x1280
}
BATCH1 = ([("default", s) for s in (MVSEC, VGA, TALL, TINY, HD)] + [("wino4", s) for s in (MVSEC, VGA, TALL, TINY)] +
          [("wino2", s) for s in (MVSEC, TALL)] + [("direct", s) for s in (MVSEC, TALL, TINY)] + [("bx3_s1", s) for s in (MVSEC, VGA)] +
          [(f, s) for f in ("s2_light", "s2_chunked", "s2_ring") for s in (MVSEC, TALL)] + [("fused12", s) for s in (VGA, TINY, HD)])


@pytest.mark.parametrize("form,size", BATCH1, ids=[f"{f}-{s[0]}x{s[1]}" for f, s in BATCH1])
def test_batch1_forms(monkeypatch, form, size):
    run_case(monkeypatch, FORM_ENVS[form], 1, *size, seed=100 + size[0] % 97)


@pytest.mark.parametrize("size", [MVSEC, TALL])
def test_batch1_eager(monkeypatch, size):
    run_case(monkeypatch, {}, 1, *size, seed=110, graph=False)


BATCHED = [(3, MVSEC, "default"), (3, TALL, "default"), (3, MVSEC, "wino4"), (4, MVSEC, "default"), (4, TALL, "default"),
           (4, VGA, "default"), (5, TALL, "bx3_s1"), (4, TINY, "default")]


@pytest.mark.parametrize("b,size,form", BATCHED, ids=[f"b{b}-{s[0]}x{s[1]}-{f}" for b, s, f in BATCHED])
def test_batched_tile_walk(monkeypatch, b, size, form):
    """Two pairs per launch on: the interleaved walk (reverse = 3) of the stride-1 layers; batch 3 keeps F(2x2) at C = 32 / 64, batch
    >= 4 takes F(4x4) everywhere.  Every image checked (two frames at 480x640)."""
    run_case(monkeypatch, FORM_ENVS[form], b, *size, seed=120 + b, frames=(0, b - 1) if size == VGA else None)


@pytest.mark.parametrize("size,form", [(MVSEC, "default"), (VGA, "default"), (HD, "default"), (MVSEC, "wino2"), (TALL, "default")])
def test_frames_in_flight_4(monkeypatch, size, form):
    """frames_in_flight = 4: fewer persistent blocks per XCD (more tiles each), F(4x4) on every stride-1 layer by default."""
    run_case(monkeypatch, FORM_ENVS[form], 1, *size, seed=130, fif=4)


@pytest.mark.parametrize("n,size", [(10, MVSEC), (16, MVSEC), (10, HD), (16, TALL)])
def test_forward_many_timed_configuration(monkeypatch, n, size):
    """bench.py's configuration: n distinct batch-1 samples per forward_many call, frames_in_flight 2 - F(4x4), the interleaved walk,
    the multi-tile grouped decoder kernel.  Every frame at the small sizes, the first and the last at 720x1280."""
    h, w = size
    pin(monkeypatch, {})
    net, sd = make_net(140 + n, h, w, fif=2)
    pairs = [tuple(torch.from_numpy(a) for a in synthetic_voxel_pair(150 + i, 1, h, w)) for i in range(n)]
    e1, e2 = torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs])
    with torch.no_grad():
        assert_forms(launches(net, e1.to(DEV), e2.to(DEV)), forms_of({}, n, 2), {}, (((w + 63) // 64) * 32) // 32, n)
        dev = [(a.to(DEV), b.to(DEV)) for a, b in pairs]
        outs = net.forward_many(dev)
        flow = torch.cat([o[1][0] for o in outs]).cpu()
    check_stages(net, sd, e1, e2, flow, forms_of({}, n, 2), (0, n - 1) if size == HD else range(n), f"forward_many {n} {h}x{w}")


@pytest.mark.parametrize("size", [MVSEC, VGA])
def test_forward_stream_flows_are_those_of_a_checked_forward_many(monkeypatch, size):
    """forward_stream, with and without a carried window, against a forward_many of the same pairs whose every stage is checked here
    (bitwise: the same kernels).  After a stream call the workspace holds windows, and eemflow_get_stage refuses to read it."""
    h, w = size
    pin(monkeypatch, {"EEM_WINO4_LAYERS": "7", "EEM_DEC_WNC": "1"})      # forms pinned: stream and forward_many batches differ
    net, sd = make_net(160, h, w, fif=2)
    vols = [torch.from_numpy(synthetic_voxel_pair(170 + i, 1, h, w)[0]) for i in range(6)]
    dv = [v.to(DEV) for v in vols]
    with torch.no_grad():
        first = net.forward_stream(dv[:3])                                 # no carried window: 2 pairs
        with pytest.raises(_lib.EEMFlowHipError, match="no forward has run"):
            net.stage("f11")
        second = net.forward_stream(dv[3:])                                # carried window: 3 pairs
        stream = [p[1][0] for p in first + second]
        outs = net.forward_many([(dv[i], dv[i + 1]) for i in range(5)])
    for i in range(5):
        assert torch.equal(stream[i], outs[i][1][0]), i
    flow = torch.cat([o[1][0] for o in outs]).cpu()
    e1, e2 = torch.cat(vols[:5]), torch.cat(vols[1:])
    check_stages(net, sd, e1, e2, flow, forms_of({"EEM_WINO4_LAYERS": "7"}, 5, 2), range(5), f"stream {h}x{w}")


@pytest.mark.parametrize("b,size,wnc,multi", [(1, (200, 256), "1", None), (1, HD, "1", None), (4, HD, "0", None),
                                              (7, MVSEC, None, "1"), (7, MVSEC, None, "0"), (4, (200, 256), None, "1")])
def test_decoder_forms(monkeypatch, b, size, wnc, multi):
    """conv1 / conv5 of the decoders on the Winograd kernel (EEM_DEC_WNC=1; its 1/64 grid needs a width that is a multiple of 4) and on
    the small-grid one (=0); the grouped convs on the one-tile (EEM_NO_TAIL_MULTI=1) and the multi-tile kernel."""
    env = {}
    if wnc is not None:
        env["EEM_DEC_WNC"] = wnc
    if multi is not None:
        env["EEM_NO_TAIL_MULTI"] = multi
    run_case(monkeypatch, env, b, *size, seed=180 + b, frames=(0, b - 1), encoder=size != HD)


@pytest.mark.parametrize("size,n", [(VGA, 2), (HD, 1)])
def test_deferred_normalisation(monkeypatch, size, n):
    """Raw voxel grids + the voxelizer's record (normalize='deferred'): pconv1_1 normalises as it reads - a1 against fp64
    (v - mean) / sd of the GPU's own raw grid and record."""
    from eemflow_amd.hrem import synthetic_hrem_events
    from eemflow_amd.voxelizer import norm_record, voxelize_many_device
    h, w = size
    pin(monkeypatch, {})
    net, sd = make_net(190, h, w)
    sets = []
    for k in range(2 * n):
        seq = EventSequence(None, {"height": h, "width": w}, features=synthetic_hrem_events(191 + k, 300_000, h, w),
                            timestamp_multiplier=1e6, convert_to_relative=True)
        sets.append(torch.from_numpy(np.ascontiguousarray(seq.features)).to(DEV))
    raw = voxelize_many_device(sets, 5, h, w, normalize="deferred")
    recs = [norm_record(r).cpu().clone() for r in raw]
    with torch.no_grad():
        outs = net.forward_many([(raw[2 * i][None], raw[2 * i + 1][None]) for i in range(n)], deferred_norm=True)
    flow = torch.cat([o[1][0] for o in outs]).cpu()
    e1 = torch.stack([raw[2 * i].cpu() for i in range(n)])
    e2 = torch.stack([raw[2 * i + 1].cpu() for i in range(n)])
    records = [recs[2 * i] for i in range(n)] + [recs[2 * i + 1] for i in range(n)]
    assert all(float(r[3]) == 1 for r in records)
    check_stages(net, sd, e1, e2, flow, forms_of({}, n, 1), range(n), f"deferred {h}x{w}", records=records)
