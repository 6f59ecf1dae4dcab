"""No inference stage turns a NaN or an infinity into a number: whole forwards of EEMFlow, EEMFlow+ and E-RAFT with one
poisoned voxel per input volume, stage by stage.  `pytest -m gpu`; the kernels' own cases are in tests/test_gpu_nonfinite_ops.py.

Every case runs the forward twice - on the clean volumes and on copies with a NaN in the first volume and an infinity in the second - in
a dispatch configuration of the model's fp64 stage module, asserts the forms that ran as that module does, and walks the recorded stages
with the module's own `check_stages` / `check_*` functions: each stage's reference is the existing fp64 function of that stage
(B.conv_ref, B.avg_pool_ref, B.corr53_ref, the decoders, er_conv_ref, er_instnorm_ref, pl_warp_ref, ...) applied to the GPU's own input
to it.  Only the criterion is exchanged: where those modules bound an error, this one calls oracle/nonfinite.py:check_nonfinite -
  (a) non-finite wherever the reference is, (b) only inside the form's output tiles that hold a non-finite reference value (the TILE
  tables of the stage modules; F(4x4) / F(2x2) forms without an entry: their 4 x 4 / 2 x 2 output tile), (c) bitwise the clean forward's
  stage wherever the stage's reference is bitwise the clean forward's (the stage's input is clean there, by (c) of the stage before).
This is where the fused epilogues GEPI_MUL / GRU / ZR / ADD_RELU / SUM2, stem7, conv_wnc, conv_wino4's residual ReLU, the tail head and
the instance norm's three roles are reached.

  * EEMFlow: 64x64 and 130x70 under every switch set of tests/test_gpu_stage_fp64.py:FORM_ENVS, batch 1 and batch 4 (one frame of the
    batch stays clean).
  * EEMFlow+: the stage module's smallest grid (128x192, levels 32x48 .. 2x3).
  * E-RAFT: the encoders (stem7 + instance norm at 128x160; the F(4x4) and the Winograd forms with their residual ReLU at batch 4 / 3)
    and one update iteration at 25x37 cells with every fused epilogue.

LEFT OUT, and why:
  * NaN or infinite lookup / warp COORDINATES: grid_sample on such coordinates is no defined reference, and the kernels clamp before the
    float -> int conversion on purpose.  E-RAFT runs ONE iteration (its coordinates are the pixel grid; the second iteration would look
    up at the first one's NaN); an EEMFlow+ warp is held to the criterion at the pixels whose flow is finite.
  * the voxelizers, IWE, tsimg, viz and augment (specified and tested bitwise elsewhere); sigmoid / tanh accuracy.

RESULTS on one MI355X, the three GPU modules (ops, models, train) in one run each.  The parent commit's library fails 146 cases:
  tests/test_gpu_nonfinite_ops.py::test_forward[NNN-<form>-relu] for all 126 forms of the table (the NaN pre-activation left as 0),
  ::test_poisoned_weight_and_bias[fwd-015-direct], [fwd-065-bx3], [fwd-087-direct], [fwd-104-direct],
  ::test_operator[act_fwd_kind1], [binary_kind3_a], [binary_kind3_b], [instnorm_fwd_hw437_relu1_res0], [..._res1], [..._res2],
  [instnorm_fwd_hw16384_relu1_res0], [bn_train_fwd_n3c3hw357_relu1], [bn_eval_fwd_n3c3hw357_relu1], [bn_train_fwd_n1c2hw16384_relu1],
  [bn_eval_fwd_n1c2hw16384_relu1], [resize_ac_bwd_gather_6x8_48x64] (a tap of weight exactly 0 skipped);
  here ::test_eraft_encoder_stages[eraft-enc-reg5_stem7], [eraft-enc-f4_b4], [eraft-enc-wnc_b3] (the norm + ReLU turns the NaN planes into
  zeros: no later stage sees the poison), ::test_eraft_update_stages[eraft-update-25x37];
  tests/test_gpu_nonfinite_train.py::*[eraft-voxel].
With the ReLU selects rewritten, three more came out: test_forward[100-fewout_wide2-relu] (0 * inf from the last channel re-read for a
spare slot), [eraft-enc-reg5_stem7] (stem7's zero-weight eighth tap carried a NaN one column further) and [eraft-voxel] (the batch norms'
ReLU gate closed on a NaN output: finite bias gradients); all fixed in their kernels.  This build passes every case of the three modules.
"""
import contextlib

import pytest
import torch

import test_gpu_eraft_stage_fp64 as ER
import test_gpu_plus_stage_fp64 as PL
import test_gpu_stage_fp64 as SG
from oracle import eemflow_oracle as O
from oracle import eemflow_plus_oracle as P
from oracle import eraft_oracle as R
from oracle import fp64_bounds as B
from oracle import nonfinite as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINO_TILE = {"f4": (4, 4), "wnc": (2, 2)}                    # E-RAFT's Winograd forms: the output tile an input transform fills


# ------------------------------------------------------------------------------------------------------------------ the exchanged criterion
class Criterion:
    """Stands in for the error bounds of oracle/fp64_bounds.py while a stage module's check functions run.  mode "record": keep every
    stage's output and reference of the clean forward by name; mode "check": hold the poisoned forward's to check_nonfinite."""

    def __init__(self):
        self.clean, self.mode, self.count, self.bad, self.seen = {}, "record", 0, 0, {}

    def hold(self, name, got, ref, tile=None, keep=None):
        got, ref = torch.as_tensor(got).detach().cpu().float(), torch.as_tensor(ref).detach().cpu()
        B.LOG.append({"name": name, "form": "nonfinite", "n": got.numel()})
        self.seen[name] = self.seen.get(name, 0) + 1               # (a name used twice in a forward: told apart by its turn)
        name = f"{name} #{self.seen[name]}" if self.seen[name] > 1 else name
        if self.mode == "record":
            self.clean[name] = (got, ref)
            return
        cg, cr = self.clean[name]
        if keep is not None:                                      # (pixels outside `keep` are left out: both sides zeroed)
            got, ref, cg, cr = (torch.where(keep, t, torch.zeros_like(t)) for t in (got, ref, cg, cr))
        reached = ~(ref == cr)                                    # the reference itself changed (a NaN differs from everything)
        rec = N.check_nonfinite(name, got, ref, clean=cg, tile=tile, reached=reached)
        self.count += 1
        self.bad += rec["nonfinite_ref"] > 0

    # the signatures of oracle/fp64_bounds.py's checks
    def check(self, name, got, ref, mag, limits, tile=None, form=None):
        self.hold(name, got, ref, tile)

    def check_decoder(self, name, got, ref64, ref32, kappa=None):
        self.hold(name, got, ref64)

    def check_form(self, name, form, got, ref, mag, tile=None, ref32=None):
        self.hold(name, got, ref, tile)

    def er_check_form(self, name, form, got, ref, mag, tile=None):
        self.hold(name, got, ref, tile or WINO_TILE.get(form))

    def pl_check_form(self, name, form, got, ref, mag):
        self.hold(name, got, ref, B.pl_tile(form))

    def check_roundings(self, name, got, ref, mag, kind, form=None):
        self.hold(name + " [roundings]", got, ref)

    def pl_check_warp(self, name, got, x, flow, mode, form="warp"):
        ok = torch.isfinite(torch.as_tensor(flow)).all(1, keepdim=True)
        safe = torch.where(ok, torch.as_tensor(flow), torch.zeros(()))
        self.hold(name, got, B.pl_warp_ref(x, safe, mode)[0], keep=ok)

    def check_bitwise(self, name, got, ref):
        g, r = B._f32(got), B._f32(ref)
        same = (g.view(torch.int32) == r.view(torch.int32)) | (torch.isnan(g) & torch.isnan(r))
        if g.shape != r.shape or not bool(same.all()):
            raise B.StageError(f"{name} [bitwise]: the copy differs from its source")


@contextlib.contextmanager
def exchanged(monkeypatch, crit, mode):
    crit.mode, crit.seen = mode, {}
    with monkeypatch.context() as m:
        for fn in ("check", "check_decoder", "check_form", "er_check_form", "pl_check_form", "check_roundings", "pl_check_warp", "check_bitwise"):
            m.setattr(B, fn, getattr(crit, fn))
        yield crit


def poisoned(idx, e1, e2, frames):
    """NaN in events1 and an infinity in events2 (its sign alternates with idx), at oracle/nonfinite.py's sites, in the images `frames`."""
    b, c, h, w = e1.shape
    s = N.sites(idx, len(frames), c, h, w, tile=(32, 64))
    p1, p2 = e1.clone(), e2.clone()
    p1[frames[s[0][0]], s[0][1], s[0][2], s[0][3]] = N.NAN
    p2[frames[s[1][0]], s[1][1], s[1][2], s[1][3]] = N.PINF if idx % 2 else N.NINF
    return p1, p2


# ------------------------------------------------------------------------------------------------------------------ the cases
EEMFLOW_SIZES = (SG.TINY, SG.TALL)                                # 64x64, 130x70
CASES = []
for _i_, (_form_, _env_) in enumerate(SG.FORM_ENVS.items()):
    for _size_ in EEMFLOW_SIZES:
        if _form_ == "fused12" and _size_ != SG.TINY:         # (the fused first layers want bottom-only padding)
            continue
        for _b_ in (1, 4):
            CASES.append({"id": f"eemflow-{_form_}-{_size_[0]}x{_size_[1]}-b{_b_}", "model": "eemflow", "env": _env_, "b": _b_, "size": _size_,
                          "idx": len(CASES), "seed": 100 + _size_[0] % 97})
CASES.append({"id": "plus-default-128x192", "model": "plus", "b": 1, "size": (128, 192), "idx": len(CASES), "seed": 3})
for _case_ in ("reg5_stem7", "f4_b4", "wnc_b3"):
    _cfg_ = ER.ENC_CASES[_case_]
    CASES.append({"id": f"eraft-enc-{_case_}", "model": "eraft-enc", "case": _case_, "b": _cfg_[1], "size": (_cfg_[2], _cfg_[3]), "idx": len(CASES), "seed": 51})
CASES.append({"id": "eraft-update-25x37", "model": "eraft-upd", "b": 2, "size": (194, 290), "idx": len(CASES), "seed": 41})


def case_inputs(case):
    """(clean e1, e2, poisoned e1, e2, the images that are poisoned) on the CPU, as the stage modules seed them."""
    from eemflow_amd.weights import synthetic_voxel_pair
    b, (h, w) = case["b"], case["size"]
    seed = {"eemflow": case["seed"] + 1, "plus": 5, "eraft-enc": 52, "eraft-upd": case["seed"] + 1}[case["model"]]
    e1, e2 = (torch.from_numpy(a) for a in synthetic_voxel_pair(seed, b, h, w))
    if case["model"] == "eemflow":
        frames = [0] if b == 1 else [0, 2, 3]                 # (batch 4: frame 1 stays clean)
    elif case["model"] == "eraft-enc":
        frames = list(ER.ENC_CASES[case["case"]][5])
    elif case["model"] == "eraft-upd":
        frames = [1]
    else:
        frames = [0]
    p1, p2 = poisoned(case["idx"], e1, e2, frames)
    return e1, e2, p1, p2, frames


def premises(case):
    """On the CPU: the model's first convolution of the poisoned volumes holds non-finite and finite values, and the oracle's forward of
    them ends in a non-finite flow (no stage on the way is allowed to lose it)."""
    e1, e2, p1, p2, frames = case_inputs(case)
    assert int((~torch.isfinite(p1)).sum()) == 1 and int((~torch.isfinite(p2)).sum()) == 1 and bool(torch.isfinite(e1).all() & torch.isfinite(e2).all())
    h, w = case["size"]
    if case["model"] == "eemflow":
        from eemflow_amd.weights import seeded_state_dict
        sd = O.to_torch_sd(seeded_state_dict(case["seed"]))
        a1 = B.first_layer_ref(torch.cat([p1, p2]), O.input_padder_pad(h, w), sd["pconv1_1.0.weight"], sd["pconv1_1.0.bias"])[0]
        flow = O.eemflow_forward(sd, p1, p2)[0]
    elif case["model"] == "plus":
        from eemflow_amd.eemflow_plus import EEMFlow_cdc
        from eemflow_amd.plus_weights import seeded_from_shapes
        sd = O.to_torch_sd(seeded_from_shapes({k: tuple(v.shape) for k, v in EEMFlow_cdc("", 3, 5).state_dict().items()}, case["seed"]))
        a1 = torch.nn.functional.conv2d(torch.cat([p1, p2]), sd["pconv1_1.0.weight"], sd["pconv1_1.0.bias"], stride=2, padding=1)
        out = P.eemflow_plus_forward(sd, p1, p2, image_size=(h, w))
        flow = (out[0] if isinstance(out, tuple) else out)[-1]
    else:
        from eemflow_amd.eraft import ERAFT
        from eemflow_amd.eraft_weights import seeded_from_shapes
        sd = O.to_torch_sd(seeded_from_shapes({k: tuple(v.shape) for k, v in ERAFT("", 5).state_dict().items()}, case["seed"]))
        a1 = torch.nn.functional.conv2d(torch.cat([p1, p2]), sd["fnet.conv1.weight"], sd["fnet.conv1.bias"], stride=2, padding=3)
        flow = R.eraft_forward(sd, p1, p2, iters=1, image_size=(h, w))[0][-1]
    N.premises(case["id"] + " first convolution", a1)
    assert not bool(torch.isfinite(flow).all()), f"{case['id']}: the oracle's flow is finite - the case is vacuous"


# ------------------------------------------------------------------------------------------------------------------ the forwards
def _twice(monkeypatch, case, body):
    """body(e1, e2, tag) runs one forward and its stage checks; first clean (recorded), then poisoned (checked)."""
    e1, e2, p1, p2, _ = case_inputs(case)
    crit = Criterion()
    with exchanged(monkeypatch, crit, "record"):
        body(e1, e2)
    with exchanged(monkeypatch, crit, "check"):
        body(p1, p2)
    print(f"{case['id']}: {crit.count} stage checks, {crit.bad} with a non-finite reference")
    assert crit.count and crit.bad, "no stage saw the poison"


@pytest.mark.parametrize("case", [c for c in CASES if c["model"] == "eemflow"], ids=lambda c: c["id"])
def test_eemflow_stages(monkeypatch, case):
    env, b, (h, w) = case["env"], case["b"], case["size"]
    SG.pin(monkeypatch, env)
    net, sd = SG.make_net(case["seed"], h, w)
    forms = SG.forms_of(env, b, 1)

    def body(e1, e2):
        d1, d2 = e1.to(DEV), e2.to(DEV)
        with torch.no_grad():
            gw = (((w + 63) // 64) * 64 // 2) // 32
            SG.assert_forms(SG.launches(net, d1, d2), forms, env, gw, b)
            flow = net(d1, d2)[1][0].cpu()
        SG.check_stages(net, sd, e1, e2, flow, forms, range(b), case["id"])
    _twice(monkeypatch, case, body)


@pytest.mark.parametrize("case", [c for c in CASES if c["model"] == "plus"], ids=lambda c: c["id"])
def test_eemflow_plus_stages(monkeypatch, case):
    h, w = case["size"]
    PL.pin(monkeypatch, {})
    net, sd = PL.make_net(case["seed"], h, w, ("",))
    tag = case["id"]

    def body(e1, e2):
        preds = PL.forward(net, e1, e2)
        st = PL.Stages(net, ("",))
        for nm, want in PL.SMALL.items():
            assert st.form(nm) == want, (nm, st.form(nm), want)
        PL.check_pyramid(st, sd, tag, e1, e2, net.image_padder._pad, [0, 1])
        PL.check_level6(st, sd, tag, 3, 1, [0])
        for l in (5, 4, 3, 2):
            PL.check_level(st, sd, tag, l, 3, 1, [0])
        PL.check_predictions(st, tag, preds, 1, [0], (h, w), False)
        PL.flush()
    _twice(monkeypatch, case, body)


@pytest.mark.parametrize("case", [c for c in CASES if c["model"] == "eraft-enc"], ids=lambda c: c["id"])
def test_eraft_encoder_stages(monkeypatch, case):
    env, b, h, w, record, imgs, cimgs, _, want = ER.ENC_CASES[case["case"]]
    ER.pin(monkeypatch, env)
    net, sd = ER.make_net(case["seed"], h, w, record, 1)
    name = case["id"]

    def body(e1, e2):
        ER.forward(net, e1, e2, 1)
        st = ER.Stages(net)
        assert want <= st.forms(), (sorted(want - st.forms()), sorted(st.forms()))
        x = B.er_pad_ref(torch.cat([e1, e2]), net.image_padder._pad)
        if "pad" in st:
            ER.soft(B.check_bitwise, f"{name} pad", st.get("pad"), x)
        fimgs = imgs + [b + i for i in imgs]
        fc = None if cimgs is None else cimgs + [b + i for i in cimgs]
        _, feat_f = ER.check_encoder(st, sd, "fnet.", x, fimgs, fc, name=name)
        _, feat_c = ER.check_encoder(st, sd, "cnet.", x[:b], imgs, cimgs, name=name)
        ER.check_heads(st, sd, feat_f, feat_c, fimgs, imgs, name)
        ER.flush()
    _twice(monkeypatch, case, body)


@pytest.mark.parametrize("case", [c for c in CASES if c["model"] == "eraft-upd"], ids=lambda c: c["id"])
def test_eraft_update_stages(monkeypatch, case):
    b, (h, w), imgs, name = case["b"], case["size"], [1], case["id"]
    ER.pin(monkeypatch, {})
    ER.STACKED[0] = True
    net, sd = ER.make_net(case["seed"], h, w, ER.UPDATE_RECORD, 1)
    pad = net.image_padder._pad
    h8, w8 = (h + pad[2] + pad[3]) // 8, (w + pad[0] + pad[1]) // 8

    def body(e1, e2):
        preds = ER.forward(net, e1, e2, 1)
        st = ER.Stages(net)
        assert "convex_up" in st.forms() and len(preds) == 1, sorted(st.forms())
        c0 = R.coords_grid(len(imgs), h8, w8)
        pyr = ER.check_pyramid(st, b, imgs, name, fmap=False)
        ER.check_iteration(st, sd, 0, st.get("net0")[imgs], pyr, imgs, c0, pad, (h, w), name, emit=True)
        ER.soft(B.check_bitwise, f"{name} pred returned", st.get("it0.pred"), preds[0])
        ER.flush()
    _twice(monkeypatch, case, body)
