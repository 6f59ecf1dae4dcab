"""oracle/nonfinite.py on the CPU: the criterion passes torch against itself and rejects six planted faults, and every case of the GPU
modules (tests/test_gpu_nonfinite_ops.py, _models.py, _train.py: the same tables, iterated here) rests on a reference that holds a
non-finite value, a finite one unless the case is marked whole-output, and - under a ReLU - a NaN whose pre-activation is a NaN, not
-inf.  No case can pass vacuously or by being all NaN."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_nonfinite_models as M
import test_gpu_nonfinite_ops as T
import test_gpu_nonfinite_train as TR
from oracle import fp64_bounds as B
from oracle import nonfinite as N

OPS = T.OPS
TILE = (4, 16)


# ------------------------------------------------------------------------------------------------------------------ the criterion
@pytest.fixture(scope="module")
def conv():
    """A 3x3 ReLU conv on a 2 x 8 x 21 x 37 input with the three poisons: (pre-activation, torch's output, torch's clean output)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 21, 37, generator=g)
    w, b = B.seeded_conv(7, 8, 12, (3, 3))
    xp = N.poison(x, N.sites(2, 2, 8, 21, 37, tile=TILE))
    pre = F.conv2d(xp, w, b, padding=1)
    return pre, torch.relu(pre), torch.relu(F.conv2d(x, w, b, padding=1))


def _reached(pre):
    return ~torch.isfinite(pre)


def test_torch_against_itself_passes(conv):
    pre, ref, clean = conv
    for tile in (None, TILE):
        rec = N.check_nonfinite("self", ref.clone(), ref, clean, tile=tile, reached=_reached(pre))
        assert rec["nonfinite_ref"] == rec["nonfinite_got"] > 0
    N.check_nonfinite("self64", ref.clone(), ref.double())                     # an fp64 reference serves alike: only the masks count
    N.premises("self", ref, pre=pre)
    assert bool((torch.isinf(pre) & (pre < 0)).any()) and bool((ref[torch.isinf(pre) & (pre < 0)] == 0).all())   # relu(-inf) = 0 is in the case
    with pytest.raises(B.StageError, match=r"\(c\)"):                          # ... and without `reached` it is no clean value
        N.check_nonfinite("self", ref.clone(), ref, clean)


def test_nan_in_place_of_an_infinity_is_allowed(conv):
    pre, ref, clean = conv
    got = torch.where(torch.isinf(ref), torch.full_like(ref, N.NAN), ref)
    assert not torch.equal(torch.isnan(got), torch.isnan(ref))
    N.check_nonfinite("inf->nan", got, ref, clean, reached=_reached(pre))


def test_a_winograd_tile_may_fill_but_not_spill(conv):
    pre, ref, clean = conv
    region = N.tiles_of(~torch.isfinite(ref), TILE)
    assert int(region.sum()) > int((~torch.isfinite(ref)).sum()) and bool((region | torch.isfinite(ref)).all())
    got = torch.where(region, torch.full_like(ref, N.NAN), ref)
    N.check_nonfinite("filled tiles", got, ref, clean, tile=TILE, reached=_reached(pre))
    with pytest.raises(B.StageError, match=r"\(b\)"):
        N.check_nonfinite("filled tiles", got, ref, clean, tile=None, reached=_reached(pre))


FAULTS = ["relu_as_select_gt", "clamp_min_via_fmax", "nan_to_num_on_one_tile", "nan_one_tile_too_far", "finite_value_changed", "inf_to_flt_max"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_rejected(conv, fault):
    pre, ref, clean = conv
    got, want, tile = ref.clone(), r"\(a\)", None
    bad = ~torch.isfinite(ref)
    n, c, y, x = (int(v) for v in torch.nonzero(torch.isnan(ref))[0])
    if fault == "relu_as_select_gt":
        got = torch.where(pre > 0, pre, torch.zeros_like(pre))
    elif fault == "clamp_min_via_fmax":
        got = torch.fmax(pre, torch.zeros_like(pre))
    elif fault == "nan_to_num_on_one_tile":
        ty, tx = y // TILE[0] * TILE[0], x // TILE[1] * TILE[1]
        got[n, c, ty:ty + TILE[0], tx:tx + TILE[1]] = torch.nan_to_num(got[n, c, ty:ty + TILE[0], tx:tx + TILE[1]], nan=0.0)
        tile = TILE
    elif fault == "nan_one_tile_too_far":
        region = N.tiles_of(bad, TILE)
        far = torch.nonzero(~region[n, c])                                   # the first element of a tile the reference keeps finite
        got[n, c, int(far[0, 0]), int(far[0, 1])] = N.NAN
        want, tile = r"\(b\)", TILE
    elif fault == "finite_value_changed":
        i = int(torch.nonzero((~_reached(pre)).reshape(-1))[-1])
        got.view(-1)[i] = torch.nextafter(got.view(-1)[i], torch.tensor(float("inf")))
        want = r"\(c\)"
    elif fault == "inf_to_flt_max":
        assert bool(torch.isinf(ref).any())
        got = torch.where(torch.isinf(ref), torch.full_like(ref, torch.finfo(torch.float32).max), ref)
    with pytest.raises(B.StageError, match=want) as e:
        N.check_nonfinite(fault, got, ref, clean, tile=tile, reached=_reached(pre))
    assert "image" in str(e.value) and "channel" in str(e.value)              # the first offending element is named
    if tile:
        assert "tile (row" in str(e.value)


def test_sites_cover_the_classes_and_stay_distinct():
    seen = set()
    for idx in range(12):
        s = N.sites(idx, 2, 48, 9, 20, tile=(2, 16), first_seg=32)
        assert len(set(s)) == 3
        seen |= {(y, x, c) for _, c, y, x in s}
    assert {(0, 0, 0), (8, 19, 47), (1, 15, 31), (5, 16, 0)} <= seen
    for idx in range(4):                                                       # a tiny, limited map: still three distinct places
        s = N.sites(idx, 1, 1, 7, 9, tile=(8, 32), ylim=(3, 3), xlim=(3, 5), channel=0)
        assert len(set(s)) == 3 and all(y == 3 and 3 <= x <= 5 for _, _, y, x in s)


# ------------------------------------------------------------------------------------------------------------------ the premises
def _premises(tag, ref, whole=()):
    outs = [k for k in ref if ":" not in k]
    assert outs
    for name in outs:
        N.premises(f"{tag}.{name}", ref[name], whole=name in whole, pre=ref.get("pre:" + name))
        if "reached:" + name in ref:
            assert bool((ref["reached:" + name] | torch.isfinite(ref[name])).all()), f"{tag}.{name}: non-finite outside `reached`"


@pytest.mark.parametrize("idx", range(len(OPS.FWD)), ids=T._ids(OPS.FWD))
def test_premises_forward(idx):
    for act in (B.ACT_NONE, B.ACT_RELU, B.ACT_LEAKY):
        _premises(f"fwd[{idx}] act {act}", T.fwd_ref(idx, act))
    assert len(set(map(tuple, N.sites(idx, OPS.FWD[idx][6], sum(OPS.FWD[idx][1]), *OPS.FWD[idx][7:9])))) == 3


@pytest.mark.parametrize("idx", range(len(OPS.DGRAD)), ids=T._ids(OPS.DGRAD))
def test_premises_data_gradient(idx):
    _premises(f"dgrad[{idx}]", T.dgrad_ref(idx))


@pytest.mark.parametrize("idx", range(len(OPS.WGRAD)), ids=T._ids(OPS.WGRAD))
def test_premises_weight_gradient(idx):
    _premises(f"wgrad[{idx}]", T.wgrad_ref(idx), whole=T.wgrad_whole(idx))


@pytest.mark.parametrize("kind,idx,family", T.PARAM, ids=[f"{k}-{i:03d}-{f}" for k, i, f in T.PARAM])
def test_premises_poisoned_weight_and_bias(kind, idx, family):
    _premises(f"param {kind}[{idx}]", T.param_ref(kind, idx), whole=T.wgrad_whole(idx, True) if kind == "wgrad" else ())


@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_premises_operator(case):
    clean_in, bad_in = case.build()
    ref = case.ref(bad_in)
    _premises(case.name, ref, whole=case.whole)
    for name, t in case.ref(clean_in).items():
        if ":" not in name:
            assert bool(torch.isfinite(t).all()), f"{case.name}.{name}: the clean reference is not finite"


@pytest.mark.parametrize("case", M.CASES, ids=[c["id"] for c in M.CASES])
def test_premises_model(case):
    M.premises(case)


@pytest.mark.parametrize("case", TR.CASES, ids=[c["id"] for c in TR.CASES])
def test_premises_training(case):
    TR.premises(case)
