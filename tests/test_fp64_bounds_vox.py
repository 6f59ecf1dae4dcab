"""The checks of tests/test_gpu_vox_fp64.py bite, shown without a GPU.

The banded path of voxel.hip is restated here in numpy: the binning kernel's move of out-of-plane votes by whole planes (its own floor
division and t2 == -1 branch, not the reference's flat index), fp64 cells rounded to fp32 once, the read-out's per-thread fp32 partial
moments in the kernel's cell-to-thread layout, vox_final's record and the fp32 normalisation.  The restatement must pass every criterion
of oracle/fp64_bounds.py on the GPU module's own inputs; each of ten planted faults must be rejected by the same check the GPU module
applies.  The conditions the criteria rest on are checked with the reference alone: the share of cells with a residual, the vote cap of
the dyadic direct-kernel cases, the cells that cancel to zero, the strays that take each branch, and that vox_plan reaches exactly the
forms of VOX_FORMS.
"""
import numpy as np
import pytest

from oracle import fp64_bounds as B

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ the restatement
def band_grid(ev, bins, h, w, plan, mutate=None):
    """vox_bin_kernel's records and vox_band_kernel's accumulation: the raw grid (flat, fp32)."""
    V = B.vox_votes(ev, bins, h, w)
    hw, total = h * w, bins * h * w
    pix, tl = V["pix"].copy(), V["tl"].copy()
    wl, wr = V["vl"].copy(), np.where(V["okr"], V["vr"], f32(0)).astype(f32)
    keep = V["okl"].copy()
    out = keep & ((pix < 0) | (pix >= hw))
    q = pix // hw                                                   # floor division
    t2 = tl + q + (1 if mutate == "plane_off" else 0)
    front = out & (t2 == -1)
    tl = np.where(out, np.where((t2 >= 0) & (t2 < bins), t2, -1), tl)
    pix = np.where(out, pix - q * hw, pix)
    tl = np.where(front, 0, tl)
    wl, wr = np.where(front, wr, wl), np.where(front, f32(0), wr)
    keep &= tl >= 0
    pix, tl, wl, wr = pix[keep], tl[keep], wl[keep], wr[keep]
    right = tl + 1 < bins
    cells = np.concatenate([pix + tl * hw, (pix + (tl + 1) * hw)[right]])
    votes = np.concatenate([wl, wr[right]])
    if mutate == "right_at_bins":                                   # the masked right vote of the last bin, added where the band ends
        extra = ~right & (wr != 0)
        assert int(extra.sum()) > 0
        cells = np.concatenate([cells, (pix + tl * hw)[extra]])
        votes = np.concatenate([votes, wr[extra]])
    if mutate == "lost_record":                                     # one record of the longest run's busiest cell
        busiest = np.bincount(cells, minlength=total).argmax()
        drop = np.nonzero((cells == busiest) & (votes != 0))[0][-1]
        cells, votes = np.delete(cells, drop), np.delete(votes, drop)
    if mutate == "fp32_cell":
        grid = np.zeros(total, dtype=f32)
        np.add.at(grid, cells, votes)                               # one fp32 rounding per vote
    else:
        grid = np.bincount(cells, weights=votes.astype(f64), minlength=total).astype(f32)
    if mutate == "short_band_last_cell":
        assert plan["last_px"] < plan["band_px"] and bool((grid.reshape(bins, hw)[:, hw - 1] != 0).any())
        grid.reshape(bins, hw)[:, hw - 1] = 0
    return grid


def band_record(grid, bins, h, w, plan, mutate=None, occupied=0):
    """The read-out loop's moments (a thread folds its K cells in fp32: bins x its pixels, four at a time with vec4), vox_final, the record."""
    hw, bpx, nb, bt = h * w, plan["band_px"], plan["nb"], plan["bt"]
    step = 4 if plan["vec4"] else 1
    per = plan["K"] // bins // step                                  # iterations of a thread over one bin's pixels
    g = np.zeros((bins, nb, per * bt * step), dtype=f32)
    flat = np.zeros((bins, nb * bpx), dtype=f32)
    flat[:, :hw] = grid.reshape(bins, hw)
    g[:, :, :bpx] = flat.reshape(bins, nb, bpx)
    a = g.reshape(bins, nb, per, bt, step).transpose(1, 3, 0, 2, 4).reshape(nb * bt, plan["K"])     # [thread][its cells in loop order]
    if mutate == "running_fp32":
        v = grid.astype(f32)
        S, Q = float(np.cumsum(v, dtype=f32)[-1]), float(np.cumsum(v * v, dtype=f32)[-1])
    else:
        sm, sq = np.zeros(a.shape[0], dtype=f32), np.zeros(a.shape[0], dtype=f32)
        for k in range(a.shape[1]):
            v = a[:, k]
            sm = sm + v
            sq = (v.astype(f64) * v.astype(f64) + sq.astype(f64)).astype(f32)          # fmaf
        S, Q = float(sm.astype(f64).sum()), float(sq.astype(f64).sum())
    # count_zeros: every cell counts; count_cancelled: every cell that received a vote, those that cancel to 0 included
    c = float(bins * hw) if mutate == "count_zeros" else float(occupied) if mutate == "count_cancelled" else float(np.count_nonzero(a))
    anyv = c != 0
    with np.errstate(all="ignore"):
        m2 = max(Q - S * S / c, 0.0) if anyv else 0.0
        mean = f32(S / c) if anyv else f32(0)
        sd = f32(np.sqrt(f64(m2) / f64(c if mutate == "c_for_c1" else c - 1)))
    scale = bool(sd > 0)
    return np.array([mean, sd if (scale or mutate == "sd_unset") else 1.0, 1.0 if scale else 0.0, 1.0 if anyv else 0.0], dtype=f32)


def normalised(grid, rec, mutate=None):
    if mutate == "shift_zeros" and rec[3] != 0:
        out = grid - rec[0]
        return (out / rec[1]).astype(f32) if rec[2] != 0 else out.astype(f32)
    return B.vox_normalise_f32(grid, rec)


def case(name, k=0):
    kind, n, h, w, bins, modes, opt = B.VOX_CASES[name]
    ev = B.vox_case_events(name)[k]
    plan, _ = B.vox_case_form(name, modes[0])
    V = B.vox_votes(ev, bins, h, w)
    return ev, bins, h, w, plan, V, B.vox_exact(ev, bins, h, w, V)


def hold_all(name, grid, rec, norm, plan, E, generic):
    B.vox_check_raw_exact(name, grid, E, "model", allow_residual=generic)
    B.vox_check_record(name, rec, grid, plan["K"], "model")
    B.vox_check_normalised(name, norm, grid, plan["K"], "model")
    B.check_bitwise(name, norm, B.vox_normalise_f32(grid, rec))


SMALL = ["bt256_v1_s6", "bt256_v4_s3", "bt512_s5", "bt512_s4", "dyadic_banded", "one_event", "one_voxel", "equal_voxels", "same_t", "bins1",
         "many1"]


@pytest.mark.parametrize("name", SMALL)
def test_the_restated_banded_path_passes_every_criterion(name):
    ev, bins, h, w, plan, V, E = case(name)
    grid = band_grid(ev, bins, h, w, plan)
    rec = band_record(grid, bins, h, w, plan)
    hold_all(name, grid, rec, normalised(grid, rec), plan, E, B.VOX_CASES[name][0] in ("clustered", "hostile"))
    B.vox_check_raw_counted(name, grid, E, "model")                 # (an exactly rounded sum is inside the direct path's counted bound too)


# ------------------------------------------------------------------------------------------------------------------ planted faults
RAW_FAULTS = [("lost_record", "bt256_v1_s6"), ("right_at_bins", "bt256_v1_s6"), ("short_band_last_cell", "bt256_v1_s6"),
              ("fp32_cell", "bt256_v4_s3"), ("plane_off", "bt256_v1_s6"), ("lost_record", "bt512_s4"), ("short_band_last_cell", "bt512_s4")]


@pytest.mark.parametrize("fault,name", RAW_FAULTS)
def test_a_fault_in_the_raw_grid_is_rejected(fault, name):
    ev, bins, h, w, plan, V, E = case(name)
    with pytest.raises(B.StageError):
        B.vox_check_raw_exact(name, band_grid(ev, bins, h, w, plan, fault), E, "model")


@pytest.mark.parametrize("fault,name", [("count_zeros", "bt256_v1_s6"), ("count_cancelled", "dyadic_banded"), ("count_cancelled", "same_t"), ("running_fp32", "running_sum"),
                                        ("c_for_c1", "bt256_v1_s6"), ("c_for_c1", "bt512_s4"), ("sd_unset", "one_voxel"),
                                        ("sd_unset", "equal_voxels"), ("sd_unset", "one_event")])
def test_a_fault_in_the_moments_is_rejected(fault, name):
    if name == "running_sum":
        # enough non-zero voxels for one running fp32 sum to leave the per-thread bound: 2 x 10^5 dyadic events on 260 x 346 x 5 (K = 20)
        bins, h, w = 5, 260, 346
        ev = B.vox_events("dyadic", 5, 200_000, h, w, bins)
        plan, occupied = B.vox_plan(len(ev), bins, h, w), 0
    else:
        ev, bins, h, w, plan, V, E = case(name)
        occupied = len(E["cells"])
    grid = band_grid(ev, bins, h, w, plan)
    B.vox_check_record(name, band_record(grid, bins, h, w, plan), grid, plan["K"], "model")
    with pytest.raises(B.StageError):
        B.vox_check_record(name, band_record(grid, bins, h, w, plan, fault, occupied), grid, plan["K"], "model")


@pytest.mark.parametrize("name", ["dyadic_banded", "same_t", "bt256_v1_s6"])
def test_the_mean_subtracted_from_zero_voxels_is_rejected(name):
    ev, bins, h, w, plan, V, E = case(name)
    grid = band_grid(ev, bins, h, w, plan)
    rec = band_record(grid, bins, h, w, plan)
    with pytest.raises(B.StageError):
        B.vox_check_normalised(name, normalised(grid, rec, "shift_zeros"), grid, plan["K"], "model")


def test_moments_of_a_faulty_record_fail_the_normalised_bound_too():
    """The normalised modes show no record: the bound on the grid itself must reject c for c - 1 and a counted zero."""
    ev, bins, h, w, plan, V, E = case("bt256_v1_s6")
    grid = band_grid(ev, bins, h, w, plan)
    for fault in ("c_for_c1", "count_zeros"):
        with pytest.raises(B.StageError):
            B.vox_check_normalised(fault, normalised(grid, band_record(grid, bins, h, w, plan, fault)), grid, plan["K"], "model")


# ------------------------------------------------------------------------------------------------------------------ the inputs' conditions
@pytest.mark.parametrize("name", [n for n, c in B.VOX_CASES.items() if not n.startswith("ept")])
def test_the_committed_inputs_keep_the_conditions(name):
    kind, n, h, w, bins, modes, opt = B.VOX_CASES[name]
    for k, ev in enumerate(B.vox_case_events(name)):
        assert bool(np.all(ev[:-1, 0] <= ev[1:, 0]))                # time-sorted
        V = B.vox_votes(ev, bins, h, w)
        E = B.vox_exact(ev, bins, h, w, V)
        share = float((E["res"] != 0).sum()) / max(1, len(E["cells"]))
        assert share <= B.VOX_RESIDUAL_SHARE, (name, k, share)
        if kind not in ("clustered", "hostile") or any(m in modes for m in ("norm", "twopass")):
            assert share == 0.0, (name, k)                          # the raw grid is decided bit for bit
        plan, _ = B.vox_case_form(name, modes[0])
        if kind == "dyadic":
            assert ev[0, 0] == 0 and ev[-1, 0] == B.VOX_T_DYADIC and bool(np.all(ev[:, 0] == np.floor(ev[:, 0])))
            assert int(((E["sum"] == 0) & (E["abs"] > 0)).sum()) > 0        # +1 and -1 votes that cancel to exactly 0
            if plan is None:
                assert int(E["count"].max()) < B.VOX_DYADIC_DIRECT_CAP, (name, int(E["count"].max()))
        if kind == "hostile" and len(ev) > 100:
            lost = V["okl"] & ~V["inl"]
            moved = V["inl"] & ((V["pix"] < 0) | (V["pix"] >= h * w))
            assert int(lost.sum()) > 0
            if bins > 1:
                assert int(moved.sum()) > 0                         # (one bin: a pixel index outside the plane is outside the grid)
                if plan is not None:                                # the binning kernel's t2 == -1 branch, with a live right vote
                    assert int(((V["tl"] + V["pix"] // (h * w) == -1) & V["inr"]).sum()) > 0
                assert int((V["okl"] & ~V["okr"]).sum()) >= min(8, len(ev))                       # events at t_last: tl = bins - 1
            assert int((ev[:, 1] >= w).sum()) > 0 and int((ev[:, 2] >= h).sum()) > 0 and int((ev[:, 2] < 0).sum()) > 0
            assert int((ev[:, 3] == 0).sum()) > 0


def test_the_plan_restated_reaches_exactly_the_table():
    forms, sgs, bt, ept, vec = set(), set(), set(), set(), set()
    for name, c in B.VOX_CASES.items():
        for mode in c[5]:
            plan, form = B.vox_case_form(name, mode)
            forms.add(form)
            if plan:
                sgs.add(plan["sgs"]), bt.add(plan["bt"]), ept.add(plan["ept"]), vec.add((plan["vec4"], bool(c[6].get("misalign")), c[2] * c[3] % 4 == 0))
    assert forms == B.VOX_FORMS, (sorted(forms ^ B.VOX_FORMS))
    assert sgs == set(B.VOX_SGS_REACHABLE) and bt == {256, 512, 1024} and ept == {1, 2, 4, 8}
    assert {(False, True, True), (False, False, False), (True, False, True)} <= vec          # vec4 off by the pointer, off by h w % 4, on
    # sgs = 2 is unreachable: no (nb, EPT) with nb <= 1023 leaves the loop at 2
    for e in (1, 2, 4, 8):
        for nb in range(1, 1024):
            lanes = 40 if 1024 * e < 4 * nb else 17
            assert 4 * 10 * nb < lanes * 1024 * e
    # the two shapes that fall to the direct kernel by size, a short last band in both vec4 forms, the many-jobs call's ragged block counts
    assert B.vox_case_form("direct_by_cells", "deferred")[0] is None and B.vox_case_form("direct_by_bins", "raw")[0] is None
    assert B.vox_plan(20_000, 64, 480, 644)is None and B.vox_plan(20_000, 63, 480, 644) is not None
    for name in ("bt256_v1_s6", "bt256_v4_s3", "bt512_s4", "ept8"):
        p = B.vox_case_form(name, B.VOX_CASES[name][5][0])[0]
        assert 0 < p["last_px"] < p["band_px"]
    blocks = {(n + 1023) // 1024 for n in B.VOX_MANY_32}
    assert B.VOX_MANY_32[0] == 1 and blocks == {1, 2, 3}
    assert [B.vox_plan(n, 3, 40, 52)["ept"] for n in (524_288, 524_289, 1_048_576, 1_048_577, 2_097_152, 2_097_153)] == [1, 2, 2, 4, 4, 8]


def test_a_cell_with_a_residual_may_take_either_neighbour_and_nothing_else():
    """No committed input has such a cell, so the rule is shown on a made one: 0.75 + 2^-60 in one of 2000 occupied cells."""
    bins, h, w = 2, 40, 50
    n = 2000
    ev = np.zeros((n + 1, 4))
    ev[:, 0] = np.concatenate([[0.0, 2.0 ** -60], np.full(n - 2, 0.75), [1.0]])
    pix = np.concatenate([[7, 7], np.arange(n - 1) + 7])                  # the 2^-60 event shares pixel 7 with the first 0.75 event
    ev[:, 1], ev[:, 2], ev[:, 3] = pix % w, pix // w, 1.0
    E = B.vox_exact(ev, bins, h, w)
    assert int((E["res"] != 0).sum()) == 1 and len(E["cells"]) >= 1000
    cell = int(E["cells"][np.nonzero(E["res"])[0][0]])
    grid = B.vox_dense(E).astype(f32)
    B.vox_check_raw_exact("rounded", grid, E, "model")
    for step, ok in ((1, True), (-1, False), (2, False)):                 # the exact sum lies just above 0.75: the neighbour above, not below
        g = grid.copy()
        for _ in range(abs(step)):
            g[cell] = np.nextafter(g[cell], f32(np.inf if step > 0 else -np.inf))
        if ok:
            B.vox_check_raw_exact("neighbour", g, E, "model")
        else:
            with pytest.raises(B.StageError):
                B.vox_check_raw_exact("not a neighbour", g, E, "model")
    with pytest.raises(B.StageError):
        B.vox_check_raw_exact("must be exact", grid, E, "model", allow_residual=False)
    at = int(np.nonzero(E["res"])[0][0])
    few = {k: (v[at:at + 3].copy() if isinstance(v, np.ndarray) else v) for k, v in E.items()}       # one of three cells: above the share
    with pytest.raises(B.StageError, match="more than"):
        B.vox_check_raw_exact("share", B.vox_dense(few).astype(f32), few, "model")
