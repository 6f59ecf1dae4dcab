"""How the persistent encoder kernels deal their tiles to blocks, restated in plain Python and proved on the host (no GPU).

Restated here, with the lines they restate:
  block_tile_range                  csrc/common.h:129-137      an XCD's contiguous range, split evenly among its blocks
  tile_coord / _retreat / _advance  csrc/common.h:138-153      tile number -> (bx, by, n), and the division-free steps
  interleaved range, stride, step   csrc/conv_wino4.hip:124-159 (reverse == 3: first = r0 + kb, count = ceil((r1 - r0 - kb) / gb), the
                                    `while` wrap); the column order (reverse == 2) and the backward walk (reverse == 1) of the same lines
  wino4_blocks                      csrc/conv_wino4.hip:710-718 the F(4x4) launcher's grid, with and without the frames-in-flight hint
  enc1_blocks                       csrc/conv_enc1.hip:224-228  pconv1_1's grid: the hint taken as a number (schedule.hip:76-77: 12 / XCD)
  bx3_blocks                        csrc/conv_bx3.hip:422-424   the stride-2 layers: one tile per block
  which walk a layer takes          csrc/schedule.hip:52-78     enc_walk: interleaved for the stride-1 layers once enc_batch >= 2

PROOF (test_every_tile_dealt_once_and_stepped_coordinates_are_the_divided_ones): for every tiles_x, tiles_y in 1..8, nimg in 1..40, and
the (tiles_x, tiles_y, nimg) of every GPU case below, on every grid the launchers produce for that T with and without the hint: every
tile (bx, by, n) is dealt exactly once and the stepped coordinates equal tile_coord(first + i stride) at every step.  The proof can
fail: four faults planted in the restatement (FAULTS) are each rejected, over the sweep and by a GPU case's own configuration.

GPU CASES (tests/test_gpu_walk_batched.py runs them; EEM_WINO4_LAYERS=7): this module computes, from the restated rules alone, the grid
every encoder launch must report, the tiles every block takes and the frames the fp64 references are computed on, and asserts that
the cases reach what they are there for (test_gpu_cases_are_not_vacuous).

What the arithmetic says otherwise than the plan these cases came from:
  * a pconv1_1 block's range NEVER spans the nimg0 boundary between the two event volumes, in any forward of this model: the padded
    height is a multiple of 64, so pconv1_1's 8-row tiles come 4 k to an image column and T = 2 B tiles_x tiles_y is a multiple of 8;
    the boundary tile T / 2 is then exactly where XCD 4's range starts (test_nimg0_boundary_is_always_an_xcd_boundary proves it for
    every padded size up to 1024 x 2048 and every batch up to 136).  What pconv1_1's ranges do cross is image boundaries (hint_c16 at
    batch 15 and 13, many_tiles) and, through the per-frame io table, frame buffers; the frames on either side of the nimg0 boundary
    are checked all the same.
  * many_16: the smallest padded size at which 32 images give T > 256 on all three channel widths with more than one tile column on
    each is 320 x 576 (9 tiles of 16 x 32 at C = 64: T = 288), not 512 x 576 (1088 x 64 is smaller still, but every layer's tiles_x is 1
    there and the stride step never leaves column 0).
"""
import itertools

import numpy as np
import pytest


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------- the restatement
FAULTS = ("if_wrap", "count_floor", "stride_minus_1", "no_clip")


def block_tile_range(T, bid, nblocks):
    """common.h:129-137 -> (first, count)."""
    cpx = (T + 7) >> 3
    xcd, kb, gb = bid & 7, bid >> 3, nblocks >> 3
    r0 = xcd * cpx
    r1 = np.minimum(r0 + cpx, T)
    per = (cpx + gb - 1) // gb
    f = r0 + kb * per
    return f, np.maximum(np.minimum(per, r1 - f), 0)


def interleaved_range(T, bid, nblocks, fault=None):
    """conv_wino4.hip:131-137 -> (first, count, stride)."""
    cpx = (T + 7) >> 3
    xcd, kb, gb = bid & 7, bid >> 3, nblocks >> 3
    r0 = xcd * cpx
    r1 = r0 + cpx if fault == "no_clip" else np.minimum(r0 + cpx, T)
    have = r1 - r0 - kb
    count = np.where(have > 0, have // gb if fault == "count_floor" else (have + gb - 1) // gb, 0)
    return r0 + kb, count, (gb - 1 if fault == "stride_minus_1" else gb)


def tile_coord(lt, tx, ty):
    """common.h:138-140."""
    return lt % tx, (lt // tx) % ty, lt // (tx * ty)


def carry(hi, wrapped, size):
    """`if (++hi == size) { hi = 0; ... }` for the blocks whose faster coordinate wrapped -> (hi, wrapped again)."""
    hi = hi + wrapped
    again = wrapped & (hi == size)
    return np.where(again, 0, hi), again


def tile_advance(t, tx, ty):
    """common.h:148-153."""
    bx, by, n = t
    bx = bx + 1
    w = bx == tx
    by, w2 = carry(by, w, ty)
    return np.where(w, 0, bx), by, n + w2


def tile_retreat(t, tx, ty):
    """common.h:142-147."""
    bx, by, n = t
    w = bx == 0
    w2 = w & (by == 0)
    return np.where(w, tx - 1, bx - 1), np.where(w2, ty - 1, by - w), n - w2


def column_coord(lt, tx, ty):
    """conv_wino4.hip:147 (reverse == 2: y fastest)."""
    return (lt // ty) % tx, lt % ty, lt // (tx * ty)


def column_step(t, tx, ty):
    """conv_wino4.hip:156."""
    bx, by, n = t
    by = by + 1
    w = by == ty
    bx, w2 = carry(bx, w, tx)
    return bx, np.where(w, 0, by), n + w2


def interleaved_step(t, stride, tx, ty, fault=None):
    """conv_wino4.hip:153-154."""
    bx, by, n = t
    bx = bx + stride
    while True:
        w = bx >= tx
        if not w.any():
            break
        by, w2 = carry(by, w, ty)
        bx, n = np.where(w, bx - tx, bx), n + w2
        if fault == "if_wrap":
            break
    return bx, by, n


def wino4_blocks(T, c, hint):
    """conv_wino4.hip:710-718: blocks of an F(4x4) launch (hint: EncConvArgs::blocks_per_xcd > 0)."""
    per_xcd = ceil_div(T, 8)
    cap = 32
    if hint and c == 16 and per_xcd > 16:
        cap = (per_xcd + 1) // 2
    return min(per_xcd, cap) * 8


def enc1_blocks(T, hint):
    """conv_enc1.hip:224-228 with schedule.hip:76-77's 12 blocks per XCD for pconv1_1 under the hint."""
    return min(ceil_div(T, 8), 12 if hint else 32) * 8


def bx3_blocks(T):
    """conv_bx3.hip:422-424: one tile per block, the grid rounded up to the eight XCDs."""
    return ceil_div(T, 8) * 8


def deal(walk, tx, ty, nimg, nblocks, fault=None):
    """Every tile every block computes, the way the kernel forms it - all blocks take their step i together, as arrays over the block
    index.  Returns one row per dealt tile, in step order: block, step, stepped (bx, by, n), divided (bx, by, n) as an [rows, 8] array.
    walk: 0 rows forward, 1 rows backward, 2 columns, 3 interleaved (EncConvArgs::reverse); 'enc1': conv_enc1.hip:58-61 (as walk 0)."""
    T = tx * ty * nimg
    bid = np.arange(nblocks, dtype=np.int64)
    if walk == 3:
        first, count, stride = interleaved_range(T, bid, nblocks, fault)
    else:
        (first, count), stride = block_tile_range(T, bid, nblocks), 1

    def divided(lt):                                              # conv_wino4.hip:146-149
        return column_coord(lt, tx, ty) if walk == 2 else tile_coord(T - 1 - lt if walk == 1 else lt, tx, ty)
    t = divided(first)                                            # conv_wino4.hip:150, conv_enc1.hip:61
    rows = []
    for i in range(int(count.max())):
        live = i < count
        rows.append(np.stack([bid, np.full_like(bid, i), *t, *divided(first + i * stride)], 1)[live])
        if walk == 3:
            t = interleaved_step(t, stride, tx, ty, fault)
        elif walk == 2:
            t = column_step(t, tx, ty)
        elif walk == 1:
            t = tile_retreat(t, tx, ty)
        else:
            t = tile_advance(t, tx, ty)
    return np.concatenate(rows) if rows else np.zeros((0, 8), np.int64)


def prove(walk, tx, ty, nimg, nblocks, fault=None):
    """Raises AssertionError unless every tile of the launch is dealt exactly once, inside the launch's images, and the stepped
    coordinates equal the divided ones at every step."""
    d = deal(walk, tx, ty, nimg, nblocks, fault)
    bx, by, n = d[:, 2], d[:, 3], d[:, 4]
    bad = (d[:, 2:5] != d[:, 5:8]).any(1)
    assert not bad.any(), f"(block, step, stepped, divided) {d[bad][0]}"
    out = (bx < 0) | (bx >= tx) | (by < 0) | (by >= ty) | (n < 0) | (n >= nimg)
    assert not out.any(), f"outside the launch: (block, step, stepped, divided) {d[out][0]}"
    times = np.bincount((n * ty + by) * tx + bx, minlength=tx * ty * nimg)
    assert (times == 1).all(), f"{(times == 0).sum()} tiles dealt to no block, {(times > 1).sum()} more than once"


def rejected(walk, tx, ty, nimg, nblocks, fault):
    try:
        prove(walk, tx, ty, nimg, nblocks, fault)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------- the GPU cases
# layer, stage, kernel family, channels, map level (1/2, 1/4, 1/8), tile (rows, columns)
LAYERS = [("pconv1_1", "a1", "enc1", 16, 1, (8, 64)), ("pconv1_2", "f11", "wino4", 16, 1, (16, 128)),
          ("pconv2_1", "a2", "bx3", 32, 2, (4, 32)), ("pconv2_2", "b2", "wino4", 32, 2, (16, 64)),
          ("pconv2_3", "f12", "wino4", 32, 2, (16, 64)), ("pconv3_1", "a3", "bx3", 64, 3, (4, 32)),
          ("pconv3_2", "b3", "wino4", 64, 3, (16, 32)), ("pconv3_3", "f13", "wino4", 64, 3, (16, 32))]

# name -> input size (a multiple of 64 both ways: no padding), the launches' (images, images of the first event volume), the
# frames_in_flight settings.  A forward of batch B has 2 B images, B of them from events1; a stream call's images are its windows
MANY16 = (320, 576)
CASES = {
    "hint_c16": dict(size=(192, 256), launches=[(32, 16), (30, 15), (26, 13)], fifs=(4, 1)),
    "many_tiles": dict(size=(64, 256), launches=[(272, 136)], fifs=(1, 4)),
    "many_16": dict(size=MANY16, launches=[(32, 16)], fifs=(1, 4)),
    "stream": dict(size=(192, 384), launches=[(16, 16), (30, 15)], fifs=(4,)),      # 16 windows; the 15 pairs as a forward_many
}
MAX_FP64_FRAMES = 24


def padded(h, w):
    return ceil_div(h, 64) * 64, ceil_div(w, 64) * 64


def layer_tiles(size, tile, level):
    """(tiles_x, tiles_y) of a layer's launch: the padded input halved `level` times (conv k3 s2 p1), cut into tiles."""
    h, w = padded(*size)
    for _ in range(level):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return ceil_div(w, tile[1]), ceil_div(h, tile[0])


def launch_plan(size, nimg, fif):
    """{layer: (walk, tiles_x, tiles_y, blocks)} of the encoder launches of one forward with F(4x4) on every stride-1 layer."""
    hint = fif >= 3
    plan = {}
    for layer, _, fam, c, level, tile in LAYERS:
        tx, ty = layer_tiles(size, tile, level)
        T = tx * ty * nimg
        if fam == "enc1":
            plan[layer] = ("enc1", tx, ty, enc1_blocks(T, hint))
        elif fam == "bx3":
            plan[layer] = (None, tx, ty, bx3_blocks(T))
        else:
            # schedule.hip:69: interleaved once enc_batch = nimg / 2 >= 2; the hint reaches the launcher for pconv1_2, 2_2, 2_3 (:76)
            plan[layer] = (3 if nimg // 2 >= 2 else 0, tx, ty, wino4_blocks(T, c, hint and c in (16, 32)))
    return plan


def expected_blocks(size, nimg, fif):
    return {layer: p[3] for layer, p in launch_plan(size, nimg, fif).items()}


def later_tiles(size, nimg, fif):
    """{layer: [per XCD: images that hold a block's second or later tile]}, tiles per block, and the largest image step, of the
    interleaved launches."""
    images, most, jump = {}, {}, {}
    for layer, (walk, tx, ty, blocks) in launch_plan(size, nimg, fif).items():
        if walk != 3:
            continue
        d = deal(3, tx, ty, nimg, blocks)
        most[layer] = int(d[:, 1].max()) + 1
        where = {(b, i): n for b, i, n in d[:, [0, 1, 4]].tolist()}
        later = d[d[:, 1] > 0]
        jump[layer] = max((n - where[b, i - 1] for b, i, n in later[:, [0, 1, 4]].tolist()), default=0)
        images[layer] = [sorted(set(later[(later[:, 0] & 7) == x, 4].tolist())) for x in range(8)]
    return images, most, jump


def frames_to_check(name, k=0):
    """Batch entries of launch k of a case whose stages go against fp64 (check_stages reads both event volumes of each): every frame
    with an image that holds some block's second or third tile under any of the case's settings, the frames on either side of the
    nimg0 boundary, the first and the last.  Where that is more than MAX_FP64_FRAMES frames (many_tiles: 136 of 136) it is thinned
    to each XCD's first and last such image per layer and setting - every XCD's stepped range stays covered at both ends.  many_16
    takes three frames: the first, the last and the one holding the most later tiles."""
    case = CASES[name]
    nimg, nimg0 = case["launches"][k]
    nframes = nimg0 if nimg0 < nimg else nimg - 1               # a stream call of n windows: n - 1 pairs, checked as a forward_many
    frame = (lambda n: n % nimg0) if nimg0 < nimg else (lambda n: min(n, nframes - 1))
    full, thin = set(), set()
    for fif in case["fifs"]:
        for per_xcd in later_tiles(case["size"], nimg, fif)[0].values():
            for imgs in per_xcd:
                full.update(frame(n) for n in imgs)
                thin.update(frame(n) for n in imgs[:1] + imgs[-1:])
    edge = {0, nframes - 1}                                       # images nimg0 - 1 | nimg0 are frames B - 1 | 0: both sides of the boundary
    if name == "many_16":
        weight = {f: 0 for f in range(nframes)}
        for fif in case["fifs"]:
            for per_xcd in later_tiles(case["size"], nimg, fif)[0].values():
                for n in itertools.chain(*per_xcd):
                    weight[frame(n)] += 1
        return sorted(edge | {max(range(1, nframes - 1), key=lambda f: weight[f])})
    return sorted(edge | (full if len(full | edge) <= MAX_FP64_FRAMES else thin))


def sweep_shapes():
    seen = set()
    for tx, ty, nimg in itertools.product(range(1, 9), range(1, 9), range(1, 41)):
        seen.add((tx, ty, nimg))
        yield tx, ty, nimg
    for case in CASES.values():
        for nimg, _ in case["launches"]:
            for _, _, _, _, level, tile in LAYERS:
                s = layer_tiles(case["size"], tile, level) + (nimg,)
                if s not in seen:
                    seen.add(s)
                    yield s


def grids_for(T):
    """(walk, blocks) of every launch the launchers can make of T tiles: the F(4x4) grid with and without the hint under each walk the
    kernel has, pconv1_1's two grids."""
    w4 = sorted({wino4_blocks(T, c, hint) for c in (16, 32, 64) for hint in (False, True)})
    e1 = sorted({enc1_blocks(T, hint) for hint in (False, True)})
    return [(walk, g) for walk in (3, 0, 1, 2) for g in w4] + [("enc1", g) for g in e1 if g not in w4]


# ------------------------------------------------------------------------------- tests
def test_every_tile_dealt_once_and_stepped_coordinates_are_the_divided_ones():
    n = 0
    for tx, ty, nimg in sweep_shapes():
        for walk, blocks in grids_for(tx * ty * nimg):
            prove(walk, tx, ty, nimg, blocks)
            n += 1
    assert n > 64 * 40 * 5


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_rejected(fault):
    """The proof fails on each planted fault: somewhere in the sweep's small shapes, and in a GPU case's own configuration."""
    small = [(tx, ty, nimg) for tx in (1, 2, 3, 5) for ty in (1, 2, 6) for nimg in (3, 30, 37, 40)]
    hits = [s for s in small if rejected(3, *s, wino4_blocks(s[0] * s[1] * s[2], 16, True), fault)]
    assert hits, fault
    assert not [s for s in small if rejected(3, *s, wino4_blocks(s[0] * s[1] * s[2], 16, True), None)]
    by_case = []
    for name, case in CASES.items():
        for (nimg, _), fif in itertools.product(case["launches"], case["fifs"]):
            for layer, (walk, tx, ty, blocks) in launch_plan(case["size"], nimg, fif).items():
                if walk == 3 and rejected(3, tx, ty, nimg, blocks, fault):
                    by_case.append((name, nimg, fif, layer))
    assert by_case, fault
    assert any(name == "hint_c16" for name, *_ in by_case), (fault, by_case)


def test_faults_are_distinct_from_the_rule():
    """Each fault changes what some block is dealt (it is not a no-op spelling of the rule)."""
    tx, ty, nimg = 1, 6, 30
    blocks = wino4_blocks(tx * ty * nimg, 16, True)
    good = deal(3, tx, ty, nimg, blocks)
    for fault in FAULTS:
        bad = deal(3, tx, ty, nimg, blocks, fault)
        assert bad.shape != good.shape or (bad != good).any(), fault


def test_nimg0_boundary_is_always_an_xcd_boundary():
    """pconv1_1: T is a multiple of 8 at every padded size and batch, so the first tile of the second event volume, T / 2, is the first
    tile of XCD 4's range and of a block's: no block's range spans the boundary, under either grid."""
    for hp, wp in itertools.product(range(64, 1025, 64), range(64, 2049, 64)):
        tx, ty = layer_tiles((hp, wp), (8, 64), 1)
        assert ty % 4 == 0
        for b in (1, 2, 3, 13, 15, 16, 136):
            T = tx * ty * 2 * b
            assert T % 8 == 0 and T // 2 == 4 * ((T + 7) >> 3)
    for case in CASES.values():
        for (nimg, nimg0), fif in itertools.product(case["launches"], case["fifs"]):
            _, tx, ty, blocks = launch_plan(case["size"], nimg, fif)["pconv1_1"]
            starts = block_tile_range(tx * ty * nimg, np.arange(blocks), blocks)[0]
            assert nimg0 == nimg or tx * ty * nimg0 in starts.tolist()


# the grids worked out by hand from the dispatch code, per case: {layer: blocks} for (images, frames_in_flight)
HAND = {
    ("hint_c16", 32, 4): {"pconv1_1": 96, "pconv1_2": 96, "pconv2_1": 768, "pconv2_2": 96, "pconv2_3": 96, "pconv3_1": 192,
                          "pconv3_2": 64, "pconv3_3": 64},
    ("hint_c16", 30, 4): {"pconv1_1": 96, "pconv1_2": 96, "pconv2_1": 720, "pconv2_2": 96, "pconv2_3": 96, "pconv3_1": 184,
                          "pconv3_2": 64, "pconv3_3": 64},
    ("hint_c16", 26, 4): {"pconv1_1": 96, "pconv1_2": 80, "pconv2_1": 624, "pconv2_2": 80, "pconv2_3": 80, "pconv3_1": 160,
                          "pconv3_2": 56, "pconv3_3": 56},
    ("hint_c16", 32, 1): {"pconv1_1": 256, "pconv1_2": 192, "pconv2_1": 768, "pconv2_2": 96, "pconv2_3": 96, "pconv3_1": 192,
                          "pconv3_2": 64, "pconv3_3": 64},
    ("many_tiles", 272, 1): {"pconv1_1": 256, "pconv1_2": 256, "pconv2_1": 2176, "pconv2_2": 256, "pconv2_3": 256, "pconv3_1": 544,
                             "pconv3_2": 256, "pconv3_3": 256},
    ("many_tiles", 272, 4): {"pconv1_1": 96, "pconv1_2": 272, "pconv2_1": 2176, "pconv2_2": 256, "pconv2_3": 256, "pconv3_1": 544,
                             "pconv3_2": 256, "pconv3_3": 256},
    ("many_16", 32, 1): {"pconv1_1": 256, "pconv1_2": 256, "pconv2_1": 3200, "pconv2_2": 256, "pconv2_3": 256, "pconv3_1": 960,
                         "pconv3_2": 256, "pconv3_3": 256},
    ("many_16", 32, 4): {"pconv1_1": 96, "pconv1_2": 480, "pconv2_1": 3200, "pconv2_2": 256, "pconv2_3": 256, "pconv3_1": 960,
                         "pconv3_2": 256, "pconv3_3": 256},
    ("stream", 30, 4): {"pconv1_1": 96, "pconv1_2": 184, "pconv2_1": 1080, "pconv2_2": 184, "pconv2_3": 184, "pconv3_1": 360,
                        "pconv3_2": 120, "pconv3_3": 120},
    ("stream", 16, 4): {"pconv1_1": 96, "pconv1_2": 96, "pconv2_1": 576, "pconv2_2": 96, "pconv2_3": 96, "pconv3_1": 192,
                        "pconv3_2": 64, "pconv3_3": 64},
}


def test_gpu_case_grids():
    for (name, nimg, fif), want in HAND.items():
        assert expected_blocks(CASES[name]["size"], nimg, fif) == want, (name, nimg, fif)


def test_gpu_cases_are_not_vacuous():
    stats = {}
    for name, case in CASES.items():
        for (nimg, nimg0), fif in itertools.product(case["launches"], case["fifs"]):
            plan = launch_plan(case["size"], nimg, fif)
            for layer, (walk, tx, ty, blocks) in plan.items():
                prove(walk or 0, tx, ty, nimg, blocks)
            _, most, jump = later_tiles(case["size"], nimg, fif)
            stats[name, nimg, fif] = (plan, most, jump)
    # hint_c16: pconv1_2 under the hint takes two tiles per block at gb = 12 / 12 / 10 (one tile per block without it), every step
    # passes two whole images, and the last XCD's range is short at 30 and 26 images
    for nimg, gb in ((32, 12), (30, 12), (26, 10)):
        plan, most, jump = stats["hint_c16", nimg, 4]
        assert plan["pconv1_2"][1:] == (1, 6, gb * 8) and most["pconv1_2"] == 2 and jump["pconv1_2"] >= 2
        assert stats["hint_c16", nimg, 1][1]["pconv1_2"] == 1
        T = 6 * nimg
        assert (8 * ceil_div(T, 8) != T) == (nimg != 32)
    # many_tiles: gb = 32 (34 at C = 16 under the hint: more blocks per XCD than CUs); three tiles per block at C = 16 without
    # the hint, two everywhere else; a step passes 16 or more images
    for fif, gb16 in ((1, 32), (4, 34)):
        plan, most, jump = stats["many_tiles", 272, fif]
        assert [plan[l][3] // 8 for l in ("pconv1_2", "pconv2_2", "pconv2_3", "pconv3_2", "pconv3_3")] == [gb16, 32, 32, 32, 32]
        assert most == {"pconv1_2": 3 if fif == 1 else 2, "pconv2_2": 2, "pconv2_3": 2, "pconv3_2": 2, "pconv3_3": 2}
        assert min(jump.values()) >= 16
    # many_16: T > 256 on all three widths, so every interleaved launch has blocks of two tiles or more, and no smaller padded size
    # with more than one tile column per layer does that
    def widths(size, nimg):
        return [layer_tiles(size, tile, level) for _, _, fam, _, level, tile in LAYERS if fam == "wino4"]
    assert all(tx * ty * 32 > 256 for tx, ty in widths(MANY16, 32)) and min(stats["many_16", 32, 1][1].values()) >= 2
    assert stats["many_16", 32, 1][1]["pconv1_2"] == 4 and stats["many_16", 32, 4][0]["pconv1_2"][1:] == (3, 10, 60 * 8)
    smaller = [(h, w) for h in range(64, 1153, 64) for w in range(64, 1153, 64) if h * w <= MANY16[0] * MANY16[1] and (h, w) != MANY16 and
               all(tx > 1 and tx * ty * 32 > 256 for tx, ty in widths((h, w), 32))]
    assert smaller == [(576, 320)], smaller                       # the same area, transposed: two tile columns at C = 64 where MANY16 has three
    # stream: 16 windows are 16 images (a pairwise call of the same 15 pairs has 30): pconv1_2 under the hint at gb = 12, two tiles each
    plan, most, jump = stats["stream", 16, 4]
    assert plan["pconv1_2"][1:] == (2, 6, 96) and most["pconv1_2"] == 2
    assert stats["stream", 30, 4][0]["pconv1_2"][3] == 184
    # pconv1_1 under the hint: 12 blocks per XCD with contiguous ranges that cross image boundaries
    crossing = 0
    for (name, nimg, fif), (plan, _, _) in stats.items():
        _, tx, ty, blocks = plan["pconv1_1"]
        assert blocks == (96 if fif >= 3 else min(ceil_div(tx * ty * nimg, 8), 32) * 8)
        d = deal("enc1", tx, ty, nimg, blocks)
        for b in range(blocks if fif >= 3 else 0):
            crossing += len(set(d[d[:, 0] == b, 4].tolist())) > 1
    assert crossing > 0
    assert max(max(m.values()) for _, m, _ in stats.values()) >= 3


def test_frames_to_check():
    assert frames_to_check("hint_c16", 0) == [0, 2, 3, 6, 7, 10, 11, 14, 15]
    for k in (1, 2):
        f = frames_to_check("hint_c16", k)
        assert f[0] == 0 and f[-1] == CASES["hint_c16"]["launches"][k][1] - 1 and len(f) <= MAX_FP64_FRAMES
    f = frames_to_check("many_tiles")
    assert f[0] == 0 and f[-1] == 135 and 8 <= len(f) <= MAX_FP64_FRAMES, f
    assert len(frames_to_check("many_16")) == 3
    f = frames_to_check("stream", 0)
    assert f[0] == 0 and f[-1] == 14 and len(f) <= 15
