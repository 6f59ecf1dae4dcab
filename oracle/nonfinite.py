"""The non-finite contract as a criterion: no kernel turns a NaN or an infinity into a number.

`check_nonfinite(tag, got, ref, clean=None, tile=None)` holds a GPU output on poisoned inputs to torch's CPU evaluation of the same
operation on the same inputs.  Only the masks of `ref` are used, so fp32 and fp64 references serve alike.  `sites` places the three
poisons (NaN, +inf, -inf) of a case; `premises` is what tests/test_nonfinite_host.py proves of every case's reference on the CPU, so that
no GPU case can pass vacuously.  Pure torch / numpy: nothing here needs a GPU.
"""
import numpy as np
import torch

from .fp64_bounds import StageError, where

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
POISONS = (NAN, PINF, NINF)


def tiles_of(mask, tile):
    """`mask` (bool, [..., H, W]) grown to whole aligned (rows, cols) tiles: True in every tile that holds a True."""
    th, tw = tile
    h, w = mask.shape[-2:]
    ph, pw = -(-h // th) * th, -(-w // tw) * tw
    m = torch.zeros(*mask.shape[:-2], ph, pw, dtype=torch.bool)
    m[..., :h, :w] = mask
    t = m.reshape(*mask.shape[:-2], ph // th, th, pw // tw, tw).any(-1).any(-2)
    return t[..., :, None, :, None].expand(*t.shape[:-2], ph // th, th, pw // tw, tw).reshape(*mask.shape[:-2], ph, pw)[..., :h, :w]


def _first(mask):
    return int(torch.nonzero(mask.reshape(-1))[0])


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def check_nonfinite(tag, got, ref, clean=None, tile=None, reached=None):
    """got: the GPU's output on poisoned inputs; ref: torch's CPU evaluation of the same operation on the same inputs (fp32 or fp64: only
    its masks count); clean: the GPU's output of the same call without the poison; tile: the (rows, cols) of the form's output tile.

      (a) no exceptions: wherever ref is non-finite, got is non-finite (NaN in place of an infinity is allowed: the bf16-piece contract);
      (b) spread: got is non-finite only inside the aligned `tile` boxes of the last two dimensions that hold a non-finite ref element
          (a Winograd input transform legitimately fills its tile); with tile=None the two masks are equal;
      (c) outside that region got equals clean bitwise.  Callers pass clean=None for outputs accumulated with atomics (weight
          gradients, the scatter adjoints): there the order of the sums, and with it the last bit, differs from run to run.
          reached: a mask of the elements the poison arrives at by the reference's own account (its non-finite pre-activation under a
          ReLU, sigmoid or tanh) - relu(-inf) = 0 and sigmoid(inf) = 1 are numbers, legitimately, and not the clean run's; (c) then
          holds outside the region and outside `reached`.

    Raises StageError naming the first offending element and its tile, as fp64_bounds.check does; returns the counts."""
    got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    if got.shape != ref.shape:
        raise StageError(f"{tag}: shape {tuple(got.shape)} against the reference's {tuple(ref.shape)}")
    bad_g, bad_r = ~torch.isfinite(got), ~torch.isfinite(ref)
    g, r = got.reshape(-1), ref.reshape(-1)
    miss = bad_r & ~bad_g
    if bool(miss.any()):
        i = _first(miss)
        raise StageError(f"{tag}: (a) a non-finite value became a number at {int(miss.sum())} of {int(bad_r.sum())} places.  First: "
                         f"{where(ref.shape, i, tile)}: got {float(g[i]):.9g}, ref {float(r[i])}")
    region = bad_r if tile is None or ref.dim() < 2 else tiles_of(bad_r, tile)
    extra = bad_g & ~region
    if bool(extra.any()):
        i = _first(extra)
        raise StageError(f"{tag}: (b) non-finite at {int(extra.sum())} places outside the {'tiles' if tile else 'elements'} where the reference "
                         f"is non-finite ({int(bad_r.sum())} elements).  First: {where(ref.shape, i, tile)}: got {float(g[i])}, ref {float(r[i]):.9g}")
    rec = {"tag": tag, "nonfinite_ref": int(bad_r.sum()), "nonfinite_got": int(bad_g.sum()), "region": int(region.sum()), "n": ref.numel()}
    if clean is not None:
        clean = torch.as_tensor(clean).detach().cpu()
        if clean.shape != got.shape or clean.dtype != got.dtype:
            raise StageError(f"{tag}: clean output {tuple(clean.shape)} {clean.dtype} against {tuple(got.shape)} {got.dtype}")
        if not bool(torch.isfinite(clean).all()):
            raise StageError(f"{tag}: the clean run's output is not finite: {where(ref.shape, _first(~torch.isfinite(clean)), tile)}")
        diff = (_bits(got) != _bits(clean)) & ~region
        if reached is not None:
            diff &= ~torch.as_tensor(reached).cpu().expand_as(diff)
        if bool(diff.any()):
            i = _first(diff)
            raise StageError(f"{tag}: (c) {int(diff.sum())} values outside the poisoned region differ from the clean run.  First: "
                             f"{where(ref.shape, i, tile)}: got {float(g[i]):.9g}, clean {float(clean.reshape(-1)[i]):.9g}")
    return rec


def premises(tag, ref, whole=False, pre=None):
    """What every GPU case rests on, proven on the CPU: the reference holds a non-finite value (the case cannot pass vacuously), a finite
    one unless the case is `whole` (a weight gradient's row, a norm's plane or channel: it cannot pass by being all NaN), and for a ReLU
    case (`pre`: the pre-activation) a NaN where the pre-activation is NaN - relu(-inf) = 0 is a legitimate number and proves nothing."""
    ref = torch.as_tensor(ref)
    bad = ~torch.isfinite(ref)
    assert bool(bad.any()), f"{tag}: the reference is finite everywhere - the case is vacuous"
    if whole:
        assert bool(bad.all()), f"{tag}: marked whole-output, but the reference holds finite values"
    else:
        assert not bool(bad.all()), f"{tag}: the reference is non-finite everywhere and the case is not marked whole-output"
    if pre is not None:
        pre = torch.as_tensor(pre)
        assert pre.shape == ref.shape, (tag, pre.shape, ref.shape)
        assert bool((torch.isnan(pre) & torch.isnan(ref)).any()), f"{tag}: no NaN pre-activation reaches the ReLU as a NaN"


def inf_to_nan(t):
    """The operand a bf16-piece kernel (conv_bx3.hip, gconvb.hip, the *_bx3 weight gradients) multiplies: a - (a & 0xffff0000) is
    inf - inf = NaN for an infinite a, so every infinity enters the sum as a NaN (the documented contract: NaN in place of an infinity)."""
    return torch.where(torch.isinf(t), torch.full_like(t, NAN), t)


def sites(idx, n, c, h, w, tile=None, first_seg=None, ylim=None, xlim=None, channel=None, snap=1):
    """Three distinct (image, channel, y, x) for NaN, +inf, -inf in a [n][c][h][w] tensor.  Four classes of position, of which case
    `idx` takes three in rotation, so that a table's cases together cover all of them with every value:
      0: (0, 0), channel 0;
      1: the last row and column (ragged tiles), the last channel;
      2: the row and the column just before a tile boundary, the last channel of the first input segment;
      3: the column just after that boundary, half way down the rest of the map, channel 0.
    The poisons go to different images where the batch allows.  ylim / xlim = (lo, hi) keep a position inside [lo, hi] (a weight
    gradient's dy away from the padding); channel fixes one channel for all three; snap rounds y and x down to its multiples (the
    input positions a strided 1 x 1 filter reads at all)."""
    th, tw = tile or (8, 32)
    ty = th if th < h else max(h // 2, 1)
    tx = tw if tw < w else max(w // 2, 1)
    classes = [(0, 0, 0), (h - 1, w - 1, c - 1), (ty - 1, tx - 1, (first_seg or c) - 1), (min((ty + h) // 2, h - 1), min(tx, w - 1), 0)]
    out = []
    for k in range(3):
        y, x, ch = classes[(idx + k) % 4]
        y, x = y // snap * snap, x // snap * snap
        if ylim is not None:
            y = min(max(y, ylim[0]), ylim[1])
        if xlim is not None:
            x = min(max(x, xlim[0]), xlim[1])
        if channel is not None:
            ch = channel
        s = ((idx + k) % n, ch, y, x)
        while s in out:                                          # (tiny maps: the classes coincide) the next column, row or channel
            s = (s[0], s[1], s[2], s[3] + 1) if s[3] + 1 <= (xlim[1] if xlim else w - 1) else \
                (s[0], s[1], s[2] + 1, s[3]) if s[2] + 1 <= (ylim[1] if ylim else h - 1) else (s[0], (s[1] + 1) % c, s[2], s[3])
        out.append(s)
    return out


def poison(t, where_, values=POISONS):
    """A copy of `t` with values[k] at where_[k] (index tuples)."""
    t = t.clone()
    for v, s in zip(values, where_):
        t[tuple(s)] = v
    return t


def poison_segments(xs, where_, values=POISONS):
    """The same for channel-concatenated segments: where_ indexes cat(xs, 1)."""
    bounds = np.cumsum([0] + [x.shape[1] for x in xs])
    xs = [x.clone() for x in xs]
    for v, (n, c, y, x) in zip(values, where_):
        s = int(np.searchsorted(bounds, c, side="right") - 1)
        xs[s][n, c - int(bounds[s]), y, x] = v
    return xs
