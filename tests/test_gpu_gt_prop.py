"""MVSEC ground truth for any window on the GPU (eemflow_gt_flow_many, eemflow_event_mask_windows, csrc/gt_prop.hip,
eemflow_amd/mvsec_raw.py) and harness.run_recording(gt=...).  The oracle of the walk is the reference's own output on the golden cases
(tests/golden/make_golden_gt_prop.py) and the NumPy restatement (tests/gt_prop_reference.py, held to those cases bitwise by
tests/test_gt_prop_host.py) elsewhere; equality is BITWISE everywhere.  The end-to-end test holds the raw route (recording + ground
truth on the device) to the dataset route (MvsecEventFlow over files) bit for bit: grids, flows, ground truth, masks, error sums.
`pytest -m gpu`."""
import numpy as np
import pytest
import torch

from eemflow_amd import harness, mvsec, mvsec_raw as M, recording as R
from eemflow_amd.metrics import flow_error_sums_many

import gt_prop_reference as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.678


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("gt_prop.npz")
    ts = g["ts"]
    stacks = {k[len("stack_"):]: g[k] for k in g.files if k.startswith("stack_")}
    cs = [dict(name=str(n), which=str(g["stacks"][i]), start=float(g["starts"][i]), end=float(g["ends"][i]),
               ref=g[f"ref_{i}"].astype(np.float32)) for i, n in enumerate(g["names"])]       # (the short branch: rounded to fp32 once)
    gts = {k: M.MvsecGroundTruth(v, ts, device=DEV) for k, v in stacks.items()}
    return ts, stacks, cs, gts


# ------------------------------------------------------------------------------------------------ the golden cases
def test_every_golden_case_alone(cases):
    ts, stacks, cs, gts = cases
    for c in cs:
        got = gts[c["which"]].flow(c["start"], c["end"])
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 20, 28)
        assert np.array_equal(bits(got.cpu().numpy()), bits(c["ref"])), c["name"]
    u, v = M.estimate_corresponding_gt_flow(stacks["base"][:, 0], stacks["base"][:, 1], ts, cs[3]["start"], cs[3]["end"], device=DEV)
    assert np.array_equal(bits(torch.stack([u, v]).cpu().numpy()), bits(cs[3]["ref"]))      # the reference's call shape


def test_all_cases_of_a_stack_in_one_launch_and_33_jobs(cases):
    ts, stacks, cs, gts = cases
    base = [c for c in cs if c["which"] == "base"]
    plans = [gts["base"].plan(c["start"], c["end"])[1] for c in base]
    assert 0 in plans and max(plans) >= 9 and len(base) <= 32           # short and long branches share the launch
    got = gts["base"].flow_many([c["start"] for c in base], [c["end"] for c in base]).cpu().numpy()
    for i, c in enumerate(base):
        assert np.array_equal(bits(got[i]), bits(c["ref"])), c["name"]
    many = [base[i % len(base)] for i in range(33)]                     # crosses the 32-per-launch split
    got = gts["base"].flow_many([c["start"] for c in many], [c["end"] for c in many]).cpu().numpy()
    assert got.shape == (33, 2, 20, 28)
    for i, c in enumerate(many):
        assert np.array_equal(bits(got[i]), bits(c["ref"])), (i, c["name"])


def test_outputs_inside_a_sentinel_buffer_stay_clean_outside(cases):
    ts, stacks, cs, gts = cases
    base = [c for c in cs if c["which"] == "base"][:5]
    n, size, gap = len(base), 2 * 20 * 28, 37
    buf = torch.full((n * (size + gap) + gap,), SENTINEL, dtype=torch.float32, device=DEV)
    outs = [buf[gap + i * (size + gap):gap + i * (size + gap) + size].view(2, 20, 28) for i in range(n)]
    back = gts["base"].flow_many([c["start"] for c in base], [c["end"] for c in base], out=outs)
    assert back is outs
    host = buf.cpu().numpy()
    for i, c in enumerate(base):
        at = gap + i * (size + gap)
        assert np.array_equal(bits(host[at:at + size].reshape(2, 20, 28)), bits(c["ref"])), c["name"]
        assert (host[at - gap:at] == np.float32(SENTINEL)).all()
    assert (host[-gap:] == np.float32(SENTINEL)).all()
    with pytest.raises(ValueError):
        gts["base"].flow_many([base[0]["start"]], [base[0]["end"]], out=[outs[0][:, :, :27]])


# ------------------------------------------------------------------------------------------------ other sizes against the restatement
def synthetic_stack(seed, t, h, w, amp=1.5, zeros=0.01):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    st = np.empty((t, 2, h, w))
    for k in range(t):
        st[k, 0] = amp * np.sin(0.05 * y + 0.3 * k) + 0.2 * rng.standard_normal((h, w))
        st[k, 1] = amp * np.cos(0.04 * x - 0.2 * k) + 0.2 * rng.standard_normal((h, w))
    st[rng.uniform(size=st.shape) < zeros] = 0.0
    return st.astype(np.float32), 50.0 + np.cumsum(0.05 + 0.002 * rng.uniform(size=t))


def windows_of(ts):
    d = np.diff(ts)
    return [(ts[1] + 0.1 * d[1], ts[1] + 0.8 * d[1]), (ts[0] + 0.5 * d[0], ts[1] + 0.6 * d[1]), (ts[0], ts[1]), (ts[1], ts[3] + 0.5 * d[3]),
            (ts[0] + 0.25 * d[0], ts[-1])]


@pytest.mark.parametrize("t,h,w", [(5, 7, 13), (6, 260, 346)])          # a frame smaller than a block; MVSEC's size, more than one block
def test_other_sizes_equal_the_restatement(t, h, w):
    st, ts = synthetic_stack(31 + h, t, h, w, amp=4.0 if h > 100 else 1.5)
    gt = M.MvsecGroundTruth(st, ts, device=DEV)
    wins = windows_of(ts)
    assert sorted({G.plan(ts, a, b)[1] for a, b in wins}) == [0, 2, 3, t - 1]
    got = gt.flow_many([a for a, _ in wins], [b for _, b in wins]).cpu().numpy()
    for i, (a, b) in enumerate(wins):
        ref = G.gt_flow(st, ts, a, b)
        assert np.array_equal(bits(got[i]), bits(ref)), (i, G.plan(ts, a, b))
        assert (ref != 0).mean() > 0.3
    part = M.MvsecGroundTruth(st, ts, device=DEV, frames=(1, 4))       # a sub-range of the stack
    assert tuple(part.stack.shape) == (3, 2, h, w)
    assert np.array_equal(bits(part.flow(*wins[3]).cpu().numpy()), bits(got[3]))
    with pytest.raises(ValueError, match="resident"):
        part.flow(*wins[4])


def test_nan_and_infinity_stay_what_the_restatement_says():
    st, ts = synthetic_stack(77, 6, 24, 40)
    st[1, 0, 5, 5], st[2, 1, 9, 9], st[4, 0, 2, 20], st[1, 1, 20, 30] = np.nan, np.inf, np.nan, -np.inf
    d = np.diff(ts)
    wins = [(ts[1] + 0.5 * d[1], ts[4] + 0.5 * d[4]), (ts[1] + 0.1 * d[1], ts[1] + 0.6 * d[1]), (ts[1], ts[2])]
    gt = M.MvsecGroundTruth(st, ts, device=DEV)
    got = gt.flow_many([a for a, _ in wins], [b for _, b in wins]).cpu().numpy()
    seen = 0
    for i, (a, b) in enumerate(wins):
        ref = G.gt_flow(st, ts, a, b)
        assert np.array_equal(np.isnan(got[i]), np.isnan(ref)) and np.array_equal(got[i], ref, equal_nan=True), i
        seen += int((~np.isfinite(ref)).sum())
    assert seen >= 6 and np.isnan(got[0][0, 5, 5]) and np.isnan(got[1][0, 5, 5])


def test_bad_jobs_are_refused_before_any_launch(cases):
    import ctypes
    from eemflow_amd import _lib
    ts, stacks, cs, gts = cases
    gt = gts["base"]
    out = torch.empty(2, 20, 28, device=DEV)

    def call(frame0, nsteps, njobs=1):
        one = lambda t, v: (t * njobs)(*([v] * njobs))
        return _lib.lib().eemflow_gt_flow_many(njobs, gt.stack.data_ptr(), 10, 20, 28, one(ctypes.c_int, frame0), one(ctypes.c_int, nsteps),
                                               one(ctypes.c_double, 1.0), one(ctypes.c_double, 1.0), one(ctypes.c_void_p, out.data_ptr()),
                                               _lib.current_stream_ptr(torch.device(DEV)))
    assert call(0, 2) == 0
    for frame0, nsteps, njobs in ((9, 2, 1), (-1, 0, 1), (10, 0, 1), (0, 1, 1), (0, 11, 1), (0, 2, 33), (0, -2, 1)):
        assert call(frame0, nsteps, njobs) != 0, (frame0, nsteps, njobs)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the event masks
def mask_columns(kind, n, h, w):
    rng = np.random.default_rng(3)
    x, y = rng.integers(0, w, n), rng.integers(0, h, n)
    x[5], y[5], x[6], y[7] = w - 1, h - 1, w - 1, h - 1                # the last column / row
    t = np.sort(rng.integers(0, 10_000_000, n)).astype(np.int64)
    p = (2 * rng.integers(0, 2, n) - 1).astype(np.int8)
    if kind == "u16":
        return t, x.astype(np.uint16), y.astype(np.uint16), p
    xf, yf = x.astype(np.float32) + rng.uniform(0, 0.99, n).astype(np.float32) * (rng.uniform(size=n) < 0.3), y.astype(np.float32)
    xf[10], yf[11] = w, h                                              # histogram2d's closed last bin
    xf[12], yf[13], xf[14], yf[15] = w + 1, h + 0.5, -0.5, -1          # outside
    return t.astype(np.float64) * 1e-6, xf, yf, p


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_event_masks_equal_the_host_mask_on_every_slice(kind):
    n, h, w = 3000, 33, 47
    cols = mask_columns(kind, n, h, w)
    rec = R.EventRecording(*cols, h, w, device=DEV, scale_a=1e-9 if kind == "u16" else 1.0)
    offsets = [0, 1, 16, 16, 1500, 1501, n]                            # one event; an EMPTY window; an odd start
    offsets = offsets + [n] * 30                                      # 36 windows: crosses the 32-per-call split, empty windows at the end
    got = M.event_mask_windows(rec, offsets).cpu().numpy()
    assert got.shape == (len(offsets) - 1, h, w) and got.dtype == np.float32
    for k, (a, b) in enumerate(zip(offsets, offsets[1:])):
        feats = np.stack([cols[0][a:b].astype(np.float64), cols[1][a:b].astype(np.float64), cols[2][a:b].astype(np.float64),
                          cols[3][a:b].astype(np.float64)], axis=1)
        want = mvsec.event_mask(feats, h, w)
        assert np.array_equal(got[k], want.astype(np.float32)), k
        if a == b:
            assert not got[k].any()
    assert got[3].sum() > 500 and got[0].sum() == 1
    whole = M.event_mask_windows(rec, [0, n]).cpu().numpy()[0]
    assert whole[h - 1, w - 1] == 1 and whole[int(cols[2][6]), w - 1] == 1 and whole[h - 1, int(np.floor(cols[1][7]))] == 1


# ------------------------------------------------------------------------------------------------ end to end: the raw route against the dataset route
@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """Eight grey frames, about 2e4 events per frame, a 6-frame ground-truth stack at 260x346; the dataset layout of the same sequence
    (event/%06d.npz as generate_fimage cuts them, flowgt_dt1/%d.npy from the host restatement) under a temporary root."""
    h, w = 260, 346
    rng = np.random.default_rng(11)
    img_ts = 1000.0 + np.concatenate([[0.0], np.cumsum([0.03, 0.055, 0.03, 0.07, 0.03, 0.03, 0.03])])     # dt1 windows of both branches
    counts = rng.integers(19000, 21000, 8)
    parts, inds = [], []
    t_prev = img_ts[0] - 0.03
    for j in range(8):                                                 # the events in front of grey frame j: [inds[j-1], inds[j])
        m = int(counts[j])
        t = np.sort(rng.uniform(t_prev, img_ts[j], m))
        parts.append(np.stack([rng.integers(0, w, m), rng.integers(0, h, m), t, 2 * rng.integers(0, 2, m) - 1], axis=1).astype(np.float64))
        inds.append(sum(len(p) for p in parts))
        t_prev = img_ts[j]
    events = np.concatenate(parts)
    inds = np.array(inds, dtype=np.int64)
    stack, _ = synthetic_stack(5, 6, h, w, amp=3.0)
    gt_ts = img_ts[1] - 0.01 + 0.05 * np.arange(6) + 0.001 * rng.uniform(size=6)
    first, last = 1, 5
    root = tmp_path_factory.mktemp("mvsec_raw")
    ev_dir, fl_dir = root / "dataset" / "MVSEC" / "seqA" / "event", root / "dataset" / "MVSEC" / "seqA" / "flowgt_dt1"
    ev_dir.mkdir(parents=True)
    fl_dir.mkdir(parents=True)
    files = G.generate_fimage_slices(inds, 1)
    for i in range(first + 1, last + 3):
        a, b = files[i]
        fd = events[a:b]
        np.savez(ev_dir / ("%06d.npz" % i), ts=fd[:, 2], x=fd[:, 0], y=fd[:, 1], p=fd[:, 3])
    branches = set()
    for i in range(first, last + 1):
        pl = G.plan(gt_ts, img_ts[i], img_ts[i + 1])
        branches.add(min(pl[1], 2))
        if pl[1] == 0:
            np.save(fl_dir / f"{i}.npy", G.short64(stack, pl[0], pl[2], pl[3]))       # float64, as the reference returns it
        else:
            np.save(fl_dir / f"{i}.npy", G.walk(stack, *pl))
    assert branches == {0, 2}
    return dict(root=str(root), events=events, img_ts=img_ts, inds=inds, stack=stack, gt_ts=gt_ts, first=first, last=last, h=h, w=w)


@pytest.fixture(scope="module")
def net():
    from eemflow_amd import EEMFlow
    from eemflow_amd.weights import seeded_state_dict
    model = EEMFlow("", 5, 5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(3).items()})
    return model.to(DEV).eval()


@pytest.mark.parametrize("eval_type", ["dense", "sparse"])
def test_raw_route_equals_the_dataset_route_bit_for_bit(sequence, net, eval_type):
    s = sequence
    first, last, crop = s["first"], s["last"], (256, 256)
    ds = mvsec.MvsecEventFlow({"eval_type": eval_type, "num_voxel_bins": 5, "sequence": "seqA"}, train=False, root=s["root"], device=DEV,
                              valid_time_index={"seqA": [(first, last + 1)]})
    assert len(ds) == 5
    want = {}
    with torch.no_grad():
        net.change_imagesize(crop)
        for chunk, targets, flows, vol_pairs in harness.stream_chunks(ds, net, 4, torch.device(DEV), with_volumes=True):
            f_gts = [t["flow"].to(DEV)[None].float() for t in targets]                          # as TestRaftEvents scores a chunk
            evs = [t["event_valid"].to(DEV).sum(0) for t in targets] if eval_type == "sparse" else None
            sums = flow_error_sums_many(f_gts, flows, evs, evaluation_type=eval_type)
            for i, idx in enumerate(chunk):
                want[idx] = dict(flow=flows[i].clone(), gt=f_gts[i], ev=targets[i]["event_valid"][0].float(), sums=sums[i].clone(),
                                 old=vol_pairs[i][0].clone(), new=vol_pairs[i][1].clone())
    assert sorted(want) == [0, 1, 2, 3, 4]

    gt = M.MvsecGroundTruth(s["stack"], s["gt_ts"], device=DEV)
    raw = M.MvsecRaw(s["events"], s["img_ts"], s["inds"], gt, height=s["h"], width=s["w"], device=DEV)
    assert raw.recording.dtypes == (np.dtype(np.float64), np.dtype(np.uint16), np.dtype(np.uint16), np.dtype(np.int8))
    offsets, t_edges = raw.frame_windows(first, last)
    assert len(offsets) == 7 and offsets[0] == s["inds"][first]
    grids = [mvsec.center_crop(g, crop) for g in R.voxelize_windows(raw.recording, offsets, 5)]
    with torch.no_grad():
        items = list(harness.run_recording(net, raw.recording, offsets, chunk=4, gt=gt, t_edges=t_edges, crop=crop, eval_type=eval_type))
    assert [it["k"] for it in items] == [0, 1, 2, 3, 4]
    torch.cuda.synchronize()
    for it in items:
        k, w_ = it["k"], want[it["k"]]
        assert torch.equal(grids[k], w_["old"]) and torch.equal(grids[k + 1], w_["new"]), k       # the voxel grids
        assert tuple(it["flow"].shape) == (1, 2, 256, 256) and torch.equal(it["flow"], w_["flow"]), k
        file32 = np.load(ds.flow_list[k]).astype(np.float32)                                      # the fp32 of the file
        assert torch.equal(it["flow_gt"].cpu()[0], mvsec.center_crop(torch.from_numpy(file32), crop)), k
        assert torch.equal(it["flow_gt"], w_["gt"]), k
        if eval_type == "sparse":
            assert torch.equal(it["event_valid"].cpu(), w_["ev"]), k                               # the masks
            assert 0.05 < float(it["event_valid"].mean()) < 0.5
        else:
            assert "event_valid" not in it
        assert it["err_sums"].dtype == torch.float64 and torch.equal(it["err_sums"], w_["sums"]), (k, it["err_sums"], w_["sums"])
    n_pts = [float(it["err_sums"][2]) for it in items]
    assert all(v > 1000 for v in n_pts)
    # without the new keywords the items are as before
    with torch.no_grad():
        net.change_imagesize((s["h"], s["w"]))
        plain = list(harness.run_recording(net, raw.recording, offsets, chunk=4))
    assert all(sorted(it) == ["flow", "k"] for it in plain) and len(plain) == 5


# ------------------------------------------------------------------------------------------------ cli mvsec
def test_cli_mvsec_prints_the_scores_of_run_recording(sequence, net, tmp_path, capsys):
    import os
    from eemflow_amd import cli, hrem
    from eemflow_amd.metrics import flow_error_from_sums
    s = sequence
    data, gtz, ckpt, out = (str(tmp_path / n) for n in ("data.npz", "gt.npz", "ckpt.pth.tar", "flows"))
    np.savez(data, events=s["events"], image_raw_ts=s["img_ts"], image_raw_event_inds=s["inds"])
    np.savez(gtz, flow_dist=s["stack"], flow_dist_ts=s["gt_ts"])
    harness.save_checkpoint(ckpt, net, 0)
    summary = cli.main(['mvsec', '--data', data, '--gt', gtz, '--checkpoint', ckpt, '--first', '1', '--eval_type', 'sparse', '--crop', '256', '256',
                        '--stream', '4', '--out', out, '--device', DEV])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('pair ')]
    assert summary['pairs'] == 5 == len(lines) and summary['events'] == int(s["inds"][7] - s["inds"][1])      # --last defaults to the last covered pair
    raw = M.MvsecRaw.from_npz(data, gtz, device=DEV)
    assert torch.equal(raw.gt.stack.cpu(), torch.from_numpy(s["stack"])) and np.array_equal(raw.gt.ts, s["gt_ts"])
    offsets, t_edges = raw.frame_windows(1, 5)
    with torch.no_grad():
        items = list(harness.run_recording(net, raw.recording, offsets, chunk=4, gt=raw.gt, t_edges=t_edges, crop=(256, 256), eval_type='sparse'))
    aees = []
    for it, line in zip(items, lines):
        aee, p1, p3 = flow_error_from_sums(it['err_sums'])[:3]
        aees.append(aee)
        assert line == 'pair {:6d}  frame {:6d}  events {:9d}  AEE: {:2.6f}  %1px: {:.6f}  %3px: {:.6f}'.format(
            it['k'], 1 + it['k'], int(offsets[it['k'] + 1] - offsets[it['k']]), aee, 1.0 - p1, 1.0 - p3)
        assert np.array_equal(hrem.read_flo(os.path.join(out, '%06d_gt.flo' % it['k'])), it['flow_gt'][0].permute(1, 2, 0).cpu().numpy())
        assert np.array_equal(hrem.read_flo(os.path.join(out, '%06d.flo' % it['k'])), it['flow'][0].permute(1, 2, 0).cpu().numpy())
    assert abs(summary['meanAEE'] - sum(aees) / 5) < 1e-12 and summary['meanAEE'] > 0
    with pytest.raises(SystemExit, match="does not cover"):
        cli.main(['mvsec', '--data', data, '--gt', gtz, '--checkpoint', ckpt, '--first', '0', '--last', '3', '--device', DEV])
