"""The synthetic MVSEC sequence of the dt4 tests (tests/test_gpu_spans.py) and of `tools/bench_recording.py --spans`: the raw arrays of a
sequence and the dataset layout of the same sequence on disk.  Host only, no test in here."""
import numpy as np

import gt_prop_reference as G


def synthetic_stack(seed, t, h, w, amp=1.5, zeros=0.01):
    """tests/test_gpu_gt_prop.py's ground-truth stack."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    st = np.empty((t, 2, h, w))
    for k in range(t):
        st[k, 0] = amp * np.sin(0.05 * y + 0.3 * k) + 0.2 * rng.standard_normal((h, w))
        st[k, 1] = amp * np.cos(0.04 * x - 0.2 * k) + 0.2 * rng.standard_normal((h, w))
    st[rng.uniform(size=st.shape) < zeros] = 0.0
    return st.astype(np.float32), None


def make_sequence(root):
    """Fourteen grey frames, about 2e4 events per frame, a ground-truth stack at 260x346 that covers the samples 1..8 at dt 4; the
    dataset layout of the same sequence (event/%06d.npz as generate_fimage cuts them, flowgt_dt4/%d.npy from the host restatement over
    [ts[i], ts[i+4]]) under a temporary root.  Eight samples are nine windows: three calls of four, the carried window crossed twice."""
    h, w, frames = 260, 346, 14
    rng = np.random.default_rng(12)
    img_ts = 1000.0 + np.concatenate([[0.0], np.cumsum([0.03, 0.055, 0.03, 0.04, 0.03, 0.03, 0.035, 0.03, 0.03, 0.045, 0.03, 0.03, 0.03])])
    counts = rng.integers(19000, 21000, frames)
    parts, inds = [], []
    t_prev = img_ts[0] - 0.03
    for j in range(frames):                                            # the events in front of grey frame j: [inds[j-1], inds[j])
        m = int(counts[j])
        t = np.sort(rng.uniform(t_prev, img_ts[j], m))
        parts.append(np.stack([rng.integers(0, w, m), rng.integers(0, h, m), t, 2 * rng.integers(0, 2, m) - 1], axis=1).astype(np.float64))
        inds.append(sum(len(p) for p in parts))
        t_prev = img_ts[j]
    events = np.concatenate(parts)
    inds = np.array(inds, dtype=np.int64)
    nstack = 11
    stack, _ = synthetic_stack(6, nstack, h, w, amp=3.0)
    gt_ts = img_ts[1] - 0.01 + 0.05 * np.arange(nstack) + 0.001 * rng.uniform(size=nstack)
    first, last = 1, 8
    assert gt_ts[-2] > img_ts[last + 4]                                # every window ends inside the stack
    ev_dir, fl_dir = root / "dataset" / "MVSEC" / "seqA" / "event", root / "dataset" / "MVSEC" / "seqA" / "flowgt_dt4"
    ev_dir.mkdir(parents=True)
    fl_dir.mkdir(parents=True)
    files = G.generate_fimage_slices(inds, 1)
    for i in range(first + 1, frames):                                 # sample i reads the files i+1 .. i+5; the last one file 13
        a, b = files[i]
        fd = events[a:b]
        np.savez(ev_dir / ("%06d.npz" % i), ts=fd[:, 2], x=fd[:, 0], y=fd[:, 1], p=fd[:, 3])
    for i in range(first, last + 1):
        pl = G.plan(gt_ts, img_ts[i], img_ts[i + 4])
        assert pl[1] >= 2                                              # four frames are longer than a ground-truth interval
        np.save(fl_dir / f"{i}.npy", G.walk(stack, *pl))
    return dict(root=str(root), events=events, img_ts=img_ts, inds=inds, stack=stack, gt_ts=gt_ts, first=first, last=last, h=h, w=w)
