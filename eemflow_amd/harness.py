"""Slim evaluation / training harness around the GPU path.

Keeps what the reference's harness does ON the path and its log lines, drops cv2 / pandas / imageio / git:

  load_checkpoint / save_checkpoint   test_EEMFlow_HREM.py:59-66, train_EEMFlow_HREM.py:127-130:
                                      torch.save({'epoch', 'state_dict'}) '.pth.tar', keys optionally 'module.'-prefixed
  TestRaftEvents.test_multi_sequence  test_mvsec.py:538-671: per sequence, every `stride`-th sample: change_imagesize,
                                      model(events1, events2), flow_error on the last prediction, the reference's summary
                                      lines; returns the mean AEE over the sequences
  TrainRaftEvents.train_iters         train_mvsec.py:229-286: model.change_imagesize, one optimisation step per batch.
                                      engine="fused" (default): EEMFlowTrainer - loss, backward, [RCCL all-reduce], clip +
                                      AdamW + OneCycle inside the library; engine="autograd": the reference's literal sequence
                                      (fetch_optimizer's torch AdamW + OneCycleLR, GradScaler, model(im1, im2) -> sequence_loss
                                      -> scaler.scale(loss).backward() -> clip_grad_norm_ -> scaler.step) through the model's
                                      torch.autograd.Function - for callers that bring their own optimizer or loss

Samples come from a dataset with the reference's dict keys ('event_volume_old', 'event_volume_new', 'flow', 'valid',
'event_valid'); tensors are moved to the model's device.  One process per GPU (eemflow_amd.parallel), not
nn.DataParallel.  Unlike the reference, save_checkpoint can also store the step count of the schedule.
"""
import collections
import itertools
import os
import sys

import torch

from .metrics import flow_error, flow_error_from_sums, flow_error_sums, flow_error_sums_many
from . import parallel
from .train import EEMFlowTrainer, contrast_loss, photo_loss, sequence_loss, smoothness_loss, ssim_loss, timestamp_loss


class Logger:
    """write_line(text, also_print) as the reference's logger is used; lines are kept in `.lines`."""

    def __init__(self, path=None, verbose=True):
        self.path, self.lines, self.verbose = path, [], verbose

    def write_line(self, text, verbose=True):
        self.lines.append(text)
        if self.path:
            with open(self.path, "a") as f:
                f.write(text + "\n")
        if verbose and self.verbose:
            print(text)
            sys.stdout.flush()


def load_checkpoint(path, model, map_location="cpu", with_iteration=False):
    """Load {'epoch', 'state_dict'}; 'module.' prefixes of nn.DataParallel checkpoints are stripped. Returns the epoch, or with
    with_iteration=True (epoch, iteration): the schedule position save_checkpoint stores (0 for the reference's own checkpoints)."""
    states = torch.load(path, map_location=map_location, weights_only=False)
    sd = collections.OrderedDict((k.replace('module.', ''), v) for k, v in states['state_dict'].items())
    model.load_state_dict(sd)
    if with_iteration:
        return states.get('epoch', 0), int(states.get('iteration', 0))
    return states.get('epoch', 0)


def save_checkpoint(path, model, epoch, trainer=None, module_prefix=False, iteration=None):
    """Write the reference's checkpoint layout.  With a trainer, the device-resident weights are synced into the
    module first and the schedule position is stored under 'iteration' (the reference does not keep it); `iteration` stores the
    position of a loop that has no fused trainer (the autograd engine)."""
    if trainer is not None:
        trainer.sync_parameters()
    sd = model.state_dict()
    if module_prefix:
        sd = collections.OrderedDict(('module.' + k, v) for k, v in sd.items())
    out = {'epoch': epoch, 'state_dict': collections.OrderedDict((k, v.detach().cpu()) for k, v in sd.items())}
    if trainer is not None:
        out['iteration'] = trainer.iteration
    elif iteration is not None:
        out['iteration'] = int(iteration)
    torch.save(out, path)


def _device_of(model):
    return next(model.parameters()).device


def stream_plan(n_samples, n):
    """The calls of a stride-1 walk over a sequence of n_samples samples (n_samples + 1 consecutive windows) by forward_stream (EEMFlow,
    EEMFlow_cdc, ERAFT), at most n windows per call: [(first_window, windows, first_sample, flows)].  The first call carries nothing in (its
    windows - 1 flows); every later one starts at the window the call before carried (as many flows as windows).  Every window is in one
    call, every sample one flow."""
    n = max(2, min(int(n), 16))
    plan, w = [], 0
    while n_samples > 0 and w <= n_samples:
        cnt = min(n, n_samples + 1 - w)
        plan.append((w, cnt, max(w - 1, 0), cnt if w > 0 else cnt - 1))
        w += cnt
    return plan


def stream_chunks(dataset, model, n, dev, fb_check=None, with_volumes=False):
    """Walk the dataset's current sequence window by window: each window read and voxelized once (dataset.get_windows), each call's
    windows through ONE model.forward_stream, the stream reset at the start.  Yields (sample indices, their targets, their flows) per call.
    fb_check = (alpha1, alpha2[, 'all' | 'obj' | 'out']): the stream runs bidirectionally (EEMFlow; at most 8 windows per call) and a
    fourth element follows, the samples' forward consistency masks (mask_fw of forward_stream(fb_check=...)).
    with_volumes: a last element follows, the samples' (event_volume_old, event_volume_new) as the [1, C, H, W] device tensors the
    model was given (sample i is windows i and i + 1; the last window of a call is kept for the next call's first sample)."""
    model.reset_stream()
    carry_target = None
    carry_volume = None
    if fb_check is not None:
        n = min(int(n), getattr(model, "MAX_STREAM_BIDIR", 8))
    for w0, cnt, s0, nflow in stream_plan(len(dataset), n):
        vols, targets = dataset.get_windows(w0, cnt)
        vols = [v.to(dev)[None].float() for v in vols]
        if fb_check is not None:
            outs = model.forward_stream(vols, bidirectional=True, fb_check=tuple(fb_check))
        else:
            outs = model.forward_stream(vols)
        pair_targets = ([carry_target] if w0 > 0 else []) + list(targets[:cnt - 1])
        carry_target = targets[cnt - 1]
        if len(outs) != nflow or len(pair_targets) != nflow:
            raise RuntimeError(f"stream_chunks: windows {w0}..{w0 + cnt - 1} gave {len(outs)} flows for {nflow} samples")
        tail = ()
        if with_volumes:
            seq = ([carry_volume] if w0 > 0 else []) + vols
            carry_volume = vols[-1]
            tail = ([(seq[i], seq[i + 1]) for i in range(nflow)],)
        if fb_check is not None:
            yield (list(range(s0, s0 + nflow)), pair_targets, [o[1][-1] for o in outs], [o[3][0] for o in outs]) + tail
        else:
            yield (list(range(s0, s0 + nflow)), pair_targets, [preds[-1] for _, preds in outs]) + tail


def lag_plan(nwin, lag, chunk):
    """The forward_stream calls of run_recording over nwin windows whose pairs are (a, a + lag), at most `chunk` windows per call:
    [(reset, windows, pairs)].  The windows fall into `lag` classes r = 0 .. lag-1 - r, r + lag, r + 2*lag, ... - and each class is an
    ordinary stream of neighbouring windows: its first call follows a reset_stream (reset True) and gives one flow fewer than it has
    windows, every later call starts at the window the call before carried and gives as many flows as windows.  windows: the indices that
    go into the call, in order; pairs: the (a, a + lag) that come out, in order.  Every window is in exactly one call, every pair comes
    out once, class by class.  lag = 1 is the walk over consecutive windows (stream_plan's calls)."""
    nwin, lag, chunk = int(nwin), int(lag), int(chunk)
    if lag < 1 or chunk < 1:
        raise ValueError(f"lag_plan: lag and chunk are positive, got {lag} and {chunk}")
    plan = []
    for r in range(min(lag, nwin)):
        members = list(range(r, nwin, lag))
        for i0 in range(0, len(members), chunk):
            part = members[i0:i0 + chunk]
            plan.append((i0 == 0, part, [(a - lag, a) for a in part if a - lag >= 0]))
    return plan


def run_recording(model, recording, offsets=None, chunk=None, fwl=False, rsat=False, bidirectional=False, fb_check=None, iters=None, gt=None,
                  t_edges=None, crop=None, eval_type='dense', is_car=False, spans=None, lag=1, t_spans=None):
    """Flow along the consecutive windows [offsets[k], offsets[k+1]) of a resident recording (eemflow_amd.recording.EventRecording): a
    generator of one dict per pair of neighbouring windows, in time order -
        'k'         the pair's first window (the flow runs from window k to window k + 1)
        'flow'      [1, 2, H, W], the last prediction of model.forward_stream
        'flow_bw', 'mask_fw', 'mask_bw'   with bidirectional / fb_check (models whose forward_stream takes them: EEMFlow)
        'FWL', 'RSAT'                     with fwl / rsat: 0-dim float64 device tensors, the flow warp loss / RSAT of window k's events
                                          under the flow (iwe.fwl_many, tsimg.rsat_many on recording.tables, t_ref="end")
    Per step `chunk` windows (default: the model's MAX_STREAM, or MAX_STREAM_BIDIR when bidirectional) are voxelized straight from the
    recording's columns by one launch sequence (recording.voxelize_windows, num_bins = model.n_first_channels) and go through ONE
    forward_stream call; the window the model carries joins the chunks, so every window is voxelized and encoded once.  The stream
    is reset at the start and the model sized to the recording's sensor.  fb_check = (alpha1, alpha2[, 'all' | 'obj' | 'out']) implies
    bidirectional; iters: E-RAFT's refinement steps per pair (forward_stream's own default when None).  The loop itself reads nothing back from the device (fwl_many / rsat_many read their windows' end times, one small
    copy per chunk).
    gt = a mvsec_raw.MvsecGroundTruth, with t_edges = the K + 1 timestamps of the window edges (offsets[k] is the first event of the
    window that starts at t_edges[k]: MvsecRaw.frame_windows gives both): every item gains
        'flow_gt'   [1, 2, h, w], the ground-truth displacement over [t_edges[k], t_edges[k+1]] (MvsecGroundTruth.flow_many)
        'err_sums'  the five doubles of metrics.flow_error_sums_many for the pair (metrics.flow_error_from_sums turns them into
                    the reference's AEE / outlier tuple); is_car drops the rows from 190 on, as Test.flow_error does
    by ONE ground-truth launch and ONE metrics launch per chunk, no synchronisation.  eval_type='sparse' scores the pixels of window k
    that hold an event (mvsec_raw.event_mask_windows on the chunk's first windows; the item gains 'event_valid', [h, w] fp32 0 / 1).
    crop = (th, tw): the voxel grids are centre-cropped (mvsec.center_crop) before forward_stream, the model is sized to the crop,
    ground truth and mask are cropped the same way - the dataset's validation branch (MVSEC.py:193-197).  crop with fwl or rsat is
    refused: the events would need the crop's offset.  Without these keywords items, launches and lines are exactly as before.
    Windows BY SPAN and pairs at a LAG: instead of offsets, spans = a (K, 2) array of [start, end) event indices whose starts and
    whose ends are each non-decreasing (windows that overlap: EventRecording.sliding_spans, MvsecRaw.frame_spans), and lag >= 1: the
    pairs are (a, a + lag), K - lag of them.  No model knows about the lag: the windows are walked class by class (lag_plan) - class r
    is the windows r, r + lag, r + 2*lag, ..., an ordinary stream of neighbouring pairs after a reset_stream - so every window is
    still voxelized once and encoded once, and E-RAFT's warm start runs along each class.  The items come out class-major, not in time
    order; with spans each also carries 'k2', the pair's second window.  FWL / RSAT / the sparse mask use window k's events.  With
    spans, gt= takes t_spans = (K - lag, 2) timestamps: pair p = (p, p + lag) is scored over [t_spans[p, 0], t_spans[p, 1]]; with
    offsets and a lag, pair k is scored over [t_edges[k], t_edges[k + lag]].  Give exactly one of offsets and spans."""
    from .recording import _windows_of, voxelize_windows
    if fb_check is not None:
        bidirectional = True
    if eval_type not in ('dense', 'sparse'):
        raise ValueError(f"run_recording: eval_type is 'dense' or 'sparse', got {eval_type!r}")
    if gt is None and (t_edges is not None or t_spans is not None or eval_type != 'dense' or is_car):
        raise ValueError("run_recording: t_edges=, t_spans=, eval_type='sparse' and is_car= qualify gt= (the ground truth they score against)")
    if crop is not None:
        if fwl or rsat:
            raise ValueError("run_recording: crop= with fwl= or rsat= is refused: the events are not moved into the crop's frame")
        crop = (int(crop[0]), int(crop[1]))
        if not (1 <= crop[0] <= recording.height and 1 <= crop[1] <= recording.width):
            raise ValueError(f"run_recording: crop {crop} does not fit the recording's {recording.height} x {recording.width} sensor")
    if bidirectional and not hasattr(model, "MAX_STREAM_BIDIR"):
        raise ValueError(f"fb_check= needs a model whose forward_stream takes bidirectional=True (EEMFlow); {type(model).__name__} has none")
    if not hasattr(model, "forward_stream"):
        raise ValueError(f"run_recording needs a model with forward_stream (EEMFlow, EEMFlow_cdc, ERAFT); {type(model).__name__} has none")
    offs, span_list = _windows_of("run_recording", offsets, spans, recording.n)
    if int(lag) != lag or int(lag) < 1:
        raise ValueError(f"run_recording: lag is a positive number of windows (the pairs are (a, a + lag)), got {lag!r}")
    lag = int(lag)
    if offs is None and any(b[0] < a[0] or b[1] < a[1] for a, b in zip(span_list, span_list[1:])):
        raise ValueError("run_recording: the spans' starts and ends must each be non-decreasing (windows in time order)")
    nwin = len(span_list)
    npairs = max(nwin - lag, 0)
    limit = model.MAX_STREAM_BIDIR if bidirectional else model.MAX_STREAM
    chunk = limit if chunk is None else int(chunk)
    if not 1 <= chunk <= limit:
        raise ValueError(f"run_recording: chunk is 1..{limit} windows per forward_stream call" + (" with bidirectional=True" if bidirectional else "")
                         + f", got {chunk}")
    pair_times = None                                                # per pair (a, a + lag), by a: the [start, end] its ground truth covers
    if gt is not None:
        if offs is not None:
            if t_spans is not None:
                raise ValueError("run_recording: t_spans= goes with spans=; with offsets give t_edges=")
            if t_edges is None or len(t_edges) != len(offs):
                raise ValueError(f"run_recording: gt= needs t_edges=, one timestamp per window edge ({len(offs)} for these offsets)")
            t_edges = [float(t) for t in t_edges]
            pair_times = [(t_edges[a], t_edges[a + lag]) for a in range(npairs)]
        else:
            if t_edges is not None:
                raise ValueError("run_recording: t_edges= goes with offsets; with spans= give t_spans=")
            rows = [] if t_spans is None else [tuple(float(v) for v in row) for row in t_spans]
            if t_spans is None or len(rows) != npairs or any(len(row) != 2 for row in rows):
                raise ValueError(f"run_recording: gt= needs t_spans=, one (start, end) per pair ({npairs} for {nwin} spans at lag {lag})")
            pair_times = rows
        if (gt.height, gt.width) != (recording.height, recording.width) or gt.device != recording.device:
            raise ValueError("run_recording: the ground truth and the recording differ in size or device")
        for t0, t1 in pair_times:
            gt.plan(t0, t1)                                          # a window the stack cannot serve is refused before any launch
    size = crop if crop is not None else (recording.height, recording.width)
    if tuple(int(v) for v in getattr(model, "image_size", None) or ()) != size:
        model.change_imagesize(size)
    model.reset_stream()
    extra = dict(bidirectional=True, **({"fb_check": tuple(fb_check)} if fb_check is not None else {})) if bidirectional else {}
    if iters is not None:
        import inspect
        if "iters" not in inspect.signature(model.forward_stream).parameters:
            raise ValueError(f"iters= needs a model whose forward_stream takes the refinement steps per pair (ERAFT); {type(model).__name__} has none")
        if int(iters) < 1:
            raise ValueError(f"run_recording: iters is a positive number of refinement steps, got {iters}")
        extra["iters"] = int(iters)
    consecutive = offs is not None and lag == 1                      # today's walk: every call's windows are neighbours in offs

    def windows_of(idx):                                             # how recording.* is told about the windows idx
        if consecutive:
            return dict(offsets=offs[idx[0]:idx[-1] + 2])
        return dict(spans=[span_list[i] for i in idx])

    for call, (reset, wins, pairs) in enumerate(lag_plan(nwin, lag, chunk)):
        if reset and call > 0:
            model.reset_stream()                                     # the next class is a stream of its own
        vols = voxelize_windows(recording, num_bins=model.n_first_channels, **windows_of(wins))
        if crop is not None:
            from .mvsec import center_crop
            vols = [center_crop(v, crop) for v in vols]
        outs = model.forward_stream(vols, **extra)
        if len(outs) != len(pairs):
            raise RuntimeError(f"run_recording: windows {wins} gave {len(outs)} flows for the pairs {pairs}")
        if not outs:
            continue                                                 # the call held one window: it is carried
        firsts = [a for a, _ in pairs]                               # the pairs' first windows
        n = len(outs)
        items = [{'k': a, 'flow': o[1][-1]} for (a, _), o in zip(pairs, outs)]
        if offs is None:
            for it, (_, b) in zip(items, pairs):
                it['k2'] = b
        if bidirectional:
            for it, o in zip(items, outs):
                it['flow_bw'] = o[2][-1]
                if fb_check is not None:
                    it['mask_fw'], it['mask_bw'] = o[3]
        if fwl or rsat:
            tables = recording.tables(**windows_of(firsts))
            flows = [it['flow'][0] for it in items]
            if fwl:
                from .iwe import fwl_many                            # (the package's attribute `iwe` is the one-job function, not the module)
                for it, v in zip(items, fwl_many(tables, flows)):
                    it['FWL'] = v
            if rsat:
                from .tsimg import rsat_many
                for it, v in zip(items, rsat_many(tables, flows)):
                    it['RSAT'] = v
        if gt is not None:
            gts = gt.flow_many([pair_times[a][0] for a in firsts], [pair_times[a][1] for a in firsts])
            masks = None
            if eval_type == 'sparse':
                from .mvsec_raw import event_mask_windows
                masks = event_mask_windows(recording, **windows_of(firsts))
            if crop is not None:
                from .mvsec import center_crop
                gts = center_crop(gts, crop).contiguous()            # (one copy for the chunk; its slices are contiguous)
                masks = center_crop(masks, crop).contiguous() if masks is not None else None
            sums = flow_error_sums_many([gts[i:i + 1] for i in range(n)], [it['flow'] for it in items],
                                        [masks[i] for i in range(n)] if masks is not None else None, is_car=is_car, evaluation_type=eval_type)
            for i, it in enumerate(items):
                it['flow_gt'], it['err_sums'] = gts[i:i + 1], sums[i]
                if masks is not None:
                    it['event_valid'] = masks[i]
        yield from items


class TestRaftEvents:
    """Evaluation loop of test_mvsec.py:538-671 on a dataset object (HREMEventFlow-like: change_test_sequence, __len__,
    __getitem__ -> sample dict)."""
    __test__ = False                      # not a pytest class

    def __init__(self, dataset, image_size, logger=None, is_car=False):
        self.dataset = dataset
        self.image_size = image_size
        self.logger = logger or Logger()
        self.is_car = is_car

    def run_network(self, model, sample, dev):
        e1 = sample['event_volume_old'].to(dev)[None].float()
        e2 = sample['event_volume_new'].to(dev)[None].float()
        _, preds = model(events1=e1, events2=e2)
        return preds[-1]

    def test_multi_sequence(self, model, epoch=0, sequence_list=(), stride=10, frames_in_flight=1, loader_threads=0, coalesce=1, stream=0,
                            fb_check=None, visualize_map=False, vis_events=False, print_epe=False, visualize_every=1, save_path=None, fwl=False,
                            rsat=False):
        """The evaluation loop of test_mvsec.py:580-597.  It reads the LAST prediction of every sample only (run_network, :1455): a
        model that can skip forming the earlier ones (ERAFT.final_only) does so for the duration of the call.
        stream = n > 0 (stride 1, a model with forward_stream - EEMFlow, EEMFlow_cdc, ERAFT - and a dataset of consecutive windows with
        get_windows - MvsecEventFlow / _dt4): each sequence is walked window by window, every window read and voxelized once, up to n per call
        (stream_plan), each call's windows through ONE model.forward_stream - sample i's flow is windows i and i + 1, the encoder runs
        once per window instead of twice.  Same per-sample lines in the same order; frames_in_flight, loader_threads and coalesce do
        not apply.  An ERAFT with warm_start = True is E-RAFT's warm-start evaluation: each sequence starts cold (reset_stream), every
        later sample from the previous sample's forward-interpolated flow.
        fb_check = (alpha1, alpha2[, 'all' | 'obj' | 'out']) (needs stream > 0 and a model whose forward_stream is bidirectional:
        EEMFlow): the stream runs in both directions and every per-sample line gains two fields - `fb consistent`, the share of pixels
        the forward-backward check (metrics.fb_check) keeps, and `AEE consistent`, the AEE over those pixels alone (the mask as the
        event image of the sparse flow_error).  Without it the lines are unchanged.
        visualize_map (the reference's keyword, test_mvsec.py:618-637; all four loops): every visualize_every-th sample (the reference:
        every one) is written as JPEG files under <save_path>/<sequence>/test/ (the reference's self.save_path is per sequence, :576):
        <idx>_flow_est.jpg - <idx>_flow_est_<AEE:.3f>.jpg with print_epe - and <idx>_flow_gt.jpg, the colour-wheel images of the
        estimated and the ground-truth flow (viz.flow_to_image), and with vis_events <idx>_events1_<density:.3f>.jpg and
        <idx>_events2_..., the red / blue images of both event volumes (viz.event_image); idx is the number the sample's line carries.
        Per chunk all estimated flows go through one conversion call and all ground truths through one more, on the chunk's stream;
        the files are encoded by an ImageWriter's threads behind the evaluation.  The key-map images (emap1/2), warp_img and the HSV
        variant are not built.  Off (the default): lines, numbers and launches are unchanged.
        fwl (all four loops; a dataset built with with_events=True): the flow warp loss of every sample's last prediction - the
        variance of the image of the old window's events warped by the flow over the variance of their count image
        (eemflow_amd.iwe.fwl_many, t_ref="end"; the measure of Test.inference_img_warp_loss, test_mvsec.py:753-852, which needs no
        ground truth) - by ONE fwl_many call per chunk on the chunk's stream.  Every per-sample line gains
        '  FWL: {:2.6f}  meanFWL:{:2.6f}' (NaN samples - a constant count image - are left out of the mean) and every sequence one
        summary line "Mean FWL: {:.6f}".  Off (the default): lines, numbers and launches are unchanged.
        rsat (all four loops; a dataset built with with_events=True): RSAT of every sample's last prediction - the average-timestamp
        loss of the old window's events warped by the flow over that loss under zero flow (eemflow_amd.tsimg.rsat_many, t_ref="end";
        below 1 where the flow sharpens the events, no ground truth needed) - by ONE rsat_many call per chunk on the chunk's stream.
        Every per-sample line gains '  RSAT: {:2.6f}  meanRSAT:{:2.6f}' (after FWL's fields; NaN samples are left out of the mean) and
        every sequence one summary line "Mean RSAT: {:.6f}".  Off (the default): lines, numbers and launches are unchanged."""
        if rsat and not getattr(self.dataset, "with_events", False):
            raise ValueError(f"rsat= needs a dataset whose samples carry their events (with_events=True: MvsecEventFlow, MvsecEventFlow_dt4, "
                             f"HREMEventFlow); {type(self.dataset).__name__} was built without")
        if fwl and not getattr(self.dataset, "with_events", False):
            raise ValueError(f"fwl= needs a dataset whose samples carry their events (with_events=True: MvsecEventFlow, MvsecEventFlow_dt4, "
                             f"HREMEventFlow); {type(self.dataset).__name__} was built without")
        if visualize_map:
            if not save_path:
                raise ValueError("visualize_map= needs save_path= (the images go to <save_path>/<sequence>/test/)")
            if int(visualize_every) < 1:
                raise ValueError(f"visualize_every must be >= 1, got {visualize_every}")
        elif vis_events or print_epe:
            raise ValueError("vis_events= / print_epe= qualify visualize_map=True")
        if fb_check is not None:
            if not stream:
                raise ValueError("fb_check= needs stream= (the backward flow comes from the bidirectional stream)")
            if not hasattr(model, "MAX_STREAM_BIDIR"):
                raise ValueError(f"fb_check= needs a model whose forward_stream takes bidirectional=True (EEMFlow); {type(model).__name__} has none")
        if stream:
            if stride != 1:
                raise ValueError(f"stream= walks consecutive windows: it needs stride == 1 (got stride={stride}, whose samples share no window)")
            if not getattr(self.dataset, "consecutive_windows", False) or not hasattr(self.dataset, "get_windows"):
                raise ValueError(f"stream= needs a dataset whose sample i is windows i and i + 1 (consecutive_windows, get_windows: MvsecEventFlow, "
                                 f"MvsecEventFlow_dt4); {type(self.dataset).__name__}'s samples are separate event files (HREM: events1.npz / "
                                 f"events2.npz) that share no window")
            if not hasattr(model, "forward_stream"):
                raise ValueError(f"stream= needs a model with forward_stream (EEMFlow, ERAFT); {type(model).__name__} has none "
                                 f"(EEMFlow_cdc has one too)")
        had = getattr(model, "final_only", None)
        if had is not None:
            model.final_only = True
        try:
            extra = {"fb_check": fb_check} if fb_check is not None else {}
            if fwl:
                extra["fwl"] = True
            if rsat:
                extra["rsat"] = True
            if visualize_map:
                extra["visualize"] = dict(vis_events=bool(vis_events), print_epe=bool(print_epe), every=int(visualize_every), save_path=save_path)
            return self._test_multi_sequence(model, epoch, sequence_list, stride, frames_in_flight, loader_threads, coalesce, stream, **extra)
        finally:
            if had is not None:
                model.final_only = had
            writer = self.__dict__.pop("_viz_writer", None)
            if writer is not None:                               # an error left the loop early: the encoder threads still stop
                writer.close(reraise=False)

    def _test_multi_sequence(self, model, epoch=0, sequence_list=(), stride=10, frames_in_flight=1, loader_threads=0, coalesce=1, stream=0,
                             fb_check=None, visualize=None, fwl=False, rsat=False):
        """coalesce > 1 (a model with forward_many - EEMFlow, EEMFlow_cdc, ERAFT - and a dataset with get_samples): that many samples are read, voxelized by
        ONE voxelizer launch sequence and handed to ONE model.forward_many call - n independent batch-1 samples riding a batch-n chain of
        launches, every sample in its own tensors; raw volumes with a normalisation record (HREMEventFlow(deferred_norm=True)) are
        normalised by the first convolution as it reads them.  Chunks alternate over min(frames_in_flight, 2) replicas / streams.  Same
        per-sample lines in the same order; the numbers agree with the one-sample loop to fp32 round-off (the batched chain uses the
        F(4x4) Winograd form on every stride-1 layer).
        frames_in_flight > 1: that many replicas of the model (model.replicate()) take the samples round robin, each on a HIP
        stream of its own - loading and voxelizing sample i + 1 and the forwards of the samples before it overlap; a sample's
        statistics are fetched (and its line printed, in order) when frames_in_flight - 1 newer samples have been enqueued.
        Same numbers as the sequential loop: every sample runs the same kernels on the same data.
        loader_threads > 0: that many host threads read and voxelize samples ahead (dataset[idx] on the thread's current stream, an
        event hands the sample over to the consuming stream) - the file reads and npz decompression release the GIL, and at 1280x720
        they are 20 ms of a sample's 20.3 ms."""
        model.change_imagesize(self.image_size)
        model.eval()
        dev = _device_of(model)
        self.logger.write_line("test in stride {:d}".format(stride), True)
        sparse = getattr(self.dataset, "evaluation_type", "dense") == "sparse"
        mean_aee, mean_out, aee_list, out_list = 0., 0., [], []
        nfl = max(1, int(frames_in_flight))
        co = max(1, int(coalesce))
        if stream:
            nfl, co, loader_threads = 1, 0, 0                    # (co = 0: neither the coalesced nor the one-sample loop below runs)
        if co > 1:
            if not (hasattr(model, "forward_many") and hasattr(self.dataset, "get_samples")):
                raise ValueError("coalesce > 1 needs a model with forward_many (EEMFlow, EEMFlow_cdc, ERAFT) and a dataset with get_samples (HREMEventFlow)")
            co = min(co, 16)
            nfl = min(nfl, 2)                                    # two batched chains fill the chip; more only share it
        replicas, streams = [model], [torch.cuda.current_stream(dev)]
        hint_before = getattr(model, "frames_in_flight", 1)
        if nfl > 1:
            model.frames_in_flight = nfl
            replicas += [model.replicate(nfl) for _ in range(nfl - 1)]
            streams = [torch.cuda.Stream(device=dev) for _ in range(nfl)]
        pool = None
        if loader_threads > 0:                                   # ONE pool for the whole evaluation (threads are not re-created per sequence)
            import concurrent.futures
            pool = concurrent.futures.ThreadPoolExecutor(max_workers=loader_threads)
        with torch.no_grad():
            for sequence in sequence_list:
                acc = collections.defaultdict(float)
                iters, n_points = 0, 0
                self.dataset.change_test_sequence(sequence)
                pending = collections.deque()
                fb_extra = {}                                    # fb_check: sample -> (consistent share, sums over the consistent pixels)
                viz_images = {}                                  # visualize: sample -> its images, converted on the chunk's stream
                fwl_extra = {}                                   # fwl: sample -> its flow warp loss (a 0-dim device tensor)
                fwl_count = 0
                rsat_extra = {}                                  # rsat: sample -> its RSAT (a 0-dim device tensor)
                rsat_count = 0

                def warp_loss(chunk, carriers, f_ests):
                    """The chunk's flow warp losses by ONE fwl_many call on the current stream (and its RSATs by ONE rsat_many
                    call); carriers: the samples (or stream targets), each with its 'events' and 'events_offset'."""
                    flows_ = [f_[0].contiguous().float() for f_ in f_ests]
                    if fwl:
                        from .iwe import fwl_many     # (the package's attribute `iwe` is the one-job function, not the module)
                        vals = fwl_many([c_['events'] for c_ in carriers], flows_, offset=carriers[0]['events_offset'])
                        for i_, idx in enumerate(chunk):
                            fwl_extra[idx] = vals[i_]
                    if rsat:
                        from .tsimg import rsat_many
                        vals = rsat_many([c_['events'] for c_ in carriers], flows_, offset=carriers[0]['events_offset'])
                        for i_, idx in enumerate(chunk):
                            rsat_extra[idx] = vals[i_]
                writer = None
                if visualize is not None:
                    from . import viz
                    writer = self._viz_writer = viz.ImageWriter(os.path.join(visualize["save_path"], sequence, "test"))

                def convert(chunk, f_ests, f_gts, volumes, norms=None):
                    """The chunk's images: ONE conversion call for the estimated flows, one for the ground truths (and one for the
                    event volumes), on the current stream; volumes: per sample (event_volume_old, event_volume_new) [1, C, H, W]."""
                    sel = [i_ for i_, idx in enumerate(chunk) if idx % visualize["every"] == 0]
                    if not sel:
                        return
                    est = viz.flow_to_image_many([f_ests[i_].contiguous().float() for i_ in sel])
                    gt = viz.flow_to_image_many([f_gts[i_].contiguous().float() for i_ in sel])
                    ev = dens = None
                    if visualize["vis_events"]:
                        flat = [volumes[i_][j_] for j_ in (0, 1) for i_ in sel]
                        recs = [norms[i_][j_] for j_ in (0, 1) for i_ in sel] if norms is not None else None
                        ev, dens = viz.event_image_many([v_ if recs is not None else v_.contiguous().float() for v_ in flat], recs)
                    for q_, i_ in enumerate(sel):
                        viz_images[chunk[i_]] = (est[q_], gt[q_]) + ((ev[q_], ev[len(sel) + q_], dens[q_::len(sel)]) if ev is not None else ())

                def submit(idx, aee):
                    """test_mvsec.py:618-637: the file names carry the number of the sample's line."""
                    est, gt, *events = viz_images.pop(idx)
                    writer.submit('{:d}_flow_est_{:.3f}.jpg'.format(idx + 1, aee) if visualize["print_epe"] else '{:d}_flow_est.jpg'.format(idx + 1), est)
                    writer.submit('{:d}_flow_gt.jpg'.format(idx + 1), gt)
                    if events:
                        d1, d2 = events[2].tolist()
                        writer.submit('{:d}_events1_{:.3f}.jpg'.format(idx + 1, d1), events[0])
                        writer.submit('{:d}_events2_{:.3f}.jpg'.format(idx + 1, d2), events[1])

                def retire():
                    nonlocal iters, n_points, fwl_count, rsat_count
                    idx, k, sums, keep = pending.popleft()
                    with torch.cuda.stream(streams[k]):
                        aee, p1, p3, n_points, s_ee, aee_gt, s_gt = flow_error_from_sums(sums)
                        fwl_val = float(fwl_extra.pop(idx)) if idx in fwl_extra else None
                        rsat_val = float(rsat_extra.pop(idx)) if idx in rsat_extra else None
                        if idx in viz_images:
                            submit(idx, aee)
                    for name, v in (("aee", aee), ("sum", s_ee), ("aee_gt", aee_gt), ("sum_gt", s_gt), ("p1", p1), ("p3", p3)):
                        acc[name] += v
                    iters += 1
                    line = '{:05d} / {:05d}  AEE: {:2.6f}  meanAEE:{:2.6f} 3 - mean %AEE: {:.6f}'.format(
                        idx + 1, len(self.dataset), aee, acc["aee"] / iters, 1. - acc["p3"] / iters)
                    if idx in fb_extra:
                        share, sums_fb = fb_extra.pop(idx)
                        line += '  fb consistent: {:.6f}  AEE consistent: {:2.6f}'.format(float(share), flow_error_from_sums(sums_fb)[0])
                    if fwl_val is not None:
                        if fwl_val == fwl_val:                   # NaN (a constant count image) stays out of the mean
                            acc["fwl"] += fwl_val
                            fwl_count += 1
                        line += '  FWL: {:2.6f}  meanFWL:{:2.6f}'.format(fwl_val, acc["fwl"] / fwl_count if fwl_count else float("nan"))
                    if rsat_val is not None:
                        if rsat_val == rsat_val:                 # NaN (no loss under zero flow) stays out of the mean
                            acc["rsat"] += rsat_val
                            rsat_count += 1
                        line += '  RSAT: {:2.6f}  meanRSAT:{:2.6f}'.format(rsat_val, acc["rsat"] / rsat_count if rsat_count else float("nan"))
                    print(line)

                indices = [idx for idx in range(len(self.dataset)) if idx % stride == 0]
                futures = collections.deque()
                if pool is not None and co == 1:                 # (the coalesced loop reads its chunks through dataset.get_samples: no
                    def load(idx):                               # per-sample futures are submitted that nobody would consume - ADVICE round 5)
                        with torch.cuda.device(dev):
                            sample = self.dataset[idx]
                            ready = torch.cuda.Event()
                            ready.record(torch.cuda.current_stream(dev))
                        return sample, ready
                    ahead = iter(indices)
                    for idx in itertools.islice(ahead, 2 * loader_threads):
                        futures.append(pool.submit(load, idx))
                count = 0
                with_vols = {"with_volumes": True} if (visualize is not None and visualize["vis_events"]) else {}
                for chunk, targets, f_ests, *fb_masks in (stream_chunks(self.dataset, model, stream, dev, fb_check, **with_vols) if stream else ()):
                    vol_pairs = fb_masks.pop() if with_vols else None
                    f_gts = [t_['flow'].to(dev)[None].float() for t_ in targets]
                    evs_ = [t_['event_valid'].to(dev).sum(0) for t_ in targets] if (sparse and all('event_valid' in t_ for t_ in targets)) else None
                    all_sums = flow_error_sums_many(f_gts, f_ests, evs_, is_car=self.is_car,
                                                    evaluation_type="sparse" if evs_ is not None else "dense")
                    if fb_masks:
                        # the consistent pixels as the event image of the sparse statistics (of a sparse evaluation: those with events too)
                        cons = [m_[0, 0] if evs_ is None else m_[0, 0] * (evs_[i_] > 0).float() for i_, m_ in enumerate(fb_masks[0])]
                        sums_fb = flow_error_sums_many(f_gts, f_ests, cons, is_car=self.is_car, evaluation_type="sparse")
                        for i_, idx in enumerate(chunk):
                            fb_extra[idx] = (fb_masks[0][i_].mean(), sums_fb[i_])
                    if fwl or rsat:
                        warp_loss(chunk, targets, f_ests)
                    if visualize is not None:
                        convert(chunk, f_ests, f_gts, vol_pairs)
                    for i_, idx in enumerate(chunk):
                        pending.append((idx, 0, all_sums[i_], (targets[i_], f_ests[i_], f_gts[i_], evs_[i_] if evs_ is not None else None)))
                    while pending:
                        retire()
                for c0 in (range(0, len(indices), co) if co > 1 else ()):
                    chunk = indices[c0:c0 + co]
                    k = count % nfl
                    count += 1
                    with torch.cuda.stream(streams[k]):
                        samples = self.dataset.get_samples(chunk)
                        frames = [(s_['event_volume_old'].to(dev)[None].float(), s_['event_volume_new'].to(dev)[None].float()) for s_ in samples]
                        deferred = all(s_.get('deferred_norm', False) for s_ in samples)
                        if deferred:                             # (.float() / [None] keep the storage: the record stays behind the volume)
                            outs = replicas[k].forward_many(frames, deferred_norm=True)
                        else:
                            outs = replicas[k].forward_many(frames)
                        f_ests = [preds[-1] for _, preds in outs]
                        f_gts = [s_['flow'].to(dev)[None].float() for s_ in samples]
                        evs_ = [s_['event_valid'].to(dev).sum(0) for s_ in samples] if (sparse and all('event_valid' in s_ for s_ in samples)) else None
                        all_sums = flow_error_sums_many(f_gts, f_ests, evs_, is_car=self.is_car,        # the chunk's statistics by one launch
                                                        evaluation_type="sparse" if evs_ is not None else "dense")
                        if fwl or rsat:
                            warp_loss(chunk, samples, f_ests)
                        if visualize is not None:
                            norms = None
                            if deferred and visualize["vis_events"]:     # raw volumes: their records normalise them inside the kernel
                                from .voxelizer import norm_record
                                norms = [(norm_record(a_), norm_record(b_)) for a_, b_ in frames]
                            convert(chunk, f_ests, f_gts, frames, norms)
                        for i_, (idx, sample) in enumerate(zip(chunk, samples)):
                            pending.append((idx, k, all_sums[i_], (sample, f_ests[i_], f_gts[i_], evs_[i_] if evs_ is not None else None)))
                    while len(pending) >= nfl * co:
                        retire()
                for idx in (indices if co == 1 else ()):      # (co == 0: the stream walk above)
                    k = count % nfl
                    count += 1
                    with torch.cuda.stream(streams[k]):
                        if pool is not None:
                            sample, ready = futures.popleft().result()
                            streams[k].wait_event(ready)
                            for nidx in itertools.islice(ahead, 1):
                                futures.append(pool.submit(load, nidx))
                        else:
                            sample = self.dataset[idx]
                        f_est = self.run_network(replicas[k], sample, dev)
                        f_gt = sample['flow'].to(dev)[None].float()
                        ev = sample['event_valid'].to(dev).sum(0) if ('event_valid' in sample and sparse) else None
                        sums = flow_error_sums(f_gt, f_est, ev, is_car=self.is_car, evaluation_type="sparse" if ev is not None else "dense")
                        if fwl or rsat:
                            warp_loss([idx], [sample], [f_est])
                        if visualize is not None and idx % visualize["every"] == 0:
                            vols_ = [(sample['event_volume_old'].to(dev)[None], sample['event_volume_new'].to(dev)[None])] if visualize["vis_events"] else None
                            convert([idx], [f_est], [f_gt], vols_)
                    pending.append((idx, k, sums, (sample, f_est, f_gt, ev)))     # the tensors stay alive until the sample retires
                    while len(pending) >= nfl:
                        retire()
                while pending:
                    retire()
                if writer is not None:
                    writer.close()                               # joins the encoders; a worker's error surfaces here
                    del self._viz_writer
                iters = max(iters, 1)
                self.logger.write_line("-------------------test_sequence_{:s}------------------".format(sequence), True)
                self.logger.write_line(
                    "Mean AEE: {:.6f}, sum AEE: {:.6f}, Mean AEE_gt: {:.6f}, sum AEE_gt: {:.6f}, 1 - mean %AEE: {:.6f}, "
                    "3 - mean %AEE: {:.6f}, # pts: {:.6f}".format(acc["aee"] / iters, acc["sum"] / iters, acc["aee_gt"] / iters,
                                                                  acc["sum_gt"] / iters, 1. - acc["p1"] / iters,
                                                                  1. - acc["p3"] / iters, n_points), True)
                if fwl:
                    self.logger.write_line("Mean FWL: {:.6f}".format(acc["fwl"] / fwl_count if fwl_count else float("nan")), True)
                if rsat:
                    self.logger.write_line("Mean RSAT: {:.6f}".format(acc["rsat"] / rsat_count if rsat_count else float("nan")), True)
                mean_aee += acc["aee"] / iters
                mean_out += 1. - acc["p3"] / iters
                aee_list.append(acc["aee"] / iters)
                out_list.append(1. - acc["p3"] / iters)
        if pool is not None:
            pool.shutdown()
        model.frames_in_flight = hint_before
        self.logger.write_line("-------------------------------------------------------", True)
        self.logger.write_line("-----------------Test after {:d} epoch-----------------".format(epoch), True)
        for name, a, o in zip(sequence_list, aee_list, out_list):
            self.logger.write_line("{:s}: Mean AEE: {:.6f},  3 - mean %AEE: {:.6f}".format(name, a, o), True)
        self.logger.write_line("-------------------------------------------------------", True)
        n = max(len(sequence_list), 1)
        self.logger.write_line("Average points: Mean AEE: {:.6f},  3 - mean %AEE: {:.6f}".format(mean_aee / n, mean_out / n), True)
        return mean_aee / n


def _target_like(pred, flow_gt, valid):
    """HREM's training target is the 16x16 mesh flow (HREM.py:254-255).  A model that predicts at another size (E-RAFT and EEMFlow+
    at full resolution) is trained against that mesh flow taken to its size the way the dataset's own evaluation branch does it
    (HREM.py:264-267: bilinear, align_corners=False; valid = finite and non-zero) - the library's resize kernel, not a torch op."""
    if tuple(flow_gt.shape[-2:]) == tuple(pred.shape[-2:]):
        return flow_gt, valid
    from . import _lib
    b, _, h, w = flow_gt.shape
    oh, ow = int(pred.shape[-2]), int(pred.shape[-1])
    src = flow_gt.contiguous()
    full = torch.empty(b, 2, oh, ow, device=src.device, dtype=torch.float32)
    _lib.check(_lib.lib().eemflow_upsample_bilinear(src.data_ptr(), full.data_ptr(), 2 * b, h, w, oh, ow, _lib.current_stream_ptr(src.device)))
    ok = (~torch.isinf(full[:, 0])) & (~torch.isinf(full[:, 1])) & (torch.linalg.norm(full, dim=1) > 0)
    return full, ok.float()


class TrainRaftEvents:
    """Training loop of train_mvsec.py:229-286 (one process per GPU; batches are this rank's shard).

    A loader that assembles its batches on the device (loader.ThreadedBatchLoader(device_batches=True)) needs nothing else here: the
    loops' `batch[key].to(dev).float()` returns the very tensor when it is float32 and already on `dev` (Tensor.to and Tensor.float
    return self when nothing changes; tests/test_gpu_augment.py holds the data pointers equal), so no copy is made.

    contrast_weight / supervised (the autograd engine only): the loss is sequence_loss + contrast_weight * train.contrast_loss(last
    prediction, batch['events'], batch['events_map']) - minus the mean flow warp loss of the batch, the ground-truth-free contrast
    term; supervised=False trains on the contrast term alone and reads neither batch['flow'] nor batch['valid'].  The batches must
    carry their events (a dataset built with with_events=True; get_batch adds 'events_map', batches without it use 'events_offset'),
    and the prediction must be at the event frame's size (not out_mesh_size).

    timestamp_weight (the autograd engine only): timestamp_weight * train.timestamp_loss(last prediction, batch['events'],
    batch['events_map']) is added to the loss - the average-timestamp term (tsimg.py), beside the contrast term and under its rules:
    the batches carry their events, the prediction is at the event frame's size.  supervised=False is satisfied by a timestamp_weight
    alone.  With timestamp_weight == 0 nothing is computed and nothing changes.

    smooth_weight (the autograd engine only): smooth_weight * train.smoothness_loss(predictions, batch['event_volume_old'] as the
    model received it) is added to the loss - the edge-aware smoothness regulariser of order smooth_order with smooth_constant,
    smooth_weight_type ('gauss', 'exp') and smooth_error ('L1', 'abs_robust'); of the last prediction, or with smooth_all=True of all
    predictions under the engine's gamma.  A prediction at mesh size (out_mesh_size=True) has no edge image of its size and is
    regularised unweighted (img=None).  supervised=False still needs a contrast_weight: smoothness alone is minimised by a constant
    flow.  With smooth_weight == 0 nothing is computed and nothing changes.

    photo_weight (the autograd engine only): photo_weight * train.photo_loss(predictions, event_volume_old, event_volume_new as the
    model received them) is added to the loss - the photometric ('abs_robust', 'charbonnier', 'L1') or 'census' loss between the old
    volume and the new one warped back by the prediction, photo_q / photo_charbonnier / photo_max_distance being census's settings; of
    the last prediction, or with photo_all=True of all predictions under the engine's gamma.  The prediction must be at the frame's
    size.  photo_occ=True runs model(new, old) under torch.no_grad(), takes mask_fw of metrics.fb_check(final forward flow, final
    backward flow) and hands it to the loss with use_occ=True; a model whose BatchNorm layers are in train mode (E-RAFT before
    freeze_bn()) is refused, because the second pass would move their running statistics.  supervised=False is satisfied by a
    contrast_weight or a photo_weight.  With photo_weight == 0 nothing is computed and nothing changes.

    ssim_weight (the autograd engine only): ssim_weight * train.ssim_loss(predictions, event_volume_old, event_volume_new as the model
    received them) is added to the loss - the weighted SSIM between the old volume and the new one warped back by the prediction, with
    ssim_c1 / ssim_c2 regularising its luminance / structure term (inf switches one off; the reference's default is the structure
    term alone); of the last prediction, or with ssim_all=True of all predictions under the engine's gamma.  The prediction must be at
    the frame's size.  ssim_occ=True weights the moments and the mean by mask_fw of the same gradient-free exchanged pass as
    photo_occ - it runs once per step when both are on.  supervised=False is satisfied by an ssim_weight too.  With ssim_weight == 0
    nothing is computed and nothing changes."""

    def __init__(self, loader, image_size, lr=1e-4, wdecay=5e-5, epsilon=1e-8, num_steps=1000000, clip=1.0, gamma=0.8,
                 logger=None, print_freq=100, engine="fused", mixed_precision=True, start_iteration=0, contrast_weight=0.0,
                 supervised=True, smooth_weight=0.0, smooth_order=1, smooth_constant=1.0, smooth_weight_type="gauss", smooth_error="L1",
                 smooth_all=False, photo_weight=0.0, photo_kind="census", photo_occ=False, photo_all=False, photo_q=0.4,
                 photo_charbonnier=False, photo_max_distance=3, ssim_weight=0.0, ssim_occ=False, ssim_all=False, ssim_c1=float("inf"),
                 ssim_c2=9e-6, timestamp_weight=0.0):
        if engine not in ("fused", "autograd"):
            raise ValueError("engine must be 'fused' or 'autograd'")
        self.contrast_weight, self.supervised = float(contrast_weight), bool(supervised)
        self.timestamp_weight = float(timestamp_weight)
        if engine == "fused" and self.timestamp_weight != 0.0:
            raise ValueError("TrainRaftEvents: the average-timestamp term (timestamp_weight != 0) is honoured by engine='autograd' only - "
                             "the fused trainer has no average-timestamp term")
        if engine == "fused" and (self.contrast_weight != 0.0 or not self.supervised):
            raise ValueError("TrainRaftEvents: the contrast term (contrast_weight != 0, supervised=False) is honoured by engine='autograd' "
                             "only - the fused trainer has no contrast term")
        self.photo_weight, self.photo_occ, self.photo_all = float(photo_weight), bool(photo_occ), bool(photo_all)
        self.photo_kw = dict(kind=photo_kind, q=photo_q, charbonnier=photo_charbonnier, max_distance=photo_max_distance)
        if self.photo_weight != 0.0:
            if engine == "fused":
                raise ValueError("TrainRaftEvents: the photometric term (photo_weight != 0) is honoured by engine='autograd' only - the "
                                 "fused trainer has no photometric term")
            from .photo import _settings as photo_settings
            photo_settings("TrainRaftEvents", photo_kind, photo_occ, photo_q, photo_charbonnier, True, photo_max_distance)
        self.ssim_weight, self.ssim_occ, self.ssim_all = float(ssim_weight), bool(ssim_occ), bool(ssim_all)
        self.ssim_kw = dict(c1=float(ssim_c1), c2=float(ssim_c2))
        if self.ssim_weight != 0.0:
            if engine == "fused":
                raise ValueError("TrainRaftEvents: the SSIM term (ssim_weight != 0) is honoured by engine='autograd' only - the fused "
                                 "trainer has no SSIM term")
            from .ssim import _settings as ssim_settings
            ssim_settings("TrainRaftEvents", ssim_occ, ssim_c1, ssim_c2, 0.01)
        if (not self.supervised and self.contrast_weight == 0.0 and self.photo_weight == 0.0 and self.ssim_weight == 0.0
                and self.timestamp_weight == 0.0):
            raise ValueError("TrainRaftEvents: supervised=False leaves no loss without a contrast_weight or a photo_weight (or an "
                             "ssim_weight or a timestamp_weight)")
        self.smooth_weight, self.smooth_all = float(smooth_weight), bool(smooth_all)
        self.smooth_kw = dict(order=smooth_order, constant=smooth_constant, weight_type=smooth_weight_type, error_type=smooth_error)
        if self.smooth_weight != 0.0:
            if engine == "fused":
                raise ValueError("TrainRaftEvents: the smoothness term (smooth_weight != 0) is honoured by engine='autograd' only - the "
                                 "fused trainer has no smoothness term")
            from .smooth import _settings
            _settings("TrainRaftEvents", smooth_order, smooth_constant, smooth_weight_type, smooth_error)
        self.loader, self.image_size = loader, image_size
        self.opt = dict(lr=lr, wdecay=wdecay, epsilon=epsilon, num_steps=num_steps, clip=clip, gamma=gamma)
        self.logger = logger or Logger()
        self.print_freq = print_freq
        self.engine, self.mixed_precision = engine, mixed_precision
        self.trainer = None
        self.optimizer = self.scheduler = self.scaler = None
        self.iteration = int(start_iteration)                   # resume: the OneCycle schedule continues where the checkpoint stopped

    def fetch_optimizer(self, model):
        """train_mvsec.py:178-183."""
        o = self.opt
        self.optimizer = torch.optim.AdamW(filter(lambda p: p.requires_grad, model.parameters()), lr=o["lr"], weight_decay=o["wdecay"],
                                           eps=o["epsilon"])
        self.scheduler = torch.optim.lr_scheduler.OneCycleLR(self.optimizer, o["lr"], o["num_steps"] + 100, pct_start=0.05,
                                                             cycle_momentum=False, anneal_strategy='linear')

    def _train_iters_autograd(self, model, start_epoch, val_iters):
        """The body of train_mvsec.py:241-258, statement for statement; in data-parallel jobs the parameter gradients are
        averaged by one RCCL all-reduce of a flat buffer before the clip (what DataParallel's gather/scatter amounts to)."""
        dev = _device_of(model)
        if self.optimizer is None:
            self.fetch_optimizer(model)
            self.scaler = torch.amp.GradScaler("cuda", enabled=self.mixed_precision)
            if self.iteration:
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")             # "scheduler.step() before optimizer.step()": positions only
                    for _ in range(self.iteration):
                        self.scheduler.step()
        done = 0
        for batch in self.loader:
            self.optimizer.zero_grad()
            if self.contrast_weight != 0.0:
                self._contrast_inputs(batch)                       # (before any GPU work: a loader without events fails at once)
            if self.timestamp_weight != 0.0:
                self._contrast_inputs(batch, "timestamp_weight")
            e1 = batch['event_volume_old'].to(dev).float()
            e2 = batch['event_volume_new'].to(dev).float()
            need_back = (self.photo_weight != 0.0 and self.photo_occ) or (self.ssim_weight != 0.0 and self.ssim_occ)
            back = self._photo_backward_flow(model, e1, e2) if need_back else None     # (one exchanged pass serves both terms)
            _, flow_list = model(e1, e2)
            if self.supervised:
                flow_gt, valid = _target_like(flow_list[-1], batch['flow'].to(dev).float(), batch['valid'].to(dev).float())
                loss, metrics = sequence_loss(flow_list, flow_gt, valid, self.opt["gamma"])
            else:
                loss, metrics = 0.0, {"epe": float("nan")}
            if self.contrast_weight != 0.0:
                loss = loss + self.contrast_weight * self._contrast_term(flow_list[-1], batch, e1)
            if self.timestamp_weight != 0.0:
                loss = loss + self.timestamp_weight * self._timestamp_term(flow_list[-1], batch, e1)
            if self.smooth_weight != 0.0:
                loss = loss + self.smooth_weight * self._smooth_term(flow_list, e1)
            if self.photo_weight != 0.0:
                loss = loss + self.photo_weight * self._photo_term(flow_list, e1, e2, back)
            if self.ssim_weight != 0.0:
                loss = loss + self.ssim_weight * self._ssim_term(flow_list, e1, e2, back)
            self.scaler.scale(loss).backward()
            if parallel.exchange_active():
                # the still-SCALED gradients are exchanged, then unscaled: an overflow on one rank reaches every rank through the
                # sum, so all ranks record the same found_inf, skip the same step and keep the same scale
                params = [p for p in model.parameters() if p.grad is not None]
                flat = torch.cat([p.grad.reshape(-1) for p in params])
                parallel.average_gradients(flat)
                off = 0
                for p in params:
                    p.grad.copy_(flat[off:off + p.numel()].view_as(p))
                    off += p.numel()
            self.scaler.unscale_(self.optimizer)
            torch.nn.utils.clip_grad_norm_(model.parameters(), self.opt["clip"])
            lr = self.optimizer.param_groups[0]["lr"]
            self.scaler.step(self.optimizer)
            self.scheduler.step()
            self.scaler.update()
            done += 1
            self.iteration += 1
            if done % self.print_freq == 0 or done == 1:
                self.logger.write_line("[epoch {:d}, {:6d}] loss {:.6f} epe {:.4f} lr {:.3e}".format(
                    start_epoch, self.iteration, loss.item(), metrics["epe"], lr), True)
            if val_iters is not None and done >= val_iters:
                break
        return model

    @staticmethod
    def _contrast_inputs(batch, what="contrast_weight"):
        """(event sets, maps) of a batch for the contrast term (and the average-timestamp term): 'events_map' where get_batch made one,
        else the pure offset maps."""
        if 'events' not in batch:
            raise ValueError(f"TrainRaftEvents: {what} needs batches that carry their events - build the dataset with "
                             "with_events=True (its get_batch / samples then have 'events')")
        maps = batch.get('events_map')
        if maps is None:
            maps = [(1.0, -float(o[0]), 1.0, -float(o[1])) for o in batch.get('events_offset', [(0, 0)] * len(batch['events']))]
        return list(batch['events']), list(maps)

    @classmethod
    def _contrast_term(cls, flow_pred, batch, volume):
        """train.contrast_loss of the last prediction on the batch's events (float32, as the supervised loss is)."""
        events, maps = cls._contrast_inputs(batch)
        if tuple(flow_pred.shape[-2:]) != tuple(volume.shape[-2:]):
            raise ValueError(f"TrainRaftEvents: the contrast term needs the prediction at the event frame's size {tuple(volume.shape[-2:])}, "
                             f"got {tuple(flow_pred.shape[-2:])} - a model with out_mesh_size=True predicts the mesh flow")
        return contrast_loss(flow_pred, events, maps).float()

    @classmethod
    def _timestamp_term(cls, flow_pred, batch, volume):
        """train.timestamp_loss of the last prediction on the batch's events (float32, as the supervised loss is)."""
        events, maps = cls._contrast_inputs(batch, "timestamp_weight")
        if tuple(flow_pred.shape[-2:]) != tuple(volume.shape[-2:]):
            raise ValueError(f"TrainRaftEvents: the average-timestamp term needs the prediction at the event frame's size "
                             f"{tuple(volume.shape[-2:])}, got {tuple(flow_pred.shape[-2:])} - a model with out_mesh_size=True predicts "
                             "the mesh flow")
        return timestamp_loss(flow_pred, events, maps).float()

    def _smooth_term(self, flow_list, volume):
        """train.smoothness_loss of the predictions against the old event volume (float32, as the supervised loss is); a prediction
        at another size than the volume (the mesh flow) is regularised unweighted."""
        img = volume if tuple(flow_list[-1].shape[-2:]) == tuple(volume.shape[-2:]) else None
        return smoothness_loss(flow_list, img, gamma=self.opt["gamma"] if self.smooth_all else None, **self.smooth_kw).float()

    @staticmethod
    def _photo_backward_flow(model, e1, e2):
        """The final flow of a gradient-free pass with the volumes exchanged, for photo_occ's mask.  It runs BEFORE the pass that is
        differentiated, so whatever the model keeps between its forward and its backward belongs to that one."""
        if any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training for m in model.modules()):
            raise ValueError("TrainRaftEvents: photo_occ=True runs the model a second time, which would move the running statistics of "
                             "its train-mode BatchNorm layers - freeze them first (E-RAFT: freeze_bn())")
        with torch.no_grad():
            _, back = model(e2, e1)
        return back[-1].float().contiguous()

    def _photo_term(self, flow_list, e1, e2, back):
        """train.photo_loss of the predictions between the two event volumes (float32, as the supervised loss is); with photo_occ the
        mask is mask_fw of the forward-backward check of the final prediction against `back`."""
        if tuple(flow_list[-1].shape[-2:]) != tuple(e1.shape[-2:]):
            raise ValueError(f"TrainRaftEvents: the photometric term needs the prediction at the event frame's size {tuple(e1.shape[-2:])}, "
                             f"got {tuple(flow_list[-1].shape[-2:])} - a model with out_mesh_size=True predicts the mesh flow")
        mask = None
        if self.photo_occ:
            from .metrics import fb_check
            mask = fb_check(flow_list[-1].detach().float().contiguous(), back)[0]
        return photo_loss(flow_list, e1, e2, gamma=self.opt["gamma"] if self.photo_all else None, mask=mask, use_occ=self.photo_occ,
                          **self.photo_kw).float()

    def _ssim_term(self, flow_list, e1, e2, back):
        """train.ssim_loss of the predictions between the two event volumes (float32, as the supervised loss is); with ssim_occ the
        mask is mask_fw of the forward-backward check of the final prediction against `back`."""
        if tuple(flow_list[-1].shape[-2:]) != tuple(e1.shape[-2:]):
            raise ValueError(f"TrainRaftEvents: the SSIM term needs the prediction at the event frame's size {tuple(e1.shape[-2:])}, "
                             f"got {tuple(flow_list[-1].shape[-2:])} - a model with out_mesh_size=True predicts the mesh flow")
        mask = None
        if self.ssim_occ:
            from .metrics import fb_check
            mask = fb_check(flow_list[-1].detach().float().contiguous(), back)[0]
        return ssim_loss(flow_list, e1, e2, gamma=self.opt["gamma"] if self.ssim_all else None, mask=mask, use_occ=self.ssim_occ,
                         **self.ssim_kw).float()

    def train_iters(self, model, start_epoch=0, val_iters=None):
        if self.image_size is None:                              # padder sized from the data (cli: un-cropped HREM frames)
            ds = getattr(self.loader, "dataset", None)
            first = ds[0] if ds is not None else next(iter(self.loader))
            self.image_size = tuple(int(v) for v in first['event_volume_old'].shape[-2:])
        model.change_imagesize(self.image_size)
        model.train()
        dev = _device_of(model)
        if self.engine == "autograd":
            return self._train_iters_autograd(model, start_epoch, val_iters)
        if self.trainer is None:
            self.trainer = EEMFlowTrainer(model, **self.opt)
            self.trainer.iteration = self.iteration
        done = 0
        for batch in self.loader:
            e1 = batch['event_volume_old'].to(dev).float()
            e2 = batch['event_volume_new'].to(dev).float()
            loss, metrics, _ = self.trainer.step(e1, e2, batch['flow'].to(dev).float(), batch['valid'].to(dev).float())
            done += 1
            if done % self.print_freq == 0 or done == 1:
                self.logger.write_line("[epoch {:d}, {:6d}] loss {:.6f} epe {:.4f} lr {:.3e}".format(
                    start_epoch, self.trainer.iteration, loss, metrics["epe"], metrics["lr"]), True)
            if val_iters is not None and done >= val_iters:
                break
        return model
