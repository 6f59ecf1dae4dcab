"""MVSEC event-pair datasets feeding the GPU voxelizer (reference: loader/MVSEC.py:23-283, loader_utils.py:41-51).

`MvsecEventFlow` (dt1) and `MvsecEventFlow_dt4` keep the reference's args dict, directory layout, sequence frame ranges
and sample keys; `root` replaces its hard-wired repository path:

    <root>/dataset/MVSEC/<sequence>/event/%06d.h5          per-frame pandas tables 'myDataset' with ts, x, y, p
    <root>/dataset/MVSEC/<sequence>/flowgt_dt{1,4}/%d.npy  ground-truth flow, (2,H,W) or (H,W,2)
    <root>/dataset/MVSEC_test/indoor_flying1/...           the dt1 exception of MVSEC.py:75-78

Event files: the reference reads them with pandas.read_hdf (PyTables).  That is still the default reader here and it
fails loudly where PyTables is missing; `events_reader=callable(path) -> (N,4) float64 [ts, x, y, p]` replaces it, and a
`%06d.npz` with arrays ts, x, y, p next to (or instead of) the .h5 is read directly (the exported form for machines
without PyTables).

Differences, all deliberate:
  * the voxel volumes stay on the GPU unless `to_cpu=True` (the reference voxelizes on the GPU and copies back);
  * the shipped module cannot be imported as is: it takes FlowAugmentor / DenseSparseAugmentor from loader_utils, which
    does not define them (MVSEC.py:20); they are in utils/augumentor.py and restated in eemflow_amd/augmentor.py.  With
    'aug_params' in args a training sample goes through DenseSparseAugmentor (flips + random crop, MVSEC.py:170-187);
    without it samples are returned un-augmented (the reference would crash there), or through a caller-supplied
    `augmentor=callable(event1, event2, flow) -> (event1, event2, flow)` (HWC numpy, MVSEC.py:183);
  * dt4: the reference's `events0.sort_values(by=['ts'])` discards its result (MVSEC.py:256-258); what orders the
    concatenated events is EventSequence's own sort, as here.
"""
import os

import numpy as np
import torch

from .voxelizer import EventSequence, EventSequenceToVoxelGrid_Pytorch

Valid_Time_Index = {                                  # MVSEC.py:23-30
    'indoor_flying1': [(314, 2199)],
    'indoor_flying2': [(314, 2199)],
    'indoor_flying3': [(314, 2199)],
    'indoor_flying4': [(196, 570)],
    'outdoor_day1': [(245, 3000)],
    'outdoor_day2': [(4375, 7002)],
}


def get_events(event_path):
    """(N,4) float64 [ts, x, y, p] of one frame's events (loader_utils.py:41-51).  `<stem>.npz` (arrays ts, x, y, p) is
    preferred when present; otherwise the pandas/PyTables table 'myDataset'."""
    npz = os.path.splitext(event_path)[0] + ".npz"
    if os.path.exists(npz):
        with np.load(npz) as f:
            return np.stack([f[k].astype(np.float64) for k in ("ts", "x", "y", "p")], axis=1)
    if not os.path.exists(event_path):
        raise FileNotFoundError(event_path)           # the reference prints and returns 0, which then fails later
    try:
        import pandas
        frame = pandas.read_hdf(event_path, "myDataset")
    except ImportError as e:                          # PyTables missing
        raise RuntimeError(f"reading {event_path} needs pandas + PyTables ({e}); export the table to "
                           f"{npz} (arrays ts, x, y, p) or pass events_reader=") from e
    return frame[['ts', 'x', 'y', 'p']].to_numpy().astype(np.float64)


def center_crop(x, size):
    """torchvision.transforms.CenterCrop((th, tw)) on the last two dims (MVSEC.py:52,193-197): top = round((H-th)/2),
    left = round((W-tw)/2), Python round (banker's) as torchvision uses."""
    th, tw = size
    h, w = x.shape[-2:]
    if h < th or w < tw:
        raise ValueError(f"center_crop: {h}x{w} is smaller than {th}x{tw}")
    top, left = int(round((h - th) / 2.0)), int(round((w - tw) / 2.0))
    return x[..., top:top + th, left:left + tw]


def event_mask(features, height, width):
    """`np.histogram2d(x, y, bins=(w,h), range=[[0,w],[0,h]]).T > 0` of MVSEC.py:143-151 for integer-valued or
    fractional coordinates: pixel (y, x) holds floor(x), floor(y) for 0 <= x < w (x == w falls into the last bin)."""
    x, y = features[:, 1], features[:, 2]
    ok = (x >= 0) & (x <= width) & (y >= 0) & (y <= height)
    xi = np.minimum(np.floor(x[ok]).astype(np.int64), width - 1)
    yi = np.minimum(np.floor(y[ok]).astype(np.int64), height - 1)
    mask = np.zeros(height * width, dtype=bool)
    mask[yi * width + xi] = True
    return mask.reshape(height, width)


class MvsecEventFlow(torch.utils.data.Dataset):
    """dt1 pairs: events of frame i+1 (old) and i+2 (new) with flowgt_dt1/i.npy (MVSEC.py:32-199)."""

    image_width = 346
    image_height = 260
    frames_per_volume = 1
    flow_dir = 'flowgt_dt1'
    # sample i is windows i and i + 1 of one sequence (MVSEC.py:115-116, :247-251): a stride-1 walk can encode every window once
    # (harness.TestRaftEvents.test_multi_sequence(stream=n), EEMFlow.forward_stream)
    consecutive_windows = True

    def __init__(self, args, train=True, root=None, device=None, to_cpu=False, augmentor=None, events_reader=None,
                 valid_time_index=None, with_events=False):
        """with_events: every sample (and every target of get_windows) also carries 'events', the OLD window's (N,4) float64 device
        tensor [t, x, y, p] - uploaded once, the voxelizer reads the same tensor - and 'events_offset', (ox, oy) of the evaluation
        crop in event coordinates (the centre crop's left / top; (0, 0) for un-cropped training samples): what eemflow_amd.iwe.fwl_many
        takes beside the predicted flow."""
        super().__init__()
        self.with_events = bool(with_events)
        self.input_type = 'events'
        self.type = 'train' if train else 'val'
        self.evaluation_type = args['eval_type']
        self.root = root if root is not None else os.environ.get("EEMFLOW_DATA_ROOT", os.getcwd())
        self.device = torch.device(device if device is not None else "cuda:0")
        self.to_cpu = to_cpu
        self.read_events = events_reader or get_events
        self.valid_time_index = valid_time_index or Valid_Time_Index
        self.num_bins = args['num_voxel_bins']
        self.voxel = EventSequenceToVoxelGrid_Pytorch(num_bins=self.num_bins, normalize=True, gpu=True,
                                                      gpu_nr=self.device.index or 0, forkserver=False)
        self.dense_augmentor = None
        if 'aug_params' in args and augmentor is None and train:
            # MVSEC.py:54-57 (which imports the classes from loader_utils, where they are not defined; they live in
            # utils/augumentor.py): samples carry d_event_volume_* keys, so __getitem__ takes the dense-sparse one (:170-176)
            from .augmentor import DenseSparseAugmentor
            self.dense_augmentor = DenseSparseAugmentor(**args['aug_params'])
        self.augmentor = augmentor
        self.change_test_sequence(args['sequence'])

    # ---------------------------------------------------------------------------------------- file lists
    def _dirs(self, sequence):
        if self.frames_per_volume == 1 and sequence == 'indoor_flying1':              # MVSEC.py:75-78
            base = os.path.join(self.root, 'dataset/MVSEC_test', sequence)
        else:
            base = os.path.join(self.root, 'dataset/MVSEC', sequence)
        return os.path.join(base, self.flow_dir), os.path.join(base, 'event')

    def change_test_sequence(self, sequence):
        self.names = [ind for s in self.valid_time_index[sequence] for ind in range(s[0], s[1])]
        self.sequence = 'outdoor_day1' if 'outdoor_day1' in sequence else sequence
        self.flowgt_path, self.event_path = self._dirs(self.sequence)
        if self.frames_per_volume == 1 and self.sequence == 'indoor_flying1':
            self.sequence = 'indoor_flying1_new'
        self.flow_list = [os.path.join(self.flowgt_path, '{:d}.npy'.format(i)) for i in self.names]
        self.event_list = [os.path.join(self.event_path, '{:06d}.h5'.format(i + 1)) for i in self.names]
        last = self.names[-1]
        extra = 1 if self.frames_per_volume == 1 else 5                                # MVSEC.py:93 / :226-227
        self.event_list += [os.path.join(self.event_path, '{:06d}.h5'.format(last + 2 + j)) for j in range(extra)]

    def summary(self, logger):
        logger.write_line("================================== Dataloader Summary ====================================", True)
        logger.write_line("Loader Type:\t\t" + self.__class__.__name__ + " for {}".format(self.type), True)

    def __len__(self):
        return len(self.names)

    # ---------------------------------------------------------------------------------------- one sample
    def _sequence(self, paths):
        feats = np.concatenate([np.asarray(self.read_events(p), dtype=np.float64) for p in paths], axis=0)
        return EventSequence(None, {'height': self.image_height, 'width': self.image_width}, features=feats,
                             timestamp_multiplier=1e6, convert_to_relative=True)

    def _upload(self, seq):
        """with_events: the sequence's events move to the device once (the voxelizer takes device-resident features); returns the host array."""
        host = seq.features
        if self.with_events:
            seq.features = torch.from_numpy(np.ascontiguousarray(host.astype('float'))).to(self.device)
        return host

    def _crop_offset(self):
        """(ox, oy) of center_crop's 256 x 256 evaluation window (its left and top)."""
        if self.type != 'val':
            return (0, 0)
        return (int(round((self.image_width - 256) / 2.0)), int(round((self.image_height - 256) / 2.0)))

    def get_sample(self, idx):
        flow = np.load(self.flow_list[idx])
        if flow.shape[-1] == 2:
            flow = flow.transpose(2, 0, 1)
        out = {'idx': self.names[idx], 'flow': torch.from_numpy(np.ascontiguousarray(flow)), 'valid': None}
        k = self.frames_per_volume
        n = len(self.event_list)
        old = self._sequence([self.event_list[idx + i] for i in range(k)])                      # MVSEC.py:119,247
        new = self._sequence([self.event_list[(idx + i + 1) % n] for i in range(k)])            # :120,251
        old_host = self._upload(old)
        vol_old, vol_new = self.voxel.pair(old, new)              # both volumes in one three-launch sequence
        if self.with_events:
            out['events'], out['events_offset'] = old.features, self._crop_offset()
        if self.to_cpu:
            vol_new, vol_old = vol_new.cpu(), vol_old.cpu()
        out['event_volume_new'] = out['d_event_volume_new'] = vol_new
        out['event_volume_old'] = out['d_event_volume_old'] = vol_old
        if self.type == 'val':
            out['event_valid'] = torch.from_numpy(event_mask(old_host, self.image_height,
                                                             self.image_width)).unsqueeze(dim=0)
        return out

    def _window_paths(self, j):
        """The event files of window j: event_volume_old of sample j, event_volume_new of sample j - 1."""
        n = len(self.event_list)
        return [self.event_list[(j + i) % n] for i in range(self.frames_per_volume)]

    def get_windows(self, first, count):
        """Windows first .. first + count - 1 of the sequence, each read and voxelized once (ONE voxelizer launch sequence for all), and
        the evaluation targets of the samples that start at them: returns (volumes, targets) - volumes[i] the [C, 256, 256] volume of window
        first + i, cropped as __getitem__ crops it; targets[i] the dict of sample first + i ('idx', 'flow', 'valid', 'event_valid', the
        same values as __getitem__ gives), None past the last sample (the last window only ends a sample).  Evaluation datasets only."""
        if self.type != 'val':
            raise ValueError("get_windows: evaluation datasets only (train=False); training samples are augmented pair by pair")
        if first < 0 or count < 1 or first + count > len(self) + 1:
            raise ValueError(f"get_windows: windows {first}..{first + count - 1} of a sequence of {len(self)} samples ({len(self) + 1} windows)")
        seqs = [self._sequence(self._window_paths(j)) for j in range(first, first + count)]
        hosts = [self._upload(s) for s in seqs]
        vols = self.voxel.many(seqs)
        crop = (256, 256)                                                                       # MVSEC.py:52,193-197
        volumes, targets = [], []
        for i, j in enumerate(range(first, first + count)):
            vol = vols[i].cpu() if self.to_cpu else vols[i]
            volumes.append(center_crop(vol, crop))
            if j >= len(self):
                targets.append(None)
                continue
            flow = np.load(self.flow_list[j])
            if flow.shape[-1] == 2:
                flow = flow.transpose(2, 0, 1)
            fl = center_crop(torch.from_numpy(np.ascontiguousarray(flow)), crop)
            ev = torch.from_numpy(event_mask(hosts[i], self.image_height, self.image_width)).unsqueeze(dim=0)
            targets.append({'idx': self.names[j], 'flow': fl, 'valid': (fl[0].abs() < 1000) & (fl[1].abs() < 1000),
                            'event_valid': center_crop(ev, crop)})
            if self.with_events:
                targets[-1]['events'], targets[-1]['events_offset'] = seqs[i].features, self._crop_offset()
        return volumes, targets

    # ---------------------------------------------------------------------------------------- batches assembled on the device
    def _batch_augmentor(self):
        if self.type != 'train':
            raise ValueError("get_batch: training datasets only (train=True); evaluation samples are centre-cropped - get_windows serves them")
        aug = self.dense_augmentor if self.dense_augmentor is not None else self.augmentor
        if aug is not None and not hasattr(aug, "draw"):
            raise ValueError("get_batch: the augmentor is a callable without draw(): its samples keep the host route (dataset[i])")
        return aug

    def draw_plans(self, idxs):
        """One AugPlan per sample, drawn from numpy.random in sample order - the draws `[self[i] for i in idxs]` would make."""
        from .augmentor import AugPlan
        aug = self._batch_augmentor()
        h, w = self.image_height, self.image_width
        return [aug.draw(h, w) if aug is not None else AugPlan(h, w) for _ in idxs]

    def read_sample(self, idx):
        """The host part of sample idx (its flow and two event sequences, as get_sample reads them): what get_batch takes as `reads`,
        so that a loader can read ahead on threads."""
        idx = idx % len(self)
        flow = np.load(self.flow_list[idx])
        if flow.shape[-1] == 2:
            flow = flow.transpose(2, 0, 1)
        flow = np.ascontiguousarray(flow)
        if flow.dtype not in (np.float32, np.float64):
            flow = flow.astype(np.float64)                        # what the host's `flow * [-1.0, 1.0]` / .float() make of it
        k, n = self.frames_per_volume, len(self.event_list)
        old = self._sequence([self.event_list[idx + i] for i in range(k)])
        new = self._sequence([self.event_list[(idx + i + 1) % n] for i in range(k)])
        self._upload(old)
        return {'idx': self.names[idx], 'flow': torch.from_numpy(flow)}, (old, new)

    def get_batch(self, idxs, plans=None, reads=None):
        """The stacked batch of `[self[i] for i in idxs]` - the same keys, dtypes, shapes and bits - with every tensor on the device and
        the event volumes never on the host: the samples are voxelized in groups of up to 16 (voxel.many) and each group is rescaled /
        flipped / cropped straight into the batch tensors by one launch (augmentor.augment_many), flow and `valid` with them.  With
        'aug_params' the d_event_volume_* keys are the event_volume_* tensors themselves (the host route passes the same arrays twice);
        with a caller's FlowAugmentor, or none, they are the un-augmented volumes, as the host route leaves them.  plans: the samples'
        AugPlans (default: drawn here, in sample order); reads: their read_sample results (default: read here).  With with_events=True the
        batch also carries 'events_map', one (ax, bx, ay, by) per sample: the sample's plan (AugPlan.event_map) behind events_offset, the
        pure offset map for a None plan - where the events lie in the augmented frame.  Training datasets only."""
        from .augmentor import AUGMENT_MAX, augment_many, event_map_after_offset
        self._batch_augmentor()
        idxs = list(idxs)
        if plans is None:
            plans = self.draw_plans(idxs)
        if reads is None:
            reads = [self.read_sample(i) for i in idxs]
        n, dev = len(idxs), self.device
        ch, cw = plans[0].crop
        old = torch.empty(n, self.num_bins, ch, cw, device=dev)
        new = torch.empty_like(old)
        flow = torch.empty(n, 2, ch, cw, device=dev)
        valid = torch.empty(n, ch, cw, device=dev)
        raw_old, raw_new = [], []
        for i0 in range(0, n, AUGMENT_MAX):
            k = min(AUGMENT_MAX, n - i0)
            vols = self.voxel.many([s for _, seqs in reads[i0:i0 + k] for s in seqs])
            flows = [out['flow'].to(dev) for out, _ in reads[i0:i0 + k]]
            augment_many(plans[i0:i0 + k], vols[0::2], vols[1::2], flows,
                         out=(old[i0:i0 + k], new[i0:i0 + k], flow[i0:i0 + k], valid[i0:i0 + k]))
            raw_old += vols[0::2]
            raw_new += vols[1::2]
        batch = {'idx': [out['idx'] for out, _ in reads], 'flow': flow, 'valid': valid}
        if self.with_events:
            batch['events'] = [seqs[0].features for _, seqs in reads]
            batch['events_offset'] = [self._crop_offset() for _ in reads]
            batch['events_map'] = [event_map_after_offset(p, self._crop_offset(), self.image_height, self.image_width) for p in plans]
        dense = self.dense_augmentor is not None
        batch['event_volume_new'], batch['event_volume_old'] = new, old
        batch['d_event_volume_new'] = new if dense else torch.stack(raw_new)
        batch['d_event_volume_old'] = old if dense else torch.stack(raw_old)
        return batch

    def __getitem__(self, idx):
        sample = self.get_sample(idx % len(self))
        if self.type == 'train':
            if self.dense_augmentor is not None:                                                # MVSEC.py:170-187
                e1 = sample['event_volume_old'].permute(1, 2, 0).cpu().numpy()
                e2 = sample['event_volume_new'].permute(1, 2, 0).cpu().numpy()
                fl = sample['flow'].permute(1, 2, 0).numpy()
                e1, e2, d1, d2, fl = self.dense_augmentor(e1, e2, e1, e2, fl)
                for key, arr in (('event_volume_old', e1), ('event_volume_new', e2), ('d_event_volume_old', d1),
                                 ('d_event_volume_new', d2)):
                    sample[key] = torch.from_numpy(arr).permute(2, 0, 1).float()
                sample['flow'] = torch.from_numpy(fl).permute(2, 0, 1)
            elif self.augmentor is not None:
                e1 = sample['event_volume_old'].permute(1, 2, 0).cpu().numpy()
                e2 = sample['event_volume_new'].permute(1, 2, 0).cpu().numpy()
                fl = sample['flow'].permute(1, 2, 0).numpy()
                e1, e2, fl = self.augmentor(e1, e2, fl)
                sample['event_volume_old'] = torch.from_numpy(np.ascontiguousarray(e1)).permute(2, 0, 1).float()
                sample['event_volume_new'] = torch.from_numpy(np.ascontiguousarray(e2)).permute(2, 0, 1).float()
                sample['flow'] = torch.from_numpy(np.ascontiguousarray(fl)).permute(2, 0, 1)
            fl = sample['flow'].float()
            sample['flow'] = fl
            sample['valid'] = (~torch.isinf(fl[0]) & ~torch.isinf(fl[1]) & (torch.linalg.norm(fl, dim=0) > 0)).float()  # :185
        else:
            crop = (256, 256)                                                                   # MVSEC.py:52,193-197
            sample['flow'] = center_crop(sample['flow'], crop)
            sample['valid'] = (sample['flow'][0].abs() < 1000) & (sample['flow'][1].abs() < 1000)
            sample['event_volume_old'] = center_crop(sample['event_volume_old'], crop)
            sample['event_volume_new'] = center_crop(sample['event_volume_new'], crop)
            sample['event_valid'] = center_crop(sample['event_valid'], crop)
        return sample


class MvsecEventFlow_dt4(MvsecEventFlow):
    """dt4: four consecutive event frames per volume, flowgt_dt4/i.npy (MVSEC.py:201-283)."""
    frames_per_volume = 4
    flow_dir = 'flowgt_dt4'
