"""Command-line entry points with the flags of the reference's train_EEMFlow_HREM.py:139-156 / test_EEMFlow_HREM.py:124-140.

    python -m eemflow_amd.cli train [flags]      # train_EEMFlow_HREM.py: HREM meshflow training, checkpoint per epoch
    python -m eemflow_amd.cli test  [flags]      # test_EEMFlow_HREM.py: evaluation over every sequence of the HREM test split
    python -m eemflow_amd.cli run   [flags]      # not in the reference: the flows along ONE recording (an events npz cut into windows)
    python -m eemflow_amd.cli mvsec [flags]      # not in the reference: one raw MVSEC sequence scored against ground truth propagated on the GPU

Same flags and defaults as the reference scripts (`--lr --wd --train_iters --val_iters --batch_size --input_type --model_name
--start-epoch --num_workers --test_only --test_sequence ...`), the `lr{lr}_we{wd}` run folder, `config.json` / `train.log` /
`lasted_ckpt.pth.tar` in it, checkpoint loading with 'module.' stripping.  Added: `--data_root` (the reference hard-wires its own
repository path), `--save_root`, `--checkpoint`, `--config` (a JSON like the reference's config/a_meshflow.json; its training and
loader defaults are built in), `test`: `--vis_events --print_epe --visualize_every` (the keywords of the reference's evaluation loop
that its script leaves at their defaults; `-v` writes the flow images under the run's save folder), `--fwl` (the flow warp loss of
Test.inference_img_warp_loss, test_mvsec.py:753-852, as a field of every evaluation line), `train`: `--device_batches` (beside `--num_workers`: every batch voxelized, flipped and assembled
on the GPU by the threaded loader, the event volumes never copied through host memory; the same batches under the same numpy seed), `train` and `test`: `--device_events` (HREM event sets prepared on the GPU from the npz columns,
eemflow_amd.events; the same samples bit for bit).
Dropped: the key-map, warped-image
and HSV visualisations, xlsx export, git metadata, nn.DataParallel (one process per GPU:
launch with torchrun for data parallelism; see eemflow_amd.parallel).  Only the models built here are accepted: EEMFlow (trained by
the fused step inside the library), `eraft` (train_EEMFlow_HREM.py:30-32) and `EEMFlow+` (both trained through the reference's own
statement sequence on the operator-level autograd route, train_mvsec.py:241-258).
"""
import argparse
import copy
import json
import os

import torch

# the fields of config/a_meshflow.json the scripts read (train_EEMFlow_HREM.py:25-68, train_mvsec.py:178-183)
DEFAULT_CONFIG = {
    "name": "mesh_flow",
    "train_img_size": [512, 960],
    "val_img_size": [720, 1280],
    "data_loader": {
        "train": {"args": {"batch_size": 6, "shuffle": True, "sequence_length": 1, "num_voxel_bins": 5, "eval_type": "dense",
                           "aug_params": {"crop_size": [512, 960], "min_scale": -0.1, "max_scale": 1.0, "do_flip": True}}},
        "test": {"args": {"batch_size": 1, "shuffle": False, "sequence_length": 1, "num_voxel_bins": 5, "align_to": "images",
                          "eval_type": "dense"}},
    },
    "train": {"lr": 1e-4, "wdecay": 5e-5, "epsilon": 1e-8, "num_steps": 1000000, "mixed_precision": True, "gamma": 0.8, "clip": 1.0},
}


# what the last train() of this process ended with (model, fused trainer, run folder, rank, world) - for callers that embed the CLI
# (tests compare the replicas of a data-parallel run through it); the scripts themselves only use the run folder
LAST_RUN = {}


def build_parser():
    p = argparse.ArgumentParser(prog="eemflow_amd.cli", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="command", required=True)

    def common(q, train):
        q.add_argument('-v', '--visualize', action='store_true',
                       help='evaluation: write the colour-wheel images of every estimated and ground-truth flow as JPEG files under '
                            '<save folder>/<sequence>/test/ (train: accepted, the training loop writes no images)')
        q.add_argument('-n', '--num_workers', default=0, type=int, help='host threads that read and voxelize samples ahead (the reference: DataLoader worker processes); 0 = in the loop')
        if train:
            q.add_argument('--device_batches', action='store_true',
                           help='build every training batch on the GPU: voxelized, flipped and assembled without a copy of the event volumes '
                                'through host memory (implies the threaded loader with at least one thread; same batches as the host route '
                                'under the same numpy seed, and reproducible for any --num_workers)')
            q.add_argument('--contrast_weight', default=0.0, type=float, metavar='W',
                           help='add W times the contrast term - minus the mean flow warp loss of the batch under the last prediction, no '
                                'ground truth needed - to the loss (not in the reference; the samples then carry their events, every model '
                                'trains through the autograd engine and EEMFlow predicts at the full frame; needs --device_batches or an '
                                'un-augmented dataset)')
            q.add_argument('--timestamp_weight', default=0.0, type=float, metavar='W',
                           help='add W times the average-timestamp term - the sum of squares of the image of average timestamps of the '
                                'batch\'s events warped by the last prediction, forward plus backward, no ground truth needed - to the '
                                'loss (not in the reference; under every rule of --contrast_weight: the samples carry their events, every '
                                'model trains through the autograd engine and EEMFlow predicts at the full frame; needs --device_batches '
                                'or an un-augmented dataset)')
            q.add_argument('--self_supervised', action='store_true',
                           help='with --contrast_weight (or --timestamp_weight, --photo_weight, --ssim_weight): train on that term alone, '
                                'the ground-truth flow is not read')
            q.add_argument('--smooth_weight', default=0.0, type=float, metavar='W',
                           help='add W times the edge-aware smoothness of the last prediction, weighted by the edges of the old event '
                                'volume, to the loss (Loss_tools.edge_aware_smoothness_order1/2 of the reference; every model then '
                                'trains through the autograd engine; a mesh-size prediction is regularised unweighted)')
            q.add_argument('--smooth_order', default=1, type=int, choices=(1, 2), help='with --smooth_weight: first or second differences')
            q.add_argument('--smooth_constant', default=1.0, type=float, metavar='A', help='with --smooth_weight: the factor on the image differences')
            q.add_argument('--smooth_weight_type', default='gauss', choices=('gauss', 'exp'), help='with --smooth_weight: exp(-mean g^2) or exp(-mean |g|)')
            q.add_argument('--smooth_error', default='L1', choices=('L1', 'abs_robust'), help='with --smooth_weight: |d| or (|d| + 0.01)^0.4')
            q.add_argument('--smooth_all', action='store_true', help='with --smooth_weight: all predictions under the sequence loss\'s gamma, not the last alone')
            q.add_argument('--photo_weight', default=0.0, type=float, metavar='W',
                           help='add W times the photometric / census loss between the old event volume and the new one warped back by the '
                                'last prediction to the loss (Loss_tools.photo_loss_multi_type / census_loss_torch of the reference, no '
                                'ground truth needed; every model then trains through the autograd engine and EEMFlow predicts at the full '
                                'frame)')
            q.add_argument('--photo_kind', default='census', choices=('abs_robust', 'charbonnier', 'L1', 'census'), help='with --photo_weight: the loss between the volumes')
            q.add_argument('--photo_occ', action='store_true',
                           help='with --photo_weight: a second forward pass with the volumes exchanged (no gradient) and the forward-backward '
                                'check give the occlusion mask of the loss')
            q.add_argument('--photo_all', action='store_true', help='with --photo_weight: all predictions under the sequence loss\'s gamma, not the last alone')
            q.add_argument('--photo_q', default=0.4, type=float, metavar='Q', help='with --photo_kind census: the exponent')
            q.add_argument('--photo_charbonnier', action='store_true', help='with --photo_kind census: (dist^2 + eps)^q in place of (|dist| + 0.01)^q')
            q.add_argument('--photo_max_distance', default=3, type=int, choices=(1, 2, 3), metavar='R', help='with --photo_kind census: patches of (2R+1)^2 cells')
            q.add_argument('--ssim_weight', default=0.0, type=float, metavar='W',
                           help='add W times the weighted SSIM loss between the old event volume and the new one warped back by the last '
                                'prediction to the loss (Loss_tools.weighted_ssim under photo_loss_multi_type of the reference, no ground '
                                'truth needed; every model then trains through the autograd engine and EEMFlow predicts at the full frame)')
            q.add_argument('--ssim_occ', action='store_true',
                           help='with --ssim_weight: the forward-backward occlusion mask of --photo_occ weights the loss (one exchanged pass '
                                'per step serves both)')
            q.add_argument('--ssim_all', action='store_true', help='with --ssim_weight: all predictions under the sequence loss\'s gamma, not the last alone')
            q.add_argument('--ssim_c1', default=float('inf'), type=float, metavar='C1', help='with --ssim_weight: regularises the luminance term (inf: off, the reference\'s default)')
            q.add_argument('--ssim_c2', default=9e-6, type=float, metavar='C2', help='with --ssim_weight: regularises the structure term (inf: off)')
        q.add_argument('--device_events', action='store_true',
                       help='prepare the event sets on the GPU from the npz columns (HREM datasets: the columns are uploaded in their file '
                            'dtypes and one launch per sample writes the float64 event tables; the same samples bit for bit, a set whose '
                            'timestamps are not in order keeps the host route)')
        q.add_argument('--train_iters', default=6000000 if train else 1000000, type=int, metavar='N', help='number of total iterations')
        q.add_argument('-se', '--start-epoch', action='store_true', help='restart from lasted_ckpt.pth.tar of the run folder')
        q.add_argument('-be', '--best_epe', default=1e5, type=float)
        q.add_argument('--val_iters', default=10000 if train else 3000, type=int, metavar='N', help='iterations per epoch (checkpoint interval)')
        q.add_argument('--lr', default=1e-5 if train else 1e-4, type=float, help='learning rate')
        q.add_argument('--wd', default=0 if train else 1e-5, type=float, help='weight decay')
        q.add_argument('--batch_size', '-bs', default=6 if train else 2, type=int, help='batch size in training')
        q.add_argument('--test_only', action='store_true')
        q.add_argument('--test_sequence', '-sq', default='indoor_flying2' if train else '', type=str)
        q.add_argument('--dense', action='store_true')
        q.add_argument('--density', '-d', default='ct0.05', type=str)
        q.add_argument('--model_name', '-model', default='EEMFlow', type=str)
        q.add_argument('--input_type', '-int', default='dt1', type=str)
        q.add_argument('--is_using_dynamic', '-dynamic', action='store_true')
        q.add_argument('--data_root', default=os.environ.get("EEMFLOW_DATA_ROOT", os.getcwd()), help='folder that holds dataset/HREM/...')
        q.add_argument('--save_root', default=os.getcwd(), help='where exp_HREM_meshflow/ (train) or HREM_testset/ (test) is created')
        q.add_argument('--checkpoint', default=None, help='test: checkpoint file (default <save_root>/checkpoints/EEMFlow_HREM_<input_type>.pth.tar)')
        q.add_argument('--config', default=None, help='JSON with the layout of config/a_meshflow.json (default: built-in copy of its used fields)')
        q.add_argument('--device', default='cuda:0')
        q.add_argument('--loader_threads', default=0, type=int, help='evaluation: host threads that read and voxelize samples ahead')
        q.add_argument('--frames_in_flight', default=1, type=int,
                       help='evaluation: samples kept in flight on as many model replicas / HIP streams (not in the reference; 4 suits one MI355X)')
        q.add_argument('--coalesce', default=1, type=int,
                       help='evaluation, EEMFlow: samples voxelized by one launch sequence and handed to one forward_many call (not in the '
                            'reference; 10 with --frames_in_flight 2 suits one MI355X); the volumes then stay raw and pconv1_1 normalises them')
        if not train:
            q.add_argument('--fwl', action='store_true',
                           help='evaluation: add the flow warp loss of every sample - the variance of the image of its events warped by the '
                                'estimated flow over the variance of the event-count image, no ground truth needed - to every line')
            q.add_argument('--rsat', action='store_true',
                           help='evaluation: add RSAT of every sample - the average-timestamp loss of its events warped by the estimated '
                                'flow over that loss under zero flow, below 1 where the flow sharpens the events, no ground truth needed - '
                                'to every line')
            q.add_argument('--vis_events', action='store_true', help='with -v: also the red / blue images of both event volumes, their density in the file name')
            q.add_argument('--print_epe', action='store_true', help="with -v: the sample's AEE in the name of the estimated flow's file")
            q.add_argument('--visualize_every', default=1, type=int, metavar='N', help='with -v: every N-th sample only (the reference: every sample)')
            q.add_argument('--stream', default=0, type=int,
                           help='evaluation: walk each sequence window by window, up to N windows per forward_stream call (not in the reference; '
                                'needs a dataset of consecutive windows - HREM samples are separate files and are refused)')
            q.add_argument('--fb_check', nargs=2, type=float, default=None, metavar=('A1', 'A2'),
                           help='evaluation, EEMFlow with --stream: run the stream bidirectionally and add the forward-backward consistency '
                                'share and the AEE over the consistent pixels to every line (threshold A1 * (|fw| + |bw|) + A2)')
    common(sub.add_parser('train', help='train_EEMFlow_HREM.py'), True)
    common(sub.add_parser('test', help='test_EEMFlow_HREM.py'), False)
    r = sub.add_parser('run', help='flows along one recording (not in the reference): the events npz is uploaded once, cut into consecutive '
                                   'windows and voxelized on the GPU straight from its columns, window pairs go through forward_stream')
    r.add_argument('--events', required=True, help='the recording: an HREM-style npz with the arrays t, x, y, p')
    r.add_argument('--height', required=True, type=int, help='sensor rows')
    r.add_argument('--width', required=True, type=int, help='sensor columns')
    r.add_argument('--model_name', '-model', default='EEMFlow', type=str)
    r.add_argument('--checkpoint', required=True, help='checkpoint file of the model')
    r.add_argument('--config', default=None, help='JSON with the layout of config/a_meshflow.json (default: built-in copy of its used fields)')
    r.add_argument('--device', default='cuda:0')
    r.add_argument('--window_ms', default=None, type=float, metavar='MS', help='cut by duration: windows of MS milliseconds from the first event')
    r.add_argument('--window_events', default=None, type=int, metavar='N', help='cut by count: windows of N events')
    r.add_argument('--stride_ms', default=None, type=float, metavar='MS', help='with --window_ms: a window starts every MS milliseconds (MS divides the window); '
                                                                               'pair m runs from window m to window m + window/stride, the one that starts where it ends')
    r.add_argument('--stride_events', default=None, type=int, metavar='N', help='with --window_events: a window starts every N events (N divides the window)')
    r.add_argument('--t_unit', default='ns', choices=('ns', 'us', 's'), help='unit of the t array (HREM: ns)')
    r.add_argument('--stream', default=0, type=int, metavar='N', help='windows per forward_stream call (default: as many as the model takes)')
    r.add_argument('--out', default=None, metavar='DIR', help='write the flow of pair k (window k -> window k + 1; with a stride, window k -> window k + window/stride) as DIR/%%06d.flo')
    r.add_argument('-v', '--visualize', action='store_true', help='with --out: also the colour-wheel image of every flow, DIR/%%06d_flow.jpg')
    r.add_argument('--fwl', action='store_true', help='the flow warp loss of every pair (the events of its first window under its flow) on its line, the mean in the summary')
    r.add_argument('--rsat', action='store_true', help='RSAT of every pair on its line, the mean in the summary')
    r.add_argument('--fb_check', nargs=2, type=float, default=None, metavar=('A1', 'A2'),
                   help='EEMFlow: run the stream bidirectionally and add the forward-backward consistent share of every pair to its line '
                        '(threshold A1 * (|fw| + |bw|) + A2); with --out the backward flows go to DIR/%%06d_bw.flo')
    m = sub.add_parser('mvsec', help='score one raw MVSEC sequence (not in the reference, which needs the files of loader/MVSEC_encoder.py): events, '
                                     'grey-frame timestamps and the ground-truth stack go to the GPU once; windows of --dt grey frames are voxelized, '
                                     'run through forward_stream and scored against ground truth propagated on the GPU')
    m.add_argument('--data', required=True, help='npz with the arrays events (N,4: x, y, t seconds, p), image_raw_ts, image_raw_event_inds')
    m.add_argument('--gt', required=True, help='npz with the arrays flow_dist (T,2,H,W) and flow_dist_ts (T,)')
    m.add_argument('--checkpoint', required=True, help='checkpoint file of the model')
    m.add_argument('--model_name', '-model', default='EEMFlow', type=str)
    m.add_argument('--config', default=None, help='JSON with the layout of config/a_meshflow.json (default: built-in copy of its used fields)')
    m.add_argument('--device', default='cuda:0')
    m.add_argument('--first', default=None, type=int, metavar='I', help='first pair: grey frame I (default: the first frame the ground truth covers)')
    m.add_argument('--last', default=None, type=int, metavar='J', help='last pair starts at grey frame <= J (default: the last one the ground truth and the frames cover)')
    m.add_argument('--dt', default=1, type=int, metavar='N', help='grey frames per window (consecutive windows unless --stride / --reference_pairs say otherwise; 1 = MvsecEventFlow\'s samples)')
    m.add_argument('--stride', default=None, type=int, metavar='S', help='a window starts every S grey frames (S divides --dt; default --dt: consecutive windows); '
                                                                         'pair m runs from window m to the window that starts where it ends')
    m.add_argument('--reference_pairs', action='store_true', help='the samples of MvsecEventFlow_dt4 (--dt 4) / MvsecEventFlow (--dt 1): windows one grey frame '
                                                                  'apart, ground truth over --dt frames')
    m.add_argument('--eval_type', default='dense', choices=('dense', 'sparse'), help='sparse: only pixels of the first window that hold an event')
    m.add_argument('--is_car', action='store_true', help='outdoor sequences: rows from 190 on are not scored')
    m.add_argument('--crop', nargs=2, type=int, default=None, metavar=('H', 'W'), help='centre crop of volumes, ground truth and mask (the dataset\'s validation branch: 256 256)')
    m.add_argument('--height', default=260, type=int, help='sensor rows')
    m.add_argument('--width', default=346, type=int, help='sensor columns')
    m.add_argument('--stream', default=0, type=int, metavar='N', help='windows per forward_stream call (default: as many as the model takes)')
    m.add_argument('--out', default=None, metavar='DIR', help='write the flow of pair k as DIR/%%06d.flo and its ground truth as DIR/%%06d_gt.flo')
    return p


def load_config(path):
    return json.load(open(path)) if path else copy.deepcopy(DEFAULT_CONFIG)


def build_model(name, config, training, mesh=True):
    if name == "EEMFlow":
        from .eemflow import EEMFlow
        # HREM's training target is the 16x16 mesh flow (HREM.py:254-255); the reference script builds the model without
        # out_mesh_size and its loss then meets a full-resolution prediction.  Training here predicts at mesh size
        # (EEMFlow.py:126-132), evaluation at full resolution against the upsampled mesh flow (HREM.py:264-267).
        return EEMFlow(config=config, n_first_channels=5, out_mesh_size=training and mesh)   # (mesh=False: the contrast term needs the full frame)
    if name == "eraft":                                             # train_EEMFlow_HREM.py:30-32 / test_EEMFlow_HREM.py
        from .eraft import ERAFT
        split = 'train' if training else 'test'
        return ERAFT(config=config, n_first_channels=config['data_loader'][split]['args']['num_voxel_bins'])
    if name in ("EEMFlow+", "EEMFlow_cdc"):
        from .eemflow_plus import EEMFlow_cdc
        return EEMFlow_cdc(config=config, n_first_channels=5)
    raise SystemExit(f"model '{name}' is not built here (EEMFlow, eraft, EEMFlow+)")


def per_rank_batch(batch_size, world):
    """`--batch_size` is the GLOBAL batch, as in the reference, whose nn.DataParallel scatters it over the GPUs
    (train_EEMFlow_HREM.py:116-118): each of the `world` processes takes batch_size / world samples per step, so that the same flags
    (lr, train_iters, val_iters) train the same way on 1 and on 8 GPUs.  Equal shards are required: the gradient exchange is a
    mean of per-rank means."""
    if batch_size % world:
        raise SystemExit(f"--batch_size {batch_size} is not divisible by the {world} processes of this job")
    return batch_size // world


def device_events_kw(args, dataset_class):
    """The dataset keyword of --device_events; only datasets that read HREM's npz columns take it (hrem.HREMEventFlow)."""
    if not getattr(args, "device_events", False):
        return {}
    if not getattr(dataset_class, "supports_device_events", False):
        raise SystemExit(f"--device_events prepares HREM event files (events1.npz / events2.npz columns) on the GPU: "
                         f"{dataset_class.__name__} has no such route")
    return {"device_events": True}


def smooth_kw(args):
    """TrainRaftEvents' smoothness arguments of the --smooth_* flags."""
    return dict(smooth_weight=float(getattr(args, "smooth_weight", 0.0)), smooth_order=int(getattr(args, "smooth_order", 1)),
                smooth_constant=float(getattr(args, "smooth_constant", 1.0)), smooth_weight_type=getattr(args, "smooth_weight_type", "gauss"),
                smooth_error=getattr(args, "smooth_error", "L1"), smooth_all=bool(getattr(args, "smooth_all", False)))


def photo_kw(args):
    """TrainRaftEvents' photometric arguments of the --photo_* flags."""
    return dict(photo_weight=float(getattr(args, "photo_weight", 0.0)), photo_kind=getattr(args, "photo_kind", "census"),
                photo_occ=bool(getattr(args, "photo_occ", False)), photo_all=bool(getattr(args, "photo_all", False)),
                photo_q=float(getattr(args, "photo_q", 0.4)), photo_charbonnier=bool(getattr(args, "photo_charbonnier", False)),
                photo_max_distance=int(getattr(args, "photo_max_distance", 3)))


def ssim_kw(args):
    """TrainRaftEvents' SSIM arguments of the --ssim_* flags."""
    return dict(ssim_weight=float(getattr(args, "ssim_weight", 0.0)), ssim_occ=bool(getattr(args, "ssim_occ", False)),
                ssim_all=bool(getattr(args, "ssim_all", False)), ssim_c1=float(getattr(args, "ssim_c1", float("inf"))),
                ssim_c2=float(getattr(args, "ssim_c2", 9e-6)))


def train(args):
    from . import harness, parallel
    from .hrem import HREMEventFlow
    photo = float(getattr(args, "photo_weight", 0.0))
    ssim = float(getattr(args, "ssim_weight", 0.0))
    tsw = float(getattr(args, "timestamp_weight", 0.0))
    if (getattr(args, "self_supervised", False) and float(getattr(args, "contrast_weight", 0.0)) == 0.0 and photo == 0.0 and ssim == 0.0
            and tsw == 0.0):
        raise SystemExit("--self_supervised needs a --contrast_weight, a --photo_weight or an --ssim_weight (or a --timestamp_weight): "
                         "there is no other loss")
    # one process per GPU under torchrun: every rank trains on its shard of the samples, the trainer all-reduces the flat gradient
    # (RCCL), rank 0 writes the logs and checkpoints
    rank, local_rank, world = parallel.init_distributed()
    if world > 1:
        args.device = "cuda:{}".format(parallel.local_device_index(local_rank))
        # this rank's host threads (the loader's workers inherit the mask) on the CPUs next to its GPU
        parallel.pin_host_threads_to_gpu_numa(parallel.local_device_index(local_rank))
    config = load_config(args.config)
    contrast = float(getattr(args, "contrast_weight", 0.0))
    on_events = contrast != 0.0 or tsw != 0.0                                        # a term that reads the samples' events
    model = build_model(args.model_name, config, training=True, mesh=contrast == 0.0 and photo == 0.0 and ssim == 0.0 and tsw == 0.0)    # (these terms need the full frame)
    config["train"]["lr"] = args.lr                                                  # train_EEMFlow_HREM.py:56-59
    config["train"]["wdecay"] = args.wd
    config["train"]["num_steps"] = args.train_iters
    config['data_loader']['train']['args']['batch_size'] = args.batch_size
    config['name'] = "lr{:5f}_we{:5f}".format(args.lr, args.wd)
    save_path = os.path.join(args.save_root, "exp_HREM_meshflow/{}_{}".format(args.model_name, args.input_type), config['name'].lower())
    config["data_loader"]["train"]["args"].update({'type': 'train', 'event_interval': args.input_type})
    if rank == 0:                                                                    # one writer: rank 0 owns the run folder and the log
        os.makedirs(save_path, exist_ok=True)
        print('Storing output in folder {}'.format(save_path))
        json.dump(config, open(os.path.join(save_path, 'config.json'), 'w'), indent=4, sort_keys=False)
    start_epoch, start_iteration = 0, 0
    if args.start_epoch:
        start_epoch, start_iteration = harness.load_checkpoint(os.path.join(save_path, 'lasted_ckpt.pth.tar'), model, with_iteration=True)
    logger = harness.Logger(os.path.join(save_path, 'train.log') if rank == 0 else None, verbose=rank == 0)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    train_set = HREMEventFlow(args=config["data_loader"]["train"]["args"], train=True, root=args.data_root, device=dev,
                              with_events=on_events, **device_events_kw(args, HREMEventFlow))
    if on_events and train_set.augmentor is not None and not args.device_batches:
        # the host route flips the volumes without telling where the events went; get_batch hands out batch['events_map']
        raise SystemExit(("--contrast_weight" if contrast != 0.0 else "--timestamp_weight") + " with an augmented dataset needs --device_batches: only batches assembled on the device carry "
                         "the event map of their augmentation")
    sampler = torch.utils.data.distributed.DistributedSampler(train_set, num_replicas=world, rank=rank, shuffle=True) if world > 1 else None
    if on_events:
        args.device_batches = True                                   # (un-augmented: get_batch all the same - it stacks nothing ragged)
    if args.num_workers > 0 or args.device_batches:   # the reference's worker count: here host threads that read / inflate / voxelize samples ahead
        from .loader import ThreadedBatchLoader
        loader = ThreadedBatchLoader(train_set, per_rank_batch(args.batch_size, world), shuffle=sampler is None, sampler=sampler,
                                     threads=max(1, args.num_workers), drop_last=True, device_batches=args.device_batches)
    else:
        loader = torch.utils.data.DataLoader(train_set, batch_size=per_rank_batch(args.batch_size, world), shuffle=sampler is None,
                                             sampler=sampler, num_workers=0, drop_last=True)
    model = model.to(dev)
    if parallel.exchange_active():                                   # replicas start from rank 0's weights
        for prm in model.parameters():
            torch.distributed.broadcast(prm.data, src=0)
        if hasattr(model, "invalidate_weights"):
            model.invalidate_weights()                               # .data writes bypass the version counter the model watches
        else:
            from . import ops
            ops.invalidate_packed_weights()                          # the operator-level models cache packed weights by version too
    tcfg = config["train"]
    # The reference trainer sizes the padder with config['train_img_size'] (train_mvsec.py:67), the size its augmentor crops to.  The
    # HREM training samples here are the un-cropped frames, so the padder is sized from the first batch itself (image_size=None).
    # EEMFlow: the fused step inside the library; E-RAFT / EEMFlow+: the reference's statement sequence over the operator-level
    # autograd route (their data-parallel exchange is the flat-gradient all-reduce in TrainRaftEvents._train_iters_autograd)
    smooth = float(getattr(args, "smooth_weight", 0.0))
    engine = "fused" if args.model_name == "EEMFlow" and contrast == 0.0 and tsw == 0.0 and photo == 0.0 and ssim == 0.0 and smooth == 0.0 else "autograd"     # (the fused trainer has none of the terms)
    tr = harness.TrainRaftEvents(loader, None, lr=tcfg["lr"], wdecay=tcfg["wdecay"], epsilon=tcfg["epsilon"],
                                 num_steps=tcfg["num_steps"], clip=tcfg["clip"], gamma=tcfg["gamma"], logger=logger,
                                 start_iteration=start_iteration, engine=engine, mixed_precision=tcfg.get("mixed_precision", True),
                                 contrast_weight=contrast, timestamp_weight=tsw, supervised=not getattr(args, "self_supervised", False), **smooth_kw(args), **photo_kw(args), **ssim_kw(args))
    for epoch in range(start_epoch, max(args.train_iters // args.val_iters, 1)):
        if sampler is not None:
            sampler.set_epoch(epoch)
        model = tr.train_iters(model, start_epoch=epoch, val_iters=args.val_iters)
        if rank == 0:
            harness.save_checkpoint(os.path.join(save_path, 'lasted_ckpt.pth.tar'), model, epoch, trainer=tr.trainer, iteration=tr.iteration)
    parallel.barrier(dev)
    LAST_RUN.update(model=model, trainer=tr.trainer, save_path=save_path, rank=rank, world=world, engine=engine,
                    iteration=tr.trainer.iteration if tr.trainer is not None else tr.iteration)
    return save_path


def test(args):
    from . import harness
    if args.fb_check is not None and not args.stream:
        raise SystemExit("--fb_check needs --stream N (the backward flow comes from the bidirectional stream)")
    if (args.vis_events or args.print_epe or args.visualize_every != 1) and not args.visualize:
        raise SystemExit("--vis_events / --print_epe / --visualize_every qualify -v (--visualize)")
    if args.visualize_every < 1:
        raise SystemExit("--visualize_every N: N >= 1")
    from .hrem import HREMEventFlow
    config = load_config(args.config)
    model = build_model(args.model_name, config, training=False)
    ckpt = args.checkpoint or os.path.join(args.save_root, 'checkpoints', 'EEMFlow_HREM_{}.pth.tar'.format(args.input_type))
    start_epoch = harness.load_checkpoint(ckpt, model)
    save_path = os.path.join(args.save_root, "HREM_testset/{}_{}".format(args.model_name, args.input_type))
    os.makedirs(save_path, exist_ok=True)
    config["data_loader"]["test"]["args"].update({"event_interval": args.input_type})
    print('Storing output in folder {}'.format(save_path))
    json.dump(config, open(os.path.join(save_path, 'config.json'), 'w'), indent=4, sort_keys=False)
    logger = harness.Logger(os.path.join(save_path, 'test.log'))
    dev = torch.device(args.device)
    coalesce = args.coalesce if args.model_name == 'EEMFlow' else 1      # (forward_many is EEMFlow's)
    test_set = HREMEventFlow(args=config["data_loader"]["test"]["args"], train=False, root=args.data_root, device=dev,
                             deferred_norm=coalesce > 1, with_events=args.fwl or args.rsat, **device_events_kw(args, HREMEventFlow))
    model = model.to(dev)
    sequences = [args.test_sequence] if args.test_sequence else list(test_set.nori_list.keys())
    ev = harness.TestRaftEvents(test_set, tuple(config["val_img_size"]), logger=logger)
    extra = {}
    if args.stream:
        extra["stream"] = args.stream
    if args.fb_check is not None:
        extra["fb_check"] = tuple(args.fb_check)
    if args.fwl:
        extra["fwl"] = True
    if args.rsat:
        extra["rsat"] = True
    if args.visualize:
        extra.update(visualize_map=True, vis_events=args.vis_events, print_epe=args.print_epe, visualize_every=args.visualize_every,
                     save_path=save_path)
    return ev.test_multi_sequence(model, start_epoch + 1, sequence_list=sequences, stride=1, frames_in_flight=args.frames_in_flight,
                                  loader_threads=args.loader_threads, coalesce=coalesce, **extra)


T_UNITS = {'ns': (1e-9, 1_000_000), 'us': (1e-6, 1_000), 's': (1.0, 1e-3)}     # unit -> (scale_a to seconds, t units per millisecond)


def run(args):
    """`cli run`: returns {'windows', 'events', 'pairs', 'frames_per_s', 'meanFWL', 'meanRSAT'} (the means None where not asked)."""
    import time
    if (args.window_ms is None) == (args.window_events is None):
        raise SystemExit("run: give exactly one of --window_ms MS and --window_events N")
    if args.window_ms is not None and not args.window_ms > 0:
        raise SystemExit("--window_ms MS: MS > 0")
    if args.window_events is not None and args.window_events < 1:
        raise SystemExit("--window_events N: N >= 1")
    if (args.stride_ms is not None and args.window_ms is None) or (args.stride_events is not None and args.window_events is None):
        raise SystemExit("run: --stride_ms MS goes with --window_ms, --stride_events N with --window_events")
    lag = 1
    if args.stride_ms is not None:
        lag = int(round(args.window_ms / args.stride_ms)) if args.stride_ms > 0 else 0
        if lag < 1 or abs(lag * args.stride_ms - args.window_ms) > 1e-9 * args.window_ms:
            raise SystemExit(f"--stride_ms {args.stride_ms}: the stride is > 0 and divides --window_ms {args.window_ms}")
    if args.stride_events is not None:
        if args.stride_events < 1 or args.window_events % args.stride_events != 0:
            raise SystemExit(f"--stride_events {args.stride_events}: the stride is >= 1 and divides --window_events {args.window_events}")
        lag = args.window_events // args.stride_events
    if args.height < 1 or args.width < 1:
        raise SystemExit("--height H --width W: the sensor size, both >= 1")
    if args.visualize and not args.out:
        raise SystemExit("-v (--visualize) writes its images beside the flows: it needs --out DIR")
    if args.fb_check is not None and args.model_name != 'EEMFlow':
        raise SystemExit(f"--fb_check needs a model whose forward_stream is bidirectional (EEMFlow); {args.model_name} has none")
    if args.stream < 0 or args.stream == 1:
        raise SystemExit("--stream N: N >= 2 windows per forward_stream call (0: as many as the model takes)")
    if not os.path.isfile(args.events):
        raise SystemExit(f"--events {args.events}: no such file")
    from . import harness
    from .hrem import write_flo
    from .recording import EventRecording
    config = load_config(args.config)
    model = build_model(args.model_name, config, training=False)
    harness.load_checkpoint(args.checkpoint, model)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    model = model.to(dev).eval()
    scale_a, per_ms = T_UNITS[args.t_unit]
    rec = EventRecording.from_npz(args.events, args.height, args.width, device=dev, scale_a=scale_a)
    def units(ms):                                                   # a duration in the units of the raw t column, an integer where it is one
        span = ms * per_ms
        return int(span) if float(span).is_integer() else span

    sliding = args.stride_ms is not None or args.stride_events is not None
    if sliding:                                                      # windows by span, pairs (m, m + lag)
        if args.stride_ms is not None:
            stride = units(args.stride_ms)
            spans = rec.sliding_spans(window=stride * lag, stride=stride)
        else:
            spans = rec.sliding_spans(count=args.window_events, stride_count=args.stride_events)
        offsets = None
        nwin = len(spans)
        counts = [int(b - a) for a, b in spans]
        total = int(spans[-1][1] - spans[0][0]) if nwin else 0
        windows_kw = dict(spans=spans, lag=lag)
    else:
        if args.window_ms is not None:
            offsets = rec.window_offsets(window=units(args.window_ms))
        else:
            offsets = rec.window_offsets(count=args.window_events)
        nwin = len(offsets) - 1
        counts = [int(offsets[k + 1] - offsets[k]) for k in range(nwin)]
        total = int(offsets[-1] - offsets[0])
        windows_kw = dict(offsets=offsets)
    if nwin < lag + 1:
        raise SystemExit(f"run: the recording's {rec.n} events give {nwin} full windows; a flow needs " + ("two" if lag == 1 else f"{lag + 1} at this stride"))
    limit = model.MAX_STREAM_BIDIR if args.fb_check is not None else model.MAX_STREAM
    if args.stream > limit:
        raise SystemExit(f"--stream {args.stream}: {args.model_name} takes at most {limit} windows per call" + (" with --fb_check" if args.fb_check is not None else ""))
    writer = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        if args.visualize:
            from .viz import ImageWriter, flow_to_image_many
            writer = ImageWriter(args.out)
    sums = {'FWL': [0.0, 0], 'RSAT': [0.0, 0]}
    pairs = 0
    torch.cuda.synchronize(dev)
    start = time.perf_counter()
    try:
        for item in harness.run_recording(model, rec, chunk=args.stream or None, fwl=args.fwl, rsat=args.rsat, fb_check=args.fb_check, **windows_kw):
            k = item['k']
            line = 'pair {:6d}  events {:9d}'.format(k, counts[k])
            for key in ('FWL', 'RSAT'):
                if key in item:
                    val = float(item[key])
                    if val == val:                                   # NaN (nothing to compare with) stays out of the mean
                        sums[key][0] += val
                        sums[key][1] += 1
                    line += '  {}: {:2.6f}'.format(key, val)
            if 'mask_fw' in item:
                line += '  consistent: {:.4f}'.format(float(item['mask_fw'].mean()))
            if args.out:
                write_flo(os.path.join(args.out, '%06d.flo' % k), item['flow'][0].permute(1, 2, 0).cpu().numpy())
                if 'flow_bw' in item:
                    write_flo(os.path.join(args.out, '%06d_bw.flo' % k), item['flow_bw'][0].permute(1, 2, 0).cpu().numpy())
                if writer is not None:
                    writer.submit('%06d_flow.jpg' % k, flow_to_image_many([item['flow']], bgr=True)[0])
            print(line)
            pairs += 1
        torch.cuda.synchronize(dev)
    finally:
        if writer is not None:
            writer.close()
    wall = time.perf_counter() - start
    mean = {key: (v[0] / v[1] if v[1] else float('nan')) for key, v in sums.items()}
    line = 'windows {}  events {}  pairs {}  {:.1f} frames/s'.format(nwin, total, pairs, pairs / wall if wall > 0 else float('nan'))
    if args.fwl:
        line += '  meanFWL: {:2.6f}'.format(mean['FWL'])
    if args.rsat:
        line += '  meanRSAT: {:2.6f}'.format(mean['RSAT'])
    print(line)
    return {'windows': nwin, 'events': total, 'pairs': pairs, 'frames_per_s': pairs / wall if wall > 0 else float('nan'),
            'meanFWL': mean['FWL'] if args.fwl else None, 'meanRSAT': mean['RSAT'] if args.rsat else None}


def mvsec_pair_range(image_raw_ts, n_frames, gt_ts, first, last, dt, frames_needed=None, step=None):
    """The pairs --first / --last select, defaults filled in: a pair starting at grey frame i needs the frames i .. i + 2*dt (two windows)
    and ground truth over [ts[i], ts[i + dt]].  frames_needed: the pair needs the frames i .. i + frames_needed instead (dt + 1 for
    --reference_pairs, whose second window starts one frame after the first); step: pairs start every `step` frames from `first`
    (default dt).  Host only."""
    import numpy as np
    from .mvsec_raw import plan_window

    def covered(i):
        try:
            plan_window(gt_ts, image_raw_ts[i], image_raw_ts[i + dt])
            return True
        except ValueError:
            return False
    step = dt if step is None else int(step)
    top = n_frames - 1 - (2 * dt if frames_needed is None else int(frames_needed))     # the last frame a pair can start at
    if top < 0:
        raise SystemExit(f"mvsec: {n_frames} grey frames give no pair of windows at --dt {dt}")
    if first is None:
        first = int(np.searchsorted(image_raw_ts, gt_ts[0], side='left'))
    if last is None:
        last = top
        while last >= first and not covered(last):
            last -= 1
    if first < 0 or last < first or last > top:
        raise SystemExit(f"--first {first} --last {last}: pairs start at grey frames 0..{top} at --dt {dt}, first <= last")
    for i in (first, first + (last - first) // step * step):
        if not covered(i):
            raise SystemExit(f"mvsec: the ground truth ({gt_ts[0]:.6f} .. {gt_ts[-1]:.6f} s) does not cover the pair at grey frame {i} "
                             f"({image_raw_ts[i]:.6f} .. {image_raw_ts[i + dt]:.6f} s)")
    return first, last


def mvsec(args):
    """`cli mvsec`: returns {'pairs', 'events', 'meanAEE', 'mean1px', 'mean3px', 'frames_per_s'}."""
    import time
    if args.dt < 1:
        raise SystemExit("--dt N: N >= 1 grey frames per window")
    if args.reference_pairs and args.stride not in (None, 1):
        raise SystemExit("--reference_pairs: the windows are one grey frame apart; --stride does not apply")
    if args.stride is not None and (args.stride < 1 or args.dt % args.stride != 0):
        raise SystemExit(f"--stride {args.stride}: S >= 1 and S divides --dt {args.dt}")
    if args.height < 1 or args.width < 1:
        raise SystemExit("--height H --width W: the sensor size, both >= 1")
    if args.crop is not None and not (1 <= args.crop[0] <= args.height and 1 <= args.crop[1] <= args.width):
        raise SystemExit(f"--crop {args.crop[0]} {args.crop[1]}: the crop must fit the {args.height} x {args.width} sensor")
    if args.stream < 0 or args.stream == 1:
        raise SystemExit("--stream N: N >= 2 windows per forward_stream call (0: as many as the model takes)")
    if (args.first is not None and args.first < 0) or (args.first is not None and args.last is not None and args.last < args.first):
        raise SystemExit("--first I --last J: 0 <= I <= J")
    for flag, path in (('--data', args.data), ('--gt', args.gt)):
        if not os.path.isfile(path):
            raise SystemExit(f"{flag} {path}: no such file")
    from . import harness
    from .hrem import write_flo
    from .metrics import flow_error_from_sums
    from .mvsec_raw import MvsecRaw
    config = load_config(args.config)
    model = build_model(args.model_name, config, training=False)
    harness.load_checkpoint(args.checkpoint, model)
    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    model = model.to(dev).eval()
    if args.stream > model.MAX_STREAM:
        raise SystemExit(f"--stream {args.stream}: {args.model_name} takes at most {model.MAX_STREAM} windows per call")
    raw = MvsecRaw.from_npz(args.data, args.gt, height=args.height, width=args.width, device=dev)
    if args.reference_pairs or args.stride not in (None, args.dt):   # windows by span: overlapping, pairs at a lag
        step = 1 if args.reference_pairs else args.stride
        first, last = mvsec_pair_range(raw.image_raw_ts, raw.image_raw_ts.shape[0], raw.gt.ts, args.first, args.last, args.dt,
                                       frames_needed=args.dt + 1 if args.reference_pairs else None, step=step)
        spans, t_spans, lag = raw.frame_spans(first, last, args.dt, stride=step, reference_pairs=args.reference_pairs)
        counts = [int(b - a) for a, b in spans]
        total = int(spans[-1][1] - spans[0][0])
        windows_kw = dict(spans=spans, lag=lag, t_spans=t_spans)
    else:
        step = args.dt
        first, last = mvsec_pair_range(raw.image_raw_ts, raw.image_raw_ts.shape[0], raw.gt.ts, args.first, args.last, args.dt)
        offsets, t_edges = raw.frame_windows(first, last, args.dt)
        counts = [int(offsets[k + 1] - offsets[k]) for k in range(len(offsets) - 1)]
        total = int(offsets[-1] - offsets[0])
        windows_kw = dict(offsets=offsets, t_edges=t_edges)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    acc = {'aee': 0.0, 'p1': 0.0, 'p3': 0.0}
    pairs = 0
    torch.cuda.synchronize(dev)
    start = time.perf_counter()
    with torch.no_grad():
        for item in harness.run_recording(model, raw.recording, chunk=args.stream or None, gt=raw.gt, crop=args.crop, eval_type=args.eval_type,
                                          is_car=args.is_car, **windows_kw):
            k = item['k']
            aee, p1, p3 = flow_error_from_sums(item['err_sums'])[:3]
            p1, p3 = 1.0 - p1, 1.0 - p3                              # the outlier shares, as the evaluation loop's "1 - mean %AEE" / "3 - mean %AEE"
            acc['aee'] += aee
            acc['p1'] += p1
            acc['p3'] += p3
            pairs += 1
            print('pair {:6d}  frame {:6d}  events {:9d}  AEE: {:2.6f}  %1px: {:.6f}  %3px: {:.6f}'.format(
                k, first + k * step, counts[k], aee, p1, p3))
            if args.out:
                write_flo(os.path.join(args.out, '%06d.flo' % k), item['flow'][0].permute(1, 2, 0).cpu().numpy())
                write_flo(os.path.join(args.out, '%06d_gt.flo' % k), item['flow_gt'][0].permute(1, 2, 0).cpu().numpy())
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - start
    n = max(pairs, 1)
    print('pairs {}  events {}  Mean AEE: {:.6f}  mean %1px: {:.6f}  mean %3px: {:.6f}  {:.1f} frames/s'.format(
        pairs, total, acc['aee'] / n, acc['p1'] / n, acc['p3'] / n, pairs / wall if wall > 0 else float('nan')))
    return {'pairs': pairs, 'events': total, 'meanAEE': acc['aee'] / n, 'mean1px': acc['p1'] / n, 'mean3px': acc['p3'] / n,
            'frames_per_s': pairs / wall if wall > 0 else float('nan')}


def main(argv=None):
    args = build_parser().parse_args(argv)
    return {'train': train, 'test': test, 'run': run, 'mvsec': mvsec}[args.command](args)


if __name__ == '__main__':
    main()
