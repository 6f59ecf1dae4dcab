"""eemflow_amd - MI355X (gfx950) implementation of EEMFlow's dense-flow hot path.

Host code is Python on PyTorch-ROCm and mirrors the reference's interfaces; every kernel lives in
libeemflow_hip.so (hand-written HIP, C ABI in include/eemflow_hip.h)."""
import os as _os

# Frames are kept in flight on separate HIP streams (one context per stream).  The runtime gives a process GPU_MAX_HW_QUEUES hardware
# queues (default 4, the null stream included) and streams that share one serialise, so a fourth stream loses throughput instead of adding
# it; the variable is read at the runtime's first call.  A value the user exported wins.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")

from .augmentor import AugPlan, apply_host, augment_many   # noqa: F401
from .dsec import VoxelGrid, flow_16bit_to_float, flow_float_to_16bit, voxel_grid_many, voxelize_windows   # noqa: F401
from .eemflow import EEMFlow            # noqa: F401
from .events import pack_events_many, read_event_columns   # noqa: F401
from .recording import EventRecording, voxelize_windows as voxelize_recording_windows   # noqa: F401
from .mvsec_raw import MvsecGroundTruth, MvsecRaw   # noqa: F401
from .iwe import contrast_many, fwl, fwl_loss, fwl_many, iwe, iwe_many, warp_events   # noqa: F401
from .tsimg import avg_timestamps, avg_timestamps_many, rsat, rsat_many, timestamp_loss, timestamp_loss_many   # noqa: F401
from .metrics import fb_check          # noqa: F401
from .padder import InputPadder         # noqa: F401
from .smooth import smoothness_loss, smoothness_many   # noqa: F401
from .photo import photo_loss, photo_many   # noqa: F401
from .ssim import ssim_loss, ssim_many   # noqa: F401
from .viz import ImageWriter, event_image, event_image_many, flow_to_image, flow_to_image_many   # noqa: F401
from .voxelizer import EventSequence, EventSequenceToVoxelGrid_Pytorch   # noqa: F401
