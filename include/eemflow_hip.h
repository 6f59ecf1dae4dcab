/*
 * eemflow_hip.h - C ABI of libeemflow_hip.so: the MI355X (gfx950) implementation of EEMFlow's
 * dense-flow hot path.  Plain pointers and sizes only; every device pointer is a HIP device
 * address on the context's device, every `stream` is a hipStream_t passed as void* (NULL = the
 * default stream).  All functions return 0 on success; on failure they return non-zero and
 * eemflow_last_error() describes the problem (thread-local, valid until the next failing call).
 *
 * The reference (boomluo02/EEMFlow) has no FFI of its own on this path: its boundary is the
 * nn.Module interface plus two third-party torch extensions.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference repo root).
 *
 * Tensors are dense NCHW fp32 unless stated.  Ownership: the caller owns every buffer it passes;
 * the context owns its weights and workspaces and never retains caller pointers beyond a call.
 * Threading: one context per host thread/stream; calls on one context must not overlap.
 */
#ifndef EEMFLOW_HIP_H
#define EEMFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Opaque contexts (declared ahead of the visibility block: their C++ members are not part of the ABI). */
typedef struct eemflow_ctx eemflow_ctx;
typedef struct eraft_ctx eraft_ctx;
typedef struct eemplus_ctx eemplus_ctx;

/* The library is built with -fvisibility=hidden: the entry points declared here (and nothing else - no kernel launcher, no C++
 * helper) are its dynamic symbols. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ABI version of this header (bumped on incompatible change). */
int eemflow_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* eemflow_last_error(void);

/* Create / destroy a model context on HIP device `device`.
 * Replaces: EEMFlow.__init__ + model.to(device)  (model/EEMFlow/EEMFlow.py:72-112,
 * test_EEMFlow_HREM.py:53-55,113). */
int eemflow_create(int device, eemflow_ctx** out);
void eemflow_destroy(eemflow_ctx* ctx);

/* Load all parameters from one flat host fp32 vector holding the 66 tensors of the reference
 * state_dict() back to back in registration order (pconv1_1.0.weight, pconv1_1.0.bias, ...,
 * out_conv.bias; 714 352 floats for n_first_channels=5, groups=5).
 * Replaces: model.load_state_dict(checkpoint['state_dict'])  (test_EEMFlow_HREM.py:62-66). */
int eemflow_load_weights(eemflow_ctx* ctx, const float* flat_host, size_t nfloats, int n_first_channels,
                         int groups);

/* New values for the parameters of an already loaded model, from a DEVICE vector in the same order: one
 * device-to-device copy plus the on-device re-pack of every kernel-side layout (no host round trip).  This is what a
 * training loop that owns its optimizer calls after optimizer.step() changed the nn.Parameters in place.
 * Replaces: the implicit "parameters are read where they live" of nn.Module (train_mvsec.py:257 scaler.step). */
int eemflow_update_weights(eemflow_ctx* ctx, const float* flat_device, size_t nfloats, void* stream);

/* Configure the replicate padder for images of `height` x `width` (pad to a multiple of 64, 'chairs'
 * mode: width split left/right, height bottom only).  pad_out = [left, right, top, bottom].
 * Replaces: EEMFlow.change_imagesize -> InputPadder(img_size, 'chairs', 64)
 * (model/EEMFlow/EEMFlow.py:114-116, utils/image_utils.py:129-137). */
int eemflow_set_image_size(eemflow_ctx* ctx, int height, int width, int pad_out[4]);

/* Replay the forward pass through a cached HIP graph (1, default) or launch kernels eagerly (0).  Graphs are keyed on shapes,
 * not on the caller's buffers: the two launches that touch events1 / events2 / flow_out read those pointers from a device
 * table that one tiny launch rewrites when a call brings other buffers, so fresh tensors every frame (the reference's
 * evaluation loop, test_mvsec.py:580-597) replay the same graph.  Up to four shapes stay cached (least recently used out). */
int eemflow_use_graph(eemflow_ctx* ctx, int enable);

/* Throughput hint: the application keeps `n` frames in flight on this GPU (one context and one HIP stream each, e.g. the
 * evaluation loop of test_mvsec.py:580-597 pipelined over several samples).  With n >= 3 the persistent encoder kernels
 * launch fewer, longer blocks - the frames time-slice the CUs and per-block prologues are CU time another frame could use
 * (1280x720, four in flight: +3.5 % frames/s, +8 % latency of a single frame).  Default 1: lowest single-frame latency.
 * Give the process enough hardware queues for its streams (GPU_MAX_HW_QUEUES). */
int eemflow_set_frames_in_flight(eemflow_ctx* ctx, int n);

/* enable != 0: the event volumes handed to eemflow_forward / eemflow_forward_many are RAW voxel grids, each followed in memory by its
 * four-float normalisation record - what eemflow_voxelize / _pair / _many write with normalize = 2.  The first convolution applies
 * (v - mean) / sd to the non-zero voxels as it reads them, so the voxelizer's read-modify-write of every grid (2 x 18.4 MB per volume at
 * 1280x720x5) is never made.  Needs the 5-bin first layer on volumes whose rows are 16-byte multiples and that pad on the bottom only
 * (HREM 1280x720: yes; MVSEC 346x260: no - normalise in the voxelizer there); the call fails otherwise.  In a contiguous batch
 * (eemflow_forward) every sample is [C*H*W + 4] floats long.  Training entry points ignore the flag.
 * Replaces: loader/loader_utils.py:527-535 (the normalisation inside EventSequenceToVoxelGrid_Pytorch.__call__) feeding
 * model/EEMFlow/EEMFlow.py:135 (pconv1_1). */
int eemflow_set_deferred_input_norm(eemflow_ctx* ctx, int enable);

/* Graph-cache statistics: out3 = {captures, replays, io-table rewrites}. */
int eemflow_graph_stats(eemflow_ctx* ctx, long long out3[3]);

/* Inference forward: events1/events2 [batch][C][in_h][in_w] -> flow_out [batch][2][out_h][out_w].
 * The reference upsamples the 1/64 grid straight to the *input* size (out_h,out_w = in_h,in_w) or,
 * in training with out_mesh_size, to 16x16.
 * Replaces: EEMFlow.forward(events1, events2)[1][0]  (model/EEMFlow/EEMFlow.py:122-183), i.e. the
 * call made by TestRaftEvents.run_network (test_mvsec.py:1444-1455). */
int eemflow_forward(eemflow_ctx* ctx, const float* events1, const float* events2, int batch, int in_h,
                    int in_w, float* flow_out, int out_h, int out_w, void* stream);

/* nframes (1..16) INDEPENDENT samples as one batch-nframes chain: events1[i] / events2[i] are [1][C][in_h][in_w] tensors and
 * flow_out[i] a [1][2][out_h][out_w] tensor, each wherever the caller has it (16-byte aligned; the three arrays are HOST arrays of
 * device pointers, read before the call returns).  Bitwise the result of eemflow_forward on the batch of those frames: the same
 * kernels in the same launch configuration - only the first conv and the upsampling find each frame through a device table of
 * per-frame pointers, which one small launch rewrites in front of the cached graph's replay.  Why: one frame's launches leave most
 * of the 256 CUs idle (64 - 120 tiles in the 32 / 64-channel layers, 240 pixels in the tail); a caller with several samples at hand -
 * the evaluation loop below - gets the batched chain without first copying them into one tensor.
 * Replaces: n iterations of `for sample in loader: model(events1=im1, events2=im2)` at batch 1, test_mvsec.py:580-597 /
 * TestRaftEvents.run_network (test_mvsec.py:1444-1455). */
int eemflow_forward_many(eemflow_ctx* ctx, int nframes, const float* const* events1, const float* const* events2,
                         float* const* flow_out, int in_h, int in_w, int out_h, int out_w, void* stream);

/* Volumes per eemflow_forward_stream call: the per-frame pointer table of eemflow_forward_many holds 16 frames. */
#define EEM_STREAM_MAX_VOLUMES 16

/* Flow along a stream of CONSECUTIVE event windows, each window encoded once.  volumes[j] (j < nvol, 1..EEM_STREAM_MAX_VOLUMES) are
 * [1][C][in_h][in_w] windows in time order and flow_out[p] [1][2][out_h][out_w] tensors (HOST arrays of 16-byte aligned device
 * pointers, as in eemflow_forward_many).  Flow p is the flow from the older window of pair p to the newer one: with a window carried
 * from the previous call the pairs are (carried, v0), (v0, v1), ... and nflow == nvol; with none, (v0, v1), ... and nflow == nvol - 1
 * (flow_out may then be NULL for nvol == 1).  Any other nflow is an error.  Afterwards the context carries v[nvol-1]: its three pooled
 * feature maps (16 + 32 + 64 channels on the 1/64 grid), in context-owned memory that forward / forward_many / training calls leave
 * alone.  Flow p is bitwise eemflow_forward_many on the pairs in the same encoder form (EEM_WINO4_LAYERS / f4 policy: the call
 * counts as nvol / 2 samples).  A carried window made with other weights (eemflow_load_weights, eemflow_update_weights, an
 * optimizer step) or at another input size is refused with an error: call eemflow_stream_reset.  eemflow_set_deferred_input_norm
 * applies as in eemflow_forward_many.  One stream per context; eemflow_get_stage has nothing to read after a stream call.
 * Replaces: the evaluation loop over consecutive samples of a sequence (test_mvsec.py:580-597 at stride 1, samples built by
 * loader/MVSEC.py:115-116 from windows i and i + 1), which runs EEMFlow.forward's encoder (model/EEMFlow/EEMFlow.py:135-154) on
 * every window twice. */
int eemflow_forward_stream(eemflow_ctx* ctx, int nvol, const float* const* volumes, float* const* flow_out, int nflow, int in_h,
                           int in_w, int out_h, int out_w, void* stream);

/* Volumes per eemflow_forward_stream_bidir call: its 2 * nflow flows share the 16 frames of the per-frame pointer table. */
#define EEM_STREAM_BIDIR_MAX_VOLUMES 8

/* eemflow_forward_stream with BOTH directions of every pair: flow_fw_out[p] is the flow from the older to the newer window of pair p
 * (what eemflow_forward_stream gives), flow_bw_out[p] the flow from the newer to the older one.  The encoder runs once per new window,
 * exactly as in eemflow_forward_stream: the pooled maps of a window do not depend on which side of a pair it sits on, so the tail
 * (correlation, rconv, decoders, out_conv, upsample) runs over 2 * nflow pairs, the second half with the two windows' roles exchanged -
 * 0.4 % of a frame's MACs per extra flow.  nvol is 1..EEM_STREAM_BIDIR_MAX_VOLUMES.  Windows, the carried window, the nflow rule, the
 * weight-version and size refusals, eemflow_stream_reset and eemflow_set_deferred_input_norm are those of eemflow_forward_stream, and
 * the two calls share the context's one stream state: either may follow the other with the carry intact.
 * In the same encoder and decoder forms (EEM_WINO4_LAYERS; EEM_DEC_WNC - the decoders' kernel choice follows the batch, here
 * 2 * nflow) flow_fw_out[p] is bitwise eemflow_forward_many on (v_p, v_p+1) and flow_bw_out[p] bitwise eemflow_forward_many on
 * (v_p+1, v_p).
 * Replaces: two passes of the evaluation loop (test_mvsec.py:580-597), the second with events1 / events2 exchanged, as the input of
 * occ_check_model (utils_luo/tools.py:1148): four runs of EEMFlow.forward's encoder (model/EEMFlow/EEMFlow.py:135-154) per pair. */
int eemflow_forward_stream_bidir(eemflow_ctx* ctx, int nvol, const float* const* volumes, float* const* flow_fw_out,
                                 float* const* flow_bw_out, int nflow, int in_h, int in_w, int out_h, int out_w, void* stream);

/* Drop the carried window: the next eemflow_forward_stream call starts a new stream.
 * Replaces: the start of a sequence in test_mvsec.py:580-597 (dataset.change_test_sequence). */
int eemflow_stream_reset(eemflow_ctx* ctx);

/* *out = 1 when a window is carried for the next eemflow_forward_stream call, else 0.
 * Replaces: nothing in the reference (it has no stream state); the query behind EEMFlow.forward_stream's bookkeeping. */
int eemflow_stream_pending(eemflow_ctx* ctx, int* out);

/* Per-kernel timing of the forward schedule: the schedule runs `reps` + 1 times as the chain it is (eagerly, the first pass warms and
 * is not counted) with a pair of HIP events around EVERY launch, recorded on `stream` (the stream the kernels run on); `ms` is the
 * average per launch - each kernel measured behind its producer, as it runs in a forward.  `flops` / `bytes` are the ALGORITHMIC
 * work of one launch (conv MACs x 2; compulsory input + output + weight bytes).  flow_out receives the correct flow.
 * reps < 0: the other form - every kernel of the schedule -reps times back to back between one pair of events (launches of a few
 * microseconds, which an event pair per launch would mostly measure the gaps of).
 * Replaces: the reference's time_eval() wall-clock loop (model/EEMFlow/EEMFlow.py:201-225), per kernel. */
typedef struct eemflow_kernel_stat {
    char name[48];
    double flops;
    double bytes;
    float ms;
    int blocks;      /* workgroups of the launch (0: not reported): the encoder's kernels are persistent, one workgroup per CU,
                        so blocks < 256 means the launch occupies that many of the 256 CUs */
    int pipe;        /* matrix pipe of the launch's contraction: 0 = fp32 MFMA, 1 = fp32 products as six bf16-piece MFMAs (conv_bx3.hip),
                        2 = Winograd F(4x4,3x3) on the fp32 MFMA (a quarter of the direct form's multiplies), 3 = F(2x2,3x3) (1 / 2.25) */
    int reserved;    /* the launcher's tag for the instantiation it chose, 0 where it has none (the 64-channel F(4x4) layers: 1 = the
                        shared-V form of conv_wino4.hip) */
} eemflow_kernel_stat;
int eemflow_time_kernels(eemflow_ctx* ctx, const float* events1, const float* events2, int batch, int in_h,
                         int in_w, float* flow_out, int out_h, int out_w, int reps, eemflow_kernel_stat* stats,
                         int max_stats, int* nstats, void* stream);

/* Copy an intermediate of the LAST forward into dst (device).  Names: "f11","f12","f13" (stage
 * outputs, images 0..B-1 = events1, B..2B-1 = events2), "pool_1".."pool_3", "cat_1".."cat_3"
 * ([cv(53) | r(16)]), "flow_1".."flow_3" (as channels 0-1, 2-3, 4-5 of "flowcat"), "flowcat",
 * "coarse".  dims_out = [n, c, h, w].  For parity tests against the oracle's stage tensors.
 *
 * While the workspace holds a training forward (eemflow_forward_train / eemflow_forward_backward, and no inference, forward_many
 * or stream call since), also: "padded" ([2B][n_first_channels][hp][wp]: both event volumes replicate-padded, events1 first) and
 * the decoders' activations "ta_k", "tb_k", "tc_k", "td_k" ([B][100][gh][gw]: conv1's output, then conv2, conv3, conv4's outputs
 * after the channel shuffle), "t64_k", "t32_k" (conv5, conv6), k = 1..3.
 * After eemflow_backward / eemflow_forward_backward for THAT forward, the gradient buffers "g_<name>" (the call fails while no
 * backward has run for the current training forward):
 *   tail, d loss / d the stored tensor: "g_flow" ([B][2][out_h][out_w], the loss kernel's d loss / d flow; eemflow_forward_backward
 *   only), "g_coarse", "g_flowcat", "g_t32_k", "g_t64_k", "g_td_k", "g_tc_k", "g_tb_k", "g_ta_k" (before the LeakyReLU' of the
 *   tensor's own layer: d loss / d its output), "g_cat_k" ([B][69][gh][gw]), "g_pool_k" ([2B][16 / 32 / 64][gh][gw]: the pooled
 *   maps of both volumes, events1 first);
 *   encoder, d loss / d the PRE-activation of the layer that produced the tensor (LeakyReLU' of its stored output applied; for the
 *   stage outputs f11 / f12 / f13 with the pooling branch added before that): "g_f13", "g_b3", "g_a3", "g_f12", "g_b2", "g_a2",
 *   "g_f11", "g_a1" ([2B][C][h][w] like the activations).  pconv1_1 gets no data gradient. */
int eemflow_get_stage(eemflow_ctx* ctx, const char* name, float* dst, size_t dst_capacity_floats,
                      int dims_out[4], void* stream);

/* One decoder (k = 1..3) on a caller-supplied [batch][69][h][w] input -> [batch][2][h][w].
 * Replaces: Decoder.forward  (model/EEMFlow/EEMFlow.py:59-69). */
int eemflow_decoder(eemflow_ctx* ctx, int k, const float* x, int batch, int h, int w, float* out, void* stream);

/* 9x9 local correlation of two [batch][c][h][w] maps, 53 selected taps, scaled by 1/c
 * -> out [batch][53][h][w].
 * Replaces: Correlation.forward + torch.index_select  (model/EEMFlow/EEMFlow.py:14-23,160), i.e.
 * spatial_correlation_sampler.SpatialCorrelationSampler(1, 9, 1, 0, 1) (requirements.txt:131). */
int eemflow_local_corr53(const float* f1, const float* f2, int batch, int c, int h, int w, float* out,
                         void* stream);

/* Bilinear resize, align_corners=False: in [nc][h][w] -> out [nc][oh][ow].
 * Replaces: EEMFlow.upsample_flow = F.interpolate(..., mode='bilinear', align_corners=False)
 * (model/EEMFlow/EEMFlow.py:118-120). */
int eemflow_upsample_bilinear(const float* in, float* out, int nc, int h, int w, int oh, int ow, void* stream);
/* Its adjoint, the kernels eemflow_backward runs: d [nc][oh][ow] -> out [nc][h][w]; tmp: [nc][oh][w] floats of scratch. */
int eemflow_upsample_bilinear_bwd(const float* d, float* tmp, float* out, int nc, int oh, int ow, int h, int w, void* stream);

/* Evaluation statistics of one flow field against its ground truth, on the device.
 * Replaces: Test.flow_error (test_mvsec.py:291-346).  flow_gt, flow_pred: [2][h][w]; event_img: [h][w] event counts for the
 * 'sparse' evaluation or NULL ('dense'); max_row: rows >= max_row are ignored (190 for the MVSEC is_car crop, else >= h -
 * note the reference passes the WIDTH there, test_mvsec.py:296).  out5 (device, 5 doubles): sum EE, sum |gt|, n_points,
 * count(EE < 1), count(EE < 3 or EE < 0.1 |gt|) over the pixels with finite non-zero ground truth (and event_img > 0). */
int eemflow_flow_error(const float* flow_gt, const float* flow_pred, const float* event_img, int h, int w, int max_row,
                       double* out5, void* stream);

/* The same statistics for n (1..16) samples of one image size by ONE launch - the samples of an eemflow_forward_many call: flow_gt[i],
 * flow_pred[i], event_img[i] (event_img may be NULL: 'dense') are HOST arrays of device pointers; out5n (device): n x 5 doubles, row i
 * as eemflow_flow_error gives for sample i.
 * Replaces: n calls of Test.flow_error in the evaluation loop (test_mvsec.py:580-597 -> :291-346). */
int eemflow_flow_error_many(int n, const float* const* flow_gt, const float* const* flow_pred, const float* const* event_img, int h,
                            int w, int max_row, double* out5n, void* stream);

/* Forward-backward consistency masks of n (1..16) bidirectional flow pairs of one image size by ONE launch: flow_fw[i], flow_bw[i]
 * ([1][2][h][w]) and mask_fw_out[i], mask_bw_out[i] ([1][1][h][w], 1.0 = consistent, 0.0 = occluded / unreliable) are HOST arrays of
 * device pointers.  With len(x) = sqrt(x_u^2 + x_v^2):
 *     thresh  = alpha1 * (len(fw) + len(bw)) + alpha2
 *     mask_fw = len(fw + torch_warp(bw, fw)) < thresh,   mask_bw = len(bw + torch_warp(fw, bw)) < thresh
 * torch_warp is eemplus_warp's mode 1 (the same device routine: normalised by W - 1 / H - 1, sampled with align_corners=False and zero
 * padding - half a pixel off, as the reference is).  mode 0 ('all'): these masks; 1 ('obj'): a pixel whose target x + flow leaves
 * [0, W-1] x [0, H-1] is forced to 1; 2 ('out'): the outgoing mask alone (1 inside, 0 leaving).  A mask is a valid `event_img` of
 * eemflow_flow_error: the statistics over the consistent pixels.
 * Replaces: occ_check_model.__call__ (utils_luo/tools.py:1148-1220, :1273-1309; occ_type 'for_back_check', scale 1) on
 * tensor_tools.torch_warp (utils_luo/tools.py:2262-2306). */
int eemflow_fb_check_many(int n, const float* const* flow_fw, const float* const* flow_bw, float* const* mask_fw_out,
                          float* const* mask_bw_out, int h, int w, float alpha1, float alpha2, int mode, void* stream);

/* Colour images of n (1..16) flow fields of one size by two launches: flow[i] ([2][h][w] fp32) and image_out[i] ([h][w][3] bytes, RGB,
 * or BGR with bgr != 0) are HOST arrays of device pointers.  The Middlebury colour wheel, normalised by each frame's own maximum radius:
 * |u| or |v| > 1e7 is unknown (black, not part of the maximum); maxrad is the fp32 maximum of sqrt(u*u + v*v), or -1 when the frame
 * holds a NaN; the divisor is (double)maxrad + 2^-52 and the normalised components, radius, angle and wheel interpolation are fp64;
 * rad <= 1 fades towards white, rad > 1 is darkened by 0.75; NaN pixels are black; a byte is floor(255 * col).
 * stats (device, n x 4 doubles, initialised by the call): [i][0] receives frame i's divisor, [i][1] is its reduction cell.
 * Stream-ordered, no host synchronisation, no allocation.
 * Replaces: tensor_tools.flow_to_image_dmax (utils_luo/tools.py:2385-2523) as Test.visualize_optical_flow_light calls it in the
 * evaluation loop (test_mvsec.py:618-629). */
int eemflow_flow_to_image_many(int n, const float* const* flow, uint8_t* const* image_out, double* stats, int h, int w, int bgr,
                               void* stream);

/* Red / blue event images of n (1..16) event volumes of one size by two launches: volume[i] ([bins][h][w] fp32) and image_out[i]
 * ([h][w][3] bytes) are HOST arrays of device pointers.  s = the channel sum (fp32, channel order); white background, s <= mean(s) - 0.2
 * is [255, 0, 0], s >= mean(s) + 0.2 is [0, 0, 255] (painted last); the mean is taken in fp64 and rounded to fp32 once.  norm: NULL
 * (normalised volumes) or a HOST array of device pointers to each raw grid's record {mean, sd, scale, any} (eemflow_voxelize with
 * normalize = 2): non-zero voxels are normalised as the first convolution does before they are summed.
 * stats (device, n x 4 doubles, initialised by the call): [i][0] receives the density count(s > 0.1) / (h*w), [i][1] the sum of s,
 * [i][2] the count.  bgr != 0 writes the channels in reverse order.  Stream-ordered, no host synchronisation, no allocation.
 * Replaces: Test.vis_map_RGB (test_mvsec.py:175-233), up to the array it hands to cv2.imwrite. */
int eemflow_event_image_many(int n, const float* const* volume, const float* const* norm, int bins, int h, int w,
                             uint8_t* const* image_out, double* stats, int bgr, void* stream);

/* Warped positions of n events under a flow: events [n][4] f64 (t, x, y, p) on the device, flow [2][h][w] fp32 (NULL: zero flow) ->
 * warped_xy [n][2] f64.  In unfused fp64: xe = x - ox, ye = y - oy; (u, v) = the bilinear sample of the flow at (xe, ye) in pixel
 * coordinates (grid_sample with align_corners=True and zero padding: a neighbour outside the frame contributes 0);
 * tau = (t - t0) * scale; xw = xe + u * tau, yw = ye + v * tau.  With ox = oy = 0 and scale = 1 this is the reference's function.
 * Replaces: warp_events_flow_torch (utils_luo/event_utils.py:9-51), as Test.inference_img_warp_loss calls it (test_mvsec.py:753-852). */
int eemflow_warp_events(const double* events, int64_t n, const float* flow, int h, int w, double t0, double scale, double ox, double oy,
                        double* warped_xy, void* stream);

/* Images of warped events of k (1..32) jobs of one frame size by ONE launch sequence: events[i] ([n[i]][4] f64, time-sorted; n[i] may be
 * 0), flows[i] ([2][h][w] fp32; a NULL entry, or flows == NULL, is the zero flow), t0[i], scale[i] and iwe[i] ([2][h][w] fp32) are HOST
 * arrays, read before the call returns.  Every event is warped as eemflow_warp_events warps it and votes bilinearly - weights
 * (1-gx)(1-gy), gx(1-gy), (1-gx)gy, gx gy around (floor(yw), floor(xw)) - into channel 0 (p > 0) or 1; a target outside the frame is
 * dropped on its own, an event with a non-finite warped position is dropped whole and counted.  Every cell is the fp64 sum of its votes
 * rounded to fp32 once, and every cell is written.  moments (device, k x 4 doubles): {h*w, sum S, sum S^2, dropped} with
 * S = iwe[0] + iwe[1] of the stored values, summed in a fixed order - the flow warp loss is var(S under the flow) / var(S under zero
 * flow).  EEM_IWE_DIRECT=1 (read per call) takes the direct atomic form instead of the binned one.  Stream-ordered, no host
 * synchronisation; scratch is owned by the library.
 * Replaces: warp_events_flow_torch (utils_luo/event_utils.py:9-51) and the image / variance-ratio part of Test.inference_img_warp_loss
 * (test_mvsec.py:753-852, the ratio at :821-824). */
int eemflow_iwe_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                     const double* scale, double ox, double oy, int h, int w, float* const* iwe, double* moments, void* stream);

/* eemflow_iwe_many with an affine event map per job in place of the offset: maps (HOST, k x 4 doubles) holds (ax, bx, ay, by), and
 * xe = ax * x + bx, ye = ay * y + by - what a resize, a flip and a crop of the frame do to event coordinates.  (1, -ox, 1, -oy) is the
 * offset (ox, oy), bit for bit; eemflow_iwe_many calls this entry with that map.  The same kernels, the same image and moments.
 * Replaces: warp_events_flow_torch (utils_luo/event_utils.py:9-51) and the image / variance-ratio part of Test.inference_img_warp_loss
 * (test_mvsec.py:753-852), for events of an augmented sample (the reference augments frames only and has no such map). */
int eemflow_iwe_map_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                         const double* scale, const double (*maps)[4], int h, int w, float* const* iwe, double* moments, void* stream);

/* Gradient of var(S) of eemflow_iwe_map_many's images with respect to the flows, times a scalar per job: grads[i] ([2][h][w] fp32,
 * HOST array of device pointers) = coef[i] * d var_i / d flows[i].  events, n, flows, t0, scale and maps are the forward's; a NULL
 * flows[i] (zero flow) skips job i, whose grads[i] is not touched.  iwe (HOST array of device pointers) and moments (device, k x 4) are
 * what the forward returned for the same jobs; coef is a DEVICE array of k doubles (the upstream gradient; -1 / var0 for the flow warp
 * loss), so no host synchronisation is needed.  In unfused fp64, with the stored image's fp32 rounding taken as the identity:
 * G = 2 (S - mean) / (h w) per cell; per event dX = sum over in-frame targets of G * wy[dy] * (dx ? +1 : -1), dY likewise with
 * wx[dx] * (dy ? +1 : -1); every in-frame sample neighbour k of (xe, ye) receives coef * w_k * tau * dX in channel 0 and
 * coef * w_k * tau * dY in channel 1.  Events the forward dropped whole add nothing.  Every cell of a gradient is written, an fp64 sum
 * rounded to fp32 once; the binned form (default) rounds each contribution to fp32 first, the direct form (EEM_IWE_DIRECT=1, frames too
 * wide for a band) does not.  The order of the sums is free: the last bits of the fp64 sums may differ from run to run.
 * Replaces: loss.backward() through warp_events_flow_torch (utils_luo/event_utils.py:9-51) and the variance of the image of warped
 * events (test_mvsec.py:821-824) - the reference evaluates this measure and never trains on it. */
int eemflow_iwe_grad_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                          const double* scale, const double (*maps)[4], int h, int w, const float* const* iwe, const double* moments,
                          const double* coef, float* const* grads, void* stream);

/* Images of average timestamps of k (1..32) jobs of one frame size by ONE launch sequence.  A job is an eemflow_iwe_map_many job (the
 * same HOST arrays, the same warp, votes and drops) plus the scalar eps > 0.  An event's timestamp value is a = max(1 - |tau|, 0),
 * tau = (t - t0) * scale, rounded to fp32 once (ah).  Per channel and cell, in unfused fp64: D = sum of the votes' weights and
 * N = sum of weight * ah, both with the fixed-point weights q / 2^31, q = round(w * 2^31), so iwe_out[i] ([2][h][w] fp32) is bitwise
 * the image eemflow_iwe_map_many's binned form writes for the job; ts_out[i] ([2][h][w] fp32) is T = N / (D + eps) rounded to fp32
 * once.  Every cell of both is written.  moments (device, k x 4 doubles): {h*w, sum T^2 over both channels of the stored T, active =
 * pixels with stored D[0] + D[1] > 0, dropped}, summed in a fixed order; the loss of a job is sum T^2 / (active + 1e-9) (or sum T^2).
 * EEM_IWE_DIRECT=1 (read per call), a frame wider than 4800 or taller than 1023 one-row bands, or more than 16.7 M events take the
 * direct atomic form (the same quantised weights, the same D).  Stream-ordered, no host synchronisation; scratch is owned by the
 * library.
 * Replaces: warp_events_flow_torch (utils_luo/event_utils.py:9-51) is the warp being composed; the loss itself (the image of average
 * timestamps of Zhu et al. 2019 / Hagenaars et al. 2021) has no counterpart in the reference. */
int eemflow_tsimg_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                       const double* scale, const double (*maps)[4], int h, int w, double eps, float* const* iwe_out,
                       float* const* ts_out, double* moments, void* stream);

/* Gradient of sum T^2 of eemflow_tsimg_many's images with respect to the flows, times a scalar per job: grads[i] ([2][h][w] fp32, HOST
 * array of device pointers) = coef[i] * d (sum T^2)_i / d flows[i].  events .. eps are the forward's; a NULL flows[i] (zero flow) skips
 * job i, whose grads[i] is not touched.  iwe and ts (HOST arrays of device pointers) are the D and T images the forward stored; coef is
 * a DEVICE array of k doubles (the upstream gradient times 1 / (active + 1e-9) for the normalised loss), so nothing synchronises.
 * Teacher-forced, fp32 roundings straight-through: for an event of channel c at an in-frame target cell
 * G = ((2.0 * T) * (ah - T)) / (D + eps) in fp64 in this order from the stored T and D of channel c (= dL/dN * ah + dL/dD); from G on
 * it is eemflow_iwe_grad_many's arithmetic and kernels: dX = sum of G * wy * (+1 or -1), dY likewise, coef * w_k * tau * dX and
 * coef * w_k * tau * dY to every in-frame sample neighbour, the same conventions at integer positions, the same binned (each
 * contribution rounded to fp32 first) and direct forms.  Every cell of a gradient is written, an fp64 sum rounded to fp32 once.
 * Replaces: warp_events_flow_torch (utils_luo/event_utils.py:9-51) is the warp being differentiated; the loss itself has no counterpart
 * in the reference. */
int eemflow_tsimg_grad_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                            const double* scale, const double (*maps)[4], int h, int w, double eps, const float* const* iwe,
                            const float* const* ts, const double* coef, float* const* grads, void* stream);

/* Test observable: the launch sequence this thread's last eemflow_tsimg_many / eemflow_tsimg_grad_many call ran, e.g.
 * "bin_e2+band1024_s3+moments", "direct", "grad_bin_e1+grad_band", "grad_direct"; "" before any call.  A refused call, and a gradient
 * call without any flow, leave it unchanged.  A string stored on the host beside the launches: no launch, no synchronisation.
 * Replaces: nothing in the reference - warp_events_flow_torch (utils_luo/event_utils.py:9-51) has one form, and the loss itself has no
 * counterpart in the reference. */
int eemflow_tsimg_last_form(char* buf, int cap);

/* Edge-aware smoothness loss of k (1..16) predictions of one shape, and its gradient, by one launch: pred[i] ([B][2][H][W] fp32,
 * contiguous), img[i] ([B][C][H][W] fp32, any C >= 1; a NULL entry, or img == NULL, means every weight is 1) and grad[i] ([B][2][H][W]
 * fp32) are HOST arrays of device pointers, read before the call returns.  For s = order in {1, 2} and both axes (axis 2 = rows, the
 * reference's `x`; axis 3 = columns), in unfused fp64 on the fp32 inputs: d = p[i] - p[i+1] (order 1) or (p[i] - p[i+1]) - (p[i+1] -
 * p[i+2]) (order 2); g_c = constant * (img_c[i] - img_c[i+s]) and w = exp(-mean_c f(g_c)) with f(g) = g * g (weight_type 0, 'gauss')
 * or |g| (1, 'exp'), one weight per (b, i, j) for both flow channels; e(d) = |d| (error_type 0, 'L1') or (|d| + 0.01)^0.4 (1,
 * 'abs_robust'); L = mean over the B*2*(H-s)*W axis-2 terms of e(d) * w + mean over the B*2*H*(W-s) axis-3 terms.
 * loss (device, k doubles; may be NULL) receives L per job - block partial sums go to scratch (device,
 * eemflow_smoothness_scratch_doubles(k, B, H, W) doubles) and are added in a fixed order, so a loss is bitwise the same from run to
 * run.  grad (may be NULL) receives grad[i] = coef[i] * dL_i / dpred_i, every cell written: the fp64 sum over the terms that touch the
 * cell of c * e'(d) * w / N_axis (c = +1, -1 or +1, -2, +1; e' = sign(d) with sign(0) = 0, or 0.4 e(d) / (|d| + 0.01) sign(d)), times
 * coef, rounded to fp32 once - a gather without atomics, bitwise reproducible.  coef is a DEVICE array of k doubles (the upstream
 * gradient; NULL: 1), so nothing visits the host.  img receives no gradient.  Consecutive jobs that name one img pointer read it and
 * compute the weights once per tile; their results are bitwise those of one-job calls.  Stream-ordered, no host synchronisation, no
 * allocation.  Errors: k out of range, H <= s or W <= s (the reference would take the mean of an empty tensor), unknown order or
 * enum values, neither loss nor grad.  Non-finite inputs propagate.
 * Replaces: Loss_tools.edge_aware_smoothness_order1 (utils_luo/tools.py:3008-3047), Loss_tools.edge_aware_smoothness_order2
 * (utils_luo/tools.py:3049-3090) and Loss_tools.flow_smooth_delta (utils_luo/tools.py:3092-3110; order 1, L1, no img), and their
 * autograd. */
int eemflow_smoothness_many(int k, const float* const* pred, const float* const* img, int B, int C, int H, int W, int order,
                            int weight_type, int error_type, double constant, const double* coef, double* loss, float* const* grad,
                            double* scratch, void* stream);

/* Doubles of scratch that eemflow_smoothness_many needs for k jobs of shape [B][2][H][W] (0 for arguments it would refuse).
 * Replaces: nothing in the reference (torch.mean owns its temporaries). */
size_t eemflow_smoothness_scratch_doubles(int k, int B, int H, int W);

/* Photometric / census loss between img1 and img2 warped back by a predicted flow, for k (1..16) predictions of one shape, and its
 * gradient with respect to the flow: the data term of ground-truth-free training.  flow[i] ([B][2][H][W] fp32), img1[i] and img2[i]
 * ([B][C][H][W] fp32, any C >= 1), mask[i] ([B][1][H][W] fp32; a NULL entry, or mask == NULL, is a mask of ones) and grad[i]
 * ([B][2][H][W] fp32) are HOST arrays of device pointers, read before the call returns; all contiguous.
 * Yw = grid_sample(img2, grid + flow) is warp_px.h mode 1 in fp32, bit for bit eemplus_warp(mode 1) and the forward-backward check;
 * everything after it is unfused fp64 on those fp32 values.  With d = img1 - Yw per element:
 *   kind 0 'abs_robust' l = (|d| + 0.01)^0.4;   1 'charbonnier' l = (d*d + 1e-6)^0.4;   2 'L1' l = |d + 1e-6|
 *   use_occ == 0: L = sum(l) / (B*C*H*W);  else L = sum(l * mask) / (sum(mask) + 1e-6), the mask broadcast over C in the numerator
 *   and summed over its own B*H*W cells in the denominator.
 *   kind 3 'census', r = max_distance in 1..3: g(I) = sum_c gray[c] * I_c (gray: DEVICE array of C doubles; NULL: 0.2989, 0.5870,
 *   0.1140 at C == 3, else 1/C each), 0 outside the frame; per centre p and the (2r+1)^2 offsets k: t_k(p) = tau(g(p+k) - g(p)),
 *   tau(x) = x / sqrt(0.81 + x*x);  e = (t_k(img1) - t_k(Yw))^2;  dist(p) = sum_k e / (0.1 + e);  mask' = mask times the indicator of
 *   r <= y < H-r, r <= x < W-r;  n = B*H*W;  then the four branches of the reference's photo_loss_function:
 *     charbonnier, use_occ:  S = sum((dist^2 + 1e-6)^q * mask'), M = sum(mask');  L = (S/n) / ((M/n)*2 + 1e-6) (average) or S / (M*2 + 1e-6)
 *     charbonnier, no occ:   sum((dist^2 + 1e-8)^q) / n (average) or the sum; no mask, the border included
 *     abs_robust, use_occ:   sum((|dist| + 0.01)^q * mask') / (2 * sum(mask') + 1e-6), whatever `average` says
 *     abs_robust, no occ:    sum((|dist| + 0.01)^q) / n (average) or the sum
 * loss (device, k doubles; may be NULL) receives L per job.  grad (may be NULL) receives coef[i] * dL_i / dflow_i, every cell written:
 * dL/dflow(p) = sum_c dL/dYw_c(p) * dYw_c/d(u,v)(p), the warp derivative being that of the bilinear blend at the fp32 tap weights
 * (corners outside the frame are zeros) times (W/2) * (2/max(W-1,1)) (and the same in H), in fp64, rounded to fp32 once; |x| has
 * derivative 0 at 0 and the denominators do not depend on the flow.  For census dL/dg(Yw)(p) is gathered over p's own taps and the
 * centres whose patch holds p from a per-centre factor plane in LDS: no atomics anywhere, losses and gradients are bitwise
 * reproducible.  coef is a DEVICE array of k doubles (the upstream gradient; NULL: 1).  scratch (device,
 * eemflow_photo_scratch_doubles(k, B, H, W) doubles) is always needed: the denominators and the per-block partial sums, added in a
 * fixed order.  Consecutive jobs that name one img1 pointer grey-combine it once per tile; a job's results are bitwise those of a
 * one-job call.  Stream-ordered, no host synchronisation, no allocation.  Errors: k out of range, unknown kind, census with r outside
 * 1..3 or H <= 2r or W <= 2r, neither loss nor grad.  Non-finite inputs propagate.
 * Replaces: Loss_tools.photo_loss_multi_type (utils_luo/tools.py:3112-3135; its 'SSIM' kind is eemflow_ssim_many), Loss_tools.photo_loss_function
 * (3137-3169) and Loss_tools.census_loss_torch (3171-3212) on tensor_tools.torch_warp (2262-2306), and their autograd. */
int eemflow_photo_many(int k, const float* const* flow, const float* const* img1, const float* const* img2, const float* const* mask,
                       int B, int C, int H, int W, int kind, int use_occ, int charbonnier, int average, int max_distance, double q,
                       const double* gray, const double* coef, double* loss, float* const* grad, double* scratch, void* stream);

/* Doubles of scratch that eemflow_photo_many needs for k jobs of shape [B][2][H][W] (0 for arguments it would refuse).
 * Replaces: nothing in the reference (torch.sum owns its temporaries). */
size_t eemflow_photo_scratch_doubles(int k, int B, int H, int W);

/* Weighted SSIM loss between img1 and img2 warped back by a predicted flow, for k (1..16) predictions of one shape, and its gradient
 * with respect to the flow: the structural data term of ground-truth-free training, beside eemflow_photo_many.  flow, img1, img2, mask
 * and grad are as there: HOST arrays of device pointers to contiguous fp32 [B][2|C|C|1|2][H][W]; a NULL mask entry, or mask == NULL, is
 * a weight of ones.  Yw = grid_sample(img2, grid + flow) is warp_px.h mode 1 in fp32, bit for bit eemplus_warp(mode 1); everything
 * after it is unfused fp64 on those fp32 values.  With x = img1, y = Yw, w = mask, per channel and per centre m of [1,H-2] x [1,W-2],
 * avg3x3(z)(m) = (the nine values of z around m, added in row-major order - rows top to bottom, each left to right) / 9:
 *   aw = avg3x3(w);  wpe = w + weight_epsilon;  inv = 1 / (aw + weight_epsilon);  P[z] = avg3x3(z * wpe) * inv
 *   mu_x = P[x], mu_y = P[y], s_x = P[x*x] - mu_x*mu_x, s_y = P[y*y] - mu_y*mu_y, s_xy = P[x*y] - mu_x*mu_y
 *   c1 == inf:  n = 2 s_xy + c2,  d = s_x + s_y + c2            (the structure term; the default with c2 = 9e-6)
 *   c2 == inf:  n = 2 mu_x mu_y + c1,  d = mu_x*mu_x + mu_y*mu_y + c1                     (the luminance term)
 *   both finite:  n and d are the products of the two
 *   l = clamp((1 - n / d) / 2, 0, 1)
 *   use_occ == 0: L = sum(l) / (B*C*(H-2)*(W-2));  else L = sum(l * aw) / (sum(aw) + 1e-6), aw broadcast over C in the numerator and
 *   summed over its own B*(H-2)*(W-2) cells in the denominator (photo_loss_multi_type's form).
 * loss (device, k doubles; may be NULL) receives L per job.  grad (may be NULL) receives coef[i] * dL_i / dflow_i, every cell written:
 * per centre the three factors dl/dmu_y, dl/dP[y*y] and dl/dP[x*y] (the clamp passes the gradient on 0 <= v <= 1, both ends included),
 * each times inv/9, aw with use_occ, and coef / (n1 D), go into LDS planes; every cell p gathers their sums SA, SB, SC over the up to
 * nine centres whose window holds it, dL/dYw_c(p) = wpe(p) * (SA + 2 y(p) SB + x(p) SC), then the derivative of the bilinear blend at
 * the fp32 tap weights times (W/2) * (2/max(W-1,1)) (and the same in H) as in eemflow_photo_many, summed over the channels in fp64 and
 * rounded to fp32 once.  The images and the mask receive no gradient and the denominators do not depend on the flow.  No atomics:
 * losses and gradients are bitwise reproducible, and a job's results are bitwise those of a one-job call.  coef is a DEVICE array of k
 * doubles (the upstream gradient; NULL: 1).  scratch (device, eemflow_ssim_scratch_doubles(k, B, H, W) doubles) is always needed: the
 * denominators and the per-block partial sums, added in a fixed order.  Stream-ordered, no host synchronisation, no allocation.
 * Errors: k out of range, H < 3 or W < 3, C < 1, c1 or c2 not positive or both infinite, weight_epsilon not positive, neither loss nor
 * grad, a NULL pointer.  Non-finite inputs propagate.
 * Replaces: Loss_tools.weighted_ssim (utils_luo/tools.py:2951-3006) under Loss_tools.photo_loss_multi_type's 'SSIM' kind (3126-3135) on
 * tensor_tools.torch_warp (2262-2306), and their autograd. */
int eemflow_ssim_many(int k, const float* const* flow, const float* const* img1, const float* const* img2, const float* const* mask,
                      int B, int C, int H, int W, int use_occ, double c1, double c2, double weight_epsilon, const double* coef,
                      double* loss, float* const* grad, double* scratch, void* stream);

/* Doubles of scratch that eemflow_ssim_many needs for k jobs of shape [B][2][H][W] (0 for arguments it would refuse).
 * Replaces: nothing in the reference (torch.sum owns its temporaries). */
size_t eemflow_ssim_scratch_doubles(int k, int B, int H, int W);

/* Event voxelization: events [n][4] f64 (t, x, y, p) on the device, time-sorted, as held by the
 * reference's EventSequence -> grid [bins][h][w] fp32.  idx_left / idx_right (optional, may be NULL)
 * receive, per event, the int64 flat index x + y*w + bin*w*h of the left / right temporal vote, or -1
 * where the reference masks the vote out.
 * normalize: 0 raw grid; 1 normalised grid (the reference's normalize=True); 2 "deferred" - the grid stays raw and the four floats
 * BEHIND it (grid[bins*h*w .. +4): the buffer must have them) receive {mean, sd, scale ? 1 : 0, any ? 1 : 0} for
 * eemflow_set_deferred_input_norm's consumer.
 * Replaces: EventSequenceToVoxelGrid_Pytorch.__call__  (loader/loader_utils.py:447-537). */
int eemflow_voxelize(const double* events, int64_t n, int bins, int h, int w, int normalize, float* grid,
                     int64_t* idx_left, int64_t* idx_right, void* stream);

/* The two event volumes of a sample (event_volume_old, event_volume_new) in ONE three-launch sequence: the same grids as two
 * eemflow_voxelize calls, bit for bit.
 * Replaces: the two EventSequenceToVoxelGrid_Pytorch calls of a dataset sample  (loader/HREM.py:226-232, loader/MVSEC.py:166-177). */
int eemflow_voxelize_pair(const double* events1, int64_t n1, const double* events2, int64_t n2, int bins, int h, int w,
                          int normalize, float* grid1, float* grid2, void* stream);

/* nsets (1..32) event sets of ONE grid shape - e.g. both volumes of every sample of an eemflow_forward_many call - voxelized by ONE
 * three-launch sequence: events[k] [n_events[k]][4] f64 (t, x, y, p) -> grids[k] [bins][h][w] f32, each bitwise what eemflow_voxelize
 * gives for that set alone.  `events`, `n_events`, `grids` are HOST arrays, read before the call returns.
 * Replaces: the per-sample calls of EventSequenceToVoxelGrid_Pytorch.__call__ (loader/loader_utils.py:459-537) in a loader that has
 * several samples at hand (loader/HREM.py:226-232 for each of them). */
int eemflow_voxelize_many(int nsets, const double* const* events, const int64_t* n_events, int bins, int h, int w, int normalize,
                          float* const* grids, void* stream);

/* TEST OBSERVABLE: what the calling thread's most recent eemflow_voxelize / _pair / _many call launched, as "j<sets>:" and the launches
 * joined with '+': "bin_e<1|2|4|8>" (the binning kernel's events per thread), "band<256|512|1024>_<v4|v1>_s<2..6>_<mode>" (the band
 * kernel's threads per block, its 16-byte or scalar read-out, log2 of the lanes per run; mode "raw", "raw_sums" - raw grid, moments left
 * for the pass that follows -, "moments", "normalised"), then "norm" (vox_norm_kernel) or "stats" (the deferred record); the direct atomic
 * kernel reports "direct", "direct+moments+norm" or "direct+moments+stats".  E.g. "j1:bin_e1+band1024_v4_s2_raw_sums+norm",
 * "j2:bin_e2+band256_v1_s4_moments+band256_v1_s4_normalised".  Several sets that fall to the direct kernel run one after the other and
 * report the last ("j1:direct...").  A few integers stored on the host per call; "" before any call, unchanged by a refused one. */
int eemflow_voxelize_last_form(char* buf, int cap);

/* The DSEC voxel grid E-RAFT was trained on: nsets (1..32) event sets of ONE grid shape by one launch sequence, each given as its four
 * COLUMNS on the device, n_events[k] >= 1 elements each.  t[k], p[k] are fp32; x[k], y[k] are fp32 sub-pixel coordinates (xy_type
 * EEMFLOW_XY_F32, rectify_maps NULL), or RAW sensor coordinates (EEMFLOW_XY_I16 / _I32) that rectify_maps[k] - [map_h][map_w][2] fp32 on the
 * device, one per set - turns into (x, y) = map[y_raw][x_raw]; an event whose raw coordinate lies outside the map is dropped.
 * Every operation is unfused fp32:  dT = t[n-1] - t[0];  tn = ((float)(bins-1) * (t_i - t[0])) / dT;  x0 = (int)x, y0 = (int)y,
 * b0 = (int)tn (truncation toward zero, so a coordinate in (-1, 0) votes with one negative weight);  val = 2 p - 1;  each of the eight
 * corners (xl, yl, bl) in {x0, x0+1} x {y0, y0+1} x {b0, b0+1} that lies inside the grid receives
 * ((val * (1 - |xl - x|)) * (1 - |yl - y|)) * (1 - |bl - tn|); corners at xl == w, yl == h, bl == bins are masked (nothing wraps).
 * An event whose x, y or tn is not finite or not below 2^31 in magnitude is dropped whole - dT == 0 (one event included) drops every
 * event and leaves a grid of +0.0.  Only t[0] and t[n-1] set the scale: the sets need not be sorted.  grids[k] [bins][h][w] fp32: every
 * cell is the fp64 sum of its votes rounded to fp32 once, every untouched cell +0.0, all cells stored (no memset needed; any 4-byte
 * alignment).  normalize: 0 raw, 1 mean / unbiased sd over the non-zero voxels (std > 0, else the mean alone).  Each grid is bitwise what
 * a call with that set alone gives.  x, y, t, p, n_events, rectify_maps and grids are HOST arrays, read before the call returns.
 * Stream-ordered, no host synchronisation.  eemflow_voxelize_last_form reports the sequence as "tri:j<sets>:" + "bin_e<1|2>[_i16|_i32]" +
 * the band kernel's form as above (+ "+norm"), or "tri:j1:direct64[...]+finish[+norm]" for the fp64-atomic form that grids beyond the
 * LDS layout (and EEM_VOX_DIRECT=1) take.
 * Replaces: VoxelGrid.convert (utils/dsec_utils.py:19-64) and, with a map, the rectification lookup in front of it. */
#define EEMFLOW_XY_F32 0
#define EEMFLOW_XY_I16 1
#define EEMFLOW_XY_I32 2
int eemflow_voxelize_trilinear_many(int nsets, const void* const* x, const void* const* y, const float* const* t, const float* const* p,
                                    const int64_t* n_events, int xy_type, const float* const* rectify_maps, int map_h, int map_w,
                                    int bins, int h, int w, int normalize, float* const* grids, void* stream);

/* Event preparation: nsets (1..EEMFLOW_PACK_MAX) event sets, each given as its four COLUMNS on the device - t[k], x[k], y[k], p[k], n_events[k]
 * elements each, of the dtype codes[4*k + 0..3] (EEMFLOW_PACK_*; a bool column is uploaded as u8) - packed by ONE launch into
 * out[k] [n_events[k]][4] f64 (t, x, y, p): the table eemflow_voxelize, the IWE entry points and a loader's `events` take.  Every value
 * is converted as NumPy's astype(float64) converts it (exact but for int64: round to nearest even); tt = ((double)t * scale_a) * scale_b
 * as two separately rounded products; out[i][0] = tt[i] - tt[0] with relative != 0, else tt[i]; out[i][1..3] = x, y, p.  p arrives
 * already as 2*p - 1, formed by the host in the column's own dtype.  The sets must be in time order already (the caller checks the raw
 * t column; eemflow_amd/events.py keeps the host route for the others).  t, x, y, p, codes, n_events and out are HOST arrays, read
 * before the call returns; column pointers are aligned to their elements, out[k] to 16 bytes.  A set with n_events[k] == 0 writes
 * nothing; nsets outside 1..EEMFLOW_PACK_MAX or an unknown code is an error return before any launch.  Stream-ordered, no host
 * synchronisation, no allocation: the job table travels as kernel arguments.
 * Replaces: get_compressed_events (loader/loader_utils.py:26-37) and EventSequence.__init__ (loader/loader_utils.py:352-397) - the
 * float64 table, the two timestamp scalings and absolute_time_to_relative, which the reference does in NumPy on the host. */
#define EEMFLOW_PACK_MAX 32
#define EEMFLOW_PACK_U8 0
#define EEMFLOW_PACK_I8 1
#define EEMFLOW_PACK_U16 2
#define EEMFLOW_PACK_I16 3
#define EEMFLOW_PACK_I32 4
#define EEMFLOW_PACK_I64 5
#define EEMFLOW_PACK_F32 6
#define EEMFLOW_PACK_F64 7
int eemflow_pack_events_many(int nsets, const void* const* t, const void* const* x, const void* const* y, const void* const* p,
                             const int* codes, const int64_t* n_events, double scale_a, double scale_b, int relative,
                             double* const* out, void* stream);

/* The consecutive windows of ONE device-resident recording, voxelized straight from its columns: t, x, y, p are the recording's four
 * base columns on the device in the dtypes codes[0..3] (EEMFLOW_PACK_*, p already 2*p - 1, the recording in time order), window k
 * is the elements [offsets[k], offsets[k+1]) of each (offsets: nwin + 1 HOST integers, ascending, offsets[0] >= 0, the columns at
 * least offsets[nwin] elements long), nwin = 1..32.  Per event of window k, in registers:
 *     tt = ((double)t * scale_a) * scale_b                 two separately rounded products, then - tt[offsets[k]] with `relative`:
 *                                                          eemflow_pack_events_many's row of that slice, bit for bit
 *     the two temporal votes of eemflow_voxelize with t0 = tt[first], dT = tt[last] - tt[first] (0 -> 1) of the WINDOW
 * so grids[k] ((bins,H,W) fp32 on the device, any 4-byte alignment; + four floats with normalize = 2) is bitwise what
 * eemflow_voxelize_many gives for the table that eemflow_pack_events_many makes of the window's slice: the same votes, the same fp64
 * cell sums rounded once, the same moments.  No float64 table is written or read: 13 B of HBM traffic per HREM event in front of
 * the records instead of 13 + 32 + 32.  A window may start at any element (an odd index of a 2-byte column too): the columns are
 * read element by element, and only each column's BASE must be aligned to its element size.
 * Empty windows (offsets[k] == offsets[k+1]) are allowed - the reference cannot be asked about one (it indexes events[-1]); here
 * an empty window's grid is all +0.0 and, with normalize = 2, its record is {0, 1, 0, 0}.
 * normalize: 0 raw, 1 normalised, 2 raw grid + record behind it (as eemflow_voxelize).  Grids beyond the LDS band layout (bins > 64,
 * band_px * bins > 19 200 cells, more than 33.5 M events in a window) and EEM_VOX_DIRECT=1 run, inside this call, as
 * eemflow_pack_events_many into a scratch table and the direct kernel, window by window (fp32 atomics: the values agree with the
 * banded form within 2e-5, not bitwise).  eemflow_voxelize_last_form reports "j<nwin>:colbin_e<1|2|4|8>+band..." (the rest as for
 * eemflow_voxelize) or "j<nwin>:pack+direct[+bin(<m>)][+moments+norm|+moments+stats]"
 * (+bin(<m>): only the longest window was beyond the bands, and m shorter ones took them behind their tables).  codes, offsets and
 * grids are HOST arrays, read before the call returns.  Stream-ordered, no host synchronisation; scratch from the library's arenas as for eemflow_voxelize_many; a bad
 * argument is an error return before any launch.
 * Replaces, for a recording cut into windows: per window a host slice, get_compressed_events and EventSequence.__init__
 * (loader/loader_utils.py:26-37, :352-397) and EventSequenceToVoxelGrid_Pytorch.__call__ (:447-537). */
int eemflow_voxelize_windows(int nwin, const void* t, const void* x, const void* y, const void* p, const int codes[4],
                             const int64_t* offsets, double scale_a, double scale_b, int relative, int bins, int h, int w,
                             int normalize, float* const* grids, void* stream);

/* Windows BY SPAN of one device-resident recording: job k is the elements [starts[k], ends[k]) of each column (starts, ends: nwin HOST
 * integers each, 0 <= starts[k] <= ends[k], the columns at least max(ends) elements long), nwin = 1..32.  There is no ordering between
 * jobs: spans may overlap, nest, repeat or be empty, so windows that slide by less than their length, or pairs of windows at a lag,
 * are voxelized by one launch sequence.  Everything else is eemflow_voxelize_windows, which is this call with starts = offsets and
 * ends = offsets + 1: the same kernels (every job's first element and length already travel separately), the same scratch layout, the
 * banded form, the direct form for grids beyond the LDS layout or under EEM_VOX_DIRECT, the empty window, the same
 * eemflow_voxelize_last_form text.  grids[k] is bitwise what eemflow_voxelize_many gives for the table eemflow_pack_events_many makes
 * of span k's slice; two jobs with the same span get the same grid (each job has its own records: a window's votes depend on its own
 * first and last timestamps).  The grids of a call must not overlap one another.  Stream-ordered, no host synchronisation; a bad
 * argument is an error return before any launch. */
int eemflow_voxelize_spans(int nwin, const void* t, const void* x, const void* y, const void* p, const int codes[4], const int64_t* starts,
                           const int64_t* ends, double scale_a, double scale_b, int relative, int bins, int h, int w, int normalize,
                           float* const* grids, void* stream);

/* MVSEC ground-truth flow of njobs (1..32) windows by ONE launch, from the device-resident ground-truth stack gt ([nframes][2][h][w]
 * fp32: MVSEC's flow_dist, 20 Hz displacement maps; frame f is the displacement between timestamps f and f + 1).  The host plans each
 * window [start, end] (eemflow_amd.mvsec_raw.MvsecGroundTruth.plan, NumPy float64, the reference's searchsorted and scale factors):
 * frame0[k], nsteps[k], a[k], b[k]; out[k] is (2,h,w) fp32 on the device.  frame0, nsteps, a, b and out are HOST arrays, read
 * before the call returns.  One thread walks one pixel of one job through all its steps, the position in registers:
 *   nsteps == 0   the window is shorter than the ground-truth interval (the reference's early return), a = dt, b = gt_dt:
 *                     out = (float)(((double)gt[frame0] * a) / b)          the reference returns this float64; rounded to fp32 ONCE here
 *   nsteps >= 2   x, y start at the pixel's integer coordinates as fp32; step s = 0 .. nsteps-1 reads frame frame0 + s with the
 *                 scale a for the first step, b for the last and 1.0 between:
 *                     ix = rint(x), iy = rint(y)                           round half to even: cv2.remap(INTER_NEAREST) on float maps (cvRound)
 *                     (fu, fv) = gt[frame0 + s][:, iy, ix], or 0 outside [0,w) x [0,h)      BORDER_CONSTANT
 *                     fu == 0 clears the x mask, fv == 0 the y mask        independent and sticky; also on a last step of scale 0
 *                     x = (float)((double)x + (double)fu * scale), y likewise               product and sum unfused, rounded to fp32 once
 *                 out = x - x0, y - y0 in fp32, 0 where the component's mask is cleared.
 *   nsteps == 1 does not occur (the long branch has a first and a last step) and is refused.
 * A NaN flow value is not == 0: it keeps its mask and its component is NaN.  A non-finite position finds no cell and reads 0; that
 * read clears the mask of a component whose own coordinate is finite and leaves a non-finite component as it is, so no NaN or infinity
 * becomes a number (cv2's integer conversion of a non-finite coordinate is undefined).  A job whose frames leave the stack, njobs
 * outside 1..32 or a NULL / misaligned pointer is an error return before any launch.  Stream-ordered, no host synchronisation, no
 * allocation: the plans travel as kernel arguments.
 * Replaces: estimate_corresponding_gt_flow and prop_flow (loader/loader_utils.py:70-161, duplicated in utils/mvsec_utils.py) as
 * loader/MVSEC_encoder.py:130-158 calls them per frame on the CPU - one cv2.remap of each component plus one add per step. */
int eemflow_gt_flow_many(int njobs, const float* gt, int nframes, int h, int w, const int* frame0, const int* nsteps, const double* a,
                         const double* b, float* const* out, void* stream);

/* The event masks of nwin (1..32) consecutive windows of ONE device-resident recording: x, y are the recording's base columns in the
 * dtypes code_x, code_y (EEMFLOW_PACK_*), window k the elements [offsets[k], offsets[k+1]) (offsets: nwin + 1 HOST integers, ascending;
 * empty windows allowed), masks[k] an [h][w] fp32 image on the device (masks: a HOST array).  Every mask is zero-filled, then pixel
 * (min(floor(y), h-1), min(floor(x), w-1)) of every event with 0 <= x <= w and 0 <= y <= h is set to 1.0f by plain stores:
 * np.histogram2d(x, y, bins=(w,h), range=[[0,w],[0,h]]).T > 0, whose last bin is closed.  Two launches, stream-ordered, no host
 * synchronisation.  A mask is a valid `event_img` of the 'sparse' eemflow_flow_error.
 * Replaces: the event_valid image of loader/MVSEC.py:132-142 (eemflow_amd.mvsec.event_mask), built on the host per sample. */
int eemflow_event_mask_windows(int nwin, const void* x, const void* y, int code_x, int code_y, const int64_t* offsets, int h, int w,
                               float* const* masks, void* stream);

/* The event masks of nwin (1..32) windows BY SPAN of one device-resident recording: window k is the elements [starts[k], ends[k]) of the
 * columns (starts, ends: nwin HOST integers each, 0 <= starts[k] <= ends[k]; no ordering between windows: they may overlap, nest, repeat
 * or be empty).  Everything else is eemflow_event_mask_windows, which is this call with starts = offsets, ends = offsets + 1: the same
 * two launches.  The masks of a call must not overlap one another. */
int eemflow_event_mask_spans(int nwin, const void* x, const void* y, int code_x, int code_y, const int64_t* starts, const int64_t* ends, int h,
                             int w, float* const* masks, void* stream);

/* Augmentation of n (1..EEMFLOW_AUGMENT_MAX) training samples of one source size and one output size by ONE launch, written into the
 * batch tensors: vol_old[i], vol_new[i] ([C][H][W] fp32), flow[i] ([2][H][W]; fp64 with flow_f64 != 0, else fp32; a NULL entry, or
 * flow == NULL, is a sample without flow: HREM's mesh flow is returned un-augmented by the reference) and plans[i] are HOST arrays, read
 * before the call returns.  Destinations (device): out_old, out_new [n][C][ch][cw], out_flow [n][2][ch][cw], out_valid [n][ch][cw], all
 * fp32; sample i fills slice i; the last two may be NULL when no sample has a flow, and are left untouched for a sample without one.
 * Output pixel (r, c) reads the resized (or original) RH x RW image at (y0 + r, x0 + c), mirrored first (vflip: row RH-1-row, hflip:
 * column RW-1-column): resize, then flips, then crop, as the host does.  Resized: RH = round(H * scale_y), RW = round(W * scale_x) (ties
 * to even); destination index d samples the source at (d + 0.5) / scale - 0.5, the two neighbours clamped, blended as
 * top = v00*(1-tx) + v01*tx, bot = v10*(1-tx) + v11*tx, out = top*(1-ty) + bot*ty in unfused fp64 and rounded to the source's type.
 * Flow: that sample, times (scale_x, scale_y) in fp64 when resized, times -1 on u for hflip and on v for vflip, rounded to fp32 once.
 * valid = 1 where both written components are finite and their fp32 norm is > 0 (both squares underflowing to 0 counts as 0), else 0.
 * Stream-ordered, no host synchronisation, no allocation: the plans travel as kernel arguments.
 * Replaces: FlowAugmentor.spatial_transform / spatial_transform_no_resize and DenseSparseAugmentor.spatial_transform
 * (utils/augumentor.py:158-257,389-419) on HWC numpy copies of the volumes, at the call sites loader/HREM.py:252 and
 * loader/MVSEC.py:170-187 (with the valid mask of MVSEC.py:185). */
#define EEMFLOW_AUGMENT_MAX 16
typedef struct eemflow_aug_plan {
    double scale_x, scale_y;   /* used when resized != 0 */
    int resized;
    int RH, RW;                /* size of the image the crop is taken from: the source's when not resized */
    int hflip, vflip;
    int y0, x0;                /* top-left corner of the crop */
    int reserved;
} eemflow_aug_plan;
int eemflow_augment_many(int n, const float* const* vol_old, const float* const* vol_new, const void* const* flow, int flow_f64,
                         const eemflow_aug_plan* plans, int C, int H, int W, int ch, int cw, float* out_old, float* out_new,
                         float* out_flow, float* out_valid, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training step of EEMFlow (train_mvsec.py:229-258).  Weights live on the device in state_dict order; one
 * flat gradient buffer in the same order is what a data-parallel job all-reduces (RCCL) between the two calls.
 * ---------------------------------------------------------------------------------------------- */

/* The two halves of autograd through EEMFlow.forward, for torch.autograd.Function (eemflow_amd/eemflow.py):
 * eemflow_forward_train runs the forward eagerly and keeps every activation in the context's workspace;
 * eemflow_backward turns d loss / d flow [batch][2][out_h][out_w] (any loss the caller differentiated) into the flat
 * parameter gradient grad_out (device, 714 352 floats, state_dict order).  `serial_out` identifies the forward whose
 * activations the context holds; eemflow_backward refuses (non-zero return) when another forward has overwritten them -
 * the caller then repeats the forward.  events1/events2 passed to eemflow_backward are that forward's inputs.
 * Replaces: model(im1, im2) under autograd + loss.backward()  (train_mvsec.py:245-253,377-386; autograd of
 * model/EEMFlow/EEMFlow.py:122-183). */
int eemflow_forward_train(eemflow_ctx* ctx, const float* events1, const float* events2, int batch, int in_h, int in_w,
                          float* flow_out, int out_h, int out_w, int64_t* serial_out, void* stream);
int eemflow_backward(eemflow_ctx* ctx, int64_t serial, const float* events1, const float* events2, const float* dflow,
                     float* grad_out, void* stream);

/* The kernel each layer's gradients took in the last backward of this context, as "<layer>.<what>=<form>;" text, e.g.
 * "upsample.bwd=rows;out_conv.wgrad=small;out_conv.dgrad=tail_conv;...;conv7.wgrad=wgrad_tail;...;pconv3_1.dgrad=dgrad_s2;
 * pconv2_2.wgrad=enc_bx3_tw16;...".  Layers: upsample, out_conv, conv1 .. conv7 (all decoders and groups of a layer share one
 * launch), rconv, corr, pool_1 .. pool_3, pconv1_1 .. pconv3_3.  Recorded on the host at dispatch (no synchronisation).  Fails
 * before any backward and when `capacity` (bytes, terminating zero included) is too small. */
int eemflow_backward_forms(eemflow_ctx* ctx, char* dst, size_t capacity);

/* One term of sequence_loss and its gradient: weight * mean over batch*2*h*w of valid*|flow - gt| with
 * valid = (valid >= 0.5) & (|gt| < 400).  dflow_out [batch][2][h][w] = d term / d flow.  stats6 (DEVICE, 6 doubles, added
 * to - the caller zeroes them): sum of valid |flow - gt| (loss term = weight * stats6[0] / (batch*2*h*w)), sum of EPE over
 * valid pixels, valid count, count(EPE < 1), count(EPE < 3), count(EPE < 5).  No host synchronisation.
 * Replaces: train.sequence_loss  (train_mvsec.py:201-227) and its autograd. */
int eemflow_sequence_loss(const float* flow, const float* flow_gt, const float* valid, int batch, int h, int w, float weight,
                          float* dflow_out, double* stats6, void* stream);

/* Forward (train-mode output size), sequence loss for the single prediction (weight = gamma^0 = 1 unless the
 * caller scales it), and the full backward pass.  flow_gt [batch][2][out_h][out_w], valid [batch][out_h][out_w];
 * flow_out [batch][2][out_h][out_w] receives the prediction; grad_out (device, 714 352 floats) receives
 * d loss / d parameter; stats_out (host, 5 doubles, may be NULL): loss, mean EPE over valid pixels, valid
 * count, fraction < 1 px, fraction < 3 px.
 * Replaces: run_network + sequence_loss + scaler.scale(loss).backward()
 * (train_mvsec.py:245-253,201-227; autograd of model/EEMFlow/EEMFlow.py:122-183). */
int eemflow_forward_backward(eemflow_ctx* ctx, const float* events1, const float* events2, const float* flow_gt,
                             const float* valid, int batch, int in_h, int in_w, int out_h, int out_w,
                             float loss_weight, float* flow_out, float* grad_out, double* stats_out, void* stream);

/* clip_grad_norm_(clip) + AdamW(lr, weight_decay, eps, betas 0.9/0.999) on the device-resident weights, then the
 * re-pack of every kernel-side weight layout.  lr is the caller's OneCycleLR value for this step.
 * A gradient with an inf / NaN in it skips the step (see eemflow_optimizer_skipped_steps).
 * Replaces: scaler.unscale_ + clip_grad_norm_ + scaler.step(optimizer)  (train_mvsec.py:254-258,178-183). */
int eemflow_optimizer_step(eemflow_ctx* ctx, const float* grad, float lr, float weight_decay, float eps, float clip,
                           void* stream);

/* The statistics of the last eemflow_forward_backward (called with stats_out = NULL) without a stream synchronisation between the
 * backward and the optimizer step: _async enqueues the copy of the raw sums to pinned host memory and an event on `stream`; the
 * caller enqueues what follows (gradient all-reduce, eemflow_optimizer_step, the next forward); _wait blocks on that event alone and
 * returns stats[5] = loss, mean EPE, valid count, fraction < 1 px, fraction < 3 px - the numbers eemflow_forward_backward returns.
 * Replaces: the .item() reads of sequence_loss's metrics (train_mvsec.py:219-226) - after the step is in flight instead of before. */
int eemflow_train_stats_async(eemflow_ctx* ctx, void* stream);
int eemflow_train_stats_wait(eemflow_ctx* ctx, double stats_out[5]);

/* Steps eemflow_optimizer_step has skipped so far: a gradient holding an inf or a NaN changes neither weights nor moments and does
 * not advance the bias corrections - what GradScaler.step does for the reference (train_mvsec.py:237,257; the schedule still
 * advances, :258).  Synchronises `stream`. */
int eemflow_optimizer_skipped_steps(eemflow_ctx* ctx, int* out, void* stream);

/* Copy the current weights (state_dict order, 714 352 floats) to a device buffer - checkpointing
 * (train_EEMFlow_HREM.py:127-130 saves model.module.state_dict()). */
int eemflow_get_weights(eemflow_ctx* ctx, float* dst, size_t nfloats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E-RAFT (model/eraft.py): feature / context encoders, all-pairs correlation pyramid, 9x9 x 4-level
 * lookup, SepConvGRU update block, convex upsampling.  Inference (eval-mode BatchNorm).
 * ---------------------------------------------------------------------------------------------- */

/* Replaces: ERAFT.__init__ + .to(device)  (model/eraft.py:40-62). */
int eraft_create(int device, eraft_ctx** out);
void eraft_destroy(eraft_ctx* ctx);

/* All float tensors of the reference state_dict() (179 entries; the integer num_batches_tracked buffers are
 * skipped) back to back in registration order: fnet.*, cnet.* (BatchNorm weight, bias, running_mean,
 * running_var; the aliased downsample.1.* entries are present, as in the checkpoint), update_block.*.
 * Replaces: load_state_dict for model/eraft.py:57-62 modules. */
int eraft_load_weights(eraft_ctx* ctx, const float* flat_host, size_t nfloats, int n_first_channels);

/* events1/2 [batch][C][in_h][in_w]; pad = [left, right, top, bottom] from InputPadder(img_size, 'chairs', 32)
 * (model/eraft.py:65-67); flow_init [batch][2][H/8][W/8] of the padded size or NULL.
 * flow_out [iters][batch][2][in_h][in_w]: every iteration's convex-upsampled, unpadded flow.
 * Replaces: ERAFT.forward(events1, events2, iters, flow_init)[1]  (model/eraft.py:97-159). */
int eraft_forward(eraft_ctx* ctx, const float* events1, const float* events2, int batch, int in_h, int in_w,
                  const int pad[4], int iters, const float* flow_init, float* flow_out, void* stream);

/* n (1..16) independent batch-1 samples, each in its own tensors (events1[i] / events2[i] [1][C][in_h][in_w]; flow_out[i]
 * [iters][1][2][in_h][in_w], or [1][1][2][in_h][in_w] after eraft_set_final_only), as ONE batch-n forward - bitwise what eraft_forward
 * returns for the samples stacked into a batch (flow_init: none).
 * Replaces: n iterations of the evaluation loop at batch 1 (test_mvsec.py:580-597 -> run_network, :1444-1455) for ERAFT. */
int eraft_forward_many(eraft_ctx* ctx, int n, const float* const* events1, const float* const* events2, int in_h, int in_w,
                       const int pad[4], int iters, float* const* flow_out, void* stream);

/* Intermediates of the LAST forward: "fmap" ([2B,256,h,w]: fmap1 then fmap2), "inp", "flow_low", "pyr0".."pyr3", and - only
 * after eraft_keep_stages(ctx, 1), which adds four device copies to every forward - "corr0" (first lookup), "net1", "mask1",
 * "delta1" (after the first update). */
int eraft_keep_stages(eraft_ctx* ctx, int enable);

/* Stage recorder, for tests that hold every launch of eraft_forward / eraft_forward_many to a reference of that one launch (off by
 * default; eraft_forward_stream records nothing).  prefixes: comma-separated name prefixes ("fnet.,pyr,it0.corr"; "" = everything),
 * NULL = off.  While on, the forward enqueues - behind every launch whose name starts with one of them, on the stream that launch ran
 * on - a device copy of that launch's output, filed under the name with the kernel form that wrote it; it launches no kernel
 * differently, and its predictions are bit for bit those of the forward with the recorder off.  Update iterations 0 .. iterations - 1
 * are recorded.  The copies live in one arena sized by the forward before: a forward whose records do not fit is run a second time.
 * Names:  "pad";  "<net>.conv1", "<net>.norm1", "<net>.layer<1..3>.<0|1>.conv1 | norm1 | conv2 | norm2 | down | norm3" for <net> =
 * "fnet" (convs without activation, every InstanceNorm) and "cnet" (convs with the eval BatchNorm, ReLU and residual folded in; no norm
 * entries);  "fmap", "net0", "inp", "czr0", "czr1", "cq0", "cq1" (the context features' share of the GRU convs);  "pyr0".."pyr3", or
 * "f2l1".."f2l3" (pooled fmap2) with eraft_set_alternate_corr;  per iteration K "itK.coords1_in", "itK.corr", "itK.flow", "itK.flo1",
 * "itK.cor1", "itK.corflo.c" (channels 0..191) and "itK.corflo.f" (192..255), "itK.motion" (channels 0..125), "itK.gru<0|1>.z",
 * ".r" (only where r itself is stored: EEM_ERAFT_NO_ZR=1), ".rh", ".h", "itK.fhid", "itK.delta", "itK.coords1_out", "itK.mhid",
 * "itK.mask", "itK.pred".  eraft_corr_lookup records "pyr0".."pyr3" and "corr".  eraft_get_stage serves the recorded names (after its
 * own); eraft_stage_list writes one line "name form n c h w" per record of the last call ("-": no form), *need = the bytes it takes
 * (buf NULL: only that). */
int eraft_record_stages(eraft_ctx* ctx, const char* prefixes, int iterations);
int eraft_stage_list(eraft_ctx* ctx, char* buf, size_t capacity, size_t* need);
/* The kernel form of this thread's last E-RAFT helper launch (padding, instance norm, all-pairs, pooling, lookup, convex upsampling,
 * ...), as eemop_last_conv_form names the convolutions': what the operator-level calls that make one such launch ran. */
int eraft_last_form(char* buf, int capacity);

/* Correlation features computed on the fly instead of from an all-pairs volume (1: on, 0 = default: the volume stays resident).
 * Replaces the `alt_cuda_corr` pattern of model/flowformer/corr.py:60-91 (RAFT's `alternate_corr`): the 81 taps of a
 * pixel at level l are bilinear samples of <fmap1[:, p], avg_pool2d^l(fmap2)[:, q]> / sqrt(C) over the 10 x 10 cells its window
 * touches - no B * (HW)^2 * 4/3 floats (829 MB per sample at 1280x720), ~250x the lookup's memory traffic per iteration.  Same
 * features up to summation order; eraft_get_stage("pyr<l>") is not available in this mode. */
int eraft_set_alternate_corr(eraft_ctx* ctx, int enable);

/* 1: eraft_forward writes ONE prediction, flow_out [1][batch][2][in_h][in_w] = the last entry of the reference's list - what the
 * evaluation loop reads (test_mvsec.py:1455 `batch['flow_list'][-1]`).  The mask head and the convex upsampling of iterations
 * 0 .. iters - 2 are not launched (their results feed nothing else: model/eraft.py:141-157); the hidden state, coords1 and the last
 * prediction are bit for bit those of the full forward.  0 = default: every iteration's prediction, as ERAFT.forward returns them. */
int eraft_set_final_only(eraft_ctx* ctx, int enable);

/* Throughput hint, as eemflow_set_frames_in_flight: the application keeps `n` E-RAFT forwards in flight on this GPU (one context
 * and HIP stream each).  With n >= 3 the 16-aligned stride-1 convs use 4-row tiles from 512 blocks on (2 048 otherwise): the
 * other frames fill the CUs a short launch leaves idle, and each weight fragment is read half as often (640x480, 12 iterations,
 * batch 4, three in flight: 168 -> 175 frames/s; one forward at a time would lose 4 %).  Default 1. */
int eraft_set_frames_in_flight(eraft_ctx* ctx, int n);
int eraft_get_stage(eraft_ctx* ctx, const char* name, float* dst, size_t dst_capacity_floats, int dims_out[4],
                    void* stream);

/* CorrBlock(fmap1, fmap2, num_levels=4, radius=4)(coords): fmaps [batch][c][h][w], coords [batch][2][h][w]
 * -> out [batch][324][h][w].  Replaces: model/corr.py:13-60 (+ model/model_utils.py:7-21). */
int eraft_corr_lookup(eraft_ctx* ctx, const float* fmap1, const float* fmap2, const float* coords, int batch, int c,
                      int h, int w, float* out, void* stream);

/* Adjoint of eraft_corr_lookup w.r.t. the correlation pyramid (the reference detaches coords every iteration,
 * model/eraft.py:141, so there is no coordinate gradient): dout [batch][324][h][w] -> dpyr_l [batch*h*w][h>>l][w>>l],
 * l = 0..3 (zeroed here, then scatter-added).  Replaces: autograd of CorrBlock.__call__  (model/corr.py:29-50). */
int eraft_corr_lookup_bwd(const float* coords, const float* dout, int batch, int h, int w, float* dpyr0, float* dpyr1,
                          float* dpyr2, float* dpyr3, void* stream);

/* Adjoint of the pyramid construction: folds dpyr3 -> dpyr2 -> dpyr1 -> dpyr0 through the avg_pool2d chain (in place:
 * dpyr0..2 are modified) and returns d fmap1, d fmap2 [batch][c][h][w] of corr = fmap1^T fmap2 / sqrt(c).  h*w % 4 == 0.
 * Replaces: autograd of CorrBlock.__init__ / CorrBlock.corr  (model/corr.py:13-27,53-60). */
int eraft_corr_pyramid_bwd(const float* fmap1, const float* fmap2, float* dpyr0, float* dpyr1, float* dpyr2, const float* dpyr3,
                           int batch, int c, int h, int w, float* dfmap1, float* dfmap2, void* stream);

/* Adjoint of eraft_convex_upsample: dout [batch][2][8h][8w] -> dflow [batch][2][h][w], dmask [batch][576][h][w].
 * Replaces: autograd of ERAFT.upsample_flow  (model/eraft.py:83-94). */
int eraft_convex_upsample_bwd(const float* flow, const float* mask, const float* dout, int batch, int h, int w, float* dflow,
                              float* dmask, void* stream);

/* Convex upsampling: flow [batch][2][h][w], mask [batch][576][h][w] -> out [batch][2][8h][8w].
 * Replaces: ERAFT.upsample_flow  (model/eraft.py:83-94). */
int eraft_convex_upsample(eraft_ctx* ctx, const float* flow, const float* mask, int batch, int h, int w, float* out,
                          void* stream);

/* Forward interpolation of a low-resolution flow, E-RAFT's warm start: flow [batch][2][h][w] -> out [batch][2][h][w] (out must not
 * alias flow).  Bit for bit the reference function on the CPU at one thread: each cell adds its four-pass contributions (floor / ceil
 * landing cells in the reference's order) in source order in fp32 and divides by the weight sum + 1e-15f; cells no source reaches are
 * 0.  `scratch` is device memory of at least eraft_forward_interpolate_scratch(batch, h, w) ints (3 h w + (h + 1)(w + 1) per sample).
 * One workgroup per sample.
 * Replaces: forward_interpolate_pytorch (utils/image_utils.py:53-84, with grid_sample_values :11-51). */
int eraft_forward_interpolate(const float* flow, float* out, int batch, int h, int w, int* scratch, size_t scratch_ints, void* stream);
size_t eraft_forward_interpolate_scratch(int batch, int h, int w);

/* Windows per eraft_forward_stream call. */
#define ERAFT_STREAM_MAX_VOLUMES 16

/* E-RAFT along a stream of CONSECUTIVE event windows, each window through the feature network once.  volumes[j] (j < nvol,
 * 1..ERAFT_STREAM_MAX_VOLUMES) are [1][C][in_h][in_w] windows in time order (a HOST array of device pointers); pair p is (window
 * p - 1, window p), window -1 being the one carried from the previous call: nflow == nvol with a carried window, nvol - 1 without
 * (flow_out may then be NULL for nvol == 1).  flow_out[p] is [iters][1][2][in_h][in_w], or [1][1][2][in_h][in_w] after
 * eraft_set_final_only, as in eraft_forward_many.  The feature network runs once over the nvol new windows; the context network over
 * each pair's first window (model/eraft.py:126); the correlation volumes of all pairs come from one buffer of feature maps.
 * warm_start = 0: one batch-nflow update loop, bitwise eraft_forward_many on the same pairs in the same kernel forms (the feature network
 * runs nvol images here, 2 nflow there).  warm_start = 1 (E-RAFT's sequential mode): pair p starts from coords0 +
 * eraft_forward_interpolate(flow_low of pair p - 1) (model/eraft.py:134-137), pair -1 being the previous call's last pair; the first
 * pair after eraft_stream_reset starts cold.  The pairs' loops then run one after another at batch 1, the interpolation between them
 * on the device.  Afterwards the context carries the last window's feature map and padded volume and the last pair's flow_low, in
 * memory that eraft_forward / eraft_forward_many / eraft_get_stage and the operator-level calls leave alone.  A call with other weights
 * (eraft_load_weights) or another size or pad than the carry's is refused with an error: call eraft_stream_reset.
 * eraft_get_stage("flow_low") afterwards is [nflow][2][h/8][w/8]: every pair's low-resolution flow.  eraft_set_alternate_corr(1) is
 * refused: the stream needs the all-pairs volume.  eraft_keep_stages does not apply.
 * Replaces: the evaluation loop over consecutive samples at stride 1 (test_mvsec.py:580-597), which runs ERAFT.forward's feature
 * network (model/eraft.py:116) on every window twice; with warm_start, that loop with flow_init = forward_interpolate_pytorch(the
 * previous pair's coords1 - coords0), which model/eraft.py:48-49,125-128 leaves commented out. */
int eraft_forward_stream(eraft_ctx* ctx, int nvol, const float* const* volumes, int in_h, int in_w, const int pad[4], int iters,
                         int warm_start, float* const* flow_out, int nflow, void* stream);

/* Drop the carried window and flow: the next eraft_forward_stream call starts a new stream (cold).
 * Replaces: the start of a sequence in test_mvsec.py:580-597 (dataset.change_test_sequence). */
int eraft_stream_reset(eraft_ctx* ctx);

/* *out = 1 when a window is carried for the next eraft_forward_stream call, else 0.
 * Replaces: nothing in the reference (it has no stream state); the query behind ERAFT.forward_stream's bookkeeping. */
int eraft_stream_pending(eraft_ctx* ctx, int* out);

/* ------------------------------------------------------------------------------------------------
 * EEMFlow+ (EEMFlow_cdc, model/EEMFlow/EEMFlow+.py + cdc_utils.py): the coarse-to-fine bilinear flow-warp loop.
 * ---------------------------------------------------------------------------------------------- */

/* Replaces: EEMFlow_cdc.__init__ + .to(device)  (model/EEMFlow/EEMFlow+.py:75-135). */
int eemplus_create(int device, eemplus_ctx** out);
void eemplus_destroy(eemplus_ctx* ctx);

/* The 136 tensors of the reference state_dict() back to back in registration order (the parameters the
 * reference registers but never uses - up3..up6, cdc_model.upsample_output_conv - are present and skipped).
 * Replaces: load_state_dict of EEMFlow_cdc. */
int eemplus_load_weights(eemplus_ctx* ctx, const float* flat_host, size_t nfloats, int n_first_channels, int groups);

/* events1/2 [batch][C][in_h][in_w], pad = [left, right, top, bottom] of InputPadder(img_size, 'chairs', 64);
 * flow_out [5][batch][2][in_h][in_w]: the predictions of levels 6, 5, 4, 3, 2 at full resolution.
 * Replaces: EEMFlow_cdc.forward(events1, events2)[1]  (model/EEMFlow/EEMFlow+.py:158-234). */
int eemplus_forward(eemplus_ctx* ctx, const float* events1, const float* events2, int batch, int in_h, int in_w,
                    const int pad[4], float* flow_out, void* stream);

/* n (1..16) independent batch-1 samples, each in its own tensors (events1[i] / events2[i] [1][C][in_h][in_w], flow_out[i]
 * [5][1][2][in_h][in_w]), as ONE batch-n chain of launches - bitwise what eemplus_forward returns for the samples stacked into a batch.
 * Replaces: n iterations of the evaluation loop at batch 1 (test_mvsec.py:580-597 -> run_network, :1444-1455) for EEMFlow_cdc. */
int eemplus_forward_many(eemplus_ctx* ctx, int n, const float* const* events1, const float* const* events2, int in_h, int in_w,
                         const int pad[4], float* const* flow_out, void* stream);

/* EEMFlow+ along a stream of CONSECUTIVE event windows, each window padded and encoded once.  volumes[j] (j < n,
 * 1..EEM_STREAM_MAX_VOLUMES) are [1][C][in_h][in_w] windows in time order (a HOST array of device pointers); pair p is (window p - 1,
 * window p), window -1 being the one carried from the previous call: nflow == n with a carried window, n - 1 without (flow_out may then
 * be NULL for n == 1: the window is encoded and carried, no flow is formed).  Any other nflow is an error.  flow_out[p] is
 * [5][1][2][in_h][in_w] - flow6 .. flow2 at full resolution, as in eemplus_forward_many.  The encoder and the three poolings run over the n
 * new windows; pair p's feature_1 is image p of the pyramid and its feature_2 image p + 1.  Pair p is bitwise eemplus_forward_many on the
 * same pairs in one call, once the kernel forms that follow the encoder's image count (n here, 2 nflow there) are pinned.  Afterwards the
 * context carries the last window's pyramid levels 2..6 in memory that eemplus_forward / eemplus_forward_many leave alone; the next call
 * moves it to image 0 with one launch.  A carry made with other weights (eemplus_load_weights) or at another size or pad is refused with
 * an error: call eemplus_stream_reset.  eemplus_get_stage (batch nflow) and eemplus_level read the last call's pyramid, stream or not.
 * Replaces: the evaluation loop over consecutive samples at stride 1 (test_mvsec.py:580-597, samples built by loader/MVSEC.py:115-116
 * from windows i and i + 1), which runs EEMFlow_cdc.forward's encoder (model/EEMFlow/EEMFlow+.py:162-175) on every window twice. */
int eemplus_forward_stream(eemplus_ctx* ctx, int n, const float* const* volumes, int in_h, int in_w, const int pad[4],
                           float* const* flow_out, int nflow, void* stream);

/* Drop the carried window: the next eemplus_forward_stream call starts a new stream.
 * Replaces: the start of a sequence in test_mvsec.py:580-597 (dataset.change_test_sequence). */
int eemplus_stream_reset(eemplus_ctx* ctx);

/* *out = 1 when a window is carried for the next eemplus_forward_stream call, else 0.
 * Replaces: nothing in the reference (it has no stream state); the query behind EEMFlow_cdc.forward_stream's bookkeeping. */
int eemplus_stream_pending(eemplus_ctx* ctx, int* out);

/* Intermediates of the LAST forward: "flow2".."flow6" (low-resolution level flows, incl. the in-place doubling
 * the reference applies to flow3..flow6), "flow_up2".."flow_up5" and "flow_init2".."flow_init5" (cdc_model's upsampled
 * input flow of each level); after them, every name the stage recorder filed in the last call (eemplus_record_stages). */
int eemplus_get_stage(eemplus_ctx* ctx, const char* name, float* dst, size_t dst_capacity_floats, int dims_out[4],
                      void* stream);

/* Stage recorder, for tests that hold every launch of eemplus_forward / eemplus_forward_many / eemplus_level to a reference of that one
 * launch (off by default; eemplus_forward_stream records nothing - its flows are bitwise eemplus_forward_many's).  prefixes:
 * comma-separated name prefixes ("pad,enc,l2."; "" = everything), NULL = off.  While on, the call enqueues - behind every launch whose
 * name starts with one of them, on the stream that launch ran on (the side stream under EEM_PLUS_SIDE=1 included) - a device copy of that
 * launch's output, filed under the name with the kernel form that wrote it; it launches no kernel differently, and the predictions are
 * bit for bit those of the call with the recorder off.  The copies live in one arena sized by the forward before: a forward whose
 * records do not fit is run a second time.  A copy is taken where a later launch overwrites the buffer (the encoder's two scratch
 * buffers, the coarse flow that the next level doubles, a level's decoder input), so it is what the consuming launch read.
 * Names:  "pad";  "enc0".."enc7" (the encoder's layers; enc4 and enc7 are pyramid levels 2 and 3);  "pool4".."pool6" (levels 4..6);
 * per level K = 6..2 "lK.a1", "lK.a2" (the 1x1 projections of feature_1 / feature_2), "lK.rconv", "lK.flow_init", "lK.coarse_scaled"
 * (level K + 1's flow after the doubling, [B][2][h_{K+1}][w_{K+1}]), "lK.warp_a2", "lK.de0".."lK.de4", "lK.xout", "lK.tw" (the mode-1
 * warp of flow_init, EEM_PLUS_NO_FUSE=1 only), "lK.flow_up", "lK.fw", "lK.corr", "lK.cat_flow" (channels 85..86 of the decoder's
 * input), "lK.dec1", "lK.decg0".."lK.decg2", "lK.dec5", "lK.dec6", "lK.flow" (level 6: corr, cat_flow, rconv and the decoder);
 * "pred" [5 * B][2][H][W] (eemplus_forward_many: "pred<sample>" [5][2][H][W]).  A launch of two jobs that writes two buffers files two
 * stages with the same form.  eemplus_level records the one level it runs.  eemplus_stage_list writes one line "name form n c h w" per
 * record of the last call ("-": no launch wrote it - a device copy), *need = the bytes it takes (buf NULL: only that). */
int eemplus_record_stages(eemplus_ctx* ctx, const char* prefixes);
int eemplus_stage_list(eemplus_ctx* ctx, char* buf, size_t capacity, size_t* need);
/* The kernel form of this thread's last launch by tail_conv_launch ("tail_k<1|3>_g<groups>_j<jobs>", "tail_multi_j<jobs>"), wnc_launch
 * ("wnc32", "wnc64", "..._m16"), enc_conv_launch ("enc1", "enc_c<cin>_<cout>_s<stride>", "wino", "enc2", ...), corr_launch ("corr_direct",
 * "corr_tiled53") or a launch of plus_kernels.hip ("warp", "upflow", "upflow_multi", "upflow_warp", "scale_flow", "blend", "warp_blend",
 * "warp_blend_warp", "copy_channels"): what eemplus_warp / eemplus_upsample_flow_as ran. */
int eemplus_last_form(char* buf, int capacity);

/* Teacher-forced level: level l (5..2) of the coarse-to-fine loop, re-run on the feature pyramid of the LAST eemplus_forward
 * from a caller-supplied flow_init [batch][2][h_l][w_l] - cdc_model's upsampled input flow, the value the discontinuous
 * `grid_sample(ones) >= 1` mask of WarpingLayer_no_div is computed from.  flow_up_out / flow_out [batch][2][h_l][w_l] (either
 * may be NULL) receive flow_up_l (cdc_model's output) and flow_l (decoder_l + flow_up_l).  Pins every level to the flow
 * tolerance separately; the chained forward can only be compared statistically past the first mask.
 * Replaces: one l-block of EEMFlow_cdc.forward  (model/EEMFlow/EEMFlow+.py:183-229, cdc_utils.py:156-174). */
int eemplus_level(eemplus_ctx* ctx, int level, const float* flow_init, float* flow_up_out, float* flow_out, void* stream);

/* Throughput hint, as eraft_set_frames_in_flight (4-row tiles of the LDS-tiled convs from 512 blocks on): EEMFlow+ 1280x720 with
 * four frames in flight 579 -> 595 frames/s.  Default 1. */
int eemplus_set_frames_in_flight(eemplus_ctx* ctx, int n);

/* Backward bilinear warp of x [batch][c][h][w] by flow [batch][2][h][w].  mode 0: EEMFlow_cdc.warp
 * (EEMFlow+.py:137-149, align_corners=True); 1: tensor_tools.torch_warp (utils_luo/tools.py:2262-2306,
 * align_corners=False); 2: WarpingLayer_no_div (cdc_utils.py:50-78, align_corners=False and the
 * grid_sample(ones) >= 1 mask). */
int eemplus_warp(const float* x, const float* flow, int batch, int c, int h, int w, int mode, float* out, void* stream);

/* Adjoint of eemplus_warp: dout [batch][c][h][w] -> dx [batch][c][h][w] (zeroed here, scatter-added), dflow [batch][2][h][w].
 * The `>= 1` mask of mode 2 carries no gradient, as in the reference.  Replaces: autograd of F.grid_sample in the three
 * warps (EEMFlow+.py:137-149, cdc_utils.py:50-78, utils_luo/tools.py:2262-2306). */
int eemplus_warp_bwd(const float* x, const float* flow, const float* dout, int batch, int c, int h, int w, int mode, float* dx,
                     float* dflow, void* stream);

/* upsample2d_flow_as(inputs, target, 'bilinear', if_rate)  (cdc_utils.py:80-103): out [batch][2][oh][ow];
 * with if_rate != 0 `inputs` is scaled in place afterwards, as the reference does. */
int eemplus_upsample_flow_as(float* inputs, int batch, int h, int w, int oh, int ow, int if_rate, float* out,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Operator-level entry points (eemop_*): the differentiable building blocks of the E-RAFT training graph - what
 * torch.autograd records when train_mvsec.py:245-258 runs model(im1, im2) -> sequence_loss -> backward on model/eraft.py with the
 * module in train() (train-mode BatchNorm in cnet, model/extractor.py:31-35; SepConvGRU / motion encoder / heads of
 * model/update.py:6-106 unrolled 12 times).  All tensors are caller-owned dense NCHW fp32 on the current device;
 * eemflow_amd/ops.py wraps each pair as a torch.autograd.Function.
 * ---------------------------------------------------------------------------------------------- */

/* Packed-weight cache of the convolution operators below.  The kernels read weights in their own packed order; without a hint every
 * call repacks `w` (one small launch).  eemop_pack_hint names the weight tensor of the NEXT conv calls of this thread: `token` is an
 * identity the caller never reuses for another tensor (0 = no caching), `version` the tensor's modification counter (torch's
 * `Tensor._version`); a packing is redone only when (token, w pointer, stream) is new or the version differs - a recurrent model that
 * applies one set of weights twelve times per step (model/eraft.py:141-157) packs them once per step and once more for the data
 * gradients.  eemop_pack_forget frees what a token holds.  No counterpart in the reference: ATen's conv reads the weights in place. */
int eemop_pack_hint(long long token, long long version);
int eemop_pack_forget(long long token);
long long eemop_pack_cache_bytes(void);   /* device bytes the cache holds (all tokens, this process) */
/* conv2d of up to three channel-concatenated inputs (the torch.cat of model/update.py:44,51,79 is never materialised):
 * x_s [n][c_s][hin][win] (x1 / x2 may be NULL), w [cout][c0+c1+c2][kh][kw], bias [cout] or NULL; act 0 none, 1 ReLU, 2 sigmoid,
 * 3 tanh; out[n][out_coff + co][hout][wout] of an out_ctotal-channel tensor = out_scale * act(conv + bias).
 * Replaces: nn.Conv2d.forward (+ the activation that follows it) in model/extractor.py, model/update.py. */
int eemop_conv2d_fwd(const float* x0, int c0, const float* x1, int c1, const float* x2, int c2, const float* w, const float* bias,
                     int n, int hin, int win, int cout, int kh, int kw, int stride, int ph, int pw, int act, float out_scale, float* out,
                     int out_ctotal, int out_coff, void* stream);
/* d loss / d x for the input-channel slice [ci0, ci0 + cic) of a conv with cin input channels: dx [n][cic][hin][win] from
 * dy [n][cout][hout][wout] (the gradient w.r.t. the conv's output BEFORE its activation).  stride 1 or 2.
 * Replaces: autograd of nn.Conv2d w.r.t. its input. */
int eemop_conv2d_bwd_data(const float* dy, const float* w, int n, int hin, int win, int cin, int ci0, int cic, int cout, int kh, int kw,
                          int stride, int ph, int pw, float* dx, void* stream);
/* dw [cout][cin][kh][kw] (slice [ci0, ci0 + cic) of the input channels) += dy (x) x, db [cout] += sum dy (db may be NULL); x is
 * that slice's input [n][cic][hin][win].  Accumulating: the caller zeroes dw / db.  Kernel shapes built: 3x3, 1x1 (stride 1, 2),
 * 1x5, 5x1, 7x7 (stride 1, 2; at most 32 input channels).  Replaces: autograd of nn.Conv2d w.r.t. weight and bias. */
int eemop_conv2d_bwd_weight(const float* x, const float* dy, int n, int hin, int win, int cin, int ci0, int cic, int cout, int kh, int kw,
                            int stride, int ph, int pw, float* dw, float* db, void* stream);
/* The same for a conv over up to three channel-concatenated inputs in ONE call (x_s [n][c_s][hin][win]; x1 / x2 may be NULL):
 * dw [cout][c0 + c1 + c2][kh][kw] += dy (x) cat(x0, x1, x2), db [cout] += sum dy when not NULL.  The segments ride one launch where that
 * is the faster form (the GRU's (1, 5) / (5, 1) convs over [h | inp | motion]), one launch per segment elsewhere.
 * Replaces: autograd of nn.Conv2d w.r.t. its weight and bias for the convs of model/update.py:33-60,63-81 whose input is a torch.cat. */
int eemop_conv2d_bwd_weight_cat(const float* x0, int c0, const float* x1, int c1, const float* x2, int c2, const float* dy, int n, int hin,
                                int win, int cout, int kh, int kw, int stride, int ph, int pw, float* dw, float* db, void* stream);
/* TEST OBSERVABLE: the name of the kernel instantiation that the calling thread's most recent eemop_conv2d_* call launched, e.g.
 * "gconv16_3x3_th3_wm4_kg1" (filter, tile rows, 16-cout tiles per block, K groups), "gconvb_1x5_th6", "generic_splitk8",
 * "fewout_k8_c4", "stem7_c5", "dgrad_s2w_128_3x3", "wgrad_enc_bx3_tw16_c32_s2", "wgrad_generic_7x7_s2_bias"; a weight gradient served by
 * one launch per input segment reports the segments' names joined with '+'.  A host-side pointer store per launch; "" before any. */
int eemop_last_conv_form(char* buf, int cap);
/* TEST OBSERVABLE: the same for the non-convolution operators - the kernel (and launch form) that the calling thread's most recent
 * eemop_* call of that kind, or eraft_corr_lookup_bwd / eraft_corr_pyramid_bwd / eraft_convex_upsample_bwd / eemplus_warp_bwd, launched:
 * "instnorm_bwd_t256" / "_t1024", "bn_train_fwd_t256", ..., "lookup_bwd_rows" / "lookup_bwd_scatter", "allpairs_bwd", "convex_up_bwd",
 * "warp_bwd_m0..2", "resize_ac", "resize_ac_bwd_gather" / "_scatter", "pool2_bwd", "act_fwd", "act_bwd", "binary", "sum_n_v4" /
 * "sum_n_scalar", "gru_blend", "gru_blend_bwd", "copy_channels", "shuffle", "scale_flow".  A call that launches nothing (zero elements,
 * refused arguments) leaves it as it was; the entry points that forward to an er_* launcher report through eraft_last_form. */
int eemop_last_op_form(char* buf, int cap);
/* out = scale * dy * act'(y) for y = act(pre): kind 1 ReLU, 2 sigmoid, 3 tanh, 0 identity.  Replaces: autograd of F.relu /
 * torch.sigmoid / torch.tanh (model/update.py:14,45-47,54-56,74-79,95; model/eraft.py:130-131) and of the 0.25 mask scale (:105). */
int eemop_act_bwd(const float* dy, const float* y, long long n, int kind, float scale, float* out, void* stream);
/* out = a + b (kind 0), a - b (1), a * b (2), relu(a + b) (3), alpha * a (4; b unused).  Replaces: coords1 - coords0, coords1 +
 * delta_flow (model/eraft.py:144,149), r * h (model/update.py:47,56), relu(x + y) (model/extractor.py:57). */
int eemop_binary(int kind, const float* a, const float* b, float alpha, long long n, float* out, void* stream);
/* out = in[0] + ... + in[count - 1] (1 <= count <= 8, host array of device pointers), one launch.  Replaces: the chain of adds autograd
 * runs when a tensor has several consumers - the hidden state, the context features, the motion features and the correlation pyramid
 * across the twelve unrolled iterations (model/eraft.py:139-157, model/update.py:43-60); Python: ops.FanOut. */
int eemop_sum_n(const float* const* in, int count, long long n, float* out, void* stream);
/* h' = (1 - z) h + z q and its adjoint (dz = dout (q - h), dh = dout (1 - z), dq = dout z).  Replaces: model/update.py:48,57. */
int eemop_gru_blend(const float* z, const float* h, const float* q, long long n, float* out, void* stream);
int eemop_gru_blend_bwd(const float* dout, const float* z, const float* h, const float* q, long long n, float* dz, float* dh, float* dq,
                        void* stream);
/* dst[n][dst_coff + c] = src[n][src_coff + c], c < cc: torch.cat([out, flow], dim=1) (model/update.py:81) and its split. */
int eemop_copy_channels(const float* src, int src_ctotal, int src_coff, float* dst, int dst_ctotal, int dst_coff, int cc, int n, int hw,
                        void* stream);
/* coords0 = coords1 = pixel grid [batch][2][h][w] (channel 0 = x, 1 = y), coords1 += flow_init when given.
 * Replaces: ERAFT.initialize_flow + the flow_init add  (model/eraft.py:73-81,136-137). */
int eemop_coords_init(float* coords0, float* coords1, const float* flow_init, int batch, int h, int w, void* stream);
/* F.pad(mode='replicate') of [nc][h][w]  (InputPadder.pad, utils/image_utils.py:139-140). */
int eemop_replicate_pad(const float* in, float* out, int nc, int h, int w, int left, int right, int top, int bottom, void* stream);
/* InstanceNorm2d(affine=False, eps 1e-5) over `planes` (n, c) planes of hw pixels: out = relu?(IN(x)) or relu(IN(x) + res) when res
 * is given; backward (x = the norm's input, y = its output) for the no-residual forms.
 * Replaces: nn.InstanceNorm2d (+ ReLU) of fnet, model/extractor.py:31-35,43-57, and its autograd. */
int eemop_instnorm_fwd(const float* x, const float* res, int planes, int hw, int relu, float* out, void* stream);
int eemop_instnorm_bwd(const float* x, const float* y, const float* dy, int planes, int hw, int relu, float* dx, void* stream);
/* BatchNorm2d in TRAINING mode: batch mean / biased variance over (n, hw) per channel, y = relu?((x - mean) rstd w + b); the running
 * statistics are updated IN PLACE (momentum, unbiased variance) and save_mean / save_rstd [c] kept for the backward, which returns
 * dx, dweight [c], dbias [c].  Replaces: nn.BatchNorm2d.forward in train() of cnet (model/extractor.py:31-35,123-133;
 * train_mvsec.py:231-235 leaves BatchNorm unfrozen) and its autograd. */
int eemop_batchnorm_train_fwd(const float* x, const float* weight, const float* bias, float* running_mean, float* running_var, int n,
                              int c, int hw, float momentum, float eps, int relu, float* y, float* save_mean, float* save_rstd,
                              void* stream);
int eemop_batchnorm_train_bwd(const float* x, const float* y, const float* dy, const float* weight, const float* save_mean,
                              const float* save_rstd, int n, int c, int hw, int relu, float* dx, float* dweight, float* dbias, void* stream);
/* BatchNorm2d in EVAL mode - frozen running statistics, an affine map per channel: y = relu?((x - running_mean) rstd w + b) with
 * rstd = 1 / sqrt(running_var + eps); backward returns dx = g w rstd, dweight [c] = sum g (x - running_mean) rstd, dbias [c] = sum g
 * (g = dy gated by the ReLU).  Replaces: nn.BatchNorm2d.forward in eval() after ERAFT.freeze_bn (model/eraft.py:69-72) and its autograd. */
int eemop_batchnorm_eval_fwd(const float* x, const float* weight, const float* bias, const float* running_mean, const float* running_var,
                             int n, int c, int hw, float eps, int relu, float* y, void* stream);
int eemop_batchnorm_eval_bwd(const float* x, const float* y, const float* dy, const float* weight, const float* running_mean,
                             const float* running_var, int n, int c, int hw, float eps, int relu, float* dx, float* dweight, float* dbias,
                             void* stream);
/* CorrBlock on caller tensors: the pyramid pyr_l [batch*h*w][h >> l][w >> l] (adjoint: eraft_corr_pyramid_bwd) and the 4-level 9x9
 * lookup at `coords` [batch][2][h][w] -> out [batch][324][h][w] (adjoint: eraft_corr_lookup_bwd).  model/corr.py:13-60. */
int eemop_corr_pyramid_fwd(const float* fmap1, const float* fmap2, int batch, int c, int h, int w, float* pyr0, float* pyr1, float* pyr2,
                           float* pyr3, void* stream);
int eemop_corr_lookup_fwd(const float* pyr0, const float* pyr1, const float* pyr2, const float* pyr3, const float* coords, int batch, int h,
                          int w, float* out, void* stream);
/* ERAFT.upsample_flow on caller tensors: flow [batch][2][h][w], mask [batch][576][h][w] -> out [batch][2][8h][8w]; `zeros` is an
 * all-zero [batch][2][h][w] tensor (adjoint: eraft_convex_upsample_bwd).  model/eraft.py:83-94. */
int eemop_convex_upsample_fwd(const float* zeros, const float* flow, const float* mask, int batch, int h, int w, float* out, void* stream);

/* ---- further operators of the EEMFlow+ autograd graph (model/EEMFlow/EEMFlow+.py:158-234, cdc_utils.py:50-177) */
/* out = act(x): 1 ReLU, 2 sigmoid, 3 tanh, 4 LeakyReLU(0.1)  (torch.sigmoid of the upsampler's mask, cdc_utils.py:166). */
int eemop_act_fwd(const float* x, long long n, int kind, float* out, void* stream);
/* channel_shuffle (EEMFlow+.py:52-58) of [n][c][hw] and its inverse (= its adjoint). */
int eemop_shuffle_channels(const float* src, float* dst, int n, int c, int groups, int hw, int inverse, void* stream);
/* out[:, 0] = su * x[:, 0], out[:, 1] = sv * x[:, 1] of a flow [n][2][hw]: the rate of upsample2d_flow_as (cdc_utils.py:85-93);
 * its own adjoint. */
int eemop_scale_flow(const float* x, int n, int hw, float su, float sv, float* out, void* stream);
/* F.avg_pool2d(2, 2) over the last two dims of [planes][h][w] and its adjoint  (EEMFlow+.py:170-175). */
int eemop_pool2_fwd(const float* x, float* out, long long planes, int h, int w, void* stream);
int eemop_pool2_bwd(const float* dy, float* dx, long long planes, int h, int w, void* stream);
/* F.interpolate(mode='bilinear', align_corners=True) of [nc][h][w] -> [nc][oh][ow] and its adjoint  (cdc_utils.py:83). */
int eemop_resize_ac_fwd(const float* in, float* out, int nc, int h, int w, int oh, int ow, void* stream);
int eemop_resize_ac_bwd(const float* dout, float* dx, int nc, int h, int w, int oh, int ow, void* stream);
/* adjoint of eemflow_local_corr53: dcv [batch][53][h][w] -> df1, df2 [batch][c][h][w]. */
int eemop_local_corr53_bwd(const float* dcv, const float* f1, const float* f2, int batch, int c, int h, int w, float* df1, float* df2,
                           void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* EEMFLOW_HIP_H */
