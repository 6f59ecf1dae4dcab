// The EEMFlow context and what api.hip (inference C ABI), train_api.hip (training step), workspace.hip (workspace management) and
// schedule.hip (the forward schedule) share.  Declarations only: every function here is defined once, in the file its section names;
// the bodies in this header are the context's trivial inline members and the Hook::run template.
#pragma once
#include <stdarg.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/eemflow_hip.h"
#include "common.h"
#include "gconv.h"
#include "eraft_kernels.h"
#include "wnc.h"

// ------------------------------------------------------------------------------- context
constexpr int kNTaps = 53;            // (kTaps53: devstate.h)
constexpr int kDecIn = kNTaps + 16;   // 69
constexpr int kDecW = 100;

struct TailW {                         // one packed small-grid conv
    size_t wpk = 0, bias = 0;          // float offsets into the weight arena
    int cin = 0, cout = 0, ksize = 3;
};

struct Shape {
    int batch = 0, in_h = 0, in_w = 0, out_h = 0, out_w = 0;
    int hp = 0, wp = 0;                // padded extent
    int h1 = 0, w1 = 0, h2 = 0, w2 = 0, h3 = 0, w3 = 0;
    int gh = 0, gw = 0;                // 1/64 grid
    // fused stage pooling (fast path): partial-sum buffer dims per stage, fuse[k] = conv epilogue pools stage k
    bool fuse[3] = {false, false, false};
    int prow[3] = {0, 0, 0}, pcol[3] = {0, 0, 0}, th[3] = {0, 0, 0};
    // the encoder's batch: nimg images, the first nimg0 of them from events1; enc_batch is the sample count its per-batch policies see
    // (f4_mask, the block walks).  A forward: 2 * batch, batch, batch.  A stream call (eemflow_forward_stream): the nvol new windows,
    // all from the per-frame table, and nvol / 2 - the sample count whose forward encodes as many images
    int nimg = 0, nimg0 = 0, enc_batch = 0;
    // stream call: `batch` pairs of consecutive windows; carry_in: pair 0 starts at the carried window, read from carry slot
    // `slot_in`; the last window's finished maps go to slot `slot_out`
    int stream = 0, carry_in = 0, slot_in = 0, slot_out = 0;
    // bidirectional stream call (eemflow_forward_stream_bidir): `batch` = 2 x the pairs, the second half with the windows exchanged
    int bidir = 0;
};

struct eemflow_ctx {
    int device = 0;
    bool weights_loaded = false;
    int cin0 = 5, groups = 5;
    // padder
    bool have_pad = false;
    int pad[4] = {0, 0, 0, 0};
    // weights: `flat` is the device-resident master copy in state_dict order; `arena` holds every packed
    // form the kernels read (MFMA fragment orders, biases, transposed weights for the data gradients) and is
    // rebuilt from `flat` by one gather kernel driven by `pack_idx` (arena[i] = flat[pack_idx[i]-1], 0 -> 0.f)
    float* flat = nullptr;
    size_t nflat = 0;
    int* pack_idx = nullptr;
    size_t arena_floats = 0;
    float* arena = nullptr;
    size_t enc_w[ENC_NUM], enc_w2[ENC_NUM], enc_b[ENC_NUM];
    bool enc_has2[ENC_NUM];
    // Winograd-domain weights of the stride-1 C->C encoder layers, both forms (F(2x2,3x3): conv_wino.hip / conv_wino32.hip,
    // F(4x4,3x3): conv_wino4.hip): computed from `flat` by wino_transform_launch when a launch first needs them after a (re)pack.
    // Slot [f4 * 2 + dir][l]: dir 0 forward weights, dir 1 W^T flipped (data gradient)
    float* wino = nullptr;
    size_t wino_off[4][ENC_NUM];
    bool wino_ok[4][ENC_NUM] = {};
    size_t s2r_off[ENC_NUM];           // the stride-2 layers' weights in conv_s2r.hip's order (same buffer, same lazy refresh)
    bool s2r_ok[ENC_NUM] = {};
    bool enc_s2r[ENC_NUM] = {};
    size_t bx3_off[ENC_NUM];           // pconv2_1's weights as pre-split bf16 fragments (conv_bx3.hip; same buffer, same lazy refresh)
    bool bx3_ok[ENC_NUM] = {};
    bool enc_bx3[ENC_NUM] = {};
    bool enc_wino[ENC_NUM];
    bool use_wino = true;              // EEM_WINO=0 in the environment keeps the direct-convolution kernels
    // which stride-1 layers run F(4x4,3x3), by channel count (bit 0: C = 16, 1: C = 32, 2: C = 64).  F(4x4) blocks are 8 waves on 16 x
    // {128, 64, 32} pixel tiles: 240 / 120 / 60 blocks per frame at 1280x720 - the C = 32 / 64 layers then occupy half / a quarter of
    // the chip for longer (24 / 38 us against 17.6 / 15.3) but cost 0.68 / 0.62 of the CU time, so they are the throughput choice
    // (several frames in flight: eemflow_set_frames_in_flight >= 3) and F(2x2) the latency choice; C = 16 wins both ways.
    // EEM_WINO=2: never; EEM_WINO4_LAYERS=<mask>: always that mask
    int f4_mask_env = -1;
    // (a forward of four or more samples has the tiles to fill the chip with F(4x4) blocks too: 8 260 against 7 400 frames/s for
    // batches of four, two in flight)
    int f4_mask(int batch) const {
        if (f4_mask_env >= 0) return f4_mask_env;
        return (frames_in_flight >= 3 || batch >= 4) ? 7 : 1;
    }
    bool layer_f4(int cin, int batch) const { return (f4_mask(batch) >> (cin == 16 ? 0 : cin == 32 ? 1 : 2)) & 1; }
    float* zero_page = nullptr;
    // the decoders' two wide 3x3 layers (conv1 69 -> 100, conv5 100 -> 64; EEMFlow.py:38-71) on the Winograd F(2x2) kernel of conv_wnc.hip:
    // their streams and slice biases, made from `flat` on the device (ensure_dec_wnc) whenever the weights have changed there
    float* dec_wnc = nullptr;
    bool dec_wnc_ok = false;
    size_t dec_w1[3][4] = {}, dec_w5[3][2] = {}, dec_b1[3] = {}, dec_b5[3] = {};      // float offsets into dec_wnc
    TailW rconv[3], dconv1[3], dgroup[3][3][5], dconv5[3], dconv6[3], dconv7[3], outc;
    // training: per-conv descriptors (flat offsets of weight/bias, packed transposed weights for gconv dgrad)
    struct ConvRef {
        size_t w = 0, b = 0, wT = 0;                 // flat offsets of weight / bias; arena offset of gconv-packed W^T
        size_t wT_enc = 0, wT_enc2 = 0, zero_bias = 0;   // stride-1 encoder layers: W^T packed for the encoder kernels
        size_t wT_tail = 0;                              // tail convs: W^T packed for tail_conv_kernel (batched data gradients)
        bool has_tail = false;
        bool fast_dgrad = false;
        int cin = 0, cout = 0, k = 3, stride = 1;
    };
    ConvRef t_enc[ENC_NUM], t_rconv[3], t_dconv1[3], t_dgroup[3][3][5], t_dconv5[3], t_dconv6[3], t_dconv7[3], t_outc;
    // training workspace + optimizer state
    DevBuf padded, g_a1, g_f11, g_a2, g_b2, g_f12, g_a3, g_b3, g_f13, g_pool[3], g_cat[3], g_ta[3], g_tb[3], g_tc[3], g_td[3],
        g_t64[3], g_t32[3], g_flowcat, g_coarse, g_flow, ups_tmp, grad_flat, adam_m, adam_v, scalars;
    long opt_step = 0;
    // eemflow_forward_train / eemflow_backward pairing: the serial of the forward whose activations the workspace holds
    const float *train_e1 = nullptr, *train_e2 = nullptr;
    bool have_train_fwd = false;
    long train_serial = 0;
    Shape train_shape;                                   // the shape of THAT forward (`last` follows every forward, inference included)
    // every entry point that writes the shared workspace without keeping the activations calls this: a pending backward then finds a
    // newer serial and its caller recomputes the forward (eemflow.py) instead of differentiating somebody else's activations
    void workspace_overwritten() { have_train_fwd = false; train_serial += 1; }
    // eemflow_get_stage("g_...") / eemflow_backward_forms: the train_serial whose backward last filled the gradient buffers (-1: none;
    // they are current while it equals train_serial), whether that was eemflow_forward_backward's (g_flow = d loss / d flow), and the
    // kernel form each layer's gradients took in it as "<layer>.<what>=<form>;" text (a fixed buffer: no allocation per step)
    long bwd_serial = -1;
    bool bwd_fused_loss = false;
    static constexpr int kFormsCap = 4096;
    char bwd_forms[kFormsCap] = {};
    int bwd_forms_len = 0;
    // backward pass: weight / bias gradients are leaves of the chain of data gradients, so they run on this context-owned side stream
    // (fork: an event after the gradient they read; join: the caller's stream waits for the last one before backward returns)
    hipStream_t wstream = nullptr;
    static constexpr int kWEvents = 32;
    hipEvent_t wev[kWEvents] = {};
    hipEvent_t wjoin = nullptr;
    hipEvent_t prep_ev = nullptr;                        // the side-stream prologue of a training forward (train_api.hip: forward_train_impl)
    bool sumsq_zeroed = false;                           // the optimizer's sum-of-squares cell: cleared once by a fill, then by each step's re-packing launch
    int wev_next = 0;
    int* taps = nullptr;
    // workspaces
    DevBuf a1, f11, a2, b2, f12, a3, b3, f13, pool[3], ppart[3], cat[3], ta[3], tb[3], tc[3], td[3], t64[3], t32[3], flowcat, coarse;
    Shape last;
    bool have_last = false;
    // graph cache: up to kMaxGraphs captured forwards keyed on SHAPES only.  The two launches that touch caller buffers (the
    // first conv, the upsample) read their pointers from `io_table` (device: {events1, events2, flow_out}), which one tiny
    // launch rewrites in front of a replay whenever the caller hands over other buffers - fresh tensors per frame replay the
    // same graph.  Every entry bakes in workspace pointers: a reallocation (ensure) drops them all.
    bool use_graph = true;
    // diagnostic (EEM_SPANS=1, eager launches): events at frame start / encoder end / frame end; every 64 frames the averages of the
    // encoder chain's and the tail chain's spans under whatever else runs on the chip go to stderr (tools/spans.sh)
    hipEvent_t span_ev[3] = {nullptr, nullptr, nullptr};
    double span_sum[2] = {0.0, 0.0};
    int span_n = 0;
    bool span_pending = false;
    bool skip_counter_zeroed = false;                    // train_api.hip: the device-side count of skipped optimizer steps
    // eemflow_train_stats_async / _wait: the loss statistics of a step on their way to pinned host memory behind an event, so that the
    // host can enqueue the optimizer step (and the next forward) before it reads them
    double* stats_host = nullptr;
    hipEvent_t stats_ev = nullptr;
    bool stats_pending = false;
    hipStream_t cstream = nullptr;                       // the statistics' copy stream: the loss sums leave right behind the loss kernel
    hipEvent_t loss_ev = nullptr;                        // (round 6), not behind the whole backward
    double stats_scale = 0.0;                            // gamma weight / (B * 2 * out_h * out_w) of the forward they belong to
    // inference leaves f13 unwritten when pconv3_3's epilogue pools it (nothing else reads it); the training forward keeps every
    // activation (keep_stage_stores), and eemflow_get_stage("f13") re-runs the layer with stores when the last forward skipped them
    bool enc0_generic = false;                           // n_first_channels != 5: pconv1_1 = replicate-pad launch + gconv.hip
    size_t enc0_gw = 0;
    bool keep_stage_stores = false;
    bool f13_skipped = false;
    // pconv1_1 computed inside pconv1_2's block (conv_enc12.hip; inference, 5-bin first layer; OPT-IN: EEM_FUSE12=1, set before the context sizes its buffers):
    // `a1` is then never written - eemflow_get_stage("a1") re-runs pconv1_1 alone on the last call's event volumes
    DevBuf fuse_scratch;
    bool a1_skipped = false;
    const float* last_e1 = nullptr;                      // the last forward's caller buffers (contiguous form) / its io-table form
    const float* last_e2 = nullptr;
    int last_io_frames = 0;
    // bumped by every change of the device-resident weights (refresh_wino): what a carried stream window was encoded with
    long weights_version = 0;
    // eemflow_forward_stream: the last window's finished pooled maps, 16 + 32 + 64 channels on the 1/64 grid, in one of two slots
    // (a call reads one and writes the other).  Owned by the context, apart from the shared workspace: forward / forward_many /
    // forward_train between two stream calls leave it alone
    DevBuf carry;
    StreamCarry stream;                                  // (its wver: weights_version the window was encoded with)
    int stream_slot = 0;                                 // the slot holding the carried window
    int frames_in_flight = 1;                            // eemflow_set_frames_in_flight: >= 3 shrinks the persistent encoder grids
    // eemflow_set_deferred_input_norm: the event volumes handed to forward / forward_many are RAW voxel grids with their normalisation
    // record behind them (eemflow_voxelize*, normalize = 2); pconv1_1 normalises as it reads
    bool deferred_norm = false;
    struct Key {
        int batch, in_h, in_w, out_h, out_w, pad[4];
        int aligned16;                                   // all three caller buffers 16-byte aligned (kernel selection depends on it)
        int io_frames;                                   // 0: one batch in contiguous tensors; n: n single-frame buffer triples (eemflow_forward_many)
        int deferred_norm;
        int stream_nvol = 0;                             // eemflow_forward_stream: windows per call (0: a forward), carry present, carry slot
        int stream_carry = 0, stream_slot = 0;           // written (the slot read is the other one)
        int stream_bidir = 0;                            // eemflow_forward_stream_bidir: both directions of every pair
        bool operator==(const Key& o) const {
            return batch == o.batch && in_h == o.in_h && in_w == o.in_w && out_h == o.out_h && out_w == o.out_w &&
                   pad[0] == o.pad[0] && pad[1] == o.pad[1] && pad[2] == o.pad[2] && pad[3] == o.pad[3] && aligned16 == o.aligned16 &&
                   io_frames == o.io_frames && deferred_norm == o.deferred_norm && stream_nvol == o.stream_nvol &&
                   stream_carry == o.stream_carry && stream_slot == o.stream_slot && stream_bidir == o.stream_bidir;
        }
    };
    struct GraphEntry {
        Key key;
        Shape shape;
        bool f13_skipped = false;                        // the captured schedule leaves f13 unwritten (every replay does, then)
        bool a1_skipped = false;                         // ... and a1 (the fused first two layers)
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        long last_use = 0;
    };
    static constexpr int kMaxGraphs = 4;
    std::vector<GraphEntry> graphs;
    long graph_clock = 0;
    const void** io_table = nullptr;                     // device: 3 * EEM_MAX_COALESCE pointers
    const void* io_host[3 * EEM_MAX_COALESCE] = {};      // what the table holds once the launches issued so far have run
    int io_host_n = 0;                                   // entries of io_host in use (3: the contiguous form)
    int cur_io_frames = 0;                               // the schedule being issued reads per-frame triples (set around run_forward)
    void* io_stream = nullptr;                           // stream of the last table write / replay
    long graph_captures = 0, graph_replays = 0, io_updates = 0;   // statistics (eemflow_graph_stats)
};

// ------------------------------------------------------------------------------- launch hook
// Every kernel launch of the schedule goes through a Hook: normally it just launches; in timing mode (eemflow_time_kernels) every
// launch of a pass is bracketed by its own pair of HIP events on the launch stream - the schedule runs as the CHAIN it is, each kernel
// behind its producer, `reps` passes - and the durations are averaged per launch with its algorithmic FLOPs / bytes.  (Until round 4 a
// kernel was repeated back to back instead: at ten frames per launch that read 11 % slow for the layers whose input the launch before
// had just left in the Infinity Cache - the rocprofv3 per-kernel averages of the timed loop said so.)
struct Hook {
    hipStream_t st = nullptr;
    bool timing = false;
    int reps = 1;
    bool repeat = false;                                 // timing, the other form: each kernel `reps` times back to back between ONE pair of events
    int pass = 0;                                        // timing: pass being issued
    size_t slot = 0;                                     // timing: launch index inside the pass
    std::vector<hipEvent_t> evs;                         // timing: two events per launch of a pass, reused pass after pass
    std::vector<eemflow_kernel_stat> stats;

    // diagnostic BUILDS only (-DEEM_DIAG: `EEM_BUILD_TAG=diag EEM_EXTRA_FLAGS=-DEEM_DIAG python -m eemflow_amd.build`, loaded through
    // EEM_LIB_PATH; the release library does not read these variables): EEM_SKIP_KERNELS="enc.pconv2_1;dec." skips the launches whose
    // name starts with one of the prefixes - the flow is garbage, the frame rate says what that launch costs BESIDE the others
    // (tools/marginal.sh); read once per process
    static bool skipped(const char* name);

    template <class F>
    int run(const char* name, double flops, double bytes, F&& launch) {
#ifdef EEM_DIAG
        if (skipped(name)) {                                  // EEM_SKIP_SPIN_US=<us>: one lane holds the launch's place in the stream for <us>
            static const float spin = sw_float<SW_EEM_SKIP_SPIN_US>();
            return spin > 0.f ? spin_launch(spin, st) : EEM_OK;
        }
#endif
        if (!timing) return launch(st);
        if (repeat) {
            // (a launch of a few microseconds is mostly the gap an event pair adds around it: the single-frame table repeats each kernel
            // instead - its inputs then come from whatever cache the repetition before left them in, which at one frame per launch is
            // where the launch before it in the chain leaves them too)
            if (evs.size() < 2) { evs.resize(2, nullptr); EEM_HIP_CHECK(hipEventCreate(&evs[0])); EEM_HIP_CHECK(hipEventCreate(&evs[1])); }
            eem_last_grid_blocks = eem_last_grid_threads = eem_last_pipe = eem_last_variant = 0;
            int rc = launch(st);
            if (rc != EEM_OK) return rc;
            EEM_HIP_CHECK(hipEventRecord(evs[0], st));
            for (int i = 0; i < reps; ++i)
                if ((rc = launch(st)) != EEM_OK) return rc;
            EEM_HIP_CHECK(hipEventRecord(evs[1], st));
            EEM_HIP_CHECK(hipEventSynchronize(evs[1]));
            float ms = 0.f;
            EEM_HIP_CHECK(hipEventElapsedTime(&ms, evs[0], evs[1]));
            eemflow_kernel_stat ks;
            memset(&ks, 0, sizeof(ks));
            strncpy(ks.name, name, sizeof(ks.name) - 1);
            ks.flops = flops; ks.bytes = bytes; ks.ms = ms;      // (divided by reps by the caller, like the chain form's sums)
            ks.blocks = eem_last_grid_blocks;
            ks.pipe = eem_last_pipe; ks.reserved = eem_last_variant;
            stats.push_back(ks);
            return EEM_OK;
        }
        if (evs.size() < 2 * (slot + 1)) {
            evs.resize(2 * (slot + 1), nullptr);
            EEM_HIP_CHECK(hipEventCreate(&evs[2 * slot]));
            EEM_HIP_CHECK(hipEventCreate(&evs[2 * slot + 1]));
        }
        eem_last_grid_blocks = eem_last_grid_threads = eem_last_pipe = eem_last_variant = 0;
        EEM_HIP_CHECK(hipEventRecord(evs[2 * slot], st));
        const int rc = launch(st);
        if (rc != EEM_OK) return rc;
        EEM_HIP_CHECK(hipEventRecord(evs[2 * slot + 1], st));
        if (pass == 0) {
            eemflow_kernel_stat ks;
            memset(&ks, 0, sizeof(ks));
            strncpy(ks.name, name, sizeof(ks.name) - 1);
            ks.flops = flops; ks.bytes = bytes; ks.ms = 0.f;
            ks.blocks = eem_last_grid_blocks;                     // 0: a launcher that does not report its grid
            ks.pipe = eem_last_pipe; ks.reserved = eem_last_variant;
            stats.push_back(ks);
        }
        ++slot;
        return EEM_OK;
    }
    // after a pass has been issued: wait for it and add its durations (pass 0 is the warm-up and is not counted when reps > 1)
    int collect(bool count);
    void release();
};

// ------------------------------------------------------------------------------- workspace.hip
extern thread_local unsigned long g_realloc_events;   // the reallocation counter: bumped whenever ensure() moves a buffer
int ensure(DevBuf& b, size_t floats);                 // devbuf_ensure for the CONTEXT's buffers: only their moves drop EEMFlow's graphs
int refresh_wino(eemflow_ctx* c, hipStream_t);
int ensure_bx3(eemflow_ctx* c, int l, hipStream_t st, const float** w_out);
int ensure_s2r(eemflow_ctx* c, int l, hipStream_t st, const float** w_out);
int ensure_wino(eemflow_ctx* c, int l, int dir, int batch, hipStream_t st, const float** w_out, int* f4_out);
int ensure_dec_wnc(eemflow_ctx* c, hipStream_t st);
int ensure_train_wino(eemflow_ctx* c, int batch, hipStream_t st);
int ensure_forward_wino(eemflow_ctx* c, int batch, hipStream_t st);
void drop_graph(eemflow_ctx* c);
int compute_shape(eemflow_ctx* c, int batch, int in_h, int in_w, int out_h, int out_w, Shape* s, int nimg = -1);
int alloc_workspace(eemflow_ctx* c, const Shape& s);

// ------------------------------------------------------------------------------- schedule.hip
// dispatch policy (switches.def.h lists every environment switch the schedule reads)
bool s2r_wanted();
bool bx3_wanted(int l);
bool dec_wnc_wanted(const eemflow_ctx* c, int gw, int batch);
// the schedule
int run_decoders(eemflow_ctx* c, int k0, int k1, const float* const cat[3], int batch, int h, int w, float* flow_dst,
                 int flow_ctotal, int kbase, Hook& hk);
int run_enc_layer(eemflow_ctx* c, const Shape& s, int li, const float* e1, const float* e2, Hook& hk, const void* const* io,
                  const float* prepadded, bool may_skip_store);
// io: nullptr (eager: the caller's pointers go into the launches) or the context's device table (graph capture)
// prepadded (optional): both event volumes already replicate-padded into one [2B][cin][hp][wp] batch (the training forward keeps that
// copy for the first layer's weight gradient anyway): the first layer then reads it with no padding of its own, which puts inputs whose
// rows are not 16-byte multiples or that pad on the left (MVSEC: 346-pixel rows, 19 columns) on the LDS-DMA kernel of conv_enc1.hip
int run_forward(eemflow_ctx* c, const Shape& s, const float* e1, const float* e2, float* out, Hook& hk,
                const void* const* io = nullptr, const float* prepadded = nullptr);
