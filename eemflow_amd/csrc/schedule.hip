// The EEMFlow forward schedule (declared in ctx.h): which kernel form every layer takes, and the chain of launches from the event
// volumes to the flow - encoder, stage pooling / correlation / rconv, decoders, out_conv and upsample.  The inference entry points
// (api.hip) and the training forward (train_api.hip) run this one copy.
#include "ctx.h"

// ------------------------------------------------------------------------------- dispatch policy
// Everything that decides a kernel FORM (the tests mirror these predicates): eemflow_ctx::f4_mask / layer_f4 (ctx.h), s2r_wanted,
// bx3_wanted, dec_wnc_wanted and enc_walk below.  The launchers apply further shape conditions of their own (conv_enc.hip's
// dispatch, wnc_supported, tail_up_supported).
// The environment switches these read, and WHEN, are rows of switches.def.h (tests pin forms with setenv inside one process: only a
// per-call read follows them).
//
// The packed forms a launch can actually take (the opt-in kernels' switches are read per launch - conv_s2r.hip, conv_bx3.hip - and so are
// these): after every optimizer step the packed copies are stale, and a transform nobody reads was six ~5 us launches in the chain of
// a training step's forward
bool s2r_wanted() { return sw_on<SW_EEM_S2R>(); }
bool bx3_wanted(int l) {
    const EncLayerDesc& d = kEncLayers[l];
    return d.stride == 2 || bx3_s1_wanted(d.cin);
}
// The decoders' conv1 / conv5 on the Winograd kernel: wanted for grids whose rows are 16-byte multiples (1280x720: 12 x 20 cells; MVSEC's
// 5 x 6 stays on the small-grid kernel) from four samples per launch on - the rule of the encoder's F(4x4) forms (f4_mask): one frame alone
// is three 20-us tiles per (decoder, slice) where the small-grid kernel needs 5 - 9 us (`latency_ms_b1` 0.192 -> 0.207 ms with the kernel
// at every batch).  EEM_DEC_WNC: 0 off, 1 at every batch (tests that compare a batch with its shards pin the form), unset: by batch.
// The training forward takes the same rule.
bool dec_wnc_wanted(const eemflow_ctx* c, int gw, int batch) {
    const char* e = sw_raw<SW_EEM_DEC_WNC>();
    if (c->dec_wnc == nullptr || gw % 4 != 0 || (e && e[0] == '0')) return false;
    return (e && e[0] == '1') || batch >= 4;
}
// The F(4x4) kernel's shared-V form (conv_wino4.hip: a tile group's input transform computed once instead of by each of its four
// waves; bitwise the other form) for the 64-channel stride-1 layers of this forward - the only channel count whose LDS holds it.
// EEM_W4_VSHARE: 0 never, 1 wherever the form is built, unset: the default - on (the two launches are 6 - 9 % shorter, +1.8 % on the
// frame rate over six alternating pairs, docs/NOTEBOOK.md section 14).  Read per launch.
static bool w4_vshare_wanted(int cin) {
    const char* e = sw_raw<SW_EEM_W4_VSHARE>();
    return cin == 64 && !(e && e[0] == '0');
}
// The tail head's LDS form (tail_fused.hip: every pooled value formed once per block, correlation and rconv operands from LDS) for
// batched launches that are no stream call, where the launch supports the shapes (tail_head_lds_supported: the three stages' fused
// partial sums, kTaps53 - the only list this schedule passes -, at most 240 cells), from four frames per launch on - the decoders' rule:
// one frame alone is 21 blocks that each pay the chunk walk where tail_head_kernel's gathers are all in flight at once.  The two forms'
// outputs are bitwise equal.  EEM_TAIL_HEAD_LDS: 0 never, 1 wherever it is supported, unset: by batch.
static bool tail_head_lds_wanted(const Shape& s, const TailHeadArgs& ha) {
    const char* e = sw_raw<SW_EEM_TAIL_HEAD_LDS>();
    if (s.stream || !tail_head_lds_supported(ha) || (e && e[0] == '0')) return false;
    return (e && e[0] == '1') || s.batch >= 4;
}

// The order in which a layer's blocks walk its tiles, its non-temporal stores and its grid under several frames in flight: the fields
// reverse / nt_store / blocks_per_xcd of the layer's launch arguments
static void enc_walk(const eemflow_ctx* c, const Shape& s, int layer, EncConvArgs& a) {
    a.reverse = 0;
    // batched chains walk their tiles in COLUMNS (EEM_COLWALK=<layer mask>; default: the two 64-channel layers of a batched chain).  Measured at ten frames
    // per launch (rocprofv3 FETCH_SIZE): the 32-pixel-wide tiles of the 64-channel layers fetch 22.3 MB per frame in row order
    // and 10.8 / 10.3 in column order (a tile row touches three cache lines for one of payload, and in row order the neighbour
    // that shares two of them comes a whole tile later); 32 channels 29.0 -> 32.2 (worse), 16 channels unchanged; frame rate the
    // same within noise either way - those layers are bound by their transforms, not their bytes
    static_assert(kSwitches[SW_EEM_COLWALK].dflt == ((1 << ENC_3_2) | (1 << ENC_3_3)), "switches.def.h: EEM_COLWALK's default");
    const int cw = sw_int_once<SW_EEM_COLWALK>();
    if (s.enc_batch >= 2 && ((cw >> layer) & 1)) a.reverse = 2;
    // ... or INTERLEAVED (EEM_WALK3=<layer mask>, round 6): an XCD's blocks take every G-th tile of its range, so neighbouring
    // tiles are in flight together (conv_wino4.hip)
    // Measured at ten frames per launch (profiles/r06_walk3.txt): FETCH_SIZE per frame pconv1_2 49.5 -> 32.8 MB (31.5 of input),
    // pconv2_2 / 2_3 29.0 -> 17.0, pconv3_2 / 3_3 10.8 / 10.3 (column walk) -> 9.9 / 9.3; encoder 342 -> 299 MB per frame;
    // 10 290 -> 10 500 frames/s over 400 steps.  Default for every stride-1 layer of a batched chain (supersedes the column walk).
    static_assert(kSwitches[SW_EEM_WALK3].dflt == ((1 << ENC_1_2) | (1 << ENC_2_2) | (1 << ENC_2_3) | (1 << ENC_3_2) | (1 << ENC_3_3)), "switches.def.h: EEM_WALK3's default");
    const int w3 = sw_int_once<SW_EEM_WALK3>();
    if (s.enc_batch >= 2 && ((w3 >> layer) & 1)) a.reverse = 3;
    a.nt_store = 0;
    // several frames in flight: kernels of different frames time-slice the CUs, so a block's prologue (DMA plan, first tile's
    // landing) is CU time another frame could use - fewer blocks with more tiles each (measured at 1280x720 with four in flight:
    // +3.5 % frames/s, +8 % single-frame latency; the 64-channel layers have one tile per CU and keep the full grid)
    // (pconv1_1, HBM-bound: 12 / 14 / 20 blocks per XCD give the same frame rate within 1 % - 8 610-8 660 / 8 580-8 620 / 8 520-8 580 -,
    // so it takes the fewest CUs: 32 us on 96 of them)
    static const int kInFlightBlocks[ENC_NUM] = {12, 24, 0, 29, 29, 0, 0, 0};
    a.blocks_per_xcd = c->frames_in_flight >= 3 ? kInFlightBlocks[layer] : 0;
}

// ------------------------------------------------------------------------------- launch hook (non-template members)
// EEM_SKIP_KERNELS (diagnostic builds; ctx.h describes it)
#ifndef EEM_DIAG
bool Hook::skipped(const char*) { return false; }
#else
bool Hook::skipped(const char* name) {
    static const std::string list = [] {
        const char* e = sw_raw_once<SW_EEM_SKIP_KERNELS>();
        if (e && e[0]) fprintf(stderr, "eemflow_hip: EEM_SKIP_KERNELS=\"%s\" is set - the launches it names are skipped and the flow is GARBAGE (diagnostic runs only)\n", e);
        return std::string(e ? e : "");
    }();
    if (list.empty()) return false;
    size_t pos = 0;
    while (pos <= list.size()) {
        size_t end = list.find(';', pos);
        if (end == std::string::npos) end = list.size();
        if (end > pos && strncmp(name, list.c_str() + pos, end - pos) == 0) return true;
        pos = end + 1;
    }
    return false;
}
#endif
int Hook::collect(bool count) {
    for (size_t i = 0; i < slot && i < stats.size(); ++i) {
        EEM_HIP_CHECK(hipEventSynchronize(evs[2 * i + 1]));
        float ms = 0.f;
        EEM_HIP_CHECK(hipEventElapsedTime(&ms, evs[2 * i], evs[2 * i + 1]));
        if (count) stats[i].ms += ms;
    }
    slot = 0;
    ++pass;
    return EEM_OK;
}
void Hook::release() {
    for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    evs.clear();
}

// ------------------------------------------------------------------------------- schedule
TailConvJob make_job(const eemflow_ctx* c, const TailW& w, const float* in, int in_ctotal, int in_coff, float* out,
                     int out_ctotal, int out_coff, int out_cmul, int act) {
    TailConvJob j;
    j.in = in; j.wpk = c->arena + w.wpk; j.bias = c->arena + w.bias; j.out = out;
    j.cin = w.cin; j.cout = w.cout;
    j.in_ctotal = in_ctotal; j.in_coff = in_coff;
    j.out_ctotal = out_ctotal; j.out_coff = out_coff; j.out_cmul = out_cmul; j.act = act;
    j.gate = nullptr; j.in_cmul = 1; j.add = nullptr;
    return j;
}

double tail_flops(const TailConvLaunch& L) {
    double f = 0;
    for (int i = 0; i < L.njobs; ++i)
        f += 2.0 * L.batch * L.h * L.w * (double)L.job[i].cout * L.job[i].cin * L.ksize * L.ksize;
    return f;
}
double tail_bytes(const TailConvLaunch& L) {
    double b = 0;
    for (int i = 0; i < L.njobs; ++i)
        b += 4.0 * ((double)L.batch * L.h * L.w * (L.job[i].cin + L.job[i].cout) +
                    (double)L.job[i].cout * L.job[i].cin * L.ksize * L.ksize + L.job[i].cout);
    return b;
}
int run_tail(Hook& hk, const char* name, const TailConvLaunch& L) {
    return hk.run(name, tail_flops(L), tail_bytes(L), [&](hipStream_t st) { return tail_conv_launch(L, st); });
}

// decoder convs 1..7 for decoders [k0,k1); input cat buffers `cat[k]`, final 2-ch flow of decoder k goes to
// channels [2*(k-kbase), +2) of `flow_dst` (which has flow_ctotal channels)
int run_decoders(eemflow_ctx* c, int k0, int k1, const float* const cat[3], int batch, int h, int w, float* flow_dst,
                 int flow_ctotal, int kbase, Hook& hk) {
    int rc;
    TailConvLaunch L;
    L.batch = batch; L.h = h; L.w = w; L.ksize = 3;
    // conv1 (69 -> 100) and conv5 (100 -> 64) on the Winograd kernel where the grid and the batch allow (dec_wnc_wanted): the decoders' 32-cout
    // slices as the jobs of one launch.  woff: the streams' offsets in dec_wnc, wper per decoder; *done says whether the launch was made
    auto wide = [&](const char* name, int cin, int cout, const float* const* in, float* const* outp, const size_t* woff, int wper,
                    const size_t* boff, bool* done) -> int {
        *done = false;
        if (!dec_wnc_wanted(c, w, batch)) return EEM_OK;
        int r2 = ensure_dec_wnc(c, hk.st);
        if (r2 != EEM_OK) return r2;
        WncArgs wa;
        memset(&wa, 0, sizeof(wa));
        wa.nchunks = wnc_chunks(cin, wa.chunk_off);
        wa.cin = cin; wa.n = batch; wa.h = h; wa.w = w; wa.act = 1; wa.m16 = 0;
        wa.zero_page = c->zero_page; wa.trash = c->zero_page + 256;
        const int ns = (cout + 31) / 32;
        for (int k = k0; k < k1; ++k)
            for (int s = 0; s < ns; ++s) {
                if (wa.njobs == WNC_MAX_JOBS) return EEM_OK;           // (more decoders than a launch has jobs: the small-grid kernel)
                WncJob& J = wa.job[wa.njobs++];
                J.in = in[k]; J.in_ctotal = cin; J.in_coff = 0;
                J.w = c->dec_wnc + woff[k * wper + s]; J.bias = c->dec_wnc + boff[k] + 32 * s;
                J.out = outp[k]; J.out_ctotal = cout; J.out_coff = 32 * s; J.out_cmul = 1; J.cout = cout - 32 * s < 32 ? cout - 32 * s : 32;
                J.res = nullptr;
            }
        if (!wnc_supported(wa)) return EEM_OK;
        const double px = (double)batch * h * w * (k1 - k0);
        r2 = hk.run(name, 2.0 * px * cin * cout * 9, 4.0 * px * (cin + cout), [&](hipStream_t st) {
            const int r3 = wnc_launch(wa, st);
            eem_last_pipe = 3;
            return r3;
        });
        *done = r2 == EEM_OK;
        return r2;
    };
    bool on_wnc = false;
    {
        float* outs[3] = {c->ta[0].p, c->ta[1].p, c->ta[2].p};
        if ((rc = wide("dec.conv1 69->100", kDecIn, kDecW, cat, outs, &c->dec_w1[0][0], 4, c->dec_b1, &on_wnc)) != EEM_OK) return rc;
    }
    if (!on_wnc) {
        L.njobs = 0;
        for (int k = k0; k < k1; ++k) L.job[L.njobs++] = make_job(c, c->dconv1[k], cat[k], kDecIn, 0, c->ta[k].p, kDecW, 0, 1, 1);
        if ((rc = run_tail(hk, "dec.conv1 69->100", L)) != EEM_OK) return rc;
    }
    // conv2..4: grouped 100 -> 100, each followed by channel_shuffle (EEMFlow.py:51-57):
    // group g, in-group channel j lands in channel j*groups + g
    const int G = c->groups, per = kDecW / G;
    const char* gname[3] = {"dec.conv2 grouped+shuffle", "dec.conv3 grouped+shuffle", "dec.conv4 grouped+shuffle"};
    for (int layer = 0; layer < 3; ++layer) {
        L.njobs = 0;
        for (int k = k0; k < k1; ++k) {
            // every activation keeps its own buffer (the training step reads them back): ta -> tb -> tc -> td
            float* chain[4] = {c->ta[k].p, c->tb[k].p, c->tc[k].p, c->td[k].p};
            float* src = chain[layer];
            float* dst = chain[layer + 1];
            for (int g = 0; g < G; ++g) {
                if (G == 1) L.job[L.njobs++] = make_job(c, c->dgroup[k][layer][g], src, kDecW, 0, dst, kDecW, 0, 1, 1);
                else L.job[L.njobs++] = make_job(c, c->dgroup[k][layer][g], src, kDecW, g * per, dst, kDecW, g, G, 1);
            }
        }
        if ((rc = run_tail(hk, gname[layer], L)) != EEM_OK) return rc;
    }
    {
        const float* ins[3] = {c->td[0].p, c->td[1].p, c->td[2].p};
        float* outs[3] = {c->t64[0].p, c->t64[1].p, c->t64[2].p};
        if ((rc = wide("dec.conv5 100->64", kDecW, 64, ins, outs, &c->dec_w5[0][0], 2, c->dec_b5, &on_wnc)) != EEM_OK) return rc;
    }
    if (!on_wnc) {
        L.njobs = 0;
        for (int k = k0; k < k1; ++k) L.job[L.njobs++] = make_job(c, c->dconv5[k], c->td[k].p, kDecW, 0, c->t64[k].p, 64, 0, 1, 1);
        if ((rc = run_tail(hk, "dec.conv5 100->64", L)) != EEM_OK) return rc;
    }
    L.njobs = 0;
    for (int k = k0; k < k1; ++k) L.job[L.njobs++] = make_job(c, c->dconv6[k], c->t64[k].p, 64, 0, c->t32[k].p, 32, 0, 1, 1);
    if ((rc = run_tail(hk, "dec.conv6 64->32", L)) != EEM_OK) return rc;
    L.njobs = 0;
    for (int k = k0; k < k1; ++k)
        L.job[L.njobs++] = make_job(c, c->dconv7[k], c->t32[k].p, 32, 0, flow_dst, flow_ctotal, 2 * (k - kbase), 1, 0);
    return run_tail(hk, "dec.conv7 32->2", L);
}

static bool spans_on() {
#ifdef EEM_DIAG
    return sw_on_once<SW_EEM_SPANS>();
#else
    return false;                                        // EEM_SPANS is a diagnostic-build switch (-DEEM_DIAG)
#endif
}
static int span_mark(eemflow_ctx* c, int i, hipStream_t st) {
    if (!spans_on()) return EEM_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (cs != hipStreamCaptureStatusNone) return EEM_OK;
    if (i == 0 && c->span_pending) {
        EEM_HIP_CHECK(hipEventSynchronize(c->span_ev[2]));
        float a = 0.f, b = 0.f;
        EEM_HIP_CHECK(hipEventElapsedTime(&a, c->span_ev[0], c->span_ev[1]));
        EEM_HIP_CHECK(hipEventElapsedTime(&b, c->span_ev[1], c->span_ev[2]));
        c->span_sum[0] += a; c->span_sum[1] += b;
        if (++c->span_n == 64) {
            fprintf(stderr, "EEM_SPANS ctx %p: encoder chain %.1f us, tail chain %.1f us (64 frames)\n", (void*)c,
                    c->span_sum[0] / 64 * 1e3, c->span_sum[1] / 64 * 1e3);
            c->span_sum[0] = c->span_sum[1] = 0.0; c->span_n = 0;
        }
        c->span_pending = false;
    }
    if (!c->span_ev[i]) EEM_HIP_CHECK(hipEventCreate(&c->span_ev[i]));
    EEM_HIP_CHECK(hipEventRecord(c->span_ev[i], st));
    if (i == 2) c->span_pending = true;
    return EEM_OK;
}

// One encoder layer of the schedule (layer index = position in the chain).  may_skip_store: a layer whose output is read only
// through its fused pooling partial sums - pconv3_3 in inference - may leave the feature map unwritten (7.9 MB per frame at
// 1280x720); eemflow_get_stage("f13") then re-runs that one layer with stores.
int run_enc_layer(eemflow_ctx* c, const Shape& s, int li, const float* e1, const float* e2, Hook& hk, const void* const* io,
                  const float* prepadded, bool may_skip_store) {
    int rc;
    const int n2 = s.nimg;
    struct Step { int layer; const char* name; const float* in; float* out; int hin, win, hout, wout; };
    const Step steps[ENC_NUM] = {
        {ENC_1_1, "enc.pconv1_1 5->16 s2 +pad", nullptr, c->a1.p, s.hp, s.wp, s.h1, s.w1},
        {ENC_1_2, "enc.pconv1_2 16->16", c->a1.p, c->f11.p, s.h1, s.w1, s.h1, s.w1},
        {ENC_2_1, "enc.pconv2_1 16->32 s2", c->f11.p, c->a2.p, s.h1, s.w1, s.h2, s.w2},
        {ENC_2_2, "enc.pconv2_2 32->32", c->a2.p, c->b2.p, s.h2, s.w2, s.h2, s.w2},
        {ENC_2_3, "enc.pconv2_3 32->32", c->b2.p, c->f12.p, s.h2, s.w2, s.h2, s.w2},
        {ENC_3_1, "enc.pconv3_1 32->64 s2", c->f12.p, c->a3.p, s.h2, s.w2, s.h3, s.w3},
        {ENC_3_2, "enc.pconv3_2 64->64", c->a3.p, c->b3.p, s.h3, s.w3, s.h3, s.w3},
        {ENC_3_3, "enc.pconv3_3 64->64", c->b3.p, c->f13.p, s.h3, s.w3, s.h3, s.w3}};
    if (li == ENC_1_1 && c->enc0_generic) {
        // n_first_channels != 5 (EEMFlow.py:72,75): replicate pad of both volumes into one batch (image_utils.py:129-140), then the generic
        // strided convolution + LeakyReLU
        const float* padded = prepadded;
        if (padded == nullptr) {
            EEM_REQUIRE(io == nullptr, "the generic first layer runs eagerly (no graph io table)");
            if ((rc = er_pad2_launch(e1, e2, c->padded.p, s.batch * c->cin0, s.in_h, s.in_w, c->pad[0], c->pad[1], c->pad[2], c->pad[3], hk.st)) != EEM_OK) return rc;
            padded = c->padded.p;
        }
        GConvArgs g;
        memset(&g, 0, sizeof(g));
        g.nseg = 1;
        g.seg[0].ptr = padded; g.seg[0].c = c->cin0; g.seg[0].ctotal = c->cin0; g.seg[0].coff = 0;
        g.wpk = c->arena + c->enc0_gw; g.shift = c->arena + c->enc_b[ENC_1_1];
        g.zero_page = c->zero_page;
        g.out = c->a1.p; g.out_ctotal = 16; g.out_coff = 0;
        g.n = n2; g.hin = s.hp; g.win = s.wp; g.hout = s.h1; g.wout = s.w1; g.cout = 16;
        g.kh = g.kw = 3; g.stride = 2; g.pad_h = g.pad_w = 1;
        g.act = GACT_LEAKY; g.epi = GEPI_PLAIN; g.out_scale = 1.f;
        const double opix = (double)n2 * s.h1 * s.w1;
        return hk.run("enc.pconv1_1 generic +pad", 2.0 * opix * 16 * c->cin0 * 9, 4.0 * ((double)n2 * s.in_h * s.in_w * c->cin0 + opix * 16),
                      [&](hipStream_t st) { return gconv_launch(g, st); });
    }
    {
        const Step& sp = steps[li];

        EncConvArgs a;
        const EncLayerDesc& d = kEncLayers[sp.layer];
        a.in0 = sp.layer == ENC_1_1 ? e1 : sp.in;
        a.in1 = sp.layer == ENC_1_1 ? e2 : nullptr;
        a.wpk = c->arena + c->enc_w[sp.layer];
        a.wpk2 = c->enc_has2[sp.layer] ? c->arena + c->enc_w2[sp.layer] : nullptr;
        a.wwino = nullptr;
        a.wino_f4 = 0;
        if (c->use_wino && c->enc_wino[sp.layer] && (rc = ensure_wino(c, sp.layer, 0, s.enc_batch, hk.st, &a.wwino, &a.wino_f4)) != EEM_OK) return rc;
        a.ws2r = nullptr;
        if (c->enc_s2r[sp.layer] && s2r_wanted() && (rc = ensure_s2r(c, sp.layer, hk.st, &a.ws2r)) != EEM_OK) return rc;
        a.wbx3 = nullptr;
        if (c->enc_bx3[sp.layer] && bx3_wanted(sp.layer) && (rc = ensure_bx3(c, sp.layer, hk.st, &a.wbx3)) != EEM_OK) return rc;
        a.zero_page = c->zero_page;
        a.trash = c->zero_page + 256;
        a.bias = c->arena + c->enc_b[sp.layer];
        a.out = sp.out;
        a.nimg = n2; a.nimg0 = sp.layer == ENC_1_1 ? s.nimg0 : n2;
        a.hin = sp.hin; a.win = sp.win; a.hout = sp.hout; a.wout = sp.wout;
        a.hraw = sp.layer == ENC_1_1 ? s.in_h : sp.hin;
        a.wraw = sp.layer == ENC_1_1 ? s.in_w : sp.win;
        a.pad_top = sp.layer == ENC_1_1 ? c->pad[2] : 0;
        a.pad_left = sp.layer == ENC_1_1 ? c->pad[0] : 0;
        if (sp.layer == ENC_1_1 && prepadded != nullptr) {
            a.in0 = prepadded;
            a.in1 = prepadded + (size_t)s.batch * c->cin0 * s.hp * s.wp;
            a.hraw = s.hp; a.wraw = s.wp; a.pad_top = 0; a.pad_left = 0;
        }
        a.act = 1;
        a.gate = nullptr;
        a.pool_partial = nullptr;
        a.pool_k = 0;
        a.io = sp.layer == ENC_1_1 ? io : nullptr;
        a.io_frames = (sp.layer == ENC_1_1 && io != nullptr) ? c->cur_io_frames : 0;
        a.in_norm = (sp.layer == ENC_1_1 && c->deferred_norm && prepadded == nullptr) ? 1 : 0;
        a.no_store = 0;
        a.vshare = w4_vshare_wanted(d.cin) ? 1 : 0;
        enc_walk(c, s, sp.layer, a);
        for (int k = 0; k < 3; ++k)
            if (s.fuse[k] && sp.layer == (k == 0 ? ENC_1_2 : k == 1 ? ENC_2_3 : ENC_3_3)) {
                a.pool_partial = c->ppart[k].p;
                a.pool_k = k == 0 ? 32 : k == 1 ? 16 : 8;
                if (k == 2 && may_skip_store) a.no_store = 1;
            }
        const double opix = (double)n2 * sp.hout * sp.wout;
        const double flops = 2.0 * opix * d.cout * d.cin * 9;
        const double ipix = sp.layer == ENC_1_1 ? (double)n2 * s.in_h * s.in_w : (double)n2 * sp.hin * sp.win;
        const double bytes = 4.0 * (ipix * d.cin + opix * d.cout + (double)d.cout * d.cin * 9 + d.cout);
        rc = hk.run(sp.name, flops, bytes,
                    [&](hipStream_t st) { return enc_conv_launch(d.cin, d.cout, d.stride, a, st); });
        if (rc != EEM_OK) return rc;
    }
    return EEM_OK;
}

// The first two encoder layers as ONE launch (conv_enc12.hip) when the schedule allows it: *done says whether it ran
int run_enc12(eemflow_ctx* c, const Shape& s, const float* e1, const float* e2, Hook& hk, const void* const* io, const float* prepadded,
              bool* done) {
    *done = false;
    // opt-in (EEM_FUSE12=1; read per schedule build - a cached graph keeps the form it was captured with): measured SLOWER than the two
    // launches it replaces, kept for the traffic it saves and as the record of that measurement
    const bool off = !sw_on<SW_EEM_FUSE12>();
    if (off || s.stream || c->deferred_norm || c->keep_stage_stores || c->enc0_generic || prepadded != nullptr || !c->use_wino || !c->enc_wino[ENC_1_2] ||
        !c->layer_f4(16, s.batch) || !s.fuse[0] || c->fuse_scratch.p == nullptr)
        return EEM_OK;
    int rc;
    Enc12Args a;
    memset(&a, 0, sizeof(a));
    a.in0 = e1; a.in1 = e2; a.io = io; a.io_frames = io != nullptr ? c->cur_io_frames : 0;
    a.wpk1 = c->arena + c->enc_w[ENC_1_1]; a.bias1 = c->arena + c->enc_b[ENC_1_1];
    int f4 = 0;
    if ((rc = ensure_wino(c, ENC_1_2, 0, s.batch, hk.st, &a.u2, &f4)) != EEM_OK) return rc;
    if (!f4) return EEM_OK;
    a.bias2 = c->arena + c->enc_b[ENC_1_2];
    a.zero_page = c->zero_page; a.trash = c->zero_page + 256;
    a.out = c->f11.p; a.pool_partial = c->ppart[0].p; a.scratch = c->fuse_scratch.p;
    a.nimg = 2 * s.batch; a.nimg0 = s.batch;
    a.hraw = s.in_h; a.wraw = s.in_w; a.pad_top = c->pad[2];
    a.hin = s.hp; a.win = s.wp; a.h1 = s.h1; a.w1 = s.w1;
    if (c->pad[0] != 0 || !enc12_supported(a)) return EEM_OK;
    const int blocks = enc12_blocks(a.nimg, a.h1, a.w1, 0);
    if (enc12_scratch_floats(blocks) > c->fuse_scratch.cap) return EEM_OK;
    const double n2 = 2.0 * s.batch, opix = n2 * s.h1 * s.w1;
    const double flops = 2.0 * opix * 16 * (5 + 16) * 9;
    const double bytes = 4.0 * (n2 * s.in_h * s.in_w * 5 + opix * 16 + 16.0 * (5 + 16) * 9 + 32);
    rc = hk.run("enc.pconv1_1+1_2 fused 5->16 s2 +pad, 16->16", flops, bytes, [&](hipStream_t st) { return enc12_launch(a, blocks, st); });
    if (rc == EEM_OK) *done = true;
    return rc;
}

int run_forward_impl(eemflow_ctx* c, const Shape& s, const float* e1, const float* e2, float* out, Hook& hk,
                     const void* const* io, const float* prepadded);
int run_forward(eemflow_ctx* c, const Shape& s, const float* e1, const float* e2, float* out, Hook& hk,
                const void* const* io, const float* prepadded) {
    int rc = span_mark(c, 0, hk.st);
    if (rc == EEM_OK) rc = run_forward_impl(c, s, e1, e2, out, hk, io, prepadded);
    if (rc == EEM_OK) rc = span_mark(c, 2, hk.st);
    return rc;
}

int run_forward_impl(eemflow_ctx* c, const Shape& s, const float* e1, const float* e2, float* out, Hook& hk,
                     const void* const* io, const float* prepadded) {
    int rc;
    const int n2 = s.nimg;
    // ---- encoder (both event volumes as one batch; shared weights, EEMFlow.py:135-140; a stream call: its new windows)
    // pconv1_1 + pconv1_2 as one launch when nothing needs a1 itself (inference; the training forward keeps every activation)
    bool fused12 = false;
    if ((rc = run_enc12(c, s, e1, e2, hk, io, prepadded, &fused12)) != EEM_OK) return rc;
    c->a1_skipped = fused12;
    for (int li = fused12 ? ENC_2_1 : 0; li < ENC_NUM; ++li)
        if ((rc = run_enc_layer(c, s, li, e1, e2, hk, io, prepadded, !c->keep_stage_stores)) != EEM_OK) return rc;
    c->f13_skipped = !c->keep_stage_stores;
    // ---- stage pooling to the common 1/64 grid (EEMFlow.py:144-154), 53-tap correlation and rconv into the decoders' input
    // [cv | r] (EEMFlow.py:160-163).  ONE launch whose correlation / rconv blocks read the conv epilogues'
    // pooling partial sums directly and whose extra blocks write the finished pooled maps (tail_fused.hip).  Stages whose conv
    // ran the generic kernel are pooled from the stored feature map first.
    const size_t g = (size_t)s.gh * s.gw;
    const int pc[3] = {16, 32, 64};
    {
        const float* feat[3] = {c->f11.p, c->f12.p, c->f13.p};
        const int hs[3] = {s.h1, s.h2, s.h3}, ws[3] = {s.w1, s.w2, s.w3}, ks[3] = {32, 16, 8};
        PoolJob pj[3];
        int np = 0;
        double fin_elems = 0, pool_elems = 0;
        for (int k = 0; k < 3; ++k) {
            if (s.fuse[k]) {
                fin_elems += (double)n2 * pc[k] * s.gh * s.gw * (ks[k] / s.th[k] + 1);
            } else {
                pj[np++] = {feat[k], c->pool[k].p, pc[k], hs[k], ws[k], ks[k]};
                pool_elems += (double)n2 * pc[k] * hs[k] * ws[k];
            }
        }
        if (np) {
            rc = hk.run("pool 32/16/8", pool_elems, 4.0 * pool_elems,
                        [&](hipStream_t st) { return pool_launch(pj, np, n2, st); });
            if (rc != EEM_OK) return rc;
        }
        if ((rc = span_mark(c, 1, hk.st)) != EEM_OK) return rc;
        // where the tail head reads stage k's pooled map: the conv epilogue's partial sums, or the finished map of the pool launch
        auto pooled_src = [&](PooledSrc& ps, int k) {
            if (s.fuse[k]) {
                const int rows = ks[k] / s.th[k];
                ps.base = c->ppart[k].p; ps.rows = rows; ps.rstride = s.pcol[k]; ps.ystride = rows * s.pcol[k];
                ps.cstride = s.prow[k] * s.pcol[k]; ps.nstride = pc[k] * ps.cstride; ps.scale = 1.f / (float)(ks[k] * ks[k]);
            } else {
                ps.base = c->pool[k].p; ps.rows = 1; ps.rstride = 0; ps.ystride = s.gw; ps.cstride = (int)g;
                ps.nstride = pc[k] * (int)g; ps.scale = 1.f;
            }
        };
        if (s.stream) {
            // consecutive windows: pair b compares window b - 1 + i2_off with the next one; the carried window's finished maps stand in for
            // window -1, and the last window's finished maps become the next call's carry (the other slot: no launch reads what it writes)
            TailHeadStreamArgs sa;
            memset(&sa, 0, sizeof(sa));
            TailHeadArgs& ha = sa.base;
            const size_t coff[3] = {0, 16 * g, 48 * g}, slot = 112 * g;
            for (int k = 0; k < 3; ++k) {
                pooled_src(ha.src[k], k);
                PooledSrc& cs = sa.carry[k];
                cs.base = s.carry_in ? c->carry.p + s.slot_in * slot + coff[k] : nullptr;
                cs.rows = 1; cs.rstride = 0; cs.ystride = s.gw; cs.cstride = (int)g; cs.nstride = pc[k] * (int)g; cs.scale = 1.f;
                ha.c[k] = pc[k];
                ha.cat[k] = c->cat[k].p;
                ha.pool_out[k] = c->carry.p + s.slot_out * slot + coff[k];
                ha.rw[k] = c->arena + c->rconv[k].wpk;
                ha.rb[k] = c->arena + c->rconv[k].bias;
            }
            ha.batch = s.batch; ha.gh = s.gh; ha.gw = s.gw; ha.ntaps = kNTaps; ha.cat_ctotal = kDecIn;
            sa.i2_off = s.carry_in ? 0 : 1;
            sa.pool_img = s.nimg - 1;
            sa.nfw = s.bidir ? s.batch / 2 : s.batch;             // bidirectional: pairs nfw .. 2 nfw - 1 are the first nfw, roles exchanged
            const double fl = 2.0 * s.batch * g * (kNTaps * (16 + 32 + 64) + 16.0 * 9 * (16 + 32 + 64));
            rc = hk.run("tail head: stream pool+corr53+rconv", fl, 4.0 * (fin_elems + 3.0 * s.batch * g * kDecIn),
                        [&](hipStream_t st) { return tail_head_stream_launch(sa, kTaps53, st); });
            if (rc != EEM_OK) return rc;
            if (s.batch == 0) return EEM_OK;                 // a first call of one window: nothing to decode, the carry is written
        } else {
            TailHeadArgs ha;
            memset(&ha, 0, sizeof(ha));
            for (int k = 0; k < 3; ++k) {
                pooled_src(ha.src[k], k);
                ha.c[k] = pc[k];
                ha.cat[k] = c->cat[k].p;
                ha.pool_out[k] = s.fuse[k] ? c->pool[k].p : nullptr;
                ha.rw[k] = c->arena + c->rconv[k].wpk;
                ha.rb[k] = c->arena + c->rconv[k].bias;
            }
            ha.batch = s.batch; ha.gh = s.gh; ha.gw = s.gw; ha.ntaps = kNTaps; ha.cat_ctotal = kDecIn;
            const double fl = 2.0 * s.batch * g * (kNTaps * (16 + 32 + 64) + 16.0 * 9 * (16 + 32 + 64));
            const bool lds_form = tail_head_lds_wanted(s, ha);
            rc = hk.run("tail head: pool+corr53+rconv", fl, 4.0 * (fin_elems + 3.0 * s.batch * g * kDecIn), [&](hipStream_t st) {
                return lds_form ? tail_head_lds_launch(ha, kTaps53, st) : tail_head_launch(ha, kTaps53, st);
            });
            if (rc != EEM_OK) return rc;
        }
    }
    TailConvLaunch L;
    L.batch = s.batch; L.h = s.gh; L.w = s.gw; L.ksize = 3; L.njobs = 0;
    // ---- decoders, out_conv, upsample (EEMFlow.py:164-181)
    const float* cats[3] = {c->cat[0].p, c->cat[1].p, c->cat[2].p};
    const bool fuse_up = tail_up_supported(s.gh, s.gw, s.out_h, s.out_w);
    if ((rc = run_decoders(c, 0, 3, cats, s.batch, s.gh, s.gw, c->flowcat.p, 6, 0, hk)) != EEM_OK) return rc;
    if (fuse_up) {
        // out_conv + bilinear upsample in one launch; `coarse` is its side output
        TailUpArgs ua;
        memset(&ua, 0, sizeof(ua));
        ua.wo = c->flat + c->t_outc.w; ua.bo = c->flat + c->t_outc.b;
        ua.flowcat = c->flowcat.p; ua.coarse = c->coarse.p; ua.out = out; ua.io = io;
        ua.io_frames = io != nullptr ? c->cur_io_frames : 0;
        ua.batch = s.batch; ua.gh = s.gh; ua.gw = s.gw; ua.oh = s.out_h; ua.ow = s.out_w;
        ua.out_aligned16 = ((uintptr_t)out & 15) == 0;
        const double opix = (double)s.batch * 2 * s.out_h * s.out_w;
        return hk.run("tail up: out_conv+upsample", 8.0 * opix + 2.0 * s.batch * g * 12,
                      4.0 * (opix + (double)s.batch * 8 * g), [&](hipStream_t st) { return tail_up_launch(ua, st); });
    }
    L.ksize = 1; L.njobs = 1;
    L.job[0] = make_job(c, c->outc, c->flowcat.p, 6, 0, c->coarse.p, 2, 0, 1, 0);
    if ((rc = run_tail(hk, "out_conv 1x1 6->2", L)) != EEM_OK) return rc;
    const double opix = (double)s.batch * 2 * s.out_h * s.out_w;
    return hk.run("upsample bilinear", 8.0 * opix, 4.0 * (opix + (double)s.batch * 2 * g), [&](hipStream_t st) {
        return upsample_launch(c->coarse.p, out, s.batch * 2, s.gh, s.gw, s.out_h, s.out_w, st, io, io != nullptr ? c->cur_io_frames : 0);
    });
}
