// Two fused launches of EEMFlow's 1/64-grid tail (EEMFlow.py:144-181).  The tail is latency-bound: 13 launches of 3-8 us
// each for 0.3 GFLOP, every one paying a kernel boundary plus a memory round trip.  These two take five of them away:
//
//   tail_head_kernel   stage pooling finish + 9x9 local correlation (53 taps) + rconv_k   (once three launches: pool finalize, corr, rconv)
//       Nothing in it waits for anything else in it: the correlation and the rconv input gathers read the conv epilogues'
//       pooling PARTIAL sums directly (2-4 loads per pooled value, all in flight) instead of a finished pooled map; the
//       pooled maps themselves are still written, by extra blocks of the same launch (parity tests and the training
//       backward read them).
//   tail_up_kernel     out_conv 1x1 (6 -> 2) + bilinear upsample   (was: out_conv, upsample)
//       A block owns an output tile no larger than one coarse cell, so at most 3x3 coarse pixels reach it; it computes
//       their out_conv values itself, keeps them in LDS and interpolates (x weights once per thread, rows walked);
//       `coarse` is written as a side output.  (Measured and dropped: conv7 in the same launch, 4 lanes per value on
//       plain FMAs - 13.7 us against 12.3 us for conv7 + out_conv + upsample as three launches.)
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ pooled operand
// ROWS > 0: the row count is a compile-time constant and a caller's loads of several values are all in flight at once (the loop
// over a run-time row count is one memory round trip per row); ROWS = 0: any row count.  Same sum order either way.
template <int ROWS>
__device__ __forceinline__ float pooled_load(const PooledSrc& s, const float* chan_base, int y, int x) {
    const float* p = chan_base + (size_t)y * s.ystride + x;
    float v = p[0];
    if (ROWS > 0) {
#pragma unroll
        for (int i = 1; i < ROWS; ++i) v += p[(size_t)i * s.rstride];
    } else {
        for (int i = 1; i < s.rows; ++i) v += p[(size_t)i * s.rstride];
    }
    return v * s.scale;
}

// Roles are picked by blockIdx.z (0-2 rconv of stage k, 3-5 correlation of stage k, 6 pooled maps) and a correlation block's tap
// by blockIdx.y, so everything a block needs from the launch arguments - its stage's source, its tap - is ONE batch of scalar
// loads issued at its first instruction, and its operand loads are the second and last round trip before the stores (see
// tail_conv_kernel in tail.hip for what a round trip costs beside other frames' kernels).
// STREAM (tail_head_stream_kernel): the pair's first image is image b + i2_off - 1 of the call, or - below 0 - the carried window;
// pairs b >= nfw (a bidirectional call) are pairs b - nfw with the two windows' roles exchanged
template <int CG, int ROWS, bool STREAM>
__device__ __forceinline__ void rconv_role(const TailHeadArgs& a, const PooledSrc* carry, int i2_off, int nfw, int k, int blk, f32x4 (*part)[64]) {
    // one block = 16 pixels x 16 couts of one (scale, sample); wave t = filter tap t (see tail_conv_kernel)
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PooledSrc src = a.src[k];
    const float* rw = a.rw[k];
    const float* rb = a.rb[k];
    float* cat = a.cat[k];
    const int gw = a.gw, gh = a.gh, cin = a.c[k];
    asm volatile("" ::"s"(src.base), "s"(src.rows), "s"(src.scale), "s"(rw), "s"(rb), "s"(cat), "s"(gw), "s"(gh), "s"(cin));
    const int g = gh * gw;
    const int ptiles = ceil_div(g, 16);
    if (blk >= ptiles * a.batch) return;
    const int b = blk / ptiles, pt = blk - b * ptiles;
    const int j = lane & 15, gq = lane >> 4;
    const int p = pt * 16 + j;
    const bool pvalid = p < g;
    const int y = p / gw, x = p - y * gw;
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    const bool valid = pvalid && yy >= 0 && yy < gh && xx >= 0 && xx < gw;
    const float* wp = rw + (size_t)t * CG * 64 + lane;
    const int i1 = !STREAM ? b : b < nfw ? b + i2_off - 1 : b - nfw + i2_off;   // (a backward pair starts at its newer window)
    const bool from_carry = STREAM && i1 < 0;
    const PooledSrc csrc = STREAM ? carry[k] : src;                         // (values, not references: no copy of the arguments in scratch)
    const float* img = from_carry ? csrc.base : src.base + (size_t)i1 * src.nstride;   // events1 half: image b
    float av[CG], bv[CG];
#pragma unroll
    for (int q = 0; q < CG; ++q) {
        const int c = q * 4 + gq;
        av[q] = wp[(size_t)q * 64];
        if (from_carry) bv[q] = (valid && c < cin) ? pooled_load<1>(csrc, img + (size_t)c * csrc.cstride, yy, xx) : 0.f;
        else bv[q] = (valid && c < cin) ? pooled_load<ROWS>(src, img + (size_t)c * src.cstride, yy, xx) : 0.f;
    }
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    if (t == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[r] = rb[gq * 4 + r];
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < CG; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], acc, 0, 0, 0);
    part[t][lane] = acc;
    __syncthreads();
    if (t != 0) return;
    acc = part[0][lane];
#pragma unroll
    for (int q = 1; q < 9; ++q) acc += part[q][lane];                       // fixed order: bitwise repeatable
    if (pvalid) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = gq * 4 + r;
            float v = acc[r] + bs[r];
            v = v > 0.f ? v : 0.1f * v;
            cat[((size_t)b * a.cat_ctotal + a.ntaps + co) * g + p] = v;
        }
    }
}

// a wave = one (sample, tap, 16-pixel tile): four adjacent lanes share one output and split its channels (see corr_kernel);
// NC = channels per lane (cin / 4): all 2 * NC * ROWS loads of a lane are issued before the first product
template <int NC, int ROWS, bool STREAM>
__device__ __forceinline__ void corr_role(const TailHeadArgs& a, const PooledSrc* carry, int i2_off, int nfw, int k) {
    const PooledSrc src = a.src[k];
    const int tap = a.tap[blockIdx.y];
    float* cat = a.cat[k];
    const int gw = a.gw, gh = a.gh, cin = a.c[k], batch = a.batch;
    asm volatile("" ::"s"(src.base), "s"(src.rows), "s"(src.scale), "s"(tap), "s"(cat), "s"(gw), "s"(gh), "s"(cin), "s"(batch));
    const int g = gh * gw;
    const int ptiles = ceil_div(g, 16);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tq = blockIdx.x * 9 + wave;
    if (tq >= ptiles * batch) return;
    const int b = tq / ptiles, pt = tq - b * ptiles;
    const int lane = threadIdx.x & 63;
    const int sub = lane & 3;
    const int p = pt * 16 + (lane >> 2);
    const bool live = p < g;
    const int y = p / gw, x = p - y * gw;
    const int yy = y + tap / 9 - 4, xx = x + tap % 9 - 4;
    float s = 0.f;
    if (live && yy >= 0 && yy < gh && xx >= 0 && xx < gw) {
        // image 2 of pair b: the events2 half of a forward, or the window after image 1 in a stream (image 1 below 0: the carry);
        // a stream's backward pair b >= nfw is forward pair b - nfw with the two windows exchanged (image 2 below 0: the carry)
        const bool bwd = STREAM && b >= nfw;
        const int newer = STREAM ? (bwd ? b - nfw : b) + i2_off : batch + b;
        const int n1 = !STREAM ? b : bwd ? newer : newer - 1;
        const int n2 = bwd ? newer - 1 : newer;
        const bool carry1 = STREAM && n1 < 0, carry2 = STREAM && n2 < 0;
        const PooledSrc csrc = STREAM ? carry[k] : src;
        const float* i1 = carry1 ? csrc.base : src.base + (size_t)n1 * src.nstride;
        const float* i2 = carry2 ? csrc.base : src.base + (size_t)n2 * src.nstride;
        if (cin == NC * 4) {
            float u[NC], v[NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                u[i] = carry1 ? pooled_load<1>(csrc, i1 + (size_t)(sub + 4 * i) * csrc.cstride, y, x)
                              : pooled_load<ROWS>(src, i1 + (size_t)(sub + 4 * i) * src.cstride, y, x);
                v[i] = carry2 ? pooled_load<1>(csrc, i2 + (size_t)(sub + 4 * i) * csrc.cstride, yy, xx)
                              : pooled_load<ROWS>(src, i2 + (size_t)(sub + 4 * i) * src.cstride, yy, xx);
            }
#pragma unroll
            for (int i = 0; i < NC; ++i) s = fmaf(u[i], v[i], s);
        } else {
            for (int c = sub; c < cin; c += 4)
                s = fmaf(carry1 ? pooled_load<1>(csrc, i1 + (size_t)c * csrc.cstride, y, x) : pooled_load<0>(src, i1 + (size_t)c * src.cstride, y, x),
                         carry2 ? pooled_load<1>(csrc, i2 + (size_t)c * csrc.cstride, yy, xx) : pooled_load<0>(src, i2 + (size_t)c * src.cstride, yy, xx), s);
        }
    }
    s = dpp_add<0xB1>(s);
    s = dpp_add<0x4E>(s);
    if (live && sub == 0) cat[((size_t)b * a.cat_ctotal + blockIdx.y) * g + p] = s / (float)cin;
}

template <bool STREAM>
__device__ __forceinline__ void tail_head_body(const TailHeadArgs& a, const PooledSrc* carry, int i2_off, int nfw, int pool_img) {
    __shared__ f32x4 part[9][64];
    const int role = blockIdx.z;
    const int blk = blockIdx.y * a.grid_x + blockIdx.x;
    if (role < 3) {
        const int rows = a.src[role].rows;                                // 16, 32, 64 input channels (EEMFlow.py:96-98)
        if (role == 0) { if (rows == 4) rconv_role<4, 4, STREAM>(a, carry, i2_off, nfw, 0, blk, part); else if (rows == 1) rconv_role<4, 1, STREAM>(a, carry, i2_off, nfw, 0, blk, part); else rconv_role<4, 0, STREAM>(a, carry, i2_off, nfw, 0, blk, part); }
        else if (role == 1) { if (rows == 2) rconv_role<8, 2, STREAM>(a, carry, i2_off, nfw, 1, blk, part); else if (rows == 1) rconv_role<8, 1, STREAM>(a, carry, i2_off, nfw, 1, blk, part); else rconv_role<8, 0, STREAM>(a, carry, i2_off, nfw, 1, blk, part); }
        else { if (rows == 1) rconv_role<16, 1, STREAM>(a, carry, i2_off, nfw, 2, blk, part); else rconv_role<16, 0, STREAM>(a, carry, i2_off, nfw, 2, blk, part); }
        return;
    }
    if (role < 6) {
        const int k = role - 3, rows = a.src[k].rows;
        if (k == 0) { if (rows == 4) corr_role<4, 4, STREAM>(a, carry, i2_off, nfw, 0); else if (rows == 1) corr_role<4, 1, STREAM>(a, carry, i2_off, nfw, 0); else corr_role<4, 0, STREAM>(a, carry, i2_off, nfw, 0); }
        else if (k == 1) { if (rows == 2) corr_role<8, 2, STREAM>(a, carry, i2_off, nfw, 1); else if (rows == 1) corr_role<8, 1, STREAM>(a, carry, i2_off, nfw, 1); else corr_role<8, 0, STREAM>(a, carry, i2_off, nfw, 1); }
        else { if (rows == 1) corr_role<16, 1, STREAM>(a, carry, i2_off, nfw, 2); else corr_role<16, 0, STREAM>(a, carry, i2_off, nfw, 2); }
        return;
    }
    // pooled maps [2B][C][gh][gw] as a side output (STREAM: image pool_img alone, [C][gh][gw])
    const int g = a.gh * a.gw;
    int idx = blk * 576 + threadIdx.x;
    for (int k = 0; k < 3; ++k) {
        const int total = (STREAM ? 1 : 2 * a.batch) * a.c[k] * g;
        if (idx < total) {
            if (a.pool_out[k] == nullptr) return;
            const int nc = idx / g;
            const int n = STREAM ? pool_img : nc / a.c[k], c = STREAM ? nc : nc - n * a.c[k];
            const int pp = idx - nc * g;
            const int y = pp / a.gw, x = pp - y * a.gw;
            const float* cb = a.src[k].base + (size_t)n * a.src[k].nstride + (size_t)c * a.src[k].cstride;
            const int rows = a.src[k].rows;
            a.pool_out[k][idx] = rows == 4 ? pooled_load<4>(a.src[k], cb, y, x) : rows == 2 ? pooled_load<2>(a.src[k], cb, y, x)
                               : rows == 1 ? pooled_load<1>(a.src[k], cb, y, x) : pooled_load<0>(a.src[k], cb, y, x);
            return;
        }
        idx -= total;
    }
}

__global__ __launch_bounds__(576) void tail_head_kernel(TailHeadArgs a) { tail_head_body<false>(a, nullptr, 0, 0, 0); }

__global__ __launch_bounds__(576) void tail_head_stream_kernel(TailHeadStreamArgs a) {
    tail_head_body<true>(a.base, a.carry, a.i2_off, a.nfw, a.pool_img);
}

// ------------------------------------------------------------------------------------------------ tail head, LDS form
// The same launch for batched calls (tail_head_lds_wanted, schedule.hip).  tail_head_kernel fetches a pooled value once per tap that
// reaches it - 128 four-byte gathers per (pixel, tap) - and a third of its grid exits at once; at ten frames per launch that is
// 6 678 blocks and 49 M lane loads for 0.5 M pooled values.  Here a block owns one (frame, stage) and either a group of THL_TG taps
// (correlation) or THL_RT pixel tiles (rconv); thread p owns cell p of the 1/64 grid.  The block walks the stage's channels in chunks
// of CH: every thread requests the partial sums of its own cell for the NEXT chunk into registers, pools the current ones by
// pooled_load's expression and puts them in LDS ([CH][THL_G] floats, 7.5 KB), and all neighbours' values - the correlation's second
// image, the rconv's B operands - come from there.  The correlation's first image is the thread's own cell and stays in registers.
// Tap group 0 also writes the finished pooled maps.  Every block has work.  131 VGPRs, no scratch.
// Measured at ten frames per launch (profiles/r07_tail_head.txt): 35.3 -> 18.1 us alone, 270 blocks for 6 678.  What is left is the
// chain of round trips - 4 / 4 / 8 chunks per stage, each waiting for its partial sums; the same time with the requests issued
// after the barriers, with 9 / 14 / 18 taps per block, with two tiles per rconv wave, and with the blocks of a (frame, stage) on one XCD.
// Bitwise tail_head_kernel: four fmaf chains over c = r (mod 4) in ascending order carried across chunks, (s0 + s1) + (s2 + s3),
// a true division by cin; the rconv's MFMA sequence per tap over ascending channel groups, taps added 0..8, bias, LeakyReLU.
constexpr int THL_G = 240;          // cells the LDS chunk is sized for (1280x720: 12 x 20)
constexpr int THL_TG = 11;          // taps per correlation block (53 taps: five blocks)
constexpr int THL_RT = 4;           // 16-pixel tiles per rconv block: one per wave
constexpr int THL_THREADS = 256;    // >= THL_G
constexpr int THL_TPW = THL_RT / (THL_THREADS / 64);

// buffer loads: the image (or the weights) as the resource, the lane's cell as the one vector offset, channel and row in the scalar
// offset - a load's address costs no vector registers, and 32 of them are in flight per thread
__device__ __forceinline__ __amdgpu_buffer_rsrc_t thl_rsrc(const float* base, int floats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, floats * 4, 0x00020000);
}
template <int CH, int ROWS>
__device__ __forceinline__ void thl_request(const PooledSrc& s, __amdgpu_buffer_rsrc_t img, int cell, int c0, float (&r)[CH * ROWS]) {
#pragma unroll
    for (int q = 0; q < CH; ++q)
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
            r[q * ROWS + i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(img, cell, ((c0 + q) * s.cstride + i * s.rstride) * 4, 0));
}
template <int ROWS>
__device__ __forceinline__ float thl_pool(const float* r, float scale) {    // pooled_load's sum order
    float v = r[0];
#pragma unroll
    for (int i = 1; i < ROWS; ++i) v += r[i];
    return v * scale;
}

template <int CIN, int CH, int ROWS>
__device__ __forceinline__ void thl_corr(const TailHeadArgs& a, int k, int b, int tg, float* lds) {
    const PooledSrc src = a.src[k];
    float* cat = a.cat[k];
    float* pool_out = tg == 0 ? a.pool_out[k] : nullptr;
    const int gw = a.gw, gh = a.gh, batch = a.batch, ntaps = a.ntaps;
    const float cinf = (float)a.c[k];
    const int g = gh * gw;
    const int p = threadIdx.x;
    const bool live = p < g;
    const int pc = live ? p : 0;                                          // idle lanes follow cell 0 and store nothing
    const int y = pc / gw, x = pc - y * gw;
    const int cell = 4 * (y * src.ystride + x);
    const __amdgpu_buffer_rsrc_t c1 = thl_rsrc(src.base + (size_t)b * src.nstride, src.nstride);
    const __amdgpu_buffer_rsrc_t c2 = thl_rsrc(src.base + (size_t)(batch + b) * src.nstride, src.nstride);
    constexpr int NR = CH * ROWS;
    float ru[NR], rv[NR];
    thl_request<CH, ROWS>(src, c1, cell, 0, ru);
    thl_request<CH, ROWS>(src, c2, cell, 0, rv);
    const int t0 = tg * THL_TG;
    int idx[THL_TG];
    unsigned ok_mask = 0;
#pragma unroll
    for (int t = 0; t < THL_TG; ++t) {
        const int tap = a.tap[t0 + t < ntaps ? t0 + t : 0];
        const int yy = y + tap / 9 - 4, xx = x + tap % 9 - 4;
        const bool ok = live && t0 + t < ntaps && yy >= 0 && yy < gh && xx >= 0 && xx < gw;
        idx[t] = ok ? yy * gw + xx : pc;                                  // an out-of-grid tap reads a cell that exists; its sum is dropped
        ok_mask |= (ok ? 1u : 0u) << t;
    }
    float acc[THL_TG][4];
#pragma unroll
    for (int t = 0; t < THL_TG; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = 0.f;
    const __amdgpu_buffer_rsrc_t po1 = thl_rsrc(pool_out ? pool_out + (size_t)b * CIN * g : nullptr, pool_out ? CIN * g : 0);
    const __amdgpu_buffer_rsrc_t po2 = thl_rsrc(pool_out ? pool_out + (size_t)(batch + b) * CIN * g : nullptr, pool_out ? CIN * g : 0);
#pragma unroll 1
    for (int c0 = 0; c0 < CIN; c0 += CH) {
        float u[CH], v[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            u[q] = thl_pool<ROWS>(ru + q * ROWS, src.scale);
            v[q] = thl_pool<ROWS>(rv + q * ROWS, src.scale);
        }
        if (c0 + CH < CIN) {                                              // in flight while this chunk is consumed
            thl_request<CH, ROWS>(src, c1, cell, c0 + CH, ru);
            thl_request<CH, ROWS>(src, c2, cell, c0 + CH, rv);
        }
        if (c0) __syncthreads();                                          // the last chunk's readers are done
        if (live) {
#pragma unroll
            for (int q = 0; q < CH; ++q) lds[q * THL_G + p] = v[q];
            if (pool_out) {
#pragma unroll
                for (int q = 0; q < CH; ++q) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(u[q]), po1, p * 4, (c0 + q) * g * 4, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), po2, p * 4, (c0 + q) * g * 4, 0);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < THL_TG; ++t)
#pragma unroll
            for (int q = 0; q < CH; ++q) acc[t][q & 3] = fmaf(u[q], lds[q * THL_G + idx[t]], acc[t][q & 3]);
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < THL_TG; ++t) {
        const float s = (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
        if (t0 + t < ntaps) cat[((size_t)b * a.cat_ctotal + t0 + t) * g + p] = ((ok_mask >> t) & 1u) ? s / cinf : 0.f;
    }
}

// wave w of rconv block rb = pixel tiles rb * THL_RT + THL_TPW w ..., all nine filter taps of each: an accumulator per (tile, tap),
// carried over the chunks
template <int CIN, int CH, int ROWS>
__device__ __forceinline__ void thl_rconv(const TailHeadArgs& a, int k, int b, int rblk, float* lds) {
    const PooledSrc src = a.src[k];
    const float* rw = a.rw[k];
    const float* rb = a.rb[k];
    float* cat = a.cat[k];
    const int gw = a.gw, gh = a.gh;
    const int g = gh * gw;
    const int p = threadIdx.x;
    const bool live = p < g;
    const int pc = live ? p : 0;
    const int y = pc / gw, x = pc - y * gw;
    const int cell = 4 * (y * src.ystride + x);
    const __amdgpu_buffer_rsrc_t c1 = thl_rsrc(src.base + (size_t)b * src.nstride, src.nstride);   // events1 half: image b
    const __amdgpu_buffer_rsrc_t wr = thl_rsrc(rw, 9 * CIN * 16);
    constexpr int NR = CH * ROWS, QN = CH / 4, CG = CIN / 4;
    float ru[NR];
    thl_request<CH, ROWS>(src, c1, cell, 0, ru);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15, gq = lane >> 4;
    float awn[QN][9];
#pragma unroll
    for (int qq = 0; qq < QN; ++qq)
#pragma unroll
        for (int t = 0; t < 9; ++t) awn[qq][t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wr, lane * 4, (t * CG + qq) * 256, 0));
    const int ptiles = ceil_div(g, 16);
    const int tile0 = rblk * THL_RT + wave * THL_TPW;
    int py[THL_TPW], px[THL_TPW], pp[THL_TPW];
    bool pv[THL_TPW];
#pragma unroll
    for (int m = 0; m < THL_TPW; ++m) {
        pp[m] = (tile0 + m) * 16 + j;
        pv[m] = tile0 + m < ptiles && pp[m] < g;
        py[m] = pp[m] / gw;
        px[m] = pp[m] - py[m] * gw;
    }
    f32x4 acc[THL_TPW][9];
#pragma unroll
    for (int m = 0; m < THL_TPW; ++m)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int c0 = 0; c0 < CIN; c0 += CH) {
        float u[CH], aw[QN][9];
#pragma unroll
        for (int q = 0; q < CH; ++q) u[q] = thl_pool<ROWS>(ru + q * ROWS, src.scale);
#pragma unroll
        for (int qq = 0; qq < QN; ++qq)
#pragma unroll
            for (int t = 0; t < 9; ++t) aw[qq][t] = awn[qq][t];
        if (c0 + CH < CIN) {
            thl_request<CH, ROWS>(src, c1, cell, c0 + CH, ru);
#pragma unroll
            for (int qq = 0; qq < QN; ++qq)
#pragma unroll
                for (int t = 0; t < 9; ++t) awn[qq][t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wr, lane * 4, (t * CG + (c0 + CH) / 4 + qq) * 256, 0));
        }
        if (c0) __syncthreads();
        if (live) {
#pragma unroll
            for (int q = 0; q < CH; ++q) lds[q * THL_G + p] = u[q];
        }
        __syncthreads();
#pragma unroll
        for (int qq = 0; qq < QN; ++qq)
#pragma unroll
            for (int m = 0; m < THL_TPW; ++m)
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int yy = py[m] + t / 3 - 1, xx = px[m] + t % 3 - 1;
                    const bool ok = pv[m] && yy >= 0 && yy < gh && xx >= 0 && xx < gw;
                    const float bv = lds[(qq * 4 + gq) * THL_G + (ok ? yy * gw + xx : 0)];
                    acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[qq][t], ok ? bv : 0.f, acc[m][t], 0, 0, 0);
                }
    }
    float bs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bs[r] = rb[gq * 4 + r];
#pragma unroll
    for (int m = 0; m < THL_TPW; ++m) {
        f32x4 s = acc[m][0];
#pragma unroll
        for (int t = 1; t < 9; ++t) s += acc[m][t];                       // tail_head_kernel's order
        if (pv[m]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = gq * 4 + r;
                float v = s[r] + bs[r];
                v = v > 0.f ? v : 0.1f * v;
                cat[((size_t)b * a.cat_ctotal + a.ntaps + co) * g + pp[m]] = v;
            }
        }
    }
}

__global__ __launch_bounds__(THL_THREADS, 3) void tail_head_lds_kernel(TailHeadArgs a) {
    __shared__ float lds[8 * THL_G];
    const int ntg = ceil_div(a.ntaps, THL_TG);
    const int per = ntg + ceil_div(ceil_div(a.gh * a.gw, 16), THL_RT);    // blocks of one (frame, stage)
    const int fs = blockIdx.x / per, r = blockIdx.x - fs * per;
    const int b = fs / 3, k = fs - 3 * b;
    if (r < ntg) {
        if (k == 0) thl_corr<16, 4, 4>(a, 0, b, r, lds);
        else if (k == 1) thl_corr<32, 8, 2>(a, 1, b, r, lds);
        else thl_corr<64, 8, 1>(a, 2, b, r, lds);
    } else {
        if (k == 0) thl_rconv<16, 4, 4>(a, 0, b, r - ntg, lds);
        else if (k == 1) thl_rconv<32, 8, 2>(a, 1, b, r - ntg, lds);
        else thl_rconv<64, 8, 1>(a, 2, b, r - ntg, lds);
    }
}

// ------------------------------------------------------------------------------------------------ conv7 + out_conv + upsample
// F.interpolate(mode='bilinear', align_corners=False): src = max(scale*(dst+0.5)-0.5, 0)   (same arithmetic as upsample_kernel)
__device__ __forceinline__ void src_index2(float scale, int dst, int in_size, int& i0, int& i1, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

__global__ __launch_bounds__(256) void tail_up_kernel(TailUpArgs a) {
    __shared__ float coarse_s[2][9];        // out_conv output at the block's <= 3x3 coarse pixels
    const int tid = threadIdx.x;
    const int txn = ceil_div(a.ow, a.tx), tyn = ceil_div(a.oh, a.ty);
    int blk = blockIdx.x;
    const int bx = blk % txn; blk /= txn;
    const int by = blk % tyn;
    const int b = blk / tyn;
    // caller's flow tensor: the argument, the graph's io table, or - eemflow_forward_many - frame b's own buffer from the table's triples
    float* __restrict__ out = a.io ? (float*)a.io[a.io_frames ? 3 * b + 2 : 2] : a.out;
    const int bo = a.io_frames ? 0 : b;                      // the sample's index inside `out`
    const int y0 = by * a.ty, x0 = bx * a.tx;
    const int y1 = min(y0 + a.ty, a.oh), x1 = min(x0 + a.tx, a.ow);
    const float sy = (float)a.gh / (float)a.oh, sx = (float)a.gw / (float)a.ow;
    int cy0, cx0, t0; float tl;
    src_index2(sy, y0, a.gh, cy0, t0, tl);
    src_index2(sx, x0, a.gw, cx0, t0, tl);
    const int g = a.gh * a.gw;
    // ---- out_conv 1x1 over the six decoder flow channels at the 3x3 coarse pixels from (cy0, cx0)
    if (tid < 18) {
        const int c = tid / 9, cp = tid - c * 9;
        const int cy = cy0 + cp / 3, cx = cx0 + cp % 3;
        float s = 0.f;
        if (cy < a.gh && cx < a.gw) {
            const float* f = a.flowcat + (size_t)b * 6 * g + cy * a.gw + cx;
            float v[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) v[m] = f[(size_t)m * g];
            s = a.bo[c];
#pragma unroll
            for (int m = 0; m < 6; ++m) s = fmaf(a.wo[c * 6 + m], v[m], s);
            if (a.coarse) a.coarse[((size_t)b * 2 + c) * g + cy * a.gw + cx] = s;   // every block that holds it writes the same value
        }
        coarse_s[c][cp] = s;
    }
    __syncthreads();
    // ---- bilinear upsample of the tile: a thread keeps one quad of columns (its four x weights are computed once) and
    // walks rows; (rows x channels) are dealt over the thread groups
    const int xq = (x1 - x0 + 3) >> 2;                       // column quads of the tile (<= 64 for tiles up to 256 wide)
    const int rows = y1 - y0;
    const bool vec = (a.ow & 3) == 0 && (a.tx & 3) == 0 && a.out_aligned16;
    const int q = tid % xq, grp = tid / xq, ngrp = 256 / xq;
    if (grp >= ngrp) return;
    int xa[4], xb[4]; float lx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ox = x0 + q * 4 + i;
        src_index2(sx, ox < a.ow ? ox : a.ow - 1, a.gw, xa[i], xb[i], lx[i]);
        xa[i] -= cx0; xb[i] -= cx0;
    }
    for (int e = grp; e < 2 * rows; e += ngrp) {
        const int c = e / rows, r = e - c * rows;
        const int oy = y0 + r;
        int ya, yb; float ly;
        src_index2(sy, oy, a.gh, ya, yb, ly);
        const float* ra = coarse_s[c] + (ya - cy0) * 3;
        const float* rb = coarse_s[c] + (yb - cy0) * 3;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float top = (1.f - lx[i]) * ra[xa[i]] + lx[i] * ra[xb[i]];
            const float bot = (1.f - lx[i]) * rb[xa[i]] + lx[i] * rb[xb[i]];
            v[i] = (1.f - ly) * top + ly * bot;
        }
        float* dst = out + (((size_t)bo * 2 + c) * a.oh + oy) * a.ow + x0 + q * 4;
        if (vec && x0 + q * 4 + 3 < x1) {
            *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + q * 4 + i < x1) dst[i] = v[i];
        }
    }
}

}  // namespace

// the launch box of the head (grid_x, filled in), its taps; pool_imgs: images of the pooled-map role
static int tail_head_prepare(TailHeadArgs& a, const int* taps_host, int pool_imgs) {
    EEM_REQUIRE(a.ntaps >= 1 && a.ntaps <= TAIL_HEAD_MAX_TAPS, "tail_head_launch: ntaps=%d", a.ntaps);
    for (int i = 0; i < a.ntaps; ++i) a.tap[i] = taps_host[i];
    const int g = a.gh * a.gw;
    const int nblk_rconv = ceil_div(g, 16) * a.batch;                     // per stage
    const int nblk_corr = ceil_div(ceil_div(g, 16) * a.batch, 9);         // per stage and tap: nine (sample, pixel tile) waves per block
    long pool_elems = 0;
    for (int k = 0; k < 3; ++k) pool_elems += (long)pool_imgs * a.c[k] * g;
    const int nblk_pool = (int)((pool_elems + 575) / 576);
    // a box of grid_x x ntaps blocks per role: correlation uses (x, tap), the other roles count it row by row
    a.grid_x = nblk_corr;
    if (ceil_div(nblk_rconv, a.ntaps) > a.grid_x) a.grid_x = ceil_div(nblk_rconv, a.ntaps);
    if (ceil_div(nblk_pool, a.ntaps) > a.grid_x) a.grid_x = ceil_div(nblk_pool, a.ntaps);
    EEM_NOTE_GRID(a.grid_x * a.ntaps * 7, 576);
    return EEM_OK;
}

int tail_head_launch(const TailHeadArgs& a0, const int* taps_host, hipStream_t stream) {
    TailHeadArgs a = a0;
    const int rc = tail_head_prepare(a, taps_host, 2 * a.batch);
    if (rc != EEM_OK) return rc;
    hipLaunchKernelGGL(tail_head_kernel, dim3(a.grid_x, a.ntaps, 7), dim3(576), 0, stream, a);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}

// the LDS form takes the fused partial sums of the three stages as the encoder's pooling epilogues leave them (rows 4 / 2 / 1 of
// 16 / 32 / 64 channels), the 53 taps, and a grid whose cells one block's threads and one LDS chunk hold
bool tail_head_lds_supported(const TailHeadArgs& a) {
    static const int kRows[3] = {4, 2, 1}, kCin[3] = {16, 32, 64};
    if (a.batch < 1 || a.gh < 1 || a.gw < 1 || a.gh * a.gw > THL_G || a.ntaps != 53) return false;
    for (int k = 0; k < 3; ++k)
        if (a.src[k].rows != kRows[k] || a.c[k] != kCin[k]) return false;
    return true;
}

int tail_head_lds_launch(const TailHeadArgs& a0, const int* taps_host, hipStream_t stream) {
    TailHeadArgs a = a0;
    EEM_REQUIRE(tail_head_lds_supported(a), "tail_head_lds_launch: batch=%d grid=%dx%d ntaps=%d rows=%d/%d/%d", a.batch, a.gh, a.gw, a.ntaps,
                a.src[0].rows, a.src[1].rows, a.src[2].rows);
    for (int i = 0; i < a.ntaps; ++i) a.tap[i] = taps_host[i];
    const int per = ceil_div(a.ntaps, THL_TG) + ceil_div(ceil_div(a.gh * a.gw, 16), THL_RT);
    const int blocks = a.batch * 3 * per;
    EEM_NOTE_GRID(blocks, THL_THREADS);
    hipLaunchKernelGGL(tail_head_lds_kernel, dim3(blocks), dim3(THL_THREADS), 0, stream, a);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}

int tail_head_stream_launch(const TailHeadStreamArgs& a0, const int* taps_host, hipStream_t stream) {
    TailHeadStreamArgs a = a0;
    EEM_REQUIRE(a.i2_off == 0 || a.i2_off == 1, "tail_head_stream_launch: i2_off=%d", a.i2_off);
    EEM_REQUIRE(a.pool_img >= 0 && a.base.batch >= 0, "tail_head_stream_launch: pool_img=%d batch=%d", a.pool_img, a.base.batch);
    EEM_REQUIRE(a.nfw == a.base.batch || 2 * a.nfw == a.base.batch, "tail_head_stream_launch: nfw=%d batch=%d", a.nfw, a.base.batch);
    for (int k = 0; k < 3; ++k) {
        EEM_REQUIRE(a.base.pool_out[k] != nullptr, "tail_head_stream_launch: stage %d has no carry output", k);
        EEM_REQUIRE(a.i2_off == 1 || (a.carry[k].base != nullptr && a.carry[k].rows == 1), "tail_head_stream_launch: stage %d: carried maps missing", k);
    }
    const int rc = tail_head_prepare(a.base, taps_host, 1);
    if (rc != EEM_OK) return rc;
    hipLaunchKernelGGL(tail_head_stream_kernel, dim3(a.base.grid_x, a.base.ntaps, 7), dim3(576), 0, stream, a);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}

bool tail_up_supported(int gh, int gw, int oh, int ow) { return oh >= 4 * gh && ow >= 4 * gw && ow / gw <= 1024; }

int tail_up_launch(const TailUpArgs& a0, hipStream_t stream) {
    TailUpArgs a = a0;
    EEM_REQUIRE(tail_up_supported(a.gh, a.gw, a.oh, a.ow), "tail_up_launch: output %dx%d too small for grid %dx%d", a.oh, a.ow, a.gh, a.gw);
    a.ty = a.oh / a.gh;                                   // a tile no taller / wider than one coarse cell: (ty - 1) * gh / oh < 1,
    a.tx = (a.ow / a.gw) & ~3;                            // so at most 3 coarse rows / columns reach it
    const int blocks = ceil_div(a.oh, a.ty) * ceil_div(a.ow, a.tx) * a.batch;
    EEM_NOTE_GRID(blocks, 256);
    hipLaunchKernelGGL(tail_up_kernel, dim3(blocks), dim3(256), 0, stream, a);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}
