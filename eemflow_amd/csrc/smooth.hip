// Edge-aware flow smoothness loss and its gradient: the regulariser beside the contrast term of the ground-truth-free training route.
// One job: a contiguous prediction pred [B][2][H][W] fp32 and an edge image img [B][C][H][W] fp32 (or none: every weight is 1).  For
// s = order in {1, 2} and each of the two axes (axis 2 = rows, the reference's `x`; axis 3 = columns), in unfused fp64
// (-ffp-contract=off) on the fp32 inputs:
//   difference  d = p[i] - p[i+1]                                  (order 1)
//               d = (p[i] - p[i+1]) - (p[i+1] - p[i+2])            (order 2, the reference's order of operations)
//   weight      g_c = constant * (img_c[i] - img_c[i+s]);  w = exp(-(sum_c f(g_c)) / C), f(g) = g * g (gauss) or |g| (exp); one weight
//               per (b, i, j), shared by both flow channels
//   error       e(d) = |d| (L1) or (|d| + 0.01)^0.4 (abs_robust)
//   loss        L = sum over axis-2 terms of e(d) * w / N2 + sum over axis-3 terms / N3,  N2 = B*2*(H-s)*W, N3 = B*2*H*(W-s)
//   gradient    dL/dp[i] = sum over the terms k that touch p[i] of c_k * q_k,  q = e'(d) * w / N_axis, c = (+1, -1) or (+1, -2, +1);
//               e'(d) = sign(d) (sign(0) = 0) or 0.4 * e(d) / (|d| + 0.01) * sign(d): one pow per term serves value and derivative
// The gradient is a GATHER: a tile of 16 x 64 cells computes the q of every term that touches it (a halo of s term rows above and s
// term columns to the left) into LDS once, then every cell reads its 2 (s + 1) terms - no atomics, so a gradient is bitwise
// reproducible; a cell is an fp64 sum, times coef, rounded to fp32 once.  The loss counts a term in the tile that holds its first
// cell, with one accumulator per axis.
//
// The tile walk, the jobs inside a tile, the partial sums and their fixed-order finish are dense_loss.h's, with its bitwise contract.
// Consecutive jobs that name the same img pointer (E-RAFT's twelve predictions, EEMFlow+'s five, all against one event volume) read
// img and take the exps once per tile.
// Planes are staged through LDS one at a time (img channel by channel, then each flow channel) with 16-byte row reads where W % 4 == 0
// and the base is 16-byte aligned; the halo columns and the ragged edge are scalar.  LDS: 40.9 KB at order 2 - three blocks per CU.
#include "dense_loss.h"

namespace {

struct SmoothJobs {
    const float* pred[DL_MAX_JOBS];
    const float* img[DL_MAX_JOBS];
    float* grad[DL_MAX_JOBS];
};

template <int S>
struct SmoothLds {
    float p[DL_TH + 2 * S][DL_TW + 2 * S];       // one plane: rows r0-S .. r0+TH+S-1, columns c0-S .. c0+TW+S-1, zero outside the frame
    double w2[(DL_TH + S) * DL_TW];              // axis-2 terms: rows r0-S .. r0+TH-1
    double w3[DL_TH * (DL_TW + S)];              // axis-3 terms: columns c0-S .. c0+TW-1
    double q2[(DL_TH + S) * DL_TW];
    double q3[DL_TH * (DL_TW + S)];
    DenseSlots<2> part;                          // loss sums per job and wave: {axis 2, axis 3}
};

template <int S>
__device__ __forceinline__ void load_plane(float (*sp)[DL_TW + 2 * S], const float* __restrict__ plane, int r0, int c0, int H, int W,
                                           bool vec, int tid) {
    constexpr int R = DL_TH + 2 * S;
    for (int idx = tid; idx < R * (DL_TW / 4); idx += DL_NT) {
        const int lr = idx / (DL_TW / 4), v = idx % (DL_TW / 4);
        const int r = r0 - S + lr, c = c0 + 4 * v;
        float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f;
        if (r >= 0 && r < H && c < W) {
            const float* src = plane + (size_t)r * W + c;
            if (vec && c + 3 < W) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(src);
                x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
            } else {
                x0 = src[0];
                if (c + 1 < W) x1 = src[1];
                if (c + 2 < W) x2 = src[2];
                if (c + 3 < W) x3 = src[3];
            }
        }
        float* d = &sp[lr][S + 4 * v];
        d[0] = x0, d[1] = x1, d[2] = x2, d[3] = x3;
    }
    for (int idx = tid; idx < R * 2 * S; idx += DL_NT) {
        const int lr = idx / (2 * S), hc = idx % (2 * S);
        const int lc = hc < S ? hc : DL_TW + hc;
        const int r = r0 - S + lr, c = c0 - S + lc;
        sp[lr][lc] = (r >= 0 && r < H && c >= 0 && c < W) ? plane[(size_t)r * W + c] : 0.0f;
    }
}

template <int S>
__device__ __forceinline__ double diff(float a, float b, float c) {
    if (S == 1) return (double)a - (double)b;
    return ((double)a - (double)b) - ((double)b - (double)c);
}

// e(d) and (with GRAD) e'(d)
template <int ERR>
__device__ __forceinline__ void error_term(double d, bool grad, double& e, double& de) {
    const double a = fabs(d);
    const double sg = (double)((d > 0.0) - (d < 0.0));
    de = 0.0;
    if (ERR == 0) {
        e = a;
        if (grad) de = sg;
    } else {
        const double b = a + 0.01;
        e = pow(b, 0.4);
        if (grad) de = 0.4 * e / b * sg;
    }
}

template <int S, int ERR>
__global__ __launch_bounds__(DL_NT) void smooth_kernel(SmoothJobs jobs, int k, int B, int C, int H, int W, int weight_type, double constant,
                                                       const double* __restrict__ coef, double* __restrict__ scratch, int want_loss,
                                                       int tiles_x, int tiles_y) {
    __shared__ SmoothLds<S> L;
    const int tid = threadIdx.x;
    constexpr int N2S = (DL_TH + S) * DL_TW, N3S = DL_TH * (DL_TW + S);
    constexpr int W3 = DL_TW + S;
    const double N2 = (double)B * 2.0 * (double)(H - S) * (double)W, N3 = (double)B * 2.0 * (double)H * (double)(W - S);
    const size_t hw = (size_t)H * W;
    const bool w4 = (W & 3) == 0;
    dense_slots_zero(L.part, tid);                             // (every job's first barrier stands before the first add)
    const long tiles = dense_tiles(B, tiles_x, tiles_y);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const auto [b, r0, c0] = dense_tile(tile, tiles_x, tiles_y);
        const float* cur = nullptr;
        bool have = false;
        for (int job = 0; job < k; ++job) {
            const float* img = jobs.img[job];
            if (!have || img != cur) {
                // ---- the weights of this tile's terms: once per run of jobs that share img
                have = true;
                cur = img;
                if (!img) {
                    __syncthreads();
                    for (int idx = tid; idx < N2S; idx += DL_NT) L.w2[idx] = 1.0;
                    for (int idx = tid; idx < N3S; idx += DL_NT) L.w3[idx] = 1.0;
                } else {
                    const bool vec = w4 && (reinterpret_cast<uintptr_t>(img) & 15) == 0;
                    for (int c = 0; c < C; ++c) {
                        __syncthreads();
                        load_plane<S>(L.p, img + ((size_t)b * C + c) * hw, r0, c0, H, W, vec, tid);
                        __syncthreads();
                        // every slot belongs to one thread for the whole phase (idx = tid + n * 256)
                        for (int idx = tid; idx < N2S; idx += DL_NT) {
                            const int lt = idx / DL_TW, lj = idx % DL_TW;
                            const double g = constant * ((double)L.p[lt][lj + S] - (double)L.p[lt + S][lj + S]);
                            const double f = weight_type == 0 ? g * g : fabs(g);
                            L.w2[idx] = c == 0 ? f : L.w2[idx] + f;
                        }
                        for (int idx = tid; idx < N3S; idx += DL_NT) {
                            const int li = idx / W3, lu = idx % W3;
                            const double g = constant * ((double)L.p[li + S][lu] - (double)L.p[li + S][lu + S]);
                            const double f = weight_type == 0 ? g * g : fabs(g);
                            L.w3[idx] = c == 0 ? f : L.w3[idx] + f;
                        }
                    }
                    for (int idx = tid; idx < N2S; idx += DL_NT) L.w2[idx] = exp(-(L.w2[idx] / (double)C));
                    for (int idx = tid; idx < N3S; idx += DL_NT) L.w3[idx] = exp(-(L.w3[idx] / (double)C));
                }
            }
            const float* pred = jobs.pred[job];
            float* grad = jobs.grad[job];
            const bool want_grad = grad != nullptr;
            const bool vec_p = w4 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0;
            const bool vec_g = w4 && (reinterpret_cast<uintptr_t>(grad) & 15) == 0;
            const double cf = want_grad && coef ? coef[job] : 1.0;
            double acc2 = 0.0, acc3 = 0.0;
            for (int ch = 0; ch < 2; ++ch) {
                const size_t plane = ((size_t)b * 2 + ch) * hw;
                __syncthreads();
                load_plane<S>(L.p, pred + plane, r0, c0, H, W, vec_p, tid);
                __syncthreads();
                for (int idx = tid; idx < N2S; idx += DL_NT) {
                    const int lt = idx / DL_TW, lj = idx % DL_TW;
                    const int t = r0 - S + lt, j = c0 + lj;
                    double q = 0.0;
                    if (t >= 0 && t < H - S && j < W) {
                        const double d = diff<S>(L.p[lt][lj + S], L.p[lt + 1][lj + S], L.p[lt + S][lj + S]);
                        const double w = L.w2[idx];
                        double e, de;
                        error_term<ERR>(d, want_grad, e, de);
                        if (lt >= S) acc2 += e * w;                // the term's first cell lies in this tile
                        q = de * w / N2;
                    }
                    if (want_grad) L.q2[idx] = q;
                }
                for (int idx = tid; idx < N3S; idx += DL_NT) {
                    const int li = idx / W3, lu = idx % W3;
                    const int i = r0 + li, u = c0 - S + lu;
                    double q = 0.0;
                    if (i < H && u >= 0 && u < W - S) {
                        const double d = diff<S>(L.p[li + S][lu], L.p[li + S][lu + 1], L.p[li + S][lu + S]);
                        const double w = L.w3[idx];
                        double e, de;
                        error_term<ERR>(d, want_grad, e, de);
                        if (lu >= S) acc3 += e * w;
                        q = de * w / N3;
                    }
                    if (want_grad) L.q3[idx] = q;
                }
                if (!want_grad) continue;
                __syncthreads();
                // ---- gather: the 2 (S + 1) terms of every cell, axis 2 then axis 3, nearest term first
                const int li = tid / (DL_TW / 4), v = tid % (DL_TW / 4);
                const int i = r0 + li, j = c0 + 4 * v;
                if (i >= H || j >= W) continue;
                float out[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int lj = 4 * v + u;
                    double g = 0.0;
#pragma unroll
                    for (int kk = 0; kk <= S; ++kk) {
                        const double ck = (S == 2 && kk == 1) ? -2.0 : (kk == 0 || kk == 2) ? 1.0 : -1.0;
                        g += ck * L.q2[(li + S - kk) * DL_TW + lj];
                    }
#pragma unroll
                    for (int kk = 0; kk <= S; ++kk) {
                        const double ck = (S == 2 && kk == 1) ? -2.0 : (kk == 0 || kk == 2) ? 1.0 : -1.0;
                        g += ck * L.q3[li * W3 + lj + S - kk];
                    }
                    out[u] = (float)(cf * g);
                }
                float* dst = grad + plane + (size_t)i * W + j;
                if (vec_g && j + 3 < W) {
                    f32x4 o;
                    o[0] = out[0], o[1] = out[1], o[2] = out[2], o[3] = out[3];
                    *reinterpret_cast<f32x4*>(dst) = o;
                } else {
                    dst[0] = out[0];
                    if (j + 1 < W) dst[1] = out[1];
                    if (j + 2 < W) dst[2] = out[2];
                    if (j + 3 < W) dst[3] = out[3];
                }
            }
            if (want_loss) dense_slots_add(L.part, tid, job, acc2, acc3);
        }
    }
    if (!want_loss) return;
    __syncthreads();
    dense_slots_write(L.part, tid, k, scratch);
}

// one wave per job: the blocks' partial sums in a fixed order, then L = sum2 / N2 + sum3 / N3
__global__ __launch_bounds__(64) void smooth_finish_kernel(const double* __restrict__ scratch, int nblk, double N2, double N3,
                                                           double* __restrict__ loss) {
    const int job = blockIdx.x, lane = threadIdx.x;
    const double* p = scratch + (size_t)job * nblk * 2;
    double s2 = 0.0, s3 = 0.0;
    for (int i = lane; i < nblk; i += 64) {
        s2 += p[2 * i];
        s3 += p[2 * i + 1];
    }
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    if (lane == 0) loss[job] = s2 / N2 + s3 / N3;
}

}  // namespace

extern "C" size_t eemflow_smoothness_scratch_doubles(int k, int B, int H, int W) { return dense_scratch_doubles(k, B, H, W, 0, 2); }

extern "C" int eemflow_smoothness_many(int k, const float* const* pred, const float* const* img, int B, int C, int H, int W, int order,
                                       int weight_type, int error_type, double constant, const double* coef, double* loss,
                                       float* const* grad, double* scratch, void* stream_) {
    EEM_REQUIRE(k >= 1 && k <= DL_MAX_JOBS, "eemflow_smoothness_many: 1..%d jobs per call; got %d", DL_MAX_JOBS, k);
    EEM_REQUIRE(order == 1 || order == 2, "eemflow_smoothness_many: order is 1 or 2; got %d", order);
    EEM_REQUIRE(weight_type == 0 || weight_type == 1, "eemflow_smoothness_many: weight_type is 0 (gauss) or 1 (exp); got %d", weight_type);
    EEM_REQUIRE(error_type == 0 || error_type == 1, "eemflow_smoothness_many: error_type is 0 (L1) or 1 (abs_robust); got %d", error_type);
    EEM_REQUIRE(dense_shape_ok(B, H, W), "eemflow_smoothness_many: bad shape B=%d H=%d W=%d", B, H, W);
    EEM_REQUIRE(H > order && W > order, "eemflow_smoothness_many: order %d needs H > %d and W > %d (the mean of no terms); got %dx%d", order,
                order, order, H, W);
    EEM_REQUIRE(pred, "eemflow_smoothness_many: pred is NULL");
    EEM_REQUIRE(loss || grad, "eemflow_smoothness_many: neither loss nor grad is asked for");
    EEM_REQUIRE(!loss || scratch, "eemflow_smoothness_many: the loss needs scratch (eemflow_smoothness_scratch_doubles)");
    SmoothJobs jobs;
    bool any_img = false;
    for (int i = 0; i < DL_MAX_JOBS; ++i) jobs.pred[i] = jobs.img[i] = nullptr, jobs.grad[i] = nullptr;
    for (int i = 0; i < k; ++i) {
        EEM_REQUIRE(pred[i], "eemflow_smoothness_many: job %d has no prediction", i);
        EEM_REQUIRE(!grad || grad[i], "eemflow_smoothness_many: job %d has no gradient buffer", i);
        jobs.pred[i] = pred[i];
        jobs.img[i] = img ? img[i] : nullptr;
        jobs.grad[i] = grad ? grad[i] : nullptr;
        any_img = any_img || jobs.img[i];
    }
    EEM_REQUIRE(!any_img || (C >= 1 && (long)B * C * H * W <= (1L << 34)), "eemflow_smoothness_many: bad channel count C=%d", C);
    hipStream_t stream = (hipStream_t)stream_;
    int tx, ty;
    const int nblk = dense_blocks(B, H, W, &tx, &ty);
    const int wl = loss ? 1 : 0;
#define EEM_SMOOTH_LAUNCH(S, E)                                                                                                       \
    hipLaunchKernelGGL((smooth_kernel<S, E>), dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, B, C, H, W, weight_type, constant, coef, scratch, \
                       wl, tx, ty)
    if (order == 1) {
        if (error_type == 0) EEM_SMOOTH_LAUNCH(1, 0); else EEM_SMOOTH_LAUNCH(1, 1);
    } else {
        if (error_type == 0) EEM_SMOOTH_LAUNCH(2, 0); else EEM_SMOOTH_LAUNCH(2, 1);
    }
#undef EEM_SMOOTH_LAUNCH
    EEM_HIP_CHECK(hipGetLastError());
    if (loss) {
        const double N2 = (double)B * 2.0 * (double)(H - order) * (double)W, N3 = (double)B * 2.0 * (double)H * (double)(W - order);
        hipLaunchKernelGGL(smooth_finish_kernel, dim3(k), dim3(64), 0, stream, scratch, nblk, N2, N3, loss);
        EEM_HIP_CHECK(hipGetLastError());
    }
    return EEM_OK;
}
