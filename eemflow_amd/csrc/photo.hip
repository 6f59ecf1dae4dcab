// Photometric and census warp losses and their gradient with respect to the flow: the data term of the ground-truth-free training
// route, beside the contrast term (iwe.hip) and the smoothness term (smooth.hip).
// One job: a flow [B][2][H][W], img1 and img2 [B][C][H][W], an optional mask [B][1][H][W], all contiguous fp32.
//   warp      Yw_c(p) = grid_sample(img2_c, p + flow(p)): warp_px.h mode 1 in fp32 - the value eemplus_warp(mode 1) and the
//             forward-backward check see, bit for bit.  Everything below is unfused fp64 (-ffp-contract=off) on those fp32 values.
//   pointwise d = img1 - Yw;  l = (|d| + 0.01)^0.4 (abs_robust), (d*d + 1e-6)^0.4 (charbonnier) or |d + 1e-6| (L1);
//             L = sum(l) / (B*C*H*W), or with use_occ sum(l * mask) / (sum(mask) + 1e-6)
//   census    g(I) = sum_c gray[c] * I_c, 0 outside the frame;  x_k(p) = g(p+k) - g(p) over the (2r+1)^2 offsets;  t = x / sqrt(0.81 + x*x);
//             e = (t_k(img1) - t_k(Yw))^2;  dist(p) = sum_k e / (0.1 + e);  rho(dist) = (dist^2 + eps)^q or (|dist| + 0.01)^q;
//             L = (sum(rho * mask') / n1) / D with the reference's four (n1, D) pairs (photo_den_kernel)
//   gradient  dL/dflow(p) = sum_c dL/dYw_c(p) * dYw_c/d(ix, iy)(p) * d(ix, iy)/d(u, v):  the derivative of the bilinear blend at the fp32
//             tap weights (corners outside the frame are zeros), as ATen's grid sampler backward; d ix/du = (W/2) * (2/max(W-1,1)).
// Census gradient.  With s(p,k) = d(e/(0.1+e))/dg2(p+k) = 0.1/(0.1+e)^2 * (-2 (t1 - t2)) * 0.81/(0.81 + x2^2)^1.5 and the per-centre factor
// F(p) = rho'(dist(p)) * mask'(p) * coef / (n1 D), cell m receives sum_k F(m-k) s(m-k,k) as a patch member and -F(m) sum_k s(m,k) as
// a centre.  x2(m-k, k) = -x2(m, -k) exactly, and every step from x to s is odd or even in x, so s(m-k,k) = -s(m,-k) bit for bit:
//   dL/dg2(m) = -sum_{k != 0} s(m,k) * (F(m) + F(m+k)),   F = 0 outside the frame
// - one stencil pass over m's own taps that GATHERS the neighbours' factors from an LDS plane: no atomics anywhere.  F needs dist on
// the tile plus r of halo, hence g on 2r of halo.  dL/dYw_c = gray[c] * dL/dg2, so the warp derivative is grey-combined with g2 in the
// staging pass and kept in registers (a thread owns the same four cells in every phase).
// The tile walk, the jobs inside a tile, the partial sums and their fixed-order finish are dense_loss.h's, with its bitwise contract;
// consecutive jobs that name one img1 pointer grey-combine it once.
// LDS (census): two g planes of 28 x 76 doubles and the factor plane of 22 x 70: 46.9 KB, static.
// What bounds it: census is bound by the fp64 sqrt and divides of its taps (two sqrt and three divides per tap in the distance pass, one
// more sqrt and two more divides in the gradient's pass); abs_robust and charbonnier by one fp64 pow per element; L1 by the four
// gathers per channel of the warp.
#include "dense_loss.h"
#include "warp_px.h"

namespace {

constexpr int PH_RMAX = 3;
constexpr int PH_GO = 2 * PH_RMAX, PH_GH = DL_TH + 2 * PH_GO, PH_GW = DL_TW + 2 * PH_GO;      // g planes: origin (r0 - 6, c0 - 6)
constexpr int PH_FO = PH_RMAX, PH_FH = DL_TH + 2 * PH_FO, PH_FW = DL_TW + 2 * PH_FO;          // factor plane: origin (r0 - 3, c0 - 3)
enum { PH_ABS_ROBUST = 0, PH_CHARBONNIER = 1, PH_L1 = 2, PH_CENSUS = 3 };

__device__ __forceinline__ double gray_of(const double* __restrict__ gray, int c, int C) {
    if (gray) return gray[c];
    if (C == 3) return c == 0 ? 0.2989 : c == 1 ? 0.5870 : 0.1140;
    return 1.0 / (double)C;
}

// ---- sums of the masks (use_occ): block partial sums of mask * [rin <= y < H - rin, rin <= x < W - rin] per job
__global__ __launch_bounds__(DL_NT) void photo_mask_kernel(DenseJobs jobs, int k, DenseShape s, int rin, double* __restrict__ part) {
    __shared__ alignas(16) DenseSlots<1> lp;
    const int tid = threadIdx.x;
    const size_t hw = (size_t)s.H * s.W;
    dense_slots_zero(lp, tid);
    __syncthreads();
    const long tiles = dense_tiles(s.B, s.tiles_x, s.tiles_y);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const auto [b, r0, c0] = dense_tile(tile, s.tiles_x, s.tiles_y);
        for (int job = 0; job < k; ++job) {
            const float* mask = jobs.mask[job];
            double acc = 0.0;
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) {
                const int y = r0 + dense_cell_row(tid, n), x = c0 + dense_cell_col(tid);
                if (y < s.H && x < s.W && y >= rin && y < s.H - rin && x >= rin && x < s.W - rin)
                    acc += mask ? (double)mask[(size_t)b * hw + (size_t)y * s.W + x] : 1.0;
            }
            dense_slots_add(lp, tid, job, acc);
        }
    }
    __syncthreads();
    dense_slots_write(lp, tid, k, part);
}

// one wave per job: den[job] = D.  mode 0: 1;  1: M + 1e-6;  2: M * 2 + 1e-6;  3: (M / n) * 2 + 1e-6
__global__ __launch_bounds__(64) void photo_den_kernel(const double* __restrict__ part, int nblk, int mode, double n, double* __restrict__ den) {
    const int job = blockIdx.x, lane = threadIdx.x;
    double m = 0.0;
    if (mode != 0) {
        for (int i = lane; i < nblk; i += 64) m += part[(size_t)job * nblk + i];
        m = wave_sum(m);
    }
    if (lane == 0) den[job] = mode == 0 ? 1.0 : mode == 1 ? m + 1e-6 : mode == 2 ? m * 2.0 + 1e-6 : (m / n) * 2.0 + 1e-6;
}

// ---- the pointwise kinds: no neighbours, no LDS but the loss sums
template <int KIND>
__global__ __launch_bounds__(DL_NT) void photo_point_kernel(DenseJobs jobs, int k, DenseShape s, int use_occ, const double* __restrict__ coef,
                                                            const double* __restrict__ den, double* __restrict__ part, int want_loss) {
    __shared__ alignas(16) DenseSlots<1> lp;
    const int tid = threadIdx.x;
    const size_t hw = (size_t)s.H * s.W;
    dense_slots_zero(lp, tid);
    __syncthreads();
    const long tiles = dense_tiles(s.B, s.tiles_x, s.tiles_y);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const auto [b, r0, c0] = dense_tile(tile, s.tiles_x, s.tiles_y);
        for (int job = 0; job < k; ++job) {
            const float* flow = jobs.flow[job] + (size_t)b * 2 * hw;
            const float* img1 = jobs.img1[job] + (size_t)b * s.C * hw;
            const float* img2 = jobs.img2[job] + (size_t)b * s.C * hw;
            const float* mask = use_occ ? jobs.mask[job] : nullptr;
            float* grad = jobs.grad[job];
            const double sc = grad ? ((coef ? coef[job] : 1.0) / s.n1) / den[job] : 0.0;
            double acc = 0.0;
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) {
                const int y = r0 + dense_cell_row(tid, n), x = c0 + dense_cell_col(tid);
                if (y >= s.H || x >= s.W) continue;
                const int p = y * s.W + x;
                const WarpTaps t = warp_taps(flow[p], flow[hw + p], s.H, s.W, p, 1);
                const double m = mask ? (double)mask[(size_t)b * hw + p] : 1.0;
                double gu = 0.0, gv = 0.0;
                for (int c = 0; c < s.C; ++c) {
                    float v[4];
                    warp_gather(img2 + (size_t)c * hw, t, v);
                    const double d = (double)img1[(size_t)c * hw + p] - (double)warp_sum(v, t);
                    double l, dl;                                   // l(d) and dl/dd
                    if (KIND == PH_ABS_ROBUST) {
                        const double a = fabs(d) + 0.01;
                        l = pow(a, 0.4);
                        dl = 0.4 * l / a * (double)((d > 0.0) - (d < 0.0));
                    } else if (KIND == PH_CHARBONNIER) {
                        const double a = d * d + 1e-6;
                        l = pow(a, 0.4);
                        dl = 0.4 * l / a * (2.0 * d);
                    } else {
                        const double a = d + 1e-6;
                        l = fabs(a);
                        dl = (double)((a > 0.0) - (a < 0.0));
                    }
                    acc += use_occ ? l * m : l;
                    if (grad) {
                        double dx, dy;
                        blend_grad(v, t, dx, dy);
                        const double gy = -(dl * m * sc);           // dL/dYw_c
                        gu += gy * dx;
                        gv += gy * dy;
                    }
                }
                if (grad) {
                    grad[(size_t)b * 2 * hw + p] = (float)(gu * s.sx);
                    grad[(size_t)b * 2 * hw + hw + p] = (float)(gv * s.sy);
                }
            }
            if (want_loss) dense_slots_add(lp, tid, job, acc);
        }
    }
    if (!want_loss) return;
    __syncthreads();
    dense_slots_write(lp, tid, k, part);
}

// ---- census
struct CensusLds {
    double g1[PH_GH * PH_GW];
    double g2[PH_GH * PH_GW];
    double f[PH_FH * PH_FW];
    DenseSlots<1> part;
};

struct CensusTap {
    double df, e, x2;
};

__device__ __forceinline__ CensusTap census_tap(double x1, double x2) {
    const double t1 = x1 / sqrt(0.81 + x1 * x1);
    const double t2 = x2 / sqrt(0.81 + x2 * x2);
    CensusTap t;
    t.df = t1 - t2;
    t.e = t.df * t.df;
    t.x2 = x2;
    return t;
}

template <int CHARB>
__global__ __launch_bounds__(DL_NT) void photo_census_kernel(DenseJobs jobs, int k, DenseShape s, int r, int use_occ, double q, double eps,
                                                             const double* __restrict__ gray, const double* __restrict__ coef,
                                                             const double* __restrict__ den, double* __restrict__ part, int want_loss) {
    __shared__ CensusLds L;
    const int tid = threadIdx.x;
    const int H = s.H, W = s.W, C = s.C;
    const size_t hw = (size_t)H * W;
    dense_slots_zero(L.part, tid);                             // (the job loop's first barrier stands before the first add)
    const long tiles = dense_tiles(s.B, s.tiles_x, s.tiles_y);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const DenseTile at = dense_tile(tile, s.tiles_x, s.tiles_y);
        const int b = at.b, r0 = at.r0, c0 = at.c0;            // (named: the lambdas below capture them)
        const float* cur1 = nullptr;
        for (int job = 0; job < k; ++job) {
            const float* flow = jobs.flow[job] + (size_t)b * 2 * hw;
            const float* img1 = jobs.img1[job] + (size_t)b * C * hw;
            const float* img2 = jobs.img2[job] + (size_t)b * C * hw;
            const float* mask = use_occ ? jobs.mask[job] : nullptr;
            float* grad = jobs.grad[job];
            const bool want_grad = grad != nullptr;
            const bool new1 = job == 0 || jobs.img1[job] != cur1;
            cur1 = jobs.img1[job];
            const double sc = want_grad ? ((coef ? coef[job] : 1.0) / s.n1) / den[job] : 0.0;
            const int hg = want_grad ? 2 * r : r;              // halo of the g planes
            double gx[DL_CELLS], gy[DL_CELLS];                 // sum_c gray[c] * dYw_c/d(ix, iy) of this thread's cells
            __syncthreads();                                   // the job (or tile) before has read the planes
            // ---- stage g1 and g2: the tile's cells by their owners, then the halo
            auto stage = [&](int y, int x, double& dxs, double& dys) {
                const int li = (y - r0 + PH_GO) * PH_GW + (x - c0 + PH_GO);
                double a1 = 0.0, a2 = 0.0;
                dxs = 0.0, dys = 0.0;
                if (y >= 0 && y < H && x >= 0 && x < W) {
                    const int p = y * W + x;
                    const WarpTaps t = warp_taps(flow[p], flow[hw + p], H, W, p, 1);
                    for (int c = 0; c < C; ++c) {
                        const double gc = gray_of(gray, c, C);
                        float v[4];
                        warp_gather(img2 + (size_t)c * hw, t, v);
                        a2 += gc * (double)warp_sum(v, t);
                        if (new1) a1 += gc * (double)img1[(size_t)c * hw + p];
                        if (want_grad) {
                            double dx, dy;
                            blend_grad(v, t, dx, dy);
                            dxs += gc * dx;
                            dys += gc * dy;
                        }
                    }
                }
                L.g2[li] = a2;
                if (new1) L.g1[li] = a1;
            };
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) stage(r0 + dense_cell_row(tid, n), c0 + dense_cell_col(tid), gx[n], gy[n]);
            {
                const int rw = DL_TW + 2 * hg, cells = (DL_TH + 2 * hg) * rw;
                for (int idx = tid; idx < cells; idx += DL_NT) {
                    const int ly = idx / rw - hg, lx = idx % rw - hg;
                    if (ly >= 0 && ly < DL_TH && lx >= 0 && lx < DL_TW) continue;
                    double u0, u1;
                    stage(r0 + ly, c0 + lx, u0, u1);
                }
            }
            __syncthreads();
            // ---- dist, rho and the factor F of every centre: the tile's cells (their rho goes into the loss), then r of halo
            auto centre = [&](int y, int x, double& term) {
                term = 0.0;
                double fac = 0.0;
                if (y >= 0 && y < H && x >= 0 && x < W) {
                    const int li = (y - r0 + PH_GO) * PH_GW + (x - c0 + PH_GO);
                    const double c1 = L.g1[li], c2 = L.g2[li];
                    double dist = 0.0;
                    for (int dy = -r; dy <= r; ++dy)
                        for (int dx = -r; dx <= r; ++dx) {
                            if (dy == 0 && dx == 0) continue;
                            const int lk = li + dy * PH_GW + dx;
                            const CensusTap t = census_tap(L.g1[lk] - c1, L.g2[lk] - c2);
                            dist += t.e / (0.1 + t.e);
                        }
                    double rho, drho;
                    if (CHARB) {
                        const double a = dist * dist + eps;
                        rho = pow(a, q);
                        drho = q * rho / a * (2.0 * dist);
                    } else {
                        const double a = fabs(dist) + 0.01;
                        rho = pow(a, q);
                        drho = q * rho / a * (double)((dist > 0.0) - (dist < 0.0));
                    }
                    double m = 1.0;
                    if (use_occ) {
                        const bool inner = y >= r && y < H - r && x >= r && x < W - r;
                        m = inner ? (mask ? (double)mask[(size_t)b * hw + (size_t)y * W + x] : 1.0) : 0.0;
                    }
                    term = use_occ ? rho * m : rho;
                    fac = drho * m * sc;
                }
                if (want_grad) L.f[(y - r0 + PH_FO) * PH_FW + (x - c0 + PH_FO)] = fac;
            };
            double acc = 0.0;
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) {
                double term;
                centre(r0 + dense_cell_row(tid, n), c0 + dense_cell_col(tid), term);
                acc += term;
            }
            if (want_loss) dense_slots_add(L.part, tid, job, acc);
            if (!want_grad) continue;                          // block-uniform
            {
                const int rw = DL_TW + 2 * r, cells = (DL_TH + 2 * r) * rw;
                for (int idx = tid; idx < cells; idx += DL_NT) {
                    const int ly = idx / rw - r, lx = idx % rw - r;
                    if (ly >= 0 && ly < DL_TH && lx >= 0 && lx < DL_TW) continue;
                    double term;
                    centre(r0 + ly, c0 + lx, term);
                }
            }
            __syncthreads();
            // ---- gather: dL/dg2(m) = -sum_k s(m,k) * (F(m) + F(m+k)), then the warp derivative
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) {
                const int ly = dense_cell_row(tid, n), lx = dense_cell_col(tid);
                const int y = r0 + ly, x = c0 + lx;
                if (y >= H || x >= W) continue;
                const int li = (ly + PH_GO) * PH_GW + (lx + PH_GO), fi = (ly + PH_FO) * PH_FW + (lx + PH_FO);
                const double c1 = L.g1[li], c2 = L.g2[li], fm = L.f[fi];
                double a = 0.0;
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        if (dy == 0 && dx == 0) continue;
                        const int lk = li + dy * PH_GW + dx;
                        const CensusTap t = census_tap(L.g1[lk] - c1, L.g2[lk] - c2);
                        const double de = 0.1 + t.e, u2 = 0.81 + t.x2 * t.x2;
                        const double sk = (0.1 / (de * de)) * (-2.0 * t.df) * (0.81 / (u2 * sqrt(u2)));
                        a += sk * (fm + L.f[fi + dy * PH_FW + dx]);
                    }
                const double dg = -a;
                const size_t p = (size_t)y * W + x;
                grad[(size_t)b * 2 * hw + p] = (float)((dg * gx[n]) * s.sx);
                grad[(size_t)b * 2 * hw + hw + p] = (float)((dg * gy[n]) * s.sy);
            }
        }
    }
    if (!want_loss) return;
    __syncthreads();
    dense_slots_write(L.part, tid, k, part);
}

}  // namespace

extern "C" size_t eemflow_photo_scratch_doubles(int k, int B, int H, int W) { return dense_scratch_doubles(k, B, H, W, DL_MAX_JOBS, 1); }

extern "C" int eemflow_photo_many(int k, const float* const* flow, const float* const* img1, const float* const* img2,
                                  const float* const* mask, int B, int C, int H, int W, int kind, int use_occ, int charbonnier, int average,
                                  int max_distance, double q, const double* gray, const double* coef, double* loss, float* const* grad,
                                  double* scratch, void* stream_) {
    EEM_REQUIRE(k >= 1 && k <= DL_MAX_JOBS, "eemflow_photo_many: 1..%d jobs per call; got %d", DL_MAX_JOBS, k);
    EEM_REQUIRE(kind >= PH_ABS_ROBUST && kind <= PH_CENSUS,
                "eemflow_photo_many: kind is 0 (abs_robust), 1 (charbonnier), 2 (L1) or 3 (census); got %d", kind);
    EEM_REQUIRE(dense_shape_ok(B, H, W), "eemflow_photo_many: bad shape B=%d H=%d W=%d", B, H, W);
    EEM_REQUIRE(C >= 1 && (long)B * C * H * W <= (1L << 34), "eemflow_photo_many: bad channel count C=%d", C);
    const int r = max_distance;
    if (kind == PH_CENSUS) {
        EEM_REQUIRE(r >= 1 && r <= PH_RMAX, "eemflow_photo_many: census max_distance is 1..%d; got %d", PH_RMAX, r);
        EEM_REQUIRE(H > 2 * r && W > 2 * r, "eemflow_photo_many: census with max_distance %d needs H > %d and W > %d; got %dx%d", r, 2 * r,
                    2 * r, H, W);
    }
    EEM_REQUIRE(loss || grad, "eemflow_photo_many: neither loss nor grad is asked for");
    EEM_REQUIRE(scratch, "eemflow_photo_many: scratch is NULL (eemflow_photo_scratch_doubles)");
    DenseJobs jobs;
    if (const int rc = dense_fill_jobs(jobs, "eemflow_photo_many", k, flow, img1, img2, mask, grad)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    DenseShape s;
    const int nblk = dense_shape(s, B, C, H, W);
    const double n = (double)B * (double)H * (double)W;
    int den_mode;
    if (kind != PH_CENSUS) {
        den_mode = use_occ ? 1 : 0;
        s.n1 = use_occ ? 1.0 : n * (double)C;
    } else if (use_occ) {
        den_mode = charbonnier && average ? 3 : 2;
        s.n1 = charbonnier && average ? n : 1.0;
    } else {
        den_mode = 0;
        s.n1 = average ? n : 1.0;
    }
    double* den = scratch;
    double* part = scratch + DL_MAX_JOBS;
    if (den_mode != 0) {
        hipLaunchKernelGGL(photo_mask_kernel, dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, kind == PH_CENSUS ? r : 0, part);
        EEM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(photo_den_kernel, dim3(k), dim3(64), 0, stream, part, nblk, den_mode, n, den);
    EEM_HIP_CHECK(hipGetLastError());
    const int wl = loss ? 1 : 0, uo = use_occ ? 1 : 0;
    if (kind == PH_ABS_ROBUST)
        hipLaunchKernelGGL((photo_point_kernel<PH_ABS_ROBUST>), dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, uo, coef, den, part, wl);
    else if (kind == PH_CHARBONNIER)
        hipLaunchKernelGGL((photo_point_kernel<PH_CHARBONNIER>), dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, uo, coef, den, part, wl);
    else if (kind == PH_L1)
        hipLaunchKernelGGL((photo_point_kernel<PH_L1>), dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, uo, coef, den, part, wl);
    else if (charbonnier)
        hipLaunchKernelGGL((photo_census_kernel<1>), dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, r, uo, q, use_occ ? 1e-6 : 1e-8, gray, coef,
                           den, part, wl);
    else
        hipLaunchKernelGGL((photo_census_kernel<0>), dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, r, uo, q, 0.0, gray, coef, den, part, wl);
    EEM_HIP_CHECK(hipGetLastError());
    if (loss) {
        hipLaunchKernelGGL(dense_finish_kernel, dim3(k), dim3(64), 0, stream, part, nblk, s.n1, den, loss);
        EEM_HIP_CHECK(hipGetLastError());
    }
    return EEM_OK;
}
