// Weighted SSIM warp loss and its gradient with respect to the flow: the structural data term of the ground-truth-free training route,
// beside the photometric and census terms (photo.hip), the contrast term (iwe.hip) and the smoothness term (smooth.hip).
// One job: a flow [B][2][H][W], img1 and img2 [B][C][H][W], an optional mask [B][1][H][W], all contiguous fp32.
//   warp      y_c(p) = Yw_c(p) = grid_sample(img2_c, p + flow(p)): warp_px.h mode 1 in fp32 - the value eemplus_warp(mode 1), the
//             forward-backward check and photo.hip see, bit for bit.  Everything below is unfused fp64 (-ffp-contract=off) on those fp32
//             values; x = img1, w = mask (ones when NULL).
//   moments   per channel and per centre m of [1,H-2] x [1,W-2], with avg3x3(z)(m) = (z(m-W-1) + z(m-W) + z(m-W+1) + z(m-1) + z(m) + z(m+1)
//             + z(m+W-1) + z(m+W) + z(m+W+1)) / 9 - the nine values added in row-major order, one after the other, then one division:
//             aw = avg3x3(w);  wpe = w + weight_epsilon;  inv = 1 / (aw + weight_epsilon);  P[z] = avg3x3(z * wpe) * inv
//             mu_x = P[x], mu_y = P[y], s_x = P[x*x] - mu_x*mu_x, s_y = P[y*y] - mu_y*mu_y, s_xy = P[x*y] - mu_x*mu_y
//   result    c1 = inf: n = 2 s_xy + c2, d = s_x + s_y + c2;  c2 = inf: n = 2 mu_x mu_y + c1, d = mu_x^2 + mu_y^2 + c1;  both finite: the
//             products nL * nS and dL * dS;  v = (1 - n / d) / 2;  l = clamp(v, 0, 1)
//   loss      L = (sum(l) / n1) / D:  n1 = B*C*(H-2)*(W-2), D = 1;  with use_occ sum(l * aw), n1 = 1 and D = sum(aw) + 1e-6 over the
//             B*(H-2)*(W-2) cells of aw (ssim_aw_kernel, ssim_den_kernel)
//   gradient  l depends on y through mu_y, P[y*y] and P[x*y], whose derivatives with respect to y(q), q in m's window, are g, 2 y(q) g and
//             x(q) g with g = wpe(q) * inv(m) / 9.  Per centre the factors FA = dl/dmu_y, FB = dl/dP[y*y], FC = dl/dP[x*y], from
//             dr/dt = (dn/dt - r dd/dt) / d and dl/dr = -1/2 where 0 <= v <= 1 (both ends included, as torch.clamp's backward; 0
//             elsewhere), each times fs(m) = inv/9 * (aw with use_occ) * coef / (n1 D), go into three LDS planes; cell p GATHERS
//             SA, SB, SC over the up to nine centres whose window holds it (row-major order, zeros where there is no centre):
//             dL/dYw_c(p) = wpe(p) * (SA + 2 y(p) SB + x(p) SC).  Then, as in photo.hip, the derivative of the bilinear blend at the fp32
//             tap weights, d ix/du = (W/2) * (2/max(W-1,1)), the sum over the channels in fp64 and one rounding to fp32.  No atomics.
// The tile walk, the jobs inside a tile, the partial sums and their fixed-order finish are dense_loss.h's, with its bitwise contract;
// inside a job the block walks the channels.  Beside its four cells of the tile a thread owns up to two cells of the two-cell ring
// around it for staging and one centre of the one-cell ring for the factors; aw, inv and fs of its centres live in registers for all
// channels, the fp32 tap weights are taken again per channel (keeping them costs 44 VGPRs and spills).
// LDS, static: x, y and w as the fp32 values they are on two cells of halo, 3 planes of 20 x 68 floats (15.9 KB); the three factor planes
// on one cell of halo, 18 x 66 doubles each (27.8 KB); the loss slots (0.5 KB): 44.3 KB - three blocks per CU by LDS, two by registers
// (253 VGPRs).  Without a gradient asked for, the outer ring of the staged planes and the factor planes are left alone.
// Barriers: two per job (before and after the mask is staged), then per channel one after staging x and y and, with a gradient, one
// after the factors and one before the next channel overwrites the planes: 3 per channel with a gradient, 2 without.
// What bounds it: fp64 arithmetic of the centres - per centre and channel 27 LDS reads, 45 multiplies and adds for the five weighted
// sums, then six fp64 divisions (five by 9, one n / d), in the forward and again in the backward; the four gathers per cell and channel
// of the warp come second.  1.7 - 1.8 ms per prediction forward + backward at 1280x720, batch 8, C = 5 (profiles/r21_ssim_bench.txt):
// about twice the arithmetic's count of issue slots, so latency that two waves per SIMD do not hide takes a share (not read from counters).
#include "dense_loss.h"
#include "warp_px.h"

#include <cmath>

namespace {

constexpr int SS_XH = DL_TH + 4, SS_XW = DL_TW + 4;              // x, y, w planes: origin (r0 - 2, c0 - 2)
constexpr int SS_FH = DL_TH + 2, SS_FW = DL_TW + 2;              // factor planes: origin (r0 - 1, c0 - 1)
constexpr int SS_RING2 = SS_XH * SS_XW - DL_TH * DL_TW;          // 336 cells around the tile, two deep
constexpr int SS_RING1 = SS_FH * SS_FW - DL_TH * DL_TW;          // 164 cells around the tile, one deep
static_assert(SS_RING1 <= DL_NT, "one ring centre per thread");

struct SsimShape : DenseShape {
    double c1, c2, eps;
    int lum, str;                // c1 finite: the luminance term takes part;  c2 finite: the structure term
};

struct SsimLds {
    float x[SS_XH * SS_XW];
    float y[SS_XH * SS_XW];
    float w[SS_XH * SS_XW];
    double fa[SS_FH * SS_FW];
    double fb[SS_FH * SS_FW];
    double fc[SS_FH * SS_FW];
    DenseSlots<1> part;
};

// cell r of the two-deep ring, relative to the tile's origin: the rows -2, -1, 16, 17 in full, then the four side columns of rows 0..15
__device__ __forceinline__ void ring2_pos(int r, int& ly, int& lx) {
    if (r < 4 * SS_XW) {
        const int row = r / SS_XW;
        ly = row < 2 ? row - 2 : DL_TH + row - 2;
        lx = r % SS_XW - 2;
    } else {
        const int q = r - 4 * SS_XW, j = q & 3;
        ly = q >> 2;
        lx = j < 2 ? j - 2 : DL_TW + j - 2;
    }
}

// cell r of the one-deep ring: the rows -1 and 16 in full, then the two side columns of rows 0..15
__device__ __forceinline__ void ring1_pos(int r, int& ly, int& lx) {
    if (r < 2 * SS_FW) {
        ly = r < SS_FW ? -1 : DL_TH;
        lx = r % SS_FW - 1;
    } else {
        const int q = r - 2 * SS_FW;
        ly = q >> 1;
        lx = (q & 1) ? DL_TW : -1;
    }
}

// aw of the centre (y, x) of sample b from global memory (1 <= y <= H-2, 1 <= x <= W-2): the nine weights in row-major order
__device__ __forceinline__ double aw_global(const float* __restrict__ mask, size_t base, int y, int x, int W) {
    if (!mask) return 1.0;                                       // nine ones add up to 9, and 9 / 9 = 1
    double a = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) a += (double)mask[base + (size_t)(y + dy) * W + (x + dx)];
    return a / 9.0;
}

// ---- sums of aw (use_occ): block partial sums over the centres per job
__global__ __launch_bounds__(DL_NT) void ssim_aw_kernel(DenseJobs jobs, int k, SsimShape s, double* __restrict__ part) {
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
                if (y >= 1 && y <= s.H - 2 && x >= 1 && x <= s.W - 2) acc += aw_global(mask, (size_t)b * hw, y, x, s.W);
            }
            dense_slots_add(lp, tid, job, acc);
        }
    }
    __syncthreads();
    dense_slots_write(lp, tid, k, part);
}

// one wave per job: den[job] = D = 1, or with use_occ sum(aw) + 1e-6
__global__ __launch_bounds__(64) void ssim_den_kernel(const double* __restrict__ part, int nblk, int use_occ, double* __restrict__ den) {
    const int job = blockIdx.x, lane = threadIdx.x;
    double m = 0.0;
    if (use_occ) {
        for (int i = lane; i < nblk; i += 64) m += part[(size_t)job * nblk + i];
        m = wave_sum(m);
    }
    if (lane == 0) den[job] = use_occ ? m + 1e-6 : 1.0;
}

// what a centre leaves: l, and the three factors before their scale fs
struct SsimCentre {
    double l, fa, fb, fc;
};

// the centre whose cell has index li in the staged planes
__device__ __forceinline__ SsimCentre ssim_centre(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pw, int li,
                                                  double inv, const SsimShape& s) {
    double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int q = li + dy * SS_XW + dx;
            const double xq = (double)px[q], yq = (double)py[q], wq = (double)pw[q] + s.eps;
            ax += xq * wq;
            ay += yq * wq;
            axx += (xq * xq) * wq;
            ayy += (yq * yq) * wq;
            axy += (xq * yq) * wq;
        }
    const double mux = (ax / 9.0) * inv, muy = (ay / 9.0) * inv;
    double nl = 1.0, dl = 1.0, ns = 1.0, ds = 1.0;
    if (s.lum) {
        nl = 2.0 * mux * muy + s.c1;
        dl = mux * mux + muy * muy + s.c1;
    }
    if (s.str) {
        const double pxx = (axx / 9.0) * inv, pyy = (ayy / 9.0) * inv, pxy = (axy / 9.0) * inv;
        const double vx = pxx - mux * mux, vy = pyy - muy * muy, vxy = pxy - mux * muy;
        ns = 2.0 * vxy + s.c2;
        ds = vx + vy + s.c2;
    }
    const double nn = s.lum && s.str ? nl * ns : s.lum ? nl : ns;
    const double dd = s.lum && s.str ? dl * ds : s.lum ? dl : ds;
    const double r = nn / dd;
    const double v = (1.0 - r) / 2.0;
    SsimCentre o;
    o.l = v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v;
    // dl/dt = -1/2 * (dn/dt - r dd/dt) / d on 0 <= v <= 1, for t = mu_y, P[y*y], P[x*y]
    const double dn_mu = (s.lum ? ns * (2.0 * mux) : 0.0) + (s.str ? nl * (-2.0 * mux) : 0.0);
    const double dd_mu = (s.lum ? ds * (2.0 * muy) : 0.0) + (s.str ? dl * (-2.0 * muy) : 0.0);
    const double h = (v >= 0.0 && v <= 1.0) ? -0.5 / dd : 0.0;
    o.fa = h * (dn_mu - r * dd_mu);
    o.fb = s.str ? h * (-(r * dl)) : 0.0;
    o.fc = s.str ? h * (2.0 * nl) : 0.0;
    return o;
}

// aw of the centre at li of the staged mask
__device__ __forceinline__ double aw_staged(const float* __restrict__ pw, int li) {
    double a = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) a += (double)pw[li + dy * SS_XW + dx];
    return a / 9.0;
}

// (two waves per SIMD: the allocator then keeps within 256 VGPRs and nothing spills; three would need 168 and spills)
__global__ __launch_bounds__(DL_NT, 2) void ssim_kernel(DenseJobs jobs, int k, SsimShape s, int use_occ, const double* __restrict__ coef,
                                                     const double* __restrict__ den, double* __restrict__ part, int want_loss) {
    __shared__ SsimLds L;
    const int tid = threadIdx.x;
    const int H = s.H, W = s.W, C = s.C;
    const size_t hw = (size_t)H * W;
    dense_slots_zero(L.part, tid);                               // (the job loop's first barrier stands before the first add)
    const int oly = tid / DL_TW, olx = tid % DL_TW;              // this thread's cell n of the tile: row oly + 4 n, column olx
    int rly, rlx;                                                // the ring centre of this thread
    const bool ract = tid < SS_RING1;
    ring1_pos(ract ? tid : 0, rly, rlx);
    const int rli = (rly + 2) * SS_XW + (rlx + 2), rfi = (rly + 1) * SS_FW + (rlx + 1);
    const long tiles = dense_tiles(s.B, s.tiles_x, s.tiles_y);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const auto [b, r0, c0] = dense_tile(tile, s.tiles_x, s.tiles_y);
        for (int job = 0; job < k; ++job) {
            const float* flow = jobs.flow[job] + (size_t)b * 2 * hw;
            const float* img1 = jobs.img1[job] + (size_t)b * C * hw;
            const float* img2 = jobs.img2[job] + (size_t)b * C * hw;
            const float* mask = jobs.mask[job] ? jobs.mask[job] + (size_t)b * hw : nullptr;
            float* grad = jobs.grad[job];
            const bool want_grad = grad != nullptr;              // block-uniform
            const double sc = want_grad ? ((coef ? coef[job] : 1.0) / s.n1) / den[job] : 0.0;
            const int ring = want_grad ? 2 : 1;                  // halo of the staged planes: the tile's own centres alone without a gradient
            __syncthreads();                                     // the job (or tile) before has read the planes
            // ---- the mask: it serves all channels
            bool in[DL_CELLS];                                   // the cell lies in the frame
            int op[DL_CELLS];
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) {
                const int ly = oly + n * (DL_NT / DL_TW), y = r0 + ly, x = c0 + olx;
                in[n] = y < H && x < W;
                op[n] = in[n] ? y * W + x : 0;
                L.w[(ly + 2) * SS_XW + (olx + 2)] = in[n] ? (mask ? mask[op[n]] : 1.f) : 0.f;
            }
            for (int r = tid; r < SS_RING2; r += DL_NT) {
                int ly, lx;
                ring2_pos(r, ly, lx);
                if (ring == 1 && (ly < -1 || ly > DL_TH || lx < -1 || lx > DL_TW)) continue;
                const int y = r0 + ly, x = c0 + lx;
                const bool inside = y >= 0 && y < H && x >= 0 && x < W;
                L.w[(ly + 2) * SS_XW + (lx + 2)] = inside ? (mask ? mask[y * W + x] : 1.f) : 0.f;
            }
            __syncthreads();
            // ---- aw, inv and the factors' scale fs of this thread's centres
            double aw[DL_CELLS], inv[DL_CELLS], fs[DL_CELLS], inv_r = 0.0, fs_r = 0.0;
            bool cv[DL_CELLS];                                   // the cell is a centre
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) {
                const int ly = oly + n * (DL_NT / DL_TW), y = r0 + ly, x = c0 + olx;
                cv[n] = y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2;
                aw[n] = 0.0, inv[n] = 0.0, fs[n] = 0.0;
                if (cv[n]) {
                    aw[n] = aw_staged(L.w, (ly + 2) * SS_XW + (olx + 2));
                    inv[n] = 1.0 / (aw[n] + s.eps);
                    fs[n] = (use_occ ? (inv[n] / 9.0) * aw[n] : inv[n] / 9.0) * sc;
                }
            }
            const bool cv_r = want_grad && ract && r0 + rly >= 1 && r0 + rly <= H - 2 && c0 + rlx >= 1 && c0 + rlx <= W - 2;
            if (cv_r) {
                const double a = aw_staged(L.w, rli);
                inv_r = 1.0 / (a + s.eps);
                fs_r = (use_occ ? (inv_r / 9.0) * a : inv_r / 9.0) * sc;
            }
            double gu[DL_CELLS], gv[DL_CELLS];
#pragma unroll
            for (int n = 0; n < DL_CELLS; ++n) gu[n] = 0.0, gv[n] = 0.0;
            double acc = 0.0;
            for (int c = 0; c < C; ++c) {
                const float* i1 = img1 + (size_t)c * hw;
                const float* i2 = img2 + (size_t)c * hw;
                if (c > 0) __syncthreads();                      // the channel before has read x, y and the factor planes
                // ---- stage x and y of this channel; the blend's derivative of the tile's own cells stays in registers
                double dxs[DL_CELLS], dys[DL_CELLS];
#pragma unroll
                for (int n = 0; n < DL_CELLS; ++n) {
                    const int li = (oly + n * (DL_NT / DL_TW) + 2) * SS_XW + (olx + 2);
                    float v[4];
                    const WarpTaps t = warp_taps(flow[op[n]], flow[hw + op[n]], H, W, op[n], 1);
                    warp_gather(i2, t, v);
                    L.x[li] = in[n] ? i1[op[n]] : 0.f;
                    L.y[li] = in[n] ? warp_sum(v, t) : 0.f;
                    blend_grad(v, t, dxs[n], dys[n]);
                }
                for (int r = tid; r < SS_RING2; r += DL_NT) {
                    int ly, lx;
                    ring2_pos(r, ly, lx);
                    if (ring == 1 && (ly < -1 || ly > DL_TH || lx < -1 || lx > DL_TW)) continue;
                    const int y = r0 + ly, x = c0 + lx, li = (ly + 2) * SS_XW + (lx + 2);
                    if (y >= 0 && y < H && x >= 0 && x < W) {    // (no centre's window reaches a cell outside the frame)
                        const int p = y * W + x;
                        const WarpTaps t = warp_taps(flow[p], flow[hw + p], H, W, p, 1);
                        float v[4];
                        warp_gather(i2, t, v);
                        L.x[li] = i1[p];
                        L.y[li] = warp_sum(v, t);
                    }
                }
                __syncthreads();
                // ---- the centres: l of the tile's own, and the three factors of all
#pragma unroll
                for (int n = 0; n < DL_CELLS; ++n) {
                    const int ly = oly + n * (DL_NT / DL_TW);
                    SsimCentre o = {0.0, 0.0, 0.0, 0.0};
                    if (cv[n]) o = ssim_centre(L.x, L.y, L.w, (ly + 2) * SS_XW + (olx + 2), inv[n], s);
                    acc += use_occ ? o.l * aw[n] : o.l;
                    if (want_grad) {
                        const int fi = (ly + 1) * SS_FW + (olx + 1);
                        L.fa[fi] = o.fa * fs[n];
                        L.fb[fi] = o.fb * fs[n];
                        L.fc[fi] = o.fc * fs[n];
                    }
                }
                if (!want_grad) continue;                        // block-uniform
                if (ract) {
                    SsimCentre o = {0.0, 0.0, 0.0, 0.0};
                    if (cv_r) o = ssim_centre(L.x, L.y, L.w, rli, inv_r, s);
                    L.fa[rfi] = o.fa * fs_r;
                    L.fb[rfi] = o.fb * fs_r;
                    L.fc[rfi] = o.fc * fs_r;
                }
                __syncthreads();
                // ---- gather the factors of the centres around every cell, then the warp derivative
#pragma unroll
                for (int n = 0; n < DL_CELLS; ++n) {
                    const int ly = oly + n * (DL_NT / DL_TW);
                    const int fi = (ly + 1) * SS_FW + (olx + 1), li = (ly + 2) * SS_XW + (olx + 2);
                    double sa = 0.0, sb = 0.0, sg = 0.0;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int q = fi + dy * SS_FW + dx;
                            sa += L.fa[q];
                            sb += L.fb[q];
                            sg += L.fc[q];
                        }
                    const double xp = (double)L.x[li], yp = (double)L.y[li], wp = (double)L.w[li] + s.eps;
                    const double gy = wp * (sa + 2.0 * yp * sb + xp * sg);              // dL/dYw_c
                    gu[n] += gy * dxs[n];
                    gv[n] += gy * dys[n];
                }
            }
            if (want_loss) dense_slots_add(L.part, tid, job, acc);
            if (want_grad) {
#pragma unroll
                for (int n = 0; n < DL_CELLS; ++n) {
                    if (!in[n]) continue;
                    grad[(size_t)b * 2 * hw + op[n]] = (float)(gu[n] * s.sx);
                    grad[(size_t)b * 2 * hw + hw + op[n]] = (float)(gv[n] * s.sy);
                }
            }
        }
    }
    if (!want_loss) return;
    __syncthreads();
    dense_slots_write(L.part, tid, k, part);
}

}  // namespace

extern "C" size_t eemflow_ssim_scratch_doubles(int k, int B, int H, int W) {
    return H >= 3 && W >= 3 ? dense_scratch_doubles(k, B, H, W, DL_MAX_JOBS, 1) : 0;
}

extern "C" int eemflow_ssim_many(int k, const float* const* flow, const float* const* img1, const float* const* img2,
                                 const float* const* mask, int B, int C, int H, int W, int use_occ, double c1, double c2,
                                 double weight_epsilon, const double* coef, double* loss, float* const* grad, double* scratch, void* stream_) {
    EEM_REQUIRE(k >= 1 && k <= DL_MAX_JOBS, "eemflow_ssim_many: 1..%d jobs per call; got %d", DL_MAX_JOBS, k);
    EEM_REQUIRE(dense_shape_ok(B, H, W), "eemflow_ssim_many: bad shape B=%d H=%d W=%d", B, H, W);
    EEM_REQUIRE(H >= 3 && W >= 3, "eemflow_ssim_many: the 3 x 3 windows need H >= 3 and W >= 3; got %dx%d", H, W);
    EEM_REQUIRE(C >= 1 && (long)B * C * H * W <= (1L << 34), "eemflow_ssim_many: bad channel count C=%d", C);
    EEM_REQUIRE(c1 > 0.0 && c2 > 0.0, "eemflow_ssim_many: c1 and c2 are positive (inf switches a term off); got c1=%g c2=%g", c1, c2);
    EEM_REQUIRE(!(std::isinf(c1) && std::isinf(c2)), "eemflow_ssim_many: c1 and c2 are both infinite: the loss would be zero");
    EEM_REQUIRE(weight_epsilon > 0.0 && std::isfinite(weight_epsilon), "eemflow_ssim_many: weight_epsilon is positive and finite; got %g",
                weight_epsilon);
    EEM_REQUIRE(loss || grad, "eemflow_ssim_many: neither loss nor grad is asked for");
    EEM_REQUIRE(scratch, "eemflow_ssim_many: scratch is NULL (eemflow_ssim_scratch_doubles)");
    DenseJobs jobs;
    if (const int rc = dense_fill_jobs(jobs, "eemflow_ssim_many", k, flow, img1, img2, mask, grad)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    SsimShape s;
    const int nblk = dense_shape(s, B, C, H, W);
    s.n1 = use_occ ? 1.0 : (double)B * (double)C * (double)(H - 2) * (double)(W - 2);
    s.c1 = c1, s.c2 = c2, s.eps = weight_epsilon;
    s.lum = std::isinf(c1) ? 0 : 1, s.str = std::isinf(c2) ? 0 : 1;
    double* den = scratch;
    double* part = scratch + DL_MAX_JOBS;
    const int uo = use_occ ? 1 : 0;
    if (uo) {
        hipLaunchKernelGGL(ssim_aw_kernel, dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, part);
        EEM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(ssim_den_kernel, dim3(k), dim3(64), 0, stream, part, nblk, uo, den);
    EEM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ssim_kernel, dim3(nblk), dim3(DL_NT), 0, stream, jobs, k, s, uo, coef, den, part, loss ? 1 : 0);
    EEM_HIP_CHECK(hipGetLastError());
    if (loss) {
        hipLaunchKernelGGL(dense_finish_kernel, dim3(k), dim3(64), 0, stream, part, nblk, s.n1, den, loss);
        EEM_HIP_CHECK(hipGetLastError());
    }
    return EEM_OK;
}
