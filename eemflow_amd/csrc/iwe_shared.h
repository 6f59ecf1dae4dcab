// What the forward (iwe_fwd_shared.h: iwe.hip, tsimg.hip) and the gradient (iwe_grad_shared.h: iwe_grad.hip, tsimg.hip) of the event
// losses share: the per-event arithmetic, the block helpers of the binning kernels, the band plan with its lanes-per-run rule and band
// launch, the entry points' argument check and the scratch arenas.  All three files are built with -ffp-contract=off: the gradient
// recomputes the forward's warp with the same expressions in the same order, so it finds the same cells bit for bit.
#pragma once

#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <mutex>

namespace {

constexpr int IWE_MAX_JOBS = 32;
constexpr int VT = 1024;                 // threads per binning block (also the maximum number of bands + 1)
constexpr unsigned NONE = 0xffffffffu;

// ------------------------------------------------------------------------------------------------ per-event arithmetic
// the affine event map of a job: xe = ax * x + bx, ye = ay * y + by (an offset (ox, oy) is {1, -ox, 1, -oy}: 1 * x is exact and
// x + (-ox) is x - ox, the same bits)
struct IweMap { double ax, bx, ay, by; };

// the four bilinear sample neighbours of (xe, ye): (y0 + dy, x0 + dx), k = 2 * dy + dx, with weight wk[k]; in[k]: inside the frame
struct IweTaps {
    double wk[4];
    bool in[4];
    int x0, y0;
    bool any;                // false: every neighbour outside (also NaN coordinates)
};

__device__ __forceinline__ IweTaps iwe_taps(double xe, double ye, int h, int w) {
    IweTaps s;
    s.any = xe > -1.0 && xe < (double)w && ye > -1.0 && ye < (double)h;
    s.x0 = s.y0 = 0;
    s.wk[0] = s.wk[1] = s.wk[2] = s.wk[3] = 0.0;
    s.in[0] = s.in[1] = s.in[2] = s.in[3] = false;
    if (!s.any) return s;
    const double xf = floor(xe), yf = floor(ye);
    const double fx = xe - xf, fy = ye - yf;
    s.x0 = (int)xf;                                                                // -1 .. w-1
    s.y0 = (int)yf;                                                                // -1 .. h-1
    const bool xl = s.x0 >= 0, xr = s.x0 + 1 <= w - 1, yt = s.y0 >= 0, yb = s.y0 + 1 <= h - 1;
    s.wk[0] = (1.0 - fx) * (1.0 - fy);
    s.wk[1] = fx * (1.0 - fy);
    s.wk[2] = (1.0 - fx) * fy;
    s.wk[3] = fx * fy;
    s.in[0] = xl && yt;
    s.in[1] = xr && yt;
    s.in[2] = xl && yb;
    s.in[3] = xr && yb;
    return s;
}

// bilinear sample of both flow channels at the neighbours `s` of (xe, ye), zero padding; a NULL flow is the zero flow
__device__ __forceinline__ void iwe_sample(const float* __restrict__ flow, const IweTaps& s, int h, int w, double& u, double& v) {
    u = 0.0;
    v = 0.0;
    if (!flow || !s.any) return;
    const long hw = (long)h * w;
    const long o = (long)s.y0 * w + s.x0;
    const double u00 = s.in[0] ? s.wk[0] * (double)flow[o] : 0.0, v00 = s.in[0] ? s.wk[0] * (double)flow[hw + o] : 0.0;
    const double u01 = s.in[1] ? s.wk[1] * (double)flow[o + 1] : 0.0, v01 = s.in[1] ? s.wk[1] * (double)flow[hw + o + 1] : 0.0;
    const double u10 = s.in[2] ? s.wk[2] * (double)flow[o + w] : 0.0, v10 = s.in[2] ? s.wk[2] * (double)flow[hw + o + w] : 0.0;
    const double u11 = s.in[3] ? s.wk[3] * (double)flow[o + w + 1] : 0.0, v11 = s.in[3] ? s.wk[3] * (double)flow[hw + o + w + 1] : 0.0;
    u = ((u00 + u01) + u10) + u11;
    v = ((v00 + v01) + v10) + v11;
}

struct IweEvent {
    double xw, yw;
    double tau;              // the time factor the warp used
    IweTaps taps;            // the sample neighbours of the mapped position (the gradient hands its contributions to them)
    int c;
};

__device__ __forceinline__ IweEvent iwe_warp(const double* __restrict__ ev, long i, const float* __restrict__ flow, double t0, double scale,
                                             const IweMap& m, int h, int w) {
    const double t = ev[i * 4 + 0], x = ev[i * 4 + 1], y = ev[i * 4 + 2], p = ev[i * 4 + 3];
    IweEvent e;
    const double xe = m.ax * x + m.bx, ye = m.ay * y + m.by;
    e.taps = iwe_taps(xe, ye, h, w);
    double u, v;
    iwe_sample(flow, e.taps, h, w, u, v);
    e.tau = (t - t0) * scale;
    e.xw = xe + u * e.tau;
    e.yw = ye + v * e.tau;
    e.c = p > 0.0 ? 0 : 1;
    return e;
}

// the votes of a warped event: rows Y0, Y0 + 1 and columns X0, X0 + 1 with weights wy[dy] * wx[dx]
struct IweVotes {
    int X0, Y0;
    double gx, gy;
    bool finite, inside;     // inside: at least one of the four targets can be in the frame
};

__device__ __forceinline__ IweVotes iwe_votes(const IweEvent& e, int h, int w) {
    IweVotes q;
    q.finite = isfinite(e.xw) && isfinite(e.yw);
    q.inside = q.finite && e.xw > -1.0 && e.xw < (double)w && e.yw > -1.0 && e.yw < (double)h;
    q.X0 = q.Y0 = 0;
    q.gx = q.gy = 0.0;
    if (q.inside) {
        const double xf = floor(e.xw), yf = floor(e.yw);
        q.X0 = (int)xf;
        q.Y0 = (int)yf;
        q.gx = e.xw - xf;
        q.gy = e.yw - yf;
    }
    return q;
}

// ------------------------------------------------------------------------------------------------ block helpers
// sums of two values over the block, by a fixed tree (wave shuffles, then the waves' sums in order; sh: 2 * NT / 64 doubles): the same
// bits whatever the schedule.  Every thread of the block calls it; the results are valid in thread 0.
template <int NT>
__device__ __forceinline__ void block_sum2(double& a, double& b, double* sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_down(a, d);
        b += __shfl_down(b, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                               // (sh may still be read from a call before)
    if (lane == 0) { sh[2 * wave] = a; sh[2 * wave + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0.0;
        for (int k = 0; k < NT / 64; ++k) { a += sh[2 * k]; b += sh[2 * k + 1]; }
    }
}

// exclusive prefix sum over the block's VT threads (sh: VT / 64 words)
__device__ __forceinline__ unsigned block_exscan(unsigned v, unsigned* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(x, d);
        if (lane >= d) x += t;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    unsigned before = 0;
#pragma unroll
    for (int k = 0; k < VT / 64; ++k) before += k < wave ? sh[k] : 0u;
    return before + x - v;
}

// ------------------------------------------------------------------------------------------------ host: the band plan
struct IwePlan {
    int rows;                // image rows per band
    int nb;                  // bands
    int cells;               // fp64 cells of a band: cpp * rows * w
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline long iwe_blocks(long n, int ept) { return (n + (long)VT * ept - 1) / ((long)VT * ept); }
constexpr long IWE_MAX_BLOCKS = 4096;                              // 16.7 M events at 4 per thread; beyond: direct form

inline bool iwe_direct_forced() { return sw_on<SW_EEM_IWE_DIRECT>(); }

// the band layout of an h x w frame for binning blocks of up to `ept_max` events per thread, or false: the direct form serves it.
// cpp: fp64 LDS cells per pixel of a band - 2 for the image and the gradient (both channels), 4 for tsimg.hip's D and N planes
inline bool iwe_plan(long nmax, int h, int w, IwePlan* pl, int ept_max = 4, int cpp = 2) {
    if (iwe_direct_forced() || iwe_blocks(nmax, ept_max) > IWE_MAX_BLOCKS) return false;
    // 9216 fp64 cells (72 KB) per band: two blocks per CU; a frame wider than that still gets one-row bands up to 150 KB of LDS
    long rows = 9216 / ((long)cpp * w);
    if (rows < 1) {
        if ((long)cpp * w > 19200) return false;                      // 150 KB of fp64 cells beside the static tables
        rows = 1;
    }
    const long spread = std::max(1L, (h + 239L) / 240);            // small frames: still up to a few hundred bands
    rows = std::min(rows, spread);
    if ((h + rows - 1) / rows > VT - 1) return false;              // thread nb of a binning block holds the slab's fill
    pl->rows = (int)rows;
    pl->nb = (int)((h + rows - 1) / rows);
    pl->cells = (int)(cpp * rows * w);
    return true;
}

// lanes per run of a band kernel, as log2: the smallest power of two >= 1.7 x the mean run length (a slab's records / bands), 4 .. 64
inline int iwe_run_lanes(const IwePlan& pl, int slab) {
    int sgs = 2;
    while (sgs < 6 && (1 << sgs) * 10L * pl.nb < 17L * slab) ++sgs;
    return sgs;
}

// the launch of a band kernel, one block per band and job: 256 threads for a small band, else VT with the band's LDS allowed; *bt: which
template <auto K256, auto KVT, class... Args>
int iwe_launch_bands(const IwePlan& pl, int njobs, hipStream_t stream, int* bt, Args... args) {
    const int lds = pl.cells * 8;
    if (pl.cells <= 3072) {
        *bt = 256;
        hipLaunchKernelGGL(K256, dim3(pl.nb, njobs), dim3(256), lds, stream, args...);
    } else {
        *bt = VT;
        if (lds > 32 * 1024) EEM_RAISE_LDS(lds, KVT);
        hipLaunchKernelGGL(KVT, dim3(pl.nb, njobs), dim3(VT), lds, stream, args...);
    }
    return EEM_OK;
}

// what every *_many entry point checks first (nonnull: its own pointer arguments, n among them), under the entry's name
inline int iwe_check_many(const char* name, int k, bool nonnull, int h, int w, const int64_t* n) {
    EEM_REQUIRE(k >= 1 && k <= IWE_MAX_JOBS, "%s: 1..%d jobs per call; got %d", name, IWE_MAX_JOBS, k);
    EEM_REQUIRE(nonnull, "%s: NULL argument", name);
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 30), "%s: bad size %dx%d", name, h, w);
    for (int i = 0; i < k; ++i) EEM_REQUIRE(n[i] >= 0 && n[i] < (1LL << 40), "%s: job %d has n=%ld events", name, i, (long)n[i]);
    return EEM_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host: scratch arenas (iwe.hip)
// The pool of scratch arenas (record slabs, run tables, partials; the direct forms' fp64 image) that the image of warped events and its
// gradient share - apart from the voxelizer's pool, which loader threads use meanwhile.  See Arena for how a caller takes one.
Arena& iwe_arena();
