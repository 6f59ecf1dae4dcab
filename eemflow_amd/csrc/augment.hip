// Training-sample augmentation on the device: the rescale / flip / crop of the reference's augmentors (FlowAugmentor.spatial_transform,
// utils/augumentor.py:158-257; DenseSparseAugmentor.spatial_transform, :389-419) applied to volumes that the voxelizer left on the GPU,
// written straight into the batch tensors the training step reads.  The random draws stay on the host (eemflow_amd/augmentor.py:
// AugPlan); this file moves the pixels.
//
// Per job (= one sample of the batch): vol_old, vol_new [C][H][W] fp32, flow [2][H][W] fp32 or fp64 (NULL: no flow, no valid mask), a
// plan {resized, scale_x, scale_y, RH, RW, hflip, vflip, y0, x0}.  Output pixel (r, c) of the [ch][cw] crop:
//   rr = y0 + r, cc = x0 + c            position in the resized (or original) RH x RW image
//   vflip: rr -> RH-1-rr, hflip: cc -> RW-1-cc        (the host resizes, then flips, then crops: the crop reads the flipped image)
//   not resized: the source element at (rr, cc)
//   resized: augmentor.resize_linear's rule in unfused fp64 (this file is built with -ffp-contract=off):
//            s = (d + 0.5) / f - 0.5, i0 = floor(s), t = s - i0, neighbours i0, i0 + 1 clamped to the source;
//            top = v00*(1-tx) + v01*tx, bot = v10*(1-tx) + v11*tx, out = top*(1-ty) + bot*ty; rounded to the source's type
//   flow:    the sample as above (an fp32 source rounded to fp32 after the interpolation, as the host's resize returns its input's
//            type), x (scale_x, scale_y) in fp64 when resized, x -1 on u for hflip and on v for vflip, rounded to fp32 once
//   valid:   MVSEC's rule ~isinf(u) & ~isinf(v) & (||(u, v)|| > 0) on the fp32 flow just written (below: aug_valid)
//
// A byte mover: no LDS, no atomics.  A thread makes VEC consecutive pixels of one output row - VEC = 4 with one 16-byte store where
// cw % 4 == 0 and the destinations are 16-byte aligned (rows of the batch tensors are, then), VEC = 1 for widths such as 346 or 21.  The
// source of a row is unaligned (x0) and, mirrored, reversed: it is read with dword loads, a wave's loads of one row still covering one
// contiguous segment.  blockIdx.z = job, blockIdx.y = plane (2C volume planes, then the flow with its mask), blockIdx.x walks the
// plane's pixels with a grid stride, the whole grid held near 2048 blocks.
#include "common.h"

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/eemflow_hip.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_GRID = 2048;               // blocks of a launch, about: 8 per CU

struct AugJob {
    const float* vol_old;
    const float* vol_new;
    const void* flow;                        // NULL: this sample has no flow (and gets no valid mask)
    double sx, sy;
    int RH, RW, y0, x0;
    int resized, hflip, vflip, pad;
};
struct AugJobs { AugJob j[EEMFLOW_AUGMENT_MAX]; };       // 64 bytes each: 1 KB of kernel arguments

// one axis of the sampling: the two source indices and the weight of the second
struct AugAxis {
    int a, b;
    double t;
};

// d: index in the (flipped back) resized image; n: source extent.  Not resized: a = b = d.
template <bool RESIZE>
__device__ __forceinline__ AugAxis aug_axis(int d, bool resized, double f, int n) {
    AugAxis x;
    if (RESIZE && resized) {
        const double s = ((double)d + 0.5) / f - 0.5;
        const double fl = floor(s);
        x.t = s - fl;
        // fl is within a few units of [-1, n]: round(n * f) >= d + 1 bounds s below n + 1 / f
        const long i0 = (long)fl;
        x.a = (int)min(max(i0, 0L), (long)n - 1);
        x.b = (int)min(max(i0 + 1, 0L), (long)n - 1);
    } else {
        x.a = x.b = d;
        x.t = 0.0;
    }
    return x;
}

template <typename T>
__device__ __forceinline__ double aug_interp(const T* __restrict__ p, long ra, long rb, const AugAxis& x, double ty) {
    const double v00 = (double)p[ra + x.a], v01 = (double)p[ra + x.b], v10 = (double)p[rb + x.a], v11 = (double)p[rb + x.b];
    const double top = v00 * (1.0 - x.t) + v01 * x.t;
    const double bot = v10 * (1.0 - x.t) + v11 * x.t;
    return top * (1.0 - ty) + bot * ty;
}

// One flow component as the host leaves it in fp32: resize (in the source's type), scale, flip sign, one rounding.
template <bool RESIZE, typename T>
__device__ __forceinline__ float aug_flow(const T* __restrict__ p, long ra, long rb, const AugAxis& x, double ty, bool resized, double scale,
                                          bool negate) {
    double v;
    if (RESIZE && resized) {
        v = aug_interp(p, ra, rb, x, ty);
        if (sizeof(T) == 4) v = (double)(float)v;                  // resize_linear returns its input's type
        v = v * scale;
    } else {
        v = (double)p[ra + x.a];
    }
    if (negate) v = v * -1.0;
    return (float)v;
}

// MVSEC.py:185 on the fp32 pair: ~isinf(u) & ~isinf(v) & (torch.linalg.norm((u, v)) > 0).  The norm is sqrt(fl(fl(u*u) + fl(v*v))) in
// fp32 (or with the second product fused into the sum): sums and square roots of non-negative numbers are positive exactly when an
// operand is, so the decision is "fl(u*u) > 0 or fl(v*v) > 0", and a square rounds to 0 exactly when it is <= 2^-150 (half the smallest
// fp32 denormal, the tie going to the even 0) - tested on the product in fp64, where it is exact.  A NaN component makes the norm NaN
// and the comparison false: isfinite on both covers that and the infinities.
__device__ __forceinline__ float aug_valid(float u, float v) {
    const double uu = (double)u * (double)u, vv = (double)v * (double)v;
    return (isfinite(u) && isfinite(v) && (uu > 0x1p-150 || vv > 0x1p-150)) ? 1.0f : 0.0f;
}

template <int VEC>
__device__ __forceinline__ void aug_store(float* __restrict__ dst, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[0] = v[0];
}

template <int VEC, bool RESIZE, typename TF>
__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(AugJobs jobs, int C, int H, int W, int ch, int cw, float* __restrict__ d_old,
                                                              float* __restrict__ d_new, float* __restrict__ d_flow,
                                                              float* __restrict__ d_valid) {
    const int job = blockIdx.z;
    const AugJob& J = jobs.j[job];
    const int item = blockIdx.y;                                   // 0 .. C-1 old planes, C .. 2C-1 new planes, 2C the flow and its mask
    const bool is_flow = item == 2 * C;
    if (is_flow && !J.flow) return;
    const bool resized = J.resized != 0, hflip = J.hflip != 0, vflip = J.vflip != 0;
    const int upr = cw / VEC;                                      // units per output row (VEC = 4 only where cw % 4 == 0)
    const long units = (long)ch * upr;
    const long hw = (long)H * W, chw = (long)ch * cw;
    const int plane = item < C ? item : item - C;
    const float* __restrict__ src = (item < C ? J.vol_old : J.vol_new) + (long)plane * hw;
    float* __restrict__ dst = (item < C ? d_old : d_new) + ((long)job * C + plane) * chw;
    const TF* __restrict__ fu = reinterpret_cast<const TF*>(J.flow);
    const TF* __restrict__ fv = fu + hw;
    float* __restrict__ du = d_flow + (long)job * 2 * chw;
    float* __restrict__ dm = d_valid + (long)job * chw;
    for (long u = (long)blockIdx.x * AUG_THREADS + threadIdx.x; u < units; u += (long)gridDim.x * AUG_THREADS) {
        const int r = (int)(u / upr);
        const int c = (int)(u - (long)r * upr) * VEC;
        int rr = J.y0 + r;
        if (vflip) rr = J.RH - 1 - rr;
        const AugAxis y = aug_axis<RESIZE>(rr, resized, J.sy, H);
        const long ra = (long)y.a * W, rb = (long)y.b * W;
        const long o = (long)r * cw + c;
        float a[VEC], b[VEC], m[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            int cc = J.x0 + c + k;
            if (hflip) cc = J.RW - 1 - cc;
            const AugAxis x = aug_axis<RESIZE>(cc, resized, J.sx, W);
            if (!is_flow) {
                a[k] = (RESIZE && resized) ? (float)aug_interp(src, ra, rb, x, y.t) : src[ra + x.a];
            } else {
                a[k] = aug_flow<RESIZE>(fu, ra, rb, x, y.t, resized, J.sx, hflip);
                b[k] = aug_flow<RESIZE>(fv, ra, rb, x, y.t, resized, J.sy, vflip);
                m[k] = aug_valid(a[k], b[k]);
            }
        }
        if (!is_flow) {
            aug_store<VEC>(dst + o, a);
        } else {
            aug_store<VEC>(du + o, a);
            aug_store<VEC>(du + chw + o, b);
            aug_store<VEC>(dm + o, m);
        }
    }
}

template <int VEC, bool RESIZE>
void aug_launch(const AugJobs& jobs, int n, int C, int H, int W, int ch, int cw, int flow_f64, bool any_flow, float* d_old, float* d_new,
                float* d_flow, float* d_valid, hipStream_t stream) {
    const int items = 2 * C + (any_flow ? 1 : 0);
    const long units = (long)ch * (cw / VEC);
    long bx = (units + AUG_THREADS - 1) / AUG_THREADS;
    const long cap = (AUG_GRID + (long)items * n - 1) / ((long)items * n);
    if (bx > cap) bx = cap;
    const dim3 grid((unsigned)bx, (unsigned)items, (unsigned)n);
    if (flow_f64)
        hipLaunchKernelGGL((augment_kernel<VEC, RESIZE, double>), grid, dim3(AUG_THREADS), 0, stream, jobs, C, H, W, ch, cw, d_old, d_new, d_flow,
                           d_valid);
    else
        hipLaunchKernelGGL((augment_kernel<VEC, RESIZE, float>), grid, dim3(AUG_THREADS), 0, stream, jobs, C, H, W, ch, cw, d_old, d_new, d_flow,
                           d_valid);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int eemflow_augment_many(int n, const float* const* vol_old, const float* const* vol_new, const void* const* flow, int flow_f64,
                                    const eemflow_aug_plan* plans, int C, int H, int W, int ch, int cw, float* out_old, float* out_new,
                                    float* out_flow, float* out_valid, void* stream) {
    EEM_REQUIRE(n >= 1 && n <= EEMFLOW_AUGMENT_MAX, "eemflow_augment_many: 1..%d samples per call; got %d", EEMFLOW_AUGMENT_MAX, n);
    EEM_REQUIRE(vol_old && vol_new && plans && out_old && out_new, "eemflow_augment_many: NULL argument");
    EEM_REQUIRE(C >= 1 && C <= 1024 && H >= 1 && W >= 1 && (long)H * W <= (1L << 30), "eemflow_augment_many: bad size %dx%dx%d", C, H, W);
    EEM_REQUIRE(ch >= 1 && cw >= 1 && (long)ch * cw <= (1L << 30), "eemflow_augment_many: bad crop %dx%d", ch, cw);
    AugJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    bool any_flow = false, any_resize = false;
    for (int i = 0; i < n; ++i) {
        const eemflow_aug_plan& p = plans[i];
        EEM_REQUIRE(vol_old[i] && vol_new[i], "eemflow_augment_many: sample %d has a NULL volume", i);
        if (p.resized) {
            EEM_REQUIRE(std::isfinite(p.scale_x) && std::isfinite(p.scale_y) && p.scale_x > 0.0 && p.scale_y > 0.0,
                        "eemflow_augment_many: sample %d has scale (%g, %g)", i, p.scale_x, p.scale_y);
            // augmentor.resize_linear: int(round(h * fy)), Python's round (ties to even) of the fp64 product
            const double rh = std::nearbyint((double)H * p.scale_y), rw = std::nearbyint((double)W * p.scale_x);
            EEM_REQUIRE(rh == (double)p.RH && rw == (double)p.RW && p.RH >= 1 && p.RW >= 1 && (long)p.RH * p.RW <= (1L << 30),
                        "eemflow_augment_many: sample %d: resized size %dx%d is not round(%d * %.17g) x round(%d * %.17g)", i, p.RH, p.RW, H,
                        p.scale_y, W, p.scale_x);
        } else {
            EEM_REQUIRE(p.RH == H && p.RW == W, "eemflow_augment_many: sample %d is not resized but its plan's size %dx%d is not the source's %dx%d",
                        i, p.RH, p.RW, H, W);
        }
        EEM_REQUIRE(p.y0 >= 0 && p.x0 >= 0 && (long)p.y0 + ch <= p.RH && (long)p.x0 + cw <= p.RW,
                    "eemflow_augment_many: sample %d: the %dx%d crop at (%d, %d) leaves the %dx%d image", i, ch, cw, p.y0, p.x0, p.RH, p.RW);
        AugJob& J = jobs.j[i];
        J.vol_old = vol_old[i];
        J.vol_new = vol_new[i];
        J.flow = flow ? flow[i] : nullptr;
        J.sx = p.scale_x;
        J.sy = p.scale_y;
        J.RH = p.RH;
        J.RW = p.RW;
        J.y0 = p.y0;
        J.x0 = p.x0;
        J.resized = p.resized ? 1 : 0;
        J.hflip = p.hflip ? 1 : 0;
        J.vflip = p.vflip ? 1 : 0;
        any_flow = any_flow || J.flow != nullptr;
        any_resize = any_resize || J.resized;
    }
    EEM_REQUIRE(!any_flow || (out_flow && out_valid), "eemflow_augment_many: a flow is given but out_flow / out_valid is NULL");
    const bool wide = cw % 4 == 0 && aligned16(out_old) && aligned16(out_new) && (!any_flow || (aligned16(out_flow) && aligned16(out_valid)));
    hipStream_t s = (hipStream_t)stream;
    if (wide) {
        if (any_resize) aug_launch<4, true>(jobs, n, C, H, W, ch, cw, flow_f64, any_flow, out_old, out_new, out_flow, out_valid, s);
        else aug_launch<4, false>(jobs, n, C, H, W, ch, cw, flow_f64, any_flow, out_old, out_new, out_flow, out_valid, s);
    } else {
        if (any_resize) aug_launch<1, true>(jobs, n, C, H, W, ch, cw, flow_f64, any_flow, out_old, out_new, out_flow, out_valid, s);
        else aug_launch<1, false>(jobs, n, C, H, W, ch, cw, flow_f64, any_flow, out_old, out_new, out_flow, out_valid, s);
    }
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}
