// One pixel of the backward warp family (reference: model/EEMFlow/EEMFlow+.py:137-149, model/EEMFlow/cdc_utils.py:50-103,
// utils_luo/tools.py:2262-2306): the four bilinear taps of F.grid_sample for the pixel's flow, the gather and the weighted sum.
// Shared by the warp kernels of plus_kernels.hip (eemplus_warp) and the forward-backward check (fb_check.hip), which must see the
// very same warped values.  Translation units that include this are built with -ffp-contract=off: the reference's
// `grid_sample(ones) >= 1.0` mask depends on the last bit of nw + ne + sw + se, so the coordinate and weight arithmetic follows
// ATen's CPU grid sampler operation by operation (separate multiplies and adds, same association).
#pragma once
#include "common.h"

struct WarpTaps {
    float nw, ne, sw, se;        // bilinear weights of the four corners
    int o_nw, o_ne, o_sw, o_se;  // their offsets in a [h][w] plane, -1: outside (zero padding)
    float m;                     // mode 2: the `grid_sample(ones) >= 1` mask, else 1
    float wx, wy;                // ix - floor(ix), iy - floor(iy): the weights' factors, for the blend's derivative (blend_grad)
};

// mode 0: align_corners=True (EEMFlow_cdc.warp); 1: align_corners=False (torch_warp);
// 2: align_corners=False + `grid_sample(ones) >= 1` mask (WarpingLayer_no_div)
__device__ __forceinline__ WarpTaps warp_taps(float fx, float fy, int h, int w, int p, int mode) {
    const int py = p / w, px = p - py * w;
    const float vx = (float)px + fx;
    const float vy = (float)py + fy;
    const float xn = 2.0f * vx / (float)max(w - 1, 1) - 1.0f;
    const float yn = 2.0f * vy / (float)max(h - 1, 1) - 1.0f;
    float ix, iy;
    if (mode == 0) {
        ix = (xn + 1.f) * ((float)(w - 1) / 2.f);
        iy = (yn + 1.f) * ((float)(h - 1) / 2.f);
    } else {
        ix = (xn + 1.f) * ((float)w / 2.f) - 0.5f;
        iy = (yn + 1.f) * ((float)h / 2.f) - 0.5f;
    }
    const float xw = floorf(ix), yn0 = floorf(iy);
    const float wgt_w = ix - xw, wgt_e = 1.f - wgt_w, wgt_n = iy - yn0, wgt_s = 1.f - wgt_n;
    WarpTaps t;
    t.nw = wgt_s * wgt_e; t.ne = wgt_s * wgt_w; t.sw = wgt_n * wgt_e; t.se = wgt_n * wgt_w;
    t.wx = wgt_w; t.wy = wgt_n;
    // the float -> int conversion must not overflow for wild flows
    const float cx = fminf(fmaxf(xw, -2.f), (float)w + 1.f), cy = fminf(fmaxf(yn0, -2.f), (float)h + 1.f);
    const int x0 = (int)cx, y0 = (int)cy;
    const bool in_w = x0 >= 0 && x0 < w, in_e = x0 + 1 >= 0 && x0 + 1 < w;
    const bool in_n = y0 >= 0 && y0 < h, in_s = y0 + 1 >= 0 && y0 + 1 < h;
    t.m = 1.f;
    if (mode == 2) {
        const float ones = (((in_n && in_w ? 1.f : 0.f) * t.nw + (in_n && in_e ? 1.f : 0.f) * t.ne) + (in_s && in_w ? 1.f : 0.f) * t.sw) +
                           (in_s && in_e ? 1.f : 0.f) * t.se;
        t.m = ones >= 1.0f ? 1.f : 0.f;
    }
    t.o_nw = (in_n && in_w) ? y0 * w + x0 : -1; t.o_ne = (in_n && in_e) ? y0 * w + x0 + 1 : -1;
    t.o_sw = (in_s && in_w) ? (y0 + 1) * w + x0 : -1; t.o_se = (in_s && in_e) ? (y0 + 1) * w + x0 + 1 : -1;
    return t;
}

// the four corner values of plane s [h][w]
__device__ __forceinline__ void warp_gather(const float* __restrict__ s, const WarpTaps& t, float v[4]) {
    // (unconditional loads from clamped offsets, the bounds applied to the values: a load in one arm of a lane-dependent
    // conditional is a branch followed by s_waitcnt vmcnt(0) - sixteen dependent round trips instead of one)
    const float a0 = s[max(t.o_nw, 0)], a1 = s[max(t.o_ne, 0)], a2 = s[max(t.o_sw, 0)], a3 = s[max(t.o_se, 0)];
    v[0] = t.o_nw >= 0 ? a0 : 0.f;
    v[1] = t.o_ne >= 0 ? a1 : 0.f;
    v[2] = t.o_sw >= 0 ? a2 : 0.f;
    v[3] = t.o_se >= 0 ? a3 : 0.f;
}

// the warped value before the mode-2 mask
__device__ __forceinline__ float warp_sum(const float v[4], const WarpTaps& t) {
    return ((v[0] * t.nw + v[1] * t.ne) + v[2] * t.sw) + v[3] * t.se;
}

// the derivative of the blend of the corner values v with respect to ix and iy, in fp64 at the fp32 tap weights (photo.hip, ssim.hip)
__device__ __forceinline__ void blend_grad(const float v[4], const WarpTaps& t, double& dx, double& dy) {
    const double ww = (double)t.wx, we = (double)(1.f - t.wx), wn = (double)t.wy, ws = (double)(1.f - t.wy);
    dx = ws * ((double)v[1] - (double)v[0]) + wn * ((double)v[3] - (double)v[2]);
    dy = we * ((double)v[2] - (double)v[0]) + ww * ((double)v[3] - (double)v[1]);
}
