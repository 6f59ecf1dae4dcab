// Forward-backward consistency check of a bidirectional flow pair (reference: occ_check_model, utils_luo/tools.py:1136-1309, on
// tensor_tools.torch_warp, :2262-2306).  With len(x) = sqrt(x_u^2 + x_v^2):
//     thresh  = alpha1 * (len(fw) + len(bw)) + alpha2
//     mask_fw = len(fw + torch_warp(bw, fw)) < thresh        mask_bw = len(bw + torch_warp(fw, bw)) < thresh
// 1 = consistent, 0 = occluded / unreliable.  torch_warp is warp_px.h's mode 1 - the routine eemplus_warp runs, so the warped values are
// that kernel's, bit for bit (normalised by W - 1 / H - 1, sampled with align_corners=False: half a pixel off, as the reference is).
// mode 0 'all': the masks above; 1 'obj': a pixel whose target x + flow leaves [0, W-1] x [0, H-1] is forced to 1
// (torch_get_obj_occ_check); 2 'out': the outgoing mask alone (torch_outgoing_occ_check: 1 inside, 0 leaving).
// ONE launch for all n pairs and both directions: blockIdx.y = pair, a lane owns four consecutive pixels - two 16-byte loads per
// flow, eight gathered corners per pixel and direction, one 16-byte store per mask.  16 B read + 8 B written per pixel (the gathers
// hit lines the coalesced loads of neighbouring lanes bring in): HBM-bound.  Built with -ffp-contract=off like the warp kernels.
#include <string.h>

#include "warp_px.h"

namespace {

struct FbMany { const float* fw[16]; const float* bw[16]; float* mfw[16]; float* mbw[16]; };

// the reference's length_sq (it takes the root): torch.pow(torch.sum(x ** 2, dim=1), 0.5)
__device__ __forceinline__ float flow_len(float u, float v) { return sqrtf(u * u + v * v); }

// torch_outgoing_occ_check: 0 where the target leaves the frame (a NaN flow stays 1, as the reference's comparisons leave it)
__device__ __forceinline__ bool outgoing(float u, float v, int px, int py, int h, int w) {
    const float pos_x = (float)px + u, pos_y = (float)py + v;
    return pos_x > (float)(w - 1) || pos_x < 0.f || pos_y > (float)(h - 1) || pos_y < 0.f;
}

template <int VEC>
__global__ __launch_bounds__(256) void fb_check_kernel(FbMany many, int h, int w, float alpha1, float alpha2, int mode) {
    const float* __restrict__ fw = many.fw[blockIdx.y];
    const float* __restrict__ bw = many.bw[blockIdx.y];
    float* __restrict__ mfw = many.mfw[blockIdx.y];
    float* __restrict__ mbw = many.mbw[blockIdx.y];
    const int hw = h * w;
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (p0 >= hw) return;                                    // (VEC == 4: hw is a multiple of 4, a run never passes the plane's end)
    float fu[VEC], fv[VEC], bu[VEC], bv[VEC];
    if (VEC == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(fw + p0), b = *reinterpret_cast<const f32x4*>(fw + hw + p0);
        const f32x4 c = *reinterpret_cast<const f32x4*>(bw + p0), d = *reinterpret_cast<const f32x4*>(bw + hw + p0);
#pragma unroll
        for (int i = 0; i < VEC; ++i) { fu[i] = a[i]; fv[i] = b[i]; bu[i] = c[i]; bv[i] = d[i]; }
    } else {
        fu[0] = fw[p0]; fv[0] = fw[hw + p0]; bu[0] = bw[p0]; bv[0] = bw[hw + p0];
    }
    float of[VEC], ob[VEC];
    if (mode == 2) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int p = p0 + i, py = p / w, px = p - py * w;
            of[i] = outgoing(fu[i], fv[i], px, py, h, w) ? 0.f : 1.f;
            ob[i] = outgoing(bu[i], bv[i], px, py, h, w) ? 0.f : 1.f;
        }
    } else {
        // all gathers of the lane's pixels go out before the first sum
        WarpTaps tf[VEC], tb[VEC];
        float gbu[VEC][4], gbv[VEC][4], gfu[VEC][4], gfv[VEC][4];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            tf[i] = warp_taps(fu[i], fv[i], h, w, p0 + i, 1);       // torch_warp(bw, fw): bw sampled at x + fw
            tb[i] = warp_taps(bu[i], bv[i], h, w, p0 + i, 1);       // torch_warp(fw, bw)
            warp_gather(bw, tf[i], gbu[i]); warp_gather(bw + hw, tf[i], gbv[i]);
            warp_gather(fw, tb[i], gfu[i]); warp_gather(fw + hw, tb[i], gfv[i]);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float thresh = alpha1 * (flow_len(fu[i], fv[i]) + flow_len(bu[i], bv[i])) + alpha2;
            const float dfu = fu[i] + warp_sum(gbu[i], tf[i]), dfv = fv[i] + warp_sum(gbv[i], tf[i]);
            const float dbu = bu[i] + warp_sum(gfu[i], tb[i]), dbv = bv[i] + warp_sum(gfv[i], tb[i]);
            bool cf = flow_len(dfu, dfv) < thresh, cb = flow_len(dbu, dbv) < thresh;
            if (mode == 1) {
                const int p = p0 + i, py = p / w, px = p - py * w;
                cf = cf || outgoing(fu[i], fv[i], px, py, h, w);
                cb = cb || outgoing(bu[i], bv[i], px, py, h, w);
            }
            of[i] = cf ? 1.f : 0.f;
            ob[i] = cb ? 1.f : 0.f;
        }
    }
    if (VEC == 4) {
        *reinterpret_cast<f32x4*>(mfw + p0) = f32x4{of[0], of[1], of[2], of[3]};
        *reinterpret_cast<f32x4*>(mbw + p0) = f32x4{ob[0], ob[1], ob[2], ob[3]};
    } else {
        mfw[p0] = of[0]; mbw[p0] = ob[0];
    }
}

}  // namespace

// n pairs (1..16) of one image size by ONE launch: flow_fw[i], flow_bw[i] [1][2][h][w] and mask_fw_out[i], mask_bw_out[i] [1][1][h][w]
// are host arrays of device pointers, read before the call returns
extern "C" int eemflow_fb_check_many(int n, const float* const* flow_fw, const float* const* flow_bw, float* const* mask_fw_out,
                                     float* const* mask_bw_out, int h, int w, float alpha1, float alpha2, int mode, void* stream) {
    EEM_REQUIRE(n >= 1 && n <= 16, "eemflow_fb_check_many: 1..16 pairs per call; got %d", n);
    EEM_REQUIRE(flow_fw && flow_bw && mask_fw_out && mask_bw_out, "eemflow_fb_check_many: NULL argument");
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 30), "eemflow_fb_check_many: bad size %dx%d", h, w);
    EEM_REQUIRE(mode >= 0 && mode <= 2, "eemflow_fb_check_many: mode %d (0 = all, 1 = obj, 2 = out)", mode);
    FbMany m;
    memset(&m, 0, sizeof(m));
    uintptr_t bits = 0;
    for (int i = 0; i < n; ++i) {
        EEM_REQUIRE(flow_fw[i] && flow_bw[i] && mask_fw_out[i] && mask_bw_out[i], "eemflow_fb_check_many: pair %d has a NULL tensor", i);
        m.fw[i] = flow_fw[i]; m.bw[i] = flow_bw[i]; m.mfw[i] = mask_fw_out[i]; m.mbw[i] = mask_bw_out[i];
        bits |= (uintptr_t)flow_fw[i] | (uintptr_t)flow_bw[i] | (uintptr_t)mask_fw_out[i] | (uintptr_t)mask_bw_out[i];
    }
    hipStream_t st = (hipStream_t)stream;
    const long hw = (long)h * w;
    const bool vec = (hw & 3) == 0 && (bits & 15) == 0;
    if (vec) hipLaunchKernelGGL(fb_check_kernel<4>, dim3((unsigned)((hw / 4 + 255) / 256), n), dim3(256), 0, st, m, h, w, alpha1, alpha2, mode);
    else hipLaunchKernelGGL(fb_check_kernel<1>, dim3((unsigned)((hw + 255) / 256), n), dim3(256), 0, st, m, h, w, alpha1, alpha2, mode);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}
