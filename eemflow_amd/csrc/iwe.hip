// Image of warped events (IWE) and its moments, the ground-truth-free quality measure of an event-camera flow (reference: the warp is
// warp_events_flow_torch, utils_luo/event_utils.py:9-51; the loop around it Test.inference_img_warp_loss, test_mvsec.py:753-852, whose
// variance-ratio form of the flow warp loss sits at :821-824).
//
// Per job: events [n][4] f64 (t, x, y, p), time-sorted; a flow [2][h][w] fp32 or NULL (zero flow); scalars t0, scale and an affine event
// map (ax, bx, ay, by) - an offset (ox, oy) is (1, -ox, 1, -oy), the same bits.  All arithmetic is fp64 and unfused (this file is built
// with -ffp-contract=off; the per-event functions live in iwe_shared.h, which the gradient, iwe_grad.hip, includes too).  This file
// holds the objective's policy, the warp-alone kernel, the scratch arena and the entry points; the kernels and the host path described
// below are iwe_fwd_shared.h's, which tsimg.hip instantiates too with its own policy:
//   warp        xe = ax * x + bx, ye = ay * y + by; (u, v) = the bilinear sample of the flow at (xe, ye) in pixel coordinates - x0 = floor(xe),
//               fx = xe - x0, the four neighbours weighted (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy and summed in that order, a
//               neighbour outside [0, w-1] x [0, h-1] contributing 0 (grid_sample, align_corners=True, zero padding);
//               tau = (t - t0) * scale; xw = xe + u * tau, yw = ye + v * tau
//   accumulate  channel c = 0 for p > 0, else 1; X0 = floor(xw), gx = xw - X0 (the same in y); four votes (1-gx)(1-gy), gx(1-gy),
//               (1-gx)gy, gx gy to (c, Y0 + dy, X0 + dx); a target outside the frame is dropped on its own (no wrap into the next
//               row); an event whose xw or yw is not finite is dropped whole and counted; every cell's votes are summed in fp64 and
//               rounded to fp32 once; every cell of the [2][h][w] fp32 image is written (no memset by the caller)
//   moments     S = (double)iwe[0] + (double)iwe[1] of the STORED fp32 values; {h*w, sum S, sum S^2, dropped} as four doubles per job,
//               the final sums in a fixed order
//
// Events arrive time-sorted, so neighbouring lanes vote into unrelated cells, and an event now makes four votes (voxel.hip: two): by
// voxel.hip's measured ~20 G scattered atomics/s to HBM, 8e6 votes of a 1280x720 sample are ~0.4 ms.  The default path therefore bins
// the votes and adds them in LDS, as the voxelizer does - up to IWE_MAX_JOBS jobs of one frame size per launch, blockIdx.y = job:
//   1. iwe_fwd_bin_kernel every block of 1024 threads warps its 1024 x EPT events (EPT = 1, 2, 4 by event count, or EEM_IWE_EPT; the
//                         flow gather is served from L2) and turns each into up to two ROW records, one for row Y0 and one for Y0 + 1: 12 bytes
//                         {cell-in-band (channel included), left weight, right weight}.  A band is `rows` whole image rows of both
//                         channels, so the two cells X0, X0 + 1 of a record never straddle bands, while the two records of an event
//                         may.  Records are ranked per band with LDS integer atomics, sorted by band IN LDS and leave as whole
//                         16-byte pieces, with a row of run offsets run_start[blk][band]: no global atomics, no counting pass.
//                         The weights travel as UNSIGNED FIXED POINT, q = round(w * 2^31): the fp32 product wy * wx would be off by
//                         up to 2^-25 (3e-8) per vote, 7.5e-6 over the 250 votes a cell may collect in the tests, which allow 1e-6
//                         beside one fp32 ulp; the fixed-point weight is off by at most 2^-32 (2.3e-10, 5.8e-8 over 250 votes) in
//                         the same 12 bytes, weights 0 and 1 are exact, and a band cell's fp64 sum of such weights is EXACT below
//                         2^22 votes, so the image does not depend on the order of the adds.
//                         X0 = -1 is stored as cell 0 with the right weight in the left slot; at X0 = w - 1 the right weight is 0.
//                         A record whose two weights are 0 is not emitted (integer coordinates emit one record per event).
//   2. iwe_fwd_band_kernel one block per band: the band as fp64 LDS cells (ds_add_f64: the LDS fp32 add is 8 - 20 x slower on this
//                         chip, profiles/r04_lds_atomics.txt), 2^sgs adjacent lanes share a run (the band's records of one binning
//                         block); one pass then rounds every cell to fp32 once, stores both channels and leaves the band's
//                         (sum S, sum S^2).  9216 cells (72 KB) at most: 3 rows at w = 1280, 240 bands at 720 rows.
//   3. iwe_fwd_moments_kernel one block per job adds the band partials and the binning blocks' drop counts in a fixed order.
// Direct form (frames too wide for a one-row band, more than 16.7 M events, or EEM_IWE_DIRECT=1): one thread per
// event adds its votes with global atomics.  The image's contract is an fp64 sum rounded once - a chain of fp32 atomic adds is off by
// up to one rounding per vote, several ulps of the cell, where one ulp is allowed - so the direct form adds fp64 atomics into a zeroed
// fp64 image in the scratch arena, and a finishing pass rounds, stores and takes the moments (memset + two launches + the moments
// launch, one job after the other).
#include "iwe_shared.h"
#include "iwe_fwd_shared.h"

namespace {

// The forward's policy (iwe_fwd_shared.h): two planes, 12-byte records without a payload; a pixel stores both channels rounded to fp32
// once and counts S = their sum of the STORED values into (sum S, sum S^2); the direct form adds the plain fp64 products
struct IwePolicy {
    static constexpr int PLANES = 2, WORDS = 3;
    static constexpr bool FIXED_DIRECT = false;
    __device__ __forceinline__ static unsigned payload(const IweEvent&) { return 0u; }
    template <bool LDS>
    __device__ __forceinline__ static void add(double* cell, long, double wgt, unsigned) { iwe_add<LDS>(cell, wgt); }
    template <class I>
    __device__ __forceinline__ void leave(const double* px, I stride, I i, float* __restrict__ out, float*, long hw, double& sm, double& sq) const {
        const float v0 = (float)px[i], v1 = (float)px[stride + i];
        out[i] = v0;
        out[hw + i] = v1;
        const double S = (double)v0 + (double)v1;
        sm += S;
        sq += S * S;
    }
};

// the warp alone: warped_xy [n][2] f64
__global__ __launch_bounds__(256) void iwe_warp_kernel(const double* __restrict__ ev, long n, const float* __restrict__ flow, double t0,
                                                       double scale, double ox, double oy, int h, int w, double* __restrict__ xy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const IweEvent e = iwe_warp(ev, i, flow, t0, scale, IweMap{1.0, -ox, 1.0, -oy}, h, w);
    xy[2 * i] = e.xw;
    xy[2 * i + 1] = e.yw;
}

Arena g_iwe_arena;

}  // namespace

Arena& iwe_arena() { return g_iwe_arena; }

extern "C" int eemflow_iwe_map_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                    const double* scale, const double (*maps)[4], int h, int w, float* const* iwe, double* moments,
                                    void* stream) {
    const int rc = iwe_check_many("eemflow_iwe_many", k, events && n && t0 && scale && maps && iwe && moments, h, w, n);
    if (rc != EEM_OK) return rc;
    for (int i = 0; i < k; ++i) EEM_REQUIRE((events[i] || n[i] == 0) && iwe[i], "eemflow_iwe_many: job %d has a NULL buffer", i);
    IweFwdForm form;
    return iwe_fwd_launch(IwePolicy{}, k, events, n, flows, t0, scale, maps, h, w, iwe, nullptr, moments, stream, &form);
}

extern "C" int eemflow_iwe_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                const double* scale, double ox, double oy, int h, int w, float* const* iwe, double* moments, void* stream) {
    EEM_REQUIRE(k >= 1 && k <= IWE_MAX_JOBS, "eemflow_iwe_many: 1..%d jobs per call; got %d", IWE_MAX_JOBS, k);
    double maps[IWE_MAX_JOBS][4];
    for (int i = 0; i < k; ++i) { maps[i][0] = 1.0; maps[i][1] = -ox; maps[i][2] = 1.0; maps[i][3] = -oy; }
    return eemflow_iwe_map_many(k, events, n, flows, t0, scale, maps, h, w, iwe, moments, stream);
}

extern "C" int eemflow_warp_events(const double* events, int64_t n, const float* flow, int h, int w, double t0, double scale, double ox,
                                   double oy, double* warped_xy, void* stream) {
    EEM_REQUIRE(n >= 0 && n < (1LL << 40), "eemflow_warp_events: n=%ld events", (long)n);
    EEM_REQUIRE((events && warped_xy) || n == 0, "eemflow_warp_events: NULL argument");
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 30), "eemflow_warp_events: bad size %dx%d", h, w);
    if (n == 0) return EEM_OK;
    hipLaunchKernelGGL(iwe_warp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, events, (long)n, flow, t0, scale,
                       ox, oy, h, w, warped_xy);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}
