// Gradient of the variance of the image of warped events (iwe.hip) with respect to the flow: the backward of the contrast-maximisation
// objective.  Per job: the forward's inputs (events [n][4] f64, flow [2][h][w] fp32, t0, scale, the affine event map), the forward's
// STORED fp32 image and its moments, and a scalar coef (fp64, read from device memory: the upstream gradient, and -1 / var0 for the flow
// warp loss).  All arithmetic is unfused fp64 (-ffp-contract=off), and the warp is recomputed by iwe_shared.h's functions, the very
// expressions of the forward, so an event finds the cells it voted into:
//   per cell    S = (double)iwe[0] + (double)iwe[1], n = h * w, mean = moments[1] / n, G = 2 * (S - mean) / n = d var / d S; the fp32
//               rounding of the stored image is the identity (straight-through).  G is not stored: an event computes it in fp64 from
//               the image at its four targets (eight fp32 gathers, L2-served like the flow's)
//   per event   dX = sum over in-frame targets of G[Y0+dy][X0+dx] * wy[dy] * (dx ? +1 : -1), dY = sum of G * wx[dx] * (dy ? +1 : -1),
//               wy = (1-gy, gy), wx = (1-gx, gx); at an integer xw the pair is (X0, X0 + 1) with gx = 0, as the forward's floor has it
//   gradient    for every in-frame sample neighbour k of (xe, ye) with weight w_k: dF[0][k] += coef * w_k * tau * dX,
//               dF[1][k] += coef * w_k * tau * dY; an event dropped whole by the forward, or with no target in the frame, adds nothing
//   output      every cell of the [2][h][w] fp32 gradient is written: an fp64 sum rounded to fp32 once
// A job without a flow (zero flow) has no gradient and is left out of the launches.
//
// An event makes up to eight scattered adds (two at integer event coordinates), to cells around its UN-warped position.  As in the
// forward, the default form bins them - up to IWE_MAX_JOBS jobs of one frame size per launch, blockIdx.y = job:
//   1. iwe_grad_bin_kernel   every block of 1024 threads takes 1024 x EPT events (EPT = 1, or 2 above 4.2 M events) and turns each into
//                            up to four 12-byte records, one per sample neighbour with a non-zero weight: {cell-in-band, du, dv}, du and
//                            dv the two channels' contributions as fp32 (each rounded once: 2^-24 relative).  A band is `rows` whole
//                            rows of BOTH flow channels (the forward's plan), so a record's two values land in one band.  Records are
//                            ranked per band with LDS integer atomics, sorted by band in LDS and leave as whole 16-byte pieces with
//                            the run table run_start[blk][band]: no global atomics.  A record of two zeros is not emitted.
//   2. iwe_grad_band_kernel  one block per band: the band as fp64 LDS cells (ds_add_f64), 2^sgs adjacent lanes share a run; one pass
//                            rounds every cell to fp32 once and stores it.
// Direct form (frames too wide for a one-row band, more than 8.4 M events, or EEM_IWE_DIRECT=1): one thread per event
// adds its contributions, unrounded, with fp64 global atomics into a zeroed fp64 [2][h][w] image in the scratch arena; a finishing pass
// rounds to fp32 (memset + two launches per job).  The order of the adds is free in both forms: the gradient is not bitwise
// reproducible from run to run (its fp64 sums differ by their last bits, far below the fp32 it is rounded to).
// The kernels are iwe_grad_shared.h's, which tsimg.hip instantiates too with its own per-target factor; this file's factor is G above.
#include "iwe_shared.h"
#include "iwe_grad_shared.h"

namespace {

// G = 2 (S - mean) / n from the stored image and the forward's moments row of the job
struct VarFactor {
    double mean, npx;
    __device__ __forceinline__ static VarFactor load(const IweGradJob& J, const double* __restrict__ moments, double) {
        VarFactor f;
        f.npx = moments[4 * J.src];
        f.mean = moments[4 * J.src + 1] / f.npx;
        return f;
    }
    __device__ __forceinline__ double at(const IweGradJob& J, long o, long hw, int, double) const {
        const double S = (double)J.img[o] + (double)J.img[hw + o];
        return 2.0 * (S - mean) / npx;
    }
};

}  // namespace

extern "C" int eemflow_iwe_grad_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                     const double* scale, const double (*maps)[4], int h, int w, const float* const* iwe,
                                     const double* moments, const double* coef, float* const* grads, void* stream_) {
    const int rc = iwe_check_many("eemflow_iwe_grad_many", k, events && n && flows && t0 && scale && maps && iwe && moments && coef && grads, h, w, n);
    if (rc != EEM_OK) return rc;
    int form = 0;
    return iwe_grad_run<VarFactor>("eemflow_iwe_grad_many", k, events, n, flows, t0, scale, maps, h, w, iwe, nullptr, moments, 0.0, coef, grads,
                                   stream_, &form);
}
