// Image of average timestamps of the warped events, its loss and the loss's gradient with respect to the flow: the objective that
// event-flow learning without ground truth minimises (Zhu et al. 2019; Hagenaars et al. 2021).  The reference has no such loss; the warp
// it is composed with is warp_events_flow_torch (utils_luo/event_utils.py:9-51), i.e. iwe_shared.h's iwe_warp, as in iwe.hip.
//
// A job is an eemflow_iwe_map_many job plus a scalar eps.  All arithmetic is unfused fp64 (-ffp-contract=off):
//   warp, votes, drops   iwe_warp and iwe_votes, unchanged: channel 0 for p > 0 else 1, out-of-frame targets dropped one by one, an event
//                        with a non-finite warped position dropped whole and counted
//   timestamp value      a = max(1 - |tau|, 0), tau = (t - t0) * scale; ah = (double)(float)a, rounded to fp32 once (with t_ref="end" the
//                        normalised timestamp, with "start" one minus it)
//   planes per channel   D = sum of q / 2^31 and N = sum of (q / 2^31) * ah over the votes of a cell, q = round(w * 2^31) the fixed-point
//                        vote weight of iwe.hip: the D sums are exact, so the stored D is bitwise iwe.hip's binned image, and a cell of
//                        one event gives N / D = ah without cancellation.  T = N / (D + eps) from the fp64 sums, rounded to fp32 once.
//                        D and T ([2][h][w] fp32 each) are written in every cell
//   moments              {h*w, sum T^2 over both channels of the STORED T, active = pixels with stored D[0] + D[1] > 0, dropped}, the
//                        final sums in a fixed order.  (N's fp64 sums depend on the order of the adds by their last bits: T is
//                        reproducible to one fp32 ulp, D bit for bit.)
// The forward is iwe_fwd_shared.h's - iwe.hip's binning, band, moments and direct kernels and its host path - under this file's policy:
// 16-byte records {cell-in-band, left weight, right weight, ah as fp32}, a record one whole 16-byte piece; four fp64 LDS planes per band
// (D and N of both channels), whose one finishing pass computes T, stores D and T and leaves the band's (sum T^2, active).  Four planes
// halve iwe.hip's rows per band: 9216 cells are one row at w = 1280, 720 bands at 720 rows; a frame wider than 4800 takes the direct
// form (also EEM_IWE_DIRECT=1, more than 16.7 M events): fp64 global atomics of the same QUANTISED weights into zeroed fp64 D and N
// planes.  What is this file's: ts_finish_px, the policy, the gradient's factor, last_form and the entry points.
//
// Gradient (eemflow_tsimg_grad_many): teacher-forced from the stored T and D, fp32 roundings straight-through.  For an event of channel
// c at an in-frame target cell G = ((2.0 * T) * (ah - T)) / (D + eps) = dL/dN * ah + dL/dD of L = sum T^2; from G on it is
// iwe_grad_shared.h's event, bin, band and direct kernels, which iwe_grad.hip uses with the variance's factor.
#include <stdio.h>

#include "iwe_fwd_shared.h"
#include "iwe_grad_shared.h"

namespace {

// what a pixel's four fp64 sums leave: D and T rounded to fp32 once each, T^2 of the stored T, and whether the pixel is active
__device__ __forceinline__ void ts_finish_px(double d0, double d1, double n0, double n1, double eps, float& D0, float& D1, float& T0, float& T1,
                                             double& sq, double& act) {
    D0 = (float)d0;
    D1 = (float)d1;
    T0 = (float)(n0 / (d0 + eps));
    T1 = (float)(n1 / (d1 + eps));
    sq += (double)T0 * (double)T0;
    sq += (double)T1 * (double)T1;
    if ((double)D0 + (double)D1 > 0.0) act += 1.0;
}

// The forward's policy (iwe_fwd_shared.h): four planes - D of channel 0, 1, then N of channel 0, 1 -, 16-byte records whose fourth word is
// ah as fp32; a weight adds itself to D and itself times ah to N; a pixel leaves ts_finish_px's; the direct form adds the same QUANTISED
// weights, so D is the binned image in both forms
struct TsPolicy {
    static constexpr int PLANES = 4, WORDS = 4;
    static constexpr bool FIXED_DIRECT = true;
    double eps;
    __device__ __forceinline__ static unsigned payload(const IweEvent& e) { return __float_as_uint(iwe_time_value(e.tau)); }
    template <bool LDS>
    __device__ __forceinline__ static void add(double* cell, long nofs, double wgt, unsigned pay) {
        iwe_add<LDS>(cell, wgt);
        iwe_add<LDS>(cell + nofs, wgt * (double)__uint_as_float(pay));
    }
    template <class I>
    __device__ __forceinline__ void leave(const double* px, I stride, I i, float* __restrict__ od, float* __restrict__ ot, long hw, double& sq,
                                          double& act) const {
        float D0, D1, T0, T1;
        ts_finish_px(px[i], px[stride + i], px[2 * stride + i], px[3 * stride + i], eps, D0, D1, T0, T1, sq, act);
        od[i] = D0;
        od[hw + i] = D1;
        ot[i] = T0;
        ot[hw + i] = T1;
    }
};

// what this thread's last call ran (eemflow_tsimg_last_form): written on the host after a call's launches went out
thread_local char ts_last_form[64] = "";

// the checks of both entry points, under the entry's name
inline int ts_check(const char* name, int k, bool nonnull, int h, int w, const int64_t* n, double eps) {
    const int rc = iwe_check_many(name, k, nonnull, h, w, n);
    if (rc != EEM_OK) return rc;
    EEM_REQUIRE(eps > 0.0 && eps < 1e300, "%s: eps=%g is not a positive finite number", name, eps);
    return EEM_OK;
}

// G = ((2 T) (ah - T)) / (D + eps) from the stored T (img) and D (img2) of the event's channel
struct TsFactor {
    double eps;
    __device__ __forceinline__ static TsFactor load(const IweGradJob&, const double*, double eps) { return TsFactor{eps}; }
    __device__ __forceinline__ double at(const IweGradJob& J, long o, long hw, int c, double ah) const {
        const double T = (double)J.img[c * hw + o], D = (double)J.img2[c * hw + o];
        return ((2.0 * T) * (ah - T)) / (D + eps);
    }
};

}  // namespace

extern "C" int eemflow_tsimg_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                  const double* scale, const double (*maps)[4], int h, int w, double eps, float* const* iwe_out,
                                  float* const* ts_out, double* moments, void* stream) {
    int rc = ts_check("eemflow_tsimg_many", k, events && n && t0 && scale && maps && iwe_out && ts_out && moments, h, w, n, eps);
    if (rc != EEM_OK) return rc;
    for (int i = 0; i < k; ++i)
        EEM_REQUIRE((events[i] || n[i] == 0) && iwe_out[i] && ts_out[i], "eemflow_tsimg_many: job %d has a NULL buffer", i);
    IweFwdForm form;
    rc = iwe_fwd_launch(TsPolicy{eps}, k, events, n, flows, t0, scale, maps, h, w, iwe_out, ts_out, moments, stream, &form);
    if (rc == EEM_OK) {
        if (form.ept == 0) snprintf(ts_last_form, sizeof(ts_last_form), "direct");
        else snprintf(ts_last_form, sizeof(ts_last_form), "bin_e%d+band%d_s%d+moments", form.ept, form.bt, form.sgs);
    }
    return rc;
}

extern "C" int eemflow_tsimg_grad_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                       const double* scale, const double (*maps)[4], int h, int w, double eps, const float* const* iwe,
                                       const float* const* ts, const double* coef, float* const* grads, void* stream) {
    int rc = ts_check("eemflow_tsimg_grad_many", k, events && n && flows && t0 && scale && maps && iwe && ts && coef && grads, h, w, n, eps);
    if (rc != EEM_OK) return rc;
    int form = 0;
    rc = iwe_grad_run<TsFactor>("eemflow_tsimg_grad_many", k, events, n, flows, t0, scale, maps, h, w, ts, iwe, nullptr, eps, coef,
                                          grads, stream, &form);
    if (rc == EEM_OK && form != 0) {
        if (form < 0) snprintf(ts_last_form, sizeof(ts_last_form), "grad_direct");
        else snprintf(ts_last_form, sizeof(ts_last_form), "grad_bin_e%d+grad_band", form);
    }
    return rc;
}

extern "C" int eemflow_tsimg_last_form(char* buf, int cap) {
    EEM_REQUIRE(buf && cap >= 1, "eemflow_tsimg_last_form: bad arguments");
    snprintf(buf, (size_t)cap, "%s", ts_last_form);
    return EEM_OK;
}
