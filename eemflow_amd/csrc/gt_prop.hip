// MVSEC ground truth for any window, on the device (eemflow_gt_flow_many): estimate_corresponding_gt_flow / prop_flow of the reference
// (loader/loader_utils.py:70-161, duplicated in utils/mvsec_utils.py).  The ground truth is a 20 Hz stack of displacement maps; the
// target of a window [t0, t1] comes from walking every pixel through the maps the window spans.  The reference does one cv2.remap
// (nearest neighbour, constant border 0) of both components plus one add per map, on the CPU, over whole images; here ONE thread
// walks ONE pixel of ONE job through all its steps with the position in registers - a dependent chain of two 4-byte gathers per step,
// so expect latency, not bandwidth, to bound it (measured: tools/bench_gt_prop.py, profiles/gt_prop_bench.txt).
// The host plans each job (mvsec_raw.MvsecGroundTruth.plan: first frame, number of steps, the scale of the first and of the last
// step); up to 32 jobs travel as kernel arguments (32 x 32 B).
// Arithmetic, bit for bit the reference's on float32 maps:
//   nsteps == 0   out = (float)(((double)gt * a) / b): the early return (the window is shorter than the ground-truth interval); the
//                 reference returns this float64, the library rounds it to fp32 once;
//   nsteps >= 2   x, y start at the pixel's coordinates as fp32; per step ix = rint(x), iy = rint(y) (half to even: cvRound), a
//                 target outside the frame reads 0; fu == 0 clears the x mask and fv == 0 the y mask (independent, sticky);
//                 x = (float)((double)x + (double)fu * scale) - product and sum unfused (-ffp-contract=off), NumPy's float64 loop
//                 of `x_indices += flow * scale` rounded into the float32 array; out = x - x0 (fp32), 0 where the mask is cleared.
// Non-finite values: a NaN flow value is not == 0, so it keeps its mask and makes its component NaN.  A later step finds no cell for a
// non-finite position and reads 0 for both components; that read clears the mask of a component whose own coordinate is still
// finite (the reference's border read), and leaves the mask of the non-finite one: the NaN (or infinity) stays in the output, where
// cv2's conversion of a NaN coordinate to an integer is undefined.  More NaN than the reference, never less.
//
// eemflow_event_mask_windows / eemflow_event_mask_spans: the event masks of the windows of a resident recording (mvsec.event_mask on each slice), read through
// event_cols.h in the columns' own dtypes: a zero-fill launch, then plain stores of 1.0f (every racing store writes the same value).
#include "event_cols.h"

#include <string.h>

#include <algorithm>

namespace {

constexpr int GT_MAX_JOBS = 32;
constexpr int GT_THREADS = 256;

struct GtJob {
    float* out;              // (2,H,W)
    int frame0, nsteps;
    double a, b;             // nsteps == 0: dt and gt_dt; else the scale of the first and of the last step
};
struct GtJobs { GtJob j[GT_MAX_JOBS]; };

__global__ __launch_bounds__(GT_THREADS) void gt_flow_kernel(const float* __restrict__ gt, GtJobs jobs, int h, int w) {
    const GtJob& J = jobs.j[blockIdx.y];
    const long hw = (long)h * w;
    const long i = (long)blockIdx.x * GT_THREADS + threadIdx.x;
    if (i >= hw) return;
    const float* frame = gt + (long)J.frame0 * 2 * hw;
    if (J.nsteps == 0) {                                               // loader_utils.py:110-111
        J.out[i] = (float)(((double)frame[i] * J.a) / J.b);
        J.out[hw + i] = (float)(((double)frame[hw + i] * J.a) / J.b);
        return;
    }
    const float x0 = (float)(int)(i % w), y0 = (float)(int)(i / w);
    float x = x0, y = y0;
    bool mx = true, my = true;
    for (int s = 0; s < J.nsteps; ++s, frame += 2 * hw) {
        const double scale = s == 0 ? J.a : (s == J.nsteps - 1 ? J.b : 1.0);
        const bool finx = __builtin_isfinite(x), finy = __builtin_isfinite(y);
        float fu = 0.f, fv = 0.f;
        if (finx && finy) {
            const float rx = rintf(x), ry = rintf(y);                  // half to even, as cvRound
            if (rx >= 0.f && rx < (float)w && ry >= 0.f && ry < (float)h) {
                const long at = (long)(int)ry * w + (int)rx;
                fu = frame[at];
                fv = frame[hw + at];
            }
        }
        if (fu == 0.f && finx) mx = false;                             // (a scale of 0 - a window ending ON a timestamp - clears as well)
        if (fv == 0.f && finy) my = false;
        x = (float)((double)x + (double)fu * scale);
        y = (float)((double)y + (double)fv * scale);
    }
    J.out[i] = mx ? x - x0 : 0.f;
    J.out[hw + i] = my ? y - y0 : 0.f;
}

struct MaskJobs {
    float* out[GT_MAX_JOBS];
    long long first[GT_MAX_JOBS];
    long long n[GT_MAX_JOBS];
};

__global__ __launch_bounds__(GT_THREADS) void mask_zero_kernel(MaskJobs jobs, long hw) {
    float* out = jobs.out[blockIdx.y];
    for (long i = (long)blockIdx.x * GT_THREADS + threadIdx.x; i < hw; i += (long)gridDim.x * GT_THREADS) out[i] = 0.f;
}

__global__ __launch_bounds__(GT_THREADS) void mask_set_kernel(MaskJobs jobs, const void* __restrict__ xcol, const void* __restrict__ ycol, int code_x,
                                                             int code_y, int h, int w) {
    float* out = jobs.out[blockIdx.y];
    const long first = (long)jobs.first[blockIdx.y], n = (long)jobs.n[blockIdx.y];
    for (long i = (long)blockIdx.x * GT_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * GT_THREADS) {
        const double x = pk_load(xcol, code_x, first + i), y = pk_load(ycol, code_y, first + i);
        if (!(x >= 0.0 && x <= (double)w && y >= 0.0 && y <= (double)h)) continue;      // (a NaN coordinate fails every comparison)
        const int xi = min((int)floor(x), w - 1), yi = min((int)floor(y), h - 1);      // histogram2d: x == w falls into the last bin
        out[(long)yi * w + xi] = 1.0f;
    }
}

}  // namespace

extern "C" int eemflow_gt_flow_many(int njobs, const float* gt, int nframes, int h, int w, const int* frame0, const int* nsteps, const double* a,
                                    const double* b, float* const* out, void* stream) {
    EEM_REQUIRE(njobs >= 1 && njobs <= GT_MAX_JOBS, "eemflow_gt_flow_many: 1..%d jobs per call; got %d", GT_MAX_JOBS, njobs);
    EEM_REQUIRE(gt && frame0 && nsteps && a && b && out, "eemflow_gt_flow_many: NULL argument");
    EEM_REQUIRE(nframes >= 1 && h >= 1 && w >= 1 && (long)h * w <= 0x7fffffffL / 2, "eemflow_gt_flow_many: bad shape frames=%d h=%d w=%d", nframes,
                h, w);
    EEM_REQUIRE(((uintptr_t)gt & 3) == 0, "eemflow_gt_flow_many: the stack is not 4-byte aligned");
    GtJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    for (int k = 0; k < njobs; ++k) {
        EEM_REQUIRE(nsteps[k] == 0 || nsteps[k] >= 2, "eemflow_gt_flow_many: job %d: 0 steps (the short branch) or at least 2; got %d", k, nsteps[k]);
        const long last = (long)frame0[k] + (nsteps[k] ? nsteps[k] - 1 : 0);
        EEM_REQUIRE(frame0[k] >= 0 && last < nframes, "eemflow_gt_flow_many: job %d reads frames %d..%ld of a stack of %d", k, frame0[k], last,
                    nframes);
        EEM_REQUIRE(out[k] != nullptr && ((uintptr_t)out[k] & 3) == 0, "eemflow_gt_flow_many: job %d has no 4-byte aligned output", k);
        jobs.j[k].out = out[k];
        jobs.j[k].frame0 = frame0[k]; jobs.j[k].nsteps = nsteps[k];
        jobs.j[k].a = a[k]; jobs.j[k].b = b[k];
    }
    const long hw = (long)h * w;
    hipLaunchKernelGGL(gt_flow_kernel, dim3((unsigned)((hw + GT_THREADS - 1) / GT_THREADS), njobs), dim3(GT_THREADS), 0, (hipStream_t)stream, gt, jobs,
                       h, w);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}

namespace {

// the body of eemflow_event_mask_windows (starts = offsets, ends = offsets + 1) and eemflow_event_mask_spans
int mask_windows(const char* who, bool offsets, int nwin, const void* x, const void* y, int code_x, int code_y, const int64_t* starts,
                 const int64_t* ends, int h, int w, float* const* masks, void* stream) {
    EEM_REQUIRE(nwin >= 1 && nwin <= GT_MAX_JOBS, "%s: 1..%d windows per call; got %d", who, GT_MAX_JOBS, nwin);
    EEM_REQUIRE(starts && ends && masks, "%s: NULL argument", who);
    EEM_REQUIRE(h >= 1 && w >= 1, "%s: bad shape h=%d w=%d", who, h, w);
    if (offsets) EEM_REQUIRE(starts[0] >= 0, "%s: offsets[0] = %ld", who, (long)starts[0]);
    const int ebx = pk_elem_bytes(code_x), eby = pk_elem_bytes(code_y);
    EEM_REQUIRE(ebx != 0 && eby != 0, "%s: unknown dtype code %d / %d", who, code_x, code_y);
    // the columns are asked about before the windows, as they always were: offsets[nwin] > offsets[0] for the consecutive form
    bool any_event = offsets && ends[nwin - 1] > starts[0];
    for (int k = 0; k < nwin && !offsets; ++k) any_event = any_event || ends[k] > starts[k];
    EEM_REQUIRE((x && y) || !any_event, "%s: a column is NULL", who);
    EEM_REQUIRE(((uintptr_t)x & (uintptr_t)(ebx - 1)) == 0 && ((uintptr_t)y & (uintptr_t)(eby - 1)) == 0, "%s: a column is not aligned to its elements",
                who);
    MaskJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    long nmax = 0;
    for (int k = 0; k < nwin; ++k) {
        if (offsets) {
            EEM_REQUIRE(ends[k] >= starts[k], "%s: the offsets must ascend (window %d: %ld .. %ld)", who, k, (long)starts[k], (long)ends[k]);
        } else {
            EEM_REQUIRE(starts[k] >= 0 && ends[k] >= starts[k], "%s: span %d is [%ld, %ld): 0 <= start <= end", who, k, (long)starts[k], (long)ends[k]);
        }
        EEM_REQUIRE(masks[k] != nullptr && ((uintptr_t)masks[k] & 3) == 0, "%s: window %d has no 4-byte aligned mask", who, k);
        jobs.out[k] = masks[k];
        jobs.first[k] = starts[k];
        jobs.n[k] = ends[k] - starts[k];
        nmax = std::max(nmax, (long)jobs.n[k]);
    }
    const long hw = (long)h * w;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mask_zero_kernel, dim3((unsigned)std::min(1024L, (hw + GT_THREADS - 1) / GT_THREADS), nwin), dim3(GT_THREADS), 0, st, jobs, hw);
    EEM_HIP_CHECK(hipGetLastError());
    if (nmax > 0) {
        hipLaunchKernelGGL(mask_set_kernel, dim3((unsigned)std::min(1024L, (nmax + GT_THREADS - 1) / GT_THREADS), nwin), dim3(GT_THREADS), 0, st, jobs, x,
                           y, code_x, code_y, h, w);
        EEM_HIP_CHECK(hipGetLastError());
    }
    return EEM_OK;
}

}  // namespace

extern "C" int eemflow_event_mask_windows(int nwin, const void* x, const void* y, int code_x, int code_y, const int64_t* offsets, int h, int w,
                                          float* const* masks, void* stream) {
    return mask_windows("eemflow_event_mask_windows", true, nwin, x, y, code_x, code_y, offsets, offsets ? offsets + 1 : nullptr, h, w, masks, stream);
}

extern "C" int eemflow_event_mask_spans(int nwin, const void* x, const void* y, int code_x, int code_y, const int64_t* starts, const int64_t* ends, int h,
                                        int w, float* const* masks, void* stream) {
    return mask_windows("eemflow_event_mask_spans", false, nwin, x, y, code_x, code_y, starts, ends, h, w, masks, stream);
}
