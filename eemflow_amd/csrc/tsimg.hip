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
// Binned form, as iwe.hip's (up to IWE_MAX_JOBS jobs of one frame size per launch, blockIdx.y = job):
//   1. ts_bin_kernel      iwe_bin_kernel with 16-byte records {cell-in-band, left weight, right weight, ah as fp32}: a record is one
//                         whole 16-byte piece
//   2. ts_band_kernel     one block per band, four fp64 LDS planes (D and N of both channels, ds_add_f64); one pass computes T, stores D
//                         and T and leaves the band's (sum T^2, active).  Four planes halve iwe.hip's rows per band: 9216 cells are one
//                         row at w = 1280, 720 bands at 720 rows; a frame wider than 4800 takes the direct form
//   3. ts_moments_kernel  one block per job adds the band partials and the binning blocks' drop counts in a fixed order
// Direct form (EEM_IWE_DIRECT=1, frames the plan refuses, more than 16.7 M events): fp64 global atomics of the same QUANTISED weights into
// zeroed fp64 D and N planes in the scratch arena, a finishing pass, the moments kernel - one job after the other.
//
// Gradient (eemflow_tsimg_grad_many): teacher-forced from the stored T and D, fp32 roundings straight-through.  For an event of channel
// c at an in-frame target cell G = ((2.0 * T) * (ah - T)) / (D + eps) = dL/dN * ah + dL/dD of L = sum T^2; from G on it is
// iwe_grad_shared.h's event, bin, band and direct kernels, which iwe_grad.hip uses with the variance's factor.
#include <stdio.h>

#include "iwe_grad_shared.h"

namespace {

struct TsJob {
    const double* ev;
    const float* flow;       // NULL: zero flow
    float* out_d;            // [2][h][w] votes
    float* out_t;            // [2][h][w] average timestamps
    u32x4* recs;             // 16-byte records, a slab of 2 * VT * EPT per binning block; behind the nblk slabs the run table
                             // run_start[nblk][nb + 1] (ts_run_table: the job stays at iwe.hip's 120 bytes of kernel arguments)
    double* part;            // [parts][2]: (sum T^2, active) of a band (binned) or of a finishing block (direct)
    double* dropped;         // [nblk]
    double t0, scale;
    IweMap map;
    long n;
    int nblk;
    int pad;
};
struct TsJobs { TsJob j[IWE_MAX_JOBS]; };        // 120 bytes each: 3.8 KB of kernel arguments at 32 jobs
static_assert(sizeof(TsJob) == 120, "TsJobs must stay below 4 KB of kernel arguments");

// the run table of a job: behind its nblk slabs of `slab` records (a slab is a multiple of 256 bytes)
__device__ __forceinline__ unsigned* ts_run_table(const TsJob& J, int slab) { return reinterpret_cast<unsigned*>(J.recs + (size_t)J.nblk * slab); }

constexpr double TS_UNIT = 1.0 / 2147483648.0;   // a fixed-point weight's unit, 2^-31

__device__ __forceinline__ unsigned ts_fix(double wgt) { return (unsigned)(wgt * 2147483648.0 + 0.5); }       // iwe.hip's iwe_fix

// ------------------------------------------------------------------------------------------------ 1. binning into slabs
template <int EPT>
__global__ __launch_bounds__(VT) void ts_bin_kernel(TsJobs jobs, int h, int w, IwePlan pl) {
    const TsJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // a shorter event set of the launch
    const double* __restrict__ ev = J.ev;
    const float* __restrict__ flow = J.flow;
    const long n = J.n;
    const double t0 = J.t0, scale = J.scale;
    __shared__ unsigned hist[VT];
    __shared__ unsigned lpos[VT];
    __shared__ unsigned sh[VT / 64];
    __shared__ unsigned ndrop;
    extern __shared__ __attribute__((aligned(16))) u32x4 stage4[];     // the slab as it goes to memory
    const int tid = threadIdx.x;
    hist[tid] = 0;
    if (tid == 0) ndrop = 0;
    __syncthreads();
    unsigned key[2 * EPT], band[2 * EPT], rank[2 * EPT], ql[2 * EPT], qr[2 * EPT], qa[EPT];
    unsigned drop = 0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long i = ((long)blockIdx.x * EPT + k) * VT + tid;
        band[2 * k] = band[2 * k + 1] = NONE;
        qa[k] = 0;
        if (i < n) {
            const IweEvent e = iwe_warp(ev, i, flow, t0, scale, J.map, h, w);
            const IweVotes q = iwe_votes(e, h, w);
            if (!q.finite) ++drop;
            if (q.inside) {
                qa[k] = __float_as_uint(iwe_time_value(e.tau));
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int Y = q.Y0 + dy;
                    const double wy = dy ? q.gy : 1.0 - q.gy;
                    if (Y >= 0 && Y < h) {
                        double wl = wy * (1.0 - q.gx), wr = wy * q.gx;
                        int X = q.X0;
                        if (X < 0) { X = 0; wl = wr; wr = 0.0; }   // the left target is outside: the right one in the left slot
                        else if (X == w - 1) wr = 0.0;             // the right target is outside (it does not wrap into the next row)
                        const unsigned a = ts_fix(wl), b = ts_fix(wr);
                        if (a | b) {
                            const unsigned bd = (unsigned)Y / (unsigned)pl.rows;
                            band[2 * k + dy] = bd;
                            key[2 * k + dy] = (unsigned)(e.c * pl.rows + (Y - (int)bd * pl.rows)) * (unsigned)w + (unsigned)X;
                            ql[2 * k + dy] = a;
                            qr[2 * k + dy] = b;
                            rank[2 * k + dy] = atomicAdd(&hist[bd], 1u);       // LDS: the returned count is the rank inside the run
                        }
                    }
                }
            }
        }
    }
    if (drop) atomicAdd(&ndrop, drop);
    __syncthreads();
    const unsigned start = block_exscan(hist[tid], sh);            // bands >= nb hold 0: thread nb gets the slab's fill
    lpos[tid] = start;
    if (tid <= pl.nb) ts_run_table(J, 2 * VT * EPT)[(size_t)blockIdx.x * (pl.nb + 1) + tid] = start;
    if (tid == 0) J.dropped[blockIdx.x] = (double)ndrop;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * EPT; ++k) {
        if (band[k] != NONE) {
            u32x4 r;
            r.x = key[k];
            r.y = ql[k];
            r.z = qr[k];
            r.w = qa[k >> 1];
            stage4[lpos[band[k]] + rank[k]] = r;
        }
    }
    __syncthreads();
    const unsigned fill = lpos[pl.nb];                             // <= 2 * VT * EPT records: inside the slab
    u32x4* slab = J.recs + (size_t)blockIdx.x * (2 * VT * EPT);
    for (unsigned i = tid; i < fill; i += VT) slab[i] = stage4[i];
}

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

// ------------------------------------------------------------------------------------------------ 2. bands in LDS
template <int BT>
__global__ __launch_bounds__(BT) void ts_band_kernel(TsJobs jobs, int slab, int h, int w, IwePlan pl, int sgs, double eps) {
    const TsJob& J = jobs.j[blockIdx.y];
    const u32x4* __restrict__ recs = J.recs;
    const unsigned* __restrict__ run_start = ts_run_table(J, slab);
    const int nblk = J.nblk;
    extern __shared__ __attribute__((aligned(16))) double cells[];     // [4][rows][w]: D of channel 0, 1, then N of channel 0, 1
    __shared__ double sh2[2 * BT / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    for (int i = tid; i < pl.cells; i += BT) cells[i] = 0.0;
    __syncthreads();
    const int plane = pl.rows * w;
    double* __restrict__ ncells = cells + 2 * plane;
    // a run = this band's records of one binning block; 2^sgs adjacent lanes share a run, so a wave's loads touch a few runs' lines
    const int sub = tid & ((1 << sgs) - 1);
    const int rpp = BT >> sgs;                                     // runs per pass of the block
    for (int s = tid >> sgs; s < nblk; s += rpp) {
        const unsigned* row = run_start + (size_t)s * (pl.nb + 1) + b;
        const unsigned st = row[0], en = row[1];
        const u32x4* base = recs + (size_t)s * slab;
        for (unsigned k = st + (unsigned)sub; k < en; k += 1u << sgs) {
            const u32x4 r = base[k];
            const unsigned cell = r.x;                             // < 2 * plane (channel included)
            const double ah = (double)__uint_as_float(r.w);
            const double wl = (double)r.y * TS_UNIT;
            atomicAdd(cells + cell, wl);
            atomicAdd(ncells + cell, wl * ah);
            if (r.z) {                                             // (0 at the row's last column: no touch of the next row)
                const double wr = (double)r.z * TS_UNIT;
                atomicAdd(cells + cell + 1, wr);
                atomicAdd(ncells + cell + 1, wr * ah);
            }
        }
    }
    __syncthreads();
    const int y0 = b * pl.rows;
    const int npx = min(pl.rows, h - y0) * w;
    const long hw = (long)h * w;
    float* __restrict__ od = J.out_d + (long)y0 * w;
    float* __restrict__ ot = J.out_t + (long)y0 * w;
    double sq = 0.0, act = 0.0;
    for (int i = tid; i < npx; i += BT) {
        float D0, D1, T0, T1;
        ts_finish_px(cells[i], cells[plane + i], ncells[i], ncells[plane + i], eps, D0, D1, T0, T1, sq, act);
        od[i] = D0;
        od[hw + i] = D1;
        ot[i] = T0;
        ot[hw + i] = T1;
    }
    block_sum2<BT>(sq, act, sh2);
    if (tid == 0) { J.part[2 * b] = sq; J.part[2 * b + 1] = act; }
}

// ------------------------------------------------------------------------------------------------ 3. moments
// one block per job: {h*w, sum T^2, active, dropped} from the partials, added in a fixed order
__global__ __launch_bounds__(256) void ts_moments_kernel(TsJobs jobs, int nparts, double hw, double* __restrict__ moments) {
    const TsJob& J = jobs.j[blockIdx.x];
    __shared__ double sh2[2 * 256 / 64];
    const int tid = threadIdx.x;
    double sq = 0.0, act = 0.0, dr = 0.0, zero = 0.0;
    for (int k = tid; k < nparts; k += 256) { sq += J.part[2 * k]; act += J.part[2 * k + 1]; }
    for (int k = tid; k < J.nblk; k += 256) dr += J.dropped[k];
    block_sum2<256>(sq, act, sh2);
    block_sum2<256>(dr, zero, sh2);
    if (tid == 0) {
        double* m = moments + 4 * blockIdx.x;
        m[0] = hw; m[1] = sq; m[2] = act; m[3] = dr;
    }
}

// ------------------------------------------------------------------------------------------------ direct form
// acc: [4][h][w] fp64, D of channel 0, 1, then N of channel 0, 1
__global__ __launch_bounds__(256) void ts_direct_kernel(const double* __restrict__ ev, long n, const float* __restrict__ flow, double t0,
                                                        double scale, IweMap map, int h, int w, double* __restrict__ acc,
                                                        unsigned long long* __restrict__ ndrop) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const IweEvent e = iwe_warp(ev, i, flow, t0, scale, map, h, w);
    const IweVotes q = iwe_votes(e, h, w);
    if (!q.finite) atomicAdd(ndrop, 1ull);
    if (!q.inside) return;
    const long hw = (long)h * w;
    const double ah = (double)iwe_time_value(e.tau);
    double* dpl = acc + (long)e.c * hw;
    double* npl = dpl + 2 * hw;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int Y = q.Y0 + dy;
        const double wy = dy ? q.gy : 1.0 - q.gy;
        if (Y < 0 || Y >= h) continue;
        const unsigned a = q.X0 >= 0 ? ts_fix(wy * (1.0 - q.gx)) : 0u, b = q.X0 + 1 <= w - 1 ? ts_fix(wy * q.gx) : 0u;
        const long o = (long)Y * w + q.X0;
        if (a) {
            const double wl = (double)a * TS_UNIT;
            unsafeAtomicAdd(dpl + o, wl);
            unsafeAtomicAdd(npl + o, wl * ah);
        }
        if (b) {
            const double wr = (double)b * TS_UNIT;
            unsafeAtomicAdd(dpl + o + 1, wr);
            unsafeAtomicAdd(npl + o + 1, wr * ah);
        }
    }
}

__global__ __launch_bounds__(256) void ts_direct_finish_kernel(const double* __restrict__ acc, const unsigned long long* __restrict__ ndrop,
                                                               float* __restrict__ od, float* __restrict__ ot, long hw, double eps,
                                                               double* __restrict__ part, double* __restrict__ dropped) {
    __shared__ double sh2[2 * 256 / 64];
    double sq = 0.0, act = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
        float D0, D1, T0, T1;
        ts_finish_px(acc[i], acc[hw + i], acc[2 * hw + i], acc[3 * hw + i], eps, D0, D1, T0, T1, sq, act);
        od[i] = D0;
        od[hw + i] = D1;
        ot[i] = T0;
        ot[hw + i] = T1;
    }
    block_sum2<256>(sq, act, sh2);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sq;
        part[2 * blockIdx.x + 1] = act;
        if (blockIdx.x == 0) dropped[0] = (double)*ndrop;
    }
}

// ------------------------------------------------------------------------------------------------ host
inline int ts_ept(long n) {                                        // iwe.hip's choice, under the same switch
    const int forced = sw_int<SW_EEM_IWE_EPT>();
    if ((forced == 1 || forced == 2 || forced == 4) && iwe_blocks(n, forced) <= IWE_MAX_BLOCKS) return forced;
    int ept = 1;
    while (ept < 4 && iwe_blocks(n, ept) > 512) ept *= 2;
    return ept;
}
constexpr int TS_DIRECT_PARTS = 256;
constexpr int TS_CPP = 4;                                          // fp64 LDS cells per pixel of a band

struct TsLayout { size_t recs, table, part, dropped, total; };

TsLayout ts_layout(long n, int ept, const IwePlan& pl) {
    const size_t nblk = (size_t)iwe_blocks(n, ept);
    TsLayout l;
    l.recs = 0;
    l.table = nblk * (size_t)(2 * VT * ept) * 16;                  // (a multiple of 256: ts_run_table finds the table there)
    l.part = l.table + up256((nblk * (size_t)(pl.nb + 1) + 1) * 4);
    l.dropped = l.part + up256((size_t)pl.nb * 16);
    l.total = l.dropped + up256((nblk + 1) * 8);
    return l;
}

template <int EPT>
int ts_launch_bin(const TsJobs& jobs, int njobs, long nblk_max, int h, int w, const IwePlan& pl, hipStream_t stream) {
    constexpr int stage_bytes = 2 * VT * EPT * 16;
    if (stage_bytes > 32 * 1024) EEM_RAISE_LDS(stage_bytes, ts_bin_kernel<EPT>);
    hipLaunchKernelGGL((ts_bin_kernel<EPT>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, h, w, pl);
    return EEM_OK;
}

// what this thread's last call ran (eemflow_tsimg_last_form): written on the host after a call's launches went out
thread_local char ts_last_form[64] = "";

int ts_launch(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0, const double* scale,
              const double (*maps)[4], int h, int w, double eps, float* const* dimg, float* const* timg, double* moments, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    long nmax = 0;
    for (int i = 0; i < k; ++i) nmax = std::max(nmax, (long)n[i]);
    const long hw = (long)h * w;
    IwePlan pl;
    const bool binned = iwe_plan(nmax, h, w, &pl, 4, TS_CPP);
    const int ept = ts_ept(nmax);
    size_t need = 0;
    if (binned)
        for (int i = 0; i < k; ++i) need += ts_layout((long)n[i], ept, pl).total;
    else
        need = up256((size_t)4 * hw * 8 + 8) + up256((size_t)TS_DIRECT_PARTS * 16) + 256;
    Arena& arena = iwe_arena();
    std::lock_guard<std::mutex> guard(arena.lock);
    char* scratch = nullptr;
    void* token = nullptr;
    int rc = arena.take(need, stream_, &scratch, &token);
    if (rc != EEM_OK) return rc;
    TsJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    if (!binned) {
        // direct form, one job after the other through one set of fp64 planes
        double* acc = reinterpret_cast<double*>(scratch);
        unsigned long long* ndrop = reinterpret_cast<unsigned long long*>(acc + 4 * hw);
        double* part = reinterpret_cast<double*>(scratch + up256((size_t)4 * hw * 8 + 8));
        double* dropped = part + 2 * TS_DIRECT_PARTS;
        const int parts = (int)std::min<long>(TS_DIRECT_PARTS, (hw + 255) / 256);
        for (int i = 0; i < k; ++i) {
            EEM_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)4 * hw * 8 + 8, stream));
            if (n[i] > 0)
                hipLaunchKernelGGL(ts_direct_kernel, dim3((unsigned)((n[i] + 255) / 256)), dim3(256), 0, stream, events[i], (long)n[i],
                                   flows ? flows[i] : nullptr, t0[i], scale[i], IweMap{maps[i][0], maps[i][1], maps[i][2], maps[i][3]}, h, w,
                                   acc, ndrop);
            hipLaunchKernelGGL(ts_direct_finish_kernel, dim3(parts), dim3(256), 0, stream, acc, ndrop, dimg[i], timg[i], hw, eps, part, dropped);
            TsJobs one;
            memset(&one, 0, sizeof(one));
            one.j[0].part = part;
            one.j[0].dropped = dropped;
            one.j[0].nblk = 1;
            hipLaunchKernelGGL(ts_moments_kernel, dim3(1), dim3(256), 0, stream, one, parts, (double)hw, moments + 4 * i);
            EEM_HIP_CHECK(hipGetLastError());
        }
        rc = arena.done(token, stream_);
        if (rc == EEM_OK) snprintf(ts_last_form, sizeof(ts_last_form), "direct");
        return rc;
    }
    long nblk_max = 0;
    char* q = scratch;
    for (int i = 0; i < k; ++i) {
        const TsLayout l = ts_layout((long)n[i], ept, pl);
        TsJob& J = jobs.j[i];
        J.ev = events[i];
        J.flow = flows ? flows[i] : nullptr;
        J.out_d = dimg[i];
        J.out_t = timg[i];
        J.recs = reinterpret_cast<u32x4*>(q + l.recs);
        J.part = reinterpret_cast<double*>(q + l.part);
        J.dropped = reinterpret_cast<double*>(q + l.dropped);
        J.t0 = t0[i];
        J.scale = scale[i];
        J.map = IweMap{maps[i][0], maps[i][1], maps[i][2], maps[i][3]};
        J.n = (long)n[i];
        J.nblk = (int)iwe_blocks((long)n[i], ept);
        nblk_max = std::max(nblk_max, (long)J.nblk);
        q += l.total;
    }
    if (nblk_max > 0) {
        switch (ept) {
            case 1: rc = ts_launch_bin<1>(jobs, k, nblk_max, h, w, pl, stream); break;
            case 2: rc = ts_launch_bin<2>(jobs, k, nblk_max, h, w, pl, stream); break;
            default: rc = ts_launch_bin<4>(jobs, k, nblk_max, h, w, pl, stream); break;
        }
        if (rc != EEM_OK) return rc;
    }
    const int lds = pl.cells * 8;
    // lanes per run: the smallest power of two >= 1.7 x the mean run length (a slab's records / bands), 4 .. 64
    int sgs = 2;
    while (sgs < 6 && (1 << sgs) * 10L * pl.nb < 17L * 2 * VT * ept) ++sgs;
    const int bt = pl.cells <= 3072 ? 256 : VT;
    if (bt == 256) {
        hipLaunchKernelGGL(ts_band_kernel<256>, dim3(pl.nb, k), dim3(256), lds, stream, jobs, 2 * VT * ept, h, w, pl, sgs, eps);
    } else {
        if (lds > 32 * 1024) EEM_RAISE_LDS(lds, ts_band_kernel<VT>);
        hipLaunchKernelGGL(ts_band_kernel<VT>, dim3(pl.nb, k), dim3(VT), lds, stream, jobs, 2 * VT * ept, h, w, pl, sgs, eps);
    }
    hipLaunchKernelGGL(ts_moments_kernel, dim3(k), dim3(256), 0, stream, jobs, pl.nb, (double)hw, moments);
    EEM_HIP_CHECK(hipGetLastError());
    rc = arena.done(token, stream_);
    if (rc == EEM_OK) snprintf(ts_last_form, sizeof(ts_last_form), "bin_e%d+band%d_s%d+moments", ept, bt, sgs);
    return rc;
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
    EEM_REQUIRE(k >= 1 && k <= IWE_MAX_JOBS, "eemflow_tsimg_many: 1..%d jobs per call; got %d", IWE_MAX_JOBS, k);
    EEM_REQUIRE(events && n && t0 && scale && maps && iwe_out && ts_out && moments, "eemflow_tsimg_many: NULL argument");
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 30), "eemflow_tsimg_many: bad size %dx%d", h, w);
    EEM_REQUIRE(eps > 0.0 && eps < 1e300, "eemflow_tsimg_many: eps=%g is not a positive finite number", eps);
    for (int i = 0; i < k; ++i) {
        EEM_REQUIRE(n[i] >= 0 && n[i] < (1LL << 40), "eemflow_tsimg_many: job %d has n=%ld events", i, (long)n[i]);
        EEM_REQUIRE((events[i] || n[i] == 0) && iwe_out[i] && ts_out[i], "eemflow_tsimg_many: job %d has a NULL buffer", i);
    }
    return ts_launch(k, events, n, flows, t0, scale, maps, h, w, eps, iwe_out, ts_out, moments, stream);
}

extern "C" int eemflow_tsimg_grad_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                       const double* scale, const double (*maps)[4], int h, int w, double eps, const float* const* iwe,
                                       const float* const* ts, const double* coef, float* const* grads, void* stream) {
    EEM_REQUIRE(k >= 1 && k <= IWE_MAX_JOBS, "eemflow_tsimg_grad_many: 1..%d jobs per call; got %d", IWE_MAX_JOBS, k);
    EEM_REQUIRE(events && n && flows && t0 && scale && maps && iwe && ts && coef && grads, "eemflow_tsimg_grad_many: NULL argument");
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 30), "eemflow_tsimg_grad_many: bad size %dx%d", h, w);
    EEM_REQUIRE(eps > 0.0 && eps < 1e300, "eemflow_tsimg_grad_many: eps=%g is not a positive finite number", eps);
    int form = 0;
    const int rc = iwe_grad_run<TsFactor>("eemflow_tsimg_grad_many", k, events, n, flows, t0, scale, maps, h, w, ts, iwe, nullptr, eps, coef,
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
