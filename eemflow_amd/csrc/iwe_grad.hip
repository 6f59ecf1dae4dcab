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
#include <string.h>

#include "iwe_shared.h"

namespace {

constexpr int GRAD_RPE = 4;                      // records per event: one per sample neighbour

struct IweGradJob {
    const double* ev;
    const float* flow;
    const float* img;        // the forward's stored image [2][h][w]
    float* out;              // [2][h][w]
    unsigned* recs;          // 12-byte records {cell-in-band, du, dv (fp32 bits)}, a slab of 4 * VT * EPT per binning block
    unsigned* run_start;     // [nblk][nb + 1]
    double t0, scale;
    IweMap map;
    long n;
    int nblk;                // binning blocks (slabs) of this job
    int src;                 // the job's index in the call: its row of moments and its coef
};
struct IweGradJobs { IweGradJob j[IWE_MAX_JOBS]; };      // 112 bytes each: 3.5 KB of kernel arguments at 32 jobs

// what an event adds: du_k = wk[k] * cu, dv_k = wk[k] * cv at the in-frame neighbours k of taps
struct IweGradEvent {
    IweTaps taps;
    double cu, cv;
    bool live;
};

__device__ __forceinline__ IweGradEvent iwe_grad_event(const double* __restrict__ ev, long i, const float* __restrict__ flow,
                                                       const float* __restrict__ img, double mean, double npx, double coef, double t0,
                                                       double scale, const IweMap& map, int h, int w) {
    IweGradEvent g;
    g.cu = g.cv = 0.0;
    g.live = false;
    const IweEvent e = iwe_warp(ev, i, flow, t0, scale, map, h, w);
    g.taps = e.taps;
    // iwe_votes' cells, and one case more: at xw = -1 exactly the forward's vote into column 0 has weight gx = 0 (iwe_votes leaves the
    // event out), but its derivative, +1, counts - the pair (X0, X0 + 1) = (-1, 0) with gx = 0, as at every integer position
    IweVotes q;
    q.finite = isfinite(e.xw) && isfinite(e.yw);
    q.inside = q.finite && e.xw >= -1.0 && e.xw < (double)w && e.yw >= -1.0 && e.yw < (double)h;
    if (!q.inside || !g.taps.any) return g;      // dropped whole / no target in the frame / no flow pixel under the event
    {
        const double xf = floor(e.xw), yf = floor(e.yw);
        q.X0 = (int)xf;
        q.Y0 = (int)yf;
        q.gx = e.xw - xf;
        q.gy = e.yw - yf;
    }
    const long hw = (long)h * w;
    double dX = 0.0, dY = 0.0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int Y = q.Y0 + dy;
        if (Y < 0 || Y >= h) continue;
        const double wy = dy ? q.gy : 1.0 - q.gy;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int X = q.X0 + dx;
            if (X < 0 || X >= w) continue;
            const double wx = dx ? q.gx : 1.0 - q.gx;
            const long o = (long)Y * w + X;
            const double S = (double)img[o] + (double)img[hw + o];
            const double G = 2.0 * (S - mean) / npx;
            dX += dx ? G * wy : -(G * wy);
            dY += dy ? G * wx : -(G * wx);
        }
    }
    g.cu = coef * e.tau * dX;
    g.cv = coef * e.tau * dY;
    g.live = true;
    return g;
}

// ------------------------------------------------------------------------------------------------ 1. binning into slabs
template <int EPT>
__global__ __launch_bounds__(VT) void iwe_grad_bin_kernel(IweGradJobs jobs, const double* __restrict__ moments, const double* __restrict__ coefs,
                                                          int h, int w, IwePlan pl) {
    const IweGradJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // a shorter event set of the launch
    const long n = J.n;
    const double npx = moments[4 * J.src], mean = moments[4 * J.src + 1] / npx, coef = coefs[J.src];
    __shared__ unsigned hist[VT];
    __shared__ unsigned lpos[VT];
    __shared__ unsigned sh[VT / 64];
    extern __shared__ __attribute__((aligned(16))) unsigned stage[];   // the slab as it goes to memory: 3 words per record
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    constexpr int R = GRAD_RPE * EPT;
    unsigned key[R], band[R], rank[R], qu[R], qv[R];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long i = ((long)blockIdx.x * EPT + k) * VT + tid;
#pragma unroll
        for (int t = 0; t < GRAD_RPE; ++t) band[GRAD_RPE * k + t] = NONE;
        if (i < n) {
            const IweGradEvent g = iwe_grad_event(J.ev, i, J.flow, J.img, mean, npx, coef, J.t0, J.scale, J.map, h, w);
            if (g.live) {
#pragma unroll
                for (int t = 0; t < GRAD_RPE; ++t) {
                    if (!g.taps.in[t]) continue;
                    const float du = (float)(g.taps.wk[t] * g.cu), dv = (float)(g.taps.wk[t] * g.cv);
                    if (du == 0.0f && dv == 0.0f) continue;
                    const int Y = g.taps.y0 + (t >> 1), X = g.taps.x0 + (t & 1);       // inside the frame (taps.in)
                    const unsigned bd = (unsigned)Y / (unsigned)pl.rows;
                    const int r = GRAD_RPE * k + t;
                    band[r] = bd;
                    key[r] = (unsigned)(Y - (int)bd * pl.rows) * (unsigned)w + (unsigned)X;
                    qu[r] = __float_as_uint(du);
                    qv[r] = __float_as_uint(dv);
                    rank[r] = atomicAdd(&hist[bd], 1u);            // LDS: the returned count is the rank inside the run
                }
            }
        }
    }
    __syncthreads();
    const unsigned start = block_exscan(hist[tid], sh);            // bands >= nb hold 0: thread nb gets the slab's fill
    lpos[tid] = start;
    if (tid <= pl.nb) J.run_start[(size_t)blockIdx.x * (pl.nb + 1) + tid] = start;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (band[r] != NONE) {
            unsigned* d = stage + 3u * (lpos[band[r]] + rank[r]);
            d[0] = key[r];
            d[1] = qu[r];
            d[2] = qv[r];
        }
    }
    __syncthreads();
    // the sorted slab leaves as whole 16-byte pieces of consecutive threads (a slab is a multiple of 16 bytes: the last piece stays inside it)
    const unsigned words = 3u * lpos[pl.nb];
    u32x4* slab = reinterpret_cast<u32x4*>(J.recs + (size_t)blockIdx.x * (GRAD_RPE * VT * EPT) * 3);
    const u32x4* st4 = reinterpret_cast<const u32x4*>(stage);
    for (unsigned i = tid; i * 4 < words; i += VT) slab[i] = st4[i];
}

// ------------------------------------------------------------------------------------------------ 2. bands in LDS
template <int BT>
__global__ __launch_bounds__(BT) void iwe_grad_band_kernel(IweGradJobs jobs, int slab, int h, int w, IwePlan pl, int sgs) {
    const IweGradJob& J = jobs.j[blockIdx.y];
    const unsigned* __restrict__ recs = J.recs;
    const unsigned* __restrict__ run_start = J.run_start;
    const int nblk = J.nblk;
    extern __shared__ __attribute__((aligned(16))) double cells[];     // [2][rows][w]
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    for (int i = tid; i < pl.cells; i += BT) cells[i] = 0.0;
    __syncthreads();
    const int plane = pl.rows * w;
    // a run = this band's records of one binning block; 2^sgs adjacent lanes share a run, so a wave's loads touch a few runs' lines
    const int sub = tid & ((1 << sgs) - 1);
    const int rpp = BT >> sgs;                                     // runs per pass of the block
    for (int s = tid >> sgs; s < nblk; s += rpp) {
        const unsigned* row = run_start + (size_t)s * (pl.nb + 1) + b;
        const unsigned st = row[0], en = row[1];
        const unsigned* base = recs + (size_t)s * slab * 3;
        for (unsigned k = st + (unsigned)sub; k < en; k += 1u << sgs) {
            const unsigned* r = base + 3u * k;
            const unsigned cell = r[0];
            const float du = __uint_as_float(r[1]), dv = __uint_as_float(r[2]);
            if (du != 0.0f) atomicAdd(cells + cell, (double)du);
            if (dv != 0.0f) atomicAdd(cells + plane + cell, (double)dv);
        }
    }
    __syncthreads();
    // one pass: both channels of every pixel of the band rounded to fp32 once and stored
    const int y0 = b * pl.rows;
    const int npx = min(pl.rows, h - y0) * w;
    const long hw = (long)h * w;
    float* __restrict__ out = J.out + (long)y0 * w;
    for (int i = tid; i < npx; i += BT) {
        out[i] = (float)cells[i];
        out[hw + i] = (float)cells[plane + i];
    }
}

// ------------------------------------------------------------------------------------------------ direct form
__global__ __launch_bounds__(256) void iwe_grad_direct_kernel(IweGradJob J, const double* __restrict__ moments, const double* __restrict__ coefs,
                                                              int h, int w, double* __restrict__ acc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= J.n) return;
    const double npx = moments[4 * J.src], mean = moments[4 * J.src + 1] / npx, coef = coefs[J.src];
    const IweGradEvent g = iwe_grad_event(J.ev, i, J.flow, J.img, mean, npx, coef, J.t0, J.scale, J.map, h, w);
    if (!g.live) return;
    const long hw = (long)h * w;
#pragma unroll
    for (int t = 0; t < GRAD_RPE; ++t) {
        if (!g.taps.in[t]) continue;
        const double du = g.taps.wk[t] * g.cu, dv = g.taps.wk[t] * g.cv;
        const long o = (long)(g.taps.y0 + (t >> 1)) * w + (g.taps.x0 + (t & 1));       // inside the frame (taps.in)
        if (du != 0.0) unsafeAtomicAdd(acc + o, du);
        if (dv != 0.0) unsafeAtomicAdd(acc + hw + o, dv);
    }
}

__global__ __launch_bounds__(256) void iwe_grad_finish_kernel(const double* __restrict__ acc, float* __restrict__ out, long cells) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long)gridDim.x * 256) out[i] = (float)acc[i];
}

// ------------------------------------------------------------------------------------------------ host
constexpr int GRAD_EPT_MAX = 2;                  // 4 x 1024 x 2 records of 12 bytes: 96 KB of LDS stage

inline int grad_ept(long nmax) { return iwe_blocks(nmax, 1) > IWE_MAX_BLOCKS ? 2 : 1; }

struct GradLayout { size_t recs, table, total; };

GradLayout grad_layout(long n, int ept, const IwePlan& pl) {
    const size_t nblk = (size_t)iwe_blocks(n, ept);
    GradLayout l;
    l.recs = 0;
    l.table = up256(nblk * (size_t)(GRAD_RPE * VT * ept) * 12);
    l.total = l.table + up256((nblk * (size_t)(pl.nb + 1) + 1) * 4);
    return l;
}

template <int EPT>
int launch_grad_bin(const IweGradJobs& jobs, int njobs, long nblk_max, const double* moments, const double* coef, int h, int w,
                    const IwePlan& pl, hipStream_t stream) {
    constexpr int stage_bytes = GRAD_RPE * VT * EPT * 12;
    EEM_RAISE_LDS(stage_bytes, iwe_grad_bin_kernel<EPT>);
    hipLaunchKernelGGL((iwe_grad_bin_kernel<EPT>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, moments, coef, h, w, pl);
    return EEM_OK;
}

}  // namespace

extern "C" int eemflow_iwe_grad_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                     const double* scale, const double (*maps)[4], int h, int w, const float* const* iwe,
                                     const double* moments, const double* coef, float* const* grads, void* stream_) {
    EEM_REQUIRE(k >= 1 && k <= IWE_MAX_JOBS, "eemflow_iwe_grad_many: 1..%d jobs per call; got %d", IWE_MAX_JOBS, k);
    EEM_REQUIRE(events && n && flows && t0 && scale && maps && iwe && moments && coef && grads, "eemflow_iwe_grad_many: NULL argument");
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 30), "eemflow_iwe_grad_many: bad size %dx%d", h, w);
    hipStream_t stream = (hipStream_t)stream_;
    IweGradJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int m = 0;                                                     // jobs with a flow: the others have no gradient
    long nmax = 0;
    for (int i = 0; i < k; ++i) {
        EEM_REQUIRE(n[i] >= 0 && n[i] < (1LL << 40), "eemflow_iwe_grad_many: job %d has n=%ld events", i, (long)n[i]);
        if (!flows[i]) continue;
        EEM_REQUIRE((events[i] || n[i] == 0) && iwe[i] && grads[i], "eemflow_iwe_grad_many: job %d has a NULL buffer", i);
        IweGradJob& J = jobs.j[m++];
        J.ev = events[i];
        J.flow = flows[i];
        J.img = iwe[i];
        J.out = grads[i];
        J.t0 = t0[i];
        J.scale = scale[i];
        J.map = IweMap{maps[i][0], maps[i][1], maps[i][2], maps[i][3]};
        J.n = (long)n[i];
        J.src = i;
        nmax = std::max(nmax, J.n);
    }
    if (m == 0) return EEM_OK;
    const long hw = (long)h * w;
    IwePlan pl;
    const bool binned = iwe_plan(nmax, h, w, &pl, GRAD_EPT_MAX);
    const int ept = grad_ept(nmax);
    size_t need = 0;
    if (binned)
        for (int i = 0; i < m; ++i) need += grad_layout(jobs.j[i].n, ept, pl).total;
    else
        need = up256((size_t)2 * hw * 8);
    Arena& arena = iwe_arena();
    std::lock_guard<std::mutex> guard(arena.lock);
    char* scratch = nullptr;
    void* token = nullptr;
    int rc = arena.take(need, stream_, &scratch, &token);
    if (rc != EEM_OK) return rc;
    if (!binned) {
        // direct form, one job after the other through one fp64 image
        double* acc = reinterpret_cast<double*>(scratch);
        const unsigned fin = (unsigned)std::min<long>(1024, (2 * hw + 255) / 256);
        for (int i = 0; i < m; ++i) {
            const IweGradJob& J = jobs.j[i];
            EEM_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)2 * hw * 8, stream));
            if (J.n > 0)
                hipLaunchKernelGGL(iwe_grad_direct_kernel, dim3((unsigned)((J.n + 255) / 256)), dim3(256), 0, stream, J, moments, coef, h, w, acc);
            hipLaunchKernelGGL(iwe_grad_finish_kernel, dim3(fin), dim3(256), 0, stream, acc, J.out, 2 * hw);
            EEM_HIP_CHECK(hipGetLastError());
        }
        return arena.done(token, stream_);
    }
    long nblk_max = 0;
    char* q = scratch;
    for (int i = 0; i < m; ++i) {
        IweGradJob& J = jobs.j[i];
        const GradLayout l = grad_layout(J.n, ept, pl);
        J.recs = reinterpret_cast<unsigned*>(q + l.recs);
        J.run_start = reinterpret_cast<unsigned*>(q + l.table);
        J.nblk = (int)iwe_blocks(J.n, ept);
        nblk_max = std::max(nblk_max, (long)J.nblk);
        q += l.total;
    }
    if (nblk_max > 0) {
        rc = ept == 1 ? launch_grad_bin<1>(jobs, m, nblk_max, moments, coef, h, w, pl, stream)
                      : launch_grad_bin<2>(jobs, m, nblk_max, moments, coef, h, w, pl, stream);
        if (rc != EEM_OK) return rc;
    }
    const int lds = pl.cells * 8;
    const int slab = GRAD_RPE * VT * ept;
    // lanes per run: the smallest power of two >= 1.7 x the mean run length (a slab's records / bands), 4 .. 64
    int sgs = 2;
    while (sgs < 6 && (1 << sgs) * 10L * pl.nb < 17L * slab) ++sgs;
    if (pl.cells <= 3072) {
        hipLaunchKernelGGL(iwe_grad_band_kernel<256>, dim3(pl.nb, m), dim3(256), lds, stream, jobs, slab, h, w, pl, sgs);
    } else {
        if (lds > 32 * 1024) EEM_RAISE_LDS(lds, iwe_grad_band_kernel<VT>);
        hipLaunchKernelGGL(iwe_grad_band_kernel<VT>, dim3(pl.nb, m), dim3(VT), lds, stream, jobs, slab, h, w, pl, sgs);
    }
    EEM_HIP_CHECK(hipGetLastError());
    return arena.done(token, stream_);
}
