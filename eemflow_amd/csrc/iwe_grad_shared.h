// The gradient kernels that iwe_grad.hip (variance of the image of warped events) and tsimg.hip (image of average timestamps) share:
// binning, bands in LDS and the direct form, see iwe_grad.hip's header comment.  The two objectives differ in ONE number only, the factor
// G = dL / d(vote weight) at a target cell; it comes from a Factor:
//   static Factor load(const IweGradJob& J, const double* aux, double eps)     per thread, once: what G needs of the job
//   double at(const IweGradJob& J, long o, long hw, int c, double ah) const    G at cell o of channel c for an event of timestamp value ah
// Both files are built with -ffp-contract=off.
#pragma once

#include <string.h>

#include "iwe_shared.h"

namespace {

constexpr int GRAD_RPE = 4;                      // records per event: one per sample neighbour

struct IweGradJob {
    const double* ev;
    const float* flow;
    const float* img;        // the forward's stored image [2][h][w] (tsimg: the image of average timestamps T)
    const float* img2;       // tsimg: the forward's stored vote image D; else NULL
    float* out;              // [2][h][w]
    unsigned* recs;          // 12-byte records {cell-in-band, du, dv (fp32 bits)}, a slab of 4 * VT * EPT per binning block
    unsigned* run_start;     // [nblk][nb + 1]
    double t0, scale;
    IweMap map;
    long n;
    int nblk;                // binning blocks (slabs) of this job
    int src;                 // the job's index in the call: its row of moments and its coef
};
struct IweGradJobs { IweGradJob j[IWE_MAX_JOBS]; };      // 120 bytes each: 3.8 KB of kernel arguments at 32 jobs
static_assert(sizeof(IweGradJob) == 120, "IweGradJobs must stay below 4 KB of kernel arguments");

// the timestamp value of an event (tsimg.hip's forward votes with the same expression): a = max(1 - |tau|, 0) rounded to fp32 once
__device__ __forceinline__ float iwe_time_value(double tau) { return (float)fmax(1.0 - fabs(tau), 0.0); }

// what an event adds: du_k = wk[k] * cu, dv_k = wk[k] * cv at the in-frame neighbours k of taps
struct IweGradEvent {
    IweTaps taps;
    double cu, cv;
    bool live;
};

template <class Factor>
__device__ __forceinline__ IweGradEvent iwe_grad_event(const IweGradJob& J, long i, const Factor& f, double coef, int h, int w) {
    IweGradEvent g;
    g.cu = g.cv = 0.0;
    g.live = false;
    const IweEvent e = iwe_warp(J.ev, i, J.flow, J.t0, J.scale, J.map, h, w);
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
    const double ah = (double)iwe_time_value(e.tau);
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
            const double G = f.at(J, (long)Y * w + X, hw, e.c, ah);
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
template <int EPT, class Factor>
__global__ __launch_bounds__(VT) void iwe_grad_bin_kernel(IweGradJobs jobs, const double* __restrict__ aux, double eps,
                                                          const double* __restrict__ coefs, int h, int w, IwePlan pl) {
    const IweGradJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // a shorter event set of the launch
    const long n = J.n;
    const Factor f = Factor::load(J, aux, eps);
    const double coef = coefs[J.src];
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
            const IweGradEvent g = iwe_grad_event(J, i, f, coef, h, w);
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
template <class Factor>
__global__ __launch_bounds__(256) void iwe_grad_direct_kernel(IweGradJob J, const double* __restrict__ aux, double eps,
                                                              const double* __restrict__ coefs, int h, int w, double* __restrict__ acc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= J.n) return;
    const Factor f = Factor::load(J, aux, eps);
    const IweGradEvent g = iwe_grad_event(J, i, f, coefs[J.src], h, w);
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

inline GradLayout grad_layout(long n, int ept, const IwePlan& pl) {
    const size_t nblk = (size_t)iwe_blocks(n, ept);
    GradLayout l;
    l.recs = 0;
    l.table = up256(nblk * (size_t)(GRAD_RPE * VT * ept) * 12);
    l.total = l.table + up256((nblk * (size_t)(pl.nb + 1) + 1) * 4);
    return l;
}

template <int EPT, class Factor>
int launch_grad_bin(const IweGradJobs& jobs, int njobs, long nblk_max, const double* aux, double eps, const double* coef, int h, int w,
                    const IwePlan& pl, hipStream_t stream) {
    constexpr int stage_bytes = GRAD_RPE * VT * EPT * 12;
    EEM_RAISE_LDS(stage_bytes, iwe_grad_bin_kernel<EPT, Factor>);
    hipLaunchKernelGGL((iwe_grad_bin_kernel<EPT, Factor>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, aux, eps, coef,
                       h, w, pl);
    return EEM_OK;
}

// The body of a gradient entry point, after iwe_check_many: `img` (and `img2`, or NULL) are the forward's stored images of the k jobs, `aux` and `eps` what
// the Factor loads from.  *form: 0 when no job had a flow (nothing ran), -1 for the direct form, else the binning kernel's EPT.
template <class Factor>
int iwe_grad_run(const char* name, int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                 const double* scale, const double (*maps)[4], int h, int w, const float* const* img, const float* const* img2,
                 const double* aux, double eps, const double* coef, float* const* grads, void* stream_, int* form) {
    hipStream_t stream = (hipStream_t)stream_;
    IweGradJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int m = 0;                                                     // jobs with a flow: the others have no gradient
    long nmax = 0;
    for (int i = 0; i < k; ++i) {
        if (!flows[i]) continue;
        EEM_REQUIRE((events[i] || n[i] == 0) && img[i] && (!img2 || img2[i]) && grads[i], "%s: job %d has a NULL buffer", name, i);
        IweGradJob& J = jobs.j[m++];
        J.ev = events[i];
        J.flow = flows[i];
        J.img = img[i];
        J.img2 = img2 ? img2[i] : nullptr;
        J.out = grads[i];
        J.t0 = t0[i];
        J.scale = scale[i];
        J.map = IweMap{maps[i][0], maps[i][1], maps[i][2], maps[i][3]};
        J.n = (long)n[i];
        J.src = i;
        nmax = std::max(nmax, J.n);
    }
    *form = 0;
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
                hipLaunchKernelGGL(iwe_grad_direct_kernel<Factor>, dim3((unsigned)((J.n + 255) / 256)), dim3(256), 0, stream, J, aux, eps, coef, h,
                                   w, acc);
            hipLaunchKernelGGL(iwe_grad_finish_kernel, dim3(fin), dim3(256), 0, stream, acc, J.out, 2 * hw);
            EEM_HIP_CHECK(hipGetLastError());
        }
        *form = -1;
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
        rc = ept == 1 ? launch_grad_bin<1, Factor>(jobs, m, nblk_max, aux, eps, coef, h, w, pl, stream)
                      : launch_grad_bin<2, Factor>(jobs, m, nblk_max, aux, eps, coef, h, w, pl, stream);
        if (rc != EEM_OK) return rc;
    }
    const int slab = GRAD_RPE * VT * ept;
    int bt = 0;
    rc = iwe_launch_bands<iwe_grad_band_kernel<256>, iwe_grad_band_kernel<VT>>(pl, m, stream, &bt, jobs, slab, h, w, pl, iwe_run_lanes(pl, slab));
    if (rc != EEM_OK) return rc;
    EEM_HIP_CHECK(hipGetLastError());
    *form = ept;
    return arena.done(token, stream_);
}

}  // namespace
