// The forward that iwe.hip (image of warped events) and tsimg.hip (image of average timestamps) share: binning, bands in LDS, moments,
// the direct form and the host path around them - the algorithm is described in iwe.hip's header comment.  The warp, the votes, the
// X < 0 / X == w - 1 edge rule and the fixed-point weights exist here once, so tsimg's vote image is iwe's binned image bit for bit by
// construction.  The two objectives differ in what travels with a vote and in what a pixel's sums become; that comes from a Policy:
//   static constexpr int PLANES, WORDS         fp64 LDS cells per pixel of a band (2 or 4) and 32-bit words per record (3 or 4)
//   static constexpr bool FIXED_DIRECT         whether the direct form votes with the fixed-point weights (tsimg) or with the plain fp64
//                                              products where they are not zero (iwe); the difference is real: tests/test_gpu_tsimg.py
//   static unsigned payload(const IweEvent&)   the record's fourth word: nothing for iwe, the fp32 bits of iwe_time_value(e.tau) for tsimg
//   static void add<LDS>(double* cell, long nofs, double wgt, unsigned payload)
//                                              what one weight of a record adds at its cell of the first PLANES / 2 planes (the planes
//                                              behind them lie nofs cells further on); LDS: the band's cells, else the direct form's image
//   void leave(const double* px, I stride, I i, float* out0, float* out1, long hw, double& p0, double& p1) const
//                                              what pixel i leaves of its PLANES sums px[j * stride + i]: it stores its fp32 outputs at
//                                              [i] and [hw + i] of the job's images and adds to the two running partials
// The policy object travels to the kernels by value (tsimg's eps).  Both files are built with -ffp-contract=off.
#pragma once

#include <string.h>

#include "iwe_shared.h"

namespace {

// One job of a launch: blockIdx.y picks it (one frame size and plan, its own events, flow, slabs, run table, partials and images)
struct IweFwdJob {
    const double* ev;
    const float* flow;       // NULL: zero flow
    float* out0;             // [2][h][w]: the image of warped events (tsimg: the vote image D)
    float* out1;             // tsimg: [2][h][w] average timestamps; else NULL
    unsigned* recs;          // records of WORDS words {cell-in-band (channel included), left weight, right weight (fixed point, 2^31 = 1)[, payload]},
                             // a slab of 2 * VT * EPT per binning block; behind the nblk slabs the run table run_start[nblk][nb + 1]
    double* part;            // [parts][2]: the two partials of a band (binned) or of a finishing block (direct)
    double* dropped;         // [nblk]: events with a non-finite warped position, per binning block (direct: one slot)
    double t0, scale;
    IweMap map;              // xe = ax * x + bx, ye = ay * y + by
    long n;
    int nblk;                // binning blocks (slabs) of this job
    int pad;
};
struct IweFwdJobs { IweFwdJob j[IWE_MAX_JOBS]; };        // 120 bytes each: 3.8 KB of kernel arguments at 32 jobs
static_assert(sizeof(IweFwdJob) == 120, "IweFwdJobs must stay below 4 KB of kernel arguments");

// the run table of a job: behind its nblk slabs of `slab` records of `words` words (a slab is a multiple of 256 bytes)
__device__ __forceinline__ unsigned* iwe_run_table(const IweFwdJob& J, int slab, int words) { return J.recs + (size_t)J.nblk * slab * words; }

constexpr double IWE_UNIT = 1.0 / 2147483648.0;          // a fixed-point weight's unit, 2^-31

__device__ __forceinline__ unsigned iwe_fix(double wgt) { return (unsigned)(wgt * 2147483648.0 + 0.5); }       // wgt in [0, 1]

template <bool LDS>
__device__ __forceinline__ void iwe_add(double* p, double v) {
    if constexpr (LDS) atomicAdd(p, v);
    else unsafeAtomicAdd(p, v);
}

// ------------------------------------------------------------------------------------------------ 1. binning into slabs
// Block `blk` owns the slab recs[blk * S .. (blk + 1) * S) (S = 2 * 1024 * EPT records): its row records sorted by band, and row
// `blk` of the run table: run_start[blk][b] = offset of band b's run inside the slab, run_start[blk][nb] = the slab's fill.
template <int EPT, class P>
__global__ __launch_bounds__(VT) void iwe_fwd_bin_kernel(IweFwdJobs jobs, int h, int w, IwePlan pl) {
    constexpr int W = P::WORDS;
    const IweFwdJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // a shorter event set of the launch
    const double* __restrict__ ev = J.ev;
    const float* __restrict__ flow = J.flow;
    const long n = J.n;
    const double t0 = J.t0, scale = J.scale;
    __shared__ unsigned hist[VT];
    __shared__ unsigned lpos[VT];
    __shared__ unsigned sh[VT / 64];
    __shared__ unsigned ndrop;
    extern __shared__ __attribute__((aligned(16))) unsigned stage[];   // the slab as it goes to memory: W words per record
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
                qa[k] = P::payload(e);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int Y = q.Y0 + dy;
                    const double wy = dy ? q.gy : 1.0 - q.gy;
                    if (Y >= 0 && Y < h) {
                        double wl = wy * (1.0 - q.gx), wr = wy * q.gx;
                        int X = q.X0;
                        if (X < 0) { X = 0; wl = wr; wr = 0.0; }   // the left target is outside: the right one in the left slot
                        else if (X == w - 1) wr = 0.0;             // the right target is outside (it does not wrap into the next row)
                        const unsigned a = iwe_fix(wl), b = iwe_fix(wr);
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
    if (tid <= pl.nb) iwe_run_table(J, 2 * VT * EPT, W)[(size_t)blockIdx.x * (pl.nb + 1) + tid] = start;
    if (tid == 0) J.dropped[blockIdx.x] = (double)ndrop;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * EPT; ++k) {
        if (band[k] != NONE) {
            const unsigned at = lpos[band[k]] + rank[k];
            if constexpr (W == 4) {                                // a record is one whole 16-byte piece
                u32x4 r;
                r.x = key[k];
                r.y = ql[k];
                r.z = qr[k];
                r.w = qa[k >> 1];
                reinterpret_cast<u32x4*>(stage)[at] = r;
            } else {
                unsigned* r = stage + 3u * at;
                r[0] = key[k];
                r[1] = ql[k];
                r[2] = qr[k];
            }
        }
    }
    __syncthreads();
    // the sorted slab leaves as whole 16-byte pieces of consecutive threads (a slab is a multiple of 16 bytes: the last piece stays inside it)
    const unsigned pieces = ((unsigned)W * lpos[pl.nb] + 3u) / 4u;
    u32x4* slab = reinterpret_cast<u32x4*>(J.recs + (size_t)blockIdx.x * (2 * VT * EPT) * W);
    const u32x4* st4 = reinterpret_cast<const u32x4*>(stage);
    for (unsigned i = tid; i < pieces; i += VT) slab[i] = st4[i];
}

// ------------------------------------------------------------------------------------------------ 2. bands in LDS
template <int BT, class P>
__global__ __launch_bounds__(BT) void iwe_fwd_band_kernel(IweFwdJobs jobs, int slab, int h, int w, IwePlan pl, int sgs, P pol) {
    constexpr int W = P::WORDS;
    const IweFwdJob& J = jobs.j[blockIdx.y];
    const unsigned* __restrict__ recs = J.recs;
    const unsigned* __restrict__ run_start = iwe_run_table(J, slab, W);
    const int nblk = J.nblk;
    extern __shared__ __attribute__((aligned(16))) double cells[];     // [PLANES][rows][w]
    __shared__ double sh2[2 * BT / 64];
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
        const unsigned* base = recs + (size_t)s * slab * W;
        for (unsigned k = st + (unsigned)sub; k < en; k += 1u << sgs) {
            unsigned cell, a, c, pay = 0;                          // cell < 2 * plane (channel included)
            if constexpr (W == 4) {
                const u32x4 r = reinterpret_cast<const u32x4*>(base)[k];
                cell = r.x; a = r.y; c = r.z; pay = r.w;
            } else {
                const unsigned* r = base + 3u * k;
                cell = r[0]; a = r[1]; c = r[2];
            }
            P::template add<true>(cells + cell, 2 * plane, (double)a * IWE_UNIT, pay);
            if (c) P::template add<true>(cells + cell + 1, 2 * plane, (double)c * IWE_UNIT, pay);      // (c == 0 at the row's last column: no touch of the next row)
        }
    }
    __syncthreads();
    // one pass: every pixel of the band leaves its rounded outputs and its share of the band's two partials
    const int y0 = b * pl.rows;
    const int npx = min(pl.rows, h - y0) * w;
    const long hw = (long)h * w;
    float* __restrict__ out0 = J.out0 + (long)y0 * w;
    float* __restrict__ out1 = J.out1 + (long)y0 * w;
    double p0 = 0.0, p1 = 0.0;
    for (int i = tid; i < npx; i += BT) pol.leave(cells, plane, i, out0, out1, hw, p0, p1);
    block_sum2<BT>(p0, p1, sh2);
    if (tid == 0) { J.part[2 * b] = p0; J.part[2 * b + 1] = p1; }
}

// ------------------------------------------------------------------------------------------------ 3. moments
// one block per job: {h*w, the two partials' sums, dropped}, added in a fixed order
__global__ __launch_bounds__(256) void iwe_fwd_moments_kernel(IweFwdJobs jobs, int nparts, double hw, double* __restrict__ moments) {
    const IweFwdJob& J = jobs.j[blockIdx.x];
    __shared__ double sh2[2 * 256 / 64];
    const int tid = threadIdx.x;
    double p0 = 0.0, p1 = 0.0, dr = 0.0, zero = 0.0;
    for (int k = tid; k < nparts; k += 256) { p0 += J.part[2 * k]; p1 += J.part[2 * k + 1]; }
    for (int k = tid; k < J.nblk; k += 256) dr += J.dropped[k];
    block_sum2<256>(p0, p1, sh2);
    block_sum2<256>(dr, zero, sh2);
    if (tid == 0) {
        double* m = moments + 4 * blockIdx.x;
        m[0] = hw; m[1] = p0; m[2] = p1; m[3] = dr;
    }
}

// ------------------------------------------------------------------------------------------------ direct form
// acc: [PLANES][h][w] fp64, zeroed
template <class P>
__global__ __launch_bounds__(256) void iwe_fwd_direct_kernel(const double* __restrict__ ev, long n, const float* __restrict__ flow, double t0,
                                                             double scale, IweMap map, int h, int w, double* __restrict__ acc,
                                                             unsigned long long* __restrict__ ndrop) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const IweEvent e = iwe_warp(ev, i, flow, t0, scale, map, h, w);
    const IweVotes q = iwe_votes(e, h, w);
    if (!q.finite) atomicAdd(ndrop, 1ull);
    if (!q.inside) return;
    const long hw = (long)h * w;
    const unsigned pay = P::payload(e);
    double* plane = acc + (long)e.c * hw;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int Y = q.Y0 + dy;
        const double wy = dy ? q.gy : 1.0 - q.gy;
        if (Y < 0 || Y >= h) continue;
        double wl = wy * (1.0 - q.gx), wr = wy * q.gx;
        if constexpr (P::FIXED_DIRECT) {
            wl = (double)iwe_fix(wl) * IWE_UNIT;
            wr = (double)iwe_fix(wr) * IWE_UNIT;
        }
        const long o = (long)Y * w + q.X0;
        if (q.X0 >= 0 && wl != 0.0) P::template add<false>(plane + o, 2 * hw, wl, pay);
        if (q.X0 + 1 <= w - 1 && wr != 0.0) P::template add<false>(plane + o + 1, 2 * hw, wr, pay);
    }
}

// every pixel leaves its rounded outputs; this block's two partials; block 0 also hands on the drop count
template <class P>
__global__ __launch_bounds__(256) void iwe_fwd_direct_finish_kernel(const double* __restrict__ acc, const unsigned long long* __restrict__ ndrop,
                                                                    float* __restrict__ out0, float* __restrict__ out1, long hw, P pol,
                                                                    double* __restrict__ part, double* __restrict__ dropped) {
    __shared__ double sh2[2 * 256 / 64];
    double p0 = 0.0, p1 = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) pol.leave(acc, hw, i, out0, out1, hw, p0, p1);
    block_sum2<256>(p0, p1, sh2);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = p0;
        part[2 * blockIdx.x + 1] = p1;
        if (blockIdx.x == 0) dropped[0] = (double)*ndrop;
    }
}

// ------------------------------------------------------------------------------------------------ host
inline int iwe_ept(long n) {
    const int forced = sw_int<SW_EEM_IWE_EPT>();                   // events per binning thread, 1 / 2 / 4 (the tests run all three)
    if ((forced == 1 || forced == 2 || forced == 4) && iwe_blocks(n, forced) <= IWE_MAX_BLOCKS) return forced;
    int ept = 1;
    while (ept < 4 && iwe_blocks(n, ept) > 512) ept *= 2;
    return ept;
}
constexpr int IWE_DIRECT_PARTS = 256;

struct IweFwdLayout { size_t table, part, dropped, total; };      // the records lie at 0

inline IweFwdLayout iwe_fwd_layout(long n, int ept, const IwePlan& pl, int words) {
    const size_t nblk = (size_t)iwe_blocks(n, ept);
    IweFwdLayout l;
    l.table = nblk * (size_t)(2 * VT * ept) * words * 4;           // (a multiple of 256: iwe_run_table finds the table there)
    l.part = l.table + up256((nblk * (size_t)(pl.nb + 1) + 1) * 4);
    l.dropped = l.part + up256((size_t)pl.nb * 16);
    l.total = l.dropped + up256((nblk + 1) * 8);
    return l;
}

template <int EPT, class P>
int iwe_fwd_launch_bin(const IweFwdJobs& jobs, int njobs, long nblk_max, int h, int w, const IwePlan& pl, hipStream_t stream) {
    constexpr int stage_bytes = 2 * VT * EPT * P::WORDS * 4;
    if (stage_bytes > 32 * 1024) EEM_RAISE_LDS(stage_bytes, iwe_fwd_bin_kernel<EPT, P>);
    hipLaunchKernelGGL((iwe_fwd_bin_kernel<EPT, P>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, h, w, pl);
    return EEM_OK;
}

// what a forward ran: ept == 0 is the direct form, else bin_e<ept> + band<bt>_s<sgs> + moments
struct IweFwdForm { int ept, bt, sgs; };

// The body of a forward entry point, arguments checked: out0 (and out1, or NULL) are the k jobs' output images.  Takes a scratch arena
// for the call's launches and hands back the form it ran.
template <class P>
int iwe_fwd_launch(const P& pol, int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                   const double* scale, const double (*maps)[4], int h, int w, float* const* out0, float* const* out1, double* moments,
                   void* stream_, IweFwdForm* form) {
    hipStream_t stream = (hipStream_t)stream_;
    long nmax = 0;
    for (int i = 0; i < k; ++i) nmax = std::max(nmax, (long)n[i]);
    const long hw = (long)h * w;
    IwePlan pl;
    const bool binned = iwe_plan(nmax, h, w, &pl, 4, P::PLANES);
    const int ept = iwe_ept(nmax);
    const size_t acc_bytes = (size_t)P::PLANES * hw * 8 + 8;       // the direct form's fp64 planes and its drop counter
    size_t need = 0;
    if (binned)
        for (int i = 0; i < k; ++i) need += iwe_fwd_layout((long)n[i], ept, pl, P::WORDS).total;
    else
        need = up256(acc_bytes) + up256((size_t)IWE_DIRECT_PARTS * 16) + 256;
    Arena& arena = iwe_arena();
    std::lock_guard<std::mutex> guard(arena.lock);
    char* scratch = nullptr;
    void* token = nullptr;
    int rc = arena.take(need, stream_, &scratch, &token);
    if (rc != EEM_OK) return rc;
    IweFwdJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    if (!binned) {
        // direct form, one job after the other through one set of fp64 planes
        double* acc = reinterpret_cast<double*>(scratch);
        unsigned long long* ndrop = reinterpret_cast<unsigned long long*>(acc + P::PLANES * hw);
        double* part = reinterpret_cast<double*>(scratch + up256(acc_bytes));
        double* dropped = part + 2 * IWE_DIRECT_PARTS;
        const int parts = (int)std::min<long>(IWE_DIRECT_PARTS, (hw + 255) / 256);
        jobs.j[0].part = part;
        jobs.j[0].dropped = dropped;
        jobs.j[0].nblk = 1;
        for (int i = 0; i < k; ++i) {
            EEM_HIP_CHECK(hipMemsetAsync(acc, 0, acc_bytes, stream));
            if (n[i] > 0)
                hipLaunchKernelGGL(iwe_fwd_direct_kernel<P>, dim3((unsigned)((n[i] + 255) / 256)), dim3(256), 0, stream, events[i], (long)n[i],
                                   flows ? flows[i] : nullptr, t0[i], scale[i], IweMap{maps[i][0], maps[i][1], maps[i][2], maps[i][3]}, h, w,
                                   acc, ndrop);
            hipLaunchKernelGGL(iwe_fwd_direct_finish_kernel<P>, dim3(parts), dim3(256), 0, stream, acc, ndrop, out0[i], out1 ? out1[i] : nullptr,
                               hw, pol, part, dropped);
            hipLaunchKernelGGL(iwe_fwd_moments_kernel, dim3(1), dim3(256), 0, stream, jobs, parts, (double)hw, moments + 4 * i);
            EEM_HIP_CHECK(hipGetLastError());
        }
        *form = IweFwdForm{0, 0, 0};
        return arena.done(token, stream_);
    }
    long nblk_max = 0;
    char* q = scratch;
    for (int i = 0; i < k; ++i) {
        const IweFwdLayout l = iwe_fwd_layout((long)n[i], ept, pl, P::WORDS);
        IweFwdJob& J = jobs.j[i];
        J.ev = events[i];
        J.flow = flows ? flows[i] : nullptr;
        J.out0 = out0[i];
        J.out1 = out1 ? out1[i] : nullptr;
        J.recs = reinterpret_cast<unsigned*>(q);
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
            case 1: rc = iwe_fwd_launch_bin<1, P>(jobs, k, nblk_max, h, w, pl, stream); break;
            case 2: rc = iwe_fwd_launch_bin<2, P>(jobs, k, nblk_max, h, w, pl, stream); break;
            default: rc = iwe_fwd_launch_bin<4, P>(jobs, k, nblk_max, h, w, pl, stream); break;
        }
        if (rc != EEM_OK) return rc;
    }
    const int slab = 2 * VT * ept;
    const int sgs = iwe_run_lanes(pl, slab);
    int bt = 0;
    rc = iwe_launch_bands<iwe_fwd_band_kernel<256, P>, iwe_fwd_band_kernel<VT, P>>(pl, k, stream, &bt, jobs, slab, h, w, pl, sgs, pol);
    if (rc != EEM_OK) return rc;
    hipLaunchKernelGGL(iwe_fwd_moments_kernel, dim3(k), dim3(256), 0, stream, jobs, pl.nb, (double)hw, moments);
    EEM_HIP_CHECK(hipGetLastError());
    *form = IweFwdForm{ept, bt, sgs};
    return arena.done(token, stream_);
}

}  // namespace
