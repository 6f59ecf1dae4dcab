// Image of warped events (IWE) and its moments, the ground-truth-free quality measure of an event-camera flow (reference: the warp is
// warp_events_flow_torch, utils_luo/event_utils.py:9-51; the loop around it Test.inference_img_warp_loss, test_mvsec.py:753-852, whose
// variance-ratio form of the flow warp loss sits at :821-824).
//
// Per job: events [n][4] f64 (t, x, y, p), time-sorted; a flow [2][h][w] fp32 or NULL (zero flow); scalars t0, scale and an affine event
// map (ax, bx, ay, by) - an offset (ox, oy) is (1, -ox, 1, -oy), the same bits.  All arithmetic is fp64 and unfused (this file is built
// with -ffp-contract=off; the per-event functions live in iwe_shared.h, which the gradient, iwe_grad.hip, includes too):
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
//   1. iwe_bin_kernel     every block of 1024 threads warps its 1024 x EPT events (EPT = 1, 2, 4 by event count, or EEM_IWE_EPT; the
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
//   2. iwe_band_kernel    one block per band: the band as fp64 LDS cells (ds_add_f64: the LDS fp32 add is 8 - 20 x slower on this
//                         chip, profiles/r04_lds_atomics.txt), 2^sgs adjacent lanes share a run (the band's records of one binning
//                         block); one pass then rounds every cell to fp32 once, stores both channels and leaves the band's
//                         (sum S, sum S^2).  9216 cells (72 KB) at most: 3 rows at w = 1280, 240 bands at 720 rows.
//   3. iwe_moments_kernel one block per job adds the band partials and the binning blocks' drop counts in a fixed order.
// Direct form (frames too wide for a one-row band, more than 16.7 M events, or EEM_IWE_DIRECT=1): one thread per
// event adds its votes with global atomics.  The image's contract is an fp64 sum rounded once - a chain of fp32 atomic adds is off by
// up to one rounding per vote, several ulps of the cell, where one ulp is allowed - so the direct form adds fp64 atomics into a zeroed
// fp64 image in the scratch arena, and a finishing pass rounds, stores and takes the moments (memset + two launches + the moments
// launch, one job after the other).
#include <string.h>

#include "iwe_shared.h"

namespace {

// One job of a launch: blockIdx.y picks it (one frame size and plan, its own events, flow, slabs, run table, partials and image)
struct IweJob {
    const double* ev;
    const float* flow;       // NULL: zero flow
    float* out;              // [2][h][w]
    unsigned* recs;          // 12-byte records {cell-in-band, left weight, right weight (fixed point, 2^31 = 1)}, a slab of 2 * VT * EPT per binning block
    unsigned* run_start;     // [nblk][nb + 1]
    double* part;            // [parts][2]: (sum S, sum S^2) of a band (binned) or of a finishing block (direct)
    double* dropped;         // [nblk]: events with a non-finite warped position, per binning block (direct: one slot)
    double t0, scale;
    IweMap map;              // xe = ax * x + bx, ye = ay * y + by
    long n;
    int nblk;                // binning blocks (slabs) of this job
    int pad;
};
struct IweJobs { IweJob j[IWE_MAX_JOBS]; };      // 120 bytes each: 3.8 KB of kernel arguments at 32 jobs

__device__ __forceinline__ unsigned iwe_fix(double wgt) { return (unsigned)(wgt * 2147483648.0 + 0.5); }       // wgt in [0, 1]

// ------------------------------------------------------------------------------------------------ 1. binning into slabs
// Block `blk` owns the slab recs[blk * S .. (blk + 1) * S) (S = 2 * 1024 * EPT records): its row records sorted by band, and row
// `blk` of the run table: run_start[blk][b] = offset of band b's run inside the slab, run_start[blk][nb] = the slab's fill.
template <int EPT>
__global__ __launch_bounds__(VT) void iwe_bin_kernel(IweJobs jobs, int h, int w, IwePlan pl) {
    const IweJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // a shorter event set of the launch
    const double* __restrict__ ev = J.ev;
    const float* __restrict__ flow = J.flow;
    const long n = J.n;
    const double t0 = J.t0, scale = J.scale;
    __shared__ unsigned hist[VT];
    __shared__ unsigned lpos[VT];
    __shared__ unsigned sh[VT / 64];
    __shared__ unsigned ndrop;
    extern __shared__ __attribute__((aligned(16))) unsigned stage[];   // the slab as it goes to memory: 3 words per record
    const int tid = threadIdx.x;
    hist[tid] = 0;
    if (tid == 0) ndrop = 0;
    __syncthreads();
    unsigned key[2 * EPT], band[2 * EPT], rank[2 * EPT], ql[2 * EPT], qr[2 * EPT];
    unsigned drop = 0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long i = ((long)blockIdx.x * EPT + k) * VT + tid;
        band[2 * k] = band[2 * k + 1] = NONE;
        if (i < n) {
            const IweEvent e = iwe_warp(ev, i, flow, t0, scale, J.map, h, w);
            const IweVotes q = iwe_votes(e, h, w);
            if (!q.finite) ++drop;
            if (q.inside) {
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
    if (tid <= pl.nb) J.run_start[(size_t)blockIdx.x * (pl.nb + 1) + tid] = start;
    if (tid == 0) J.dropped[blockIdx.x] = (double)ndrop;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * EPT; ++k) {
        if (band[k] != NONE) {
            unsigned* r = stage + 3u * (lpos[band[k]] + rank[k]);
            r[0] = key[k];
            r[1] = ql[k];
            r[2] = qr[k];
        }
    }
    __syncthreads();
    // the sorted slab leaves as whole 16-byte pieces of consecutive threads (a slab is a multiple of 16 bytes: the last piece stays inside it)
    const unsigned words = 3u * lpos[pl.nb];
    u32x4* slab = reinterpret_cast<u32x4*>(J.recs + (size_t)blockIdx.x * (2 * VT * EPT) * 3);
    const u32x4* st4 = reinterpret_cast<const u32x4*>(stage);
    for (unsigned i = tid; i * 4 < words; i += VT) slab[i] = st4[i];
}

// ------------------------------------------------------------------------------------------------ 2. bands in LDS
template <int BT>
__global__ __launch_bounds__(BT) void iwe_band_kernel(IweJobs jobs, int slab, int h, int w, IwePlan pl, int sgs) {
    const IweJob& J = jobs.j[blockIdx.y];
    const unsigned* __restrict__ recs = J.recs;
    const unsigned* __restrict__ run_start = J.run_start;
    const int nblk = J.nblk;
    extern __shared__ __attribute__((aligned(16))) double cells[];     // [2][rows][w]
    __shared__ double sh2[2 * BT / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    for (int i = tid; i < pl.cells; i += BT) cells[i] = 0.0;
    __syncthreads();
    // a run = this band's records of one binning block; 2^sgs adjacent lanes share a run, so a wave's loads touch a few runs' lines
    const int sub = tid & ((1 << sgs) - 1);
    const int rpp = BT >> sgs;                                     // runs per pass of the block
    for (int s = tid >> sgs; s < nblk; s += rpp) {
        const unsigned* row = run_start + (size_t)s * (pl.nb + 1) + b;
        const unsigned st = row[0], en = row[1];
        const unsigned* base = recs + (size_t)s * slab * 3;
        for (unsigned k = st + (unsigned)sub; k < en; k += 1u << sgs) {
            const unsigned* r = base + 3u * k;
            const unsigned cell = r[0], a = r[1], c = r[2];
            atomicAdd(cells + cell, (double)a * (1.0 / 2147483648.0));
            if (c) atomicAdd(cells + cell + 1, (double)c * (1.0 / 2147483648.0));  // (c == 0 at the row's last column: no touch of the next row)
        }
    }
    __syncthreads();
    // one pass: both channels of every pixel rounded to fp32 once, stored, S = their sum counted into the band's moments
    const int y0 = b * pl.rows;
    const int npx = min(pl.rows, h - y0) * w;
    const int plane = pl.rows * w;
    const long hw = (long)h * w;
    float* __restrict__ out = J.out + (long)y0 * w;
    double sm = 0.0, sq = 0.0;
    for (int i = tid; i < npx; i += BT) {
        const float v0 = (float)cells[i], v1 = (float)cells[plane + i];
        out[i] = v0;
        out[hw + i] = v1;
        const double S = (double)v0 + (double)v1;
        sm += S;
        sq += S * S;
    }
    block_sum2<BT>(sm, sq, sh2);
    if (tid == 0) { J.part[2 * b] = sm; J.part[2 * b + 1] = sq; }
}

// ------------------------------------------------------------------------------------------------ 3. moments
// one block per job: {h*w, sum S, sum S^2, dropped} from the partials, added in a fixed order
__global__ __launch_bounds__(256) void iwe_moments_kernel(IweJobs jobs, int nparts, double hw, double* __restrict__ moments) {
    const IweJob& J = jobs.j[blockIdx.x];
    __shared__ double sh2[2 * 256 / 64];
    const int tid = threadIdx.x;
    double sm = 0.0, sq = 0.0, dr = 0.0, zero = 0.0;
    for (int k = tid; k < nparts; k += 256) { sm += J.part[2 * k]; sq += J.part[2 * k + 1]; }
    for (int k = tid; k < J.nblk; k += 256) dr += J.dropped[k];
    block_sum2<256>(sm, sq, sh2);
    block_sum2<256>(dr, zero, sh2);
    if (tid == 0) {
        double* m = moments + 4 * blockIdx.x;
        m[0] = hw; m[1] = sm; m[2] = sq; m[3] = dr;
    }
}

// ------------------------------------------------------------------------------------------------ direct form
__global__ __launch_bounds__(256) void iwe_direct_kernel(const double* __restrict__ ev, long n, const float* __restrict__ flow, double t0,
                                                         double scale, IweMap map, int h, int w, double* __restrict__ acc,
                                                         unsigned long long* __restrict__ ndrop) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const IweEvent e = iwe_warp(ev, i, flow, t0, scale, map, h, w);
    const IweVotes q = iwe_votes(e, h, w);
    if (!q.finite) atomicAdd(ndrop, 1ull);
    if (!q.inside) return;
    double* plane = acc + (long)e.c * h * w;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int Y = q.Y0 + dy;
        const double wy = dy ? q.gy : 1.0 - q.gy;
        if (Y < 0 || Y >= h) continue;
        const double wl = wy * (1.0 - q.gx), wr = wy * q.gx;
        if (q.X0 >= 0 && wl != 0.0) unsafeAtomicAdd(plane + (long)Y * w + q.X0, wl);
        if (q.X0 + 1 <= w - 1 && wr != 0.0) unsafeAtomicAdd(plane + (long)Y * w + q.X0 + 1, wr);
    }
}

// rounds the fp64 image to fp32 once, stores it and leaves this block's (sum S, sum S^2); block 0 also hands on the drop count
__global__ __launch_bounds__(256) void iwe_direct_finish_kernel(const double* __restrict__ acc, const unsigned long long* __restrict__ ndrop,
                                                                float* __restrict__ out, long hw, double* __restrict__ part,
                                                                double* __restrict__ dropped) {
    __shared__ double sh2[2 * 256 / 64];
    double sm = 0.0, sq = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long)gridDim.x * 256) {
        const float v0 = (float)acc[i], v1 = (float)acc[hw + i];
        out[i] = v0;
        out[hw + i] = v1;
        const double S = (double)v0 + (double)v1;
        sm += S;
        sq += S * S;
    }
    block_sum2<256>(sm, sq, sh2);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sm;
        part[2 * blockIdx.x + 1] = sq;
        if (blockIdx.x == 0) dropped[0] = (double)*ndrop;
    }
}

// the warp alone: warped_xy [n][2] f64
__global__ __launch_bounds__(256) void iwe_warp_kernel(const double* __restrict__ ev, long n, const float* __restrict__ flow, double t0,
                                                       double scale, double ox, double oy, int h, int w, double* __restrict__ xy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const IweEvent e = iwe_warp(ev, i, flow, t0, scale, IweMap{1.0, -ox, 1.0, -oy}, h, w);
    xy[2 * i] = e.xw;
    xy[2 * i + 1] = e.yw;
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


struct IweLayout { size_t recs, table, part, dropped, total; };

IweLayout iwe_layout_binned(long n, int ept, const IwePlan& pl) {
    const size_t nblk = (size_t)iwe_blocks(n, ept);
    IweLayout l;
    l.recs = 0;
    l.table = up256(nblk * (size_t)(2 * VT * ept) * 12);
    l.part = l.table + up256(nblk * (size_t)(pl.nb + 1) * 4);
    l.dropped = l.part + up256((size_t)pl.nb * 16);
    l.total = l.dropped + up256((nblk + 1) * 8);
    return l;
}

template <int EPT>
int launch_bin(const IweJobs& jobs, int njobs, long nblk_max, int h, int w, const IwePlan& pl, hipStream_t stream) {
    constexpr int stage_bytes = 2 * VT * EPT * 12;
    if (stage_bytes > 32 * 1024) EEM_RAISE_LDS(stage_bytes, iwe_bin_kernel<EPT>);
    hipLaunchKernelGGL((iwe_bin_kernel<EPT>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, h, w, pl);
    return EEM_OK;
}

size_t iwe_scratch_bytes(int k, const int64_t* n, int h, int w) {
    long nmax = 0;
    for (int i = 0; i < k; ++i) nmax = std::max(nmax, (long)n[i]);
    IwePlan pl;
    if (!iwe_plan(nmax, h, w, &pl))
        return up256((size_t)2 * h * w * 8 + 8) + up256((size_t)IWE_DIRECT_PARTS * 16) + 256;
    const int ept = iwe_ept(nmax);
    size_t total = 0;
    for (int i = 0; i < k; ++i) total += iwe_layout_binned((long)n[i], ept, pl).total;
    return total;
}

int iwe_launch(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0, const double* scale,
               const double (*maps)[4], int h, int w, float* const* iwe, double* moments, char* scratch, hipStream_t stream) {
    long nmax = 0;
    for (int i = 0; i < k; ++i) nmax = std::max(nmax, (long)n[i]);
    const long hw = (long)h * w;
    IwePlan pl;
    IweJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    if (!iwe_plan(nmax, h, w, &pl)) {
        // direct form, one job after the other through one fp64 image
        double* acc = reinterpret_cast<double*>(scratch);
        unsigned long long* ndrop = reinterpret_cast<unsigned long long*>(acc + 2 * hw);
        double* part = reinterpret_cast<double*>(scratch + up256((size_t)2 * hw * 8 + 8));
        double* dropped = part + 2 * IWE_DIRECT_PARTS;
        const int parts = (int)std::min<long>(IWE_DIRECT_PARTS, (hw + 255) / 256);
        for (int i = 0; i < k; ++i) {
            EEM_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)2 * hw * 8 + 8, stream));
            if (n[i] > 0)
                hipLaunchKernelGGL(iwe_direct_kernel, dim3((unsigned)((n[i] + 255) / 256)), dim3(256), 0, stream, events[i], (long)n[i],
                                   flows ? flows[i] : nullptr, t0[i], scale[i],
                                   IweMap{maps[i][0], maps[i][1], maps[i][2], maps[i][3]}, h, w, acc, ndrop);
            hipLaunchKernelGGL(iwe_direct_finish_kernel, dim3(parts), dim3(256), 0, stream, acc, ndrop, iwe[i], hw, part, dropped);
            IweJobs one;
            memset(&one, 0, sizeof(one));
            one.j[0].part = part;
            one.j[0].dropped = dropped;
            one.j[0].nblk = 1;
            hipLaunchKernelGGL(iwe_moments_kernel, dim3(1), dim3(256), 0, stream, one, parts, (double)hw, moments + 4 * i);
            EEM_HIP_CHECK(hipGetLastError());
        }
        return EEM_OK;
    }
    const int ept = iwe_ept(nmax);
    long nblk_max = 0;
    char* q = scratch;
    for (int i = 0; i < k; ++i) {
        const IweLayout l = iwe_layout_binned((long)n[i], ept, pl);
        IweJob& J = jobs.j[i];
        J.ev = events[i];
        J.flow = flows ? flows[i] : nullptr;
        J.out = iwe[i];
        J.recs = reinterpret_cast<unsigned*>(q + l.recs);
        J.run_start = reinterpret_cast<unsigned*>(q + l.table);
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
        int rc;
        switch (ept) {
            case 1: rc = launch_bin<1>(jobs, k, nblk_max, h, w, pl, stream); break;
            case 2: rc = launch_bin<2>(jobs, k, nblk_max, h, w, pl, stream); break;
            default: rc = launch_bin<4>(jobs, k, nblk_max, h, w, pl, stream); break;
        }
        if (rc != EEM_OK) return rc;
    }
    const int lds = pl.cells * 8;
    // lanes per run: the smallest power of two >= 1.7 x the mean run length (a slab's records / bands), 4 .. 64
    int sgs = 2;
    while (sgs < 6 && (1 << sgs) * 10L * pl.nb < 17L * 2 * VT * ept) ++sgs;
    if (pl.cells <= 3072) {
        hipLaunchKernelGGL(iwe_band_kernel<256>, dim3(pl.nb, k), dim3(256), lds, stream, jobs, 2 * VT * ept, h, w, pl, sgs);
    } else {
        if (lds > 32 * 1024) EEM_RAISE_LDS(lds, iwe_band_kernel<VT>);
        hipLaunchKernelGGL(iwe_band_kernel<VT>, dim3(pl.nb, k), dim3(VT), lds, stream, jobs, 2 * VT * ept, h, w, pl, sgs);
    }
    hipLaunchKernelGGL(iwe_moments_kernel, dim3(k), dim3(256), 0, stream, jobs, pl.nb, (double)hw, moments);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}

Arena g_iwe_arena;

}  // namespace

Arena& iwe_arena() { return g_iwe_arena; }

extern "C" int eemflow_iwe_map_many(int k, const double* const* events, const int64_t* n, const float* const* flows, const double* t0,
                                    const double* scale, const double (*maps)[4], int h, int w, float* const* iwe, double* moments,
                                    void* stream) {
    EEM_REQUIRE(k >= 1 && k <= IWE_MAX_JOBS, "eemflow_iwe_many: 1..%d jobs per call; got %d", IWE_MAX_JOBS, k);
    EEM_REQUIRE(events && n && t0 && scale && maps && iwe && moments, "eemflow_iwe_many: NULL argument");
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 30), "eemflow_iwe_many: bad size %dx%d", h, w);
    for (int i = 0; i < k; ++i) {
        EEM_REQUIRE(n[i] >= 0 && n[i] < (1LL << 40), "eemflow_iwe_many: job %d has n=%ld events", i, (long)n[i]);
        EEM_REQUIRE((events[i] || n[i] == 0) && iwe[i], "eemflow_iwe_many: job %d has a NULL buffer", i);
    }
    std::lock_guard<std::mutex> guard(g_iwe_arena.lock);
    char* scratch = nullptr;
    void* token = nullptr;
    int rc = g_iwe_arena.take(iwe_scratch_bytes(k, n, h, w), stream, &scratch, &token);
    if (rc != EEM_OK) return rc;
    rc = iwe_launch(k, events, n, flows, t0, scale, maps, h, w, iwe, moments, scratch, (hipStream_t)stream);
    if (rc == EEM_OK) rc = g_iwe_arena.done(token, stream);
    return rc;
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
