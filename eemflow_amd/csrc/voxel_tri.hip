// The DSEC voxel grid (reference: utils/dsec_utils.py:19-64, VoxelGrid.convert) - the input E-RAFT's published weights were trained on:
// N events given as fp32 columns x, y, t, p vote TRILINEARLY into a (bins, H, W) fp32 grid - sub-pixel (rectified) x and y, so eight
// votes per event - followed by the same mean / unbiased-sd normalisation over the non-zero voxels as voxel.hip's.
//
// Per event, every operation fp32 and unfused (this file is built with -ffp-contract=off):
//     dT  = t[n-1] - t[0]                                   only t[0] and t[n-1] set the scale: the set need not be sorted
//     tn  = ((float)(bins-1) * (t_i - t[0])) / dT
//     x0  = (int)x_i, y0 = (int)y_i, b0 = (int)tn           TRUNCATION toward zero, as torch's .int() - not floor
//     val = 2 p_i - 1
//     for xl in (x0, x0+1), yl in (y0, y0+1), bl in (b0, b0+1), where 0 <= xl < W, 0 <= yl < H, 0 <= bl < bins:
//         grid[bl][yl][xl] += ((val * (1 - |xl - x_i|)) * (1 - |yl - y_i|)) * (1 - |bl - tn|)
// What follows from it, and is reproduced: x = -0.5 truncates to x0 = 0 and votes +0.5 into column 0 and -0.5 into column 1 (negative
// y and tn alike; tn < 0 where t_i < t[0]); corners at xl == W, yl == H, bl == bins are masked and wrap nowhere (voxel.hip's reference
// wraps x >= W into the next row: another quirk, another file); the last event has tn == bins-1 and votes into the last bin only.
// An event whose x, y or tn is not finite or not below 2^31 in magnitude is dropped whole (the reference's cast is undefined there):
// with dT == 0 - a single event included - tn is NaN or inf everywhere, every vote is dropped and the grid is all +0.0.
//
// A trilinear event is four pixels x (bin b, bin b+1): four records of exactly the 12-byte format {pixel-in-band | bin << 16, left vote,
// right vote} that vox_band_kernel consumes (vox_shared.h), so the launch sequence is voxel.hip's with another first kernel:
//   1. voxtri_bin_kernel   1024 threads x EPT (1, 2) events: reads the four columns, derives up to four records per event - one per pixel
//                          inside the image; the two rows of an event may fall into different bands - ranks them per band with LDS integer
//                          atomics and leaves its slab of 4096 x EPT records sorted by band, plus its row of the run table.  No global
//                          atomics.  b0 == -1 (tn in (-2, -1]) has only its RIGHT vote inside the grid: the record then carries it as the
//                          left vote of bin 0 beside a zero; b0 == bins-1 needs nothing, the band kernel drops a right vote past the last
//                          bin.  Optional fused rectification: x, y are then RAW int16 / int32 sensor coordinates and a per-set
//                          (Hmap, Wmap, 2) fp32 map supplies (x', y') = map[y][x] (DSEC's loading step: saves writing and reading
//                          8 B of rectified coordinates per event, and the gather launch); a raw coordinate outside the map is dropped;
//   2. vox_band_kernel     unchanged: fp64 LDS cells, every cell rounded to fp32 once and stored (zeros included: no memset);
//   3. vox_norm_kernel     unchanged (normalize = 1).
// Grids the LDS layout cannot hold (band_px * bins > 19 200 cells, bins > 64), more than 8.4 M events, and EEM_VOX_DIRECT=1 take the
// direct form, one set at a time: voxtri_scatter_kernel adds the same votes with fp64 atomics into an fp64 image in scratch (so a cell
// is still the fp64 sum of its votes rounded once; voxel.hip's direct kernel adds in fp32), voxtri_finish_kernel rounds it into the grid
// and leaves the moments.
#include "vox_shared.h"

namespace {

struct TriJob {
    const void* x;           // fp32, or raw int16 / int32 with `map`
    const void* y;
    const float* t;
    const float* p;
    const float* map;        // [map_h][map_w][2] fp32 (x', y'), or NULL
    long n;
    unsigned* run_start;
    unsigned* recs;          // a slab of 4 * VT * EPT records per binning block
    int nblk;
    int pad;
};
struct TriJobs { TriJob j[VOX_MAX_JOBS]; };      // (72 bytes each: 2.3 KB of kernel arguments at 32 jobs)

// ------------------------------------------------------------------------------------------------ per-event arithmetic
struct TriVote {
    int x0, y0;              // the corner's pixel; the other three lie at +1
    int tl;                  // the records' left bin
    float ax[2];             // val * (1 - |xl - x|) at x0, x0 + 1
    float wy[2];             // 1 - |yl - y| at y0, y0 + 1
    float wl, wr;            // temporal weights of the left and right vote
    bool ok;
};

template <int XY>
__device__ __forceinline__ bool tri_xy(const TriJob& J, long i, int map_h, int map_w, float* x, float* y) {
    if constexpr (XY == EEMFLOW_XY_F32) {
        *x = static_cast<const float*>(J.x)[i];
        *y = static_cast<const float*>(J.y)[i];
        return true;
    } else {
        int xr, yr;
        if constexpr (XY == EEMFLOW_XY_I16) { xr = static_cast<const short*>(J.x)[i]; yr = static_cast<const short*>(J.y)[i]; }
        else { xr = static_cast<const int*>(J.x)[i]; yr = static_cast<const int*>(J.y)[i]; }
        if ((unsigned)xr >= (unsigned)map_w || (unsigned)yr >= (unsigned)map_h) return false;      // outside the map: dropped
        const float* m = J.map + ((size_t)yr * map_w + xr) * 2;
        *x = m[0];
        *y = m[1];
        return true;
    }
}

__device__ __forceinline__ TriVote tri_vote(float x, float y, float t, float p, float t0, float dT, int bins) {
    TriVote v;
    const float tn = ((float)(bins - 1) * (t - t0)) / dT;
    const float lim = 2147483648.f;
    v.ok = fabsf(x) < lim && fabsf(y) < lim && fabsf(tn) < lim;    // false for NaN and inf too (dT == 0: every event)
    if (!v.ok) return v;
    v.x0 = (int)x;                                                 // .int() truncates, dsec_utils.py:35-37
    v.y0 = (int)y;
    const int b0 = (int)tn;
    const float val = 2.f * p - 1.f;                               // :39
    v.ax[0] = val * (1.f - fabsf((float)v.x0 - x));                // :46, in its order: ((val * wx) * wy) * wt
    v.ax[1] = val * (1.f - fabsf((float)(v.x0 + 1) - x));
    v.wy[0] = 1.f - fabsf((float)v.y0 - y);
    v.wy[1] = 1.f - fabsf((float)(v.y0 + 1) - y);
    const float wt0 = 1.f - fabsf((float)b0 - tn), wt1 = 1.f - fabsf((float)(b0 + 1) - tn);
    if (b0 >= 0 && b0 < bins) { v.tl = b0; v.wl = wt0; v.wr = wt1; }          // (b0 + 1 == bins: the consumer drops the right vote)
    else if (b0 == -1) { v.tl = 0; v.wl = wt1; v.wr = 0.f; }                  // only bin b0 + 1 = 0 is inside: it travels as the left vote
    else v.ok = false;
    return v;
}

// ------------------------------------------------------------------------------------------------ 1. binning into slabs
// As vox_bin_kernel (voxel.hip), with up to four records per event: block `blk` owns the slab recs[blk * S .. (blk + 1) * S)
// (S = 4 * 1024 * EPT records) and row `blk` of the run table.
template <int EPT, int XY>
__global__ __launch_bounds__(VT) void voxtri_bin_kernel(TriJobs jobs, int bins, int h, int w, int map_h, int map_w, VoxPlan pl) {
    const TriJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // a shorter event set
    const long n = J.n;
    __shared__ unsigned hist[VT];
    __shared__ unsigned lpos[VT];
    __shared__ unsigned sh[VT / 64];
    extern __shared__ __attribute__((aligned(16))) unsigned stage[];   // the slab as it goes to memory: 3 words per record
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    const float t0 = J.t[0];
    const float dT = J.t[n - 1] - t0;
    constexpr int R = 4 * EPT;
    unsigned key[R], band[R], rank[R];
    float vl[R], vr[R];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long i = ((long)blockIdx.x * EPT + k) * VT + tid;
#pragma unroll
        for (int q = 0; q < 4; ++q) band[k * 4 + q] = 0xffffffffu;
        float x, y;
        if (i < n && tri_xy<XY>(J, i, map_h, map_w, &x, &y)) {
            const TriVote v = tri_vote(x, y, J.t[i], J.p[i], t0, dT, bins);
            if (v.ok) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int xl = v.x0 + (q & 1), yl = v.y0 + (q >> 1);
                    if ((unsigned)xl < (unsigned)w && (unsigned)yl < (unsigned)h) {    // :45 - xl == w, yl == h are masked, nothing wraps
                        const unsigned pix = (unsigned)yl * (unsigned)w + (unsigned)xl;
                        const unsigned bd = pix / (unsigned)pl.band_px;
                        const float a = v.ax[q & 1] * v.wy[q >> 1];
                        band[k * 4 + q] = bd;
                        key[k * 4 + q] = (pix - bd * (unsigned)pl.band_px) | ((unsigned)v.tl << 16);
                        vl[k * 4 + q] = a * v.wl;
                        vr[k * 4 + q] = a * v.wr;
                        rank[k * 4 + q] = atomicAdd(&hist[bd], 1u);    // LDS: the returned count is the rank inside the run
                    }
                }
            }
        }
    }
    vox_slab_out<R>(key, band, rank, vl, vr, hist, lpos, sh, stage, J.run_start, J.recs, pl);
}

// ------------------------------------------------------------------------------------------------ direct form
// the same votes, added with fp64 atomics into an fp64 image [bins][h][w] (zeroed by the host path)
template <int XY>
__global__ __launch_bounds__(256) void voxtri_scatter_kernel(TriJob J, int bins, int h, int w, int map_h, int map_w, double* __restrict__ img) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= J.n) return;
    float x, y;
    if (!tri_xy<XY>(J, i, map_h, map_w, &x, &y)) return;
    const float t0 = J.t[0];
    const TriVote v = tri_vote(x, y, J.t[i], J.p[i], t0, J.t[J.n - 1] - t0, bins);
    if (!v.ok) return;
    const long hw = (long)h * w;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int xl = v.x0 + (q & 1), yl = v.y0 + (q >> 1);
        if ((unsigned)xl < (unsigned)w && (unsigned)yl < (unsigned)h) {
            const float a = v.ax[q & 1] * v.wy[q >> 1];
            double* cell = img + (long)v.tl * hw + (long)yl * w + xl;
            unsafeAtomicAdd(cell, (double)(a * v.wl));
            if (v.tl + 1 < bins) unsafeAtomicAdd(cell + hw, (double)(a * v.wr));
        }
    }
}

// every cell rounded to fp32 once and stored; the block's moments of the non-zero voxels in its slot
__global__ __launch_bounds__(VT) void voxtri_finish_kernel(const double* __restrict__ img, float* __restrict__ grid, long total,
                                                           VoxSums* __restrict__ acc) {
    __shared__ double sh3[VT / 64 * 3];
    double c = 0.0, sm = 0.0, q = 0.0;
    for (long i = (long)blockIdx.x * VT + threadIdx.x; i < total; i += (long)gridDim.x * VT) {
        const float v = (float)img[i];
        grid[i] = v;
        if (v != 0.f) { c += 1.0; sm += (double)v; q += (double)v * (double)v; }
    }
    vox_store_sums(c, sm, q, acc + blockIdx.x, sh3);
}

// ------------------------------------------------------------------------------------------------ host
constexpr int TRI_MAX_EPT = 2;                                     // 8 192 records = 96 KB of slab in LDS

bool tri_plan(int64_t n, int bins, int h, int w, VoxPlan* pl, int* lds_bytes) {
    return vox_blocks((long)n, TRI_MAX_EPT) <= VOX_MAX_BLOCKS && make_plan(1, bins, h, w, nullptr, pl, lds_bytes);
}

inline long tri_slots(int64_t n) { return (4 * (long)n + 8191) / 8192 * 8192 + 8192; }     // whole slabs of either size: round up

template <int EPT, int XY>
int launch_tri_bin(const TriJobs& jobs, int njobs, long nblk_max, int bins, int h, int w, int map_h, int map_w, const VoxPlan& pl,
                   hipStream_t stream) {
    constexpr int stage_bytes = VT * EPT * 4 * 12;
    if (stage_bytes > 48 * 1024) EEM_RAISE_LDS(stage_bytes, voxtri_bin_kernel<EPT, XY>);
    hipLaunchKernelGGL((voxtri_bin_kernel<EPT, XY>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, bins, h, w, map_h,
                       map_w, pl);
    return EEM_OK;
}

template <int XY>
int launch_tri_bin_xy(int ept, const TriJobs& jobs, int njobs, long nblk_max, int bins, int h, int w, int map_h, int map_w, const VoxPlan& pl,
                      hipStream_t stream) {
    return ept == 1 ? launch_tri_bin<1, XY>(jobs, njobs, nblk_max, bins, h, w, map_h, map_w, pl, stream)
                    : launch_tri_bin<2, XY>(jobs, njobs, nblk_max, bins, h, w, map_h, map_w, pl, stream);
}

const char* const kTriXY[3] = {"", "_i16", "_i32"};

}  // namespace

// sums + the record slots (four per event, 16 bytes each as voxel.hip sizes them) + the run table; the direct form: sums + an fp64 image.
// nmax: the longest set of the call - one set beyond the banded form sends ALL of them to the direct one, so all are sized for it
size_t voxel_tri_scratch_bytes(int64_t n, int64_t nmax, int bins, int h, int w) {
    const long m = n > 0 ? (long)n : 0;
    VoxPlan pl;
    int lds = 0;
    if (bins < 1 || h < 1 || w < 1) return sizeof(VoxScratch);
    if (!tri_plan(std::max((long)nmax, m), bins, h, w, &pl, &lds)) return sizeof(VoxScratch) + (size_t)bins * h * w * sizeof(double);
    const long blocks = std::max(512L, std::min(VOX_MAX_BLOCKS, vox_blocks(m, TRI_MAX_EPT) + 1));
    return sizeof(VoxScratch) + (size_t)tri_slots(m) * 16 + (size_t)blocks * VT * sizeof(unsigned);
}

// njobs trilinear voxelizations of one grid shape in one launch sequence; scratch[k] >= voxel_tri_scratch_bytes(n[k], max n, ...) each
int voxel_tri_launch_jobs(int njobs, const void* const* x, const void* const* y, const float* const* t, const float* const* p, const int64_t* n,
                          int xy_type, const float* const* maps, int map_h, int map_w, int bins, int h, int w, int normalize,
                          float* const* grid, void* const* scratch, hipStream_t stream) {
    EEM_REQUIRE(njobs >= 1 && njobs <= VOX_MAX_JOBS, "voxelize_trilinear: %d jobs (1..%d per launch sequence)", njobs, VOX_MAX_JOBS);
    for (int k = 0; k < njobs; ++k)
        EEM_REQUIRE(n[k] >= 1, "voxelize_trilinear: need at least one event (the reference indexes t[-1], dsec_utils.py:33), got n=%ld", (long)n[k]);
    EEM_REQUIRE(bins > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31), "voxelize_trilinear: bad shape bins=%d h=%d w=%d", bins, h, w);
    // (the entry point in api.hip has checked normalize, xy_type and its pairing with the maps)
    const long total = (long)bins * h * w;
    VoxPlan pl;
    int lds = 0;
    bool planned = true;
    int64_t nmax = n[0];
    for (int k = 0; k < njobs; ++k) {
        planned = planned && tri_plan(n[k], bins, h, w, &pl, &lds);
        nmax = std::max(nmax, n[k]);
    }
    VoxJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    char form[128];
    if (!planned) {                                                    // the direct form, one set after the other
        const int nsums = (int)std::min(512L, (total + 4095) / 4096);
        for (int k = 0; k < njobs; ++k) {
            VoxScratch* sc = (VoxScratch*)scratch[k];
            double* img = reinterpret_cast<double*>(sc + 1);
            const TriJob J = {x[k], y[k], t[k], p[k], maps ? maps[k] : nullptr, (long)n[k], nullptr, nullptr, 0, 0};
            EEM_HIP_CHECK(hipMemsetAsync(img, 0, (size_t)total * sizeof(double), stream));
            const dim3 g((unsigned)((n[k] + 255) / 256));
            switch (xy_type) {
                case EEMFLOW_XY_F32: hipLaunchKernelGGL(voxtri_scatter_kernel<EEMFLOW_XY_F32>, g, dim3(256), 0, stream, J, bins, h, w, map_h, map_w, img); break;
                case EEMFLOW_XY_I16: hipLaunchKernelGGL(voxtri_scatter_kernel<EEMFLOW_XY_I16>, g, dim3(256), 0, stream, J, bins, h, w, map_h, map_w, img); break;
                default: hipLaunchKernelGGL(voxtri_scatter_kernel<EEMFLOW_XY_I32>, g, dim3(256), 0, stream, J, bins, h, w, map_h, map_w, img); break;
            }
            hipLaunchKernelGGL(voxtri_finish_kernel, dim3(nsums), dim3(VT), 0, stream, img, grid[k], total, sc->acc);
            EEM_HIP_CHECK(hipGetLastError());
            if (normalize) {
                VoxJobs one;
                memset(&one, 0, sizeof(one));
                one.j[0].grid = grid[k]; one.j[0].acc = sc->acc;
                const int rc = vox_launch_norm(one, 1, total, nsums, stream);
                if (rc != EEM_OK) return rc;
            }
        }
        snprintf(form, sizeof(form), "tri:j1:direct64%s+finish%s", kTriXY[xy_type], normalize ? "+norm" : "");
        voxel_note_form(form);
        return EEM_OK;
    }
    // one EPT for all jobs (the longest set's): a shorter one's slabs are the same size, it just fills fewer of them
    const int ept = vox_blocks((long)nmax, 1) > 512 ? TRI_MAX_EPT : 1;
    const int slab = VT * ept * 4;
    TriJobs tj;
    memset(&tj, 0, sizeof(tj));
    long nblk_max = 0;
    for (int k = 0; k < njobs; ++k) {
        VoxScratch* sc = (VoxScratch*)scratch[k];
        const long slots = tri_slots(n[k]);
        VoxJob& J = jobs.j[k];
        J.n = (long)n[k];
        J.recs = reinterpret_cast<unsigned*>(sc + 1);
        J.run_start = J.recs + slots * 3;                              // (the scratch is sized at 16 bytes per slot)
        J.grid = grid[k]; J.acc = sc->acc;
        J.nblk = (int)vox_blocks((long)n[k], ept);
        EEM_REQUIRE((long)J.nblk * slab <= slots, "voxelize_trilinear: slab budget (n=%ld, ept=%d)", (long)n[k], ept);
        tj.j[k] = {x[k], y[k], t[k], p[k], maps ? maps[k] : nullptr, (long)n[k], J.run_start, J.recs, J.nblk, 0};
        nblk_max = std::max(nblk_max, (long)J.nblk);
    }
    int rc;
    switch (xy_type) {
        case EEMFLOW_XY_F32: rc = launch_tri_bin_xy<EEMFLOW_XY_F32>(ept, tj, njobs, nblk_max, bins, h, w, map_h, map_w, pl, stream); break;
        case EEMFLOW_XY_I16: rc = launch_tri_bin_xy<EEMFLOW_XY_I16>(ept, tj, njobs, nblk_max, bins, h, w, map_h, map_w, pl, stream); break;
        default: rc = launch_tri_bin_xy<EEMFLOW_XY_I32>(ept, tj, njobs, nblk_max, bins, h, w, map_h, map_w, pl, stream); break;
    }
    if (rc != EEM_OK) return rc;
    const int vec4 = vox_vec4(pl, njobs, grid);
    const int sgs = vox_sgs(slab, pl.nb);
    int bt = 0;
    if ((rc = vox_launch_band(jobs, njobs, slab, bins, pl, lds, vec4, normalize, (int)VOX_BAND_RAW, sgs, &bt, stream)) != EEM_OK) return rc;
    EEM_HIP_CHECK(hipGetLastError());
    if (normalize && (rc = vox_launch_norm(jobs, njobs, total, pl.nb, stream)) != EEM_OK) return rc;
    snprintf(form, sizeof(form), "tri:j%d:bin_e%d%s+band%d_%s_s%d_%s", njobs, ept, kTriXY[xy_type], bt, vec4 ? "v4" : "v1", sgs,
             normalize ? "raw_sums+norm" : "raw");
    voxel_note_form(form);
    return EEM_OK;
}
