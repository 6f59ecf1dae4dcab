// Event voxelization (reference: loader/loader_utils.py:447-537, EventSequenceToVoxelGrid_Pytorch):
// temporal-bilinear voting of N events (t, x, y, p) into a (bins, H, W) fp32 grid, then mean /
// unbiased-std normalisation over the non-zero voxels.
//
// Integer work is bit-exact with the reference: the f64 time scaling is evaluated in the same
// order ((bins-1)*(t-t0))/dT with IEEE mul/div (this file is built with -ffp-contract=off), floor,
// truncating casts and the flat index x + y*W + bin*W*H are int64.
//
// Events arrive time-sorted, so neighbouring lanes vote into unrelated voxels: two fp32 atomics per event
// straight to HBM run at ~20 G atomics/s whatever the kernel does (0.2 ms for 2e6 events).  The default path
// therefore bins first and adds in LDS.  Up to VOX_MAX_JOBS event sets of one grid shape share each launch (blockIdx.y = job:
// eemflow_voxelize_pair / eemflow_voxelize_many - at 2e5 events per set the launches sit at their fixed costs, so a call per set pays
// them per set):
//   1. vox_bin_kernel     every block of 1024 threads derives the votes of its 1024 x EPT events (EPT = 1, 2, 4, 8 by event count), ranks
//                         them per band of `band_px` consecutive pixels with LDS integer atomics (the return value is the vote's rank
//                         in its run), scans the counts and builds its slab of 12-BYTE records {pixel-in-band | bin << 16, left
//                         vote, right vote} sorted by band IN LDS, from where the slab leaves as whole 16-byte pieces of
//                         consecutive threads, plus a row of run offsets (run_start[blk][band]): no global atomics, no counting
//                         pass; also the optional int64 index outputs (event order);
//   2. vox_band_kernel    one block per band (BT = 256 / 512 / 1024 threads by the band's LDS size; 9216 cells = 72 KB of fp64 by
//                         default -> 1024 threads, two blocks per CU; 57 VGPRs, no scratch).  A run = the band's records of one
//                         binning block; 2^sgs adjacent lanes share a run (1.7 x the mean run length), eight runs per thread in
//                         flight: their table entries as one batch of buffer loads, then their first records as one batch of
//                         12-byte buffer loads (out-of-range lanes read zeros: no branches), the rare longer runs in a clean-up
//                         loop.  The band accumulates in fp64 LDS cells (ds_add_f64: ds_add_f32 runs at 0.33 lanes per clock and CU
//                         on this chip, 8 - 20 x slower, profiles/r04_lds_atomics.txt).  One pass then rounds every cell to fp32
//                         once, stores it (zeros included: no memset of the grid) and leaves the f64 (count, sum, sum of squares)
//                         of the band's non-zero voxels (a thread's few dozen cells as an integer count and fp32 partial sums, widened
//                         once: round 6).  The band is zeroed under the first table round trip (LDS-only block wait);
//   3. normalisation (loader_utils.py:527-535), one of
//        vox_norm_kernel   (normalize = 1) adds the band sums in a fixed order, mean / unbiased sd, rewrites the non-zero voxels;
//        vox_stats_kernel  (normalize = 2, "deferred") writes {mean, sd, scale, any} into the four floats BEHIND the grid and leaves
//                          the grid raw: the first encoder layer normalises as it reads (conv_enc1.hip, NORM) - at 2e5 events per
//                          volume the rewrite is half of a sample's voxelization time (37 -> 18 us per sample, ten per call).
// Optional (EEM_VOX_TWOPASS=<r>, off by default): with fewer than one event per r voxels the band kernel runs twice instead of
// step 3 - a moments-only launch, then a launch that accumulates the bands again and stores them already normalised.  Measured at
// 2e5 events per 4.6 M voxels: no gain.
// HBM traffic: 32 B (event) + 12 B written + 12 B read (record) per event + 4 B per voxel (normalize = 1: + 8 B per voxel).
// An event with x >= W lands in a neighbouring row exactly as the reference's flat index_add_ puts it; votes whose
// flat pixel index x + y*W falls outside the image (the reference raises) are dropped on this path, the index
// outputs still report them.  Grid values: every voxel's votes are summed exactly (fp64) and rounded once - within 2e-5 of the
// reference's fp32 index_add_, whose order is not defined either; the integer indices are bit-exact.
// Grids too large for the LDS band layout (band_px * bins > 19 200 cells, bins > 64) and more than 33.5 M events
// take the direct atomic kernel (one job at a time).
// Which of these a call ran is reported by eemflow_voxelize_last_form (a test observable: integers stored on the host, no launch).
// Everything behind the binning kernel - the record format, the band kernel, the moments, the normalisation / statistics kernels, the
// plan - lives in vox_shared.h, which the DSEC trilinear voxelizer (voxel_tri.hip: four records per event) includes too; so does the per-event
// arithmetic of this file's votes, which voxel_cols.hip applies to the raw columns of a recording (no float64 table in between).
#include <string.h>

#include "common.h"

#include <algorithm>
#include <cstdlib>

#include "vox_shared.h"

namespace {

// ------------------------------------------------------------------------------------------------ per-event arithmetic (vox_shared.h: VoxVote, VoxTime, vox_vote, vox_record)
__device__ __forceinline__ VoxTime vox_time(const double* __restrict__ ev, long n) {
    VoxTime tm;
    tm.t0 = ev[0];
    tm.dT = ev[(n - 1) * 4] - tm.t0;
    if (tm.dT == 0.0) tm.dT = 1.0;                                 // loader_utils.py:485-486
    return tm;
}

// ------------------------------------------------------------------------------------------------ direct atomic path
__global__ __launch_bounds__(256) void voxel_scatter_kernel(const double* __restrict__ ev, long n, int bins, int h,
                                                            int w, float* __restrict__ grid,
                                                            long long* __restrict__ idx_left,
                                                            long long* __restrict__ idx_right) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const VoxTime tm = vox_time(ev, n);
    const VoxVote v = vox_vote(ev[i * 4 + 0], ev[i * 4 + 1], ev[i * 4 + 2], ev[i * 4 + 3], tm, bins, h, w);
    // the reference adds at the FLAT index (index_add_ on the flattened grid, loader_utils.py:505-521): a pixel index outside
    // [0, h*w) lands in a neighbouring bin's plane as long as the flat index stays inside the grid; outside the grid the
    // reference raises - those votes are dropped here (writing past the allocation is not an option)
    const long long total = (long long)bins * h * w;
    if (v.okl && v.il >= 0 && v.il < total) atomicAdd(grid + v.il, v.vl);
    if (v.okr && v.ir >= 0 && v.ir < total) atomicAdd(grid + v.ir, v.vr);
    if (idx_left) idx_left[i] = v.okl ? v.il : -1;
    if (idx_right) idx_right[i] = v.okr ? v.ir : -1;
}

// ------------------------------------------------------------------------------------------------ 1. binning into slabs
// Block `blk` owns the slab recs[blk * E .. (blk + 1) * E) (E = 1024 * EPT events per block): its votes, sorted by band, and
// row `blk` of the run table: run_start[blk][b] = offset of band b's run inside the slab, run_start[blk][nb] = its end.
template <int EPT>
__global__ __launch_bounds__(VT) void vox_bin_kernel(VoxJobs jobs, int bins, int h, int w, VoxPlan pl) {
    const VoxJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // the shorter event set of a pair
    const double* __restrict__ ev = J.ev;
    const long n = J.n;
    long long* __restrict__ idx_left = J.idx_left;
    long long* __restrict__ idx_right = J.idx_right;
    __shared__ unsigned hist[VT];
    __shared__ unsigned lpos[VT];
    __shared__ unsigned sh[VT / 64];
    extern __shared__ __attribute__((aligned(16))) unsigned stage[];   // the slab as it goes to memory: 3 words per record
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    const VoxTime tm = vox_time(ev, n);
    const f64x2* e2 = reinterpret_cast<const f64x2*>(ev);
    unsigned key[EPT], band[EPT], rank[EPT];
    float vl[EPT], vr[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long i = ((long)blockIdx.x * EPT + k) * VT + tid;
        band[k] = 0xffffffffu;
        if (i < n) {
            const f64x2 a = e2[i * 2], b = e2[i * 2 + 1];
            const VoxVote v = vox_vote(a[0], a[1], b[0], b[1], tm, bins, h, w);
            if (idx_left) idx_left[i] = v.okl ? v.il : -1;
            if (idx_right) idx_right[i] = v.okr ? v.ir : -1;
            unsigned bd;
            if (vox_record(v, bins, pl, &bd, &key[k], &vl[k], &vr[k])) {
                band[k] = bd;
                rank[k] = atomicAdd(&hist[bd], 1u);                // LDS: the returned count is the rank inside the run
            }
        }
    }
    vox_slab_out<EPT>(key, band, rank, vl, vr, hist, lpos, sh, stage, J.run_start, J.recs, pl);
}

template <int EPT>
int launch_bin(const VoxJobs& jobs, int njobs, long nblk_max, int bins, int h, int w, const VoxPlan& pl, hipStream_t stream) {
    constexpr int stage_bytes = VT * EPT * 12;
    if (stage_bytes > 48 * 1024) EEM_RAISE_LDS(stage_bytes, vox_bin_kernel<EPT>);
    hipLaunchKernelGGL((vox_bin_kernel<EPT>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, bins, h, w, pl);
    return EEM_OK;
}

// what this thread's last launch sequence ran (eemflow_voxelize_last_form)
thread_local VoxForm t_vox_form = {0, 0, 0, 0, 0, 0, 0};
thread_local char t_vox_text[128] = "";   // not empty: the last sequence was voxel_tri.hip's or voxel_cols.hip's and this is its report

}  // namespace

extern "C" int eemflow_voxelize_last_form(char* buf, int cap) {
    EEM_REQUIRE(buf && cap >= 1, "eemflow_voxelize_last_form: bad arguments");
    if (t_vox_text[0]) snprintf(buf, (size_t)cap, "%s", t_vox_text);
    else vox_form_text(t_vox_form, "bin", buf, (size_t)cap);
    return EEM_OK;
}

#ifdef EEM_VOX_STAMPS
extern "C" __attribute__((visibility("default"))) int eemflow_debug_read_vox_stamps(unsigned long long* dst, size_t n) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_vox_stamps), n * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
#endif


// sums + one 16-byte record slot per event (slabs are whole blocks: round up) + the run table
size_t voxel_scratch_bytes(int64_t n) {
    const long m = n > 0 ? (long)n : 0;
    const long slots = (m + 8191) / 8192 * 8192 + 8192;
    const long blocks = std::max(512L, std::min(VOX_MAX_BLOCKS, vox_blocks(m, 8) + 1));
    return sizeof(VoxScratch) + (size_t)slots * 16 + (size_t)blocks * VT * sizeof(unsigned);
}

// njobs (1 or 2) voxelizations of the same grid shape in one launch sequence; scratch[k] >= voxel_scratch_bytes(n[k]) each
int voxel_launch_jobs(int njobs, const double* const* events, const int64_t* n, int bins, int h, int w, int normalize, float* const* grid,
                      int64_t* const* idx_left, int64_t* const* idx_right, void* const* scratch, hipStream_t stream) {
    EEM_REQUIRE(njobs >= 1 && njobs <= VOX_MAX_JOBS, "voxelize: %d jobs (1..%d per launch sequence)", njobs, VOX_MAX_JOBS);
    for (int k = 0; k < njobs; ++k)
        EEM_REQUIRE(n[k] >= 1, "voxelize: need at least one event (the reference indexes events[-1], "
                               "loader_utils.py:476), got n=%ld", (long)n[k]);
    EEM_REQUIRE(bins > 0 && h > 0 && w > 0, "voxelize: bad shape bins=%d h=%d w=%d", bins, h, w);
    EEM_REQUIRE(normalize >= 0 && normalize <= 2, "voxelize: normalize is 0 (raw), 1 (normalised grid) or 2 (raw grid + record); got %d", normalize);
    const long total = (long)bins * h * w;
    VoxPlan pl;
    int lds = 0;
    int nsums = 0;
    int64_t nmax = n[0];
    for (int k = 1; k < njobs; ++k) nmax = n[k] > nmax ? n[k] : nmax;
    bool planned = true;
    for (int k = 0; k < njobs; ++k) planned = planned && make_plan(n[k], bins, h, w, events[k], &pl, &lds);
    if (!planned && njobs >= 2) {                                      // the direct kernel has no multi-job form: one after the other
        for (int k = 0; k < njobs; ++k) {
            const int rc = voxel_launch_jobs(1, events + k, n + k, bins, h, w, normalize, grid + k, idx_left + k, idx_right + k, scratch + k, stream);
            if (rc != EEM_OK) return rc;
        }
        return EEM_OK;
    }
    VoxJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    VoxForm vf = {njobs, 0, 0, 0, 0, normalize ? 1 : 0, normalize};   // (host only: what eemflow_voxelize_last_form reports)
    if (planned) {
        const int ept = vox_ept((long)nmax);                           // the run table is sized for these block counts
        // one EPT for both jobs (the longer set's): the shorter one's slabs are the same size, it just fills fewer of them
        long nblk_max = 0;
        for (int k = 0; k < njobs; ++k) {
            VoxScratch* sc = (VoxScratch*)scratch[k];
            const long slots = ((long)n[k] + 8191) / 8192 * 8192 + 8192;
            VoxJob& J = jobs.j[k];
            J.ev = events[k]; J.n = (long)n[k];
            J.recs = reinterpret_cast<unsigned*>(sc + 1);
            J.run_start = J.recs + slots * 3;                          // (the scratch is sized at 16 bytes per slot)
            J.idx_left = (long long*)idx_left[k]; J.idx_right = (long long*)idx_right[k];
            J.grid = grid[k]; J.acc = sc->acc;
            J.nblk = (int)vox_blocks((long)n[k], ept);
            EEM_REQUIRE((long)J.nblk * VT * ept <= slots, "voxelize: slab budget (n=%ld, ept=%d)", (long)n[k], ept);
            nblk_max = std::max(nblk_max, (long)J.nblk);
        }
        int rc;
        switch (ept) {
            case 1: rc = launch_bin<1>(jobs, njobs, nblk_max, bins, h, w, pl, stream); break;
            case 2: rc = launch_bin<2>(jobs, njobs, nblk_max, bins, h, w, pl, stream); break;
            case 4: rc = launch_bin<4>(jobs, njobs, nblk_max, bins, h, w, pl, stream); break;
            default: rc = launch_bin<8>(jobs, njobs, nblk_max, bins, h, w, pl, stream); break;
        }
        if (rc != EEM_OK) return rc;
        if ((rc = vox_launch_after_bin(jobs, njobs, ept, (long)nmax, bins, total, normalize, pl, lds, grid, &vf, stream)) != EEM_OK) return rc;
        t_vox_form = vf;
        t_vox_text[0] = 0;
        return EEM_OK;
    }
    VoxScratch* sc = (VoxScratch*)scratch[0];
    jobs.j[0].grid = grid[0]; jobs.j[0].acc = sc->acc;
    EEM_HIP_CHECK(hipMemsetAsync(grid[0], 0, total * sizeof(float), stream));
    hipLaunchKernelGGL(voxel_scatter_kernel, dim3((unsigned)((n[0] + 255) / 256)), dim3(256), 0, stream, events[0],
                       (long)n[0], bins, h, w, grid[0], (long long*)idx_left[0], (long long*)idx_right[0]);
    if (normalize) {
        nsums = (int)((total + 4095) / 4096 < 512 ? (total + 4095) / 4096 : 512);
        hipLaunchKernelGGL(vox_moments_kernel, dim3(nsums), dim3(VT), 0, stream, grid[0], total, sc->acc);
    }
    EEM_HIP_CHECK(hipGetLastError());
    if (normalize == 2) {                                              // deferred: the record behind each grid, no pass over the grids
        hipLaunchKernelGGL(vox_stats_kernel, dim3(njobs), dim3(VT), 0, stream, jobs, total, nsums);
        EEM_HIP_CHECK(hipGetLastError());
        t_vox_form = vf;
        t_vox_text[0] = 0;
        return EEM_OK;
    }
    if (normalize) {
        const int rc = vox_launch_norm(jobs, njobs, total, nsums, stream);
        if (rc != EEM_OK) return rc;
    }
    t_vox_form = vf;
    t_vox_text[0] = 0;
    return EEM_OK;
}

// voxel_tri.hip's and voxel_cols.hip's launch sequences report through the same observable, in their own words
void voxel_note_form(const char* text) {
    snprintf(t_vox_text, sizeof(t_vox_text), "%s", text);
}

int voxel_launch(const double* events, int64_t n, int bins, int h, int w, int normalize, float* grid,
                 int64_t* idx_left, int64_t* idx_right, void* scratch, hipStream_t stream) {
    return voxel_launch_jobs(1, &events, &n, bins, h, w, normalize, &grid, &idx_left, &idx_right, &scratch, stream);
}
