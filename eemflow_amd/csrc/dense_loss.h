// What the dense loss terms of the ground-truth-free training route share: photo.hip (photometric and census), ssim.hip (weighted SSIM)
// and smooth.hip (edge-aware smoothness).  All three are built with -ffp-contract=off and keep one bitwise contract, stated here once:
// A block walks tiles of 16 x 64 cells: the grid is the number of tiles, capped at 2048 blocks that stride over them, so it depends on
// the shape alone.  Inside a tile the block walks the up to 16 jobs of the launch.  A thread owns the same four cells of the tile in
// every phase.  Per-thread fp64 sums are reduced per wave by shuffles and added, by the wave's lane 0, to the wave's own slot of the
// job in LDS - tiles arrive in the block's fixed order.  After the tile loop a block adds its waves' slots and writes one partial sum
// per job (and accumulator) to scratch; a one-wave-per-job launch adds the blocks' partial sums in a fixed order.  No atomics anywhere,
// and a job's arithmetic and summation order do not depend on its neighbours: a job's loss and gradient are bitwise the same from run
// to run and bitwise those of a one-job call.
#pragma once
#include "common.h"

#include <algorithm>

namespace {

constexpr int DL_TH = 16, DL_TW = 64;            // cells per tile
constexpr int DL_NT = 256;
constexpr int DL_WAVES = DL_NT / 64;
constexpr int DL_CELLS = DL_TH * DL_TW / DL_NT;  // cells of the tile per thread
constexpr int DL_MAX_JOBS = 16;
constexpr int DL_MAX_BLOCKS = 2048;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---- the tile walk: `for (long tile = blockIdx.x; tile < dense_tiles(..); tile += gridDim.x)`
struct DenseTile {
    int b, r0, c0;               // the sample, and the frame position of the tile's first cell
};

__device__ __forceinline__ long dense_tiles(int B, int tiles_x, int tiles_y) { return (long)B * tiles_y * tiles_x; }

__device__ __forceinline__ DenseTile dense_tile(long tile, int tiles_x, int tiles_y) {
    const int rem = (int)(tile % ((long)tiles_y * tiles_x));
    return {(int)(tile / ((long)tiles_y * tiles_x)), (rem / tiles_x) * DL_TH, (rem % tiles_x) * DL_TW};
}

// cell n of thread t is row (t + 256 n) / 64, column t % 64 of the tile
__device__ __forceinline__ int dense_cell_row(int tid, int n) { return (tid + n * DL_NT) / DL_TW; }
__device__ __forceinline__ int dense_cell_col(int tid) { return tid % DL_TW; }

// ---- the loss slots: NACC accumulators per job and wave, a member of each kernel's own LDS struct (a kernel with no other LDS
// declares them alignas(16): the write-out then reads 128 bits at a time)
template <int NACC>
struct DenseSlots {
    double v[DL_MAX_JOBS][DL_WAVES][NACC];
};

// at entry; no barrier: the caller's first __syncthreads() stands between this and the first dense_slots_add
template <int NACC>
__device__ __forceinline__ void dense_slots_zero(DenseSlots<NACC>& s, int tid) {
    static_assert(DL_MAX_JOBS * DL_WAVES * NACC <= DL_NT, "one slot per thread");
    if (tid < DL_MAX_JOBS * DL_WAVES * NACC) (&s.v[0][0][0])[tid] = 0.0;
}

// wave-uniform: every lane of the wave arrives here.  A wave owns its slot, tiles arrive in the block's fixed order.
// (one overload per accumulator count, the sums by value: an array parameter changed the callers' register allocation)
__device__ __forceinline__ void dense_slots_add(DenseSlots<1>& s, int tid, int job, double acc) {
    acc = wave_sum(acc);
    if ((tid & 63) == 0) s.v[job][tid >> 6][0] += acc;
}

__device__ __forceinline__ void dense_slots_add(DenseSlots<2>& s, int tid, int job, double acc0, double acc1) {
    acc0 = wave_sum(acc0), acc1 = wave_sum(acc1);
    if ((tid & 63) == 0) {
        s.v[job][tid >> 6][0] += acc0;
        s.v[job][tid >> 6][1] += acc1;
    }
}

// after the tile loop and a __syncthreads(): part[(job * gridDim.x + blockIdx.x) * NACC + a] = the block's sum
template <int NACC>
__device__ __forceinline__ void dense_slots_write(const DenseSlots<NACC>& s, int tid, int k, double* __restrict__ part) {
    if (tid < NACC * k) {
        const int job = tid / NACC, a = tid % NACC;
        double v = 0.0;
#pragma unroll
        for (int wv = 0; wv < DL_WAVES; ++wv) v += s.v[job][wv][a];
        part[((size_t)job * gridDim.x + blockIdx.x) * NACC + a] = v;
    }
}

// one wave per job: the blocks' partial sums in a fixed order, then L = (S / n1) / D (photo.hip, ssim.hip; smooth.hip's two sums have
// a finish of their own)
__global__ __launch_bounds__(64) void dense_finish_kernel(const double* __restrict__ part, int nblk, double n1, const double* __restrict__ den,
                                                          double* __restrict__ loss) {
    const int job = blockIdx.x, lane = threadIdx.x;
    double v = 0.0;
    for (int i = lane; i < nblk; i += 64) v += part[(size_t)job * nblk + i];
    v = wave_sum(v);
    if (lane == 0) loss[job] = (v / n1) / den[job];
}

// ---- the host side
inline int dense_blocks(int B, int H, int W, int* tx, int* ty) {
    *tx = ceil_div(W, DL_TW);
    *ty = ceil_div(H, DL_TH);
    const long tiles = (long)B * *tx * *ty;
    return (int)std::min<long>(tiles, DL_MAX_BLOCKS);
}

inline bool dense_shape_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= (1L << 30); }

// doubles of scratch for k jobs: `dens` denominators first (DL_MAX_JOBS or none), then nacc partial sums per job and block
inline size_t dense_scratch_doubles(int k, int B, int H, int W, int dens, int nacc) {
    if (k < 1 || k > DL_MAX_JOBS || !dense_shape_ok(B, H, W)) return 0;
    int tx, ty;
    return dens + (size_t)k * dense_blocks(B, H, W, &tx, &ty) * nacc;
}

// the shape of a warp term's launch
struct DenseShape {
    int B, C, H, W, tiles_x, tiles_y;
    double sx, sy;               // d ix / du, d iy / dv of the align_corners=False grid sample
    double n1;                   // the numerator's divisor: the term sets it
};

// fills all but n1; returns the grid
inline int dense_shape(DenseShape& s, int B, int C, int H, int W) {
    s.B = B, s.C = C, s.H = H, s.W = W;
    s.sx = ((double)W / 2.0) * (2.0 / (double)std::max(W - 1, 1));
    s.sy = ((double)H / 2.0) * (2.0 / (double)std::max(H - 1, 1));
    return dense_blocks(B, H, W, &s.tiles_x, &s.tiles_y);
}

// the jobs of a warp term's launch
struct DenseJobs {
    const float* flow[DL_MAX_JOBS];
    const float* img1[DL_MAX_JOBS];
    const float* img2[DL_MAX_JOBS];
    const float* mask[DL_MAX_JOBS];
    float* grad[DL_MAX_JOBS];
};

// fills the table from the entry point's arrays (mask, grad: NULL or one per job); `name`: the entry point, for the messages
inline int dense_fill_jobs(DenseJobs& jobs, const char* name, int k, const float* const* flow, const float* const* img1,
                           const float* const* img2, const float* const* mask, float* const* grad) {
    EEM_REQUIRE(flow && img1 && img2, "%s: flow, img1 or img2 is NULL", name);
    for (int i = 0; i < DL_MAX_JOBS; ++i) jobs.flow[i] = jobs.img1[i] = jobs.img2[i] = jobs.mask[i] = nullptr, jobs.grad[i] = nullptr;
    for (int i = 0; i < k; ++i) {
        EEM_REQUIRE(flow[i] && img1[i] && img2[i], "%s: job %d lacks its flow, img1 or img2 (NULL)", name, i);
        EEM_REQUIRE(!grad || grad[i], "%s: job %d has no gradient buffer (NULL)", name, i);
        jobs.flow[i] = flow[i];
        jobs.img1[i] = img1[i];
        jobs.img2[i] = img2[i];
        jobs.mask[i] = mask ? mask[i] : nullptr;
        jobs.grad[i] = grad ? grad[i] : nullptr;
    }
    return EEM_OK;
}

}  // namespace
