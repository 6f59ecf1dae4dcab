// What the two voxelizers share: voxel.hip (MVSEC / HREM: integer pixels, two temporal votes per event) and voxel_tri.hip (DSEC:
// sub-pixel coordinates, eight trilinear votes per event).  Both bin their votes into slabs of 12-byte records
// {pixel-in-band | bin << 16, left vote, right vote} sorted by band, beside a run table; from there on the work is the same and lives
// here once: the band kernel that adds the records in fp64 LDS cells and rounds every cell to fp32 once, the moments, the
// normalisation / statistics kernels, the plan that sizes the bands and the host helpers that launch them.  The algorithm is
// described in voxel.hip's header comment.  A third binning kernel, voxel_cols.hip's, makes voxel.hip's two votes from the raw columns
// of a recording: the per-event arithmetic of those votes (vox_vote, vox_record) and the second half of every binning block
// (vox_slab_out) live here too, once.  All three files are built with -ffp-contract=off.
#pragma once

#include <string.h>

#include "common.h"

#include <algorithm>
#include <cstdlib>

namespace {

struct VoxSums {             // (count, sum, sum of squares) of one block's non-zero voxels
    double count, sum, sumsq, pad;
};

// ------------------------------------------------------------------------------------------------ block helpers
constexpr int VT = 1024;                 // threads per block of the binned path (also the maximum number of bands)

// sum over the wave, in every lane: the four steps inside a 16-lane row are DPP moves (VALU), only the two across rows go through
// ds_bpermute - with all six as __shfl_xor a 3-value reduction was 36 dependent LDS round trips (~1.5 us in front of every
// moments store and every normalisation)
template <int CTRL>
__device__ __forceinline__ double dpp_add64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return v + __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ double wave_sum(double v) {
    v = dpp_add64<0xB1>(v);                     // quad_perm [1,0,3,2]
    v = dpp_add64<0x4E>(v);                     // quad_perm [2,3,0,1]
    v = dpp_add64<0x141>(v);                    // row_half_mirror
    v = dpp_add64<0x140>(v);                    // row_mirror
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// exclusive prefix sum over the block's NT threads (sh: NT / 64 words)
template <int NT = 1024>
__device__ __forceinline__ unsigned block_exscan(unsigned v, unsigned* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(x, d);
        if (lane >= d) x += t;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    unsigned before = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) before += k < wave ? sh[k] : 0u;
    return before + x - v;
}

struct VoxPlan {
    int band_px;             // pixels per band (multiple of 4 unless it covers the whole image)
    int nb;                  // bands
    unsigned hw;             // H * W
};
// ------------------------------------------------------------------------------------------------ per-event arithmetic (two temporal votes)
// What voxel.hip's binning kernel (events from the float64 table) and voxel_cols.hip's (events from a recording's raw columns) do with one
// event [t, x, y, p] once it is four doubles: the same text, so the same votes bit for bit.
struct VoxVote {
    long long il, ir;        // flat int64 indices of the two votes (valid where okl / okr)
    long long pix;           // x + y*W
    int tl;                  // left bin
    float vl, vr;
    bool okl, okr;
};

struct VoxTime {
    double t0, dT;
};

__device__ __forceinline__ VoxVote vox_vote(double t, double x, double y, double p, const VoxTime& tm, int bins, int h,
                                            int w) {
    VoxVote v;
    const double ts = ((double)(bins - 1) * (t - tm.t0)) / tm.dT;  // :488
    const long long xs = (long long)x;                             // .long() truncates, :490-491
    const long long ys = (long long)y;
    float pol = (float)p;
    if (pol == 0.f) pol = -1.f;                                    // :493
    const double tis = floor(ts);
    const long long tl = (long long)tis;
    const float dts = (float)(ts - tis);
    v.vl = pol * (1.0f - dts);
    v.vr = pol * dts;
    const long long plane = (long long)w * h;
    v.okl = (tis < (double)bins) && (tis >= 0.0);                  // :502-503
    v.okr = ((tis + 1.0) < (double)bins) && (tis >= 0.0);          // :517-518
    v.pix = xs + ys * w;
    v.il = v.pix + tl * plane;
    v.ir = v.pix + (tl + 1) * plane;
    v.tl = (int)tl;
    return v;
}

// The 12-byte record of an event's pair of votes: false where nothing of it lands inside the grid; else *band = its band and
// {*key, *vl, *vr} = {pixel-in-band | bin << 16, left vote, right vote}
__device__ __forceinline__ bool vox_record(const VoxVote& v, int bins, const VoxPlan& pl, unsigned* band, unsigned* key, float* vl,
                                           float* vr) {
    long long pix = v.pix;
    int tl = v.tl;
    float wl = v.vl, wr_ = v.okr ? v.vr : 0.f;                     // a masked right vote stays masked wherever the pair lands
    if (v.okl && (unsigned long long)pix >= (unsigned long long)pl.hw) {
        // flat-index semantics of the reference (see voxel_scatter_kernel): a pixel index outside the plane moves the
        // pair of votes by whole planes; each vote survives while ITS flat index stays inside the grid
        long long q = pix / (long long)pl.hw;
        if (pix - q * (long long)pl.hw < 0) --q;                   // floor division
        pix -= q * (long long)pl.hw;
        const long long t2 = (long long)tl + q;
        if (t2 == -1) { tl = 0; wl = wr_; wr_ = 0.f; }             // left vote in front of the grid, right vote in plane 0
        else tl = (t2 >= 0 && t2 < bins) ? (int)t2 : -1;
    }
    if (!(v.okl && tl >= 0)) return false;
    const unsigned bd = (unsigned)pix / (unsigned)pl.band_px;
    *band = bd;
    *key = ((unsigned)pix - bd * (unsigned)pl.band_px) | ((unsigned)tl << 16);
    *vl = wl;
    *vr = wr_;
    return true;
}

// One voxelization of a launch: blockIdx.y picks the job, so the two event sets of a sample (loader/HREM.py:226-232) share each of
// the three launches (same grid shape and plan, their own events, slabs, run tables, moments and grid)
struct VoxJob {
    const double* ev;
    long n;
    unsigned* run_start;
    unsigned* recs;          // 12-byte records {pixel-in-band | bin << 16, left vote, right vote}, a slab of VT * EPT per binning block
    long long* idx_left;
    long long* idx_right;
    float* grid;
    VoxSums* acc;
    int nblk;                // binning blocks (slabs) of this job
};
struct VoxJobs { VoxJob j[VOX_MAX_JOBS]; };      // (72 bytes each: 2.3 KB of kernel arguments at 32 jobs)

// The second half of a binning block (all VT threads call it, after the last rank was taken from hist[]): scans the band counts, writes
// row blockIdx.x of the run table, sorts the thread's up to R records {key, vl, vr} (band == 0xffffffff: none) by band into the LDS slab
// `stage` and stores the slab - R * VT record slots from recs on - as whole 16-byte pieces of consecutive threads (scattered 12-byte
// stores ran at half the rate).  hist, lpos: VT words of LDS; sh: VT / 64.
template <int R>
__device__ __forceinline__ void vox_slab_out(const unsigned (&key)[R], const unsigned (&band)[R], const unsigned (&rank)[R], const float (&vl)[R],
                                             const float (&vr)[R], unsigned* hist, unsigned* lpos, unsigned* sh, unsigned* stage,
                                             unsigned* __restrict__ run_start, unsigned* __restrict__ recs, const VoxPlan& pl) {
    const int tid = threadIdx.x;
    __syncthreads();
    const unsigned start = block_exscan(hist[tid], sh);            // bands >= nb hold 0: thread nb gets the slab's fill
    lpos[tid] = start;
    if (tid <= pl.nb) run_start[(size_t)blockIdx.x * (pl.nb + 1) + tid] = start;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (band[k] != 0xffffffffu) {
            unsigned* r = stage + 3u * (lpos[band[k]] + rank[k]);
            r[0] = key[k];
            r[1] = __float_as_uint(vl[k]);
            r[2] = __float_as_uint(vr[k]);
        }
    }
    __syncthreads();
    const unsigned words = 3u * lpos[pl.nb];
    u32x4* slab = reinterpret_cast<u32x4*>(recs + (size_t)blockIdx.x * (VT * R) * 3);
    const u32x4* st4 = reinterpret_cast<const u32x4*>(stage);
    for (unsigned i = tid; i * 4 < words; i += VT) slab[i] = st4[i];   // (the last piece may carry up to three stale words: nobody reads them)
}

// ------------------------------------------------------------------------------------------------ moments
// Every block stores the f64 (count, sum, sum of squares) of its non-zero voxels in its own slot; the normalisation
// kernel's waves each add the slots up again (<= 1023 x 24 B from L2, no barrier).  Measured alternatives: f64 atomics
// into shared accumulators serialise (376 blocks on one line: +16 us, on 64 lines: +5 us), a ticket with the last block
// merging costs ~20 us of serial latency.
__device__ __forceinline__ void vox_store_sums(double c, double s, double q, VoxSums* __restrict__ mine, double* sh3) {
    c = wave_sum(c);
    s = wave_sum(s);
    q = wave_sum(q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    if (lane == 0) { sh3[wave * 3] = c; sh3[wave * 3 + 1] = s; sh3[wave * 3 + 2] = q; }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // (not __syncthreads: that would wait for the band's stores in flight too)
    if (threadIdx.x == 0) {
        c = s = q = 0.0;
        for (int k = 0; k < nw; ++k) { c += sh3[k * 3]; s += sh3[k * 3 + 1]; q += sh3[k * 3 + 2]; }
        mine->count = c;
        mine->sum = s;
        mine->sumsq = q;
    }
}

// mean / unbiased sd of the non-zero voxels from the per-block slots: slots strided over the threads, wave sums, then every
// thread adds the wave results in the same order (all NT threads of the block call this)
struct VoxNorm {
    float mean, sd;
    bool any, scale;
};

template <int NT = 1024>
__device__ __forceinline__ VoxNorm vox_final(const VoxSums* __restrict__ acc, int nsums, double* sh3) {
    const int tid = threadIdx.x;
    double c = 0.0, sm = 0.0, sq = 0.0;
    for (int k = tid; k < nsums; k += NT) { c += acc[k].count; sm += acc[k].sum; sq += acc[k].sumsq; }
    c = wave_sum(c);
    sm = wave_sum(sm);
    sq = wave_sum(sq);
    if ((tid & 63) == 0) { sh3[(tid >> 6) * 3] = c; sh3[(tid >> 6) * 3 + 1] = sm; sh3[(tid >> 6) * 3 + 2] = sq; }
    __syncthreads();
    c = sm = sq = 0.0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) { c += sh3[k * 3]; sm += sh3[k * 3 + 1]; sq += sh3[k * 3 + 2]; }
    VoxNorm nm;
    nm.any = c != 0.0;                                             // :529
    double m2 = nm.any ? sq - sm * sm / c : 0.0;                   // sum (v - mean)^2
    if (m2 < 0.0) m2 = 0.0;                                        // equal voxels: rounding only
    nm.mean = nm.any ? (float)(sm / c) : 0.f;
    nm.sd = (float)sqrt(m2 / (c - 1.0));                           // unbiased; NaN when c == 1
    nm.scale = nm.sd > 0.f;                                        // :532 (false for NaN)
    return nm;
}

// ------------------------------------------------------------------------------------------------ 3. bands in LDS
// what a band block does with its accumulated band: store it (and, with `acc`, leave its moments for vox_norm_kernel); leave the
// moments only; or read every block's moments and store the band normalised (after a VOX_BAND_MOMENTS launch)
enum { VOX_BAND_RAW = 0, VOX_BAND_MOMENTS = 1, VOX_BAND_NORMALISED = 2 };

#ifdef EEM_VOX_STAMPS
// stamps build only (EEM_EXTRA_FLAGS=-DEEM_VOX_STAMPS, tools/vox_stamps.py): s_memtime of wave 0 of the first 1024 band blocks at the phase
// boundaries: [0] start [1] band zeroed [2] table entries in [3] first records in [4] adds done, block through [5] read out [6] end
__device__ unsigned long long g_vox_stamps[1024 * 8];
#define VSTAMP(i) { __builtin_amdgcn_sched_barrier(0); vst[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#else
#define VSTAMP(i)
#endif

template <int BT>
__global__ __launch_bounds__(BT, BT / 128) void vox_band_kernel(VoxJobs jobs, int slab, int bins, VoxPlan pl, int vec4, int with_moments, int mode, int sgs) {
    const VoxJob& J = jobs.j[blockIdx.y];
    const unsigned* __restrict__ recs = J.recs;
    const unsigned* __restrict__ run_start = J.run_start;
    const int nblk = J.nblk;
    float* __restrict__ grid = J.grid;
    VoxSums* __restrict__ acc = with_moments ? J.acc : nullptr;
    // [bins][band_px] fp64 cells: the LDS fp32 add runs at a third of a lane per clock and CU on this chip, the fp64 add 8 - 20 times faster
    // (profiles/r04_lds_atomics.txt); the sum of a cell's votes is rounded to fp32 once, when the band leaves
    extern __shared__ __attribute__((aligned(16))) double band[];
    __shared__ double sh3[BT / 64 * 3];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int bpx = pl.band_px;
    const unsigned p0 = (unsigned)b * (unsigned)bpx;
    const int npx = min(bpx, (int)(pl.hw - p0));
    const int nfl = bins * bpx;
#ifdef EEM_VOX_STAMPS
    unsigned long long vst[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    VSTAMP(0)
    // A run = this band's votes of one binning block: `len` consecutive 12-byte records.  2^sgs adjacent lanes share a run (sized so
    // that nearly every run is one record per lane): a wave's load then touches a few runs' lines instead of 64 unrelated ones - with a
    // thread per run (and, before, a thread per vote with a binary search for its run) the address unit's one line per clock was the
    // kernel: 24 of 35 us.  Eight runs per thread are in flight: all their table entries, then all their first records, then the adds.
    constexpr int NP = 8;
    typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
    const int sub = tid & ((1 << sgs) - 1);
    const int rpp = BT >> sgs;                                     // runs per pass of the block
    // both streams as buffer loads with 32-bit offsets (a run past the last binning block and a lane past its run's end read zeros:
    // no branches around the loads, all of a phase in flight together)
    const __amdgpu_buffer_rsrc_t trs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(run_start), (short)0, nblk * (pl.nb + 1) * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(recs), (short)0, (unsigned)nblk * (unsigned)slab * 12u, 0x00020000);
    constexpr int kOut = 0x7ffffff0;
    for (int g0 = 0; g0 < nblk; g0 += NP * rpp) {
        unsigned st[NP];
        int ln[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int sidx = g0 + q * rpp + (tid >> sgs);
            const int off = sidx < nblk ? (sidx * (pl.nb + 1) + b) * 4 : kOut;
            st[q] = __builtin_amdgcn_raw_buffer_load_b32(trs, off, 0, 0);
            ln[q] = (int)__builtin_amdgcn_raw_buffer_load_b32(trs, off, 4, 0);
        }
        if (g0 == 0) {
            // the band is zeroed UNDER the first table round trip (round 6; in-kernel stamps, tools/vox_stamps.py: zeroing + the block's
            // start-up skew 2 000 cycles, table entries 2 700, first records 1 600, adds 3 700, read-out 4 800 of a block's 14 800): an
            // LDS-only block wait - __syncthreads would drain the table loads first
            for (int i = tid * 2; i < nfl; i += BT * 2) *reinterpret_cast<f64x2*>(band + i) = f64x2{0.0, 0.0};
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            VSTAMP(1)
        }
        u32x3 r0[NP];
#ifdef EEM_VOX_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        VSTAMP(2)
#endif
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int sidx = g0 + q * rpp + (tid >> sgs);
            ln[q] -= (int)st[q];
            st[q] = ((unsigned)sidx * (unsigned)slab + st[q] + (unsigned)sub) * 12u;     // byte offset of this lane's first record
            r0[q] = __builtin_amdgcn_raw_buffer_load_b96(rrs, sub < ln[q] ? (int)st[q] : kOut, 0, 0);
        }
#ifdef EEM_VOX_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        VSTAMP(3)
#endif
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if (sub < ln[q]) {
                const int tl = (int)(r0[q][0] >> 16);
                double* cell = band + tl * bpx + (int)(r0[q][0] & 0xffffu);
                atomicAdd(cell, (double)__uint_as_float(r0[q][1]));
                if (tl + 1 < bins) atomicAdd(cell + bpx, (double)__uint_as_float(r0[q][2]));
            }
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) {                             // the rare longer runs
            for (int k = sub + (1 << sgs); k < ln[q]; k += 1 << sgs) {
                const u32x3 r = __builtin_amdgcn_raw_buffer_load_b96(rrs, (int)(st[q] + (unsigned)(k - sub) * 12u), 0, 0);
                const int tl = (int)(r[0] >> 16);
                double* cell = band + tl * bpx + (int)(r[0] & 0xffffu);
                atomicAdd(cell, (double)__uint_as_float(r[1]));
                if (tl + 1 < bins) atomicAdd(cell + bpx, (double)__uint_as_float(r[2]));
            }
        }
    }
    __syncthreads();
    VSTAMP(4)
    float mean = 0.f, sd = 1.f;
    bool scale = false, shift = false;
    if (mode == VOX_BAND_NORMALISED) {
        const VoxNorm nm = vox_final<BT>(acc, pl.nb, sh3);
        mean = nm.mean; sd = nm.sd; scale = nm.scale; shift = nm.any;
    }
    auto fin = [&](float v) { return (shift && v != 0.f) ? (scale ? (v - mean) / sd : (v - mean)) : v; };
    // one pass over the band: every cell is rounded to fp32 once, counted into the moments and stored
    const bool want_sums = acc && mode != VOX_BAND_NORMALISED;
    const bool store = mode != VOX_BAND_MOMENTS;
    // a thread's share of the band's moments (at most a few dozen cells) in fp32 and an integer count, widened once below: zeros add
    // nothing, so no branch - the fp64 form (compare, branch, convert, two adds and an fma per cell, 9 216 cells per band) made the
    // read-out the longest phase of a band block (stamps: 4 800 of 14 800 cycles, vector-pipe bound: fp64 runs at half rate)
    int cnz = 0;
    float sm32 = 0.f, sq32 = 0.f;
    auto note = [&](float v) { cnz += v != 0.f ? 1 : 0; sm32 += v; sq32 = __builtin_fmaf(v, v, sq32); };
    for (int bin = 0; bin < bins; ++bin) {
        const double* src = band + bin * bpx;
        float* dst = grid + (size_t)bin * pl.hw + p0;
        if (vec4) {
            for (int i = tid * 4; i < npx; i += BT * 4) {
                const f64x2 lo = *reinterpret_cast<const f64x2*>(src + i), hi = *reinterpret_cast<const f64x2*>(src + i + 2);
                f32x4 v = {(float)lo[0], (float)lo[1], (float)hi[0], (float)hi[1]};
#pragma unroll
                for (int q = 0; q < 4; ++q) { note(v[q]); v[q] = fin(v[q]); }
                if (store) *reinterpret_cast<f32x4*>(dst + i) = v;
            }
        } else {
            for (int i = tid; i < npx; i += BT) {
                const float v = (float)src[i];
                note(v);
                if (store) dst[i] = fin(v);
            }
        }
    }
    VSTAMP(5)
    if (want_sums) vox_store_sums((double)cnz, (double)sm32, (double)sq32, acc + b, sh3);
#ifdef EEM_VOX_STAMPS
    VSTAMP(6)
    if (tid == 0 && blockIdx.y == 0 && blockIdx.x < 1024)
        for (int i = 0; i < 8; ++i) g_vox_stamps[blockIdx.x * 8 + i] = vst[i];
#endif
}

// ------------------------------------------------------------------------------------------------ 4. normalisation
__global__ __launch_bounds__(VT) void vox_norm_kernel(VoxJobs jobs, long total, int nsums) {
    float* __restrict__ grid = jobs.j[blockIdx.y].grid;
    const VoxSums* __restrict__ acc = jobs.j[blockIdx.y].acc;
    __shared__ double sh3[VT / 64 * 3];
    const int tid = threadIdx.x;
    // the first NPRE 16-byte pieces of this thread are requested before the sums are known (5 cover 1280x720x5 and
    // 640x480x15 entirely with 256 blocks)
    constexpr int NPRE = 5;
    const bool vec = (total & 3) == 0 && ((uintptr_t)grid & 15) == 0;
    f32x4* g4 = reinterpret_cast<f32x4*>(grid);
    const long n4 = total / 4, stride = (long)gridDim.x * VT, first = (long)blockIdx.x * VT + tid;
    f32x4 pre[NPRE];
    if (vec) {
#pragma unroll
        for (int k = 0; k < NPRE; ++k)
            if (first + k * stride < n4) pre[k] = g4[first + k * stride];
    }
    const VoxNorm nm = vox_final(acc, nsums, sh3);
    if (!nm.any) return;                                           // :529
    const float mean = nm.mean, sd = nm.sd;
    const bool scale = nm.scale;
    if (vec) {
        auto apply = [&](f32x4 v, long i) {
            bool any = false;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (v[q] != 0.f) { v[q] = scale ? (v[q] - mean) / sd : (v[q] - mean); any = true; }
            if (any) g4[i] = v;
        };
#pragma unroll
        for (int k = 0; k < NPRE; ++k)
            if (first + k * stride < n4) apply(pre[k], first + k * stride);
        for (long i = first + NPRE * stride; i < n4; i += stride) apply(g4[i], i);
    } else {
        for (long i = (long)blockIdx.x * VT + tid; i < total; i += (long)gridDim.x * VT) {
            const float v = grid[i];
            if (v != 0.f) grid[i] = scale ? (v - mean) / sd : (v - mean);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 4b. normalisation left to the consumer
// normalize == 2 ("deferred"): the grid stays RAW and the four floats behind it - grid[total .. total + 4) - receive the record
// {mean, sd, scale ? 1 : 0, any ? 1 : 0} of loader_utils.py:527-535; the first encoder layer applies (v - mean) / sd to the non-zero voxels
// as it reads them (conv_enc1.hip), so the 2 x 18.4 MB read-modify-write of vox_norm_kernel never happens.  One block per job.
__global__ __launch_bounds__(VT) void vox_stats_kernel(VoxJobs jobs, long total, int nsums) {
    __shared__ double sh3[VT / 64 * 3];
    const VoxNorm nm = vox_final(jobs.j[blockIdx.x].acc, nsums, sh3);
    if (threadIdx.x == 0) {
        float* rec = jobs.j[blockIdx.x].grid + total;
        rec[0] = nm.mean; rec[1] = nm.scale ? nm.sd : 1.f; rec[2] = nm.scale ? 1.f : 0.f; rec[3] = nm.any ? 1.f : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ direct path: moments
__global__ __launch_bounds__(VT) void vox_moments_kernel(const float* __restrict__ grid, long total, VoxSums* __restrict__ acc) {
    __shared__ double sh3[VT / 64 * 3];
    double c = 0.0, sm = 0.0, q = 0.0;
    for (long i = (long)blockIdx.x * VT + threadIdx.x; i < total; i += (long)gridDim.x * VT) {
        const float v = grid[i];
        if (v != 0.f) { c += 1.0; sm += (double)v; q += (double)v * (double)v; }
    }
    vox_store_sums(c, sm, q, acc + blockIdx.x, sh3);
}

struct VoxScratch {
    VoxSums acc[VT];
};

// blocks of the binning kernel for n events at EPT events per thread; the run table has (nb + 1) <= 1024 words per block
inline long vox_blocks(long n, int ept) { return (n + (long)VT * ept - 1) / ((long)VT * ept); }
inline int vox_ept(long n) {
    int ept = 1;
    while (ept < 8 && vox_blocks(n, ept) > 512) ept *= 2;
    return ept;
}
constexpr long VOX_MAX_BLOCKS = 4096;                              // 33.5 M events at 8 per thread; beyond: direct kernel

// (events: voxel.hip's table, read as 16-byte pieces; voxel_tri.hip reads columns and passes NULL)
bool make_plan(int64_t n, int bins, int h, int w, const void* events, VoxPlan* pl, int* lds_bytes) {
    const long hw = (long)h * w;
    if (bins > 64 || vox_blocks(n, 8) > VOX_MAX_BLOCKS || hw >= (1L << 31) || ((uintptr_t)events & 15)) return false;
    if (sw_on<SW_EEM_VOX_DIRECT>()) return false;
    // 9216 fp64 cells (72 KB) per band by default -> vox_band_kernel<1024>, two blocks per CU; EEM_VOX_BAND_FLOATS=<cells> picks another
    // band size (<= 3072 cells: 256-thread blocks, <= 5120: 512) - 2304 .. 18432 cells measure the same within 3 % at 2e5 and 2e6 events
    const long band_env = sw_long_once<SW_EEM_VOX_BAND_FLOATS>();
    const long band_floats = band_env >= 256 ? band_env : 9216L;
    long band_px = (band_floats / bins) & ~3L;
    if (band_px < 64) band_px = 64;
    const long spread = ((hw + 511) / 512 + 3) & ~3L;              // small images: still a few hundred bands
    if (band_px > spread) band_px = spread < 64 ? 64 : spread;
    if ((hw + band_px - 1) / band_px > VT - 1) band_px = ((hw + VT - 2) / (VT - 1) + 3) & ~3L;   // thread nb holds the record count
    if (band_px * bins > 19200 || band_px > 65535) return false;   // 150 KiB of LDS (fp64 cells) beside the static tables, 16-bit pixel-in-band
    pl->band_px = (int)band_px;
    pl->nb = (int)((hw + band_px - 1) / band_px);
    pl->hw = (unsigned)hw;
    *lds_bytes = (int)(band_px * bins * 8);
    return true;
}

// ------------------------------------------------------------------------------------------------ host: the launches after the binning
// lanes per run of the band kernel: the smallest power of two >= 4.0 for sparse sets, else 1.7 (the rule through round 5), x the mean run
// length (slab records / bands), 4 .. 64: a run longer than its lanes costs its block a dependent round trip in the clean-up loop, and
// with 196 runs of mean length 2 per band and four lanes each nearly every block had one (stamps: 3 700 cycles in the adds)
// (sparse sets only - mean run below 4 records: at 2e6 events per grid the wider runs idle more lanes than they save, 53.0 against
// 50.6 us per sample)
inline int vox_sgs(long slab, int nb) {
    const long lanes_x10 = slab < 4L * nb ? 40L : 17L;
    int sgs = 2;
    while (sgs < 6 && (1 << sgs) * 10L * nb < lanes_x10 * slab) ++sgs;
    return sgs;
}

// 16-byte read-out of the bands: whole pieces in every band and plane, every grid aligned
inline int vox_vec4(const VoxPlan& pl, int njobs, float* const* grid) {
    bool aligned = true;
    for (int k = 0; k < njobs; ++k) aligned = aligned && ((uintptr_t)grid[k] & 15) == 0;
    return (pl.band_px % 4 == 0 && pl.hw % 4 == 0 && aligned) ? 1 : 0;
}

// one launch of the band kernel over every band of every job (slab: records per binning block); *bt receives its threads per block
inline int vox_launch_band(const VoxJobs& jobs, int njobs, int slab, int bins, const VoxPlan& pl, int lds, int vec4, int with_moments, int mode,
                           int sgs, int* bt, hipStream_t stream) {
    if (lds > 64 * 1024 - 12 * 1024) EEM_RAISE_LDS(lds, vox_band_kernel<VT>);
    if (lds <= 24 * 1024) {
        *bt = 256;
        hipLaunchKernelGGL(vox_band_kernel<256>, dim3(pl.nb, njobs), dim3(256), lds, stream, jobs, slab, bins, pl, vec4, with_moments, mode, sgs);
    } else if (lds <= 40 * 1024) {
        *bt = 512;
        hipLaunchKernelGGL(vox_band_kernel<512>, dim3(pl.nb, njobs), dim3(512), lds, stream, jobs, slab, bins, pl, vec4, with_moments, mode, sgs);
    } else {
        *bt = VT;
        hipLaunchKernelGGL(vox_band_kernel<VT>, dim3(pl.nb, njobs), dim3(VT), lds, stream, jobs, slab, bins, pl, vec4, with_moments, mode, sgs);
    }
    return EEM_OK;
}

// vox_norm_kernel over the grids of every job, from `nsums` moment slots each
inline int vox_launch_norm(const VoxJobs& jobs, int njobs, long total, int nsums, hipStream_t stream) {
    long blocks = (total / 4 + VT - 1) / VT;
    blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);   // one block per CU: the sums are re-added once per block
    if (njobs >= 2 && blocks > 256 / njobs) blocks = std::max(16L, 256L / njobs);     // the jobs share the chip
    hipLaunchKernelGGL(vox_norm_kernel, dim3((unsigned)blocks, njobs), dim3(VT), 0, stream, jobs, total, nsums);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}

// what a launch sequence ran (eemflow_voxelize_last_form): small integers stored on the host beside the launches
struct VoxForm {
    int njobs;               // 0: no sequence yet
    int ept;                 // binning kernel's events per thread; 0: the direct kernel
    int bt, vec4, sgs;       // band kernel: threads per block, 16-byte read-out, log2 of the lanes per run
    int moments;             // the raw band launch left its moments / vox_moments_kernel followed the direct kernel
    int after;               // 0 nothing, 1 vox_norm_kernel, 2 vox_stats_kernel, 3 the two band passes
};

// the report of a form; bin: the binning kernel's name in it ("bin": vox_bin_kernel, "colbin": vox_bin_cols_kernel)
inline void vox_form_text(const VoxForm& f, const char* bin, char* buf, size_t cap) {
    static const char* const kAfter[4] = {"", "+norm", "+stats", ""};
    if (f.njobs == 0) {
        buf[0] = 0;
    } else if (f.ept == 0) {
        snprintf(buf, cap, "j%d:direct%s%s", f.njobs, f.moments ? "+moments" : "", kAfter[f.after]);
    } else {
        char band[48];
        snprintf(band, sizeof(band), "band%d_%s_s%d", f.bt, f.vec4 ? "v4" : "v1", f.sgs);
        if (f.after == 3)
            snprintf(buf, cap, "j%d:%s_e%d+%s_moments+%s_normalised", f.njobs, bin, f.ept, band, band);
        else
            snprintf(buf, cap, "j%d:%s_e%d+%s_%s%s", f.njobs, bin, f.ept, band, f.moments ? "raw_sums" : "raw", kAfter[f.after]);
    }
}

// The launches behind a binning kernel that has left the slabs and run tables of `jobs` (ept events per thread, the longest set nmax
// events): the band kernel and, by `normalize`, vox_norm_kernel or vox_stats_kernel - or the two band passes of EEM_VOX_TWOPASS.  Fills
// in what *vf reports of them.
inline int vox_launch_after_bin(const VoxJobs& jobs, int njobs, int ept, long nmax, int bins, long total, int normalize, const VoxPlan& pl,
                                int lds, float* const* grid, VoxForm* vf, hipStream_t stream) {
    int rc;
    const int vec4 = vox_vec4(pl, njobs, grid);
    // Few events per voxel: accumulating the bands twice (16 B per vote from L2 / HBM each time) is cheaper than the normalisation's
    // read + write of the whole grid - a moments-only launch, then a launch that stores the bands already normalised
    const long two_pass_ratio = sw_long<SW_EEM_VOX_TWOPASS>();   // (the tests run both forms in one process)
    const int sgs = vox_sgs((long)VT * ept, pl.nb);
    vf->ept = ept; vf->vec4 = vec4; vf->sgs = sgs;
    auto band = [&](int with_moments, int mode) {
        return vox_launch_band(jobs, njobs, VT * ept, bins, pl, lds, vec4, with_moments, mode, sgs, &vf->bt, stream);
    };
    if (normalize == 1 && two_pass_ratio > 0 && nmax * two_pass_ratio <= total) {
        if ((rc = band(1, (int)VOX_BAND_MOMENTS)) != EEM_OK || (rc = band(1, (int)VOX_BAND_NORMALISED)) != EEM_OK) return rc;
        EEM_HIP_CHECK(hipGetLastError());
        vf->after = 3;
        return EEM_OK;
    }
    if ((rc = band(normalize ? 1 : 0, (int)VOX_BAND_RAW)) != EEM_OK) return rc;
    EEM_HIP_CHECK(hipGetLastError());
    if (normalize == 2) {                                              // deferred: the record behind each grid, no pass over the grids
        hipLaunchKernelGGL(vox_stats_kernel, dim3(njobs), dim3(VT), 0, stream, jobs, total, pl.nb);
        EEM_HIP_CHECK(hipGetLastError());
    } else if (normalize) {
        if ((rc = vox_launch_norm(jobs, njobs, total, pl.nb, stream)) != EEM_OK) return rc;
    }
    return EEM_OK;
}

}  // namespace
