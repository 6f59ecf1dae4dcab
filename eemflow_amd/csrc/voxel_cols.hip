// The windows of one device-resident recording, voxelized straight from its raw columns (eemflow_voxelize_windows, and by span
// - overlapping, nested, repeated windows in any order - eemflow_voxelize_spans; one body, cols_voxelize): voxel.hip's two
// temporal votes per event, without the float64 table in between.  Cutting a recording into windows through the table costs, per
// event, 13 B read + 32 B written by event_pack_kernel and 32 B read again by vox_bin_kernel; here the binning kernel reads the 13 B
// (t int64, x and y uint16, p one byte in an HREM-style npz) and does event_pack_kernel's arithmetic in registers:
//   1. vox_bin_cols_kernel  a sibling of vox_bin_kernel: lane i of a block loads element first + i of each column in the column's
//                           own dtype (pk_load of event_cols.h: element-wise loads, so a window may start at any element; HREM's own
//                           dtypes have an instantiation without the dtype switch, the same conversions), forms
//                           tt = ((double)t * scale_a) * scale_b - two separately rounded products - and, with `relative`, subtracts
//                           the window's own tt[first]; then vox_vote / vox_record / vox_slab_out of vox_shared.h, which are
//                           vox_bin_kernel's: the same 12-byte records and run table;
//   2. everything behind it is voxel.hip's, unchanged (vox_launch_after_bin: the band kernel, the moments, vox_norm_kernel /
//      vox_stats_kernel, EEM_VOX_TWOPASS).
// So a window's grid is bitwise what eemflow_voxelize_many gives for the table eemflow_pack_events_many makes of the window's slice (this
// file is built with -ffp-contract=off, as both of those are).
// The windows of a call share the recording: the four base pointers, their dtype codes and the scales travel once, each job's first
// element beside the VoxJobs (2.3 KB + 256 B + 72 B of kernel arguments at 32 jobs).
// An EMPTY window (the reference cannot be asked: it indexes events[-1]) gets one binning block that finds no event and writes a run
// table row of zeros: the band kernel then stores an all-zero grid and zero moments, and vox_stats_kernel's record is {0, 1, 0, 0}.
// Grids the LDS band layout cannot take (make_plan false, EEM_VOX_DIRECT) run as eemflow_pack_events_many into a scratch table plus
// voxel.hip's direct kernel, window by window.
#include "vox_shared.h"

#include "event_cols.h"

namespace {

struct ColsRecording {
    const void* col[4];      // t, x, y, p: the recording's base columns
    int code[4];             // EEMFLOW_PACK_*
    double scale_a, scale_b;
    int relative;
    int pad;
};
struct ColsFirst { long long first[VOX_MAX_JOBS]; };               // the first element of each job's window

// One event's four column values as doubles.  HREM: the columns are the npz layout of HREM (t int64, x and y uint16, p one byte, signed
// or not) - the dtype switch of pk_load is gone at compile time, so a thread's loads are all in flight together; behind the switch
// every branch waits for its own load (what DESIGN.md section 7 suspects of event_pack_kernel).  The conversions are pk_load's.
template <bool HREM>
__device__ __forceinline__ void cols_load(const ColsRecording& rec, long i, double* t, double* x, double* y, double* p) {
    if constexpr (HREM) {
        const long long tv = static_cast<const long long*>(rec.col[0])[i];
        const uint16_t xv = static_cast<const uint16_t*>(rec.col[1])[i];
        const uint16_t yv = static_cast<const uint16_t*>(rec.col[2])[i];
        const uint8_t pv = static_cast<const uint8_t*>(rec.col[3])[i];
        *t = (double)tv;                                           // round to nearest even
        *x = (double)xv;
        *y = (double)yv;
        *p = rec.code[3] == EEMFLOW_PACK_I8 ? (double)(int8_t)pv : (double)pv;
    } else {
        *t = pk_load(rec.col[0], rec.code[0], i);
        *x = pk_load(rec.col[1], rec.code[1], i);
        *y = pk_load(rec.col[2], rec.code[2], i);
        *p = pk_load(rec.col[3], rec.code[3], i);
    }
}

template <bool HREM>
__device__ __forceinline__ double cols_load_t(const ColsRecording& rec, long i) {
    if constexpr (HREM) return (double)static_cast<const long long*>(rec.col[0])[i];
    else return pk_load(rec.col[0], rec.code[0], i);
}

// ------------------------------------------------------------------------------------------------ 1. binning into slabs
template <int EPT, bool HREM>
__global__ __launch_bounds__(VT) void vox_bin_cols_kernel(VoxJobs jobs, ColsFirst firsts, ColsRecording rec, int bins, int h, int w, VoxPlan pl) {
    const VoxJob& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.nblk) return;                         // a shorter window
    const long n = J.n;
    const long first = (long)firsts.first[blockIdx.y];
    __shared__ unsigned hist[VT];
    __shared__ unsigned lpos[VT];
    __shared__ unsigned sh[VT / 64];
    extern __shared__ __attribute__((aligned(16))) unsigned stage[];   // the slab as it goes to memory: 3 words per record
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    const double scale_a = rec.scale_a, scale_b = rec.scale_b;
    const bool relative = rec.relative != 0;
    // the window's time scale, from the table rows event_pack_kernel would write for its first and last event (vox_time of voxel.hip
    // on them): two loads of the same address in every lane.  An empty window (n == 0) loads nothing
    VoxTime tm = {0.0, 1.0};
    double tfirst = 0.0;
    if (n > 0) {
        double ta = (cols_load_t<HREM>(rec, first) * scale_a) * scale_b;
        double tb = (cols_load_t<HREM>(rec, first + n - 1) * scale_a) * scale_b;
        if (relative) { tfirst = ta; ta = ta - tfirst; tb = tb - tfirst; }
        tm.t0 = ta;
        tm.dT = tb - tm.t0;
        if (tm.dT == 0.0) tm.dT = 1.0;                             // loader_utils.py:485-486
    }
    unsigned key[EPT], band[EPT], rank[EPT];
    float vl[EPT], vr[EPT];
    double t[EPT], x[EPT], y[EPT], p[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {                                    // all of the thread's loads first (event_pack_kernel's order)
        const long i = ((long)blockIdx.x * EPT + k) * VT + tid;
        if (i < n) cols_load<HREM>(rec, first + i, &t[k], &x[k], &y[k], &p[k]);
    }
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const long i = ((long)blockIdx.x * EPT + k) * VT + tid;
        band[k] = 0xffffffffu;
        if (i < n) {
            double tt = (t[k] * scale_a) * scale_b;
            if (relative) tt = tt - tfirst;
            const VoxVote v = vox_vote(tt, x[k], y[k], p[k], tm, bins, h, w);
            unsigned bd;
            if (vox_record(v, bins, pl, &bd, &key[k], &vl[k], &vr[k])) {
                band[k] = bd;
                rank[k] = atomicAdd(&hist[bd], 1u);                // LDS: the returned count is the rank inside the run
            }
        }
    }
    vox_slab_out<EPT>(key, band, rank, vl, vr, hist, lpos, sh, stage, J.run_start, J.recs, pl);
}

template <int EPT, bool HREM>
int launch_bin_cols_as(const VoxJobs& jobs, const ColsFirst& firsts, const ColsRecording& rec, int njobs, long nblk_max, int bins, int h, int w,
                       const VoxPlan& pl, hipStream_t stream) {
    constexpr int stage_bytes = VT * EPT * 12;
    if (stage_bytes > 48 * 1024) EEM_RAISE_LDS(stage_bytes, vox_bin_cols_kernel<EPT, HREM>);
    hipLaunchKernelGGL((vox_bin_cols_kernel<EPT, HREM>), dim3((unsigned)nblk_max, njobs), dim3(VT), stage_bytes, stream, jobs, firsts, rec, bins, h,
                       w, pl);
    return EEM_OK;
}

template <int EPT>
int launch_bin_cols(const VoxJobs& jobs, const ColsFirst& firsts, const ColsRecording& rec, int njobs, long nblk_max, int bins, int h, int w,
                    const VoxPlan& pl, hipStream_t stream) {
    const bool hrem = rec.code[0] == EEMFLOW_PACK_I64 && rec.code[1] == EEMFLOW_PACK_U16 && rec.code[2] == EEMFLOW_PACK_U16 &&
                      (rec.code[3] == EEMFLOW_PACK_U8 || rec.code[3] == EEMFLOW_PACK_I8);
    return hrem ? launch_bin_cols_as<EPT, true>(jobs, firsts, rec, njobs, nblk_max, bins, h, w, pl, stream)
                : launch_bin_cols_as<EPT, false>(jobs, firsts, rec, njobs, nblk_max, bins, h, w, pl, stream);
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the banded form: the launch sequence of voxel.hip's planned path with the other first kernel
int cols_launch_banded(const char* who, int nwin, const ColsRecording& rec, const int64_t* starts, const int64_t* ends, int bins, int h, int w, int normalize, float* const* grid,
                       void* const* scratch, const VoxPlan& pl, int lds, hipStream_t stream) {
    VoxJobs jobs;
    ColsFirst firsts;
    memset(&jobs, 0, sizeof(jobs));
    memset(&firsts, 0, sizeof(firsts));
    int64_t nmax = 0;
    for (int k = 0; k < nwin; ++k) nmax = std::max(nmax, ends[k] - starts[k]);
    const int ept = vox_ept((long)nmax);                               // one EPT for all windows (the longest one's)
    long nblk_max = 0;
    for (int k = 0; k < nwin; ++k) {
        const long n = (long)(ends[k] - starts[k]);
        VoxScratch* sc = (VoxScratch*)scratch[k];
        const long slots = (n + 8191) / 8192 * 8192 + 8192;            // (voxel_scratch_bytes)
        VoxJob& J = jobs.j[k];
        J.n = n;
        J.recs = reinterpret_cast<unsigned*>(sc + 1);
        J.run_start = J.recs + slots * 3;
        J.grid = grid[k]; J.acc = sc->acc;
        J.nblk = (int)std::max(1L, vox_blocks(n, ept));                // an empty window: one block, a run table row of zeros
        EEM_REQUIRE((long)J.nblk * VT * ept <= slots, "%s: slab budget (n=%ld, ept=%d)", who, n, ept);
        firsts.first[k] = (long long)starts[k];
        nblk_max = std::max(nblk_max, (long)J.nblk);
    }
    int rc;
    switch (ept) {
        case 1: rc = launch_bin_cols<1>(jobs, firsts, rec, nwin, nblk_max, bins, h, w, pl, stream); break;
        case 2: rc = launch_bin_cols<2>(jobs, firsts, rec, nwin, nblk_max, bins, h, w, pl, stream); break;
        case 4: rc = launch_bin_cols<4>(jobs, firsts, rec, nwin, nblk_max, bins, h, w, pl, stream); break;
        default: rc = launch_bin_cols<8>(jobs, firsts, rec, nwin, nblk_max, bins, h, w, pl, stream); break;
    }
    if (rc != EEM_OK) return rc;
    VoxForm vf = {nwin, 0, 0, 0, 0, normalize ? 1 : 0, normalize};
    if ((rc = vox_launch_after_bin(jobs, nwin, ept, (long)nmax, bins, (long)bins * h * w, normalize, pl, lds, grid, &vf, stream)) != EEM_OK) return rc;
    char form[128];
    vox_form_text(vf, "colbin", form, sizeof(form));
    voxel_note_form(form);
    return EEM_OK;
}

// the other grids: the windows' tables into scratch (behind each window's voxelizer scratch), then voxel.hip's direct kernel window by window
int cols_launch_direct(int nwin, const ColsRecording& rec, const int64_t* starts, const int64_t* ends, int bins, int h, int w, int normalize, float* const* grid,
                       void* const* scratch, hipStream_t stream) {
    const long total = (long)bins * h * w;
    const void* col[4][VOX_MAX_JOBS];
    int codes[4 * VOX_MAX_JOBS];
    int64_t n[VOX_MAX_JOBS];
    double* table[VOX_MAX_JOBS];
    for (int k = 0; k < nwin; ++k) {
        n[k] = ends[k] - starts[k];
        table[k] = reinterpret_cast<double*>((char*)scratch[k] + up256(voxel_scratch_bytes(n[k])));
        for (int c = 0; c < 4; ++c) {
            col[c][k] = (const char*)rec.col[c] + (size_t)starts[k] * pk_elem_bytes(rec.code[c]);
            codes[4 * k + c] = rec.code[c];
        }
    }
    int nbanded = 0;
    int rc = eemflow_pack_events_many(nwin, col[0], col[1], col[2], col[3], codes, n, rec.scale_a, rec.scale_b, rec.relative, table, stream);
    if (rc != EEM_OK) return rc;
    for (int k = 0; k < nwin; ++k) {
        if (n[k] == 0) {                                               // an all-zero grid; deferred: the record of no voxels, {0, 1, 0, 0}
            EEM_HIP_CHECK(hipMemsetAsync(grid[k], 0, total * sizeof(float), stream));
            if (normalize == 2) {
                VoxJobs one;
                memset(&one, 0, sizeof(one));
                one.j[0].grid = grid[k]; one.j[0].acc = ((VoxScratch*)scratch[k])->acc;
                hipLaunchKernelGGL(vox_stats_kernel, dim3(1), dim3(VT), 0, stream, one, total, 0);
                EEM_HIP_CHECK(hipGetLastError());
            }
            continue;
        }
        const double* ev = table[k];
        int64_t* none = nullptr;
        VoxPlan own;
        int own_lds = 0;
        if (make_plan(n[k], bins, h, w, ev, &own, &own_lds)) ++nbanded;    // (voxel_launch_jobs plans this window for itself, the same way)
        if ((rc = voxel_launch_jobs(1, &ev, &n[k], bins, h, w, normalize, grid + k, &none, &none, scratch + k, stream)) != EEM_OK) return rc;
    }
    // the call came here because its LONGEST window is beyond the banded form (or the grid, or EEM_VOX_DIRECT: then every window is);
    // shorter windows of such a call still take the bands behind their tables, and the report says how many
    char form[128], mixed[32] = "";
    if (nbanded) snprintf(mixed, sizeof(mixed), "+bin(%d)", nbanded);
    snprintf(form, sizeof(form), "j%d:pack+direct%s%s", nwin, mixed, normalize == 2 ? "+moments+stats" : normalize ? "+moments+norm" : "");
    voxel_note_form(form);
    return EEM_OK;
}

// the body of both entry points: job k is the elements [starts[k], ends[k]) of the recording.  `who` names the entry point in the error
// messages; `offsets` (the consecutive form: starts = offsets, ends = offsets + 1) only words two of them
int cols_voxelize(const char* who, bool offsets, int nwin, const void* t, const void* x, const void* y, const void* p, const int codes[4],
                  const int64_t* starts, const int64_t* ends, double scale_a, double scale_b, int relative, int bins, int h, int w, int normalize,
                  float* const* grids, void* stream) {
    static Arena arena;                                                // its own pool of scratch arenas, handled as eemflow_voxelize_many's
    EEM_REQUIRE(nwin >= 1 && nwin <= VOX_MAX_JOBS, "%s: 1..%d windows per call; got %d", who, VOX_MAX_JOBS, nwin);
    EEM_REQUIRE(codes && starts && ends && grids, "%s: NULL argument", who);
    EEM_REQUIRE(bins > 0 && h > 0 && w > 0, "%s: bad shape bins=%d h=%d w=%d", who, bins, h, w);
    EEM_REQUIRE(normalize >= 0 && normalize <= 2, "%s: normalize is 0 (raw), 1 (normalised grid) or 2 (raw grid + record); got %d", who, normalize);
    if (offsets) EEM_REQUIRE(starts[0] >= 0, "%s: offsets[0] = %ld", who, (long)starts[0]);
    bool any_event = false;
    for (int k = 0; k < nwin; ++k) {
        if (offsets) {
            EEM_REQUIRE(ends[k] >= starts[k], "%s: the offsets must ascend (window %d: %ld .. %ld)", who, k, (long)starts[k], (long)ends[k]);
        } else {
            EEM_REQUIRE(starts[k] >= 0 && ends[k] >= starts[k], "%s: span %d is [%ld, %ld): 0 <= start <= end", who, k, (long)starts[k], (long)ends[k]);
        }
        EEM_REQUIRE(grids[k] != nullptr && ((uintptr_t)grids[k] & 3) == 0, "%s: window %d has no 4-byte aligned grid", who, k);
        any_event = any_event || ends[k] > starts[k];
    }
    ColsRecording rec;
    memset(&rec, 0, sizeof(rec));
    const void* col[4] = {t, x, y, p};
    for (int c = 0; c < 4; ++c) {
        const int eb = pk_elem_bytes(codes[c]);
        EEM_REQUIRE(eb != 0, "%s: column %d: unknown dtype code %d", who, c, codes[c]);
        EEM_REQUIRE(col[c] != nullptr || !any_event, "%s: column %d is NULL", who, c);
        EEM_REQUIRE((reinterpret_cast<uintptr_t>(col[c]) & (uintptr_t)(eb - 1)) == 0, "%s: column %d is not aligned to its %d-byte elements", who, c,
                    eb);
        rec.col[c] = col[c];
        rec.code[c] = codes[c];
    }
    rec.scale_a = scale_a; rec.scale_b = scale_b; rec.relative = relative ? 1 : 0;
    int64_t nmax = 0;
    for (int k = 0; k < nwin; ++k) nmax = std::max(nmax, ends[k] - starts[k]);
    VoxPlan pl;
    int lds = 0;
    const bool banded = make_plan(nmax, bins, h, w, nullptr, &pl, &lds);
    size_t part[VOX_MAX_JOBS] = {}, need = 0;
    for (int k = 0; k < nwin; ++k) {
        const int64_t n = ends[k] - starts[k];
        part[k] = up256(voxel_scratch_bytes(n)) + (banded ? 0 : up256((size_t)n * 32));
        need += part[k];
    }
    std::lock_guard<std::mutex> guard(arena.lock);
    char* base = nullptr;
    void* token = nullptr;
    int rc = arena.take(need, stream, &base, &token);
    if (rc != EEM_OK) return rc;
    void* scratch[VOX_MAX_JOBS];
    for (int k = 0; k < nwin; ++k) { scratch[k] = base; base += part[k]; }
    rc = banded ? cols_launch_banded(who, nwin, rec, starts, ends, bins, h, w, normalize, grids, scratch, pl, lds, (hipStream_t)stream)
                : cols_launch_direct(nwin, rec, starts, ends, bins, h, w, normalize, grids, scratch, (hipStream_t)stream);
    return rc == EEM_OK ? arena.done(token, stream) : rc;
}

}  // namespace

extern "C" int eemflow_voxelize_windows(int nwin, const void* t, const void* x, const void* y, const void* p, const int codes[4],
                                        const int64_t* offsets, double scale_a, double scale_b, int relative, int bins, int h, int w,
                                        int normalize, float* const* grids, void* stream) {
    // (the body refuses nwin outside 1..32 before it reads an element; offsets + 1 of a NULL offsets must stay NULL)
    return cols_voxelize("eemflow_voxelize_windows", true, nwin, t, x, y, p, codes, offsets, offsets ? offsets + 1 : nullptr, scale_a, scale_b,
                         relative, bins, h, w, normalize, grids, stream);
}

extern "C" int eemflow_voxelize_spans(int nwin, const void* t, const void* x, const void* y, const void* p, const int codes[4], const int64_t* starts,
                                      const int64_t* ends, double scale_a, double scale_b, int relative, int bins, int h, int w, int normalize,
                                      float* const* grids, void* stream) {
    return cols_voxelize("eemflow_voxelize_spans", false, nwin, t, x, y, p, codes, starts, ends, scale_a, scale_b, relative, bins, h, w, normalize,
                         grids, stream);
}
