// Event preparation on the device: the four columns of an events npz (t, x, y, p in their file dtypes) -> the (N,4) float64 table
// [t, x, y, p] that the voxelizer, the IWE kernels and `with_events` consume.  Replaces the host's NumPy passes of
// loader/loader_utils.py:26-37 (get_compressed_events: the float64 table, t * 1e-9) and EventSequence.__init__, :352-397 (the
// timestamp multiplier and absolute_time_to_relative) for event sets whose raw timestamps are already in order - the host decides
// that (eemflow_amd/events.py) and keeps its own route, argsort included, for the others.
//
// Arithmetic, bit for bit what NumPy does (this file is built with -ffp-contract=off: a fused or re-associated product gives other
// last bits):
//   every column value -> double as astype(float64) converts it: exact for u8 .. i32, f32 and f64; int64 rounds to nearest even,
//                         which is what (double) of an int64_t gives
//   tt      = ((double)t * scale_a) * scale_b        two separately rounded products (HREM: 1e-9, then 1e6); x 1.0 is the identity
//   out[i]  = {relative ? tt[i] - tt[0] : tt[i], x, y, p}
// p arrives already as 2*p - 1: the host forms it in the column's own dtype (N one-byte operations), which keeps NumPy's uint8
// 0 -> 255 and bool -> int64.
//
// A byte mover: 13 B in and 32 B out per HREM event, no LDS, no atomics.  Up to EEMFLOW_PACK_MAX event sets share the launch: the job
// table travels as kernel arguments (64 bytes per job), blockIdx.y = job, blockIdx.x walks the job's events with a grid stride, the
// whole grid held near 2048 blocks.  A thread makes PK_EPT events per step, event (step * PK_EPT + k) * PK_THREADS + tid: the lanes of
// a wave read consecutive elements of each column and write consecutive 32-byte rows, each row as two 16-byte stores; every event
// is bounds-checked on its own, so any N works.  tt[0] is one load of t[0] per thread, the same address in every lane.
#include "common.h"

#include <cstdint>
#include <cstring>

#include "event_cols.h"   // pk_load, pk_elem_bytes

namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_EPT = 4;
constexpr int PK_GRID = 2048;                // blocks of a launch, about: 8 per CU

struct PackJob {
    const void* col[4];                      // t, x, y, p
    double* out;                             // [n][4]
    long n;
    int code[4];
};
struct PackJobs { PackJob j[EEMFLOW_PACK_MAX]; };        // 64 bytes each: 2 KB of kernel arguments at 32 jobs

__global__ __launch_bounds__(PK_THREADS) void event_pack_kernel(PackJobs jobs, double scale_a, double scale_b, int relative) {
    const PackJob& J = jobs.j[blockIdx.y];
    const long n = J.n;
    if ((long)blockIdx.x * (PK_THREADS * PK_EPT) >= n) return;     // a shorter (or empty) set of the call
    const int ct = J.code[0], cx = J.code[1], cy = J.code[2], cp = J.code[3];
    const void* __restrict__ pt = J.col[0];
    const void* __restrict__ px = J.col[1];
    const void* __restrict__ py = J.col[2];
    const void* __restrict__ pp = J.col[3];
    f64x2* __restrict__ out = reinterpret_cast<f64x2*>(J.out);
    const double t0 = relative ? (pk_load(pt, ct, 0) * scale_a) * scale_b : 0.0;
    const long step = (long)gridDim.x * (PK_THREADS * PK_EPT);
    for (long base = (long)blockIdx.x * (PK_THREADS * PK_EPT); base < n; base += step) {
        double t[PK_EPT], x[PK_EPT], y[PK_EPT], p[PK_EPT];
#pragma unroll
        for (int k = 0; k < PK_EPT; ++k) {
            const long i = base + k * PK_THREADS + threadIdx.x;
            if (i < n) {
                t[k] = pk_load(pt, ct, i);
                x[k] = pk_load(px, cx, i);
                y[k] = pk_load(py, cy, i);
                p[k] = pk_load(pp, cp, i);
            }
        }
#pragma unroll
        for (int k = 0; k < PK_EPT; ++k) {
            const long i = base + k * PK_THREADS + threadIdx.x;
            if (i < n) {
                double tt = (t[k] * scale_a) * scale_b;
                if (relative) tt = tt - t0;
                out[i * 2] = f64x2{tt, x[k]};
                out[i * 2 + 1] = f64x2{y[k], p[k]};
            }
        }
    }
}

}  // namespace

extern "C" int eemflow_pack_events_many(int nsets, const void* const* t, const void* const* x, const void* const* y, const void* const* p,
                                        const int* codes, const int64_t* n_events, double scale_a, double scale_b, int relative,
                                        double* const* out, void* stream) {
    EEM_REQUIRE(nsets >= 1 && nsets <= EEMFLOW_PACK_MAX, "eemflow_pack_events_many: 1..%d event sets per call; got %d", EEMFLOW_PACK_MAX, nsets);
    EEM_REQUIRE(t && x && y && p && codes && n_events && out, "eemflow_pack_events_many: NULL argument");
    PackJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int64_t nmax = 0;
    for (int k = 0; k < nsets; ++k) {
        PackJob& J = jobs.j[k];
        EEM_REQUIRE(n_events[k] >= 0, "eemflow_pack_events_many: set %d has n = %ld", k, (long)n_events[k]);
        const void* col[4] = {t[k], x[k], y[k], p[k]};
        for (int c = 0; c < 4; ++c) {
            const int code = codes[k * 4 + c];
            const int eb = pk_elem_bytes(code);
            EEM_REQUIRE(eb != 0, "eemflow_pack_events_many: set %d, column %d: unknown dtype code %d", k, c, code);
            if (n_events[k] == 0) continue;
            EEM_REQUIRE(col[c] != nullptr, "eemflow_pack_events_many: set %d, column %d is NULL", k, c);
            EEM_REQUIRE((reinterpret_cast<uintptr_t>(col[c]) & (uintptr_t)(eb - 1)) == 0,
                        "eemflow_pack_events_many: set %d, column %d is not aligned to its %d-byte elements", k, c, eb);
            J.col[c] = col[c];
            J.code[c] = code;
        }
        if (n_events[k] == 0) continue;                               // writes nothing: its blocks leave at once
        EEM_REQUIRE(out[k] != nullptr && (reinterpret_cast<uintptr_t>(out[k]) & 15) == 0,
                    "eemflow_pack_events_many: set %d: the output must be a 16-byte aligned device buffer", k);
        J.out = out[k];
        J.n = (long)n_events[k];
        nmax = n_events[k] > nmax ? n_events[k] : nmax;
    }
    if (nmax == 0) return EEM_OK;
    const long per_block = (long)PK_THREADS * PK_EPT;
    long blocks = (long)((nmax + per_block - 1) / per_block);
    const long cap = PK_GRID / nsets > 1 ? PK_GRID / nsets : 1;         // the jobs share the chip; the rest is the grid stride
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(event_pack_kernel, dim3((unsigned)blocks, (unsigned)nsets), dim3(PK_THREADS), 0, (hipStream_t)stream, jobs, scale_a,
                       scale_b, relative ? 1 : 0);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}
