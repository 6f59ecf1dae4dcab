// E-RAFT's warm start: forward interpolation of a low-resolution flow (utils/image_utils.py:11-84, forward_interpolate_pytorch via
// grid_sample_values), bit for bit.  Built with -ffp-contract=off (build.py): the reference rounds z * weight and every sum on its own.
//
// Per sample and channel z in {dx, dy}: source (x0, y0) lands at x1 = x0 + dx, y1 = y0 + dy; four passes in the reference's order -
// (floor x1, floor y1), (floor x1, ceil y1), (ceil x1, floor y1), (ceil x1, ceil y1) - each add z * w and w, w = (1 - |x1 - xv|) *
// (1 - |y1 - yv|), to the in-grid cell (xv, yv); out = sum(z * w) / (sum(w) + 1e-15f).  The reference's put_(accumulate=True) adds
// in (pass, source index) order, so every cell here does too, sequentially in fp32.
//
// One workgroup per sample.  A stable counting sort buckets the sources by their floor cell on the grid [-1, w) x [-1, h) (a cell
// takes contributions only from its own floor cell and its left / upper / upper-left neighbours): integer counts, an exclusive scan,
// placement, then each bucket ordered by source index.  One lane per target cell merges its four buckets in ascending source index
// once per pass and accumulates.
#include "common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kLdsInts = 16384;               // 64 KB: the bucket counts stay in LDS while (h + 1)(w + 1) + kThreads fits

__host__ __device__ inline size_t fi_ints_per_sample(int h, int w) {
    return (size_t)3 * h * w + (size_t)(h + 1) * (w + 1);
}

__global__ __launch_bounds__(kThreads) void forward_interp_kernel(const float* __restrict__ flow, float* __restrict__ out, int h, int w,
                                                                  int* __restrict__ ws, int counts_in_lds) {
    extern __shared__ int lds[];
    const int b = blockIdx.x, tid = threadIdx.x, bs = blockDim.x;
    const int N = h * w, W1 = w + 1, NB = (h + 1) * (w + 1);
    const float* dx = flow + (size_t)b * 2 * N;
    const float* dy = dx + N;
    int* key = ws + (size_t)b * fi_ints_per_sample(h, w);   // bucket of each source (-1: reaches no cell)
    int* l0 = key + N;                                       // sources by bucket, in placement order
    int* l1 = l0 + N;                                        // sources by bucket, ascending index
    int* part = lds;                                         // per-thread sums of the scan
    int* cnt = counts_in_lds ? lds + kThreads : l1 + N;      // counts -> bucket starts -> bucket ends
    for (int i = tid; i < NB; i += bs) cnt[i] = 0;
    __syncthreads();
    for (int s = tid; s < N; s += bs) {
        const float x1 = (float)(s % w) + dx[s], y1 = (float)(s / w) + dy[s];
        const float fx = floorf(x1), fy = floorf(y1);
        int k = -1;
        if (fx >= -1.f && fx < (float)w && fy >= -1.f && fy < (float)h) k = ((int)fy + 1) * W1 + (int)fx + 1;
        key[s] = k;
        if (k >= 0) atomicAdd(&cnt[k], 1);
    }
    __syncthreads();
    {   // exclusive scan of cnt[0, NB): contiguous runs per thread, then a Hillis-Steele scan of the run sums
        const int per = (NB + bs - 1) / bs, lo = min(tid * per, NB), hi = min(lo + per, NB);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += cnt[i];
        part[tid] = sum;
        __syncthreads();
        for (int off = 1; off < bs; off <<= 1) {
            const int v = tid >= off ? part[tid - off] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        int run = part[tid] - sum;
        for (int i = lo; i < hi; ++i) { const int c = cnt[i]; cnt[i] = run; run += c; }
    }
    __syncthreads();
    for (int s = tid; s < N; s += bs) {                      // placement: afterwards cnt[k] is the END of bucket k
        const int k = key[s];
        if (k >= 0) l0[atomicAdd(&cnt[k], 1)] = s;
    }
    __syncthreads();
    const int placed = cnt[NB - 1];
    for (int p = tid; p < placed; p += bs) {                 // each bucket in ascending source index (indices are unique)
        const int s = l0[p], k = key[s];
        const int beg = k ? cnt[k - 1] : 0, end = cnt[k];
        int r = 0;
        for (int q = beg; q < end; ++q) r += l0[q] < s;
        l1[beg + r] = s;
    }
    __syncthreads();
    for (int t = tid; t < N; t += bs) {
        const int tx = t % w, ty = t / w;
        const float ftx = (float)tx, fty = (float)ty;
        const int kb = (ty + 1) * W1 + tx + 1;
        const int ks[4] = {kb - W1 - 1, kb - W1, kb - 1, kb};   // floor cells (tx-1, ty-1), (tx, ty-1), (tx-1, ty), (tx, ty)
        int beg[4], end[4];
        for (int j = 0; j < 4; ++j) { beg[j] = ks[j] ? cnt[ks[j] - 1] : 0; end[j] = cnt[ks[j]]; }
        float vx = 0.f, vy = 0.f, ws_ = 0.f;
        for (int pass = 0; pass < 4; ++pass) {
            const bool cx = pass >= 2, cy = pass & 1;
            int i[4] = {beg[0], beg[1], beg[2], beg[3]};
            while (true) {                                   // four-way merge by source index
                int jm = -1, sm = 0x7fffffff;
                for (int j = 0; j < 4; ++j)
                    if (i[j] < end[j] && l1[i[j]] < sm) { sm = l1[i[j]]; jm = j; }
                if (jm < 0) break;
                ++i[jm];
                const float ddx = dx[sm], ddy = dy[sm];
                const float x1 = (float)(sm % w) + ddx, y1 = (float)(sm / w) + ddy;
                const float xv = cx ? ceilf(x1) : floorf(x1), yv = cy ? ceilf(y1) : floorf(y1);
                if (xv != ftx || yv != fty) continue;
                const float wt = (1.f - fabsf(x1 - xv)) * (1.f - fabsf(y1 - yv));
                vx = vx + ddx * wt;
                vy = vy + ddy * wt;
                ws_ = ws_ + wt;
            }
        }
        const float den = ws_ + 1e-15f;
        out[(size_t)b * 2 * N + t] = vx / den;
        out[(size_t)b * 2 * N + N + t] = vy / den;
    }
}

}  // namespace

extern "C" size_t eraft_forward_interpolate_scratch(int batch, int h, int w) {
    if (batch < 1 || h < 1 || w < 1) return 0;
    return (size_t)batch * fi_ints_per_sample(h, w);
}

extern "C" int eraft_forward_interpolate(const float* flow, float* out, int batch, int h, int w, int* scratch, size_t scratch_ints,
                                         void* stream) {
    EEM_REQUIRE(flow && out && scratch, "eraft_forward_interpolate: NULL argument");
    EEM_REQUIRE(batch >= 1 && h >= 1 && w >= 1 && (long)h * w <= (1L << 24), "eraft_forward_interpolate: bad size %d x %d x %d", batch, h, w);
    EEM_REQUIRE(flow != out, "eraft_forward_interpolate: out must not alias flow");
    const size_t need = eraft_forward_interpolate_scratch(batch, h, w);
    EEM_REQUIRE(scratch_ints >= need, "eraft_forward_interpolate: scratch holds %zu ints, %zu needed", scratch_ints, need);
    const int nb = (h + 1) * (w + 1);
    const int in_lds = nb + kThreads <= kLdsInts;
    const size_t lds = (size_t)(in_lds ? kThreads + nb : kThreads) * sizeof(int);
    hipLaunchKernelGGL(forward_interp_kernel, dim3(batch), dim3(kThreads), lds, (hipStream_t)stream, flow, out, h, w, scratch, in_lds);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}
