// Visualisation on the device: the colour image of a flow field and the red / blue image of an event volume, as the reference's
// evaluation loop writes them with visualize_map (test_mvsec.py:618-637).
//
// eemflow_flow_to_image_many: the Middlebury colour wheel of tensor_tools.flow_to_image_dmax (utils_luo/tools.py:2385-2523) for a float32
// flow, which is how visualize_optical_flow_light calls it.  The arithmetic contract ("Visualisation"):
//   * |u| > 1e7 or |v| > 1e7 (infinities included): the pixel is unknown, counts as (0, 0) for the maximum and is black;
//   * maxrad = max over the frame of sqrtf(u*u + v*v) in fp32 - taken as sqrtf(max(u*u + v*v)), the root being monotone and correctly
//     rounded; a NaN anywhere in the frame makes Python's max(-1, nan) return -1;
//   * divisor = (double)maxrad + 2^-52, and everything from the division on is fp64: normalised components, radius, angle, wheel
//     interpolation; rad <= 1 fades towards white, rad > 1 (about half of the maximum-radius pixels land there) darkens by 0.75;
//   * NaN pixels are black; the byte is uint8(floor(255 * col)).
// Two launches: pass 1 reduces each frame's maximum of u*u + v*v onto one 32-bit cell of the caller's stats row (atomic max on the bit
// pattern, non-negative floats order like unsigned integers; all-ones = "a NaN was seen"); pass 2 turns the cell into the frame's divisor
// and colours.  The cell is private to its frame: n frames of one call get n divisors.
//
// eemflow_event_image_many: vis_map_RGB (test_mvsec.py:175-233) - s = the channel sum in fp32, density = count(s > 0.1) / (h*w), white
// background, s <= mean - 0.2 red, s >= mean + 0.2 blue (painted last).  Pass 1 adds s (fp64) and the count per frame, pass 2 rounds the
// fp64 mean to fp32 once and paints.
//
// Both: blockIdx.y = frame, a lane owns four consecutive pixels - two (bins) 16-byte loads, three dword stores of twelve packed bytes;
// frames whose plane size is not a multiple of 4 (or whose pointers are not aligned) take one pixel loads, a last partial group of
// pixels byte stores.  Built with -ffp-contract=off: the decisions rad <= 1 and floor() sit on the last bit.
#include <math.h>
#include <string.h>

#include "common.h"

namespace {

constexpr int NCOLS = 55;                                  // RY 15 + YG 6 + GC 4 + CB 11 + BM 13 + MR 6
constexpr unsigned NAN_SEEN = 0xFFFFFFFFu;

struct VizMany { const float* in[16]; const float* norm[16]; unsigned char* out[16]; };

// the reference's unknown-flow test on fp32 values (1e7 is exact in fp32)
__device__ __forceinline__ bool flow_unknown(float u, float v) { return fabsf(u) > 1e7f || fabsf(v) > 1e7f; }

// Middlebury wheel entry k (0..54), channel ch, as the integer the reference's floor(255 * i / N) gives
__device__ __forceinline__ int wheel_entry(int k, int ch) {
    int r, g, b;
    if (k < 15) { r = 255; g = 255 * k / 15; b = 0; }
    else if (k < 21) { r = 255 - 255 * (k - 15) / 6; g = 255; b = 0; }
    else if (k < 25) { r = 0; g = 255; b = 255 * (k - 21) / 4; }
    else if (k < 36) { r = 0; g = 255 - 255 * (k - 25) / 11; b = 255; }
    else if (k < 49) { r = 255 * (k - 36) / 13; g = 0; b = 255; }
    else { r = 255; g = 0; b = 255 - 255 * (k - 49) / 6; }
    return ch == 0 ? r : ch == 1 ? g : b;
}

__device__ __forceinline__ void load4(const float* __restrict__ plane, long p0, long hw, bool vec, float (&x)[4]) {
    if (vec) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(plane + p0);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = a[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = p0 + i < hw ? plane[p0 + i] : 0.f;
    }
}

// twelve bytes (four pixels) as three dwords, or the valid pixels' bytes one by one
__device__ __forceinline__ void store_pixels(unsigned char* __restrict__ img, long p0, long hw, bool dword_ok, const unsigned char (&b)[12]) {
    if (dword_ok && p0 + 4 <= hw) {
        unsigned* o = reinterpret_cast<unsigned*>(img + 3 * p0);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            o[q] = (unsigned)b[4 * q] | ((unsigned)b[4 * q + 1] << 8) | ((unsigned)b[4 * q + 2] << 16) | ((unsigned)b[4 * q + 3] << 24);
    } else {
        for (int i = 0; i < 4 && p0 + i < hw; ++i) {
            img[3 * (p0 + i)] = b[3 * i]; img[3 * (p0 + i) + 1] = b[3 * i + 1]; img[3 * (p0 + i) + 2] = b[3 * i + 2];
        }
    }
}

// ------------------------------------------------------------------------------------------------ flow, pass 1: the frame's maximum
__global__ __launch_bounds__(256) void flow_max_kernel(VizMany many, long hw, int vec, double* __restrict__ stats) {
    const float* __restrict__ fu = many.in[blockIdx.y];
    const float* __restrict__ fv = fu + hw;
    unsigned best = 0;
    const long step = (long)gridDim.x * 256 * 4;
    for (long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4; p0 < hw; p0 += step) {
        float u[4], v[4];
        load4(fu, p0, hw, vec, u);
        load4(fv, p0, hw, vec, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool unk = flow_unknown(u[i], v[i]);
            const float uu = unk ? 0.f : u[i], vv = unk ? 0.f : v[i];
            const float r2 = uu * uu + vv * vv;                       // (at most 2e14: no overflow below the unknown threshold)
            const unsigned bits = r2 != r2 ? NAN_SEEN : __float_as_uint(r2);
            best = max(best, bits);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
    __shared__ unsigned red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = max(max(red[0], red[1]), max(red[2], red[3]));
        if (best) atomicMax(reinterpret_cast<unsigned*>(stats + 4 * blockIdx.y + 1), best);      // (the cell starts at 0)
    }
}

// ------------------------------------------------------------------------------------------------ flow, pass 2: the colours
__global__ __launch_bounds__(256) void flow_color_kernel(VizMany many, long hw, int vec, int dword_ok, int bgr, double* __restrict__ stats) {
    __shared__ double wheel[NCOLS * 3];                              // colorwheel / 255, fp64 as the reference divides
    for (int t = threadIdx.x; t < NCOLS * 3; t += 256) wheel[t] = (double)wheel_entry(t / 3, t % 3) / 255.0;
    const unsigned cell = *reinterpret_cast<const unsigned*>(stats + 4 * blockIdx.y + 1);
    // max(-1, np.max(rad)) + np.finfo(float).eps: -1 when the frame holds a NaN
    const double divisor = (cell == NAN_SEEN ? -1.0 : (double)sqrtf(__uint_as_float(cell))) + 0x1p-52;
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[4 * blockIdx.y] = divisor;
    __syncthreads();

    const float* __restrict__ fu = many.in[blockIdx.y];
    const float* __restrict__ fv = fu + hw;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= hw) return;
    float u[4], v[4];
    load4(fu, p0, hw, vec, u);
    load4(fv, p0, hw, vec, v);
    unsigned char bytes[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool black = flow_unknown(u[i], v[i]) || u[i] != u[i] || v[i] != v[i];
        const double ud = (double)u[i] / divisor, vd = (double)v[i] / divisor;
        const double rad = sqrt(ud * ud + vd * vd);
        const double a = atan2(-vd, -ud) / M_PI;
        const double fk = (a + 1.0) / 2.0 * (double)(NCOLS - 1) + 1.0;
        int k0 = (int)floor(fk);
        k0 = black ? 1 : min(max(k0, 1), NCOLS);                     // (fk is in [1, 55] for every finite pixel)
        const int k1 = k0 + 1 == NCOLS + 1 ? 1 : k0 + 1;
        const double f = fk - (double)k0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            double col = (1.0 - f) * wheel[(k0 - 1) * 3 + ch] + f * wheel[(k1 - 1) * 3 + ch];
            if (rad <= 1.0) col = 1.0 - rad * (1.0 - col);
            else col *= 0.75;
            const unsigned char byte = black ? 0 : (unsigned char)(int)floor(255.0 * col);
            bytes[3 * i + (bgr ? 2 - ch : ch)] = byte;
        }
    }
    store_pixels(many.out[blockIdx.y], p0, hw, dword_ok != 0, bytes);
}

// ------------------------------------------------------------------------------------------------ events
// the channel sum of four pixels in fp32, in channel order; a raw grid's non-zero voxels are normalised as conv_enc1.hip reads them:
// (x - mean) * (1 / sd), or x - mean where the record says the deviation does not scale
__device__ __forceinline__ void event_sums(const float* __restrict__ vol, const float* __restrict__ rec, int bins, long p0, long hw,
                                           bool vec, float (&s)[4]) {
    float n_mean = 0.f, n_inv = 1.f;
    bool n_on = false;
    if (rec) {
        n_mean = rec[0];
        n_inv = rec[2] != 0.f ? 1.f / rec[1] : 1.f;
        n_on = rec[3] != 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = 0.f;
    for (int c = 0; c < bins; ++c) {
        float x[4];
        load4(vol + (long)c * hw, p0, hw, vec, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float xn = (n_on && x[i] != 0.f) ? (x[i] - n_mean) * n_inv : x[i];
            s[i] = c == 0 ? xn : s[i] + xn;
        }
    }
}

__global__ __launch_bounds__(256) void event_stats_kernel(VizMany many, int bins, long hw, int vec, double* __restrict__ stats) {
    const float* __restrict__ vol = many.in[blockIdx.y];
    const float* __restrict__ rec = many.norm[blockIdx.y];
    double sum = 0.0, cnt = 0.0;
    const long step = (long)gridDim.x * 256 * 4;
    for (long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4; p0 < hw; p0 += step) {
        float s[4];
        event_sums(vol, rec, bins, p0, hw, vec, s);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (p0 + i < hw) { sum += (double)s[i]; cnt += s[i] > 0.1f ? 1.0 : 0.0; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    __shared__ double red[2][4];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sum; red[1][threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        atomicAdd(stats + 4 * blockIdx.y + 1 + threadIdx.x, t);       // [1] sum of s, [2] count(s > 0.1)
    }
}

__global__ __launch_bounds__(256) void event_paint_kernel(VizMany many, int bins, long hw, int vec, int dword_ok, int bgr,
                                                          double* __restrict__ stats) {
    const float mean = (float)(stats[4 * blockIdx.y + 1] / (double)hw);      // the fp64 mean, rounded to fp32 once
    const float lo = mean - 0.2f, hi = mean + 0.2f;
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[4 * blockIdx.y] = stats[4 * blockIdx.y + 2] / (double)hw;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= hw) return;
    float s[4];
    event_sums(many.in[blockIdx.y], many.norm[blockIdx.y], bins, p0, hw, vec, s);
    unsigned char bytes[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned char c0 = 255, c1 = 255, c2 = 255;
        if (s[i] <= lo) { c1 = 0; c2 = 0; }                              // [255, 0, 0]
        if (s[i] >= hi) { c0 = 0; c1 = 0; c2 = 255; }                    // [0, 0, 255], painted afterwards
        bytes[3 * i] = bgr ? c2 : c0; bytes[3 * i + 1] = c1; bytes[3 * i + 2] = bgr ? c0 : c2;
    }
    store_pixels(many.out[blockIdx.y], p0, hw, dword_ok != 0, bytes);
}

int reduce_blocks(long hw) {
    long b = (hw + 4095) / 4096;                                         // four passes of a 256 x 4 block at least
    return (int)(b > 64 ? 64 : b < 1 ? 1 : b);
}

}  // namespace

// n frames (1..16) of one size: flow[i] [2][h][w] and image_out[i] [h][w][3] are host arrays of device pointers, read before the call
// returns.  stats (device, n x 4 doubles) is initialised here: [i][0] receives frame i's divisor, [i][1] is the reduction cell.
extern "C" int eemflow_flow_to_image_many(int n, const float* const* flow, uint8_t* const* image_out, double* stats, int h, int w, int bgr,
                                          void* stream) {
    EEM_REQUIRE(n >= 1 && n <= 16, "eemflow_flow_to_image_many: 1..16 frames per call; got %d", n);
    EEM_REQUIRE(flow && image_out && stats, "eemflow_flow_to_image_many: NULL argument");
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 28), "eemflow_flow_to_image_many: bad size %dx%d", h, w);
    EEM_REQUIRE(((uintptr_t)stats & 7) == 0, "eemflow_flow_to_image_many: stats must be 8-byte aligned");
    VizMany m;
    memset(&m, 0, sizeof(m));
    uintptr_t in_bits = 0, out_bits = 0;
    for (int i = 0; i < n; ++i) {
        EEM_REQUIRE(flow[i] && image_out[i], "eemflow_flow_to_image_many: frame %d has a NULL tensor", i);
        m.in[i] = flow[i]; m.out[i] = image_out[i];
        in_bits |= (uintptr_t)flow[i]; out_bits |= (uintptr_t)image_out[i];
    }
    hipStream_t st = (hipStream_t)stream;
    const long hw = (long)h * w;
    const int vec = (hw & 3) == 0 && (in_bits & 15) == 0, dword_ok = (out_bits & 3) == 0;
    EEM_HIP_CHECK(hipMemsetAsync(stats, 0, (size_t)n * 4 * sizeof(double), st));
    hipLaunchKernelGGL(flow_max_kernel, dim3(reduce_blocks(hw), n), dim3(256), 0, st, m, hw, vec, stats);
    hipLaunchKernelGGL(flow_color_kernel, dim3((unsigned)((hw + 1023) / 1024), n), dim3(256), 0, st, m, hw, vec, dword_ok, bgr != 0, stats);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}

// n volumes (1..16) of one size: volume[i] [bins][h][w]; norm == NULL (normalised volumes) or norm[i] = the four floats {mean, sd, scale,
// any} of a raw grid (eemflow_voxelize with normalize = 2).  stats (device, n x 4 doubles), initialised here: [i][0] receives the density
// count(s > 0.1) / (h*w), [i][1] the sum of s, [i][2] the count.
extern "C" int eemflow_event_image_many(int n, const float* const* volume, const float* const* norm, int bins, int h, int w,
                                        uint8_t* const* image_out, double* stats, int bgr, void* stream) {
    EEM_REQUIRE(n >= 1 && n <= 16, "eemflow_event_image_many: 1..16 volumes per call; got %d", n);
    EEM_REQUIRE(volume && image_out && stats, "eemflow_event_image_many: NULL argument");
    EEM_REQUIRE(bins >= 1 && bins <= 64, "eemflow_event_image_many: bins %d (1..64)", bins);
    EEM_REQUIRE(h >= 1 && w >= 1 && (long)h * w <= (1L << 28), "eemflow_event_image_many: bad size %dx%d", h, w);
    EEM_REQUIRE(((uintptr_t)stats & 7) == 0, "eemflow_event_image_many: stats must be 8-byte aligned");
    VizMany m;
    memset(&m, 0, sizeof(m));
    uintptr_t in_bits = 0, out_bits = 0;
    for (int i = 0; i < n; ++i) {
        EEM_REQUIRE(volume[i] && image_out[i] && (!norm || norm[i]), "eemflow_event_image_many: volume %d has a NULL tensor", i);
        m.in[i] = volume[i]; m.out[i] = image_out[i]; m.norm[i] = norm ? norm[i] : nullptr;
        in_bits |= (uintptr_t)volume[i]; out_bits |= (uintptr_t)image_out[i];
    }
    hipStream_t st = (hipStream_t)stream;
    const long hw = (long)h * w;
    const int vec = (hw & 3) == 0 && (in_bits & 15) == 0, dword_ok = (out_bits & 3) == 0;
    EEM_HIP_CHECK(hipMemsetAsync(stats, 0, (size_t)n * 4 * sizeof(double), st));
    hipLaunchKernelGGL(event_stats_kernel, dim3(reduce_blocks(hw), n), dim3(256), 0, st, m, bins, hw, vec, stats);
    hipLaunchKernelGGL(event_paint_kernel, dim3((unsigned)((hw + 1023) / 1024), n), dim3(256), 0, st, m, bins, hw, vec, dword_ok, bgr != 0, stats);
    EEM_HIP_CHECK(hipGetLastError());
    return EEM_OK;
}
