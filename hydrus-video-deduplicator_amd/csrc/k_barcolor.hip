// k_barcolor.hip -- bar-colour content rectangle: the content rectangle of k_autocrop.hip for bars that are not
// black. One bar colour c = (c0, c1, c2) per video, in the byte order of the pixel (gray: c0 only), packed as
// int32 = c0 | c1 << 8 | c2 << 16.
//
// The rule (integers only): a pixel p is content iff max_k |p_k - c_k| > bar_level; rows, columns, frame box, video box and the
// per-axis fallback below 64 are DESIGN 4.7's with "bright" read as "content". The automatic colour of a video comes from the
// four corner pixels of all its frames: lo_k / hi_k = min / max per channel; hi_k - lo_k <= bar_level on every channel gives
// c_k = (lo_k + hi_k) >> 1, anything else (and a video without frames) gives c = 0, the black rule.
//
//   k_corner_init           accumulators {lo0, lo1, lo2, hi0, hi1, hi2, -, -} = {INT_MAX x 3, -1 x 3} per video, in caller scratch
//   k_corner_fold           one lane per frame: its 4 corners -> atomicMin / atomicMax into its video's accumulators
//   k_corner_finish         the rule above -> the packed colour
//   k_content_rect_color    k_content_rect's pass (k_autocrop.hip) under the colour predicate
// The rectangle accumulators are initialised and closed by k_autocrop.hip's k_rect_init / k_rect_finish, and everything
// behind the rectangle is shared as it is. The pass is written out here and not shared with k_content_rect: moving that
// kernel's body into a header changed its instruction stream.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_pdq_dev.h"

namespace hvd {

namespace {

// the video that holds frame f: the last v with offsets[v] <= f (videos without frames are skipped); always in [0, V)
__device__ __forceinline__ int video_of_frame(const long long* __restrict__ offsets, int V, long long f) {
    int lo = 0, hi = V;  // offsets[lo] <= f < offsets[hi] by the CSR's contract
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}

constexpr int kAcc = 8;  // int32 words of corner accumulator per video: lo[3], hi[3], 2 unused (one 32-byte record)

__global__ __launch_bounds__(256) void k_corner_init(int32_t* __restrict__ acc, int V) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int32_t* a = acc + kAcc * (size_t)v;
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] = INT_MAX; a[3 + k] = -1; }
}

// 4 * CH bytes per frame. The merge is integer min / max, so the result does not depend on the order of the frames.
template <int CH>
__global__ __launch_bounds__(256) void k_corner_fold(const uint8_t* __restrict__ frames, long long n, int h, int w,
                                                     const long long* __restrict__ offsets, int V,
                                                     int32_t* __restrict__ acc) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const uint8_t* src = frames + (size_t)f * h * w * CH;
    const size_t corner[4] = {0, (size_t)(w - 1) * CH, (size_t)(h - 1) * w * CH, ((size_t)h * w - 1) * CH};
    int32_t* a = acc + kAcc * (size_t)video_of_frame(offsets, V, f);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        int lo = 255, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = src[corner[c] + k];
            lo = min(lo, p);
            hi = max(hi, p);
        }
        atomicMin(&a[k], lo);
        atomicMax(&a[3 + k], hi);
    }
}

__global__ __launch_bounds__(256) void k_corner_finish(const int32_t* __restrict__ acc, int V, int channels, int bar_level,
                                                       int32_t* __restrict__ colors) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int32_t* a = acc + kAcc * (size_t)v;
    int c = 0;
    bool uniform = true;
    for (int k = 0; k < channels; ++k) {
        const int lo = a[k], hi = a[3 + k];
        uniform = uniform && hi >= lo && hi - lo <= bar_level;  // hi < lo: the video has no frames
        c |= ((lo + hi) >> 1 & 0xFF) << (8 * k);
    }
    colors[v] = uniform ? c : 0;
}

constexpr int kUnit = 16;  // pixels a lane takes from a row: 16 B of gray, 48 B of RGB24 = whole 16-byte loads

// |p_k - c_k| > L on any channel, as one subtract and one unsigned compare per channel: with lo'_k = max(0, c_k - L) and
// span_k = min(255, c_k + L) - lo'_k, a byte p lies in [lo'_k, lo'_k + span_k] iff (uint32)(p - lo'_k) <= span_k (below lo'_k
// the difference wraps to >= 2^32 - 255), and inside [0, 255] that interval is exactly |p - c_k| <= L.
struct ColorPred {
    uint32_t lo[3], span[3];
    __device__ __forceinline__ ColorPred(int color, int bar_level) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = (color >> (8 * k)) & 0xFF;
            const int l = max(0, c - bar_level);
            lo[k] = (uint32_t)l;
            span[k] = (uint32_t)(min(255, c + bar_level) - l);
        }
    }
    __device__ __forceinline__ bool gray(uint32_t p) const { return p - lo[0] > span[0]; }
    __device__ __forceinline__ bool rgb(uint32_t a, uint32_t b, uint32_t c) const {
        return (a - lo[0] > span[0]) | (b - lo[1] > span[1]) | (c - lo[2] > span[2]);
    }
};

// Content pixels per row and per column of one frame, one workgroup of 256 lanes per frame: k_content_rect's decomposition
// (k_autocrop.hip). The lanes form R = 256 / P rows of P = pow2 >= ceil(w / 16) lanes; lane (r, u) reads pixels
// [16u, 16u + 16) of rows r, r + R, ... and keeps the 16 column counts of its unit in registers for the whole frame. A row's
// count is a segmented wave reduction (P <= 64: the row lies inside one wave) folded into LDS; the column counts are folded
// into LDS once per frame. The workgroup looks up its video and that video's colour once; lo' and span are wave-uniform.
// WIDE: w % 16 == 0 and the frame base is 16-byte aligned, so every unit is CH aligned 16-byte loads; otherwise byte loads.
// LDS: int rowcnt[h], colcnt[w] (dynamic), 4 words of box.
template <int CH, bool WIDE>
__global__ __launch_bounds__(256) void k_content_rect_color(const uint8_t* __restrict__ frames, int h, int w,
                                                            const long long* __restrict__ offsets, int V,
                                                            const int32_t* __restrict__ colors, int bar_level,
                                                            int min_bright, int32_t* __restrict__ boxes) {
    extern __shared__ int lds[];
    int* rowcnt = lds;
    int* colcnt = lds + h;
    __shared__ int box[4];
    const int tid = threadIdx.x;
    const long long frame = blockIdx.x;
    const uint8_t* src = frames + (size_t)frame * h * w * CH;
    const int video = video_of_frame(offsets, V, frame);
    const ColorPred pred(colors[video], bar_level);

    for (int i = tid; i < h + w; i += 256) lds[i] = 0;
    if (tid == 0) { box[0] = INT_MAX; box[1] = -1; box[2] = INT_MAX; box[3] = -1; }
    __syncthreads();

    const int units = (w + kUnit - 1) / kUnit;
    int P = 1;
    while (P < units) P <<= 1;  // <= 256 (w <= 4096)
    const int R = 256 / P;
    const int u = tid & (P - 1), r0 = tid / P;
    const int x0 = u * kUnit;
    const bool live = u < units;

    int cnt[kUnit];
#pragma unroll
    for (int p = 0; p < kUnit; ++p) cnt[p] = 0;

    for (int yb = 0; yb < h; yb += R) {
        const int y = yb + r0;
        int rc = 0;
        if (live && y < h) {
            const uint8_t* row = src + ((size_t)y * w + x0) * CH;
            if (WIDE) {
                uint32_t q[4 * CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const uint4 t = reinterpret_cast<const uint4*>(row)[c];
                    q[4 * c] = t.x; q[4 * c + 1] = t.y; q[4 * c + 2] = t.z; q[4 * c + 3] = t.w;
                }
#pragma unroll
                for (int p = 0; p < kUnit; ++p) {
                    bool b;
                    if (CH == 1) {
                        b = pred.gray(byte_of(q[p >> 2], p & 3));
                    } else {
                        const int e = 3 * p;
                        b = pred.rgb(byte_of(q[e >> 2], e & 3), byte_of(q[(e + 1) >> 2], (e + 1) & 3),
                                     byte_of(q[(e + 2) >> 2], (e + 2) & 3));
                    }
                    cnt[p] += b ? 1 : 0;
                    rc += b ? 1 : 0;
                }
            } else {
#pragma unroll
                for (int p = 0; p < kUnit; ++p) {
                    bool b = false;
                    if (x0 + p < w) {
                        if (CH == 1) b = pred.gray((uint32_t)row[p]);
                        else b = pred.rgb((uint32_t)row[3 * p], (uint32_t)row[3 * p + 1], (uint32_t)row[3 * p + 2]);
                    }
                    cnt[p] += b ? 1 : 0;
                    rc += b ? 1 : 0;
                }
            }
        }
        // the row's count: lanes of one row are P consecutive lanes (a segment of the wave, or whole waves)
        for (int m = (P < 64 ? P : 64) >> 1; m > 0; m >>= 1) rc += __shfl_xor(rc, m);
        if ((tid & ((P < 64 ? P : 64) - 1)) == 0 && y < h && rc) atomicAdd(&rowcnt[y], rc);
    }
    if (live) {
#pragma unroll
        for (int p = 0; p < kUnit; ++p)
            if (cnt[p] && x0 + p < w) atomicAdd(&colcnt[x0 + p], cnt[p]);
    }
    __syncthreads();

    int top = INT_MAX, bot = -1, left = INT_MAX, right = -1;
    for (int y = tid; y < h; y += 256)
        if (rowcnt[y] >= min_bright) { top = min(top, y); bot = max(bot, y); }
    for (int x = tid; x < w; x += 256)
        if (colcnt[x] >= min_bright) { left = min(left, x); right = max(right, x); }
    if (bot >= 0) { atomicMin(&box[0], top); atomicMax(&box[1], bot); }
    if (right >= 0) { atomicMin(&box[2], left); atomicMax(&box[3], right); }
    __syncthreads();
    if (tid == 0 && box[1] >= 0 && box[3] >= 0) {
        int32_t* vb = boxes + 4 * (size_t)video;
        atomicMin(&vb[0], box[0]);
        atomicMax(&vb[1], box[1]);
        atomicMin(&vb[2], box[2]);
        atomicMax(&vb[3], box[3]);
    }
}

// the middle step of launch_content_rects_color, between k_autocrop.hip's rect init and finish
hipError_t rect_fold_color(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets, uint32_t V,
                           const int32_t* d_colors, int bar_level, int min_bright, int32_t* d_rects, hipStream_t s) {
    // 64 x 64 frames: no box can be smaller than the frame and at least 64 long, so every rectangle is the full frame
    if (n <= 0 || (h == 64 && w == 64)) return hipSuccess;
    const size_t lds = sizeof(int) * (size_t)(h + w);
    const bool wide = (w % kUnit) == 0 && ((uintptr_t)d_frames & 15u) == 0;
    const dim3 gf((unsigned)n);
#define HVD_CRC(CH, WIDE) hipLaunchKernelGGL((k_content_rect_color<CH, WIDE>), gf, dim3(256), lds, s, d_frames, h, w, d_offsets, (int)V, d_colors, bar_level, min_bright, d_rects)
    if (channels == 3) {
        if (wide) HVD_CRC(3, true);
        else HVD_CRC(3, false);
    } else {
        if (wide) HVD_CRC(1, true);
        else HVD_CRC(1, false);
    }
#undef HVD_CRC
    return hipGetLastError();
}

}  // namespace

size_t bar_colors_scratch_bytes(uint32_t V) { return sizeof(int32_t) * kAcc * (size_t)V; }

hipError_t launch_bar_colors(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets,
                             uint32_t V, int bar_level, int32_t* d_acc, int32_t* d_colors, hipStream_t s) {
    if (V == 0) return hipSuccess;
    const dim3 gv((V + 255) / 256), gf((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_corner_init, gv, dim3(256), 0, s, d_acc, (int)V);
    if (n > 0) {
        if (channels == 3)
            hipLaunchKernelGGL(k_corner_fold<3>, gf, dim3(256), 0, s, d_frames, (long long)n, h, w, d_offsets, (int)V, d_acc);
        else
            hipLaunchKernelGGL(k_corner_fold<1>, gf, dim3(256), 0, s, d_frames, (long long)n, h, w, d_offsets, (int)V, d_acc);
    }
    hipLaunchKernelGGL(k_corner_finish, gv, dim3(256), 0, s, (const int32_t*)d_acc, (int)V, channels, bar_level, d_colors);
    return hipGetLastError();
}

hipError_t launch_content_rects_color(const uint8_t* d_frames, int64_t n, int h, int w, int channels,
                                      const long long* d_offsets, uint32_t V, const int32_t* d_colors, int bar_level,
                                      int min_bright, int32_t* d_rects, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipError_t e = launch_rect_init(d_rects, V, s);
    if (e == hipSuccess)
        e = rect_fold_color(d_frames, n, h, w, channels, d_offsets, V, d_colors, bar_level, min_bright, d_rects, s);
    if (e == hipSuccess) e = launch_rect_finish(d_rects, V, h, w, s);
    return e;
}

}  // namespace hvd
