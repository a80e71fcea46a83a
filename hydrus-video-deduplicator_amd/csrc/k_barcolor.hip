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
// behind the rectangle is shared as it is. The pass itself is hvd_content_rect_dev.h's content_rect_fold, the one body of
// k_content_rect and k_content_rect_color.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "hvd_content_rect_dev.h"
#include "hvd_kernels.h"

namespace hvd {

namespace {

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

// Content pixels per row and per column of one frame, one workgroup of 256 lanes per frame: content_rect_fold
// (hvd_content_rect_dev.h) under the colour predicate. The workgroup looks up its video and that video's colour once, before
// the fold; lo' and span are wave-uniform.
template <int CH, bool WIDE>
__global__ __launch_bounds__(256) void k_content_rect_color(const uint8_t* __restrict__ frames, int h, int w,
                                                            const long long* __restrict__ offsets, int V,
                                                            const int32_t* __restrict__ colors, int bar_level,
                                                            int min_bright, int32_t* __restrict__ boxes) {
    extern __shared__ int lds[];
    __shared__ int box[4];
    const long long frame = blockIdx.x;
    const int video = video_of_frame(offsets, V, frame);
    const ColorPred pred(colors[video], bar_level);
    content_rect_fold<CH, WIDE>(frames + (size_t)frame * h * w * CH, h, w, pred, min_bright, lds, box, boxes, [&] { return video; });
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

// the colour rule's fold (launch_rect_fold, k_autocrop.hip)
hipError_t rect_fold_color(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets, uint32_t V,
                           const int32_t* d_colors, int bar_level, int min_bright, int32_t* d_rects, hipStream_t s) {
    return rect_fold_dispatch(d_frames, n, h, w, channels, [&](auto ch, auto wide, dim3 grid, size_t lds) {
        hipLaunchKernelGGL((k_content_rect_color<decltype(ch)::value, decltype(wide)::value>), grid, dim3(256), lds, s, d_frames, h,
                           w, d_offsets, (int)V, d_colors, bar_level, min_bright, d_rects);
    });
}

}  // namespace hvd
