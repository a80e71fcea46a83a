// k_autocrop.hip -- content-rectangle PDQ: find the rectangle a video's black bars leave, and run the generic
// four-pass down-sampler inside it, with a geometry per video.
//
// The rule (integers only): a pixel is bright iff max(R, G, B) > black_level; a row (column) of a frame is content iff it
// holds >= min_bright bright pixels; a frame's box is the bounding box of its content rows x content columns (none if either
// is empty); a video's box is the bounding box of its frames' boxes; an axis whose box is missing or shorter than 64 keeps the
// full extent. Record: int32[4] = {top, left, height, width}.
//
//   k_rect_init        box accumulators {top, bottom, left, right} = {INT_MAX, -1, INT_MAX, -1}, in the rectangle buffer itself
//   k_content_rect     one workgroup per frame: bright counts per row and per column, frame box -> atomicMin / atomicMax
//   k_rect_finish      fallbacks, {top, bottom, left, right} -> {top, left, height, width}
//   k_frame_geom       frame -> its video's rectangle (binary search in the CSR), checked against the frame
//   k_box_scan_rect    the generic line pass (hvd_pdq_dev.h: box_scan_lines, k_pdq.hip's k_box_scan_T) with {origin, lines,
//                      len, win, pitch} taken from that table
//   k_luma64_rect      the plane of a 64 x 64 rectangle: the crop's luma, unfiltered
// Frames up to 512 x 512 take the same four passes fused into one launch instead: k_down_rect, k_autocrop_fused.hip.
// Luma and the line pass are hvd_pdq_dev.h's, the one home of the bit-exactness contract.
// init -> fold -> finish is written here for every rule (launch_content_rects, launch_rect_fold: the one switch over
// RectRule::kind); what the three rules' folds share is hvd_content_rect_dev.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "hvd_content_rect_dev.h"
#include "hvd_kernels.h"
#include "hvd_pdq_dev.h"

namespace hvd {

namespace {

__global__ __launch_bounds__(256) void k_rect_init(int32_t* __restrict__ rects, int V) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < V) reinterpret_cast<int4*>(rects)[v] = make_int4(INT_MAX, -1, INT_MAX, -1);
}

__global__ __launch_bounds__(256) void k_rect_finish(int32_t* __restrict__ rects, int V, int h, int w) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int4 b = reinterpret_cast<const int4*>(rects)[v];
    int top = b.x, hh = b.y - b.x + 1, left = b.z, ww = b.w - b.z + 1;
    if (b.y < b.x || hh < 64) { top = 0; hh = h; }
    if (b.w < b.z || ww < 64) { left = 0; ww = w; }
    reinterpret_cast<int4*>(rects)[v] = make_int4(top, left, hh, ww);
}

// max(R, G, B) > level
struct BrightPred {
    uint32_t level;
    __device__ __forceinline__ bool gray(uint32_t p) const { return p > level; }
    __device__ __forceinline__ bool rgb(uint32_t a, uint32_t b, uint32_t c) const { return max(max(a, b), c) > level; }
};

// Bright pixels per row and per column of one frame, one workgroup of 256 lanes per frame: content_rect_fold
// (hvd_content_rect_dev.h) under the bright predicate. The frame's video is looked up by the one lane that merges the box.
template <int CH, bool WIDE>
__global__ __launch_bounds__(256) void k_content_rect(const uint8_t* __restrict__ frames, int h, int w,
                                                      const long long* __restrict__ offsets, int V, int black_level,
                                                      int min_bright, int32_t* __restrict__ boxes) {
    extern __shared__ int lds[];
    __shared__ int box[4];
    const long long frame = blockIdx.x;
    content_rect_fold<CH, WIDE>(frames + (size_t)frame * h * w * CH, h, w, BrightPred{(uint32_t)black_level}, min_bright, lds, box,
                                boxes, [&] { return video_of_frame(offsets, V, frame); });
}

// frame -> {top, left, height, width} of its video. A record that does not lie inside the frame or is shorter than 64 on an
// axis (never produced by k_rect_finish) is replaced by the full frame, so that the down-sampler cannot read out of bounds.
__global__ __launch_bounds__(256) void k_frame_geom(const long long* __restrict__ offsets, int V,
                                                    const int32_t* __restrict__ rects, long long n, int h, int w,
                                                    int4* __restrict__ geom) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    int4 r = reinterpret_cast<const int4*>(rects)[video_of_frame(offsets, V, f)];
    const bool ok = r.x >= 0 && r.y >= 0 && r.z >= 64 && r.w >= 64 && r.z <= h && r.w <= w && r.x <= h - r.z && r.y <= w - r.w;
    if (!ok) r = make_int4(0, 0, h, w);
    geom[f] = r;
}

// The generic down-sampler's pass (k_pdq.hip: k_box_scan_T -- upstream's sequential running-sum box filter along the lines
// of a row-major [lines][len] image, one lane per line, output transposed, passes 3 and 4 keep the 64 sampled positions
// only), with the geometry of every frame taken from geom[frame] = {top, left, hh, ww} instead of the launch arguments:
//   PASS 1  frame bytes (pitch w, origin (top, left))  lines hh, len ww   -> [ww][hh]
//   PASS 2  [ww][hh]                                   lines ww, len hh   -> [hh][ww]
//   PASS 3  [hh][ww]                                   lines hh, len ww   -> [64][hh]
//   PASS 4  [64][hh]                                   lines 64, len hh   -> [64][64]
// Window jarosz_window(len). The recurrence is k_box_scan_T's own (one definition: box_scan_lines), so the planes are those
// of the contiguous crop, bit for bit. The grid covers the full frame's lines; a workgroup beyond its frame's lines returns at once.
// A 64 x 64 rectangle is no work here: the plain hash of a 64 x 64 frame is taken from its luma as it is (upstream's shortcut:
// no filter, and a window-1 running sum is not the identity in float), k_luma64_rect writes that plane.
template <int SRC, int PASS>  // SRC 0: float, 1: gray u8, 3: rgb24 (PASS 1 only)
__global__ __launch_bounds__(64) void k_box_scan_rect(const void* __restrict__ in, float* __restrict__ out,
                                                      const int4* __restrict__ geom, int w, long long in_frame_stride,
                                                      long long out_frame_stride) {
    const int4 rc = geom[blockIdx.y];
    const int lines = (PASS == 1 || PASS == 3) ? rc.z : PASS == 2 ? rc.w : 64;
    const int len = (PASS == 1 || PASS == 3) ? rc.w : rc.z;
    const int nsel = PASS >= 3 ? 64 : 0;
    if ((int)(blockIdx.x * 64) >= lines || (rc.z == 64 && rc.w == 64)) return;
    // (passes 2 - 4 read the contiguous [lines][len] image the pass before wrote: pitch and origin are pass 1's)
    box_scan_lines<SRC>(in, out, in_frame_stride, out_frame_stride, w, rc.x, rc.y, lines, len, jarosz_window(len), nsel);
}

// The plane of a frame whose rectangle is 64 x 64: the luma of the crop, unfiltered. One workgroup per frame.
template <int CH>
__global__ __launch_bounds__(256) void k_luma64_rect(const uint8_t* __restrict__ frames, float* __restrict__ out64,
                                                     const int4* __restrict__ geom, int w, long long in_frame_stride) {
    const int4 rc = geom[blockIdx.x];
    if (rc.z != 64 || rc.w != 64) return;
    const uint8_t* src = frames + (long long)blockIdx.x * in_frame_stride;
    float* dst = out64 + (size_t)blockIdx.x * 4096;
    for (int p = threadIdx.x; p < 4096; p += 256) {
        const long long e = (long long)(rc.x + (p >> 6)) * w + (rc.y + (p & 63));
        dst[p] = CH == 1 ? luma_gray(src[e]) : luma_rgb((float)src[3 * e], (float)src[3 * e + 1], (float)src[3 * e + 2]);
    }
}

}  // namespace

bool g_pdq_fused_rect = true;  // A/B switch (hvd_debug_set "pdq_fused_rect"): 0 forces the four generic passes

// init -> the rule's fold -> finish
hipError_t launch_content_rects(const RectRule& rule, const int32_t* d_colors, const uint8_t* d_frames, int64_t n, int h, int w,
                                int channels, const long long* d_offsets, uint32_t V, int32_t* d_rects, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipError_t e = launch_rect_init(d_rects, V, s);
    if (e == hipSuccess) e = launch_rect_fold(rule, d_colors, d_frames, n, h, w, channels, d_offsets, V, d_rects, s);
    if (e == hipSuccess) e = launch_rect_finish(d_rects, V, h, w, s);
    return e;
}

// The three steps of launch_content_rects one by one, for a caller that folds a video's frames batch by batch (the streaming
// hasher): init once, fold every batch (the atomicMin / atomicMax merge is order-free), finish once.
hipError_t launch_rect_init(int32_t* d_rects, uint32_t V, hipStream_t s) {
    hipLaunchKernelGGL(k_rect_init, dim3((V + 255) / 256), dim3(256), 0, s, d_rects, (int)V);
    return hipGetLastError();
}

hipError_t launch_rect_fold(const RectRule& rule, const int32_t* d_colors, const uint8_t* d_frames, int64_t n, int h, int w,
                            int channels, const long long* d_offsets, uint32_t V, int32_t* d_rects, hipStream_t s) {
    switch (rule.kind) {
        case RectKind::Black: return rect_fold_black(d_frames, n, h, w, channels, d_offsets, V, rule.level, rule.count, d_rects, s);
        case RectKind::Color: return rect_fold_color(d_frames, n, h, w, channels, d_offsets, V, d_colors, rule.level, rule.count, d_rects, s);
        case RectKind::Detail: return rect_fold_detail(d_frames, n, h, w, channels, d_offsets, V, rule.level, rule.count, d_rects, s);
    }
    return hipErrorInvalidValue;
}

hipError_t rect_fold_black(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets, uint32_t V,
                           int black_level, int min_bright, int32_t* d_rects, hipStream_t s) {
    return rect_fold_dispatch(d_frames, n, h, w, channels, [&](auto ch, auto wide, dim3 grid, size_t lds) {
        hipLaunchKernelGGL((k_content_rect<decltype(ch)::value, decltype(wide)::value>), grid, dim3(256), lds, s, d_frames, h, w,
                           d_offsets, (int)V, black_level, min_bright, d_rects);
    });
}

hipError_t launch_rect_finish(int32_t* d_rects, uint32_t V, int h, int w, hipStream_t s) {
    hipLaunchKernelGGL(k_rect_finish, dim3((V + 255) / 256), dim3(256), 0, s, d_rects, (int)V, h, w);
    return hipGetLastError();
}

size_t pdq_rects_geom_bytes(int64_t n) { return 16 * (size_t)n; }

hipError_t launch_pdq_downsample_rects(const uint8_t* d_frames, int64_t n, int h, int w, int channels,
                                       const long long* d_offsets, uint32_t V, const int32_t* d_rects, void* d_geom,
                                       float* d_ws, float* d_out64, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (jarosz_window(h) > kTW || jarosz_window(w) > kTW || V == 0) return hipErrorInvalidValue;
    int4* geom = (int4*)d_geom;
    hipLaunchKernelGGL(k_frame_geom, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_offsets, (int)V, d_rects,
                       (long long)n, h, w, geom);
    const size_t hw = (size_t)h * w;
    if (h <= kDownRectMax && w <= kDownRectMax && g_pdq_fused_rect) {
        launch_down_rect(d_frames, n, h, w, channels, geom, d_out64, s);
        if (channels == 3)
            hipLaunchKernelGGL(k_luma64_rect<3>, dim3((unsigned)n), dim3(256), 0, s, d_frames, d_out64, geom, w, (long long)hw * 3);
        else
            hipLaunchKernelGGL(k_luma64_rect<1>, dim3((unsigned)n), dim3(256), 0, s, d_frames, d_out64, geom, w, (long long)hw);
        return hipGetLastError();
    }
    // slabs of 1024 frames, workspace laid out as the generic path lays it out for the full h x w (crops are never larger)
    const int64_t slab = 1024;
    for (int64_t f0 = 0; f0 < n; f0 += slab) {
        const int64_t m = (n - f0) < slab ? (n - f0) : slab;
        const size_t cnt = (size_t)(n < slab ? n : slab);
        float* buf1 = d_ws;                 // [m] x [ww][hh]
        float* buf2 = d_ws + cnt * hw;      // [m] x [hh][ww]
        float* buf3 = d_ws + 2 * cnt * hw;  // [m] x [64][hh]
        const uint8_t* src = d_frames + (size_t)f0 * hw * channels;
        const int4* gs = geom + f0;
        dim3 g1((h + 63) / 64, (unsigned)m), g2((w + 63) / 64, (unsigned)m), g4(1, (unsigned)m);
        if (channels == 3)
            hipLaunchKernelGGL((k_box_scan_rect<3, 1>), g1, dim3(64), 0, s, (const void*)src, buf1, gs, w, (long long)hw * 3,
                               (long long)hw);
        else
            hipLaunchKernelGGL((k_box_scan_rect<1, 1>), g1, dim3(64), 0, s, (const void*)src, buf1, gs, w, (long long)hw,
                               (long long)hw);
        hipLaunchKernelGGL((k_box_scan_rect<0, 2>), g2, dim3(64), 0, s, (const void*)buf1, buf2, gs, w, (long long)hw,
                           (long long)hw);
        hipLaunchKernelGGL((k_box_scan_rect<0, 3>), g1, dim3(64), 0, s, (const void*)buf2, buf3, gs, w, (long long)hw,
                           (long long)64 * h);
        hipLaunchKernelGGL((k_box_scan_rect<0, 4>), g4, dim3(64), 0, s, (const void*)buf3, d_out64 + (size_t)f0 * 4096, gs, w,
                           (long long)64 * h, (long long)4096);
        if (channels == 3)
            hipLaunchKernelGGL(k_luma64_rect<3>, dim3((unsigned)m), dim3(256), 0, s, src, d_out64 + (size_t)f0 * 4096, gs, w,
                               (long long)hw * 3);
        else
            hipLaunchKernelGGL(k_luma64_rect<1>, dim3((unsigned)m), dim3(256), 0, s, src, d_out64 + (size_t)f0 * 4096, gs, w,
                               (long long)hw);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace hvd
