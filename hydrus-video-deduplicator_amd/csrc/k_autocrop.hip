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

constexpr int kUnit = 16;  // pixels a lane takes from a row: 16 B of gray, 48 B of RGB24 = whole 16-byte loads

// Bright pixels per row and per column of one frame, one workgroup of 256 lanes per frame. The lanes form R = 256 / P rows of
// P = pow2 >= ceil(w / 16) lanes; lane (r, u) reads pixels [16u, 16u + 16) of rows r, r + R, ... and keeps the 16 column counts
// of its unit in registers for the whole frame. A row's count is a segmented wave reduction (P <= 64: the row lies inside one
// wave) folded into LDS; the column counts are folded into LDS once per frame.
// WIDE: w % 16 == 0 and the frame base is 16-byte aligned, so every unit is CH aligned 16-byte loads (the geometries users
// have: 64, 512, 640, 1920, ...); otherwise byte loads (any width, any alignment).
// LDS: int rowcnt[h], colcnt[w] (dynamic), 4 words of box.
template <int CH, bool WIDE>
__global__ __launch_bounds__(256) void k_content_rect(const uint8_t* __restrict__ frames, int h, int w,
                                                      const long long* __restrict__ offsets, int V, int black_level,
                                                      int min_bright, int32_t* __restrict__ boxes) {
    extern __shared__ int lds[];
    int* rowcnt = lds;
    int* colcnt = lds + h;
    __shared__ int box[4];
    const int tid = threadIdx.x;
    const long long frame = blockIdx.x;
    const uint8_t* src = frames + (size_t)frame * h * w * CH;
    const uint32_t level = (uint32_t)black_level;

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
                        b = byte_of(q[p >> 2], p & 3) > level;
                    } else {
                        const int e = 3 * p;
                        b = max(max(byte_of(q[e >> 2], e & 3), byte_of(q[(e + 1) >> 2], (e + 1) & 3)),
                                byte_of(q[(e + 2) >> 2], (e + 2) & 3)) > level;
                    }
                    cnt[p] += b ? 1 : 0;
                    rc += b ? 1 : 0;
                }
            } else {
#pragma unroll
                for (int p = 0; p < kUnit; ++p) {
                    bool b = false;
                    if (x0 + p < w) {
                        if (CH == 1) b = (uint32_t)row[p] > level;
                        else b = max(max((uint32_t)row[3 * p], (uint32_t)row[3 * p + 1]), (uint32_t)row[3 * p + 2]) > level;
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
        int32_t* vb = boxes + 4 * (size_t)video_of_frame(offsets, V, frame);
        atomicMin(&vb[0], box[0]);
        atomicMax(&vb[1], box[1]);
        atomicMin(&vb[2], box[2]);
        atomicMax(&vb[3], box[3]);
    }
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

hipError_t launch_content_rects(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets,
                                uint32_t V, int black_level, int min_bright, int32_t* d_rects, hipStream_t s) {
    if (V == 0) return hipSuccess;
    hipError_t e = launch_rect_init(d_rects, V, s);
    if (e == hipSuccess) e = launch_rect_fold(d_frames, n, h, w, channels, d_offsets, V, black_level, min_bright, d_rects, s);
    if (e == hipSuccess) e = launch_rect_finish(d_rects, V, h, w, s);
    return e;
}

// The three steps of launch_content_rects one by one, for a caller that folds a video's frames batch by batch (the streaming
// hasher): init once, fold every batch (the atomicMin / atomicMax merge is order-free), finish once.
hipError_t launch_rect_init(int32_t* d_rects, uint32_t V, hipStream_t s) {
    hipLaunchKernelGGL(k_rect_init, dim3((V + 255) / 256), dim3(256), 0, s, d_rects, (int)V);
    return hipGetLastError();
}

hipError_t launch_rect_fold(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets,
                            uint32_t V, int black_level, int min_bright, int32_t* d_rects, hipStream_t s) {
    // 64 x 64 frames: no box can be smaller than the frame and at least 64 long, so every rectangle is the full frame
    if (n <= 0 || (h == 64 && w == 64)) return hipSuccess;
    const size_t lds = sizeof(int) * (size_t)(h + w);
    const bool wide = (w % kUnit) == 0 && ((uintptr_t)d_frames & 15u) == 0;
    const dim3 gf((unsigned)n);
#define HVD_CR(CH, WIDE) hipLaunchKernelGGL((k_content_rect<CH, WIDE>), gf, dim3(256), lds, s, d_frames, h, w, d_offsets, (int)V, black_level, min_bright, d_rects)
    if (channels == 3) {
        if (wide) HVD_CR(3, true);
        else HVD_CR(3, false);
    } else {
        if (wide) HVD_CR(1, true);
        else HVD_CR(1, false);
    }
#undef HVD_CR
    return hipGetLastError();
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
