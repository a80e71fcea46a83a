// hvd_content_rect_dev.h -- what the three content-rectangle folds share, one definition of each piece: k_autocrop.hip (the black
// rule), k_barcolor.hip (the bar-colour rule) and k_detail.hip (the detail rule) include
// it and add what tells a rule from the others: which pixels (or pixel pairs) count. (hvd_rect_dev.h is another header: the
// fused down-sampler's.)
//
// The shape of a fold: one workgroup of 256 lanes per frame. The lanes form lane-rows of P = pow2 >= ceil(w / 16) lanes; lane
// (r, u) reads pixels [16u, 16u + 16) of its rows and keeps the 16 column counts of its unit in registers. A row's count is a
// segmented wave reduction (P <= 64: the row lies inside one wave) folded into LDS; the column counts are folded into LDS
// once per frame. Rows and columns with >= min_count counted pixels are content; their bounding box is the frame's box, merged
// into the video's by atomicMin / atomicMax. LDS: int rowcnt[h], colcnt[w] (dynamic), 4 words of box (static, in the kernel).
// WIDE: w % 16 == 0 and the frame base is 16-byte aligned, so every unit is CH aligned 16-byte loads (the geometries users
// have: 64, 512, 640, 1920, ...); otherwise byte loads (any width, any alignment).
// Every device function is __forceinline__: a kernel that calls them compiles to the code it has with the statements written out.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <type_traits>

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

constexpr int kUnit = 16;  // pixels a lane takes from a row: 16 B of gray, 48 B of RGB24 = whole 16-byte loads

// Where a lane stands in its lane-row. The lane-row's index and the rows it takes are the kernel's own (k_content_rect_fold
// strides the rows, k_content_rect_detail walks a band of them).
struct RectLanes {
    int units, P, u, x0, seg;
    bool live;
    __device__ __forceinline__ RectLanes(int w, int tid) {
        units = (w + kUnit - 1) / kUnit;
        P = 1;
        while (P < units) P <<= 1;  // <= 256 (w <= 4096)
        u = tid & (P - 1);
        x0 = u * kUnit;
        live = u < units;
        seg = P < 64 ? P : 64;  // lanes of one row are P consecutive lanes: a segment of the wave, or whole waves
    }
};

// lds = rowcnt[h] | colcnt[w], all zero; no box yet
__device__ __forceinline__ void rect_counts_clear(int* lds, int* box, int h, int w, int tid) {
    for (int i = tid; i < h + w; i += 256) lds[i] = 0;
    if (tid == 0) { box[0] = INT_MAX; box[1] = -1; box[2] = INT_MAX; box[3] = -1; }
    __syncthreads();
}

// rc: what this lane counted in row y. Every lane of the wave takes this step (a lane past the frame's last row with rc of any
// value: it is not folded).
__device__ __forceinline__ void rect_fold_row(int* rowcnt, const RectLanes& L, int tid, int y, int h, int rc) {
    for (int m = L.seg >> 1; m > 0; m >>= 1) rc += __shfl_xor(rc, m);
    if ((tid & (L.seg - 1)) == 0 && y < h && rc) atomicAdd(&rowcnt[y], rc);
}

// cnt: what this lane counted in the 16 columns of its unit, over all its rows
__device__ __forceinline__ void rect_fold_columns(int* colcnt, const RectLanes& L, int w, const int (&cnt)[kUnit]) {
    if (L.live) {
#pragma unroll
        for (int p = 0; p < kUnit; ++p)
            if (cnt[p] && L.x0 + p < w) atomicAdd(&colcnt[L.x0 + p], cnt[p]);
    }
}

// counts -> the frame's box -> the video's box. video_of(): the frame's video, asked by one lane and only if there is a box.
template <class VideoOf>
__device__ __forceinline__ void rect_close(const int* rowcnt, const int* colcnt, int* box, int h, int w, int tid, int min_count,
                                           int32_t* __restrict__ boxes, VideoOf video_of) {
    __syncthreads();
    int top = INT_MAX, bot = -1, left = INT_MAX, right = -1;
    for (int y = tid; y < h; y += 256)
        if (rowcnt[y] >= min_count) { top = min(top, y); bot = max(bot, y); }
    for (int x = tid; x < w; x += 256)
        if (colcnt[x] >= min_count) { left = min(left, x); right = max(right, x); }
    if (bot >= 0) { atomicMin(&box[0], top); atomicMax(&box[1], bot); }
    if (right >= 0) { atomicMin(&box[2], left); atomicMax(&box[3], right); }
    __syncthreads();
    if (tid == 0 && box[1] >= 0 && box[3] >= 0) {
        int32_t* vb = boxes + 4 * (size_t)video_of();
        atomicMin(&vb[0], box[0]);
        atomicMax(&vb[1], box[1]);
        atomicMin(&vb[2], box[2]);
        atomicMax(&vb[3], box[3]);
    }
}

// The fold of a rule that counts single pixels (black, bar colour): pred.gray(p) / pred.rgb(a, b, c) says whether a pixel
// counts. The lanes form R = 256 / P lane-rows; lane (r, u) takes rows r, r + R, ...
template <int CH, bool WIDE, class Pred, class VideoOf>
__device__ __forceinline__ void content_rect_fold(const uint8_t* __restrict__ src, int h, int w, const Pred& pred, int min_count,
                                                  int* lds, int* box, int32_t* __restrict__ boxes, VideoOf video_of) {
    int* rowcnt = lds;
    int* colcnt = lds + h;
    const int tid = threadIdx.x;
    rect_counts_clear(lds, box, h, w, tid);

    const RectLanes L(w, tid);
    const int R = 256 / L.P, r0 = tid / L.P;
    const int x0 = L.x0;

    int cnt[kUnit];
#pragma unroll
    for (int p = 0; p < kUnit; ++p) cnt[p] = 0;

    for (int yb = 0; yb < h; yb += R) {
        const int y = yb + r0;
        int rc = 0;
        if (L.live && y < h) {
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
        rect_fold_row(rowcnt, L, tid, y, h, rc);
    }
    rect_fold_columns(colcnt, L, w, cnt);
    rect_close(rowcnt, colcnt, box, h, w, tid, min_count, boxes, video_of);
}

// ---- host ----

// Launches the <CH, WIDE> form of a fold kernel that the frames call for: launch(ch, wide, grid, lds_bytes) with ch and wide
// std::integral_constant (decltype(ch)::value is the template argument). One workgroup per frame.
template <class Launch>
hipError_t rect_fold_dispatch(const uint8_t* d_frames, int64_t n, int h, int w, int channels, Launch launch) {
    // 64 x 64 frames: no box can be smaller than the frame and at least 64 long, so every rectangle is the full frame
    if (n <= 0 || (h == 64 && w == 64)) return hipSuccess;
    const size_t lds = sizeof(int) * (size_t)(h + w);
    const bool wide = (w % kUnit) == 0 && ((uintptr_t)d_frames & 15u) == 0;
    const dim3 grid((unsigned)n);
    using C1 = std::integral_constant<int, 1>;
    using C3 = std::integral_constant<int, 3>;
    if (channels == 3) {
        if (wide) launch(C3{}, std::true_type{}, grid, lds);
        else launch(C3{}, std::false_type{}, grid, lds);
    } else {
        if (wide) launch(C1{}, std::true_type{}, grid, lds);
        else launch(C1{}, std::false_type{}, grid, lds);
    }
    return hipGetLastError();
}

}  // namespace

}  // namespace hvd
