// k_detail.hip -- detail content rectangle: the content rectangle of k_autocrop.hip for bars that have no one
// colour (blurred pillars, gradients) -- what tells them from picture is that they are smooth.
//
// The rule (integers only), parameters detail_level L and min_detail m:
//   dh(y, x) = max_k |p[y][x][k] - p[y][x+1][k]| > L   (x in [0, w-2]);  ROW y is content iff #{x : dh(y, x)} >= m
//   dv(y, x) = max_k |p[y][x][k] - p[y+1][x][k]| > L   (y in [0, h-2]);  COLUMN x is content iff #{y : dv(y, x)} >= m
// Rows count horizontal differences only and columns vertical ones only, so the step between a bar and the picture never
// lands on a bar row or a bar column. Frame box, video box and the per-axis fallback below 64 are DESIGN 4.7's.
//
//   k_content_rect_detail   one workgroup per frame: dh counts per row, dv counts per column, frame box -> atomicMin / atomicMax
// The rectangle accumulators are initialised and closed by k_autocrop.hip's k_rect_init / k_rect_finish, and everything
// behind the rectangle is shared as it is. The lane layout, the count folds and the closing step are
// hvd_content_rect_dev.h's, shared with the other two rules' fold; the band walk and the pixel pairs are this file's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "hvd_content_rect_dev.h"
#include "hvd_kernels.h"

namespace hvd {

namespace {

// |a - b| of two bytes held in 32-bit registers: one v_sad_u32
__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return __usad(a, b, 0u); }

// A lane's 16-pixel unit of one row as 4 * CH packed dwords.
template <int CH>
struct Unit {
    uint32_t q[4 * CH];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < 4 * CH; ++i) q[i] = 0;
    }
    // byte k of pixel p (p in [0, 16))
    __device__ __forceinline__ uint32_t at(int p, int k) const { return byte_of(q[(CH * p + k) >> 2], (CH * p + k) & 3); }
};

// row: the unit's first byte; npix: pixels of the row from there on (> 0). The byte form reads pixel min(p, npix - 1) for pixel p:
// past the row's end the last pixel repeats, so a horizontal pair there differs by 0 and needs no gate.
template <int CH, bool WIDE>
__device__ __forceinline__ void load_unit(Unit<CH>& u, const uint8_t* __restrict__ row, int npix) {
    if (WIDE) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint4 t = reinterpret_cast<const uint4*>(row)[c];
            u.q[4 * c] = t.x; u.q[4 * c + 1] = t.y; u.q[4 * c + 2] = t.z; u.q[4 * c + 3] = t.w;
        }
    } else {
        u.clear();
#pragma unroll
        for (int p = 0; p < kUnit; ++p) {
            const uint8_t* px = row + min(p, npix - 1) * CH;
#pragma unroll
            for (int k = 0; k < CH; ++k) u.q[(CH * p + k) >> 2] |= (uint32_t)px[k] << (8 * ((CH * p + k) & 3));
        }
    }
}

// max_k |a_k - b_k| > level of pixel pa of A against pixel pb of B
template <int CH>
__device__ __forceinline__ bool differs(const Unit<CH>& A, int pa, const Unit<CH>& B, int pb, uint32_t level) {
    if (CH == 1) return absdiff(A.at(pa, 0), B.at(pb, 0)) > level;
    return max(max(absdiff(A.at(pa, 0), B.at(pb, 0)), absdiff(A.at(pa, 1), B.at(pb, 1))), absdiff(A.at(pa, 2), B.at(pb, 2))) > level;
}

// Detail counts per row and per column of one frame, one workgroup of 256 lanes per frame. The lanes form R = 256 / P lane-rows
// of P = pow2 >= ceil(w / 16) lanes, as in k_content_rect; lane-row r takes the BAND of rows [r * B, r * B + B), B = ceil(h / R),
// and lane (r, u) pixels [16u, 16u + 16) of them. Every frame byte comes from HBM once, plus one row per band:
//   vertical    the band is walked top down with the row below read one step ahead; it becomes the current row in registers.
//               The band's last step reads the first row of the next band (the extra row) for dv of its last row.
//   horizontal  pixel 16u + 16 is the first pixel of lane u + 1's unit: its first dword, taken by a lane shuffle. Lane 63 of a
//               wave has no such neighbour: where the row goes on (w > 1024) it loads the CH bytes. A lane-row's last lane
//               (u = P - 1) never needs the pixel: 16 P >= w.
// A lane keeps the 16 dv counts of its columns in registers for the whole band and folds them into LDS once; a row's dh count
// is a segmented wave reduction folded into LDS.
// WIDE: w % 16 == 0 and the frame base is 16-byte aligned, so every unit is CH aligned 16-byte loads; otherwise byte loads.
// LDS: int rowcnt[h], colcnt[w] (dynamic), 4 words of box.
template <int CH, bool WIDE>
__global__ __launch_bounds__(256) void k_content_rect_detail(const uint8_t* __restrict__ frames, int h, int w,
                                                             const long long* __restrict__ offsets, int V, int detail_level,
                                                             int min_detail, int32_t* __restrict__ boxes) {
    extern __shared__ int lds[];
    int* rowcnt = lds;
    int* colcnt = lds + h;
    __shared__ int box[4];
    const int tid = threadIdx.x;
    const long long frame = blockIdx.x;
    const uint8_t* src = frames + (size_t)frame * h * w * CH;
    const uint32_t level = (uint32_t)detail_level;
    rect_counts_clear(lds, box, h, w, tid);

    const RectLanes L(w, tid);
    const int lg = __ffs(L.P) - 1;    // P = 1 << lg: shifts, no division
    const int R = 256 >> lg;
    const int B = (h + R - 1) >> (8 - lg);
    const int r0 = tid >> lg;
    const int x0 = L.x0;
    const bool live = L.live;
    const int npix = w - x0;                   // pixels of a row from the unit's first on (live: > 0)
    const bool more = x0 + kUnit < w;          // pixel x0 + 16 exists
    const bool edge = more && (tid & 63) == 63;  // ... in another wave

    int cnt[kUnit];
#pragma unroll
    for (int p = 0; p < kUnit; ++p) cnt[p] = 0;

    Unit<CH> cur, nxt;
    cur.clear();
    const int y0 = r0 * B;
    if (live && y0 < h) load_unit<CH, WIDE>(cur, src + ((size_t)y0 * w + x0) * CH, npix);

    for (int i = 0; i < B; ++i) {
        const int y = y0 + i;
        const bool below = live && y + 1 < h;  // (y + 1 < h implies y < h)
        if (below) load_unit<CH, WIDE>(nxt, src + ((size_t)(y + 1) * w + x0) * CH, npix);
        else nxt = cur;                        // no row below: no vertical difference
        // pixel x0 + 16 of row y: every lane shuffles (the lanes of a wave take this step together)
        Unit<CH> nb;
        nb.clear();
        nb.q[0] = __shfl_down(cur.q[0], 1);
        if (edge && y < h) {
            const uint8_t* px = src + ((size_t)y * w + x0 + kUnit) * CH;
            uint32_t d = 0;
#pragma unroll
            for (int k = 0; k < CH; ++k) d |= (uint32_t)px[k] << (8 * k);
            nb.q[0] = d;
        }
        int rc = 0;
#pragma unroll
        for (int p = 0; p < kUnit; ++p) {
            // dh(y, x0 + p). Inside the unit a pair past the row's end differs by 0 (load_unit; a dead lane holds zeros); the
            // pair with the next unit is gated. A step past the frame's last row counts into rc, which is then not folded.
            bool bh = p + 1 < kUnit ? differs<CH>(cur, p, cur, p + 1, level) : (differs<CH>(cur, p, nb, 0, level) && more);
            rc += bh ? 1 : 0;
            // dv(y, x0 + p); the counts of columns past the row's end are dropped at the fold
            bool bv = differs<CH>(cur, p, nxt, p, level);
            cnt[p] += bv ? 1 : 0;
        }
        rect_fold_row(rowcnt, L, tid, y, h, rc);
        cur = nxt;
    }
    rect_fold_columns(colcnt, L, w, cnt);
    rect_close(rowcnt, colcnt, box, h, w, tid, min_detail, boxes, [&] { return video_of_frame(offsets, V, frame); });
}

}  // namespace

// the detail rule's fold (launch_rect_fold, k_autocrop.hip)
hipError_t rect_fold_detail(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets, uint32_t V,
                            int detail_level, int min_detail, int32_t* d_rects, hipStream_t s) {
    return rect_fold_dispatch(d_frames, n, h, w, channels, [&](auto ch, auto wide, dim3 grid, size_t lds) {
        hipLaunchKernelGGL((k_content_rect_detail<decltype(ch)::value, decltype(wide)::value>), grid, dim3(256), lds, s, d_frames, h,
                           w, d_offsets, (int)V, detail_level, min_detail, d_rects);
    });
}

}  // namespace hvd
