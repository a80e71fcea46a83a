// hvd_rect_dev.h -- the fused rectangle down-sampler's per-frame body, one definition: k_autocrop_fused.hip (k_down_rect: one
// rectangle per frame from a table) and k_crops.hip (k_down_crops: every frame under a short call-uniform list of
// rectangles) include it and add their loops. Same recurrence, same operation order as the generic passes: the
// 64 x 64 planes are those of the oracle on the contiguous crop, bit for bit. Luma is hvd_pdq_dev.h's, the home of that contract.
// Every device function is __forceinline__: a kernel that calls them compiles to the code it had with the statements written out.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_pdq_dev.h"

namespace hvd {

namespace {

// The four passes of k_autocrop.hip's k_box_scan_rect in ONE launch, for frames with h <= 512 and w <= 512 ("fused
// rectangle down-sampler"). k_pdq.hip's k_down512 with the rectangle's origin, its sides and the two windows (1..4, one per axis) as
// run-time values: one workgroup of 512 lanes per frame, lane = row of the rectangle, strips of 32 filter steps along the row,
// the frame read from HBM once, every intermediate in LDS.
//   A  (lanes < hh, lane = row)   pass 1 along the row: step s = 32k + c consumes pixel s and leaves output s - lag in
//                                 buf[row][c] (lag = win / 2 = half - 1: an output trails its last input by that much)
//   B  (wave 0, lane = column c)  pass 2 down each buffer column, in place (the lagging operand lives in registers)
//   C  (all lanes, lane = row)    pass 3 along the row over the buffer columns; keeps only the columns the decimation
//                                 samples, cs[slot][row] (at most one per step: 32 slots)
//   D  (wave 1, lane = slot)      pass 4 down each sampled column of the strip before; keeps the 64 sampled rows ->
//                                 out64[frame][i][j]; runs while B walks the next strip
// The windows differ per frame, so every pass exists for windows 1..4 and a wave-uniform switch picks one: the ring of the
// last four inputs is then indexed statically and the steady-state divisor is a constant. A strip (a chunk of 8 steps in
// B / D) in which every step has its full window takes the branch-free form; the first and the last ones take the EDGE form,
// which is box1DFloat's recurrence step by step with its running divisor. Passes 3 and 4 only ever keep outputs with a full
// window: the first sample len >> 7 is at least win - 1 steps in, the last one, len - win, lies before the window shrinks.
// LDS: buf 512 x 33 + cs 32 x 513 floats = 133 248 bytes, so ONE workgroup per CU (8 waves, 2 per SIMD, <= 256 VGPRs).
// A rectangle of 64 columns has a sample in every step, hence the 32 slots; 4 slots (512 columns) would let two workgroups
// share a CU as k_down512<CH, 32> does, at the price of a kernel per width class.
constexpr int kRS = 32;            // filter steps per strip
constexpr int kRMax = 512;         // largest frame side the kernel takes
constexpr int kRBufLd = kRS + 1;
constexpr int kRCsLd = kRMax + 1;

template <int WIN>
__device__ __forceinline__ float box_scale(float sum) {  // the steady-state divisor: exact multiply for powers of two
    if (WIN == 3) return __fdiv_rn(sum, 3.0f);
    return __fmul_rn(sum, 1.0f / (float)WIN);
}

__device__ __forceinline__ float box_divide(float sum, int cur) {  // 1 <= cur <= 4, as k_box_scan_rect divides
    return cur == 3 ? __fdiv_rn(sum, 3.0f) : __fmul_rn(sum, cur == 1 ? 1.0f : cur == 2 ? 0.5f : 0.25f);
}

// divisor of step s of a line of len elements (len >= 64 > win): the window grows, is full, shrinks
__device__ __forceinline__ int box_cur(int win, int s, int len) { return s < win ? s + 1 : s < len ? win : win - (s - len + 1); }

// The last four inputs of a recurrence. The branch-free forms keep input s in slot s & 3 (static there: they start at a
// multiple of 4); the edge forms, rolled loops with the window at run time, shift them through d[0] = x[s - 1] ..
// d[3] = x[s - 4]. Both views agree wherever s is a multiple of 4: slot (-i) & 3 is x[s - i].
struct Ring4 {
    float d[4];
    __device__ __forceinline__ explicit Ring4(const float (&lag)[4]) : d{lag[3], lag[2], lag[1], lag[0]} {}
    __device__ __forceinline__ float back(int win) const { return win == 1 ? d[0] : win == 2 ? d[1] : win == 3 ? d[2] : d[3]; }
    __device__ __forceinline__ void push(float x) { d[3] = d[2]; d[2] = d[1]; d[1] = d[0]; d[0] = x; }
    __device__ __forceinline__ void store(float (&lag)[4]) const { lag[3] = d[0]; lag[2] = d[1]; lag[1] = d[2]; lag[0] = d[3]; }
};

// Pass A, steps s0 .. s0 + 31 of one row (s0 a multiple of 32): v[c] is pixel s0 + c, every step with its full window.
template <int WIN>
__device__ __forceinline__ void rect_pass_a(const float (&v)[kRS], float& sum, float (&lag)[4], float* __restrict__ brow) {
#pragma unroll
    for (int c = 0; c < kRS; ++c) {
        sum = __fadd_rn(sum, v[c]);
        sum = __fsub_rn(sum, lag[(c - WIN) & 3]);
        lag[c & 3] = v[c];
        brow[c] = box_scale<WIN>(sum);
    }
}

// The same for a strip in which some step lacks its full window (s < win, or s >= len: up to lag steps that consume nothing)
// or lies beyond the last step len + lag - 1: box1DFloat's recurrence step by step with its running divisor. The pixels are
// parked in the buffer row first, so that one rolled loop serves the four windows (the first and the last strips of a row
// only); step s reads column c before it writes output s - lag there. A value pushed at s >= len is never read back.
__device__ __forceinline__ void rect_edge_a(const float (&v)[kRS], int win, int s0, int len, float& sum, float (&lag)[4],
                                            float* brow) {
#pragma unroll
    for (int c = 0; c < kRS; ++c) brow[c] = v[c];
    const int lg = win >> 1;
    Ring4 r(lag);
#pragma unroll 1
    for (int c = 0; c < kRS; ++c) {
        const int s = s0 + c;
        const float x = brow[c];
        if (s < len) sum = __fadd_rn(sum, x);
        if (s >= win && s < len + lg) sum = __fsub_rn(sum, r.back(win));
        r.push(x);
        if (s >= lg && s < len + lg) brow[c] = box_divide(sum, box_cur(win, s, len));
    }
    r.store(lag);
}

// Pass C over the buffer columns of strip k: column c is pass 3's input t = 32k + c - lag (ring slot c & 3), its output
// t - lag is kept iff it is the next decimation sample ((2j + 1) * len) >> 7. The bookkeeping is the same in every lane.
// This form: k >= 1 and all 32 columns hold a value.
template <int WIN>
__device__ __forceinline__ void rect_pass_c(const float* __restrict__ brow, int k, int len, float& sum, float (&lag)[4],
                                            int& next_j, int& next_sel, int& slot, float* __restrict__ csy) {
    constexpr int LAG = WIN / 2;
#pragma unroll
    for (int c = 0; c < kRS; ++c) {
        const float x = brow[c];
        sum = __fadd_rn(sum, x);
        sum = __fsub_rn(sum, lag[(c - WIN) & 3]);
        lag[c & 3] = x;
        if (kRS * k + c - 2 * LAG == next_sel && next_j < 64) {
            csy[slot * kRCsLd] = box_scale<WIN>(sum);
            ++slot;
            ++next_j;
            next_sel = ((2 * next_j + 1) * len) >> 7;
        }
    }
}

// ... and the first / last strips: columns [c_lo, c_hi), the window still growing in strip 0 (c_lo = lag there, and the
// ring is shifted by c_lo so that it stands where a strip that began at column 0 would have left it).
__device__ __forceinline__ void rect_edge_c(const float* __restrict__ brow, int win, int k, int c_lo, int c_hi, int len,
                                            float& sum, float (&lag)[4], int& next_j, int& next_sel, int& slot,
                                            float* __restrict__ csy) {
    const int lg = win >> 1;
    Ring4 r(lag);
#pragma unroll 1
    for (int c = c_lo; c < kRS; ++c) {
        const float x = c < c_hi ? brow[c] : 0.0f;
        if (c < c_hi) {
            const int t = kRS * k + c - lg;
            sum = __fadd_rn(sum, x);
            if (t >= win) sum = __fsub_rn(sum, r.back(win));
            if (t - lg == next_sel && next_j < 64) {
                csy[slot * kRCsLd] = box_divide(sum, win);
                ++slot;
                ++next_j;
                next_sel = ((2 * next_j + 1) * len) >> 7;
            }
        }
        r.push(x);
    }
    r.store(lag);
}

// Eight branch-free steps s0 .. s0 + 7 (s0 a multiple of 8) of a column pass with the inputs in x[]. INPLACE (pass B): output
// s - lag goes back to the column; otherwise (pass D) only the decimation samples go to dst[i * 64 + j].
template <int WIN, bool INPLACE>
__device__ __forceinline__ void rect_col_chunk(const float (&x)[8], int s0, int len, float& sum, float (&lag)[4], float* col,
                                               int stride, float* __restrict__ dst, int j, int& next_i, int& next_sel) {
    constexpr int LAG = WIN / 2;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sum = __fadd_rn(sum, x[e]);
        sum = __fsub_rn(sum, lag[(e - WIN) & 3]);
        lag[e & 3] = x[e];
        o[e] = box_scale<WIN>(sum);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int oi = s0 + e - LAG;
        if (INPLACE) {
            col[oi * stride] = o[e];
        } else if (oi == next_sel && next_i < 64) {
            dst[next_i * 64 + j] = o[e];
            ++next_i;
            next_sel = ((2 * next_i + 1) * len) >> 7;
        }
    }
}

// Steps [s_lo, s_hi) of a column pass one by one (s_lo a multiple of 4): the head, where the window grows, and the tail,
// the last len % 8 elements and the lag steps behind them. The next input is read before an output is written.
template <bool INPLACE>
__device__ __forceinline__ void rect_col_edge(int win, int s_lo, int s_hi, int len, float& sum, float (&lag)[4], float* col,
                                              int stride, float* __restrict__ dst, int j, int& next_i, int& next_sel) {
    const int lg = win >> 1;
    Ring4 r(lag);
    float x = s_lo < len ? col[s_lo * stride] : 0.0f;
#pragma unroll 1
    for (int s = s_lo; s < s_hi; ++s) {
        const float xn = s + 1 < len ? col[(s + 1) * stride] : 0.0f;
        if (s < len) sum = __fadd_rn(sum, x);
        if (s >= win) sum = __fsub_rn(sum, r.back(win));
        r.push(x);
        const int oi = s - lg;
        if (oi >= 0) {
            const float o = box_divide(sum, box_cur(win, s, len));
            if (INPLACE) {
                col[oi * stride] = o;
            } else if (oi == next_sel && next_i < 64) {
                dst[next_i * 64 + j] = o;
                ++next_i;
                next_sel = ((2 * next_i + 1) * len) >> 7;
            }
        }
        x = xn;
    }
    r.store(lag);
}

// One column pass (B or D) over len elements at col[0], col[stride], ...: a lone lane's sequential recurrence, the next eight
// inputs always in flight. An in-place output lands at most at the row just read, never ahead of it.
template <int WIN, bool INPLACE>
__device__ __forceinline__ void rect_col_pass(float* col, int stride, int len, float* __restrict__ dst, int j) {
    constexpr int LAG = WIN / 2;
    float sum = 0.0f, lag[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int next_i = 0, next_sel = len >> 7;
    rect_col_edge<INPLACE>(WIN, 0, 8, len, sum, lag, col, stride, dst, j, next_i, next_sel);
    float a[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = col[(8 + e) * stride];
    int s0 = 8;  // a[] holds rows s0 .. s0 + 7, all of them inside the column (len >= 64)
#pragma unroll 2
    for (; s0 + 16 <= len; s0 += 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] = col[(s0 + 8 + e) * stride];
        rect_col_chunk<WIN, INPLACE>(a, s0, len, sum, lag, col, stride, dst, j, next_i, next_sel);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = b[e];
    }
    rect_col_chunk<WIN, INPLACE>(a, s0, len, sum, lag, col, stride, dst, j, next_i, next_sel);
    rect_col_edge<INPLACE>(WIN, s0 + 8, len + LAG, len, sum, lag, col, stride, dst, j, next_i, next_sel);
}

template <bool INPLACE>
__device__ __forceinline__ void rect_col_pass_win(int win, float* col, int stride, int len, float* __restrict__ dst, int j) {
    switch (win) {
        case 1: rect_col_pass<1, INPLACE>(col, stride, len, dst, j); break;
        case 2: rect_col_pass<2, INPLACE>(col, stride, len, dst, j); break;
        case 3: rect_col_pass<3, INPLACE>(col, stride, len, dst, j); break;
        default: rect_col_pass<4, INPLACE>(col, stride, len, dst, j); break;
    }
}

// The 32 pixels of a strip as aligned 32-bit words: q[i] is the word at (p & ~3) + 4i, or, past the row's last byte, that
// last byte's word again (a pixel beyond the row is never used), so that nothing outside the words that hold the frames'
// bytes is touched and no load is predicated. A rectangle's left edge is at any byte address; rect_strip_luma shifts the
// lead (p & 3) bytes out. full: all 32 pixels lie inside the row, so only the word behind them can lie outside.
template <int CH>
struct RectRaw {
    static constexpr int NW = kRS * CH / 4;
    uint32_t q[NW + 1];
};

template <int CH>
__device__ __forceinline__ void rect_load_raw(const uint8_t* p, const uint8_t* row_end, bool full, RectRaw<CH>& raw) {
    constexpr int NW = RectRaw<CH>::NW;
    const uint8_t* a = p - ((uintptr_t)p & 3u);
    const int last = (int)((row_end - 1 - a) & ~(ptrdiff_t)3);  // >= 0: p itself is a pixel of the row
    if (full) {
#pragma unroll
        for (int i = 0; i < NW; ++i) raw.q[i] = reinterpret_cast<const uint32_t*>(a)[i];
        raw.q[NW] = *reinterpret_cast<const uint32_t*>(a + min(4 * NW, last));
    } else {
#pragma unroll
        for (int i = 0; i <= NW; ++i) raw.q[i] = *reinterpret_cast<const uint32_t*>(a + min(4 * i, last));
    }
}

template <int CH>
__device__ __forceinline__ void rect_strip_luma(const RectRaw<CH>& raw, uint32_t lead, float (&v)[kRS]) {
    constexpr int NW = RectRaw<CH>::NW;
    uint32_t wd[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i)
        wd[i] = (uint32_t)((((unsigned long long)raw.q[i + 1] << 32) | raw.q[i]) >> (8 * lead));
#pragma unroll
    for (int c = 0; c < kRS; ++c) {
        if (CH == 3) {
            const int b0 = 3 * c, b1 = 3 * c + 1, b2 = 3 * c + 2;
            v[c] = luma_rgb((float)byte_of(wd[b0 >> 2], b0 & 3), (float)byte_of(wd[b1 >> 2], b1 & 3),
                            (float)byte_of(wd[b2 >> 2], b2 & 3));
        } else {
            v[c] = luma_gray(byte_of(wd[c >> 2], c & 3));
        }
    }
}

// The plane of ONE rectangle {top, left, hh, ww} of frame f (inside the frame, both sides in [64, 512], not 64 x 64: that one is
// the crop's unfiltered luma) -> plane number `plane` of out64. Called by all 512 lanes of the workgroup with wave-uniform arguments; buf and cs are
// the workgroup's LDS (133 248 bytes), free again when the call returns (it ends on a barrier).
template <int CH>
__device__ __forceinline__ void rect_frame_plane(const uint8_t* frames, long long f, int h, int w, int top, int left,
                                                 int hh, int ww, float* out64, size_t plane, float (&buf)[kRMax][kRBufLd],
                                                 float (&cs)[kRS][kRCsLd], int y, int wave, int lane) {
    const int wx = (ww + 127) >> 7, wy = (hh + 127) >> 7;
    const int lagx = wx >> 1;
    const int nst = (ww + lagx + kRS - 1) / kRS;  // strips of 32 steps that hold the ww + lagx steps of a row
    const bool active = y < hh;
    const uint8_t* row = frames + ((size_t)f * h * w + (size_t)(top + (active ? y : 0)) * w + left) * CH;
    const uint8_t* row_end = row + (size_t)ww * CH;
    const uint32_t lead = (uint32_t)((uintptr_t)row & 3u);  // kRS * CH is a multiple of 4: the same in every strip
    float* dst = out64 + plane * 4096;
    float sA = 0.0f, lagA[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float sC = 0.0f, lagC[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int next_j = 0, next_sel = ww >> 7;  // pass 3's next sample
    int d_j0 = 0, d_cnt = 0;             // what pass C left in cs for pass D: samples d_j0 .. d_j0 + d_cnt - 1
    RectRaw<CH> raw;
    if (active) rect_load_raw<CH>(row, row_end, kRS <= ww, raw);

#pragma unroll 1
    for (int k = 0; k < nst; ++k) {
        const int s0 = kRS * k;
        // ---------------- A ----------------
        if (active) {
            float v[kRS];
            rect_strip_luma<CH>(raw, lead, v);
            if (s0 + kRS < ww)  // in flight during B / C of this strip
                rect_load_raw<CH>(row + (size_t)(s0 + kRS) * CH, row_end, s0 + 2 * kRS <= ww, raw);
            const bool edge = k == 0 || s0 + kRS > ww;
            float* brow = buf[y];
            if (edge) {
                rect_edge_a(v, wx, s0, ww, sA, lagA, brow);
            } else {
                switch (wx) {
                    case 1: rect_pass_a<1>(v, sA, lagA, brow); break;
                    case 2: rect_pass_a<2>(v, sA, lagA, brow); break;
                    case 3: rect_pass_a<3>(v, sA, lagA, brow); break;
                    default: rect_pass_a<4>(v, sA, lagA, brow); break;
                }
            }
        }
        __syncthreads();

        // ---------------- B: down the buffer columns (in place) ‖ D of the strip before ----------------
        const int c_lo = k == 0 ? lagx : 0;
        const int c_hi = min(kRS, ww + lagx - s0);
        if (wave == 0) {
            if (lane >= c_lo && lane < c_hi) rect_col_pass_win<true>(wy, &buf[0][lane], kRBufLd, hh, nullptr, 0);
        } else if (wave == 1) {
            if (lane < d_cnt) rect_col_pass_win<false>(wy, cs[lane], 1, hh, dst, d_j0 + lane);
        }
        __syncthreads();

        // ---------------- C: along the row over the buffer columns (every lane: rows beyond hh feed nothing) ----
        {
            d_j0 = next_j;
            int slot = 0;
            const bool edge = k == 0 || c_hi < kRS;
            const float* brow = buf[y];
            float* csy = &cs[0][y];
            if (edge) {
                rect_edge_c(brow, wx, k, c_lo, c_hi, ww, sC, lagC, next_j, next_sel, slot, csy);
            } else {
                switch (wx) {
                    case 1: rect_pass_c<1>(brow, k, ww, sC, lagC, next_j, next_sel, slot, csy); break;
                    case 2: rect_pass_c<2>(brow, k, ww, sC, lagC, next_j, next_sel, slot, csy); break;
                    case 3: rect_pass_c<3>(brow, k, ww, sC, lagC, next_j, next_sel, slot, csy); break;
                    default: rect_pass_c<4>(brow, k, ww, sC, lagC, next_j, next_sel, slot, csy); break;
                }
            }
            d_cnt = slot;
        }
        __syncthreads();
    }

    // D for the last strip's samples
    if (wave == 1 && lane < d_cnt) rect_col_pass_win<false>(wy, cs[lane], 1, hh, dst, d_j0 + lane);
    __syncthreads();  // cs / buf are reused by the next rectangle
}

}  // namespace

}  // namespace hvd
