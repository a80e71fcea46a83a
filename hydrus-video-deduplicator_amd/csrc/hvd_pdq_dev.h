// hvd_pdq_dev.h -- the PDQ path's bit-exact device arithmetic, one definition of every step, shared by the kernel files
// that hash frames (k_pdq.hip, k_pdq_dihedral.hip) and that down-sample them (k_pdq.hip, k_autocrop.hip, k_autocrop_fused.hip).
//
// The contract (oracle/hvd_oracle.c): every float operation is a separately rounded binary32 operation in the oracle's
// order. Everything that must match is spelled __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn, which hipcc never contracts
// into an FMA. "This exact sequence of roundings" is what a front-end has to reproduce, so the sequences live here and
// nowhere else: a new front-end calls them, and a fix to a step touches one definition. Every function is
// __device__ __forceinline__: a kernel that calls them compiles to the code it had with the statements written out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- luma ---------------------------------------------------------------------------------------------------------------
// The oracle's order: y = 0.299 r; y += 0.587 g; y += 0.114 b, every step rounded.
__device__ __forceinline__ float luma_rgb(float r, float g, float b) {
    float y = __fmul_rn(0.299f, r);
    y = __fadd_rn(y, __fmul_rn(0.587f, g));
    y = __fadd_rn(y, __fmul_rn(0.114f, b));
    return y;
}

// A gray byte is r = g = b. (Not the identity: luma_gray(g) != float(g) for 35 of the 256 bytes, by 1 ulp.)
__device__ __forceinline__ float luma_gray(uint32_t g) {
    const float v = (float)g;
    return luma_rgb(v, v, v);
}

__device__ __forceinline__ uint32_t byte_of(uint32_t word, int i) { return (word >> (8 * i)) & 0xFFu; }

// ---- quality ------------------------------------------------------------------------------------------------------------
// |(int)(((u - v) * 100) / 255)| (pdqhashing.cpp quality metric) as a non-negative integer-valued
// float, WITHOUT the IEEE division (10+ VALU ops). The multiplier is the float just BELOW 1/255
// (RN(1/255) = 0x1.010102p-8 lies above the true value), so q = |x| * c stays below the true
// quotient even after its own rounding: trunc(q) is floor(|x|/255) or one less. The remainder
// r = |x| - 255*m is exact in one fma (|x| and 255*m are multiples of ulp(|x|) and close) and
// r >= 255 says when to add one. Equality with (int)(x / 255.0f) is checked for EVERY float
// |x| <= 26000 by tests/tools/check_div255.c (2.4e9 values, 0 mismatches); |x| <= 25500.01 here
// because luma and its box-filter averages never exceed 255.0001. The fma is this term's own
// exact-arithmetic device, not a contraction of reference arithmetic.
// The term is m + (r >= 255): the caller accumulates the m's as floats (exact: integers far below
// 2^24) and the corrections as an integer count (v_cmp + add-with-carry).
__device__ __forceinline__ void grad_term(float u, float v, float& acc_m, int& acc_c) {
    const float ax = fabsf(__fmul_rn(__fsub_rn(u, v), 100.0f));
    const float m = truncf(__fmul_rn(ax, 0x1.0101p-8f));
    const float r = __fmaf_rn(-255.0f, m, ax);
    acc_m += m;
    acc_c += (r >= 255.0f) ? 1 : 0;
}

// The same term for GRAY BYTE input in one multiply: there the operands are luma_gray(g) of a byte g, so (u, v) takes
// only 256 x 256 values, and for every one of them trunc(|u - v| * RN(100/255)) equals the reference's
// |(int)(((u - v) * 100) / 255)| -- checked exhaustively (tests/test_oracle.py::test_quality_term_gray_shortcut_is_exact
// on the host, test_k1_quality_all_byte_pairs on the GPU). 4 VALU ops per term instead of 8; the quality metric was a
// quarter of the hash kernel's instructions (profiles/r01_pmc_k1.txt). Float frames (the down-sampler's output) keep the
// general form above.
__device__ __forceinline__ void grad_term_gray(float u, float v, int& acc) {
    // (int)x IS the truncation (v_cvt_i32_f32 rounds toward zero); an explicit truncf in front of it cost one more VALU
    // instruction per term, 127 per frame (round 3)
    acc += (int)__fmul_rn(fabsf(__fsub_rn(u, v)), 0x1.919192p-2f /* RN(100/255) = 0x3EC8C8C9 */);
}

// Lane l reads lane l+1 of the whole 64-lane wave (lane 63 reads 0 and is ignored by callers): the DPP
// wave_shl:1 control of the GFX9 family, which folds into the consuming VALU instruction instead
// of a trip through the LDS crossbar (ds_bpermute).
__device__ __forceinline__ float wave_next_lane(float v) {
    const int x = __float_as_int(v);
    return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x130 /* wave_shl:1 */, 0xF, 0xF, true));
}

__device__ __forceinline__ float wave_sum_f32(float v) {  // exact: integer-valued, far below 2^24
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The clamped quality of the frame whose column `lane` is a[]: vertical gradients in-lane, horizontal ones via the
// neighbour lane, summed over the wave. KIND 0: a[] is luma_gray of bytes (the one-multiply term). KIND 1: any float luma.
template <int KIND>
__device__ __forceinline__ int pdq_quality(const float (&a)[64], int lane) {
    int gsum;
    if (KIND == 0) {
        int qs = 0, qh = 0;
#pragma unroll
        for (int k = 0; k < 63; ++k) grad_term_gray(a[k], a[k + 1], qs);
#pragma unroll
        for (int k = 0; k < 64; ++k) grad_term_gray(a[k], wave_next_lane(a[k]), qh);
        if (lane < 63) qs += qh;  // column 63 has no right neighbour
        gsum = (int)wave_sum_f32((float)qs);
    } else {
        float gs = 0.0f, gh = 0.0f;
        int cs_ = 0, ch_ = 0;
#pragma unroll
        for (int k = 0; k < 63; ++k) grad_term(a[k], a[k + 1], gs, cs_);
#pragma unroll
        for (int k = 0; k < 64; ++k) grad_term(a[k], wave_next_lane(a[k]), gh, ch_);
        if (lane < 63) {  // column 63 has no right neighbour
            gs += gh;
            cs_ += ch_;
        }
        gsum = (int)wave_sum_f32(gs + (float)cs_);
    }
    const int qual = gsum / 90;
    return qual > 100 ? 100 : qual;
}

// ---- the strict 16x16 DCT of a 64x64 frame: one wave64 per frame, kWaves frames per workgroup --------------------------
constexpr int kWaves = 4;  // frames in flight per workgroup
constexpr int kLd = 68;    // padded LDS row stride (floats): 272 B, 16-B aligned, bank-skewed

struct alignas(16) PdqLds {
    float T[kWaves][16][kLd];
    float D[16][kLd];
    float luma_lut[256];  // luma_gray(g) for every byte value
};

// T[wave] is private to its wave: wave-scope ordering is all a hand-over through it needs (LDS operations of one wave
// execute in order), so the waves of a workgroup -- independent frames -- never wait for each other.
__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Stage 0: column `lane` of frame f into a[]. KIND 0: uint8 gray 64x64 frames (luma from the LDS table). KIND 1: float
// 64x64 buffers (the down-samplers' output).
template <int KIND>
__device__ __forceinline__ void pdq_load_column(const PdqLds& lds, const void* __restrict__ in, long long f, int lane,
                                                float (&a)[64]) {
    if (KIND == 0) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(in) + f * 4096 + lane;
#pragma unroll
        for (int k = 0; k < 64; ++k) a[k] = lds.luma_lut[src[k * 64]];
    } else {
        const float* src = reinterpret_cast<const float*>(in) + f * 4096 + lane;
#pragma unroll
        for (int k = 0; k < 64; ++k) a[k] = src[k * 64];
    }
}

// Stage 2: B[i][j] = sum_k T[i][k] * D[j][k], k ascending, from the padded LDS. Lane l -> (i0 = l >> 4, j = l & 15),
// b[r] = B[i0 + 4r][j] = coefficient l + 64 r.
__device__ __forceinline__ void pdq_dct_stage2(const PdqLds& lds, int wave, int lane, float (&out)[4]) {
    const int j = lane & 15, i0 = lane >> 4;
    float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k4 = 0; k4 < 16; ++k4) {
        const float4 dv = *reinterpret_cast<const float4*>(&lds.D[j][4 * k4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 tv = *reinterpret_cast<const float4*>(&lds.T[wave][i0 + 4 * r][4 * k4]);
            b[r] = __fadd_rn(b[r], __fmul_rn(tv.x, dv.x));
            b[r] = __fadd_rn(b[r], __fmul_rn(tv.y, dv.y));
            b[r] = __fadd_rn(b[r], __fmul_rn(tv.z, dv.z));
            b[r] = __fadd_rn(b[r], __fmul_rn(tv.w, dv.w));
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = b[r];
}

// ---- median -------------------------------------------------------------------------------------------------------------
// 128th smallest of the wave's 256 values (4 per lane; Torben's result): a radix select over order-preserving keys with
// wave ballots.
__device__ __forceinline__ float wave_median256(const float (&b)[4]) {
    uint32_t key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t u = __float_as_uint(b[r]);
        key[r] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving
    }
    uint32_t prefix = 0, mask = 0;
    int kth = 128, remaining = 256;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t bsel = 1u << bit;
        const uint32_t m2 = mask | bsel;
        int cnt0 = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) cnt0 += __popcll(__ballot((key[r] & m2) == prefix));
        if (kth > cnt0) {
            kth -= cnt0;
            remaining -= cnt0;
            prefix |= bsel;
        } else {
            remaining = cnt0;
        }
        mask = m2;
        if (remaining == 1) break;  // a single key carries this prefix: it is the median
    }
    if (mask != 0xFFFFFFFFu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned long long bm = __ballot((key[r] & mask) == prefix);
            if (bm) prefix = __builtin_amdgcn_readlane(key[r], (int)__builtin_ctzll(bm));
        }
    }
    const uint32_t mu = (prefix & 0x80000000u) ? (prefix ^ 0x80000000u) : ~prefix;
    return __uint_as_float(mu);
}

// ---- the generic down-sampler's line pass ---------------------------------------------------------------------------------
constexpr int kTW = 32;         // columns per staged tile
constexpr int kRing = 2 * kTW;  // LDS ring (window <= 32 looks back at most one tile)

// Jarosz window of an axis of `dim` elements (upstream: computeJaroszFilterWindowSize(dim, 64)).
constexpr int jarosz_window(int dim) { return (dim + 2 * 64 - 1) / (2 * 64); }

// Upstream's sequential running-sum box filter (box1DFloat) along the lines of a row-major image, one lane per line. The
// launch shape is part of the pass: workgroup (x, y) of 64 lanes takes lines 64 x .. 64 x + 63 of frame y (read from the
// block index here, not passed in: as arguments they cost the callers 6 % more instructions and 4 - 6 VGPRs,
// profiles/r11_pdq_isa_diff.txt). The output goes out TRANSPOSED, [kept positions][lines]. The running sum
// makes the filter a sequential float recurrence, so the parallelism is across lines; the input is staged through an LDS
// ring with coalesced loads and the stores are coalesced across lanes. nsel != 0: only the nsel sample positions the
// decimation keeps are emitted (the recurrence still runs over every element).
// Input: frames in_frame_stride elements apart (bytes for SRC 3). Bytes (SRC 1, 3): element (ln, col) is
// pixel (oy + ln) * pitch + (ox + col), so a whole frame is pitch = len, oy = ox = 0 and a rectangle of it is the frame's
// pitch and the rectangle's origin. Floats (SRC 0) are the contiguous [lines][len] image a pass before wrote: ln * len + col.
template <int SRC>  // 0: float, 1: gray u8, 3: rgb24 (luma fused into the load)
__device__ __forceinline__ void box_scan_lines(const void* in, float* out, long long in_frame_stride,
                                               long long out_frame_stride, int pitch, int oy, int ox, int lines, int len,
                                               int win, int nsel) {
    const long long frame = blockIdx.y;
    const int line0 = blockIdx.x * 64;
    __shared__ float ring[64][kRing + 1];
    const int lane = threadIdx.x;
    const int my_line = line0 + lane;
    const int half = (win + 2) / 2;
    const int steps = len + half - 1;
    const int out_lines = lines;  // transposed output: [kept positions][lines]
    float* dst = out + frame * out_frame_stride;

    float sum = 0.0f;
    int cur = 0;
    int next_j = 0;
    int next_sel = nsel ? (int)(((0 + 0.5) * len) / 64) : 0;

    for (int s = 0; s < steps; ++s) {
        if (s < len && (s % kTW) == 0) {
            // stage columns [s, s+kTW) of the 64 lines into ring slot (s/kTW)&1
            __syncthreads();
            const int c = lane & (kTW - 1);
            const int col = s + c;
#pragma unroll 4
            for (int rr = lane / kTW; rr < 64; rr += 64 / kTW) {
                const int ln = line0 + rr;
                float v = 0.0f;
                if (ln < lines && col < len) {
                    if (SRC == 0) {
                        v = reinterpret_cast<const float*>(in)[frame * in_frame_stride + (long long)ln * len + col];
                    } else {
                        const long long e = (long long)(oy + ln) * pitch + (ox + col);
                        if (SRC == 1) {
                            v = luma_gray(reinterpret_cast<const uint8_t*>(in)[frame * in_frame_stride + e]);
                        } else {
                            const uint8_t* p = reinterpret_cast<const uint8_t*>(in) + frame * in_frame_stride + 3 * e;
                            v = luma_rgb((float)p[0], (float)p[1], (float)p[2]);
                        }
                    }
                }
                ring[rr][col & (kRing - 1)] = v;
            }
            __syncthreads();
        }
        if (s < len) {
            sum = __fadd_rn(sum, ring[lane][s & (kRing - 1)]);
            if (s < win) ++cur;
        }
        if (s >= win) {
            sum = __fsub_rn(sum, ring[lane][(s - win) & (kRing - 1)]);
            if (s >= len) --cur;
        }
        if (s >= half - 1) {
            const int oi = s - (half - 1);
            bool keep = true;
            int slot = oi;
            if (nsel) {
                keep = (next_j < nsel) && (oi == next_sel);
                slot = next_j;
            }
            if (keep) {
                float o;
                if ((cur & (cur - 1)) == 0)
                    o = __fmul_rn(sum, 1.0f / (float)cur);  // exact: power-of-two divisor
                else
                    o = __fdiv_rn(sum, (float)cur);
                if (my_line < lines) dst[(long long)slot * out_lines + my_line] = o;
                if (nsel) {
                    ++next_j;
                    next_sel = (int)(((next_j + 0.5) * len) / 64);
                }
            }
        }
    }
}
