// k_pdq_dihedral.hip -- the 8 dihedral PDQ hashes of a frame for gfx950 (MI355X).
//
// The hashes of a frame's mirror images and rotations follow from the frame's own 16x16 DCT
// (DESIGN.md 4.6): with sx(j) = +1 for odd j, -1 for even j (sy likewise on the row index),
//   0 identity  B[i][j]          4 transpose      B[j][i]
//   1 flip_h    sx(j) B[i][j]    5 antitranspose  sx(i) sy(j) B[j][i]
//   2 flip_v    sy(i) B[i][j]    6 rot90_ccw      sx(i) B[j][i]
//   3 rot180    sx(j)sy(i)B[i][j] 7 rot90_cw      sy(j) B[j][i]
// each thresholded at its own median. A transpose leaves the multiset of values alone, so variant
// 4 / 5 / 6 / 7 is the transposed BIT matrix of variant 0 / 3 / 1 / 2: 4 medians, 4 comparisons,
// 4 bit transposes per frame.
//
// k_pdq_dihedral64: one wave64 per frame, 4 frames per workgroup, static grid stride -- k_pdq_hash64's
// strict layout (k_pdq.hip) up to the median, with the same bit-exactness contract: stage 1 and 2
// are __fmul_rn/__fadd_rn, k ascending, in K1's order, with the context's DCT matrix, so variant 0
// is bit-identical to K1's hash and the coefficients are the oracle's.
//   stage 0  lane j loads column j of the 64x64 frame
//   quality  as K1
//   stage 1  T = D*A: lane j owns column j, D[i][k] wave-uniform -> scalar loads
//   stage 2  B = T*D^T through LDS, lane l -> (i0=l>>4, j=l&15), b[r] = B[i0+4r][j] = coefficient l+64r
//   median   4 radix selects with wave ballots (K1's), one per sign pattern
//   bits     ballot(B' > median) for variants 0-3; 4-7 by a per-lane bit gather from those ballots
// The sign flips are exact (negation), and a sign pattern only depends on the lane: j = l&15 and
// i = (l>>4) + 4r have r-independent parities.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_kernels.h"

namespace {

constexpr int kWaves = 4;  // frames in flight per workgroup
constexpr int kLd = 68;    // padded LDS row stride (floats), as k_pdq.hip

struct alignas(16) DihedralLds {
    float T[kWaves][16][kLd];
    float D[16][kLd];
    float luma_lut[256];
};

// ---- helpers copied from k_pdq.hip (kept there unchanged; see that file for their derivations) ----
__device__ __forceinline__ float luma_gray(uint32_t g) {
    const float v = (float)g;
    float y = __fmul_rn(0.299f, v);
    y = __fadd_rn(y, __fmul_rn(0.587f, v));
    y = __fadd_rn(y, __fmul_rn(0.114f, v));
    return y;
}

// |(int)(((u - v) * 100) / 255)| for float luma: trunc(|x| * (float below 1/255)) plus a remainder correction
__device__ __forceinline__ void grad_term(float u, float v, float& acc_m, int& acc_c) {
    const float ax = fabsf(__fmul_rn(__fsub_rn(u, v), 100.0f));
    const float m = truncf(__fmul_rn(ax, 0x1.0101p-8f));
    const float r = __fmaf_rn(-255.0f, m, ax);
    acc_m += m;
    acc_c += (r >= 255.0f) ? 1 : 0;
}

// the same term for luma of gray bytes: one multiply by RN(100/255), exact for all 256 x 256 byte pairs
__device__ __forceinline__ void grad_term_gray(float u, float v, int& acc) {
    acc += (int)__fmul_rn(fabsf(__fsub_rn(u, v)), 0x1.919192p-2f);
}

__device__ __forceinline__ float wave_next_lane(float v) {  // lane l reads lane l+1 (DPP wave_shl:1)
    const int x = __float_as_int(v);
    return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x130, 0xF, 0xF, true));
}

__device__ __forceinline__ float wave_sum_f32(float v) {  // exact: integer-valued, far below 2^24
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 128th smallest of the wave's 256 values (4 per lane): K1's radix select over order-preserving keys
__device__ __forceinline__ float wave_median256(const float (&b)[4]) {
    uint32_t key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t u = __float_as_uint(b[r]);
        key[r] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
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

// Hash words of B' > median (word r = bits 64r..64r+63 = lane l, value r) for the sign pattern `neg` of this lane.
__device__ __forceinline__ void signed_bits(const float (&b)[4], bool neg, unsigned long long (&m)[4]) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = neg ? -b[r] : b[r];
    const float med = wave_median256(v);
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = __ballot(v[r] > med);
}

// The transposed bit matrix: output bit (i, j) = input bit (j, i). Lane l builds output bit l + 64r, i.e.
// i = (l>>4) + 4r, j = l&15, from input bit 16j + i: word j>>2 (the same for every r), bit 16(j&3) + i.
__device__ __forceinline__ void transpose_bits(const unsigned long long (&m)[4], int lane, unsigned long long (&t)[4]) {
    const int w = (lane >> 2) & 3;
    const unsigned long long src = w == 0 ? m[0] : w == 1 ? m[1] : w == 2 ? m[2] : m[3];
    const int base = 16 * (lane & 3) + (lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = __ballot((src >> (base + 4 * r)) & 1ull);
}

__device__ __forceinline__ void store_hash(uint8_t* hashes, long long f, int v, int lane, const unsigned long long (&m)[4]) {
    if (lane < 4) {
        const unsigned long long w = lane == 0 ? m[0] : lane == 1 ? m[1] : lane == 2 ? m[2] : m[3];
        reinterpret_cast<unsigned long long*>(hashes)[(f * 8 + v) * 4 + lane] = w;
    }
}

// KIND 0: uint8 gray 64x64 frames. KIND 1: float 64x64 luma (the front-ends' output).
// hashes: n * 8 * 32 bytes (variant-major within a frame), quality: n int32.
template <int KIND>
__global__ __launch_bounds__(256) void k_pdq_dihedral64(const void* __restrict__ in, long long n,
                                                        const float* __restrict__ dct, uint8_t* __restrict__ hashes,
                                                        int32_t* __restrict__ quality) {
    __shared__ DihedralLds lds;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    for (int e = threadIdx.x; e < 16 * 64; e += 256) lds.D[e >> 6][e & 63] = dct[e];
    lds.luma_lut[threadIdx.x] = luma_gray(threadIdx.x);
    __syncthreads();

    const long long groups = (n + kWaves - 1) / kWaves;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long f = g * kWaves + wave;
        const bool valid = f < n;  // wave-uniform

        if (valid) {
            // ---- stage 0: column `lane` of the frame ----
            float a[64];
            if (KIND == 0) {
                const uint8_t* src = reinterpret_cast<const uint8_t*>(in) + f * 4096 + lane;
#pragma unroll
                for (int k = 0; k < 64; ++k) a[k] = lds.luma_lut[src[k * 64]];
            } else {
                const float* src = reinterpret_cast<const float*>(in) + f * 4096 + lane;
#pragma unroll
                for (int k = 0; k < 64; ++k) a[k] = src[k * 64];
            }

            // ---- quality (one value for all 8 variants) ----
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
                if (lane < 63) {
                    gs += gh;
                    cs_ += ch_;
                }
                gsum = (int)wave_sum_f32(gs + (float)cs_);
            }
            int qual = gsum / 90;
            qual = qual > 100 ? 100 : qual;

            // ---- stage 1: T[i][lane] = sum_k D[i][k] * a[k], k ascending ----
#pragma unroll 1
            for (int i0 = 0; i0 < 16; i0 += 4) {
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
                // wave-uniform -> s_load; one base pointer for the 4 rows (immediate offsets) keeps the SGPRs within
                // budget: with one pointer per row the frame pointer was spilled to a VGPR lane
                const float* d = dct + i0 * 64;
#pragma unroll
                for (int k = 0; k < 64; ++k) {
                    s0 = __fadd_rn(s0, __fmul_rn(d[k], a[k]));
                    s1 = __fadd_rn(s1, __fmul_rn(d[64 + k], a[k]));
                    s2 = __fadd_rn(s2, __fmul_rn(d[128 + k], a[k]));
                    s3 = __fadd_rn(s3, __fmul_rn(d[192 + k], a[k]));
                }
                lds.T[wave][i0 + 0][lane] = s0;
                lds.T[wave][i0 + 1][lane] = s1;
                lds.T[wave][i0 + 2][lane] = s2;
                lds.T[wave][i0 + 3][lane] = s3;
            }
            if (lane == 0) quality[f] = qual;
        }
        wave_lds_handover();  // T[wave] is private to this wave

        if (valid) {
            // ---- stage 2: B[i][j] = sum_k T[i][k] * D[j][k], k ascending ----
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

            // ---- 4 sign patterns -> 4 medians -> 8 hashes ----
            const bool nx = (j & 1) == 0;   // sx(j) = -1
            const bool ny = (i0 & 1) == 0;  // sy(i) = -1 (i = i0 + 4r has i0's parity)
            unsigned long long m[4], t[4];
            signed_bits(b, false, m);  // 0 identity
            store_hash(hashes, f, 0, lane, m);
            transpose_bits(m, lane, t);  // 4 transpose
            store_hash(hashes, f, 4, lane, t);
            signed_bits(b, nx, m);  // 1 flip_h
            store_hash(hashes, f, 1, lane, m);
            transpose_bits(m, lane, t);  // 6 rot90_ccw
            store_hash(hashes, f, 6, lane, t);
            signed_bits(b, ny, m);  // 2 flip_v
            store_hash(hashes, f, 2, lane, m);
            transpose_bits(m, lane, t);  // 7 rot90_cw
            store_hash(hashes, f, 7, lane, t);
            signed_bits(b, nx != ny, m);  // 3 rot180
            store_hash(hashes, f, 3, lane, m);
            transpose_bits(m, lane, t);  // 5 antitranspose
            store_hash(hashes, f, 5, lane, t);
        }
        wave_lds_handover();  // T[wave] is rewritten by this wave's next frame
    }
}

}  // namespace

namespace hvd {

hipError_t launch_pdq_dihedral64(const void* d_in, int kind, int64_t n, const float* d_dct, uint8_t* d_hashes8,
                                 int32_t* d_quality, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t groups = (n + kWaves - 1) / kWaves;
    // static stride over what is resident at once: 107 / 101 VGPRs = 4 waves per SIMD = 4 workgroups per CU (22 784 B of LDS
    // each), so no second dispatch round of a few workgroups trails the launch
    const int64_t max_grid = 256 * 4;
    const dim3 grid((unsigned)(groups < max_grid ? groups : max_grid));
    if (kind == 0)
        hipLaunchKernelGGL(k_pdq_dihedral64<0>, grid, dim3(256), 0, s, d_in, (long long)n, d_dct, d_hashes8, d_quality);
    else
        hipLaunchKernelGGL(k_pdq_dihedral64<1>, grid, dim3(256), 0, s, d_in, (long long)n, d_dct, d_hashes8, d_quality);
    return hipGetLastError();
}

}  // namespace hvd
