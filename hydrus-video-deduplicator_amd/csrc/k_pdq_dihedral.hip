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
// strict layout (k_pdq.hip) up to the median, built from the same definitions (hvd_pdq_dev.h, the home of the
// bit-exactness contract): stage 1 and 2 are __fmul_rn/__fadd_rn, k ascending, in K1's order, with the context's
// DCT matrix, so variant 0 is bit-identical to K1's hash and the coefficients are the oracle's.
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
#include "hvd_pdq_dev.h"

namespace {

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
    __shared__ PdqLds lds;
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
            float a[64];
            pdq_load_column<KIND>(lds, in, f, lane, a);             // stage 0
            const int qual = pdq_quality<KIND>(a, lane);  // one value for all 8 variants

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
            float b[4];
            pdq_dct_stage2(lds, wave, lane, b);
            const int j = lane & 15, i0 = lane >> 4;  // b[r] = B[i0 + 4r][j]

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
