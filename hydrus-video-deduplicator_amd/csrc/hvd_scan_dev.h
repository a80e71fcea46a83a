// hvd_scan_dev.h -- the block-sum prefix pattern, one definition: "which of n int32 values are >= a bound, and how many such
// values lie before each". k_vmatch.hip uses it on the frame qualities (the stream compaction of VideoHasher.finish),
// k_group.hip on the component sizes (the group records, in root order). Three pieces, for workgroups of kScanBlk values
// (256 lanes x 4):
//   k_keep_count        one launch of ceil(n / kScanBlk) workgroups: block_sums[b] = kept values of block b
//   k_scan_block_sums   one workgroup: exclusive scan of the block sums in place, total[0] = the number of kept values
//   keep_prefix         inside a scatter kernel with the same grid: this lane's four keep flags and the number of kept values
//                       before its first one
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t kScanBlk = 1024;  // values per workgroup (256 lanes x 4)

__global__ __launch_bounds__(256) void k_keep_count(const int32_t* __restrict__ quality, unsigned long long n, int min_q,
                                                    uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t part[4];
    const unsigned long long base = (unsigned long long)blockIdx.x * kScanBlk + threadIdx.x * 4u;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + k < n && quality[base + k] >= min_q) ++c;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// exclusive scan of the block sums in place (one workgroup walks them in chunks of 1024 with a carry);
// total[0] = number of kept values
__global__ __launch_bounds__(1024) void k_scan_block_sums(uint32_t* __restrict__ sums, uint32_t nb,
                                                          unsigned long long* __restrict__ total) {
    __shared__ uint32_t buf[1024];
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < nb; c0 += 1024u) {
        const uint32_t idx = c0 + threadIdx.x;
        const uint32_t v = idx < nb ? sums[idx] : 0u;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t off = 1; off < 1024u; off <<= 1) {  // Hillis-Steele inclusive scan
            const uint32_t add = threadIdx.x >= off ? buf[threadIdx.x - off] : 0u;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        const uint32_t carry = carry_s;
        if (idx < nb) sums[idx] = carry + buf[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023u) carry_s = carry + buf[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry_s;
}

// The keep flags of this lane's 4 values and the number of kept values before its first one (block_prefix: the scanned
// block sums): an exclusive scan of the lanes' counts, by shuffles inside a wave, then over the 4 wave totals.
__device__ __forceinline__ uint32_t keep_prefix(const int32_t* __restrict__ quality, unsigned long long n, int min_q,
                                                const uint32_t* __restrict__ block_prefix, unsigned long long base,
                                                bool (&keep)[4]) {
    __shared__ uint32_t wave_sum[4];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        keep[k] = base + k < n && quality[base + k] >= min_q;
        c += keep[k] ? 1u : 0u;
    }
    uint32_t incl = c;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += up;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = block_prefix[blockIdx.x] + incl - c;
    for (uint32_t w = 0; w < wave; ++w) before += wave_sum[w];
    return before;
}

}  // namespace
