// k_index_order.hip -- the low-byte pass of the pigeonhole index build for the partitions that fit LDS (the build and its
// other kernels: k_hamming_index.hip).
//
// The high-byte pass (k_index_scatter.hip) has laid every (block, high byte) partition out as one contiguous run of records. A partition of at most
// kOrderMax records (hvd_index_dev.h: every one of a uniform DB of 2^20 hashes, and of some way beyond) is ordered by ONE workgroup in ONE
// kernel: the low bytes counted in 256 LDS counters, scanned, every record ranked by a returning LDS atomic and laid out in
// final order in LDS, then copied out as two contiguous streams -- where the chunk kernels (k_index_count, k_index_offsets,
// k_index_place) read the records twice and k_index_place stores every word and every row to a cache line of its own. The
// workgroup holds its records in registers between the count and the rank, so they are read once. Larger partitions, and
// empty ones, are left to the chunk kernels, which skip what this kernel took: the same size test, index_dev::orders_whole.
// The kernel runs behind the probe's gate like the other build kernels and BEFORE the statistics decide: when the index then
// loses the pass, its words and rows were written for nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_index_dev.h"
#include "hvd_kernels.h"

namespace {

using namespace hvd::index_dev;

constexpr uint32_t kOrderThreads = 512u;
constexpr uint32_t kOrderPer = kOrderMax / kOrderThreads;  // records per thread, in registers
static_assert(kOrderMax % kOrderThreads == 0u, "whole rounds of the workgroup");
static_assert(8u * kOrderMax + 4u * 256u + 16u <= 65536u, "static LDS of k_index_order");

// One workgroup per partition p = (b, h). Thread t < 256 = key h * 256 + t: cnt[b][key], off[b][key] (and off[b][65536] = n
// from the block's last key), as k_index_offsets writes them. hw[b][pbase + .] = the records' words, rows[b][pbase + .] =
// their rows, in key order; inside a bucket in whatever order the atomics give (the join does not depend on it).
__global__ __launch_bounds__(kOrderThreads) void k_index_order(const uint2* __restrict__ rec, uint32_t n, const uint32_t* __restrict__ ptotal,
                                                               const uint32_t* __restrict__ pbase, uint32_t* __restrict__ cnt,
                                                               uint32_t* __restrict__ off, uint32_t* __restrict__ hw,
                                                               uint32_t* __restrict__ rows, const uint32_t* __restrict__ select) {
    __shared__ uint32_t cur[256];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t sw[kOrderMax], sr[kOrderMax];
    if (select[hvd::kSelIdxGate] == 0u) return;
    const uint32_t p = blockIdx.x, b = p >> 8, total = ptotal[p];
    if (!orders_whole(total)) return;  // (uniform over the workgroup)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t first = pbase[p];
    const size_t at = (size_t)b * n + first;  // the partition's first record inside rec, its first position inside hw and rows
    if (tid < 256u) cur[tid] = 0u;
    const uint2* __restrict__ r = rec + at;
    uint2 rc[kOrderPer];
#pragma unroll
    for (uint32_t j = 0; j < kOrderPer; ++j) {
        const uint32_t e = j * kOrderThreads + tid;
        rc[j] = e < total ? r[e] : make_uint2(0u, 0u);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kOrderPer; ++j)
        if (j * kOrderThreads + tid < total) (void)lds_add(&cur[rc[j].y & 255u]);
    __syncthreads();
    // the first four waves scan the 256 counters (whole waves: the shuffles see every lane)
    uint32_t c = 0, incl = 0;
    if (tid < 256u) {
        c = cur[tid];
        incl = wave_incl_scan(c, lane);
        if (lane == 63u) wsum[wave] = incl;
    }
    __syncthreads();
    if (tid < 256u) {
        uint32_t pos = incl - c;  // inside the partition
        for (uint32_t w = 0; w < wave; ++w) pos += wsum[w];
        cur[tid] = pos;
        const uint32_t key = (p & 255u) * 256u + tid;
        cnt[b * kKeys + key] = c;
        off[(size_t)b * (kKeys + 1u) + key] = first + pos;
        if (key == kKeys - 1u) off[(size_t)b * (kKeys + 1u) + kKeys] = n;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kOrderPer; ++j)
        if (j * kOrderThreads + tid < total) {
            const uint32_t pos = lds_add(&cur[rc[j].y & 255u]);
            if (pos < kOrderMax) {  // (always: the cursors were counted from these records)
                sw[pos] = rc[j].y;
                sr[pos] = rc[j].x;
            }
        }
    __syncthreads();
    for (uint32_t e = tid; e < total; e += kOrderThreads) {
        hw[at + e] = sw[e];
        rows[at + e] = sr[e];
    }
}

}  // namespace

namespace hvd {

hipError_t launch_index_order(const uint2* rec, uint32_t n, const uint32_t* ptotal, const uint32_t* pbase, uint32_t* cnt, uint32_t* off,
                              uint32_t* hw, uint32_t* rows, const uint32_t* d_select, hipStream_t s) {
    hipLaunchKernelGGL(k_index_order, dim3(kParts), dim3(kOrderThreads), 0, s, rec, n, ptotal, pbase, cnt, off, hw, rows, d_select);
    return hipGetLastError();
}

}  // namespace hvd
