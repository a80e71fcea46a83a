// hvd_index_dev.h -- what the kernel files of the pigeonhole index build share (k_hamming_index.hip: the chunked counting
// sort and the join; k_index_scatter.hip: the high-byte pass staged in LDS; k_index_order.hip: the partitions that fit
// LDS): the geometry of the keys, which tile a workgroup of the tile kernels takes, the two LDS / wave helpers,
// and the ONE size test that says which of the two files orders a partition. Device code: HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hvd {
namespace index_dev {

constexpr uint32_t kBlocks = 16, kKeys = 65536;
constexpr uint32_t kParts = kBlocks * 256u;  // partitions: (block, high byte of the key)

// A partition of at most this many records is ordered whole by one workgroup of k_index_order, which lays it out in LDS (8
// bytes per record: 48 KiB, three workgroups per compute unit); a larger one goes through the chunk kernels. A uniform DB of
// 2^20 hashes has partitions of 4096 +- 64 records: 32 standard deviations below. (7680, two workgroups per compute
// unit: 49 .. 50 us at 1 M hashes against 46.)
constexpr uint32_t kOrderMax = 6144;
// (an empty partition has nothing to order: k_index_offsets writes its 256 zero counts as ever)
__host__ __device__ constexpr bool orders_whole(uint32_t records) { return records - 1u < kOrderMax; }

// The hardware deals the workgroups of a grid to the 8 XCDs in turn, so workgroups id and id + 1 write through different
// L2 caches. Where neighbouring work items write neighbouring pieces of one cache line -- the runs of tiles t and t + 1 in
// a partition of rec, the counts of tiles t and t + 1 in a row of tcnt -- neither L2 ever holds the whole line and both
// write a partial one back. This turns the id into a work item such that the workgroups that share an XCD (id % 8 labels
// them; which XCD that is does not matter) take consecutive items: a bijection of 0 .. items - 1 for any number of items.
// It moves work between workgroups and nothing else: results do not depend on it.
__device__ __forceinline__ uint32_t xcd_consecutive(uint32_t id, uint32_t items) {
    const uint32_t q = items / 8u, r = items % 8u, x = id % 8u;
    return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + id / 8u;
}

__device__ __forceinline__ uint32_t lds_add(uint32_t* p) {
    return __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(v, d);
        if (lane >= (uint32_t)d) v += y;
    }
    return v;
}

}  // namespace index_dev
}  // namespace hvd
