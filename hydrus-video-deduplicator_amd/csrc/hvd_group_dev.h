// hvd_group_dev.h -- what the kernels over a list of 16-byte edge records share, one definition: k_group.hip (connected
// components) and k_keeper.hip (keeper-first groups) judge a record by the same predicate, take the
// same number of records, and aggregate their atomics on one destination per wave the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// Is record r an edge, and between which nodes? kind 0: every record with two distinct nodes below V. kind 1: an hvd_vmatch,
// and the pair predicate of the reference on top (dedup.py:445-502), in 64-bit integers: with na = len[a], nb = len[b],
// qa = na > 0 and 100 q_hits >= T na, tb likewise; policy "min": qa and tb, the others: qa or tb. A length beyond 100 (2^32 - 1)
// can pass with no 32-bit counter, and is set aside before the product that it would overflow.
template <int KIND>
__device__ __forceinline__ bool edge_of(const uint4 r, uint32_t V, const long long* __restrict__ len, uint32_t T, bool is_min,
                                        uint32_t* u, uint32_t* v) {
    *u = r.x;
    *v = r.y;
    if (r.x >= V || r.y >= V || r.x == r.y) return false;
    if constexpr (KIND == 0) return true;
    constexpr long long kLongest = 100ll * 0xFFFFFFFFll;
    const long long na = len[r.x], nb = len[r.y];
    const bool qa = na > 0 && na <= kLongest && 100ull * r.z >= (unsigned long long)T * (unsigned long long)na;
    const bool tb = nb > 0 && nb <= kLongest && 100ull * r.w >= (unsigned long long)T * (unsigned long long)nb;
    return is_min ? (qa && tb) : (qa || tb);
}

// The records that count: all n_records, or as many of them as the all-pairs pass in front has counted.
__device__ __forceinline__ unsigned long long record_count(unsigned long long n_records, const unsigned long long* d_count) {
    if (!d_count) return n_records;
    const unsigned long long c = *d_count;
    return c < n_records ? c : n_records;
}

// arr[dst] += 1 for every active lane, called by the whole wave: the lanes that share the destination of the first active lane
// go as one atomic, the others one by one (the records of one cluster lie together; a giant component is one destination).
__device__ __forceinline__ void add_one(uint32_t* arr, uint32_t dst, bool active) {
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const uint32_t first = __shfl(dst, __ffsll((long long)act) - 1);
    const bool same = active && dst == first;
    const unsigned long long m = __ballot(same);
    const uint32_t lane = threadIdx.x & 63u;
    if (same) {
        if (lane == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(arr + first, (uint32_t)__popcll(m));
    } else if (active) {
        atomicAdd(arr + dst, 1u);
    }
}

// arr[dst] = max(arr[dst], key) the same way (key > 0 on every active lane)
__device__ __forceinline__ void max_key(unsigned long long* arr, uint32_t dst, unsigned long long key, bool active) {
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const uint32_t first = __shfl(dst, __ffsll((long long)act) - 1);
    const bool same = active && dst == first;
    unsigned long long k = same ? key : 0ull;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = o > k ? o : k;
    }
    const unsigned long long m = __ballot(same);
    const uint32_t lane = threadIdx.x & 63u;
    if (same) {
        if (lane == (uint32_t)__ffsll((long long)m) - 1u) atomicMax(arr + first, k);
    } else if (active) {
        atomicMax(arr + dst, key);
    }
}

}  // namespace
