// hvd_group_dev.h -- what the kernels over a list of 16-byte edge records share, one definition: k_group.hip (connected
// components) and k_keeper.hip (keeper-first groups) judge a record by the same predicate, take the
// same number of records, and aggregate their atomics on one destination per wave the same way. Device code first; the last
// section is host code, what the two launchers share: the grid of the grid-stride kernels, the min flag, the
// choice of the kernels' record kind, and the launches that close either grouping with its group records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hvd_kernels.h"
#include "hvd_scan_dev.h"

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

// ---- host code: what the two launchers share ---------------------------------------------------------------------------
constexpr unsigned kMaxGrid = 16384;  // grid-stride kernels

inline unsigned grid_for(unsigned long long n) {
    const unsigned long long b = (n + 255ull) / 256ull;
    return (unsigned)(b < 1 ? 1 : b > kMaxGrid ? kMaxGrid : b);
}

// workgroups of the block-sum pattern over the V nodes (hvd_scan_dev.h); the scratch holds one block sum more
inline unsigned scan_blocks(unsigned long long V) { return (unsigned)((V + kScanBlk - 1) / kScanBlk); }

// the is_min argument of every kernel over the records: the policy counts for the VMATCH predicate alone
inline int min_flag(const hvd::EdgeList& in) { return in.kind == HVD_EDGES_VMATCH && in.is_min ? 1 : 0; }

// launch(kind) enqueues one kernel over the records, kind a std::integral_constant<int, KIND>: the kernel's template argument.
// An empty list gets no launch.
template <class Launch>
void launch_over_records(const hvd::EdgeList& in, Launch launch) {
    if (in.n_records <= 0) return;
    if (in.kind == HVD_EDGES_VMATCH)
        launch(std::integral_constant<int, 1>{});
    else
        launch(std::integral_constant<int, 0>{});
}

// The group records, the close of either grouping: the nodes whose size is >= 2 counted block by block, the block sums scanned
// (*d_count = the number of groups), then emit(nb): the caller's emit kernel, on the grid of k_keep_count.
template <class Emit>
hipError_t launch_group_records(uint32_t V, const uint32_t* size, uint32_t* sums, unsigned long long* d_count, hipStream_t s,
                                Emit emit) {
    const unsigned nb = scan_blocks(V);
    hipLaunchKernelGGL(k_keep_count, dim3(nb), dim3(256), 0, s, (const int32_t*)size, (unsigned long long)V, 2, sums);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, s, sums, nb, d_count);
    emit(nb);
    return hipGetLastError();
}

}  // namespace
