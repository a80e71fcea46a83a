// k_group.hip -- duplicate groups with a keeper: the connected components of a pair list, where the list lies (DESIGN.md 4.11;
// the rule: include/hvd_mi355x.h, hvd_group_edges). Records are 16 bytes with the two node indices in words 0 and 1 (hvd_pair,
// hvd_vmatch). Five steps, one launch each (the emit step is the three launches of the block-sum pattern, hvd_scan_dev.h), all
// on the caller's scratch, nothing allocated, no host synchronisation in between:
//   init     parent[v] = v; size, edges, key cleared
//   hook     one lane per record: the roots of both ends, the LARGER root hung under the SMALLER by compare-and-swap
//   flatten  label[v] = root of v; size[root] += 1; key[root] = max(key[root], score[v] << 32 | ~v)
//   count    edges[label[u]] += 1 per record that is an edge
//   emit     the roots with size >= 2, in root order: (root, size, edges, keeper)
// The invariant of hook and flatten: parent[x] <= x, always, with equality exactly at the roots. A root is only ever written by
// the compare-and-swap that hangs it under a smaller index; a node that is no root is only ever written by a compression, with an
// ancestor of its own, which is smaller still. So every chain strictly decreases: a find terminates whatever it reads, stale
// values included, no write can close a cycle, and when the hook kernel has finished the root of a component is its smallest
// member -- whatever the order of the records and of the lanes. That is what makes the labels a function of the input alone.
// parent is read with relaxed agent-scope atomic loads and written with relaxed atomic stores or the compare-and-swap inside
// these two kernels: the L2 caches of the XCDs are not coherent for plain accesses inside a launch. Between launches plain
// accesses do.
// Every index read from a record is checked against V before it is used; the group records are written below cap only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_group_dev.h"

namespace {

__device__ __forceinline__ uint32_t ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(uint32_t* p, uint32_t x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above x, with path halving: every second node of the walk is re-pointed at its grandparent.
__device__ __forceinline__ uint32_t find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = ld(parent + x);
        if (p == x) return x;
        const uint32_t gp = ld(parent + p);
        if (gp == p) return p;
        st(parent + x, gp);  // gp <= p < x, an ancestor of x
        x = gp;
    }
}

__global__ __launch_bounds__(256) void k_group_init(uint32_t V, uint32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                    uint32_t* __restrict__ edges, unsigned long long* __restrict__ key) {
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256u + threadIdx.x; v < V; v += (unsigned long long)gridDim.x * 256u) {
        parent[v] = (uint32_t)v;
        size[v] = 0u;
        edges[v] = 0u;
        key[v] = 0ull;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_group_hook(const uint4* __restrict__ records, unsigned long long n_records,
                                                    const unsigned long long* __restrict__ d_count, uint32_t V,
                                                    const long long* __restrict__ len, uint32_t T, int is_min,
                                                    uint32_t* parent) {
    const unsigned long long E = record_count(n_records, d_count);
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x; e < E; e += (unsigned long long)gridDim.x * 256u) {
        uint32_t u, v;
        if (!edge_of<KIND>(records[e], V, len, T, is_min != 0, &u, &v)) continue;
        uint32_t ru = find(parent, u), rv = find(parent, v);
        while (ru != rv) {
            const uint32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
            const uint32_t seen = atomicCAS(parent + hi, hi, lo);
            if (seen == hi) break;
            // hi had been hung elsewhere in the meantime (seen < hi): go on from there, and from wherever lo has got to
            ru = find(parent, seen);
            rv = find(parent, lo);
        }
    }
}

__global__ __launch_bounds__(256) void k_group_flatten(uint32_t V, uint32_t* parent, const uint32_t* __restrict__ score,
                                                       int32_t* __restrict__ label, uint32_t* size, unsigned long long* key) {
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < V; base += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long v = base + threadIdx.x;
        const bool active = v < V;
        uint32_t r = 0;
        unsigned long long k = 0;
        if (active) {
            r = find(parent, (uint32_t)v);
            label[v] = (int32_t)r;
            k = ((unsigned long long)(score ? score[v] : 0u) << 32) | (0xFFFFFFFFu - (uint32_t)v);  // largest score, then smallest index
        }
        add_one(size, r, active);
        max_key(key, r, k, active);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_group_count(const uint4* __restrict__ records, unsigned long long n_records,
                                                     const unsigned long long* __restrict__ d_count, uint32_t V,
                                                     const long long* __restrict__ len, uint32_t T, int is_min,
                                                     const int32_t* __restrict__ label, uint32_t* edges) {
    const unsigned long long E = record_count(n_records, d_count);
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < E; base += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long e = base + threadIdx.x;
        uint32_t u = 0, v = 0;
        const bool active = e < E && edge_of<KIND>(records[e], V, len, T, is_min != 0, &u, &v);
        add_one(edges, active ? (uint32_t)label[u] : 0u, active);
    }
}

// The grid of k_keep_count over size with the bound 2: a root of a group is a node whose size is >= 2 (the others hold 1 or 0).
__global__ __launch_bounds__(256) void k_group_emit(uint32_t V, const uint32_t* __restrict__ size, const uint32_t* __restrict__ edges,
                                                    const unsigned long long* __restrict__ key,
                                                    const uint32_t* __restrict__ block_prefix, uint4* __restrict__ out,
                                                    unsigned long long cap) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kScanBlk + threadIdx.x * 4u;
    bool keep[4];
    unsigned long long at = keep_prefix((const int32_t*)size, V, 2, block_prefix, base, keep);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!keep[k]) continue;
        const unsigned long long v = base + k;
        if (at < cap) out[at] = make_uint4((uint32_t)v, size[v], edges[v], 0xFFFFFFFFu - (uint32_t)key[v]);
        ++at;
    }
}

}  // namespace

namespace hvd {

// key 8 V | parent, size, edges 4 V each | block sums 4 (ceil(V / 1024) + 1), rounded up to 16
size_t group_scratch_bytes(unsigned long long V) { return (size_t)((20ull * V + 4ull * (scan_blocks(V) + 1) + 15ull) & ~15ull); }

hipError_t launch_group_edges(const EdgeList& in, const GroupsOut& out, hipStream_t s) {
    const uint32_t V = (uint32_t)in.V, T = (uint32_t)in.T;
    const unsigned long long n_records = (unsigned long long)in.n_records;
    const int is_min = min_flag(in);
    unsigned long long* key = (unsigned long long*)out.scratch;
    uint32_t* parent = (uint32_t*)(key + V);
    uint32_t* size = parent + V;
    uint32_t* edges = size + V;
    uint32_t* sums = edges + V;
    const uint4* recs = (const uint4*)in.records;
    hipLaunchKernelGGL(k_group_init, dim3(grid_for(V)), dim3(256), 0, s, V, parent, size, edges, key);
    launch_over_records(in, [&](auto kind) {
        hipLaunchKernelGGL(k_group_hook<decltype(kind)::value>, dim3(grid_for(n_records)), dim3(256), 0, s, recs, n_records,
                           in.d_record_count, V, in.d_lengths, T, is_min, parent);
    });
    hipLaunchKernelGGL(k_group_flatten, dim3(grid_for(V)), dim3(256), 0, s, V, parent, in.d_score, out.node, size, key);
    launch_over_records(in, [&](auto kind) {
        hipLaunchKernelGGL(k_group_count<decltype(kind)::value>, dim3(grid_for(n_records)), dim3(256), 0, s, recs, n_records,
                           in.d_record_count, V, in.d_lengths, T, is_min, out.node, edges);
    });
    return launch_group_records(V, size, sums, out.count, s, [&](unsigned nb) {
        hipLaunchKernelGGL(k_group_emit, dim3(nb), dim3(256), 0, s, V, size, edges, key, sums, (uint4*)out.groups,
                           (unsigned long long)out.cap);
    });
}

}  // namespace hvd
