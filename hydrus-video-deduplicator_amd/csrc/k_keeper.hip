// k_keeper.hip -- keeper-first duplicate groups: every member of a group is a direct match of the group's keeper, and no two
// keepers match (the rule: include/hvd_mi355x.h, hvd_keeper_groups). The keepers are the lexicographically first
// maximal independent set of the graph under the priority key(v) = score[v] << 32 | ~v; every other node is a member of its best
// adjacent keeper. Records, edge predicate and launch shape are those of k_group.hip (hvd_group_dev.h): 16-byte records with the
// two node indices in words 0 and 1, workgroups of 256, grid-stride up to kMaxGrid, the caller's scratch, nothing allocated.
//   init     state, stamps, size, edges, best cleared; the control words set
//   rounds   two launches each, until no node is undecided:
//     edges  one lane per record: with hi the end of higher priority and lo the other, lo undecided: hi a keeper -> stamp lo
//            "member in round r"; hi undecided -> stamp lo "blocked in round r"
//     nodes  one lane per undecided node: a member stamp of r -> member; no blocked stamp of r -> keeper; else it stays, and is
//            counted
//   assign   per edge between a keeper and a member: best[member] = max(best[member], key(keeper))
//   label    keeper_of[v] = v for a keeper, the node of best[v] for a member; size[keeper_of[v]] += 1
//   count    edges[keeper_of[u]] += 1 per record that is an edge with keeper_of[u] == keeper_of[v]
//   emit     the keepers with size >= 2, in keeper order: (keeper, size, edges, keeper)
// Why the result, and the number of rounds, are functions of the input alone: the edge pass reads `state` only, which an earlier
// launch wrote, and writes only stamps, whose value is the round number -- lanes that race on a stamp write the same word, and
// nothing has to be cleared between rounds (a stamp of an earlier round is no stamp). The node pass reads the stamps of the
// launch before it and writes state[v] of its own node alone. No kernel reads what another workgroup of the same launch writes,
// so plain accesses do. The best undecided node of a component is never blocked, so every round decides one node at least:
// V rounds suffice.
// The control words: count[3], the undecided nodes after round r in count[r % 3] -- round r reads count[(r - 1) % 3] (zero: both
// launches return at once), adds into count[r % 3] and clears count[(r + 1) % 3] -- and `rounds`, the last round that ran.
// Every index read from a record is checked against V before it is used; the group records are written below cap only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_group_dev.h"

namespace {

constexpr uint32_t kUndecided = 0, kKeeper = 1, kMember = 2;
constexpr uint32_t kCtlRounds = 3, kCtlWords = 4;  // behind count[0..2]
constexpr uint32_t kBatch = 32;                    // rounds enqueued between two read-backs of the undecided count

// larger is better: the larger score, then the smaller index (the key of k_group_flatten); never 0, since v < 2^31
__device__ __forceinline__ unsigned long long key_of(const uint32_t* __restrict__ score, uint32_t v) {
    return ((unsigned long long)(score ? score[v] : 0u) << 32) | (0xFFFFFFFFu - v);
}

__global__ __launch_bounds__(256) void k_keeper_init(uint32_t V, uint32_t* __restrict__ state, uint32_t* __restrict__ member_stamp,
                                                     uint32_t* __restrict__ blocked_stamp, uint32_t* __restrict__ size,
                                                     uint32_t* __restrict__ edges, unsigned long long* __restrict__ best,
                                                     uint32_t* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x < kCtlWords) ctl[threadIdx.x] = threadIdx.x == 0 ? V : 0u;  // count[0]: before round 1
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256u + threadIdx.x; v < V; v += (unsigned long long)gridDim.x * 256u) {
        state[v] = kUndecided;
        member_stamp[v] = 0u;  // rounds count from 1
        blocked_stamp[v] = 0u;
        size[v] = 0u;
        edges[v] = 0u;
        best[v] = 0ull;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_keeper_edges(const uint4* __restrict__ records, unsigned long long n_records,
                                                      const unsigned long long* __restrict__ d_count, uint32_t V,
                                                      const long long* __restrict__ len, uint32_t T, int is_min,
                                                      const uint32_t* __restrict__ score, const uint32_t* __restrict__ state,
                                                      uint32_t* member_stamp, uint32_t* blocked_stamp,
                                                      const uint32_t* __restrict__ ctl, uint32_t round) {
    if (ctl[(round + 2u) % 3u] == 0u) return;  // the round before left nothing undecided
    const unsigned long long E = record_count(n_records, d_count);
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x; e < E; e += (unsigned long long)gridDim.x * 256u) {
        uint32_t u, v;
        if (!edge_of<KIND>(records[e], V, len, T, is_min != 0, &u, &v)) continue;
        const uint32_t su = state[u], sv = state[v];
        if (su != kUndecided && sv != kUndecided) continue;
        const bool u_hi = key_of(score, u) > key_of(score, v);
        const uint32_t lo = u_hi ? v : u, s_lo = u_hi ? sv : su, s_hi = u_hi ? su : sv;
        if (s_lo != kUndecided) continue;
        if (s_hi == kKeeper)
            member_stamp[lo] = round;
        else if (s_hi == kUndecided)
            blocked_stamp[lo] = round;
    }
}

__global__ __launch_bounds__(256) void k_keeper_nodes(uint32_t V, uint32_t* __restrict__ state,
                                                      const uint32_t* __restrict__ member_stamp,
                                                      const uint32_t* __restrict__ blocked_stamp, uint32_t* ctl, uint32_t round) {
    const uint32_t before = ctl[(round + 2u) % 3u];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first) ctl[(round + 1u) % 3u] = 0u;  // the next round counts into it; also when this one returns, so that zero stays zero
    if (before == 0u) return;
    if (first) ctl[kCtlRounds] = round;
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < V; base += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long v = base + threadIdx.x;
        bool stays = false;
        if (v < V && state[v] == kUndecided) {
            if (member_stamp[v] == round)
                state[v] = kMember;
            else if (blocked_stamp[v] != round)
                state[v] = kKeeper;
            else
                stays = true;
        }
        add_one(ctl + round % 3u, 0u, stays);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_keeper_assign(const uint4* __restrict__ records, unsigned long long n_records,
                                                       const unsigned long long* __restrict__ d_count, uint32_t V,
                                                       const long long* __restrict__ len, uint32_t T, int is_min,
                                                       const uint32_t* __restrict__ score, const uint32_t* __restrict__ state,
                                                       unsigned long long* best) {
    const unsigned long long E = record_count(n_records, d_count);
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < E; base += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long e = base + threadIdx.x;
        uint32_t u = 0, v = 0, member = 0;
        unsigned long long k = 0;
        bool active = e < E && edge_of<KIND>(records[e], V, len, T, is_min != 0, &u, &v);
        if (active) {
            const uint32_t su = state[u], sv = state[v];
            active = (su == kKeeper && sv == kMember) || (su == kMember && sv == kKeeper);
            member = su == kMember ? u : v;
            if (active) k = key_of(score, su == kMember ? v : u);
        }
        max_key(best, member, k, active);
    }
}

__global__ __launch_bounds__(256) void k_keeper_label(uint32_t V, const uint32_t* __restrict__ state,
                                                      const unsigned long long* __restrict__ best, int32_t* __restrict__ keeper_of,
                                                      uint32_t* size) {
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < V; base += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long v = base + threadIdx.x;
        const bool active = v < V;
        uint32_t k = 0;
        if (active) {
            k = state[v] == kMember ? 0xFFFFFFFFu - (uint32_t)best[v] : (uint32_t)v;
            if (k >= V) k = (uint32_t)v;  // (a member has a keeper beside it; an index is checked all the same)
            keeper_of[v] = (int32_t)k;
        }
        add_one(size, k, active);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_keeper_count(const uint4* __restrict__ records, unsigned long long n_records,
                                                      const unsigned long long* __restrict__ d_count, uint32_t V,
                                                      const long long* __restrict__ len, uint32_t T, int is_min,
                                                      const int32_t* __restrict__ keeper_of, uint32_t* edges) {
    const unsigned long long E = record_count(n_records, d_count);
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < E; base += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long e = base + threadIdx.x;
        uint32_t u = 0, v = 0, k = 0;
        bool active = e < E && edge_of<KIND>(records[e], V, len, T, is_min != 0, &u, &v);
        if (active) {
            k = (uint32_t)keeper_of[u];
            active = k == (uint32_t)keeper_of[v];
        }
        add_one(edges, k, active);
    }
}

// The grid of k_keep_count over size with the bound 2: a keeper with a member holds >= 2, every other node 1 or 0.
__global__ __launch_bounds__(256) void k_keeper_emit(uint32_t V, const uint32_t* __restrict__ size, const uint32_t* __restrict__ edges,
                                                     const uint32_t* __restrict__ block_prefix, uint4* __restrict__ out,
                                                     unsigned long long cap) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kScanBlk + threadIdx.x * 4u;
    bool keep[4];
    unsigned long long at = keep_prefix((const int32_t*)size, V, 2, block_prefix, base, keep);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!keep[k]) continue;
        const unsigned long long v = base + k;
        if (at < cap) out[at] = make_uint4((uint32_t)v, size[v], edges[v], (uint32_t)v);
        ++at;
    }
}

}  // namespace

namespace hvd {

// best 8 V | state, member stamp, blocked stamp, size, edges 4 V each | block sums 4 (ceil(V / 1024) + 1) | 4 control words,
// rounded up to 16
size_t keeper_scratch_bytes(unsigned long long V) {
    return (size_t)((28ull * V + 4ull * (scan_blocks(V) + 1) + 4ull * kCtlWords + 15ull) & ~15ull);
}

hipError_t launch_keeper_groups(const EdgeList& in, const GroupsOut& out, hipStream_t s, long long* rounds, bool* settled) {
    const uint32_t V = (uint32_t)in.V, T = (uint32_t)in.T;
    const unsigned long long n_records = (unsigned long long)in.n_records;
    const int is_min = min_flag(in);
    unsigned long long* best = (unsigned long long*)out.scratch;
    uint32_t* state = (uint32_t*)(best + V);
    uint32_t* member_stamp = state + V;
    uint32_t* blocked_stamp = member_stamp + V;
    uint32_t* size = blocked_stamp + V;
    uint32_t* edges = size + V;
    uint32_t* sums = edges + V;
    uint32_t* ctl = sums + scan_blocks(V) + 1;
    const uint4* recs = (const uint4*)in.records;
    *settled = false;
    hipLaunchKernelGGL(k_keeper_init, dim3(grid_for(V)), dim3(256), 0, s, V, state, member_stamp, blocked_stamp, size, edges, best, ctl);
    uint32_t undecided = V, round = 0;
    while (undecided != 0 && round < V) {
        for (uint32_t k = 0; k < kBatch; ++k) {
            ++round;
            launch_over_records(in, [&](auto kind) {
                hipLaunchKernelGGL(k_keeper_edges<decltype(kind)::value>, dim3(grid_for(n_records)), dim3(256), 0, s, recs, n_records,
                                   in.d_record_count, V, in.d_lengths, T, is_min, in.d_score, state, member_stamp, blocked_stamp, ctl,
                                   round);
            });
            hipLaunchKernelGGL(k_keeper_nodes, dim3(grid_for(V)), dim3(256), 0, s, V, state, member_stamp, blocked_stamp, ctl, round);
        }
        if (hipError_t e = hipGetLastError()) return e;
        if (hipError_t e = hipMemcpyAsync(&undecided, ctl + round % 3u, 4, hipMemcpyDeviceToHost, s)) return e;
        if (hipError_t e = hipStreamSynchronize(s)) return e;
    }
    if (undecided != 0) return hipSuccess;  // more than V rounds: the caller's HVD_ERR_STATE
    *settled = true;
    if (rounds) {
        uint32_t ran = 0;
        if (hipError_t e = hipMemcpyAsync(&ran, ctl + kCtlRounds, 4, hipMemcpyDeviceToHost, s)) return e;
        if (hipError_t e = hipStreamSynchronize(s)) return e;
        *rounds = (long long)ran;
    }
    launch_over_records(in, [&](auto kind) {
        hipLaunchKernelGGL(k_keeper_assign<decltype(kind)::value>, dim3(grid_for(n_records)), dim3(256), 0, s, recs, n_records,
                           in.d_record_count, V, in.d_lengths, T, is_min, in.d_score, state, best);
    });
    hipLaunchKernelGGL(k_keeper_label, dim3(grid_for(V)), dim3(256), 0, s, V, state, best, out.node, size);
    launch_over_records(in, [&](auto kind) {
        hipLaunchKernelGGL(k_keeper_count<decltype(kind)::value>, dim3(grid_for(n_records)), dim3(256), 0, s, recs, n_records,
                           in.d_record_count, V, in.d_lengths, T, is_min, out.node, edges);
    });
    return launch_group_records(V, size, sums, out.count, s, [&](unsigned nb) {
        hipLaunchKernelGGL(k_keeper_emit, dim3(nb), dim3(256), 0, s, V, size, edges, sums, (uint4*)out.groups,
                           (unsigned long long)out.cap);
    });
}

}  // namespace hvd
