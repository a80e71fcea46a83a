// k_vmatch_weighted.hip -- the duration-weighted video search: every frame carries an integer weight (the run
// of the static-scene filter, DESIGN 4.19: the frames a kept frame stands for), the fold adds that weight where the plain fold
// of k_vmatch.hip adds 1, and the per-video weight totals take the place of the frame counts as denominators.
//   * k_keys_to_pairs_weighted   key set -> pair map, as k_keys_to_pairs: q_hits / t_hits become sums of capped weights.
//   * k_video_weights            totals[v] = sum of the capped weights of video v's frames, int64 per video.
// The cap: w = max_weight ? min(weight, max_weight) : weight, in uint32. max_weight 1 makes every weight 1 (the plain fold),
// 0 leaves them as they are. Nothing is validated here: a weight below 1 or a sum past 2^32 - 1 gives wrong counters
// (mod 2^32), never an access outside the buffers -- a weight is only ever read at a frame index that a key or a clamped
// CSR range names. Both kernels are O(frames) next to the O(frames^2) compare.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_devhash.h"
#include "hvd_kernels.h"

namespace {

using hvd::kEmptyKey;

__device__ __forceinline__ uint32_t capped(int32_t weight, uint32_t max_weight) {
    const uint32_t w = (uint32_t)weight;
    return max_weight != 0u && w > max_weight ? max_weight : w;
}

// src / pkeys / pcnt / counters as k_keys_to_pairs takes them, and the same key -> (a, b, is_q) rule (hvd::vkey_pair). The
// frame of a key is a query-side frame in the symmetric form and at a side-0 key (weight_q), a target-side frame at a side-1
// key (weight_t). A key set holds every key once, and the host clears pkeys AND pcnt before every pass (build_table), so a
// pass repeated after a table that was too small starts from zero sums: nothing is counted twice.
__global__ __launch_bounds__(256) void k_keys_to_pairs_weighted(
    const unsigned long long* __restrict__ src, unsigned long long n_src, const int32_t* __restrict__ vid_q,
    const int32_t* __restrict__ vid_t, int rect, const int32_t* __restrict__ weight_q, const int32_t* __restrict__ weight_t,
    uint32_t max_weight, unsigned long long* __restrict__ pkeys, uint2* __restrict__ pcnt, unsigned long long pmask,
    unsigned long long* __restrict__ counters) {
    for (unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x; idx < n_src;
         idx += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long k = src[idx];
        if (k == kEmptyKey) continue;
        const hvd::VideoPairOfKey p = hvd::vkey_pair(k, vid_q, vid_t, rect);
        bool is_new;
        const unsigned long long slot = hvd::table_insert(pkeys, pmask, ((unsigned long long)p.a << 32) | p.b, &is_new);
        if (slot == ~0ull) {
            atomicAdd(&counters[0], 1ull);
            continue;
        }
        const int32_t* __restrict__ weight = rect && hvd::vkey_side(k) != 0u ? weight_t : weight_q;
        atomicAdd(p.is_q ? &pcnt[slot].x : &pcnt[slot].y, capped(weight[hvd::vkey_frame(k)], max_weight));
    }
}

// Ownership as k_frame_runs': a workgroup takes 4 videos at a time, wave k video 4 g + k, and strides over the groups of four
// by the grid (hvd::kVideoWeightsMaxBlocks caps it). No barrier, no LDS, no atomic: a wave without a video goes on to its next
// group. The video index is wave-uniform, so its two offsets are scalar loads; the range is clamped to [0, n], so offsets that
// are no CSR over the n frames give other totals, never an access out of bounds. Lane l adds frames lo + l, lo + l + 64, ...
// in 64 bits; six lane exchanges fold the 64 partial sums, and lane 0 writes the total with one plain 8-byte store. A video
// however long stays on its one wave (the limit of DESIGN 4.19, here as there).
__global__ __launch_bounds__(256) void k_video_weights(const int32_t* __restrict__ weight, const long long* __restrict__ offsets,
                                                       uint32_t V, unsigned long long n, uint32_t max_weight,
                                                       long long* __restrict__ totals) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long groups = ((unsigned long long)V + 3ull) / 4ull;
    for (unsigned long long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const unsigned long long v = grp * 4ull + wave;
        if (v >= V) continue;
        unsigned long long lo = (unsigned long long)offsets[v], hi = (unsigned long long)offsets[v + 1u];
        hi = hi < n ? hi : n;
        lo = lo < hi ? lo : hi;
        unsigned long long sum = 0;
        for (unsigned long long f = lo + lane; f < hi; f += 64ull) sum += capped(weight[f], max_weight);
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) sum += (unsigned long long)__shfl_xor((long long)sum, step, 64);
        if (lane == 0u) totals[v] = (long long)sum;
    }
}

unsigned grid_for(unsigned long long n) {
    unsigned long long b = (n + 255ull) / 256ull;
    if (b < 1) b = 1;
    if (b > 16384ull) b = 16384ull;  // grid-stride kernel
    return (unsigned)b;
}

}  // namespace

namespace hvd {

hipError_t launch_keys_to_pairs_weighted(const unsigned long long* d_src, unsigned long long n_src, const int32_t* d_vid_q,
                                         const int32_t* d_vid_t, bool rect, const int32_t* d_weight_q, const int32_t* d_weight_t,
                                         uint32_t max_weight, unsigned long long* d_pkeys, void* d_pcnt, unsigned long long pmask,
                                         unsigned long long* d_counters, hipStream_t s) {
    if (n_src == 0) return hipSuccess;
    hipLaunchKernelGGL(k_keys_to_pairs_weighted, dim3(grid_for(n_src)), dim3(256), 0, s, d_src, n_src, d_vid_q, d_vid_t,
                       rect ? 1 : 0, d_weight_q, d_weight_t, max_weight, d_pkeys, (uint2*)d_pcnt, pmask, d_counters);
    return hipGetLastError();
}

// d_totals: int64[V]. One launch.
hipError_t launch_video_weights(const int32_t* d_weight, const long long* d_offsets, uint32_t V, unsigned long long n,
                                uint32_t max_weight, long long* d_totals, hipStream_t s) {
    if (V == 0) return hipSuccess;
    unsigned blocks = (V + 3u) / 4u;
    if (blocks > kVideoWeightsMaxBlocks) blocks = kVideoWeightsMaxBlocks;  // grid-stride
    hipLaunchKernelGGL(k_video_weights, dim3(blocks), dim3(256), 0, s, d_weight, d_offsets, V, n, max_weight, d_totals);
    return hipGetLastError();
}

}  // namespace hvd
