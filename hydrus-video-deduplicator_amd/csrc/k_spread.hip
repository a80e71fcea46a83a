// k_spread.hip -- the common-frame filter: frames that occur in many videos (a studio logo, a channel
// intro, an end card) are found from the key set of the video search and deleted before it.
//   * k_keys_to_spread   key set (frame f, video v) of hvd_devhash.h -> spread[f] = the number of keys frame f owns = the
//                        number of OTHER videos f occurs in (keys are distinct, frames of f's own video are never compared);
//   * k_keys_to_spread_cross  the key set of the rectangular search (new batch Q x library T), both sides: the
//                        number of T's videos a frame of Q occurs in, and the number of Q's videos a frame of T occurs in;
//   * k_common_rule      per video: count its frames with spread > max_videos, decide whether the video is an intro carrier
//                        (it has common frames and they are at most max_share per cent of it), write keep[f];
//   * k_gather_kept_i32  stream compaction of an int32 array by the keep flags (the positions of a library ride along with
//                        hvd_dev_compact_kept, which moves the hashes and rebuilds the CSR).
// O(keys) and O(frames) memory passes next to the O(frames^2) compare.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_devhash.h"
#include "hvd_kernels.h"
#include "hvd_scan_dev.h"

namespace {

using hvd::kEmptyKey;

// src: a table (kEmptyKey = free slot) or a dense list, as k_keys_to_pairs takes it. Side-1 keys (target frames of the
// rectangular form) are in another frame space and are skipped. Integer atomics: the result does not depend on scheduling.
// No per-wave combine of equal frames: mix64 scatters a frame's keys over the table, neighbouring slots hold other frames.
__global__ __launch_bounds__(256) void k_keys_to_spread(const unsigned long long* __restrict__ src, unsigned long long n_src,
                                                        unsigned long long n, int32_t* __restrict__ spread) {
    for (unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x; idx < n_src;
         idx += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long k = src[idx];
        if (k == kEmptyKey || hvd::vkey_side(k) != 0u) continue;
        const uint32_t f = hvd::vkey_frame(k);
        if (f < n) atomicAdd(&spread[f], 1);
    }
}

// The rectangular form's key set, both sides read: a side-0 key (query frame f, target video) adds one to
// spread_q[f], a side-1 key (target frame g, query video) one to spread_t[g]. Either output may be null: that side is skipped.
// The counts are ADDED to what the arrays hold (the launcher zeroes them, or not). src / n_src as k_keys_to_spread.
__global__ __launch_bounds__(256) void k_keys_to_spread_cross(const unsigned long long* __restrict__ src, unsigned long long n_src,
                                                              unsigned long long nq, unsigned long long nt,
                                                              int32_t* __restrict__ spread_q, int32_t* __restrict__ spread_t) {
    for (unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x; idx < n_src;
         idx += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long k = src[idx];
        if (k == kEmptyKey) continue;
        const bool target = hvd::vkey_side(k) != 0u;
        int32_t* const out = target ? spread_t : spread_q;
        const uint32_t f = hvd::vkey_frame(k);
        if (out != nullptr && f < (target ? nt : nq)) atomicAdd(&out[f], 1);
    }
}

constexpr uint32_t kWaveVideoMax = 2048;  // frames: a longer video is counted and swept by its whole workgroup

// A workgroup owns 4 videos, wave k video 4 b + k; a video of more than kWaveVideoMax frames is taken by all 4 waves
// together when its turn comes (the test is uniform over the workgroup, so every lane reaches the barriers). Two sweeps of
// the video's CSR range: the count of common frames, then -- the carrier test in between -- the keep flags. Ranges are
// clamped to [0, n]: offsets that are no CSR over the n frames give other flags, never an access out of bounds.
__global__ __launch_bounds__(256) void k_common_rule(const int32_t* __restrict__ spread, const long long* __restrict__ offsets,
                                                     uint32_t V, unsigned long long n, int max_videos, uint32_t max_share,
                                                     int32_t* __restrict__ keep) {
    __shared__ uint32_t part[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t k = 0; k < 4u; ++k) {
        const unsigned long long v = (unsigned long long)blockIdx.x * 4u + k;
        if (v >= V) break;
        unsigned long long lo = (unsigned long long)offsets[v], hi = (unsigned long long)offsets[v + 1u];
        hi = hi < n ? hi : n;
        lo = lo < hi ? lo : hi;
        const unsigned long long len = hi - lo;
        const bool wide = len > kWaveVideoMax;
        if (!wide && wave != k) continue;
        const uint32_t first = wide ? threadIdx.x : lane, step = wide ? 256u : 64u;
        uint32_t c = 0;
        for (unsigned long long f = lo + first; f < hi; f += step) c += spread[f] > max_videos ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        c = __shfl(c, 0);
        if (wide) {
            if (lane == 0u) part[wave] = c;
            __syncthreads();
            c = part[0] + part[1] + part[2] + part[3];
            __syncthreads();  // (part serves the next wide video of this workgroup)
        }
        const bool carrier = c > 0u && 100ull * c <= (unsigned long long)max_share * len;
        for (unsigned long long f = lo + first; f < hi; f += step) keep[f] = carrier && spread[f] > max_videos ? 0 : 1;
    }
}

// out[j] = in[f] for the j-th frame f with keep[f] >= 1 (block_prefix: k_keep_count + k_scan_block_sums over keep, bound 1)
__global__ __launch_bounds__(256) void k_gather_kept_i32(const int32_t* __restrict__ in, const int32_t* __restrict__ keep,
                                                         unsigned long long n, const uint32_t* __restrict__ block_prefix,
                                                         int32_t* __restrict__ out) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kScanBlk + threadIdx.x * 4u;
    bool kept[4];
    uint32_t before = keep_prefix(keep, n, 1, block_prefix, base, kept);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (kept[k]) out[before++] = in[base + k];  // (kept[k] implies base + k < n)
}

}  // namespace

namespace hvd {

// d_spread: int32[n], zeroed here on the same stream
hipError_t launch_keys_to_spread(const unsigned long long* d_src, unsigned long long n_src, unsigned long long n,
                                 int32_t* d_spread, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_spread, 0, 4 * (size_t)n, s);
    if (e != hipSuccess || n_src == 0) return e;
    unsigned long long blocks = (n_src + 255ull) / 256ull;
    if (blocks > 16384ull) blocks = 16384ull;  // grid-stride
    hipLaunchKernelGGL(k_keys_to_spread, dim3((unsigned)blocks), dim3(256), 0, s, d_src, n_src, n, d_spread);
    return hipGetLastError();
}

// d_spread_q: int32[nq], d_spread_t: int32[nt]; either may be null. Zeroed here on the same stream unless `accumulate`.
hipError_t launch_keys_to_spread_cross(const unsigned long long* d_src, unsigned long long n_src, unsigned long long nq,
                                       unsigned long long nt, bool accumulate, int32_t* d_spread_q, int32_t* d_spread_t,
                                       hipStream_t s) {
    if (!accumulate) {
        if (d_spread_q != nullptr && nq > 0)
            if (hipError_t e = hipMemsetAsync(d_spread_q, 0, 4 * (size_t)nq, s)) return e;
        if (d_spread_t != nullptr && nt > 0)
            if (hipError_t e = hipMemsetAsync(d_spread_t, 0, 4 * (size_t)nt, s)) return e;
    }
    if (n_src == 0 || nq == 0 || nt == 0 || (d_spread_q == nullptr && d_spread_t == nullptr)) return hipSuccess;
    unsigned long long blocks = (n_src + 255ull) / 256ull;
    if (blocks > 16384ull) blocks = 16384ull;  // grid-stride
    hipLaunchKernelGGL(k_keys_to_spread_cross, dim3((unsigned)blocks), dim3(256), 0, s, d_src, n_src, nq, nt, d_spread_q,
                       d_spread_t);
    return hipGetLastError();
}

hipError_t launch_common_rule(const int32_t* d_spread, const long long* d_offsets, uint32_t V, unsigned long long n,
                              int max_videos, int max_share, int32_t* d_keep, hipStream_t s) {
    if (n == 0 || V == 0) return hipSuccess;
    hipLaunchKernelGGL(k_common_rule, dim3((V + 3u) / 4u), dim3(256), 0, s, d_spread, d_offsets, V, n, max_videos,
                       (uint32_t)max_share, d_keep);
    return hipGetLastError();
}

// d_scratch: compact_scratch_bytes(n) (only the block sums are used). d_total: one uint64 (device), receives the kept count.
hipError_t launch_gather_kept_i32(const int32_t* d_in, const int32_t* d_keep, unsigned long long n, int32_t* d_out,
                                  void* d_scratch, unsigned long long* d_total, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned long long nb = (n + kScanBlk - 1) / kScanBlk;
    uint32_t* sums = (uint32_t*)d_scratch;
    hipLaunchKernelGGL(k_keep_count, dim3((unsigned)nb), dim3(256), 0, s, d_keep, n, 1, sums);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, s, sums, (uint32_t)nb, d_total);
    hipLaunchKernelGGL(k_gather_kept_i32, dim3((unsigned)nb), dim3(256), 0, s, d_in, d_keep, n, sums, d_out);
    return hipGetLastError();
}

}  // namespace hvd
