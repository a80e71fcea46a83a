// k_vmatch.hip -- the parts of the video-level search (K3, BASELINE config 5) that are not the all-pairs
// kernel itself:
//   * reduction of the device set of (frame, video) keys (hvd_devhash.h) to per-video-pair vPDQ counters
//     (q_hits = distinct frames of a with a match in b, t_hits the converse; vpdqpy/vpdqpy.py:49-56) and their
//     emission as hvd_vmatch records;
//   * list <-> set conversion for the key exchange between ranks (each rank sees only its tiles' hits, a key
//     may be found by two ranks);
//   * VideoHasher.finish() for a whole library on the device: stream compaction of the frames with
//     quality >= tolerance, per-video CSR offsets and the frame -> video map (vpdqpy/vpdqpy.py:119,
//     db/DedupeDB.py:550-553, dedup.py:74-86), so that frames -> hashes -> search never leaves HBM; its dihedral form
//     also lays out the query set of the transformed search.
// All of this is O(frames) byte shuffling next to the O(frames^2) compare; none of it is on the roofline.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_devhash.h"
#include "hvd_kernels.h"
#include "hvd_scan_dev.h"

namespace {

using hvd::kEmptyKey;

// ---- set of keys -> pair map ---------------------------------------------------------------------------------
// src: either a table (slots entries, kEmptyKey = free) or a dense list. pkeys/pcnt: open-addressing map
// (a<<32|b) -> (q_hits, t_hits).
__global__ __launch_bounds__(256) void k_keys_to_pairs(const unsigned long long* __restrict__ src, unsigned long long n_src,
                                                       const int32_t* __restrict__ vid_q, const int32_t* __restrict__ vid_t,
                                                       int rect, unsigned long long* __restrict__ pkeys,
                                                       uint2* __restrict__ pcnt, unsigned long long pmask,
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
        atomicAdd(p.is_q ? &pcnt[slot].x : &pcnt[slot].y, 1u);
    }
}

__global__ __launch_bounds__(256) void k_pairs_emit(const unsigned long long* __restrict__ pkeys,
                                                    const uint2* __restrict__ pcnt, unsigned long long slots,
                                                    hvd_vmatch* __restrict__ out, unsigned long long cap,
                                                    unsigned long long* __restrict__ count) {
    for (unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x; idx < slots;
         idx += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long k = pkeys[idx];
        if (k == kEmptyKey) continue;
        const unsigned long long o = atomicAdd(count, 1ull);
        if (o < cap) {
            hvd_vmatch m;
            m.a = (uint32_t)(k >> 32);
            m.b = (uint32_t)k;
            m.q_hits = pcnt[idx].x;
            m.t_hits = pcnt[idx].y;
            out[o] = m;
        }
    }
}

// table -> dense list (for the exchange between ranks); count[0] receives the number of keys
__global__ __launch_bounds__(256) void k_set_to_list(const unsigned long long* __restrict__ tab, unsigned long long slots,
                                                     unsigned long long* __restrict__ list, unsigned long long cap,
                                                     unsigned long long* __restrict__ count) {
    for (unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x; idx < slots;
         idx += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long k = tab[idx];
        if (k == kEmptyKey) continue;
        const unsigned long long o = atomicAdd(count, 1ull);
        if (o < cap) list[o] = k;
    }
}

// dense list (kEmptyKey entries = padding of the all-gather) -> table, de-duplicating
__global__ __launch_bounds__(256) void k_list_to_set(const unsigned long long* __restrict__ list, unsigned long long n,
                                                     unsigned long long* __restrict__ tab, unsigned long long mask,
                                                     unsigned long long* __restrict__ counters) {
    for (unsigned long long idx = (unsigned long long)blockIdx.x * 256u + threadIdx.x; idx < n;
         idx += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long k = list[idx];
        if (k == kEmptyKey) continue;
        bool is_new;
        const unsigned long long slot = hvd::table_insert(tab, mask, k, &is_new);
        if (slot == ~0ull)
            atomicAdd(&counters[0], 1ull);
        else if (is_new)
            atomicAdd(&counters[1], 1ull);
    }
}

// ---- quality filter: stream compaction + CSR ---------------------------------------------------------------
constexpr uint32_t kBlk = kScanBlk;  // frames per workgroup; k_keep_count, k_scan_block_sums, keep_prefix: hvd_scan_dev.h

__device__ __forceinline__ uint32_t video_of_frame(const long long* __restrict__ offsets, uint32_t V, unsigned long long f) {
    // last v with offsets[v] <= f (empty videos share an offset with their successor and own no frame)
    uint32_t lo = 0, hi = V;  // invariant: offsets[lo] <= f < offsets[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((unsigned long long)offsets[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

// pos[f] = number of kept frames before raw frame f; kept frames are copied to their slot together with their
// video index
__global__ __launch_bounds__(256) void k_keep_scatter(const uint4* __restrict__ hashes, const int32_t* __restrict__ quality,
                                                      unsigned long long n, int min_q,
                                                      const uint32_t* __restrict__ block_prefix,
                                                      const long long* __restrict__ offsets, uint32_t V,
                                                      uint4* __restrict__ out_hashes, int32_t* __restrict__ out_video,
                                                      uint32_t* __restrict__ pos) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kBlk + threadIdx.x * 4u;
    bool keep[4];
    uint32_t before = keep_prefix(quality, n, min_q, block_prefix, base, keep);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long f = base + k;
        if (f >= n) break;
        pos[f] = before;
        if (keep[k]) {
            out_hashes[(size_t)before * 2u] = hashes[f * 2u];
            out_hashes[(size_t)before * 2u + 1u] = hashes[f * 2u + 1u];
            out_video[before] = (int32_t)video_of_frame(offsets, V, f);
            ++before;
        }
    }
}

// k_keep_scatter without the hash copy (the dihedral compaction moves the hashes in k_keep_variants, once the per-video
// kept lengths are known)
__global__ __launch_bounds__(256) void k_keep_positions(const int32_t* __restrict__ quality, unsigned long long n, int min_q,
                                                        const uint32_t* __restrict__ block_prefix,
                                                        const long long* __restrict__ offsets, uint32_t V,
                                                        int32_t* __restrict__ out_video, uint32_t* __restrict__ pos) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kBlk + threadIdx.x * 4u;
    bool keep[4];
    uint32_t before = keep_prefix(quality, n, min_q, block_prefix, base, keep);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long f = base + k;
        if (f >= n) break;
        pos[f] = before;
        if (keep[k]) out_video[before++] = (int32_t)video_of_frame(offsets, V, f);
    }
}

// The raw index inside its video of every kept frame, in kept order (the keep rule and the prefix of k_keep_scatter): the
// timeline of the alignment (k_valign.hip), which a dropped fade or black frame must not shift.
__global__ __launch_bounds__(256) void k_kept_positions(const int32_t* __restrict__ quality, unsigned long long n, int min_q,
                                                        const uint32_t* __restrict__ block_prefix,
                                                        const long long* __restrict__ offsets, uint32_t V,
                                                        int32_t* __restrict__ out_pos) {
    const unsigned long long base = (unsigned long long)blockIdx.x * kBlk + threadIdx.x * 4u;
    bool keep[4];
    uint32_t before = keep_prefix(quality, n, min_q, block_prefix, base, keep);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long f = base + k;
        if (f >= n) break;
        if (keep[k]) out_pos[before++] = (int32_t)(f - (unsigned long long)offsets[video_of_frame(offsets, V, f)]);
    }
}

__global__ __launch_bounds__(256) void k_keep_offsets(const long long* __restrict__ offsets, uint32_t V, unsigned long long n,
                                                      const uint32_t* __restrict__ pos,
                                                      const unsigned long long* __restrict__ total,
                                                      long long* __restrict__ out_offsets) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u > V) return;
    const unsigned long long r = (unsigned long long)offsets[u];
    out_offsets[u] = r >= n ? (long long)total[0] : (long long)pos[r];
}

// Dihedral compaction, hash pass: every selected variant of every kept frame is read once and written to its place.
// hashes8: n x 8 x 32 B (transform-minor). S selected variants, sel = their transform indices, 4 bits each, identity
// (0) first. One lane per 16 B chunk: a frame takes 2S lanes of a group of 1 << lg_w (lanes past 2S idle), so the
// selected bytes of a frame are read by neighbouring lanes. Variant 0 goes to the identity library at the frame's kept
// index j; variant s > 0 (k = s - 1, K = S - 1) of a frame at position i of video v (kept offset o, kept length L) goes
// to query slot K*o + k*L + i, query video v*K + k, exclusion id v -- the host layout of search.transformed_pairs.
__global__ __launch_bounds__(256) void k_keep_variants(const uint4* __restrict__ hashes8, const int32_t* __restrict__ quality,
                                                       unsigned long long n, int min_q, const uint32_t* __restrict__ pos,
                                                       const int32_t* __restrict__ kept_video,
                                                       const long long* __restrict__ kept_offsets, uint32_t sel, uint32_t S,
                                                       uint32_t lg_w, unsigned long long q_cap,
                                                       uint4* __restrict__ out_hashes, uint4* __restrict__ q_hashes,
                                                       int32_t* __restrict__ q_video, int32_t* __restrict__ q_excl) {
    const uint32_t c = threadIdx.x & ((1u << lg_w) - 1u);
    if (c >= 2u * S) return;
    const uint32_t s = c >> 1, half = c & 1u, t = (sel >> (4u * s)) & 7u, K = S - 1u;
    const uint32_t per = 256u >> lg_w;  // frames per workgroup and step
    for (unsigned long long f = (unsigned long long)blockIdx.x * per + (threadIdx.x >> lg_w); f < n;
         f += (unsigned long long)gridDim.x * per) {
        if (quality[f] < min_q) continue;
        const uint4 val = hashes8[f * 16u + t * 2u + half];
        const unsigned long long j = pos[f];
        if (s == 0u) {
            out_hashes[j * 2u + half] = val;
            continue;
        }
        const uint32_t v = (uint32_t)kept_video[j];
        const unsigned long long o = (unsigned long long)kept_offsets[v];
        const unsigned long long len = (unsigned long long)kept_offsets[v + 1u] - o;
        const unsigned long long slot = K * o + (s - 1u) * len + (j - o);
        if (slot >= q_cap) continue;  // only raw offsets that are no CSR over the n frames get here
        q_hashes[slot * 2u + half] = val;
        if (half == 0u) {
            q_video[slot] = (int32_t)(v * K + s - 1u);
            q_excl[slot] = (int32_t)v;
        }
    }
}

// frame -> video map from CSR offsets (for libraries that arrive as hashes + offsets)
__global__ __launch_bounds__(256) void k_video_of_frames(const long long* __restrict__ offsets, uint32_t V, unsigned long long n,
                                                         int32_t* __restrict__ out_video) {
    const unsigned long long f = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (f < n) out_video[f] = (int32_t)video_of_frame(offsets, V, f);
}

unsigned grid_for(unsigned long long n) {
    unsigned long long b = (n + 255ull) / 256ull;
    if (b < 1) b = 1;
    if (b > 16384ull) b = 16384ull;  // grid-stride kernels
    return (unsigned)b;
}

}  // namespace

namespace hvd {

hipError_t launch_keys_to_pairs(const unsigned long long* d_src, unsigned long long n_src, const int32_t* d_vid_q,
                                const int32_t* d_vid_t, bool rect, unsigned long long* d_pkeys, void* d_pcnt,
                                unsigned long long pmask, unsigned long long* d_counters, hipStream_t s) {
    if (n_src == 0) return hipSuccess;
    hipLaunchKernelGGL(k_keys_to_pairs, dim3(grid_for(n_src)), dim3(256), 0, s, d_src, n_src, d_vid_q, d_vid_t, rect ? 1 : 0,
                       d_pkeys, (uint2*)d_pcnt, pmask, d_counters);
    return hipGetLastError();
}

hipError_t launch_pairs_emit(const unsigned long long* d_pkeys, const void* d_pcnt, unsigned long long slots, hvd_vmatch* d_out,
                             unsigned long long cap, unsigned long long* d_count, hipStream_t s) {
    hipLaunchKernelGGL(k_pairs_emit, dim3(grid_for(slots)), dim3(256), 0, s, d_pkeys, (const uint2*)d_pcnt, slots, d_out, cap,
                       d_count);
    return hipGetLastError();
}

hipError_t launch_set_to_list(const unsigned long long* d_tab, unsigned long long slots, unsigned long long* d_list,
                              unsigned long long cap, unsigned long long* d_count, hipStream_t s) {
    hipLaunchKernelGGL(k_set_to_list, dim3(grid_for(slots)), dim3(256), 0, s, d_tab, slots, d_list, cap, d_count);
    return hipGetLastError();
}

hipError_t launch_list_to_set(const unsigned long long* d_list, unsigned long long n, unsigned long long* d_tab,
                              unsigned long long mask, unsigned long long* d_counters, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_list_to_set, dim3(grid_for(n)), dim3(256), 0, s, d_list, n, d_tab, mask, d_counters);
    return hipGetLastError();
}

size_t compact_scratch_bytes(unsigned long long n) {
    const unsigned long long nb = (n + kBlk - 1) / kBlk;
    return (size_t)(4ull * (nb + 1) + 4ull * (n + 1) + 16ull);
}

// d_scratch: compact_scratch_bytes(n). d_total: one uint64 (device) receiving the kept count.
hipError_t launch_compact_kept(const void* d_hashes, const int32_t* d_quality, unsigned long long n, const long long* d_offsets,
                               uint32_t V, int min_q, void* d_out_hashes, long long* d_out_offsets, int32_t* d_out_video,
                               void* d_scratch, unsigned long long* d_total, hipStream_t s) {
    const unsigned long long nb = (n + kBlk - 1) / kBlk;
    uint32_t* sums = (uint32_t*)d_scratch;
    uint32_t* pos = sums + (nb + 1);
    if (n > 0) {
        hipLaunchKernelGGL(k_keep_count, dim3((unsigned)nb), dim3(256), 0, s, d_quality, n, min_q, sums);
        hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, s, sums, (uint32_t)nb, d_total);
        hipLaunchKernelGGL(k_keep_scatter, dim3((unsigned)nb), dim3(256), 0, s, (const uint4*)d_hashes, d_quality, n, min_q,
                           sums, d_offsets, V, (uint4*)d_out_hashes, d_out_video, pos);
    } else {
        hipError_t e = hipMemsetAsync(d_total, 0, 8, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_keep_offsets, dim3((V + 1u + 255u) / 256u), dim3(256), 0, s, d_offsets, V, n, pos, d_total,
                       d_out_offsets);
    return hipGetLastError();
}

// Dihedral form of launch_compact_kept. mask: bit t = transform t of the 8 hashes per frame (bit 0 set). The identity
// library (out_hashes, out_offsets, out_video) is what launch_compact_kept makes of the plain hashes; q_*: the query
// library of the K = popcount(mask) - 1 other variants (k_keep_variants).
hipError_t launch_compact_kept_dihedral(const void* d_hashes8, const int32_t* d_quality, unsigned long long n,
                                        const long long* d_offsets, uint32_t V, int min_q, uint32_t mask, void* d_out_hashes,
                                        long long* d_out_offsets, int32_t* d_out_video, void* d_q_hashes, int32_t* d_q_video,
                                        int32_t* d_q_excl, void* d_scratch, unsigned long long* d_total, hipStream_t s) {
    const unsigned long long nb = (n + kBlk - 1) / kBlk;
    uint32_t* sums = (uint32_t*)d_scratch;
    uint32_t* pos = sums + (nb + 1);
    if (n > 0) {
        hipLaunchKernelGGL(k_keep_count, dim3((unsigned)nb), dim3(256), 0, s, d_quality, n, min_q, sums);
        hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, s, sums, (uint32_t)nb, d_total);
        hipLaunchKernelGGL(k_keep_positions, dim3((unsigned)nb), dim3(256), 0, s, d_quality, n, min_q, sums, d_offsets, V,
                           d_out_video, pos);
    } else {
        hipError_t e = hipMemsetAsync(d_total, 0, 8, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_keep_offsets, dim3((V + 1u + 255u) / 256u), dim3(256), 0, s, d_offsets, V, n, pos, d_total,
                       d_out_offsets);
    if (n > 0) {
        uint32_t sel = 0, S = 0;
        for (uint32_t t = 0; t < 8u; ++t)
            if (mask >> t & 1u) sel |= t << (4u * S++);
        uint32_t lg_w = 1;
        while ((1u << lg_w) < 2u * S) ++lg_w;
        const unsigned long long groups = (n + (256u >> lg_w) - 1u) / (256u >> lg_w);
        hipLaunchKernelGGL(k_keep_variants, dim3((unsigned)(groups < 16384ull ? groups : 16384ull)), dim3(256), 0, s,
                           (const uint4*)d_hashes8, d_quality, n, min_q, pos, d_out_video, d_out_offsets, sel, S, lg_w,
                           (unsigned long long)(S - 1u) * n, (uint4*)d_out_hashes, (uint4*)d_q_hashes, d_q_video, d_q_excl);
    }
    return hipGetLastError();
}

// d_scratch: compact_scratch_bytes(n) (only the block sums are used). d_total: one uint64 (device), receives the kept count.
hipError_t launch_kept_positions(const int32_t* d_quality, unsigned long long n, const long long* d_offsets, uint32_t V, int min_q,
                                 int32_t* d_out_pos, void* d_scratch, unsigned long long* d_total, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned long long nb = (n + kBlk - 1) / kBlk;
    uint32_t* sums = (uint32_t*)d_scratch;
    hipLaunchKernelGGL(k_keep_count, dim3((unsigned)nb), dim3(256), 0, s, d_quality, n, min_q, sums);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, s, sums, (uint32_t)nb, d_total);
    hipLaunchKernelGGL(k_kept_positions, dim3((unsigned)nb), dim3(256), 0, s, d_quality, n, min_q, sums, d_offsets, V, d_out_pos);
    return hipGetLastError();
}

hipError_t launch_video_of_frames(const long long* d_offsets, uint32_t V, unsigned long long n, int32_t* d_out_video,
                                  hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_video_of_frames, dim3((unsigned)((n + 255ull) / 256ull)), dim3(256), 0, s, d_offsets, V, n,
                       d_out_video);
    return hipGetLastError();
}

}  // namespace hvd
