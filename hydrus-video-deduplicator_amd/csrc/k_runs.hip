// k_runs.hip -- the static-scene filter: a run of near-identical consecutive frames of one video (a held
// shot, a slide, a title card, a freeze frame, frames repeated by a frame-rate conversion) keeps its first frame alone.
//   * k_frame_runs   per video, over its frames in CSR order: the first frame is the anchor and is kept; a later frame within
//                    max_dist bits of the ANCHOR (not of its predecessor: slow drift cannot chain a video into one run) is
//                    dropped while the anchor's run holds fewer than max_run frames (0 = no limit); any other frame is kept
//                    and becomes the anchor. keep[f] = 1 / 0; run[f] = the frames a kept frame stands for, 0 at a dropped one.
// The rule is sequential inside a video, so a video is one wave's: 64 frames per step, one per lane, and a ballot finds the
// next frame that opens a run. O(frames) memory traffic (32 B read, 8 B written per frame) next to the O(frames^2) compare.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_kernels.h"

namespace {

// Ownership as k_common_rule's: a workgroup takes 4 videos at a time, wave k video 4 g + k, and strides over the groups of
// four by the grid (hvd::kFrameRunsMaxBlocks caps it). No barrier, no LDS: a wave without a video goes on to its next group.
//
// A wave takes its video in chunks of 64 frames, lane l frame base + l, the hash loaded once as two 16-byte words and held in
// eight registers. The anchor is eight wave-uniform words with its frame index and its count. One pass of xor / popcount / add
// gives every lane its distance to the anchor; the ballot of "beyond max_dist" among the lanes not yet judged names the first
// lane p that opens a new run -- or the lane at which the run is full, when max_run is set and that comes earlier. Lanes
// before p are dropped, lane p's hash becomes the anchor by eight lane reads, and the lanes after p are judged again from the
// registers they hold: a chunk is never loaded twice, however many runs it contains (64 at the most).
//
// Every keep and run word is written exactly once, by a plain vector store. keep[f] and the run word of every frame but the
// current anchor go out at the end of the chunk (a run that opened and closed inside the chunk left its count in its lane's
// register); the anchor's own run word is written by one lane when its run closes in a later chunk, or at the video's end.
// run may be null. Ranges are clamped to [0, n]: offsets that are no CSR over the n frames give other flags, never an access
// out of bounds. A video however long stays on its one wave (open ends).
__global__ __launch_bounds__(256) void k_frame_runs(const uint4* __restrict__ hashes, const long long* __restrict__ offsets,
                                                    uint32_t V, unsigned long long n, uint32_t max_dist, uint32_t max_run,
                                                    int32_t* __restrict__ keep, int32_t* __restrict__ run) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long groups = ((unsigned long long)V + 3ull) / 4ull;
    for (unsigned long long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const unsigned long long v = grp * 4ull + wave;
        if (v >= V) continue;
        unsigned long long lo = (unsigned long long)offsets[v], hi = (unsigned long long)offsets[v + 1u];
        hi = hi < n ? hi : n;
        lo = lo < hi ? lo : hi;
        uint32_t a[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the anchor's hash,
        unsigned long long anchor = lo;                     // its frame
        uint32_t count = 0;                                 // and the frames of its run so far; 0: the video has not begun
        for (unsigned long long base = lo; base < hi; base += 64ull) {
            const uint32_t m = hi - base < 64ull ? (uint32_t)(hi - base) : 64u;  // frames of this chunk
            const unsigned long long f = base + lane;
            const bool valid = lane < m;
            uint32_t h[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            if (valid) {
                const uint4 x = hashes[2ull * f], y = hashes[2ull * f + 1ull];
                h[0] = x.x, h[1] = x.y, h[2] = x.z, h[3] = x.w, h[4] = y.x, h[5] = y.y, h[6] = y.z, h[7] = y.w;
            }
            int32_t kept = 0, mine = 0;  // this lane's keep and run words
            uint32_t start = 0;          // lanes below are judged; start < m at the top of every pass
            for (;;) {
                uint32_t p = 0;  // the lane that opens the next run (the video's first frame does)
                if (count != 0u) {
                    uint32_t d = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) d += (uint32_t)__popc(h[k] ^ a[k]);
                    const unsigned long long far = __ballot(valid && lane >= start && d > max_dist);
                    p = far != 0ull ? (uint32_t)__builtin_ctzll(far) : m;
                    if (max_run != 0u && start + (max_run - count) < p) p = start + (max_run - count);  // (count <= max_run)
                    count += p - start;  // lanes [start, p) are dropped
                    if (p >= m) break;
                    if (anchor >= base) {  // the run that closes here opened in this chunk: its lane keeps the count
                        if (lane == (uint32_t)(anchor - base)) mine = (int32_t)count;
                    } else if (run != nullptr && lane == 0u) {
                        run[anchor] = (int32_t)count;
                    }
                }
                const int src = __builtin_amdgcn_readfirstlane((int)p);
#pragma unroll
                for (int k = 0; k < 8; ++k) a[k] = (uint32_t)__builtin_amdgcn_readlane((int)h[k], src);
                if (lane == p) kept = 1;
                anchor = base + p;
                count = 1u;
                start = p + 1u;
                if (start >= m) break;
            }
            if (valid) {
                keep[f] = kept;
                if (run != nullptr && f != anchor) run[f] = mine;
            }
        }
        if (run != nullptr && count != 0u && lane == 0u) run[anchor] = (int32_t)count;
    }
}

}  // namespace

namespace hvd {

// d_keep: int32[n]; d_run: int32[n] or nullptr. One launch.
hipError_t launch_frame_runs(const void* d_hashes, const long long* d_offsets, uint32_t V, unsigned long long n, int max_dist,
                             int max_run, int32_t* d_keep, int32_t* d_run, hipStream_t s) {
    if (n == 0 || V == 0) return hipSuccess;
    unsigned blocks = (V + 3u) / 4u;
    if (blocks > kFrameRunsMaxBlocks) blocks = kFrameRunsMaxBlocks;  // grid-stride
    hipLaunchKernelGGL(k_frame_runs, dim3(blocks), dim3(256), 0, s, (const uint4*)d_hashes, d_offsets, V, n, (uint32_t)max_dist,
                       (uint32_t)max_run, d_keep, d_run);
    return hipGetLastError();
}

}  // namespace hvd
