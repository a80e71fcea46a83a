// k_valign_cover.hip -- coverage of a video by several others: a compilation of clips, a film next to its parts.
// k_valign.hip answers, per listed pair, which frames of either video lie on the pair's best band, counts them and throws the
// bit words away; this kernel is the same single-offset loop over hvd_valign_dev.h with one step more: after pass 2 the bit
// words of a side that holds at least min_aligned aligned frames are ORed into one bitmap over the frames of the library, so
// that the union over all of a video's partners stays on the device. The rule, integers only (include/hvd_mi355x.h has the
// full text), in the notation of hvd_valign_dev.h:
//   per pair (a, b): the hvd_valign record of k_valign, word for word; on_a / on_b = the aligned frames of a / of b;
//   the pair contributes on_a to video a iff a != b and |on_a| >= min_aligned, and on_b to video b iff a != b and
//   |on_b| >= min_aligned (a pair with the INT32_MIN record has no aligned frames);
//   per video v: covered = |union of what was contributed to v|, sources = the list entries that contributed,
//   best_single = the largest contribution, frames = the video's clamped length.
// The bitmap is flat: bit offsets[v] + i is frame i of video v, with the offsets clamped as pair_geometry clamps them, so a
// local flag word lands in two neighbouring global words, shifted by offsets[v] & 31; neighbouring videos share words, and the
// OR is a vector atomic. OR, add and max commute: the result does not depend on which workgroup arrives first. Every word
// index is checked against the bitmap's length before it is used. k_cover_count then counts each video's bit range.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_valign_dev.h"

namespace {

static_assert(sizeof(hvd_vcover) == 16 && offsetof(hvd_vcover, sources) == 4 && offsetof(hvd_vcover, best_single) == 8, "record layout");

// the operands of the alignment, as the kernel keeps them in LDS (the arrangement of k_valign_rates); what the cover step takes
// -- the bitmap, its length, the cover records, min_aligned -- stays in the scalar file: kernel arguments are known to be
// global memory, so the OR is a global atomic, not a flat one
struct Operands {
    Libraries lib;  // one library, on both sides
    const uint2* pairs;
    hvd_valign* out;
    uint32_t M, max_dist, slack, slot_words;
};

// The aligned frames of one side into the bitmap: flags = the side's run of flag words (bits past X.n are zero), first_bit =
// the side's first frame in the library. Lanes stride over the words; lane 0 counts the source.
__device__ __forceinline__ void contribute(uint32_t* __restrict__ bitmap, uint32_t words, hvd_vcover* __restrict__ cover,
                                           const uint32_t* flags, uint32_t n, unsigned long long first_bit, uint32_t video,
                                           uint32_t cnt) {
    const uint32_t shift = (uint32_t)first_bit & 31u;
    const unsigned long long w0 = first_bit >> 5;
    for (uint32_t k = threadIdx.x; k < (n + 31u) / 32u; k += 256u) {
        const uint32_t w = flags[k];
        if (w == 0u) continue;
        const unsigned long long g = w0 + k;
        const uint32_t lo = w << shift, hi = shift ? w >> (32u - shift) : 0u;
        if (lo && g < words) atomicOr(&bitmap[g], lo);
        if (hi && g + 1u < words) atomicOr(&bitmap[g + 1u], hi);
    }
    if (threadIdx.x == 0) {
        hvd_vcover* c = cover + video;
        atomicAdd(&c->sources, 1u);
        atomicMax(&c->best_single, cnt);
    }
}

// BIG false: every pair whose histogram fits LDS, and the INT32_MIN record of a pair index out of range. BIG true: the pairs
// that do not fit LDS, each workgroup with its own slot of slot_words words at scratch (histogram, then the flag words); a
// pair that does not fit its slot gets the INT32_MIN record and contributes nothing.
template <bool BIG>
__global__ __launch_bounds__(256) void k_valign_cover(const uint4* __restrict__ hashes, const long long* __restrict__ offsets,
                                                      uint32_t V, const int32_t* __restrict__ pos,
                                                      const uint2* __restrict__ pairs, uint32_t M, uint32_t max_dist,
                                                      uint32_t slack, uint32_t min_aligned, uint32_t* __restrict__ scratch,
                                                      uint32_t slot_words, hvd_valign* __restrict__ out,
                                                      uint32_t* __restrict__ bitmap, uint32_t bitmap_words,
                                                      hvd_vcover* __restrict__ cover) {
    __shared__ uint32_t stage[kStage * 9u];
    __shared__ int32_t spos[kStage];
    __shared__ uint32_t lds_words[BIG ? 1u : kLdsBins + kFlagWords];  // histogram, then the flag words
    __shared__ uint32_t red[12];
    __shared__ Best wbest[4];
    __shared__ Operands K;
    const uint32_t tid = threadIdx.x;
    uint32_t* const hist = BIG ? scratch + (size_t)blockIdx.x * slot_words : lds_words;
    // The operands go through LDS once and are read back where they are used, as vector registers with short lives: held in
    // the scalar file over the pair loop they spill (k_valign is at 106 SGPRs with four arguments fewer).
    if (tid == 0)
        K = {{hashes, offsets, pos, hashes, offsets, pos, V, V}, pairs, out, M, max_dist, slack, slot_words};
    __syncthreads();
#pragma unroll 1
    for (uint32_t p = blockIdx.x; p < K.M; p += gridDim.x) {
        const uint2 ab = K.pairs[p];
        const uint32_t slack = uni(K.slack);
        const Geometry geo = pair_geometry(K.lib, ab, slack);
        if (geo.big() != BIG) continue;  // the other launch's pair (bad and empty pairs belong to the LDS launch)
        Side A = geo.A, B = geo.B;
        const int32_t dmin = geo.dmin;
        bool bad = geo.bad;
        const uint32_t nbins = (uint32_t)geo.bins, wa = (A.n + 31u) / 32u, wb = (B.n + 31u) / 32u;
        if (BIG && (unsigned long long)nbins + wa + wb > K.slot_words) bad = true;  // no room in the slot
        // the record is written as its words become known (lane 0): nothing of it has to stay in registers over the passes
        hvd_valign* rec = K.out + p;
        if (tid == 0) {
            hvd_valign zero = {};
            zero.a = ab.x;
            zero.b = ab.y;
            if (bad) zero.offset = INT32_MIN;
            *rec = zero;
        }
        if (bad || geo.empty) continue;
        __syncthreads();  // the pair before is done with LDS
        // the pair's lengths and the tolerance are what the inner loops turn on: back into the scalar file
        A.n = uni(A.n);
        B.n = uni(B.n);
        const uint32_t max_dist = uni(K.max_dist);
        uint32_t* const flags = hist + nbins;
        // ---- pass 1 ----
        for (uint32_t k = tid; k < nbins; k += 256u) hist[k] = 0u;
        for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
        const uint32_t core = nbins - 2u * slack;
        scan_pair<1, false>(A, B, max_dist, stage, spos, hist, nbins, nbins + wa, 0u, 0u, dmin, core, slack, 0, true);
        if (store_hit_counts(rec, flags, wa, A, B, red) == 0u) continue;  // H is empty
        const Best best = best_offset<false>(hist, nbins, slack, dmin, wbest);
        if (tid == 0) {
            rec->offset = best.d;
            rec->band_votes = best.S;
        }
        // ---- pass 2 ----
        for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
        scan_pair<2, false>(A, B, max_dist, stage, spos, hist, nbins, nbins + wa, 0u, 0u, dmin, core, slack, best.d, true);
        const uint32_t on_a = store_aligned<false>(rec, flags, A, red);
        const uint32_t on_b = store_aligned<true>(rec, flags + wa, B, red);
        // ---- the cover: a side's bit words into the library's bitmap (the flag words stay as they are until the next pair) ----
        if (ab.x == ab.y) continue;
        if (on_a >= min_aligned)
            contribute(bitmap, bitmap_words, cover, flags, A.n, (unsigned long long)(A.hashes - hashes) >> 1, ab.x, on_a);
        if (on_b >= min_aligned)
            contribute(bitmap, bitmap_words, cover, flags + wa, B.n, (unsigned long long)(B.hashes - hashes) >> 1, ab.y, on_b);
    }
}

// One wave per video (grid-stride): the set bits of the video's range of the bitmap -> cover[v].covered, the clamped length
// -> cover[v].frames. The two end words are masked; a video inside one word takes both masks.
__global__ __launch_bounds__(256) void k_cover_count(const long long* __restrict__ offsets, uint32_t V,
                                                     const uint32_t* __restrict__ bitmap, uint32_t bitmap_words,
                                                     hvd_vcover* __restrict__ cover) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long waves = (unsigned long long)gridDim.x * 4u;
    const long long n_all = offsets[V];
#pragma unroll 1
    for (unsigned long long v = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6); v < V; v += waves) {
        const long long a0 = min(max(offsets[v], 0ll), n_all), a1 = min(max(offsets[v + 1u], a0), n_all);  // pair_geometry's clamp
        uint32_t c = 0;
        if (a1 > a0) {
            const unsigned long long first = (unsigned long long)a0 >> 5, last = (unsigned long long)(a1 - 1) >> 5;
            const uint32_t mask_first = 0xffffffffu << ((uint32_t)a0 & 31u), mask_last = 0xffffffffu >> (31u - ((uint32_t)(a1 - 1) & 31u));
            for (unsigned long long g = first + lane; g <= last; g += 64u) {
                if (g >= bitmap_words) break;
                uint32_t w = bitmap[g];
                if (g == first) w &= mask_first;
                if (g == last) w &= mask_last;
                c += __popc(w);
            }
        }
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        if (lane == 0) {
            cover[v].covered = c;
            cover[v].frames = (uint32_t)min(a1 - a0, 0xffffffffll);
        }
    }
}

}  // namespace

namespace hvd {

size_t cover_bitmap_bytes(unsigned long long n_frames) { return (size_t)(((n_frames + 31u) / 32u * 4u + 15u) & ~15ull); }

size_t cover_scratch_bytes(unsigned long long n_frames, unsigned long long max_bins) {
    return cover_bitmap_bytes(n_frames) + ((slot_scratch_bytes(max_bins, 1u) + 15u) & ~(size_t)15u);
}

// op.align.scratch: the bitmap (cover_bitmap_bytes(op.n_frames)), then the slots of the scratch launch
hipError_t launch_valign_cover(const CoverOperands& op, hipStream_t s) {
    const AlignOperands& al = op.align;
    const size_t bitmap_bytes = cover_bitmap_bytes((unsigned long long)op.n_frames);
    const uint32_t V = (uint32_t)al.VQ, bitmap_words = (uint32_t)(bitmap_bytes / 4u);
    uint32_t* const bitmap = (uint32_t*)al.scratch;
    hipError_t e = hipSuccess;
    if (bitmap_bytes && (e = hipMemsetAsync(bitmap, 0, bitmap_bytes, s)) != hipSuccess) return e;
    // (without a video there is nothing to clear or to count, but every listed pair still gets its INT32_MIN record)
    if (V && (e = hipMemsetAsync(op.cover, 0, sizeof(hvd_vcover) * (size_t)V, s)) != hipSuccess) return e;
    AlignOperands slots = al;
    slots.scratch = al.scratch_bytes > bitmap_bytes ? (char*)al.scratch + bitmap_bytes : nullptr;
    slots.scratch_bytes = al.scratch_bytes > bitmap_bytes ? al.scratch_bytes - bitmap_bytes : 0u;
    e = launch_lds_then_scratch(slots, [&](auto big, unsigned grid, uint32_t* scratch, uint32_t slot_words) {
        hipLaunchKernelGGL(k_valign_cover<decltype(big)::value>, dim3(grid), dim3(256), 0, s, (const uint4*)al.hashes_q,
                           (const long long*)al.offsets_q, V, (const int32_t*)al.pos_q, (const uint2*)al.pairs, (uint32_t)al.M,
                           (uint32_t)al.max_dist, (uint32_t)al.slack, (uint32_t)op.min_aligned, scratch, slot_words,
                           (hvd_valign*)al.out, bitmap, bitmap_words, (hvd_vcover*)op.cover);
    });
    if (e != hipSuccess || V == 0u) return e;
    const unsigned count_grid = (unsigned)(((unsigned long long)V + 3u) / 4u < 4096ull ? ((unsigned long long)V + 3u) / 4u : 4096ull);
    hipLaunchKernelGGL(k_cover_count, dim3(count_grid), dim3(256), 0, s, (const long long*)al.offsets_q, V, (const uint32_t*)bitmap,
                       bitmap_words, (hvd_vcover*)op.cover);
    return hipGetLastError();
}

}  // namespace hvd
