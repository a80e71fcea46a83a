// k_valign_segments.hip -- multi-segment time alignment of listed video pairs: a short video that is several
// pieces of a longer one (a highlight reel, a trailer, a re-cut). k_valign.hip fits one line p_b = p_a + d* per pair; this
// kernel peels up to max_segments of them, greedily. The rule, integers only (include/hvd_mi355x.h has the full text), in
// the notation of hvd_valign_dev.h (H, delta, votes, S, slack, the tie order):
//   taken_a = taken_b = {};  for r = 1..K:
//     H_r = {(i, j) in H : i not in taken_a, j not in taken_b};  votes, S, d*_r: the rule of k_valign on H_r;
//     stop if H_r is empty or S(d*_r) < min_band_votes;
//     segment r = (d*_r, S(d*_r), the frames of a / of b with a hit of H_r within slack of d*_r: number, first, last);
//     taken |= those frames;  stop if every frame of a, or every frame of b, is taken.
// The shape, the passes and the bounds checks are hvd_valign_dev.h's; this file is the loop of rounds over them. Per pair there
// are two more runs of bit words beside the flag words -- the taken sets, which the passes skip -- and the histogram is cleared
// every round. The hit bits (q_hits / t_hits) are set in round 1 only. Segment 1 is, word for word, the k_valign record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_valign_dev.h"

namespace {

constexpr uint32_t kRecWords = sizeof(hvd_vsegments) / 4u;
static_assert(sizeof(hvd_vsegments) == 288 && sizeof(hvd_vsegment) == 32 && sizeof(hvd_vsegments) % 16 == 0, "record layout");

// the operands of a launch, as the kernel keeps them in LDS
struct Operands {
    Libraries lib;
    const uint2* pairs;
    hvd_vsegments* out;
    uint32_t M, max_dist, slack, max_segments, min_band_votes, slot_words;
};

// BIG false: every pair whose histogram fits LDS, and the INT32_MIN record of a pair index out of range. BIG true: the pairs
// that do not fit LDS, each workgroup with its own slot of slot_words words at scratch (histogram, flag words, taken words); a
// pair that does not fit its slot gets the INT32_MIN record.
template <bool BIG>
__global__ __launch_bounds__(256) void k_valign_segments(const uint4* __restrict__ hashes_q, const long long* __restrict__ offsets_q,
                                                         uint32_t VQ, const int32_t* __restrict__ pos_q,
                                                         const uint4* __restrict__ hashes_t, const long long* __restrict__ offsets_t,
                                                         uint32_t VT, const int32_t* __restrict__ pos_t,
                                                         const uint2* __restrict__ pairs, uint32_t M, uint32_t max_dist,
                                                         uint32_t slack, uint32_t max_segments, uint32_t min_band_votes,
                                                         uint32_t* __restrict__ scratch, uint32_t slot_words,
                                                         hvd_vsegments* __restrict__ out) {
    __shared__ uint32_t stage[kStage * 9u];
    __shared__ int32_t spos[kStage];
    __shared__ uint32_t lds_words[BIG ? 1u : kLdsBins + 2u * kFlagWords];  // histogram, flag words, taken words
    __shared__ uint32_t red[12];
    __shared__ Best wbest[4];
    __shared__ Operands K;
    const uint32_t tid = threadIdx.x;
    uint32_t* const hist = BIG ? scratch + (size_t)blockIdx.x * slot_words : lds_words;
    // The operands go through LDS once and are read back where they are used, as vector registers with short lives: held
    // in the scalar file over the whole pair loop, beside the state of the rounds, they would spill.
    if (tid == 0)
        K = {{hashes_q, offsets_q, pos_q, hashes_t, offsets_t, pos_t, VQ, VT}, pairs, out, M, max_dist, slack,
             min(max_segments, (uint32_t)HVD_ALIGN_MAX_SEGMENTS), max(min_band_votes, 1u), slot_words};
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
        if (BIG && (unsigned long long)nbins + 2ull * (wa + wb) > K.slot_words) bad = true;  // no room in the slot
        // the record: zeroed here, then written word by word as its words become known (lane 0)
        hvd_vsegments* rec = K.out + p;
        if (tid == 0) {
            uint4* w = (uint4*)rec;
            w[0] = make_uint4(ab.x, ab.y, 0u, 0u);
            w[1] = make_uint4(0u, 0u, 0u, 0u);
            w[2] = make_uint4(bad ? 0x80000000u : 0u, 0u, 0u, 0u);
#pragma unroll 1
            for (uint32_t k = 3; k < kRecWords / 4u; ++k) w[k] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (bad || geo.empty) continue;
        __syncthreads();  // the pair before is done with LDS
        // the pair's lengths and the tolerance are what the inner loops turn on: back into the scalar file
        A.n = uni(A.n);
        B.n = uni(B.n);
        const uint32_t max_dist = uni(K.max_dist), max_segments = uni(K.max_segments), min_band_votes = uni(K.min_band_votes);
        uint32_t* const flags = hist + nbins;
        const uint32_t flagA = nbins, flagB = flagA + wa, takenA = flagB + wb, takenB = takenA + wa;
        const uint32_t core = nbins - 2u * slack;
        for (uint32_t k = tid; k < 2u * (wa + wb); k += 256u) flags[k] = 0u;  // (scan_pair opens with a barrier)
        uint32_t q_covered = 0, t_covered = 0;
#pragma unroll 1
        for (uint32_t r = 0; r < max_segments; ++r) {
            // ---- pass 1 on what is left ----
            for (uint32_t k = tid; k < nbins; k += 256u) hist[k] = 0u;
            scan_pair<1, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, dmin, core, slack, 0, r == 0u);
            uint32_t cnt, first, last;
            if (r == 0u) {
                count_bits(flags + wa, B.n, red, &cnt, &first, &last);
                if (tid == 0) rec->t_hits = cnt;
                count_bits(flags, A.n, red, &cnt, &first, &last);
                if (tid == 0) rec->q_hits = cnt;
                if (cnt == 0u) break;  // H is empty
            }
            const Best best = best_offset<true>(hist, nbins, slack, dmin, wbest);
            if (best.S < min_band_votes) break;  // H_r is empty (S = 0), or its best band is below the caller's floor
            // ---- pass 2: the frames of the segment ----
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
            scan_pair<2, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, dmin, core, slack, best.d, true);
            hvd_vsegment* seg = rec->seg + r;
            count_bits(flags, A.n, red, &cnt, &first, &last);
            q_covered += cnt;
            if (tid == 0) {
                seg->offset = best.d;
                seg->band_votes = best.S;
                seg->q_aligned = cnt;
                seg->q_first = pos_of(A, min(first, A.n - 1u));
                seg->q_last = pos_of(A, min(last, A.n - 1u));
                rec->q_covered = q_covered;
                rec->n_segments = r + 1u;
            }
            count_bits(flags + wa, B.n, red, &cnt, &first, &last);
            t_covered += cnt;
            if (tid == 0) {
                seg->t_aligned = cnt;
                seg->t_first = pos_of(B, min(first, B.n - 1u));
                seg->t_last = pos_of(B, min(last, B.n - 1u));
                rec->t_covered = t_covered;
            }
            if (q_covered >= A.n || t_covered >= B.n) break;  // nothing is left of one side: no further pass
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[wa + wb + k] |= flags[k];  // taken |= aligned
        }
    }
}

}  // namespace

namespace hvd {

hipError_t launch_valign_segments(const AlignMode& mode, const AlignOperands& op, hipStream_t s) {
    return launch_lds_then_scratch(op, [&](auto big, unsigned grid, uint32_t* scratch, uint32_t slot_words) {
        hipLaunchKernelGGL(k_valign_segments<decltype(big)::value>, dim3(grid), dim3(256), 0, s, (const uint4*)op.hashes_q,
                           (const long long*)op.offsets_q, (uint32_t)op.VQ, (const int32_t*)op.pos_q, (const uint4*)op.hashes_t,
                           (const long long*)op.offsets_t, (uint32_t)op.VT, (const int32_t*)op.pos_t, (const uint2*)op.pairs,
                           (uint32_t)op.M, (uint32_t)op.max_dist, (uint32_t)op.slack, (uint32_t)mode.max_segments,
                           (uint32_t)mode.min_band_votes, scratch, slot_words, (hvd_vsegments*)op.out);
    });
}

}  // namespace hvd
