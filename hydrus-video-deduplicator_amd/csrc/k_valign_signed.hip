// k_valign_signed.hip -- time alignment with negative rates: a clip played backwards, a "rewind" piece inside a
// reel, a reversed re-upload. The rule is k_valign_rate_segments.hip's rule, word for word, with signed numerators
// (include/hvd_mi355x.h has the full text): a rate (num, den) models p_b = (num / den) p_a + c, and num < 0 says that b runs
// backwards against a.
//   per rate r = (num, den):  delta_r = den p_b - num p_a;  slack_r = slack max(|num|, den);
//     bins_r = |num| span_a + den span_b + 1 + 2 slack_r;
//     the smallest delta is den p_b0 - num p_a1 for num > 0 and den p_b0 - num p_a0 for num < 0.
// The rounds, the taken sets, min_band_votes, the tie order, the bound-skip, the 2^20-bin limit at ANY listed rate, the INT32_MIN
// record and the zero record are the sibling's. The list travels as three words: nums and dens hold |num| and den, so
// pair_geometry<true> sizes the histogram as it does for the sibling, and bit r of revs says that entry r is negative. scan_pair
// multiplies the staged positions by its `num` in 32-bit wrap-around: handed num_s = 0 - |num| it forms
// delta = den p_b + |num| p_a with the code that is there. The shape, the passes and the bounds checks are hvd_valign_dev.h's;
// this file is the sibling's loop of rounds x rates over them. (One definition for the two files is left to a change that
// brings DESIGN.md 4.21's timing comparison with it.)
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_valign_dev.h"

namespace {

constexpr uint32_t kRecWords = sizeof(hvd_vssegments) / 4u;
static_assert(sizeof(hvd_vssegments) == 416 && sizeof(hvd_vssegment) == 48 && sizeof(hvd_vssegments) % 16 == 0 &&
                  offsetof(hvd_vssegment, rate_num) == sizeof(hvd_vsegment) && offsetof(hvd_vssegments, seg) == 32 &&
                  sizeof(hvd_vssegments) == sizeof(hvd_vrsegments) && offsetof(hvd_vssegment, rate_den) == offsetof(hvd_vrsegment, rate_den),
              "record layout");

// the operands of a launch, as the kernel keeps them in LDS; n_rates 0: a broken list
struct Operands {
    Libraries lib;
    const uint2* pairs;
    hvd_vssegments* out;
    uint32_t M, max_dist, slack, nums, dens, revs, n_rates, max_segments, min_band_votes, slot_words;
};

// BIG false: every pair whose largest histogram fits LDS, and the INT32_MIN record of a pair index out of range or of a broken
// list. BIG true: the pairs that do not fit LDS, each workgroup with its own slot of slot_words words at scratch (histogram,
// flag words, taken words); a pair that does not fit its slot gets the INT32_MIN record.
template <bool BIG>
__global__ __launch_bounds__(256) void k_valign_signed(
    const uint4* __restrict__ hashes_q, const long long* __restrict__ offsets_q, uint32_t VQ, const int32_t* __restrict__ pos_q,
    const uint4* __restrict__ hashes_t, const long long* __restrict__ offsets_t, uint32_t VT, const int32_t* __restrict__ pos_t,
    const uint2* __restrict__ pairs, uint32_t M, uint32_t max_dist, uint32_t slack, uint32_t nums, uint32_t dens, uint32_t revs,
    uint32_t max_segments, uint32_t min_band_votes, uint32_t* __restrict__ scratch, uint32_t slot_words,
    hvd_vssegments* __restrict__ out) {
    __shared__ uint32_t stage[kStage * 9u];
    __shared__ int32_t spos[kStage];
    __shared__ uint32_t lds_words[BIG ? 1u : kLdsBins + 2u * kFlagWords];  // histogram (of the largest bins_r), flag words, taken words
    __shared__ uint32_t red[12];
    __shared__ Best wbest[4];
    __shared__ Operands K;
    __shared__ Spans P;                           // of the pair at hand
    __shared__ uint32_t ub[HVD_ALIGN_MAX_RATES];  // of the pair at hand: S_r(d*_r) of rate r's last evaluation
    const uint32_t tid = threadIdx.x;
    uint32_t* const hist = BIG ? scratch + (size_t)blockIdx.x * slot_words : lds_words;
    // the operands go through LDS once and are read back where they are used (the arrangement of the sibling)
    if (tid == 0)
        K = {{hashes_q, offsets_q, pos_q, hashes_t, offsets_t, pos_t, VQ, VT}, pairs, out, M, max_dist, slack, nums, dens, revs,
             hvd::signed_rate_list_length(nums, dens, revs), min(max_segments, (uint32_t)HVD_ALIGN_MAX_SEGMENTS),
             max(min_band_votes, 1u), slot_words};
    __syncthreads();
#pragma unroll 1
    for (uint32_t p = blockIdx.x; p < K.M; p += gridDim.x) {
        const uint2 ab = K.pairs[p];
        const uint32_t slack = uni(K.slack), R = uni(K.n_rates);
        Spans spans = {0u, 0u, 0, 0};
        const Geometry geo = pair_geometry<true>(K.lib, ab, slack, K.nums, K.dens, R, &spans);  // (the magnitudes: bins_r)
        if (geo.big() != BIG) continue;  // the other launch's pair (bad and empty pairs belong to the LDS launch)
        Side A = geo.A, B = geo.B;
        bool bad = geo.bad;
        const uint32_t nbins_max = (uint32_t)geo.bins, wa = (A.n + 31u) / 32u, wb = (B.n + 31u) / 32u;
        if (BIG && (unsigned long long)nbins_max + 2ull * (wa + wb) > K.slot_words) bad = true;  // no room in the slot
        // the record: zeroed here, then written word by word as its words become known (lane 0)
        hvd_vssegments* rec = K.out + p;
        if (tid == 0) {
            uint4* w = (uint4*)rec;
            w[0] = make_uint4(ab.x, ab.y, 0u, 0u);
            w[1] = make_uint4(0u, 0u, 0u, 0u);
            w[2] = make_uint4(bad ? 0x80000000u : 0u, 0u, 0u, 0u);
#pragma unroll 1
            for (uint32_t k = 3; k < kRecWords / 4u; ++k) w[k] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (bad || geo.empty) continue;
        if (tid == 0) P = spans;  // (the rounds of the pair before read theirs ahead of a barrier of scan_pair's)
        __syncthreads();          // the pair before is done with LDS
        A.n = uni(A.n);
        B.n = uni(B.n);
        const uint32_t max_dist = uni(K.max_dist);
        uint32_t* const flags = hist + nbins_max;
        const uint32_t flagA = nbins_max, flagB = flagA + wa, takenA = flagB + wb, takenB = takenA + wa;
        // a scratch slot serves many pairs: the taken words are cleared per pair, like the flag words
        for (uint32_t k = tid; k < 2u * (wa + wb); k += 256u) flags[k] = 0u;  // (scan_pair opens with a barrier)
        uint32_t q_covered = 0, t_covered = 0;
#pragma unroll 1
        for (uint32_t s = 0; s < uni(K.max_segments); ++s) {
            // ---- pass 1 on what is left, rate by rate: the round's winner stays in three registers (win_r == R: none yet) ----
            uint32_t win_S = 0, win_r = R;
            int32_t win_d = 0;
#pragma unroll 1
            for (uint32_t r = 0; r < R; ++r) {
                if (s != 0u) {  // the bound-skip (ub[r] was written a barrier of scan_pair's ago at the least)
                    const uint32_t u = uni(ub[r]);
                    if (u < uni(K.min_band_votes) || (win_r != R && u <= win_S)) continue;
                }
                const uint32_t num = uni((K.nums >> (4u * r)) & 15u), den = uni((K.dens >> (4u * r)) & 15u);
                const uint32_t rev = uni((K.revs >> r) & 1u), num_s = uni(rev ? 0u - num : num);  // num as a two's-complement word
                const uint32_t slack_r = slack * max(num, den);
                const uint32_t core = uni(num * P.a + den * P.b + 1u), nbins = core + 2u * slack_r;  // (nbins <= nbins_max)
                // the smallest delta: a's last position under a positive num, its first (p_a1 - span_a) under a negative one
                const uint32_t pa_far = uni((uint32_t)P.pa1 - (rev ? P.a : 0u));
                const int32_t dmin = (int32_t)uni(den * (uint32_t)P.pb0 - num_s * pa_far);
                for (uint32_t k = tid; k < nbins; k += 256u) hist[k] = 0u;
                scan_pair<1, true, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, dmin, core, slack_r, 0,
                                         (s | r) == 0u, num_s, den);
                // H is empty: the round is left without a winner
                if ((s | r) == 0u && store_hit_counts(rec, flags, wa, A, B, red) == 0u) break;
                const Best best = best_offset<true>(hist, nbins, slack_r, dmin, wbest);
                if (tid == 0) ub[r] = best.S;
                if (win_r == R || best.S > win_S) {  // ties go to the earlier rate
                    win_S = best.S;
                    win_d = best.d;
                    win_r = r;
                }
            }
            // H is empty, or every rate was passed over; or H_s is empty (S = 0) or its best band is below the caller's floor
            if (win_r == R || win_S < uni(K.min_band_votes)) break;
            // ---- pass 2 at the winning rate: the frames of the segment ----
            const uint32_t num = uni((K.nums >> (4u * win_r)) & 15u), den = uni((K.dens >> (4u * win_r)) & 15u);
            const uint32_t num_s = uni((K.revs >> win_r) & 1u ? 0u - num : num);
            // (unrolled or interleaved, the bit-word loops keep loop-invariant lane masks that spill out of the scalar file)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
            scan_pair<2, true, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, 0, 0u, slack * max(num, den),
                                     win_d, true, num_s, den);
            hvd_vssegment* seg = rec->seg + s;
            q_covered += store_aligned<false>(seg, flags, A, red);
            if (tid == 0) {
                seg->offset = win_d;
                seg->band_votes = win_S;
                seg->rate_num = (int32_t)num_s;
                seg->rate_den = den;
                seg->rate_index = win_r;
                rec->q_covered = q_covered;
                rec->n_segments = s + 1u;
            }
            t_covered += store_aligned<true>(seg, flags + wa, B, red);
            if (tid == 0) rec->t_covered = t_covered;
            if (q_covered >= A.n || t_covered >= B.n) break;  // nothing is left of one side: no further pass
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[wa + wb + k] |= flags[k];  // taken |= aligned
        }
    }
}

}  // namespace

namespace hvd {

hipError_t launch_valign_signed(const AlignMode& mode, const AlignOperands& op, hipStream_t s) {
    return launch_lds_then_scratch(op, [&](auto big, unsigned grid, uint32_t* scratch, uint32_t slot_words) {
        hipLaunchKernelGGL(k_valign_signed<decltype(big)::value>, dim3(grid), dim3(256), 0, s, (const uint4*)op.hashes_q,
                           (const long long*)op.offsets_q, (uint32_t)op.VQ, (const int32_t*)op.pos_q, (const uint4*)op.hashes_t,
                           (const long long*)op.offsets_t, (uint32_t)op.VT, (const int32_t*)op.pos_t, (const uint2*)op.pairs,
                           (uint32_t)op.M, (uint32_t)op.max_dist, (uint32_t)op.slack, mode.nums, mode.dens, mode.revs,
                           (uint32_t)mode.max_segments, (uint32_t)mode.min_band_votes, scratch, slot_words, (hvd_vssegments*)op.out);
    });
}

}  // namespace hvd
