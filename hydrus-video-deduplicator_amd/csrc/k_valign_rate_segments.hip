// k_valign_rate_segments.hip -- rate-aware multi-segment time alignment of listed video pairs: a reel cut from
// several scenes whose pieces were also sped up or slowed down. k_valign_segments.hip peels up to eight lines of slope one off a
// pair, k_valign_rates.hip fits one line at the best of up to eight listed rates; this kernel peels up to max_segments lines and
// chooses the rate of each. The rule, integers only (include/hvd_mi355x.h has the full text), in the notation of
// hvd_valign_dev.h (H, votes, S, the tie order) and of its two siblings:
//   taken_a = taken_b = {};  for s = 1..K:
//     H_s = {(i, j) in H : i not in taken_a, j not in taken_b};  stop if H_s is empty;
//     for each rate r = (num, den), in list order:  delta_r = den p_b - num p_a;  slack_r = slack max(num, den);
//       votes_r, S_r, d*_r: the rule of k_valign on H_s, delta_r, slack_r;
//     w = the rate of the largest S_r(d*_r), ties to the earlier one;  stop if S_w(d*_w) < min_band_votes;
//     segment s = (d*_w, S_w(d*_w), the frames of a / of b with a hit of H_s within slack_w of d*_w at rate w, the rate w);
//     taken |= those frames;  stop if every frame of a, or every frame of b, is taken.
// The shape, the passes and the bounds checks are hvd_valign_dev.h's; this file is the loop of rounds x rates over them. The
// histogram of a pair is sized by its largest bins_r; behind it lie the flag words and the taken words, in one place for all
// rounds and rates. The hit bits (q_hits / t_hits) are set in round 1 at rate 0 only.
// The bound-skip: H_s only shrinks, so every S_r(d) -- and with it the value S_r(d*_r) of rate r's last evaluation -- is an upper
// bound ub_r of what rate r can reach in any later round. After round 1 a rate is passed over when a winner of the round exists
// and ub_r <= its S (r comes later in the list and loses ties, so it cannot win), and for good once ub_r < min_band_votes (it
// can only win a round that stops). The records are those of the rule with every rate evaluated every round.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_valign_dev.h"

namespace {

constexpr uint32_t kRecWords = sizeof(hvd_vrsegments) / 4u;
static_assert(sizeof(hvd_vrsegments) == 416 && sizeof(hvd_vrsegment) == 48 && sizeof(hvd_vrsegments) % 16 == 0 &&
                  offsetof(hvd_vrsegment, rate_num) == sizeof(hvd_vsegment) && offsetof(hvd_vrsegments, seg) == 32,
              "record layout");

// the operands of a launch, as the kernel keeps them in LDS; n_rates 0: a broken list
struct Operands {
    Libraries lib;
    const uint2* pairs;
    hvd_vrsegments* out;
    uint32_t M, max_dist, slack, nums, dens, n_rates, max_segments, min_band_votes, slot_words;
};

// BIG false: every pair whose largest histogram fits LDS, and the INT32_MIN record of a pair index out of range or of a broken
// list. BIG true: the pairs that do not fit LDS, each workgroup with its own slot of slot_words words at scratch (histogram,
// flag words, taken words); a pair that does not fit its slot gets the INT32_MIN record.
template <bool BIG>
__global__ __launch_bounds__(256) void k_valign_rate_segments(
    const uint4* __restrict__ hashes_q, const long long* __restrict__ offsets_q, uint32_t VQ, const int32_t* __restrict__ pos_q,
    const uint4* __restrict__ hashes_t, const long long* __restrict__ offsets_t, uint32_t VT, const int32_t* __restrict__ pos_t,
    const uint2* __restrict__ pairs, uint32_t M, uint32_t max_dist, uint32_t slack, uint32_t nums, uint32_t dens,
    uint32_t max_segments, uint32_t min_band_votes, uint32_t* __restrict__ scratch, uint32_t slot_words,
    hvd_vrsegments* __restrict__ out) {
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
    // The operands go through LDS once and are read back where they are used, as vector registers with short lives (the
    // arrangement of k_valign_segments): held in the scalar file over the pair loop, beside the state of the rounds, they spill.
    if (tid == 0)
        K = {{hashes_q, offsets_q, pos_q, hashes_t, offsets_t, pos_t, VQ, VT}, pairs, out, M, max_dist, slack, nums, dens,
             hvd::rate_list_length(nums, dens), min(max_segments, (uint32_t)HVD_ALIGN_MAX_SEGMENTS), max(min_band_votes, 1u),
             slot_words};
    __syncthreads();
#pragma unroll 1
    for (uint32_t p = blockIdx.x; p < K.M; p += gridDim.x) {
        const uint2 ab = K.pairs[p];
        const uint32_t slack = uni(K.slack), R = uni(K.n_rates);
        Spans spans = {0u, 0u, 0, 0};
        const Geometry geo = pair_geometry<true>(K.lib, ab, slack, K.nums, K.dens, R, &spans);
        if (geo.big() != BIG) continue;  // the other launch's pair (bad and empty pairs belong to the LDS launch)
        Side A = geo.A, B = geo.B;
        bool bad = geo.bad;
        const uint32_t nbins_max = (uint32_t)geo.bins, wa = (A.n + 31u) / 32u, wb = (B.n + 31u) / 32u;
        if (BIG && (unsigned long long)nbins_max + 2ull * (wa + wb) > K.slot_words) bad = true;  // no room in the slot
        // the record: zeroed here, then written word by word as its words become known (lane 0)
        hvd_vrsegments* rec = K.out + p;
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
        // the pair's lengths and the tolerance are what the inner loops turn on: back into the scalar file
        A.n = uni(A.n);
        B.n = uni(B.n);
        const uint32_t max_dist = uni(K.max_dist);  // (the limits of the rounds are read where they are used: fewer scalars live)
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
                const uint32_t slack_r = slack * max(num, den);
                const uint32_t core = uni(num * P.a + den * P.b + 1u), nbins = core + 2u * slack_r;  // (nbins <= nbins_max)
                const int32_t dmin = (int32_t)uni(den * (uint32_t)P.pb0 - num * (uint32_t)P.pa1);
                for (uint32_t k = tid; k < nbins; k += 256u) hist[k] = 0u;
                scan_pair<1, true, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, dmin, core, slack_r, 0,
                                         (s | r) == 0u, num, den);
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
            // (unrolled or interleaved, the bit-word loops keep loop-invariant lane masks that spill out of the scalar file)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
            scan_pair<2, true, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, 0, 0u, slack * max(num, den),
                                     win_d, true, num, den);
            hvd_vrsegment* seg = rec->seg + s;
            q_covered += store_aligned<false>(seg, flags, A, red);
            if (tid == 0) {
                seg->offset = win_d;
                seg->band_votes = win_S;
                seg->rate_num = num;
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

hipError_t launch_valign_rate_segments(const AlignMode& mode, const AlignOperands& op, hipStream_t s) {
    return launch_lds_then_scratch(op, [&](auto big, unsigned grid, uint32_t* scratch, uint32_t slot_words) {
        hipLaunchKernelGGL(k_valign_rate_segments<decltype(big)::value>, dim3(grid), dim3(256), 0, s, (const uint4*)op.hashes_q,
                           (const long long*)op.offsets_q, (uint32_t)op.VQ, (const int32_t*)op.pos_q, (const uint4*)op.hashes_t,
                           (const long long*)op.offsets_t, (uint32_t)op.VT, (const int32_t*)op.pos_t, (const uint2*)op.pairs,
                           (uint32_t)op.M, (uint32_t)op.max_dist, (uint32_t)op.slack, mode.nums, mode.dens,
                           (uint32_t)mode.max_segments, (uint32_t)mode.min_band_votes, scratch, slot_words, (hvd_vrsegments*)op.out);
    });
}

}  // namespace hvd
