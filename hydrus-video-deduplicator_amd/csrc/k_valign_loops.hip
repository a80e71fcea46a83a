// k_valign_loops.hip -- time alignment where a frame of the source serves more than once: a looped clip, a
// ping-pong / boomerang GIF, a 3-second moment of a film repeated for a minute. The rule is k_valign_signed.hip's rule with two
// changes (include/hvd_mi355x.h has the full text): video b has no taken set, and the rounds go on past the eight segments a
// record stores.
//   round r works on H_r = the hits of H whose frame OF A no earlier round owns; votes, S, d*, the winning rate, the tie order
//   and the bound-skip are the sibling's on H_r (H_{r+1} is a subset of H_r, so a rate's S never grows and the skip stays sound);
//   the frames of a within slack_r of d* join taken_a, those of b join seen_b, which is counted and never consulted;
//   the pair ends when a round's best band is below min_band_votes, when taken_a holds every frame of a, or after max_rounds.
// The loop is therefore the a side: b's frames serve any number of rounds, a's serve one.
// A record stores the first eight rounds as segments; a later round adds to rounds, q_covered and t_covered only.
// q_covered = |taken_a| (the rounds' frames of a are disjoint), t_covered = |seen_b|, DISTINCT frames of b.
// Behind the histogram lie runs of bit words, wa for a and wb for b each time: the flag words of a and of b; then the taken words
// of a and the seen words of b, side by side as the sibling's two taken runs are, so that its one loop `taken |= aligned` serves
// both; then wb words that stay zero for the whole pair, which scan_pair<., true, true> reads as b's taken words -- scan_pair
// itself is unchanged. A slot is sized for three pairs of runs (AlignMode::slot_runs() = 3). seen_b is counted once, after the last
// round, and rec->t_covered is written only then (rounds and q_covered are written round by round); a record is read after the
// kernel, so nothing sees the difference. The shape, the passes and the bounds checks are hvd_valign_dev.h's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_valign_dev.h"

namespace {

constexpr uint32_t kRecWords = sizeof(hvd_vloops) / 4u;
static_assert(sizeof(hvd_vloops) == 416 && sizeof(hvd_vloops) % 16 == 0 && offsetof(hvd_vloops, seg) == 32 &&
                  offsetof(hvd_vloops, rounds) == offsetof(hvd_vssegments, reserved) &&
                  offsetof(hvd_vloops, t_covered) == offsetof(hvd_vssegments, t_covered) && sizeof(hvd_vssegment) == 48,
              "record layout");
static_assert(HVD_ALIGN_MAX_ROUNDS >= HVD_ALIGN_MAX_SEGMENTS, "the stored segments are the first rounds");

// the operands of a launch, as the kernel keeps them in LDS; n_rates 0: a broken list
struct Operands {
    Libraries lib;
    const uint2* pairs;
    hvd_vloops* out;
    uint32_t M, max_dist, slack, nums, dens, revs, n_rates, max_rounds, min_band_votes, slot_words;
};

// BIG false: every pair whose largest histogram fits LDS, and the INT32_MIN record of a pair index out of range or of a broken
// list. BIG true: the pairs that do not fit LDS, each workgroup with its own slot of slot_words words at scratch (histogram,
// flag words, taken words, seen words); a pair that does not fit its slot gets the INT32_MIN record.
template <bool BIG>
__global__ __launch_bounds__(256) void k_valign_loops(
    const uint4* __restrict__ hashes_q, const long long* __restrict__ offsets_q, uint32_t VQ, const int32_t* __restrict__ pos_q,
    const uint4* __restrict__ hashes_t, const long long* __restrict__ offsets_t, uint32_t VT, const int32_t* __restrict__ pos_t,
    const uint2* __restrict__ pairs, uint32_t M, uint32_t max_dist, uint32_t slack, uint32_t nums, uint32_t dens, uint32_t revs,
    uint32_t max_rounds, uint32_t min_band_votes, uint32_t* __restrict__ scratch, uint32_t slot_words,
    hvd_vloops* __restrict__ out) {
    __shared__ uint32_t stage[kStage * 9u];
    __shared__ int32_t spos[kStage];
    __shared__ uint32_t lds_words[BIG ? 1u : kLdsBins + 3u * kFlagWords];  // histogram (of the largest bins_r), flag, taken, seen words
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
             hvd::signed_rate_list_length(nums, dens, revs), min(max_rounds, (uint32_t)HVD_ALIGN_MAX_ROUNDS),
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
        if (BIG && (unsigned long long)nbins_max + 3ull * (wa + wb) > K.slot_words) bad = true;  // no room in the slot
        // the record: zeroed here, then written word by word as its words become known (lane 0)
        hvd_vloops* rec = K.out + p;
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
        // flag words of a, of b | taken words of a, seen words of b | the words scan_pair reads as taken words of b: never written
        const uint32_t flagA = nbins_max, flagB = flagA + wa, takenA = flagB + wb, takenB = takenA + wa + wb;
        // a scratch slot serves many pairs: the taken and the seen words are cleared per pair, like the flag words
        for (uint32_t k = tid; k < 2u * (wa + wb) + wb; k += 256u) flags[k] = 0u;  // (scan_pair opens with a barrier)
        uint32_t q_covered = 0;
#pragma unroll 1
        for (uint32_t s = 0; s < uni(K.max_rounds); ++s) {
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
            // ---- pass 2 at the winning rate: the frames of the round ----
            const uint32_t num = uni((K.nums >> (4u * win_r)) & 15u), den = uni((K.dens >> (4u * win_r)) & 15u);
            const uint32_t num_s = uni((K.revs >> win_r) & 1u ? 0u - num : num);
            // (unrolled or interleaved, the bit-word loops keep loop-invariant lane masks that spill out of the scalar file)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
            scan_pair<2, true, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, 0, 0u, slack * max(num, den),
                                     win_d, true, num_s, den);
            // the first eight rounds are the record's segments; a later one writes none and only counts
            uint32_t cnt, first, last;
            count_bits(flags, A.n, red, &cnt, &first, &last);
            q_covered += cnt;
            if (tid == 0) {
                if (s < (uint32_t)HVD_ALIGN_MAX_SEGMENTS) {
                    hvd_vssegment* seg = rec->seg + s;
                    seg->q_aligned = cnt;
                    seg->q_first = pos_of(A, min(first, A.n - 1u));
                    seg->q_last = pos_of(A, min(last, A.n - 1u));
                    seg->offset = win_d;
                    seg->band_votes = win_S;
                    seg->rate_num = (int32_t)num_s;
                    seg->rate_den = den;
                    seg->rate_index = win_r;
                    rec->n_segments = s + 1u;
                }
                rec->q_covered = q_covered;
                rec->rounds = s + 1u;
            }
            count_bits(flags + wa, B.n, red, &cnt, &first, &last);
            if (tid == 0 && s < (uint32_t)HVD_ALIGN_MAX_SEGMENTS) {
                hvd_vssegment* seg = rec->seg + s;
                seg->t_aligned = cnt;
                seg->t_first = pos_of(B, min(first, B.n - 1u));
                seg->t_last = pos_of(B, min(last, B.n - 1u));
            }
            // taken_a |= the round's frames of a, seen_b |= its frames of b: one loop, the sibling's. seen_b is counted once,
            // below, and never read as a filter.
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[wa + wb + k] |= flags[k];
            if (q_covered >= A.n) break;  // nothing is left of a: no further pass
        }
        // t_covered = |seen_b|: the DISTINCT frames of b over all rounds, however many of them a frame served (no round: it
        // stays the zero the record was opened with)
        if (q_covered == 0u) continue;
        __syncthreads();
        uint32_t t_covered, first, last;
        count_bits(flags + 2u * wa + wb, B.n, red, &t_covered, &first, &last);
        if (tid == 0) rec->t_covered = t_covered;
    }
}

}  // namespace

namespace hvd {

hipError_t launch_valign_loops(const AlignMode& mode, const AlignOperands& op, hipStream_t s) {
    return launch_lds_then_scratch(op, [&](auto big, unsigned grid, uint32_t* scratch, uint32_t slot_words) {
        hipLaunchKernelGGL(k_valign_loops<decltype(big)::value>, dim3(grid), dim3(256), 0, s, (const uint4*)op.hashes_q,
                           (const long long*)op.offsets_q, (uint32_t)op.VQ, (const int32_t*)op.pos_q, (const uint4*)op.hashes_t,
                           (const long long*)op.offsets_t, (uint32_t)op.VT, (const int32_t*)op.pos_t, (const uint2*)op.pairs,
                           (uint32_t)op.M, (uint32_t)op.max_dist, (uint32_t)op.slack, mode.nums, mode.dens, mode.revs,
                           (uint32_t)mode.max_segments, (uint32_t)mode.min_band_votes, scratch, slot_words, (hvd_vloops*)op.out);
    });
}

}  // namespace hvd
