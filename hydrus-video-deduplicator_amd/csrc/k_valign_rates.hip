// k_valign_rates.hip -- rate-aware time alignment of listed video pairs: a copy or an excerpt that was sped up
// or slowed down. k_valign.hip fits one line of slope one, p_b = p_a + d*; this kernel fits p_b = (num / den) p_a + c for each
// of up to eight listed rates and keeps the rate whose best band holds the most frame hits. The rule, integers only
// (include/hvd_mi355x.h has the full text), in the notation of hvd_valign_dev.h (H, votes, S, the tie order):
//   for each rate r = (num, den), in list order:
//     delta_r = den p_b - num p_a;  slack_r = slack max(num, den);  votes_r, S_r, d*_r: the rule of k_valign on delta_r, slack_r;
//   w = the rate of the largest S_r(d*_r), ties to the earlier one;  aligned frames: a hit within slack_w of d*_w at rate w.
// The shape, the passes and the bounds checks are hvd_valign_dev.h's; this file is the loop of rates over them: R rounds of
// (clear the histogram, pass 1 on the scaled delta, arg-max) and one pass 2 at the winner -- R + 1 passes over the Hamming
// matrix. The hit bits (q_hits / t_hits) are set in round 1 only, and a pair without a hit stops there. The histogram of a pair
// is sized by its largest bins_r: that decides which launch owns the pair and whether it fits its slot, and the flag words
// lie behind it, in one place for all rounds. With the list [(1, 1)] the record's first twelve words are k_valign's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_valign_dev.h"

namespace {

static_assert(sizeof(hvd_vrate) == 64 && offsetof(hvd_vrate, rate_num) == sizeof(hvd_valign), "record layout");

// the operands of a launch, as the kernel keeps them in LDS; n_rates 0: a broken list
struct Operands {
    Libraries lib;
    const uint2* pairs;
    hvd_vrate* out;
    uint32_t M, max_dist, slack, nums, dens, n_rates, slot_words;
};

// BIG false: every pair whose largest histogram fits LDS, and the INT32_MIN record of a pair index out of range or of a broken
// list. BIG true: the pairs that do not fit LDS, each workgroup with its own slot of slot_words words at scratch (histogram,
// then the flag words); a pair that does not fit its slot gets the INT32_MIN record.
template <bool BIG>
__global__ __launch_bounds__(256) void k_valign_rates(const uint4* __restrict__ hashes_q, const long long* __restrict__ offsets_q,
                                                      uint32_t VQ, const int32_t* __restrict__ pos_q,
                                                      const uint4* __restrict__ hashes_t, const long long* __restrict__ offsets_t,
                                                      uint32_t VT, const int32_t* __restrict__ pos_t,
                                                      const uint2* __restrict__ pairs, uint32_t M, uint32_t max_dist,
                                                      uint32_t slack, uint32_t nums, uint32_t dens,
                                                      uint32_t* __restrict__ scratch, uint32_t slot_words,
                                                      hvd_vrate* __restrict__ out) {
    __shared__ uint32_t stage[kStage * 9u];
    __shared__ int32_t spos[kStage];
    __shared__ uint32_t lds_words[BIG ? 1u : kLdsBins + kFlagWords];  // histogram (of the largest bins_r), then the flag words
    __shared__ uint32_t red[12];
    __shared__ Best wbest[4];
    __shared__ Operands K;
    __shared__ Spans P;  // of the pair at hand
    const uint32_t tid = threadIdx.x;
    uint32_t* const hist = BIG ? scratch + (size_t)blockIdx.x * slot_words : lds_words;
    // The operands go through LDS once and are read back where they are used, as vector registers with short lives (the
    // arrangement of k_valign_segments): held in the scalar file over the pair loop, beside the state of the rounds, they spill.
    if (tid == 0)
        K = {{hashes_q, offsets_q, pos_q, hashes_t, offsets_t, pos_t, VQ, VT}, pairs, out, M, max_dist, slack, nums, dens,
             hvd::rate_list_length(nums, dens), slot_words};
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
        if (BIG && (unsigned long long)nbins_max + wa + wb > K.slot_words) bad = true;  // no room in the slot
        // the record: zeroed here, then written word by word as its words become known (lane 0)
        hvd_vrate* rec = K.out + p;
        if (tid == 0) {
            uint4* w = (uint4*)rec;
            w[0] = make_uint4(ab.x, ab.y, 0u, 0u);
            w[1] = make_uint4(bad ? 0x80000000u : 0u, 0u, 0u, 0u);
            w[2] = make_uint4(0u, 0u, 0u, 0u);
            w[3] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (bad || geo.empty) continue;
        if (tid == 0) P = spans;  // (the rounds of the pair before read theirs ahead of a barrier of scan_pair's)
        __syncthreads();          // the pair before is done with LDS
        // the pair's lengths and the tolerance are what the inner loops turn on: back into the scalar file
        A.n = uni(A.n);
        B.n = uni(B.n);
        const uint32_t max_dist = uni(K.max_dist);
        uint32_t* const flags = hist + nbins_max;
        const uint32_t flagA = nbins_max, flagB = flagA + wa;
        for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;  // (scan_pair opens with a barrier)
        // ---- R rounds of pass 1: the winner stays in four registers ----
        uint32_t win_S = 0, win_r = 0, hits = 0;
        int32_t win_d = 0;
#pragma unroll 1
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t num = uni((K.nums >> (4u * r)) & 15u), den = uni((K.dens >> (4u * r)) & 15u);
            const uint32_t slack_r = slack * max(num, den);
            const uint32_t core = uni(num * P.a + den * P.b + 1u), nbins = core + 2u * slack_r;  // (nbins <= nbins_max)
            const int32_t dmin = (int32_t)uni(den * (uint32_t)P.pb0 - num * (uint32_t)P.pa1);
            for (uint32_t k = tid; k < nbins; k += 256u) hist[k] = 0u;
            scan_pair<1, false, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, 0u, 0u, dmin, core, slack_r, 0, r == 0u, num,
                                      den);
            if (r == 0u) {
                hits = store_hit_counts(rec, flags, wa, A, B, red);
                if (hits == 0u) break;  // H is empty
            }
            const Best best = best_offset<true>(hist, nbins, slack_r, dmin, wbest);
            if (r == 0u || best.S > win_S) {  // ties go to the earlier rate
                win_S = best.S;
                win_d = best.d;
                win_r = r;
            }
        }
        if (hits == 0u) continue;
        // ---- pass 2 at the winning rate ----
        const uint32_t num = uni((K.nums >> (4u * win_r)) & 15u), den = uni((K.dens >> (4u * win_r)) & 15u);
        if (tid == 0) {
            rec->offset = win_d;
            rec->band_votes = win_S;
            rec->rate_num = num;
            rec->rate_den = den;
            rec->rate_index = win_r;
        }
        for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
        scan_pair<2, false, true>(A, B, max_dist, stage, spos, hist, flagA, flagB, 0u, 0u, 0, 0u, slack * max(num, den), win_d, true,
                                  num, den);
        store_aligned<false>(rec, flags, A, red);
        store_aligned<true>(rec, flags + wa, B, red);
    }
}

}  // namespace

namespace hvd {

hipError_t launch_valign_rates(const AlignMode& mode, const AlignOperands& op, hipStream_t s) {
    return launch_lds_then_scratch(op, [&](auto big, unsigned grid, uint32_t* scratch, uint32_t slot_words) {
        hipLaunchKernelGGL(k_valign_rates<decltype(big)::value>, dim3(grid), dim3(256), 0, s, (const uint4*)op.hashes_q,
                           (const long long*)op.offsets_q, (uint32_t)op.VQ, (const int32_t*)op.pos_q, (const uint4*)op.hashes_t,
                           (const long long*)op.offsets_t, (uint32_t)op.VT, (const int32_t*)op.pos_t, (const uint2*)op.pairs,
                           (uint32_t)op.M, (uint32_t)op.max_dist, (uint32_t)op.slack, mode.nums, mode.dens, scratch, slot_words,
                           (hvd_vrate*)op.out);
    });
}

}  // namespace hvd
