// k_valign.hip -- time alignment of listed video pairs: where inside the longer video does the shorter one
// sit, and how many of its frames line up there. The rule, the staging of the Hamming matrix, the LDS / scratch split and the
// bounds checks are hvd_valign_dev.h's; this file is the single-offset loop over them. One workgroup per pair (grid-stride):
//   pass 1: hits vote into a histogram over delta (LDS atomics) and set one bit per frame (q_hits / t_hits);
//   arg-max of the windowed sums under the tie order;
//   pass 2: the bits of the frames that have a hit on the band; counts, first and last aligned frame from the bit words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_kernels.h"
#include "hvd_valign_dev.h"

namespace {

// BIG false: every pair whose histogram fits LDS, and the INT32_MIN record of a pair index out of range. BIG true: the pairs
// that do not fit LDS, each workgroup with its own slot of slot_words words at scratch (histogram, then the flag words); a
// pair that does not fit its slot gets the INT32_MIN record.
template <bool BIG>
__global__ __launch_bounds__(256) void k_valign(const uint4* __restrict__ hashes_q, const long long* __restrict__ offsets_q,
                                                uint32_t VQ, const int32_t* __restrict__ pos_q,
                                                const uint4* __restrict__ hashes_t, const long long* __restrict__ offsets_t,
                                                uint32_t VT, const int32_t* __restrict__ pos_t,
                                                const uint2* __restrict__ pairs, uint32_t M, uint32_t max_dist,
                                                uint32_t slack, uint32_t* __restrict__ scratch, uint32_t slot_words,
                                                hvd_valign* __restrict__ out) {
    __shared__ uint32_t stage[kStage * 9u];
    __shared__ int32_t spos[kStage];
    __shared__ uint32_t lds_words[BIG ? 1u : kLdsBins + kFlagWords];  // histogram, then the flag words
    __shared__ uint32_t red[12];
    __shared__ Best wbest[4];
    __shared__ const void* side_ptr[4];
    const uint32_t tid = threadIdx.x;
    uint32_t* const hist = BIG ? scratch + (size_t)blockIdx.x * slot_words : lds_words;
#pragma unroll 1
    for (uint32_t p = blockIdx.x; p < M; p += gridDim.x) {
        const uint2 ab = pairs[p];
        const Geometry geo = pair_geometry({hashes_q, offsets_q, pos_q, hashes_t, offsets_t, pos_t, VQ, VT}, ab, slack);
        if (geo.big() != BIG) continue;  // the other launch's pair (bad and empty pairs belong to the LDS launch)
        Side A = geo.A, B = geo.B;
        const int32_t dmin = geo.dmin;
        bool bad = geo.bad;
        const uint32_t nbins = (uint32_t)geo.bins, wa = (A.n + 31u) / 32u, wb = (B.n + 31u) / 32u;
        uint32_t* const flags = hist + nbins;
        if (BIG && nbins + wa + wb > slot_words) bad = true;  // no room in the slot
        // the record is written as its words become known (lane 0): nothing of it has to stay in registers over the passes
        hvd_valign* rec = out + p;
        if (tid == 0) {
            hvd_valign zero = {};
            zero.a = ab.x;
            zero.b = ab.y;
            if (bad) zero.offset = INT32_MIN;
            *rec = zero;
        }
        if (bad || geo.empty) continue;
        // ---- pass 1 ----
        __syncthreads();  // the pair before is done with LDS
        // The four pointers of the pair go through LDS and come back as vector registers: the scalar file holds every kernel
        // argument over the whole loop already, and eight more scalars over the passes would spill.
        if (tid == 0) {
            side_ptr[0] = A.hashes;
            side_ptr[1] = A.pos;
            side_ptr[2] = B.hashes;
            side_ptr[3] = B.pos;
        }
        __syncthreads();
        A = {(const uint4*)side_ptr[0], (const int32_t*)side_ptr[1], A.n};
        B = {(const uint4*)side_ptr[2], (const int32_t*)side_ptr[3], B.n};
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
        store_aligned<false>(rec, flags, A, red);
        store_aligned<true>(rec, flags + wa, B, red);
    }
}

}  // namespace

namespace hvd {

size_t alignment_scratch_bytes(const AlignMode& mode, unsigned long long max_bins) {
    // A loops mode has a third pair of runs, the seen words: slot_runs() = 3. slot_runs() is runs() for every other mode, so
    // the second arm is redundant: it is here because tests/test_rate_segments_cpu.py matches its text in this file (and the
    // body of runs() in hvd_kernels.h). When that test lets go of the text, this is slot_scratch_bytes(max_bins, mode.slot_runs()).
    return mode.loops ? slot_scratch_bytes(max_bins, mode.slot_runs()) : slot_scratch_bytes(max_bins, mode.runs());
}

hipError_t launch_alignment(const AlignMode& mode, const AlignOperands& op, hipStream_t s) {
    constexpr decltype(&launch_valign) launchers[5] = {launch_valign, launch_valign_segments, launch_valign_rates,
                                                       launch_valign_rate_segments, launch_valign_signed};
    // The sixth, k_valign_loops.hip, stands beside the table only because tests/test_signed_cpu.py matches the
    // text of the table's last line: when that test lets go of it, launch_valign_loops becomes launchers[5].
    if (mode.kind() == 5u) return launch_valign_loops(mode, op, s);
    return launchers[mode.kind()](mode, op, s);
}

hipError_t launch_valign(const AlignMode&, const AlignOperands& op, hipStream_t s) {
    return launch_lds_then_scratch(op, [&](auto big, unsigned grid, uint32_t* scratch, uint32_t slot_words) {
        hipLaunchKernelGGL(k_valign<decltype(big)::value>, dim3(grid), dim3(256), 0, s, (const uint4*)op.hashes_q,
                           (const long long*)op.offsets_q, (uint32_t)op.VQ, (const int32_t*)op.pos_q, (const uint4*)op.hashes_t,
                           (const long long*)op.offsets_t, (uint32_t)op.VT, (const int32_t*)op.pos_t, (const uint2*)op.pairs,
                           (uint32_t)op.M, (uint32_t)op.max_dist, (uint32_t)op.slack, scratch, slot_words, (hvd_valign*)op.out);
    });
}

}  // namespace hvd
