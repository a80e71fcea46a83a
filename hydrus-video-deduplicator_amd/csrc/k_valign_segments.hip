// k_valign_segments.hip -- multi-segment time alignment of listed video pairs: a short video that is several
// pieces of a longer one (a highlight reel, a trailer, a re-cut). k_valign.hip fits one line p_b = p_a + d* per pair; this
// kernel peels up to max_segments of them, greedily. The rule, integers only (include/hvd_mi355x.h has the full text), in
// the notation of k_valign.hip (H, delta, votes, S, slack, the tie order):
//   taken_a = taken_b = {};  for r = 1..K:
//     H_r = {(i, j) in H : i not in taken_a, j not in taken_b};  votes, S, d*_r: the rule of k_valign on H_r;
//     stop if H_r is empty or S(d*_r) < min_band_votes;
//     segment r = (d*_r, S(d*_r), the frames of a / of b with a hit of H_r within slack of d*_r: number, first, last);
//     taken |= those frames;  stop if every frame of a, or every frame of b, is taken.
// The shape is k_valign's: one 256-lane workgroup per pair (grid-stride), video a staged through LDS in chunks of kStage frames
// (rows padded to 9 words), one frame of video b per lane in registers, short b sides dealt over 256 / nb lanes, two passes over
// the recomputed Hamming matrix per round (8 xor + 8 popcount per comparison). Per pair there are two more runs of bit words
// beside the flag words -- the taken sets -- and the histogram is cleared every round. A taken frame of b skips its lane's
// row; the taken bit of a frame of a is read AFTER the distance test: hits are rare, and a comparison that misses pays nothing
// for the sets. The hit bits (q_hits / t_hits) are set in round 1 only. Segment 1 is, word for word, the k_valign record.
// The histogram lives in LDS up to HVD_ALIGN_LDS_BINS bins (k_valign_segments<false>); larger pairs are left to a second
// launch (k_valign_segments<true>) whose workgroups own one slot each of the caller's scratch -- histogram, flag words, taken
// words -- up to 2^20 bins. Every bin index, frame range and slot size is checked before it is used: a broken CSR, pair list
// or position array gives wrong or INT32_MIN records, never an access out of bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hvd_kernels.h"

namespace {

constexpr uint32_t kLdsBins = HVD_ALIGN_LDS_BINS;
constexpr uint32_t kMaxBins = 1u << 20;
constexpr uint32_t kStage = 256;                     // frames of video a per LDS chunk
constexpr uint32_t kFlagWords = kLdsBins / 32u + 4u;  // na + nb <= bins + 1 bits, in two word-aligned runs
constexpr uint32_t kRecWords = sizeof(hvd_vsegments) / 4u;
static_assert(sizeof(hvd_vsegments) == 288 && sizeof(hvd_vsegment) == 32 && sizeof(hvd_vsegments) % 16 == 0, "record layout");

// one video of a pair: its hashes and positions (nullptr: the index inside the video), both from its first frame on
struct Side {
    const uint4* hashes;  // 2 per frame
    const int32_t* pos;
    uint32_t n;
};

__device__ __forceinline__ int32_t pos_of(const Side& s, uint32_t f) { return s.pos ? s.pos[f] : (int32_t)f; }

// the operands of a launch, as the kernel keeps them in LDS
struct Operands {
    const uint4* hashes_q;
    const long long* offsets_q;
    const int32_t* pos_q;
    const uint4* hashes_t;
    const long long* offsets_t;
    const int32_t* pos_t;
    const uint2* pairs;
    hvd_vsegments* out;
    uint32_t VQ, VT, M, max_dist, slack, max_segments, min_band_votes, slot_words;
};

// a value every lane holds alike, as a scalar
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

struct Best {
    uint32_t S, v;
    int32_t d;
};

__device__ __forceinline__ uint32_t iabs(int32_t d) { return d < 0 ? 0u - (uint32_t)d : (uint32_t)d; }

// the tie order: larger S, larger votes[d], smaller |d|, smaller d
__device__ __forceinline__ bool better(const Best& x, const Best& y) {
    if (x.S != y.S) return x.S > y.S;
    if (x.v != y.v) return x.v > y.v;
    if (iabs(x.d) != iabs(y.d)) return iabs(x.d) < iabs(y.d);
    return x.d < y.d;
}

// number, lowest and highest set bit of a run of flag words, over the workgroup; red: 12 words of LDS
__device__ __forceinline__ void count_bits(const uint32_t* flags, uint32_t n_bits, uint32_t* red, uint32_t* cnt, uint32_t* first,
                                           uint32_t* last) {
    uint32_t c = 0, lo = 0xffffffffu, hi = 0;
    for (uint32_t k = threadIdx.x; k < (n_bits + 31u) / 32u; k += 256u) {
        const uint32_t w = flags[k];
        if (w) {
            c += __popc(w);
            lo = min(lo, k * 32u + (uint32_t)__ffs((int)w) - 1u);
            hi = max(hi, k * 32u + 31u - (uint32_t)__clz((int)w));
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        c += __shfl_down(c, off);
        lo = min(lo, (uint32_t)__shfl_down(lo, off));
        hi = max(hi, (uint32_t)__shfl_down(hi, off));
    }
    __syncthreads();  // red may still be read from the call before
    if ((threadIdx.x & 63u) == 0u) {
        red[(threadIdx.x >> 6) * 3u] = c;
        red[(threadIdx.x >> 6) * 3u + 1u] = lo;
        red[(threadIdx.x >> 6) * 3u + 2u] = hi;
    }
    __syncthreads();
    *cnt = red[0] + red[3] + red[6] + red[9];
    *first = min(min(red[1], red[4]), min(red[7], red[10]));
    *last = max(max(red[2], red[5]), max(red[8], red[11]));
}

// One pass over the part of the Hamming matrix that is not taken. PASS 1: votes, and with hit_bits (round 1) one bit per frame
// with a hit. PASS 2: the bits of the frames with a hit within slack of dstar. Video a is staged, chunk by chunk; a lane keeps
// one frame of video b. flagA / flagB / takenA / takenB: where the runs of bit words start behind hist.
template <int PASS>
__device__ __forceinline__ void scan_pair(const Side& A, const Side& B, uint32_t max_dist, uint32_t* stage, int32_t* spos,
                                          uint32_t* hist, uint32_t flagA, uint32_t flagB, uint32_t takenA, uint32_t takenB,
                                          int32_t dmin, uint32_t core, uint32_t slack, int32_t dstar, bool hit_bits) {
    const uint32_t tid = threadIdx.x;
    const uint32_t nsplit = B.n >= 256u ? 1u : 256u / B.n;
    const uint32_t j_small = tid % B.n, part_small = tid / B.n;
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < A.n; i0 += kStage) {
        const uint32_t ci = min(kStage, A.n - i0);
        __syncthreads();  // the chunk before is done with
        for (uint32_t k = tid; k < ci * 2u; k += 256u) {
            const uint4 v = A.hashes[(size_t)i0 * 2u + k];
            uint32_t* d = stage + (k >> 1) * 9u + (k & 1u) * 4u;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        for (uint32_t k = tid; k < ci; k += 256u) spos[k] = pos_of(A, i0 + k);
        __syncthreads();
#pragma unroll 1
        for (uint32_t base = 0; base < B.n; base += 256u) {
            const uint32_t j = nsplit == 1u ? base + tid : j_small;
            const uint32_t part = nsplit == 1u ? 0u : part_small;
            if (j >= B.n || part >= nsplit) continue;
            if ((hist[takenB + (j >> 5)] >> (j & 31u)) & 1u) continue;  // a segment before owns this frame of b
            const uint4 q0 = B.hashes[(size_t)j * 2u], q1 = B.hashes[(size_t)j * 2u + 1u];
            const int32_t pb = pos_of(B, j);
            bool any = false;
#pragma unroll 1
            for (uint32_t i = part; i < ci; i += nsplit) {
                const uint32_t* c = stage + i * 9u;
                uint32_t d = __popc(q0.x ^ c[0]) + __popc(q0.y ^ c[1]) + __popc(q0.z ^ c[2]) + __popc(q0.w ^ c[3]);
                d += __popc(q1.x ^ c[4]) + __popc(q1.y ^ c[5]) + __popc(q1.z ^ c[6]) + __popc(q1.w ^ c[7]);
                if (d > max_dist) continue;
                const uint32_t f = i0 + i;
                if ((hist[takenA + (f >> 5)] >> (f & 31u)) & 1u) continue;  // a segment before owns this frame of a
                const int32_t delta = pb - spos[i];
                if (PASS == 1) {
                    const uint32_t bin = (uint32_t)(delta - dmin);
                    if (bin < core) atomicAdd(&hist[bin + slack], 1u);  // (only broken positions fail the check)
                    if (!hit_bits) continue;
                } else if (iabs(delta - dstar) > slack) {
                    continue;
                }
                any = true;
                atomicOr(&hist[flagA + (f >> 5)], 1u << (f & 31u));
            }
            if (any) atomicOr(&hist[flagB + (j >> 5)], 1u << (j & 31u));
        }
    }
    __syncthreads();
}

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
        K = {hashes_q, offsets_q, pos_q, hashes_t, offsets_t, pos_t, pairs, out, VQ, VT, M, max_dist, slack,
             min(max_segments, (uint32_t)HVD_ALIGN_MAX_SEGMENTS), max(min_band_votes, 1u), slot_words};
    __syncthreads();
#pragma unroll 1
    for (uint32_t p = blockIdx.x; p < K.M; p += gridDim.x) {
        const uint2 ab = K.pairs[p];
        const uint32_t slack = uni(K.slack);
        // ---- geometry of the pair (the same on every lane) ----
        bool bad = ab.x >= K.VQ || ab.y >= K.VT, empty = false;
        Side A = {nullptr, nullptr, 0}, B = {nullptr, nullptr, 0};
        long long bins = 0;
        int32_t dmin = 0;
        if (!bad) {
            const long long* const oq = K.offsets_q;
            const long long* const ot = K.offsets_t;
            const long long nq_all = oq[K.VQ], nt_all = ot[K.VT];
            const long long a0 = min(max(oq[ab.x], 0ll), nq_all), a1 = min(max(oq[ab.x + 1u], a0), nq_all);
            const long long b0 = min(max(ot[ab.y], 0ll), nt_all), b1 = min(max(ot[ab.y + 1u], b0), nt_all);
            empty = a1 == a0 || b1 == b0;
            bad = a1 - a0 > (long long)kMaxBins || b1 - b0 > (long long)kMaxBins;
            if (!bad && !empty) {
                A = {K.hashes_q + a0 * 2, K.pos_q ? K.pos_q + a0 : nullptr, (uint32_t)(a1 - a0)};
                B = {K.hashes_t + b0 * 2, K.pos_t ? K.pos_t + b0 : nullptr, (uint32_t)(b1 - b0)};
                const long long pa0 = pos_of(A, 0), pa1 = pos_of(A, A.n - 1u), pb0 = pos_of(B, 0), pb1 = pos_of(B, B.n - 1u);
                // strictly increasing positions make a video's span at least its length - 1; the bit words rely on it
                bad = pa0 < 0 || pb0 < 0 || pa1 - pa0 + 1 < (long long)A.n || pb1 - pb0 + 1 < (long long)B.n;
                bins = (pa1 - pa0) + (pb1 - pb0) + 1 + 2 * (long long)slack;
                bad = bad || bins > (long long)kMaxBins;
                dmin = (int32_t)(pb0 - pa1);
            }
        }
        const bool big = !bad && !empty && bins > (long long)kLdsBins;
        if (big != BIG) continue;  // the other launch's pair (bad and empty pairs belong to the LDS launch)
        const uint32_t nbins = (uint32_t)bins, wa = (A.n + 31u) / 32u, wb = (B.n + 31u) / 32u;
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
        if (bad || empty) continue;
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
            scan_pair<1>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, dmin, core, slack, 0, r == 0u);
            uint32_t cnt, first, last;
            if (r == 0u) {
                count_bits(flags + wa, B.n, red, &cnt, &first, &last);
                if (tid == 0) rec->t_hits = cnt;
                count_bits(flags, A.n, red, &cnt, &first, &last);
                if (tid == 0) rec->q_hits = cnt;
                if (cnt == 0u) break;  // H is empty
            }
            // ---- best offset: windowed sums, arg-max under the tie order ----
            Best best = {0u, 0u, 0};
#pragma unroll 1
            for (uint32_t k = tid; k < nbins; k += 256u) {
                const uint32_t u0 = k >= slack ? k - slack : 0u, u1 = min(nbins - 1u, k + slack);
                Best c = {0u, hist[k], dmin - (int32_t)slack + (int32_t)k};
#pragma unroll 1
                for (uint32_t u = u0; u <= u1; ++u) c.S += hist[u];
                if (better(c, best)) best = c;
            }
            for (int off = 32; off > 0; off >>= 1) {
                Best o = {(uint32_t)__shfl_down(best.S, off), (uint32_t)__shfl_down(best.v, off), __shfl_down(best.d, off)};
                if (better(o, best)) best = o;
            }
            __syncthreads();  // wbest may still be read from the round before
            if ((tid & 63u) == 0u) wbest[tid >> 6] = best;
            __syncthreads();
            best = wbest[0];
            for (int w = 1; w < 4; ++w)
                if (better(wbest[w], best)) best = wbest[w];
            if (best.S < min_band_votes) break;  // H_r is empty (S = 0), or its best band is below the caller's floor
            // ---- pass 2: the frames of the segment ----
            for (uint32_t k = tid; k < wa + wb; k += 256u) flags[k] = 0u;
            scan_pair<2>(A, B, max_dist, stage, spos, hist, flagA, flagB, takenA, takenB, dmin, core, slack, best.d, true);
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

// workgroups of the scratch launch: one slot each
constexpr unsigned kSegmentSlots = 64;

size_t segments_scratch_bytes(unsigned long long max_bins) {
    if (max_bins <= kLdsBins) return 0;
    if (max_bins > kMaxBins) max_bins = kMaxBins;
    // histogram + two runs of flag words + two runs of taken words (na + nb <= bins + 1 bits each)
    return (size_t)kSegmentSlots * 4u * (size_t)(max_bins + 2u * ((max_bins + 1u) / 32u + 3u));
}

hipError_t launch_valign_segments(const void* d_hashes_q, const long long* d_offsets_q, uint32_t VQ, const int32_t* d_pos_q,
                                  const void* d_hashes_t, const long long* d_offsets_t, uint32_t VT, const int32_t* d_pos_t,
                                  const uint32_t* d_pairs, unsigned long long M, uint32_t max_dist, uint32_t slack,
                                  uint32_t max_segments, uint32_t min_band_votes, void* d_scratch, size_t scratch_bytes,
                                  hvd_vsegments* d_out, hipStream_t s) {
    if (M == 0) return hipSuccess;
    const unsigned grid = (unsigned)(M < 8192ull ? M : 8192ull);
    hipLaunchKernelGGL(k_valign_segments<false>, dim3(grid), dim3(256), 0, s, (const uint4*)d_hashes_q, d_offsets_q, VQ, d_pos_q,
                       (const uint4*)d_hashes_t, d_offsets_t, VT, d_pos_t, (const uint2*)d_pairs, (uint32_t)M, max_dist, slack,
                       max_segments, min_band_votes, (uint32_t*)nullptr, 0u, d_out);
    // the pairs beyond the LDS histogram: found again from the same geometry, by as many workgroups as there are slots
    unsigned long long slot_words = d_scratch ? scratch_bytes / 4u / kSegmentSlots : 0ull;
    if (slot_words > 2u * kMaxBins) slot_words = 2u * kMaxBins;  // (more than any pair needs)
    const unsigned big_grid = (unsigned)(M < kSegmentSlots ? M : kSegmentSlots);
    hipLaunchKernelGGL(k_valign_segments<true>, dim3(big_grid), dim3(256), 0, s, (const uint4*)d_hashes_q, d_offsets_q, VQ, d_pos_q,
                       (const uint4*)d_hashes_t, d_offsets_t, VT, d_pos_t, (const uint2*)d_pairs, (uint32_t)M, max_dist, slack,
                       max_segments, min_band_votes, (uint32_t*)d_scratch, (uint32_t)slot_words, d_out);
    return hipGetLastError();
}

}  // namespace hvd
