// hvd_valign_dev.h -- what the time-alignment kernels share, one definition of each piece: k_valign.hip (one offset per pair,
// DESIGN.md 4.8), k_valign_segments.hip (up to eight), k_valign_rates.hip (one offset at the best of up to eight
// listed rates) and k_valign_rate_segments.hip (rate x segments) include it and add their kernel
// and its loops; what they write into a record alike -- the hit counts of round one, a side's aligned count, first and last -- is
// here too (k_valign_segments writes them out: with the helpers it was rescheduled and measurably moved). Device code first; the last section is host code: the slot count, the scratch sizing, the helper that enqueues the
// two launches, and the four files' launchers, which hvd::launch_alignment (k_valign.hip) chooses among by the mode.
//
// The rule, integers only (include/hvd_mi355x.h has the full text):
//   H = {(i, j) : hamming(A_i, B_j) <= max_dist},  delta(i, j) = p_b(j) - p_a(i),  votes[d] = |{(i, j) in H : delta = d}|,
//   S(d) = votes[d - slack] + ... + votes[d + slack];  d* = the d of the largest S, ties by larger votes[d], smaller |d|,
//   smaller d;  a frame is aligned iff one of its hits lies within slack of d*.
// The shape: one 256-lane workgroup per pair. The na x nb Hamming matrix is recomputed pass by pass, never stored: 8 xor + 8
// popcount per comparison on the packed hashes, the integer form of k_hamming.hip. Video a is staged through LDS in chunks of
// kStage = 256 frames (rows padded to 9 words: lanes that read different rows hit different banks), so a video of any length
// is served out of LDS; every lane keeps one frame of video b in registers, and with fewer than 256 frames in b the staged
// frames are dealt out over 256 / nb lanes per frame, so that a 64 x 64 pair keeps all 256 lanes busy. Behind the histogram
// over delta lie runs of bit words, one bit per frame (na + nb <= bins + 1 bits a pair of runs): the flag words, and in
// k_valign_segments the taken words. Histogram and bit words live in LDS up to HVD_ALIGN_LDS_BINS bins (the <false> kernels);
// pairs with more bins are left to a second launch (the <true> kernels) whose workgroups own one slot each of the caller's
// scratch -- up to 2^20 bins.
// RATE (k_valign_rates; defaulted template parameters and trailing arguments, so the other two kernels compile to the code they
// had): the lines are p_b = (num / den) p_a + c, delta = den p_b - num p_a, and slack is the caller's slack_r = slack max(num, den).
// The promise: every bin index, frame range and slot size is checked against its bound before it is used. A broken CSR, pair
// list or position array gives wrong or INT32_MIN records, never an access out of bounds.
// Every device function is __forceinline__: a kernel that calls them compiles to the code it had with the statements written out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hvd_kernels.h"

namespace {

constexpr uint32_t kLdsBins = HVD_ALIGN_LDS_BINS;
constexpr uint32_t kMaxBins = 1u << 20;
constexpr uint32_t kStage = 256;                     // frames of video a per LDS chunk
constexpr uint32_t kFlagWords = kLdsBins / 32u + 4u;  // na + nb <= bins + 1 bits, in two word-aligned runs

// one video of a pair: its hashes and positions (nullptr: the index inside the video), both from its first frame on
struct Side {
    const uint4* hashes;  // 2 per frame
    const int32_t* pos;
    uint32_t n;
};

__device__ __forceinline__ int32_t pos_of(const Side& s, uint32_t f) { return s.pos ? s.pos[f] : (int32_t)f; }

// a value every lane holds alike, as a scalar
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

__device__ __forceinline__ uint32_t iabs(int32_t d) { return d < 0 ? 0u - (uint32_t)d : (uint32_t)d; }

// ---- geometry of a pair -------------------------------------------------------------------------------------------------
// the two libraries of a launch: hashes, CSR offsets (V + 1 of them), positions or nullptr
struct Libraries {
    const uint4* hashes_q;
    const long long* offsets_q;
    const int32_t* pos_q;
    const uint4* hashes_t;
    const long long* offsets_t;
    const int32_t* pos_t;
    uint32_t VQ, VT;
};

struct Geometry {
    Side A, B;
    long long bins;  // span of p_a + span of p_b + 1 + 2 slack
    int32_t dmin;    // the delta of bin `slack`
    bool bad;        // the INT32_MIN record
    bool empty;      // a video without frames: the zero record
    __device__ __forceinline__ bool big() const { return !bad && !empty && bins > (long long)kLdsBins; }  // the scratch launch's
};

// what every rate's geometry is made of: bins_r = num span_a + den span_b + 1 + 2 slack_r, dmin_r = den p_b0 - num p_a1
struct Spans {
    uint32_t a, b;  // p_a1 - p_a0, p_b1 - p_b0
    int32_t pa1, pb0;
};

// The same on every lane. Frame ranges are clamped to [0, offsets[V]]; A and B stay empty unless the pair is neither bad nor empty.
// RATE: entry r of the list is (nums >> 4r & 15, dens >> 4r & 15), n_rates of them (0: a broken list, every pair is bad);
// bins is then the largest bins_r of the list, dmin is not set, and *spans is (for a pair neither bad nor empty).
template <bool RATE = false>
__device__ __forceinline__ Geometry pair_geometry(const Libraries& L, uint2 ab, uint32_t slack, uint32_t nums = 0u,
                                                  uint32_t dens = 0u, uint32_t n_rates = 0u, Spans* spans = nullptr) {
    Geometry g = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}, 0, 0, ab.x >= L.VQ || ab.y >= L.VT, false};
    if (RATE && n_rates == 0u) g.bad = true;
    if (g.bad) return g;
    const long long* const oq = L.offsets_q;
    const long long* const ot = L.offsets_t;
    const long long nq_all = oq[L.VQ], nt_all = ot[L.VT];
    const long long a0 = min(max(oq[ab.x], 0ll), nq_all), a1 = min(max(oq[ab.x + 1u], a0), nq_all);
    const long long b0 = min(max(ot[ab.y], 0ll), nt_all), b1 = min(max(ot[ab.y + 1u], b0), nt_all);
    g.empty = a1 == a0 || b1 == b0;
    g.bad = a1 - a0 > (long long)kMaxBins || b1 - b0 > (long long)kMaxBins;
    if (g.bad || g.empty) return g;
    g.A = {L.hashes_q + a0 * 2, L.pos_q ? L.pos_q + a0 : nullptr, (uint32_t)(a1 - a0)};
    g.B = {L.hashes_t + b0 * 2, L.pos_t ? L.pos_t + b0 : nullptr, (uint32_t)(b1 - b0)};
    const long long pa0 = pos_of(g.A, 0), pa1 = pos_of(g.A, g.A.n - 1u), pb0 = pos_of(g.B, 0), pb1 = pos_of(g.B, g.B.n - 1u);
    // strictly increasing positions make a video's span at least its length - 1; the bit words rely on it
    g.bad = pa0 < 0 || pb0 < 0 || pa1 - pa0 + 1 < (long long)g.A.n || pb1 - pb0 + 1 < (long long)g.B.n;
    if constexpr (RATE) {
        if (g.bad) return g;  // (the spans below may be anything)
#pragma unroll 1
        for (uint32_t r = 0; r < n_rates; ++r) {
            const long long num = (nums >> (4u * r)) & 15u, den = (dens >> (4u * r)) & 15u;
            g.bins = max(g.bins, num * (pa1 - pa0) + den * (pb1 - pb0) + 1 + 2 * (long long)slack * max(num, den));
        }
        g.bad = g.bins > (long long)kMaxBins;
        *spans = {(uint32_t)(pa1 - pa0), (uint32_t)(pb1 - pb0), (int32_t)pa1, (int32_t)pb0};
        return g;
    }
    g.bins = (pa1 - pa0) + (pb1 - pb0) + 1 + 2 * (long long)slack;
    g.bad = g.bad || g.bins > (long long)kMaxBins;
    g.dmin = (int32_t)(pb0 - pa1);
    return g;
}

// ---- bit words ----------------------------------------------------------------------------------------------------------
// number, lowest and highest set bit of a run of bit words, over the workgroup; red: 12 words of LDS
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

// ---- what the kernels write into a record alike (lane 0 writes) -------------------------------------------------------------
// after pass 1 of round one: the frames of b and of a with a hit at all -> rec->t_hits, rec->q_hits; returns q_hits (0: H is empty)
template <class Rec>
__device__ __forceinline__ uint32_t store_hit_counts(Rec* rec, const uint32_t* flags, uint32_t wa, const Side& A, const Side& B,
                                                     uint32_t* red) {
    uint32_t cnt, first, last;
    count_bits(flags + wa, B.n, red, &cnt, &first, &last);
    if (threadIdx.x == 0) rec->t_hits = cnt;
    count_bits(flags, A.n, red, &cnt, &first, &last);
    if (threadIdx.x == 0) rec->q_hits = cnt;
    return cnt;
}

// after pass 2: the aligned frames of one side X (T_SIDE: video b, flags: its run of flag words) into a record or a segment
// of one: their number, the first and the last position. -> the number
template <bool T_SIDE, class Seg>
__device__ __forceinline__ uint32_t store_aligned(Seg* seg, const uint32_t* flags, const Side& X, uint32_t* red) {
    uint32_t cnt, first, last;
    count_bits(flags, X.n, red, &cnt, &first, &last);
    if (threadIdx.x == 0) {
        (T_SIDE ? seg->t_aligned : seg->q_aligned) = cnt;
        (T_SIDE ? seg->t_first : seg->q_first) = pos_of(X, min(first, X.n - 1u));
        (T_SIDE ? seg->t_last : seg->q_last) = pos_of(X, min(last, X.n - 1u));
    }
    return cnt;
}

// ---- one pass over the Hamming matrix -----------------------------------------------------------------------------------
// PASS 1: votes, and with hit_bits one bit per frame with a hit. PASS 2: the bits of the frames with a hit within slack of dstar.
// Video a is staged, chunk by chunk; a lane keeps one frame of video b. flagA / flagB / takenA / takenB: where the runs of bit
// words start behind hist. TAKEN (k_valign_segments): the pass skips the frames in the taken sets -- a taken frame of b skips its
// lane's row; the taken bit of a frame of a is read AFTER the distance test: hits are rare, and a comparison that misses pays
// nothing for the sets. Without TAKEN there are no taken words, and hit_bits is true unless RATE. RATE: delta = den p_b - num p_a
// (the staged positions are num p_a, a lane's is den p_b; 32-bit wrap-around, which the bin check is indifferent to), and dmin,
// core, slack and dstar are the rate's, in its scaled units.
template <int PASS, bool TAKEN, bool RATE = false>
__device__ __forceinline__ void scan_pair(const Side& A, const Side& B, uint32_t max_dist, uint32_t* stage, int32_t* spos,
                                          uint32_t* hist, uint32_t flagA, uint32_t flagB, uint32_t takenA, uint32_t takenB,
                                          int32_t dmin, uint32_t core, uint32_t slack, int32_t dstar, bool hit_bits,
                                          uint32_t num = 1u, uint32_t den = 1u) {
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
        for (uint32_t k = tid; k < ci; k += 256u) spos[k] = RATE ? (int32_t)(num * (uint32_t)pos_of(A, i0 + k)) : pos_of(A, i0 + k);
        __syncthreads();
#pragma unroll 1
        for (uint32_t base = 0; base < B.n; base += 256u) {
            const uint32_t j = nsplit == 1u ? base + tid : j_small;
            const uint32_t part = nsplit == 1u ? 0u : part_small;
            if (j >= B.n || part >= nsplit) continue;
            if (TAKEN && ((hist[takenB + (j >> 5)] >> (j & 31u)) & 1u)) continue;  // a segment before owns this frame of b
            const uint4 q0 = B.hashes[(size_t)j * 2u], q1 = B.hashes[(size_t)j * 2u + 1u];
            const int32_t pb = RATE ? (int32_t)(den * (uint32_t)pos_of(B, j)) : pos_of(B, j);
            bool any = false;
#pragma unroll 1
            for (uint32_t i = part; i < ci; i += nsplit) {
                const uint32_t* c = stage + i * 9u;
                uint32_t d = __popc(q0.x ^ c[0]) + __popc(q0.y ^ c[1]) + __popc(q0.z ^ c[2]) + __popc(q0.w ^ c[3]);
                d += __popc(q1.x ^ c[4]) + __popc(q1.y ^ c[5]) + __popc(q1.z ^ c[6]) + __popc(q1.w ^ c[7]);
                if (d > max_dist) continue;
                const uint32_t f = i0 + i;
                if (TAKEN && ((hist[takenA + (f >> 5)] >> (f & 31u)) & 1u)) continue;  // a segment before owns this frame of a
                const int32_t delta = pb - spos[i];
                if (PASS == 1) {
                    const uint32_t bin = (uint32_t)(delta - dmin);
                    if (bin < core) atomicAdd(&hist[bin + slack], 1u);  // (only broken positions fail the check)
                    if ((TAKEN || RATE) && !hit_bits) continue;
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

// ---- the best offset ----------------------------------------------------------------------------------------------------
struct Best {
    uint32_t S, v;
    int32_t d;
};

// the tie order: larger S, larger votes[d], smaller |d|, smaller d
__device__ __forceinline__ bool better(const Best& x, const Best& y) {
    if (x.S != y.S) return x.S > y.S;
    if (x.v != y.v) return x.v > y.v;
    if (iabs(x.d) != iabs(y.d)) return iabs(x.d) < iabs(y.d);
    return x.d < y.d;
}

// Windowed sums and their arg-max under the tie order, the same on every lane: lanes stride over the bins (the window summed
// directly: 2 slack + 1 reads clamped to the histogram, <= 33 for k_valign and k_valign_segments, <= 257 at k_valign_rates'
// slack_r = 16 * 8), wave shuffles, then the four waves through wbest (4 Best of LDS). AGAIN: the caller may come back
// with no barrier since the call before, whose wbest some wave may still be reading (the rounds of k_valign_segments).
template <bool AGAIN>
__device__ __forceinline__ Best best_offset(const uint32_t* hist, uint32_t nbins, uint32_t slack, int32_t dmin, Best* wbest) {
    const uint32_t tid = threadIdx.x;
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
    if (AGAIN) __syncthreads();
    if ((tid & 63u) == 0u) wbest[tid >> 6] = best;
    __syncthreads();
    best = wbest[0];
    for (int w = 1; w < 4; ++w)
        if (better(wbest[w], best)) best = wbest[w];
    return best;
}

// ---- the two launches ---------------------------------------------------------------------------------------------------
constexpr unsigned kSlots = 64;  // workgroups of the scratch launch: one slot of the caller's scratch each

// bytes of scratch for pairs of up to max_bins bins: per slot the histogram and `runs` pairs of runs of bit words
inline size_t slot_scratch_bytes(unsigned long long max_bins, unsigned runs) {
    if (max_bins <= kLdsBins) return 0;
    if (max_bins > kMaxBins) max_bins = kMaxBins;
    return (size_t)kSlots * 4u * (size_t)(max_bins + runs * ((max_bins + 1u) / 32u + 3u));
}

// launch(big, grid, scratch, slot_words) enqueues kernel<big>, big a std::bool_constant. First every pair whose histogram fits
// LDS, one workgroup per pair up to 8192; then the pairs beyond: found again from the same geometry, by as many workgroups as
// there are slots.
template <class Launch>
hipError_t launch_lds_then_scratch(const hvd::AlignOperands& op, Launch launch) {
    const unsigned long long M = (unsigned long long)op.M;
    if (M == 0) return hipSuccess;
    const unsigned grid = (unsigned)(M < 8192ull ? M : 8192ull);
    launch(std::false_type{}, grid, (uint32_t*)nullptr, 0u);
    unsigned long long slot_words = op.scratch ? op.scratch_bytes / 4u / kSlots : 0ull;
    if (slot_words > 2u * kMaxBins) slot_words = 2u * kMaxBins;  // (more than any pair needs)
    const unsigned big_grid = (unsigned)(M < kSlots ? M : kSlots);
    launch(std::true_type{}, big_grid, (uint32_t*)op.scratch, (uint32_t)slot_words);
    return hipGetLastError();
}

}  // namespace

namespace hvd {

// one per kernel file, each with its file's only kernel launch; launch_alignment (k_valign.hip) goes by mode.kind()
hipError_t launch_valign(const AlignMode& mode, const AlignOperands& op, hipStream_t s);
hipError_t launch_valign_segments(const AlignMode& mode, const AlignOperands& op, hipStream_t s);
hipError_t launch_valign_rates(const AlignMode& mode, const AlignOperands& op, hipStream_t s);
hipError_t launch_valign_rate_segments(const AlignMode& mode, const AlignOperands& op, hipStream_t s);
hipError_t launch_valign_signed(const AlignMode& mode, const AlignOperands& op, hipStream_t s);  // k_valign_signed.hip, DESIGN.md 4.25
hipError_t launch_valign_loops(const AlignMode& mode, const AlignOperands& op, hipStream_t s);   // k_valign_loops.hip, DESIGN.md 4.26

}  // namespace hvd
