// hvd_kernels.h -- internal launch interface between the C-ABI host layer
// (hvd_api.cpp) and the gfx950 kernels (k_hamming.hip, k_pdq.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hvd_mi355x.h"
#include "hvd_devhash.h"
#include "hvd_mfma_forms.h"

namespace hvd {

struct AllPairsArgs {
    const void* d_db;        // n * 32 bytes (FP4-MFMA forms: optional, the packed hashes of the image's rows)
    const void* d_db_q = nullptr;  // rectangular form: the packed query hashes (optional)
    uint32_t n;
    const int32_t* d_group;  // nullable
    uint32_t max_dist;
    uint32_t rank, world;
    hvd_pair* d_pairs;
    unsigned long long cap;
    unsigned long long* d_count;
    int variant;
    uint32_t col_chunk;      // 0 = pick automatically
    int ctx_id = 0;          // the caller's context: selects the FP4-MFMA forms' per-context select/context words
    VideoSink sink = {nullptr, 0, nullptr, nullptr, nullptr};  // FP4-MFMA form only: reduce to video level (K3)
    // auto variant only. false: probe and all candidate forms are enqueued, the unchosen ones return at once -- no host
    // synchronisation (the device-resident entry points promise that). true (callers that wait for the result anyway: the video
    // search, the host-buffer entry): the host reads the probe's decision and launches the chosen form alone -- on a 2.9 M-frame
    // library the two empty launches are ~1e6 workgroups each, 0.2 + 0.4 ms.
    bool sync_decide = false;
};

hipError_t launch_allpairs(const AllPairsArgs& a, hipStream_t s);
bool allpairs_geometry(uint32_t n, int variant, uint32_t* rows_per_block, uint32_t* col_chunk);

// FP4-MFMA forms (k_hamming_mfma.hip): the variants of hvd_mfma_forms.h's table, and its auto variant. d_img:
// fp4_rows_padded(n)*128 bytes. The knobs (hvd_debug_set keys of the same names; defined in one block in k_hamming_mfma.hip):
extern uint32_t g_mfma_col_chunk_max, g_mfma_auto_mid, g_mfma_auto_mid_max_x100, g_mfma_queue_packed, g_mfma_probe_packed;
extern int g_mfma_force_sel;
hipError_t launch_expand_fp4(const void* d_db, uint32_t n, void* d_img, hipStream_t s);
hipError_t launch_pack_fp4(const void* d_img, uint32_t n, void* d_db, hipStream_t s);  // image -> packed 32-byte hashes
// data-dependent bit order of the video search (k_hamming_mfma.hip): co-occurrence counts of a strided sample, and the rewrite
hipError_t launch_bit_cooc(const void* d_bits, uint32_t stride, uint32_t words, void* d_rows, void* d_cooc, hipStream_t s);
hipError_t launch_reorder_bits(const void* d_bits_in, uint32_t n, const uint8_t perm[256], void* d_bits_out, void* d_img, hipStream_t s);
hipError_t launch_allpairs_mfma(const AllPairsArgs& a, const void* d_img, hipStream_t s);
// a.n / a.d_group describe the target set; rows are the nq query hashes (image d_img_q, groups a.d_group
// for queries and d_group_t for targets; pass both or neither).
hipError_t launch_cross_mfma(const AllPairsArgs& a, const void* d_img_q, uint32_t nq, const void* d_img_t,
                             const int32_t* d_group_t, hipStream_t s);
hipError_t mfma_select_buffer(int ctx_id, uint32_t** out);  // per context: the select words, hit context and clock words below

// The select buffer, one per CONTEXT of the library (a context = one stream on one device; a group may hold two contexts on one
// device, whose passes run concurrently on their own streams): kSelectWords select words, cleared in front of every pass of
// the auto variant; the pass's hit context (HitCtx, k_hamming_mfma.hip); the clock telemetry's four 64-bit accumulators.
enum : int {
    kSelectWords = 16,
    kSelCtxWord = 16,    // 32-bit word offset of the hit context (byte 64)
    kSelClkWord = 192,   // ... of the clock accumulators (byte 768)
    kSelectBytes = 1024,  // allocated
};
constexpr size_t kHitCtxMaxBytes = 4u * (kSelClkWord - kSelCtxWord);  // (k_hamming_mfma.hip asserts that HitCtx fits)
static_assert(kSelectWords <= kSelCtxWord && kSelCtxWord < kSelClkWord && 4 * kSelClkWord + 4 * 8 <= kSelectBytes, "select buffer layout");
// The probe's select words (k_prefilter_probe, probe_decide):
enum : int {
    kSelForm = 0,          // the form to run (the auto variant's launches of every other form return at once)
    kSelSurvivorsLo = 1,   // first-stage survivors the probe counted over bits 0..127
    kSelSurvivorsHi = 2,   // ... over bits 128..255
    kSelSelection = 3,     // the selection the first stage runs on: 0 = bits 0..127, 1 = bits 128..255, 2 = bits 0..63 + 192..255
    kSelProbeTicket = 4,   // the probe's last workgroup decides
    kSelSurvivorsMix = 5,  // ... over bits 0..63 + 192..255
};

// Pigeonhole index path of the auto variant's self all-pairs pass (k_hamming_index.hip): 16 blocks of 16 bits; two hashes
// within max_dist <= 31 agree to within r bits (r = 1 for max_dist 16..31, 0 below 16) in at least one block, so only pairs
// that share a block key or whose keys differ in one bit are compared. Select words it owns (cleared with the probe's words in
// front of every pass):
enum : int {
    kSelIdxClose = 6,    // probe: sampled pairs x blocks with block distance <= r
    kSelIdxUsed = 7,     // 1: the index path runs this pass (the matrix-core forms return at once)
    kSelIdxCand = 8,     // words 8, 9: exact candidates of the pass (sum over blocks of the pairs within r in that block)
    kSelIdxMaxWalk = 10,  // the longest work item: max over (b, u) of c_u x (c_u + the counts of its neighbours above u)
    kSelIdxTicket = 11,  // the statistics kernel's last workgroup decides
    kSelIdxGate = 12,    // the probe's estimate lets the keys be sorted and counted at all
};
// The cost rule (calibrated on MI355X): nanoseconds of the index pass against the matrix-core pass.
struct IndexRule {
    double pairs;         // n (n - 1) / 2 (every rank does 1/world of either pass)
    double n;
    uint32_t r;           // block radius
    uint32_t force;       // 1: the index path whenever eligible (hvd_debug_set "allpairs_index" 1)
    uint32_t world;
    float fs_mfma_fetch;  // femtoseconds per comparison of form 9 / of the other matrix-core forms
    float fs_mfma_other;
    float ps_cand;        // picoseconds per candidate (join)
    float ps_hash;        // picoseconds per hash (counting sort: what of it grows with n)
    float ps_crit;        // picoseconds per pair of the longest work item: one wave walks it alone (critical path)
    float fixed_ns;       // launches of the index pass and its kernels whose length does not depend on n
};
// (form: the matrix-core form the probe chose; any other value prices the costlier forms)
__host__ __device__ inline bool index_wins(const IndexRule& q, double cand, double max_walk, uint32_t form) {
    if (q.force) return true;
    const double t_mfma = q.pairs / q.world * (form == (uint32_t)kFormFetch ? q.fs_mfma_fetch : q.fs_mfma_other) * 1e-6;
    const double t_idx = q.fixed_ns + q.n * q.ps_hash * 1e-3 + cand / q.world * q.ps_cand * 1e-3 + max_walk * q.ps_crit * 1e-3;
    return t_idx < t_mfma;
}
extern int g_allpairs_index;       // hvd_debug_set "allpairs_index": -1 auto, 0 never, 1 force when eligible
extern int g_allpairs_index_fail;  // fault injection (tests): context (value - 1) fails to reserve its index scratch; 0 = off
extern int g_index_stage;          // hvd_debug_set "index_stage": 1 the high-byte pass lays a tile's runs out in LDS (k_index_scatter), 0 k_index_partition
extern int g_index_join_wgs;       // tests: workgroups of the join; 0 = sized by the device and, above 2^20 hashes, by n (index_join_workgroups)
// Eligible: self pass (not query x target, not the video sink), max_dist <= 31, packed hashes at hand, not switched off, and
// -- unless forced -- a DB large enough that the index could win even with no candidates at all. Depends only on what every
// rank of a pass shares (arguments, n, world, the process-wide key), so all ranks agree.
bool index_eligible(const AllPairsArgs& a, bool rect, uint32_t* r);
IndexRule index_rule(const AllPairsArgs& a, uint32_t r);
// Grows the context's index scratch (~28 B x 16 per hash: half-hash copies, rows, partition records). Called outside the launch lock: growing frees the old buffer,
// which waits for the whole device.
hipError_t index_reserve(int ctx_id, uint32_t n);
// Counting sort of the keys (partition, per-key counts, offsets), exact statistics and decision (select[kSelIdxUsed]); then
// place and join. Every kernel of the first call
// returns at once unless the probe's gate is set, every kernel of the second unless the decision is.
hipError_t launch_index_decide(const AllPairsArgs& a, uint32_t* d_select, const IndexRule& q, hipStream_t s);
hipError_t launch_index_join(const AllPairsArgs& a, uint32_t* d_select, uint32_t r, hipStream_t s);
// the partitions that fit LDS, ordered whole (k_index_order.hip): launched by launch_index_decide behind the partition pass
hipError_t launch_index_order(const uint2* rec, uint32_t n, const uint32_t* ptotal, const uint32_t* pbase, uint32_t* cnt, uint32_t* off,
                              uint32_t* hw, uint32_t* rows, const uint32_t* d_select, hipStream_t s);
// the high-byte pass with a tile's runs laid out in LDS (k_index_scatter.hip): launched by launch_index_decide where
// k_index_partition was, same arguments, unless "index_stage" is 0; its grid is (ntiles, split), split = 1, 2 or 4
hipError_t launch_index_scatter(const uint4* db, uint32_t n, uint32_t ntiles, uint32_t split, const uint32_t* tcnt, const uint32_t* pbase,
                                uint2* rec, const uint32_t* d_select, hipStream_t s);
// block groups per tile of k_index_scatter for n hashes on a device of `cus` compute units (host arithmetic only)
uint32_t index_tile_split(uint32_t n, uint32_t cus);
extern int g_index_tile_split;  // tests: 1 | 2 | 4 forces that split; 0 = index_tile_split
// tests (hvd_debug_index_tiles): the build up to the partition records into the caller's buffers; d_parts = ptotal[4096],
// pbase[4096], pfirst[4096 + 4], chunk_p; d_tcnt_raw = the tile counts before the scan over the tiles
hipError_t index_tiles_debug(const void* d_db, uint32_t n, const uint32_t* d_select, uint32_t* d_tcnt_raw, uint32_t* d_tcnt, uint32_t* d_parts,
                             void* d_rec, hipStream_t s);
// the join's grid for n hashes on the current device (or what "index_join_wgs" sets): the same for every n <= 2^20
hipError_t index_join_workgroups(uint32_t n, uint32_t* wgs);
void index_release();
// clock telemetry of a context's all-pairs passes: {shader cycles, constant-rate ticks, sampled workgroups, 0} since the reset
hipError_t mfma_clock_reset(int ctx_id, hipStream_t s);
hipError_t mfma_clock_read(int ctx_id, hipStream_t s, unsigned long long out[4]);
void mfma_release();
void pdq_release();           // k_pdq.hip: free the hash kernel's work-counter ring (hvd_shutdown)
void stream_release_cache();  // hvd_stream.cpp: free the parked hasher slot sets (hvd_shutdown)
void stream_set_copy_nt(int on);  // hvd_stream.cpp / copy_pool.h: non-temporal stores into the pinned ring (debug key "copy_nt")
int stream_copy_nt_level();
long long stream_take_ns(int which);  // 0 copy, 1 submit, 2 wait: host time of the streaming feed since the last read
bool allpairs_mfma_geometry(uint32_t n, int variant, uint32_t* rows_per_block, uint32_t* col_chunk);

// Video-level reduction and quality compaction (k_vmatch.hip).
hipError_t launch_keys_to_pairs(const unsigned long long* d_src, unsigned long long n_src, const int32_t* d_vid_q,
                                const int32_t* d_vid_t, bool rect, unsigned long long* d_pkeys, void* d_pcnt,
                                unsigned long long pmask, unsigned long long* d_counters, hipStream_t s);
hipError_t launch_pairs_emit(const unsigned long long* d_pkeys, const void* d_pcnt, unsigned long long slots, hvd_vmatch* d_out,
                             unsigned long long cap, unsigned long long* d_count, hipStream_t s);
hipError_t launch_set_to_list(const unsigned long long* d_tab, unsigned long long slots, unsigned long long* d_list,
                              unsigned long long cap, unsigned long long* d_count, hipStream_t s);
hipError_t launch_list_to_set(const unsigned long long* d_list, unsigned long long n, unsigned long long* d_tab,
                              unsigned long long mask, unsigned long long* d_counters, hipStream_t s);
size_t compact_scratch_bytes(unsigned long long n);
hipError_t launch_compact_kept(const void* d_hashes, const int32_t* d_quality, unsigned long long n, const long long* d_offsets,
                               uint32_t V, int min_q, void* d_out_hashes, long long* d_out_offsets, int32_t* d_out_video,
                               void* d_scratch, unsigned long long* d_total, hipStream_t s);
hipError_t launch_compact_kept_dihedral(const void* d_hashes8, const int32_t* d_quality, unsigned long long n,
                                        const long long* d_offsets, uint32_t V, int min_q, uint32_t mask, void* d_out_hashes,
                                        long long* d_out_offsets, int32_t* d_out_video, void* d_q_hashes, int32_t* d_q_video,
                                        int32_t* d_q_excl, void* d_scratch, unsigned long long* d_total, hipStream_t s);
hipError_t launch_video_of_frames(const long long* d_offsets, uint32_t V, unsigned long long n, int32_t* d_out_video,
                                  hipStream_t s);

hipError_t launch_kept_positions(const int32_t* d_quality, unsigned long long n, const long long* d_offsets, uint32_t V, int min_q,
                                 int32_t* d_out_pos, void* d_scratch, unsigned long long* d_total, hipStream_t s);

// Common-frame filter (k_spread.hip). launch_keys_to_spread: d_src / n_src as launch_keys_to_pairs takes them, d_spread
// int32[n], zeroed by the launcher on s. launch_common_rule: d_keep int32[n], 1 or 0. launch_gather_kept_i32: d_scratch of
// compact_scratch_bytes(n), d_total one uint64 (device) that receives the kept count.
hipError_t launch_keys_to_spread(const unsigned long long* d_src, unsigned long long n_src, unsigned long long n,
                                 int32_t* d_spread, hipStream_t s);
// launch_keys_to_spread_cross: the rectangular key set, side 0 -> d_spread_q int32[nq], side 1 -> d_spread_t
// int32[nt]; either may be nullptr. Zeroed by the launcher on s unless `accumulate`: the counts are then added to what is there.
hipError_t launch_keys_to_spread_cross(const unsigned long long* d_src, unsigned long long n_src, unsigned long long nq,
                                       unsigned long long nt, bool accumulate, int32_t* d_spread_q, int32_t* d_spread_t,
                                       hipStream_t s);
hipError_t launch_common_rule(const int32_t* d_spread, const long long* d_offsets, uint32_t V, unsigned long long n,
                              int max_videos, int max_share, int32_t* d_keep, hipStream_t s);
hipError_t launch_gather_kept_i32(const int32_t* d_in, const int32_t* d_keep, unsigned long long n, int32_t* d_out,
                                  void* d_scratch, unsigned long long* d_total, hipStream_t s);

// Static-scene filter (k_runs.hip): d_hashes 32 B per frame, d_offsets a CSR over the n frames -> d_keep int32[n],
// 1 or 0, and d_run int32[n] (may be nullptr), the frames a kept frame stands for. One launch of at most kFrameRunsMaxBlocks
// workgroups (4 waves per SIMD on 256 compute units), each striding over groups of four videos.
constexpr unsigned kFrameRunsMaxBlocks = 1024;
hipError_t launch_frame_runs(const void* d_hashes, const long long* d_offsets, uint32_t V, unsigned long long n, int max_dist,
                             int max_run, int32_t* d_keep, int32_t* d_run, hipStream_t s);

// Duration-weighted video search (k_vmatch_weighted.hip). launch_keys_to_pairs_weighted: launch_keys_to_pairs
// with an int32 weight per frame of each side (d_weight_t == d_weight_q in the symmetric form); every key adds
// max_weight ? min(weight, max_weight) : weight to its counter instead of 1. launch_video_weights: d_totals int64[V], the sum
// of the capped weights per video of a CSR over the n frames (ranges clamped to [0, n]); one launch of at most
// kVideoWeightsMaxBlocks workgroups, each striding over groups of four videos.
constexpr unsigned kVideoWeightsMaxBlocks = 1024;
hipError_t launch_keys_to_pairs_weighted(const unsigned long long* d_src, unsigned long long n_src, const int32_t* d_vid_q,
                                         const int32_t* d_vid_t, bool rect, const int32_t* d_weight_q, const int32_t* d_weight_t,
                                         uint32_t max_weight, unsigned long long* d_pkeys, void* d_pcnt, unsigned long long pmask,
                                         unsigned long long* d_counters, hipStream_t s);
hipError_t launch_video_weights(const int32_t* d_weight, const long long* d_offsets, uint32_t V, unsigned long long n,
                                uint32_t max_weight, long long* d_totals, hipStream_t s);

// Time alignment of listed video pairs: one offset per pair (k_valign.hip, 4.8), up to eight (k_valign_segments.hip,
// 4.9), one line at the best of the listed rates (k_valign_rates.hip, 4.10), rate x segments (k_valign_rate_segments.hip, 4.18).
// A fifth, rate x segments with negative numerators for clips played backwards (k_valign_signed.hip, 4.25), came later, and a
// sixth, the fifth without a taken set on the b side and with up to 64 rounds, for looped clips (k_valign_loops.hip, 4.26).
// AlignMode says which of them a call is and carries what only some of them take; everything that differs between them on
// the host is read off it.
struct AlignMode {
    uint32_t nums, dens;               // rated: the packed list (pack_rate_list below); 0, 0: a broken list
    int max_segments, min_band_votes;  // segmented: as the caller gave them (check_segment_limits judges them)
    bool rated, segmented;
    bool args_first;  // the host entry judges its arguments before the library's state (the rate entries), not after
    // signed_: rate x segments with negative numerators (k_valign_signed.hip; `signed` is a keyword). nums and
    // dens then hold |num| and den, and bit r of revs says that entry r is negative (pack_signed_rate_list below).
    bool signed_ = false;
    uint32_t revs = 0u;
    // loops: the signed rule without b's taken set (k_valign_loops.hip); max_segments then holds max_rounds, up to
    // HVD_ALIGN_MAX_ROUNDS, and a slot of scratch holds a third pair of runs of bit words, the seen words
    bool loops = false;
    static AlignMode of(bool rated, bool segmented, int max_segments = 0, int min_band_votes = 1) {
        return {0u, 0u, max_segments, min_band_votes, rated, segmented, rated};
    }
    static AlignMode of_signed(int max_segments, int min_band_votes) {
        AlignMode m = of(true, true, max_segments, min_band_votes);
        m.signed_ = true;
        return m;
    }
    static AlignMode of_loops(int max_rounds, int min_band_votes) {
        AlignMode m = of_signed(max_rounds, min_band_votes);
        m.loops = true;
        return m;
    }
    unsigned kind() const { return loops ? 5u : signed_ ? 4u : (rated ? 2u : 0u) + (segmented ? 1u : 0u); }
    size_t record_bytes() const {
        constexpr size_t bytes[6] = {sizeof(hvd_valign), sizeof(hvd_vsegments), sizeof(hvd_vrate), sizeof(hvd_vrsegments),
                                     sizeof(hvd_vssegments), sizeof(hvd_vloops)};
        return bytes[kind()];
    }
    unsigned runs() const { return segmented ? 2u : 1u; }  // pairs of runs of bit words: the flag words, and the taken words
    // ... and the seen words of a loops mode: what a slot is sized for. (Separate from runs() only because
    // tests/test_rate_segments_cpu.py matches the text of the line above; one function once that test lets go of it.)
    unsigned slot_runs() const { return loops ? 3u : runs(); }
    bool records16() const { return rated || segmented; }  // the kernel zeroes its records 16 bytes at a time
};

// The operands every alignment takes, as the C entries name them: on the device for launch_alignment, host buffers (scratch
// unused) for the host entries. hashes: 32 bytes per frame; offsets: int64 CSR; pos: int32 per frame or nullptr; pairs: uint32[M][2].
struct AlignOperands {
    const void *hashes_q, *offsets_q;
    int64_t VQ;
    const void *pos_q, *hashes_t, *offsets_t;
    int64_t VT;
    const void *pos_t, *pairs;
    int64_t M;
    int max_dist, slack;
    void* scratch;
    size_t scratch_bytes;
    void* out;
};

// Two launches: the pairs whose (largest) delta histogram fits LDS, then the larger ones out of op.scratch
// (alignment_scratch_bytes(mode, max_bins), max_bins: the largest bins, or bins_r of any listed rate, of any pair; may be
// nullptr / 0: such pairs then get the INT32_MIN record). A slot of a segmented mode's scratch also holds the pair's taken sets.
size_t alignment_scratch_bytes(const AlignMode& mode, unsigned long long max_bins);
hipError_t launch_alignment(const AlignMode& mode, const AlignOperands& op, hipStream_t s);

// Coverage of a video by several others (k_valign_cover.hip): the slope-one alignment with a second output, not a
// fifth mode. align: one library on both sides (the q operands are read), out = M hvd_valign; its scratch holds the bitmap
// over the n_frames frames of the library (cover_bitmap_bytes, 16-byte aligned), then the slots of the scratch launch
// (alignment_scratch_bytes of the slope-one mode). cover: VQ hvd_vcover. Enqueued: the clear of the bitmap and of the cover
// records, the two launches, the count.
struct CoverOperands {
    AlignOperands align;
    int64_t n_frames;
    int min_aligned;
    void* cover;
};
size_t cover_bitmap_bytes(unsigned long long n_frames);
size_t cover_scratch_bytes(unsigned long long n_frames, unsigned long long max_bins);
hipError_t launch_valign_cover(const CoverOperands& op, hipStream_t s);

// The rate list of the rate-aware alignments travels as two kernel arguments: entry r = (num, den) in bits 4r .. 4r + 3 of nums and
// of dens, and it ends at the first entry whose two nibbles are 0. rate_list_length: its length R, or 0 for a broken list (a
// value outside 1..8, a pair with a common factor, a rate listed twice, something behind the end, no entry) -- the one definition
// of a sound list, for the host entries and for the kernel (which then gives every pair the INT32_MIN record).
constexpr uint32_t rate_list_length(uint32_t nums, uint32_t dens) {
    uint32_t R = 0;
    while (R < (uint32_t)HVD_ALIGN_MAX_RATES && (((nums | dens) >> (4u * R)) & 15u)) ++R;
    if (R < (uint32_t)HVD_ALIGN_MAX_RATES && ((nums | dens) >> (4u * R))) return 0u;
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t num = (nums >> (4u * r)) & 15u, den = (dens >> (4u * r)) & 15u;
        if (num - 1u >= 8u || den - 1u >= 8u) return 0u;
        for (uint32_t f = 2; f <= 7u; ++f)
            if (num % f == 0u && den % f == 0u) return 0u;
        for (uint32_t q = 0; q < r; ++q)
            if (((nums >> (4u * q)) & 15u) == num && ((dens >> (4u * q)) & 15u) == den) return 0u;
    }
    return R;
}
// (num, den) x n_rates as the caller lists them -> the two words; false (and 0, 0: a broken list) unless the list is sound
inline bool pack_rate_list(const int32_t* rates, int n_rates, uint32_t* nums, uint32_t* dens) {
    *nums = *dens = 0u;
    if (!rates || n_rates < 1 || n_rates > HVD_ALIGN_MAX_RATES) return false;
    uint32_t nn = 0, dd = 0;
    for (int r = 0; r < n_rates; ++r) {
        if (rates[2 * r] < 1 || rates[2 * r] > 8 || rates[2 * r + 1] < 1 || rates[2 * r + 1] > 8) return false;
        nn |= (uint32_t)rates[2 * r] << (4 * r);
        dd |= (uint32_t)rates[2 * r + 1] << (4 * r);
    }
    if (rate_list_length(nn, dd) != (uint32_t)n_rates) return false;
    *nums = nn;
    *dens = dd;
    return true;
}
// The signed list of the alignment with negative rates travels as three words: nums and dens as above with |num|
// in nums, and revs, bit r set when entry r is negative. signed_rate_list_length: its length R, or 0 for a broken list -- the
// magnitudes judged as rate_list_length judges them, except that a pair may be listed once per sign; a bit of revs at or
// behind the end breaks the list. The one definition of a sound signed list, for the host entry and for the kernel.
constexpr uint32_t signed_rate_list_length(uint32_t nums, uint32_t dens, uint32_t revs) {
    uint32_t R = 0;
    while (R < (uint32_t)HVD_ALIGN_MAX_RATES && (((nums | dens) >> (4u * R)) & 15u)) ++R;
    if (R < (uint32_t)HVD_ALIGN_MAX_RATES && ((nums | dens) >> (4u * R))) return 0u;
    if (revs >> R) return 0u;
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t num = (nums >> (4u * r)) & 15u, den = (dens >> (4u * r)) & 15u;
        if (num - 1u >= 8u || den - 1u >= 8u) return 0u;
        for (uint32_t f = 2; f <= 7u; ++f)
            if (num % f == 0u && den % f == 0u) return 0u;
        for (uint32_t q = 0; q < r; ++q)
            if (((nums >> (4u * q)) & 15u) == num && ((dens >> (4u * q)) & 15u) == den && (((revs >> q) ^ (revs >> r)) & 1u) == 0u)
                return 0u;
    }
    return R;
}
// (num, den) x n_rates as the caller lists them, num of either sign -> the three words; false (and 0, 0, 0: a broken list)
// unless the list is sound as a signed list
inline bool pack_signed_rate_list(const int32_t* rates, int n_rates, uint32_t* nums, uint32_t* dens, uint32_t* revs) {
    *nums = *dens = *revs = 0u;
    if (!rates || n_rates < 1 || n_rates > HVD_ALIGN_MAX_RATES) return false;
    uint32_t nn = 0, dd = 0, vv = 0;
    for (int r = 0; r < n_rates; ++r) {
        const int32_t num = rates[2 * r], den = rates[2 * r + 1];
        if (num < -8 || num > 8 || num == 0 || den < 1 || den > 8) return false;
        nn |= (uint32_t)(num < 0 ? -num : num) << (4 * r);
        dd |= (uint32_t)den << (4 * r);
        vv |= (num < 0 ? 1u : 0u) << r;
    }
    if (signed_rate_list_length(nn, dd, vv) != (uint32_t)n_rates) return false;
    *nums = nn;
    *dens = dd;
    *revs = vv;
    return true;
}

// The two groupings over a list of 16-byte edge records: connected components (k_group.hip) and
// keeper-first groups (k_keeper.hip) take the same operands and fill the same outputs.
// EdgeList: the records in HBM, named and typed as by the C entries (group_on_device judges the ranges, the launchers narrow).
// d_record_count: nullptr, or the uint64 an all-pairs pass counted its records in (the kernels then take min(*d_record_count,
// n_records)); d_lengths, T, is_min: the pair predicate of HVD_EDGES_VMATCH; d_score: uint32 per node or nullptr.
struct EdgeList {
    const void* records;
    int64_t n_records;
    const unsigned long long* d_record_count;
    int kind;
    const long long* d_lengths;
    int T;
    bool is_min;
    int64_t V;
    const uint32_t* d_score;
};
// GroupsOut: scratch: group_scratch_bytes(V) or keeper_scratch_bytes(V), 8-byte aligned; node: int32 per node, the labels or
// keeper_of; groups: room for cap records; count: one uint64, receives the number of groups.
struct GroupsOut {
    void* scratch;
    int32_t* node;
    hvd_group* groups;
    int64_t cap;
    unsigned long long* count;
};
size_t group_scratch_bytes(unsigned long long V);
hipError_t launch_group_edges(const EdgeList& edges, const GroupsOut& out, hipStream_t s);
// The keeper-first rounds are enqueued in batches of 32 with the undecided count read back in between, so the call synchronises
// the stream; *settled: no node was left undecided within V rounds (else nothing else was launched); *rounds (may be nullptr):
// the rounds that ran.
size_t keeper_scratch_bytes(unsigned long long V);
hipError_t launch_keeper_groups(const EdgeList& edges, const GroupsOut& out, hipStream_t s, long long* rounds, bool* settled);

// Synthetic 64x64 gray video frames generated in HBM (k_synth.hip; workload generator, not on the hashing path).
hipError_t launch_synth_frames64(uint8_t* d_out, long long v0, uint32_t frames_per_video, unsigned long long n_frames,
                                 uint64_t seed, const int32_t* d_copy_of, hipStream_t s);

hipError_t launch_match_two(const uint32_t* d_a, uint32_t na, const uint32_t* d_b, uint32_t nb, uint32_t max_dist,
                            uint32_t* d_tflags, int32_t* d_hits, hipStream_t s);
uint32_t match_two_small_limit();
hipError_t launch_match_server(const uint32_t* ops, int32_t* hdr, uint32_t last, int32_t launch_id, unsigned long long idle_ticks,
                               unsigned long long life_ticks, hipStream_t s);
hipError_t launch_match_two_small(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb, uint32_t max_dist,
                                  int32_t* hits, int32_t seq, hipStream_t s);

// PDQ frame hashing. d_dct: 16*64 floats (host-computed, uploaded once).
// kind 0: gray u8 64x64 frames; kind 1: float 64x64 buffers (output of the
// down-sampler). d_in strides are implied by kind.
extern int g_pdq_dct_from_lds;
void pdq_dct_table_copy(float* out_16x64);               // the compiled-in DCT matrix (csrc/dct_table.inc): authoritative
bool pdq_dct_table_matches(const float* host_16x64);  // the kernels' compile-time DCT table vs the host's computation
extern int g_pdq_hash_grid;
extern int g_pdq_dct_mode;
extern bool g_pdq_fused_down512;
extern int g_pdq_down512_wave;
extern int g_pdq_down512_wave_grid;
extern int g_pdq_down512_strip;
hipError_t launch_pdq_hash64(const void* d_in, int kind, int64_t n, const float* d_dct, uint8_t* d_hashes,
                             int32_t* d_quality, hipStream_t s);
// The 8 dihedral hashes of every frame (k_pdq_dihedral.hip, strict DCT only): d_hashes8 n*8*32 bytes, identity first.
hipError_t launch_pdq_dihedral64(const void* d_in, int kind, int64_t n, const float* d_dct, uint8_t* d_hashes8,
                                 int32_t* d_quality, hipStream_t s);

// Luma + 2x Jarosz box filter + decimate to 64x64 float, for h,w != 64 (the
// reference's 512x512 rgb24 frames, vpdqpy/vpdqpy.py:90-95,113).
// d_ws: min(n,1024) * pdq_downsample_ws_floats(h,w) floats of workspace.
size_t pdq_downsample_ws_floats(int h, int w);
size_t pdq_down512_ws_floats(int64_t n);  // of those, what a 512 x 512 call needs while g_pdq_fused_down512 is on
hipError_t launch_pdq_downsample(const uint8_t* d_frames, int64_t n, int h, int w, int channels, float* d_ws,
                                 float* d_out64, hipStream_t s);
// 64x64 rgb24 frames: luma only (no blur, as upstream's 64x64 shortcut).
hipError_t launch_pdq_luma64_rgb(const uint8_t* d_frames, int64_t n, float* d_out64, hipStream_t s);

// Content-rectangle PDQ (k_autocrop.hip). d_offsets: the int64[V+1] CSR of the n frames; d_rects: int32[V][4]
// {top, left, height, width}, also the kernels' accumulator (nothing else is allocated).
// The rule that finds the rectangle: a row (column) is content iff it holds >= count of what the kind counts --
//   Black   pixels with max(R, G, B) > level                                          (level = black_level, count = min_bright)
//   Color   pixels with max_k |p_k - c_k| > level, c the video's colour in d_colors   (bar_level, min_bright)
//   Detail  horizontal (vertical) neighbour pairs with max_k |p_k - p'_k| > level     (detail_level, min_detail)
// d_colors: int32[V] = c0 | c1 << 8 | c2 << 16 for Color, unused (nullptr) otherwise.
enum class RectKind { Black, Color, Detail };
struct RectRule {
    RectKind kind;
    int level, count;
};
hipError_t launch_content_rects(const RectRule& rule, const int32_t* d_colors, const uint8_t* d_frames, int64_t n, int h, int w,
                                int channels, const long long* d_offsets, uint32_t V, int32_t* d_rects, hipStream_t s);
// ... and its three steps one by one (rectangle accumulators are folded batch by batch by the streaming hasher).
hipError_t launch_rect_init(int32_t* d_rects, uint32_t V, hipStream_t s);
hipError_t launch_rect_fold(const RectRule& rule, const int32_t* d_colors, const uint8_t* d_frames, int64_t n, int h, int w,
                            int channels, const long long* d_offsets, uint32_t V, int32_t* d_rects, hipStream_t s);
hipError_t launch_rect_finish(int32_t* d_rects, uint32_t V, int h, int w, hipStream_t s);
// what launch_rect_fold chooses from: the fold of one kind, in that kind's file (k_autocrop.hip, k_barcolor.hip, k_detail.hip)
hipError_t rect_fold_black(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets, uint32_t V,
                           int black_level, int min_bright, int32_t* d_rects, hipStream_t s);
hipError_t rect_fold_color(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets, uint32_t V,
                           const int32_t* d_colors, int bar_level, int min_bright, int32_t* d_rects, hipStream_t s);
hipError_t rect_fold_detail(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets, uint32_t V,
                            int detail_level, int min_detail, int32_t* d_rects, hipStream_t s);
// The generic four-pass down-sampler inside every frame's video rectangle. d_geom: pdq_rects_geom_bytes(n) bytes (the
// frame -> rectangle table); d_ws as for launch_pdq_downsample (sized for the full h x w).
// Frames with h <= 512 and w <= 512 take the fused k_down_rect (one launch, same planes bit for bit) unless
// g_pdq_fused_rect is off (hvd_debug_set "pdq_fused_rect").
extern bool g_pdq_fused_rect;
constexpr int kDownRectMax = 512;  // largest frame side k_down_rect takes (k_autocrop_fused.hip)
void launch_down_rect(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const void* d_geom, float* d_out64,
                      hipStream_t s);
size_t pdq_rects_geom_bytes(int64_t n);
hipError_t launch_pdq_downsample_rects(const uint8_t* d_frames, int64_t n, int h, int w, int channels,
                                       const long long* d_offsets, uint32_t V, const int32_t* d_rects, void* d_geom,
                                       float* d_ws, float* d_out64, hipStream_t s);

// Bar-colour content rectangle (k_barcolor.hip). d_colors: int32[V] = c0 | c1 << 8 | c2 << 16, the bar colour
// of every video. launch_bar_colors finds it from the four corner pixels of every frame; d_acc: bar_colors_scratch_bytes(V)
// bytes of accumulators. The rectangles then come from launch_content_rects with a RectKind::Color rule.
size_t bar_colors_scratch_bytes(uint32_t V);
hipError_t launch_bar_colors(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const long long* d_offsets,
                             uint32_t V, int bar_level, int32_t* d_acc, int32_t* d_colors, hipStream_t s);

// Crop-ladder PDQ (k_crops.hip). crops: HOST int32[K][4] {top, left, height, width}; crops_valid: 1 <= K <=
// HVD_MAX_CROPS and every crop inside the h x w frame with both sides >= 64 -- the one definition of a sound list.
bool crops_valid(const int32_t* crops, int K, int h, int w);
size_t pdq_crops_scratch_bytes(int64_t n, int h, int w, int K);
hipError_t launch_pdq_hash_crops(const uint8_t* d_frames, int64_t n, int h, int w, int channels, const int32_t* crops, int K,
                                 const float* d_dct, void* d_scratch, uint8_t* d_hashes8, int32_t* d_quality,
                                 int32_t* d_crop_quality, hipStream_t s);

}  // namespace hvd
