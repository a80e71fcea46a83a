/* hvd_mi355x_bench.h -- NOT part of the drop-in boundary.
 *
 * Entry points that exist for this repository's own tests and bench.py only: a workload generator and a test hook. The
 * reference's FFI for this path would bind none of them; they are kept out of include/hvd_mi355x.h so
 * that header is exactly the interface a maintainer binds. A product build may leave them out of the library with
 * -DHVD_NO_BENCH_SYMBOLS. Same conventions as hvd_mi355x.h (int return = HVD_OK or a negative code). */
#ifndef HVD_MI355X_BENCH_H
#define HVD_MI355X_BENCH_H
#include "hvd_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Workload generator (tests / bench.py, BASELINE config 5): writes n_videos * frames_per_video synthetic 64x64 gray
 * frames for videos [v0, v0 + n_videos) to d_frames. Every frame is a pure function of (seed, video, frame index):
 * smooth random field + noise, ~5 % exact constants; d_copy_of (int32 per video of the WHOLE library, indexed by
 * absolute video number, or NULL): videos with copy_of[v] = s >= 0 are video s with +-2 noise per pixel. */
int hvd_dev_synth_video_frames(void* d_frames, int64_t v0, int64_t n_videos, int frames_per_video, uint64_t seed,
                               const void* d_copy_of);

/* Test hook, host only (no device needed): one frame copy through the streaming hasher's helper-thread pool, exactly as
 * hvd_hasher_push does it for a frame of n bytes with `threads` copy threads. tests/test_copy_pool.py hammers it from
 * several threads with different thread counts (the generation race of round 3's pool needed exactly that). */
int hvd_debug_parallel_copy(void* dst, const void* src, size_t n, int threads);

/* Fault injection, tests only: hvd_debug_set("allpairs_index_fail_ctx", c + 1) makes context c's reservation of the
 * pigeonhole index's scratch fail, as if its device were out of memory: a pass of world > 1 then fails on every rank, a
 * lone pass falls back to the matrix cores; 0 = off. Same build rule as the key below.
 * Tests only, same build rule: hvd_debug_set("index_join_wgs", n) launches the pigeonhole index's join with exactly n
 * workgroups (1 .. 2^20) instead of as many as the device holds at once (0, the default), so that one wave walks many work
 * items, or crosses a block, on a DB small enough to check against the oracle; hvd_debug_get of the same key returns the
 * workgroups the next launch takes. Results do not depend on it.
 * Tests only, same build rule: hvd_debug_set("index_tile_split", G) launches the high-byte pass of the pigeonhole index's
 * build (k_index_scatter) on a grid of (tiles, G), G = 1 | 2 | 4 block groups per tile, instead of the G that n and the
 * device's compute units give (0, the default: 1 or 2); process-wide like "index_stage". Results do not depend on
 * it. Two entry points of the same build rule belong to it, which tests/test_gpu_index_tile_split.py and
 * tests/test_index_tile_split_rule.py bind by hand -- they have no prototype here and no row in the ctypes table:
 *   hvd_index_tile_split(int64_t n, int cus) -> the G of n hashes on a device of cus compute units (host arithmetic only);
 *   hvd_debug_index_tiles(const void* d_db, int64_t n, const void* d_select, void* d_tcnt_raw, void* d_tcnt, void* d_parts,
 *   void* d_rec) -> HVD_OK: the build up to the partition records, as a pass launches it, into the caller's device buffers --
 *   d_select: 16 words with word 12 (the gate) set; d_tcnt_raw, d_tcnt: 4096 x tiles words, the tile counts and their scan
 *   over the tiles; d_parts: ptotal[4096], pbase[4096], pfirst[4096 + 4], chunk_p[6144]; d_rec: 16 n records of 8 bytes.
 *   Does not synchronise.
 * Fault injection, tests only: hvd_debug_set("vmatch_fail_rank", r + 1) makes rank r of the next video-level search fail
 * before the key exchange, so that the agreement step (every rank leaves the collective with the same error instead of
 * hanging) can be tested; 0 = off. Like the two entry points above it is absent from -DHVD_NO_BENCH_SYMBOLS builds (the
 * key is then unknown: HVD_ERR_ARG), and it is deliberately NOT in the key list of hvd_mi355x.h.
 * Tests only, same build rule: hvd_debug_set("hash_staging_bytes", v) lowers the frames a host-buffer hashing entry
 * (hvd_pdq_hash_frames_*) stages per batch from 1 GiB to v >= 4096 bytes (at least one frame), so that the multi-batch
 * paths run at shapes that take milliseconds; 0 = the default. Results do not depend on it, except that the autocrop
 * entries refuse (HVD_ERR_ARG) a video with more frames than one batch holds.
 * Tests only, same build rule: hvd_debug_set("match_seq", v) sets the call counter of hvd_match_two's two small-operand
 * routes to v, taken as 32 bits; the next such call carries the number after it (v + 1, or 1 after 0xFFFFFFFF: 0 is
 * skipped), so that the wrap of the 21 bits the match server's request word carries, the step past 0x7FFFFFFF and the wrap
 * of the counter itself are reached in a few calls instead of millions. The answer word is set to v as well: it cannot be
 * taken for the next call's. hvd_debug_get of the same key reads the counter (its 32 bits as an int). Answers do not
 * depend on it. hvd_debug_get("match_server_launches") returns the id of the last match server launched: it rises by one
 * per launch, and stays when the per-call kernel or the device-buffer kernel serves a call. */

/* Test hooks: the pieces of the video search's data-dependent bit order ("vmatch_bit_order"), one at a time, so that
 * tests/test_bit_order_cpu.py and tests/test_gpu_bit_order.py can compare each with numpy. Every one of them calls what the
 * search itself calls; none changes what a search does.
 *
 * hvd_dev_bit_cooc: the search's sample of the n packed 32-byte hashes at d_bits -- *sample = min(n, 16384) rounded down to
 * a multiple of 64, every *stride = n / *sample -th hash from hash 0 on -- and the co-occurrence counts of its bits in
 * d_cooc (256 * 256 uint32: [i][j] = sampled hashes with bits i and j both set). Fewer than 4096 hashes (force != 0: fewer
 * than 64) are too few to choose an order from: *sample = *stride = 0 and d_cooc is not written. Synchronises. */
int hvd_dev_bit_cooc(const void* d_bits, int64_t n, int force, void* d_cooc, uint32_t* sample, uint32_t* stride);

/* Host only (no device needed): the order the search chooses from such counts: perm[0..127] = the 128 kept bits,
 * ascending, perm[128..255] = the dropped ones, ascending; bit k of a rewritten hash is bit perm[k] of the original. */
int hvd_bit_order_from_cooc(const uint32_t* cooc, uint32_t sample, uint8_t* perm);

/* The rewrite: n packed hashes -> n packed hashes at d_bits_out and their FP4 image (hvd_fp4_image_bytes(n)) at d_img, both
 * in the order perm. HVD_ERR_ARG, and nothing launched, unless perm is a permutation of 0..255. Does not synchronise. */
int hvd_dev_reorder_bits(const void* d_bits, int64_t n, const uint8_t* perm, void* d_bits_out, void* d_img);

/* The packed hashes of the first n rows of an FP4 image (the inverse of hvd_dev_expand_fp4), as the searches that are
 * handed images only derive them. Does not synchronise. */
int hvd_dev_pack_fp4(const void* d_img, int64_t n, void* d_bits);

#ifdef __cplusplus
}
#endif
#endif /* HVD_MI355X_BENCH_H */
