/*
 * hvd_mi355x.h -- C-ABI of libhvd_mi355x.so: the MI355X (gfx950) replacement for the
 * native module `hvdaccelerators.vpdq` that hydrus-video-deduplicator calls for its
 * perceptual-hash hot path. Paths below are relative to the reference tree.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns
 * HVD_OK (0) or a negative error code, never throws, and never keeps a caller
 * pointer past the call. hvd_last_error() gives the message for the last failure on
 * the calling thread. There is NO CPU fallback: without a usable gfx950 device
 * hvd_init() fails with HVD_ERR_NO_DEVICE and every compute entry point fails with
 * HVD_ERR_STATE.
 *
 * Layouts
 *   frame hash  : 32 bytes = 256 bits; DCT coefficient bit k = i*16+j is byte k>>3,
 *                 bit k&7 (little-endian image of PDQ's uint16 w[16];
 *                 db/DedupeDB.py:535-559, dedup.py:83).
 *   video hash  : concatenation of N>=0 frame hashes (dedup.py:77-86).
 *   hvd_pair    : one frame-level hit (i<j, Hamming distance).
 *   hvd_vmatch  : one video-level hit (a<b) with the vPDQ counters: q_hits = frames
 *                 of a that have >=1 frame of b within max_dist, t_hits the converse.
 *   hvd_group   : one group of duplicates (a connected component of a pair list) with its keeper.
 */
#ifndef HVD_MI355X_H
#define HVD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVD_OK 0
#define HVD_ERR_ARG (-1)       /* bad argument */
#define HVD_ERR_HIP (-2)       /* HIP runtime error */
#define HVD_ERR_OVERFLOW (-3)  /* output buffer too small; *out_count holds the required size */
#define HVD_ERR_NO_DEVICE (-4) /* no gfx950 device visible */
#define HVD_ERR_RCCL (-5)      /* RCCL error */
#define HVD_ERR_STATE (-6)     /* hvd_init() not called / comm not initialised */

#define HVD_BYTES_PER_PDQ_HASH 32 /* == vpdq.VpdqHash.bytesPerPdqHash, dedup.py:83 */
#define HVD_UNIQUE_ID_BYTES 128
#define HVD_ABI_VERSION 6 /* 6 (round 6): + hvd_group_rearm; later, still 6 (additions only, backward compatible): + hvd_dev_pdq_hash_frames_dihedral, hvd_pdq_hash_frames_dihedral_gray_u8 / _rgb24_u8, then + hvd_hasher_create_dihedral, hvd_hasher_finish_dihedral, then + hvd_dev_compact_kept_dihedral, then + hvd_align_scratch_bytes, hvd_dev_vpdq_align_videos, hvd_dev_kept_positions, hvd_vpdq_align_videos, then + hvd_hasher_create_autocrop, hvd_hasher_finish_autocrop, then + hvd_segments_scratch_bytes, hvd_dev_vpdq_align_segments, hvd_vpdq_align_segments, then + hvd_rates_scratch_bytes, hvd_dev_vpdq_align_rates, hvd_vpdq_align_rates, then + hvd_group_scratch_bytes, hvd_dev_group_edges, hvd_group_edges, then + hvd_pdq_crops_scratch_bytes, hvd_dev_pdq_hash_frames_crops, hvd_pdq_hash_frames_crops_gray_u8 / _rgb24_u8, then + hvd_dev_content_rects_detail, hvd_pdq_hash_frames_detail_gray_u8 / _rgb24_u8, hvd_hasher_create_autocrop_detail, then + hvd_dev_vpdq_frame_spread_cross, hvd_vpdq_frame_spread_cross, then + hvd_rate_segments_scratch_bytes, hvd_dev_vpdq_align_rate_segments, hvd_vpdq_align_rate_segments, then + hvd_dev_frame_runs, hvd_vpdq_frame_runs, then + hvd_dev_video_weights, hvd_dev_vpdq_match_videos_weighted, hvd_dev_vpdq_match_videos_cross_weighted, hvd_vpdq_match_videos_weighted, hvd_vpdq_match_videos_cross_weighted, then + hvd_cover_scratch_bytes, hvd_dev_vpdq_cover_videos, hvd_vpdq_cover_videos, then + hvd_signed_scratch_bytes, hvd_dev_vpdq_align_signed, hvd_vpdq_align_signed, then + hvd_loops_scratch_bytes, hvd_dev_vpdq_align_loops, hvd_vpdq_align_loops; 5 (round 5): + hvd_hasher_acquire_n, hvd_hasher_commit_n, hvd_group_abort, hvd_runtime_info, hvd_timer_mark, hvd_timer_between; 4 (round 4): + hvd_init_devices, hvd_context_count, hvd_set_context, hvd_get_context, hvd_group_exchange; 3 (round 3): + hvd_host_malloc/free, hvd_hasher_set_threads, hvd_dev_vpdq_emit_again, hvd_comm_abort, hvd_dct_matrix_libm */
/* All-pairs kernel the host entry points use: FP4-MFMA with a 128-bit first stage; which of its two forms runs
 * (survivors fetch their other half | second stage out of registers) is chosen per launch from a probe of the data. */
#define HVD_DEFAULT_VARIANT 13

typedef struct {
    uint32_t i, j, dist, pad;
} hvd_pair;

typedef struct {
    uint32_t a, b, q_hits, t_hits;
} hvd_vmatch;

/* One aligned video pair (hvd_vpdq_align_videos / hvd_dev_vpdq_align_videos), twelve 32-bit words. q_hits / t_hits:
 * the vPDQ counters of the pair (what hvd_vmatch holds). offset: the best offset d* of the target's timeline against the
 * query's (p_b = p_a + d*). band_votes: frame hits within slack of d*. q_aligned / t_aligned: frames of a / b with such a hit;
 * *_first / *_last: the smallest and largest position among them. A pair without a frame hit: every word after b is 0. A pair
 * the device entry cannot align (index out of range, positions that are not strictly increasing from >= 0, more than 2^20
 * histogram bins, no room in the scratch): offset = INT32_MIN, the other words after b 0. */
typedef struct hvd_valign {
    uint32_t a, b, q_hits, t_hits;
    int32_t offset;
    uint32_t band_votes, q_aligned, t_aligned;
    int32_t q_first, q_last, t_first, t_last;
} hvd_valign;
/* One video's coverage by its partners of a pair list (hvd_vpdq_cover_videos / hvd_dev_vpdq_cover_videos), four
 * 32-bit words. covered: the size of the union of the frame sets contributed to the video; sources: the number of list entries
 * that contributed; best_single: the largest single contribution; frames: the video's length as the kernel clamps it. */
typedef struct hvd_vcover {
    uint32_t covered, sources, best_single, frames;
} hvd_vcover;
/* Pairs of up to this many histogram bins (span of p_a + span of p_b + 1 + 2 slack) are aligned out of LDS alone. */
#define HVD_ALIGN_LDS_BINS 4096

/* One video pair aligned on up to HVD_ALIGN_MAX_SEGMENTS offsets (hvd_vpdq_align_segments / hvd_dev_vpdq_align_segments;
 * DESIGN 4.9): a highlight reel, a trailer cut from several scenes, a re-cut. A segment is eight 32-bit words, the words of
 * hvd_valign from offset on, computed on the frame hits that no earlier segment owns; a record is 72 words: a, b, q_hits, t_hits
 * (the vPDQ counters of the pair, as in hvd_valign), n_segments, q_covered / t_covered = the sums of q_aligned / t_aligned over
 * the segments, a reserved word (0), then the segments in the order they were found; unused slots are 0. A pair without a frame
 * hit: every word after b is 0. A pair the device entry cannot align (the conditions of hvd_valign): n_segments = 0,
 * seg[0].offset = INT32_MIN, the other words after b 0. */
#define HVD_ALIGN_MAX_SEGMENTS 8
typedef struct hvd_vsegment {
    int32_t offset;
    uint32_t band_votes, q_aligned, t_aligned;
    int32_t q_first, q_last, t_first, t_last;
} hvd_vsegment;
typedef struct hvd_vsegments {
    uint32_t a, b, q_hits, t_hits, n_segments, q_covered, t_covered, reserved;
    hvd_vsegment seg[HVD_ALIGN_MAX_SEGMENTS];
} hvd_vsegments;

/* One video pair aligned at the best of up to HVD_ALIGN_MAX_RATES listed rates (hvd_vpdq_align_rates / hvd_dev_vpdq_align_rates;
 * DESIGN 4.10): a sped-up or slowed-down copy or excerpt. Sixteen 32-bit words: the twelve of hvd_valign, in its order, then the
 * winning rate p_b = (rate_num / rate_den) p_a + offset / rate_den, its index in the caller's list and a reserved word (0).
 * offset is d* in the rate's scaled units (den p_b - num p_a), band_votes the frame hits within slack_r of it. A pair without a
 * frame hit, or with an empty video: every word after b is 0. A pair the device entry cannot align (the conditions of
 * hvd_valign; more than 2^20 bins at ANY listed rate; a broken rate list): offset = INT32_MIN, the other words after b 0. */
#define HVD_ALIGN_MAX_RATES 8
typedef struct hvd_vrate {
    uint32_t a, b, q_hits, t_hits;
    int32_t offset;
    uint32_t band_votes, q_aligned, t_aligned;
    int32_t q_first, q_last, t_first, t_last;
    uint32_t rate_num, rate_den, rate_index, reserved;
} hvd_vrate;

/* One video pair aligned on up to HVD_ALIGN_MAX_SEGMENTS lines, each at the best of up to HVD_ALIGN_MAX_RATES listed rates
 * (hvd_vpdq_align_rate_segments / hvd_dev_vpdq_align_rate_segments): a reel cut from several scenes whose pieces
 * were also sped up or slowed down. A segment (hvd_vrsegment) is twelve 32-bit words: the eight of hvd_vsegment, in its order,
 * then rate_num, rate_den, rate_index and a reserved word (0) as in hvd_vrate; offset and band_votes are in the rate's scaled
 * units, as in hvd_vrate. A record (hvd_vrsegments) is 104 words = 416 bytes, 16-byte aligned: the eight-word head of
 * hvd_vsegments, then the segments in the order they were found; unused slots are 0. A pair without a frame hit, or with an
 * empty video: every word after b is 0. A pair the device entry cannot align (the conditions of hvd_vrate): n_segments = 0,
 * seg[0].offset = INT32_MIN, the other words after b 0. */
typedef struct hvd_vrsegment {
    int32_t offset;
    uint32_t band_votes, q_aligned, t_aligned;
    int32_t q_first, q_last, t_first, t_last;
    uint32_t rate_num, rate_den, rate_index, reserved;
} hvd_vrsegment;
typedef struct hvd_vrsegments {
    uint32_t a, b, q_hits, t_hits, n_segments, q_covered, t_covered, reserved;
    hvd_vrsegment seg[HVD_ALIGN_MAX_SEGMENTS];
} hvd_vrsegments;

/* One video pair aligned on up to HVD_ALIGN_MAX_SEGMENTS lines, each at the best of up to HVD_ALIGN_MAX_RATES listed rates
 * whose numerators may be NEGATIVE (hvd_vpdq_align_signed / hvd_dev_vpdq_align_signed): a clip played backwards,
 * a "rewind" piece inside a reel. The layout is hvd_vrsegments' (416 bytes, 16-byte aligned; a segment is 48 bytes) with
 * rate_num a signed word: rate_num < 0 says b runs backwards against a in that segment. offset is d* in the rate's scaled
 * units (den p_b - num p_a), so c = offset / rate_den. The zero record and the INT32_MIN record are hvd_vrsegments'. */
typedef struct hvd_vssegment {
    int32_t offset;
    uint32_t band_votes, q_aligned, t_aligned;
    int32_t q_first, q_last, t_first, t_last;
    int32_t rate_num;
    uint32_t rate_den, rate_index, reserved;
} hvd_vssegment;
typedef struct hvd_vssegments {
    uint32_t a, b, q_hits, t_hits, n_segments, q_covered, t_covered, reserved;
    hvd_vssegment seg[HVD_ALIGN_MAX_SEGMENTS];
} hvd_vssegments;

/* One video pair aligned where a frame of b may serve MORE THAN ONCE (hvd_vpdq_align_loops / hvd_dev_vpdq_align_loops; DESIGN
 * 4.26): a looped clip, a ping-pong / boomerang loop, a short moment repeated. The layout is hvd_vssegments' (416 bytes, 16-byte
 * aligned) with `rounds` in the place of the reserved word. seg[0 .. n_segments - 1] are the first min(rounds, 8) rounds in the
 * order found; a round past the eighth writes no segment and adds to rounds, q_covered and t_covered only. q_covered: the frames
 * of a in any round (the rounds' frames of a are disjoint: the sum of q_aligned over ALL rounds); t_covered: the DISTINCT frames
 * of b in any round, so t_covered <= the sum of t_aligned. The zero record and the INT32_MIN record are hvd_vssegments'. */
#define HVD_ALIGN_MAX_ROUNDS 64
typedef struct hvd_vloops {
    uint32_t a, b, q_hits, t_hits, n_segments, q_covered, t_covered, rounds;
    hvd_vssegment seg[HVD_ALIGN_MAX_SEGMENTS];
} hvd_vloops;

/* One duplicate group (hvd_group_edges / hvd_dev_group_edges): a connected component of size >= 2 of the graph
 * whose edges are the records of a search. root: the smallest member, which is also the label of every member; size: members;
 * edges: input records that are edges inside the group (a repeated record counts each time); keeper: the member with the largest
 * score, ties to the smaller index -- Hydrus' "king". The group is complete (every member pairs with every other) iff
 * edges == size (size - 1) / 2, given that the list holds each pair once, as the searches emit them.
 * The keeper-first grouping (hvd_keeper_groups / hvd_dev_keeper_groups) writes the same record with root = keeper =
 * the keeper's index, which is then the label of every member (keeper_of), size = 1 + its members, and edges counted inside the
 * group the same way. */
typedef struct hvd_group {
    uint32_t root, size, edges, keeper;
} hvd_group;
#define HVD_EDGES_ALL 0    /* every record is an edge (hvd_pair, or any 16-byte record with the two nodes in words 0 and 1) */
#define HVD_EDGES_VMATCH 1 /* hvd_vmatch records; a record is an edge iff the reference's pair predicate holds */

/* ------------------------------------------------------------ lifecycle -- */

int hvd_abi_version(void);
/* Number of visible HIP devices (0 and HVD_OK when there is none). */
int hvd_device_count(int* out_n);
/* Bind this process to one GPU, create the library stream, upload the 16x64 DCT matrix. Idempotent for the same
 * device. With HVD_DEVICES=0,1,2,... in the environment (the list must start with `device`) this is
 * hvd_init_devices() on that list: every binding of this library that calls hvd_init -- the vpdq-shaped Python
 * surface, the search, the VpTreeManager facade, the SQLite adapter -- then uses all listed GPUs, no launcher. */
int hvd_init(int device);
/* Bind this process to a GROUP of GPUs: one context per listed device (its own stream, scratch pool, select/context
 * words, communicator). The reference is ONE process (entrypoint.py:235 -> dedup.py:213); a group is how that one
 * process uses 8 MI355X. The host-buffer entry points (hvd_pdq_hash_frames_*, hvd_allpairs_hamming256,
 * hvd_vpdq_match_videos[_cross]) then shard by themselves -- frames in contiguous ranges; the hash DB replicated on
 * every device, tile (rb, cb) of the pair matrix on context (rb + cb) % n, one host thread per context, candidates /
 * video keys exchanged with RCCL all-gathers over xGMI (ncclCommInitAll: one communicator per device, one process) --
 * and return what a single device returns. Everything else works on the calling thread's CURRENT context
 * (hvd_set_context; context 0 by default): a caller that wants to drive the device-resident API on every GPU itself
 * runs one thread per context with rank = context index, world = group size (hvd_amd.pipeline, bench.py
 * --single-process). A device may be listed twice (two contexts, two streams on one GPU: a test configuration; RCCL
 * refuses duplicate devices, so such a group exchanges through host memory -- hvd_group_exchange() == 2). */
int hvd_init_devices(const int* devices, int n_devices);
int hvd_context_count(int* out_n);  /* contexts of the group (1 after hvd_init, 0 before) */
int hvd_set_context(int index);     /* the calling thread's current context (and HIP device) from now on */
int hvd_get_context(void);
int hvd_group_exchange(void);       /* 0: no group (one context); 1: RCCL between the devices; 2: host memory */
/* A caller that drives the contexts from its own threads (one per context) and fails on ONE of them before that thread
 * reaches an exchange step calls this so that the others do not wait for it for ever: the host-memory barrier is broken
 * (waiters return HVD_ERR_RCCL), RCCL communicators of the group are aborted (ncclCommAbort releases a collective that is
 * already waiting on the device). The group has no exchange afterwards until hvd_group_rearm() -- or hvd_init_devices()
 * with the same device list, which calls it -- forms it again; the library does the same by itself when one context of a
 * host-buffer call fails hard (a failure every rank left in lock-step through an agreement step aborts nothing). */
int hvd_group_abort(void);
/* ABI 6: put a group back to work after an abandoned exchange -- re-arms the host-memory barrier and re-creates RCCL
 * communicators that were aborted (ncclCommInitAll over the group's devices). Call it when no thread is inside a group call
 * (hvd_amd.multigpu.run_on_contexts does, before it starts its threads). HVD_OK on a healthy group; HVD_ERR_RCCL if the
 * communicators cannot be re-created (the group then exchanges through host memory). */
int hvd_group_rearm(void);
/* What this process runs on, as one JSON object in buf (NUL-terminated, truncated to len): HIP runtime / driver versions,
 * RCCL version and the path of the librccl that is actually loaded, every visible device (name, PCI bus id, gcnArch, CUs,
 * memory) and the peer matrix of the group's devices (hipDeviceCanAccessPeer, link type and hop count from
 * hipExtGetLinkTypeAndHopCount: xGMI or PCIe). bench.py prints it with every measurement so that a multi-GPU run can be
 * read without access to the box. Callable before hvd_init. */
int hvd_runtime_info(char* buf, size_t len);
int hvd_shutdown(void);
/* Copies the calling thread's last error message (NUL-terminated) into buf. */
int hvd_last_error(char* buf, size_t len);
/* The DCT matrix the kernels use (16*64 floats): the table compiled into the library (csrc/dct_table.inc), which is
 * authoritative -- hashes do not depend on the host's libm. hvd_dct_matrix_libm() recomputes it on this host the way
 * upstream does (float scale * double cos, rounded once); the parity tests assert the two are bit-identical. */
int hvd_dct_matrix(float* out_16x64);
int hvd_dct_matrix_libm(float* out_16x64);

/* ------------------------------------------ host-buffer entry points ------ */
/* These are what the Python `vpdq`-shaped shim binds; each stages through HBM,
 * runs the HIP kernels on the library stream and copies results back. */

/* Replaces the per-frame work of vpdq.VideoHasher.hash_frame (vpdqpy/vpdqpy.py:118)
 * for a batch of pre-decoded frames. frames: n*h*w bytes (gray; luma is defined as
 * the RGB formula with R=G=B) or n*h*w*3 bytes packed RGB24 row-major, exactly what
 * bytes(frame.planes[0]) yields at vpdqpy.py:118. h,w >= 64. Outputs: n*32 hash
 * bytes and n int32 qualities (0..100). Quality filtering (>=31 kept,
 * db/DedupeDB.py:550-553) is the caller's job (VideoHasher.finish, vpdqpy.py:119). */
int hvd_pdq_hash_frames_gray_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes,
                                int32_t* out_quality);
int hvd_pdq_hash_frames_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes,
                                 int32_t* out_quality);
/* Dihedral PDQ: 8 hashes per frame in the order of the table in DESIGN (identity first), n*8*32 bytes:
 * identity, flip_h, flip_v, rot180, transpose, antitranspose, rot90_ccw, rot90_cw -- the PDQ hash of the frame's 64x64
 * luma mirrored / rotated that way, computed from the frame's one DCT (sign flips and a transpose), each variant
 * thresholded at its own median. Hash k of frame f is bytes [(8f+k)*32, (8f+k+1)*32); variant 0 is bit-identical to
 * hvd_pdq_hash_frames_*. One quality per frame (the same for all 8). Same geometry rules and device-group sharding as
 * hvd_pdq_hash_frames_*. Strict DCT mode only: HVD_ERR_STATE while hvd_set_pdq_dct_mode(1) is active. */
int hvd_pdq_hash_frames_dihedral_gray_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes8,
                                         int32_t* out_quality);
int hvd_pdq_hash_frames_dihedral_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, uint8_t* out_hashes8,
                                          int32_t* out_quality);
/* Content-rectangle PDQ on host buffers (the rule: hvd_dev_content_rects below): the n frames are the V videos of the CSR
 * offsets (int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n; checked); every frame is hashed inside its video's
 * rectangle. out_rects: int32[V][4] = {top, left, height, width}. A call whose rectangles are all the full frame runs the
 * plain kernels of hvd_pdq_hash_frames_*. Frames are staged in batches of whole videos (<= 1 GiB), so that a video's
 * rectangle always sees all its frames; a single video larger than that is HVD_ERR_ARG (it is not split). Under a device
 * group the call runs on the calling thread's current context alone (same bytes as on one context). Both DCT modes. */
int hvd_pdq_hash_frames_autocrop_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                         int black_level, int min_bright, uint8_t* out_hashes, int32_t* out_quality,
                                         int32_t* out_rects);
int hvd_pdq_hash_frames_autocrop_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                          int black_level, int min_bright, uint8_t* out_hashes, int32_t* out_quality,
                                          int32_t* out_rects);
/* Bar-colour content-rectangle PDQ on host buffers (the rule: hvd_dev_bar_colors below): hvd_pdq_hash_frames_autocrop_* with
 * "a pixel is content iff max_k |p_k - c_k| > bar_level" in place of "bright", c the bar colour of the frame's video. colors:
 * int32[V], c0 | c1 << 8 | c2 << 16 per video (gray: c0 alone; anything else is HVD_ERR_ARG), or NULL: every video's colour
 * is found from the corners of its frames. out_colors: int32[V], the colours that were used; out_rects as above. Staged and
 * batched as hvd_pdq_hash_frames_autocrop_* (whole videos per batch, same limits, same errors). Both DCT modes. */
int hvd_pdq_hash_frames_barcolor_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                         const int32_t* colors, int bar_level, int min_bright, uint8_t* out_hashes,
                                         int32_t* out_quality, int32_t* out_rects, int32_t* out_colors);
int hvd_pdq_hash_frames_barcolor_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                          const int32_t* colors, int bar_level, int min_bright, uint8_t* out_hashes,
                                          int32_t* out_quality, int32_t* out_rects, int32_t* out_colors);
/* Detail content-rectangle PDQ on host buffers (the rule: hvd_dev_content_rects_detail below): hvd_pdq_hash_frames_autocrop_*
 * with the detail rule as its rectangle step -- bars that are smooth (blurred, gradient, any colour) are left out. detail_level
 * 0..254, min_detail >= 1 (HVD_ERR_ARG otherwise). Staged and batched as hvd_pdq_hash_frames_autocrop_* (whole videos per batch,
 * same limits, same errors, the plain kernels when every rectangle of a batch is full). Both DCT modes. */
int hvd_pdq_hash_frames_detail_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                       int detail_level, int min_detail, uint8_t* out_hashes, int32_t* out_quality,
                                       int32_t* out_rects);
int hvd_pdq_hash_frames_detail_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int64_t* offsets, int64_t V,
                                        int detail_level, int min_detail, uint8_t* out_hashes, int32_t* out_quality,
                                        int32_t* out_rects);
/* Crop-ladder PDQ on host buffers (the rule: hvd_dev_pdq_hash_frames_crops below): every frame under the full frame and under
 * the K crops of the caller's list. out_hashes8: n*8*32 bytes in the dihedral layout (slot 0 the full frame, slots 1..K the
 * crops in list order, the rest zero); out_quality: int32[n], the full frame's; out_crop_quality: int32[n*8] per slot, or
 * NULL. Frames are staged in batches as hvd_pdq_hash_frames_dihedral_* stages them. Under a device group the call runs on
 * the calling thread's current context alone (same bytes as on one context). Both DCT modes. */
int hvd_pdq_hash_frames_crops_gray_u8(const uint8_t* frames, int64_t n, int h, int w, const int32_t* crops, int K,
                                      uint8_t* out_hashes8, int32_t* out_quality, int32_t* out_crop_quality);
int hvd_pdq_hash_frames_crops_rgb24_u8(const uint8_t* frames, int64_t n, int h, int w, const int32_t* crops, int K,
                                       uint8_t* out_hashes8, int32_t* out_quality, int32_t* out_crop_quality);

/* Replaces the O(visited nodes) stream of vpdq.matchHashBytes calls issued by the
 * VP-tree (db/vptree.py:29-31,737; dedup.py:445-502) with one brute-force pass:
 * all i<j with hamming(db[i],db[j]) <= max_dist and, when group != NULL,
 * group[i] != group[j]. out receives min(count,cap) records sorted by (i,j);
 * *out_count the true count (HVD_ERR_OVERFLOW if it exceeds cap). n < 2^32. */
int hvd_allpairs_hamming256(const uint8_t* db, int64_t n, const int32_t* group, int max_dist, hvd_pair* out,
                            int64_t cap, int64_t* out_count);

/* Replaces one vpdq.matchHash / vpdq.matchHashBytes call (vpdqpy/vpdqpy.py:56,
 * db/vptree.py:31): a, b are concatenated frame hashes (na, nb frames). Returns the
 * two vPDQ counters; the percentage policy lives in the host shim. */
int hvd_match_two(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb, int max_dist, int32_t* q_hits,
                  int32_t* t_hits);

/* Replaces HydrusVideoDeduplicator.find_potential_duplicates' tree search
 * (dedup.py:445-502) for a whole library: frames = all videos' frame hashes
 * concatenated, offsets[V+1] = CSR boundaries in frames. out receives every video
 * pair a<b with >=1 frame hit, sorted by (a,b). */
int hvd_vpdq_match_videos(const uint8_t* frames, const int64_t* offsets, int64_t V, int max_dist, hvd_vmatch* out,
                          int64_t cap, int64_t* out_count);

/* In how many OTHER videos does every frame occur? out_spread[f] (int32 per frame hash) = the number of videos
 * v != video(f) that hold at least one frame within max_dist of frame f: two matching frames of one video count once, frames of
 * f's own video never. A studio logo, a channel intro or an end card has a large spread; the common-frame filter
 * (hvd_dev_common_frames) deletes such frames before a search. frames / offsets / V as hvd_vpdq_match_videos; max_dist in
 * [0, 127]. Upload, FP4 image, frame -> video map, then hvd_dev_vpdq_frame_spread; under a device group it runs on the calling
 * thread's current context alone. */
int hvd_vpdq_frame_spread(const uint8_t* frames, const int64_t* offsets, int64_t V, int max_dist, int32_t* out_spread);

/* One keyframe per run of near-identical consecutive frames: the host-buffer form of hvd_dev_frame_runs, whose
 * comment holds the rule and what follows from it. frames / offsets / V as hvd_vpdq_match_videos; out_keep int32 per frame, 1 or
 * 0; out_run int32 per frame (may be NULL), the frames a kept frame stands for, 0 at a dropped one. max_dist in [0, 127] (0: a
 * dropped frame equals its anchor -- the lossless choice), max_run in [0, 2^20] (0 = no limit). A parameter out of range, a CSR
 * that does not start at 0 or decreases, a NULL buffer: HVD_ERR_ARG, returned BEFORE the library asks whether a device is
 * there. Then: upload of hashes and offsets, hvd_dev_frame_runs, copy back, one synchronisation; library-owned scratch; under
 * a device group it runs on the calling thread's current context alone. */
int hvd_vpdq_frame_runs(const uint8_t* frames, const int64_t* offsets, int64_t V, int max_dist, int max_run, int32_t* out_keep,
                        int32_t* out_run);

/* Query-set x target-set form of the same search: the steady-state workload after the first
 * run (new videos against the existing library; semantics of VpTreeManager.search_file,
 * db/vptree.py:865-902, for a batch of files). out: every (a = query video, b = target video)
 * with >=1 frame hit; q_hits counts frames of the query video, t_hits frames of the target.
 * ids_q / ids_t (both or neither): videos with equal ids are not compared with each other (a
 * query that is itself in the target set must not match itself). max_dist in [0,127]. */
int hvd_vpdq_match_videos_cross(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* ids_q,
                                const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* ids_t,
                                int max_dist, hvd_vmatch* out, int64_t cap, int64_t* out_count);

/* Duration-weighted video search: hvd_vpdq_match_videos where every frame carries an integer weight -- the `run`
 * of hvd_vpdq_frame_runs, the frames a kept frame stands for -- and a matched frame adds its weight to q_hits / t_hits where the
 * plain search adds 1. weights: int32 per frame hash, each at least 1. max_weight caps a weight at min(w, max_weight); 0 = no
 * cap, 1 = the plain search. out_totals (int64[V], may be NULL) receives the capped weight total of every video: the
 * denominators that take the place of the frame counts. Two identities: with max_weight 1 the records are those of
 * hvd_vpdq_match_videos on the same library; and on a library collapsed by the static-scene filter at max_dist 0 (a dropped
 * frame equals its anchor) with weights = run and no cap, the records are those of hvd_vpdq_match_videos on the library BEFORE
 * the collapse, and the totals are its frame counts. Records sorted by (a, b); cap / HVD_ERR_OVERFLOW as hvd_vpdq_match_videos;
 * max_dist in [0, 127]. HVD_ERR_ARG, returned BEFORE the library asks whether a device is there: a CSR that does not start at
 * 0 or decreases, a NULL frames or weights array, a weight below 1, max_weight < 0, a video whose capped total exceeds
 * 2^32 - 1 (the counters are uint32). Under a device group it runs on the calling thread's current context alone. */
int hvd_vpdq_match_videos_weighted(const uint8_t* frames, const int64_t* offsets, int64_t V, const int32_t* weights, int max_weight,
                                   int max_dist, hvd_vmatch* out, int64_t cap, int64_t* out_count, int64_t* out_totals);
/* Query-set x target-set form, as hvd_vpdq_match_videos_cross: q_hits sums weights_q over the matched query frames, t_hits
 * weights_t over the matched target frames; out_totals_q int64[VQ] / out_totals_t int64[VT] (each may be NULL). The same
 * refusals, on either side, before a device is asked for; on the calling thread's current context alone. */
int hvd_vpdq_match_videos_cross_weighted(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* ids_q,
                                         const int32_t* weights_q, const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT,
                                         const int32_t* ids_t, const int32_t* weights_t, int max_weight, int max_dist,
                                         hvd_vmatch* out, int64_t cap, int64_t* out_count, int64_t* out_totals_q,
                                         int64_t* out_totals_t);

/* New files against the library: the rectangular spread. Q is a new batch (frames_q / offsets_q / VQ), T the
 * library (frames_t / offsets_t / VT), both as hvd_vpdq_match_videos takes them; their video sets are disjoint.
 * out_spread_q[f] (int32 per frame of Q) = the number of videos of T that hold at least one frame within max_dist of f;
 * out_spread_t[g] (int32 per frame of T) = the number of videos of Q that hold at least one frame within max_dist of g. Two
 * matching frames of one video count once; frames of Q are never compared with frames of Q, nor T's with T's. With the
 * symmetric spreads of Q and of T alone (hvd_vpdq_frame_spread) they add up to the spread of the union T || Q. max_dist in
 * [0, 127]. Both sides are uploaded to the slots hvd_vpdq_match_videos_cross uses, then hvd_dev_vpdq_frame_spread_cross; under
 * a device group it runs on the calling thread's current context alone. */
int hvd_vpdq_frame_spread_cross(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const uint8_t* frames_t,
                                const int64_t* offsets_t, int64_t VT, int max_dist, int32_t* out_spread_q, int32_t* out_spread_t);

/* Time alignment of listed video pairs: is video a an excerpt of video b (or b of a), and where. The rule,
 * integers only. Position p(f) of a frame: positions[f] if given (int32 per frame of the library; non-negative, strictly
 * increasing inside a video, below 2^20), else the frame's index inside its video. H = {(i, j) : hamming(A_i, B_j) <= max_dist}
 * over the frames of a and b; delta(i, j) = p_b(j) - p_a(i); votes[d] = |{(i, j) in H : delta = d}|; S(d) = the sum of
 * votes[d - slack .. d + slack]. Best offset d*: the largest S(d), ties by the larger votes[d], then the smaller |d|, then the
 * smaller d. A frame i of a is aligned iff some (i, j) in H has |delta(i, j) - d*| <= slack; likewise the frames of b.
 * pairs: uint32[M][2] = (a = video of the query library, b = video of the target library); the self form passes one library
 * twice. out: M hvd_valign records in the order of the pair list. max_dist in [0, 127], slack in [0, 16].
 * This host-buffer form checks the offsets (as hvd_vpdq_match_videos), the positions, the pair indices and the 2^20-bin limit of
 * every pair (HVD_ERR_ARG), stages, runs the kernels and copies the records back. Under a device group it runs on the calling
 * thread's current context alone. positions_q / positions_t may be NULL. */
int hvd_vpdq_align_videos(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                          const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                          const uint32_t* pairs, int64_t M, int max_dist, int slack, hvd_valign* out);

/* Coverage of a video by SEVERAL others: a compilation of clips that are all in the library, a film next to its parts, a stream
 * archive next to its per-segment uploads. hvd_vpdq_align_videos judges one pair at a time; here the aligned
 * frames of every pair a video takes part in are united. The rule, integers only. One library (frames / offsets / positions
 * as above), pairs: uint32[M][2] = (a, b), both videos of that library; max_dist in [0, 127], slack in [0, 16], min_aligned >= 1.
 * Per pair: out_align[p] is the hvd_valign record of hvd_vpdq_align_videos on the same operands, word for word. Let on_a / on_b
 * be the pair's aligned frame sets -- frame indices inside the video, the sets whose sizes are q_aligned / t_aligned. The pair
 * contributes on_a to video a iff a != b, the record's offset is not INT32_MIN and |on_a| >= min_aligned; independently it
 * contributes on_b to video b iff a != b, the offset is not INT32_MIN and |on_b| >= min_aligned.
 * Per video v: out_cover[v] (hvd_vcover) = covered: the size of the union of the frame sets contributed to v; sources: the
 * number of list entries that contributed to v; best_single: the largest single contribution; frames: the length of v.
 * Five consequences: (a) best_single <= covered <= min(frames, the sum of the contributions); (b) sources == 0 iff covered == 0;
 * (c) listing a pair twice, or as (a, b) and as (b, a), changes sources and nothing else -- callers pass each unordered pair
 * once, as the records of hvd_vpdq_match_videos do; (d) a video that no pair names has the record (0, 0, 0, frames); (e) the
 * alignment records do not depend on min_aligned. covered > best_single says that no single partner explains the video.
 * This host-buffer form checks what hvd_vpdq_align_videos checks, and min_aligned, before it asks whether a device is there
 * (HVD_ERR_ARG with or without one); then it stages, runs and copies both outputs back. M == 0 is legal and gives the records
 * of (d). out_align: M records (may be NULL when M == 0); out_cover: V records. positions may be NULL. */
int hvd_vpdq_cover_videos(const uint8_t* frames, const int64_t* offsets, int64_t V, const int32_t* positions, const uint32_t* pairs,
                          int64_t M, int max_dist, int slack, int min_aligned, hvd_valign* out_align, hvd_vcover* out_cover);

/* Multi-segment time alignment of listed video pairs: a short video that is SEVERAL pieces of a longer one. The
 * notation and the operands of hvd_vpdq_align_videos apply (H, delta, votes, S, slack, the tie order). The rule, integers only,
 * one answer per pair, with K = max_segments in [1, HVD_ALIGN_MAX_SEGMENTS] and min_band_votes >= 1:
 *   taken_a = taken_b = {}
 *   for r = 1..K:
 *     H_r = {(i, j) in H : i not in taken_a and j not in taken_b};  if H_r is empty: stop
 *     votes, S, d*_r: the rule and tie order of hvd_vpdq_align_videos, on H_r;  if S(d*_r) < min_band_votes: stop
 *     aligned_a = {i : some (i, j) in H_r has |delta - d*_r| <= slack};  aligned_b likewise
 *     segment r = (offset d*_r, band_votes S(d*_r), q_aligned, t_aligned, q_first, q_last, t_first, t_last)
 *     taken_a |= aligned_a;  taken_b |= aligned_b
 * Three consequences: (a) segment 1 is, word for word, the hvd_valign record of the pair (offset .. t_last; q_hits / t_hits are
 * the same too); (b) band_votes never increases from one segment to the next, because H_{r+1} is a subset of H_r; (c) the
 * aligned sets of the segments are disjoint, so q_covered = the sum of q_aligned and t_covered = the sum of t_aligned. Once
 * every frame of a or of b is taken, H_r is empty: a full copy is one segment.
 * out: M hvd_vsegments records in the order of the pair list. This host-buffer form validates what hvd_vpdq_align_videos
 * validates and max_segments / min_band_votes (HVD_ERR_ARG), stages, runs the kernels and copies the records back; under a
 * device group it runs on the calling thread's current context alone. */
int hvd_vpdq_align_segments(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                            const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                            const uint32_t* pairs, int64_t M, int max_dist, int slack, int max_segments, int min_band_votes,
                            hvd_vsegments* out);

/* Rate-aware time alignment of listed video pairs: a copy or an excerpt that was sped up or slowed down. The
 * notation and the operands of hvd_vpdq_align_videos apply (positions p, the hit set H, max_dist, slack, the tie order). One
 * input is new: rates, int32[n_rates][2] = (num_r, den_r) with 1 <= n_rates <= HVD_ALIGN_MAX_RATES, 1 <= num, den <= 8,
 * gcd(num, den) = 1, pairwise distinct. Rate (num, den) models p_b = (num / den) p_a + c: video b runs through the content
 * num / den times as slowly as a (a is the sped-up one when num > den). The rule, integers only, one answer per pair:
 *   for each rate r, in list order:
 *     delta_r(i, j) = den p_b(j) - num p_a(i)  for (i, j) in H
 *     slack_r = slack max(num, den)   (the rounding of a resampled timeline alone spreads delta_r over +-den / 2; at (1, 1)
 *                                      slack_r = slack)
 *     votes_r[d] = |{(i, j) in H : delta_r = d}|;  S_r(d) = the sum of votes_r[d - slack_r .. d + slack_r];
 *     d*_r: the largest S_r(d), ties by the larger votes_r[d], then the smaller |d|, then the smaller d
 *   the winning rate w: the largest S_r(d*_r), ties to the earlier rate of the list
 *   a frame i of a is aligned iff some (i, j) in H has |delta_w(i, j) - d*_w| <= slack_w; likewise the frames of b
 * The record (hvd_vrate): a, b, q_hits, t_hits as in hvd_valign; offset = d*_w in the scaled units, so c = offset / rate_den;
 * band_votes = S_w(d*_w); q_aligned .. t_last as in hvd_valign, on the aligned frames above; rate_num, rate_den, rate_index = w
 * (0-based); a reserved zero word. Special cases: no hit, or an empty video -> all zero apart from a and b. offset = INT32_MIN
 * and every other word after b zero: under the conditions of hvd_valign, and when ANY listed rate needs more than 2^20 bins,
 * bins_r = num span_a + den span_b + 1 + 2 slack_r (span: last position - first position of the video). The device entry gives
 * the INT32_MIN record to every pair when the rate list is broken; this host entry rejects a broken list, and everything else
 * named here, with HVD_ERR_ARG -- and does so before it touches the device.
 * Four consequences: (a) with rates = [(1, 1)], words 0-11 are the pair's hvd_valign record, word for word, and words 12-15 are
 * 1, 1, 0, 0; (b) with (1, 1) anywhere in the list, band_votes >= the pair's hvd_valign.band_votes; (c) q_hits and t_hits do not
 * depend on the list; (d) reordering the list changes the record (apart from rate_index) only when two rates tie on S.
 * S is compared raw across rates although a window of slack_r units is not equally wide in time at every rate: on smooth content
 * (neighbouring frames within max_dist of each other) a neighbouring listed rate may win. rate_num / rate_den is the
 * best-fitting LISTED rate; what detection rests on is the coverage (q_aligned / t_aligned).
 * out: M hvd_vrate records in the order of the pair list. Under a device group it runs on the calling thread's current context
 * alone. */
int hvd_vpdq_align_rates(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                         const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                         const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                         hvd_vrate* out);

/* Rate-aware multi-segment time alignment of listed video pairs: a short video that is SEVERAL pieces of a longer one, each
 * sped up or slowed down by a listed rate. The notation and the operands are those of hvd_vpdq_align_videos (H,
 * votes, S, the tie order), hvd_vpdq_align_segments (K = max_segments in [1, HVD_ALIGN_MAX_SEGMENTS], min_band_votes >= 1) and
 * hvd_vpdq_align_rates (the list, delta_r, slack_r). The rule, integers only, one answer per pair:
 *   taken_a = taken_b = {}
 *   for s = 1..K:
 *     H_s = {(i, j) in H : i not in taken_a and j not in taken_b};  if H_s is empty: stop
 *     for each rate r = (num, den), in list order:
 *       delta_r(i, j) = den p_b(j) - num p_a(i)  for (i, j) in H_s;  slack_r = slack max(num, den)
 *       votes_r, S_r, d*_r: the rule and tie order of hvd_vpdq_align_videos on H_s, delta_r, slack_r
 *     w = the rate of the largest S_r(d*_r), ties to the earlier rate of the list;  if S_w(d*_w) < min_band_votes: stop
 *     aligned_a = {i : some (i, j) in H_s has |delta_w - d*_w| <= slack_w};  aligned_b likewise
 *     segment s = (offset d*_w, band_votes S_w(d*_w), q_aligned, t_aligned, q_first, q_last, t_first, t_last,
 *                  rate_num, rate_den, rate_index = w (0-based), 0)
 *     taken_a |= aligned_a;  taken_b |= aligned_b;  if every frame of a, or every frame of b, is taken: stop
 * Rate-list validity, the 2^20-bin limit at ANY listed rate and the INT32_MIN conditions are hvd_vpdq_align_rates'; max_segments
 * and min_band_votes are hvd_vpdq_align_segments'. Four consequences: (a) with rates = [(1, 1)], the head and words 0-7 of every
 * segment are the pair's hvd_vsegments record, word for word, and words 8-11 of a used segment are 1, 1, 0, 0; (b) with
 * max_segments = 1 and min_band_votes = 1, the head's a .. t_hits and seg[0] are the pair's hvd_vrate record (its words 0-3 and
 * 4-15); (c) q_hits and t_hits depend on neither the list nor K; (d) band_votes never increases from one segment to the next (H_s
 * shrinks, so no S_r(d) grows), and a segment's q_aligned and t_aligned never exceed its band_votes (every aligned frame has a
 * hit in the band). S is compared raw across rates, as in hvd_vpdq_align_rates: a band at a neighbouring listed rate may claim
 * frames before the true one is looked at.
 * out: M hvd_vrsegments records in the order of the pair list. This host-buffer form rejects a broken list, max_segments /
 * min_band_votes out of range and everything hvd_vpdq_align_rates rejects with HVD_ERR_ARG, before it touches the device; under
 * a device group it runs on the calling thread's current context alone. */
int hvd_vpdq_align_rate_segments(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                                 const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                                 const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                                 int max_segments, int min_band_votes, hvd_vrsegments* out);

/* Time alignment with negative rates: a clip played BACKWARDS, a reversed piece inside a reel. The rule is
 * hvd_vpdq_align_rate_segments' rule, word for word, with signed numerators:
 *   rates: int32[n_rates][2] = (num_r, den_r), 1 <= n_rates <= HVD_ALIGN_MAX_RATES, 1 <= |num| <= 8, 1 <= den <= 8,
 *   gcd(|num|, den) = 1, the entries pairwise distinct AS SIGNED PAIRS: (1, 1) and (-1, 1) may both be listed.
 *   (num, den) models p_b = (num / den) p_a + c; num < 0: b runs backwards against a.
 *   per rate: delta_r = den p_b - num p_a;  slack_r = slack max(|num|, den);
 *             bins_r = |num| span_a + den span_b + 1 + 2 slack_r;
 *             the smallest delta is den p_b0 - num p_a1 for num > 0 and den p_b0 - num p_a0 for num < 0.
 * The rounds, the taken sets on both sides, min_band_votes, the tie order (larger S, larger votes[d], smaller |d|, smaller d,
 * the earlier rate), the 2^20-bin limit at ANY listed rate, the INT32_MIN record and the zero record are unchanged. A segment's
 * offset is d*_w in the scaled units of its rate, c = offset / rate_den; rate_num is stored signed.
 * Four consequences: (a) with every num > 0 the records are hvd_vpdq_align_rate_segments' records word for word, and with
 * max_segments = 1 seg[0] is then hvd_vpdq_align_rates' record; (b) q_hits and t_hits do not depend on the list; (c) ties go
 * forward by list order: with (1, 1) listed before (-1, 1), a pair the two tie on -- one hit, a static pair -- is reported
 * forward (50 against 80 copies of one frame: rate (1, 1), offset 1, band_votes 150 at slack 1), and listing (-1, 1) first
 * reports it as (-1, 1), offset 50, band_votes 150; (d) reflection: reversing a's frame order (index positions) and negating
 * every num gives, for a pair without a tie on |d|, the same band_votes, q_aligned, t_aligned, t_first and t_last per
 * segment, offset' = offset + num (n_a - 1) with num the original segment's, and q_first' = n_a - 1 - q_last.
 * out: M hvd_vssegments records in the order of the pair list. This host-buffer form rejects with HVD_ERR_ARG, before it asks
 * for a device, everything hvd_vpdq_align_rate_segments rejects and a list that is not sound as a signed list. The other
 * alignment entries keep rejecting a negative num. */
int hvd_vpdq_align_signed(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                          const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                          const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                          int max_segments, int min_band_votes, hvd_vssegments* out);

/* Time alignment where a frame of the source serves more than once: looped clips and boomerangs. The rule is
 * hvd_vpdq_align_signed's rule with two changes: the taken set of b is dropped, and the rounds may go on past the eight stored
 * segments. rates: a signed list exactly as hvd_vpdq_align_signed takes it. max_rounds in [1, HVD_ALIGN_MAX_ROUNDS],
 * min_band_votes >= 1. With taken_a = {} and seen_b = {}, for r = 1 .. max_rounds:
 *   H_r = the hits of H whose frame OF A is not in taken_a; stop if it is empty;
 *   votes, S, d*, the winning rate and the tie order as hvd_vpdq_align_signed's on H_r; stop if S < min_band_votes;
 *   the frames of a and of b with a hit of H_r within slack_r of d* are round r: those of a join taken_a, those of b join
 *   seen_b, which is never consulted as a filter;
 *   stop when taken_a holds every frame of a.
 * b's frames may serve any number of rounds, a's serve one: the loop is the A side, and the caller chooses the orientation.
 * The record is hvd_vloops (above): the first eight rounds as segments, then counts only. Five consequences: (1) seg[0], q_hits
 * and t_hits are hvd_vpdq_align_signed's for the same arguments, word for word; (2) band_votes never increases from one round to
 * the next (H_{r+1} is a subset of H_r); (3) q_covered is the sum of q_aligned over the stored segments whenever rounds <= 8;
 * (4) a record with rounds = 1 is hvd_vpdq_align_signed's record at max_segments = 1, the `rounds` word aside; (5) on a pair
 * where no frame of b lies in two rounds and rounds <= 8, the segments are those of the signed rule WITH ITS b-FILTER OFF --
 * not an identity with hvd_vpdq_align_signed itself, whose b-filter changes H_r even there.
 * out: M hvd_vloops records in the order of the pair list. This host-buffer form rejects with HVD_ERR_ARG, before it asks for a
 * device, a list that is not sound as a signed list, max_rounds outside [1, HVD_ALIGN_MAX_ROUNDS], min_band_votes < 1 and
 * everything hvd_vpdq_align_signed rejects in the other arguments. */
int hvd_vpdq_align_loops(const uint8_t* frames_q, const int64_t* offsets_q, int64_t VQ, const int32_t* positions_q,
                         const uint8_t* frames_t, const int64_t* offsets_t, int64_t VT, const int32_t* positions_t,
                         const uint32_t* pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                         int max_rounds, int min_band_votes, hvd_vloops* out);

/* Duplicate groups with a keeper: the connected components of a pair list. The rule, integers only, one answer per
 * input. V nodes, 1 <= V < 2^31. E records of 16 bytes, E < 2^32, words 0 and 1 the two node indices u, v (hvd_pair and
 * hvd_vmatch have this shape). kind:
 *   HVD_EDGES_ALL     every record is an edge; either orientation and repeated records are allowed.
 *   HVD_EDGES_VMATCH  the record is an hvd_vmatch and is an edge iff the reference's pair predicate holds (dedup.py:445-502).
 *                     With na = lengths[u], nb = lengths[v] (int64 per node) and T = threshold in [1, 100]:
 *                       qa = na > 0 and 100 q_hits >= T na;   tb = nb > 0 and 100 t_hits >= T nb
 *                     policy_is_min != 0 (policy "min"): edge iff qa and tb; else ("max", "query", "target"): iff qa or tb. All of
 *                     it in 64-bit integers. The reference divides in floating point and truncates: floor(100 q / n) >= T
 *                     <=> 100 q >= T n, so these are exactly its pairs.
 * A record with u >= V, v >= V or u == v is no edge: the device entry ignores it, this host entry rejects it (HVD_ERR_ARG).
 * score: uint32 per node, or NULL: every score 0.
 * out_label: int32[V]; label[v] = the smallest index in v's component (label[v] == v for a node on its own).
 * out_groups: one hvd_group per component of size >= 2, sorted by root ascending; min(count, cap) are written. *out_count: the
 * true number of groups; HVD_ERR_OVERFLOW if it exceeds cap (the labels and the first cap groups are valid then). There are at
 * most min(V / 2, E) groups.
 * Nothing in the result depends on the order of the records or on scheduling.
 * This host-buffer form validates everything -- V and E in range, kind, T, lengths with kind 1, every record -- before it asks
 * for a device (HVD_ERR_ARG with or without one), then uploads, runs the kernels and downloads. Under a device group it runs on
 * the calling thread's current context alone. */
int hvd_group_edges(const void* records, int64_t E, int kind, const int64_t* lengths, int threshold, int policy_is_min, int64_t V,
                    const uint32_t* score, int32_t* out_label, hvd_group* out_groups, int64_t cap, int64_t* out_count);

/* Keeper-first duplicate groups: every member of a group is a direct match of the group's keeper. The components
 * of hvd_group_edges are single linkage: a chain A~B~C without A~C is one group, whose keeper may be A, no duplicate of C. This
 * grouping is for a caller that acts on its groups. The rule, integers only, one answer per input; V, the records, kind,
 * lengths, threshold, policy_is_min and score mean what they mean for hvd_group_edges, and the same records are edges:
 *   priority   key(v) = score[v] << 32 | (2^32 - 1 - v); larger is better: the larger score, then the smaller index.
 *   adjacent   u and v, iff some record is an edge between them; orientation and repeats do not matter.
 *   keeper     v, iff no adjacent node of higher priority is a keeper (well founded from the highest priority down: the
 *              lexicographically first maximal independent set). A node without edges is a keeper.
 *   member     every other node; it has an adjacent keeper by definition. keeper_of[v] = its adjacent keeper of highest
 *              priority; keeper_of[v] = v for a keeper.
 *   group      one per keeper with at least one member: size = 1 + its members; edges = the records that are edges with both
 *              ends in the group, each repeat counted; complete iff edges == size (size - 1) / 2.
 * Equivalently: walk the nodes in descending priority; a node nobody has claimed becomes a keeper and claims every unclaimed
 * neighbour. What follows:
 *   (a) every member has a record that is an edge to its keeper;
 *   (b) no two keepers are adjacent: once the members are deleted, no pair of the input remains among the kept nodes;
 *   (c) nothing in the result depends on the order of the records or on scheduling -- nor does *out_rounds.
 * out_keeper: int32[V], keeper_of. out_groups: one hvd_group per group with root = keeper = the keeper's index, sorted by keeper
 * ascending; min(count, cap) are written. *out_count: the true number of groups; HVD_ERR_OVERFLOW if it exceeds cap (keeper_of
 * and the first cap groups are valid then). There are at most min(V / 2, E) groups. out_rounds: NULL, or receives the number of
 * rounds the device took (hvd_dev_keeper_groups), at least 1.
 * This host-buffer form validates everything hvd_group_edges validates, every record included, before it asks for a device
 * (HVD_ERR_ARG with or without one, nothing written), then uploads, runs the kernels and downloads. */
int hvd_keeper_groups(const void* records, int64_t E, int kind, const int64_t* lengths, int threshold, int policy_is_min, int64_t V,
                      const uint32_t* score, int32_t* out_keeper, hvd_group* out_groups, int64_t cap, int64_t* out_count,
                      int64_t* out_rounds);

/* ------------------------------------------------ streaming frame hasher -- */
/* The native side of vpdq.VideoHasher (vpdqpy/vpdqpy.py:113-119): frames are pushed one at a
 * time (as a decoder yields them), staged in a ring of pinned batch slots, and each batch is
 * uploaded, hashed and downloaded on its own HIP stream, so PCIe transfer overlaps the kernels.
 * hvd_hasher_push blocks only when every slot is still in flight (back-pressure,
 * vpdqpy.py:115-117). One hasher per decoder thread; not thread-safe per handle. */
typedef struct hvd_hasher hvd_hasher;
int hvd_hasher_create(int width, int height, int channels, int64_t batch_frames, hvd_hasher** out);
int hvd_hasher_push(hvd_hasher* hs, const uint8_t* frame);
/* Host threads that share the copy of one frame inside hvd_hasher_push (the caller included; <= 0: library default = a quarter of the usable CPUs, between 2 and 8;
 * at most 8): what VideoHasher's num_threads (vpdqpy/vpdqpy.py:113) means on this path. One thread moves ~20 GB/s into
 * the pinned ring, the PCIe link behind it takes ~57. Frames below ~200 KB are copied by the caller alone. */
int hvd_hasher_set_threads(hvd_hasher* hs, int n);
/* Zero-copy feed: *out_frame is where the next frame (width*height*channels bytes) belongs inside the pinned
 * batch slot, so a decoder can reformat straight into it instead of handing over a copy (the reference copies
 * every frame into a Python bytes object, vpdqpy/vpdqpy.py:118); hvd_hasher_commit() makes it count.
 * acquire blocks like push; push == acquire + memcpy + commit. */
int hvd_hasher_acquire(hvd_hasher* hs, uint8_t** out_frame);
int hvd_hasher_commit(hvd_hasher* hs);
/* The same for a run of frames: *out_frames is where the next frames belong, back to back, *out_n (1 <= *out_n <= want)
 * how many fit there (what is left of the current batch: batches start small and grow per video); hvd_hasher_commit_n(n) makes the first n count
 * (0 <= n <= *out_n). One FFI round trip per run instead of two per frame: what a decoder of small frames wants. */
int hvd_hasher_acquire_n(hvd_hasher* hs, int64_t want, uint8_t** out_frames, int64_t* out_n);
int hvd_hasher_commit_n(hvd_hasher* hs, int64_t n);
int hvd_hasher_pending(hvd_hasher* hs, int64_t* out_frames);
/* All hashes (n*32 bytes) and qualities in push order; the hasher is reusable afterwards. */
int hvd_hasher_finish(hvd_hasher* hs, uint8_t* out_hashes, int32_t* out_quality, int64_t cap, int64_t* out_n);
int hvd_hasher_destroy(hvd_hasher* hs);
/* Dihedral streaming hasher: the same ring, every batch hashed by the dihedral kernel (the 8 hashes of
 * hvd_dev_pdq_hash_frames_dihedral per frame). push / acquire[_n] / commit[_n] / pending / set_threads / destroy work on
 * it unchanged; its results come from hvd_hasher_finish_dihedral: n*8*32 bytes (a frame's 8 variants back to back, the
 * order of hvd_dev_pdq_hash_frames_dihedral) and n qualities in push order. hvd_hasher_finish on a dihedral hasher and
 * hvd_hasher_finish_dihedral on a plain one return HVD_ERR_STATE. Strict DCT mode only: create returns HVD_ERR_STATE
 * in the fma mode, and a call that submits a batch (push, commit, finish) after a switch to fma returns HVD_ERR_STATE;
 * the batch stays staged and is submitted by the next call. */
int hvd_hasher_create_dihedral(int width, int height, int channels, int64_t batch_frames, hvd_hasher** out);
int hvd_hasher_finish_dihedral(hvd_hasher* hs, uint8_t* out_hashes8, int32_t* out_quality, int64_t cap, int64_t* out_n);
/* Autocrop streaming hasher (content-rectangle PDQ, see hvd_dev_content_rects): for any sequence of frames, out_hashes,
 * out_quality and out_rect ({top, left, height, width}) of hvd_hasher_finish_autocrop are what
 * hvd_pdq_hash_frames_autocrop_gray_u8 / _rgb24_u8 return for the same frames as one video (V = 1) with the same
 * black_level (0..254) / min_bright (>= 1; else HVD_ERR_ARG) -- byte for byte, in push order, in the DCT mode active at
 * finish. The rectangle is known only after the last frame, so the video's frames stay in device memory until finish: a
 * batch is uploaded straight into a store of device blocks, the rectangle is folded batch by batch behind the uploads,
 * and finish hashes every retained frame under it. push / acquire[_n] / commit[_n] / pending / set_threads / destroy
 * work on it unchanged. max_retained_bytes (<= 0: the library default, 8 GiB) bounds the frames one video keeps: the
 * push / acquire[_n] of the frame that would pass it returns HVD_ERR_OVERFLOW before the frame is taken (acquire_n hands
 * out at most what is left), the frames already taken stay and finish returns their result. A block that cannot be
 * allocated is HVD_ERR_HIP with the same guarantee (room for a batch is reserved when the batch begins). No frames:
 * out_n = 0 and the full-frame rectangle. hvd_hasher_finish / _finish_dihedral on an autocrop hasher and
 * hvd_hasher_finish_autocrop on the other kinds return HVD_ERR_STATE. What is kept after finish / destroy: the slot set
 * (parked per geometry and kind, as for the other kinds; no slot-sized device frame buffers here) and the store's first
 * block, at most 6 batches of frames -- what a plain hasher's slots hold in device frame buffers; every other block is
 * freed at finish, and hvd_shutdown frees everything. */
int hvd_hasher_create_autocrop(int width, int height, int channels, int64_t batch_frames, int black_level, int min_bright,
                               int64_t max_retained_bytes, hvd_hasher** out);
int hvd_hasher_finish_autocrop(hvd_hasher* hs, uint8_t* out_hashes, int32_t* out_quality, int64_t cap, int64_t* out_n,
                               int32_t out_rect[4]);
/* The autocrop streaming hasher under the detail rule (hvd_dev_content_rects_detail): the per-batch fold is the detail kernel,
 * everything else -- retain, finish with hvd_hasher_finish_autocrop, reset, limits, errors -- is hvd_hasher_create_autocrop's.
 * For any sequence of frames the result equals hvd_pdq_hash_frames_detail_gray_u8 / _rgb24_u8 on the same frames as one video
 * with the same detail_level (0..254) / min_detail (>= 1; else HVD_ERR_ARG). The rule is order-free per frame, so it streams. */
int hvd_hasher_create_autocrop_detail(int width, int height, int channels, int64_t batch_frames, int detail_level, int min_detail,
                                      int64_t max_retained_bytes, hvd_hasher** out);

/* --------------------------------------------- device-resident API ------- */
/* For pipelines that keep data in HBM (hash on the GPU, then search) and for the
 * benchmark. Pointers named d_* are device pointers from hvd_dev_malloc. Kernels are
 * enqueued on the library stream and return immediately; hvd_dev_sync() waits. */

int hvd_dev_malloc(void** out_ptr, size_t bytes);
int hvd_dev_free(void* d_ptr);
/* Page-locked host memory: hvd_memcpy_h2d/d2h from/to it run at the DMA rate (a decoder that cannot write into
 * the hasher's slots -- hvd_hasher_acquire -- should at least decode into this); bench.py's H2D probe uses it. */
int hvd_host_malloc(void** out_ptr, size_t bytes);
int hvd_host_free(void* h_ptr);
int hvd_dev_memset(void* d_ptr, int value, size_t bytes);
int hvd_memcpy_h2d(void* d_dst, const void* src, size_t bytes);
int hvd_memcpy_d2h(void* dst, const void* d_src, size_t bytes);
int hvd_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes); /* enqueued on the library stream */
int hvd_dev_sync(void);
/* hipDeviceSynchronize(): every stream of the bound device (the library stream, the hashers' streams, RCCL's). */
int hvd_device_synchronize(void);

/* DCT accumulation mode of the frame hash. HVD_DCT_STRICT (default): every `sum += D*A` is a
 * separately rounded multiply and add -- the numerics of upstream's x86-64 builds and of the
 * oracle's default mode. HVD_DCT_FMA (opt-in): one fused multiply-add per step, executed by
 * v_mfma_f32_16x16x4_f32 -- the numerics upstream has where the compiler contracts that statement
 * (its arm64 builds); bit-exact against the oracle's fma mode, about 2 % of hash bits differ from
 * the strict mode. Quality values do not depend on the mode. Process-wide. */
#define HVD_DCT_STRICT 0
#define HVD_DCT_FMA 1
int hvd_set_pdq_dct_mode(int mode);
int hvd_get_pdq_dct_mode(void);

/* Developer switches for A/B measurements; results never change, only which kernel form runs:
 *   "pdq_dct_from_lds" 0|2|3                               (64x64 hash kernel's DCT operands: SGPRs | literals | by batch size)
 *   "pdq_fused_down512" 0|1                                (0: generic 4-launch down-sampler)
 *   "pdq_down512_wave" 0|1|2                               (wave-per-frame kernel: never | batches >= 704 | always)
 *   "pdq_down512_wave_grid" n                              (waves in flight; 0 = what is resident at once)
 *   "pdq_down512_strip" 0|32|64                            (workgroup-per-frame kernel's strip width: by batch size | 32 | 64)
 *   "mfma_col_chunk_max"                                   (FP4-MFMA Hamming kernel: largest column chunk of a tile)
 *   "mfma_auto_mid" 0|18, "mfma_auto_mid_max_x100" n       (auto variant: may it pick the panel-mark queue form -- 18 -- and the
 *                                                           survivor density per 1024-pair tile, x 0.01, up to which it does -- 500)
 *   "mfma_queue_packed" 0|1                                (0: the pair queue settles from the FP4 images only)
 *   "mfma_probe_packed" 0|1                                (auto variant, index-eligible self pass: the probe counts over the packed
 *                                                           hashes -- 1, default -- | over the FP4 image like every other probe; the
 *                                                           words it leaves, "mfma_probe_close" among them, are the same integers)
 *   "allpairs_index" -1|0|1                                (auto variant, self pass, max_dist <= 31: the exact pigeonhole index path --
 *                                                           -1 the device decides from its histograms (default) | never | whenever
 *                                                           eligible; not the query x target or video searches)
 *   "index_stage" 0|1                                      (index build, high-byte pass: direct stores -- k_index_partition -- | a tile's
 *                                                           runs laid out in LDS and copied out in order -- k_index_scatter, default)
 *   "mfma_force_sel" -1|0|1|2                              (which 128 bits the first stage sees: the probe's choice | bits 0..127 |
 *                                                           128..255 | 0..63 + 192..255)
 *   "pdq_hash_grid" n                                      (64x64 hash kernel: forced grid; 0 = by batch size)
 *   "vmatch_exchange" 0|1|2                                (key exchange of the video search: iff world > 1 | always | never)
 *   "vmatch_slots_log2" 0|4..30                            (initial size of the video-reduction tables; tests the regrowth)
 *   "vmatch_variant" 0|8|9|12|13|18                        (all-pairs form of the video-level searches; 0 = the auto variant)
 *   "vmatch_bit_order" 0|1|2                               (video search: hashes rewritten with the 128 least entangled bits first: never |
 *                                                           from 65 536 frames on (default) | always; results never change)
 *   "match_server" 0|1                                     (hvd_match_two, small operands: one launch per call | a workgroup that stays
 *                                                           resident between calls and polls pinned host memory -- the default)
 *   "pdq_fused_rect" 0|1                                   (content-rectangle down-sampler, frames up to 512 x 512: four generic passes | fused kernel; same bits)
 *   "copy_nt" 0|1                                          (hvd_hasher_push: plain memcpy | non-temporal stores where the CPU has them)
 *   "mfma_clock_reset" 1                                   (telemetry: clear this context's clock accumulators, in stream order)
 * Unknown keys and out-of-range values return HVD_ERR_ARG. */
int hvd_debug_set(const char* key, int value);
/* "mfma_auto_form": the form (9, 18 or 12) the last auto-variant launch ran;
 * "mfma_probe_survivors" / "mfma_probe_survivors_hi" / "mfma_probe_survivors_mix": what its probe counted over bits 0..127 /
 * 128..255 / 0..63 + 192..255; "mfma_auto_half": the selection the first stage ran on (0 / 1 / 2 in that order).
 * "mfma_auto_form" keeps meaning the matrix-core form the probe chose, also when the pass ran on the pigeonhole index.
 * "mfma_probe_close": over the same sample, the 16-bit block pairs (16 per hash pair) within the pigeonhole index's block radius
 * (1 for max_dist 16..31, 0 below); 0 when the pass was not index-eligible (the probe sums it only then). Read-only.
 * (hvd_debug_set "mfma_probe_packed" 1, the default: on such a pass these words are counted over the packed hashes instead of
 * the FP4 image; 0: over the image as on every other pass. The same integers either way, and process-wide, so all ranks agree.)
 * "memcpy_d2h_small_max": the largest hvd_memcpy_d2h copy, in bytes, that goes through the context's page-locked bounce buffer
 * (larger ones are copied straight into the destination); a constant of the build, needs no device.
 * "allpairs_index_used": 1 if the last auto-variant pass ran on the pigeonhole index, else 0; "allpairs_index_kcand": its exact
 * candidate count / 1000 (0 when the probe's estimate kept the histograms from being built).
 * "allpairs_index_cand_lo": the low 31 bits of that exact count; "allpairs_index_max_walk": its longest work item, max over
 * (block, key u) of c_u x (c_u + the counts of the one-bit neighbours above u when the radius is 1), as min(value, 2^31 - 1).
 * Synchronises the library stream.
 * "vmatch_us_local" / "vmatch_us_exchange" / "vmatch_us_fold": host microseconds of the three phases of the last video-level
 * search on the calling thread's context (local: packed hashes, probe, all-pairs pass, key set; exchange: agreement words,
 * all-gather of the key lists, merged set -- 0 at world 1; fold: keys -> pair map). "copy_nt": 0 | 2 | 3 = plain memcpy |
 * AVX2 | AVX-512 streaming stores in hvd_hasher_push (hvd_debug_set "copy_nt" 0|1; HVD_COPY_NT=0 in the environment).
 * "vmatch_bit_order_used": 1 if the last video search on this context rewrote its hashes in a chosen bit order.
 * "hasher_us_copy" / "hasher_us_submit" / "hasher_us_wait": host microseconds the streaming hashers of this process spent copying
 * frames into the ring, enqueueing batches and waiting for a slot since the last read (reading clears).
 * "mfma_pass_khz": the shader clock (kHz) the FP4-MFMA all-pairs passes of this context ran at since the last
 * "mfma_clock_reset": one workgroup in eight brackets its lifetime with s_memtime (shader cycles) and s_memrealtime (constant
 * rate); cycles / ticks x hipDeviceAttributeWallClockRate. "mfma_clock_samples": how many workgroups contributed (0: none,
 * and "mfma_pass_khz" reads 0). Both wait for the library stream. */
int hvd_debug_get(const char* key, int* out_value);

/* Bytes of device scratch hvd_dev_pdq_hash_frames needs for this geometry (0 for
 * 64x64 gray): the 64x64 float luma of every frame plus the blur workspace.
 * Layout contract: after hvd_dev_pdq_hash_frames[_dihedral] the first 4096*n floats of the scratch hold the n
 * frame-major, row-major 64x64 planes that were hashed (tests/test_gpu_pdq_planes.py compares them with the oracle's). */
int hvd_pdq_scratch_bytes(int64_t n, int h, int w, int channels, size_t* out_bytes);
/* channels: 1 (gray u8) or 3 (RGB24). d_scratch: hvd_pdq_scratch_bytes() bytes
 * (NULL when that is 0). h,w in [64,4096]. */
int hvd_dev_pdq_hash_frames(const void* d_frames, int64_t n, int h, int w, int channels, void* d_scratch,
                            void* d_hashes, void* d_quality);
/* Dihedral PDQ: 8 hashes per frame in the order of the table in DESIGN (identity first), n*8*32 bytes. */
int hvd_dev_pdq_hash_frames_dihedral(const void* d_frames, int64_t n, int h, int w, int channels, void* d_scratch,
                                     void* d_hashes8, void* d_quality);      /* scratch: hvd_pdq_scratch_bytes */

/* ---- content-rectangle PDQ: re-uploads with black bars (letterbox, pillarbox) hash like the original ----
 * The rule, integers only: a pixel is bright iff max(R, G, B) > black_level (0..254); a row (column) of a frame is content
 * iff it holds >= min_bright (>= 1) bright pixels; a frame's rectangle is the bounding box of its content rows x the bounding
 * box of its content columns (none if either is empty); a VIDEO's rectangle is the bounding box of the rectangles of all its
 * frames. Per axis: no rectangle in any frame, or a box shorter than 64 -> the full extent. A video without frames gets the
 * full frame. Record: int32[4] = {top, left, height, width}. The hash of a frame under its video's rectangle is the plain PDQ
 * hash and quality of the contiguous height x width crop.
 * d_offsets: int64[V+1] CSR of the n frames in device memory (offsets[0] = 0, non-decreasing, offsets[V] = n; the host-buffer
 * entries check that, the device-resident ones cannot without a synchronisation: a frame is looked up by binary search and
 * always lands in [0, V), so a broken CSR gives wrong rectangles, never an access out of bounds).
 * d_rects: int32[V][4], 16-byte aligned (the kernels access a record as one 16-byte word; HVD_ERR_ARG otherwise); nothing
 * else is allocated. d_frames needs no alignment. Enqueued on the library stream, no host synchronisation. */
int hvd_dev_content_rects(const void* d_frames, int64_t n, int h, int w, int channels, const void* d_offsets, int64_t V,
                          int black_level, int min_bright, void* d_rects);
/* Scratch of hvd_dev_pdq_hash_frames_rects: hvd_pdq_scratch_bytes, rounded up to 16, plus 16 bytes per frame (at 64x64:
 * hvd_pdq_scratch_bytes as it is, 0 for gray). d_scratch and d_rects must be 16-byte aligned (HVD_ERR_ARG otherwise). The layout
 * contract of hvd_pdq_scratch_bytes holds: afterwards the first 4096*n floats are the planes that were hashed. */
int hvd_pdq_rects_scratch_bytes(int64_t n, int h, int w, int channels, size_t* out_bytes);
/* Hashes every frame inside its video's rectangle d_rects[video] (from hvd_dev_content_rects, or the caller's own: any
 * rectangle inside the frame with both sides >= 64; a record that is not is taken as the full frame). Enqueues without a
 * host synchronisation, so it does not look at the rectangles: every geometry but 64x64 (where the rule leaves only the full
 * frame, and the plain kernels run) takes the table-driven generic down-sampler, full rectangles included. A caller that
 * knows all its rectangles are full calls hvd_dev_pdq_hash_frames instead (same bits, fused 512x512 kernels). Both DCT modes. */
int hvd_dev_pdq_hash_frames_rects(const void* d_frames, int64_t n, int h, int w, int channels, const void* d_offsets,
                                  int64_t V, const void* d_rects, void* d_scratch, void* d_hashes, void* d_quality);

/* ---- bar-colour content rectangle: re-uploads behind white, grey or coloured bars hash like the original ----
 * The rule, integers only. Parameters: bar_level L (0..254), min_bright (>= 1), and one bar colour per video, c = (c0, c1, c2),
 * each 0..255, in the byte order of the pixel (gray frames use c0 only). Colour record: int32 per video = c0 | c1 << 8 | c2 << 16.
 *  1. A pixel p is content iff max_k |p_k - c_k| > L. Everything else is the content-rectangle rule above word for word, with
 *     "bright" read as "content": content rows and columns with min_bright, the frame box, the video box as the union of the
 *     frame boxes, the per-axis fallback below 64, the full frame for a video without frames. With c = 0 it IS that rule with
 *     black_level = L.
 *  2. Explicit colour: the caller writes d_colors.
 *  3. Automatic colour (hvd_dev_bar_colors), per video, from the four corner pixels (0,0), (0,w-1), (h-1,0), (h-1,w-1) of all
 *     its frames: per channel lo_k / hi_k are the min / max over those pixels; if hi_k - lo_k <= L on every channel,
 *     c_k = (lo_k + hi_k) >> 1; otherwise c = (0, 0, 0), the black rule; a video without frames gets c = 0.
 * The hash of a frame under the rectangle is the plain PDQ hash of the contiguous crop (hvd_dev_pdq_hash_frames_rects).
 * d_offsets: as for hvd_dev_content_rects (a broken CSR gives wrong results, never an access out of bounds). d_scratch:
 * hvd_bar_colors_scratch_bytes(V) bytes, 4-byte aligned; d_colors: int32[V], 4-byte aligned; d_rects: int32[V][4], 16-byte
 * aligned (HVD_ERR_ARG otherwise). Nothing is allocated. 64x64 frames: every rectangle is the full frame and no frame is read
 * for it. All enqueued on the library stream, no host synchronisation. */
int hvd_bar_colors_scratch_bytes(int64_t V, size_t* out_bytes);
int hvd_dev_bar_colors(const void* d_frames, int64_t n, int h, int w, int channels, const void* d_offsets, int64_t V,
                       int bar_level, void* d_scratch, void* d_colors);
int hvd_dev_content_rects_color(const void* d_frames, int64_t n, int h, int w, int channels, const void* d_offsets, int64_t V,
                                const void* d_colors, int bar_level, int min_bright, void* d_rects);

/* ---- detail content rectangle: re-uploads behind blurred, gradient or any other smooth bars hash like the original ----
 * The rule, integers only. Parameters: detail_level L (0..254), min_detail m (>= 1). For a frame p[y][x][k], h rows, w columns:
 *  1. dh(y, x) = max_k |p[y][x][k] - p[y][x+1][k]| > L, x in [0, w-2]. ROW y is content iff #{x : dh(y, x)} >= m.
 *  2. dv(y, x) = max_k |p[y][x][k] - p[y+1][x][k]| > L, y in [0, h-2]. COLUMN x is content iff #{y : dv(y, x)} >= m.
 *  3. Everything else is the content-rectangle rule of hvd_dev_content_rects word for word: the frame box from content rows x
 *     content columns, the video box as the union of the frame boxes, the per-axis fallback below 64, the full frame for a
 *     video without frames. Rows count horizontal differences only and columns vertical ones only, so the step between a bar
 *     and the picture never makes a bar row or a bar column content.
 * No colour and no corner enters the rule: it covers black, coloured, gradient and blurred bars alike, and misses bars that
 * carry text, a logo or noise above L. Arguments, alignment, the 64x64 shortcut and the broken-CSR guarantee are
 * hvd_dev_content_rects'. Enqueued on the library stream, no host synchronisation, nothing allocated. */
int hvd_dev_content_rects_detail(const void* d_frames, int64_t n, int h, int w, int channels, const void* d_offsets, int64_t V,
                                 int detail_level, int min_detail, void* d_rects);

/* ---- crop-ladder PDQ: aspect-ratio re-crops and pan-and-scan copies hash like the original under the same rectangle
 * A crop is int32[4] = {top, left, height, width} in pixels of the call's h x w frame; it is valid iff it lies inside the frame
 * and both sides are >= 64. The full frame is a valid crop, duplicates are allowed, a call takes 1 <= K <= HVD_MAX_CROPS crops
 * in HOST memory (they travel as kernel arguments). Anything else is HVD_ERR_ARG, decided before a device is asked for: a
 * caller's list is an argument, not data (hvd_dev_pdq_hash_frames_rects, whose rectangles are data, substitutes the full frame).
 * The hash and quality of a frame under a crop are the plain PDQ hash and quality of the contiguous height x width crop (a
 * 64 x 64 crop: of its unfiltered luma). Output, the dihedral layout, so that hvd_dev_compact_kept_dihedral with the mask
 * (1 << (K + 1)) - 1 serves as it is: d_hashes8 n*8*32 bytes, hash of frame f in slot k at bytes [(8f+k)*32, (8f+k+1)*32), slot
 * 0 the full frame (bit-identical to hvd_dev_pdq_hash_frames), slots 1..K the crops in list order, slots above K zero;
 * d_quality int32[n], the full frame's; d_crop_quality int32[n*8] per slot (0 above K), or NULL. Frames up to 512 x 512 go
 * through one kernel that loops over the rectangles of a frame (at exactly 512 x 512 the full frame is hashed by the plain
 * front-end instead, so such a frame is read twice); larger ones take the generic passes once per rectangle. d_scratch:
 * hvd_pdq_crops_scratch_bytes(n, h, w, K) bytes, 16-byte aligned; bounded, the frames are taken in slabs. d_hashes8, d_quality
 * and d_crop_quality: 4-byte aligned. Enqueued on the library stream, no host synchronisation. n == 0 is legal. Both DCT modes. */
#define HVD_MAX_CROPS 7
int hvd_pdq_crops_scratch_bytes(int64_t n, int h, int w, int K, size_t* out_bytes);
int hvd_dev_pdq_hash_frames_crops(const void* d_frames, int64_t n, int h, int w, int channels, const int32_t* crops, int K,
                                  void* d_scratch, void* d_hashes8, void* d_quality, void* d_crop_quality);

/* Brute-force pass over the tiles owned by `rank` of `world` (tile (rb,cb) belongs
 * to rank (rb+cb) % world; world=1 => everything). Appends hvd_pair records to
 * d_pairs[cap] and bumps the uint64 at d_count (the caller zeroes it). Records are
 * unordered. variant: 0 = the integer form of the north star (8 xor + 8 popcount per comparison), 1 = the same behind a
 * 128-bit prefilter (the independent path of the full-size parity tests). */
int hvd_dev_allpairs_hamming256(const void* d_db, int64_t n, const void* d_group, int max_dist, int rank, int world,
                                void* d_pairs, int64_t cap, void* d_count, int variant);

/* Matrix-core form of the same pass (variants 8, 9, 12, 18 and 13 = chosen per launch by a probe): the DB is first
 * rewritten as its FP4 image (every bit b as the e2m1 number 1-2b; 128 bytes per hash,
 * rows padded to a multiple of 1024), then v_mfma_f32_32x32x64_f8f6f4 produces
 * 256 - 2*hamming for 32x32 pairs at a time. Output contract identical to
 * hvd_dev_allpairs_hamming256 (bit-identical pair set). */
int hvd_fp4_image_bytes(int64_t n, size_t* out_bytes);
int hvd_dev_expand_fp4(const void* d_db, int64_t n, void* d_img);
int hvd_dev_allpairs_hamming256_mfma(const void* d_db, const void* d_img, int64_t n, const void* d_group, int max_dist, int rank,
                                     int world, void* d_pairs, int64_t cap, void* d_count, int variant);

/* Rectangular form on two FP4 images (nq query hashes x nt target hashes): appends (i = query
 * row, j = target row, dist). d_group_q / d_group_t (both or neither): pairs with equal group
 * values are dropped. max_dist in [0,127]. */
int hvd_dev_cross_hamming256_mfma(const void* d_img_q, int64_t nq, const void* d_img_t, int64_t nt,
                                  const void* d_group_q, const void* d_group_t, int max_dist, int rank, int world,
                                  void* d_pairs, int64_t cap, void* d_count);

/* ---- video-level search with everything resident in HBM (BASELINE config 5: hash on the GPU, then search) ----
 * The three calls below use library-owned grow-only scratch, synchronise the library stream before returning
 * and are serialised against each other. */

/* d_out_video[f] = index of the video that owns frame f, from CSR offsets (int64[V+1] on the device). */
int hvd_dev_video_of_frames(const void* d_offsets, int64_t V, int64_t n, void* d_out_video);

/* VideoHasher.finish() for a whole library at once (vpdqpy/vpdqpy.py:119; keep/drop contract of dedup.py:74-86,
 * quality >= min_quality kept as in db/DedupeDB.py:550-553): stream compaction of the kept frame hashes in frame
 * order. In: d_hashes n*32 B, d_quality int32[n], d_offsets int64[V+1] over the n raw frames. Out: d_out_hashes
 * (room for n*32 B), d_out_offsets int64[V+1] over the kept frames, d_out_video int32[kept] (room for n),
 * *out_kept. A video may end up with 0 frames (legal: dedup.py:82-86). */
int hvd_dev_compact_kept(const void* d_hashes, const void* d_quality, int64_t n, const void* d_offsets, int64_t V,
                         int min_quality, void* d_out_hashes, void* d_out_offsets, void* d_out_video, int64_t* out_kept);

/* hvd_dev_compact_kept for the dihedral hashes (hvd_dev_pdq_hash_frames_dihedral: d_hashes8 n*8*32 B) and a transform
 * mask (bit t = transform t of the DESIGN table; bit 0, identity, required; bits >= 8 refused). Identity library:
 * d_out_hashes / d_out_offsets / d_out_video / *out_kept, byte for byte what hvd_dev_compact_kept makes of the variant-0
 * hashes. Query library of the K = popcount(mask) - 1 other variants, k in mask order: a kept frame at position i of
 * video v (kept offset o, kept length L) under the k-th variant goes to slot K*o + k*L + i of d_out_qhashes (room for
 * K*n*32 B), with query video v*K + k in d_out_qvideo and exclusion id v in d_out_qexcl (int32, room for K*n each) --
 * the operands of hvd_dev_vpdq_match_videos_cross against the identity library (its d_out_video as d_excl_t). The query
 * outputs may be NULL when K = 0. Only the selected variants are read. */
int hvd_dev_compact_kept_dihedral(const void* d_hashes8, const void* d_quality, int64_t n, const void* d_offsets, int64_t V,
                                  int min_quality, int transform_mask, void* d_out_hashes, void* d_out_offsets,
                                  void* d_out_video, void* d_out_qhashes, void* d_out_qvideo, void* d_out_qexcl,
                                  int64_t* out_kept);

/* The raw index inside its video of every kept frame, in kept order: d_out_pos int32[kept] (room for n), the positions operand
 * of hvd_dev_vpdq_align_videos for a library made by hvd_dev_compact_kept from the same d_quality / d_offsets (raw CSR, int64[V+1])
 * / min_quality. Without it a dropped frame shifts the timeline of every frame after it. Enqueued on the library stream, no
 * host synchronisation; library-owned scratch. */
int hvd_dev_kept_positions(const void* d_quality, int64_t n, const void* d_offsets, int64_t V, int min_quality, void* d_out_pos);

/* Device-resident alignment (the rule: hvd_vpdq_align_videos above). d_hashes_*: packed hashes (n*32 B, 16-byte aligned);
 * d_offsets_*: int64[V+1] CSR; d_pos_*: int32 per frame or NULL; d_pairs: uint32[M][2]; d_out: M hvd_valign records. Pairs
 * whose histogram has more than HVD_ALIGN_LDS_BINS bins need d_scratch: hvd_align_scratch_bytes(max_bins) bytes serve every
 * pair of up to max_bins bins (<= 2^20; 0 bytes up to HVD_ALIGN_LDS_BINS, d_scratch may then be NULL). Enqueued on the library
 * stream: no host synchronisation, nothing allocated -- so nothing on the device is validated: a pair index outside [0, V), a
 * pair beyond 2^20 bins or beyond the scratch, and positions that are visibly not increasing give the INT32_MIN record (see
 * hvd_valign); frame ranges are clamped to [0, offsets[V]] and every bin index is checked, so broken operands give wrong
 * records, never an access out of bounds. */
int hvd_align_scratch_bytes(int64_t max_bins, size_t* out_bytes);
int hvd_dev_vpdq_align_videos(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                              const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                              const void* d_pairs, int64_t M, int max_dist, int slack, void* d_scratch, size_t scratch_bytes,
                              void* d_out);

/* Device-resident coverage (the rule: hvd_vpdq_cover_videos above). One library: d_hashes (n_frames * 32 B, 16-byte aligned),
 * d_offsets int64[V+1], d_pos int32 per frame or NULL; d_pairs: uint32[M][2]; d_out_align: M hvd_valign records; d_out_cover: V
 * hvd_vcover records, 16-byte aligned. d_scratch (16-byte aligned) holds one bit per frame of the library -- bit offsets[v] + i
 * is frame i of video v -- and behind it the scratch of hvd_dev_vpdq_align_videos: hvd_cover_scratch_bytes(n_frames, max_bins)
 * = the bitmap, (n_frames + 31) / 32 words rounded up to 16 bytes, plus hvd_align_scratch_bytes(max_bins). The entry enqueues,
 * on the library stream, the clear of the bitmap and of the V cover records, the two launches of the alignment and the count:
 * no host synchronisation, nothing allocated, nothing on the device validated. A pair the entry cannot align (the conditions of
 * hvd_valign) gets the INT32_MIN record and contributes nothing; frame ranges are clamped to [0, offsets[V]] and every word
 * index of the bitmap is checked against its length, so broken operands give wrong records, never an access out of bounds.
 * HVD_ERR_ARG: what hvd_dev_vpdq_align_videos rejects, min_aligned < 1, n_frames outside [0, 2^32 - 2], a scratch smaller
 * than the bitmap needs. M == 0 is legal: every video gets (0, 0, 0, frames). */
int hvd_cover_scratch_bytes(int64_t n_frames, int64_t max_bins, size_t* out_bytes);
int hvd_dev_vpdq_cover_videos(const void* d_hashes, const void* d_offsets, int64_t V, int64_t n_frames, const void* d_pos,
                              const void* d_pairs, int64_t M, int max_dist, int slack, int min_aligned, void* d_scratch,
                              size_t scratch_bytes, void* d_out_align, void* d_out_cover);

/* Device-resident multi-segment alignment (the rule: hvd_vpdq_align_segments above). The operands of
 * hvd_dev_vpdq_align_videos, plus max_segments in [1, HVD_ALIGN_MAX_SEGMENTS] and min_band_votes >= 1 (HVD_ERR_ARG otherwise);
 * d_out: M hvd_vsegments records, 16-byte aligned. The scratch of a pair beyond HVD_ALIGN_LDS_BINS bins also holds the taken
 * sets: hvd_segments_scratch_bytes(max_bins) bytes serve every pair of up to max_bins bins (<= 2^20). Enqueued on the library
 * stream: no host synchronisation, nothing allocated, nothing on the device validated -- what gives the INT32_MIN record of
 * hvd_dev_vpdq_align_videos gives the one of hvd_vsegments here, and broken operands give wrong records, never an access out
 * of bounds. A pair stops without another pass over its frames once q_covered or t_covered reaches the video's length. */
int hvd_segments_scratch_bytes(int64_t max_bins, size_t* out_bytes);
int hvd_dev_vpdq_align_segments(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                                const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                                const void* d_pairs, int64_t M, int max_dist, int slack, int max_segments, int min_band_votes,
                                void* d_scratch, size_t scratch_bytes, void* d_out);

/* Device-resident rate-aware alignment (the rule: hvd_vpdq_align_rates above). The operands of hvd_dev_vpdq_align_videos, plus
 * rates / n_rates: the list, in HOST memory (it is packed into two kernel arguments); d_out: M hvd_vrate records, 16-byte aligned.
 * A pair's histogram is sized by its largest bins_r over the list: beyond HVD_ALIGN_LDS_BINS the pair needs d_scratch, and
 * hvd_rates_scratch_bytes(max_bins) bytes serve every pair whose largest bins_r is up to max_bins (<= 2^20). Two launches are
 * enqueued on the library stream: no host synchronisation, nothing allocated, nothing on the device validated. What gives the
 * INT32_MIN record of hvd_dev_vpdq_align_videos gives it here, and so do a rate that needs more than 2^20 bins and a broken
 * rate list (every pair then); broken operands give wrong records, never an access out of bounds. HVD_ERR_ARG: rates NULL or
 * n_rates < 0, and what hvd_dev_vpdq_align_videos rejects. R listed rates cost R + 1 passes over the pair's Hamming matrix. */
int hvd_rates_scratch_bytes(int64_t max_bins, size_t* out_bytes);
int hvd_dev_vpdq_align_rates(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                             const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                             const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                             void* d_scratch, size_t scratch_bytes, void* d_out);

/* Device-resident rate-aware multi-segment alignment (the rule: hvd_vpdq_align_rate_segments above). The operands of
 * hvd_dev_vpdq_align_rates, plus max_segments in [1, HVD_ALIGN_MAX_SEGMENTS] and min_band_votes >= 1 (HVD_ERR_ARG otherwise)
 * between the rate list and the scratch; d_out: M hvd_vrsegments records, 16-byte aligned. A pair's histogram is sized by its
 * largest bins_r over the list, and its scratch slot also holds the taken sets: hvd_rate_segments_scratch_bytes(max_bins) bytes
 * serve every pair whose largest bins_r is up to max_bins (<= 2^20). Two launches are enqueued on the library stream: no host
 * synchronisation, nothing allocated, nothing on the device validated. What gives the INT32_MIN record of
 * hvd_dev_vpdq_align_rates gives the one of hvd_vrsegments here (a broken list: every pair); broken operands give wrong records,
 * never an access out of bounds. K rounds of R rates cost at most K (R + 1) passes over the pair's Hamming matrix; after round 1
 * a rate whose last best band cannot beat the round's winner is passed over, so a full copy costs R + 1. */
int hvd_rate_segments_scratch_bytes(int64_t max_bins, size_t* out_bytes);
int hvd_dev_vpdq_align_rate_segments(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                                     const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                                     const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                                     int max_segments, int min_band_votes, void* d_scratch, size_t scratch_bytes, void* d_out);

/* Device-resident alignment with negative rates (the rule: hvd_vpdq_align_signed above). The operands of
 * hvd_dev_vpdq_align_rate_segments; rates may hold negative numerators; d_out: M hvd_vssegments records, 16-byte aligned. A
 * pair's histogram is sized by its largest bins_r = |num| span_a + den span_b + 1 + 2 slack max(|num|, den) over the list:
 * hvd_signed_scratch_bytes(max_bins) bytes serve every pair of up to max_bins bins (<= 2^20). Two launches are enqueued on the
 * library stream: no host synchronisation, nothing allocated, nothing on the device validated. A list that is not sound as a
 * signed list gives every pair the INT32_MIN record; broken operands give wrong records, never an access out of bounds. */
int hvd_signed_scratch_bytes(int64_t max_bins, size_t* out_bytes);
int hvd_dev_vpdq_align_signed(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                              const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                              const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                              int max_segments, int min_band_votes, void* d_scratch, size_t scratch_bytes, void* d_out);

/* Device-resident alignment of looped clips (the rule: hvd_vpdq_align_loops above). The operands of hvd_dev_vpdq_align_signed
 * with max_rounds in the place of max_segments; d_out: M hvd_vloops records, 16-byte aligned. A slot of the scratch holds the
 * histogram and three pairs of runs of bit words (flag, taken, seen): hvd_loops_scratch_bytes(max_bins) bytes serve every pair
 * of up to max_bins bins (<= 2^20), 0 up to HVD_ALIGN_LDS_BINS. Two launches are enqueued on the library stream: no host
 * synchronisation, nothing allocated, nothing on the device validated. A list that is not sound as a signed list gives every
 * pair the INT32_MIN record; broken operands give wrong records, never an access out of bounds. */
int hvd_loops_scratch_bytes(int64_t max_bins, size_t* out_bytes);
int hvd_dev_vpdq_align_loops(const void* d_hashes_q, const void* d_offsets_q, int64_t VQ, const void* d_pos_q,
                             const void* d_hashes_t, const void* d_offsets_t, int64_t VT, const void* d_pos_t,
                             const void* d_pairs, int64_t M, int max_dist, int slack, const int32_t* rates, int n_rates,
                             int max_rounds, int min_band_votes, void* d_scratch, size_t scratch_bytes, void* d_out);

/* Device-resident grouping (the rule: hvd_group_edges above). d_records: n_records records of 16 bytes, 16-byte aligned;
 * d_record_count: NULL, or the uint64 the all-pairs entries bump -- the kernels then take min(*d_record_count, n_records)
 * records, so the call chains behind hvd_dev_allpairs_hamming256[_mfma] (d_pairs, cap, d_count) with no read-back. d_lengths:
 * int64[V] (HVD_EDGES_VMATCH only); d_score: uint32[V] or NULL; d_scratch: hvd_group_scratch_bytes(V) bytes (20 per node and 4
 * per 1024 nodes), 8-byte aligned; d_out_label: int32[V]; d_out_groups: cap records, 16-byte aligned (may be NULL when cap is
 * 0); d_out_count: one uint64, the true number of groups. Enqueued on the library stream: no host synchronisation, nothing
 * allocated. Records that are no edge (an index >= V, u == v) are ignored; every index is checked before use, so a broken list
 * gives other groups, never an access out of bounds. */
int hvd_group_scratch_bytes(int64_t V, size_t* out_bytes);
int hvd_dev_group_edges(const void* d_records, int64_t n_records, const void* d_record_count, int kind, const void* d_lengths,
                        int threshold, int policy_is_min, int64_t V, const void* d_score, void* d_scratch, void* d_out_label,
                        void* d_out_groups, int64_t cap, void* d_out_count);

/* Device-resident keeper-first grouping (the rule: hvd_keeper_groups above). The operands are those of hvd_dev_group_edges,
 * d_record_count included; d_scratch: hvd_keeper_scratch_bytes(V) bytes (28 per node, 4 per 1024 nodes and 16), 8-byte aligned;
 * d_out_keeper: int32[V]; d_out_groups: cap records, 16-byte aligned (may be NULL when cap is 0); d_out_count: one uint64, the
 * true number of groups; out_rounds: a HOST int64, or NULL. The keepers are decided in rounds of two launches; a round decides
 * at least the best undecided node of every component, so V rounds suffice, and a few do unless priority runs monotone along
 * long chains. Unlike hvd_dev_group_edges this entry DOES synchronise: it enqueues the rounds in batches of 32
 * on the library stream and between batches reads the number of undecided nodes back, one 4-byte copy, until that is zero;
 * the closing launches are then enqueued behind, as hvd_dev_group_edges' are. More than V rounds: HVD_ERR_STATE. Nothing is
 * allocated. Records that are no edge are ignored; every index is checked before use. */
int hvd_keeper_scratch_bytes(int64_t V, size_t* out_bytes);
int hvd_dev_keeper_groups(const void* d_records, int64_t n_records, const void* d_record_count, int kind, const void* d_lengths,
                          int threshold, int policy_is_min, int64_t V, const void* d_score, void* d_scratch, void* d_out_keeper,
                          void* d_out_groups, int64_t cap, void* d_out_count, int64_t* out_rounds);

/* Every video pair a<b with >= 1 frame hit, with its vPDQ counters (semantics of vpdqpy/vpdqpy.py:49-56 for all
 * pairs at once; replaces the tree walk of dedup.py:468-475). d_img: FP4 image of the n frame hashes; d_video:
 * int32[n] frame -> video (frames of one video are never compared). The counters are reduced ON THE DEVICE: the
 * all-pairs kernel records "frame f has a match in video v" in a set in HBM, which is then folded into one
 * hvd_vmatch per video pair -- frame-level hits never leave the GPU. world > 1: this rank compares its tiles,
 * the key sets are all-gathered over RCCL (hvd_comm_init required) and every rank returns the full result.
 * d_out[cap] receives min(count, cap) unordered records, the uint64 at d_count the true count. max_dist in
 * [0,127]. */
int hvd_dev_vpdq_match_videos(const void* d_img, int64_t n, const void* d_video, int max_dist, int rank, int world,
                              void* d_out, int64_t cap, void* d_count);
/* The records of the LAST hvd_dev_vpdq_match_videos[_cross] call once more, into a (larger) buffer: only the emit
 * step runs -- no compare, no exchange, so in a multi-rank pass a rank whose buffer was too small does not drag the
 * others into another collective. The pair map of that call stays valid until the next video search on this
 * process (the host-buffer entry points hvd_vpdq_match_videos[_cross] included). */
int hvd_dev_vpdq_emit_again(void* d_out, int64_t cap, void* d_count);
/* Device-resident form of hvd_vpdq_frame_spread: d_img / n / d_video as hvd_dev_vpdq_match_videos, d_out_spread int32[n]. The
 * compare and the key set of that search without its fold: every key (frame f, video v) adds one to spread[f], no pair map
 * is built, and the pair map of the last search stays valid for hvd_dev_vpdq_emit_again. Runs on the calling thread's context
 * alone (no rank / world), uses library-owned scratch, is serialised with the video searches and synchronises the library
 * stream before returning. max_dist in [0, 127]; n < 2 zeroes the output. */
int hvd_dev_vpdq_frame_spread(const void* d_img, int64_t n, const void* d_video, int max_dist, void* d_out_spread);
/* The rule of the common-frame filter, integers only. d_spread int32[n], d_offsets int64[V+1] (a CSR over the n frames) ->
 * d_out_keep int32[n], 1 or 0. A frame is common iff spread > max_videos; a video is a carrier iff it has c > 0 common frames
 * and 100 c <= max_share len (64-bit); a frame is dropped (keep 0) iff it is common and its video is a carrier -- so a video
 * that is mass-copied as a whole, or is nothing but the intro, keeps every frame. max_videos >= 0, max_share in [0, 100]
 * (HVD_ERR_ARG otherwise, nothing launched). d_out_keep is the d_quality operand of hvd_dev_compact_kept /
 * hvd_dev_kept_positions with min_quality 1. One launch, enqueued on the library stream, no host synchronisation, nothing
 * allocated; ranges are clamped to [0, n], so broken offsets give other flags, never an access out of bounds. */
int hvd_dev_common_frames(const void* d_spread, const void* d_offsets, int64_t V, int64_t n, int max_videos, int max_share,
                          void* d_out_keep);
/* d_out[j] = d_in[f] for the j-th frame f with d_keep[f] >= 1 (int32 each; d_out: room for n): carries the positions of a
 * library through the compaction hvd_dev_compact_kept does on its hashes. Enqueued on the library stream, no host
 * synchronisation; library-owned scratch. */
int hvd_dev_gather_kept_i32(const void* d_in, const void* d_keep, int64_t n, void* d_out);
/* The static-scene filter: one keyframe per run of near-identical consecutive frames -- a held shot, a slide, a
 * title card, a freeze frame, the repeated frames of a 24 -> 60 fps conversion. The rule, integers only, one answer per library.
 * d_hashes 32 B per frame, d_offsets int64[V+1] (a CSR over the n frames). For every video, over its frames in CSR order:
 *     anchor = the first frame; keep it; run[anchor] = 1
 *     for each later frame f, in order:
 *         if hamming(h_f, h_anchor) <= max_dist and (max_run == 0 or run[anchor] < max_run):
 *             drop f; run[anchor] += 1; run[f] = 0
 *         else:
 *             anchor = f; keep it; run[f] = 1
 * -> d_out_keep int32[n], 1 or 0, and d_out_run int32[n] (may be NULL): the number of frames a kept frame stands for, 0 at a
 * dropped frame. A frame is compared with its ANCHOR, not with its predecessor, so slow drift cannot chain a whole video into
 * one run. What follows from the rule:
 *   (a) the first frame of every non-empty video is kept;
 *   (b) every dropped frame is within max_dist of the nearest kept frame before it in its video, and fewer than max_run frames
 *       behind it when max_run > 0;
 *   (c) for two consecutive kept frames k1 < k2 of one video, hamming(k1, k2) > max_dist or run[k1] == max_run;
 *   (d) run sums to each video's length;
 *   (e) with max_run == 0 the rule is idempotent: applied to its own output it drops nothing;
 *   (f) with max_run == 1 nothing is dropped;
 *   (g) with max_dist == 0 a dropped frame EQUALS its anchor, so the set of (frame, video) hit facts of any search is unchanged
 *       and only the counts shrink: 0 is the lossless choice.
 * max_dist in [0, 127], max_run in [0, 2^20] (0 = no limit), V and n not negative: HVD_ERR_ARG otherwise, nothing launched.
 * d_out_keep is the d_quality operand of hvd_dev_compact_kept / hvd_dev_kept_positions with min_quality 1; the kept frame
 * carries the position of the FIRST frame of its run. One launch, enqueued on the library stream, no host synchronisation,
 * nothing allocated; ranges are clamped to [0, n], so offsets that are no CSR over n give other flags, never an access outside
 * the buffers. A video is one wave's, however long it is. */
int hvd_dev_frame_runs(const void* d_hashes, const void* d_offsets, int64_t V, int64_t n, int max_dist, int max_run,
                       void* d_out_keep, void* d_out_run);
/* Device-resident forms of the duration-weighted search. d_weight: int32 per frame, as hvd_dev_frame_runs and
 * hvd_dev_gather_kept_i32 leave the run words of a collapsed library. Nothing is validated on the device: a weight below 1 or
 * a total past 2^32 - 1 gives wrong counters (mod 2^32), never an access outside the buffers.
 * hvd_dev_video_weights: d_out_totals int64[V] = per video of the CSR d_offsets (int64[V+1] over the n frames, ranges clamped
 * to [0, n]) the sum of max_weight ? min(w, max_weight) : w. One launch on the library stream, no host synchronisation,
 * nothing allocated; a video is one wave's, however long it is (as in hvd_dev_frame_runs).
 * hvd_dev_vpdq_match_videos_weighted / _cross_weighted: hvd_dev_vpdq_match_videos[_cross] on the calling thread's context
 * alone (rank 0 of 1) with the weighted fold; serialised with the other video searches; library-owned scratch; the pair map
 * stays for hvd_dev_vpdq_emit_again, which then emits the weighted counters again. */
int hvd_dev_video_weights(const void* d_weight, const void* d_offsets, int64_t V, int64_t n, int max_weight, void* d_out_totals);
int hvd_dev_vpdq_match_videos_weighted(const void* d_img, int64_t n, const void* d_video, const void* d_weight, int max_weight,
                                       int max_dist, void* d_out, int64_t cap, void* d_count);
int hvd_dev_vpdq_match_videos_cross_weighted(const void* d_img_q, int64_t nq, const void* d_video_q, const void* d_excl_q,
                                             const void* d_weight_q, const void* d_img_t, int64_t nt, const void* d_video_t,
                                             const void* d_excl_t, const void* d_weight_t, int max_weight, int max_dist,
                                             void* d_out, int64_t cap, void* d_count);
/* Device-resident form of hvd_vpdq_frame_spread_cross: operands as hvd_dev_vpdq_match_videos_cross without exclusion maps,
 * d_spread_q int32[nq], d_spread_t int32[nt]. The compare and the key set of that search without its fold (rank 0 of 1): a
 * side-0 key (query frame f, target video) adds one to d_spread_q[f], a side-1 key (target frame g, query video) one to
 * d_spread_t[g]. Either output may be NULL (that side is skipped), not both. accumulate == 0: the outputs are zeroed first;
 * otherwise the counts are added to what the arrays hold (spread_T + st in one pass). nq == 0 or nt == 0: the
 * outputs are zeroed unless accumulate, nothing else is launched. No pair map is built: hvd_dev_vpdq_emit_again still returns
 * the last search. Runs on the calling thread's context alone, is serialised with the video searches and synchronises the
 * library stream before returning. HVD_ERR_ARG (nothing launched): both outputs NULL, sizes out of range, max_dist outside
 * [0, 127], an image or video map NULL while both sides are non-empty. */
int hvd_dev_vpdq_frame_spread_cross(const void* d_img_q, int64_t nq, const void* d_video_q, const void* d_img_t, int64_t nt,
                                    const void* d_video_t, int max_dist, int accumulate, void* d_spread_q, void* d_spread_t);
/* Query library x target library form (VpTreeManager.search_file for a batch, db/vptree.py:865-902).
 * d_excl_q / d_excl_t (both or neither): int32 per frame, frames with equal values are not compared. */
int hvd_dev_vpdq_match_videos_cross(const void* d_img_q, int64_t nq, const void* d_video_q, const void* d_excl_q,
                                    const void* d_img_t, int64_t nt, const void* d_video_t, const void* d_excl_t,
                                    int max_dist, int rank, int world, void* d_out, int64_t cap, void* d_count);

/* Host-only: the tile geometry hvd_dev_allpairs_hamming256 uses for (n, variant): a
 * tile is rows [rb*rows_per_block, +rows_per_block) x columns [cb*col_chunk, +col_chunk). */
int hvd_allpairs_tile_geometry(int64_t n, int variant, uint32_t* rows_per_block, uint32_t* col_chunk);

/* hipEvent pair on the library stream: wall time of everything enqueued between. */
int hvd_timer_start(void);
int hvd_timer_stop(float* out_ms);
/* Eight event slots per context for split timings without extra synchronisation (ABI 5): hvd_timer_mark(k) records event k
 * on the library stream and returns at once; hvd_timer_between(a, b, &ms) waits for event b and returns the device time
 * between the two. bench.py marks expand | kernel | end of a step and reads both intervals after the step's own sync. */
int hvd_timer_mark(int slot);
int hvd_timer_between(int slot_a, int slot_b, float* out_ms);

/* ----------------------------------------------- multi-GPU exchange ------ */
/* One process per GPU; rank 0 creates the id, the caller's control channel hands it to the other ranks
 * (hvd_amd.rendezvous: a loopback TCP star -- no torch; bench.py and hvd_amd.multigpu.connect_rccl use it),
 * every rank calls hvd_comm_init (collective). */
int hvd_comm_unique_id(uint8_t out_id[HVD_UNIQUE_ID_BYTES]);
int hvd_comm_init(const uint8_t id[HVD_UNIQUE_ID_BYTES], int rank, int world);
/* RCCL all-gather over xGMI of each rank's candidate pairs: counts first, then the
 * records padded to the max count. Every rank receives the concatenation (rank
 * order) in out_host[cap]; *out_total is the total number of records. */
int hvd_comm_allgather_pairs(const void* d_pairs, int64_t count, hvd_pair* out_host, int64_t cap, int64_t* out_total);
/* RCCL all-gather of equally sized device buffers (hash shards produced on-device). */
int hvd_comm_allgather_bytes(const void* d_send, void* d_recv, size_t bytes_per_rank);
int hvd_comm_destroy(void);
/* Tear the communicator down WITHOUT the collective handshake of ncclCommDestroy: for a rank whose own
 * hvd_comm_init succeeded while another rank's failed or timed out (hvd_amd.multigpu.connect_rccl) -- the
 * half-formed communicator must neither be used nor destroyed normally. Idempotent. */
int hvd_comm_abort(void);

#ifdef __cplusplus
}
#endif
#endif /* HVD_MI355X_H */
