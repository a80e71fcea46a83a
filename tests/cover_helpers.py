"""Numpy restatement of the cover rule (include/hvd_mi355x.h: hvd_vpdq_cover_videos) on top of
tests/align_helpers.py: per pair the hit matrix and the band are recomputed, the aligned frame sets are checked against
align_pair's counts, and the sets that reach min_aligned are united per video. The reference of tests/test_cover_cpu.py and
tests/test_gpu_cover.py; nothing here touches the device."""
import numpy as np

import align_helpers as AH

VCOVER_DTYPE = np.dtype([("covered", "<u4"), ("sources", "<u4"), ("best_single", "<u4"), ("frames", "<u4")])
INT32_MIN = AH.INT32_MIN


def aligned_sets(A, B, pa=None, pb=None, max_dist=31, slack=1):
    """(the ten words of align_pair, on_a, on_b): the frame indices of A and of B with a hit within slack of the best offset."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    words = AH.align_pair(A, B, pa, pb, max_dist, slack)
    none = np.zeros(0, np.int64)
    if len(A) == 0 or len(B) == 0 or words[0] == 0:
        return words, none, none
    pa = np.arange(len(A), dtype=np.int64) if pa is None else np.asarray(pa, dtype=np.int64)
    pb = np.arange(len(B), dtype=np.int64) if pb is None else np.asarray(pb, dtype=np.int64)
    i, j = np.nonzero(AH.hamming_matrix(A, B) <= max_dist)
    on = np.abs(pb[j] - pa[i] - words[2]) <= slack
    on_a, on_b = np.unique(i[on]), np.unique(j[on])
    assert (on_a.size, on_b.size) == (words[4], words[5])  # the sets whose sizes are q_aligned / t_aligned
    return words, on_a, on_b


def cover_videos(frames, offsets, pairs, positions=None, max_dist=31, slack=1, min_aligned=4, lost=()):
    """Reference of search.cover_videos: (VALIGN_DTYPE records in the order of the pair list, VCOVER_DTYPE records per video).
    A pair index outside the library gives the INT32_MIN record, as the device entry does; lost: list entries the caller
    knows the device entry cannot align (no room in the scratch) -- the INT32_MIN record, no contribution. The rule runs once
    per distinct pair; `sources` counts list entries."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    V = offsets.size - 1
    aligned = np.zeros(pairs.shape[0], dtype=AH.VALIGN_DTYPE)
    cover = np.zeros(V, dtype=VCOVER_DTYPE)
    cover["frames"] = np.diff(offsets)
    union = [np.zeros(int(n), bool) for n in np.diff(offsets)]
    seen = {}
    for k, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if a >= V or b >= V or k in lost:
            aligned[k] = (a, b, 0, 0, INT32_MIN, 0, 0, 0, 0, 0, 0, 0)
            continue
        if (a, b) not in seen:
            sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets[b], offsets[b + 1])
            seen[a, b] = aligned_sets(frames[sa], frames[sb], None if positions is None else np.asarray(positions)[sa],
                                      None if positions is None else np.asarray(positions)[sb], max_dist, slack)
        words, on_a, on_b = seen[a, b]
        aligned[k] = (a, b) + tuple(words)
        if a == b:
            continue
        for v, on in ((a, on_a), (b, on_b)):
            if on.size >= min_aligned:
                union[v][on] = True
                cover[v]["sources"] += 1
                cover[v]["best_single"] = max(int(cover[v]["best_single"]), on.size)
    cover["covered"] = [int(u.sum()) for u in union]
    return aligned, cover


class ReferenceMatcher:
    """match_videos / cover_videos on the reference: what search.compilation_pairs takes as `matcher` (no device)."""

    match_videos = staticmethod(AH.ReferenceMatcher.match_videos)
    cover_videos = staticmethod(cover_videos)


BASE_LENGTHS = (33, 31, 60, 1, 65, 40, 30, 30)
BASE_PAIRS = [(0, 2), (1, 2), (2, 4), (5, 6), (5, 7), (6, 7)]
# by hand: video 2 = three clips of 20 frames; 6 and 7 overlap on frames 10..29 of video 5 and are each held whole by it
BASE_COVER = dict(covered=(20, 20, 60, 0, 20, 40, 30, 30), sources=(1, 1, 3, 0, 1, 2, 2, 2), best_single=(20, 20, 20, 0, 20, 30, 30, 30))


def base_case(seed=230):
    """Eight videos at offsets 0, 33, 64, 124, 125, 190, 230, 260, 290 -- all but 64 off the bitmap's word boundaries: video 2 is frames 5..24 of
    video 0, then 11..30 of video 1, then 40..59 of video 4 (a compilation); videos 6 and 7 are frames 0..29 and 10..39 of
    video 5 (two overlapping parts); video 3 is one unrelated frame, one bit between two covered videos inside one bitmap
    word. Random 256-bit hashes, copies with at most 8 flipped bits a frame. -> list of uint8[n, 32]."""
    rng = np.random.default_rng(seed)
    vids = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in BASE_LENGTHS]
    vids[2] = np.concatenate([AH.noisy(rng, vids[0][5:25], 8), AH.noisy(rng, vids[1][11:31], 8), AH.noisy(rng, vids[4][40:60], 8)])
    vids[6] = AH.noisy(rng, vids[5][0:30], 8)
    vids[7] = AH.noisy(rng, vids[5][10:40], 8)
    return vids


def join(videos):
    off = np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int64)
    fr = np.concatenate(videos) if len(videos) else np.zeros((0, 32), np.uint8)
    return np.ascontiguousarray(fr, dtype=np.uint8).reshape(-1, 32), off
