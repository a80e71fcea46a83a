"""Numpy restatement of the multi-segment alignment rule (include/hvd_mi355x.h: hvd_vpdq_align_segments), on top of
tests/align_helpers.py: the single-offset rule applied to the hit matrix with the taken rows and columns struck out, round
after round. The reference of tests/test_segments_cpu.py and tests/test_gpu_segments.py; nothing here touches the device."""
import numpy as np

import align_helpers as AH

MAX_SEGMENTS = 8
VSEGMENT_DTYPE = np.dtype([("offset", "<i4"), ("band_votes", "<u4"), ("q_aligned", "<u4"), ("t_aligned", "<u4"),
                           ("q_first", "<i4"), ("q_last", "<i4"), ("t_first", "<i4"), ("t_last", "<i4")])
VSEGMENTS_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4"), ("n_segments", "<u4"),
                            ("q_covered", "<u4"), ("t_covered", "<u4"), ("reserved", "<u4"),
                            ("seg", VSEGMENT_DTYPE, (MAX_SEGMENTS,))])
INT32_MIN = AH.INT32_MIN


def segments_of_pair(A, B, pa=None, pb=None, max_dist=31, slack=1, max_segments=MAX_SEGMENTS, min_band_votes=1) -> tuple:
    """(q_hits, t_hits, [segment, ...]) of one pair; a segment is the eight words offset, band_votes, q_aligned, t_aligned,
    q_first, q_last, t_first, t_last."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    na, nb = A.shape[0], B.shape[0]
    if na == 0 or nb == 0:
        return 0, 0, []
    pa = np.arange(na, dtype=np.int64) if pa is None else np.asarray(pa, dtype=np.int64)
    pb = np.arange(nb, dtype=np.int64) if pb is None else np.asarray(pb, dtype=np.int64)
    assert pa.shape == (na,) and pb.shape == (nb,) and 1 <= max_segments <= MAX_SEGMENTS and min_band_votes >= 1
    hit = AH.hamming_matrix(A, B) <= max_dist
    q_hits, t_hits = int(hit.any(1).sum()), int(hit.any(0).sum())
    taken_a, taken_b = np.zeros(na, bool), np.zeros(nb, bool)
    segs = []
    for _ in range(max_segments):
        left = hit & ~taken_a[:, None] & ~taken_b[None, :]  # H_r
        i, j = np.nonzero(left)
        if i.size == 0:
            break
        delta = pb[j] - pa[i]
        lo = int(delta.min()) - slack
        votes = np.bincount(delta - lo, minlength=int(delta.max()) + slack - lo + 1).astype(np.int64)
        padded = np.concatenate([np.zeros(slack, np.int64), votes, np.zeros(slack, np.int64)])
        csum = np.concatenate([[0], np.cumsum(padded)])
        S = csum[2 * slack + 1:] - csum[:-(2 * slack + 1)]  # S[k] = sum of votes[k - slack .. k + slack]
        d = np.arange(votes.size, dtype=np.int64) + lo
        best = np.lexsort((d, np.abs(d), -votes, -S))[0]  # largest S, then largest votes, then smallest |d|, then smallest d
        if int(S[best]) < min_band_votes:
            break
        on = np.abs(delta - int(d[best])) <= slack
        qa, ta = np.unique(i[on]), np.unique(j[on])
        segs.append((int(d[best]), int(S[best]), qa.size, ta.size, int(pa[qa].min()), int(pa[qa].max()), int(pb[ta].min()),
                     int(pb[ta].max())))
        taken_a[qa] = True
        taken_b[ta] = True
    return q_hits, t_hits, segs


def record(a, b, q_hits, t_hits, segs) -> np.ndarray:
    """One VSEGMENTS_DTYPE record from the pair's counters and its list of segments."""
    rec = np.zeros((), dtype=VSEGMENTS_DTYPE)
    rec["a"], rec["b"], rec["q_hits"], rec["t_hits"], rec["n_segments"] = a, b, q_hits, t_hits, len(segs)
    rec["q_covered"], rec["t_covered"] = sum(s[2] for s in segs), sum(s[3] for s in segs)
    for k, s in enumerate(segs):
        rec["seg"][k] = s
    return rec


def lost_record(a, b) -> np.ndarray:
    """The record of a pair the device entry cannot align."""
    rec = np.zeros((), dtype=VSEGMENTS_DTYPE)
    rec["a"], rec["b"] = a, b
    rec["seg"][0]["offset"] = INT32_MIN
    return rec


def align_segments(frames, offsets, pairs, positions=None, max_dist=31, slack=1, frames_t=None, offsets_t=None,
                   positions_t=None, max_segments=MAX_SEGMENTS, min_band_votes=1) -> np.ndarray:
    """Reference of search.align_segments: VSEGMENTS_DTYPE records in the order of the pair list."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, dtype=np.int64)
    if frames_t is None:
        frames_t, offsets_t, positions_t = frames, offsets, positions
    frames_t = np.asarray(frames_t, dtype=np.uint8).reshape(-1, 32)
    offsets_t = np.asarray(offsets_t, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(pairs.shape[0], dtype=VSEGMENTS_DTYPE)
    for k, (a, b) in enumerate(pairs):
        sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets_t[b], offsets_t[b + 1])
        out[k] = record(a, b, *segments_of_pair(frames[sa], frames_t[sb], None if positions is None else np.asarray(positions)[sa],
                                                None if positions_t is None else np.asarray(positions_t)[sb], max_dist, slack,
                                                max_segments, min_band_votes))
    return out


def planted_pieces_library(seed, max_dist, lengths=(0, 1, 2, 3, 17, 64, 65, 130, 255, 256, 257, 300)):
    """test_gpu_align.planted_library -- ragged videos, video v holding a noisy stretch of video v - 1 with frame pairs at
    exactly max_dist and max_dist + 1 on and off that diagonal -- with one to three more noisy pieces of video v - 1 planted
    into video v at other places: two to four pieces per pair of neighbours."""
    from test_gpu_align import planted_library

    vids = planted_library(seed, max_dist, lengths)
    rng = np.random.default_rng(seed + 50000)
    for v in range(1, len(vids)):
        A, B = vids[v - 1], vids[v]
        if min(len(A), len(B)) < 8:
            continue
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(2, min(len(A), len(B)) // 6 + 2))
            ia, ib = int(rng.integers(0, len(A) - n + 1)), int(rng.integers(0, len(B) - n + 1))
            B[ib:ib + n] = AH.noisy(rng, A[ia:ia + n], min(max_dist, 24))
    return vids


def gapped(rng, offsets, max_gap=3) -> np.ndarray:
    """Positions with gaps: per video a random start and steps of 1..max_gap."""
    from test_gpu_align import gapped_positions

    return gapped_positions(rng, offsets, max_gap)


class ReferenceMatcher(AH.ReferenceMatcher):
    """match_videos / align_videos / align_segments on the reference: what search.segmented_excerpt_pairs takes as `matcher`."""

    align_segments = staticmethod(align_segments)


def same(got, want):
    assert got.dtype == VSEGMENTS_DTYPE and got.shape == want.shape
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(got[k].tolist(), want[k].tolist()) for k in bad[:3]]
