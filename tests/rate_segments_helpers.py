"""Numpy restatement of the rate-aware multi-segment alignment rule (include/hvd_mi355x.h: hvd_vpdq_align_rate_segments; DESIGN
4.18): the peel loop of segments_helpers.segments_of_pair with rates_helpers.best_band asked at every listed rate in every
round -- no rate is ever passed over, which is what the kernel's bound-skip is compared with. The reference of
tests/test_rate_segments_cpu.py and tests/test_gpu_rate_segments.py; nothing here touches the device."""
import numpy as np

import align_helpers as AH
import rates_helpers as RH
import segments_helpers as SH

MAX_SEGMENTS = SH.MAX_SEGMENTS
INT32_MIN = AH.INT32_MIN
VRSEGMENT_DTYPE = np.dtype(SH.VSEGMENT_DTYPE.descr + [("rate_num", "<u4"), ("rate_den", "<u4"), ("rate_index", "<u4"),
                                                      ("reserved", "<u4")])
VRSEGMENTS_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4"), ("n_segments", "<u4"),
                             ("q_covered", "<u4"), ("t_covered", "<u4"), ("reserved", "<u4"),
                             ("seg", VRSEGMENT_DTYPE, (MAX_SEGMENTS,))])
LOST = "lost"


def rate_segments_pair(A, B, pa=None, pb=None, max_dist=31, slack=1, rates=RH.DEFAULT_RATES, max_segments=MAX_SEGMENTS,
                       min_band_votes=1):
    """(q_hits, t_hits, [segment, ...]) of one pair, or LOST when a listed rate needs more than 2^20 bins; a segment is the
    twelve words offset, band_votes, q_aligned, t_aligned, q_first, q_last, t_first, t_last, rate_num, rate_den, rate_index, 0.
    The list is taken as it is: the rule alone."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    na, nb = A.shape[0], B.shape[0]
    if na == 0 or nb == 0:
        return 0, 0, []
    pa = np.arange(na, dtype=np.int64) if pa is None else np.asarray(pa, dtype=np.int64)
    pb = np.arange(nb, dtype=np.int64) if pb is None else np.asarray(pb, dtype=np.int64)
    assert pa.shape == (na,) and pb.shape == (nb,) and 1 <= max_segments <= MAX_SEGMENTS and min_band_votes >= 1
    for num, den in rates:  # bins_r of every listed rate, hit or no hit
        if num * int(pa[-1] - pa[0]) + den * int(pb[-1] - pb[0]) + 1 + 2 * slack * max(num, den) > RH.MAX_BINS:
            return LOST
    hit = AH.hamming_matrix(A, B) <= max_dist
    q_hits, t_hits = int(hit.any(1).sum()), int(hit.any(0).sum())
    taken_a, taken_b = np.zeros(na, bool), np.zeros(nb, bool)
    segs = []
    for _ in range(max_segments):
        i, j = np.nonzero(hit & ~taken_a[:, None] & ~taken_b[None, :])  # H_s
        if i.size == 0:
            break
        win = None
        for r, (num, den) in enumerate(rates):  # every rate, every round
            delta = den * pb[j] - num * pa[i]
            d, S = RH.best_band(delta, slack * max(num, den))
            if win is None or S > win[1]:  # ties go to the earlier rate
                win = (d, S, r, delta)
        d, S, r, delta = win
        if S < min_band_votes:
            break
        num, den = rates[r]
        on = np.abs(delta - d) <= slack * max(num, den)
        qa, ta = np.unique(i[on]), np.unique(j[on])
        segs.append((d, S, qa.size, ta.size, int(pa[qa].min()), int(pa[qa].max()), int(pb[ta].min()), int(pb[ta].max()),
                     int(num), int(den), r, 0))
        taken_a[qa] = True
        taken_b[ta] = True
    return q_hits, t_hits, segs


def record(a, b, q_hits, t_hits, segs) -> np.ndarray:
    """One VRSEGMENTS_DTYPE record from the pair's counters and its list of segments."""
    rec = np.zeros((), dtype=VRSEGMENTS_DTYPE)
    rec["a"], rec["b"], rec["q_hits"], rec["t_hits"], rec["n_segments"] = a, b, q_hits, t_hits, len(segs)
    rec["q_covered"], rec["t_covered"] = sum(s[2] for s in segs), sum(s[3] for s in segs)
    for k, s in enumerate(segs):
        rec["seg"][k] = s
    return rec


def lost_record(a, b) -> np.ndarray:
    """The record of a pair the device entry cannot align."""
    rec = np.zeros((), dtype=VRSEGMENTS_DTYPE)
    rec["a"], rec["b"] = a, b
    rec["seg"][0]["offset"] = INT32_MIN
    return rec


def align_rate_segments(frames, offsets, pairs, positions=None, rates=RH.DEFAULT_RATES, slack=1, max_dist=31, frames_t=None,
                        offsets_t=None, positions_t=None, max_segments=MAX_SEGMENTS, min_band_votes=1) -> np.ndarray:
    """Reference of search.align_rate_segments and of the device entry: VRSEGMENTS_DTYPE records in the order of the pair
    list. A pair index out of range, and every pair under a broken list, is the INT32_MIN record."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, dtype=np.int64)
    if frames_t is None:
        frames_t, offsets_t, positions_t = frames, offsets, positions
    frames_t = np.asarray(frames_t, dtype=np.uint8).reshape(-1, 32)
    offsets_t = np.asarray(offsets_t, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rates = [tuple(int(x) for x in r) for r in rates]
    out = np.zeros(pairs.shape[0], dtype=VRSEGMENTS_DTYPE)
    for k, (a, b) in enumerate(pairs):
        if not RH.sound(rates) or a >= offsets.size - 1 or b >= offsets_t.size - 1:
            out[k] = lost_record(a, b)
            continue
        sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets_t[b], offsets_t[b + 1])
        got = rate_segments_pair(frames[sa], frames_t[sb], None if positions is None else np.asarray(positions)[sa],
                                 None if positions_t is None else np.asarray(positions_t)[sb], max_dist, slack, rates,
                                 max_segments, min_band_votes)
        out[k] = lost_record(a, b) if got is LOST else record(a, b, *got)
    return out


class ReferenceMatcher(SH.ReferenceMatcher):
    """match_videos / align_videos / align_segments / align_rates / align_rate_segments on the reference: what
    search.rate_segmented_excerpt_pairs takes as `matcher`."""

    align_rates = staticmethod(RH.align_rates)
    align_rate_segments = staticmethod(align_rate_segments)


def same(got, want):
    assert got.dtype == VRSEGMENTS_DTYPE and got.shape == want.shape
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(k, got[k].tolist(), want[k].tolist()) for k in bad[:3]]


# ---- the reels of the issue: pieces of one source, each at its own rate ----

REEL_B = ((40, 3, 2, 300.3), (30, 2, 1, 50.6), (20, 1, 1, 500.0), (60, 5, 4, 400.2))  # (frames, num, den, c) per piece
REEL_C = ((30, 2, 1, 300.3), (30, 2, 1, 50.6), (30, 2, 1, 180.2))


def reel(seed, pieces, n_source=600, max_flips=20):
    """(source, reel): a source of independent random hashes and the pieces, resampled from it one after the other, up to
    max_flips bits flipped per frame. As video a against the source as b, piece (n, num, den, c) lies on rate (num, den)."""
    rng = np.random.default_rng(seed)
    source = RH._rand(rng, n_source)
    cut = np.concatenate([RH.resampled(source, n, num, den, c) for n, num, den, c in pieces])
    return source, AH.noisy(rng, cut, max_flips)


def reel_b():
    return reel(91, REEL_B)


def reel_c():
    return reel(92, REEL_C)
