"""Numpy restatement of the time alignment with negative rates (include/hvd_mi355x.h: hvd_vpdq_align_signed):
rate_segments_helpers.rate_segments_pair with |num| in the bins and in the slack -- the peel loop with rates_helpers.best_band
asked at every listed rate in every round, no rate ever passed over. The reference of tests/test_signed_cpu.py and
tests/test_gpu_signed.py; nothing here touches the device."""
from math import gcd

import numpy as np

import align_helpers as AH
import rate_segments_helpers as RS
import rates_helpers as RH
import segments_helpers as SH

MAX_SEGMENTS = SH.MAX_SEGMENTS
INT32_MIN = AH.INT32_MIN
VSSEGMENT_DTYPE = np.dtype(SH.VSEGMENT_DTYPE.descr + [("rate_num", "<i4"), ("rate_den", "<u4"), ("rate_index", "<u4"),
                                                      ("reserved", "<u4")])
VSSEGMENTS_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4"), ("n_segments", "<u4"),
                             ("q_covered", "<u4"), ("t_covered", "<u4"), ("reserved", "<u4"),
                             ("seg", VSSEGMENT_DTYPE, (MAX_SEGMENTS,))])
LOST = RS.LOST
REVERSED_RATES = ((1, 1), (-1, 1))
FOUR_RATES = ((1, 1), (-1, 1), (2, 1), (-2, 1))
# every legal magnitude that needs the top bit of a nibble, on either side, with the signs mixed
WIDE_SIGNED = ((1, 1), (8, 7), (-7, 8), (-8, 3), (5, 8), (-1, 8), (7, 2), (-8, 1))
BROKEN_LISTS = (((-1, 1), (-1, 1)), ((-2, 2),), ((0, 1),), ((1, -1),), ((-9, 1),), REVERSED_RATES + RH.NINE_RATES[2:9], ())


def sound_signed(rates) -> bool:
    """1..8 pairs (num, den) with 1 <= |num| <= 8, 1 <= den <= 8, gcd(|num|, den) = 1, pairwise distinct as signed pairs."""
    rates = [tuple(int(x) for x in r) for r in rates]
    return (1 <= len(rates) <= RH.MAX_RATES
            and all(len(r) == 2 and 1 <= abs(r[0]) <= 8 and 1 <= r[1] <= 8 and gcd(abs(r[0]), r[1]) == 1 for r in rates)
            and len(set(rates)) == len(rates))


def bins_of(span_a, span_b, rates, slack) -> int:
    """The largest bins_r of a pair."""
    return max(abs(n) * span_a + d * span_b + 1 + 2 * slack * max(abs(n), d) for n, d in rates)


def signed_pair(A, B, pa=None, pb=None, max_dist=31, slack=1, rates=REVERSED_RATES, max_segments=MAX_SEGMENTS, min_band_votes=1):
    """(q_hits, t_hits, [segment, ...]) of one pair, or LOST when a listed rate needs more than 2^20 bins; a segment is the
    twelve words offset, band_votes, q_aligned, t_aligned, q_first, q_last, t_first, t_last, rate_num (signed), rate_den,
    rate_index, 0. The list is taken as it is: the rule alone."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    na, nb = A.shape[0], B.shape[0]
    if na == 0 or nb == 0:
        return 0, 0, []
    pa = np.arange(na, dtype=np.int64) if pa is None else np.asarray(pa, dtype=np.int64)
    pb = np.arange(nb, dtype=np.int64) if pb is None else np.asarray(pb, dtype=np.int64)
    assert pa.shape == (na,) and pb.shape == (nb,) and 1 <= max_segments <= MAX_SEGMENTS and min_band_votes >= 1
    if bins_of(int(pa[-1] - pa[0]), int(pb[-1] - pb[0]), rates, slack) > RH.MAX_BINS:  # bins_r of every listed rate, hit or no hit
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
            d, S = RH.best_band(delta, slack * max(abs(num), den))
            if win is None or S > win[1]:  # ties go to the earlier rate
                win = (d, S, r, delta)
        d, S, r, delta = win
        if S < min_band_votes:
            break
        num, den = rates[r]
        on = np.abs(delta - d) <= slack * max(abs(num), den)
        qa, ta = np.unique(i[on]), np.unique(j[on])
        segs.append((d, S, qa.size, ta.size, int(pa[qa].min()), int(pa[qa].max()), int(pb[ta].min()), int(pb[ta].max()),
                     int(num), int(den), r, 0))
        taken_a[qa] = True
        taken_b[ta] = True
    return q_hits, t_hits, segs


def no_tie_on_d(A, B, max_dist=31, slack=1, rates=REVERSED_RATES, max_segments=MAX_SEGMENTS, min_band_votes=1) -> bool:
    """True iff in every round of the pair (index positions) the winning rate's largest (S, votes[d]) is reached by one d alone:
    the tie order then never gets as far as |d|, which a reflection of a's timeline changes (as rates_helpers.non_tying picks
    the pairs on which reordering a list changes nothing)."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    hit = AH.hamming_matrix(A, B) <= max_dist
    taken_a, taken_b = np.zeros(len(A), bool), np.zeros(len(B), bool)
    for _ in range(max_segments):
        i, j = np.nonzero(hit & ~taken_a[:, None] & ~taken_b[None, :])
        if i.size == 0:
            return True
        tops = []
        for num, den in rates:
            delta = den * j - num * i
            w = slack * max(abs(num), den)
            lo = int(delta.min()) - w
            votes = np.bincount(delta - lo, minlength=int(delta.max()) + w - lo + 1).astype(np.int64)
            S = np.convolve(votes, np.ones(2 * w + 1, np.int64), "same")
            key = S * (i.size + 1) + votes
            tops.append((int(S.max()), int((key == key.max()).sum()), delta, int(lo + key.argmax()), w))
        best = max(t[0] for t in tops)
        if best < min_band_votes:
            return True
        _, n_top, delta, d, w = next(t for t in tops if t[0] == best)
        if n_top != 1:
            return False
        on = np.abs(delta - d) <= w
        taken_a[np.unique(i[on])] = True
        taken_b[np.unique(j[on])] = True
    return True


def record(a, b, q_hits, t_hits, segs) -> np.ndarray:
    """One VSSEGMENTS_DTYPE record from the pair's counters and its list of segments."""
    rec = np.zeros((), dtype=VSSEGMENTS_DTYPE)
    rec["a"], rec["b"], rec["q_hits"], rec["t_hits"], rec["n_segments"] = a, b, q_hits, t_hits, len(segs)
    rec["q_covered"], rec["t_covered"] = sum(s[2] for s in segs), sum(s[3] for s in segs)
    for k, s in enumerate(segs):
        rec["seg"][k] = s
    return rec


def lost_record(a, b) -> np.ndarray:
    """The record of a pair the device entry cannot align."""
    rec = np.zeros((), dtype=VSSEGMENTS_DTYPE)
    rec["a"], rec["b"] = a, b
    rec["seg"][0]["offset"] = INT32_MIN
    return rec


def align_signed(frames, offsets, pairs, positions=None, rates=REVERSED_RATES, slack=1, max_dist=31, frames_t=None,
                 offsets_t=None, positions_t=None, max_segments=MAX_SEGMENTS, min_band_votes=1) -> np.ndarray:
    """Reference of search.align_signed and of the device entry: VSSEGMENTS_DTYPE records in the order of the pair list. A
    pair index out of range, and every pair under a broken list, is the INT32_MIN record."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, dtype=np.int64)
    if frames_t is None:
        frames_t, offsets_t, positions_t = frames, offsets, positions
    frames_t = np.asarray(frames_t, dtype=np.uint8).reshape(-1, 32)
    offsets_t = np.asarray(offsets_t, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rates = [tuple(int(x) for x in r) for r in rates]
    out = np.zeros(pairs.shape[0], dtype=VSSEGMENTS_DTYPE)
    for k, (a, b) in enumerate(pairs):
        if not sound_signed(rates) or a >= offsets.size - 1 or b >= offsets_t.size - 1:
            out[k] = lost_record(a, b)
            continue
        sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets_t[b], offsets_t[b + 1])
        got = signed_pair(frames[sa], frames_t[sb], None if positions is None else np.asarray(positions)[sa],
                          None if positions_t is None else np.asarray(positions_t)[sb], max_dist, slack, rates, max_segments,
                          min_band_votes)
        out[k] = lost_record(a, b) if got is LOST else record(a, b, *got)
    return out


def restated(frames, offsets, pairs, *args, **kwargs):
    """align_signed, computed once per distinct pair of the list."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    return align_signed(frames, offsets, uniq, *args, **kwargs)[inv.reshape(-1)]


class ReferenceMatcher(RS.ReferenceMatcher):
    """match_videos / align_* on the reference, align_signed among them: what search.signed_excerpt_pairs takes as `matcher`."""

    align_signed = staticmethod(align_signed)


def same(got, want):
    assert got.dtype == VSSEGMENTS_DTYPE and got.shape == want.shape
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(k, got[k].tolist(), want[k].tolist()) for k in bad[:3]]


def same_words(got, want):
    """Records of VSSEGMENTS_DTYPE and of VRSEGMENTS_DTYPE, word for word."""
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize == 416
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---- the table of the issue: clips of one 600-frame source (seed 70), up to 20 bits flipped per frame ----

def reversed_at(source, n, num, den, c):
    """n frames of `source`: frame t is source[round(c - t num / den)] -- backwards at rate num / den from c."""
    idx = np.floor(c - np.arange(n) * num / den + 0.5).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < len(source)
    return source[idx].copy()


_table = {}


def table():
    """{name: video}, built in the table's order: the source; `rev` = frames 100..159 reversed; `rev32` = 40 frames,
    frame t = source[round(300.3 - 1.5 t)]; `reel` = 50..89 forward, 400..439 reversed, 30 frames reversed at 2x from 299.6;
    then `shuffled` = 60 frames of 100..159 in shuffled order. Computed once per process; the arrays are read-only."""
    if not _table:
        rng = np.random.default_rng(70)
        source = RH._rand(rng, 600)
        _table["source"] = source
        _table["rev"] = AH.noisy(rng, source[100:160][::-1], 20)
        _table["rev32"] = AH.noisy(rng, reversed_at(source, 40, 3, 2, 300.3), 20)
        _table["reel"] = AH.noisy(rng, np.concatenate([source[50:90], source[400:440][::-1], reversed_at(source, 30, 2, 1, 299.6)]), 20)
        _table["shuffled"] = AH.noisy(rng, source[100 + rng.permutation(60)], 20)
        for v in _table.values():
            v.setflags(write=False)
    return _table


LIST_32 = RH.DEFAULT_RATES[:7] + ((-3, 2),)  # (-3, 2) in the 8th place


def table_library():
    """(frames, offsets, pairs): videos 0..4 = source, rev, rev32, reel, shuffled; every clip against the source, both ways."""
    t = table()
    frames, offsets = RH.join([t["source"], t["rev"], t["rev32"], t["reel"], t["shuffled"]])
    return frames, offsets, [(1, 0), (0, 1), (2, 0), (0, 2), (3, 0), (0, 3), (4, 0), (0, 4)]


def flipped(rates):
    """Every num negated."""
    return tuple((-n, d) for n, d in rates)


def planted_signed(seed, n_source=300, clip=36):
    """(videos, pairs): video 0 a source of n_source random hashes; one clip per rate of WIDE_SIGNED, forward from a small c
    or backwards from a large one, up to 20 bits flipped per frame; a static pair; 9 random frames; no frame. Pairs: every
    clip against the source in both orientations, the static pair both ways, the random and the empty video."""
    rng = np.random.default_rng(seed)
    source = RH._rand(rng, n_source)
    h = RH._rand(rng, 1)
    vids = [source]
    for k, (num, den) in enumerate(WIDE_SIGNED):
        v = RH.resampled(source, clip, num, den, 3.3 + 1.7 * k) if num > 0 else reversed_at(source, clip, -num, den,
                                                                                          n_source - 4.4 - 1.7 * k)
        vids.append(AH.noisy(rng, v, 20))
    vids += [np.repeat(h, 7, axis=0), np.repeat(h, 12, axis=0), RH._rand(rng, 9), np.zeros((0, 32), np.uint8)]
    pairs = [(v, 0) for v in range(1, 9)] + [(0, v) for v in range(1, 9)] + [(9, 10), (10, 9), (11, 0), (12, 0)]
    return vids, pairs
