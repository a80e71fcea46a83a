"""Numpy restatement of the rate-aware alignment rule (include/hvd_mi355x.h: hvd_vpdq_align_rates), on
align_helpers.hamming_matrix, and a generator of resampled clips. The reference of tests/test_rates_cpu.py and
tests/test_gpu_rates.py; nothing here touches the device."""
from math import gcd

import numpy as np

import align_helpers as AH

VRATE_FIELDS = AH.VALIGN_FIELDS + ("rate_num", "rate_den", "rate_index", "reserved")
VRATE_DTYPE = np.dtype(AH.VALIGN_DTYPE.descr + [("rate_num", "<u4"), ("rate_den", "<u4"), ("rate_index", "<u4"),
                                                ("reserved", "<u4")])
INT32_MIN = AH.INT32_MIN
MAX_RATES = 8
MAX_BINS = 1 << 20
# the issue's nine; the product's default is the first eight (tests/test_rates_cpu.py checks that)
NINE_RATES = ((1, 1), (5, 4), (4, 5), (4, 3), (3, 4), (3, 2), (2, 3), (2, 1), (1, 2))
DEFAULT_RATES = NINE_RATES[:MAX_RATES]
PLANTED_RATES = ((5, 4), (4, 5), (4, 3), (3, 2), (2, 1), (1, 2), (1, 1))
ZERO = (0,) * 14
LOST = (0, 0, INT32_MIN) + (0,) * 11


def sound(rates) -> bool:
    """1..8 pairs (num, den) with 1 <= num, den <= 8 in lowest terms, pairwise distinct."""
    rates = [tuple(int(x) for x in r) for r in rates]
    return (1 <= len(rates) <= MAX_RATES and all(len(r) == 2 and 1 <= r[0] <= 8 and 1 <= r[1] <= 8 and gcd(*r) == 1 for r in rates)
            and len(set(rates)) == len(rates))


def best_band(delta: np.ndarray, slack: int) -> tuple:
    """(d*, S(d*)) of the deltas of the hit set: the largest windowed sum, ties by larger votes[d], smaller |d|, smaller d."""
    lo = int(delta.min()) - slack
    votes = np.bincount(delta - lo, minlength=int(delta.max()) + slack - lo + 1).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(np.concatenate([np.zeros(slack, np.int64), votes, np.zeros(slack, np.int64)]))])
    S = csum[2 * slack + 1:] - csum[:-(2 * slack + 1)]
    d = np.arange(votes.size, dtype=np.int64) + lo
    best = np.lexsort((d, np.abs(d), -votes, -S))[0]
    return int(d[best]), int(S[best])


def rates_pair(A, B, pa=None, pb=None, max_dist=31, slack=1, rates=DEFAULT_RATES) -> tuple:
    """The fourteen words after (a, b) of one record. The list is taken as it is (any length): the rule alone."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    na, nb = A.shape[0], B.shape[0]
    if na == 0 or nb == 0:
        return ZERO
    pa = np.arange(na, dtype=np.int64) if pa is None else np.asarray(pa, dtype=np.int64)
    pb = np.arange(nb, dtype=np.int64) if pb is None else np.asarray(pb, dtype=np.int64)
    assert pa.shape == (na,) and pb.shape == (nb,)
    for num, den in rates:  # bins_r of every listed rate, hit or no hit
        if num * int(pa[-1] - pa[0]) + den * int(pb[-1] - pb[0]) + 1 + 2 * slack * max(num, den) > MAX_BINS:
            return LOST
    i, j = np.nonzero(AH.hamming_matrix(A, B) <= max_dist)
    if i.size == 0:
        return ZERO
    win = None
    for r, (num, den) in enumerate(rates):
        delta = den * pb[j] - num * pa[i]
        d, S = best_band(delta, slack * max(num, den))
        if win is None or S > win[1]:  # ties go to the earlier rate
            win = (d, S, r, delta)
    d, S, r, delta = win
    num, den = rates[r]
    on = np.abs(delta - d) <= slack * max(num, den)
    qa, ta = np.unique(i[on]), np.unique(j[on])
    return (np.unique(i).size, np.unique(j).size, d, S, qa.size, ta.size, int(pa[qa].min()), int(pa[qa].max()),
            int(pb[ta].min()), int(pb[ta].max()), int(num), int(den), r, 0)


def align_rates(frames, offsets, pairs, positions=None, rates=DEFAULT_RATES, slack=1, max_dist=31, frames_t=None,
                offsets_t=None, positions_t=None) -> np.ndarray:
    """Reference of search.align_rates and of the device entry: VRATE_DTYPE records in the order of the pair list. A pair
    index out of range, and every pair under a broken list, is the INT32_MIN record."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, dtype=np.int64)
    if frames_t is None:
        frames_t, offsets_t, positions_t = frames, offsets, positions
    frames_t = np.asarray(frames_t, dtype=np.uint8).reshape(-1, 32)
    offsets_t = np.asarray(offsets_t, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rates = [tuple(int(x) for x in r) for r in rates]
    out = np.zeros(pairs.shape[0], dtype=VRATE_DTYPE)
    for k, (a, b) in enumerate(pairs):
        if not sound(rates) or a >= offsets.size - 1 or b >= offsets_t.size - 1:
            out[k] = (a, b) + LOST
            continue
        sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets_t[b], offsets_t[b + 1])
        out[k] = (a, b) + rates_pair(frames[sa], frames_t[sb], None if positions is None else np.asarray(positions)[sa],
                                     None if positions_t is None else np.asarray(positions_t)[sb], max_dist, slack, rates)
    return out


class ReferenceMatcher:
    """match_videos / align_videos / align_rates on the reference: what search.rate_excerpt_pairs takes as `matcher`."""
    match_videos = AH.ReferenceMatcher.match_videos
    align_videos = staticmethod(AH.align_videos)
    align_rates = staticmethod(align_rates)


def resampled(source: np.ndarray, n: int, num: int, den: int, c: float) -> np.ndarray:
    """n frames of `source` at rate num / den: frame t is source[round(t num / den + c)]. As video a against the source as b
    this is rate (num, den): p_b = (num / den) p_a + c."""
    idx = np.floor(np.arange(n) * num / den + c + 0.5).astype(np.int64)
    assert idx[0] >= 0 and idx[-1] < len(source)
    return source[idx].copy()


def planted_clips(seed=70, n_source=600, n=60, c=100.3, max_flips=0):
    """(source, {rate: clip}): a source of independent random hashes and one n-frame clip per rate of PLANTED_RATES."""
    rng = np.random.default_rng(seed)
    source = rng.integers(0, 256, (n_source, 32), dtype=np.uint8)
    clips = {r: resampled(source, n, r[0], r[1], c) for r in PLANTED_RATES}
    if max_flips:
        clips = {r: AH.noisy(rng, v, max_flips) for r, v in clips.items()}
    return source, clips


def _rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def list_with(rate):
    """The default list, its last entry given up for `rate` if that is not on it (the list holds eight)."""
    return DEFAULT_RATES if rate in DEFAULT_RATES else DEFAULT_RATES[:-1] + (rate,)


def mixed_library(seed):
    """Planted clips at several rates in both orientations, a 1x excerpt, a shuffle, a static pair, noise, an empty video."""
    rng = np.random.default_rng(seed)
    L1, L2 = _rand(rng, 180), _rand(rng, 140)
    h = _rand(rng, 1)
    vids = [L1, AH.noisy(rng, resampled(L1, 40, 5, 4, 20.3), 20), AH.noisy(rng, resampled(L1, 40, 2, 3, 90.6), 20),
            L2, AH.noisy(rng, resampled(L2, 30, 3, 2, 11.2), 20), AH.noisy(rng, L2[40:75], 20),
            AH.noisy(rng, L1[rng.permutation(180)[:40]], 20), np.repeat(h, 20, axis=0), np.repeat(h, 33, axis=0), _rand(rng, 25),
            np.zeros((0, 32), np.uint8), AH.noisy(rng, resampled(L2, 64, 2, 1, 3.0), 20)]
    return vids


def join(videos):
    off = np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int64)
    fr = np.concatenate(videos) if len(videos) else np.zeros((0, 32), np.uint8)
    return np.ascontiguousarray(fr, dtype=np.uint8), off
