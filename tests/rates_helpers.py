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


# ---- the grid of tests/test_rates_grid_cpu.py and tests/test_gpu_rates_grid.py: rates up to 8, every tolerance and slack ----

# every legal value that needs the top bit of a nibble, on either side, and (1, 1) for the header's consequence (b)
WIDE_RATES = ((1, 1), (8, 7), (7, 8), (8, 1), (1, 8), (7, 2), (5, 8), (8, 3))
GRID = tuple((max_dist, slack) for max_dist in (0, 30, 31, 32, 127) for slack in (0, 1, 3, 16))
WIDE_CLIP = 36  # frames of a planted clip: 8 * 35 + c stays inside a 300-frame source


def rotated(rates, k):
    """The list with its first k entries moved behind the others."""
    return tuple(rates[k:]) + tuple(rates[:k])


def rate_tops(A, B, pa=None, pb=None, max_dist=31, slack=1, rates=WIDE_RATES) -> list:
    """S_r(d*_r) of every listed rate, each on its own (0 for a pair without a hit)."""
    return [rates_pair(A, B, pa, pb, max_dist, slack, (r,))[3] for r in rates]


# case 4: single rates with an 8, WIDE_RATES with (8, 1) and with (1, 8) in the eighth entry, an 8 in the first and the eighth
TOP_BIT_LISTS = (((8, 1),), ((1, 8),), ((8, 7),), ((7, 8),), rotated(WIDE_RATES, 4), rotated(WIDE_RATES, 5),
                 ((1, 8), (1, 1), (8, 7), (7, 8), (7, 2), (5, 8), (8, 3), (8, 1)))
REORDER_POINTS = ((31, 1), (127, 1), (31, 3))  # (max_dist, slack) at which at least nine pairs of wide_library(300) do not tie


def non_tying(frames, offsets, pairs, max_dist, slack, rates=WIDE_RATES) -> list:
    """Indices of the pairs with a hit whose largest S_r(d*_r) is reached by one listed rate alone (index positions)."""
    out = []
    for p, (a, b) in enumerate(pairs):
        tops = rate_tops(frames[offsets[a]:offsets[a + 1]], frames[offsets[b]:offsets[b + 1]], None, None, max_dist, slack, rates)
        if max(tops) > 0 and tops.count(max(tops)) == 1:
            out.append(p)
    return out


def wide_library(n_source, seed):
    """(videos, pairs). Video 0: a source of n_source independent random hashes; 1..8: one WIDE_CLIP-frame clip per rate of
    WIDE_RATES, source index round(t num / den + c), up to 20 bits flipped per frame; 9, 10: 7 and 12 frames of one hash; 11:
    9 random frames; 12: no frame. Pairs: every clip against the source in both orientations, the static pair in both
    orientations, the 8/7 clip against the 1x clip (which it runs through at 8/7) and back, the random frames and the empty
    video against the source."""
    rng = np.random.default_rng(seed)
    source = _rand(rng, n_source)
    h = _rand(rng, 1)
    vids = [source]
    for k, (num, den) in enumerate(WIDE_RATES):
        vids.append(AH.noisy(rng, resampled(source, WIDE_CLIP, num, den, 3.3 + 1.7 * k), 20))
    vids += [np.repeat(h, 7, axis=0), np.repeat(h, 12, axis=0), _rand(rng, 9), np.zeros((0, 32), np.uint8)]
    pairs = [(v, 0) for v in range(1, 9)] + [(0, v) for v in range(1, 9)] + [(9, 10), (10, 9), (2, 1), (1, 2), (11, 0), (12, 0)]
    return vids, pairs


_wide = {}


def wide_case(n_source):
    """(frames, offsets, pairs, {(max_dist, slack): the restatement's records under WIDE_RATES}) of wide_library(n_source),
    over GRID. Computed once per process and shared: the arrays are read-only."""
    if n_source not in _wide:
        vids, pairs = wide_library(n_source, 80 + n_source)
        frames, offsets = join(vids)
        want = {}
        for max_dist, slack in GRID:
            want[(max_dist, slack)] = align_rates(frames, offsets, pairs, None, WIDE_RATES, slack, max_dist)
            want[(max_dist, slack)].setflags(write=False)
        frames.setflags(write=False)
        offsets.setflags(write=False)
        _wide[n_source] = (frames, offsets, tuple(pairs), want)
    return _wide[n_source]


def wide_bins(n_source, slack, pair) -> int:
    """The largest bins_r of a pair of wide_library(n_source) under WIDE_RATES (index positions: span = length - 1)."""
    _, offsets, _, _ = wide_case(n_source)
    sa, sb = (int(offsets[v + 1] - offsets[v]) - 1 for v in pair)
    return max(num * sa + den * sb + 1 + 2 * slack * max(num, den) for num, den in WIDE_RATES)


def edge_library(seed=83, n_source=300):
    """(videos, pairs): the source and one clip per rate of WIDE_RATES as in wide_library, but frame t of a clip differs from
    its source frame in exactly 31 bits when t is even and in exactly 32 when t is odd. Pairs: every clip against the source
    in both orientations."""
    rng = np.random.default_rng(seed)
    source = _rand(rng, n_source)
    vids = [source]
    for k, (num, den) in enumerate(WIDE_RATES):
        clip = resampled(source, WIDE_CLIP, num, den, 4.4 + 1.3 * k)
        vids.append(np.stack([AH.flip_bits(rng, f, 31 + (t & 1)) for t, f in enumerate(clip)]))
    return vids, [(v, 0) for v in range(1, 9)] + [(0, v) for v in range(1, 9)]


def tiny_library(seed=84):
    """(videos, pairs): 1, 1, 2, 3, 7 and 12 frames of one hash, then the same lengths of independent random hashes; the pairs
    1 x 1, 2 x 3 and 7 x 12 of each kind, the longer ones in both orientations. pairs[3] is the static 7 x 12 pair."""
    rng = np.random.default_rng(seed)
    h = _rand(rng, 1)
    lengths = (1, 1, 2, 3, 7, 12)
    vids = [np.repeat(h, n, axis=0) for n in lengths] + [_rand(rng, n) for n in lengths]
    pairs = [(0, 1), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (8, 9), (9, 8), (10, 11), (11, 10)]
    return vids, pairs


def bin_limit_library(seed=85):
    """(videos, positions, span_a, spans_b): three videos of two frames at positions [0, span]. Under [(1, 1), (8, 1)] at slack 1
    the pair (0, 1) has 8 * 100000 + 248559 + 1 + 16 = 2^20 bins at (8, 1), the pair (0, 2) one more; under [(1, 1), (1, 8)] the
    pairs (1, 0) and (2, 0) have the same. Frame i of videos 1 and 2 is within 20 bits of frame 1 - i of video 0 and far from
    frame i: two hits, (0, 1) and (1, 0), the last and the first core bin of the histogram at either rate. Their deltas lie far
    apart, so both rates hold bands of one vote and (1, 1), listed first, keeps the tie. (With positions [0, span] and 2 x 2
    frames no pair of exactly 2^20 bins can give (1, 1) two votes in a band and (8, 1) one: two deltas of (1, 1) within 2 of each
    other need span_a <= 2, which (8, 1) gathers as well, or span_b <= 2 or |span_b - span_a| <= 2, which
    8 span_a + span_b = 2^20 - 17 rules out.)"""
    rng = np.random.default_rng(seed)
    A = _rand(rng, 2)
    span_a, spans_b = 100000, (248559, 248560)
    vids = [A, AH.noisy(rng, A[::-1], 20), AH.noisy(rng, A[::-1], 20)]
    positions = np.array([0, span_a, 0, spans_b[0], 0, spans_b[1]], dtype=np.int32)
    return vids, positions, span_a, spans_b


MAX_POSITION = (1 << 20) - 1  # the largest position the host entry accepts (check_positions of hvd_search.cpp)


def far_positions_library(seed=86):
    """(videos, positions): video 0, 60 random frames at positions 0..59; video 1, 8 frames that end at MAX_POSITION, frame t
    a noisy copy of frame 8 t + 3 of video 0. As a against video 0 as b that is rate (8, 1) with
    offset = p_b - 8 p_a = 3 - 8 (MAX_POSITION - 7), about -2^23; as b against a it is (1, 8) and the offset is the opposite."""
    rng = np.random.default_rng(seed)
    Q = _rand(rng, 60)
    P = AH.noisy(rng, Q[8 * np.arange(8) + 3], 20)
    positions = np.concatenate([np.arange(60), MAX_POSITION - 7 + np.arange(8)]).astype(np.int32)
    return [Q, P], positions
