"""Builders of tests/test_gpu_rate_segments_grid.py and tests/test_rate_segments_grid_cpu.py: multi-piece reels whose pieces lie on
rates with an 8, the restatement's records of them (rate_segments_helpers) over rates_helpers.GRID, reels at exactly 31 and 32 bits
from their source, and a pair of exactly HVD_ALIGN_LDS_BINS bins with the longest bit words an LDS pair can have. Nothing here
touches the device."""
import numpy as np

import align_helpers as AH
import rate_segments_helpers as RS
import rates_helpers as RH

W = RH.WIDE_RATES
LDS_BINS = 4096  # HVD_ALIGN_LDS_BINS
SETTINGS = ((8, 1), (8, 4), (2, 1))  # (max_segments, min_band_votes)
KINDS = ("index", "gapped")
# (frames, num, den, c) per piece, c for a 300-frame source; every piece of a reel but the last lies on a rate with an 8 or a 7
REEL_A = ((30, 8, 1, 3.3), (28, 7, 2, 60.4), (24, 8, 3, 150.2), (20, 1, 1, 250.0))
REEL_B = ((36, 8, 7, 5.5), (36, 5, 8, 100.3), (30, 1, 1, 200.0))
SEED = 40


def cut(source, pieces, k=1.0):
    """The pieces, resampled from the source one after the other; c of every piece but the first is scaled by k."""
    return np.concatenate([RH.resampled(source, n, num, den, c if p == 0 else c * k)
                           for p, (n, num, den, c) in enumerate(pieces)])


def wide_reels(n_source, seed):
    """(videos, pairs). Video 0: a source of n_source independent random hashes; 1: reel A, 2: reel B (REEL_A, REEL_B, c scaled
    by n_source / 300), up to 20 bits flipped per frame; 3, 4: 7 and 12 frames of one hash; 5: 9 random frames; 6: no frame.
    Pairs: each reel against the source and reel against reel, the static pair, all in both orientations; the random frames
    and the empty video against the source."""
    rng = np.random.default_rng(seed)
    source = RH._rand(rng, n_source)
    k = n_source / 300
    h = RH._rand(rng, 1)
    vids = [source, AH.noisy(rng, cut(source, REEL_A, k), 20), AH.noisy(rng, cut(source, REEL_B, k), 20),
            np.repeat(h, 7, axis=0), np.repeat(h, 12, axis=0), RH._rand(rng, 9), np.zeros((0, 32), np.uint8)]
    pairs = [(1, 0), (0, 1), (2, 0), (0, 2), (1, 2), (2, 1), (3, 4), (4, 3), (5, 0), (6, 0)]
    return vids, pairs


def gaps(rng, offsets):
    """Positions with gaps, as tests/test_gpu_rate_segments.py builds them: per video a start of 0..4 and steps of 1 or 2."""
    return np.concatenate([int(rng.integers(0, 5)) + np.cumsum(rng.integers(1, 3, int(n))) for n in np.diff(offsets)]).astype(np.int32)


def index_positions(offsets):
    """The index inside the video, as an array: what the device makes of positions = None."""
    return (np.arange(int(offsets[-1])) - np.repeat(offsets[:-1], np.diff(offsets))).astype(np.int32)


def bins_of(span_a, span_b, rates, slack):
    return max(n * span_a + d * span_b + 1 + 2 * slack * max(n, d) for n, d in rates)


def pair_bins(offsets, positions, pair, rates, slack):
    """The largest bins_r of a pair (0 for a pair with an empty video)."""
    spans = []
    for v in pair:
        if offsets[v + 1] == offsets[v]:
            return 0
        spans.append(int(offsets[v + 1] - offsets[v]) - 1 if positions is None
                     else int(positions[offsets[v + 1] - 1]) - int(positions[offsets[v]]))
    return bins_of(spans[0], spans[1], rates, slack)


class WideReels:
    """frames, offsets, pairs, positions {kind: None or int32 per frame}, want {(kind, setting, (max_dist, slack)): records}."""

    def __init__(self, n_source):
        vids, pairs = wide_reels(n_source, SEED + n_source)
        self.n_source = n_source
        self.frames, self.offsets = RH.join(vids)
        self.pairs = tuple(pairs)
        self.positions = {"index": None, "gapped": gaps(np.random.default_rng(SEED + 1 + n_source), self.offsets)}
        self.want = {}
        for kind in KINDS:
            for K, floor in SETTINGS:
                for max_dist, slack in RH.GRID:
                    recs = RS.align_rate_segments(self.frames, self.offsets, pairs, self.positions[kind], W, slack, max_dist,
                                                  max_segments=K, min_band_votes=floor)
                    recs.setflags(write=False)
                    self.want[(kind, (K, floor), (max_dist, slack))] = recs
        for x in (self.frames, self.offsets, self.positions["gapped"]):
            x.setflags(write=False)
        # the launches: at 300 every pair on index positions is an LDS pair, at 600 every pair with the source a scratch pair
        reel_source = [p for p in pairs if 0 in p and (1 in p or 2 in p)]
        for slack in (0, 1, 3, 16):
            on_index = {p: pair_bins(self.offsets, None, p, W, slack) for p in pairs}
            if n_source == 300:  # (the widest rate of a 102 x 300 pair is (7, 8) or (8, 7), not (1, 8))
                assert max(on_index.values()) == 7 * 101 + 8 * 299 + 1 + 16 * slack <= 3356 <= LDS_BINS
            if n_source == 600:
                assert min(on_index[p] for p in reel_source) == 7 * 101 + 8 * 599 + 1 + 16 * slack >= 5500 > LDS_BINS
                assert on_index[(5, 0)] > LDS_BINS and max(b for p, b in on_index.items() if 0 not in p) <= LDS_BINS

    def max_bins(self, kind):
        """The largest bins_r of any pair at any slack of the grid: what the scratch of a device call is sized for."""
        return max(pair_bins(self.offsets, self.positions[kind], p, W, 16) for p in self.pairs)


_reels = {}


def wide_reels_case(n_source):
    """The WideReels of a source length: computed once per process and shared, its arrays read-only."""
    if n_source not in _reels:
        _reels[n_source] = WideReels(n_source)
    return _reels[n_source]


# ---- windows wider than the histogram; ties in rounds after the first ----

# (rotation of WIDE_RATES, max_dist, slack, (max_segments, min_band_votes)) on rates_helpers.tiny_library(). At slack 16 every
# window holds every hit of these pairs: one segment a pair, every rate tying. The segments of one vote that every rate ties on
# in rounds after the first need a window that leaves hits behind: the same pairs at slack 0.
CASE_3 = tuple((k, max_dist, slack, setting) for k in (0, 3, 5) for max_dist, slack in ((31, 16), (127, 16), (127, 0))
               for setting in ((8, 1), (8, 2)))


# ---- the tolerance edge ----

EDGE_A = ((20, 8, 3, 4.4), (16, 7, 2, 100.6))   # a reel as video a against the source: rates (8, 3) and (7, 2)
EDGE_B = ((20, 8, 1, 3.3), (16, 8, 5, 330.2))   # a reel as video b against the source as a: rates (1, 8) and (5, 8)


def edge_reels(seed=87):
    """(videos, pairs): a 400-frame source and two reels of two pieces (20 and 16 frames) at two rates of WIDE_RATES each, one
    for either orientation. Every frame of a piece 1 differs from its source frame in exactly 31 bits, every frame of a
    piece 2 in exactly 32. Pairs: (1, 0) and (0, 2)."""
    rng = np.random.default_rng(seed)
    source = RH._rand(rng, 400)
    vids = [source]
    for pieces in (EDGE_A, EDGE_B):
        clip = cut(source, pieces)
        vids.append(np.stack([AH.flip_bits(rng, f, 31 if t < pieces[0][0] else 32) for t, f in enumerate(clip)]))
    return vids, [(1, 0), (0, 2)]


# ---- either side of the LDS limit, the bit words at their largest ----

def lds_edge_pair(seed=88):
    """(videos, pairs): video 0, 2 049 random frames; video 1, 2 048 frames, and video 2, 2 049: random but for two stretches of
    300 frames, noisy copies (up to 20 bits) of frames 700.. and 50.. of video 0 at frames 100.. and 1 200... On index positions
    under [(1, 1)] at slack 0 the pair (0, 1) has 2048 + 2047 + 1 = 4 096 bins and 65 + 64 words a run of bit words, the pair
    (0, 2) has 4 097 bins. Pairs: (0, 1), (0, 2)."""
    rng = np.random.default_rng(seed)
    a = RH._rand(rng, 2049)
    vids = [a]
    for n in (2048, 2049):
        b = RH._rand(rng, n)
        b[100:400] = AH.noisy(rng, a[700:1000], 20)
        b[1200:1500] = AH.noisy(rng, a[50:350], 20)
        vids.append(b)
    return vids, [(0, 1), (0, 2)]
