"""Numpy restatement of the time alignment where a frame of b serves more than once (include/hvd_mi355x.h:
hvd_vpdq_align_loops): signed_helpers.signed_pair's loop of rounds with rates_helpers.best_band asked at every
listed rate in every round -- no rate is ever passed over; the bound-skip is the kernel's pruning only -- without a taken set on
the b side, with up to 64 rounds, and with seen_b counted. The reference of tests/test_loops_cpu.py and tests/test_gpu_loops.py;
nothing here touches the device."""
import numpy as np

import align_helpers as AH
import rates_helpers as RH
import signed_helpers as SG

MAX_SEGMENTS = SG.MAX_SEGMENTS
MAX_ROUNDS = 64
INT32_MIN = AH.INT32_MIN
LOST = SG.LOST
REVERSED_RATES = SG.REVERSED_RATES
VLOOPS_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4"), ("n_segments", "<u4"),
                         ("q_covered", "<u4"), ("t_covered", "<u4"), ("rounds", "<u4"),
                         ("seg", SG.VSSEGMENT_DTYPE, (MAX_SEGMENTS,))])


def loops_pair(A, B, pa=None, pb=None, max_dist=31, slack=1, rates=REVERSED_RATES, max_rounds=MAX_ROUNDS, min_band_votes=1):
    """(q_hits, t_hits, [round, ...], t_covered) of one pair, or LOST when a listed rate needs more than 2^20 bins. A round is
    a segment's twelve words (signed_helpers.signed_pair); ALL rounds are returned, the record keeps the first eight.
    t_covered: the distinct frames of b in any round. The list is taken as it is: the rule alone."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    na, nb = A.shape[0], B.shape[0]
    if na == 0 or nb == 0:
        return 0, 0, [], 0
    pa = np.arange(na, dtype=np.int64) if pa is None else np.asarray(pa, dtype=np.int64)
    pb = np.arange(nb, dtype=np.int64) if pb is None else np.asarray(pb, dtype=np.int64)
    assert pa.shape == (na,) and pb.shape == (nb,) and 1 <= max_rounds <= MAX_ROUNDS and min_band_votes >= 1
    if SG.bins_of(int(pa[-1] - pa[0]), int(pb[-1] - pb[0]), rates, slack) > RH.MAX_BINS:
        return LOST
    hit = AH.hamming_matrix(A, B) <= max_dist
    q_hits, t_hits = int(hit.any(1).sum()), int(hit.any(0).sum())
    taken_a, seen_b = np.zeros(na, bool), np.zeros(nb, bool)
    rounds = []
    for _ in range(max_rounds):
        i, j = np.nonzero(hit & ~taken_a[:, None])  # H_r: b is not filtered
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
        rounds.append((d, S, qa.size, ta.size, int(pa[qa].min()), int(pa[qa].max()), int(pb[ta].min()), int(pb[ta].max()),
                       int(num), int(den), r, 0))
        taken_a[qa] = True
        seen_b[ta] = True
        if taken_a.all():
            break
    return q_hits, t_hits, rounds, int(seen_b.sum())


def shared_b_frames(A, B, **kw) -> int:
    """How many frames of b lie in more than one round of the pair (index positions): sum of t_aligned - t_covered."""
    _, _, rounds, t_covered = loops_pair(A, B, **kw)
    return sum(s[3] for s in rounds) - t_covered


def record(a, b, q_hits, t_hits, rounds, t_covered) -> np.ndarray:
    """One VLOOPS_DTYPE record from the pair's counters and ALL its rounds."""
    rec = np.zeros((), dtype=VLOOPS_DTYPE)
    rec["a"], rec["b"], rec["q_hits"], rec["t_hits"] = a, b, q_hits, t_hits
    rec["n_segments"], rec["rounds"] = min(len(rounds), MAX_SEGMENTS), len(rounds)
    rec["q_covered"], rec["t_covered"] = sum(s[2] for s in rounds), t_covered
    for k, s in enumerate(rounds[:MAX_SEGMENTS]):
        rec["seg"][k] = s
    return rec


def lost_record(a, b) -> np.ndarray:
    """The record of a pair the device entry cannot align."""
    rec = np.zeros((), dtype=VLOOPS_DTYPE)
    rec["a"], rec["b"] = a, b
    rec["seg"][0]["offset"] = INT32_MIN
    return rec


def align_loops(frames, offsets, pairs, positions=None, rates=REVERSED_RATES, max_rounds=MAX_ROUNDS, min_band_votes=1, slack=1,
                max_dist=31, frames_t=None, offsets_t=None, positions_t=None) -> np.ndarray:
    """Reference of search.align_loops and of the device entry: VLOOPS_DTYPE records in the order of the pair list. A pair
    index out of range, and every pair under a broken list, is the INT32_MIN record."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, dtype=np.int64)
    if frames_t is None:
        frames_t, offsets_t, positions_t = frames, offsets, positions
    frames_t = np.asarray(frames_t, dtype=np.uint8).reshape(-1, 32)
    offsets_t = np.asarray(offsets_t, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rates = [tuple(int(x) for x in r) for r in rates]
    out = np.zeros(pairs.shape[0], dtype=VLOOPS_DTYPE)
    for k, (a, b) in enumerate(pairs):
        if not SG.sound_signed(rates) or a >= offsets.size - 1 or b >= offsets_t.size - 1:
            out[k] = lost_record(a, b)
            continue
        sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets_t[b], offsets_t[b + 1])
        got = loops_pair(frames[sa], frames_t[sb], None if positions is None else np.asarray(positions)[sa],
                         None if positions_t is None else np.asarray(positions_t)[sb], max_dist, slack, rates, max_rounds,
                         min_band_votes)
        out[k] = lost_record(a, b) if got is LOST else record(a, b, *got)
    return out


def restated(frames, offsets, pairs, *args, **kwargs):
    """align_loops, computed once per distinct pair of the list."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    return align_loops(frames, offsets, uniq, *args, **kwargs)[inv.reshape(-1)]


class ReferenceMatcher(SG.ReferenceMatcher):
    """match_videos / align_* on the reference, align_loops among them: what search.looped_excerpt_pairs takes as `matcher`."""

    align_loops = staticmethod(align_loops)


def same(got, want):
    assert got.dtype == VLOOPS_DTYPE and got.shape == want.shape
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(k, got[k].tolist(), want[k].tolist()) for k in bad[:3]]


# ---- the table of the issue: loops of one 600-frame source (seed 71), up to 20 bits flipped per frame ----

_table = {}


def table():
    """{name: video}, built in the table's order: the source; `boom` = frames 100..159, then the same reversed; `loop5` = those
    60 frames five times; `loop12` = frames 300..319 twelve times; `boom3` = (100..129 forward, then reversed) three times.
    Drawn after them, so that the table's videos are the proposal's: `clip` = frames 200..259, a plain excerpt. Computed once
    per process; the arrays are read-only."""
    if not _table:
        rng = np.random.default_rng(71)
        source = RH._rand(rng, 600)
        _table["source"] = source
        half = source[100:160]
        _table["boom"] = AH.noisy(rng, np.concatenate([half, half[::-1]]), 20)
        _table["loop5"] = AH.noisy(rng, np.tile(half, (5, 1)), 20)
        _table["loop12"] = AH.noisy(rng, np.tile(source[300:320], (12, 1)), 20)
        _table["boom3"] = AH.noisy(rng, np.tile(np.concatenate([source[100:130], source[100:130][::-1]]), (3, 1)), 20)
        _table["clip"] = AH.noisy(rng, source[200:260], 20)
        for v in _table.values():
            v.setflags(write=False)
    return _table


def static_pair():
    """The static pair of DESIGN 4.9: 50 against 80 copies of one frame."""
    h = RH._rand(np.random.default_rng(78), 1)
    return np.repeat(h, 50, axis=0), np.repeat(h, 80, axis=0)


def planted_loops(seed, n_source=120):
    """(videos, pairs): video 0 a source of n_source random hashes; a boomerang of 12 + 12 frames; a 3 x 10 loop; 10 repetitions
    of 6 frames; a plain 20-frame excerpt; a reversed 15-frame clip; a static pair (7 and 12 copies of one frame); 9 random
    frames; no frame. Up to 20 bits flipped per frame. Pairs: every clip against the source in both orientations, the static pair
    both ways, the random and the empty video."""
    rng = np.random.default_rng(seed)
    source = RH._rand(rng, n_source)
    h = RH._rand(rng, 1)
    vids = [source,
            AH.noisy(rng, np.concatenate([source[30:42], source[30:42][::-1]]), 20),
            AH.noisy(rng, np.tile(source[50:60], (3, 1)), 20),
            AH.noisy(rng, np.tile(source[70:76], (10, 1)), 20),
            AH.noisy(rng, source[80:100], 20),
            AH.noisy(rng, source[5:20][::-1], 20),
            np.repeat(h, 7, axis=0), np.repeat(h, 12, axis=0), RH._rand(rng, 9), np.zeros((0, 32), np.uint8)]
    pairs = [(v, 0) for v in range(1, 6)] + [(0, v) for v in range(1, 6)] + [(6, 7), (7, 6), (8, 0), (9, 0), (0, 9)]
    return vids, pairs
