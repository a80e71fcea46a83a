"""The inputs of tests/test_gpu_rates_grid.py, judged on the numpy restatement alone (tests/rates_helpers.py): each
library does what its case needs, so that no GPU case is vacuous. Case numbers are those of the GPU file's docstring. The last
test restates the rule with one slip at a time -- the slips a kernel could hold without the older GPU tests noticing -- and shows
that each changes a record of the case that is said to pin it. Nothing here touches the device; every comparison is equality."""
import numpy as np
import pytest

import align_helpers as AH
import rates_helpers as RH

W = RH.WIDE_RATES
LDS_BINS = 4096  # HVD_ALIGN_LDS_BINS (tests/test_align_cpu.py checks the header against _lib)


def words(rec):
    return rec.tolist()[2:]


def packed(rates):
    """The two kernel arguments of a list (pack_rate_list of hvd_kernels.h)."""
    return (sum(n << 4 * r for r, (n, d) in enumerate(rates)), sum(d << 4 * r for r, (n, d) in enumerate(rates)))


# ---- case 1: the wide-rate libraries ----

def test_the_wide_list_is_sound_and_needs_every_nibble_bit():
    assert RH.sound(W) and len(W) == RH.MAX_RATES and W[0] == (1, 1)
    assert sum(n == 8 for n, d in W) == 3 and sum(d == 8 for n, d in W) == 3  # the top bit of a nibble, in nums and in dens
    assert len(RH.GRID) == 20 and (127, 16) in RH.GRID and (0, 0) in RH.GRID


@pytest.mark.parametrize("n_source", [300, 600])
def test_wide_library_plants_every_rate_on_either_side_of_the_lds_limit(n_source):
    frames, offsets, pairs, want = RH.wide_case(n_source)
    assert np.diff(offsets).tolist() == [n_source] + [RH.WIDE_CLIP] * 8 + [7, 12, 9, 0] and len(pairs) == 22
    source_pairs = [p for p in pairs if 0 in p and 12 not in p]
    assert len(source_pairs) == 17
    for slack in (0, 1, 3, 16):
        bins = [RH.wide_bins(n_source, slack, p) for p in source_pairs]
        if n_source == 300:  # the LDS launch at every slack: at most 7 * 35 + 8 * 299 + 1 + 2 * 16 * 8 = 2894 bins
            assert max(RH.wide_bins(300, slack, p) for p in pairs) <= 2894 <= LDS_BINS
        else:                # the scratch launch at every slack: at least 7 * 8 + 8 * 599 + 1 bins (the 9 random frames),
                             # 4828 for a clip
            assert min(bins) == 7 * 8 + 8 * 599 + 1 + 16 * slack > LDS_BINS
            assert min(b for b, p in zip(bins, source_pairs) if 11 not in p) >= 4828
            assert max(RH.wide_bins(600, slack, p) for p in pairs if 0 not in p) <= 15 * 35 + 1 + 256  # the others stay in LDS
    # 8 of 8 planted rates win at (31, 1), with every frame of the clip in the band -- and at 30 and 32
    for max_dist in (30, 31, 32):
        recs = want[(max_dist, 1)]
        assert [(r["rate_num"], r["rate_den"], r["rate_index"]) for r in recs[:8]] == [W[k] + (k,) for k in range(8)]
    assert (want[(31, 1)]["band_votes"][:8] == RH.WIDE_CLIP).all() and (want[(31, 1)]["q_aligned"][:8] == RH.WIDE_CLIP).all()
    # the source as a: the inverse rate, where W lists it
    back = want[(31, 1)][8:16]
    assert [(r["rate_num"], r["rate_den"]) for r in back[:5]] == [(1, 1), (7, 8), (8, 7), (1, 8), (8, 1)]
    assert (back["offset"][:5] == -want[(31, 1)]["offset"][:5]).all()
    # every rate of W is the winner of some record; every grid point has records with and without a hit
    winners = {int(r["rate_index"]) for recs in want.values() for r in recs if r["q_hits"]}
    assert winners == set(range(8))
    for key, recs in want.items():
        assert (recs["q_hits"] > 0).sum() >= 2 and words(recs[21]) == RH.ZERO, key  # (the empty video)
        assert (recs["offset"] != RH.INT32_MIN).all()
    assert 2 <= (want[(0, 0)]["q_hits"] > 0).sum() < 21 == (want[(127, 16)]["q_hits"] > 0).sum()
    # the slack matters: at slack 16 some record's winner is not its winner at slack 1
    moved = [(m, k) for m in (0, 30, 31, 32, 127) for k in range(22)
             if want[(m, 1)][k]["q_hits"] and want[(m, 1)][k]["rate_index"] != want[(m, 16)][k]["rate_index"]]
    assert len(moved) >= 20 and {m for m, k in moved} >= {31, 127}
    # and the records of neighbouring tolerances and slacks differ
    for m in (0, 30, 31, 32, 127):
        assert len({want[(m, s)].tobytes() for s in (0, 1, 3, 16)}) == 4
    for s in (0, 1, 3, 16):  # (clips within 20 bits of the source: two of 30, 31, 32 may agree -- case 2 tells them apart)
        assert len({want[(m, s)].tobytes() for m in (0, 30, 31, 32, 127)}) >= 4


def test_wide_grid_is_shared_and_read_only():
    a, b = RH.wide_case(300), RH.wide_case(300)
    assert a is b
    with pytest.raises(ValueError):
        a[3][(31, 1)]["offset"][0] = 1


# ---- case 2: the tolerance edge ----

def test_edge_clips_sit_at_31_and_32_bits():
    vids, pairs = RH.edge_library()
    for clip, (num, den), k in zip(vids[1:], W, range(8)):
        idx = np.floor(np.arange(RH.WIDE_CLIP) * num / den + 4.4 + 1.3 * k + 0.5).astype(np.int64)
        d = AH.hamming_matrix(clip, vids[0])
        assert d[np.arange(RH.WIDE_CLIP), idx].tolist() == [31, 32] * (RH.WIDE_CLIP // 2)
        d[np.arange(RH.WIDE_CLIP), idx] = 999
        far = d if den == 1 or num >= den else None  # (slow clips repeat a source frame: its other copies are near too)
        assert far is None or far.min() > 32
    frames, offsets = RH.join(vids)
    recs = {m: RH.align_rates(frames, offsets, pairs, None, W, 1, m) for m in (30, 31, 32)}
    even = RH.WIDE_CLIP // 2
    for k in range(16):
        assert len({recs[m][k].tobytes() for m in (30, 31, 32)}) == 3, k  # pairwise different
        assert words(recs[30][k]) == RH.ZERO
    assert (recs[31]["q_hits"][:8] == even).all() and (recs[31]["t_hits"][8:] == even).all()
    assert (recs[32]["q_hits"][:8] == RH.WIDE_CLIP).all() and (recs[32]["t_hits"][8:] == RH.WIDE_CLIP).all()
    assert (recs[31]["band_votes"][:8] == even).all() and (recs[32]["band_votes"][:8] == RH.WIDE_CLIP).all()
    assert [int(r["rate_index"]) for r in recs[31][:8]] == list(range(8)) == [int(r["rate_index"]) for r in recs[32][:8]]


# ---- case 3: windows wider than the histogram, ties across rates ----

def test_tiny_pairs_tie_at_every_rate_and_the_first_listed_wins():
    vids, pairs = RH.tiny_library()
    frames, offsets = RH.join(vids)
    assert pairs[3] == (4, 5) and [len(vids[v]) for v in pairs[3]] == [7, 12]
    # slack_r = 16 * 8 = 128: a window of 257 bins over a core of at most 7 * 6 + 8 * 11 + 1 = 131
    assert max(n * 6 + d * 11 + 1 for n, d in W) == 131 < 2 * 128 + 1
    assert RH.rate_tops(vids[4], vids[5], slack=16) == [84] * 8
    for k in range(8):
        rates = RH.rotated(W, k)
        recs = RH.align_rates(frames, offsets, pairs, None, rates, 16, 127)
        assert words(recs[3]) == (7, 12, 0, 84, 7, 12, 0, 6, 0, 11) + rates[0] + (0, 0)
        assert (recs["rate_index"] == 0).all()  # every pair ties: a window holds every hit at every rate
        at_31 = RH.align_rates(frames, offsets, pairs, None, rates, 16, 31)
        assert at_31[:5].tolist() == recs[:5].tolist() and not at_31["q_hits"][5:].any()  # random frames: hits at 127 only
    recs = RH.align_rates(frames, offsets, pairs, None, W, 16, 127)
    assert (recs["q_hits"][6:] > 0).all() and recs["band_votes"][8] == 49 < 84


def test_reordering_changes_rate_index_alone_where_no_rates_tie():
    """The header's consequence (d) on the 300-frame library at RH.REORDER_POINTS: the pairs whose largest S belongs to one rate
    alone -- at (31, 1) the eight clips against the source among them -- keep every word but rate_index under a rotated list."""
    frames, offsets, pairs, want = RH.wide_case(300)
    for max_dist, slack in RH.REORDER_POINTS:
        loose = RH.non_tying(frames, offsets, pairs, max_dist, slack)
        assert len(loose) >= 9 and ((max_dist, slack) != (31, 1) or set(range(8)) <= set(loose))
        for k in (3, 5):
            turned = RH.align_rates(frames, offsets, pairs, None, RH.rotated(W, k), slack, max_dist)
            for p in loose:
                w, t = want[(max_dist, slack)][p], turned[p]
                assert w.tolist()[:14] == t.tolist()[:14] and (t["rate_index"] + k) % 8 == w["rate_index"]
            assert (turned["rate_index"] != want[(max_dist, slack)]["rate_index"]).sum() >= 9


# ---- case 4: the top nibble bit and the eighth entry ----

CASE4_LISTS = RH.TOP_BIT_LISTS


def test_lists_that_need_bit_3_of_a_nibble_and_bit_31_of_a_word():
    frames, offsets, pairs, want = RH.wide_case(300)
    assert all(RH.sound(r) for r in CASE4_LISTS)
    assert CASE4_LISTS[4][7] == (8, 1) and CASE4_LISTS[5][7] == (1, 8)
    bit31 = [(n >> 31, d >> 31) for n, d in map(packed, CASE4_LISTS)]
    assert bit31 == [(0, 0)] * 4 + [(1, 0), (0, 1), (1, 0)] and packed(CASE4_LISTS[6])[1] & 15 == 8
    for rates in CASE4_LISTS:
        recs = RH.align_rates(frames, offsets, pairs, None, rates, 1, 31)
        for k, rate in enumerate(W):  # the planted clip of every listed rate is found whole, at its place in the list
            if rate in rates:
                assert recs[k].tolist()[5:7] == (36, 36) and recs[k].tolist()[12:15] == rate + (rates.index(rate),)
        if len(rates) == 8:
            assert recs[W.index(rates[7])]["rate_index"] == 7  # the eighth entry wins a record
        else:                # a single rate: the other clips fall apart
            assert sorted(recs["band_votes"][:8])[-2] < 20


# ---- case 5: the 2^20-bin rule through a rate, positions at the host entry's bound ----

def test_bin_limit_pairs_sit_on_the_limit_and_one_past_it():
    vids, positions, span_a, spans_b = RH.bin_limit_library()
    frames, offsets = RH.join(vids)
    bins = lambda sa, sb, rates: max(n * sa + d * sb + 1 + 2 * max(n, d) for n, d in rates)  # noqa: E731 (slack 1)
    two, owt = ((1, 1), (8, 1)), ((1, 1), (1, 8))
    assert bins(span_a, spans_b[0], two) == 1 << 20 == bins(spans_b[0], span_a, owt)
    assert bins(span_a, spans_b[1], two) == (1 << 20) + 1 == bins(spans_b[1], span_a, owt)
    assert LDS_BINS < bins(span_a, spans_b[1], two[:1]) == span_a + spans_b[1] + 3 < 1 << 19
    assert positions.max() < RH.MAX_POSITION
    d = AH.hamming_matrix(vids[0], vids[1])
    assert d[0, 1] <= 20 and d[1, 0] <= 20 and d[0, 0] > 64 and d[1, 1] > 64
    recs = RH.align_rates(frames, offsets, [(0, 1), (0, 2)], positions, two, 1)
    assert recs.tolist() == [(0, 1, 2, 2, -span_a, 1, 1, 1, span_a, span_a, 0, 0, 1, 1, 0, 0), (0, 2) + RH.LOST]
    back = RH.align_rates(frames, offsets, [(1, 0), (2, 0)], positions, owt, 1)
    assert back.tolist() == [(1, 0, 2, 2, span_a, 1, 1, 1, 0, 0, span_a, span_a, 1, 1, 0, 0), (2, 0) + RH.LOST]
    # (8, 1) has no chance: a band of one vote at either rate, and (1, 1) stands first
    assert RH.rate_tops(vids[0], vids[1], positions[0:2], positions[2:4], rates=two) == [1, 1]
    # the rule is about ANY listed rate: alone, (1, 1) aligns the pair that is lost under the list
    alone = RH.align_rates(frames, offsets, [(0, 1), (0, 2)], positions, two[:1], 1)
    assert alone[0] == recs[0] and words(alone[1]) == words(recs[0])


def test_positions_at_the_host_bound_scale_to_two_to_the_23():
    vids, positions = RH.far_positions_library()
    frames, offsets = RH.join(vids)
    assert positions.max() == RH.MAX_POSITION == (1 << 20) - 1
    recs = RH.align_rates(frames, offsets, [(1, 0), (0, 1)], positions, W, 1)
    off = 3 - 8 * (RH.MAX_POSITION - 7)
    assert recs.tolist() == [(1, 0, 8, 8, off, 8, 8, 8, RH.MAX_POSITION - 7, RH.MAX_POSITION, 3, 59, 8, 1, 3, 0),
                             (0, 1, 8, 8, -off, 8, 8, 8, 3, 59, RH.MAX_POSITION - 7, RH.MAX_POSITION, 1, 8, 4, 0)]
    assert (1 << 23) - 128 < -off < 1 << 23
    assert max(n * 59 + d * 7 + 1 + 2 * max(n, d) for n, d in W) <= LDS_BINS


# ---- what each case pins: the rule with one slip, on the case's own input ----

def slipped_pair(A, B, max_dist, slack, rates, slip):
    """rates_helpers.rates_pair on index positions with one slip. "lt": d < max_dist for d <= max_dist; "min": slack_r =
    slack min(num, den) in both passes; "pass2": the caller's slack, unscaled, in pass 2; "ge": a later rate takes a tie;
    "mask": entries read through a 3-bit mask (8 reads as 0)."""
    i, j = np.nonzero(AH.hamming_matrix(A, B) < max_dist if slip == "lt" else AH.hamming_matrix(A, B) <= max_dist)
    if i.size == 0:
        return RH.ZERO
    pick = min if slip == "min" else max
    win = None
    for r, (num, den) in enumerate(rates):
        num, den = (num & 7, den & 7) if slip == "mask" else (num, den)
        delta = den * j - num * i
        d, S = RH.best_band(delta, slack * pick(num, den))
        if win is None or S > win[1] or (slip == "ge" and S == win[1]):
            win = (d, S, r, delta, num, den)
    d, S, r, delta, num, den = win
    on = np.abs(delta - d) <= (slack if slip == "pass2" else slack * pick(num, den))
    qa, ta = np.unique(i[on]), np.unique(j[on])
    ends = (int(qa.min()), int(qa.max()), int(ta.min()), int(ta.max())) if on.any() else (None,) * 4  # (d* may hold no vote)
    return (np.unique(i).size, np.unique(j).size, d, S, qa.size, ta.size) + ends + (int(num), int(den), r, 0)


def slipped(frames, offsets, pairs, max_dist, slack, rates, slip):
    return [slipped_pair(frames[offsets[a]:offsets[a + 1]], frames[offsets[b]:offsets[b + 1]], max_dist, slack, rates, slip)
            for a, b in pairs]


def test_every_slip_changes_a_record_of_the_case_that_pins_it():
    frames, offsets, pairs, want = RH.wide_case(300)
    pairs = list(pairs)
    model = lambda key: [words(r) for r in want[key]]  # noqa: E731
    # (the slip-free restatement of this file is the model)
    assert slipped(frames, offsets, pairs, 31, 1, W, None) == model((31, 1))
    assert slipped(frames, offsets, pairs, 127, 16, W, None) == model((127, 16))
    # case 1: slack * max(num, den) in pass 1 and in pass 2, at every slack above 0
    for slack in (1, 3, 16):
        assert slipped(frames, offsets, pairs, 31, slack, W, "min") != model((31, slack))
        assert slipped(frames, offsets, pairs, 31, slack, W, "pass2") != model((31, slack))
        bands = [(a[:4], a[10:]) for a in slipped(frames, offsets, pairs, 31, slack, W, "pass2")]
        assert bands == [(b[:4], b[10:]) for b in model((31, slack))]  # (pass 1 is untouched: the aligned sets alone move)
    # case 2: the tolerance compare, on frames at exactly 31 and 32 bits
    vids, edge_pairs = RH.edge_library()
    fr, off = RH.join(vids)
    for max_dist in (31, 32):
        exact = [words(r) for r in RH.align_rates(fr, off, edge_pairs, None, W, 1, max_dist)]
        loose = slipped(fr, off, edge_pairs, max_dist, 1, W, "lt")
        assert all(a != b for a, b in zip(exact, loose))
    # case 1's noisy clips (0..20 bits flipped) do not sit on the tolerances of the grid: the edge clips are needed
    assert slipped(frames, offsets, pairs[:16], 31, 1, W, "lt") == model((31, 1))[:16]
    # case 3: ties go to the EARLIER rate
    vids, tiny_pairs = RH.tiny_library()
    fr, off = RH.join(vids)
    exact = [words(r) for r in RH.align_rates(fr, off, tiny_pairs, None, W, 16, 127)]
    late = slipped(fr, off, tiny_pairs, 127, 16, W, "ge")
    assert all(a[12] == 0 and b[12] == 7 for a, b in zip(exact, late) if a[0])
    # case 4: the top bit of a nibble
    for rates in CASE4_LISTS:
        exact = [words(r) for r in RH.align_rates(frames, offsets, pairs, None, rates, 1, 31)]
        assert slipped(frames, offsets, pairs, 31, 1, rates, None) == exact
        assert slipped(frames, offsets, pairs, 31, 1, rates, "mask") != exact
