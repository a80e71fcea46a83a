"""The inputs of tests/test_gpu_rate_segments_grid.py, judged without a device. Case numbers are those of the GPU
file's docstring. Three things are shown here: the builders of tests/rate_segments_grid_helpers.py do what the cases need (bins on
the stated side of a limit, distances of exactly 31 and 32 bits, segments in rounds after the first at rates with an 8); the model
of one workgroup (tests/rate_segments_model.py: the kernel statement by statement, bound-skip included) gives the restatement's
records at every grid point and setting of case 1, and its traces say that the skip is at work there -- rates passed over behind
a winner, passed over for good, and evaluated again after having been passed over; and the model with one line slipped
(GRID_FAULTS G1..G6) gives other records on the case that is said to pin that line, while the model without a slip gives the
restatement's on every case -- no slip is needed to explain a record. Nothing here touches the device; every comparison is
equality."""
import functools

import numpy as np
import pytest

import align_helpers as AH
import rate_segments_grid_helpers as G
import rate_segments_helpers as RS
import rate_segments_model as MD
import rates_helpers as RH

W = RH.WIDE_RATES
ONES = 0xFFFFFFFF  # what the words and ub hold before a workgroup's first pair, in the runs without a fault


def has_8(seg):
    return 8 in (int(seg["rate_num"]), int(seg["rate_den"]))


def segs(rec):
    return rec["seg"][:rec["n_segments"]]


def model(frames, offsets, positions, pairs, rates, slack, max_dist, settings, faults=()):
    """The model's two launches over a pair list, one Pair per entry shared by the settings -> {setting: (records, traces)}."""
    faults = frozenset(faults)
    pos = G.index_positions(offsets) if positions is None else positions
    entries = [MD.Pair(frames, offsets, pos, a, b, rates, slack, max_dist, faults) for a, b in pairs]
    slot = MD.slot_words(max(e.bins for e in entries))
    return {(K, floor): MD.model_call(entries, rates, slack, K, floor, slot, faults, 0 if faults else ONES) for K, floor in settings}


def differing(got, want):
    return np.flatnonzero(got != want)


# ---- case 1: the builders ----

@pytest.mark.parametrize("n_source", [300, 600])
def test_wide_reels_lie_on_their_rates_on_either_side_of_the_lds_limit(n_source):
    c = G.wide_reels_case(n_source)
    assert np.diff(c.offsets).tolist() == [n_source, 102, 102, 7, 12, 9, 0] and len(c.pairs) == 10
    assert RH.sound(W) and len(set(c.pairs)) == 10
    bins = {s: [G.pair_bins(c.offsets, None, p, W, s) for p in c.pairs] for s in (0, 1, 3, 16)}
    if n_source == 300:  # the LDS launch at every slack
        assert max(bins[16]) == 7 * 101 + 8 * 299 + 1 + 256 == 3356 <= G.LDS_BINS
    else:                # the scratch launch for every pair with the source (the last pair has an empty video)
        assert [b > G.LDS_BINS for b in bins[0]] == [True] * 4 + [False] * 4 + [True, False]
        assert min(bins[0][:4]) == 7 * 101 + 8 * 599 + 1 == 5500
    assert c.max_bins("gapped") > G.LDS_BINS  # gapped positions push pairs of the 300-frame source past LDS as well
    # the reels as video a lie on their pieces' rates: at (31, 1) every piece's rate has a segment, and the reel is covered
    # (the lines cross inside the wide bands: a band also claims the frames of other pieces that lie in it)
    for v, pieces in ((1, G.REEL_A), (2, G.REEL_B)):
        rec = c.want[("index", (8, 1), (31, 1))][c.pairs.index((v, 0))]
        found = {(int(s["rate_num"]), int(s["rate_den"])): int(s["q_aligned"]) for s in segs(rec)}
        assert all(found.get((num, den), 0) >= n // 2 for n, num, den, _ in pieces) and rec["q_covered"] >= 95, found
    for max_dist, slack in RH.GRID:
        full = c.want[("index", (8, 1), (max_dist, slack))]
        if 0 < max_dist < 127 and slack <= 3:
            assert (full["n_segments"] >= 3).sum() >= 4
            assert sum(has_8(s) for r in full for s in segs(r)[1:]) >= 1
        if (max_dist, slack) == (127, 16):  # the first band takes nearly everything
            assert full["n_segments"].tolist() == [1] * 9 + [0]
        for kind in G.KINDS:
            full, floor4, cap2 = (c.want[(kind, s, (max_dist, slack))] for s in G.SETTINGS)
            assert full["n_segments"].max() <= 8 and (cap2["n_segments"] == np.minimum(full["n_segments"], 2)).all()
            assert (floor4["n_segments"] <= full["n_segments"]).all() and (full["seg"]["offset"] != RS.INT32_MIN).all()
            assert full[9].tolist()[2:8] == (0,) * 6  # (the empty video)
    assert max(c.want[("index", (8, 1), p)]["n_segments"].max() for p in RH.GRID) == 8
    assert any((c.want[(k, (8, 4), p)]["n_segments"] < c.want[(k, (8, 1), p)]["n_segments"]).any() for k in G.KINDS for p in RH.GRID)
    # gapped positions are another problem, not the same one shifted
    assert all(c.want[("index", (8, 1), p)].tobytes() != c.want[("gapped", (8, 1), p)].tobytes() for p in RH.GRID)


def test_wide_reels_case_is_shared_and_read_only():
    a, b = G.wide_reels_case(300), G.wide_reels_case(300)
    assert a is b
    with pytest.raises(ValueError):
        a.want[("index", (8, 1), (31, 1))]["q_hits"][0] = 1
    with pytest.raises(ValueError):
        a.frames[0, 0] = 1


# ---- case 1: the model is the restatement, and the skip is at work ----

@functools.lru_cache(maxsize=None)
def case_1_model(n_source, kind):
    """{(setting, point): (records, traces)} of the model without a fault."""
    c = G.wide_reels_case(n_source)
    out = {}
    for max_dist, slack in RH.GRID:
        got = model(c.frames, c.offsets, c.positions[kind], c.pairs, W, slack, max_dist, G.SETTINGS)
        out.update({(setting, (max_dist, slack)): v for setting, v in got.items()})
    return out


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("n_source", [300, 600])
def test_the_model_reproduces_the_restatement_over_the_grid(n_source, kind):
    c = G.wide_reels_case(n_source)
    for (setting, point), (got, _) in case_1_model(n_source, kind).items():
        bad = differing(got, c.want[(kind, setting, point)])
        assert not bad.size, (setting, point, bad[:3])


def test_the_grid_exercises_the_bound_skip():
    total = {setting: dict(bound=0, again_less=0, floor=0, unled=0, evaluated=0) for setting in ((8, 1), (8, 4))}
    for n_source in (300, 600):
        for kind in G.KINDS:
            for (setting, _), (_, traces) in case_1_model(n_source, kind).items():
                if setting in total:
                    for t in traces:
                        if t is not None:
                            for what in total[setting]:
                                total[setting][what] += t[what]
    print(total)
    assert total[(8, 1)]["bound"] > 1000 and total[(8, 1)]["again_less"] > 1000 and total[(8, 1)]["floor"] == 0
    assert total[(8, 4)]["floor"] > 0 and total[(8, 4)]["bound"] > 0 and total[(8, 4)]["again_less"] > 0
    assert total[(8, 1)]["unled"] + total[(8, 4)]["unled"] > 0 and total[(8, 4)]["unled"] > 0


# ---- case 2: the tolerance edge ----

def test_edge_reels_sit_at_31_and_32_bits():
    vids, pairs = G.edge_reels()
    assert pairs == [(1, 0), (0, 2)] and [len(v) for v in vids] == [400, 36, 36]
    for reel, pieces in zip(vids[1:], (G.EDGE_A, G.EDGE_B)):
        idx = np.concatenate([np.floor(np.arange(n) * num / den + c + 0.5).astype(np.int64) for n, num, den, c in pieces])
        d = AH.hamming_matrix(reel, vids[0])
        assert d[np.arange(36), idx].tolist() == [31] * 20 + [32] * 16
        d[np.arange(36), idx] = 999
        assert d.min() > 32 and len(set(idx.tolist())) == 36
    frames, offsets = RH.join(vids)
    assert max(G.pair_bins(offsets, None, p, W, 1) for p in pairs) <= G.LDS_BINS
    want = {m: RS.align_rate_segments(frames, offsets, pairs, None, W, 1, m) for m in (30, 31, 32)}
    on = ("q_aligned", "t_aligned")
    for k, rates in enumerate((((8, 3), (7, 2)), ((1, 8), (5, 8)))):
        assert want[30][k].tolist()[2:7] == (0, 0, 0, 0, 0)
        assert want[31][k].tolist()[2:7] == (20, 20, 1, 20, 20) and want[32][k].tolist()[2:7] == (36, 36, 2, 36, 36)
        assert [tuple(s)[8:10] for s in segs(want[31][k])] == [rates[0]]
        assert [tuple(s)[8:10] for s in segs(want[32][k])] == list(rates)
        assert [int(s[on[k]]) for s in segs(want[32][k])] == [20, 16] and want[32][k]["seg"][0] == want[31][k]["seg"][0]


# ---- case 3: windows wider than the histogram, under taken sets ----

CASE_3 = G.CASE_3


def test_tiny_pairs_tie_at_slack_16_and_peel_tying_segments_at_slack_0():
    vids, pairs = RH.tiny_library()
    frames, offsets = RH.join(vids)
    assert max(n * 6 + d * 11 + 1 for n, d in W) == 131 < 2 * 128 + 1  # a window of 257 bins over a core of at most 131
    assert {(m, s) for _, m, s, _ in CASE_3} == {(31, 16), (127, 16), (127, 0)} and len(CASE_3) == 3 * 3 * 2
    for k, max_dist, slack, (K, floor) in CASE_3:
        rates = RH.rotated(W, k)
        want = RS.align_rate_segments(frames, offsets, pairs, None, rates, slack, max_dist, max_segments=K, min_band_votes=floor)
        if slack == 16:
            # the static 7 x 12 pair: one segment of 84 votes at list entry 0; the first band takes every frame
            assert want[3].tolist()[2:8] == (7, 12, 1, 7, 12, 0)
            assert want[3]["seg"][0].tolist() == (0, 84, 7, 12, 0, 6, 0, 11) + rates[0] + (0, 0)
            # even the narrowest window of slack 16, 33 bins at (1, 1), is wider than that rate's core of 7 + 12 - 1 bins: the
            # first band holds every hit of a pair at every rate, all rates tie, and no frame with a hit is left for a round 2
            assert want["n_segments"].max() == 1 and (want["seg"][:, 0]["rate_index"] == 0).all()
            assert want["q_hits"][5:].any() == (max_dist == 127)
            tops = [RH.rate_tops(vids[a], vids[b], max_dist=max_dist, slack=16, rates=rates) for a, b in pairs]
            assert all(len(set(t)) == 1 for t in tops)
        elif floor == 1:
            # the random 7 x 12 pairs at slack 0: a band of five votes, then segments of one vote, where every rate ties and
            # the first listed one keeps the segment
            assert (want["n_segments"] >= 3).sum() >= 2
            later = [s for r in want[8:] for s in segs(r)[1:]]
            assert len(later) >= 4 and all(s["band_votes"] == 1 and s["rate_index"] == 0 for s in later)
        else:
            assert want["n_segments"][8:].tolist() == [1, 1]  # the floor of two votes ends the pair at its second round


# ---- case 4: the top nibble bit in pass 2 and in later rounds ----

def test_an_eighth_entry_with_an_8_wins_segments_after_the_first():
    c = G.wide_reels_case(300)
    for max_dist, slack in ((31, 1), (31, 3)):
        eighth = later = 0
        for rates in RH.TOP_BIT_LISTS:
            want = RS.align_rate_segments(c.frames, c.offsets, c.pairs, None, rates, slack, max_dist)
            hits = [(k, has_8(s)) for r in want for k, s in enumerate(segs(r)) if s["rate_index"] == 7]
            if len(rates) == 8:  # every list with an eighth entry shows it
                assert any(e for _, e in hits) and 8 in rates[7], rates
            eighth += sum(e for _, e in hits)
            later += sum(e for k, e in hits if k >= 1)
        assert eighth >= 3 and later >= 1, (max_dist, slack, eighth, later)


# ---- case 5: the bin limit through a rate ----

def test_bin_limit_pairs_give_two_segments_of_one_vote():
    vids, positions, span_a, spans_b = RH.bin_limit_library()
    frames, offsets = RH.join(vids)
    for rates, pairs in ((((1, 1), (8, 1)), [(0, 1), (0, 2)]), (((1, 1), (1, 8)), [(1, 0), (2, 0)])):
        assert [G.pair_bins(offsets, positions, p, rates, 1) for p in pairs] == [1 << 20, (1 << 20) + 1]
        want = RS.align_rate_segments(frames, offsets, pairs, positions, rates, 1)
        sign = 1 if pairs[0] == (0, 1) else -1
        assert want[0].tolist()[2:8] == (2, 2, 2, 2, 2, 0) and want[1] == RS.lost_record(*pairs[1])
        assert [tuple(s)[:2] + tuple(s)[8:] for s in segs(want[0])] == [(-sign * span_a, 1, 1, 1, 0, 0),
                                                                        (sign * spans_b[0], 1, 1, 1, 0, 0)]
        # the two votes are the first and the last core bin of (1, 1)'s histogram
        dmin = (positions[2] - positions[1]) if sign == 1 else (positions[0] - positions[3])
        assert sorted(int(s["offset"]) - int(dmin) for s in segs(want[0])) == [0, span_a + spans_b[0]]
        alone = RS.align_rate_segments(frames, offsets, pairs, positions, rates[:1], 1)
        assert alone[0].tobytes() == want[0].tobytes() and alone[1]["n_segments"] == 2  # the rule is about ANY listed rate
        assert sorted(abs(int(s["offset"])) for s in segs(alone[1])) == [span_a, spans_b[1]]
    # the slot of the pair at the limit: histogram, a word of flags and a word of taken bits per side
    P = MD.Pair(frames, offsets, positions, 0, 1, ((1, 1), (8, 1)), 1)
    assert (P.bins, P.wa, P.wb, P.need) == (1 << 20, 1, 1, (1 << 20) + 2 * (1 + 1)) and P.need <= MD.slot_words(1 << 20)
    entries = [P, MD.Pair(frames, offsets, positions, 0, 2, ((1, 1), (8, 1)), 1)]
    want = RS.align_rate_segments(frames, offsets, [(0, 1), (0, 2)], positions, ((1, 1), (8, 1)), 1)
    for slot, first in ((P.need, want[0]), (P.need - 1, RS.lost_record(0, 1)), (0, RS.lost_record(0, 1))):
        got, traces = MD.model_call(entries, ((1, 1), (8, 1)), 1, 8, 1, slot, (), ONES)
        assert got[0].tobytes() == first.tobytes() and got[1].tobytes() == want[1].tobytes()
    # round 2 of the pair at the limit evaluates (1, 1) again and passes (8, 1) over: its bound of one vote cannot beat the tie
    got, traces = MD.model_call(entries, ((1, 1), (8, 1)), 1, 8, 1, P.need, (), ONES)
    assert traces[0]["evaluated"] == 3 and traces[0]["bound"] == 1


# ---- case 6: positions at the host entry's bound ----

def test_far_positions_give_offsets_near_two_to_the_23():
    vids, positions = RH.far_positions_library()
    frames, offsets = RH.join(vids)
    pairs = [(1, 0), (0, 1), (1, 1), (0, 0)]
    assert positions.max() == RH.MAX_POSITION
    for slack in (0, 1):
        for K in (8, 1):
            want = RS.align_rate_segments(frames, offsets, pairs, positions, W, slack, max_segments=K)
            assert want["seg"][:2, 0]["offset"].tolist() == [-8388541, 8388541] and want["seg"][:2, 0]["band_votes"].tolist() == [8, 8]
            assert [tuple(s)[8:11] for s in want["seg"][:2, 0]] == [(8, 1, 3), (1, 8, 4)] and want["n_segments"].tolist() == [1] * 4
            got = model(frames, offsets, positions, pairs, W, slack, 31, [(K, 1)])[(K, 1)][0]
            assert not differing(got, want).size
    assert max(G.pair_bins(offsets, positions, p, W, 1) for p in pairs) <= G.LDS_BINS


# ---- case 7: either side of the LDS limit ----

def test_lds_edge_pair_has_4096_and_4097_bins():
    vids, pairs = G.lds_edge_pair()
    frames, offsets = RH.join(vids)
    unit = ((1, 1),)
    assert [G.pair_bins(offsets, None, p, unit, 0) for p in pairs] == [G.LDS_BINS, G.LDS_BINS + 1]
    P = [MD.Pair(frames, offsets, G.index_positions(offsets), a, b, unit, 0) for a, b in pairs]
    assert (P[0].wa, P[0].wb, P[0].need) == (65, 64, 4096 + 2 * 129) and not P[0].big and P[0].need <= MD.LDS_WORDS
    assert P[1].big and P[1].need == 4097 + 2 * 130 <= MD.slot_words(4097)
    want = RS.align_rate_segments(frames, offsets, pairs, None, unit, 0)
    assert (want["n_segments"] >= 2).all() and want["seg"][:, :2]["q_aligned"].tolist() == [[300, 300]] * 2
    got, _ = MD.model_call(P, unit, 0, 8, 1, MD.slot_words(4097), (), ONES)
    assert not differing(got, want).size
    lost, _ = MD.model_call(P, unit, 0, 8, 1, 0, (), ONES)
    assert lost[0] == want[0] and lost[1] == RS.lost_record(0, 2)


# ---- what each case pins: the model with one line slipped, on the case's own input ----

def changed(frames, offsets, positions, pairs, rates, slack, max_dist, setting, fault, want):
    """Indices of the records that the fault changes; the model without a fault must give `want`."""
    right = model(frames, offsets, positions, pairs, rates, slack, max_dist, [setting])[setting][0]
    assert not differing(right, want).size, (fault, "the model without a fault is not the restatement")
    wrong = model(frames, offsets, positions, pairs, rates, slack, max_dist, [setting], (fault,))[setting][0]
    return differing(wrong, right)


def test_the_switches_are_listed_apart_from_the_many_pairs_faults():
    assert list(MD.GRID_FAULTS) == ["G1", "G2", "G3", "G4", "G5", "G6"] and not set(MD.GRID_FAULTS) & set(MD.FAULTS)


@pytest.mark.parametrize("fault", ["G1", "G2", "G5"])
def test_slack_slips_change_records_of_case_1_at_slack_16(fault):
    c = G.wide_reels_case(300)
    n = 0
    for max_dist in (30, 31, 32, 127):
        n += changed(c.frames, c.offsets, None, c.pairs, W, 16, max_dist, (8, 1), fault, c.want[("index", (8, 1), (max_dist, 16))]).size
    print(f"{fault} ({MD.GRID_FAULTS[fault]}): {n} records of case 1 at slack 16 change")
    assert n >= 4


def test_g6_changes_every_record_of_case_2():
    vids, pairs = G.edge_reels()
    frames, offsets = RH.join(vids)
    for max_dist in (31, 32):
        want = RS.align_rate_segments(frames, offsets, pairs, None, W, 1, max_dist)
        assert changed(frames, offsets, None, pairs, W, 1, max_dist, (8, 1), "G6", want).tolist() == [0, 1]
    # case 1's noisy reels (0..20 bits flipped) do not sit on a tolerance of the grid: the edge reels are needed
    c = G.wide_reels_case(300)
    assert not changed(c.frames, c.offsets, None, c.pairs[:6], W, 1, 31, (8, 1), "G6", c.want[("index", (8, 1), (31, 1))][:6]).size


@pytest.mark.parametrize("fault", ["G4", "G5"])
def test_tie_and_window_slips_change_records_of_case_3(fault):
    vids, pairs = RH.tiny_library()
    frames, offsets = RH.join(vids)
    n = 0
    for k, max_dist, slack, (K, floor) in CASE_3:
        rates = RH.rotated(W, k)
        want = RS.align_rate_segments(frames, offsets, pairs, None, rates, slack, max_dist, max_segments=K, min_band_votes=floor)
        bad = changed(frames, offsets, None, pairs, rates, slack, max_dist, (K, floor), fault, want)
        n += bad.size
        # (slack 0 has no window to clamp, and under a floor of two votes its pairs end at a first round that one rate wins alone)
        assert bad.size >= 1 or (slack == 0 and (fault == "G5" or floor == 2)), (fault, k, max_dist, slack, K, floor)
    print(f"{fault} ({MD.GRID_FAULTS[fault]}): {n} records of case 3 change")


def test_g3_changes_records_of_case_4():
    c = G.wide_reels_case(300)
    for max_dist, slack in ((31, 1), (31, 3)):
        for rates in RH.TOP_BIT_LISTS:
            want = RS.align_rate_segments(c.frames, c.offsets, c.pairs, None, rates, slack, max_dist)
            assert changed(c.frames, c.offsets, None, c.pairs, rates, slack, max_dist, (8, 1), "G3", want).size >= 1, rates
