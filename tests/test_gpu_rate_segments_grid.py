"""The rate-aware multi-segment alignment kernel over tolerances, slacks and rates up to 8 (run with -m gpu on an MI355X; DESIGN
4.18): the device entry hvd_dev_vpdq_align_rate_segments -- through test_gpu_rate_segments.dev_call / dev, whose record and scratch
buffers end in sentinel tails -- and the host entry search.align_rate_segments against the numpy restatement
rate_segments_helpers.align_rate_segments, which evaluates every rate in every round: record for record and all 104 words, by
equality (RS.same). The inputs are the builders of rate_segments_grid_helpers and rates_helpers;
tests/test_rate_segments_grid_cpu.py shows without a device that each does what its case needs, that a model of the kernel with
its bound-skip gives these records, and that a slip in the line a case pins changes that case's records.

What each case pins (csrc/k_valign_rate_segments.hip, csrc/hvd_valign_dev.h):
 1. Reels of three and four pieces at rates with an 8, over max_dist {0, 30, 31, 32, 127} x slack {0, 1, 3, 16}, at
    (max_segments, min_band_votes) (8, 1), (8, 4), (2, 1), on index and on gapped positions; a 300-frame source (on index
    positions every pair in the LDS launch, at most 7 * 101 + 8 * 299 + 1 + 256 = 3 356 bins) and a 600-frame one (every pair
    with the source in the scratch launch, at least 7 * 101 + 8 * 599 + 1 = 5 500 bins): `slack_r = slack * max(num, den)` of
    pass 1 and the `slack * max(num, den)` handed to pass 2, up to 128; `nbins = core + 2 * slack_r` inside a histogram sized by
    the largest bins_r, the flag and taken words behind it; `if (d > max_dist) continue` followed by the taken test at every
    tolerance; the bound-skip `u < min_band_votes || (win_r != R && u <= win_S)` where it passes rates over, for good, and
    lets them in again. At (127, 16) the first band takes nearly every frame and each pair has one segment; the point is run
    like every other.
 2. Reel frames at exactly 31 and 32 bits from their source frames, max_dist 30, 31, 32 -- no segment, piece 1 alone, both
    pieces: `if (d > max_dist) continue` of scan_pair where the taken test follows it.
 3. Pairs of 1 x 1 to 7 x 12 frames at slack 16 (windows of 33 to 257 bins over 19 to 131, the flag and taken words right
    behind), under three rotations of the list: the clamps `u0`, `u1` of best_offset<true>, `best.S > win_S` with every rate
    tying, and `q_covered >= A.n` ending the rounds of the static pair. At slack 16 no window leaves a hit behind, so no such
    pair has a second segment; the same pairs at slack 0 and max_dist 127 peel segments of one vote on which every rate ties
    in rounds after the first: `best.S > win_S` and the skip's `u <= win_S` there.
 4. Lists with an 8 in the eighth entry of nums or of dens (bit 31 of the word), alone, and in the first entry: the nibble unpack
    `(K.nums >> (4u * r)) & 15u` of pass 1 and `(K.nums >> (4u * win_r)) & 15u` of pass 2, in segments after the first.
 5. Two frames a side at positions [0, span]: exactly 2^20 bins at (8, 1) or (1, 8) is aligned (two segments of one vote, the
    first and the last core bin of (1, 1)), one bin more is the INT32_MIN record (host entry: HVD_ERR_ARG): `g.bad = g.bins >
    kMaxBins` over the largest bins_r. The slot-fit test `nbins_max + 2 * (wa + wb) > slot_words` at 2^20 + 4 words and at one
    word less.
 6. Positions that end at 2^20 - 1, the largest the host entry takes: offsets of -+8 388 541; this kernel's
    `dmin = den * (uint32_t)P.pb0 - num * (uint32_t)P.pa1` and the staged `num * p_a`.
 7. 2 049 x 2 048 frames under [(1, 1)] at slack 0: exactly 4 096 bins and 65 + 64 words a run, the flag and taken words closest
    to the end of `lds_words`; one frame more is the scratch launch's: `geo.big() != BIG`.
 8. The header's identities on the device entries' own records at every grid point of case 1: q_hits / t_hits are
    hvd_dev_vpdq_align_videos', under [(1, 1)] the head and words 0-7 of every segment are k_valign_segments', and with
    max_segments = 1 and min_band_votes = 1 segment 0 is k_valign_rates' record.
Measured on an MI355X: the whole file runs in 4.6 s, the restatement's records of case 1 included (the slowest test, the device
entry of the 600-frame source on index positions, 1.3 s); case 5, six of whose calls have a scratch of 64 slots of 2^20 bins,
runs in 0.11 s."""
import numpy as np
import pytest

import rate_segments_grid_helpers as G
import rate_segments_helpers as RS
import rates_helpers as RH
from test_gpu_align import dev_align
from test_gpu_rate_segments import HEAD, LDS_BINS, SLOTS, dev, dev_call
from test_gpu_rates import dev_rates
from test_gpu_segments import dev_segments

pytestmark = pytest.mark.gpu

W = RH.WIDE_RATES
_dev = {}


def has_8(seg):
    return 8 in (int(seg["rate_num"]), int(seg["rate_den"]))


def dev_grid(gpu, n_source, kind):
    """The device entry's records of wide_reels_case(n_source) under W, at every setting and grid point: one run, shared by
    cases 1 and 8. The scratch is hvd_rate_segments_scratch_bytes of the largest bins_r of the library (none at all for the
    300-frame source on index positions)."""
    if (n_source, kind) not in _dev:
        c = G.wide_reels_case(n_source)
        pos = c.positions[kind]
        big = c.max_bins(kind)
        assert (big <= LDS_BINS) == ((n_source, kind) == (300, "index"))
        _dev[(n_source, kind)] = {
            (setting, (m, s)): dev(gpu, c.frames, c.offsets, pos, c.frames, c.offsets, pos, c.pairs, W, m, s, setting[0], setting[1],
                                   scratch_bins=big if big > LDS_BINS else 0)
            for setting in G.SETTINGS for m, s in RH.GRID}
    return _dev[(n_source, kind)]


# ---- case 1 ----

@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("n_source", [300, 600])
def test_wide_reels_grid_device_entry(gpu, hvd, n_source, kind):
    c = G.wide_reels_case(n_source)
    if kind == "index":
        for max_dist, slack in RH.GRID:
            full = c.want[("index", (8, 1), (max_dist, slack))]
            if 0 < max_dist < 127 and slack <= 3:
                assert (full["n_segments"] >= 3).sum() >= 4
                assert any(has_8(s) for r in full for s in r["seg"][1:r["n_segments"]])
    got = dev_grid(gpu, n_source, kind)
    for setting in G.SETTINGS:
        for point in RH.GRID:
            RS.same(got[(setting, point)], c.want[(kind, setting, point)])


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("n_source", [300, 600])
def test_wide_reels_grid_host_entry(gpu, hvd, n_source, kind):
    c = G.wide_reels_case(n_source)
    for K, floor in G.SETTINGS:
        for max_dist, slack in RH.GRID:
            got = hvd.search.align_rate_segments(c.frames, c.offsets, c.pairs, c.positions[kind], W, slack, max_dist,
                                                 max_segments=K, min_band_votes=floor)
            RS.same(got, c.want[(kind, (K, floor), (max_dist, slack))])


# ---- case 2 ----

def test_tolerance_edge_at_31_and_32_bits(gpu, hvd):
    vids, pairs = G.edge_reels()
    frames, offsets = RH.join(vids)
    for max_dist in (30, 31, 32):
        want = RS.align_rate_segments(frames, offsets, pairs, None, W, 1, max_dist)
        assert want["n_segments"].tolist() == [{30: 0, 31: 1, 32: 2}[max_dist]] * 2
        assert want["q_hits"].tolist() == [{30: 0, 31: 20, 32: 36}[max_dist]] * 2
        if max_dist == 32:  # piece 1, then piece 2, each at its rate
            assert [[tuple(s)[8:10] for s in r["seg"][:2]] for r in want] == [[(8, 3), (7, 2)], [(1, 8), (5, 8)]]
            assert want["seg"][:, :2]["band_votes"].tolist() == [[20, 16]] * 2
        RS.same(dev(gpu, frames, offsets, None, frames, offsets, None, pairs, W, max_dist, 1), want)
        RS.same(hvd.search.align_rate_segments(frames, offsets, pairs, None, W, 1, max_dist), want)


# ---- case 3 ----

def test_windows_wider_than_the_histogram_and_ties_under_taken_sets(gpu, hvd):
    vids, pairs = RH.tiny_library()
    frames, offsets = RH.join(vids)
    for k, max_dist, slack, (K, floor) in G.CASE_3:
        rates = RH.rotated(W, k)
        want = RS.align_rate_segments(frames, offsets, pairs, None, rates, slack, max_dist, max_segments=K, min_band_votes=floor)
        if slack == 16:  # the static 7 x 12 pair: one segment of 84 votes at list entry 0, every frame taken
            assert want[3].tolist()[2:8] == (7, 12, 1, 7, 12, 0)
            assert want[3]["seg"][0].tolist() == (0, 84, 7, 12, 0, 6, 0, 11) + rates[0] + (0, 0)
        elif floor == 1:  # the random 7 x 12 pairs: segments of one vote after the first, every rate tying
            assert (want["n_segments"] >= 3).sum() >= 1
        RS.same(dev(gpu, frames, offsets, None, frames, offsets, None, pairs, rates, max_dist, slack, K, floor), want)
        RS.same(hvd.search.align_rate_segments(frames, offsets, pairs, None, rates, slack, max_dist, max_segments=K,
                                               min_band_votes=floor), want)


# ---- case 4 ----

def test_top_nibble_bit_in_pass_2_and_in_later_rounds(gpu, hvd):
    c = G.wide_reels_case(300)
    for max_dist, slack in ((31, 1), (31, 3)):
        eighth = later = 0
        for rates in RH.TOP_BIT_LISTS:
            want = RS.align_rate_segments(c.frames, c.offsets, c.pairs, None, rates, slack, max_dist)
            at_7 = [k for r in want for k, s in enumerate(r["seg"][:r["n_segments"]]) if s["rate_index"] == 7 and has_8(s)]
            eighth, later = eighth + len(at_7), later + sum(k >= 1 for k in at_7)
            RS.same(dev(gpu, c.frames, c.offsets, None, c.frames, c.offsets, None, c.pairs, rates, max_dist, slack), want)
            RS.same(hvd.search.align_rate_segments(c.frames, c.offsets, c.pairs, None, rates, slack, max_dist), want)
        assert eighth >= 1 and later >= 1


# ---- case 5 ----

def test_bin_limit_through_a_rate_and_the_slot_fit_at_the_limit(gpu, hvd):
    vids, positions, span_a, spans_b = RH.bin_limit_library()
    frames, offsets = RH.join(vids)
    need = SLOTS * 4 * ((1 << 20) + 2 * (1 + 1))  # a slot: the histogram, a flag word and a taken word per side
    for rates, pairs in ((((1, 1), (8, 1)), [(0, 1), (0, 2)]), (((1, 1), (1, 8)), [(1, 0), (2, 0)])):
        args = (gpu, frames, offsets, positions, frames, offsets, positions, pairs)
        want = RS.align_rate_segments(frames, offsets, pairs, positions, rates, 1)
        assert want[0].tolist()[4:7] == (2, 2, 2) and want[1] == RS.lost_record(*pairs[1])
        assert [tuple(s)[1:4] + tuple(s)[8:] for s in want[0]["seg"][:2]] == [(1, 1, 1, 1, 1, 0, 0)] * 2
        assert sorted(abs(int(d)) for d in want[0]["seg"][:2]["offset"]) == [span_a, spans_b[0]]  # the first and the last core bin
        RS.same(dev(*args, rates, scratch_bins=1 << 20), want)
        RS.same(hvd.search.align_rate_segments(frames, offsets, pairs[:1], positions, rates), want[:1])
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_rate_segments(frames, offsets, pairs[1:], positions, rates)
        assert e.value.code == gpu.HVD_ERR_ARG
        # the slot fit: told of exactly 64 slots of 2^20 + 4 words the pair at the limit is aligned, told of 16 bytes less it is
        # lost; without scratch it is lost and nothing is written past the records
        lost = np.array([RS.lost_record(*p) for p in pairs], dtype=RS.VRSEGMENTS_DTYPE)
        RS.same(dev(*args, rates, scratch_bins=1 << 20, scratch_bytes=need), want)
        RS.same(dev(*args, rates, scratch_bins=1 << 20, scratch_bytes=need - 16), lost)
        RS.same(dev(*args, rates, scratch_bins=0), lost)
        # the same pairs under [(1, 1)] alone are ordinary records
        alone = RS.align_rate_segments(frames, offsets, pairs, positions, rates[:1], 1)
        assert alone[0].tobytes() == want[0].tobytes() and alone[1]["n_segments"] == 2
        RS.same(dev(*args, rates[:1], scratch_bins=span_a + spans_b[1] + 3), alone)
        RS.same(hvd.search.align_rate_segments(frames, offsets, pairs, positions, rates[:1]), alone)


# ---- case 6 ----

def test_positions_at_the_host_entrys_bound(gpu, hvd):
    vids, positions = RH.far_positions_library()
    frames, offsets = RH.join(vids)
    pairs = [(1, 0), (0, 1), (1, 1), (0, 0)]
    for slack in (0, 1):
        for K, floor in ((8, 1), (1, 1)):
            want = RS.align_rate_segments(frames, offsets, pairs, positions, W, slack, max_segments=K, min_band_votes=floor)
            assert want["seg"][:2, 0]["offset"].tolist() == [-8388541, 8388541] and want["seg"][:2, 0]["band_votes"].tolist() == [8, 8]
            RS.same(dev(gpu, frames, offsets, positions, frames, offsets, positions, pairs, W, 31, slack, K, floor), want)
            RS.same(hvd.search.align_rate_segments(frames, offsets, pairs, positions, W, slack, max_segments=K,
                                                   min_band_votes=floor), want)
    with pytest.raises(gpu.HvdError) as e:  # one more is past the bound
        hvd.search.align_rate_segments(frames, offsets, pairs, positions + (positions > 59), W)
    assert e.value.code == gpu.HVD_ERR_ARG


# ---- case 7 ----

def test_either_side_of_the_lds_limit_with_the_longest_bit_words(gpu, hvd):
    vids, pairs = G.lds_edge_pair()
    frames, offsets = RH.join(vids)
    unit = ((1, 1),)
    assert [G.pair_bins(offsets, None, p, unit, 0) for p in pairs] == [LDS_BINS, LDS_BINS + 1]
    want = RS.align_rate_segments(frames, offsets, pairs, None, unit, 0)
    assert (want["n_segments"] >= 2).all()
    args = (gpu, frames, offsets, None, frames, offsets, None, pairs, unit, 31, 0)
    lost = want.copy()
    lost[1] = RS.lost_record(*pairs[1])
    RS.same(dev(*args, scratch_bins=0), lost)  # 4 096 bins: the LDS launch, no scratch at all; 4 097: lost without scratch
    RS.same(dev(*args, scratch_bins=LDS_BINS + 1), want)
    RS.same(hvd.search.align_rate_segments(frames, offsets, pairs, None, unit, 0), want)


# ---- case 8 ----

@pytest.mark.parametrize("n_source", [300, 600])
def test_the_headers_identities_on_the_device_entries_own_records(gpu, hvd, n_source):
    c = G.wide_reels_case(n_source)
    lib = (c.frames, c.offsets, None, c.frames, c.offsets, None, c.pairs)
    wide = dev_grid(gpu, n_source, "index")
    big = c.max_bins("index")
    big = big if big > LDS_BINS else 0
    for max_dist, slack in RH.GRID:
        single = dev_align(gpu, *lib, max_dist, slack, 0)  # (at most 299 + 599 + 1 + 32 bins)
        for setting in G.SETTINGS:  # the counters are the pair's, whatever the limits
            full = wide[(setting, (max_dist, slack))]
            assert np.array_equal(full["q_hits"], single["q_hits"]) and np.array_equal(full["t_hits"], single["t_hits"])
        # (a) the unit list is the slope-one peel
        peel = dev_segments(gpu, *lib, max_dist, slack, 8, 1, 0)
        unit = dev(gpu, *lib, ((1, 1),), max_dist, slack)
        for u, s in zip(unit, peel):
            assert [u[n] for n in HEAD] == [s[n] for n in HEAD]
            assert [x.tolist()[:8] for x in u["seg"]] == [x.tolist() for x in s["seg"]]
            n = int(s["n_segments"])
            assert [x.tolist()[8:] for x in u["seg"]] == [(1, 1, 0, 0)] * n + [(0, 0, 0, 0)] * (8 - n)
        # (b) one segment is the rate alignment
        line = dev_rates(gpu, *lib, W, max_dist, slack, scratch_bins=big)
        one = dev(gpu, *lib, W, max_dist, slack, 1, 1, scratch_bins=big)
        for g, r in zip(one, line):
            assert g.tolist()[:4] == r.tolist()[:4] and g["seg"][0].tolist() == r.tolist()[4:]
            assert g["n_segments"] == (1 if r["q_hits"] else 0) and not g["seg"][1:].view(np.uint32).any()
        # ... and the first segment of every other setting
        assert np.array_equal(wide[((8, 1), (max_dist, slack))]["seg"][:, 0], one["seg"][:, 0])
