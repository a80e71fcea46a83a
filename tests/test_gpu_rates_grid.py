"""The rate-aware alignment kernel over tolerances, slacks and rates up to 8 (run with -m gpu on an MI355X): the
device entry hvd_dev_vpdq_align_rates -- through test_gpu_rates.dev_rates, whose record and scratch buffers end in sentinel
tails -- and the host entry search.align_rates against the numpy restatement rates_helpers.align_rates, record for record and
all sixteen words, by equality. The inputs are rates_helpers' builders; tests/test_rates_grid_cpu.py shows on the restatement
that each does what its case needs, and that a slip in the line a case pins changes that case's records.

What each case pins (csrc/k_valign_rates.hip, csrc/hvd_valign_dev.h):
 1. Wide-rate libraries over max_dist {0, 30, 31, 32, 127} x slack {0, 1, 3, 16}, a 300-frame source (every pair in the LDS
    launch, at most 2 894 bins) and a 600-frame one (every pair with the source in the scratch launch, at least 4 849 bins):
    `slack_r = slack * max(num, den)` of the rounds (pass 1: where the votes land, `nbins`, the window of `best_offset`) and the
    `slack * max(num, den)` handed to pass 2 (the aligned sets), up to slack_r = 128; the sizing by the largest bins_r.
 2. Clip frames at exactly 31 and 32 bits from their source frames, max_dist 30, 31, 32: `if (d > max_dist) continue` of
    scan_pair.
 3. Pairs of 1 x 1 to 7 x 12 frames at slack 16 (a window of 257 bins over at most 131): the clamps `u0`, `u1` of
    best_offset; every rate ties, under three rotations of the list: `best.S > win_S`, ties to the earlier rate. On the pairs
    of case 1 that do not tie, a rotated list changes rate_index alone (the header's consequence (d)).
 4. Lists with an 8 -- alone, in the eighth entry of nums and of dens (bit 31 of the word), in the first and the eighth: the
    nibble unpack `(nums >> 4r) & 15` of pair_geometry and of the rounds, and rate_list_length.
 5. Two frames a side at positions [0, span]: exactly 2^20 bins at (8, 1) or (1, 8) is aligned out of scratch sized by
    hvd_rates_scratch_bytes(1 << 20), one bin more is the INT32_MIN record (host entry: HVD_ERR_ARG) although (1, 1) alone
    aligns the pair: `g.bad = g.bins > kMaxBins` over the largest bins_r. The two hits are the first and the last core bin.
    Positions that end at 2^20 - 1, the largest the host entry takes: offsets of -+8 388 541, `dmin` in unsigned arithmetic
    (`den * (uint32_t)P.pb0 - num * (uint32_t)P.pa1`) and the staged `num * p_a`.
 6. The header's consequences (b) and (c) at every grid point of case 1, against hvd_dev_vpdq_align_videos: q_hits / t_hits
    are its counters, band_votes is at least its band's, and under [(1, 1)] words 0-11 are its record.
 7. k_valign_segments at the grid points tests/test_gpu_segments.py leaves out (max_dist 30, 32; slack 16), against
    segments_helpers.align_segments: `best_offset`'s window of 33 reads under the taken sets.
The calls at 2^20 bins are quick on an MI355X (the whole of case 5 ran in 0.1 s): its lists are the issue's two entries."""
import numpy as np
import pytest

import rates_helpers as RH
import segments_helpers as SH
from test_gpu_align import all_pairs, dev_align, gapped_positions
from test_gpu_rates import LDS_BINS, dev_rates, same
from test_gpu_segments import dev_segments

pytestmark = pytest.mark.gpu

W = RH.WIDE_RATES
_dev = {}


def scratch_bins(n_source):
    """What the scratch of a call on wide_library(n_source) is sized for: the largest bins_r of any pair at slack 16."""
    _, _, pairs, _ = RH.wide_case(n_source)
    return max(RH.wide_bins(n_source, 16, p) for p in pairs)


def dev_grid(gpu, n_source):
    """The device entry's records of wide_library(n_source) under W at every grid point: one run, shared by cases 1, 3 and 6."""
    if n_source not in _dev:
        frames, offsets, pairs, _ = RH.wide_case(n_source)
        _dev[n_source] = {(m, s): dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, W, m, s,
                                            scratch_bins=scratch_bins(n_source)) for m, s in RH.GRID}
    return _dev[n_source]


# ---- case 1 ----

@pytest.mark.parametrize("n_source", [300, 600])
def test_wide_rates_grid_device_entry(gpu, hvd, n_source):
    _, _, pairs, want = RH.wide_case(n_source)
    source_pairs = [p for p in pairs if 0 in p and 12 not in p]
    for slack in (0, 1, 3, 16):
        if n_source == 300:  # the LDS launch: no scratch is needed (and none is given: hvd_rates_scratch_bytes is 0)
            assert max(RH.wide_bins(300, slack, p) for p in pairs) <= 2894 <= LDS_BINS
        else:                # the scratch launch, with hvd_rates_scratch_bytes of the computed maximum
            assert min(RH.wide_bins(600, slack, p) for p in source_pairs) >= 4849 > LDS_BINS
    assert scratch_bins(n_source) == 7 * 35 + 8 * (n_source - 1) + 1 + 256
    got = dev_grid(gpu, n_source)
    for key in RH.GRID:
        same(got[key], want[key])


@pytest.mark.parametrize("n_source", [300, 600])
def test_wide_rates_grid_host_entry(gpu, hvd, n_source):
    frames, offsets, pairs, want = RH.wide_case(n_source)
    for max_dist, slack in RH.GRID:
        same(hvd.search.align_rates(frames, offsets, pairs, None, W, slack, max_dist), want[(max_dist, slack)])


# ---- case 2 ----

def test_tolerance_edge_at_31_and_32_bits(gpu, hvd):
    vids, pairs = RH.edge_library()
    frames, offsets = RH.join(vids)
    for max_dist in (30, 31, 32):
        want = RH.align_rates(frames, offsets, pairs, None, W, 1, max_dist)
        assert want["q_hits"][:8].tolist() == [{30: 0, 31: 18, 32: 36}[max_dist]] * 8
        same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, W, max_dist, 1), want)
        same(hvd.search.align_rates(frames, offsets, pairs, None, W, 1, max_dist), want)


# ---- case 3 ----

def test_windows_wider_than_the_histogram_and_ties_across_rates(gpu, hvd):
    vids, pairs = RH.tiny_library()
    frames, offsets = RH.join(vids)
    for k in (0, 3, 5):
        rates = RH.rotated(W, k)
        for max_dist in (31, 127):
            want = RH.align_rates(frames, offsets, pairs, None, rates, 16, max_dist)
            assert want[3].tolist()[2:] == (7, 12, 0, 84, 7, 12, 0, 6, 0, 11) + rates[0] + (0, 0)
            same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, rates, max_dist, 16), want)
            same(hvd.search.align_rates(frames, offsets, pairs, None, rates, 16, max_dist), want)


def test_reordering_changes_rate_index_alone_where_no_rates_tie(gpu, hvd):
    """Consequence (d) on the device entry's own records: the 300-frame library under two rotations of W."""
    frames, offsets, pairs, _ = RH.wide_case(300)
    for max_dist, slack in RH.REORDER_POINTS:
        first = dev_grid(gpu, 300)[(max_dist, slack)]
        loose = RH.non_tying(frames, offsets, pairs, max_dist, slack)
        assert len(loose) >= 9
        for k in (3, 5):
            rates = RH.rotated(W, k)
            turned = dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, rates, max_dist, slack)
            same(turned, RH.align_rates(frames, offsets, pairs, None, rates, slack, max_dist))
            for p in loose:
                assert turned[p].tolist()[:14] == first[p].tolist()[:14] and turned[p]["reserved"] == 0
                assert (turned[p]["rate_index"] + k) % 8 == first[p]["rate_index"]


# ---- case 4 ----

def test_top_nibble_bit_and_the_eighth_entry(gpu, hvd):
    frames, offsets, pairs, _ = RH.wide_case(300)
    for rates in RH.TOP_BIT_LISTS:
        want = RH.align_rates(frames, offsets, pairs, None, rates, 1, 31)
        assert len(rates) == 1 or want[W.index(rates[7])]["rate_index"] == 7
        same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, rates, 31, 1), want)
        same(hvd.search.align_rates(frames, offsets, pairs, None, rates, 1, 31), want)


# ---- case 5 ----

def test_bin_limit_through_a_rate(gpu, hvd):
    vids, positions, span_a, spans_b = RH.bin_limit_library()
    frames, offsets = RH.join(vids)
    for rates, pairs in ((((1, 1), (8, 1)), [(0, 1), (0, 2)]), (((1, 1), (1, 8)), [(1, 0), (2, 0)])):
        want = RH.align_rates(frames, offsets, pairs, positions, rates, 1)
        assert want[0]["band_votes"] == 1 and want[0]["rate_index"] == 0 and want[1].tolist()[2:] == RH.LOST
        got = dev_rates(gpu, frames, offsets, positions, frames, offsets, positions, pairs, rates, 31, 1, scratch_bins=1 << 20)
        same(got, want)
        same(hvd.search.align_rates(frames, offsets, pairs[:1], positions, rates), want[:1])
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_rates(frames, offsets, pairs[1:], positions, rates)
        assert e.value.code == gpu.HVD_ERR_ARG
        # the same pairs under [(1, 1)] alone are ordinary records
        alone = RH.align_rates(frames, offsets, pairs, positions, rates[:1], 1)
        assert alone[1].tolist()[2:] == want[0].tolist()[2:] and alone[0] == want[0]
        same(dev_rates(gpu, frames, offsets, positions, frames, offsets, positions, pairs, rates[:1], 31, 1,
                       scratch_bins=span_a + spans_b[1] + 3), alone)
        same(hvd.search.align_rates(frames, offsets, pairs, positions, rates[:1]), alone)
    # without scratch the pair at the limit is lost as well, and nothing is written past the records
    got = dev_rates(gpu, frames, offsets, positions, frames, offsets, positions, [(0, 1)], ((1, 1), (8, 1)), 31, 1, scratch_bins=0)
    assert got.tolist() == [(0, 1) + RH.LOST]


def test_positions_at_the_host_entrys_bound(gpu, hvd):
    vids, positions = RH.far_positions_library()
    frames, offsets = RH.join(vids)
    pairs = [(1, 0), (0, 1), (1, 1), (0, 0)]
    for slack in (0, 1):
        want = RH.align_rates(frames, offsets, pairs, positions, W, slack)
        assert want["offset"][:2].tolist() == [-8388541, 8388541] and want["band_votes"][:2].tolist() == [8, 8]
        same(dev_rates(gpu, frames, offsets, positions, frames, offsets, positions, pairs, W, 31, slack), want)
        same(hvd.search.align_rates(frames, offsets, pairs, positions, W, slack), want)
    with pytest.raises(gpu.HvdError) as e:  # one more is past the bound
        hvd.search.align_rates(frames, offsets, pairs, positions + (positions > 59), W)
    assert e.value.code == gpu.HVD_ERR_ARG


# ---- case 6 ----

@pytest.mark.parametrize("n_source", [300, 600])
def test_counters_and_unit_band_against_the_single_offset_kernel(gpu, hvd, n_source):
    frames, offsets, pairs, _ = RH.wide_case(n_source)
    wide = dev_grid(gpu, n_source)
    for max_dist, slack in RH.GRID:
        single = dev_align(gpu, frames, offsets, None, frames, offsets, None, pairs, max_dist, slack, 0)  # (668 bins at most)
        full = wide[(max_dist, slack)]
        assert np.array_equal(full["q_hits"], single["q_hits"]) and np.array_equal(full["t_hits"], single["t_hits"])  # (c)
        assert (full["band_votes"] >= single["band_votes"]).all()                                                    # (b)
        unit = dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, ((1, 1),), max_dist, slack)
        for s, u in zip(single, unit):                                                                               # (a)
            assert u.tolist()[:12] == s.tolist() and u.tolist()[12:] == ((1, 1, 0, 0) if s["q_hits"] else (0, 0, 0, 0))


# ---- case 7 ----

SEGMENT_POINTS = [(m, s) for m in (30, 32) for s in (0, 1, 3, 16)] + [(m, 16) for m in (0, 31, 127)]


@pytest.mark.parametrize("max_dist,slack", SEGMENT_POINTS)
def test_segments_at_the_grid_points_left_out(gpu, hvd, max_dist, slack):
    """test_gpu_segments.test_planted_pieces_match_the_reference at the remaining points of k_valign's 5 x 4 grid. (At
    max_dist 127 and slack 16 nearly half of all frame pairs hit and the first band takes almost every frame: 123 of the 150
    pairs have a segment, at most two have a second.)"""
    rng = np.random.default_rng(100 * slack + max_dist)
    frames, offsets = RH.join(SH.planted_pieces_library(1000 + max_dist, max_dist))
    pairs = all_pairs(len(offsets) - 1, rng)
    for positions in (None, gapped_positions(rng, offsets)):
        for K in (1, 2, 8):
            for floor in (1, 4):
                want = SH.align_segments(frames, offsets, pairs, positions, max_dist, slack, max_segments=K, min_band_votes=floor)
                if K == 8 and floor == 1 and max_dist:
                    assert (want["n_segments"] >= 2).sum() > 10 or (max_dist == 127 and (want["n_segments"] == 1).sum() > 100)
                SH.same(dev_segments(gpu, frames, offsets, positions, frames, offsets, positions, pairs, max_dist, slack, K, floor,
                                     0), want)
                SH.same(hvd.search.align_segments(frames, offsets, pairs, positions, max_dist, slack, max_segments=K,
                                                  min_band_votes=floor), want)
