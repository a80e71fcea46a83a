"""Rate-aware multi-segment time alignment on the GPU (run with -m gpu on an MI355X): k_valign_rate_segments against
the numpy restatement of the rule (tests/rate_segments_helpers.py), which evaluates every rate in every round where the kernel
passes rates over -- record for record and word for word, through the host entry, the device entry, Vpdq.align_rate_segments
and the chained pipeline. Every comparison is equality."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import align_helpers as AH
import rate_segments_helpers as RS
import rates_helpers as RH
import segments_helpers as SH
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

LDS_BINS = 4096   # HVD_ALIGN_LDS_BINS
LDS_GRID = 8192   # workgroups of the LDS launch at most (launch_lds_then_scratch)
SLOTS = 64        # workgroups of the scratch launch, one slot of the scratch each
REC = 416         # bytes of a record
HEAD = ("a", "b", "q_hits", "t_hits", "n_segments", "q_covered", "t_covered", "reserved")


def rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def bins_of(na_span, nb_span, rates, slack):
    return max(n * na_span + d * nb_span + 1 + 2 * slack * max(n, d) for n, d in rates)


def dev_call(gpu, fq, oq, pq, ft, ot, pt, pairs, rates, max_dist=31, slack=1, max_segments=8, min_band_votes=1, scratch_bins=0,
             scratch_bytes=None):
    """hvd_dev_vpdq_align_rate_segments with its own buffers: records and scratch end in sentinel tails that must stay intact.
    scratch_bytes: what the entry is TOLD it has (the buffer itself is sized for scratch_bins). -> (return code, records)."""
    lib = gpu.ensure()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.uint32)
    rates = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).reshape(-1, 2))
    M = pairs.shape[0]
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_rate_segments_scratch_bytes(scratch_bins, C.byref(sb)))
    told = sb.value if scratch_bytes is None else scratch_bytes
    assert told <= sb.value
    up = lambda x: gpu.DeviceBuffer.from_array(x) if x is not None and x.size else None  # noqa: E731
    bufs = dict(fq=up(fq), oq=up(np.asarray(oq, np.int64)), pq=up(None if pq is None else np.asarray(pq, np.int32)),
                ft=up(ft), ot=up(np.asarray(ot, np.int64)), pt=up(None if pt is None else np.asarray(pt, np.int32)),
                pairs=up(pairs), out=_sentinel_buffer(gpu, REC * M), scr=_sentinel_buffer(gpu, sb.value) if sb.value else None)
    ptr = lambda k: bufs[k].ptr if bufs[k] is not None else None  # noqa: E731
    try:
        rc = lib.hvd_dev_vpdq_align_rate_segments(ptr("fq"), ptr("oq"), len(oq) - 1, ptr("pq"), ptr("ft"), ptr("ot"), len(ot) - 1,
                                                  ptr("pt"), ptr("pairs"), M, max_dist, slack, rates.ctypes.data, rates.shape[0],
                                                  max_segments, min_band_votes, ptr("scr"), told, ptr("out"))
        gpu.check(lib.hvd_dev_sync())
        out = bufs["out"].to_array(RS.VRSEGMENTS_DTYPE, M)
        assert _tail_intact(gpu, bufs["out"], REC * M), "record buffer overrun"
        assert bufs["scr"] is None or _tail_intact(gpu, bufs["scr"], sb.value), "scratch overrun"
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return rc, out


def dev(gpu, *args, **kwargs):
    rc, out = dev_call(gpu, *args, **kwargs)
    gpu.check(rc)
    return out


def restated(frames, offsets, pairs, *args, **kwargs):
    """RS.align_rate_segments, computed once per distinct pair of the list."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    return RS.align_rate_segments(frames, offsets, uniq, *args, **kwargs)[inv.reshape(-1)]


# ---- the reels, LDS form ----

@pytest.fixture(scope="module")
def reels():
    source, b = RS.reel_b()
    source_c, c = RS.reel_c()
    frames, offsets = RH.join([b, source, c, source_c])
    return frames, offsets, [(0, 1), (1, 0), (2, 3), (3, 2)]


@pytest.mark.parametrize("listed", ["default", "with_half"])
def test_reels_as_a_and_as_b(gpu, hvd, reels, listed):
    frames, offsets, pairs = reels
    rates = RH.DEFAULT_RATES if listed == "default" else RH.list_with((1, 2))
    assert max(bins_of(149, 599, rates, 1), bins_of(599, 149, rates, 1)) <= LDS_BINS  # the LDS form
    for floor in (1, 4):
        for K in (1, 3, 8):
            want = RS.align_rate_segments(frames, offsets, pairs, None, rates, max_segments=K, min_band_votes=floor)
            if K == 8 and listed == "default":  # the records of the proposal: reel B in four segments, reel C in three
                assert [tuple(s)[8:10] for s in want[0]["seg"][:4]] == [(5, 4), (3, 2), (2, 1), (1, 1)]
                assert want[0].tolist()[4:7] == (4, 150, 150) and want[2].tolist()[4:7] == (3, 90, 90)
                assert want[2]["seg"][:3]["offset"].tolist() == [-9, 60, 300]
            if K == 8 and listed == "with_half":  # (1, 2) in place of (2, 1): the reels are whole as the b side
                assert want[3].tolist()[4:7] == (3, 90, 90) and want[3]["seg"][:3]["rate_index"].tolist() == [7, 7, 7]
                assert want[3]["seg"][:3]["offset"].tolist() == [9, -60, -300]
            RS.same(hvd.search.align_rate_segments(frames, offsets, pairs, rates=rates, max_segments=K, min_band_votes=floor), want)
            RS.same(dev(gpu, frames, offsets, None, frames, offsets, None, pairs, rates, max_segments=K, min_band_votes=floor), want)
            if floor == 1:
                for (a, b), w in zip(pairs, want):
                    rec = hvd.Vpdq.align_rate_segments(frames[offsets[a]:offsets[a + 1]].tobytes(),
                                                       hvd.VpdqHash(frames[offsets[b]:offsets[b + 1]].tobytes()), rates=rates,
                                                       max_segments=K)
                    assert [rec[n] for n in HEAD] == [0, 1] + [w[n] for n in HEAD[2:]] and (rec["seg"] == w["seg"]).all()


# ---- the identities on the device ----

def test_unit_list_is_the_slope_one_peel(gpu, hvd):
    """(a): rates = [(1, 1)] against search.align_segments on the planted pieces -- the head and words 0-7 of every segment word
    for word, 1, 1, 0, 0 behind every used one -- at slack 0, 1 and 3, on index and on gapped positions."""
    vids = SH.planted_pieces_library(81, 31)
    assert [len(v) for v in vids] == [0, 1, 2, 3, 17, 64, 65, 130, 255, 256, 257, 300]
    frames, offsets = RH.join(vids)
    V = len(vids)
    rng = np.random.default_rng(81)
    pairs = [(v - 1, v) for v in range(1, V)] + [(v, v - 1) for v in range(1, V)] + [(11, 11), (4, 9), (10, 5)]
    for positions in (None, SH.gapped(rng, offsets)):
        for slack in (0, 1, 3):
            for floor in (1, 3):
                peel = hvd.search.align_segments(frames, offsets, pairs, positions, slack=slack, min_band_votes=floor)
                got = hvd.search.align_rate_segments(frames, offsets, pairs, positions, ((1, 1),), slack, min_band_votes=floor)
                for g, s in zip(got, peel):
                    assert [g[n] for n in HEAD] == [s[n] for n in HEAD]
                    assert [x.tolist()[:8] for x in g["seg"]] == [x.tolist() for x in s["seg"]]
                    assert [x.tolist()[8:] for x in g["seg"]] == [(1, 1, 0, 0)] * int(s["n_segments"]) + [(0, 0, 0, 0)] * (
                        8 - int(s["n_segments"]))
                RS.same(got, RS.align_rate_segments(frames, offsets, pairs, positions, ((1, 1),), slack, min_band_votes=floor))
        assert (peel["n_segments"] >= 2).sum() >= 6
    # the whole list on the same pairs: device entry and host entry
    want = RS.align_rate_segments(frames, offsets, pairs, positions, RH.DEFAULT_RATES, 1)
    big = bins_of(1000, 1000, RH.DEFAULT_RATES, 1)  # (gapped positions of 300 frames pass the LDS limit at the wider rates)
    RS.same(dev(gpu, frames, offsets, positions, frames, offsets, positions, pairs, RH.DEFAULT_RATES, scratch_bins=big), want)
    RS.same(hvd.search.align_rate_segments(frames, offsets, pairs, positions), want)


def test_one_segment_is_the_rate_alignment(gpu, hvd):
    """(b): max_segments = 1, min_band_votes = 1 against search.align_rates on every ordered pair of the mixed library -- its
    static 20 x 33 pair included, where every frame hits every frame and the bands of the rates differ by their widths alone. (c): the counters are those
    of every other K and list."""
    frames, offsets = RH.join(RH.mixed_library(82))
    V = len(offsets) - 1
    pairs = [(a, b) for a in range(V) for b in range(V)]
    line = hvd.search.align_rates(frames, offsets, pairs)
    got = hvd.search.align_rate_segments(frames, offsets, pairs, max_segments=1)
    for g, r in zip(got, line):
        assert g.tolist()[:4] == r.tolist()[:4] and g["seg"][0].tolist() == r.tolist()[4:]
        assert g["n_segments"] == (1 if r["q_hits"] else 0) and not g["seg"][1:].view(np.uint32).any()
    static = pairs.index((7, 8))
    assert got[static]["seg"][0]["band_votes"] > got[static]["t_hits"] == 33  # every frame hits every frame: bands of many votes
    RS.same(got, RS.align_rate_segments(frames, offsets, pairs, max_segments=1))
    want = RS.align_rate_segments(frames, offsets, pairs)
    full = dev(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES)
    RS.same(full, want)
    assert np.array_equal(full["q_hits"], line["q_hits"]) and np.array_equal(full["t_hits"], line["t_hits"])
    assert (full["n_segments"] >= 2).sum() >= 4
    for rec in full:  # (d)
        segs = rec["seg"][:rec["n_segments"]]
        assert (np.diff(segs["band_votes"].astype(np.int64)) <= 0).all()
        assert (segs["q_aligned"] <= segs["band_votes"]).all() and (segs["t_aligned"] <= segs["band_votes"]).all()
    three = dev(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES[:3], max_segments=3, min_band_votes=2)
    RS.same(three, RS.align_rate_segments(frames, offsets, pairs, None, RH.DEFAULT_RATES[:3], max_segments=3, min_band_votes=2))
    assert np.array_equal(three["q_hits"], line["q_hits"]) and np.array_equal(three["t_hits"], line["t_hits"])


# ---- chunk and lane-split edges ----

def test_chunk_and_lane_split_edges(gpu, hvd):
    """na in {1, 255, 256, 257, 513} (the 256-frame chunks of video a) against nb in {1, 3, 255, 256, 257} (one frame of b per
    lane; short b sides dealt over 256 // nb lanes): a is a prefix of one source, b holds two pieces of that source, one run
    through at 5/4 and one at 2/3, so that a pair has two segments at two rates where a is long enough. Index positions, and
    positions with gaps at slack 2."""
    rng = np.random.default_rng(83)
    S = rand(rng, 513)
    a_vids = [S[:n].copy() for n in (1, 255, 256, 257, 513)]
    b_vids = []
    for n in (1, 3, 255, 256, 257):
        first = n // 2
        pieces = [RH.resampled(S, m, num, den, c) for m, num, den, c in ((first, 5, 4, 0.3), (n - first, 2, 3, 200.4)) if m]
        b_vids.append(AH.noisy(rng, np.concatenate(pieces), 20))
    fq, oq = RH.join(a_vids)
    ft, ot = RH.join(b_vids)
    pairs = [(a, b) for a in range(5) for b in range(5)]
    gaps = lambda off: np.concatenate([int(rng.integers(0, 5)) + np.cumsum(rng.integers(1, 3, int(n)))  # noqa: E731
                                       for n in np.diff(off)]).astype(np.int32)
    for pq, pt, slack in ((None, None, 1), (gaps(oq), gaps(ot), 2)):
        want = RS.align_rate_segments(fq, oq, pairs, pq, RH.DEFAULT_RATES, slack, 31, ft, ot, pt)
        if pq is None:  # 513 x 257: 128 frames of b at p_b = 4/5 p_a, 129 at p_b = 3/2 p_a + c
            assert max(bins_of(512, 256, RH.DEFAULT_RATES, 1), bins_of(256, 512, RH.DEFAULT_RATES, 1)) <= LDS_BINS
            # (the two lines cross: the first band also claims the frames of the other piece that lie on it)
            assert sorted(tuple(s)[8:10] for s in want[24]["seg"][:2]) == [(3, 2), (4, 5)] and (want[24]["seg"][:2]["t_aligned"] >= 100).all()
            assert want[24]["n_segments"] >= 2 and want[24]["t_covered"] >= 250 and (want["n_segments"] >= 1).sum() >= 20
        RS.same(hvd.search.align_rate_segments(fq, oq, pairs, pq, RH.DEFAULT_RATES, slack, None, ft, ot, pt), want)
        big = bins_of(int(2 * 513), int(2 * 257), RH.DEFAULT_RATES, slack)  # (gapped positions may pass the LDS limit)
        RS.same(dev(gpu, fq, oq, pq, ft, ot, pt, pairs, RH.DEFAULT_RATES, 31, slack, scratch_bins=big), want)


# ---- the scratch form ----

N_BIG = SLOTS + 5


@pytest.fixture(scope="module")
def scratch_case():
    """Three 300-frame reels of two pieces (150 frames at 5/4, 150 at 3/2) of a 1200-frame source, beside LDS pairs: under the
    default list a reel against the source has 4 * 299 + 5 * 1199 + 1 + 10 = 7202 bins. 64 + 5 such pairs open the list, the
    reels in rotation: the workgroup of slot w serves pair w and then pair 64 + w, another reel, in the same slot -- where the
    first one's taken words still lie."""
    rng = np.random.default_rng(84)
    source, clips = RH.planted_clips(seed=74, max_flips=20)
    L = rand(rng, 1200)
    cut = lambda c1, c2: AH.noisy(rng, np.concatenate([RH.resampled(L, 150, 5, 4, c1), RH.resampled(L, 150, 3, 2, c2)]), 20)  # noqa: E731
    frames, offsets = RH.join([source, clips[(5, 4)], L, cut(17.4, 600.2), cut(300.6, 40.3), cut(707.1, 333.3)])
    big = [(3 + k % 3, 2) if k % 2 == 0 else (2, 3 + k % 3) for k in range(N_BIG)]
    assert all(big[w][0] + big[w][1] != big[SLOTS + w][0] + big[SLOTS + w][1] for w in range(5))
    pairs = big + [(1, 0), (0, 1), (3, 3), (1, 3)]
    want = restated(frames, offsets, pairs)
    return frames, offsets, pairs, want


def lost_where_big(pairs, want):
    lost = want.copy()
    for k in range(N_BIG):
        lost[k] = RS.lost_record(*pairs[k])
    return lost


def test_scratch_form_beside_lds_pairs(gpu, hvd, scratch_case):
    frames, offsets, pairs, want = scratch_case
    bins = bins_of(299, 1199, RH.DEFAULT_RATES, 1)
    assert bins == 7202 > LDS_BINS and bins_of(1199, 299, RH.DEFAULT_RATES, 1) == 7202
    assert max(bins_of(299, 299, RH.DEFAULT_RATES, 1), bins_of(59, 299, RH.DEFAULT_RATES, 1)) <= LDS_BINS  # the pairs behind
    for k in range(N_BIG):  # two segments, the two pieces whole
        on = "q_aligned" if pairs[k][1] == 2 else "t_aligned"
        assert want[k]["n_segments"] == 2 and sorted(want[k]["seg"][:2][on].tolist()) == [150, 150], k
    assert sorted(tuple(s)[8:10] for s in want[0]["seg"][:2]) == [(3, 2), (5, 4)]
    assert sorted(tuple(s)[8:10] for s in want[1]["seg"][:2]) == [(2, 3), (4, 5)]
    RS.same(hvd.search.align_rate_segments(frames, offsets, pairs), want)
    RS.same(dev(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES, scratch_bins=bins), want)
    # both launches write their own records and skip the other's: without scratch the scratch launch's pairs are lost, the
    # LDS launch's are intact
    RS.same(dev(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES, scratch_bins=0), lost_where_big(pairs, want))


def test_scratch_sixteen_bytes_too_small(gpu, hvd, scratch_case):
    """A slot holds the pair's largest histogram, its flag words and its taken words: 7202 + 2 * (ceil(300 / 32) +
    ceil(1200 / 32)) = 7298 words. Told of exactly 64 such slots the entry aligns the pairs; told of 16 bytes less it gives
    them the INT32_MIN record, and the LDS pairs are intact."""
    frames, offsets, pairs, want = scratch_case
    need = 7202 + 2 * (10 + 38)
    assert need == 7298
    args = (gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES)
    RS.same(dev(*args, scratch_bins=7202, scratch_bytes=4 * SLOTS * need), want)
    RS.same(dev(*args, scratch_bins=7202, scratch_bytes=4 * SLOTS * need - 16), lost_where_big(pairs, want))


# ---- grid stride, broken calls, reordering ----

def test_many_small_pairs_grid_stride(gpu, hvd):
    """8 200 pairs of 4 x 4 frames, more than the 8 192 workgroups of the LDS launch: the first workgroups serve a second pair.
    Among them pair indices out of range (INT32_MIN), empty videos (the zero record) and pairs without a hit."""
    rng = np.random.default_rng(85)
    base = [rand(rng, 8) for _ in range(12)]
    vids = []
    for S in base:  # four 4-frame videos of one 8-frame source: 1x, 2x, 1x shifted, 1/2x
        vids += [S[0:4].copy(), S[[0, 2, 4, 6]].copy(), S[2:6].copy(), S[[1, 1, 2, 2]].copy()]
    vids += [np.zeros((0, 32), np.uint8), rand(rng, 4)]
    frames, offsets = RH.join(vids)
    V = len(vids)
    pairs = rng.integers(0, V, (LDS_GRID + 8, 2))
    pairs[rng.integers(0, len(pairs), 40), rng.integers(0, 2, 40)] = V + rng.integers(0, 3, 40)  # out of range
    pairs[[0, LDS_GRID - 1, LDS_GRID, LDS_GRID + 7]] = [(0, 1), (3, 0), (1, 0), (V, 0)]      # the first and the second round
    want = restated(frames, offsets, pairs)
    assert (want["seg"][:, 0]["offset"] == RS.INT32_MIN).sum() >= 30 and (want["q_hits"] == 0).sum() > 4000
    assert (want["q_hits"] > 0).sum() > 300
    RS.same(dev(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES), want)


def test_broken_lists_and_limits(gpu, hvd, reels):
    """The device entry: under a broken list every pair gets the INT32_MIN record; max_segments outside [1, 8] and
    min_band_votes < 1 are HVD_ERR_ARG and write nothing. The host entry: HVD_ERR_ARG for all of them."""
    frames, offsets, pairs = reels
    some = pairs[:3] + [(0, 9)]
    for bad in (RH.NINE_RATES, [(2, 4)], [(1, 1), (1, 1)], [(0, 1)], [(1, 9)]):
        got = dev(gpu, frames, offsets, None, frames, offsets, None, some, bad)
        RS.same(got, np.array([RS.lost_record(*p) for p in some], dtype=RS.VRSEGMENTS_DTYPE))
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_rate_segments(frames, offsets, pairs, rates=bad)
        assert e.value.code == gpu.HVD_ERR_ARG
    for kwargs in (dict(max_segments=0), dict(max_segments=9), dict(min_band_votes=0), dict(min_band_votes=-1)):
        rc, out = dev_call(gpu, frames, offsets, None, frames, offsets, None, some, RH.DEFAULT_RATES, **kwargs)
        assert rc == gpu.HVD_ERR_ARG and (out.view(np.uint8) == out.view(np.uint8)[0]).all(), kwargs  # (the sentinel fill)
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_rate_segments(frames, offsets, pairs, **kwargs)
        assert e.value.code == gpu.HVD_ERR_ARG
    with pytest.raises(gpu.HvdError) as e:
        hvd.search.align_rate_segments(frames, offsets, [(0, 9)])
    assert e.value.code == gpu.HVD_ERR_ARG


def test_reordering_the_list_changes_the_rate_index_alone(gpu, hvd):
    """Rotating the list: on the pairs whose largest S_r(d*_r) one rate reaches alone (RH.non_tying) the first segment changes in
    rate_index only, and maps back to the same rate. Every rotation equals the restatement under that rotation: the bound-skip
    walks the list in its order, and which rates it passes over depends on that order."""
    frames, offsets, pairs, _ = RH.wide_case(300)
    pairs = list(pairs)
    alone = RH.non_tying(frames, offsets, pairs, 31, 1)
    assert len(alone) >= 9
    assert max(RH.wide_bins(300, 1, p) for p in pairs) <= LDS_BINS
    base = dev(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.WIDE_RATES)
    RS.same(base, RS.align_rate_segments(frames, offsets, pairs, None, RH.WIDE_RATES))
    for k in (1, 3, 6):
        turned_list = RH.rotated(RH.WIDE_RATES, k)
        turned = dev(gpu, frames, offsets, None, frames, offsets, None, pairs, turned_list)
        RS.same(turned, RS.align_rate_segments(frames, offsets, pairs, None, turned_list))
        for p in alone:
            b, t = base[p]["seg"][0], turned[p]["seg"][0]
            assert b.tolist()[:10] == t.tolist()[:10] and RH.WIDE_RATES[b["rate_index"]] == turned_list[t["rate_index"]]
            assert [base[p][n] for n in HEAD[:4]] == [turned[p][n] for n in HEAD[:4]]


# ---- end to end ----

def test_find_rate_segmented_excerpts_end_to_end(gpu, hvd):
    """A 40-video library of frames in HBM with a four-piece, four-rate reel (B) and a three-piece 2x reel (C) planted, both
    shortened. Host entry, chained pipeline (positions from the quality filter through k_kept_positions: dropped frames leave
    gaps) and the rule on the restatement agree; reel C is reported by this search alone; the unit list is the segmented
    search and one segment is the rate search."""
    S = hvd.synth
    longs = [S.frames_gray(300, seed=41, const_fraction=0.0), S.frames_gray(260, seed=42, const_fraction=0.0)]
    longs[0][[3, 40, 41, 177]] = 77  # constant frames: quality 0, dropped by the filter
    idx = lambda n, num, den, c: np.floor(np.arange(n) * num / den + c + 0.5).astype(np.int64)  # noqa: E731
    reel_b = np.concatenate([idx(20, 3, 2, 100.3), idx(16, 2, 1, 20.6), idx(12, 1, 1, 200.0), idx(24, 5, 4, 150.2)])
    reel_c = np.concatenate([idx(12, 2, 1, 100.3), idx(12, 2, 1, 20.6), idx(12, 2, 1, 160.2)])
    vids = [longs[0][reel_b].copy(), longs[0], longs[1][reel_c].copy(), longs[1], longs[1][30:60].copy()]
    vids += [S.frames_gray(12, seed=200 + k, const_fraction=0.0) for k in range(35)]
    assert len(vids) == 40
    raw_off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate(vids))
    hashes, quality = hvd.vpdq.hash_frames(flat)
    keep = quality >= 31
    assert not keep[raw_off[1] + np.array([3, 40, 41, 177])].any()
    kept_off = np.concatenate([[0], np.cumsum([keep[raw_off[v]:raw_off[v + 1]].sum() for v in range(40)])]).astype(np.int64)
    raw_pos = (np.arange(len(flat)) - np.repeat(raw_off[:-1], np.diff(raw_off)))[keep]
    blobs = [hashes[keep][kept_off[v]:kept_off[v + 1]].tobytes() for v in range(40)]
    positions = [raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(40)]
    want = hvd.search.rate_segmented_excerpt_pairs(blobs, positions=positions, matcher=RS.ReferenceMatcher)
    by = {(e.short, e.long): e for e in want}
    assert by[(0, 1)].coverage >= 90.0 and {s.rate for s in by[(0, 1)].segments} >= {Fraction(3, 2), Fraction(5, 4)}
    assert by[(2, 3)].coverage >= 90.0 and len(by[(2, 3)].segments) == 3 and {s.rate for s in by[(2, 3)].segments} == {2}
    assert by[(4, 3)].coverage >= 90.0 and [s.rate for s in by[(4, 3)].segments] == [1]
    got = hvd.find_rate_segmented_excerpts(blobs, positions=positions)
    assert got == want
    # reel C: three pieces of twelve frames at 2x -- one line holds a third of it, no band of slope one holds four frames
    peel = hvd.find_segmented_excerpts(blobs, positions=positions)
    line = hvd.find_rate_excerpts(blobs, positions=positions)
    assert (2, 3) not in {(e.short, e.long) for e in peel} and (2, 3) not in {(e.short, e.long) for e in line}
    # the unit list is the segmented search, field for field apart from rate = 1; one segment is the rate search
    unit = hvd.find_rate_segmented_excerpts(blobs, rates=((1, 1),), positions=positions)
    assert len(peel) >= 1 and [e[:4] for e in unit] == [e[:4] for e in peel]
    assert [[tuple(s)[1:] for s in e.segments] for e in unit] == [[tuple(s) for s in e.segments] for e in peel]
    assert all(s.rate == 1 for e in unit for s in e.segments)
    one = hvd.find_rate_segmented_excerpts(blobs, positions=positions, max_segments=1)
    assert len(line) >= 1 and [(e.short, e.long, e.segments[0].rate, e.segments[0].offset, e.coverage) for e in one] == [
        (e.short, e.long, e.rate, e.offset, e.coverage) for e in line]
    d_fr = gpu.DeviceBuffer.from_array(flat)
    try:
        chained, recs, aligned, library = hvd.pipeline.find_rate_segmented_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1,
                                                                                              keep_library=True)
        assert chained == want
        assert np.array_equal(library.positions(), raw_pos) and np.array_equal(library.offsets(), kept_off)
        library.free()
        RS.same(aligned, RS.align_rate_segments(hashes[keep], kept_off, np.stack([recs["a"], recs["b"]], axis=1), raw_pos,
                                                min_band_votes=4))
    finally:
        d_fr.free()
